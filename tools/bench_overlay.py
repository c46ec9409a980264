#!/usr/bin/env python3
"""Times the scene renderer (ops.SceneRenderer) and the tool built on it, and sets them against the CPU path they replace.

  bench_overlay.py [--out profiles/r10_overlay.json] [--commit HASH] [--frames 256] [--frames-per-call 64] [--cpu-frames 4]
                   [--tool-frames 32] [--step-timeout 600]

The driver starts one child process per step (this file with --step NAME), each under its own time limit, and stops at the first
step that fails: nothing more is started on a device after a fault or a hang.  Steps:
  rgb_exact      the 78 single-mesh renders of tests/test_scene_gpu.py: how many rgb pixels differ from tests/scene_ref.py at all
  frames_WxH_I   640x480 and 1280x720 with 1 / 16 / 64 instances of the bench mesh (synth.box_mesh(CRACKER_BOX_HALF_EXTENTS)),
                 --frames frames in calls of --frames-per-call: kernel time per frame (HIP events: visibility, resolve), end to end
                 with upload and read-back, the resolve pass against the bytes it must move (per pixel 8 B of key + 3 B of
                 background in + 3 B of image out) as a fraction of the 8 TB/s HBM figure of DESIGN section 0, and
                 oracle.render_depth at divider 1 on one core for the poses of --cpu-frames of the frames (depth only: a lower
                 bound for the CPU)
  tool_WxH       tools/render_results.py on a sequence of --tool-frames PNG frames: frames per second with PNG decode and encode
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_BYTES_PER_S = 8e12   # the datasheet figure DESIGN section 0 uses
SHAPES = ((640, 480), (1280, 720))
INSTANCES = (1, 16, 64)


def camera(W, H):
    from roft_amd import _lib as L
    f = 1229.4285612615463 * W / 1280.0
    return L.Camera(W, H, f, f, W / 2.0, H / 2.0)


def scene_poses(n_frames, n_inst, seed=3):
    """n_inst boxes on a grid that fills the image, each turning a little from frame to frame."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(n_inst * 16 / 9.0)))
    rows = int(np.ceil(n_inst / cols))
    z = 0.45 * max(cols, 1.6)   # far enough for the grid to fit
    q0 = rng.normal(size=(n_inst, 4))
    out = np.zeros((n_frames, n_inst, 7))
    for i in range(n_inst):
        gx, gy = (i % cols + 0.5) / cols - 0.5, (i // cols + 0.5) / rows - 0.5
        for f in range(n_frames):
            q = q0[i] + 0.02 * f * np.array([0.3, 1.0, -0.5, 0.2])
            out[f, i] = np.concatenate([[gx * z * 0.95, gy * z * 0.53, z + 0.05 * np.sin(0.1 * f + i)], q / np.linalg.norm(q)])
    return out


def step_rgb_exact():
    from roft_amd import ops
    import scene_util as su
    differing = worst = covered = renders = 0
    for size in su.SIZES:
        for name, (v, t, _) in su.zoo().items():
            out = ops.render_scene(su.lib_cam(su.cam(*size)), [(v, t)], [0], np.stack(su.POSES)[:, None], outputs=("rgb", "instance"))
            for k in range(len(su.POSES)):
                ref = su.reference(name, k, size)
                d = np.abs(out["rgb"][k].astype(np.int32) - ref["rgb"].astype(np.int32)).max(axis=2)
                differing += int((d > 0).sum())
                worst = max(worst, int(d.max()))
                covered += int((ref["instance"] >= 0).sum())
                renders += 1
    return dict(renders=renders, covered_pixels=covered, rgb_pixels_differing=differing, rgb_max_level_difference=worst)


def step_frames(W, H, n_inst, args):
    from roft_amd import ops, synth
    from oracle import binding as ob
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)
    v, t = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)
    cam = camera(W, H)
    per_call = min(args.frames_per_call, args.frames)
    poses = scene_poses(args.frames, n_inst)
    rng = np.random.default_rng(1)
    bg = rng.integers(0, 256, (per_call, H, W, 3), dtype=np.uint8)
    r = ops.SceneRenderer(cam, [(v, t)], max_frames_per_call=per_call)
    idx = np.zeros(n_inst, np.int32)
    r.render(idx, poses[:per_call], background=bg, gray_background=True, outputs=("rgb",))   # warm-up: buffers, code object
    vis = res = wall = 0.0
    covered = 0
    for k in range(0, args.frames, per_call):
        p = poses[k:k + per_call]
        t0 = time.perf_counter()
        out = r.render(idx, p, background=bg[:len(p)], gray_background=True, outputs=("rgb",))
        wall += time.perf_counter() - t0
        a, b = r.kernel_ms()
        vis += a
        res += b
    maps = r.render(idx, poses[:1], outputs=("instance",))
    covered = float((maps["instance"] >= 0).mean())
    r.close()
    del out
    # the CPU path: the oracle's depth render of every instance, one core
    m = ob.make_mesh(v, t)
    oc = ob.camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    t0 = time.perf_counter()
    for f in range(args.cpu_frames):
        for i in range(n_inst):
            ob.render_depth(m, poses[f, i, :3], poses[f, i, 3:], oc, 1)
    cpu_ms = 1e3 * (time.perf_counter() - t0) / args.cpu_frames
    n = float(args.frames)
    declared = W * H * (8 + 3 + 3)
    resolve_s = res * 1e-3 / n
    return dict(width=W, height=H, instances=n_inst, triangles_per_instance=int(len(t)), frames=args.frames, frames_per_call=per_call,
                covered_fraction_frame0=covered, visibility_us_per_frame=1e3 * vis / n, resolve_us_per_frame=1e3 * res / n,
                kernel_us_per_frame=1e3 * (vis + res) / n, end_to_end_ms_per_frame=1e3 * wall / n,
                cpu_oracle_depth_ms_per_frame=cpu_ms, cpu_frames_timed=args.cpu_frames, cpu_over_kernels=cpu_ms * 1e3 / (1e3 * (vis + res) / n),
                cpu_over_end_to_end=cpu_ms / (1e3 * wall / n), resolve_declared_bytes_per_frame=declared,
                resolve_bytes_per_s=declared / resolve_s, resolve_fraction_of_hbm=declared / resolve_s / HBM_BYTES_PER_S)


def step_tool(W, H, args):
    import render_results
    from roft_amd import io, synth
    v, t = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)
    n = args.tool_frames
    poses = scene_poses(n, 1)[:, 0]
    rng = np.random.default_rng(2)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "rgb"))
        cam = camera(W, H)
        json.dump(dict(width=W, height=H, fx=cam.fx, fy=cam.fy, cx=cam.cx, cy=cam.cy), open(os.path.join(d, "cam_K.json"), "w"))
        # a smooth image with some noise: compresses like a photograph rather than like white noise
        yy, xx = np.mgrid[0:H, 0:W]
        for k in range(n):
            img = np.stack([(xx + 3 * k) % 256, (yy * 2) % 256, (xx + yy) // 4 % 256], 2) + rng.integers(0, 8, (H, W, 3))
            io.write_png(os.path.join(d, "rgb", "%d.png" % k), np.clip(img, 0, 255).astype(np.uint8))
        io.write_obj(os.path.join(d, "model.obj"), v, t)
        io.write_poses(os.path.join(d, "poses.txt"), poses)
        argv = ["--root", d, "--mesh", os.path.join(d, "model.obj"), "--poses", os.path.join(d, "poses.txt"), "--out", os.path.join(d, "out")]
        render_results.main(argv + ["--frames", "0"])   # warm-up
        t0 = time.perf_counter()
        render_results.main(argv)
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        for k in range(n):
            io.write_png(os.path.join(d, "out", "%d.png" % k), io.read_png(os.path.join(d, "rgb", "%d.png" % k)))
        png = time.perf_counter() - t0
    return dict(width=W, height=H, frames=n, tool_frames_per_s=n / dt, tool_ms_per_frame=1e3 * dt / n, png_decode_encode_ms_per_frame=1e3 * png / n,
                png_share_of_tool=png / dt)


def run_step(name, args):
    if name == "rgb_exact":
        return step_rgb_exact()
    kind, shape = name.split("_")[0], name.split("_")[1]
    W, H = [int(x) for x in shape.split("x")]
    if kind == "tool":
        return step_tool(W, H, args)
    return step_frames(W, H, int(name.split("_")[2]), args)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_overlay.json"))
    ap.add_argument("--commit", default=None)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--frames-per-call", type=int, default=64)
    ap.add_argument("--cpu-frames", type=int, default=4)
    ap.add_argument("--tool-frames", type=int, default=32)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--step", default=None, help="(a child run) one step; prints its record as one JSON line")
    args = ap.parse_args(argv)
    from roft_amd import _lib as L
    L.require_device()
    if args.step:
        print(json.dumps(run_step(args.step, args)), flush=True)
        return 0
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    steps = ["rgb_exact"] + ["frames_%dx%d_%d" % (w, h, i) for w, h in SHAPES for i in INSTANCES] + ["tool_%dx%d" % s for s in SHAPES]
    record = dict(commit=commit, hbm_bytes_per_s=HBM_BYTES_PER_S, mesh="synth.box_mesh(CRACKER_BOX_HALF_EXTENTS)", steps={})
    rc = 0
    for name in steps:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", name, "--frames", str(args.frames),
               "--frames-per-call", str(args.frames_per_call), "--cpu-frames", str(args.cpu_frames), "--tool-frames", str(args.tool_frames)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            record["steps"][name] = dict(failed=r.returncode, stderr=r.stderr[-800:])
            print("step %s failed with %d: nothing more is started" % (name, r.returncode), flush=True)
            rc = 1
            break
        record["steps"][name] = json.loads(r.stdout.strip().splitlines()[-1])
        print(name, json.dumps(record["steps"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return rc


if __name__ == "__main__":
    sys.exit(main())
