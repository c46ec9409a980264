#!/usr/bin/env python3
"""What scoring pose hypotheses costs (roft_pose_hypotheses_score, roft_engine_score_hypotheses; include/roft_engine.h, section 3j).

Shape: 640 x 480, divider 2; two meshes -- the 15 552-triangle box of the benchmark stream and the reference's cracker box
(tests/golden/ref_meshes) --; n = 13 / 169 / 2 197 poses drawn around the true pose.  One process, --repeats rounds; inside a round
every variant runs once, in turn (alternated), each after one untimed call of its own shape.  Reported per variant: the median of the
rounds in hypotheses per second, and all rounds.

  operator          one roft_pose_hypotheses_score call on host buffers (its uploads and the mesh's preparation included)
  engine            one roft_engine_score_hypotheses call on an engine that has stepped --engine-frames frames of the stream
  track_quality     BASELINE, today's only way: one roft_track_quality call per pose in the same process (on the first 169 poses of a
                    larger n: its rate per pose does not depend on n)
  cpu               BASELINE, on 8 hypotheses: the oracle's render_depth plus the numpy form of the record (tests/quality_ref.py)
  relocalise        one ROFTFilterBatch.relocalise call from a pose 12 / -9 / 15 mm and 9 degrees off the estimate: wall time, rounds

The records of every GPU variant must be equal bit for bit -- checked, not reported.  Writes profiles/r28_pose_hypotheses.json.  No
ratio is asserted.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402


def poses_around(x, q, n, seed):
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 7))
    out[:, :3] = x + rng.uniform(-0.02, 0.02, (n, 3))
    quats = q + rng.uniform(-0.08, 0.08, (n, 4))
    out[:, 3:] = quats / np.linalg.norm(quats, axis=1)[:, None]
    out[0, :3], out[0, 3:] = x, q
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--sizes", type=int, nargs="+", default=[13, 169, 2197])
    p.add_argument("--scale", type=int, default=1, help="divide the camera (a quick look on a small shape)")
    p.add_argument("--engine-frames", type=int, default=3)
    p.add_argument("--cpu-poses", type=int, default=8)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_pose_hypotheses.json"))
    args = p.parse_args()

    import torch
    import quality_ref as qr
    import util
    from oracle import binding as ob
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import io, ops, relocalise, synth

    L.require_device()
    ob.build()
    dev = torch.device("cuda", 0)
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    divider = 2 if cam.width == 640 else 4
    st = synth.make_stream(4500, args.engine_frames, cam, flow_type=L.FLOW_F32C2, device=dev)
    dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    ocam = util.oracle_camera(ob, cam)
    k_last = args.engine_frames - 1
    depth = st.depth[st.image(k_last)].cpu().numpy().astype(np.float32)
    meshes = {"box_15552": st.mesh, "cracker_box": io.load_obj(util.ref_cracker_box(os.path.join(tempfile.gettempdir(), "roft_ref_meshes_%d" % os.getuid())))}
    meshes = {k: (np.ascontiguousarray(v, np.float32), np.ascontiguousarray(t, np.int32)) for k, (v, t) in meshes.items()}
    TOL, DMAX = 0.01, 2.0

    # the engine: one slot per mesh on the same stream, stepped to its last frame
    cfg = E.default_config(cam.width, cam.height, st.flow_type, max_objects=len(meshes), max_batch_frames=1)
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
    cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
    eng = E.ROFTFilterBatch(cfg)
    m0 = synth.initial_pose_from_stream(st)
    for v, t in meshes.values():
        d = E.default_object()
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, v, t)
    for k in range(args.engine_frames):
        mi = int(st.mask_delivery[k])
        pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
        i = st.image(k)
        f = dict(depth=st.depth[i].data_ptr(), flow=st.flow[i].data_ptr() if st.flow_valid[k] else None,
                 mask=st.mask_gt[mi].data_ptr() if mi >= 0 else None, pose=pose, dt=st.dt, mem_kind=L.MEM_DEVICE)
        eng.submit([f] * len(meshes))
        eng.step()
    eng.sync()
    est = eng.outputs()
    DMAX = eng.cfg.depth_maximum

    def timed(fn):
        t0 = time.perf_counter()
        r = fn()
        return time.perf_counter() - t0, r

    result = dict(config=dict(width=cam.width, height=cam.height, divider=divider, repeats=args.repeats, sizes=args.sizes,
                              engine_frames=args.engine_frames, depth_tolerance=TOL, depth_maximum=DMAX), meshes={}, identical_records=True)
    for o, (name, (v, t)) in enumerate(meshes.items()):
        dmesh = ops.make_mesh(v, t)
        x, q = np.array(est[o].pose[6:9]), np.array(est[o].pose[9:13])
        mask = np.where(eng.mask(o) != 0, 255, 0).astype(np.uint8)
        per_mesh = dict(vertices=int(len(v)), triangles=int(len(t)), sizes={})
        for n in args.sizes:
            P = poses_around(x, q, n, 7 + n)
            n_base = min(n, 169)

            variants = {
                "operator": lambda: ops.pose_hypotheses_score(dcam, divider, depth, mask, dmesh, P, TOL, DMAX),
                "engine": lambda: eng.score_hypotheses(o, P, TOL),
                "track_quality": lambda: np.array([ops.track_quality(dcam, divider, depth, mask, dmesh, r[:3], r[3:], TOL, DMAX) for r in P[:n_base]]),
            }
            times, recs = {k: [] for k in variants}, {}
            for fn in variants.values():
                fn()                                           # every shape once, untimed
            for _ in range(args.repeats):
                for k, fn in variants.items():
                    dt, r = timed(fn)
                    times[k].append(dt)
                    recs[k] = r
            result["identical_records"] &= recs["track_quality"].tobytes() == recs["operator"][:n_base].tobytes()
            e = recs["engine"].copy()
            e["frame"] = 0
            result["identical_records"] &= e.tobytes() == recs["operator"].tobytes()
            per_mesh["sizes"][str(n)] = {k: dict(hypotheses_per_s=float((n_base if k == "track_quality" else n) / np.median(v_)), ms_median=float(1e3 * np.median(v_)),
                                                 ms_all=[float(1e3 * s) for s in v_]) for k, v_ in times.items()}
            print(name, n, {k: round(d["hypotheses_per_s"]) for k, d in per_mesh["sizes"][str(n)].items()}, flush=True)
        # the CPU path on a few hypotheses
        P = poses_around(x, q, args.cpu_poses, 3)
        cpu_t = []
        for _ in range(args.repeats):
            dt, r = timed(lambda: [qr.quality(ob, ocam, divider, depth, mask > 1, (v, t), r_[:3], r_[3:], TOL, DMAX) for r_ in P])
            cpu_t.append(dt)
        got = ops.pose_hypotheses_score(dcam, divider, depth, mask, dmesh, P, TOL, DMAX)
        result["identical_records"] &= all(qr.same(qr.as_dict(g), w) for g, w in zip(got, r))
        per_mesh["cpu"] = dict(poses=args.cpu_poses, hypotheses_per_s=float(args.cpu_poses / np.median(cpu_t)), ms_all=[float(1e3 * s) for s in cpu_t])
        # one relocalise call from a pose off the estimate
        x0 = x + np.array([0.012, -0.009, 0.015])
        a = math.radians(9.0) / 2
        q0 = relocalise.quat_mul(np.concatenate([[math.cos(a)], math.sin(a) * np.array([1.0, 2.0, -1.0]) / math.sqrt(6.0)]), q)
        eng.relocalise(o, x0, q0)
        rel_t, rel = [], None
        for _ in range(args.repeats):
            dt, rel = timed(lambda: eng.relocalise(o, x0, q0))
            rel_t.append(dt)
        xr, qr_, trace = rel
        per_mesh["relocalise"] = dict(ms_median=float(1e3 * np.median(rel_t)), ms_all=[float(1e3 * s) for s in rel_t], rounds=len(trace),
                                      disagreement_start=trace[0][1], disagreement_end=trace[-1][1],
                                      distance_to_estimate_start_mm=float(1e3 * np.linalg.norm(x0 - x)), distance_to_estimate_end_mm=float(1e3 * np.linalg.norm(xr - x)))
        print(name, "cpu", per_mesh["cpu"]["hypotheses_per_s"], "relocalise", per_mesh["relocalise"], flush=True)
        result["meshes"][name] = per_mesh
    eng.close()
    if not result["identical_records"]:
        raise SystemExit("bench_pose_hypotheses.py: the variants did not give identical records")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
