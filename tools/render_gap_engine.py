#!/usr/bin/env python3
"""The GPU counterpart of tools/render_gap.py: how far apart are the engine's two render modes of the outlier test
(roft_config::render_mode: ROFT_RENDER_CONTRACT, the default, and ROFT_RENDER_GL, the numerics of the reference's OpenGL pipeline)
on the workloads of BASELINE configs #3 - #5 -- the streams and seeds of tools/render_gap.py -- and what does the GL mode cost?

Every config runs through the engine twice, once per mode, one frame per submit, and every outlier test's likelihoods and decision
are read back.  Reported per config: tests, decisions that differ between the modes (ROFTFilter.cpp:581-583: L0 > 2 L1), max and
mean |dL| / L of GL against the contract, and the outlier test's launch group (HIP events around outlier_fused_kernel, timing level
2) in microseconds per launch in each mode.  Config #4 also gets its object-frames/s in each mode: the frames submitted and stepped
back to back, timed from the first submit to the device's completion of the last step, after a warm-up pass.

usage: python tools/render_gap_engine.py [--frames3 98] [--frames4 98] [--objects4 64] [--frames5 300] [--objects5 16]
                                         [--out profiles/r07_render_gap_engine.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import synth
import util


def object_stream(which, o, n_frames):
    """Object o of BASELINE config #`which` (tools/render_gap.py's streams), generated on the device."""
    if which == 3:
        return synth.make_stream(3000 + o, n_frames, synth.Camera.shape_b(), flow_type=synth.FLOW_S16C2,
                                 half_extents=synth.FAST_YCB_HALF_EXTENTS[o], device="cuda")
    if which == 4:
        scale = 0.8 + 0.4 * (((o % 64) * 7) % 10) / 9.0
        half = tuple(h * scale for h in synth.CRACKER_BOX_HALF_EXTENTS)
        return synth.make_stream(4000 + o, n_frames, synth.Camera.shape_a(), flow_type=synth.FLOW_F32C2, half_extents=half, device="cuda")
    return synth.make_stream(5000 + o, 0, synth.Camera.shape_b(), flow_type=synth.FLOW_S16C2, half_extents=synth.FAST_YCB_HALF_EXTENTS[o % 5],
                             period=60, n_schedule=n_frames, device="cuda")


def make_engine(streams, mode):
    st0 = streams[0]
    cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=len(streams), render_mode=mode)
    c = st0.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st0.flow_grid, st0.flow_scale
    eng = E.ROFTFilterBatch(cfg)
    for st in streams:
        d = E.default_object()
        m0 = synth.initial_pose_from_stream(st)
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, *st.mesh)
    return eng


def run_tests(streams, n_frames, mode):
    """(rows [test: frame, object, L0, L1, selected], outlier launch group us per launch)"""
    eng = make_engine(streams, mode)
    eng.enable_timing(2)
    eng.timing()   # (reset)
    rows = []
    for k in range(n_frames):
        eng.submit([util.device_frame(st, k) for st in streams])
        eng.step()
        for o, out in enumerate(eng.outputs()):
            if out.outlier_selected >= 0:
                rows.append((k, o, out.outlier_L[0], out.outlier_L[1], out.outlier_selected))
    t = eng.timing().get("outlier_render_likelihood", (0.0, 0))
    eng.close()
    return np.array(rows, np.float64).reshape(-1, 5), (1e3 * t[0] / t[1] if t[1] else None), int(t[1])


def throughput(streams, n_frames, mode):
    eng = make_engine(streams, mode)
    frames = lambda k: [util.device_frame(st, k) for st in streams]
    for k in range(min(n_frames, 12)):   # warm-up
        eng.submit(frames(k))
        eng.step()
    eng.sync()
    eng.close()
    eng = make_engine(streams, mode)
    t0 = time.perf_counter()
    for k in range(n_frames):
        eng.submit(frames(k))
        eng.step()
    eng.sync()
    dt = time.perf_counter() - t0
    eng.close()
    return len(streams) * n_frames / dt


def summarise(rc, rg):
    out = {"tests_contract": int(len(rc)), "tests_gl": int(len(rg))}
    key = lambda r: (int(r[0]), int(r[1]))
    gl = {key(r): r for r in rg}
    both = [(r, gl[key(r)]) for r in rc if key(r) in gl]
    out["tests"] = len(both)
    out["decisions_flipped"] = int(sum(a[4] != b[4] for a, b in both))
    rel = [abs(b[2 + i] - a[2 + i]) / a[2 + i] for a, b in both for i in range(2) if a[2 + i] < 1e300 and b[2 + i] < 1e300 and a[2 + i] > 0]
    out["max_rel_dL"] = float(max(rel)) if rel else None
    out["mean_rel_dL"] = float(np.mean(rel)) if rel else None
    out["vel_only_chosen_contract"] = int(sum(a[4] for a, _ in both))
    out["vel_only_chosen_gl"] = int(sum(b[4] for _, b in both))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames3", type=int, default=98)
    p.add_argument("--frames4", type=int, default=98)
    p.add_argument("--objects4", type=int, default=64)
    p.add_argument("--frames5", type=int, default=300)
    p.add_argument("--objects5", type=int, default=16)
    p.add_argument("--out", default="")
    p.add_argument("--commit", default="", help="commit the measured tree is stamped with (default: git rev-parse HEAD)")
    a = p.parse_args()
    L.require_device()
    commit = a.commit or None
    if commit is None:
        try:
            commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
        except OSError:
            pass
    rep = {"what": "the engine in both render modes (contract / gl) on the streams of tools/render_gap.py, one frame per submit; "
                   "object_frames_per_s is that frame-at-a-time loop (host-bound), not bench.py's batched measurement; tools/render_gap_engine.py",
           "commit": commit, "args": vars(a)}
    for which, nf, no in ((3, a.frames3, 5), (4, a.frames4, a.objects4), (5, a.frames5, a.objects5)):
        if nf <= 0:
            continue
        t0 = time.time()
        streams = [object_stream(which, o, nf) for o in range(no)]
        rc, us_c, n_c = run_tests(streams, nf, L.RENDER_CONTRACT)
        rg, us_g, n_g = run_tests(streams, nf, L.RENDER_GL)
        r = dict(summarise(rc, rg), objects=no, frames=nf, outlier_fused_us_per_launch={"contract": us_c, "gl": us_g},
                 outlier_launches={"contract": n_c, "gl": n_g})
        if us_c and us_g:
            r["gl_over_contract_kernel_time"] = us_g / us_c
        if which == 4:
            r["object_frames_per_s"] = {"contract": throughput(streams, nf, L.RENDER_CONTRACT), "gl": throughput(streams, nf, L.RENDER_GL)}
        r["seconds"] = round(time.time() - t0, 1)
        rep["config_%d" % which] = r
        print("config #%d: %s" % (which, json.dumps(r)), flush=True)
        del streams
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
