#!/usr/bin/env python3
"""What roft_objects_restart costs.  Nothing here is a pass bar.

Call time.  64 objects at 640 x 480 resident in HBM, one batch stepped, the engine idle: the host time of ONE call that restarts 1
and 64 slots -- with the box mesh of the stream, with the reference's 15 728-triangle cracker box (classification and upload on
the host's side of the call), and with ROFT_RESTART_KEEP_MESH.  Median and range of --reps calls.

Throughput.  The same 64 objects over --frames frames in batches of --batch, one shared scene resident in HBM, with one restart
call (one slot, KEEP_MESH, in turn through the slots) every 1, 3 or 10 batches and with none: object-frames per second, --rounds
alternated rounds per case, median and spread.  The call waits for the device like roft_sync, so this is the price of serving
restarts on an idle engine.

Writes profiles/r16_object_restart.json.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=240)
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--scale", type=int, default=1, help="divide the camera (a quick look on a small shape)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_object_restart.json"))
    args = p.parse_args()

    import torch
    import util
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import io, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    period = 48
    st = synth.make_stream(4600, 0, cam, flow_type=L.FLOW_F32C2, device=dev, period=period, n_schedule=args.frames + T)
    m0 = synth.initial_pose_from_stream(st)
    cracker = io.load_obj(util.ref_cracker_box(os.path.join(tempfile.gettempdir(), "roft_ref_meshes_%d" % os.getuid())))
    cracker = (np.ascontiguousarray(cracker[0], np.float32), np.ascontiguousarray(cracker[1], np.int32))

    def desc():
        d = E.default_object()
        for i in range(13):
            d.p_mean0[i] = m0[i]
        return d

    def frame(k):
        mi = int(st.mask_delivery[k])
        pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
        i = st.image(k)
        return dict(depth=st.depth[i].data_ptr(), flow=st.flow[i].data_ptr() if st.flow_valid[k] else None,
                    mask=st.mask_gt[mi].data_ptr() if mi >= 0 else None, pose=pose, dt=st.dt, mem_kind=L.MEM_DEVICE)

    def engine():
        cfg = E.default_config(cam.width, cam.height, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        for _ in range(n_obj):
            eng.add_object(desc(), *st.mesh)
        return eng

    # ---- the call on an idle engine
    eng = engine()
    eng.submit_batch([[frame(k)] * n_obj for k in range(T)])
    eng.step()
    eng.sync()
    calls = {}
    for name, mesh, keep in (("box_mesh_%d_triangles" % st.mesh[1].shape[0], st.mesh, False),
                             ("cracker_box_%d_triangles" % cracker[1].shape[0], cracker, False), ("keep_mesh", st.mesh, True)):
        for n in (1, n_obj):
            items = [(o, desc(), mesh[0], mesh[1]) for o in range(n)]
            us = []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                eng.restart_objects(items, keep_mesh=keep)
                us.append(1e6 * (time.perf_counter() - t0))
            calls["%s/%d_slots" % (name, n)] = dict(median_us=float(np.median(us)), min_us=min(us), max_us=max(us))
            print(name, n, "slots: %.0f us (%.0f - %.0f)" % (np.median(us), min(us), max(us)))
    eng.close()

    # ---- throughput with a restart call every `every` batches
    def leg(every):
        eng = engine()
        # the batches are built once, ahead of the timed region; a restarted slot's first frame gets its mask patched in
        batches = []
        for k0 in range(0, args.frames + T, T):
            arr, keep, t = eng.build_batch([[frame(k)] * n_obj for k in range(k0, k0 + T)])
            batches.append((k0, arr, keep, t))
        victim = 0
        t1 = None
        for b, (k0, arr, _keep, t) in enumerate(batches):
            if b == 1:              # the first batch is not timed
                eng.sync()
                t1 = time.perf_counter()
            patched = None
            if every and b > 1 and b % every == 0:
                eng.restart_objects([(victim, desc(), None, None)], keep_mesh=True)
                patched = (victim, arr[victim].mask)
                arr[victim].mask = st.mask_gt[st.image(k0)].data_ptr()   # (the first frame of a track must deliver a mask)
                victim = (victim + 1) % n_obj
            eng.submit_batch_raw(arr, t)
            eng.step()
            if patched:
                arr[patched[0]].mask = patched[1]
        eng.sync()
        dt = time.perf_counter() - t1
        n_calls = eng.restart_stats()["calls"]
        eng.close()
        return n_obj * args.frames / dt, n_calls

    cases = (("none", 0), ("every_10_batches", 10), ("every_3_batches", 3), ("every_batch", 1))
    runs = {name: [] for name, _ in cases}
    n_calls = {}
    for _ in range(args.rounds):
        for name, every in cases:
            v, n_calls[name] = leg(every)
            runs[name].append(v)
            print(name, "%.3e" % v)
    thr = {name: dict(median=float(np.median(v)), min=min(v), max=max(v), rounds=v, restart_calls=n_calls[name]) for name, v in runs.items()}
    base = thr["none"]["median"]
    for name in thr:
        thr[name]["ratio_to_none"] = thr[name]["median"] / base
    out = dict(shape=dict(objects=n_obj, width=cam.width, height=cam.height, frames=args.frames, batch=T, inputs="one shared scene resident in HBM"),
               call_us=calls, throughput_object_frames_per_s=thr)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: round(v["median"]) for k, v in thr.items()}))


if __name__ == "__main__":
    main()
