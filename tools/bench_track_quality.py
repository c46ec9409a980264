#!/usr/bin/env python3
"""What track quality costs (roft_engine_enable_quality).

Throughput.  64 objects at 640 x 480 on one shared scene resident in HBM, full batches of --batch frames, the first batch
untimed; three engines alternate in one process, --windows times each: quality off, every = 1, every = 6.  Reported per variant:
the median window in object-frames/s and all windows.  One more, untimed pass of each quality variant samples the kernel's time
per launch (roft_debug_quality_kernel_ms: the HIP events bound to its dispatch).  The three variants must track to identical
log rows, and `every = 6` must give the records `every = 1` gives on its frames -- checked, not reported.

Cost when off (--off-cost PARENT.so PR.so, both under build_ab/): bench.py in the driver's shape (--steps 20 --warmup 5),
alternating the two libraries through ROFT_LIB_SO, --pairs times; both medians and the parent's own window-to-window spread go
into the same JSON.

--marks FILE: one more pass with every = 1 under full timing (roft_engine_enable_timing(e, 2)) dumps the HIP event marks of every
launch group to FILE, the input of tools/marks_timeline.py: where the quality launch sits on lane 1 and what it waits for.

Writes profiles/r13_track_quality.json.  No ratio is asserted.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def off_cost(parent, pr, pairs):
    def one(so):
        env = dict(os.environ, ROFT_LIB_SO=os.path.join(ROOT, "build_ab", so))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                            "--pcie-frames", "0", "--no-kernel-timing", "--json-out", os.devnull], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("bench.py failed with %s:\n%s" % (so, r.stderr[-2000:]))
        return float(json.loads(r.stdout.strip().splitlines()[-1])["value"])

    vals = {parent: [], pr: []}
    for _ in range(pairs):
        for so in (parent, pr):
            vals[so].append(one(so))
            print(so, round(vals[so][-1]))
    a, b = vals[parent], vals[pr]
    return dict(shape="bench.py --gpus 1 --steps 20 --warmup 5", pairs=pairs, parent=a, this=b, parent_median=float(np.median(a)),
                this_median=float(np.median(b)), parent_min=min(a), parent_max=max(a), ratio_this_over_parent=float(np.median(b) / np.median(a)),
                this_median_inside_parent_spread=bool(min(a) <= np.median(b) <= max(a)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=48, help="timed frames per window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--scale", type=int, default=1, help="divide the camera (a quick look on a small shape)")
    p.add_argument("--off-cost", nargs=2, default=None, metavar=("PARENT.so", "PR.so"))
    p.add_argument("--pairs", type=int, default=5)
    p.add_argument("--marks", default=None, metavar="FILE")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_track_quality.json"))
    args = p.parse_args()

    # (first, before this process opens the device: the two libraries alternate in processes of their own)
    cost = off_cost(args.off_cost[0], args.off_cost[1], args.pairs) if args.off_cost else None

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    n_run = T + args.frames
    st = synth.make_stream(4500, n_run, cam, flow_type=L.FLOW_F32C2, device=dev)
    m0 = synth.initial_pose_from_stream(st)

    def frame(k):
        mi = int(st.mask_delivery[k])
        pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
        i = st.image(k)
        return dict(depth=st.depth[i].data_ptr(), flow=st.flow[i].data_ptr() if st.flow_valid[k] else None,
                    mask=st.mask_gt[mi].data_ptr() if mi >= 0 else None, pose=pose, dt=st.dt, mem_kind=L.MEM_DEVICE)

    def leg(every, sample_kernel=False, marks=None):
        cfg = E.default_config(cam.width, cam.height, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        for _ in range(n_obj):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, *st.mesh)
        eng.enable_log(max(n_run, 5 * T, 6))
        if every:
            eng.enable_quality(every=every)
        batches = []
        for k0 in range(0, n_run, T):
            t = min(T, n_run - k0)
            arr, keep, t_ = eng.build_batch([[frame(k)] * n_obj for k in range(k0, k0 + t)])
            batches.append((arr, keep, t_))
        arr, _keep, t = batches[0]
        eng.submit_batch_raw(arr, t)
        eng.step()
        eng.sync()
        kern_us = []
        if marks:
            eng.enable_timing(2)
        s0 = eng.stats()
        t1 = time.perf_counter()
        for arr, _keep, t in batches[1:]:
            eng.submit_batch_raw(arr, t)
            eng.step()
            if sample_kernel:
                kern_us.append(1e3 * eng.quality_kernel_ms())
        eng.sync()
        dt = time.perf_counter() - t1
        if marks:
            os.environ["ROFT_DUMP_MARKS"] = marks
            eng.timing()
            del os.environ["ROFT_DUMP_MARKS"]
        s1 = eng.stats()
        frames = s1["frames"] - s0["frames"]
        res = dict(value=n_obj * frames / dt, ms_per_step=1e3 * dt / frames, launches_per_step=(s1["launches"] - s0["launches"]) / frames,
                   rows=eng.get_log_rows(0, n_run), rec=eng.quality(0, n_run) if every else None, kernel_us=kern_us)
        eng.close()
        return res

    variants = (("off", 0), ("every_1", 1), ("every_6", 6))
    runs, rows, recs = {name: [] for name, _ in variants}, {}, {}
    for _ in range(args.windows):
        for name, every in variants:
            r = leg(every)
            rows.setdefault(name, r["rows"])
            recs.setdefault(name, r["rec"])
            runs[name].append(r["value"])
    same = all(np.array_equal(rows["off"], rows[name], equal_nan=True) for name, _ in variants)
    due = np.arange(n_run) % 6 == 0
    same = same and recs["every_6"][due].tobytes() == recs["every_1"][due].tobytes() and bool((recs["every_6"]["frame"][~due] == -1).all())
    result = dict(config=dict(objects=n_obj, width=cam.width, height=cam.height, batch=T, timed_frames=args.frames, windows=args.windows,
                              inputs="one shared scene, DEVICE memory"), throughput={}, identical_results=bool(same))
    for name, every in variants:
        v = sorted(runs[name])
        result["throughput"][name] = dict(object_frames_per_s=v[len(v) // 2], windows=v)
        if every:
            k = leg(every, sample_kernel=True)["kernel_us"]
            result["throughput"][name].update(kernel_us_per_launch=float(np.median(k)), kernel_us_min=float(min(k)), kernel_us_max=float(max(k)),
                                              record_frames_per_batch=float(np.mean([sum(1 for f in range(k0, min(k0 + T, n_run)) if f % every == 0)
                                                                                     for k0 in range(T, n_run, T)])))
        print(name, json.dumps(result["throughput"][name]))
    off = result["throughput"]["off"]["object_frames_per_s"]
    for name in ("every_1", "every_6"):
        result["throughput"][name]["ratio_over_off"] = result["throughput"][name]["object_frames_per_s"] / off
    r1 = recs["every_1"]
    result["records_of_the_run"] = dict(overlap_median=float(np.nanmedian(r1["n_both"][1:] / np.maximum(r1["n_mask"][1:] + r1["n_render"][1:] - r1["n_both"][1:], 1))),
                                        depth_err_median_m=float(np.median(r1["depth_err"][1:][r1["n_depth"][1:] > 0])) if (r1["n_depth"][1:] > 0).any() else None)
    if not same:
        raise SystemExit("bench_track_quality.py: the variants did not give identical results")
    if args.marks:
        leg(1, marks=args.marks)
    if cost:
        result["cost_when_off"] = cost
        print("cost_when_off", json.dumps(cost))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
