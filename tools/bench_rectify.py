#!/usr/bin/env python3
"""Lens distortion on the engine against frames the caller rectified beforehand.

bench.py's shared-scene HOST leg in the deployment form: one camera stream for all objects, label-image masks, camera images (the
engine computes the flow), float depth, pinned host buffers handed over as ROFT_MEM_HOST, full batches of --batch frames, the first
batch untimed.  Variant "on" submits the sensor's (distorted) frames to an engine with enable_rectification(); variant "off"
submits the products of ops.rectify, made BEFORE the loop, to a plain engine -- so "off" is the engine as it was, and the host-side
rectification a caller would have to run per frame (four image streams) is not in its time.  The two alternate in one process,
--rounds times each; reported are the object-frames/s of every round and their medians, the rectification launch's microseconds per
batch (HIP events, roft_debug_rectify_kernel_ms, from one more, untimed pass) and its bytes (sources read + products written,
roft_engine_rectify_stats) over that time as a fraction of the HBM rate (--hbm-tbs, 8.0 TB/s: the MI355X's specified peak).

Writes profiles/r25_rectify.json.  No ratio is asserted: the tool reports what it finds and checks only that both variants tracked
to identical poses.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

DIST = (-0.05, 0.01, 0.001, 0.0005, 0.0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=48, help="timed frames per round")
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--scale", type=int, default=1, help="divide the camera (a quick look on a small shape)")
    p.add_argument("--hbm-tbs", type=float, default=8.0)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_rectify.json"))
    args = p.parse_args()

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import ops, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    W, H = cam.width, cam.height
    n_run = T + args.frames
    st = synth.make_stream(4500, n_run, cam, flow_type=L.FLOW_F32C2, device=dev, with_gray=True)
    sensor = ops.lens(L.Camera(W, H, cam.fx * 1.02, cam.fy * 0.99, cam.cx + 3.0, cam.cy - 2.0), DIST)
    deal = ((np.arange(W)[None, :] + 3 * np.arange(H)[:, None]) % n_obj + 1).astype(np.uint8)

    def pinned(a):
        return torch.from_numpy(np.ascontiguousarray(a)).pin_memory()

    # the sensor's frames, and what a caller would have made of them on the host: both in pinned memory, one buffer per frame
    frames = {"on": [], "off": []}
    for k in range(n_run):
        mi = int(st.mask_delivery[k])
        src = dict(depth=st.depth[k].cpu().numpy(), image=st.gray[k].cpu().numpy(),
                   labels=np.where(st.mask_gt[mi].cpu().numpy() > 0, deal, 0).astype(np.uint8) if mi >= 0 else None)
        frames["on"].append({key: None if v is None else pinned(v) for key, v in src.items()})
        frames["off"].append(dict(depth=pinned(ops.rectify(src["depth"], sensor, cam)), image=pinned(ops.rectify(src["image"], sensor, cam)),
                                  labels=None if src["labels"] is None else pinned(ops.rectify(src["labels"], sensor, cam, nearest=True))))
    batches_kt = [(k0, min(T, n_run - k0)) for k0 in range(0, n_run, T)]

    def leg(form, sample_kernels=False):
        cfg = E.default_config(W, H, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        m0 = synth.initial_pose_from_stream(st)
        for _ in range(n_obj):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, *st.mesh)
        eng.enable_flow()
        if form == "on":
            eng.enable_rectification(sensor)
        eng.enable_log(n_run)
        batches = []
        for k0, t in batches_kt:
            fl = []
            for k in range(k0, k0 + t):
                pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                fr = frames[form][k]
                row = []
                for o in range(n_obj):
                    f = dict(depth=fr["depth"].data_ptr(), mask=None, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST, image=fr["image"].data_ptr(),
                             image_type=L.IMAGE_GRAY8)
                    if fr["labels"] is not None:
                        f.update(labels=fr["labels"].data_ptr(), label_type=L.LABEL_U8, label=o + 1)
                    row.append(f)
                fl.append(row)
            arr, keep, t_ = eng.build_batch(fl)
            batches.append((arr, keep, t_, eng.batch_labels(keep), eng.batch_images(keep)))
        kern_us = []
        arr, _keep, t, lab, img = batches[0]
        eng.submit_batch_raw(arr, t, lab, img)   # first batch: allocations, first touch of the pinned pages
        eng.step()
        eng.sync()
        s0, r0 = eng.stats(), eng.rectify_stats()
        t1 = time.perf_counter()
        for arr, _keep, t, lab, img in batches[1:]:
            eng.submit_batch_raw(arr, t, lab, img)
            if sample_kernels:
                kern_us.append(1e3 * eng.rectify_kernel_ms())
            eng.step()
        eng.sync()
        dt = time.perf_counter() - t1
        s1, r1 = eng.stats(), eng.rectify_stats()
        n_frames = s1["frames"] - s0["frames"]
        n_batches = max(len(batches) - 1, 1)
        res = dict(value=n_obj * n_frames / dt, ms_per_step=1e3 * dt / n_frames, us_per_batch=1e6 * dt / n_batches,
                   h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / n_frames / 1e6, launches_per_step=(s1["launches"] - s0["launches"]) / n_frames,
                   rectify_products_per_batch=(r1["products"] - r0["products"]) / n_batches, rectify_bytes_per_batch=(r1["bytes"] - r0["bytes"]) / n_batches,
                   rectify_kernel_us_per_batch=float(np.median(kern_us)) if kern_us else None, rows=eng.get_log_rows(0, n_run))
        eng.close()
        return res

    runs, rows = {"off": [], "on": []}, {}
    for r in range(args.rounds):
        for form in (("off", "on") if r % 2 == 0 else ("on", "off")):
            res = leg(form)
            rows.setdefault(form, res.pop("rows"))
            res.pop("rows", None)
            runs[form].append(res)
    timed = leg("on", sample_kernels=True)
    same = bool(np.array_equal(rows["off"], rows["on"], equal_nan=True))

    def summary(form):
        vals = [r["value"] for r in runs[form]]
        med = dict(sorted(runs[form], key=lambda r: r["value"])[len(vals) // 2])
        med.update(rounds=vals, median=float(np.median(vals)), unit="object-frames/s")
        return med

    off, on = summary("off"), summary("on")
    us, nbytes = timed["rectify_kernel_us_per_batch"], timed["rectify_bytes_per_batch"]
    result = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, rounds=args.rounds, lens=DIST, hbm_TBs=args.hbm_tbs),
                  rectification_off_prerectified_frames=off, rectification_on=on, ratio_on_over_off=on["median"] / off["median"],
                  rectify_kernel_us_per_batch=us, rectify_bytes_per_batch=nbytes, rectify_products_per_batch=timed["rectify_products_per_batch"],
                  rectify_GBs=nbytes / us / 1e3 if us else None, rectify_fraction_of_hbm=nbytes / (us * 1e-6) / (args.hbm_tbs * 1e12) if us else None,
                  identical_results=same)
    print(json.dumps({k: v for k, v in result.items() if not isinstance(v, dict)}))
    for form, r in (("off", off), ("on", on)):
        print(" ", form, json.dumps({k: r[k] for k in ("median", "rounds", "h2d_MB_per_step", "us_per_batch", "launches_per_step")}))
    if not same:
        raise SystemExit("bench_rectify.py: the two variants did not track to identical poses")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
