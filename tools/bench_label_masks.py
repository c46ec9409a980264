#!/usr/bin/env python3
"""Shared-scene HOST leg of bench.py, once with per-object masks and once with ONE label image per delivery.

The construction is bench.py's `pcie_leg(shared=True)`: one camera stream (depth + CV_32FC2 flow) for all objects in pinned host
buffers handed over as ROFT_MEM_HOST, full batches of --batch frames, the first batch untimed (allocations, first touch of the
pinned pages), the median of three runs.  The two forms alternate in one process (A B A B A B), so that both see the same device
state.

Inputs.  The objects of a shared scene all look at the same thing, so their true masks coincide; a label image gives every pixel
to one value.  The image of a delivery is therefore composed by dealing the pixels of the stream's mask to the objects,
(u + 3 v) mod n_objects, value = object + 1: no two objects overlap, every object keeps a scattered 1 / n_objects of the mask.
The per-object engine gets the masks EXPANDED from that image, (labels == value) * 255, one pinned buffer per object and
delivery: both engines track identical inputs (the tool checks that their logged poses are equal).  Each object therefore
carries fewer mask pixels than in bench.py's own leg, where every object gets the whole mask: the rates here are not
comparable with bench.py's `value_pcie_inclusive_shared_scene`, only with each other.

Writes profiles/r09_label_masks.json: object-frames/s, h2d_MB_per_step, h2d_GB_per_s of both forms and their ratio, and the
preparation's time per delivery (control-block upload + mask ingest: the `mask_prepare` mark of roft_engine_enable_timing, read
from engines created with ROFT_PREP_AHEAD=2 so that both forms run their preparation where the mark brackets it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=48, help="timed frames per run (bench.py --pcie-frames)")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--scale", type=int, default=1, help="divide the 640 x 480 camera (a quick look on a small shape)")
    p.add_argument("--label-type", default="u8", choices=["u8", "u16"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_label_masks.json"))
    args = p.parse_args()

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import synth

    L.require_device()
    dev = torch.device("cuda", 0)
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    n_run = T + args.frames
    st = synth.make_stream(4000, n_run, cam, flow_type=synth.FLOW_F32C2, device=dev)
    W, H = cam.width, cam.height
    ldt = np.uint8 if args.label_type == "u8" else np.uint16
    if n_obj > np.iinfo(ldt).max:
        raise SystemExit("%d objects do not fit a %s label image" % (n_obj, args.label_type))

    depth = st.depth[:n_run].cpu().pin_memory()
    flow = st.flow[:n_run].cpu().pin_memory()
    deal = torch.from_numpy(((np.arange(W)[None, :] + 3 * np.arange(H)[:, None]) % n_obj + 1).astype(np.int32))
    labels, masks = {}, {}      # per delivering frame: the pinned label image; the pinned expanded masks [n_obj, H, W]
    for k in range(n_run):
        mi = int(st.mask_delivery[k])
        if mi < 0:
            continue
        lab = torch.where(st.mask_gt[mi].cpu() > 0, deal, torch.zeros_like(deal))
        masks[k] = (lab[None] == torch.arange(1, n_obj + 1, dtype=torch.int32)[:, None, None]).to(torch.uint8).mul_(255).pin_memory()
        labels[k] = (lab.to(torch.uint8) if ldt == np.uint8 else lab.to(torch.int16)).pin_memory()   # (values < 2^15: the bits are the u16's)
    label_type = L.LABEL_U8 if ldt == np.uint8 else L.LABEL_U16
    batches_kt = [(k0, min(T, n_run - k0)) for k0 in range(0, n_run, T)]
    n_deliveries = sum(1 for k in labels if k >= T)

    def new_engine():
        cfg = E.default_config(W, H, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        eng = E.ROFTFilterBatch(cfg)
        m0 = synth.initial_pose_from_stream(st)
        for _ in range(n_obj):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, *st.mesh)
        return eng

    def build(eng, form):
        out = []
        for k0, t in batches_kt:
            fl = []
            for k in range(k0, k0 + t):
                pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                row = []
                for o in range(n_obj):
                    f = dict(depth=depth[k].data_ptr(), flow=flow[k].data_ptr() if st.flow_valid[k] else None, mask=None, pose=pose, dt=st.dt,
                             mem_kind=L.MEM_HOST)
                    if k in labels and form == "labels":
                        f.update(labels=labels[k].data_ptr(), label_type=label_type, label=o + 1)
                    elif k in labels:
                        f["mask"] = masks[k][o].data_ptr()
                    row.append(f)
                fl.append(row)
            arr, keep, t_ = eng.build_batch(fl)
            out.append((arr, keep, t_, eng.batch_labels(keep)))
        return out

    def leg(form, timing=False):
        if timing:
            os.environ["ROFT_PREP_AHEAD"] = "2"     # (read when the engine is created)
        try:
            eng = new_engine()
        finally:
            os.environ.pop("ROFT_PREP_AHEAD", None)
        eng.enable_log(n_run)
        batches = build(eng, form)
        eng.submit_batch_raw(batches[0][0], batches[0][2], batches[0][3])   # first batch: allocations, first touch of the pinned pages
        eng.step()
        eng.sync()
        if timing:
            eng.enable_timing(2)
        s0 = eng.stats()
        t1 = time.perf_counter()
        for arr, _keep, t, lab in batches[1:]:
            eng.submit_batch_raw(arr, t, lab)
            eng.step()
        eng.sync()
        dt = time.perf_counter() - t1
        s1 = eng.stats()
        res = dict(frames=s1["frames"] - s0["frames"])
        if timing:
            ms, marks = eng.timing().get("mask_prepare", (0.0, 0))
            res.update(mask_prepare_ms_total=float(ms), mask_prepare_marks=int(marks), deliveries=n_deliveries,
                       prepare_us_per_delivery=1e3 * float(ms) / max(n_deliveries, 1))
        else:
            res.update(value=n_obj * res["frames"] / dt, unit="object-frames/s", ms_per_step=1e3 * dt / res["frames"],
                       h2d_GB_per_s=(s1["h2d_bytes"] - s0["h2d_bytes"]) / dt / 1e9,
                       h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / res["frames"] / 1e6,
                       h2d_copies_per_step=(s1["h2d_copies"] - s0["h2d_copies"]) / res["frames"],
                       launches_per_step=(s1["launches"] - s0["launches"]) / res["frames"])
        res["rows"] = eng.get_log_rows(0, n_run)
        eng.close()
        return res

    runs = {"masks": [], "labels": []}
    rows = {}
    for _ in range(args.runs):
        for form in ("masks", "labels"):
            r = leg(form)
            rows.setdefault(form, r.pop("rows"))
            r.pop("rows", None)
            runs[form].append(r)
    same = bool(np.array_equal(rows["masks"], rows["labels"], equal_nan=True))
    timing = {}
    for form in ("masks", "labels"):
        r = leg(form, timing=True)
        r.pop("rows")
        timing[form] = r

    def median(form):
        rs = sorted(runs[form], key=lambda r: r["value"])
        med = dict(rs[len(rs) // 2])
        med["runs"] = [r["value"] for r in rs]
        return med

    out = dict(
        config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, runs=args.runs, label_type=args.label_type,
                    flow="CV_32FC2", deliveries_in_timed_frames=n_deliveries),
        per_object_masks=median("masks"), label_image=median("labels"),
        identical_results=same,
        preparation_timing=dict(timing, note="mask_prepare of roft_engine_enable_timing(2) on engines created with ROFT_PREP_AHEAD=2: control-block "
                                             "upload + mask ingest of a batch on the upload stream, summed over the timed batches and divided by "
                                             "their deliveries; a separate, instrumented run of each form (never the rates above)"),
        note="bench.py's shared-scene HOST leg (pinned buffers, first batch untimed, median of the runs) with the masks of a delivery as n "
             "per-object byte images or as one label image; both forms alternate in one process.  The label image deals the stream's mask "
             "to the objects, (u + 3 v) mod n + 1, and the per-object engine gets the masks expanded from it: identical inputs, each "
             "object with 1 / n of the mask's pixels -- the rates compare with each other, not with bench.py's leg.")
    out["ratio_label_over_masks"] = out["label_image"]["value"] / out["per_object_masks"]["value"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("config", "identical_results", "ratio_label_over_masks")}))
    for form in ("per_object_masks", "label_image"):
        print(form, json.dumps({k: out[form][k] for k in ("value", "h2d_MB_per_step", "h2d_GB_per_s", "ms_per_step", "runs")}))
    print("preparation", json.dumps({f: timing[f].get("prepare_us_per_delivery") for f in timing}))
    if not same:
        raise SystemExit("bench_label_masks.py: the two forms did not track to identical poses")


if __name__ == "__main__":
    main()
