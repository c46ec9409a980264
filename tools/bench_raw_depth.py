#!/usr/bin/env python3
"""Raw sensor depth on the engine against float depth prepared by the caller.

Throughput.  bench.py's shared-scene HOST leg in the deployment form: one camera stream for all objects, label-image masks,
camera images (the engine computes the flow), pinned host buffers handed over as ROFT_MEM_HOST, full batches of --batch frames,
the first batch untimed.  The sensor delivers 16-bit frames (the stream's depth quantised to millimetres).  Variant (a) is
today's caller: `raw.astype(float32) * scale` into a pinned float buffer, timed as part of the loop, and the floats submitted;
variant (b) submits the 16-bit frames to an engine with enable_raw_depth().  The two alternate in one process, --windows times
each; the median window is reported with object-frames/s, MB per step, the host microseconds per submit call and per roft_step
(roft_batch_trace) and the host conversion's microseconds per batch; the depth kernels' microseconds per batch (HIP events,
roft_debug_depth_kernel_ms) come from one more, untimed pass.

The same with `align` on: a 424 x 240 depth camera with a 15 mm baseline registered to the colour camera on the device.  There
variant (a) submits floats that were aligned BEFORE the loop (by ops.depth_align): the host-side registration a caller would
have to run per frame is not in its time, so (a) is a lower bound of today's path.

Live latency.  One object, 1280 x 720, one frame per submit with the state read back after each, both ways.

Writes profiles/r12_raw_depth.json.  No ratio is asserted: the tool reports what it finds and checks only that both variants
tracked to identical poses.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402

SCALE = 0.001


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=48, help="timed frames per window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--scale", type=int, default=1, help="divide the cameras (a quick look on a small shape)")
    p.add_argument("--live-frames", type=int, default=40)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_raw_depth.json"))
    args = p.parse_args()

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import ops, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))

    def quantise(depth):
        return torch.clamp(torch.round(depth / SCALE), 0, 65535).to(torch.int32).cpu().numpy().astype(np.uint16)

    def make_engine(st, cam, n, max_batch):
        cfg = E.default_config(cam.width, cam.height, st.flow_type, max_objects=n, max_batch_frames=max_batch)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        m0 = synth.initial_pose_from_stream(st)
        for _ in range(n):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, *st.mesh)
        return eng

    # ---- throughput ------------------------------------------------------------------------------------------------------
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    W, H = cam.width, cam.height
    n_run = T + args.frames
    ft = L.FLOW_F32C2
    st = synth.make_stream(4300, n_run, cam, flow_type=ft, device=dev, with_gray=True)
    gray = st.gray[:n_run].cpu().pin_memory()
    raw_np = quantise(st.depth[:n_run])
    deal = torch.from_numpy(((np.arange(W)[None, :] + 3 * np.arange(H)[:, None]) % n_obj + 1).astype(np.int32))
    labels = {}
    for k in range(n_run):
        mi = int(st.mask_delivery[k])
        if mi >= 0:
            labels[k] = torch.where(st.mask_gt[mi].cpu() > 0, deal, torch.zeros_like(deal)).to(torch.uint8).pin_memory()
    batches_kt = [(k0, min(T, n_run - k0)) for k0 in range(0, n_run, T)]
    # the depth camera of the align legs: 424 x 240 in front of the colour camera, a 15 mm baseline
    dW, dH = max(424 // args.scale, 8), max(240 // args.scale, 8)
    fd = cam.fx * dW / W
    dcam = synth.Camera(dW, dH, fd, fd, (dW - 1) / 2.0, (dH - 1) / 2.0)
    align_t = np.array([0.015, 0.0, 0.0])
    xx = np.clip(np.rint((np.arange(dW) - dcam.cx) * (cam.fx / fd) + cam.cx).astype(np.int64), 0, W - 1)
    yy = np.clip(np.rint((np.arange(dH) - dcam.cy) * (cam.fy / fd) + cam.cy).astype(np.int64), 0, H - 1)
    raw_small_np = np.ascontiguousarray(raw_np[:, yy][:, :, xx])     # the scene sampled at the depth camera's pixels
    result = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, windows=args.windows, depth_scale=SCALE,
                              align_depth_camera=[dW, dH], align_baseline_m=float(align_t[0])), throughput={})

    for name, align in (("convert", False), ("align", True)):
        src_np = raw_small_np if align else raw_np
        raw_pin = torch.from_numpy(src_np.view(np.int16)).pin_memory()      # (torch has no uint16: the bytes are what travels)
        raw_view = raw_pin.numpy().view(np.uint16)
        fbuf = torch.zeros((T, H, W), dtype=torch.float32).pin_memory()     # variant (a): one pinned float frame per frame of a batch
        fbuf_np = fbuf.numpy()
        pre = None
        if align:
            pre = np.stack([ops.depth_align(src_np[k], dcam, cam, SCALE, None, align_t) for k in range(n_run)])

        def leg(form, sample_kernels=False):
            eng = make_engine(st, cam, n_obj, T)
            eng.enable_flow()
            if form == "raw":
                if align:
                    eng.enable_raw_depth(SCALE, cam=dcam, t=align_t)
                else:
                    eng.enable_raw_depth(SCALE)
            eng.enable_log(n_run)
            batches = []
            for k0, t in batches_kt:
                fl = []
                for j, k in enumerate(range(k0, k0 + t)):
                    pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                    depth = raw_pin[k].data_ptr() if form == "raw" else fbuf[j].data_ptr()
                    row = []
                    for o in range(n_obj):
                        f = dict(depth=depth, mask=None, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST, image=gray[k].data_ptr(), image_type=L.IMAGE_GRAY8)
                        if k in labels:
                            f.update(labels=labels[k].data_ptr(), label_type=L.LABEL_U8, label=o + 1)
                        row.append(f)
                    fl.append(row)
                arr, keep, t_ = eng.build_batch(fl)
                batches.append((k0, arr, keep, t_, eng.batch_labels(keep), eng.batch_images(keep)))

            conv_us, kern_us = [], []

            def prepare(k0, t):
                """variant (a): what the caller does to the sensor's frames before it can submit them"""
                if form == "raw":
                    return
                c0 = time.perf_counter()
                for j in range(t):
                    if align:
                        fbuf_np[j][...] = pre[k0 + j]
                    else:
                        np.multiply(raw_view[k0 + j].astype(np.float32), np.float32(SCALE), out=fbuf_np[j])
                conv_us.append(1e6 * (time.perf_counter() - c0))

            k0, arr, _keep, t, lab, img = batches[0]
            prepare(k0, t)
            eng.submit_batch_raw(arr, t, lab, img)   # first batch: allocations, first touch of the pinned pages
            eng.step()
            eng.sync()
            del conv_us[:]
            s0 = eng.stats()
            t1 = time.perf_counter()
            for k0, arr, _keep, t, lab, img in batches[1:]:
                prepare(k0, t)
                eng.submit_batch_raw(arr, t, lab, img)
                if sample_kernels and form == "raw":
                    kern_us.append(1e3 * eng.depth_kernel_ms())
                eng.step()
            eng.sync()
            dt = time.perf_counter() - t1
            s1 = eng.stats()
            frames = s1["frames"] - s0["frames"]
            tr = [b for b in eng.batch_trace() if b["batch"] >= 1]
            res = dict(value=n_obj * frames / dt, unit="object-frames/s", ms_per_step=1e3 * dt / frames,
                       h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / frames / 1e6,
                       host_us_per_submit=float(np.median([b["submit_us"] - b["wait_us"] for b in tr])),
                       wait_us_per_submit=float(np.median([b["wait_us"] for b in tr])),
                       host_us_per_step=float(np.median([b["step_us"] for b in tr])), us_per_batch=1e6 * dt / max(len(batches) - 1, 1),
                       host_convert_us_per_batch=float(np.median(conv_us)) if conv_us else 0.0,
                       launches_per_step=(s1["launches"] - s0["launches"]) / frames, depth_stats=eng.depth_stats(),
                       depth_kernel_us_per_batch=float(np.median(kern_us)) if kern_us else None, rows=eng.get_log_rows(0, n_run))
            eng.close()
            return res

        runs, rows = {"float": [], "raw": []}, {}
        for _ in range(args.windows):
            for form in ("float", "raw"):
                r = leg(form)
                rows.setdefault(form, r.pop("rows"))
                r.pop("rows", None)
                runs[form].append(r)
        kernels = leg("raw", sample_kernels=True)["depth_kernel_us_per_batch"]

        def median(form):
            rs = sorted(runs[form], key=lambda r: r["value"])
            med = dict(rs[len(rs) // 2])
            med["windows"] = [r["value"] for r in rs]
            return med

        same = bool(np.array_equal(rows["float"], rows["raw"], equal_nan=True))
        a, b = median("float"), median("raw")
        b["depth_kernel_us_per_batch"] = kernels
        b["depth_kernel_us_per_frame"] = kernels / T if kernels is not None else None
        result["throughput"][name] = dict(host_float_depth=a, raw_depth=b, ratio_raw_over_float=b["value"] / a["value"],
                                          bytes_ratio_float_over_raw=a["h2d_MB_per_step"] / b["h2d_MB_per_step"], identical_results=same)
        print(name, json.dumps({k: result["throughput"][name][k] for k in ("ratio_raw_over_float", "bytes_ratio_float_over_raw", "identical_results")}))
        for form, r in (("float", a), ("raw", b)):
            print(" ", form, json.dumps({k: r[k] for k in ("value", "h2d_MB_per_step", "host_us_per_submit", "host_us_per_step", "us_per_batch",
                                                           "wait_us_per_submit", "host_convert_us_per_batch", "depth_kernel_us_per_batch", "windows")}))
        if not same:
            raise SystemExit("bench_raw_depth.py: the two variants did not track to identical poses (%s)" % name)

    # ---- live latency ----------------------------------------------------------------------------------------------------
    camb = synth.Camera.shape_b()
    if args.scale > 1:
        camb = camb.scaled(args.scale)
    n_live = args.live_frames
    stb = synth.make_stream(4400, n_live, camb, flow_type=L.FLOW_S16C2, device=dev, with_gray=True)
    raw_b, gray_b, masks_b = quantise(stb.depth), stb.gray.cpu().numpy(), stb.mask_gt.cpu().numpy()

    def live(form):
        eng = make_engine(stb, camb, 1, 1)
        eng.enable_flow()
        if form == "raw":
            eng.enable_raw_depth(SCALE)
        lat, poses = [], []
        for k in range(n_live):
            mi = int(stb.mask_delivery[k])
            pose = (stb.pose_meas[k, :3], stb.pose_meas[k, 3:]) if stb.pose_valid[k] else None
            f = dict(mask=masks_b[mi] if mi >= 0 else None, pose=pose, dt=stb.dt, image=gray_b[k])
            t0 = time.perf_counter()
            f["depth"] = raw_b[k] if form == "raw" else raw_b[k].astype(np.float32) * np.float32(SCALE)
            eng.submit([f])
            eng.step()
            poses.append(eng.state(0)[0])
            lat.append(1e6 * (time.perf_counter() - t0))
        eng.close()
        return lat, np.array(poses)

    live_res, live_poses = {}, {}
    for rep in range(2):           # (the first pass of each form warms allocations; the second is reported)
        for form in ("float", "raw"):
            lat, live_poses[form] = live(form)
            steady = lat[2:]
            live_res[form] = dict(median_us=float(np.median(steady)), p90_us=float(np.percentile(steady, 90)), frames=len(steady))
    result["live_latency"] = dict(config=dict(width=camb.width, height=camb.height, flow="camera images, CV_16SC2", objects=1),
                                  host_convert_then_submit=live_res["float"], raw_frame_on_engine=live_res["raw"],
                                  identical_results=bool(np.array_equal(live_poses["float"], live_poses["raw"])),
                                  ratio_today_over_engine=live_res["float"]["median_us"] / live_res["raw"]["median_us"])
    print("live", json.dumps(result["live_latency"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
