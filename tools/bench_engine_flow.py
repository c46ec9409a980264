#!/usr/bin/env python3
"""Camera images on the engine against flow frames over the bus.

Throughput.  bench.py's shared-scene HOST leg with label-image masks: one camera stream for all objects in pinned host buffers
handed over as ROFT_MEM_HOST, full batches of --batch frames, the first batch untimed.  Variant (a) hands the flow frame of every
camera frame (what ops.optical_flow gives for the stream's gray images, so both variants track identical inputs), variant (b) the
gray image itself on an engine with enable_flow().  For CV_32FC2 and for CV_16SC2 the two variants alternate in one process,
--windows times each; the median window is reported with object-frames/s, MB per step and GB/s over the bus, and the host
microseconds per submit call and per roft_step (roft_batch_trace: submit_us - wait_us, step_us) next to the period of a batch:
where the two host times add up to the period, the leg is bound by the host's serial submit + step, not by the device.  The
producer's kernel time per batch is measured apart, with HIP events around one batch's worth of work (T images, T pairs) of the
same kernels on a producer of the same shape.

Live latency.  One object, 1280 x 720 CV_16SC2, one frame per submit with the state read back after each: today's path
(ops.optical_flow on the two gray images, then a submit with the HOST flow) against the image handed to the engine.

Writes profiles/r11_engine_flow.json.  No ratio is asserted: the tool reports what it finds and checks only that both variants
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


def consistency_legs(args, default_out):
    """Images on the engine, check on / off alternated args.windows times: n_obj objects of ONE scene in batches of T frames at
    640 x 480 (object-frames/s), and one object fed frame by frame at 1280 x 720 (submit + step + state, microseconds)."""
    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))

    def engine(st, cam, n, t, on):
        cfg = E.default_config(cam.width, cam.height, L.FLOW_F32C2, max_objects=n, max_batch_frames=t)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        m0 = synth.initial_pose_from_stream(st)
        for _ in range(n):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, *st.mesh)
        eng.enable_flow(consistency=True if on else None)
        return eng

    def scaled(cam):
        return cam.scaled(args.scale) if args.scale > 1 else cam

    # ---- shared scene, batches -------------------------------------------------------------------------------------------
    cam = scaled(synth.Camera.shape_a())
    n_run = T + args.frames
    st = synth.make_stream(4100, n_run, cam, flow_type=L.FLOW_F32C2, device=dev, with_gray=True)
    depth, gray = st.depth[:n_run].cpu().pin_memory(), st.gray[:n_run].cpu().pin_memory()
    masks = st.mask_gt.cpu().pin_memory()

    def leg(on):
        eng = engine(st, cam, n_obj, T, on)
        batches = []
        for k0 in range(0, n_run, T):
            fl = []
            for k in range(k0, min(n_run, k0 + T)):
                pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                mi = int(st.mask_delivery[k])
                fl.append([dict(depth=depth[k].data_ptr(), mask=masks[mi].data_ptr() if mi >= 0 else None, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST,
                                image=gray[k].data_ptr(), image_type=L.IMAGE_GRAY8) for _ in range(n_obj)])
            arr, keep, t_ = eng.build_batch(fl)
            batches.append((arr, keep, t_, eng.batch_labels(keep), eng.batch_images(keep)))
        eng.submit_batch_raw(*[batches[0][i] for i in (0, 2, 3, 4)])
        eng.step()
        eng.sync()
        f0 = eng.stats()["frames"]
        t1 = time.perf_counter()
        for arr, _keep, t, lab, img in batches[1:]:
            eng.submit_batch_raw(arr, t, lab, img)
            eng.step()
        eng.sync()
        dt = time.perf_counter() - t1
        frames = eng.stats()["frames"] - f0
        pairs = eng.flow_stats()["pairs"]
        eng.close()
        return n_obj * frames / dt, 1e3 * dt / frames, pairs

    shared = dict(off=[], on=[])
    for _ in range(args.windows):
        for name in ("off", "on"):
            shared[name].append(leg(name == "on"))

    # ---- live, frame by frame ----------------------------------------------------------------------------------------------
    camb = scaled(synth.Camera.shape_b())
    n_live = args.live_frames
    sb = synth.make_stream(4200, n_live, camb, flow_type=L.FLOW_F32C2, device=dev, with_gray=True)
    depth_b, gray_b, masks_b = sb.depth.cpu().numpy(), sb.gray.cpu().numpy(), sb.mask_gt.cpu().numpy()

    def live(on):
        eng = engine(sb, camb, 1, 1, on)
        lat = []
        for k in range(n_live):
            mi = int(sb.mask_delivery[k])
            pose = (sb.pose_meas[k, :3], sb.pose_meas[k, 3:]) if sb.pose_valid[k] else None
            f = dict(depth=depth_b[k], mask=masks_b[mi] if mi >= 0 else None, pose=pose, dt=sb.dt, image=gray_b[k])
            t0 = time.perf_counter()
            eng.submit([f])
            eng.step()
            eng.state(0)
            lat.append(1e6 * (time.perf_counter() - t0))
        eng.close()
        return float(np.median(lat[2:]))

    lives = dict(off=[], on=[])
    for rnd in range(args.windows + 1):      # (round 0 warms allocations)
        for name in ("off", "on"):
            v = live(name == "on")
            if rnd:
                lives[name].append(v)

    med = lambda v: float(sorted(v)[len(v) // 2])
    result = dict(
        shared_scene=dict(config=dict(objects=n_obj, width=cam.width, height=cam.height, batch=T, timed_frames=args.frames, windows=args.windows),
                          object_frames_per_s_off=med([r[0] for r in shared["off"]]), object_frames_per_s_on=med([r[0] for r in shared["on"]]),
                          ms_per_step_off=med([r[1] for r in shared["off"]]), ms_per_step_on=med([r[1] for r in shared["on"]]),
                          windows_off=[r[0] for r in shared["off"]], windows_on=[r[0] for r in shared["on"]],
                          pairs_off=shared["off"][0][2], pairs_on=shared["on"][0][2]),
        live_latency=dict(config=dict(width=camb.width, height=camb.height, flow="CV_32FC2", objects=1, frames=n_live - 2, rounds=args.windows),
                          median_us_off=med(lives["off"]), median_us_on=med(lives["on"]), rounds_off=lives["off"], rounds_on=lives["on"]))
    print(json.dumps(result))
    if args.out != default_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=48, help="timed frames per window")
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--scale", type=int, default=1, help="divide the cameras (a quick look on a small shape)")
    p.add_argument("--live-frames", type=int, default=40)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_engine_flow.json"))
    p.add_argument("--consistency", action="store_true",
                   help="instead of flows against images: images with the forward-backward check (roft_engine_enable_flow_consistency) "
                        "ON against OFF, CV_32FC2, alternated in one process -- the shared-scene throughput leg and the live leg; "
                        "prints one JSON line (and writes --out when it is given explicitly)")
    args = p.parse_args()
    if args.consistency:
        return consistency_legs(args, p.get_default("out"))

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import ops, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))

    def produced_flows(gray, ft):
        """[n, ...] flow frames of a gray stream (frame 0: zeros, not valid), by the batched producer"""
        n, H, W = gray.shape
        g = gray.to(dev)
        shape = (H, W, 2) if ft == L.FLOW_F32C2 else (H // 4, W // 4, 2)
        out = torch.zeros((n,) + shape, dtype=torch.float32 if ft == L.FLOW_F32C2 else torch.int16, device=dev)
        fp = ops.FlowProducer(W, H, 16, ft)
        torch.cuda.synchronize()
        for k0 in range(1, n, 16):
            ks = range(k0, min(n, k0 + 16))
            fp.run([g[k - 1].data_ptr() for k in ks], [g[k].data_ptr() for k in ks], [out[k].data_ptr() for k in ks])
            fp.sync()
        # the producer's kernels for one batch of the engine's shape: T images of a stream, T pairs
        s = torch.cuda.ExternalStream(fp.stream)
        ks = range(1, min(n, T + 1))
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            fp.run([g[k - 1].data_ptr() for k in ks], [g[k].data_ptr() for k in ks], [out[k].data_ptr() for k in ks])
            e1.record(s)
            fp.sync()
            times.append(e0.elapsed_time(e1) * 1e3)
        fp.close()
        return out.cpu(), dict(pairs=len(ks), pyramids=len(ks) + 1, kernel_us_per_batch=float(np.median(times)))

    # ---- throughput ------------------------------------------------------------------------------------------------------
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    W, H = cam.width, cam.height
    n_run = T + args.frames
    result = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, windows=args.windows), throughput={})
    for name, ft in (("f32c2", L.FLOW_F32C2), ("s16c2", L.FLOW_S16C2)):
        st = synth.make_stream(4100, n_run, cam, flow_type=ft, device=dev, with_gray=True)
        depth = st.depth[:n_run].cpu().pin_memory()
        gray = st.gray[:n_run].cpu().pin_memory()
        flow_t, producer = produced_flows(st.gray[:n_run], ft)
        flow = flow_t.pin_memory()
        deal = torch.from_numpy(((np.arange(W)[None, :] + 3 * np.arange(H)[:, None]) % n_obj + 1).astype(np.int32))
        labels = {}
        for k in range(n_run):
            mi = int(st.mask_delivery[k])
            if mi >= 0:
                labels[k] = torch.where(st.mask_gt[mi].cpu() > 0, deal, torch.zeros_like(deal)).to(torch.uint8).pin_memory()
        batches_kt = [(k0, min(T, n_run - k0)) for k0 in range(0, n_run, T)]

        def leg(form):
            cfg = E.default_config(W, H, ft, max_objects=n_obj, max_batch_frames=T)
            cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
            cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
            eng = E.ROFTFilterBatch(cfg)
            m0 = synth.initial_pose_from_stream(st)
            for _ in range(n_obj):
                d = E.default_object()
                for i in range(13):
                    d.p_mean0[i] = m0[i]
                eng.add_object(d, *st.mesh)
            if form == "images":
                eng.enable_flow()
            eng.enable_log(n_run)
            batches = []
            for k0, t in batches_kt:
                fl = []
                for k in range(k0, k0 + t):
                    pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                    row = []
                    for o in range(n_obj):
                        f = dict(depth=depth[k].data_ptr(), mask=None, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST)
                        if form == "images":
                            f.update(image=gray[k].data_ptr(), image_type=L.IMAGE_GRAY8)
                        elif k > 0:
                            f["flow"] = flow[k].data_ptr()
                        if k in labels:
                            f.update(labels=labels[k].data_ptr(), label_type=L.LABEL_U8, label=o + 1)
                        row.append(f)
                    fl.append(row)
                arr, keep, t_ = eng.build_batch(fl)
                batches.append((arr, keep, t_, eng.batch_labels(keep), eng.batch_images(keep)))
            eng.submit_batch_raw(*[batches[0][i] for i in (0, 2, 3, 4)])   # first batch: allocations, first touch of the pinned pages
            eng.step()
            eng.sync()
            s0 = eng.stats()
            t1 = time.perf_counter()
            for arr, _keep, t, lab, img in batches[1:]:
                eng.submit_batch_raw(arr, t, lab, img)
                eng.step()
            eng.sync()
            dt = time.perf_counter() - t1
            s1 = eng.stats()
            frames = s1["frames"] - s0["frames"]
            tr = [b for b in eng.batch_trace() if b["batch"] >= 1]
            res = dict(value=n_obj * frames / dt, unit="object-frames/s", ms_per_step=1e3 * dt / frames,
                       h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / frames / 1e6, h2d_GB_per_s=(s1["h2d_bytes"] - s0["h2d_bytes"]) / dt / 1e9,
                       host_us_per_submit=float(np.median([b["submit_us"] - b["wait_us"] for b in tr])),
                       wait_us_per_submit=float(np.median([b["wait_us"] for b in tr])),
                       host_us_per_step=float(np.median([b["step_us"] for b in tr])), us_per_batch=1e6 * dt / max(len(batches) - 1, 1),
                       launches_per_step=(s1["launches"] - s0["launches"]) / frames, flow_stats=eng.flow_stats(),
                       rows=eng.get_log_rows(0, n_run))
            eng.close()
            return res

        runs, rows = {"flows": [], "images": []}, {}
        for _ in range(args.windows):
            for form in ("flows", "images"):
                r = leg(form)
                rows.setdefault(form, r.pop("rows"))
                r.pop("rows", None)
                runs[form].append(r)

        def median(form):
            rs = sorted(runs[form], key=lambda r: r["value"])
            med = dict(rs[len(rs) // 2])
            med["windows"] = [r["value"] for r in rs]
            return med

        same = bool(np.array_equal(rows["flows"], rows["images"], equal_nan=True))
        a, b = median("flows"), median("images")
        result["throughput"][name] = dict(host_flow_frames=a, host_gray_images=b, ratio_images_over_flows=b["value"] / a["value"],
                                          bytes_ratio_flows_over_images=a["h2d_MB_per_step"] / b["h2d_MB_per_step"],
                                          producer=producer, identical_results=same)
        print(name, json.dumps({k: result["throughput"][name][k] for k in ("ratio_images_over_flows", "bytes_ratio_flows_over_images", "identical_results", "producer")}))
        for form, r in (("flows", a), ("images", b)):
            print(" ", form, json.dumps({k: r[k] for k in ("value", "h2d_MB_per_step", "h2d_GB_per_s", "host_us_per_submit", "host_us_per_step", "us_per_batch", "wait_us_per_submit", "windows")}))
        if not same:
            raise SystemExit("bench_engine_flow.py: the two variants did not track to identical poses (%s)" % name)

    # ---- live latency ----------------------------------------------------------------------------------------------------
    camb = synth.Camera.shape_b()
    if args.scale > 1:
        camb = camb.scaled(args.scale)
    n_live = args.live_frames
    st = synth.make_stream(4200, n_live, camb, flow_type=L.FLOW_S16C2, device=dev, with_gray=True)
    depth, gray, masks = st.depth.cpu().numpy(), st.gray.cpu().numpy(), st.mask_gt.cpu().numpy()

    def live(form):
        cfg = E.default_config(camb.width, camb.height, L.FLOW_S16C2, max_objects=1)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = camb.fx, camb.fy, camb.cx, camb.cy
        cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
        eng = E.ROFTFilterBatch(cfg)
        d = E.default_object()
        m0 = synth.initial_pose_from_stream(st)
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, *st.mesh)
        if form == "images":
            eng.enable_flow()
        lat, poses = [], []
        for k in range(n_live):
            mi = int(st.mask_delivery[k])
            pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
            f = dict(depth=depth[k], mask=masks[mi] if mi >= 0 else None, pose=pose, dt=st.dt)
            t0 = time.perf_counter()
            if form == "images":
                f["image"] = gray[k]
            elif k > 0:
                f["flow"] = ops.optical_flow(gray[k - 1], gray[k], flow_type=L.FLOW_S16C2)
            eng.submit([f])
            eng.step()
            poses.append(eng.state(0)[0])
            lat.append(1e6 * (time.perf_counter() - t0))
        eng.close()
        return lat, np.array(poses)

    live_res, live_poses = {}, {}
    for rep in range(2):           # (the first pass of each form warms allocations; the second is reported)
        for form in ("flows", "images"):
            lat, live_poses[form] = live(form)
            steady = lat[2:]
            live_res[form] = dict(median_us=float(np.median(steady)), p90_us=float(np.percentile(steady, 90)), frames=len(steady))
    result["live_latency"] = dict(config=dict(width=camb.width, height=camb.height, flow="CV_16SC2", objects=1), optical_flow_then_submit=live_res["flows"],
                                  image_on_engine=live_res["images"], identical_results=bool(np.array_equal(live_poses["flows"], live_poses["images"])),
                                  ratio_today_over_engine=live_res["flows"]["median_us"] / live_res["images"]["median_us"])
    print("live", json.dumps(result["live_latency"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
