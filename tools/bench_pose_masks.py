#!/usr/bin/env python3
"""Masks from poses against per-object HOST masks: what the feature saves on the bus and what it costs on the device.

Two legs, each once with the silhouettes of the delivered poses handed over as per-object byte masks (form "masks": one buffer per
object and delivery) and once with the objects enrolled and no mask at all (form "pose": roft_engine_enable_pose_masks):
  * host      bench.py's shared-scene HOST leg -- one camera stream (depth + CV_32FC2 flow) for all objects in pinned host buffers
              handed over as ROFT_MEM_HOST, the masks of form "masks" in pinned buffers too;
  * resident  the same inputs in device memory (ROFT_MEM_DEVICE): nothing crosses the bus in either form, the silhouette launch is
              pure cost.
Full batches of --batch frames, the first batch untimed, the median of --runs runs; the two forms alternate in one process
(A B A B A B).  The byte masks of form "masks" are the contract's definition rendered by the CPU oracle (ro_render_depth at divider
1, > 0), so both forms track identical inputs: the tool compares their logs before it reports, and fails when they differ; it also
records whether the stand-alone operator (roft_pose_silhouette) returns those masks.

A third, instrumented pass (roft_engine_enable_timing(2), never the rates above) reads: the silhouette launch's device time per
delivering batch (roft_debug_pose_mask_kernel_ms after every batch), the `pose_silhouettes` mark next to the other marks of the same
run, and -- on engines created with ROFT_PREP_AHEAD=2, where the preparation runs on the upload stream and the mark brackets it --
`mask_prepare` per batch for both forms.  With --marks FILE the marks of the "pose" form's host leg are dumped (ROFT_DUMP_MARKS) and
summarised by tools/marks_timeline.py into FILE: where the launch sits in a burst and in the steady state.

Writes profiles/r14_pose_masks.json.

--occlusion: the shared scene with poses laid out so that the objects OVERLAP (an 8-column grid of offsets around the stream's
pose, staggered in depth), three forms of the host leg alternated in one process, --runs rounds, medians:
  * occlusion  the objects enrolled and declared one scene (roft_engine_enable_pose_mask_occlusion): each keeps the pixels where it
               is the nearest surface;
  * pose       the objects enrolled without the mode (plain silhouettes: other masks, the same work elsewhere);
  * masks      the RESOLVED silhouettes -- the CPU oracle's renders resolved in numpy by the header's definition -- uploaded as
               per-object HOST masks: the caller the mode replaces.  Its log must equal the occlusion form's.
An instrumented pass reads the silhouette stage's device time (roft_debug_pose_mask_kernel_ms: draw + resolve) per delivering batch
with the mode on and off.  Prints the share of the plain silhouettes' pixels the resolve removed.  Writes
profiles/r15_pose_mask_occlusion.json.

--depth-gate: what roft_engine_enable_pose_mask_depth_gate costs.  The shared scene's host leg in the shape of the "pose" form above
(the plain path: every pair drawn alone) and in the overlapping layout of --occlusion with the mode on (the occlusion path: draw +
resolve), each with the gate on and off, alternated in one process for --runs rounds (5 unless given): object-frames/s, medians, and
-- from an instrumented pass -- the silhouette stage's device time per delivering batch (roft_debug_pose_mask_kernel_ms).  The gate
reads the stream's own depth, with the front tolerance 0.02 and the behind test at 0.05.  Writes
profiles/r17_pose_mask_depth_gate.json.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--objects", type=int, default=64)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--frames", type=int, default=96, help="timed frames per run")
    p.add_argument("--runs", type=int, default=3)
    p.add_argument("--scale", type=int, default=1, help="divide the 640 x 480 camera (a quick look on a small shape)")
    p.add_argument("--marks", default=os.path.join(ROOT, "profiles", "r14_marks_timeline.txt"))
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_pose_masks.json"))
    p.add_argument("--occlusion", action="store_true", help="the three forms of the overlapping shared scene (see above)")
    p.add_argument("--depth-gate", action="store_true", help="the depth gate on against off, on the plain and the occlusion path (see above)")
    args = p.parse_args()
    if args.depth_gate:
        if args.out.endswith("r14_pose_masks.json"):
            args.out = os.path.join(ROOT, "profiles", "r17_pose_mask_depth_gate.json")
        if "--runs" not in sys.argv:
            args.runs = 5
        return depth_gate(args)
    if args.occlusion:
        if args.out.endswith("r14_pose_masks.json"):
            args.out = os.path.join(ROOT, "profiles", "r15_pose_mask_occlusion.json")
        return occlusion(args)

    import torch
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import ops, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    n_run = T + args.frames
    st = synth.make_stream(4000, n_run, cam, flow_type=synth.FLOW_F32C2, device=dev, mesh_n=12)
    W, H = cam.width, cam.height
    verts, tris = st.mesh
    lib_cam = L.Camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)

    depth_h = st.depth[:n_run].cpu().pin_memory()
    flow_h = st.flow[:n_run].cpu().pin_memory()
    depth_d, flow_d = st.depth[:n_run].contiguous(), st.flow[:n_run].contiguous()
    deliveries = [k for k in range(n_run) if st.pose_valid[k]]
    # the byte masks of form "masks": the contract's own definition, rendered by the CPU oracle; the stand-alone operator must agree
    from oracle import binding as ob
    o_mesh, o_cam = ob.make_mesh(verts, tris), ob.camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    sil = {k: np.ascontiguousarray((ob.render_depth(o_mesh, st.pose_meas[k, :3], st.pose_meas[k, 3:], o_cam, 1) > 0).astype(np.uint8) * 255)
           for k in deliveries}
    operator_agrees = all(np.array_equal(ops.pose_silhouette(lib_cam, (verts, tris), st.pose_meas[k, :3], st.pose_meas[k, 3:])[0], sil[k])
                          for k in deliveries)
    masks_h = {k: torch.from_numpy(m)[None].repeat(n_obj, 1, 1).pin_memory() for k, m in sil.items()}   # one buffer per object
    masks_d = {k: m.to(dev) for k, m in masks_h.items()}
    batches_kt = [(k0, min(T, n_run - k0)) for k0 in range(0, n_run, T)]
    delivering_batches = sum(1 for k0, t in batches_kt[1:] if any(k0 <= k < k0 + t for k in deliveries))

    def new_engine(form, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v                   # (read when the engine is created)
        try:
            cfg = E.default_config(W, H, st.flow_type, max_objects=n_obj, max_batch_frames=T)
            cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
            eng = E.ROFTFilterBatch(cfg)
        finally:
            for k in (env or {}):
                os.environ.pop(k, None)
        m0 = synth.initial_pose_from_stream(st)
        for _ in range(n_obj):
            d = E.default_object()
            for i in range(13):
                d.p_mean0[i] = m0[i]
            eng.add_object(d, verts, tris)
        if form == "pose":
            eng.enable_pose_masks()
        return eng

    def build(eng, form, leg_kind):
        host = leg_kind == "host"
        depth, flow, masks = (depth_h, flow_h, masks_h) if host else (depth_d, flow_d, masks_d)
        out = []
        for k0, t in batches_kt:
            fl = []
            for k in range(k0, k0 + t):
                pose = (st.pose_meas[k, :3], st.pose_meas[k, 3:]) if st.pose_valid[k] else None
                row = []
                for o in range(n_obj):
                    f = dict(depth=depth[k].data_ptr(), flow=flow[k].data_ptr() if st.flow_valid[k] else None, mask=None, pose=pose, dt=st.dt,
                             mem_kind=L.MEM_HOST if host else L.MEM_DEVICE)
                    if form == "masks" and k in masks:
                        f["mask"] = masks[k][o].data_ptr()
                    row.append(f)
                fl.append(row)
            arr, keep, t_ = eng.build_batch(fl)
            out.append((arr, keep, t_))
        return out

    def leg(form, leg_kind, timing=False, env=None, marks=None, read_kernel=False):
        eng = new_engine(form, env)
        eng.enable_log(n_run)
        batches = build(eng, form, leg_kind)
        eng.submit_batch_raw(batches[0][0], batches[0][2])   # first batch: allocations, first touch of the pinned pages
        eng.step()
        eng.sync()
        if timing:
            eng.enable_timing(2)
        kernel_us, last_drawn = [], eng.pose_mask_stats()["silhouettes"]
        s0 = eng.stats()
        t1 = time.perf_counter()
        for arr, _keep, t in batches[1:]:
            eng.submit_batch_raw(arr, t)
            eng.step()
            if read_kernel:   # (waits for the launch: this pass is not a timeline)
                drawn = eng.pose_mask_stats()["silhouettes"]
                if drawn != last_drawn:
                    last_drawn = drawn
                    try:
                        kernel_us.append(1e3 * eng.pose_mask_kernel_ms())
                    except L.RoftError:
                        kernel_us.append(None)    # (ended with the preparation's event: not timed)
        eng.sync()
        dt = time.perf_counter() - t1
        s1 = eng.stats()
        res = dict(frames=s1["frames"] - s0["frames"])
        if timing:
            if marks:
                os.environ["ROFT_DUMP_MARKS"] = marks
            try:
                tm = eng.timing()
            finally:
                os.environ.pop("ROFT_DUMP_MARKS", None)
            res["marks_us_avg"] = {name: dict(n=int(n), avg_us=1e3 * float(ms) / max(int(n), 1)) for name, (ms, n) in tm.items()}
            timed = [u for u in kernel_us if u is not None]
            if read_kernel:
                res.update(silhouette_launches_timed=len(timed), silhouette_launches_untimed=len(kernel_us) - len(timed),
                           silhouette_kernel_us=dict(median=float(np.median(timed)), min=float(np.min(timed)), max=float(np.max(timed))) if timed else None)
        else:
            res.update(value=n_obj * res["frames"] / dt, unit="object-frames/s", ms_per_step=1e3 * dt / res["frames"],
                       h2d_GB_per_s=(s1["h2d_bytes"] - s0["h2d_bytes"]) / dt / 1e9,
                       h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / res["frames"] / 1e6,
                       launches_per_step=(s1["launches"] - s0["launches"]) / res["frames"])
        res["rows"] = eng.get_log_rows(0, n_run)
        if form == "pose":
            res["pose_mask_stats"] = eng.pose_mask_stats()
        eng.close()
        return res

    out = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, runs=args.runs, flow="CV_32FC2",
                           mesh_vertices=int(verts.shape[0]), mesh_triangles=int(tris.shape[0]), deliveries=len(deliveries),
                           delivering_batches_timed=delivering_batches))
    same = True
    for leg_kind in ("host", "resident"):
        runs, rows = {"masks": [], "pose": []}, {}
        for _ in range(args.runs):
            for form in ("masks", "pose"):
                r = leg(form, leg_kind)
                rows.setdefault(form, r["rows"])
                r.pop("rows")
                runs[form].append(r)
        same = same and bool(np.array_equal(rows["masks"], rows["pose"], equal_nan=True))

        def median(form):
            rs = sorted(runs[form], key=lambda r: r["value"])
            med = dict(rs[len(rs) // 2])
            med["runs"] = [r["value"] for r in rs]
            return med

        out[leg_kind] = dict(per_object_masks=median("masks"), pose_masks=median("pose"))
        out[leg_kind]["ratio_pose_over_masks"] = out[leg_kind]["pose_masks"]["value"] / out[leg_kind]["per_object_masks"]["value"]
    out["identical_results"] = same
    out["operator_equals_oracle"] = bool(operator_agrees)

    # instrumented passes
    marks_raw = os.path.join(tempfile.mkdtemp(), "marks.txt") if args.marks else None
    timing = {}
    for form in ("masks", "pose"):
        r = leg(form, "host", timing=True, marks=marks_raw if form == "pose" else None)
        r.pop("rows")
        timing[form] = r
        if form == "pose":
            k = leg(form, "host", timing=True, read_kernel=True)
            timing[form].update({key: k[key] for key in ("silhouette_launches_timed", "silhouette_launches_untimed", "silhouette_kernel_us")})
        r = leg(form, "host", timing=True, env={"ROFT_PREP_AHEAD": "2"}, read_kernel=form == "pose")
        r.pop("rows")
        timing[form + "_prep_ahead"] = dict(mask_prepare=r["marks_us_avg"].get("mask_prepare"), silhouette_kernel_us=r.get("silhouette_kernel_us"),
                                            silhouette_launches_untimed=r.get("silhouette_launches_untimed"))
    out["timing"] = dict(timing, note="separate, instrumented runs of the host leg under roft_engine_enable_timing(2); marks_us_avg: every "
                                      "mark's average; silhouette_kernel_us: roft_debug_pose_mask_kernel_ms after each delivering batch; "
                                      "*_prep_ahead: engines created with ROFT_PREP_AHEAD=2, where mask_prepare brackets the whole preparation "
                                      "of a batch on the upload stream (control blocks + ingest, and the silhouette launch in the pose form)")
    if marks_raw and os.path.exists(marks_raw):
        txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "marks_timeline.py"), marks_raw, "--list"], capture_output=True, text=True).stdout
        with open(args.marks, "w") as f:
            f.write("# tools/bench_pose_masks.py: the pose form's host leg, %d objects %d x %d, batches of %d -- batches 1 .. 5 behind the sync are a burst,\n"
                    "# later ones the steady state (plan_batch); columns of the list: stream, mark, start us, end us, duration us\n" % (n_obj, W, H, T))
            f.write(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(dict(config=out["config"], identical_results=same, operator_equals_oracle=bool(operator_agrees))))
    for leg_kind in ("host", "resident"):
        for form in ("per_object_masks", "pose_masks"):
            print(leg_kind, form, json.dumps({k: out[leg_kind][form][k] for k in ("value", "h2d_MB_per_step", "h2d_GB_per_s", "ms_per_step", "runs")}))
        print(leg_kind, "ratio pose / masks %.3f" % out[leg_kind]["ratio_pose_over_masks"])
    print("timing", json.dumps({k: (v.get("silhouette_kernel_us") if isinstance(v, dict) else None) for k, v in timing.items()}))
    print("mask_prepare", json.dumps({k: v.get("mask_prepare") for k, v in timing.items() if k.endswith("_prep_ahead")}))
    if not same:
        raise SystemExit("bench_pose_masks.py: the two forms did not track to identical poses")


def occlusion(args):
    import torch
    from oracle import binding as ob
    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import ops, synth

    L.require_device()
    dev = torch.device("cuda", 0)
    cam = synth.Camera.shape_a()
    if args.scale > 1:
        cam = cam.scaled(args.scale)
    n_obj, T = args.objects, max(1, min(args.batch, L.MAX_BATCH_FRAMES))
    n_run = T + args.frames
    st = synth.make_stream(4000, n_run, cam, flow_type=synth.FLOW_F32C2, device=dev, mesh_n=12)
    W, H = cam.width, cam.height
    verts, tris = st.mesh
    depth_h = st.depth[:n_run].cpu().pin_memory()
    flow_h = st.flow[:n_run].cpu().pin_memory()
    deliveries = [k for k in range(n_run) if st.pose_valid[k]]
    # object o: the stream's pose moved to column o % 8, row o // 8 of a grid whose step is a third of the box, staggered in depth
    offsets = np.array([[(o % 8 - 3.5) * 0.06, (o // 8 - 3.5) * 0.045, 0.02 * ((o * 37) % 64) / 8.0] for o in range(n_obj)])

    def pose_of(k, o):
        return st.pose_meas[k, :3] + offsets[o], st.pose_meas[k, 3:]

    o_mesh, o_cam = ob.make_mesh(verts, tris), ob.camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy)
    resolved, raw_pixels, kept_pixels, hidden = {}, 0, 0, 0
    for k in deliveries:
        R = np.stack([np.array(ob.render_depth(o_mesh, *pose_of(k, o), o_cam, 1), np.float32) for o in range(n_obj)])
        raw = R > 0
        res = raw & (np.argmin(np.where(raw, R, np.float32(np.inf)), axis=0)[None] == np.arange(n_obj)[:, None, None])
        resolved[k] = torch.from_numpy(np.ascontiguousarray(res.astype(np.uint8) * 255)).pin_memory()
        raw_pixels += int(raw.sum())
        kept_pixels += int(res.sum())
        hidden += int((raw.any(axis=(1, 2)) & ~res.any(axis=(1, 2))).sum())
    k0 = deliveries[0]
    got = ops.pose_silhouettes_occluded(L.Camera(W, H, cam.fx, cam.fy, cam.cx, cam.cy), [(verts, tris)] * n_obj,
                                        [pose_of(k0, o)[0] for o in range(n_obj)], [pose_of(k0, o)[1] for o in range(n_obj)])[0]
    operator_agrees = bool(np.array_equal(got, resolved[k0].numpy()))
    batches_kt = [(b, min(T, n_run - b)) for b in range(0, n_run, T)]

    def leg(form, timing=False):
        cfg = E.default_config(W, H, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        eng = E.ROFTFilterBatch(cfg)
        for o in range(n_obj):
            d = E.default_object()
            x0, q0 = pose_of(0, o)
            for i in range(13):
                d.p_mean0[i] = 0.0 if i < 6 else (x0[i - 6] if i < 9 else q0[i - 9])
            eng.add_object(d, verts, tris)
        if form != "masks":
            eng.enable_pose_masks()
        if form == "occlusion":
            eng.enable_pose_mask_occlusion()
        eng.enable_log(n_run)
        batches = []
        for b, t in batches_kt:
            fl = []
            for k in range(b, b + t):
                row = []
                for o in range(n_obj):
                    f = dict(depth=depth_h[k].data_ptr(), flow=flow_h[k].data_ptr() if st.flow_valid[k] else None, mask=None,
                             pose=pose_of(k, o) if st.pose_valid[k] else None, dt=st.dt, mem_kind=L.MEM_HOST)
                    if form == "masks" and k in resolved:
                        f["mask"] = resolved[k][o].data_ptr()
                    row.append(f)
                fl.append(row)
            batches.append(eng.build_batch(fl))
        eng.submit_batch_raw(batches[0][0], batches[0][2])
        eng.step()
        eng.sync()
        if timing:
            eng.enable_timing(2)
        stage_us, last_drawn = [], eng.pose_mask_stats()["silhouettes"]
        s0 = eng.stats()
        t1 = time.perf_counter()
        for arr, _keep, t in batches[1:]:
            eng.submit_batch_raw(arr, t)
            eng.step()
            if timing:
                drawn = eng.pose_mask_stats()["silhouettes"]
                if drawn != last_drawn:
                    last_drawn = drawn
                    stage_us.append(1e3 * eng.pose_mask_kernel_ms())
        eng.sync()
        dt = time.perf_counter() - t1
        s1 = eng.stats()
        frames = s1["frames"] - s0["frames"]
        res = dict(value=n_obj * frames / dt, unit="object-frames/s", ms_per_step=1e3 * dt / frames,
                   h2d_MB_per_step=(s1["h2d_bytes"] - s0["h2d_bytes"]) / frames / 1e6, launches_per_step=(s1["launches"] - s0["launches"]) / frames,
                   rows=eng.get_log_rows(0, n_run))
        if timing:
            res["stage_us"] = dict(median=float(np.median(stage_us)), min=float(np.min(stage_us)), max=float(np.max(stage_us)), n=len(stage_us))
        if form == "occlusion":
            res["occlusion_stats"] = eng.pose_mask_occlusion_stats()
        eng.close()
        return res

    forms = ("occlusion", "pose", "masks")
    runs, rows, stats = {f: [] for f in forms}, {}, None
    for _ in range(args.runs):
        for form in forms:
            r = leg(form)
            rows.setdefault(form, r.pop("rows"))
            r.pop("rows", None)
            stats = r.pop("occlusion_stats", stats)
            runs[form].append(r)
    same = bool(np.array_equal(rows["occlusion"], rows["masks"], equal_nan=True))
    out = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, runs=args.runs, flow="CV_32FC2",
                           mesh_vertices=int(verts.shape[0]), mesh_triangles=int(tris.shape[0]), deliveries=len(deliveries)),
               oracle=dict(silhouettes=len(deliveries) * n_obj, hidden=hidden, pixels_plain=raw_pixels, pixels_resolved=kept_pixels,
                           share_removed=1.0 - kept_pixels / max(raw_pixels, 1)),
               engine_stats=stats, identical_results=same, operator_equals_oracle=operator_agrees)
    for form in forms:
        rs = sorted(runs[form], key=lambda r: r["value"])
        out[form] = dict(rs[len(rs) // 2], runs=[r["value"] for r in runs[form]])
    out["ratio_occlusion_over_masks"] = out["occlusion"]["value"] / out["masks"]["value"]
    out["ratio_occlusion_over_pose"] = out["occlusion"]["value"] / out["pose"]["value"]
    out["stage_us"] = {form: leg(form, timing=True)["stage_us"] for form in ("occlusion", "pose")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("config", "oracle", "engine_stats", "identical_results", "operator_equals_oracle")}))
    for form in forms:
        print(form, json.dumps({k: out[form][k] for k in ("value", "h2d_MB_per_step", "ms_per_step", "launches_per_step", "runs")}))
    print("ratio occlusion / masks %.3f, occlusion / pose %.3f, share of pixels removed %.3f" %
          (out["ratio_occlusion_over_masks"], out["ratio_occlusion_over_pose"], out["oracle"]["share_removed"]))
    print("stage_us", json.dumps(out["stage_us"]))
    if not same:
        raise SystemExit("bench_pose_masks.py --occlusion: the occlusion form and the resolved host masks did not track to identical poses")


def depth_gate(args):
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
    st = synth.make_stream(4000, n_run, cam, flow_type=synth.FLOW_F32C2, device=dev, mesh_n=12)
    W, H = cam.width, cam.height
    verts, tris = st.mesh
    depth_h = st.depth[:n_run].cpu().pin_memory()
    flow_h = st.flow[:n_run].cpu().pin_memory()
    offsets = np.array([[(o % 8 - 3.5) * 0.06, (o // 8 - 3.5) * 0.045, 0.02 * ((o * 37) % 64) / 8.0] for o in range(n_obj)])
    batches_kt = [(b, min(T, n_run - b)) for b in range(0, n_run, T)]

    def leg(path, gate, timing=False):
        off = offsets if path == "occlusion" else np.zeros_like(offsets)
        pose_of = lambda k, o: (st.pose_meas[k, :3] + off[o], st.pose_meas[k, 3:])
        cfg = E.default_config(W, H, st.flow_type, max_objects=n_obj, max_batch_frames=T)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
        eng = E.ROFTFilterBatch(cfg)
        for o in range(n_obj):
            d = E.default_object()
            x0, q0 = pose_of(0, o)
            for i in range(13):
                d.p_mean0[i] = 0.0 if i < 6 else (x0[i - 6] if i < 9 else q0[i - 9])
            eng.add_object(d, verts, tris)
        eng.enable_pose_masks()
        if path == "occlusion":
            eng.enable_pose_mask_occlusion()
        if gate:
            eng.enable_pose_mask_depth_gate(0.02, 0.05)
        batches = []
        for b, t in batches_kt:
            fl = [[dict(depth=depth_h[k].data_ptr(), flow=flow_h[k].data_ptr() if st.flow_valid[k] else None, mask=None,
                        pose=pose_of(k, o) if st.pose_valid[k] else None, dt=st.dt, mem_kind=L.MEM_HOST) for o in range(n_obj)]
                  for k in range(b, b + t)]
            batches.append(eng.build_batch(fl))
        eng.submit_batch_raw(batches[0][0], batches[0][2])
        eng.step()
        eng.sync()
        if timing:
            eng.enable_timing(2)
        stage_us, last_drawn = [], eng.pose_mask_stats()["silhouettes"]
        s0 = eng.stats()
        t1 = time.perf_counter()
        for arr, _keep, t in batches[1:]:
            eng.submit_batch_raw(arr, t)
            eng.step()
            if timing:
                drawn = eng.pose_mask_stats()["silhouettes"]
                if drawn != last_drawn:
                    last_drawn = drawn
                    stage_us.append(1e3 * eng.pose_mask_kernel_ms())
        eng.sync()
        dt = time.perf_counter() - t1
        s1 = eng.stats()
        frames = s1["frames"] - s0["frames"]
        res = dict(value=n_obj * frames / dt, unit="object-frames/s", ms_per_step=1e3 * dt / frames,
                   launches_per_step=(s1["launches"] - s0["launches"]) / frames, event_ops_per_step=(s1["event_ops"] - s0["event_ops"]) / frames)
        if timing:
            res["stage_us"] = dict(median=float(np.median(stage_us)), min=float(np.min(stage_us)), max=float(np.max(stage_us)), n=len(stage_us))
        res["gate_stats"] = eng.pose_mask_gate_stats()
        res["silhouettes"] = eng.pose_mask_stats()["silhouettes"]
        eng.close()
        return res

    out = dict(config=dict(objects=n_obj, width=W, height=H, batch=T, timed_frames=args.frames, rounds=args.runs, flow="CV_32FC2",
                           mesh_vertices=int(verts.shape[0]), mesh_triangles=int(tris.shape[0]), front_tolerance=0.02, behind_tolerance=0.05))
    for path in ("plain", "occlusion"):
        runs = {True: [], False: []}
        for _ in range(args.runs):
            for gate in (True, False):
                runs[gate].append(leg(path, gate))
        res = {}
        for gate, name in ((True, "gate_on"), (False, "gate_off")):
            rs = sorted(runs[gate], key=lambda r: r["value"])
            res[name] = dict(rs[len(rs) // 2], runs=[r["value"] for r in runs[gate]])
        res["ratio_on_over_off"] = res["gate_on"]["value"] / res["gate_off"]["value"]
        res["same_launches_and_event_ops"] = bool(res["gate_on"]["launches_per_step"] == res["gate_off"]["launches_per_step"]
                                                  and res["gate_on"]["event_ops_per_step"] == res["gate_off"]["event_ops_per_step"])
        res["stage_us"] = {name: leg(path, gate, timing=True)["stage_us"] for gate, name in ((True, "gate_on"), (False, "gate_off"))}
        out[path] = res
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["config"]))
    for path in ("plain", "occlusion"):
        r = out[path]
        print(path, "on %.0f off %.0f object-frames/s (ratio %.3f); stage us on %s off %s; gate stats %s" %
              (r["gate_on"]["value"], r["gate_off"]["value"], r["ratio_on_over_off"], json.dumps(r["stage_us"]["gate_on"]),
               json.dumps(r["stage_us"]["gate_off"]), json.dumps(r["gate_on"]["gate_stats"])))


if __name__ == "__main__":
    main()
