#!/usr/bin/env python3
"""Runs the MI355X engine on one object of a Fast-YCB / HO-3D style sequence directory and writes the reference's log
files (`pose_estimate`, `velocity_estimate`, ROFTFilter.cpp:386-394) -- what `test/test.sh` does with `ROFT-tracker`.

  run_sequence.py --root DIR --object NAME --mesh model.obj [--flow-set nvof_1_slow] [--mask-set NAME]
                  [--pose-set dope] [--out PREFIX] [--compute-flow nvof1|nvof2 | --flow-on-engine nvof1|nvof2] [--no-delay]
                  [--init-pose x y z qw qx qy qz] [--raw-depth SCALE]
                  [--start-at-first-detection] [--score-on-device] [--render-overlay DIR] [--quality FILE] [--masks-from-pose]
                  [--pose-mask-depth-gate FRONT[,BEHIND]] [--lens k1,k2,p1,p2,k3 [--lens-camera fx,fy,cx,cy]]
                  [--from config_fast_ycb.cfg [--group::key value ...]]

--from reads the filter parameters from one of the reference's configuration files (config/config_fast_ycb.cfg,
config/config_ho3d.cfg) and applies `--a::b::c value` overrides exactly as ROFT-tracker's ConfigParser does
(roft_amd/config.py); without it the defaults of those files are used (roft_default_config / roft_default_object).

The camera comes from DIR/cam_K.json (width, height, fx, fy, cx, cy).  --compute-flow first runs tools/flow_dumper.py
on DIR/rgb (the MI355X replacement of the NVOF dumper) into DIR/optical_flow/<flow-set>.  --flow-on-engine hands the frames
DIR/rgb/<i>.png to the engine instead, which computes the same flow itself (roft_frames_submit_images: the flow never leaves the
device, no flow directory is read or written) -- the logs are those of --compute-flow, byte for byte.  --raw-depth SCALE
tracks from the 16-bit frames DIR/depth/<i>.png (the form YCB-Video and HO-3D ship; SCALE metres per unit, 0.001 for millimetres)
without a float copy: the engine converts them on the device (roft_engine_enable_raw_depth).  With DIR/gt/poses.txt present
the ADD-S / ADD AUC and the RMSE metrics of evaluation/metrics.py are printed as one JSON line.  --score-on-device adds the
ADD-S and ADD of the same frames on EVERY vertex of the mesh, computed on the GPU from the engine's device-side log
(roft_engine_score_log: the estimates never leave the device).  --render-overlay DIR draws the estimate over the sequence's
grayed RGB frames (DIR/<frame>.png) with tools/render_results.py once the logs are written.  --quality FILE turns track quality on
(roft_engine_enable_quality) and writes one row per frame: frame, the seven counts of roft_quality_record, depth_err and the overlap
n_both / (n_mask + n_render - n_both), space separated under a header line.  --masks-from-pose tracks a directory that has
<pose-set>/poses.txt and NO masks: the object is enrolled with roft_engine_enable_pose_masks and every delivered pose brings the
silhouette of the mesh at that pose as the frame's mask, drawn on the device (DIR/masks is not read; the first frame uses the
initial pose when it brings none).  The pose source's delay is the mask's delay then: keep mask_frames_between equal to
pose_frames_between.  --pose-mask-depth-gate FRONT[,BEHIND] (with --masks-from-pose) compares every silhouette with the depth of
the image its pose was computed on (roft_engine_enable_pose_mask_depth_gate): pixels where the sensor saw something more than
FRONT metres nearer than the mesh -- a hand, clutter -- are left out, and with BEHIND > 0 those where it saw something more than
BEHIND metres farther; the report carries the gate's counts.  --lens k1,k2,p1,p2,k3 (with --flow-on-engine) says that the
directory holds the sensor's DISTORTED frames, with those Brown-Conrady coefficients (OpenCV's order): the engine rectifies depth,
masks and camera frames into the pinhole camera of cam_K.json on the device (roft_engine_enable_rectification; include/roft_engine.h
section 3g).  --lens-camera fx,fy,cx,cy gives the sensor's own intrinsics where they differ from cam_K.json's; the report carries
the rectification's counts.  (A list that starts with a minus sign is written --lens=-0.05,0.01,...)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", required=True)
    ap.add_argument("--object", required=True)
    ap.add_argument("--mesh", required=True)
    ap.add_argument("--flow-set", default="nvof_1_slow")
    ap.add_argument("--mask-set", default="mrcnn_ycbv_bop_pbr")
    ap.add_argument("--pose-set", default="dope")
    ap.add_argument("--out", default=None)
    ap.add_argument("--compute-flow", choices=["nvof1", "nvof2"], default=None)
    ap.add_argument("--flow-on-engine", choices=["nvof1", "nvof2"], default=None,
                    help="hand the camera frames rgb/<i>.png to the engine, which computes the flow (nvof1: CV_16SC2 grid 4, nvof2: CV_32FC2)")
    ap.add_argument("--flow-consistency", action="store_true",
                    help="forward-backward check of the computed flow (include/roft_engine.h section 3f): occluded pixels become "
                         "invalid; with --compute-flow nvof2 or --flow-on-engine nvof2")
    ap.add_argument("--raw-depth", type=float, default=None, metavar="SCALE",
                    help="read depth/<i>.png (16-bit gray, SCALE metres per unit) and let the engine convert it on the device")
    ap.add_argument("--no-delay", action="store_true")
    ap.add_argument("--start-at-first-detection", action="store_true",
                    help="start where test/test_ho3d.sh:68-80 starts the tracker: at the frame and with the pose "
                         "tools/dataset/dope_pose_finder/pose_finder.py reports for the 5 fps pose source")
    ap.add_argument("--init-pose", type=float, nargs=7, default=None, metavar=("X", "Y", "Z", "QW", "QX", "QY", "QZ"),
                    help="initial_condition.pose (default: the first valid detection)")
    ap.add_argument("--score-on-device", action="store_true",
                    help="also score the run on the object's full mesh with roft_engine_score_log (needs gt/poses.txt)")
    ap.add_argument("--render-overlay", default=None, metavar="DIR",
                    help="after the run, draw the estimate over SEQ/rgb/<i>.png into DIR/<i>.png (tools/render_results.py)")
    ap.add_argument("--quality", default=None, metavar="FILE",
                    help="score every estimate against its frame's mask and depth on the device; one row per frame into FILE")
    ap.add_argument("--masks-from-pose", action="store_true",
                    help="no segmentation masks: the engine draws the silhouette of every delivered pose on the device and tracks with it")
    ap.add_argument("--pose-mask-depth-gate", default=None, metavar="FRONT[,BEHIND]",
                    help="with --masks-from-pose: gate the silhouettes against the depth of the pose's own frame (tolerances in metres; BEHIND 0: off)")
    ap.add_argument("--lens", default=None, metavar="K1,K2,P1,P2,K3",
                    help="with --flow-on-engine: the frames are the sensor's distorted ones; the engine rectifies them on the device")
    ap.add_argument("--lens-camera", default=None, metavar="FX,FY,CX,CY",
                    help="with --lens: the sensor's intrinsics (default: those of cam_K.json)")
    ap.add_argument("--symmetry", default=None, metavar="FILE",
                    help="BOP models_info.json: the object's discrete symmetry group goes to the engine (a delivered pose is replaced by its "
                         "equivalent nearest to the belief) and the report gains MSSD / MSPD; needs --symmetry-id")
    ap.add_argument("--symmetry-id", type=int, default=None, metavar="N", help="the object's id in --symmetry")
    ap.add_argument("--symmetry-unit-scale", type=float, default=0.001, help="model units of --symmetry in metres (BOP: millimetres)")
    ap.add_argument("--from", dest="cfg_file", default=None, help="ROFT configuration file (libconfig), overrides as --a::b::c value")
    args, overrides = ap.parse_known_args(argv)

    from roft_amd import _lib as L
    from roft_amd import engine as E
    from roft_amd import io, metrics

    if args.compute_flow and args.flow_on_engine:
        ap.error("--compute-flow and --flow-on-engine exclude each other")
    gate = None
    if args.pose_mask_depth_gate is not None:
        if not args.masks_from_pose:
            ap.error("--pose-mask-depth-gate needs --masks-from-pose")
        try:
            gate = [float(v) for v in args.pose_mask_depth_gate.split(",")]
        except ValueError:
            gate = []
        if len(gate) not in (1, 2):
            ap.error("--pose-mask-depth-gate takes FRONT or FRONT,BEHIND (metres)")
        gate = (gate + [0.0])[:2]
    lens = None
    if args.lens_camera is not None and args.lens is None:
        ap.error("--lens-camera needs --lens")
    if args.lens is not None:
        if not args.flow_on_engine:
            ap.error("--lens needs --flow-on-engine (a flow computed between distorted frames cannot be rectified)")
        try:
            lens = [float(v) for v in args.lens.split(",")], [float(v) for v in args.lens_camera.split(",")] if args.lens_camera else None
        except ValueError:
            lens = [], None
        if len(lens[0]) != 5 or (lens[1] is not None and len(lens[1]) != 4):
            ap.error("--lens takes k1,k2,p1,p2,k3 and --lens-camera fx,fy,cx,cy")
    if args.flow_consistency and "nvof2" not in (args.compute_flow, args.flow_on_engine):
        ap.error("--flow-consistency needs --compute-flow nvof2 or --flow-on-engine nvof2 (CV_16SC2 has no invalid vector)")
    L.require_device()
    cam = json.load(open(os.path.join(args.root, "cam_K.json")))
    W, H = int(cam["width"]), int(cam["height"])
    if args.compute_flow:
        out = os.path.join(args.root, "optical_flow", args.flow_set)
        rc = subprocess.call([sys.executable, os.path.join(ROOT, "tools", "flow_dumper.py"), args.root, "txt", "png", "1", "0",
                              str(W), str(H), args.compute_flow, out] + (["--consistency"] if args.flow_consistency else []))
        if rc != 0:
            return rc
    start = 0
    if args.start_at_first_detection:
        found = io.find_initial_pose(os.path.join(args.root, args.pose_set, "poses.txt"), 5.0)
        if found is None:
            sys.stderr.write("no valid detection on the 5 fps grid\n")
            return 1
        start = found[0]
        aa = [float(v) for v in found[1].split()]
        if args.init_pose is None:
            args.init_pose = aa[:3] + list(io.axis_angle_to_quat(np.array(aa[3:6]), aa[6]))
    seq = io.Sequence(args.root, args.object, flow_set=args.flow_set, mask_set=args.mask_set, pose_set=args.pose_set,
                      width=W, height=H, delayed=not args.no_delay, first_frame=start)
    if args.flow_on_engine:
        ftype, grid, scale = (L.FLOW_S16C2, 4, 32.0) if args.flow_on_engine == "nvof1" else (L.FLOW_F32C2, 1, 1.0)
    else:
        first = None
        for k in range(len(seq)):
            ok, first = io.read_flow(os.path.join(seq.flow_dir, "%d.float" % k))
            if ok:
                break
        if first is None:
            sys.stderr.write("no optical flow frames in %s\n" % seq.flow_dir)
            return 1
        ftype, grid, scale = io.flow_format(first, W)
    init_from_cfg = False
    if args.cfg_file:
        from roft_amd import config as K
        # the sequence's own camera (cam_K.json) unless the command line says otherwise, as test/test.sh passes it
        cam_over = []
        for k in ("width", "height", "fx", "fy", "cx", "cy"):
            if "--camera_dataset::" + k not in overrides:
                cam_over += ["--camera_dataset::" + k, str(cam[k])]
        init_from_cfg = any(o.startswith("--initial_condition::pose::") for o in overrides)
        cfg, d, _extras, rest = K.load(args.cfg_file, cam_over + overrides, flow_type=ftype, flow_grid=grid, flow_scale=scale)
        if rest:
            ap.error("unknown arguments: %s" % " ".join(rest))
        if (cfg.cam.width, cfg.cam.height) != (W, H):
            ap.error("camera_dataset::width / height do not match the sequence")
    else:
        if overrides:
            ap.error("unknown arguments: %s (settings need --from FILE)" % " ".join(overrides))
        cfg = E.default_config(W, H, ftype, max_objects=1)
        cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam["fx"], cam["fy"], cam["cx"], cam["cy"]
        cfg.flow_grid, cfg.flow_scale = grid, scale
        d = E.default_object()
    eng = E.ROFTFilterBatch(cfg)
    verts, tris = io.load_obj(args.mesh)
    # initial condition: the configuration's when it was given on the command line (test/test.sh:120-123 passes the first
    # detection that way), else the first valid detection of the sequence
    if args.start_at_first_detection:
        init_from_cfg = False
    if not init_from_cfg:
        k0 = int(np.argmax(seq.pose_ok)) if seq.pose_ok.any() else 0
        init = args.init_pose if args.init_pose is not None else list(seq.poses[k0])
        for i in range(7):
            d.p_mean0[6 + i] = init[i]
    eng.add_object(d, verts, tris)
    symmetries = None
    if args.symmetry:
        if args.symmetry_id is None:
            ap.error("--symmetry needs --symmetry-id")
        symmetries = io.read_bop_symmetries(args.symmetry, args.symmetry_id, args.symmetry_unit_scale)
        eng.set_symmetry(0, symmetries)
    n = len(seq) - start
    if n <= 0:
        sys.stderr.write("the first detection arrives after the last frame\n")
        return 1
    eng.enable_log(max(n, 6) if args.quality else n)   # (the quality ring: at least the six one-frame batches that can be in flight)
    if args.quality:
        eng.enable_quality()
    if args.flow_on_engine:
        eng.enable_flow(consistency=True if args.flow_consistency else None)
    if args.raw_depth is not None:
        eng.enable_raw_depth(args.raw_depth)
    if lens:
        fx, fy, cx, cy = lens[1] if lens[1] else (cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy)
        eng.enable_rectification(lens[0], cam=L.Camera(W, H, fx, fy, cx, cy))
    if args.masks_from_pose:
        if cfg.mask_frames_between != cfg.pose_frames_between:
            sys.stderr.write("note: mask_frames_between %d != pose_frames_between %d: a silhouette is as old as its pose\n" %
                             (cfg.mask_frames_between, cfg.pose_frames_between))
        eng.enable_pose_masks([0])
        if gate:
            eng.enable_pose_mask_depth_gate(gate[0], gate[1])
    for k in range(start, len(seq)):
        frame = seq.frame(k, with_image=bool(args.flow_on_engine), depth_raw=args.raw_depth is not None)
        if args.masks_from_pose:
            frame["mask"] = None
        eng.submit([frame])
        eng.step()
    pose, twist, npts, sel = eng.get_log(0, n)
    gt_path = os.path.join(args.root, "gt", "poses.txt")
    device_scores = {}
    if args.score_on_device and os.path.exists(gt_path) and n > 12:
        g = io.read_poses(gt_path)[0][start + 12:start + n]
        for kind in ("adi", "add"):
            device_scores[kind] = eng.score_log(kind, 0, 12, len(g), g)
        if symmetries is not None:
            for kind in ("mssd", "mspd"):
                device_scores[kind] = eng.score_log(kind, 0, 12, len(g), g, symmetries=symmetries)
    if args.quality:
        from roft_amd.ops import quality_overlap
        rec = eng.quality(0, n)[:, 0]
        iou = quality_overlap(rec)
        with open(args.quality, "w") as f:
            f.write("# frame n_mask n_render n_both n_depth n_front n_behind depth_err overlap\n")
            for r, o in zip(rec, iou):
                f.write("%d %d %d %d %d %d %d %.17g %.6f\n" % (start + r["frame"], r["n_mask"], r["n_render"], r["n_both"], r["n_depth"],
                                                              r["n_front"], r["n_behind"], r["depth_err"], o))
    pose_mask_stats = eng.pose_mask_stats() if args.masks_from_pose else None
    gate_stats = dict(eng.pose_mask_gate_stats(), front_tolerance=gate[0], behind_tolerance=gate[1]) if gate else None
    rectify_stats = eng.rectify_stats() if lens else None
    eng.close()
    prefix = args.out if args.out is not None else os.path.join(args.root, "roft_mi355x_")
    io.write_estimate_logs(prefix, pose[:, 0], twist[:, 0])
    report = dict(frames=n, first_frame=start, logs=[prefix + "pose_estimate", prefix + "velocity_estimate"], flow_type=int(ftype), flow_grid=int(grid))
    if os.path.exists(gt_path):
        gt, _ = io.read_poses(gt_path)
        est = np.concatenate([pose[:, 0, 6:9], pose[:, 0, 9:13]], 1)
        pts = verts.astype(np.float64)[:: max(1, len(verts) // 500)]
        g = gt[start + 12:start + n]
        dist = metrics.trajectory_adds(est[12:], g, pts)
        report.update(adds_mm_mean=1e3 * float(dist.mean()), adds_auc=metrics.auc(dist),
                      rmse_position_cm=metrics.rmse_cartesian_3d(g[:, :3], est[12:, :3]),
                      rmse_orientation_deg=metrics.rmse_angular(g[:, 3:], est[12:, 3:]))
        if symmetries is not None:
            cam4 = (cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy)
            report.update(symmetry_elements=int(len(symmetries)),
                          mssd_mm_mean=1e3 * float(metrics.trajectory_mssd(est[12:], g, pts, symmetries).mean()),
                          mspd_px_mean=float(metrics.trajectory_mspd(est[12:], g, pts, cam4, symmetries).mean()))
            if "mssd" in device_scores:
                report.update(mssd_full_mesh_mm_mean=1e3 * float(device_scores["mssd"].mean()),
                              mspd_full_mesh_px_mean=float(device_scores["mspd"].mean()))
        if device_scores:
            report.update(full_mesh_points=int(len(verts)), adds_full_mesh_mm_mean=1e3 * float(device_scores["adi"].mean()),
                          adds_full_mesh_auc=metrics.auc(device_scores["adi"]), add_full_mesh_mm_mean=1e3 * float(device_scores["add"].mean()),
                          add_full_mesh_auc=metrics.auc(device_scores["add"]))
    if args.render_overlay:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import render_results
        rc = render_results.main(["--root", args.root, "--mesh", args.mesh, "--poses", prefix + "pose_estimate", "--out", args.render_overlay,
                                  "--first-frame", str(start)] + (["--lens=" + args.lens] if lens else []) +
                                 (["--lens-camera=" + args.lens_camera] if lens and args.lens_camera else []))
        if rc != 0:
            return rc
        report["overlay"] = args.render_overlay
    if args.quality:
        report["quality"] = args.quality
    if args.masks_from_pose:
        report["pose_masks"] = pose_mask_stats
    if gate_stats:
        report["pose_mask_gate"] = gate_stats
    if rectify_stats:
        report["rectification"] = rectify_stats
    print(json.dumps(report))
    return 0


if __name__ == "__main__":
    sys.exit(main())
