#!/usr/bin/env python3
"""Metrics table of tracking results, the step right after the filtering path: what evaluation/evaluate.py of the
reference computes for its 'ours' entries -- per object and pooled over ALL -- printed as a Markdown table.

  evaluate_results.py --results DIR --dataset DIR [--objects NAME ...] [--points DIR] [--metrics m1,m2,...] [--of-ms 0]
                      [--device] [--all-points] [--symmetry models_info.json --symmetry-ids NAME=ID ... [--mssd] [--mspd]]
                      [--vsd] [--ar]

DIR/<object>/{pose_estimate[_ycb].txt, velocity_estimate.txt, execution_times.txt} are the log files ROFT-tracker (or
ROFT-tracker-batch, or tools/run_sequence.py with --out DIR/<object>/) leaves; dataset/<object>/gt/poses.txt holds the ground-truth
poses (x y z axis angle) and, optionally, gt/velocities.txt the ground-truth velocities.  ADD / ADD-S use <points>/<object>/points.xyz
when --points is given (the reference's YCB_Video_Models layout), else every k-th vertex of dataset/<object>/model.obj (about 500;
--all-points: every vertex).  --device computes the ADD / ADD-S distances on the GPU (roft_pose_errors: brute force in double
precision, the same numbers to 1e-12 m), once per object: the ALL row pools them instead of computing them again.
--mssd / --mspd add the mean of BOP's symmetry-aware distances (mm / px) under the objects' discrete symmetry groups of --symmetry
(metrics.trajectory_mssd / trajectory_mspd: numpy, or the device with --device); MSPD projects with dataset/<object>/cam_K.json.
--vsd adds BOP's average recall of the Visible Surface Discrepancy (AR_VSD), --ar that, AR_MSSD, AR_MSPD and their mean AR (BOP19's
thresholds: metrics.bop_average_recall).  Both run on the device (ops.pose_errors_vsd, ops.pose_errors_sym; no CPU fallback): the
mesh is dataset/<object>/model.obj, the camera dataset/<object>/cam_K.json (or --camera, with the size of the depth frames), the
depth frame of estimate k dataset/<object>/depth/<first-frame + k>.float, the symmetry groups those of --symmetry (without it: the
identity alone); an object's diameter is the `diameter` of its entry in --symmetry, else the largest distance between two vertices
of its mesh.  The ALL row pools the objects' estimates, each error against its own object's thresholds.
As in evaluate.py: the leading six velocity columns of the pose log are dropped (data_loader.py:238-241), the estimates are compared
with as many ground-truth rows as there are estimates (from the row the run started at: --first-frame), the linear velocity is
moved from the camera origin to the object position before it is compared (v = v_O + w x r, evaluate.py:514-521), and --of-ms is
added to the execution times (the reference adds what its optical-flow source costs per frame, evaluate.py:470-484).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roft_amd import io, metrics  # noqa: E402

DEFAULT = "rmse_cartesian_3d,rmse_angular,add,adi,rmse_linear_velocity,rmse_angular_velocity,time,excess_33_ms"
UNITS = dict(rmse_cartesian_3d="cm", rmse_cartesian_x="cm", rmse_cartesian_y="cm", rmse_cartesian_z="cm", rmse_angular="deg", add="AUC %", adi="AUC %",
             rmse_linear_velocity="cm/s", rmse_angular_velocity="deg/s", max_linear_velocity="m/s", max_angular_velocity="deg/s", time="ms", excess_33_ms="frames",
             mssd="mean mm", mspd="mean px", AR_VSD="recall", AR_MSSD="recall", AR_MSPD="recall", AR="recall")
VSD_FRAMES_PER_CALL = 64   # depth frames read and handed to the device at a time


def first_existing(*paths):
    for p in paths:
        if os.path.exists(p):
            return p
    return None


def load_object(results, dataset, name, first_frame, of_ms):
    d = os.path.join(results, name)
    pose_path = first_existing(os.path.join(d, "pose_estimate_ycb.txt"), os.path.join(d, "pose_estimate.txt"), os.path.join(d, "pose_estimate"))
    if pose_path is None:
        raise FileNotFoundError("no pose_estimate in " + d)
    pose = io.read_log(pose_path, skip_cols=6)
    gt_all = np.loadtxt(os.path.join(dataset, name, "gt", "poses.txt"), ndmin=2)
    gt = gt_all[first_frame:first_frame + len(pose)]
    pose = pose[:len(gt)]
    out = dict(pose=pose, gt_pose=gt)
    vel_path = first_existing(os.path.join(d, "velocity_estimate.txt"), os.path.join(d, "velocity_estimate"))
    gt_vel_path = os.path.join(dataset, name, "gt", "velocities.txt")
    if vel_path and os.path.exists(gt_vel_path):
        vel = io.read_log(vel_path)[:len(gt)]
        out["vel"] = metrics.object_velocity_from_twist(vel, gt[:, :3])
        out["gt_vel"] = np.loadtxt(gt_vel_path, ndmin=2)[first_frame:first_frame + len(vel)]
    t_path = first_existing(os.path.join(d, "execution_times.txt"), os.path.join(d, "execution_times"))
    if t_path:
        t = io.read_log(t_path)
        t[:, 0] += of_ms
        out["time"] = t
    return out


def object_camera(dataset, name, camera_arg, depth_shape):
    """(width, height, fx, fy, cx, cy) of an object's sequence: cam_K.json, or --camera with the size of its depth frames"""
    cam_path = os.path.join(dataset, name, "cam_K.json")
    if camera_arg:
        fx, fy, cx, cy = (float(v) for v in camera_arg.split(","))
        return depth_shape[1], depth_shape[0], fx, fy, cx, cy
    if not os.path.exists(cam_path):
        raise FileNotFoundError("no %s; give --camera=FX,FY,CX,CY" % cam_path)
    cam = json.load(open(cam_path))
    return int(cam.get("width", depth_shape[1])), int(cam.get("height", depth_shape[0])), cam["fx"], cam["fy"], cam["cx"], cam["cy"]


def bop_scores(args, names, data, points, ids):
    """{object: dict(vsd [F, 10], mssd [F], mspd [F], diameter, width)} on the device; mssd / mspd only with --ar"""
    from roft_amd import _lib, ops
    out = {}
    for n in names:
        mesh_path = first_existing(os.path.join(args.dataset, n, "model.obj"), os.path.join(args.dataset, n, n + ".obj"))
        if mesh_path is None:
            raise FileNotFoundError("--vsd / --ar: no model.obj of " + n)
        verts, tris = io.load_obj(mesh_path)
        est, ref = metrics.Metric._poses(data[n]["pose"]), metrics.Metric._poses(data[n]["gt_pose"])
        k = min(len(est), len(ref))
        est, ref = est[:k], ref[:k]
        depth_path = lambda f: os.path.join(args.dataset, n, "depth", "%d.float" % (args.first_frame + f))
        width, height, fx, fy, cx, cy = object_camera(args.dataset, n, args.camera, io.read_depth(depth_path(0)).shape)
        diameter = None
        if args.symmetry and n in ids:
            entry = json.load(open(args.symmetry)).get(str(int(ids[n])), {})
            if "diameter" in entry:
                diameter = float(entry["diameter"]) * args.symmetry_unit_scale
        if diameter is None:
            diameter = metrics.model_diameter(verts)
        cam, mesh = _lib.Camera(width, height, fx, fy, cx, cy), ops.make_mesh(verts, tris)
        vsd = np.zeros((k, len(metrics.BOP_VSD_TAUS)))
        for f0 in range(0, k, VSD_FRAMES_PER_CALL):
            f1 = min(k, f0 + VSD_FRAMES_PER_CALL)
            depth = np.stack([io.read_depth(depth_path(f)) for f in range(f0, f1)])
            vsd[f0:f1] = ops.pose_errors_vsd(cam, mesh, est[f0:f1], ref[f0:f1], depth, taus=metrics.BOP_VSD_TAUS, diameter=diameter)
        out[n] = dict(vsd=vsd, diameter=diameter, width=width)
        if args.ar:
            if n not in points:
                raise FileNotFoundError("--ar: no model points of " + n)
            sym = io.read_bop_symmetries(args.symmetry, int(ids[n]), args.symmetry_unit_scale) if args.symmetry and n in ids else None
            out[n]["mssd"] = ops.pose_errors_sym("mssd", points[n], est, ref, sym)
            out[n]["mspd"] = ops.pose_errors_sym("mspd", points[n], est, ref, sym, (fx, fy, cx, cy))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--results", required=True)
    ap.add_argument("--dataset", required=True)
    ap.add_argument("--objects", nargs="*", default=None)
    ap.add_argument("--points", default=None)
    ap.add_argument("--metrics", default=DEFAULT)
    ap.add_argument("--first-frame", type=int, default=0)
    ap.add_argument("--of-ms", type=float, default=0.0)
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    ap.add_argument("--device", action="store_true", help="ADD / ADD-S distances on the GPU (no CPU fallback)")
    ap.add_argument("--all-points", action="store_true", help="ADD / ADD-S on every vertex of model.obj instead of about 500")
    ap.add_argument("--symmetry", default=None, metavar="FILE", help="BOP models_info.json with the objects' discrete symmetry groups (for --mssd / --mspd)")
    ap.add_argument("--symmetry-ids", nargs="*", default=[], metavar="NAME=ID", help="an object's id in --symmetry (an object not named here: the identity alone)")
    ap.add_argument("--symmetry-unit-scale", type=float, default=0.001, help="model units of --symmetry in metres (BOP: millimetres)")
    ap.add_argument("--mssd", action="store_true", help="a column with the mean MSSD (mm) under the groups of --symmetry")
    ap.add_argument("--mspd", action="store_true", help="a column with the mean MSPD (px; the camera is dataset/<object>/cam_K.json, or --camera)")
    ap.add_argument("--camera", default=None, metavar="FX,FY,CX,CY", help="the intrinsics --mspd / --vsd / --ar project with, for every object")
    ap.add_argument("--vsd", action="store_true", help="a column with BOP's average recall of VSD (on the device)")
    ap.add_argument("--ar", action="store_true", help="columns AR_VSD, AR_MSSD, AR_MSPD and their mean AR (on the device)")
    args = ap.parse_args(argv)
    if (args.mssd or args.mspd) and not args.symmetry:
        ap.error("--mssd / --mspd need --symmetry FILE")
    names = args.objects or sorted(n for n in os.listdir(args.results) if os.path.isdir(os.path.join(args.results, n)))
    data = {n: load_object(args.results, args.dataset, n, args.first_frame, args.of_ms) for n in names}
    points = {}
    for n in names:
        if args.points:
            points[n] = np.loadtxt(os.path.join(args.points, n, "points.xyz"), ndmin=2)
        else:
            mesh = first_existing(os.path.join(args.dataset, n, "model.obj"), os.path.join(args.dataset, n, n + ".obj"))
            if mesh:
                v, _ = io.load_obj(mesh)
                points[n] = v.astype(np.float64)[:: 1 if args.all_points else max(1, len(v) // 500)]
    wanted = [m for m in args.metrics.split(",") if m]
    table = {}
    for m in wanted:
        metric = metrics.Metric(m, auc_points=points, backend="hip" if args.device else "cpu")
        vel_metric = "velocity" in m
        row = {}
        have = [n for n in names if ("vel" in data[n] if vel_metric else True) and (m not in ("time", "excess_33_ms") or "time" in data[n])
                and (m not in ("add", "adi") or n in points)]
        if args.device and m in ("add", "adi"):
            dist = {n: metric.distances(n, data[n]["gt_pose"], data[n]["pose"], m) for n in have}
            row = {n: metrics.auc(dist[n]) for n in have}
            if have:
                row["ALL"] = metrics.auc(np.concatenate([dist[n] for n in have]))
            table[m] = row
            continue
        for n in have:
            ref, sig = (data[n]["gt_vel"], data[n]["vel"]) if vel_metric else (data[n]["gt_pose"], data[n]["pose"])
            row[n] = metric.evaluate(n, ref, sig, data[n].get("time"))
        if have:
            pick = (lambda k: {n: data[n][k] for n in have})
            ref, sig = (pick("gt_vel"), pick("vel")) if vel_metric else (pick("gt_pose"), pick("pose"))
            row["ALL"] = metric.evaluate("ALL", ref, sig, {n: data[n]["time"] for n in have} if all("time" in data[n] for n in have) else None)
        table[m] = row
    # the symmetry-aware distances: per object the mean over its frames, ALL the mean over the pooled frames
    ids = dict(item.split("=", 1) for item in args.symmetry_ids)
    for m, on in (("mssd", args.mssd), ("mspd", args.mspd)):
        if not on:
            continue
        dist = {}
        for n in (n for n in names if n in points):
            sym = io.read_bop_symmetries(args.symmetry, int(ids[n]), args.symmetry_unit_scale) if n in ids else None
            est, ref = metrics.Metric._poses(data[n]["pose"]), metrics.Metric._poses(data[n]["gt_pose"])
            k = min(len(est), len(ref))
            backend = "hip" if args.device else "numpy"
            if m == "mssd":
                dist[n] = 1e3 * metrics.trajectory_mssd(est[:k], ref[:k], points[n], sym, backend)
            else:
                cam_path = os.path.join(args.dataset, n, "cam_K.json")
                if args.camera:
                    cam4 = tuple(float(v) for v in args.camera.split(","))
                elif os.path.exists(cam_path):
                    cam = json.load(open(cam_path))
                    cam4 = (cam["fx"], cam["fy"], cam["cx"], cam["cy"])
                else:
                    ap.error("--mspd: no %s; give --camera=FX,FY,CX,CY" % cam_path)
                dist[n] = metrics.trajectory_mspd(est[:k], ref[:k], points[n], cam4, sym, backend)
        table[m] = {n: float(d.mean()) for n, d in dist.items()}
        if dist:
            table[m]["ALL"] = float(np.concatenate(list(dist.values())).mean())
        wanted.append(m)
    if args.vsd or args.ar:
        scores = bop_scores(args, names, data, points, ids)
        keys = ("AR_VSD", "AR_MSSD", "AR_MSPD", "AR") if args.ar else ("AR_VSD",)
        for key in keys:
            table[key] = {}
        empty = np.zeros(0)
        for n, sc in scores.items():
            ar = metrics.bop_average_recall(sc["vsd"], sc.get("mssd", empty), sc.get("mspd", empty), sc["diameter"], sc["width"])
            for key in keys:
                table[key][n] = ar[key]
        if scores:   # every error in units of its own object's thresholds, then pooled
            pool = lambda f: np.concatenate([f(sc) for sc in scores.values()])
            ar = metrics.bop_average_recall(pool(lambda sc: sc["vsd"].reshape(-1)), pool(lambda sc: sc.get("mssd", empty) / sc["diameter"]),
                                            pool(lambda sc: sc.get("mspd", empty) * (640.0 / sc["width"])), 1.0, 640)
            for key in keys:
                table[key]["ALL"] = ar[key]
        wanted += keys
    cols = [m for m in wanted if table[m]]
    print("| object | " + " | ".join("%s (%s)" % (m, UNITS[m]) for m in cols) + " |")
    print("|---|" + "---|" * len(cols))
    for n in names + ["ALL"]:
        print("| %s | " % n + " | ".join(("%.3f" % table[m][n]) if n in table[m] else "-" for m in cols) + " |")
    if args.json:
        json.dump(table, open(args.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
