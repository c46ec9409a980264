#!/usr/bin/env python3
"""Times the ADD-S scoring of trajectories: the CPU path (metrics.trajectory_adds, backend "cpu": one KD-tree per pose on one
core) against the device path (ops.pose_errors, end to end: upload and read-back included), in one process.

  bench_pose_errors.py [--out profiles/r08_pose_errors.json] [--commit HASH] [--cpu-poses 1000] [--repeats 5]
  bench_pose_errors.py --vsd [--out profiles/r27_pose_errors_vsd.json] [--commit HASH] [--cpu-poses 8] [--repeats 5]

Cases: P in {500, 2 620, every vertex of synth.box_mesh(CRACKER_BOX_HALF_EXTENTS) = 8 214} x F in {1 000, 48 000} pose pairs.
The CPU path is run on --cpu-poses poses; for F = 48 000 that time is scaled (its cost per pose does not depend on F).  The
device path: median of --repeats calls after one warm-up; the kernel-only time comes from HIP events around the call's kernels.
The achieved fp64 rate counts the nearest-neighbour kernel's own operations per pair (7: 3 sub, 1 mul, 2 fma, 1 min; an fma is
ONE operation) and is set against the device's peak in the same unit.  The search is also timed once in the oracle's operation
order (9 operations, ROFT_POSE_ERRORS_FMA=0, in a child process: the switch is read once per process).
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roft_amd import _lib as L  # noqa: E402
from roft_amd import metrics, ops, synth  # noqa: E402

# AMD Instinct MI355X data sheet: peak double-precision VECTOR (FP64) performance 78.6 TFLOP/s, an fma counted as two
# floating-point operations = 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3e12 fp64 VALU operations per second
PEAK_FP64_VECTOR_TFLOPS = 78.6
PEAK_FP64_VALU_OPS = PEAK_FP64_VECTOR_TFLOPS * 1e12 / 2.0
PEAK_SOURCE = "AMD Instinct MI355X data sheet, peak FP64 vector 78.6 TFLOP/s (fma = 2 flop); not measured here"


def clouds():
    rng = np.random.default_rng(8)
    box = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)[0].astype(np.float64)
    return [("500", rng.uniform(-0.1, 0.1, (500, 3))), ("2620", rng.uniform(-0.1, 0.1, (2620, 3))), ("box_8214", box)]


def poses(n, seed=1):
    """Tracker-like pairs: random ground truth within 1.5 m, estimates off by millimetres and a few milliradians."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-0.8, 0.8, (n, 3))
    dq = np.concatenate([np.ones((n, 1)), rng.normal(0, 5e-3, (n, 3))], 1)
    qe = np.array([synth.quat_mul(a, b) for a, b in zip(q, dq)])
    qe /= np.linalg.norm(qe, axis=1, keepdims=True)
    return np.concatenate([t + rng.normal(0, 3e-3, (n, 3)), qe], 1), np.concatenate([t, q], 1)


def time_device(pts, est, ref, repeats):
    ops.pose_errors("adi", pts, est, ref)   # warm-up: buffers, code object
    wall, kern = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = ops.pose_errors("adi", pts, est, ref)
        wall.append(time.perf_counter() - t0)
        kern.append(ops.pose_errors_kernel_ms() * 1e-3)
    return float(np.median(wall)), float(np.median(kern)), out


def symmetry_cases(cpu_poses, repeats):
    """MSSD and MSPD under a box's four-element group at the same point x pose sizes: the numpy path (metrics.trajectory_mssd /
    trajectory_mspd, one core, timed on cpu_poses poses and scaled) against ops.pose_errors_sym end to end and kernel only."""
    group = np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0, 1]], float)   # identity, three half turns
    cam = (614.7142806307731, 614.7142806307731, 320.0, 240.0)
    est_all, ref_all = poses(48000)
    est_all[:, 2] += 2.0   # (in front of the camera: MSPD of a pose behind it is +inf)
    ref_all[:, 2] += 2.0
    out = []
    for name, pts in clouds():
        for kind in ("mssd", "mspd"):
            c = cam if kind == "mspd" else None
            t0 = time.perf_counter()
            if kind == "mssd":
                cpu = metrics.trajectory_mssd(est_all[:cpu_poses], ref_all[:cpu_poses], pts, group)
            else:
                cpu = metrics.trajectory_mspd(est_all[:cpu_poses], ref_all[:cpu_poses], pts, cam, group)
            cpu_ms_per_pose = 1e3 * (time.perf_counter() - t0) / cpu_poses
            for F in (1000, 48000):
                est, ref = est_all[:F], ref_all[:F]
                ops.pose_errors_sym(kind, pts, est, ref, group, c)
                wall, kern = [], []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    got = ops.pose_errors_sym(kind, pts, est, ref, group, c)
                    wall.append(time.perf_counter() - t0)
                    kern.append(ops.pose_errors_kernel_ms() * 1e-3)
                n_cmp = min(F, cpu_poses)
                case = dict(kind=kind, points=len(pts), cloud=name, poses=F, elements=len(group), numpy_ms_per_pose=cpu_ms_per_pose,
                            numpy_poses_timed=cpu_poses, numpy_s=cpu_ms_per_pose * 1e-3 * F, device_s=float(np.median(wall)),
                            device_kernel_s=float(np.median(kern)), speedup=cpu_ms_per_pose * 1e-3 * F / float(np.median(wall)),
                            max_abs_diff_vs_numpy=float(np.abs(got[:n_cmp] - cpu[:n_cmp]).max()))
                out.append(case)
                print(json.dumps(case), flush=True)
    return out


def vsd_cases(cpu_poses, repeats, n_img=1000):
    """VSD (ops.pose_errors_vsd, end to end) at 640 x 480 on the 15 552-triangle box: 1 000 and 48 000 pose pairs, with a depth image
    per pair and with one image under every pair, the four cases alternated `repeats` times after one warm-up each.  The host
    block holds 1 000 images (1.2 GB); the 48 000 pairs with an image each go through it in 48 calls of 1 000 (the library sends a
    call's images in chunks of 64 anyway).  The CPU path on one core -- the oracle's two renders and tests/vsd_ref.py's per-pixel
    restatement, and next to it the numpy form metrics.vsd_from_depths -- is timed on cpu_poses pairs and scaled."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import vsd_ref
    from oracle import binding as ob
    W, H, f = 640, 480, 614.7142806307731
    cam = L.Camera(W, H, f, f, W / 2.0, H / 2.0)
    verts, tris = synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)
    mesh = ops.make_mesh(verts, tris)
    diameter = metrics.model_diameter(verts)
    rng = np.random.default_rng(27)
    n_all = 48000
    est_all, ref_all = poses(n_all)
    for a in (est_all, ref_all):   # in view: within 10 cm of the axis, 0.5 .. 1.0 m away (the estimate keeps its millimetres)
        a[:, :2] *= 0.125
    z = rng.uniform(0.5, 1.0, n_all)
    est_all[:, 2] += z - ref_all[:, 2]
    ref_all[:, 2] = z
    # the sensor's images: a wall 2 m away behind everything (every drawn pixel is visible and is scored), shifted a little per image
    images = np.full((n_img, H, W), 2.0, np.float32) + rng.uniform(0.0, 0.01, (n_img, 1, 1)).astype(np.float32)
    kw = dict(delta=0.015, taus=metrics.BOP_VSD_TAUS, diameter=diameter)

    def run(F, shared):
        if shared:
            return ops.pose_errors_vsd(cam, mesh, est_all[:F], ref_all[:F], images[0], **kw)
        return np.concatenate([ops.pose_errors_vsd(cam, mesh, est_all[f0:f0 + n_img], ref_all[f0:f0 + n_img], images, **kw) for f0 in range(0, F, n_img)])

    # the CPU path
    t_render = t_ref = t_numpy = 0.0
    cpu = []
    omesh, ocam = ob.make_mesh(verts, tris), ob.camera(W, H, f, f, W / 2.0, H / 2.0)
    for k in range(cpu_poses):
        t0 = time.perf_counter()
        De = ob.render_depth(omesh, est_all[k, :3], est_all[k, 3:], ocam, 1)
        Dg = ob.render_depth(omesh, ref_all[k, :3], ref_all[k, 3:], ocam, 1)
        t1 = time.perf_counter()
        e_ref, _ = vsd_ref.vsd(De, Dg, images[k], cam, 0.015, metrics.BOP_VSD_TAUS, diameter)
        t2 = time.perf_counter()
        e_np = metrics.vsd_from_depths(De, Dg, images[k], (f, f, W / 2.0, H / 2.0), **kw)
        t3 = time.perf_counter()
        t_render, t_ref, t_numpy = t_render + (t1 - t0), t_ref + (t2 - t1), t_numpy + (t3 - t2)
        assert np.array_equal(e_ref, e_np)
        cpu.append(e_ref)
    cpu = np.array(cpu)
    cpu_s_per_pair = (t_render + t_ref) / cpu_poses
    shapes = [(1000, False), (1000, True), (48000, False), (48000, True)]
    got = {sh: run(*sh) for sh in shapes}   # warm-up: buffers, code object
    wall = {sh: [] for sh in shapes}
    for _ in range(repeats):
        for sh in shapes:
            t0 = time.perf_counter()
            run(*sh)
            wall[sh].append(time.perf_counter() - t0)
    bus_s_per_pair = W * H * 4 / 40e9   # 1.2 MB per pair at the ~40 GB/s the README reports for host-to-device copies
    out = []
    for F, shared in shapes:
        w = wall[(F, shared)]
        med = float(np.median(w))
        equal = bool(np.array_equal(got[(F, shared)][:cpu_poses], cpu)) if not shared else None
        case = dict(poses=F, images="one under every pair" if shared else "one per pair", width=W, height=H, triangles=len(tris), vertices=len(verts),
                    device_s=med, device_s_repeats=w, device_us_per_pair=1e6 * med / F, pairs_per_s=F / med,
                    cpu_s_per_pair=cpu_s_per_pair, cpu_s=cpu_s_per_pair * F, cpu_pairs_timed=cpu_poses, speedup=cpu_s_per_pair * F / med,
                    bus_floor_s=None if shared else bus_s_per_pair * F, times_the_bus_floor=None if shared else med / (bus_s_per_pair * F),
                    errors_equal_to_the_cpu_path=equal, mean_error=float(got[(F, shared)].mean()))
        out.append(case)
        print(json.dumps(case), flush=True)
    cpu_split = dict(oracle_renders_s_per_pair=t_render / cpu_poses, vsd_ref_s_per_pair=t_ref / cpu_poses, numpy_form_s_per_pair=t_numpy / cpu_poses)
    return out, cpu_split


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--symmetry-only", action="store_true",
                    help="only the MSSD / MSPD lines (roft_pose_errors_sym under a four-element group, against the numpy path): {symmetry_cases: [...]} -> --out")
    ap.add_argument("--vsd", action="store_true",
                    help="only the VSD lines (roft_pose_errors_vsd at 640 x 480, against the oracle's renders + tests/vsd_ref.py on one core): "
                         "{vsd_cases: [...]} -> --out (default profiles/r27_pose_errors_vsd.json; --cpu-poses default 8)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--cpu-poses", type=int, default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-only", action="store_true", help="(the child run) print the kernel time of the full mesh x 1 000 poses")
    args = ap.parse_args(argv)
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r27_pose_errors_vsd.json" if args.vsd else "r08_pose_errors.json")
    if args.cpu_poses is None:
        args.cpu_poses = 8 if args.vsd else 1000
    L.require_device()
    fma = os.environ.get("ROFT_POSE_ERRORS_FMA", "1")[:1] != "0"
    ops_per_pair = 7 if fma else 9
    if args.kernel_only:
        pts = clouds()[-1][1]
        est, ref = poses(1000)
        _, kern, _ = time_device(pts, est, ref, args.repeats)
        print(json.dumps(dict(kernel_s=kern, ops_per_pair=ops_per_pair)))
        return 0
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
        except Exception:
            commit = "unknown"
    if args.vsd:
        cases, cpu_split = vsd_cases(args.cpu_poses, args.repeats)
        record = dict(commit=commit, device_count=int(L.lib().roft_device_count()), kind="VSD (roft_pose_errors_vsd), BOP19 parameters",
                      cpu_path="oracle render_depth x 2 + tests/vsd_ref.py (one core); timed on cpu_pairs_timed pairs, scaled to F", cpu_path_split=cpu_split,
                      device_path="ops.pose_errors_vsd end to end (upload, kernels, read-back): median of %d alternated repeats after one warm-up; "
                                  "48 000 pairs with an image each = 48 calls over one block of 1 000 images" % args.repeats,
                      bus_floor="640 x 480 x 4 B = 1.2 MB per pair at 40 GB/s", vsd_cases=cases)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
        return 0
    if args.symmetry_only:
        record = dict(commit=commit, device_count=int(L.lib().roft_device_count()), kind="MSSD / MSPD (roft_pose_errors_sym)",
                      numpy_path="metrics.trajectory_mssd / trajectory_mspd backend='numpy' (one core); timed on numpy_poses_timed poses, scaled to F",
                      device_path="ops.pose_errors_sym end to end (upload, kernel, read-back): median of %d calls after one warm-up" % args.repeats,
                      symmetry_cases=symmetry_cases(min(args.cpu_poses, 200), args.repeats))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
        return 0
    cases = []
    all_faster = True
    est_all, ref_all = poses(48000)   # every case scores the leading rows of the same trajectory
    for name, pts in clouds():
        P = len(pts)
        est_c, ref_c = est_all[:args.cpu_poses], ref_all[:args.cpu_poses]
        t0 = time.perf_counter()
        cpu_out = metrics.trajectory_adds(est_c, ref_c, pts, backend="cpu")
        cpu_ms_per_pose = 1e3 * (time.perf_counter() - t0) / args.cpu_poses
        for F in (1000, 48000):
            est, ref = est_all[:F], ref_all[:F]
            wall, kern, out = time_device(pts, est, ref, args.repeats)
            n_cmp = min(F, args.cpu_poses)
            pairs = float(F) * P * P
            rate = pairs * ops_per_pair / kern
            case = dict(points=P, cloud=name, poses=F, cpu_ms_per_pose=cpu_ms_per_pose, cpu_poses_timed=args.cpu_poses,
                        cpu_scaled=F != args.cpu_poses, cpu_s=cpu_ms_per_pose * 1e-3 * F,
                        device_ms_per_pose=1e3 * wall / F, device_s=wall, device_kernel_s=kern, speedup=cpu_ms_per_pose * 1e-3 * F / wall,
                        pair_distances_per_s=pairs / wall, pair_distances_per_s_kernel=pairs / kern,
                        fp64_valu_ops_per_s=rate, fraction_of_fp64_vector_peak=rate / PEAK_FP64_VALU_OPS,
                        max_abs_diff_vs_cpu_m=float(np.abs(out[:n_cmp] - cpu_out[:n_cmp]).max()))
            all_faster = all_faster and wall < case["cpu_s"]
            cases.append(case)
            print(json.dumps(case), flush=True)
    # the same search in the oracle's operation order, kernel only
    env = dict(os.environ, ROFT_POSE_ERRORS_FMA="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", "--repeats", str(args.repeats)], env=env,
                       capture_output=True, text=True, timeout=600)
    no_fma = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 and r.stdout.strip() else dict(error=r.stderr[-500:])
    with_fma = next(c for c in cases if c["cloud"] == "box_8214" and c["poses"] == 1000)["device_kernel_s"]
    record = dict(commit=commit, device_count=int(L.lib().roft_device_count()), kind="ADD-S (ROFT_POSE_ERROR_ADDS)",
                  kernel_ops_per_pair=ops_per_pair, kernel_ops="3 sub, 1 mul, 2 fma, 1 min (an fma is one operation)" if fma else "3 sub, 3 mul, 2 add, 1 min",
                  peak_fp64_valu_ops_per_s=PEAK_FP64_VALU_OPS, peak_source=PEAK_SOURCE,
                  cpu_path="metrics.trajectory_adds backend='cpu' (scipy cKDTree, one core); timed on cpu_poses_timed poses, scaled to F where cpu_scaled",
                  device_path="ops.pose_errors end to end (upload, kernels, read-back): median of %d calls after one warm-up" % args.repeats,
                  cases=cases, device_faster_in_every_case=bool(all_faster),
                  operation_order_ab=dict(case="box_8214 x 1000 poses, kernel only", fma_7_ops_kernel_s=with_fma, oracle_order_9_ops=no_fma))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "device faster in every case:", all_faster)
    return 0 if all_faster else 1


if __name__ == "__main__":
    sys.exit(main())
