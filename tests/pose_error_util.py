"""Shared by tests/test_pose_errors_cpu.py and tests/test_pose_errors_gpu.py: seeded pose pairs and a small results tree for
tools/evaluate_results.py."""
import contextlib
import io as pyio
import os
import sys

import numpy as np

from roft_amd import io, metrics, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit(q):
    q = np.asarray(q, float)
    return q / np.linalg.norm(q)


def small_rotation(rng, angle):
    axis = unit(rng.normal(size=3))
    return np.concatenate([[np.cos(angle / 2.0)], np.sin(angle / 2.0) * axis])


def pose_pairs(seed, n):
    """(est, ref) [n, 7] rows x y z, q wxyz.  ref: random orientations, translations up to 1.5 m.  est: pair 0 equals ref, pairs 1 - 3
    are ref flipped by 180 degrees about the object's x / y / z axis, the others are ref disturbed by 1e-4 .. 0.3 rad and
    1e-4 .. 0.1 m (log-spaced, so that the errors run from a tenth of a millimetre to decimetres)."""
    rng = np.random.default_rng(seed)
    ref = np.zeros((n, 7))
    est = np.zeros((n, 7))
    for k in range(n):
        q = unit(rng.normal(size=4))
        t = unit(rng.normal(size=3)) * rng.uniform(0.0, 1.5)
        ref[k, :3], ref[k, 3:] = t, q
        if k == 0:
            est[k] = ref[k]
        elif k <= 3:
            flip = np.zeros(4)
            flip[k] = 1.0
            est[k, :3], est[k, 3:] = t, synth.quat_mul(q, flip)
        else:
            s = (k - 4) / max(n - 5, 1)
            ang, off = 1e-4 * (0.3 / 1e-4) ** s, 1e-4 * (0.1 / 1e-4) ** s
            est[k, :3] = t + unit(rng.normal(size=3)) * off
            est[k, 3:] = unit(synth.quat_mul(q, small_rotation(rng, ang)))
    return est, ref


def cpu_errors(f, pts, est, ref):
    """f(R_est, t_est, R_gt, t_gt, pts) pose by pose (metrics.add / metrics.adds / the oracle's)."""
    return np.array([f(metrics.quat_to_rot(e[3:]), e[:3], metrics.quat_to_rot(r[3:]), r[:3], pts) for e, r in zip(est, ref)])


def write_results_tree(root, n_frames=8, mesh_n=12):
    """root/results/<object>/{pose_estimate, velocity_estimate}, root/dataset/<object>/{gt/poses.txt, model.obj} for two objects;
    returns (results, dataset, names)."""
    names = ["003_cracker_box", "004_sugar_box"]
    results, dataset = os.path.join(str(root), "results"), os.path.join(str(root), "dataset")
    for i, name in enumerate(names):
        est, ref = pose_pairs(70 + i, n_frames + 4)
        est, ref = est[4:], ref[4:]   # the disturbed pairs
        # (errors of millimetres to a few centimetres: inside the AUC's 0.1 m threshold)
        est[:, :3] = ref[:, :3] + (est[:, :3] - ref[:, :3]) * 0.2
        os.makedirs(os.path.join(results, name), exist_ok=True)
        os.makedirs(os.path.join(dataset, name, "gt"), exist_ok=True)
        pose13 = np.zeros((n_frames, 13))
        pose13[:, 6:] = est
        io.write_estimate_logs(os.path.join(results, name, ""), pose13, np.zeros((n_frames, 6)))
        io.write_poses(os.path.join(dataset, name, "gt", "poses.txt"), ref)
        he = synth.CRACKER_BOX_HALF_EXTENTS
        io.write_obj(os.path.join(dataset, name, "model.obj"), *synth.box_mesh(np.asarray(he) * (1.0 - 0.3 * i), n=mesh_n))
    return results, dataset, names


def run_evaluate(results, dataset, *flags):
    """tools/evaluate_results.py in process: the printed table."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import evaluate_results
    finally:
        sys.path.pop(0)
    buf = pyio.StringIO()
    with contextlib.redirect_stdout(buf):
        assert evaluate_results.main(["--results", results, "--dataset", dataset, "--metrics", "rmse_cartesian_3d,rmse_angular,add,adi"] + list(flags)) == 0
    return buf.getvalue()


def parse_table(text):
    """{object: {column title: cell}} of the Markdown table."""
    lines = [l for l in text.strip().splitlines() if l.startswith("|")]
    head = [c.strip() for c in lines[0].strip("|").split("|")]
    out = {}
    for l in lines[2:]:
        cells = [c.strip() for c in l.strip("|").split("|")]
        out[cells[0]] = dict(zip(head[1:], cells[1:]))
    return out


def make_engine(streams, **over):
    """The engine of tests/test_engine_gpu.py: one object per synthetic stream."""
    from roft_amd import engine as E
    st0 = streams[0]
    cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=len(streams))
    c = st0.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st0.flow_grid, st0.flow_scale
    for k, v in over.items():
        setattr(cfg, k, v)
    eng = E.ROFTFilterBatch(cfg)
    for st in streams:
        d = E.default_object()
        m0 = synth.initial_pose_from_stream(st)
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, *st.mesh)
    return eng
