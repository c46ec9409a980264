"""roft_pose_errors / roft_engine_score_log without a device: argument validation, no CPU fallback, the backends of
roft_amd.metrics and the table of tools/evaluate_results.py."""
import ctypes as C
import os

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import io, metrics

import pose_error_util as pu


def test_argument_validation_comes_before_the_device():
    lib = L.lib()
    pts, est, ref, out = np.zeros((4, 3)), np.zeros((2, 7)), np.zeros((2, 7)), np.full(2, 7.0)
    p = lambda a: a.ctypes.data   # noqa: E731
    f = lib.roft_pose_errors
    assert f(2, p(pts), 4, p(est), p(ref), 2, p(out)) == -1      # unknown kind
    assert f(-1, p(pts), 4, p(est), p(ref), 2, p(out)) == -1
    for kind in (L.POSE_ERROR_ADD, L.POSE_ERROR_ADDS):
        assert f(kind, None, 4, p(est), p(ref), 2, p(out)) == -1
        assert f(kind, p(pts), 4, None, p(ref), 2, p(out)) == -1
        assert f(kind, p(pts), 4, p(est), None, 2, p(out)) == -1
        assert f(kind, p(pts), 4, p(est), p(ref), 2, None) == -1
        assert f(kind, p(pts), 0, p(est), p(ref), 2, p(out)) == -1
        assert f(kind, p(pts), -3, p(est), p(ref), 2, p(out)) == -1
        assert f(kind, p(pts), 4, p(est), p(ref), -1, p(out)) == -1
        assert f(kind, p(pts), 4, p(est), p(ref), 0, p(out)) == 0   # nothing to do: ROFT_OK with or without a device
    assert np.all(out == 7.0), "a refused or empty call touches nothing"
    g = lib.roft_engine_score_log
    assert g(None, L.POSE_ERROR_ADDS, 0, 0, 1, p(pts), 4, p(ref), p(out)) == -1


def _case():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.1, 0.1, (60, 3))
    est, ref = pu.pose_pairs(11, 9)
    return pts, est, ref


def test_cpu_backend_is_the_old_path():
    pts, est, ref = _case()
    want_s = pu.cpu_errors(metrics.adds, pts, est, ref)
    want_a = pu.cpu_errors(metrics.add, pts, est, ref)
    # the default and backend="cpu": what metrics.adds / metrics.add return, pose by pose, bit for bit
    for got in (metrics.trajectory_adds(est, ref, pts), metrics.trajectory_adds(est, ref, pts, backend="cpu")):
        assert np.array_equal(got.view(np.uint64), want_s.view(np.uint64))
    for got in (metrics.trajectory_add(est, ref, pts), metrics.trajectory_add(est, ref, pts, backend="cpu")):
        assert np.array_equal(got.view(np.uint64), want_a.view(np.uint64))
    with pytest.raises(ValueError):
        metrics.trajectory_adds(est, ref, pts, backend="gpu")


def test_no_cpu_fallback():
    pts, est, ref = _case()
    want_s = pu.cpu_errors(metrics.adds, pts, est, ref)
    want_a = pu.cpu_errors(metrics.add, pts, est, ref)
    if L.lib().roft_device_count() > 0:
        pytest.skip("a HIP device is present")
    from roft_amd import ops
    with pytest.raises(L.RoftError):
        ops.pose_errors("adi", pts, est, ref)
    assert b"no HIP device" in L.lib().roft_last_error_string()
    with pytest.raises(L.RoftError):
        ops.pose_errors("add", pts, est, ref)
    with pytest.raises(L.RoftError):
        metrics.trajectory_adds(est, ref, pts, backend="hip")
    with pytest.raises(L.RoftError):
        metrics.trajectory_add(est, ref, pts, backend="hip")
    # "auto" without a device is the CPU path
    assert np.array_equal(metrics.trajectory_adds(est, ref, pts, backend="auto").view(np.uint64), want_s.view(np.uint64))
    assert np.array_equal(metrics.trajectory_add(est, ref, pts, backend="auto").view(np.uint64), want_a.view(np.uint64))


def test_metric_auc_is_what_it_was():
    """Metric.auc converts the axis-angle rows once per trajectory: the distances are those of two rotation matrices per frame."""
    pts, est, ref = _case()
    rows = lambda p: np.array([np.concatenate([r[:3], io.quat_to_axis_angle(r[3:])[0], [io.quat_to_axis_angle(r[3:])[1]]]) for r in p])   # noqa: E731
    sig, gt = rows(est), rows(ref)
    for name, f in (("add", metrics.add), ("adi", metrics.adds)):
        m = metrics.Metric(name, auc_points={"a": pts, "b": pts[:40]})
        assert m.backend == "cpu"
        want = np.array([f(m._rot(s[3:7]), s[:3], m._rot(r[3:7]), r[:3], pts) for r, s in zip(gt, sig)])
        d, a = m.auc("a", gt, sig, name)
        assert np.array_equal(d.view(np.uint64), want.view(np.uint64)) and a == metrics.auc(want)
        want_b = np.array([f(m._rot(s[3:7]), s[:3], m._rot(r[3:7]), r[:3], pts[:40]) for r, s in zip(gt[:5], sig[:5])])
        d, a = m.auc("ALL", {"a": gt, "b": gt[:5]}, {"a": sig, "b": sig[:5]}, name)
        assert np.array_equal(d.view(np.uint64), np.concatenate([want, want_b]).view(np.uint64))
        assert m.evaluate("ALL", {"a": gt, "b": gt[:5]}, {"a": sig, "b": sig[:5]}, None) == a


def _expected_table(results, dataset, names, all_points):
    """The add / adi / rmse cells computed with metrics.Metric directly, as the tool did before it had flags."""
    data, points = {}, {}
    for n in names:
        pose = io.read_log(os.path.join(results, n, "pose_estimate"), skip_cols=6)
        gt = np.loadtxt(os.path.join(dataset, n, "gt", "poses.txt"), ndmin=2)[:len(pose)]
        data[n] = (gt, pose)
        v, _ = io.load_obj(os.path.join(dataset, n, "model.obj"))
        points[n] = v.astype(np.float64)[:: 1 if all_points else max(1, len(v) // 500)]
    table = {}
    for m, unit in (("rmse_cartesian_3d", "cm"), ("rmse_angular", "deg"), ("add", "AUC %"), ("adi", "AUC %")):
        metric = metrics.Metric(m, auc_points=points)
        col = "%s (%s)" % (m, unit)
        for n in names:
            table.setdefault(n, {})[col] = "%.3f" % metric.evaluate(n, data[n][0], data[n][1], None)
        table.setdefault("ALL", {})[col] = "%.3f" % metric.evaluate("ALL", {n: data[n][0] for n in names}, {n: data[n][1] for n in names}, None)
    return table


def test_evaluate_results_table(tmp_path):
    results, dataset, names = pu.write_results_tree(tmp_path)
    plain = pu.parse_table(pu.run_evaluate(results, dataset))
    assert plain == _expected_table(results, dataset, names, all_points=False)
    assert set(plain) == set(names) | {"ALL"}
    for row in plain.values():   # a table worth comparing: the AUCs are neither 0 nor 100
        assert 1.0 < float(row["adi (AUC %)"]) < 99.9 and 1.0 < float(row["add (AUC %)"]) < 99.9
    full = pu.parse_table(pu.run_evaluate(results, dataset, "--all-points"))
    assert full == _expected_table(results, dataset, names, all_points=True)
    for n in plain:
        for col in plain[n]:
            if not col.startswith(("add", "adi")):
                assert full[n][col] == plain[n][col], "--all-points changes only the add / adi columns"
    assert any(full[n][c] != plain[n][c] for n in plain for c in plain[n]), "every vertex instead of every second one: some cell moves"
