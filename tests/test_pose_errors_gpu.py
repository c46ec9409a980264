"""ADD / ADD-S on the device (roft_pose_errors, roft_engine_score_log) against the reference-made fixtures, the oracle's brute
force and the CPU path of roft_amd.metrics.

The bar is 1e-12 m everywhere.  Coordinates are below 4 m, so an ulp is 8.9e-16; about six roundings per transformed coordinate
give <= 2.7e-15 per cloud, the difference of two clouds is <= 5.8e-15 per component, i.e. <= 1.0e-14 on a distance, also at
distance 0; the reference's own BLAS / KD-tree arithmetic is of the same order.  1e-12 leaves a factor of about 20 on top of
the few multiples of that which a fused multiply-add or another summation order can move."""
import json
import os

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import metrics, ops, synth

import pose_error_util as pu
import util

pytestmark = pytest.mark.gpu

TOL = 1e-12   # m


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def rot_to_quat(R):
    """Rotation matrix -> unit quaternion (w, x, y, z), the branch with the largest pivot."""
    R = np.asarray(R, float)
    t = np.trace(R)
    if t > 0.0:
        s = 2.0 * np.sqrt(1.0 + t)
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k])
        q = [0.0] * 4
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = 0.25 * s
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return pu.unit(q)


def test_reference_fixtures():
    fx = json.load(open(os.path.join(util.GOLDEN, "bop_fixtures.json")))
    pts = np.array(fx["points"], float)
    cases = fx["cases"]
    assert len(cases) == 20
    est = np.array([np.concatenate([c["t_est"], rot_to_quat(c["R_est"])]) for c in cases])
    ref = np.array([np.concatenate([c["t_gt"], rot_to_quat(c["R_gt"])]) for c in cases])
    for c, e, r in zip(cases, est, ref):   # the round trip reproduces the matrices
        assert np.abs(metrics.quat_to_rot(e[3:]) - np.array(c["R_est"])).max() < 1e-14
        assert np.abs(metrics.quat_to_rot(r[3:]) - np.array(c["R_gt"])).max() < 1e-14
    for kind, key in (("add", "add"), ("adi", "adi")):
        got = ops.pose_errors(kind, pts, est, ref)   # all 20 in one call
        want = np.array([c[key] for c in cases])
        err = np.abs(got - want)
        print(kind, "max |device - fixture| = %.3g m" % err.max())
        assert np.all(err <= TOL), (kind, err.max())


def _cloud(P):
    if P == "box":
        return synth.box_mesh(synth.CRACKER_BOX_HALF_EXTENTS)[0].astype(np.float64)
    return np.random.default_rng(1000 + P).uniform(-0.1, 0.1, (P, 3))


@pytest.mark.parametrize("P", [1, 2, 63, 64, 65, 255, 257, 500, 2620, "box"])
def test_oracle_and_cpu_path(oracle, P):
    pts = _cloud(P)
    if P == "box":
        assert len(pts) == 8214
    est, ref = pu.pose_pairs(31, 64)
    for kind, f_cpu, f_or in (("add", metrics.add, oracle.add), ("adi", metrics.adds, oracle.adds)):
        got = ops.pose_errors(kind, pts, est, ref)
        via_metrics = metrics.trajectory_add(est, ref, pts, backend="hip") if kind == "add" else metrics.trajectory_adds(est, ref, pts, backend="hip")
        assert np.array_equal(bits(got), bits(via_metrics))
        auto = metrics.trajectory_add(est, ref, pts, backend="auto") if kind == "add" else metrics.trajectory_adds(est, ref, pts, backend="auto")
        assert np.array_equal(bits(got), bits(auto)), "a device is present: 'auto' is the device"
        for name, want in (("oracle", pu.cpu_errors(f_or, pts, est, ref)), ("metrics", pu.cpu_errors(f_cpu, pts, est, ref))):
            err = np.abs(got - want)
            print(P, kind, name, "max err %.3g m, errors %.3g .. %.3g m" % (err.max(), want.min(), want.max()))
            assert np.all(err <= TOL), (P, kind, name, int(np.argmax(err)), err.max())   # every pair
        assert got[0] <= TOL                     # est == ref
        if len(pts) > 2:
            assert got[4:].min() < 1e-3 and got.max() > 5e-3   # from sub-millimetre errors to centimetres


def test_determinism_contract():
    pts = _cloud(500)
    est, ref = pu.pose_pairs(77, 1000)
    k = 613
    rng = np.random.default_rng(3)
    for kind in ("add", "adi"):
        whole = ops.pose_errors(kind, pts, est, ref)
        for _ in range(3):
            assert np.array_equal(bits(ops.pose_errors(kind, pts, est, ref)), bits(whole))
        alone = ops.pose_errors(kind, pts, est[k:k + 1], ref[k:k + 1])
        assert bits(alone)[0] == bits(whole)[k]
        order = np.concatenate([[k], np.delete(np.arange(1000), k)])
        assert bits(ops.pose_errors(kind, pts, est[order], ref[order]))[0] == bits(whole)[k]          # first
        order = order[::-1].copy()
        assert bits(ops.pose_errors(kind, pts, est[order], ref[order]))[-1] == bits(whole)[k]         # last
        perm = rng.permutation(1000)
        assert np.array_equal(bits(ops.pose_errors(kind, pts, est[perm], ref[perm])), bits(whole[perm]))   # shuffled: every pair


def test_non_finite_pose_stays_in_its_entry():
    pts = _cloud(257)
    est, ref = pu.pose_pairs(5, 10)
    for kind in ("add", "adi"):
        clean = ops.pose_errors(kind, pts, est, ref)
        assert np.all(np.isfinite(clean))
        for side, col, bad in ((0, 1, np.nan), (1, 4, np.nan), (0, 0, np.inf), (1, 2, -np.inf)):
            e, r = est.copy(), ref.copy()
            (e if side == 0 else r)[6, col] = bad
            got = ops.pose_errors(kind, pts, e, r)
            assert not np.isfinite(got[6]), (kind, side, col, bad, got[6])
            keep = np.arange(10) != 6
            assert np.array_equal(bits(got[keep]), bits(clean[keep]))
            assert metrics.auc(got) <= metrics.auc(clean)   # counted as a miss


def _run(streams, n, log_cap, score=None):
    """n frames through the engine with a log of log_cap frames; score(eng) is called after them; then 5 more frames.  Returns the
    log rows of the last 5 frames."""
    eng = pu.make_engine(streams)
    eng.enable_log(log_cap)
    out = None
    for k in range(n + 5):
        frames = []
        for st in streams:
            depth, flow, mask, pose = util.frame_inputs(st, k)
            frames.append(dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt))
        eng.submit(frames)
        eng.step()
        if k == n - 1:
            eng.sync()
            if score:
                out = score(eng)
    tail = eng.get_log_rows(n, 5)
    eng.close()
    return out, tail


def _score_rc(eng, kind, obj, first, n, ref, pts=None):
    out = np.zeros(max(n, 1))
    ref = np.ascontiguousarray(ref, np.float64)
    return L.lib().roft_engine_score_log(eng._h, kind, obj, first, n, None if pts is None else pts.ctypes.data, 0 if pts is None else len(pts),
                                         ref.ctypes.data, out.ctypes.data)


@pytest.mark.parametrize("log_cap", [40, 8])
def test_engine_log(oracle, log_cap):
    n = 30
    streams = [util.stream(100 + i, n + 5, scale=2) for i in range(2)]
    gts = [np.concatenate([np.asarray(st.gt.x, float), np.asarray(st.gt.q, float)], 1) for st in streams]
    given = _cloud(255)
    first, cnt = (0, n) if log_cap >= n else (n - log_cap, log_cap)

    def score(eng):
        rows = eng.get_log_rows(first, cnt)
        checked = 0
        for obj, st in enumerate(streams):
            est = np.ascontiguousarray(rows[:, obj, 6:13])
            ref = gts[obj][first:first + cnt]
            for pts in (None, given):
                p = st.mesh[0].astype(np.float64) if pts is None else pts
                for kind, f_or in (("add", oracle.add), ("adi", oracle.adds)):
                    got = eng.score_log(kind, obj, first, cnt, ref, points=pts)
                    assert np.array_equal(bits(got), bits(ops.pose_errors(kind, p, est, ref))), (obj, kind, pts is None)
                    err = np.abs(got - pu.cpu_errors(f_or, p, est, ref))
                    assert np.all(err <= TOL), (obj, kind, err.max())
                    assert np.all(np.isfinite(got)) and got.max() > 0.0
                    checked += 1
            # a part of the range, not starting at its first frame
            got = eng.score_log("adi", obj, first + 3, 4, ref[3:7], points=given)
            assert np.array_equal(bits(got), bits(ops.pose_errors("adi", given, est[3:7], ref[3:7])))
        ref = gts[0]
        assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, first, cnt, ref[first:first + cnt]) == 0
        assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, first, 0, ref[:1]) == 0                            # empty range
        assert _score_rc(eng, L.POSE_ERROR_ADDS, 2, first, cnt, ref[first:first + cnt]) == -1        # bad obj_id
        assert _score_rc(eng, L.POSE_ERROR_ADDS, -1, first, cnt, ref[first:first + cnt]) == -1
        assert _score_rc(eng, 7, 0, first, cnt, ref[first:first + cnt]) == -1                          # unknown kind
        assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, n - 1, 2, ref[n - 1:n + 1]) == -1                  # a frame not stepped yet
        assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, -1, 2, ref[:2]) == -1
        if log_cap < n:   # the ring has wrapped: frames before n - log_cap are overwritten
            assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, first - 1, 2, ref[first - 1:first + 1]) == -1
            assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, 0, 1, ref[:1]) == -1
            assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, first - 1, log_cap + 1, ref[first - 1:n]) == -1
        return checked

    checked, tail_scored = _run(streams, n, log_cap, score)
    assert checked == 8
    # scoring changes nothing of the trajectory: 5 more frames equal those of a run that never scored
    _, tail_plain = _run(streams, n, log_cap, None)
    assert np.array_equal(bits(tail_scored), bits(tail_plain))


def test_engine_score_log_needs_the_log():
    streams = [util.stream(100, 35, scale=2)]
    eng = pu.make_engine(streams)
    depth, flow, mask, pose = util.frame_inputs(streams[0], 0)
    eng.submit([dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=streams[0].dt)])
    eng.step()
    ref = np.zeros((1, 7))
    ref[0, 3] = 1.0
    assert _score_rc(eng, L.POSE_ERROR_ADDS, 0, 0, 1, ref) == -1
    with pytest.raises(L.RoftError):
        eng.score_log("adi", 0, 0, 1, ref)
    eng.close()


def test_evaluate_results_on_the_device(tmp_path):
    results, dataset, names = pu.write_results_tree(tmp_path)
    plain = pu.run_evaluate(results, dataset)
    assert pu.run_evaluate(results, dataset, "--device") == plain
    assert pu.run_evaluate(results, dataset, "--device", "--all-points") == pu.run_evaluate(results, dataset, "--all-points")
    for row in pu.parse_table(plain).values():
        for cell in row.values():
            assert len(cell.split(".")[1]) == 3   # three decimals
