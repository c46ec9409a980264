"""MSSD and MSPD on the device (roft_pose_errors_sym, roft_engine_score_log_sym; include/roft_engine.h section 3h) against the numpy
restatement tests/symmetry_ref.py.  Bars: 1e-12 m (the bar of the ADD / ADD-S tests) and 1e-9 px (the same relative headroom on
pixel coordinates of magnitude ~1e3).  Point counts at the kernel's edges: a lane (1), a wave (63, 64, 65), the workgroup's stride
(255, 256, 257) and several rounds of it (1025); element counts at the edges of its batches of four (1, 2, 4, 5) and at the cap."""
import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import ops

import symmetry_ref as S
import util

pytestmark = pytest.mark.gpu

TOL_M, TOL_PX = 1e-12, 1e-9
CAM = (614.7142806307731, 610.0, 320.0, 240.0)
POINTS = (1, 63, 64, 65, 255, 256, 257, 1025)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def cloud(n, seed=0):
    return np.random.default_rng(seed).uniform(-0.1, 0.1, (n, 3))


def poses(n, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    x = rng.uniform(-0.15, 0.15, (n, 3)) + [0.0, 0.0, 0.8]
    return np.concatenate([x, q], 1)


def group(n):
    """n elements: the identity, then rotations about various axes through various centres (closure is not asked for)"""
    rng = np.random.default_rng(100 + n)
    out = [list(S.IDENTITY)]
    for k in range(1, n):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        out.append(list(rng.uniform(-0.03, 0.03, 3)) + list(q))
    return np.array(out)


@pytest.mark.parametrize("n_sym", [1, 2, 4, 5, L.MAX_SCORE_SYMMETRIES])
def test_against_the_restatement(n_sym):
    sym = group(n_sym)
    est, ref = poses(3, 1), poses(3, 2)
    for P in (POINTS if n_sym <= 5 else (1, 65, 257)):
        pts = cloud(P, P)
        got = ops.pose_errors_sym("mssd", pts, est, ref, sym)
        want = S.pose_errors_sym("mssd", pts, est, ref, sym)
        print("mssd n_sym %d P %d: largest difference %.3g m" % (n_sym, P, np.abs(got - want).max()))
        assert np.all(np.abs(got - want) <= TOL_M), (n_sym, P, got, want)
        got = ops.pose_errors_sym("mspd", pts, est, ref, sym, CAM)
        want = S.pose_errors_sym("mspd", pts, est, ref, sym, CAM)
        print("mspd n_sym %d P %d: largest difference %.3g px" % (n_sym, P, np.abs(got - want).max()))
        assert np.all(np.isfinite(want)) and np.all(np.abs(got - want) <= TOL_PX), (n_sym, P, got, want)


@pytest.mark.parametrize("kind", ["mssd", "mspd"])
def test_pose_counts_and_position_in_the_call(kind):
    sym, pts = group(5), cloud(257, 3)
    est, ref = poses(3, 4), poses(3, 5)
    cam = CAM if kind == "mspd" else None
    assert ops.pose_errors_sym(kind, pts, est[:0], ref[:0], sym, cam).shape == (0,)
    whole = ops.pose_errors_sym(kind, pts, est, ref, sym, cam)
    for f in range(3):
        alone = ops.pose_errors_sym(kind, pts, est[f:f + 1], ref[f:f + 1], sym, cam)
        assert np.array_equal(bits(alone), bits(whole[f:f + 1])), f
    shuffled = ops.pose_errors_sym(kind, pts, est[::-1], ref[::-1], sym, cam)
    assert np.array_equal(bits(shuffled[::-1]), bits(whole))
    assert np.array_equal(bits(ops.pose_errors_sym(kind, pts, est, ref, sym, cam)), bits(whole)), "equal inputs, equal bits"


def test_identity_alone_is_at_least_add_and_a_flip_costs_nothing_under_its_group():
    pts = cloud(300, 6)
    est, ref = poses(4, 7), poses(4, 8)
    mssd = ops.pose_errors_sym("mssd", pts, est, ref)
    add = ops.pose_errors("add", pts, est, ref)
    assert np.all(mssd >= add), "a maximum is at least the mean"
    # the estimate right-multiplied by a group element: under the group it scores like the unflipped one under the identity
    sym = np.array([S.IDENTITY, S.half_turn(2, (0.01, -0.02, 0.0)), S.half_turn(0), S.half_turn(1, (0.0, 0.0, 0.02))])
    near = ref.copy()   # an estimate a few millimetres and a degree off the reference
    near[:, :3] += [0.002, -0.001, 0.003]
    near[:, 3:] = [S.quat_mul(r[3:], [np.cos(0.01), np.sin(0.01), 0.0, 0.0]) for r in ref]
    for g in range(1, 4):
        # on a point set that has the symmetry (p and G p), the estimate flipped by g scores under {e, g} what the unflipped one
        # scores under the identity: the element g pairs E G p with R G p, the same pairs over the same set
        Rg = np.array(S.quat_to_rot(sym[g, 3:])).reshape(3, 3)
        pts_g = np.concatenate([pts, pts @ Rg.T + sym[g, :3]])
        near_flipped = np.array([np.concatenate(S.flip_pose(e[:3], e[3:], sym[g])) for e in near])
        under = ops.pose_errors_sym("mssd", pts_g, near_flipped, ref, sym[[0, g]])
        plain = ops.pose_errors_sym("mssd", pts_g, near, ref)
        assert np.all(np.abs(under - plain) <= TOL_M) and np.all(plain > 1e-3), (g, under, plain)
        assert np.all(ops.pose_errors_sym("mssd", pts_g, near_flipped, ref) > 10 * plain), "without the group the flip shows"
        flipped = np.array([np.concatenate(S.flip_pose(r[:3], r[3:], sym[g])) for r in ref])
        same = ops.pose_errors_sym("mssd", pts, flipped, ref, sym[[0, g]])
        assert np.all(same <= 1e-12 + TOL_M), (g, same)   # the flipped pose IS the reference pose under the group
        px = ops.pose_errors_sym("mspd", pts, flipped, ref, sym[[0, g]], CAM)
        assert np.all(px <= 1e-9), (g, px)
        assert np.all(ops.pose_errors_sym("mssd", pts, flipped, ref) > 0.01), "... and is far from it without"


def test_points_behind_the_camera_and_non_finite_poses_stay_in_their_entry():
    pts, sym = cloud(65, 9), group(2)
    est, ref = poses(3, 10), poses(3, 11)
    clean_px = ops.pose_errors_sym("mspd", pts, est, ref, sym, CAM)
    clean_m = ops.pose_errors_sym("mssd", pts, est, ref, sym)
    for side in (0, 1):
        e, r = est.copy(), ref.copy()
        (e if side == 0 else r)[1, 2] = 0.05   # the object straddles Z = 0: some points at Z <= 0
        got = ops.pose_errors_sym("mspd", pts, e, r, sym, CAM)
        assert got[1] == np.inf and np.array_equal(bits(got[[0, 2]]), bits(clean_px[[0, 2]])), (side, got)
        assert S.pose_errors_sym("mspd", pts, e, r, sym, CAM)[1] == np.inf
        assert np.isfinite(ops.pose_errors_sym("mssd", pts, e, r, sym)[1]), "MSSD has no such rule"
    for bad in (np.nan, np.inf):
        e = est.copy()
        e[1, 4] = bad
        got = ops.pose_errors_sym("mssd", pts, e, ref, sym)
        assert not np.isfinite(got[1]) and np.array_equal(bits(got[[0, 2]]), bits(clean_m[[0, 2]])), (bad, got)
        got = ops.pose_errors_sym("mspd", pts, e, ref, sym, CAM)
        assert not np.isfinite(got[1]) and np.array_equal(bits(got[[0, 2]]), bits(clean_px[[0, 2]])), (bad, got)


def test_score_log_sym_equals_the_operator_on_the_logs_rows():
    import test_symmetry_gpu as G
    streams = S.streams()[:2]
    n = 8
    eng = G.make_engine(streams)
    eng.enable_log(6)   # (the ring wraps: frames 2 .. 7 are in it)
    keep = G.run(eng, streams, 0, n)
    first, cnt = 2, 6
    rows = eng.get_log_rows(first, cnt)
    sym, given = S.d2_group(), cloud(257, 12)
    c = streams[0].camera
    cam = (c.fx, c.fy, c.cx, c.cy)
    for obj, st in enumerate(streams):
        est = np.ascontiguousarray(rows[:, obj, 6:13])
        ref = np.concatenate([np.asarray(st.gt.x, float), np.asarray(st.gt.q, float)], 1)[first:first + cnt]
        for pts in (None, given):
            p = st.mesh[0].astype(np.float64) if pts is None else pts
            for kind in ("mssd", "mspd"):
                got = eng.score_log(kind, obj, first, cnt, ref, points=pts, symmetries=sym)
                want = ops.pose_errors_sym(kind, p, est, ref, sym, cam)
                assert np.array_equal(bits(got), bits(want)) and np.all(np.isfinite(got)) and got.max() > 0.0, (obj, kind, pts is None)
    out = np.zeros(cnt)
    ref = np.ascontiguousarray(ref)
    call = L.lib().roft_engine_score_log_sym
    assert call(eng._h, L.POSE_ERROR_MSSD, 0, first, cnt, None, 0, ref.ctypes.data, sym.ctypes.data, 4, out.ctypes.data) == L.OK
    assert call(eng._h, L.POSE_ERROR_MSSD, 0, first, 0, None, 0, ref.ctypes.data, sym.ctypes.data, 4, out.ctypes.data) == L.OK
    assert call(eng._h, L.POSE_ERROR_ADD, 0, first, cnt, None, 0, ref.ctypes.data, sym.ctypes.data, 4, out.ctypes.data) == L.ERR_INVALID
    assert call(eng._h, L.POSE_ERROR_MSSD, 2, first, cnt, None, 0, ref.ctypes.data, sym.ctypes.data, 4, out.ctypes.data) == L.ERR_INVALID
    assert call(eng._h, L.POSE_ERROR_MSSD, 0, first - 1, cnt, None, 0, ref.ctypes.data, sym.ctypes.data, 4, out.ctypes.data) == L.ERR_INVALID
    assert call(eng._h, L.POSE_ERROR_MSSD, 0, first, cnt, None, 0, ref.ctypes.data, sym.ctypes.data, 0, out.ctypes.data) == L.ERR_INVALID
    eng.close()
