"""The velocity filter's HIP kernel (roft_amd/csrc/k_skf.hip, skf_core) on every median route, storage path and branch,
against the EXACT correction of tests/skf_ref.py (extended precision, information form) at the project's bar SKF_RTOL = 1e-8.
tests/test_skf_ref_cpu.py shows, without a GPU, that each case moves by more than 1e3 x that bar when the defect it aims at
(median rank off by one, rank N/2 taken for rank N/2 - 1, exchanged noise variances, no clamp, row-major pairing, the
weighted / unweighted switch inverted) is put into the reference.

Largest deviation from the exact reference per family, max over x (relative to max |x_ref|) and P (relative to max |P_ref|):

    family                 oracle (CPU, sequential)   HIP (MI355X, information form)
    fallback_duplicates    6.0e-15                    1.6e-15
    fallback_rank_edge     6.4e-15                    2.2e-15
    gross_outliers         4.3e-15                    1.6e-15
    straddle               2.3e-15                    1.7e-15
    small_ties             1.3e-14                    8.1e-15
    all_zero               1.3e-15                    6.5e-16
    scale_switch           1.1e-13                    9.5e-14
    clamp                  3.9e-15                    6.3e-16
    edges                  3.4e-14                    2.7e-14
    unequal_noise          3.1e-15                    9.2e-16
    prior_conditioning     2.2e-15                    6.8e-16
    no_reweight            3.4e-15                    1.8e-15
    point entry (records)  --                         1.2e-15
    engine chain           --                         4.1e-15

The bar stays at SKF_RTOL: it is the project's statement, not a fit to these figures (docs/notebook.md has the discussion).
"""
import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops

import skf_ref as R
from test_parity_gpu import SKF_RTOL

pytestmark = pytest.mark.gpu


def _report(kind, family, name, x, P, x_ref, P_ref):
    print("SKFDEV %s %-20s %-32s dx %.2e dP %.2e" % ((kind, family, name) + R.deviation(x, P, x_ref, P_ref)))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------
# explicit (y, H): every case of the table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.cases()))
def test_skf_correct_case_against_exact(name):
    c = R.cases()[name]
    st, x_ref, P_ref, _ = R.exact(name)
    rc, x, P = ops.skf_correct(c.x_pred, c.P_pred, c.y, c.H, c.rdiag, c.reweight)
    assert rc == st == 0
    _report("hip", c.family, name, x, P, x_ref, P_ref)
    R.assert_close(x, P, x_ref, P_ref, SKF_RTOL, name)
    assert np.array_equal(P, P.T)
    if c.family == "all_zero":
        assert np.array_equal(_bits(x), _bits(c.x_pred))


def test_skf_correct_empty_measurement():
    c = R.cases()["edge_3"]
    rc, x, P = ops.skf_correct(R.X_TRUE, c.P_pred, np.zeros(0), np.zeros((0, 6)))
    assert rc == 1 and np.array_equal(x, R.X_TRUE) and np.array_equal(P, c.P_pred)


# ---------------------------------------------------------------------------------------------
# flow points: the record accessor (H rows rebuilt on the device with reciprocal multiplies)
# ---------------------------------------------------------------------------------------------
def _lcam(cam):
    return L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)


def _points(cam, n, seed):
    """n flow points: integer pixels with the four corners, the principal point, u = cx and v = cy among them, float32 depth in
    [0.05, 2.0] and a float32 flow of a rigid motion with Laplacian noise and 5 % gross outliers."""
    rng = np.random.default_rng(seed)
    uv, _ = R.random_points(rng, n, cam)
    W, H, cx, cy = cam.width, cam.height, int(cam.cx), int(cam.cy)
    assert cx == cam.cx and cy == cam.cy
    special = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (cx, cy)]
    special += [(cx, int(v)) for v in rng.integers(0, H, 6)] + [(int(u), cy) for u in rng.integers(0, W, 6)]
    where = rng.choice(n, len(special), replace=False)
    uv[where] = np.array(special, np.int32)
    z = rng.uniform(0.05, 2.0, n).astype(np.float32)
    z[where[:2]] = np.float32(0.05), np.float32(2.0)
    Hd = R.yh_from_points_f64(cam, R.DT, uv, z, np.zeros((n, 2), np.float32))[1]
    flow = (Hd @ R.X_TRUE + rng.laplace(0.0, 0.5, 2 * n)).reshape(n, 2)
    bad = rng.random(n) < 0.05
    flow[bad] += rng.uniform(-20.0, 20.0, (int(bad.sum()), 2))
    return uv, z, flow.astype(np.float32)


@pytest.mark.parametrize("reweight", [True, False])
@pytest.mark.parametrize("n", [700, 4096, 4097])
@pytest.mark.parametrize("cam", [R.CAM_VGA, R.CAM_HD], ids=["640x480", "1920x1080"])
def test_skf_correct_points_against_exact_and_arrays(cam, n, reweight):
    uv, z, flow = _points(cam, n, 5000 + n)
    xp, Pp, rd = 0.8 * R.X_TRUE, R.P_GENERIC, (0.25, 4.0)
    st, x_ref, P_ref = R.skf_exact_points(cam, R.DT, xp, Pp, uv, z, flow, rd, reweight)
    rc, x, P = ops.skf_correct_points(_lcam(cam), R.DT, xp, Pp, uv, z, flow, rd, reweight)
    assert rc == st == 0
    _report("hip", "points", "%dx%d_n%d_rw%d" % (cam.width, cam.height, n, reweight), x, P, x_ref, P_ref)
    R.assert_close(x, P, x_ref, P_ref, SKF_RTOL)
    # the same measurement as explicit (y, H) with the literal divisions of the measurement model
    y, Hd = R.yh_from_points_f64(cam, R.DT, uv, z, flow)
    rc2, x2, P2 = ops.skf_correct(xp, Pp, y, Hd, rd, reweight)
    assert rc2 == 0
    R.assert_close(x, P, x2, P2, SKF_RTOL)
    R.assert_close(x2, P2, x_ref, P_ref, SKF_RTOL)


def test_skf_correct_points_sees_the_noise_variances_in_order():
    """(0.25, 4.0) and (4.0, 0.25) through the record accessor: each matches its own exact result, and the two differ."""
    uv, z, flow = _points(R.CAM_VGA, 700, 5001)
    xp, Pp = 0.8 * R.X_TRUE, R.P_GENERIC
    res = []
    for rd in ((0.25, 4.0), (4.0, 0.25)):
        _, x_ref, P_ref = R.skf_exact_points(R.CAM_VGA, R.DT, xp, Pp, uv, z, flow, rd, True)
        rc, x, P = ops.skf_correct_points(_lcam(R.CAM_VGA), R.DT, xp, Pp, uv, z, flow, rd, True)
        assert rc == 0
        R.assert_close(x, P, x_ref, P_ref, SKF_RTOL)
        res.append((x_ref, P_ref))
    assert max(R.deviation(res[1][0], res[1][1], res[0][0], res[0][1])) > 1e3 * SKF_RTOL


# ---------------------------------------------------------------------------------------------
# status 3: P_pred (or the information matrix) not positive definite -- a documented return, the belief is left as it was
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["negative_eigenvalue", "zero_pivot", "nan_diagonal"])
def test_status_3_leaves_the_belief_bit_for_bit(kind):
    Pbad = R.bad_priors()[kind]
    xp = R.X_TRUE.copy()
    c = R.cases()["edge_65"]
    assert R.skf_exact(xp, Pbad, c.y, c.H)[0] == 3
    rc, x, P = ops.skf_correct(xp, Pbad, c.y, c.H)
    assert rc == 3
    assert np.array_equal(_bits(x), _bits(xp)) and np.array_equal(_bits(P), _bits(Pbad))
    uv, z, flow = _points(R.CAM_VGA, 65, 5002)
    rc, x, P = ops.skf_correct_points(_lcam(R.CAM_VGA), R.DT, xp, Pbad, uv, z, flow)
    assert rc == 3
    assert np.array_equal(_bits(x), _bits(xp)) and np.array_equal(_bits(P), _bits(Pbad))
    # the library is as usable as before
    rc, x, P = ops.skf_correct(c.x_pred, c.P_pred, c.y, c.H)
    R.assert_close(x, P, R.exact("edge_65")[1], R.exact("edge_65")[2], SKF_RTOL)


# ---------------------------------------------------------------------------------------------
# engine chain (skf_chain_kernel) against operator chain (skf_records_kernel): the same skf_core<RecAccessor>
# ---------------------------------------------------------------------------------------------
def _engine_scene(n_frames):
    """160 x 120, three objects with their own masks, depths and flows: two keep more than 4096 points per frame at a
    sub-sampling radius of 1 (innovations and norms in the global scratch, one slice per object), one keeps 2 (unobservable)."""
    Wd, Hd = 160, 120
    rng = np.random.default_rng(77)
    rects = [(10, 80, 20, 100), (30, 105, 60, 126), None]       # rows r0:r1, columns c0:c1 -- 5600 and 4950 pixels
    drift = [np.array([1.5, -0.8]), np.array([-2.0, 1.2]), np.array([0.3, 0.3])]
    objs = []
    for o in range(3):
        frames = []
        for k in range(n_frames):
            mask = np.zeros((Hd, Wd), np.uint8)
            if rects[o]:
                r0, r1, c0, c1 = rects[o]
                mask[r0 + k:r1 + k, c0 + 2 * k:c1 + 2 * k] = 255
            else:
                mask[50 + k, 70] = mask[90, 20 + k] = 255
            depth = rng.uniform(0.4, 1.2, (Hd, Wd)).astype(np.float32)
            flow = drift[o] * (1.0 + 0.1 * k) + rng.laplace(0.0, 0.6, (Hd, Wd, 2))
            bad = rng.random((Hd, Wd)) < 0.04
            flow[bad] += rng.uniform(-15.0, 15.0, (int(bad.sum()), 2))
            frames.append(dict(mask=mask, depth=depth, flow=flow.astype(np.float32), pose=None, dt=R.DT))
        objs.append(frames)
    return Wd, Hd, objs


def test_engine_chain_equals_operator_chain_bit_for_bit():
    n_frames, T = 6, 3
    Wd, Hd, objs = _engine_scene(n_frames)
    cam = R.Camera(Wd, Hd, 150.0, 148.5, 80.0, 60.0)
    rd = (0.25, 4.0)
    cfg = E.default_config(Wd, Hd, L.FLOW_F32C2, max_objects=3, max_batch_frames=T)
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = cam.fx, cam.fy, cam.cx, cam.cy
    cfg.flow_grid, cfg.flow_scale = 1, 1.0
    cfg.subsampling_radius = 1.0
    cfg.flow_weighting = 1
    cfg.flow_aided_segmentation = 0      # the mask of frame k - 1, as submitted, is the flow measurement's mask of frame k
    cfg.use_pose_resync = 0
    cfg.outlier_rejection = 0
    eng = E.ROFTFilterBatch(cfg)
    verts = np.array([[x, y, z] for x in (-0.03, 0.03) for y in (-0.03, 0.03) for z in (-0.03, 0.03)], np.float32)
    tris = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                     [1, 5, 7], [1, 7, 3]], np.int32)
    beliefs, vq = [], []
    for o in range(3):
        d = E.default_object()
        d.p_mean0[6:9] = (0.0, 0.0, 0.6)
        d.p_mean0[9:13] = (1.0, 0.0, 0.0, 0.0)
        for i in range(6):
            d.v_mean0[i] = 0.01 * (i + 1) * (o + 1)
        d.v_meas_cov_flow[0], d.v_meas_cov_flow[1] = rd
        eng.add_object(d, verts, tris)
        beliefs.append([np.array(d.v_mean0[:]), np.diag(np.array(d.v_cov0_diag[:]))])
        vq.append(np.array(d.v_q_diag[:]))
    eng.enable_log(n_frames)
    start = [b[0].copy() for b in beliefs]

    lcam = _lcam(cam)
    worst = 0.0
    large_inputs = {}
    try:
        for first in range(0, n_frames, T):
            eng.submit_batch([[objs[o][k] for o in range(3)] for k in range(first, first + T)])
            eng.step()
            _, twist, npts, _ = eng.get_log(first, T)
            for k in range(first, first + T):
                for o in range(3):
                    x, P = beliefs[o]
                    if k == 0:
                        n = -1                    # no previous frame: no flow measurement
                    else:
                        prev, cur = objs[o][k - 1], objs[o][k]
                        n, uv, y, _ = ops.flow_measurement(lcam, prev["mask"], prev["depth"], cur["flow"], R.DT, radius=1.0)
                        assert n == (2 if o == 2 else np.count_nonzero(prev["mask"]))
                        assert (n > 4096) if o < 2 else (n < 3)
                    assert npts[k - first, o] == n, (k, o)
                    if n >= 3:                    # N < 3: unobservable, the belief stays as it was before the prediction
                        z, fxy = prev["depth"][uv[:, 1], uv[:, 0]], cur["flow"][uv[:, 1], uv[:, 0]]
                        assert np.array_equal(fxy.astype(np.float64).reshape(-1), y)
                        xp, Pp = ops.kf_predict(x, P, vq[o])
                        rc, x1, P1 = ops.skf_correct_points(lcam, R.DT, xp, Pp, uv, z, fxy, rd, True)
                        assert rc == 0
                        st, x_ref, P_ref = R.skf_exact_points(cam, R.DT, xp, Pp, uv, z, fxy, rd, True)
                        assert st == 0
                        _report("hip", "engine", "frame%d_obj%d_n%d" % (k, o, n), x1, P1, x_ref, P_ref)
                        worst = max(worst, *R.deviation(x1, P1, x_ref, P_ref))
                        R.assert_close(x1, P1, x_ref, P_ref, SKF_RTOL, (k, o))
                        beliefs[o] = [x1, P1]
                        large_inputs.setdefault(k, {})[o] = (uv, fxy)
                    assert np.array_equal(_bits(twist[k - first, o]), _bits(beliefs[o][0])), (k, o)
            for o in range(3):
                _, _, tw, Pv = eng.state(o)
                assert np.array_equal(_bits(tw), _bits(beliefs[o][0])), (first, o)
                assert np.array_equal(_bits(Pv), _bits(beliefs[o][1])), (first, o)
    finally:
        eng.close()
    # the two large objects had distinct measurements and ended at distinct beliefs: overlapping scratch slices would show
    for k, per in large_inputs.items():
        assert set(per) == {0, 1}
        assert per[0][0].shape != per[1][0].shape or not np.array_equal(per[0][0], per[1][0])
    assert max(R.deviation(beliefs[1][0], beliefs[1][1], beliefs[0][0], beliefs[0][1])) > 1e3 * SKF_RTOL
    assert np.array_equal(beliefs[2][0], start[2]) and np.any(start[2] != 0.0)     # the unobservable object never moved
    print("SKFDEV hip engine worst %.2e" % worst)
