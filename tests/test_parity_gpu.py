"""GPU parity tests: every HIP operator, called through the C ABI, against the CPU oracle on the
same seeded inputs.  Bars (see DESIGN.md "Parity"):
  * integer / index / byte work (flow point selection, mask propagation, render coverage): bit exact;
  * the float rasteriser and the double H-matrix assembly: bit exact (same operation order,
    -ffp-contract=off on both sides);
  * filter algebra whose summation order differs from the sequential CPU form (SKF information
    form, UKF, likelihood tree reduction): stated tolerances below.
"""
import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import ops, synth

import util

pytestmark = pytest.mark.gpu

# stated tolerances
SKF_RTOL = 1e-8        # information form vs the sequential 2-row recursion
UKF_ATOL = 1e-9        # block-wise parallel Jacobi vs cyclic Jacobi of the augmented covariance
LIK_RTOL = 1e-12       # tree reduction vs sequential double accumulation of float terms


def _cam(st):
    c = st.camera
    return L.Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy)


# ---------------------------------------------------------------------------------------------
# velocity stage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow_type,scale,shape", [
    (synth.FLOW_F32C2, 2, "A"), (synth.FLOW_S16C2, 2, "A"), (synth.FLOW_F32C2, 1, "A"), (synth.FLOW_S16C2, 2, "B")])
def test_flow_measurement_bit_exact(oracle, flow_type, scale, shape):
    st = util.stream(11, 4, scale=scale, flow_type=flow_type, shape=shape)
    ocam = util.oracle_camera(oracle, st.camera)
    for k in (1, 3):
        mask = st.mask_gt[k - 1].numpy()
        depth = st.depth[k - 1].numpy()
        flow = st.flow[k].numpy()
        n0, uv0, y0, H0 = oracle.flow_measurement(ocam, mask, depth, flow, st.dt)
        n1, uv1, y1, H1 = ops.flow_measurement(_cam(st), mask, depth, flow, st.dt)
        assert n0 > 10
        assert n1 == n0
        assert np.array_equal(uv0, uv1)
        assert np.array_equal(y0, y1)
        assert np.array_equal(H0, H1)


def test_flow_measurement_edge_cases(oracle):
    st = util.stream(12, 2, scale=2)
    ocam = util.oracle_camera(oracle, st.camera)
    cam = _cam(st)
    H, W = st.camera.height, st.camera.width
    depth = st.depth[0].numpy()
    flow = st.flow[1].numpy()
    rng = np.random.default_rng(0)
    cases = {
        "empty": np.zeros((H, W), np.uint8),
        "full": np.full((H, W), 255, np.uint8),
        "single": np.pad(np.array([[255]], np.uint8), ((H // 2, H - H // 2 - 1), (W // 2, W - W // 2 - 1))),
        "random": (rng.random((H, W)) < 0.3).astype(np.uint8) * 255,
        "last_pixel": np.pad(np.array([[255]], np.uint8), ((H - 1, 0), (W - 1, 0))),
    }
    for name, mask in cases.items():
        for radius in (35.0, 1.0, 7.0):
            if name == "full" and radius == 1.0:
                continue
            n0, uv0, y0, H0 = oracle.flow_measurement(ocam, mask, depth, flow, st.dt, radius=radius)
            n1, uv1, y1, H1 = ops.flow_measurement(cam, mask, depth, flow, st.dt, radius=radius)
            assert n1 == n0, (name, radius)
            assert np.array_equal(uv0, uv1) and np.array_equal(y0, y1) and np.array_equal(H0, H1), (name, radius)
    # plane sizes that are not a multiple of 16 bytes take the LDS variant of the kernel
    for W2, H2 in ((96, 54), (32, 6), (160, 90)):
        c2 = synth.Camera(W2, H2, 1.2 * W2, 1.2 * W2, W2 / 2.0, H2 / 2.0)
        ocam2, cam2 = util.oracle_camera(oracle, c2), L.Camera(W2, H2, c2.fx, c2.fy, c2.cx, c2.cy)
        mask2 = (rng.random((H2, W2)) < 0.4).astype(np.uint8) * 255
        depth2 = rng.uniform(0.3, 1.5, (H2, W2)).astype(np.float32)
        flow2 = (3.0 * rng.standard_normal((H2, W2, 2))).astype(np.float32)
        for radius in (1.0, 3.0, 35.0):
            n0, uv0, y0, H0 = oracle.flow_measurement(ocam2, mask2, depth2, flow2, st.dt, radius=radius)
            n1, uv1, y1, H1 = ops.flow_measurement(cam2, mask2, depth2, flow2, st.dt, radius=radius)
            assert n1 == n0 and n0 > 0, (W2, H2, radius)
            assert np.array_equal(uv0, uv1) and np.array_equal(y0, y1) and np.array_equal(H0, H1), (W2, H2, radius)
    # all depth invalid / beyond the gate -> nothing kept
    for bad in (np.zeros_like(depth), np.full_like(depth, 2.5), np.full_like(depth, np.nan)):
        n1, *_ = ops.flow_measurement(cam, st.mask_gt[0].numpy(), bad, flow, st.dt)
        assert n1 == 0
    # all flow invalid
    n1, *_ = ops.flow_measurement(cam, st.mask_gt[0].numpy(), depth, np.full_like(flow, np.nan), st.dt)
    assert n1 == 0
    n1, *_ = ops.flow_measurement(cam, st.mask_gt[0].numpy(), depth, np.full_like(flow, 1e10), st.dt)
    assert n1 == 0


def test_kf_predict(oracle):
    rng = np.random.default_rng(3)
    x = rng.normal(size=6)
    A = rng.normal(size=(6, 6))
    P = A @ A.T
    q = rng.random(6)
    x0, P0 = oracle.kf_predict(x, P, q)
    x1, P1 = ops.kf_predict(x, P, q)
    assert np.array_equal(x0, x1) and np.array_equal(P0, P1)


@pytest.mark.parametrize("reweight", [True, False])
def test_skf_correct_parity(oracle, reweight):
    st = util.stream(13, 6, scale=1)
    ocam = util.oracle_camera(oracle, st.camera)
    x = np.zeros(6)
    P = np.eye(6) * 1e-3
    worst = 0.0
    for k in range(1, 6):
        n, uv, y, Hm = oracle.flow_measurement(ocam, st.mask_gt[k - 1].numpy(), st.depth[k - 1].numpy(),
                                               st.flow[k].numpy(), st.dt)
        xp, Pp = oracle.kf_predict(x, P, np.full(6, 0.1))
        for nn in (n, n - 1):   # even and odd measurement counts (median of two / middle element)
            rc0, x0, P0 = oracle.skf_correct(xp, Pp, y[:2 * nn], Hm[:2 * nn], reweight=reweight)
            rc1, x1, P1 = ops.skf_correct(xp, Pp, y[:2 * nn], Hm[:2 * nn], reweight=reweight)
            assert rc0 == 0 and rc1 == 0
            sx = np.sqrt(np.diag(P0))
            worst = max(worst, np.max(np.abs(x1 - x0) / sx))
            np.testing.assert_allclose(x1, x0, rtol=SKF_RTOL, atol=SKF_RTOL * np.max(np.abs(x0)))
            np.testing.assert_allclose(P1, P0, rtol=SKF_RTOL, atol=SKF_RTOL * np.max(np.abs(P0)))
        x, P = x0, P0
    assert worst < 1e-6  # mean differs by far less than its own standard deviation


def test_skf_correct_large_n_bucket_select(oracle):
    """N of 1024 .. 2 500 and more on an ordinary stream: the median through the 1024-bin bucket select (several values per
    bucket, ranked by counting).  N does not choose the median's route, the clustering of the norms does: the radix-select
    fallback, N > 4096 and the other branches are aimed at in test_skf_paths_gpu.py."""
    st = util.stream(13, 3, scale=1)
    ocam = util.oracle_camera(oracle, st.camera)
    n, uv, y, Hm = oracle.flow_measurement(ocam, st.mask_gt[1].numpy(), st.depth[1].numpy(), st.flow[2].numpy(), st.dt,
                                           radius=7.0)
    assert n > 2500
    xp, Pp = oracle.kf_predict(np.zeros(6), np.eye(6) * 1e-3, np.full(6, 0.1))
    for nn in (n, n - 1, 1025, 1024):
        rc0, x0, P0 = oracle.skf_correct(xp, Pp, y[:2 * nn], Hm[:2 * nn], reweight=True)
        rc1, x1, P1 = ops.skf_correct(xp, Pp, y[:2 * nn], Hm[:2 * nn], reweight=True)
        assert rc0 == 0 and rc1 == 0
        np.testing.assert_allclose(x1, x0, rtol=SKF_RTOL, atol=SKF_RTOL * np.max(np.abs(x0)))
        np.testing.assert_allclose(P1, P0, rtol=SKF_RTOL, atol=SKF_RTOL * np.max(np.abs(P0)))


def test_skf_correct_small_and_empty(oracle):
    rng = np.random.default_rng(5)
    xp = rng.normal(size=6) * 0.1
    Pp = np.eye(6) * 0.1
    Hm = rng.normal(size=(6, 6)) * 10
    y = rng.normal(size=6)
    for n in (0, 1, 2, 3):
        rc0, x0, P0 = oracle.skf_correct(xp, Pp, y[:2 * n], Hm[:2 * n])
        rc1, x1, P1 = ops.skf_correct(xp, Pp, y[:2 * n], Hm[:2 * n])
        assert rc0 == rc1
        np.testing.assert_allclose(x1, x0, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(P1, P0, rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------------------------------------
# mask stage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flow_type,scale", [(synth.FLOW_F32C2, 2), (synth.FLOW_S16C2, 2), (synth.FLOW_F32C2, 1)])
def test_mask_propagate_bit_exact(oracle, flow_type, scale):
    st = util.stream(14, 8, scale=scale, flow_type=flow_type)
    flows = [st.flow[k].numpy() for k in range(1, 8)]
    m = st.mask_gt[0].numpy()
    for nfl in (0, 1, 3, 6):
        a = oracle.mask_propagate(m, flows[:nfl])
        b = ops.mask_propagate(m, flows[:nfl])
        assert np.array_equal(a, b), nfl
        assert a.any()
    # 7 flows given, only the last 6 are used (hpp:239-245)
    a = oracle.mask_propagate(m, flows[:7], 6)
    assert np.array_equal(a, ops.mask_propagate(m, flows[:7], 6))
    assert np.array_equal(a, ops.mask_propagate(m, flows[1:7], 6))
    # chained single-flow propagation, the every-frame path (hpp:221-226)
    a = b = m
    for k in range(1, 6):
        a2 = a.copy(); a2[0, 0] = 0
        b2 = b.copy(); b2[0, 0] = 0
        a = oracle.mask_propagate(a2, [flows[k - 1]])
        b = ops.mask_propagate(b2, [flows[k - 1]])
        assert np.array_equal(a, b), k


def test_mask_propagate_edge_cases(oracle):
    st = util.stream(15, 3, scale=2)
    H, W = st.camera.height, st.camera.width
    rng = np.random.default_rng(1)
    flow = (rng.normal(size=(H, W, 2)) * 4).astype(np.float32)
    flow[rng.random((H, W)) < 0.02] = np.nan
    flow[rng.random((H, W)) < 0.02] = 1e10
    flow[rng.random((H, W)) < 0.02] = -1e10
    flow2 = (rng.normal(size=(H, W, 2)) * 30).astype(np.float32)   # many targets leave the image
    masks = {
        "empty": np.zeros((H, W), np.uint8),
        "full": np.full((H, W), 255, np.uint8),
        "values_0_1_255": rng.choice(np.array([0, 1, 255], np.uint8), size=(H, W)),
        "corner_set": np.pad(np.full((8, 8), 255, np.uint8), ((0, H - 8), (0, W - 8))),  # mask(0,0) != 0
        "blob": st.mask_gt[0].numpy(),
    }
    for name, m in masks.items():
        for fl in ([flow], [flow2], [flow, flow2], [flow2, flow, flow2]):
            a = oracle.mask_propagate(m, fl)
            b = ops.mask_propagate(m, fl)
            assert np.array_equal(a, b), name


# ---------------------------------------------------------------------------------------------
# pose stage
# ---------------------------------------------------------------------------------------------
def _random_belief(rng, scale=1e-3):
    mean = np.zeros(13)
    mean[:9] = rng.normal(size=9) * np.array([.1, .1, .1, .5, .5, .5, .1, .1, .1]) + np.array([0] * 6 + [0, 0, .7])
    q = rng.normal(size=4)
    mean[9:] = q / np.linalg.norm(q)
    A = rng.normal(size=(12, 12))
    P = A @ A.T * scale + np.eye(12) * scale
    return mean, P


def test_ukf_predict_parity(oracle):
    rng = np.random.default_rng(21)
    for i in range(6):
        mean, P = _random_belief(rng)
        if i == 0:
            P = np.eye(12) * 1e-3            # degenerate spectrum (the initial condition)
        T = 1.0 / 30.0 if i < 4 else 0.05
        Q = oracle.process_noise([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], T)
        m0, P0 = oracle.ukf_predict(mean, P, Q, T)
        m1, P1 = ops.ukf_predict(mean, P, Q, T)
        np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
        np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)
        assert np.array_equal(ops.process_noise([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], T), Q)


@pytest.mark.parametrize("mtype", [L.MEAS_VELOCITY, L.MEAS_POSE_VELOCITY, L.MEAS_POSE])
def test_ukf_correct_parity(oracle, mtype):
    rng = np.random.default_rng(22 + mtype)
    rv = [0.1] * 3 + [1e-4] * 3
    rp = [1e-3] * 3 + [1e-4] * 3
    for i in range(6):
        mean, P = _random_belief(rng)
        if i == 0:
            P = np.eye(12) * 1e-3
        vel = rng.normal(size=6) * 0.3
        q = mean[9:] + rng.normal(size=4) * 0.05
        if i == 3:
            q = -q                           # double cover: -q is the same rotation
        pose = np.concatenate([mean[6:9] + rng.normal(size=3) * 0.01, q / np.linalg.norm(q)])
        if mtype == L.MEAS_VELOCITY:
            meas, rd = vel, rv
        elif mtype == L.MEAS_POSE:
            meas, rd = pose, rp
        else:
            meas, rd = np.concatenate([vel, pose]), rv + rp
        rc0, m0, P0 = oracle.ukf_correct(mean, P, mtype, meas, rd)
        rc1, m1, P1 = ops.ukf_correct(mean, P, mtype, meas, rd)
        assert rc0 == 0 and rc1 == 0
        np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
        np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)


def test_ukf_wide_sigma_clusters_take_the_general_paths(oracle):
    """Rotational standard deviations of ~0.35 rad: the sigma rotations (1.5 rad and more) are far outside the
    small-angle polynomials of k_ukf.hip and the sigma quaternions are a wide cluster, so the library sine / cosine /
    atan2 paths and the squaring scheme of the quaternion mean run instead of the fast paths."""
    rng = np.random.default_rng(77)
    rp = [1e-3] * 3 + [1e-4] * 3
    for i in range(4):
        mean, P = _random_belief(rng, scale=1e-2)
        T = 1.0 / 30.0
        Q = oracle.process_noise([1.0, 1.0, 1.0], [1.0, 1.0, 1.0], T)
        m0, P0 = oracle.ukf_predict(mean, P, Q, T)
        m1, P1 = ops.ukf_predict(mean, P, Q, T)
        np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
        np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)
        q = mean[9:] + rng.normal(size=4) * 0.05
        pose = np.concatenate([mean[6:9] + rng.normal(size=3) * 0.01, q / np.linalg.norm(q)])
        rc0, m0, P0 = oracle.ukf_correct(mean, P, L.MEAS_POSE, pose, rp)
        rc1, m1, P1 = ops.ukf_correct(mean, P, L.MEAS_POSE, pose, rp)
        assert rc0 == rc1 == 0
        np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
        np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)


def test_ukf_correct_sigma_rotations_beyond_pi(oracle):
    """Rotational standard deviations of ~0.9 rad: sigma rotations of sqrt(18) x that, well beyond pi.  The input deviation of
    such a column is what bfl computes from the sigma point -- the shortest-arc logarithm of q_sigma q_mean^-1, which wraps --
    and not the drawn offset itself (the shortcut k_ukf.hip takes below pi): cross covariance and gain follow the oracle."""
    rng = np.random.default_rng(91)
    rp = [1e-3] * 3 + [1e-4] * 3
    rv = [0.1] * 3 + [1e-4] * 3
    wrapped = 0
    for i in range(4):
        mean, P = _random_belief(rng, scale=1e-3)
        P[9:, 9:] += np.eye(3) * (0.8 + 0.1 * i)                      # var(theta) ~ 0.8 .. 1.1 rad^2
        wrapped += int(np.sqrt(18 * np.linalg.eigvalsh(P[9:, 9:]).max()) > np.pi)
        q = mean[9:] + rng.normal(size=4) * 0.05
        pose = np.concatenate([mean[6:9] + rng.normal(size=3) * 0.01, q / np.linalg.norm(q)])
        for mtype, meas, rd in ((L.MEAS_POSE, pose, rp), (L.MEAS_POSE_VELOCITY, np.concatenate([rng.normal(size=6) * 0.3, pose]), rv + rp)):
            rc0, m0, P0 = oracle.ukf_correct(mean, P, mtype, meas, rd)
            rc1, m1, P1 = ops.ukf_correct(mean, P, mtype, meas, rd)
            assert rc0 == rc1
            # (1e-6: a cluster this wide is ill-conditioned -- the two eigen square roots agree to ~1e-8 here; taking the drawn
            #  offset for the wrapped deviation is an error of order 1)
            np.testing.assert_allclose(m1, m0, rtol=0, atol=1e-6)
            np.testing.assert_allclose(P1, P0, rtol=0, atol=1e-6)
    assert wrapped == 4


def test_ukf_correct_no_measurement(oracle):
    rng = np.random.default_rng(2)
    mean, P = _random_belief(rng)
    rc, m1, P1 = ops.ukf_correct(mean, P, L.MEAS_NONE, np.zeros(6), np.ones(6))
    assert rc == 1
    assert np.array_equal(m1, mean) and np.array_equal(P1, P)


# ---------------------------------------------------------------------------------------------
# outlier rejection
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,mesh_n", [(2, 12), (1, 36)])
def test_render_depth_bit_exact(oracle, scale, mesh_n):
    st = util.stream(16, 2, scale=scale, mesh_n=mesh_n)
    verts, tris = st.mesh
    ocam = util.oracle_camera(oracle, st.camera)
    omesh = oracle.make_mesh(verts, tris)
    mesh = ops.make_mesh(verts, tris)
    div = 2 if st.camera.width == 640 else 4
    for k in range(2):
        x, q = st.gt.x[k], st.gt.q[k]
        t0 = oracle.render_depth(omesh, x, q, ocam, div)
        t1 = ops.render_depth(mesh, x, q, _cam(st), div)
        assert (t0 > 0).sum() > 50
        assert np.array_equal(t0, t1)
    # object behind the camera / off screen -> empty tile
    t1 = ops.render_depth(mesh, [0, 0, -1.0], [1, 0, 0, 0], _cam(st), div)
    assert not t1.any()
    t1 = ops.render_depth(mesh, [50.0, 0, 1.0], [1, 0, 0, 0], _cam(st), div)
    assert not t1.any()


# The engine's own outlier test (features_kernel -> outlier_fused_kernel -> deciding pose chain segment), one object, in
# every launch shape the engine can choose: 1 ... 8 workgroups per alternative sharing its triangles (windows merged in memory)
# and / or the rows of its window, the whole window in LDS or strips of a few rows, projected vertices cached in LDS or
# re-projected per triangle.  Render: bit exact against
# oracle/ro_render.c; likelihood: same samples, LIK_RTOL; decision identical.
@pytest.mark.parametrize("shape,scale,mesh_n,div", [("A", 1, 36, 2), ("B", 1, 24, 4), ("A", 2, 12, 2)])
def test_outlier_test_hot_path_kernel(oracle, shape, scale, mesh_n, div):
    st = util.stream(18, 2, scale=scale, mesh_n=mesh_n, shape=shape)
    verts, tris = st.mesh
    ocam = util.oracle_camera(oracle, st.camera)
    omesh = oracle.make_mesh(verts, tris)
    mesh = ops.make_mesh(verts, tris)
    depth = st.depth[0].numpy()
    mask = st.mask_gt[0].numpy()
    tw = st.camera.width // div
    # alternative 0 off by a few centimetres and degrees (an outlier pose), alternative 1 near the truth
    ang = 0.15
    dq = np.array([np.cos(ang / 2), 0.0, np.sin(ang / 2), 0.0])
    q0 = st.gt.q[0]
    q_off = np.array([dq[0] * q0[0] - dq[1:] @ q0[1:], *(dq[0] * q0[1:] + q0[0] * dq[1:] + np.cross(dq[1:], q0[1:]))])
    cases = [
        (np.stack([st.gt.x[0] + [0.03, -0.02, 0.05], st.gt.x[0] + [0.001, 0.0, 0.002]]), np.stack([q_off, q0]), 1),
        (np.stack([st.gt.x[0] + [0.002, 0.0, 0.001], st.gt.x[0] + [0.004, 0.001, 0.0]]), np.stack([q0, q0]), 0),
        # alternative 1 off screen: no sample -> DBL_MAX, alternative 0 kept
        (np.stack([st.gt.x[0], st.gt.x[0] + [50.0, 0.0, 0.0]]), np.stack([q0, q0]), 0),
    ]
    # (several workgroups per alternative share its TRIANGLES and merge their windows in memory -- and the rows of its window as
    #  well when it does not fit the LDS in one piece (window_pixels) -- or only its rows (split=False): both ways for 2 ... 8)
    shapes = [dict(bands=1), dict(bands=2), dict(bands=8), dict(bands=0), dict(bands=1, window_pixels=3 * tw),
              dict(bands=2, window_pixels=tw), dict(bands=1, vertex_cache=False), dict(bands=8, vertex_cache=False, window_pixels=2 * tw),
              dict(bands=8, split=False), dict(bands=8, split=True), dict(bands=4), dict(bands=4, split=False), dict(bands=2, split=True),
              dict(bands=8, split=True, vertex_cache=False), dict(bands=4, split=True, window_pixels=tw), dict(bands=3, split=True)]
    for x2, q2, want_sel in cases:
        t_ref = [oracle.render_depth(omesh, x2[k], q2[k], ocam, div) for k in range(2)]
        ref = [oracle.depth_likelihood(ocam, depth, mask, t_ref[k], div) for k in range(2)]
        assert (t_ref[0] > 0).sum() > 50
        L_first = None
        for kw in shapes:
            Lv, ns, sel, tiles = ops.outlier_test(_cam(st), div, depth, mask, mesh, x2, q2, **kw)
            # exact (integer) sums: the likelihood does not depend on bands, strips or the vertex cache, to the last bit
            L_first = list(Lv) if L_first is None else L_first
            assert list(Lv) == L_first, (kw, list(Lv), L_first)
            for k in range(2):
                assert np.array_equal(tiles[k], t_ref[k]), (kw, k, int((tiles[k] != t_ref[k]).sum()))
                assert ns[k] == ref[k][1], (kw, k)
                if ref[k][1] == 0:
                    assert Lv[k] == ref[k][0] == np.finfo(np.float64).max
                else:
                    assert abs(Lv[k] - ref[k][0]) <= LIK_RTOL * abs(ref[k][0]), (kw, k)
            assert sel == (1 if ref[0][0] > 2.0 * ref[1][0] else 0) == want_sel, kw


def test_render_and_outlier_test_on_a_mesh_of_the_reference(oracle, tmp_path):
    """The reference's own 003_cracker_box.obj (7 866 vertices, 15 728 triangles of very different sizes, as Meshlab wrote it; a
    fixture under tests/golden/ref_meshes) instead of the synthetic subdivided boxes: depth render bit exact against
    oracle/ro_render.c at both shapes, and the engine's outlier test in all its launch shapes on a scene rendered from that mesh."""
    from roft_amd import io, synth
    verts, tris = io.load_obj(util.ref_cracker_box(tmp_path))
    omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
    rng = np.random.default_rng(21)
    for cam, div in ((synth.Camera.shape_a(), 2), (synth.Camera.shape_b(), 4)):
        ocam = util.oracle_camera(oracle, cam)
        dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
        for _ in range(3):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            x = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.5, 0.9)])
            t0 = oracle.render_depth(omesh, x, q, ocam, div)
            t1 = ops.render_depth(mesh, x, q, dcam, div)
            assert (t0 > 0).sum() > 500 and np.array_equal(t0, t1)
        # a scene of that object: full-resolution depth = the oracle's render over a background plane, mask = its silhouette
        full = oracle.render_depth(omesh, x, q, ocam, 1)
        depth = np.where(full > 0, full, 1.5).astype(np.float32)
        mask = (full > 0).astype(np.uint8) * 255
        ang = 0.2
        dq = np.array([np.cos(ang / 2), np.sin(ang / 2), 0.0, 0.0])
        q_off = np.array([dq[0] * q[0] - dq[1:] @ q[1:], *(dq[0] * q[1:] + q[0] * dq[1:] + np.cross(dq[1:], q[1:]))])
        x2 = np.stack([x + [0.03, 0.02, 0.04], x + [0.001, 0.0, 0.001]])
        q2 = np.stack([q_off, q])
        t_ref = [oracle.render_depth(omesh, x2[k], q2[k], ocam, div) for k in range(2)]
        ref = [oracle.depth_likelihood(ocam, depth, mask, t_ref[k], div) for k in range(2)]
        tw = cam.width // div
        for kw in (dict(bands=1), dict(bands=2), dict(bands=8), dict(bands=0), dict(bands=2, window_pixels=tw), dict(bands=1, vertex_cache=False),
                   dict(bands=8, split=False), dict(bands=2, split=True), dict(bands=5, split=True)):
            Lv, ns, sel, tiles = ops.outlier_test(dcam, div, depth, mask, mesh, x2, q2, **kw)
            for k in range(2):
                assert np.array_equal(tiles[k], t_ref[k]), (kw, k, int((tiles[k] != t_ref[k]).sum()))
                assert ns[k] == ref[k][1] > 0 and abs(Lv[k] - ref[k][0]) <= LIK_RTOL * abs(ref[k][0]), (kw, k)
            assert sel == 1 == (1 if ref[0][0] > 2.0 * ref[1][0] else 0), kw


@pytest.mark.parametrize("name", ["box", "box_reversed", "box_random_windings", "box_open", "box_duplicate_triangle", "box_unwelded",
                                  "two_components", "projective_plane", "torus", "torus_open", "hollow_box"])
def test_render_follows_the_back_face_rule_of_the_contract(oracle, name):
    """Round 6: a mesh the classification accepts as a closed surface is rendered without the triangles that face away (and in a
    walk order of the engine's own); open / non-manifold / non-orientable meshes are drawn whole.  Either way the tile equals
    oracle/ro_render.c bit for bit, in every launch shape, and with the camera INSIDE the surface (a vertex behind the near plane:
    the rule is off for that render)."""
    import mesh_zoo
    from roft_amd import synth
    verts, tris, closed = mesh_zoo.zoo(14)[name]
    if name == "projective_plane":
        verts = (verts * 2.0).astype(np.float32)
    assert ops.mesh_classify(verts, tris)[0] == closed == oracle.mesh_classify(verts, tris)[0]
    omesh, mesh = oracle.make_mesh(verts, tris), ops.make_mesh(verts, tris)
    cam = synth.Camera.shape_a()
    ocam = util.oracle_camera(oracle, cam)
    dcam = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    rng = np.random.default_rng(31)
    poses = []
    for _ in range(4):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        poses.append((np.array([rng.uniform(-0.12, 0.12), rng.uniform(-0.08, 0.08), rng.uniform(0.35, 0.8)]), q))
    poses.append((np.array([0.0, 0.0, 0.02]), np.array([1.0, 0, 0, 0])))     # the camera inside the box: vertices behind it
    poses.append((np.array([0.0, 0.0, 0.09]), np.array([1.0, 0, 0, 0])))     # just in front of it: every vertex visible, rule on
    drawn = []
    for x, q in poses:
        t0 = oracle.render_depth(omesh, x, q, ocam, 2)
        t1 = ops.render_depth(mesh, x, q, dcam, 2)
        assert np.array_equal(t0, t1), (name, x, int((t0 != t1).sum()))
        drawn.append(int((t0 > 0).sum()))
    assert min(drawn[:4]) > 100, drawn     # (the two poses at the camera may leave a small mesh behind it)
    # the outlier test on a scene of that mesh, several launch shapes
    x, q = poses[0]
    full = oracle.render_depth(omesh, x, q, ocam, 1)
    depth = np.where(full > 0, full, 1.5).astype(np.float32)
    mask = (full > 0).astype(np.uint8) * 255
    x2 = np.stack([x + [0.02, 0.01, 0.03], x + [0.001, 0.0, 0.001]])
    q2 = np.stack([poses[1][1], q])
    t_ref = [oracle.render_depth(omesh, x2[k], q2[k], ocam, 2) for k in range(2)]
    ref = [oracle.depth_likelihood(ocam, depth, mask, t_ref[k], 2) for k in range(2)]
    for kw in (dict(bands=1), dict(bands=2), dict(bands=8), dict(bands=4, split=False), dict(bands=1, vertex_cache=False), dict(bands=2, window_pixels=320)):
        Lv, ns, sel, tiles = ops.outlier_test(dcam, 2, depth, mask, mesh, x2, q2, **kw)
        for k in range(2):
            assert np.array_equal(tiles[k], t_ref[k]), (name, kw, k, int((tiles[k] != t_ref[k]).sum()))
            assert ns[k] == ref[k][1]
            if ref[k][1]:
                assert abs(Lv[k] - ref[k][0]) <= LIK_RTOL * abs(ref[k][0]), (name, kw, k)
        assert sel == (1 if ref[0][0] > 2.0 * ref[1][0] else 0)


def test_outlier_test_no_samples(oracle):
    st = util.stream(18, 2, scale=2, mesh_n=12)
    mesh = ops.make_mesh(*st.mesh)
    x2 = np.stack([st.gt.x[0], st.gt.x[0]])
    q2 = np.stack([st.gt.q[0], st.gt.q[0]])
    depth = st.depth[0].numpy()
    mask = st.mask_gt[0].numpy()
    big = np.finfo(np.float64).max
    # empty mask; depth out of the hard-coded (0, 2) gate (ROFTFilter.cpp:561)
    for d, m in ((depth, np.zeros_like(mask)), (np.full_like(depth, 2.5), mask), (np.zeros_like(depth), mask)):
        Lv, ns, sel, _ = ops.outlier_test(_cam(st), 2, d, m, mesh, x2, q2, tiles=False)
        assert list(ns) == [0, 0] and Lv[0] == big and Lv[1] == big and sel == 0   # DBL_MAX > 2 DBL_MAX (= inf) is false


def test_depth_likelihood_parity(oracle):
    st = util.stream(17, 2, scale=1, mesh_n=24)
    verts, tris = st.mesh
    ocam = util.oracle_camera(oracle, st.camera)
    omesh = oracle.make_mesh(verts, tris)
    div = 2
    depth = st.depth[0].numpy()
    mask = st.mask_gt[0].numpy()
    for dx in (0.0, 0.02, 0.3):
        x = st.gt.x[0] + np.array([dx, 0, dx])
        tile = oracle.render_depth(omesh, x, st.gt.q[0], ocam, div)
        L0, n0 = oracle.depth_likelihood(ocam, depth, mask, tile, div)
        L1, n1 = ops.depth_likelihood(_cam(st), depth, mask, tile, div)
        assert n0 == n1
        if n0 == 0:
            assert L0 == L1 == np.finfo(np.float64).max
        else:
            assert abs(L1 - L0) <= LIK_RTOL * abs(L0)
    # no samples: empty mask, empty render
    L1, n1 = ops.depth_likelihood(_cam(st), depth, np.zeros_like(mask), tile, div)
    assert n1 == 0 and L1 == np.finfo(np.float64).max
    L1, n1 = ops.depth_likelihood(_cam(st), depth, mask, np.zeros_like(tile), div)
    assert n1 == 0 and L1 == np.finfo(np.float64).max


# ---------------------------------------------------------------------------------------------
# the committed conformance vectors (tests/golden/oracle_vectors): the HIP operators against golden DATA, not only against
# the oracle run next to them
# ---------------------------------------------------------------------------------------------
def test_hip_operators_against_the_committed_conformance_vectors():
    import glob
    import json
    import os

    def vec(c, key, dtype=np.float64):
        return np.array([[np.nan if x is None else x for x in row] for row in c[key]], dtype=np.float64).astype(dtype)

    files = sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_vectors", "*.json")))
    checked = 0
    for path in files:
        name = os.path.basename(path)[:-5]
        c = json.load(open(path))
        if name.startswith("ukf_predict"):
            m1, P1 = ops.ukf_predict(vec(c, "mean")[0], vec(c, "P"), vec(c, "Q"), c["T"][0][0], tuple(c["ut"][0]))
            np.testing.assert_allclose(m1, vec(c, "mean_out")[0], rtol=0, atol=UKF_ATOL)
            np.testing.assert_allclose(P1, vec(c, "P_out"), rtol=0, atol=UKF_ATOL)
        elif name.startswith("ukf_correct"):
            rc, m1, P1 = ops.ukf_correct(vec(c, "mean")[0], vec(c, "P"), int(c["type"][0][0]), vec(c, "meas")[0], vec(c, "Rdiag")[0], tuple(c["ut"][0]))
            atol = 1e-6 if "beyond_pi" in name else UKF_ATOL   # (see test_ukf_correct_sigma_rotations_beyond_pi)
            assert rc == c["status"][0][0]
            np.testing.assert_allclose(m1, vec(c, "mean_out")[0], rtol=0, atol=atol)
            np.testing.assert_allclose(P1, vec(c, "P_out"), rtol=0, atol=atol)
        elif name.startswith("skf_correct"):
            rc, x1, P1 = ops.skf_correct(vec(c, "x_pred")[0], vec(c, "P_pred"), vec(c, "y")[0], vec(c, "H"), tuple(c["Rdiag"][0]), bool(c["reweight"][0][0]))
            assert rc == c["status"][0][0]
            np.testing.assert_allclose(x1, vec(c, "x_out")[0], rtol=SKF_RTOL, atol=1e-12)
            np.testing.assert_allclose(P1, vec(c, "P_out"), rtol=SKF_RTOL, atol=1e-14)
        elif name.startswith("flow_measurement"):
            W, H = c["width"][0][0], c["height"][0][0]
            cam = L.Camera(W, H, *c["cam"][0])
            n, uv, y, Hm = ops.flow_measurement(cam, vec(c, "mask", np.uint8), vec(c, "depth", np.float32), vec(c, "flow", np.float32).reshape(H, W, 2),
                                                c["dt"][0][0], radius=c["radius"][0][0], depth_max=c["depth_max"][0][0])
            assert n == c["n"][0][0]
            assert np.array_equal(np.asarray(uv).reshape(-1, 2), vec(c, "uv", np.int64))
            assert np.array_equal(y, vec(c, "y")[0]) and np.array_equal(np.asarray(Hm).reshape(-1, 6), vec(c, "H"))
        elif name.startswith("mask_propagate"):
            W, H = c["width"][0][0], c["height"][0][0]
            flows = [vec(c, "flow%d" % k, np.float32).reshape(H, W, 2) for k in range(3)]
            assert np.array_equal(ops.mask_propagate(vec(c, "mask", np.uint8), flows), vec(c, "mask_out", np.uint8))
        else:
            continue
        checked += 1
    assert checked >= 15
