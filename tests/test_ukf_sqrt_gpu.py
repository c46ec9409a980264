"""The square roots of the pose UKF (k_ukf.hip): what a rewritten factorisation could break and the parity cases do not aim at.

Where each factorisation is reached.  The operator level (ops.ukf_predict / ops.ukf_correct) runs with both Cholesky guards at
0 -- always the eigen square root -- so it exercises only the factorisation of the innovation covariance Py (6 x 6 for a
velocity or a pose measurement, 12 x 12 for both) and the triangular solves behind it.  The two 12 x 12 factorisations of the
state covariance run only inside an ENGINE with the default guards.

(a) ops.ukf_correct against the oracle at UKF_ATOL (1e-9, the bar of tests/test_parity_gpu.py), all three measurement types,
    over covariances with condition numbers 1 ... 4.3e3.  The upper end is what the oracle's own tracker reaches on BASELINE
    config #5 (1280 x 720, S16C2 flow, pose re-sync and outlier rejection; objects 0 - 3, 600 frames, the corrected pose
    covariance of every frame): condition numbers 280 (first frame) to 4282 (3907 - 4282 over the four objects).  Plus singular
    innovation covariances: status 2 and the belief handed through unchanged, compared for equality.
(b) Engine runs with the default guards against the oracle tracker, poses AND covariances, frame by frame (single frames) and
    in batches of six (poses of every frame from the log, the covariance after every batch):
      * a stream that starts far above the guards (initial variances 5e-2 against the guard 4e-4) and converges below them:
        eigen square roots first, Cholesky factors afterwards, and the switch between them;
      * streams whose initial covariance is diag(1e-4) -- below the guard, so the first prediction takes the Cholesky path --
        with ONE entry set to 0: an exactly zero pivot in the first prediction, i.e. the non-positive-pivot path (flag 0 ->
        eigen fall-back) inside the guard.  Zero at index 0, 6 and 9 (first pivot, a position, a rotation).
    Bars: poses 1e-8 to the oracle and 1e-10 between the default guards and guards 0, as the existing guard tests have them.
    Covariances: the project had no bar; the largest deviation from the oracle, relative to the matrix's largest entry, measured
    on these streams with the library of the commit BEFORE the factorisations were touched is PARENT_COV_DEV below (1.03e-9), and
    the bar is ten times that, 1.03e-8 (reordered f64 sums move last bits; a wrong factor shows orders of magnitude above).  The
    library this file came with gives the same figures to the last digit: its factorisations keep every f64 operation.

Every input is chosen so that the oracle alone returns the expected status and stays finite over the whole run:
test_oracle_alone_accepts_every_input checks that without a GPU."""
import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import synth

import util

UKF_ATOL = 1e-9                      # tests/test_parity_gpu.py
POSE_TOL_ORACLE = 1e-8               # tests/test_engine_gpu.py::test_prediction_cholesky_guard_changes_nothing_measurable
POSE_TOL_GUARDS = 1e-10              # ... between the default guards and guards 0
PARENT_COV_DEV = 1.03e-9             # max over the streams below of max |P - P_oracle| / max |P_oracle| with the library of commit
                                     # a6aaeb2 (converging stream 1.03e-9, zero-pivot streams 8.8e-10, single frames and batches alike;
                                     # 1e-12 with guards 0: the figure is the Cholesky-against-eigen sigma set, not rounding noise)
COV_BAR = 10.0 * PARENT_COV_DEV

CONDITION_NUMBERS = [1.0, 30.0, 280.0, 1.0e3, 4.3e3]
MTYPES = [L.MEAS_VELOCITY, L.MEAS_POSE, L.MEAS_POSE_VELOCITY]
RV = [0.1] * 3 + [1e-4] * 3          # measurement noise diagonals of tests/test_parity_gpu.py
RP = [1e-3] * 3 + [1e-4] * 3


def belief(rng, cond, lam_max=1e-3):
    """Random belief whose covariance has eigenvalues log-spaced from lam_max down to lam_max / cond in a random basis."""
    mean = np.zeros(13)
    mean[:6] = rng.normal(size=6) * 0.1
    mean[6:9] = rng.normal(size=3) * 0.3 + np.array([0.0, 0.0, 0.8])
    q = rng.normal(size=4)
    mean[9:] = q / np.linalg.norm(q)
    U, _ = np.linalg.qr(rng.normal(size=(12, 12)))
    lam = lam_max * cond ** (-np.arange(12) / 11.0)
    P = (U * lam) @ U.T
    return mean, 0.5 * (P + P.T)


def measurement(rng, mean, mtype):
    vel = rng.normal(size=6) * 0.3
    q = mean[9:] + rng.normal(size=4) * 0.05
    pose = np.concatenate([mean[6:9] + rng.normal(size=3) * 0.01, q / np.linalg.norm(q)])
    if mtype == L.MEAS_VELOCITY:
        return vel, RV
    if mtype == L.MEAS_POSE:
        return pose, RP
    return np.concatenate([vel, pose]), RV + RP


def correct_cases():
    """(mean, P, mtype, measurement, R diagonal) for every measurement type and condition number, two draws each."""
    out = []
    for mtype in MTYPES:
        rng = np.random.default_rng(700 + mtype)
        for cond in CONDITION_NUMBERS:
            for _ in range(2):
                mean, P = belief(rng, cond)
                meas, rd = measurement(rng, mean, mtype)
                out.append((cond, mean, P, mtype, meas, rd))
    return out


def singular_cases():
    """(mean, P, mtype, measurement, R diagonal, expected status): innovation covariances that are exactly singular, and the
    regular neighbour of them."""
    rng = np.random.default_rng(5)
    mean, _ = belief(rng, 1.0)
    vel = rng.normal(size=6) * 0.3
    P3 = np.zeros((12, 12))
    P3[0, 0] = P3[1, 1] = P3[2, 2] = 1e-4
    return [(mean, np.zeros((12, 12)), L.MEAS_VELOCITY, vel, [0.0] * 6, 2),
            (mean, P3, L.MEAS_VELOCITY, vel, [0.0] * 6, 2),
            (mean, np.eye(12) * 1e-4, L.MEAS_VELOCITY, vel, [1e-4] * 6, 0)]


# ---- engine streams ------------------------------------------------------------------------------------------------------
def converging_stream():
    return util.stream(41, 40, 2), [5e-2] * 12, 40


def zero_pivot_stream(zero_at):
    cov0 = [1e-4] * 12
    if zero_at is not None:
        cov0[zero_at] = 0.0
    return util.stream(41, 20, 2), cov0, 20


def run_oracle(st, cov0, n):
    from oracle import binding as ob
    cfg = util.oracle_config(ob, st)
    for i in range(12):
        cfg.p_cov0_diag[i] = cov0[i]
    verts, tris = st.mesh
    trk = ob.Tracker(cfg, verts, tris)
    poses, covs, sel, npts = [], [], [], []
    for k in range(n):
        depth, flow, mask, pose = util.frame_inputs(st, k)
        r = trk.step(st.dt, depth, flow, mask, pose)
        poses.append(np.array(r.pose))
        covs.append(np.array(r.pose_cov).reshape(12, 12))
        sel.append(r.outlier_selected)
        npts.append(r.n_flow_points)
    trk.close()
    return np.array(poses), np.array(covs), sel, npts


def run_engine(st, cov0, n, T, guards=True):
    """Poses of every frame and the covariance after every submission (frame index -> matrix)."""
    from roft_amd import engine as E
    c = st.camera
    ecfg = E.default_config(c.width, c.height, st.flow_type, max_objects=1)
    ecfg.cam.fx, ecfg.cam.fy, ecfg.cam.cx, ecfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    ecfg.flow_grid, ecfg.flow_scale = st.flow_grid, st.flow_scale
    ecfg.max_batch_frames = T
    assert ecfg.ukf_cholesky_guard > 0.0 and ecfg.ukf_cholesky_guard_bilinear > 0.0   # the defaults are what is tested
    assert max(cov0) > ecfg.ukf_cholesky_guard or max(cov0) < ecfg.ukf_cholesky_guard / 2
    if not guards:
        ecfg.ukf_cholesky_guard = 0.0
        ecfg.ukf_cholesky_guard_bilinear = 0.0
    eng = E.ROFTFilterBatch(ecfg)
    d = E.default_object()
    m0 = synth.initial_pose_from_stream(st)
    for i in range(13):
        d.p_mean0[i] = m0[i]
    for i in range(12):
        d.p_cov0_diag[i] = cov0[i]
    eng.add_object(d, *st.mesh)
    eng.enable_log(n)
    covs = {}
    k = 0
    while k < n:
        t = min(T, n - k)
        frames = []
        for j in range(t):
            depth, flow, mask, pose = util.frame_inputs(st, k + j)
            frames.append([dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt)])
        if t == 1:
            eng.submit(frames[0])
        else:
            eng.submit_batch(frames)
        eng.step()
        k += t
        covs[k - 1] = eng.state(0)[1]
    pose, _twist, npts, sel = eng.get_log(0, n)
    eng.close()
    return pose[:, 0], covs, sel[:, 0], npts[:, 0]


def cov_deviation(covs, ref_covs):
    return max(float(np.abs(P - ref_covs[k]).max() / np.abs(ref_covs[k]).max()) for k, P in covs.items())


def check_engine_run(name, st, cov0, n, T):
    ref_pose, ref_cov, ref_sel, ref_n = run_oracle(st, cov0, n)
    pose, covs, sel, npts = run_engine(st, cov0, n, T)
    pose0, covs0, _, _ = run_engine(st, cov0, n, T, guards=False)
    assert len(covs) == (n if T == 1 else -(-n // T))
    dev_pose = float(np.abs(pose - ref_pose).max())
    dev_guard = float(np.abs(pose - pose0).max())
    dev_cov = cov_deviation(covs, ref_cov)
    dev_cov0 = cov_deviation(covs0, ref_cov)
    print("%s, batches of %d: max |pose - oracle| = %.3g, |pose - pose(guards 0)| = %.3g, covariance deviation %.3g (guards 0: %.3g)"
          % (name, T, dev_pose, dev_guard, dev_cov, dev_cov0))
    assert np.array_equal(npts, np.array(ref_n)) and np.array_equal(sel, np.array(ref_sel))
    assert np.isfinite(pose).all() and all(np.isfinite(P).all() for P in covs.values())
    assert dev_pose < POSE_TOL_ORACLE
    assert dev_guard < POSE_TOL_GUARDS
    assert dev_cov <= COV_BAR
    return covs


# ---- without a GPU -----------------------------------------------------------------------------------------------------------
def test_oracle_alone_accepts_every_input():
    """The oracle returns status 0 and finite results for every conditioned case, the expected status (2 with the belief
    untouched, or 0) for the singular ones, and its tracker stays finite on every engine stream -- on the zero-pivot streams
    close to the run without the zero."""
    from oracle import binding as ob
    for cond, mean, P, mtype, meas, rd in correct_cases():
        w = np.linalg.eigvalsh(P)
        assert abs(w[-1] / w[0] / cond - 1.0) < 1e-6
        rc, m, Pn = ob.ukf_correct(mean, P, mtype, meas, rd)
        assert rc == 0 and np.isfinite(m).all() and np.isfinite(Pn).all(), (cond, mtype)
    for mean, P, mtype, meas, rd, want in singular_cases():
        rc, m, Pn = ob.ukf_correct(mean, P, mtype, meas, rd)
        assert rc == want
        if want == 2:
            assert np.array_equal(m, mean) and np.array_equal(Pn, P)
    st, cov0, n = converging_stream()
    pose, cov, _, _ = run_oracle(st, cov0, n)
    assert np.isfinite(pose).all() and np.isfinite(cov).all()
    var_theta = np.array([P[9:, 9:].diagonal().max() for P in cov])
    assert cov0[9] > 4e-4 > var_theta.max()            # starts above the guard, is below it after the first pose measurement
    st, cov0, n = zero_pivot_stream(None)
    base, _, _, _ = run_oracle(st, cov0, n)
    for zero_at in (0, 6, 9):
        st, cov0, n = zero_pivot_stream(zero_at)
        pose, cov, _, _ = run_oracle(st, cov0, n)
        assert np.isfinite(pose).all() and np.isfinite(cov).all(), zero_at
        # (the zero changes the filter's prior, not only its arithmetic: the runs differ, by less than the prior's own standard
        #  deviation sqrt(1e-4) -- 2e-5, 5e-4 and 7e-3 for the three positions of the zero)
        print("zero at %d: max |pose - pose(no zero)| = %.3g" % (zero_at, np.abs(pose - base).max()))
        assert np.abs(pose - base).max() < 1e-2, zero_at


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mtype", MTYPES)
def test_ukf_correct_over_the_condition_numbers_of_a_long_run(mtype):
    from oracle import binding as ob
    from roft_amd import ops
    worst = 0.0
    n = 0
    for cond, mean, P, mt, meas, rd in correct_cases():
        if mt != mtype:
            continue
        rc0, m0, P0 = ob.ukf_correct(mean, P, mt, meas, rd)
        rc1, m1, P1 = ops.ukf_correct(mean, P, mt, meas, rd)
        dev = max(float(np.abs(m1 - m0).max()), float(np.abs(P1 - P0).max()))
        print("measurement type %d, condition number %.3g: status %d / %d, max deviation %.3g" % (mt, cond, rc0, rc1, dev))
        assert rc0 == 0 and rc1 == 0
        np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
        np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)
        worst = max(worst, dev)
        n += 1
    assert n == 2 * len(CONDITION_NUMBERS)


@pytest.mark.gpu
def test_singular_innovation_covariance_hands_the_belief_through():
    from oracle import binding as ob
    from roft_amd import ops
    for mean, P, mtype, meas, rd, want in singular_cases():
        rc0, m0, P0 = ob.ukf_correct(mean, P, mtype, meas, rd)
        rc1, m1, P1 = ops.ukf_correct(mean, P, mtype, meas, rd)
        assert rc0 == want and rc1 == want
        if want == 2:
            assert np.array_equal(m1, mean) and np.array_equal(P1, P)
        else:
            np.testing.assert_allclose(m1, m0, rtol=0, atol=UKF_ATOL)
            np.testing.assert_allclose(P1, P0, rtol=0, atol=UKF_ATOL)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 6])
def test_engine_converges_from_above_the_guards_to_below_them(T):
    """Eigen square roots while the variances are above the guards, Cholesky factors once they are below: both paths and the
    switch, poses and covariances against the oracle (which always takes the eigen square root)."""
    st, cov0, n = converging_stream()
    covs = check_engine_run("converging stream", st, cov0, n, T)
    var_theta = [P[9:, 9:].diagonal().max() for P in covs.values()]
    assert cov0[9] > 4e-4 > max(var_theta)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 6])
@pytest.mark.parametrize("zero_at", [0, 6, 9])
def test_engine_takes_the_eigen_fall_back_on_a_zero_pivot_inside_the_guard(zero_at, T):
    """diag(1e-4) with one zero entry: inside the guard, so the first prediction factorises -- and meets an exactly zero
    pivot.  The flag comes back 0 and the step decomposes instead; the run follows the oracle like any other."""
    st, cov0, n = zero_pivot_stream(zero_at)
    check_engine_run("zero pivot at %d" % zero_at, st, cov0, n, T)
