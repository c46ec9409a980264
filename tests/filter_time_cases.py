"""Case tables of tests/test_filter_time_cpu.py (the oracle alone: every case is usable and able to discriminate) and
tests/test_filter_time_gpu.py (the engine and the operators against the oracle): what parameterises the two filters in time and
per object -- the depth of the re-sync replay, the per-object noise of roft_object_desc, the time step of every (frame, object),
the parameters of the unscented transform -- at settings other than the defaults every other GPU test runs.

Two appliers take ONE dict of fields to both sides: engine_desc() to a roft_object_desc, oracle_over() to the keyword arguments of
util.oracle_config (one oracle tracker per object, as in util.run_oracle_tracker).

UT_SETS leaves alpha = 1e-3 out on purpose: there the two CPU references (oracle/ro_ukf.c and tests/ukf_numpy.py) already differ by
1e-10 .. 4e-10 -- lambda = alpha^2 (n + kappa) - n is within 2e-5 of -n, so c = n + lambda ~ 2e-5 and the centre weights are ~ -1e6 --
too close to the 1e-9 bar to tell a wrong kernel from rounding.  No set has alpha below 1e-2."""
import copy
import ctypes as C

import numpy as np

import util

# ---------------------------------------------------------------------------------------------------------------------------------
# per-object parameters
# ---------------------------------------------------------------------------------------------------------------------------------
# every field anisotropic with ratios >= 10 between the axes of a group of three (v_meas_cov_flow: between u and v), the ratios'
# ORDER different in every set, so that a swapped axis, a wrong offset into the parameter block or another object's block shows
PARAM_SETS = [
    dict(p_sigma_ang_vel=[0.1, 1.0, 10.0], p_psd_lin_acc=[10.0, 0.1, 1.0],
         p_meas_cov_v=[0.01, 0.1, 1.0], p_meas_cov_w=[1e-3, 1e-4, 1e-5], p_meas_cov_x=[1e-2, 1e-4, 1e-3], p_meas_cov_q=[1e-5, 1e-3, 1e-4],
         p_cov0_diag=[1e-4, 1e-3, 1e-2, 2e-2, 2e-4, 2e-3, 3e-3, 3e-5, 3e-4, 5e-5, 5e-3, 5e-4],
         v_q_diag=[0.01, 0.1, 1.0, 1.0, 0.01, 0.1], v_cov0_diag=[1e-2, 1e-4, 1e-3, 2e-4, 2e-3, 2e-2], v_meas_cov_flow=[0.3, 3.0]),
    dict(p_sigma_ang_vel=[5.0, 0.05, 0.5], p_psd_lin_acc=[0.2, 2.0, 20.0],
         p_meas_cov_v=[2.0, 0.02, 0.2], p_meas_cov_w=[3e-5, 3e-3, 3e-4], p_meas_cov_x=[2e-4, 2e-3, 2e-2], p_meas_cov_q=[4e-4, 4e-5, 4e-3],
         p_cov0_diag=[7e-3, 7e-4, 7e-5, 6e-4, 6e-3, 6e-2, 4e-5, 4e-4, 4e-3, 8e-3, 8e-5, 8e-4],
         v_q_diag=[2.0, 0.02, 0.2, 0.05, 0.5, 5.0], v_cov0_diag=[3e-4, 3e-3, 3e-2, 5e-2, 5e-4, 5e-3], v_meas_cov_flow=[4.0, 0.4]),
    dict(p_sigma_ang_vel=[2.0, 20.0, 0.2], p_psd_lin_acc=[0.5, 5.0, 0.05],
         p_meas_cov_v=[0.05, 5.0, 0.5], p_meas_cov_w=[6e-4, 6e-5, 6e-3], p_meas_cov_x=[5e-3, 5e-4, 5e-5], p_meas_cov_q=[2e-3, 2e-4, 2e-5],
         p_cov0_diag=[9e-4, 9e-2, 9e-3, 1.5e-3, 1.5e-2, 1.5e-4, 2.5e-4, 2.5e-3, 2.5e-5, 6.5e-4, 6.5e-5, 6.5e-3],
         v_q_diag=[0.3, 3.0, 0.03, 0.7, 0.07, 7.0], v_cov0_diag=[8e-3, 8e-2, 8e-4, 4e-3, 4e-4, 4e-2], v_meas_cov_flow=[0.2, 2.5]),
]
PARAM_FIELDS = tuple(PARAM_SETS[0])


def rotated(fields, name):
    """`fields` with the one field `name` rotated by one axis inside every group of three (the two flow variances swap)"""
    v = list(fields[name])
    g = 3 if len(v) % 3 == 0 else len(v)
    out = dict(fields)
    out[name] = [v[(i // g) * g + (i % g + 1) % g] for i in range(len(v))]
    return out


def engine_desc(st, fields=None, m0=None):
    """roft_object_desc of a stream's object: the engine's defaults, the initial pose, then `fields`"""
    from roft_amd import engine as E
    from roft_amd import synth
    d = E.default_object()
    m0 = synth.initial_pose_from_stream(st) if m0 is None else m0
    for i in range(13):
        d.p_mean0[i] = m0[i]
    for name, v in (fields or {}).items():
        a = getattr(d, name)
        assert len(a) == len(v), name
        for i, x in enumerate(v):
            a[i] = x
    return d


def oracle_over(fields=None):
    """The same fields as keyword arguments of util.oracle_config / restart_util.oracle_track (a TrackerConfig's array fields)"""
    return {name: (C.c_double * len(v))(*v) for name, v in (fields or {}).items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# time steps: per (frame, object)
# ---------------------------------------------------------------------------------------------------------------------------------
DT0 = 1.0 / 30.0
FALLBACK_SAMPLE_TIME = 0.04


def _jitter(seed, n):
    return DT0 * (1.0 + np.random.default_rng(seed).uniform(-0.3, 0.3, n))


# name -> (n_frames, n_objects) -> dt[n_frames, n_objects] as the ENGINE is fed it
DT_SCHEDULES = {
    "constant": lambda n, m: np.full((n, m), DT0),
    "jitter": lambda n, m: np.repeat(_jitter(5, n)[:, None], m, axis=1),                 # the camera's: one dt per frame
    "jitter_per_object": lambda n, m: np.stack([_jitter(50 + o, n) for o in range(m)], axis=1),
    "fallback": lambda n, m: np.repeat(np.where(np.arange(n) % 2 == 0, 0.0, -1.0)[:, None], m, axis=1),
}
# what goes with a schedule into BOTH configurations
DT_CONFIG = {"constant": {}, "jitter": {}, "jitter_per_object": {}, "fallback": dict(sample_time=FALLBACK_SAMPLE_TIME)}


def oracle_dt(dts, sample_time=DT0):
    """roft_frame_input::dt: `<= 0 means cfg.sample_time` -- what the oracle is fed for the engine's dt"""
    return np.where(dts > 0.0, dts, sample_time)


# ---------------------------------------------------------------------------------------------------------------------------------
# replay depth
# ---------------------------------------------------------------------------------------------------------------------------------
K_MAX_STEPS = 10   # roft_device.h


class ReplayCase:
    """A pose source that delivers every `period` frames, an engine configured with pose_frames_between = `depth`, and the frames
    whose pose is withheld.  kind: how the case relates to depth == period on the same stream."""

    def __init__(self, period, depth, drop=(), n=30):
        self.period, self.depth, self.drop, self.n = period, depth, tuple(drop), n
        self.kind = "equal" if depth == period else "below" if 0 < depth < period else "above" if depth > period else "unknown"
        self.id = "period%d-depth%d" % (period, depth) + ("-drop%s" % "_".join(map(str, drop)) if drop else "")


REPLAY_CASES = [ReplayCase(p, d) for p, d in ((3, 3), (6, 6), (8, 8),            # equal
                                              (6, 1), (6, 3), (8, 3), (8, 6),    # depth below the period: the front of the buffer is trimmed
                                              (3, 6), (3, 8),                    # above: nothing to trim
                                              (6, 0), (6, -1), (3, 0))]          # unknown: replay everything
# the boundary: with the depth unknown a period of 9 replays 10 = kMaxSteps buffered twists (11 corrections under outlier rejection:
# asserted on the oracle's n_ukf_corrections in test_filter_time_cpu.py); a period of 10 is refused
REPLAY_CASES.append(ReplayCase(9, 0))
REPLAY_CASES.append(ReplayCase(6, 6, drop=(12,)))
REPLAY_SEED = 41


def replay_case(name):
    return [c for c in REPLAY_CASES if c.id == name][0]


def replay_stream(case, seed=REPLAY_SEED, device="cpu"):
    """The case's stream: no randomly dropped poses (the schedule is the case's), its withheld poses taken out"""
    st = util.stream(seed, case.n, 2, pose_period=case.period, pose_drop_prob=0.0, device=device)
    return prepared(st, drop=case.drop)


def prepared(st, dts=None, drop=()):
    """A copy of a (cached, shared) stream with its own schedules: dt_frames[k] is what util.device_frame hands as frame k's dt, and
    the poses of the frames `drop` are withheld"""
    c = copy.copy(st)
    c.pose_valid = st.pose_valid.copy()
    for k in drop:
        assert c.pose_valid[k], k
        c.pose_valid[k] = False
    if dts is not None:
        c.dt_frames = np.asarray(dts, np.float64).copy()
    return c


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's side of an engine-level case
# ---------------------------------------------------------------------------------------------------------------------------------
def run_oracle(ob, st, n, fields=None, dts=None, withheld=(), **over):
    """util.run_oracle_tracker with per-object fields, a dt per frame (None: the stream's) and withheld poses; the rows also carry
    the covariance and the number of UKF corrections of the frame"""
    cfg = util.oracle_config(ob, st, **dict(over, **oracle_over(fields)))
    trk = ob.Tracker(cfg, *st.mesh)
    out = []
    for k in range(n):
        depth, flow, mask, pose = util.frame_inputs(st, k)
        if k in withheld:
            pose = None
        r = trk.step(st.dt if dts is None else float(dts[k]), depth, flow, mask, pose)
        out.append(dict(pose=np.array(r.pose), twist=np.array(r.twist), n=r.n_flow_points, sel=r.outlier_selected, L=np.array(r.outlier_L),
                        mask=trk.mask(), cov=np.array(r.pose_cov), nc=r.n_ukf_corrections))
    trk.close()
    return out


def trajectory_distance(a, b):
    """max over frames and components of |pose_a - pose_b| (13 numbers, the quaternion's sign resolved) of two oracle runs"""
    d = 0.0
    for ra, rb in zip(a, b):
        pa, pb = ra["pose"], rb["pose"]
        d = max(d, np.abs(pa[:9] - pb[:9]).max(), min(np.abs(pa[9:] - pb[9:]).max(), np.abs(pa[9:] + pb[9:]).max()))
    return float(d)


def debug_plan(cfg, pose_valid):
    """roft_debug_plan (host logic, no device) over a pose schedule: (steps, corrections, outlier step) per frame; the return code
    when the plan is refused"""
    from roft_amd import _lib as L
    n = len(pose_valid)
    pv = (C.c_int * n)(*[int(v) for v in pose_valid])
    ns, nc, out = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    rc = L.lib().roft_debug_plan(C.byref(cfg), pv, n, ns, nc, out, None)
    return rc if rc != 0 else (list(ns), list(nc), list(out))


# ---------------------------------------------------------------------------------------------------------------------------------
# operators: UT parameters, anisotropic R and Q on full covariances
# ---------------------------------------------------------------------------------------------------------------------------------
UKF_ATOL = 1e-9   # tests/test_parity_gpu.py
UT_DEFAULT = (1.0, 2.0, 0.0)
UT_SETS = [(0.5, 2.0, 1.0), (1.0, 2.0, 3.0), (0.1, 2.0, 0.0), (0.01, 2.0, 0.0)]
UT_BETA_ONLY = (1.0, 0.0, 0.0)   # moves a prediction by 1e-6 only (the centre column's covariance weight): velocity corrections only
OPERATIONS = ("predict", "correct_velocity", "correct_pose_velocity", "correct_pose")
OP_T = DT0
OP_PSD, OP_SIGMA_ANG = [2.0, 0.5, 1.0], [0.3, 1.0, 2.0]
OP_R_VELOCITY = [0.01, 0.1, 1.0, 1e-3, 1e-4, 1e-5]     # cov_v | cov_w of PARAM_SETS[0]
OP_R_POSE = [1e-2, 1e-4, 1e-3, 1e-5, 1e-3, 1e-4]       # cov_x | cov_q
OP_DRAWS = 3


def operator_cases():
    """[(name, operation, mean, P, measurement, Rdiag)]: OP_DRAWS beliefs per operation -- full covariances A A^T s + I s with s = 1e-2
    and means as _random_belief of tests/test_parity_gpu.py draws them, measurements as its test_ukf_correct_parity"""
    out = []
    for oi, op in enumerate(OPERATIONS):
        rng = np.random.default_rng(500 + oi)
        for i in range(OP_DRAWS):
            mean = np.zeros(13)
            mean[:9] = rng.normal(size=9) * np.array([.1, .1, .1, .5, .5, .5, .1, .1, .1]) + np.array([0] * 6 + [0, 0, .7])
            q = rng.normal(size=4)
            mean[9:] = q / np.linalg.norm(q)
            A = rng.normal(size=(12, 12))
            P = A @ A.T * 1e-2 + np.eye(12) * 1e-2
            vel = rng.normal(size=6) * 0.3
            q = mean[9:] + rng.normal(size=4) * 0.05
            pose = np.concatenate([mean[6:9] + rng.normal(size=3) * 0.01, q / np.linalg.norm(q)])
            meas, rd = {"predict": (None, None), "correct_velocity": (vel, OP_R_VELOCITY), "correct_pose": (pose, OP_R_POSE),
                        "correct_pose_velocity": (np.concatenate([vel, pose]), OP_R_VELOCITY + OP_R_POSE)}[op]
            out.append(("%s-%d" % (op, i), op, mean, P, meas, rd))
    return out


def run_operator(mod, L, case, ut, Q):
    """One operator case through `mod` (the oracle binding or roft_amd.ops; L: where the MEAS_* constants are): (status, mean, P)"""
    _, op, mean, P, meas, rd = case
    if op == "predict":
        m, Po = mod.ukf_predict(mean, P, Q, OP_T, ut)
        return 0, m, Po
    mtype = {"correct_velocity": L.MEAS_VELOCITY, "correct_pose": L.MEAS_POSE, "correct_pose_velocity": L.MEAS_POSE_VELOCITY}[op]
    return mod.ukf_correct(mean, P, mtype, meas, rd, ut)


def belief_distance(m0, P0, m1, P1):
    """max |difference| of two beliefs, the quaternion's sign resolved as tests/test_oracle_cpu.py does"""
    return float(max(np.abs(m0[:9] - m1[:9]).max(), min(np.abs(m0[9:] - m1[9:]).max(), np.abs(m0[9:] + m1[9:]).max()), np.abs(P0 - P1).max()))


# (UT set, operation) -> (bar on the GPU = max(UKF_ATOL, 100 floor), floor = max |oracle - ukf_numpy| over the operation's draws,
# effect = min over the draws of max |oracle(ut) - oracle(1, 2, 0)|): computed by test_filter_time_cpu.py, which asserts that the
# bars are the ones it computes and that effect >= 1000 bar for every pair.
# Not in the table, because the reference alone cannot meet effect >= 1000 bar: every UT set with "correct_pose" -- the pose
# measurement is linear in the state and its noise, the transform is exact for it whatever its parameters (measured effect 0 ..
# 2e-12, i.e. the references' own rounding); and UT_BETA_ONLY with anything but "correct_velocity" (3e-7 on a prediction).
OP_TABLE = {
    ((0.5, 2.0, 1.0), "predict"): (1e-9, 8.0e-16, 2.37e-4),
    ((0.5, 2.0, 1.0), "correct_velocity"): (1e-9, 2.6e-15, 1.01e-2),
    ((0.5, 2.0, 1.0), "correct_pose_velocity"): (1e-9, 1.1e-15, 3.49e-2),
    ((1.0, 2.0, 3.0), "predict"): (1e-9, 1.3e-15, 4.69e-5),
    ((1.0, 2.0, 3.0), "correct_velocity"): (1e-9, 2.9e-15, 2.15e-3),
    ((1.0, 2.0, 3.0), "correct_pose_velocity"): (1e-9, 1.6e-15, 3.19e-3),
    ((0.1, 2.0, 0.0), "predict"): (1e-9, 1.9e-14, 3.16e-4),
    ((0.1, 2.0, 0.0), "correct_velocity"): (1e-9, 1.4e-14, 1.40e-2),
    ((0.1, 2.0, 0.0), "correct_pose_velocity"): (1e-9, 3.8e-14, 6.13e-2),
    ((0.01, 2.0, 0.0), "predict"): (1e-9, 1.9e-12, 3.19e-4),
    ((0.01, 2.0, 0.0), "correct_velocity"): (1e-9, 6.9e-12, 1.42e-2),
    ((0.01, 2.0, 0.0), "correct_pose_velocity"): (1e-9, 5.4e-12, 6.22e-2),
    (UT_BETA_ONLY, "correct_velocity"): (1e-9, 2.6e-15, 4.34e-4),
}
