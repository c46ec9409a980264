"""The pose and velocity filters at other settings than the ones every other GPU test runs (tests/filter_time_cases.py): replay
depths pose_frames_between = 1 .. 8 and unknown on pose sources of period 3 .. 9, anisotropic noise that differs from object to
object, a time step per (frame, object), UT parameters other than (1, 2, 0) -- the engine against one oracle tracker per object at
the bars of tests/test_engine_gpu.py (point counts, decisions and masks equal; pose, rotation and twist within 1e-6; likelihoods
within 1e-9), the operators against the oracle at the bars of the case table.  tests/test_filter_time_cpu.py shows on the oracle
alone that every one of these settings moves the result by at least 100 (engine) or 1000 (operators) times its bar.

Streams: util.stream(seed, 30, scale=2, pose_period=...) -- 320 x 240, a 12-subdivision box -- at most three objects per engine.
Every test prints its largest deviation (docs/notebook.md)."""
import ctypes as C
import functools

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops

import filter_time_cases as F
import restart_util as R
import util
from test_engine_gpu import POS_TOL, compare, make_engine

pytestmark = pytest.mark.gpu

N = 30
NO_GUARDS = dict(ukf_cholesky_guard=0.0, ukf_cholesky_guard_bilinear=0.0)


def _show(what, rep):
    print("%s: max deviation from the oracle: position / velocity state %.3g, rotation %.3g, twist %.3g, likelihood (relative) %.3g"
          % (what, rep["pos"], rep["rot"], rep["twist"], rep["lik"]))


def _streams(seeds, **kw):
    return [util.stream(s, N, 2, **kw) for s in seeds]


# ---- per-object parameters ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guards", [{}, NO_GUARDS], ids=["default-guards", "guards-0"])
@pytest.mark.parametrize("schedule", ["constant", "jitter"])
@pytest.mark.parametrize("seeds", [(41, 41, 41), (41, 42, 43)], ids=["one-stream", "three-streams"])
def test_every_object_follows_the_oracle_for_its_own_parameters(seeds, schedule, guards):
    """Three objects, three parameter sets, then the same engine with the sets dealt in another order: ukf_one_step's copy of the
    head of ObjParams, Q(T) built from it in the kernel, R of the three measurement types, the velocity filter's Q and R, both
    initial covariances -- per object, per axis.  With the square roots' Cholesky guards at their defaults and at 0 (eigen only)."""
    streams = _streams(seeds)
    dts = F.DT_SCHEDULES[schedule](N, 3)
    tests = 0
    for order in ((0, 1, 2), (2, 0, 1)):
        rep = {}
        tests += compare(streams, N, descs=[F.PARAM_SETS[i] for i in order], dts=dts, report=rep, **guards)
        _show("sets %s, dt %s" % (order, schedule), rep)
    assert tests >= 12   # (outlier tests: the pose arrivals of three objects, twice)


# ---- time steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,guards", [("constant", {}), ("jitter", {}), ("jitter", NO_GUARDS), ("jitter_per_object", {}),
                                             ("jitter_per_object", NO_GUARDS), ("fallback", {})],
                         ids=["constant", "jitter", "jitter-guards-0", "jitter_per_object", "jitter_per_object-guards-0", "fallback"])
def test_time_step_per_frame_and_object(schedule, guards):
    """dt enters the flow measurement's rows, Q(T), the motion model and the prediction's Cholesky guard; every step of a re-sync
    replay uses the delivering frame's; <= 0 means roft_config::sample_time.  The jittered schedules also with the guards at 0."""
    streams = _streams((41, 42, 43))
    rep = {}
    compare(streams, N, descs=[None, F.PARAM_SETS[1], F.PARAM_SETS[2]], dts=F.DT_SCHEDULES[schedule](N, 3), report=rep,
            **dict(F.DT_CONFIG[schedule], **guards))
    _show("dt %s" % schedule, rep)


def _logged(streams, descs, n, **kw):
    return util.run_engine_logged(functools.partial(make_engine, descs=descs), streams, n, **kw)


def _same(a, b, what):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y), what
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), what


def test_a_time_step_of_zero_or_less_is_the_sample_time_bit_for_bit():
    streams = _streams((41, 42))
    descs = [None, F.PARAM_SETS[0]]
    fb = F.DT_SCHEDULES["fallback"](N, 2)
    fed = [util.to_device(F.prepared(st, fb[:, o])) for o, st in enumerate(streams)]
    explicit = [util.to_device(F.prepared(st, np.full(N, F.FALLBACK_SAMPLE_TIME))) for st in streams]
    a = _logged(fed, descs, N, sample_time=F.FALLBACK_SAMPLE_TIME)
    b = _logged(explicit, descs, N, sample_time=F.FALLBACK_SAMPLE_TIME)
    c = _logged(explicit, descs, N)                       # (an explicit dt does not read sample_time)
    d = _logged([util.to_device(st) for st in streams], descs, N)
    _same(a, b, "dt <= 0 against dt = sample_time")
    _same(b, c, "sample_time with every dt given")
    assert np.abs(a[0][0] - d[0][0]).max() > 1e-4         # ... and 0.04 is not 1/30


# ---- replay depth ---------------------------------------------------------------------------------------------------------------
def _replay_setup(case):
    """two objects on the case's pose schedule: default parameters and a parameter set; the withheld poses as compare takes them"""
    streams = [util.stream(F.REPLAY_SEED + o, case.n, 2, pose_period=case.period, pose_drop_prob=0.0) for o in range(2)]
    withheld = {(k, o) for k in case.drop for o in range(2)}
    return streams, [None, F.PARAM_SETS[1]], withheld


@pytest.mark.parametrize("case", F.REPLAY_CASES, ids=lambda c: c.id)
def test_replay_depth(case):
    """build_pose_program at depths other than 6: the trimming of the buffered twists, the ring slot of the first replayed step,
    depth above the period and unknown depth (replay everything), exactly kMaxSteps steps, a withheld pose."""
    streams, descs, withheld = _replay_setup(case)
    rep = {}
    tests = compare(streams, case.n, descs=descs, withheld=withheld, report=rep, pose_frames_between=case.depth)
    _show(case.id, rep)
    assert tests >= 2 * (len(range(case.period, case.n, case.period)) - len(case.drop))
    # the frame programs replay as deep as the oracle: corrections per frame, on every frame
    cfg = E.default_config(320, 240)
    cfg.pose_frames_between = case.depth
    valid = [bool(streams[0].pose_valid[k]) and (k, 0) not in withheld for k in range(case.n)]
    steps, corrections, _ = F.debug_plan(cfg, valid)
    assert corrections == [r["nc"] for r in rep["ref"][0]]
    arrival = [k for k in range(case.period, case.n) if valid[k] and valid[k - case.period]][-1]
    assert steps[arrival] == (case.depth + 1 if 0 < case.depth < case.period else case.period + 1)
    if case.id == "period9-depth0":
        assert steps[arrival] == F.K_MAX_STEPS
    for k in case.drop:      # the arrival behind a withheld pose: two periods buffered, trimmed to depth + 1
        assert steps[k] == 1 and steps[k + case.period] == case.depth + 1 < 2 * case.period


# ---- launch shapes --------------------------------------------------------------------------------------------------------------
LAUNCH_CASES = ["params-jitter", "period8-depth8", "period6-depth3", "period3-depth8", "period6-depth0", "period9-depth0",
                "period6-depth6-drop12"]


@pytest.mark.parametrize("name", LAUNCH_CASES)
def test_batches_hand_over_and_early_lanes_change_nothing(name, monkeypatch):
    """The property of test_batch_gpu.py::test_batches_equal_single_frames_bit_for_bit at other depths than 6: batch_plan.h's early
    lanes and frame-by-frame hand-over reason about `the twist of pose_frames_between frames ago`.  Batches of 6, of (4, 8, 2) and of
    (5, 2, 7), with ROFT_HANDOFF 0 and 2 and without early lanes, equal the single-frame run in every logged row and in the masks."""
    if name == "params-jitter":
        n, over, descs = N, {}, F.PARAM_SETS
        dts = F.DT_SCHEDULES["jitter_per_object"](N, 3)
        streams = [F.prepared(st, dts[:, o]) for o, st in enumerate(_streams((41, 42, 43)))]
    else:
        case = F.replay_case(name)
        n, over = case.n, dict(pose_frames_between=case.depth)
        plain, descs, _ = _replay_setup(case)
        streams = [F.prepared(st, drop=case.drop) for st in plain]
    dev = [util.to_device(st) for st in streams]
    for var in ("ROFT_HANDOFF", "ROFT_EARLY_LANES"):
        monkeypatch.delenv(var, raising=False)
    ref = _logged(dev, descs, n, T=1, **over)
    assert (ref[0][3] >= 0).sum() >= 4
    for env in (dict(ROFT_HANDOFF="0"), dict(ROFT_HANDOFF="2"), dict(ROFT_EARLY_LANES="0")):
        for var, v in env.items():
            monkeypatch.setenv(var, v)
        for kw in (dict(T=6), dict(splits=(4, 8, 2)), dict(splits=(5, 2, 7))):
            _same(ref, _logged(dev, descs, n, **dict(kw, **over)), (name, env, kw))
        for var in env:
            monkeypatch.delenv(var)


# ---- restart --------------------------------------------------------------------------------------------------------------------
class ParamTrack(R.Track):
    """restart_util.Track whose description carries a parameter set"""

    def __init__(self, F_, st, fields, **kw):
        super().__init__(F_, st, **kw)
        self.fields = fields

    def desc(self):
        return F.engine_desc(self.st, self.fields, self.m0)


def test_restart_with_another_parameter_set(oracle):
    """roft_objects_restart with ROFT_RESTART_KEEP_MESH and a description whose noise differs from the slot's: the slot continues
    like the object of a new engine created with that description (bit for bit) and follows its oracle; the others are untouched."""
    n, at = 26, 8
    A, B, Cs = _streams((41, 42, 43))
    new_track = functools.partial(ParamTrack, st=B, fields=F.PARAM_SETS[2], k0=at, m0=R.gt_mean(B, at), first_mask_gt=True, keep_mesh=True)
    plans = [[ParamTrack(0, A, F.PARAM_SETS[0])], [ParamTrack(0, B, F.PARAM_SETS[1]), new_track(at)], [ParamTrack(0, Cs, F.PARAM_SETS[2])]]
    got = R.run(plans, n)
    assert got["restart_stats"] == dict(calls=1, objects=1, meshes_replaced=0)
    ref = R.oracle_track(oracle, plans[1][1], n - at, **F.oracle_over(F.PARAM_SETS[2]))
    assert R.assert_matches_oracle(got["log"], got["masks"], 1, at, ref) >= 2
    for slot, s in ((0, 0), (2, 2)):
        assert R.assert_matches_oracle(got["log"], got["masks"], slot, 0, R.oracle_track(oracle, plans[slot][0], n, **F.oracle_over(F.PARAM_SETS[s]))) >= 3
    new = R.run([[new_track(0)]], n - at)
    R.assert_same_bits(got, 1, at, new, 0, 0, n - at, "the restarted slot against a new engine with that description")
    plain = R.run([plans[0], plans[1][:1], plans[2]], n)
    R.assert_same_bits(got, 0, 0, plain, 0, 0, n, "slot 0")
    R.assert_same_bits(got, 2, 0, plain, 2, 0, n, "slot 2")
    R.assert_same_bits(got, 1, 0, plain, 1, 0, at, "slot 1 before its restart")
    old = R.oracle_track(oracle, plans[1][0], n, **F.oracle_over(F.PARAM_SETS[1]))
    assert F.trajectory_distance(old[at:], ref) > 100 * POS_TOL     # (the new description is not the old one)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_a_replay_depth_the_frame_program_cannot_hold_is_refused_at_create():
    for depth, want in ((9, L.ERR_INVALID), (8, L.OK), (0, L.OK), (-1, L.OK)):
        cfg = E.default_config(320, 240, max_objects=1)
        cfg.pose_frames_between = depth
        h = C.c_void_p()
        assert L.lib().roft_engine_create(C.byref(cfg), C.byref(h)) == want, depth
        if want == L.OK:
            L.check(L.lib().roft_engine_destroy(h))
        else:
            assert b"pose_frames_between" in L.lib().roft_last_error_string()


@pytest.mark.parametrize("splits", [None, (5, 8, 5)], ids=["one-frame", "batches-5-8-5"])
def test_a_replay_longer_than_the_frame_program_is_refused_and_consumes_nothing(splits):
    """Depth unknown and 12 frames between two poses: the frame that delivers the second would replay 13 twists, the submit returns
    ROFT_ERR_CAPACITY -- here when the first object's frames (and, in the batch, all earlier frames of the second) have been scheduled:
    build_pose_program has by then moved the twist buffer, the belief slot and the feature ring.  The same frames WITHOUT that pose
    then continue bit for bit like an engine that never saw the refused call."""
    n, at = 18, 12
    full = [util.stream(F.REPLAY_SEED, n, 2, pose_period=6, pose_drop_prob=0.0), util.stream(F.REPLAY_SEED + 1, n, 2, pose_period=12, pose_drop_prob=0.0)]
    assert full[1].pose_valid[at] and not full[1].pose_valid[1:at].any()
    held = [full[0], F.prepared(full[1], drop=(at,))]
    descs = [F.PARAM_SETS[0], None]
    dev_full, dev_held = [util.to_device(st) for st in full], [util.to_device(st) for st in held]
    kw = dict(splits=splits) if splits else dict(T=1)
    ref = _logged(dev_held, descs, n, pose_frames_between=0, **kw)
    eng = make_engine(dev_full, descs, max_batch_frames=max(splits) if splits else 1, pose_frames_between=0)
    eng.enable_log(n)
    k = i = refused = 0
    while k < n:
        t = min(splits[i % len(splits)], n - k) if splits else 1
        i += 1
        batch = lambda devs: [[util.device_frame(st, k + j) for st in devs] for j in range(t)]
        if k <= at < k + t:
            arr, keep, T = eng.build_batch(batch(dev_full))
            call = L.lib().roft_frames_submit if splits else (lambda h, a, m, T_: L.lib().roft_frame_submit(h, a, m))
            assert call(eng._h, arr, eng.n_objects, T) == L.ERR_CAPACITY
            assert b"kMaxSteps" in L.lib().roft_last_error_string()
            with pytest.raises(L.RoftError):
                eng.step()                                                      # nothing was submitted
            refused += 1
        eng.submit_batch(batch(dev_held)) if splits else eng.submit(batch(dev_held)[0])
        eng.step()
        k += t
    got = eng.get_log(0, n), [eng.mask(o) for o in range(2)]
    eng.close()
    assert refused == 1
    _same(ref, got, "after the refused submit")


# ---- operators ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ut", F.UT_SETS + [F.UT_BETA_ONLY], ids=lambda u: "ut-%g-%g-%g" % u)
def test_operators_with_other_ut_parameters(oracle, ut):
    """ukf_predict folds the 18 noise columns into column 0 (wm0 + 18 wi), ukf_correct 2 n_add of them; wm0 is 0 at (1, 2, 0) and
    negative here.  Full covariances, anisotropic R and Q; the bars of F.OP_TABLE (1e-9 throughout).  Measured: at most 8.1e-10, on
    the draw correct_pose_velocity-0 at (1, 2, 3) -- the same draw gives 7.4e-10 at (1, 2, 0): its conditioning, not the weights; every
    other case stays below 2.4e-10, the sets with alpha <= 0.1 below 1e-11."""
    Q = oracle.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T)
    assert np.array_equal(ops.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T), Q)
    cases = F.operator_cases()
    worst = {}
    for (u, op), (bar, _, _) in F.OP_TABLE.items():
        if u != ut:
            continue
        for case in [c for c in cases if c[1] == op]:
            rc0, m0, P0 = F.run_operator(oracle, oracle, case, ut, Q)
            rc1, m1, P1 = F.run_operator(ops, L, case, ut, Q)
            assert rc0 == 0 and rc1 == 0, case[0]
            worst[case[0]] = max(np.abs(m1 - m0).max(), np.abs(P1 - P0).max())
    print("ut %s: max |operator - oracle| per case: %s" % (ut, ", ".join("%s %.3g" % kv for kv in worst.items())))
    assert worst
    for name, d in worst.items():
        assert d <= F.OP_TABLE[(ut, name.rsplit("-", 1)[0])][0], (name, d)


def test_operators_with_anisotropic_noise_at_the_default_ut(oracle):
    """The axis order of L.par[12 .. 23] and the R indexing of sigma_delta: every operation at (1, 2, 0) with R and Q anisotropic."""
    Q = oracle.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T)
    worst = {}
    for case in F.operator_cases():
        rc0, m0, P0 = F.run_operator(oracle, oracle, case, F.UT_DEFAULT, Q)
        rc1, m1, P1 = F.run_operator(ops, L, case, F.UT_DEFAULT, Q)
        assert rc0 == 0 and rc1 == 0, case[0]
        worst[case[0]] = max(np.abs(m1 - m0).max(), np.abs(P1 - P0).max())
    print("ut (1, 2, 0): max |operator - oracle| per case: %s" % ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) <= F.UKF_ATOL, worst
