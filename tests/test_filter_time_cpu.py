"""The oracle alone on the cases of tests/filter_time_cases.py (no GPU): every input of tests/test_filter_time_gpu.py is usable -- the
oracle stays finite and never refuses a step -- and able to discriminate: a parameter field rotated by one axis, another object's
set, a jittered or a fallen-back time step, a shallower replay each move the oracle's trajectory by at least 1e-4 = 100 x the 1e-6
within which the engine must follow it (so an engine that got any of them wrong cannot pass), while a replay depth at or above the
pose period, or an unknown one, changes nothing at all (those cases test the engine's trimming, not its arithmetic).  For the
operator cases the file computes the bar the GPU file uses -- max(1e-9, 100 x the distance of the two CPU references) -- and
asserts that every UT parameter set moves the result by at least 1000 bars.  Figures: docs/notebook.md."""
import ctypes as C

import numpy as np
import pytest

import filter_time_cases as F
import util

MARGIN = 1e-4   # 100 x POS_TOL of tests/test_engine_gpu.py
N = 30


def _usable(run):
    return all(np.isfinite(r["pose"]).all() and np.isfinite(r["twist"]).all() and np.isfinite(r["cov"]).all() for r in run)


@pytest.fixture(scope="module")
def st():
    return util.stream(41, N, 2)


@pytest.fixture(scope="module")
def set_runs(oracle, st):
    return [F.run_oracle(oracle, st, N, s) for s in F.PARAM_SETS]


def test_parameter_sets_are_anisotropic_and_differ():
    assert len(F.PARAM_SETS) == 3
    for s in F.PARAM_SETS:
        assert tuple(s) == F.PARAM_FIELDS
        assert len(set(s["p_cov0_diag"])) == 12
        for name, v in s.items():
            g = 3 if len(v) % 3 == 0 else len(v)
            for k in range(0, len(v), g):
                w = sorted(v[k:k + g])
                assert all(b / a >= 9.999 for a, b in zip(w, w[1:])), (name, v)
    for name in F.PARAM_FIELDS:   # no two sets order a field's axes alike
        orders = [tuple(np.argsort(s[name][:3 if len(s[name]) % 3 == 0 else 2])) for s in F.PARAM_SETS]
        assert len(set(orders)) == (3 if len(orders[0]) == 3 else 2), name


@pytest.mark.parametrize("si", range(3))
def test_every_field_rotated_by_one_axis_moves_the_trajectory(oracle, st, set_runs, si):
    assert _usable(set_runs[si])
    least = {}
    for name in F.PARAM_FIELDS:
        r = F.run_oracle(oracle, st, N, F.rotated(F.PARAM_SETS[si], name))
        assert _usable(r), name
        least[name] = F.trajectory_distance(set_runs[si], r)
    print("set %d, rotated field -> distance: %s" % (si, ", ".join("%s %.3g" % kv for kv in least.items())))
    assert min(least.values()) >= MARGIN, least


def test_sets_swapped_between_objects_move_the_trajectory(set_runs):
    d = {(i, j): F.trajectory_distance(set_runs[i], set_runs[j]) for i in range(3) for j in range(i + 1, 3)}
    print("set against set on one stream:", d)
    assert min(d.values()) >= MARGIN


def test_time_step_schedules_move_the_trajectory(oracle, st, set_runs):
    assert list(F.DT_SCHEDULES) == ["constant", "jitter", "jitter_per_object", "fallback"]
    const = F.DT_SCHEDULES["constant"](N, 3)
    assert np.array_equal(const, np.full((N, 3), st.dt))
    jit, per = F.DT_SCHEDULES["jitter"](N, 3), F.DT_SCHEDULES["jitter_per_object"](N, 3)
    assert np.array_equal(jit[:, 0], jit[:, 2]) and np.abs(jit / F.DT0 - 1).max() <= 0.3 and np.abs(jit / F.DT0 - 1).max() > 0.2
    assert np.abs(per[:, 0] - per[:, 1]).max() > 0.1 * F.DT0 and np.abs(per[:, 1] - per[:, 2]).max() > 0.1 * F.DT0
    fb = F.DT_SCHEDULES["fallback"](N, 3)
    assert set(fb[::2].ravel()) == {0.0} and set(fb[1::2].ravel()) == {-1.0}
    assert np.array_equal(F.oracle_dt(fb, F.FALLBACK_SAMPLE_TIME), np.full((N, 3), 0.04))
    for name in ("jitter", "jitter_per_object", "fallback"):
        over = F.DT_CONFIG[name]
        dts = F.oracle_dt(F.DT_SCHEDULES[name](N, 3), over.get("sample_time", F.DT0))
        d = []
        for o in range(3):
            r = F.run_oracle(oracle, st, N, F.PARAM_SETS[o], dts[:, o], **over)
            assert _usable(r), (name, o)
            d.append(F.trajectory_distance(set_runs[o], r))
        print("dt %s against constant 1/30, per object: %s" % (name, ["%.3g" % x for x in d]))
        assert min(d) >= MARGIN, (name, d)
    a = F.run_oracle(oracle, st, N, F.PARAM_SETS[0], per[:, 0])
    b = F.run_oracle(oracle, st, N, F.PARAM_SETS[0], per[:, 1])
    assert F.trajectory_distance(a, b) >= MARGIN   # (an object fed another object's time steps)


@pytest.mark.parametrize("case", F.REPLAY_CASES, ids=lambda c: c.id)
def test_replay_depth_cases(oracle, case):
    s = F.replay_stream(case)
    assert [k for k in range(case.n) if s.pose_valid[k]] == [k for k in range(0, case.n, case.period) if k not in case.drop]
    for fields in (None, F.PARAM_SETS[1]):
        r = F.run_oracle(oracle, s, case.n, fields, pose_frames_between=case.depth)
        e = F.run_oracle(oracle, s, case.n, fields, pose_frames_between=case.period)
        assert _usable(r)
        assert max(np.abs(x["pose"][6:9] - s.gt.x[k]).max() for k, x in enumerate(r)) < 0.08   # it keeps tracking
        d = F.trajectory_distance(r, e)
        print("%s (%s), %s parameters: distance to depth == period %.3g" % (case.id, case.kind, "default" if fields is None else "set 1", d))
        if case.kind == "below":
            assert d >= MARGIN
        else:
            assert d == 0.0 and all(np.array_equal(x["pose"], y["pose"]) and np.array_equal(x["cov"], y["cov"]) for x, y in zip(r, e))
        # corrections of a pose arrival in the steady state: the replayed twists, + 1 for the second alternative of the outlier test
        buffered = case.period + 1 if case.kind != "below" else case.depth + 1
        arrivals = [k for k in range(case.period, case.n) if s.pose_valid[k] and s.pose_valid[k - case.period]]
        assert arrivals and all(r[k]["nc"] == buffered + 1 for k in arrivals), [x["nc"] for x in r]
        for k in case.drop:   # the arrival after a withheld pose: twice the period buffered, trimmed to depth + 1
            assert r[k]["nc"] == 1 and r[k + case.period]["nc"] == min(2 * case.period, case.depth) + 2
        # ... and the engine's frame programs (host logic: roft_debug_plan) hold as many
        from roft_amd import _lib as L
        cfg = L.Config()
        L.check(L.lib().roft_default_config(C.byref(cfg), 640, 480, L.FLOW_F32C2))
        cfg.pose_frames_between = case.depth
        plan = F.debug_plan(cfg, s.pose_valid[:case.n])
        assert not isinstance(plan, int) and plan[1] == [x["nc"] for x in r]
    if case.id == "period9-depth0":
        assert max(plan[0]) == F.K_MAX_STEPS      # the boundary: exactly as many steps as a frame program holds


def test_the_refusals_of_the_host_logic():
    """roft_debug_plan: one more buffered twist than the boundary case is refused with ROFT_ERR_CAPACITY"""
    from roft_amd import _lib as L
    cfg = L.Config()
    L.check(L.lib().roft_default_config(C.byref(cfg), 640, 480, L.FLOW_F32C2))
    cfg.pose_frames_between = 0
    assert F.debug_plan(cfg, [k % 10 == 0 for k in range(11)]) == L.ERR_CAPACITY
    assert F.debug_plan(cfg, [k % 12 == 0 for k in range(13)]) == L.ERR_CAPACITY
    assert not isinstance(F.debug_plan(cfg, [k % 9 == 0 for k in range(19)]), int)


def test_operator_bars_and_the_effect_of_the_ut_parameters(oracle):
    """floor = max |oracle - ukf_numpy|, bar = max(UKF_ATOL, 100 floor), effect = max |oracle(ut) - oracle(1, 2, 0)|: the bars of
    F.OP_TABLE are the ones computed here, and every (UT set, operation) pair of the table moves the result by >= 1000 bars.
    Pairs the references cannot hold to that are not in the table (see its comment)."""
    import ukf_numpy as U
    cases = F.operator_cases()
    Q = oracle.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T)
    assert np.array_equal(Q, U.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T)) or np.allclose(Q, U.process_noise(F.OP_PSD, F.OP_SIGMA_ANG, F.OP_T), rtol=1e-15, atol=0)

    def numpy_side(case, ut):
        _, op, mean, P, meas, rd = case
        if op == "predict":
            return U.predict(mean, P, Q, F.OP_T, ut=ut)
        return U.correct(mean, P, {"correct_velocity": U.VELOCITY, "correct_pose": U.POSE, "correct_pose_velocity": U.POSE_VELOCITY}[op], meas, rd, ut=ut)

    default = {}
    for case in cases:
        rc, m, P = F.run_operator(oracle, oracle, case, F.UT_DEFAULT, Q)
        assert rc == 0
        default[case[0]] = (m, P)
        assert F.belief_distance(m, P, *numpy_side(case, F.UT_DEFAULT)) < 1e-11     # the anisotropic R and Q alone
    computed = {}
    for ut in F.UT_SETS + [F.UT_BETA_ONLY]:
        for op in F.OPERATIONS:
            floor, effect = 0.0, np.inf
            for case in [c for c in cases if c[1] == op]:
                rc, m, P = F.run_operator(oracle, oracle, case, ut, Q)
                assert rc == 0 and np.isfinite(m).all() and np.isfinite(P).all()
                floor = max(floor, F.belief_distance(m, P, *numpy_side(case, ut)))
                effect = min(effect, F.belief_distance(m, P, *default[case[0]]))
            computed[(ut, op)] = (max(F.UKF_ATOL, 100.0 * floor), floor, effect)
            print("ut %s %-22s floor %.2g effect %.3g" % (ut, op, floor, effect))
    wanted = [k for k in computed if k[1] != "correct_pose" and (k[0] != F.UT_BETA_ONLY or k[1] == "correct_velocity")]
    assert sorted(F.OP_TABLE) == sorted(wanted)
    # what is left out cannot discriminate: a pose correction is the same whatever the UT set, beta alone moves a prediction by < 1e-6
    assert all(computed[(ut, "correct_pose")][2] < 1e-10 for ut in F.UT_SETS + [F.UT_BETA_ONLY])
    assert computed[(F.UT_BETA_ONLY, "predict")][2] < 1000.0 * F.UKF_ATOL
    for key, (bar, floor, effect) in F.OP_TABLE.items():
        bar_now, floor_now, effect_now = computed[key]
        assert bar == bar_now == F.UKF_ATOL, (key, floor_now)          # floors of at most 1e-11: the bar stays 1e-9 for every pair
        assert floor_now <= 1e-11 and floor <= 1e-11
        assert effect_now >= 1000.0 * bar, (key, effect_now)
        assert 0.5 * effect <= effect_now <= 2.0 * effect, (key, effect_now, effect)   # the table's figures are the measured ones
