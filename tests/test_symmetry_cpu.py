"""Symmetric objects without a GPU (include/roft_engine.h section 3h): roft_pose_nearest_equivalent -- host arithmetic -- bit for bit
against the numpy restatement tests/symmetry_ref.py; every refusal of the new entry points that is made before a device is looked
for; the reader of BOP's models_info.json; and, with the oracle alone, the condition tests/test_symmetry_gpu.py rests on."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import io as rio
from roft_amd import metrics, ops

import symmetry_ref as S
import util

INVALID, STATE = L.ERR_INVALID, L.ERR_STATE


def _unit(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _group_with_translation():
    return np.array([S.IDENTITY, S.half_turn(2, (0.01, -0.02, 0.03)), S.half_turn(0, (0.0, 0.015, -0.01))])


def _same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


@pytest.mark.parametrize("name,group", [("one", np.array([S.IDENTITY])), ("two", np.array([S.IDENTITY, S.half_turn(1)])),
                                        ("d2", S.d2_group()), ("cap", S.cyclic_group(L.MAX_SYMMETRIES)),
                                        ("translation", _group_with_translation())])
def test_nearest_equivalent_is_the_restatement_bit_for_bit(name, group):
    rng = np.random.default_rng(len(group) * 31 + len(name))
    seen = set()
    for trial in range(200):
        qh, x = _unit(rng), rng.normal(size=3)
        # a measurement near an equivalent of the belief, in either hemisphere, sometimes anywhere
        g = int(rng.integers(len(group)))
        m = np.array(S.quat_mul(S.quat_mul(qh, group[g, 3:]), _unit(rng) * 0.05 + np.array([1.0, 0, 0, 0])))
        m = m / np.linalg.norm(m) * (1.0 if trial % 2 else -1.0)
        if trial % 7 == 0:
            m = _unit(rng) * 1.3   # (used as given, not normalised)
        xr, qr, gr = S.nearest_equivalent(group, qh, x, m)
        xo, qo, go = ops.pose_nearest_equivalent(group, qh, x, m)
        assert go == gr, (name, trial)
        assert _same_bits(xo, xr) and _same_bits(qo, qr), (name, trial, xo - xr, qo - qr)
        seen.add(go)
    assert seen == set(range(len(group))), "every element is chosen at least once"


def test_identity_returns_the_input_bits_and_stays_in_its_hemisphere():
    group = S.d2_group()
    qh = np.array([0.9, 0.1, -0.3, 0.2])
    qh /= np.linalg.norm(qh)
    m = -(qh + np.array([0.0, 0.01, 0.0, -0.01]))   # close to qh's pose, opposite hemisphere, not of unit length
    x = np.array([0.1, -0.2, 0.7])
    xo, qo, g = ops.pose_nearest_equivalent(group, qh, x, m)
    assert g == 0 and _same_bits(xo, x) and _same_bits(qo, m)
    assert S.quat_dot(qh, qo) < 0.0, "the identity applies no sign change"


def test_a_non_identity_choice_in_the_opposite_hemisphere_is_negated():
    group = _group_with_translation()
    qh = np.array([0.7, -0.2, 0.5, 0.1])
    qh /= np.linalg.norm(qh)
    x = np.array([0.05, 0.02, 0.6])
    for g in (1, 2):
        for sign in (1.0, -1.0):
            # the belief's pose flipped by g: the rule must undo it with g (a half turn is its own inverse, up to the sign of q)
            m = sign * np.array(S.quat_mul(qh, group[g, 3:]))
            xo, qo, go = ops.pose_nearest_equivalent(group, qh, x, m)
            xr, qr, gr = S.nearest_equivalent(group, qh, x, m)
            assert go == gr == g
            assert _same_bits(xo, xr) and _same_bits(qo, qr)
            assert S.quat_dot(qh, qo) > 0.99, "m' is in qh's hemisphere"
            p = S.quat_mul(m, group[g, 3:])
            assert _same_bits(qo, [-v for v in p]) == (S.quat_dot(qh, p) < 0.0)
            assert np.abs(xo - x).max() > 1e-3, "the element's translation moved the position"
    negated = [S.quat_dot(qh, S.quat_mul(s * np.array(S.quat_mul(qh, group[1, 3:])), group[1, 3:])) < 0 for s in (1.0, -1.0)]
    assert sorted(negated) == [False, True], "one of the two signs takes the negation"


def test_an_exact_tie_goes_to_the_lower_index():
    # qh = identity, m = a quarter turn about z: under {e, half turn about z} both elements give |qh . p| = cos(45 deg) from the
    # SAME two products (w = c * 1 for e, -(s * -1)... = s for g), and c == s is made exact by using one number for both
    c = math.sqrt(0.5)
    group = np.array([S.IDENTITY, S.half_turn(2), S.half_turn(2)])
    qh, m, x = np.array([1.0, 0, 0, 0]), np.array([c, 0.0, 0.0, c]), np.zeros(3)
    cs = S.closeness(group, qh, m)
    assert cs[0] == cs[1] == cs[2], cs
    xo, qo, g = ops.pose_nearest_equivalent(group, qh, x, m)
    assert g == 0 and _same_bits(qo, m)
    # the tie between two non-identity elements that beat the identity: the lower of the two
    m2 = np.array([0.0, 0.0, 0.0, 1.0])
    xo, qo, g = ops.pose_nearest_equivalent(group, qh, x, m2)
    assert g == 1 == S.nearest_equivalent(group, qh, x, m2)[2]


def _rc(call, *args):
    rc = call(*args)
    return rc, L.lib().roft_last_error_string().decode()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bad_groups(cap):
    ok = S.d2_group()
    not_identity = ok.copy()
    not_identity[0, 3] = 1.0 - 1e-16
    moved_identity = ok.copy()
    moved_identity[0, 0] = 1e-300
    nan = ok.copy()
    nan[2, 1] = np.nan
    inf = ok.copy()
    inf[1, 4] = np.inf
    long_q = ok.copy()
    long_q[3, 3:] *= 1.0 + 1e-6
    too_many = np.tile(np.array(S.IDENTITY), (cap + 1, 1))
    return [("not the identity", not_identity, 4), ("translated identity", moved_identity, 4), ("nan", nan, 4), ("inf", inf, 4),
            ("not of unit length", long_q, 4), ("more than the cap", too_many, cap + 1), ("no element", ok, 0), ("negative count", ok, -1)]


def test_refusals_are_made_without_a_device():
    lib = L.lib()
    ok = S.d2_group()
    v3, v4, o3, o4 = np.zeros(3), np.array([1.0, 0, 0, 0]), np.zeros(3), np.zeros(4)
    pts, poses, out = np.zeros((5, 3)), np.tile(np.array(S.IDENTITY), (2, 1)), np.zeros(2)
    cam = L.Camera(160, 120, 150.0, 150.0, 80.0, 60.0)
    # the selection operator
    for what, g, n in bad_groups(L.MAX_SYMMETRIES):
        rc, why = _rc(lib.roft_pose_nearest_equivalent, _ptr(g), n, _ptr(v4), _ptr(v3), _ptr(v4), _ptr(o3), _ptr(o4), None)
        assert rc == INVALID and "symmetry group" in why, (what, rc, why)
    assert lib.roft_pose_nearest_equivalent(None, 4, _ptr(v4), _ptr(v3), _ptr(v4), _ptr(o3), _ptr(o4), None) == INVALID
    for hole in range(2, 7):
        args = [_ptr(ok), 4, _ptr(v4), _ptr(v3), _ptr(v4), _ptr(o3), _ptr(o4), None]
        args[hole] = None
        assert lib.roft_pose_nearest_equivalent(*args) == INVALID, hole
    assert lib.roft_pose_nearest_equivalent(_ptr(ok), 4, _ptr(v4), _ptr(v3), _ptr(v4), _ptr(o3), _ptr(o4), None) == L.OK   # (index_out may be NULL)
    # scoring: its own cap, the kinds, the camera; every refusal comes before the device (there is none here, and OK for n_poses == 0)
    for what, g, n in bad_groups(L.MAX_SCORE_SYMMETRIES):
        rc, why = _rc(lib.roft_pose_errors_sym, L.POSE_ERROR_MSSD, _ptr(pts), 5, _ptr(poses), _ptr(poses), 2, _ptr(g), n, None, _ptr(out))
        assert rc == INVALID and "symmetry group" in why, (what, rc, why)
    many = S.cyclic_group(L.MAX_SYMMETRIES + 1)   # more than the filter takes, fine for scoring
    assert lib.roft_pose_errors_sym(L.POSE_ERROR_MSSD, _ptr(pts), 5, _ptr(poses), _ptr(poses), 0, _ptr(many), len(many), None, _ptr(out)) == L.OK
    assert lib.roft_pose_nearest_equivalent(_ptr(many), len(many), _ptr(v4), _ptr(v3), _ptr(v4), _ptr(o3), _ptr(o4), None) == INVALID
    for kind in (L.POSE_ERROR_ADD, L.POSE_ERROR_ADDS, 4, -1):
        rc, why = _rc(lib.roft_pose_errors_sym, kind, _ptr(pts), 5, _ptr(poses), _ptr(poses), 2, _ptr(ok), 4, C.byref(cam), _ptr(out))
        assert rc == INVALID and "kind" in why, kind
    rc, why = _rc(lib.roft_pose_errors_sym, L.POSE_ERROR_MSPD, _ptr(pts), 5, _ptr(poses), _ptr(poses), 2, _ptr(ok), 4, None, _ptr(out))
    assert rc == INVALID and "camera" in why
    for hole in (1, 3, 4, 6, 9):
        args = [L.POSE_ERROR_MSSD, _ptr(pts), 5, _ptr(poses), _ptr(poses), 2, _ptr(ok), 4, C.byref(cam), _ptr(out)]
        args[hole] = None
        assert lib.roft_pose_errors_sym(*args) == INVALID, hole
    assert lib.roft_pose_errors_sym(L.POSE_ERROR_MSSD, _ptr(pts), 0, _ptr(poses), _ptr(poses), 2, _ptr(ok), 4, None, _ptr(out)) == INVALID
    assert lib.roft_pose_errors_sym(L.POSE_ERROR_MSSD, _ptr(pts), 5, _ptr(poses), _ptr(poses), -1, _ptr(ok), 4, None, _ptr(out)) == INVALID
    assert lib.roft_pose_errors_sym(L.POSE_ERROR_MSPD, _ptr(pts), 5, _ptr(poses), _ptr(poses), 0, _ptr(ok), 4, C.byref(cam), _ptr(out)) == L.OK
    # the engine's entry points with a NULL engine
    rc, why = _rc(lib.roft_object_set_symmetry, None, 0, _ptr(ok), 4)
    assert rc == INVALID and "engine" in why
    rc, why = _rc(lib.roft_engine_score_log_sym, None, L.POSE_ERROR_MSSD, 0, 0, 1, None, 0, _ptr(poses), _ptr(ok), 4, _ptr(out))
    assert rc == INVALID and "engine" in why


def test_read_bop_symmetries():
    path = os.path.join(util.GOLDEN, "models_info_small.json")
    none = rio.read_bop_symmetries(path, 1)
    assert none.shape == (1, 7) and none.tolist() == [list(S.IDENTITY)]
    two = rio.read_bop_symmetries(path, 2, unit_scale=0.001)
    assert two.shape == (3, 7) and two[0].tolist() == list(S.IDENTITY), "the identity is prepended"
    np.testing.assert_allclose(two[1], [0.02, -0.03, 0.0, 0.0, 0.0, 0.0, 1.0], atol=1e-15)   # half turn about z, millimetres scaled
    np.testing.assert_allclose(two[2], [0.0, 0.0, 0.005, 0.0, 1.0, 0.0, 0.0], atol=1e-15)    # half turn about x
    assert rio.read_bop_symmetries(path, 2, unit_scale=1.0)[1, 0] == 20.0
    # what was read is a group the library accepts
    xo, qo, g = ops.pose_nearest_equivalent(two, [1.0, 0, 0, 0], [0.0, 0, 0], [0.0, 0.0, 0.0, 1.0])
    assert g == 1
    with pytest.raises(ValueError, match="discretise_axis"):
        rio.read_bop_symmetries(path, 3)
    with pytest.raises(KeyError):
        rio.read_bop_symmetries(path, 4)
    ring = rio.discretise_axis([0, 0, 1], [0.01, 0.0, 0.0], 8)
    assert ring.shape == (8, 7) and ring[0].tolist() == list(S.IDENTITY)
    np.testing.assert_allclose(ring[4], [0.02, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0], atol=1e-15)   # the half turn about z through (0.01, 0, 0)
    ops.pose_nearest_equivalent(ring, [1.0, 0, 0, 0], [0.0, 0, 0], [1.0, 0.0, 0.0, 0.0])


def test_numpy_scores_of_the_package_are_the_restatement():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-0.1, 0.1, (40, 3))
    group = _group_with_translation()
    est = np.concatenate([rng.normal(0, 0.1, (3, 3)) + [0, 0, 0.8], np.array([_unit(rng) for _ in range(3)])], 1)
    ref = np.concatenate([rng.normal(0, 0.1, (3, 3)) + [0, 0, 0.8], np.array([_unit(rng) for _ in range(3)])], 1)
    cam = (150.0, 151.0, 80.0, 60.0)
    assert _same_bits(metrics.trajectory_mssd(est, ref, pts, group), S.pose_errors_sym("mssd", pts, est, ref, group))
    assert _same_bits(metrics.trajectory_mspd(est, ref, pts, cam, group), S.pose_errors_sym("mspd", pts, est, ref, group, cam))
    # a flipped estimate scores like the unflipped one under the group, and much worse without it
    x, q = S.flip_pose(ref[0, :3], ref[0, 3:], group[1])
    flipped = np.concatenate([x, q])[None]
    assert metrics.trajectory_mssd(flipped, ref[:1], pts, group)[0] < 1e-12
    assert metrics.trajectory_mssd(flipped, ref[:1], pts)[0] > 0.05


def _rot_angle(qa, qb):
    return 2.0 * math.acos(min(1.0, abs(float(np.dot(qa, qb)))))


def test_the_setting_of_the_gpu_test_discriminates_and_is_never_close_to_a_tie(oracle):
    """With the oracle alone: at every delivery of the GPU test's streams the best element (qh = the clean oracle's estimate of the
    frame before) undoes the flip with a margin of at least 0.05 to the second best; the oracle fed the flipped poses without a
    remedy leaves the clean one by more than 0.5 rad; and the oracle fed NEGATED quaternions moves by what the assertion message
    records (6.66e-8 when this was written, the smallest margin 0.828: docs/notebook.md) -- the hemisphere rule leans on that being
    inside the parity bar, 1e-6."""
    streams, groups = S.streams(), S.groups()
    worst_margin, worst_negation = np.inf, 0.0
    for o in (0, 1):
        st, group = streams[o], groups[o]
        clean = S.run_oracle(oracle, st)
        fl, used = S.flipped(st, group, seed=900 + o)
        assert set(used.values()) == set(range(len(group))), "every element is used, the identity included"
        p0 = S.initial_pose(st)
        for k, g in used.items():
            qh = p0[9:13] if k == 0 else clean[k - 1]["pose"][9:13]
            c = S.closeness(group, qh, fl.pose_meas[k, 3:])
            order = np.argsort(c)
            best, second = int(order[-1]), int(order[-2])
            worst_margin = min(worst_margin, c[best] - c[second])
            assert c[best] - c[second] >= 0.05, (o, k, c)
            # the best element undoes the flip: flipped (x) best is the clean measurement again, up to rounding and sign
            x, q, chosen = S.nearest_equivalent(group, qh, fl.pose_meas[k, :3], fl.pose_meas[k, 3:])
            assert chosen == best
            assert _rot_angle(q, st.pose_meas[k, 3:]) < 1e-7 and np.abs(x - st.pose_meas[k, :3]).max() < 1e-12, (o, k)
        # ... and the library's operator takes the same decisions and returns the same bits on these inputs
        rem_ref, chosen_ref = S.remedied(fl, group, clean, p0)(S.nearest_equivalent)
        rem_lib, chosen_lib = S.remedied(fl, group, clean, p0)(ops.pose_nearest_equivalent)
        assert chosen_ref == chosen_lib and _same_bits(rem_ref.pose_meas, rem_lib.pose_meas)
        broken = S.run_oracle(oracle, st, fed=fl)
        assert max(_rot_angle(broken[k]["pose"][9:], clean[k]["pose"][9:]) for k in range(S.N_FRAMES)) > 0.5, \
            "without a remedy the flipped deliveries take the oracle away from the clean trajectory"
        neg = copy.copy(st)   # the clean stream with every delivered quaternion negated
        neg.pose_meas = st.pose_meas.copy()
        neg.pose_meas[:, 3:] = -st.pose_meas[:, 3:]
        moved = S.run_oracle(oracle, st, fed=neg)
        for k in range(S.N_FRAMES):
            worst_negation = max(worst_negation, float(np.abs(moved[k]["pose"][:9] - clean[k]["pose"][:9]).max()),
                                 _rot_angle(moved[k]["pose"][9:], clean[k]["pose"][9:]), float(np.abs(moved[k]["twist"] - clean[k]["twist"]).max()))
    print("smallest margin %.3f, largest move of the oracle under negated measurements %.3g" % (worst_margin, worst_negation))
    assert worst_negation < 1e-6, "the oracle moves by %.3g when measurements are replaced by their negated quaternions" % worst_negation
