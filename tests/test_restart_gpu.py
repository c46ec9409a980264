"""roft_objects_restart on the GPU (include/roft_engine.h, "restart object slots on a running engine").  The contract is an
equivalence: from the engine's next frame on a restarted slot returns, bit for bit, what the same slot of a NEW engine returns
from its first frame on, and every other slot returns what it returns without the call.  So every test runs engines fed from one
description of the tracks (restart_util.Track) and asks for EQUAL bytes -- log records (pose, twist, point count, decision,
likelihoods), masks, and where they exist quality records, produced flows and depths; the oracle comparisons use the bars of
tests/test_engine_gpu.py on a fresh oracle tracker per track, whose windows hold at least two outlier tests (asserted; the seeds were
picked on the CPU so that the oracle alone meets this).

Shapes: util.stream(seed, n, scale=2) is 320 x 240 with box meshes."""
import numpy as np
import pytest

from roft_amd import _lib as L

import restart_util as R
import util

pytestmark = pytest.mark.gpu

B_HALF = (0.05, 0.08, 0.03)   # stream B: another box, another tessellation


def _A(n=14):
    return util.stream(2100, n, scale=2)


def _B():
    return util.stream(2101, 14, scale=2, half_extents=B_HALF, mesh_n=8)


def _C(n=28):
    return util.stream(2104, n, scale=2)


def _S():
    return util.stream(2202, 26, scale=2)   # (its oracle takes the velocity-only alternative once inside the windows below)


def _reacquire(st, F, at=None, **kw):
    """the track that starts at stream frame F from the ground truth of that frame, with that frame's mask; at: its engine frame"""
    return R.Track(F if at is None else at, st, k0=F, m0=R.gt_mean(st, F), first_mask_gt=True, **kw)


@pytest.fixture(scope="module")
def ob(oracle):
    return oracle


# ---- 1. slot reuse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [None, [4, 4, 4, 2]], ids=["one-frame", "batches-4-4-4-2"])
def test_slot_reuse(ob, splits):
    A, B, C = _A(), _B(), _C()
    assert B.mesh[0].shape != A.mesh[0].shape and B.half_extents != A.half_extents
    seen = {}

    def after_restart(eng, f):
        # until the slot's next step: the old track's last row, and no mask to read -- as on a new engine
        seen["outs"] = np.array(eng.outputs()[0].pose[:])
        seen["last_row"] = eng.get_log_rows(f - 1, 1)[0, 0, :13]
        with pytest.raises(L.RoftError):
            eng.mask(0)
        seen["mask_error"] = L.lib().roft_last_error_string()
        assert eng.mask(1).any()

    def finish(eng, got):
        # roft_engine_score_log without points scores with the slot's CURRENT mesh
        ref = np.concatenate([B.gt.x[:14], B.gt.q[:14]], axis=1)
        seen["add"] = [eng.score_log("add", 0, 14, 14, ref, points=pts) for pts in (None, B.mesh[0].astype(np.float64), A.mesh[0].astype(np.float64))]

    plans = [[R.Track(0, A), R.Track(14, B)], [R.Track(0, C)]]
    got = R.run(plans, 28, splits, after_restart=after_restart, finish=finish)
    assert np.array_equal(seen["add"][0], seen["add"][1]) and not np.array_equal(seen["add"][0], seen["add"][2])
    assert got["restart_stats"] == dict(calls=1, objects=1, meshes_replaced=1)
    assert np.array_equal(seen["outs"], seen["last_row"]) and b"no stepped frame" in seen["mask_error"]
    ref = R.oracle_track(ob, plans[0][1], 14)
    assert R.assert_matches_oracle(got["log"], got["masks"], 0, 14, ref) >= 2
    new = R.run([[R.Track(0, B)], [R.Track(0, B)]], 14, splits)
    R.assert_same_bits(got, 0, 14, new, 0, 0, 14, "slot 0 on B against a new engine")
    plain = R.run([[R.Track(0, _A(28))], [R.Track(0, C)]], 28, splits)
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 28, "slot 1 against the run without the call")


# ---- 2. re-acquisition inside one sequence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [7, 8])
def test_reacquisition_inside_a_sequence(ob, F):
    """F = 7 and 8: both batch parities of the mask tables.  The stream's flow is handed at F (and must be unused); the delayed
    poses that follow carry content older than F."""
    S, C = _S(), _C()
    assert S.flow_valid[F] and S.pose_valid[12] and S.mask_delivery[F] < 0
    plans = [[R.Track(0, S), _reacquire(S, F)], [R.Track(0, C)]]
    got = R.run(plans, 26)
    ref = R.oracle_track(ob, plans[0][1], 26 - F)
    assert R.assert_matches_oracle(got["log"], got["masks"], 0, F, ref) >= 2
    new = R.run([[_reacquire(S, F, at=0)], [_reacquire(S, F, at=0)]], 26 - F)
    R.assert_same_bits(got, 0, F, new, 0, 0, 26 - F, "restarted slot against a new engine")
    plain = R.run([[R.Track(0, S)], [R.Track(0, C)]], 26)
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 26, "the other slot")
    R.assert_same_bits(got, 0, 0, plain, 0, 0, F, "the slot before its restart")


# ---- 3. past the rings --------------------------------------------------------------------------------------------------------
def test_restarts_past_the_rings():
    """80 frames, restarts at 33 and 70 -- the second past kPlaneSlots and kTwistRing (64), both past several turns of kFeatRing --
    with batches in flight when the call comes (no mask is read on the way)."""
    X, Y, Z, W = util.stream(2300, 33, scale=2), util.stream(2301, 47, scale=2), util.stream(2302, 70, scale=2), util.stream(2303, 10, scale=2)
    plans = [[R.Track(0, X), R.Track(33, Y)], [R.Track(0, Z), R.Track(70, W)]]
    got = R.run(plans, 80, read_masks=False)
    assert got["restart_stats"] == dict(calls=2, objects=2, meshes_replaced=2)
    new_y = R.run([[R.Track(0, Y)], [R.Track(0, Y)]], 47, read_masks=False)
    R.assert_same_bits(got, 0, 33, new_y, 0, 0, 47, "slot 0 from frame 33")
    new_w = R.run([[R.Track(0, W)], [R.Track(0, W)]], 10, read_masks=False)
    R.assert_same_bits(got, 1, 70, new_w, 1, 0, 10, "slot 1 from frame 70")
    plain = R.run([[R.Track(0, Z)], [R.Track(0, Z)]], 70, read_masks=False)
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 70, "slot 1 before its restart", need_mask=False)
    assert sum(1 for f in range(33, 80) if got["log"][f][0][3] >= 0) >= 2 and sum(1 for f in range(70, 80) if got["log"][f][1][3] >= 0) >= 1


# ---- 4. with everything on ----------------------------------------------------------------------------------------------------
def test_restart_with_log_quality_pose_masks_and_occlusion():
    """(a) quality (every = 2), pose masks and occlusion in one scene, no mask delivered: the restarted slot's first mask is the
    silhouette of its new p_mean0 (frame 14 brings no pose), later ones those of the delivered poses."""
    A, C = _A(28), _C()
    F = 14
    assert not A.pose_valid[F] and not C.pose_valid[F]

    def setup(eng):
        eng.enable_quality(every=2)
        eng.enable_pose_masks()
        eng.enable_pose_mask_occlusion()

    def runq(plans, n):
        def fin(eng, got):
            got["quality"] = eng.quality(0, n)
            got["pm"] = eng.pose_mask_stats()
        return R.run(plans, n, mode="nomask", setup=setup, finish=fin)

    restarted = R.Track(F, A, k0=F, m0=R.gt_mean(A, F))
    got = runq([[R.Track(0, A), restarted], [R.Track(0, C)]], 28)
    new = runq([[R.Track(0, A, k0=F, m0=R.gt_mean(A, F))], [R.Track(0, C, k0=F, first_mask_gt=True)]], 28 - F)
    plain = runq([[R.Track(0, A)], [R.Track(0, C)]], 28)
    assert got["pm"]["silhouettes"] == plain["pm"]["silhouettes"] + 1   # the one of the new p_mean0
    R.assert_same_bits(got, 0, F, new, 0, 0, 28 - F, "restarted slot against a new engine")
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 28, "the other slot")
    fields = [n for n in got["quality"].dtype.names if n != "frame"]
    compared = 0
    for k in range(28 - F):
        a, b = got["quality"][F + k, 0], new["quality"][k, 0]
        if a["frame"] >= 0 and b["frame"] >= 0:
            assert a["frame"] == F + k and b["frame"] == k     # records keep the engine's frame numbering
            assert all(a[n].tobytes() == b[n].tobytes() for n in fields), (k, a, b)
            compared += 1
    assert compared == (28 - F) // 2
    assert got["quality"][:, 1].tobytes() == plain["quality"][:, 1].tobytes()
    assert got["quality"][:F, 0].tobytes() == plain["quality"][:F, 0].tobytes()   # records of earlier frames stay readable


def test_restart_with_camera_images_raw_depth_and_label_masks():
    """(b) a shared scene: both slots name ONE camera image, raw depth frame and label image per frame.  The restarted slot's flow
    starts over (none at F); the other slot still takes its flow from the shared pair (F - 1, F)."""
    G = util.stream(2400, 22, scale=2, with_gray=True)
    F = 9

    def setup(eng):
        eng.enable_flow()
        eng.enable_raw_depth(R.RAW_SCALE)

    def per_step(eng, f, got):
        for slot in range(2):
            try:
                flow = eng.produced_flow(slot).tobytes()
            except L.RoftError:
                flow = None
            got["extra"][(f, slot)] = (flow, eng.depth(slot).tobytes())

    def runi(plans, n):
        return R.run(plans, n, mode="images", setup=setup, per_step=per_step)

    got = runi([[R.Track(0, G), _reacquire(G, F)], [R.Track(0, G)]], 22)
    new = runi([[_reacquire(G, F, at=0)], [_reacquire(G, F, at=0)]], 22 - F)
    plain = runi([[R.Track(0, G)], [R.Track(0, G)]], 22)
    R.assert_same_bits(got, 0, F, new, 0, 0, 22 - F, "restarted slot against a new engine")
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 22, "the other slot")
    assert got["extra"][(F, 0)][0] is None and got["extra"][(F, 1)][0] is not None and got["extra"][(F + 1, 0)][0] is not None
    for k in range(22 - F):
        assert got["extra"][(F + k, 0)] == new["extra"][(k, 0)], k
    for f in range(22):
        assert got["extra"][(f, 1)] == plain["extra"][(f, 1)], f
    assert sum(1 for f in range(F, 22) if got["log"][f][0][3] >= 0) >= 2


# ---- 5. variants and refusals -------------------------------------------------------------------------------------------------
def test_keep_mesh_equals_handing_the_same_mesh_again():
    S, C = _S(), _C()
    a = R.run([[R.Track(0, S), _reacquire(S, 7, keep_mesh=True)], [R.Track(0, C)]], 20)
    b = R.run([[R.Track(0, S), _reacquire(S, 7)], [R.Track(0, C)]], 20)
    assert a["restart_stats"] == dict(calls=1, objects=1, meshes_replaced=0) and b["restart_stats"]["meshes_replaced"] == 1
    for slot in range(2):
        R.assert_same_bits(a, slot, 0, b, slot, 0, 20, "slot %d" % slot)


def test_three_restarts_in_a_row_and_all_slots_at_once():
    """Frame 7: slot 0 is restarted twice with another object's description and mesh, then both slots in one call; each then equals
    a new engine."""
    S, C, B = _S(), _C(), _B()

    def between(eng, f):
        if f == 7:
            t = R.Track(0, B)
            eng.restart_objects([(0, t.desc(), *B.mesh)])
            eng.restart_objects([(0, t.desc(), *B.mesh)], keep_mesh=True)

    got = R.run([[R.Track(0, S), _reacquire(S, 7)], [R.Track(0, C), _reacquire(C, 7)]], 20, between=between)
    assert got["restart_stats"] == dict(calls=3, objects=4, meshes_replaced=3)
    new = R.run([[_reacquire(S, 7, at=0)], [_reacquire(C, 7, at=0)]], 13)
    for slot in range(2):
        R.assert_same_bits(got, slot, 7, new, slot, 0, 13, "slot %d" % slot)
    assert sum(1 for f in range(7, 20) if got["log"][f][0][3] >= 0) >= 2


def test_restart_before_the_first_frame_equals_add():
    A, B, C = _A(), _B(), _C()

    def before_first(eng):
        eng.restart_objects([(0, R.Track(0, A).desc(), *A.mesh)])
        eng.restart_objects([(0, R.Track(0, B).desc(), *B.mesh), (1, R.Track(0, C).desc(), *C.mesh)])

    a = R.run([[R.Track(0, B)], [R.Track(0, C)]], 14, before_first=before_first)
    b = R.run([[R.Track(0, B)], [R.Track(0, C)]], 14)
    assert a["restart_stats"] == dict(calls=2, objects=3, meshes_replaced=3)
    for slot in range(2):
        R.assert_same_bits(a, slot, 0, b, slot, 0, 14, "slot %d" % slot)


def test_device_inputs_across_a_restart():
    S, C = _S(), _C()
    got = R.run([[R.Track(0, S), _reacquire(S, 7)], [R.Track(0, C)]], 20, splits=[4, 3], mode="device", read_masks=False)
    new = R.run([[_reacquire(S, 7, at=0)], [_reacquire(S, 7, at=0)]], 13, splits=[4, 3], mode="device", read_masks=False)
    plain = R.run([[R.Track(0, S)], [R.Track(0, C)]], 20, splits=[4, 3], mode="device", read_masks=False)
    R.assert_same_bits(got, 0, 7, new, 0, 0, 13, "restarted slot against a new engine")
    R.assert_same_bits(got, 1, 0, plain, 1, 0, 20, "the other slot")


def test_refused_calls_change_nothing():
    """Every refusal -- ROFT_ERR_INVALID at batch boundaries, ROFT_ERR_STATE between a submit and its step -- leaves the run bit for
    bit what it is without the calls."""
    import ctypes as C_
    S, C = _S(), _C()
    lib = L.lib()
    codes = []

    def call(eng, ids, descs, n, flags=0):
        arr_i = (C_.c_int * max(len(ids), 1))(*ids)
        arr_d = (L.ObjectDesc * max(len(descs), 1))(*descs)
        rc = lib.roft_objects_restart(eng._h, arr_i if ids else None, arr_d if descs else None, n, flags)
        codes.append((rc, lib.roft_last_error_string()))
        return rc

    def with_mesh(st, d):
        d.mesh = L.Mesh(st.mesh[0].ctypes.data, st.mesh[0].shape[0], st.mesh[1].ctypes.data, st.mesh[1].shape[0])
        return d

    good = with_mesh(S, R.Track(0, S).desc())

    def between(eng, f):
        if f in (5, 11):
            assert call(eng, [2], [good], 1) == -1                          # not an object of the engine
            assert call(eng, [-1], [good], 1) == -1
            assert call(eng, [0, 0], [good, good], 2) == -1                 # named twice
            assert call(eng, [0], [good], 1, flags=2) == -1                 # unknown flag bits
            assert call(eng, [0], [good], -1) == -1
            assert call(eng, [], [], 1) == -1                               # n > 0 with NULL arrays
            assert call(eng, [0], [R.Track(0, S).desc()], 1) == -1          # outlier rejection needs a mesh
            bad = S.mesh[1].copy()
            bad[3, 2] = S.mesh[0].shape[0]
            d = R.Track(0, S).desc()
            d.mesh = L.Mesh(S.mesh[0].ctypes.data, S.mesh[0].shape[0], bad.ctypes.data, bad.shape[0])
            assert call(eng, [1, 0], [good, d], 2) == -1                    # a triangle that names no vertex: nothing of the call happens
            assert call(eng, [], [], 0) == 0                                # nothing to do

    def after_submit(eng, f):
        if f in (5, 6, 12):
            assert call(eng, [0], [good], 1) == -4 and b"not been stepped" in codes[-1][1]
            assert call(eng, [0], [good], 1, flags=L.RESTART_KEEP_MESH) == -4

    a = R.run([[R.Track(0, S)], [R.Track(0, C)]], 20, between=between, after_submit=after_submit)
    b = R.run([[R.Track(0, S)], [R.Track(0, C)]], 20)
    assert a["restart_stats"] == dict(calls=0, objects=0, meshes_replaced=0)
    assert all(len(msg) > 5 for rc, msg in codes if rc != 0)
    for slot in range(2):
        R.assert_same_bits(a, slot, 0, b, slot, 0, 20, "slot %d" % slot)
