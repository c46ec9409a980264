"""Enrolled objects of one scene hide each other's silhouettes, on the device (roft_engine_enable_pose_mask_occlusion,
roft_pose_silhouettes_occluded; pose_silhouette_kernel<true> and pose_resolve_kernel in roft_amd/csrc/k_silhouette.hip).  The
contract is an equivalence (include/roft_engine.h, section 3e): an enrolled engine with the mode on behaves, bit for bit, like a
plain engine handed the RESOLVED silhouettes as HOST masks.  So every engine test here runs twins on identical inputs and asks
for equal logs and masks after every step.  The expected masks always come from the oracle's ro_render_depth on the CPU, resolved
in numpy by the definition (tests/pose_mask_occlusion_cases.py), never from the kernels under test.

Shapes: four objects (the same box mesh) on ONE stream, util.stream(1500, 14, scale=4) = 160 x 120, poses on every even frame on
trajectories of this file: objects 0 and 1 cross each other, object 2 stands in front of object 3, which moves behind it."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_mask_cases as pc
import pose_mask_occlusion_cases as oc
import util
from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops
from test_label_masks_gpu import Holder, _assert_same, _read_log

pytestmark = pytest.mark.gpu

N_FRAMES = 14
SPLITS = [4, 8, 2]
N_OBJ = 4
ONE_SCENE = {0: 0, 1: 0, 2: 0, 3: 0}


# ---- 1. the operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(oc.CASES))
def test_operator_case_equals_the_oracle_in_every_launch_shape(name):
    scene = oc.CASES[name][0]
    _, want = oc.expected(name)
    meshes = [oc.meshes()[m] for m, _ in scene]
    xs, qs = np.array([p[:3] for _, p in scene]), np.array([p[3:] for _, p in scene])
    cam = L.Camera(*oc.CAM)
    for bands in (0, 1, 3, oc.H):
        for vertex_cache in (False, True):
            got, counts = ops.pose_silhouettes_occluded(cam, meshes, xs, qs, bands, vertex_cache)
            assert np.array_equal(got, want), (name, bands, vertex_cache, (got != want).sum(axis=(1, 2)).tolist())
            assert counts.tolist() == (want > 0).sum(axis=(1, 2)).tolist(), (name, bands, vertex_cache)


@pytest.mark.parametrize("name", sorted(pc.AIMED))
def test_operator_with_one_object_is_the_plain_silhouette(name):
    mesh, p = pc.cases()[name]
    cam = L.Camera(*pc.CAM)
    got, counts = ops.pose_silhouettes_occluded(cam, [pc.meshes()[mesh]], [p[:3]], [p[3:]])
    plain, count = ops.pose_silhouette(cam, pc.meshes()[mesh], p[:3], p[3:])
    assert np.array_equal(got[0], plain) and np.array_equal(plain, pc.expected(name))
    assert counts.tolist() == [count]


# ---- the twin-engine harness -------------------------------------------------------------------------------------------
def _stream():
    return util.stream(1500, N_FRAMES, scale=4)


def traj(k, i):
    """pose [7] of object i on frame k"""
    if i == 0:
        return pc.pose([-0.07 + 0.002 * k, 0.0, 0.50], [0, 1, 0], 0.6)
    if i == 1:
        return pc.pose([-0.07 - 0.002 * k, 0.0, 0.50], [0, 1, 0], -0.6)
    if i == 2:
        return pc.pose([0.085, 0.0, 0.40], [1, 2, 3], 0.7 + 0.01 * k)
    return pc.pose([0.40 - 0.026 * k, 0.02, 0.95], [1, 2, 3], 0.7)


def _default_pose(k, i):
    if k % 2:
        return None
    p = traj(k, i)
    return p[:3].copy(), p[3:].copy()


@functools.lru_cache(maxsize=None)
def _render(pose_bytes):
    """R of the definition for the objects' mesh at a pose (7 doubles as bytes: computed once)."""
    st = _stream()
    c = st.camera
    assert all(np.array_equal(a, b) for a, b in zip(st.mesh, oc.meshes()["box12"]))
    R = oc.render("box12", np.frombuffer(pose_bytes), (c.width, c.height, c.fx, c.fy, c.cx, c.cy))
    R.setflags(write=False)
    return R


class Scenario:
    """What the twins are handed per frame k and object i: pose(k, i) -> (x, q) or None; delivered(k, i) -> a byte mask handed to
    every engine, or None.  scene_of: object -> scene for the engine with the mode on (objects it does not name are scenes of their
    own).  Every object is enrolled; the first frame without a pose is drawn from the pose the object was added with, traj(0, i)."""

    def __init__(self, scene_of=ONE_SCENE, pose=None, delivered=None):
        self.scene_of = scene_of
        self.pose = pose or _default_pose
        self.delivered = delivered or (lambda k, i: None)

    def drawn_pose(self, k, i):
        """the pose whose silhouette is object i's mask on frame k, or None when the mask arrives another way or not at all"""
        if self.delivered(k, i) is not None:
            return None
        p = self.pose(k, i)
        if p is None:
            return traj(0, i) if k == 0 else None
        return np.concatenate(p)

    @functools.lru_cache(maxsize=None)
    def frame_masks(self, k, resolved=True):
        """object -> (plain silhouette, expected mask) as bool arrays, for the objects drawn on frame k; with resolved=False the
        expected masks of an engine WITHOUT the mode (the plain silhouettes)."""
        drawn = {i: self.drawn_pose(k, i) for i in range(N_OBJ)}
        drawn = {i: p for i, p in drawn.items() if p is not None}
        R = {i: _render(np.ascontiguousarray(p, np.float64).tobytes()) for i, p in drawn.items()}
        out = {i: (R[i] > 0, R[i] > 0) for i in drawn}
        if resolved:
            scenes = {}
            for i in sorted(drawn):
                if i in self.scene_of:
                    scenes.setdefault(self.scene_of[i], []).append(i)
            for members in scenes.values():
                raw, res = oc.resolve(np.stack([R[i] for i in members]))
                for j, i in enumerate(members):
                    out[i] = (raw[j], res[j])
        return out

    def expected_stats(self, n=N_FRAMES):
        resolved = hidden = removed = 0
        for k in range(n):
            masks = self.frame_masks(k)
            for i, (raw, res) in masks.items():
                mates = [j for j in masks if j != i and i in self.scene_of and self.scene_of.get(j) == self.scene_of[i]]
                if mates:
                    resolved += 1
                    hidden += bool(raw.any() and not res.any())
                    removed += int(raw.sum() - res.sum())
        return dict(resolved=resolved, hidden=hidden, pixels_removed=removed)

    def frames(self, holder, k, engine):
        """engine "host": a plain engine, handed the expected masks as HOST masks (a hidden silhouette: all zeros); "plain_host": the
        same with the plain silhouettes; "occl": enrolled, the mode on; "enrolled": enrolled, the mode off"""
        st = _stream()
        depth, flow, _, _ = util.frame_inputs(st, k)
        depth, flow = holder.put(depth), holder.put(flow)
        out = []
        for i in range(N_OBJ):
            f = dict(depth=depth, flow=flow, mask=holder.put(self.delivered(k, i)), pose=self.pose(k, i), dt=st.dt, mem_kind=holder.kind)
            if engine in ("host", "plain_host") and f["mask"] is None:
                masks = self.frame_masks(k, engine == "host")
                if i in masks:
                    f["mask"] = holder.put(np.ascontiguousarray(masks[i][1].astype(np.uint8) * 255))
            out.append(f)
        return out


def _make_engine(**over):
    st = _stream()
    cfg = E.default_config(st.camera.width, st.camera.height, st.flow_type, max_objects=N_OBJ)
    c = st.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st.flow_grid, st.flow_scale
    for k, v in over.items():
        setattr(cfg, k, v)
    eng = E.ROFTFilterBatch(cfg)
    for i in range(N_OBJ):
        d = E.default_object()
        p0 = traj(0, i)
        for j in range(13):
            d.p_mean0[j] = p0[j - 6] if j >= 6 else 0.0
        eng.add_object(d, *st.mesh)
    return eng


def _run(sc, engine, splits, mem="pageable", n=N_FRAMES):
    """Returns (log, final masks, stats, masks after every step, occlusion stats)."""
    holder = Holder(mem)
    eng = _make_engine(max_batch_frames=8 if splits else 1)
    eng.enable_log(n)
    if engine in ("occl", "enrolled"):
        eng.enable_pose_masks()
    if engine == "occl":
        eng.enable_pose_mask_occlusion(sc.scene_of)
    seen = []
    k = i = 0
    while k < n:
        t = 1 if splits is None else min(splits[i % len(splits)], n - k)
        i += 1
        if splits is None:
            eng.submit(sc.frames(holder, k, engine))
        else:
            eng.submit_batch([sc.frames(holder, k + j, engine) for j in range(t)])
        eng.step()
        k += t
        seen.append([eng.mask(o) for o in range(N_OBJ)])
    out = _read_log(eng, n), [eng.mask(o) for o in range(N_OBJ)], eng.stats(), seen, eng.pose_mask_occlusion_stats()
    eng.close()
    return out


def _twins(sc, splits, mem="pageable", first="host", second="occl"):
    a, b = _run(sc, first, splits, mem), _run(sc, second, splits, mem)
    _assert_same(b[:3], a[:3], (splits, mem))
    assert len(a[3]) == len(b[3]) > 0
    for s, (ma, mb) in enumerate(zip(a[3], b[3])):
        for o in range(N_OBJ):
            assert np.array_equal(ma[o], mb[o]), ("mask after step", s, "object", o)
    assert (a[0]["npts"] > 0).any() and (a[0]["sel"] >= 0).any(), "the run tracks: flow points and outlier tests"
    return a, b


def test_the_trajectories_cross_and_hide():
    sc = Scenario()
    crossing = hidden = partly = 0
    for k in range(0, N_FRAMES, 2):
        m = sc.frame_masks(k)
        both = m[0][0] & m[1][0]
        crossing += bool((m[0][1] & both).any() and (m[1][1] & both).any())
        hidden += bool(m[3][0].any() and not m[3][1].any())
        partly += bool(m[3][1].any() and m[3][1].sum() < m[3][0].sum())
    assert crossing >= 1 and hidden >= 1 and partly >= 1
    assert sc.expected_stats()["hidden"] >= 1


# ---- 3. engine parity, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "device"])
@pytest.mark.parametrize("splits", [None, SPLITS], ids=["frame_by_frame", "splits_4_8_2"])
def test_engine_parity_with_resolved_host_silhouettes(splits, mem):
    sc = Scenario()
    a, b = _twins(sc, splits, mem)
    # ---- 6. the statistics, against what the numpy resolve counts
    assert b[4] == sc.expected_stats() and b[4]["resolved"] == 4 * 7 and b[4]["hidden"] >= 1 and b[4]["pixels_removed"] > 0
    assert a[4] == dict(resolved=0, hidden=0, pixels_removed=0)


@pytest.mark.parametrize("env", ["ROFT_ONE_STREAM=1", "ROFT_PREP_AHEAD=2", "ROFT_CTRL_INGEST=0"])
def test_engine_parity_under_the_scheduling_switches(env, monkeypatch):
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    sc = Scenario()
    for splits in (SPLITS, None):
        a, b = _twins(sc, splits)
        assert b[4] == sc.expected_stats()


def test_the_mode_changes_what_the_engine_computes():
    """the same engine without the mode equals the PLAIN silhouettes as host masks, and differs from the resolved ones: the parity
    above is not vacuous"""
    sc = Scenario()
    _twins(sc, SPLITS, first="plain_host", second="enrolled")
    on, off = _run(sc, "occl", SPLITS), _run(sc, "enrolled", SPLITS)
    assert any(not np.array_equal(x, y) for x, y in zip(on[1], off[1]))
    assert off[4] == dict(resolved=0, hidden=0, pixels_removed=0)


# ---- 4. membership of D ------------------------------------------------------------------------------------------------
def test_an_object_with_a_delivered_mask_neither_hides_nor_is_hidden():
    st = _stream()
    net = st.mask_gt[6].numpy()
    sc = Scenario(delivered=lambda k, i: net if (k, i) == (6, 2) else None)
    m = sc.frame_masks(6)
    assert 2 not in m and m[3][1].any() and np.array_equal(m[3][1], m[3][0]), "object 3 is behind object 2 on frame 6, and whole"
    assert not Scenario().frame_masks(6)[3][1].any()
    for splits in (None, SPLITS):
        a, b = _twins(sc, splits)
        assert b[4] == sc.expected_stats() and b[4]["resolved"] == 4 * 7 - 1


def test_an_object_whose_pose_was_dropped_is_not_drawn_and_hides_nothing():
    sc = Scenario(pose=lambda k, i: None if (k, i) == (6, 2) else _default_pose(k, i))
    m = sc.frame_masks(6)
    assert 2 not in m and np.array_equal(m[3][1], m[3][0]) and m[3][1].any()
    for splits in (None, SPLITS):
        a, b = _twins(sc, splits)
        assert b[4] == sc.expected_stats() and b[4]["resolved"] == 4 * 7 - 1


def test_objects_of_different_scenes_keep_their_whole_silhouettes():
    sc = Scenario(scene_of={0: 0, 1: 1, 2: 5, 3: 5})
    m = sc.frame_masks(4)
    assert (m[0][0] & m[1][0]).any() and np.array_equal(m[0][1], m[0][0]) and np.array_equal(m[1][1], m[1][0])
    assert (m[2][0] & m[0][0]).any() and np.array_equal(m[2][1], m[2][0]) and not m[3][1].any()
    for splits in (None, SPLITS):
        a, b = _twins(sc, splits)
        assert b[4] == sc.expected_stats() and b[4]["resolved"] == 2 * 7


def test_frame_zero_without_poses_resolves_the_initial_poses():
    sc = Scenario(pose=lambda k, i: None if k == 0 else _default_pose(k, i))
    m = sc.frame_masks(0)
    assert sorted(m) == [0, 1, 2, 3] and any(res.sum() < raw.sum() for raw, res in m.values())
    for splits in (None, SPLITS):
        a, b = _twins(sc, splits)
        assert b[4] == sc.expected_stats() and b[4]["resolved"] == 4 * 7


# ---- 5. inert when there is nothing to resolve -------------------------------------------------------------------------
def test_every_object_a_scene_of_its_own_is_the_engine_without_the_mode():
    sc = Scenario(scene_of={0: 0, 1: 1, 2: 2, 3: 3})
    for splits in (None, SPLITS):
        on, off = _run(sc, "occl", splits), _run(sc, "enrolled", splits)
        _assert_same(on[:3], off[:3], splits)
        for ma, mb in zip(on[3], off[3]):
            assert all(np.array_equal(x, y) for x, y in zip(ma, mb))
        assert on[4] == dict(resolved=0, hidden=0, pixels_removed=0)
        assert on[2]["launches"] == off[2]["launches"] and on[2]["event_ops"] == off[2]["event_ops"]


def test_a_batch_with_silhouettes_to_resolve_is_one_launch_more():
    sc = Scenario()
    on, off = _run(sc, "occl", SPLITS), _run(sc, "enrolled", SPLITS)
    assert on[2]["launches"] - off[2]["launches"] == 3       # three batches, each delivers: the resolve launch
    assert on[2]["event_ops"] == off[2]["event_ops"]


# ---- 7. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device():
    lib = L.lib()
    sc = Scenario()
    ints = lambda *v: (C.c_int * len(v))(*v)

    def code(eng, ids, scenes, n):
        rc = lib.roft_engine_enable_pose_mask_occlusion(eng._h, ids, scenes, n)
        assert rc == 0 or len(lib.roft_last_error_string()) > 10
        return rc

    def runs_a_frame(eng, engine):
        eng.submit(sc.frames(Holder("pageable"), 0, engine))
        eng.step()
        assert all(eng.mask(o).any() for o in (0, 1, 2))

    # pose masks are not enabled
    eng = _make_engine()
    assert code(eng, ints(0, 1), ints(0, 0), 2) == -4
    assert code(eng, None, None, 0) == -4
    runs_a_frame(eng, "host")
    eng.close()
    # an id that is not enrolled
    eng = _make_engine()
    eng.enable_pose_masks([0, 1, 2])
    assert code(eng, ints(0, 3), ints(0, 0), 2) == -1 and b"enrolled" in lib.roft_last_error_string()
    eng.enable_pose_masks([3])
    assert code(eng, ints(0, 3), ints(0, 0), 2) == 0
    runs_a_frame(eng, "occl")
    eng.close()
    # the arguments
    eng = _make_engine()
    eng.enable_pose_masks()
    assert code(eng, ints(4), ints(0), 1) == -1               # not an object of the engine
    assert code(eng, ints(-1), ints(0), 1) == -1
    assert code(eng, ints(0, 1), ints(0, -1), 2) == -1        # a negative scene
    assert code(eng, ints(0, 1), ints(0, 0), -1) == -1
    assert code(eng, None, ints(0, 0), 2) == -1               # ids announced, an array missing
    assert code(eng, ints(0, 1), None, 2) == -1
    st = L.EnginePoseMaskOcclusionStats()
    assert lib.roft_engine_get_pose_mask_occlusion_stats(eng._h, C.byref(st)) == 0 and (st.resolved, st.hidden, st.pixels_removed) == (0, 0, 0)
    assert code(eng, ints(0, 1), ints(7, 7), 2) == 0
    assert code(eng, ints(1, 2, 3), ints(3, 3, 3), 3) == 0    # a later call replaces an object's scene: 0 is alone now
    eng.submit(sc.frames(Holder("pageable"), 0, "occl"))
    assert code(eng, None, None, 0) == -4                     # a frame is submitted
    eng.step()
    assert code(eng, ints(0, 1), ints(0, 0), 2) == -4
    twin = _run(Scenario(scene_of={1: 3, 2: 3, 3: 3}), "host", None, n=1)
    for o in range(N_OBJ):
        assert np.array_equal(eng.mask(o), twin[1][o]), o
    assert eng.pose_mask_occlusion_stats()["resolved"] == 3
    ms = C.c_double(0.0)
    assert lib.roft_debug_pose_mask_kernel_ms(eng._h, C.byref(ms)) == 0 and 0.0 < ms.value < 1000.0
    eng.close()
