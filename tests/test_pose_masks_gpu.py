"""Masks from poses on the device (roft_engine_enable_pose_masks, roft_pose_silhouette; pose_silhouette_kernel in
roft_amd/csrc/k_silhouette.hip).  The contract is an equivalence (include/roft_engine.h, section 3e): an enrolled object whose
frame brings no mask behaves, bit for bit, as if it had been handed the HOST mask roft_render_depth(mesh, pose, cam, 1) > 0 ? 255 :
0.  So every engine test here runs two engines on identical inputs -- engine A is handed the silhouettes as masks through the
existing call, engine B is enrolled and handed none -- and asks for EQUAL logs and masks.  The expected masks always come from the
oracle's ro_render_depth on the CPU (tests/pose_mask_cases.py), never from the kernel under test.

Shapes: util.stream(seed, 14, scale=4) is 160 x 120 -- five plane words per row, two bands of the kernel's default split -- with
poses at frames 0, 6 and 12; the operator's cases are the table of pose_mask_cases.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_mask_cases as pc
import util
from oracle import binding as ob
from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops, synth
from test_engine_gpu import POS_TOL, ROT_TOL, TWIST_TOL, make_engine, rot_err
from test_label_masks_gpu import Holder, _assert_same, _read_log

pytestmark = pytest.mark.gpu

N_FRAMES = 14          # poses at frames 0, 6 and 12
SPLITS = [4, 8, 2]     # batches: a silhouette first in a batch, in the middle of one, and first in the last
N_OBJ = 3


def _lib_mesh(v, t):
    return L.Mesh(v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0])


# ---- 1. the operator ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pc.cases()))
def test_operator_case_equals_the_oracle_in_every_launch_shape(name):
    mesh, p = pc.cases()[name]
    want = pc.expected(name)
    m = _lib_mesh(*pc.meshes()[mesh])
    cam = L.Camera(*pc.CAM)
    for bands in (0, 1, 2, 8):
        for vertex_cache in (True, False):
            got, count = ops.pose_silhouette(cam, m, p[:3], p[3:], bands, vertex_cache)
            assert np.array_equal(got, want), (name, bands, vertex_cache, int((got != want).sum()))
            assert count == int((want > 0).sum()), (name, bands, vertex_cache)


@pytest.mark.parametrize("size", [(1280, 720), (1920, 1080)], ids=["1280x720", "1920x1080"])
def test_operator_large_image_mostly_covered(size):
    """The object fills most of the image: bands are needed (a whole plane is 115 / 259 KB), and one band (bands = 1) is drawn in
    strips of the LDS window."""
    Wd, Hd = size
    cam = (Wd, Hd, 0.96 * Wd, 0.96 * Wd, Wd / 2.0, Hd / 2.0)
    p = pc.pose([0.0, 0.0, 0.26], [1, 2, 3], 0.3)
    want = pc.silhouette("box12", p, cam)
    assert (want > 0).mean() > 0.5 and want[0].any() and not want[:, 0].any()
    m = _lib_mesh(*pc.meshes()["box12"])
    for bands, vertex_cache in ((0, True), (1, False), (7, True)):
        got, count = ops.pose_silhouette(L.Camera(*cam), m, p[:3], p[3:], bands, vertex_cache)
        assert np.array_equal(got, want), (size, bands, int((got != want).sum()))
        assert count == int((want > 0).sum())


# ---- the two-engine harness --------------------------------------------------------------------------------------------
def _streams():
    streams = [util.stream(1400 + i, N_FRAMES, scale=4) for i in range(N_OBJ)]
    assert all([k for k in range(N_FRAMES) if st.pose_valid[k]] == [0, 6, 12] for st in streams)
    return streams


@functools.lru_cache(maxsize=None)
def _oracle_mesh(i):
    return ob.make_mesh(*_streams()[i].mesh)


@functools.lru_cache(maxsize=None)
def _silhouette(i, pose_bytes):
    """The mask the contract defines for object i at a pose (7 doubles as bytes: computed once)."""
    st = _streams()[i]
    c = st.camera
    return pc.silhouette(_oracle_mesh(i), np.frombuffer(pose_bytes), (c.width, c.height, c.fx, c.fy, c.cx, c.cy))


def _pose0(i):
    return synth.initial_pose_from_stream(_streams()[i])[6:13]


class Scenario:
    """What both engines are handed, per frame k and object i: pose(k, i) -> (x, q) or None; delivered(k, i) -> a byte mask handed to
    BOTH engines or None; label(k, i) -> True when engine B gets object i's delivered mask as a value of a label image instead.
    enrolled: the objects engine B enrols (None: roft_engine_enable_pose_masks with n_ids == 0).  Engine A gets, where nothing is
    delivered to an enrolled object, the silhouette the contract names -- of the frame's pose, or on frame 0 of the initial pose."""

    def __init__(self, enrolled=None, pose=None, delivered=None, label=None):
        self.enrolled = enrolled
        self.pose = pose or (lambda k, i: util.frame_inputs(_streams()[i], k)[3])
        self.delivered = delivered or (lambda k, i: None)
        self.label = label or (lambda k, i: False)

    def is_enrolled(self, i):
        return self.enrolled is None or i in self.enrolled

    def mask_a(self, k, i):
        m = self.delivered(k, i)
        if m is not None or not self.is_enrolled(i):
            return m
        pose = self.pose(k, i)
        if pose is None and k > 0:
            return None
        p = np.concatenate(pose) if pose is not None else _pose0(i)
        return _silhouette(i, np.ascontiguousarray(p, np.float64).tobytes())

    def frames(self, holder, k, engine):
        out, lab = [], None
        for i, st in enumerate(_streams()):
            depth, flow, _, _ = util.frame_inputs(st, k)
            f = dict(depth=holder.put(depth), flow=holder.put(flow), mask=None, pose=self.pose(k, i), dt=st.dt, mem_kind=holder.kind)
            if engine == "A":
                f["mask"] = holder.put(self.mask_a(k, i))
            elif self.delivered(k, i) is not None:
                if self.label(k, i):
                    if lab is None:   # one label image per frame: the delivered masks of its label objects, in order
                        img = np.zeros((st.camera.height, st.camera.width), np.uint8)
                        for j in range(N_OBJ):
                            if self.label(k, j) and self.delivered(k, j) is not None:
                                assert not (img[self.delivered(k, j) > 0]).any(), "label objects of the test do not overlap"
                                img[self.delivered(k, j) > 0] = j + 1
                        lab = holder.put(img)
                    f["labels"], f["label"] = lab, i + 1
                    if isinstance(lab, int):
                        f["label_type"] = L.LABEL_U8
                else:
                    f["mask"] = holder.put(self.delivered(k, i))
            out.append(f)
        return out


def _run(sc, engine, splits, mem="pageable", setup=None, n=N_FRAMES, per_step=None):
    """Returns (log, final masks, stats, pose mask stats)."""
    holder = Holder(mem)
    eng = make_engine(_streams(), max_batch_frames=8 if splits else 1)
    eng.enable_log(n)
    if setup:
        setup(eng)
    if engine == "B":
        eng.enable_pose_masks(sc.enrolled)
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
        if per_step:
            per_step(eng, k)
    out = _read_log(eng, n), [eng.mask(o) for o in range(N_OBJ)], eng.stats(), eng.pose_mask_stats()
    eng.close()
    return out


def _pair(sc, splits, mem="pageable", setup=None):
    """Engines A and B over the scenario, every object's mask compared after every step."""
    seen = {"A": [], "B": []}

    def keep(which):
        return lambda eng, k: seen[which].append([eng.mask(o) for o in range(N_OBJ)])

    a = _run(sc, "A", splits, mem, setup, per_step=keep("A"))
    b = _run(sc, "B", splits, mem, setup, per_step=keep("B"))
    _assert_same(b[:3], a[:3], (splits, mem))
    assert len(seen["A"]) == len(seen["B"]) > 0
    for s, (ma, mb) in enumerate(zip(seen["A"], seen["B"])):
        for o in range(N_OBJ):
            assert np.array_equal(ma[o], mb[o]), ("mask after step", s, "object", o)
    assert a[3] == dict(silhouettes=0, frames=0)
    assert (a[0]["npts"] > 0).any() and (a[0]["sel"] >= 0).any(), "the run tracks: flow points and outlier tests"
    return a, b


# ---- 2. engine parity, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "device"])
@pytest.mark.parametrize("splits", [None, SPLITS], ids=["frame_by_frame", "splits_4_8_2"])
def test_engine_parity_with_host_silhouettes(splits, mem):
    a, b = _pair(Scenario(), splits, mem)
    assert b[3] == dict(silhouettes=3 * N_OBJ, frames=3)
    assert all(m.any() for m in b[1])
    # ONE launch per batch that delivers, whatever the number of objects.  Counted against engine A: here (a burst of three objects,
    # no preparation ahead) A's per-object masks ride in the control-block launch, so a delivering batch costs A one launch for both;
    # B uploads the control blocks and draws the silhouettes, two launches -- one more per delivering batch, three batches deliver.
    assert b[2]["launches"] - a[2]["launches"] == 3
    assert b[2]["event_ops"] == a[2]["event_ops"]


@pytest.mark.parametrize("env", ["ROFT_ONE_STREAM=1", "ROFT_PREP_AHEAD=2", "ROFT_CTRL_INGEST=0"])
def test_engine_parity_under_the_scheduling_switches(env, monkeypatch):
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    _pair(Scenario(), SPLITS)
    _pair(Scenario(), None)


def test_operator_on_stream_poses_at_640x480_next_to_live_engines():
    """The operator in the situation of tools/bench_pose_masks.py: 640 x 480, the poses and the mesh of a synthetic stream, in a
    process that holds an engine.  The mesh goes in as arrays (ops.pose_silhouette makes them C-contiguous: the address of a
    Fortran-ordered triangle array, which column selections produce, names other triangles), also deliberately Fortran-ordered."""
    st = util.stream(1400, N_FRAMES, scale=1)
    c = st.camera
    cam = (c.width, c.height, c.fx, c.fy, c.cx, c.cy)
    v, t = st.mesh
    assert v.flags["C_CONTIGUOUS"] and t.flags["C_CONTIGUOUS"], "synth.box_mesh hands out arrays whose address is the mesh"
    eng = make_engine(_streams())
    eng.enable_pose_masks()
    eng.submit(Scenario().frames(Holder("pageable"), 0, "B"))
    eng.step()
    mesh_o = ob.make_mesh(v, t)
    for k in (0, 6, 12):
        p = st.pose_meas[k]
        want = pc.silhouette(mesh_o, p, cam)
        assert (want > 0).sum() > 10000
        for mesh in ((v, t), (np.asfortranarray(v), np.asfortranarray(t)), _lib_mesh(v, t)):
            got, count = ops.pose_silhouette(L.Camera(*cam), mesh, p[:3], p[3:])
            assert np.array_equal(got, want), (k, int((got != want).sum()))
            assert count == int((want > 0).sum())
    eng.close()


# ---- 3. mixing and rules -----------------------------------------------------------------------------------------------
def _stream_mask(k, i):
    st = _streams()[i]
    return st.mask_gt[st.mask_delivery[k]].numpy() if st.mask_delivery[k] >= 0 else None


@pytest.mark.parametrize("splits", [None, SPLITS], ids=["frame_by_frame", "splits_4_8_2"])
def test_enrolled_plain_and_label_objects_in_one_frame(splits):
    """object 0 enrolled, object 1 its network mask, object 2 a value of a label image -- in the same frames"""
    sc = Scenario(enrolled=[0], delivered=lambda k, i: _stream_mask(k, i) if i > 0 else None, label=lambda k, i: i == 2)
    a, b = _pair(sc, splits)
    assert b[3] == dict(silhouettes=3, frames=3)


def test_a_delivered_mask_wins_on_a_pose_frame():
    sc = Scenario(delivered=lambda k, i: _stream_mask(k, i) if (k, i) == (6, 1) else None)
    assert not np.array_equal(_stream_mask(6, 1), Scenario().mask_a(6, 1))
    a, b = _pair(sc, SPLITS)
    assert b[3] == dict(silhouettes=3 * N_OBJ - 1, frames=3)


def test_a_dropped_pose_delivers_nothing():
    base = Scenario()
    sc = Scenario(pose=lambda k, i: None if (k, i) == (6, 1) else base.pose(k, i))
    a, b = _pair(sc, SPLITS)
    assert b[3] == dict(silhouettes=3 * N_OBJ - 1, frames=3)


def test_an_off_screen_pose_is_ignored_like_an_empty_mask():
    base = Scenario()
    off = (np.array([1.0, 0.0, 0.45]), np.array([1.0, 0.0, 0.0, 0.0]))
    sc = Scenario(pose=lambda k, i: off if (k, i) == (6, 2) else base.pose(k, i))
    assert not sc.mask_a(6, 2).any() and sc.mask_a(6, 1).any()
    for splits in (None, SPLITS):
        a, b = _pair(sc, splits)
        assert b[3] == dict(silhouettes=3 * N_OBJ, frames=3)      # drawn, found empty, ignored: the mask went on from the one before
        assert b[1][2].any()


def test_frame_zero_without_a_pose_uses_the_initial_pose():
    base = Scenario()
    sc = Scenario(pose=lambda k, i: None if k == 0 and i != 1 else base.pose(k, i))
    assert sc.mask_a(0, 0).any()
    for splits in (None, SPLITS):
        a, b = _pair(sc, splits)
        assert b[3] == dict(silhouettes=3 * N_OBJ, frames=3)


def test_no_ids_enrols_every_object():
    every = _run(Scenario(enrolled=None), "B", SPLITS)
    listed = _run(Scenario(enrolled=[0, 1, 2]), "B", SPLITS)
    _assert_same(every[:3], listed[:3])
    assert every[3] == listed[3] == dict(silhouettes=3 * N_OBJ, frames=3)
    assert every[2]["launches"] == listed[2]["launches"]


def test_an_object_that_is_not_enrolled_still_needs_its_mask():
    eng = make_engine(_streams())
    eng.enable_pose_masks([0, 2])
    holder = Holder("pageable")
    with pytest.raises(L.RoftError) as err:
        eng.submit(Scenario(enrolled=[0, 2]).frames(holder, 0, "B"))
    assert "error -4:" in str(err.value)
    eng.close()


# ---- 4. everything on --------------------------------------------------------------------------------------------------
def test_everything_on_flow_raw_depth_quality_and_pose_masks():
    """camera images instead of flows, 16-bit depth, track quality and pose masks in one engine: equal to the same engine handed the
    silhouettes as HOST masks, quality records included"""
    n, scale = N_FRAMES, 0.001
    streams = [util.stream(1400 + i, n, scale=4, with_gray=True) for i in range(N_OBJ)]
    grays = [[np.ascontiguousarray(st.gray[k].numpy()) for k in range(n)] for st in streams]
    raws = [[np.clip(np.rint(st.depth[k].numpy() / scale), 0, 65535).astype(np.uint16) for k in range(n)] for st in streams]
    sc = Scenario()

    def run(engine):
        eng = make_engine(streams, max_batch_frames=8)
        eng.enable_flow()
        eng.enable_raw_depth(scale)
        eng.enable_log(40)
        eng.enable_quality()
        if engine == "B":
            eng.enable_pose_masks()
        k = 0
        for t in SPLITS:
            batch = []
            for j in range(t):
                kk = k + j
                batch.append([dict(depth=raws[i][kk], image=grays[i][kk], flow=None, pose=sc.pose(kk, i), dt=streams[i].dt,
                                   mask=sc.mask_a(kk, i) if engine == "A" else None) for i in range(N_OBJ)])
            eng.submit_batch(batch)
            eng.step()
            k += t
        out = _read_log(eng, n), [eng.mask(o) for o in range(N_OBJ)], eng.stats(), eng.quality(0, n)
        eng.close()
        return out

    a, b = run("A"), run("B")
    _assert_same(b[:3], a[:3])
    assert a[3].tobytes() == b[3].tobytes() and (b[3]["n_both"] > 0).all()
    assert (b[0]["npts"] > 0).any()


# ---- 5. against the oracle tracker ---------------------------------------------------------------------------------------
def test_enrolled_engine_matches_the_oracle_tracker_fed_the_silhouettes():
    streams = _streams()
    sc = Scenario()
    ref = []
    for i, st in enumerate(streams):
        trk = ob.Tracker(util.oracle_config(ob, st), *st.mesh)
        rows = []
        for k in range(N_FRAMES):
            depth, flow, _, pose = util.frame_inputs(st, k)
            r = trk.step(st.dt, depth, flow, sc.mask_a(k, i), pose)
            rows.append(dict(pose=np.array(r.pose), twist=np.array(r.twist), n=r.n_flow_points, sel=r.outlier_selected, mask=trk.mask()))
        trk.close()
        ref.append(rows)
    eng = make_engine(streams)
    eng.enable_pose_masks()
    holder = Holder("pageable")
    tests = 0
    for k in range(N_FRAMES):
        eng.submit(sc.frames(holder, k, "B"))
        eng.step()
        outs = eng.outputs()
        for o in range(N_OBJ):
            got, exp = outs[o], ref[o][k]
            assert got.n_flow_points == exp["n"], (k, o)
            assert got.outlier_selected == exp["sel"], (k, o)
            tests += exp["sel"] >= 0
            assert np.array_equal(eng.mask(o), exp["mask"]), (k, o)
            pose = np.array(got.pose)
            np.testing.assert_allclose(pose[:9], exp["pose"][:9], rtol=0, atol=POS_TOL, err_msg="frame %d obj %d" % (k, o))
            assert rot_err(pose[9:], exp["pose"][9:]) < ROT_TOL, (k, o)
            np.testing.assert_allclose(np.array(got.twist), exp["twist"], rtol=0, atol=TWIST_TOL)
    eng.close()
    assert tests >= 2 * N_OBJ


# ---- the sequence tool -------------------------------------------------------------------------------------------------
def test_run_sequence_tracks_a_directory_without_masks(tmp_path, capsys):
    """tools/run_sequence.py --masks-from-pose on a sequence directory whose masks were deleted: it tracks, and its logs are those of a
    run over the same directory with the silhouettes of the delivered poses written out as the mask files"""
    import importlib.util
    import json
    import os
    import shutil
    from roft_amd import io
    n = 14
    st = util.stream(1400, n, scale=4)
    root = str(tmp_path / "seq")
    mesh = io.write_sequence(root, st, "box", flow_set="analytic")
    shutil.rmtree(os.path.join(root, "masks"))
    spec = importlib.util.spec_from_file_location("run_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_sequence.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    common = ["--root", root, "--object", "box", "--mesh", mesh, "--flow-set", "analytic"]
    with pytest.raises(L.RoftError):
        rs.main(common + ["--out", str(tmp_path / "none_")])          # no masks, not enrolled: the first frame is refused
    assert rs.main(common + ["--out", str(tmp_path / "b_"), "--masks-from-pose"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["pose_masks"] == dict(silhouettes=3, frames=3) and report["frames"] == n
    assert report["rmse_position_cm"] < 5.0
    # the same directory with the silhouettes as mask files: frame k delivers the mask file of frame k - 6 and the pose row of
    # frame k - 6, so the file of frame j holds the silhouette of detection j
    seq = io.Sequence(root, "box", flow_set="analytic", mask_set="sil", width=st.camera.width, height=st.camera.height)
    os.makedirs(seq.mask_dir)
    v, t = io.load_obj(mesh)
    c = st.camera
    for j in range(n):
        if seq.pose_ok[j]:
            io.write_png(os.path.join(seq.mask_dir, "box_%d.png" % j),
                         pc.silhouette(ob.make_mesh(v, t), seq.poses[j], (c.width, c.height, c.fx, c.fy, c.cx, c.cy)))
    assert rs.main(common + ["--out", str(tmp_path / "a_"), "--mask-set", "sil"]) == 0
    for name in ("pose_estimate", "velocity_estimate"):
        assert open(str(tmp_path / ("a_" + name)), "rb").read() == open(str(tmp_path / ("b_" + name)), "rb").read()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device():
    lib = L.lib()
    streams = _streams()
    ids = (C.c_int * 2)(0, 1)

    def code(eng, arr, n):
        rc = lib.roft_engine_enable_pose_masks(eng._h, arr, n)
        assert rc == 0 or len(lib.roft_last_error_string()) > 10
        return rc

    eng = make_engine(streams)
    assert code(eng, (C.c_int * 1)(3), 1) == -1           # not an object of the engine
    assert code(eng, (C.c_int * 1)(-1), 1) == -1
    assert code(eng, None, 2) == -1                       # ids announced, none given
    assert code(eng, ids, -1) == -1
    assert code(eng, ids, 2) == 0
    assert code(eng, None, 0) == 0                        # more than once: the sets add up
    holder = Holder("pageable")
    eng.submit(Scenario().frames(holder, 0, "B"))
    assert code(eng, ids, 2) == -4                        # a frame is submitted
    eng.step()
    assert code(eng, ids, 2) == -4
    ms = C.c_double(0.0)
    assert lib.roft_debug_pose_mask_kernel_ms(eng._h, C.byref(ms)) == 0 and 0.0 < ms.value < 1000.0
    eng.close()

    stamped = make_engine(streams, stamped_masks=1)
    assert code(stamped, ids, 2) == -1 and b"stamp" in lib.roft_last_error_string()
    stamped.close()
    gl = make_engine(streams, render_mode=L.RENDER_GL)
    assert code(gl, ids, 2) == -1 and b"ROFT_RENDER_GL" in lib.roft_last_error_string()
    gl.close()
    # an object added without a mesh cannot be named
    cfg = E.default_config(160, 120, L.FLOW_F32C2, max_objects=1)
    cfg.outlier_rejection = 0
    bare = E.ROFTFilterBatch(cfg)
    bare.add_object(E.default_object(), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert code(bare, (C.c_int * 1)(0), 1) == -1 and b"mesh" in lib.roft_last_error_string()
    fresh = L.EnginePoseMaskStats()
    assert lib.roft_engine_get_pose_mask_stats(bare._h, C.byref(fresh)) == 0 and (fresh.silhouettes, fresh.frames) == (0, 0)
    assert lib.roft_debug_pose_mask_kernel_ms(bare._h, C.byref(ms)) == -4
    bare.close()
