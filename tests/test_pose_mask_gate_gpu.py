"""Silhouettes gated against the depth of the pose's own frame, on the device (roft_engine_enable_pose_mask_depth_gate,
roft_pose_silhouettes_gated; pose_silhouette_kernel<.., kGate> and pose_resolve_kernel<kGate> in roft_amd/csrc/k_silhouette.hip).
The contract is an equivalence (include/roft_engine.h, section 3e): a gated silhouette behaves, bit for bit, like the HOST mask
(R > 0 && keep(R, D_g)) ? 255 : 0 with D_g the depth of the pose's own frame.  So every engine test runs two engines on identical
inputs -- engine A is handed those masks through the existing call, engine B is enrolled with the gate on -- and asks for EQUAL logs
and masks.  The expected masks come from the oracle's ro_render_depth on the CPU and the keep formula in numpy float32
(tests/pose_mask_gate_cases.py), never from the kernels under test.

Shapes: those of the pose-mask tests -- 160 x 120, 14 frames, poses on frames 0, 6 and 12, each six frames old -- with an occluder
painted into every frame's depth: a bar 12 columns wide over the object, 0.15 m in front of it, which moves with the object, so a
gate against the wrong frame's depth yields another mask (checked on the CPU reference before any engine runs)."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_mask_gate_cases as gc
import restart_util as ru
import util
from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops, synth
from test_engine_gpu import make_engine
from test_label_masks_gpu import Holder, _assert_same, _read_log

pytestmark = pytest.mark.gpu

N_FRAMES = gc.N_FRAMES
SPLITS = [4, 8, 2]
oc, pc = gc.oc, gc.pc


def _lib_meshes(case):
    return [oc.meshes()[mesh] for mesh, _ in gc.operator_cases()[case]]


# ---- 1. the operator against the reference in every launch shape -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gc.operator_cases()))
def test_operator_case_equals_the_reference_in_every_launch_shape(name):
    case = gc.operator_cases()[name]
    meshes = _lib_meshes(name)
    xs, qs = np.array([p[:3] for _, p in case]), np.array([p[3:] for _, p in case])
    cam = L.Camera(*pc.CAM)
    for kind in gc.DEPTHS:
        D, tb, want, counts, removed = gc.operator_expected(name, kind)
        for bands, vcache in gc.LAUNCH_SHAPES:
            got, n, rem = ops.pose_silhouettes_gated(cam, meshes, xs, qs, D, float(gc.TF), tb, bands, bool(vcache))
            what = (name, kind, bands, vcache)
            assert np.array_equal(got, want), what + (int((got != want).sum()),)
            assert np.array_equal(n, counts), what + (n.tolist(), counts.tolist())
            assert np.array_equal(rem, removed), what + (rem.tolist(), removed.tolist())


@pytest.mark.parametrize("name", ["centred", "touches_top", "cracker_box_front", "box_over_cache_front", "straddles_near_plane"])
def test_operator_with_nothing_to_remove_is_the_plain_silhouette(name):
    (mesh, p), = gc.operator_cases()[name]
    cam = L.Camera(*pc.CAM)
    D = np.zeros((pc.H, pc.W), np.float32)
    for bands, vcache in gc.LAUNCH_SHAPES:
        plain, count = ops.pose_silhouette(cam, oc.meshes()[mesh], p[:3], p[3:], bands, bool(vcache))
        got, n, rem = ops.pose_silhouettes_gated(cam, [oc.meshes()[mesh]], [p[:3]], [p[3:]], D, bands=bands, vertex_cache=bool(vcache))
        assert np.array_equal(got[0], plain) and n[0] == count and not rem.any()


def test_operator_at_640x480_draws_a_band_in_strips():
    """a third of the window's rows per strip: at 640 x 480 and one band the gated draw needs four strips where the plain one needs two"""
    cam = (640, 480, 600.0, 600.0, 320.0, 240.0)
    p = pc.pose([0.0, 0.0, 0.3], [1, 2, 3], 0.3)
    R = oc.render("box12", p, cam)
    assert (R > 0).mean() > 0.3
    D = np.where(R > 0, R, np.float32(0)).astype(np.float32)
    D[:, 300:340] = np.float32(0.1)
    D[100:140, :] = np.float32(gc.FAR)
    kept, front, behind = gc.gate(R, D, gc.TF, gc.TB)
    assert front.sum() > 1000 and behind.sum() > 1000 and kept.sum() > 10000
    for bands, vcache in gc.LAUNCH_SHAPES:
        got, n, rem = ops.pose_silhouettes_gated(L.Camera(*cam), [oc.meshes()["box12"]], [p[:3]], [p[3:]], D, float(gc.TF), float(gc.TB), bands, bool(vcache))
        assert np.array_equal(got[0] > 0, kept), (bands, int(((got[0] > 0) != kept).sum()))
        assert n[0] == kept.sum() and rem.tolist() == [[int(front.sum()), int(behind.sum())]]


# ---- the two-engine harness ------------------------------------------------------------------------------------------------
class Scenario:
    """What both engines are handed, per frame k and object i.  pose(k, i) -> (x, q) or None; delivered(k, i) -> a byte mask handed to
    BOTH engines or None; flow_ok(k, i): the frame brings its flow; depth(k, i): the depth image.  occlusion: the objects share scene
    0.  restart: (frame, object): both engines restart that slot before that frame, at the ground-truth pose of the frame, and the
    frame hands it no pose.  Engine A gets, where engine B draws, the mask the contract names."""

    def __init__(self, n_obj=3, fb=6, tf=float(gc.TF), tb=0.0, pose=None, delivered=None, flow_ok=None, depth=None, occlusion=False, restart=None):
        self.n_obj, self.fb, self.tf, self.tb, self.occlusion, self.restart = n_obj, fb, tf, tb, occlusion, restart
        self.streams = gc.streams(n_obj)
        base_pose = lambda k, i: util.frame_inputs(self.streams[i], k)[3]
        self.pose = pose or base_pose
        if restart:
            self.pose = lambda k, i: None if (k, i) == restart else (pose or base_pose)(k, i)
        self.delivered = delivered or (lambda k, i: None)
        self.flow_ok = flow_ok or (lambda k, i: True)
        self.depth = depth or (lambda k, i: gc.depth(i, k))

    def start(self, k, i):
        return self.restart[0] if self.restart and self.restart[1] == i and k >= self.restart[0] else 0

    def pose0(self, k, i):
        """the initial pose of the track frame k of object i belongs to (13 doubles)"""
        return ru.gt_mean(self.streams[i], k) if self.start(k, i) else np.array(synth.initial_pose_from_stream(self.streams[i]))

    def draws(self, k, i):
        return self.delivered(k, i) is None and (self.pose(k, i) is not None or k == self.start(k, i))

    def render(self, k, i):
        pose = self.pose(k, i)
        p = np.concatenate(pose) if pose is not None else self.pose0(k, i)[6:13]
        return gc.render_pose(i, np.ascontiguousarray(p, np.float64).tobytes())

    @functools.lru_cache(maxsize=None)
    def gated(self, k, i):
        """(kept, front, behind) of the pair the contract draws on frame k for object i"""
        s = self.start(k, i)
        g = gc.gate_frames(N_FRAMES, lambda f: self.delivered(f, i) is not None or self.draws(f, i), lambda f: f > 0 and self.flow_ok(f, i), self.fb, s)[k]
        R = self.render(k, i)
        own = R > 0
        if self.occlusion:
            members = [j for j in range(self.n_obj) if self.draws(k, j)]
            own = oc.resolve(np.stack([self.render(k, j) for j in members]))[1][members.index(i)]
        return gc.gate(R, self.depth(g, i), self.tf, self.tb, own)

    def reference_stats(self):
        pairs = [self.gated(k, i) for k in range(N_FRAMES) for i in range(self.n_obj) if self.draws(k, i)]
        return dict(gated=len(pairs), emptied=sum(bool((f | b).any() and not kp.any()) for kp, f, b in pairs),
                    pixels_front=int(sum(f.sum() for _, f, _ in pairs)), pixels_behind=int(sum(b.sum() for _, _, b in pairs)))

    def mask_a(self, k, i):
        m = self.delivered(k, i)
        if m is not None or not self.draws(k, i):
            return m
        return np.ascontiguousarray(self.gated(k, i)[0].astype(np.uint8) * 255)

    def frames(self, holder, k, engine):
        out = []
        for i, st in enumerate(self.streams):
            _, flow, _, _ = util.frame_inputs(st, k)
            f = dict(depth=holder.put(np.array(self.depth(k, i))), flow=holder.put(flow if self.flow_ok(k, i) else None), pose=self.pose(k, i), dt=st.dt,
                     mem_kind=holder.kind, mask=holder.put(self.mask_a(k, i) if engine == "A" else self.delivered(k, i)))
            out.append(f)
        return out


def _run(sc, engine, splits, mem="pageable", gate=True, per_step=None, refused_before=()):
    """engine "A": HOST masks; "B": enrolled, the gate on (gate=False: plain pose masks).  refused_before: frames in front of which a
    submit that is refused behind its first objects is made (frame by frame only).  Returns (log, final masks, stats, gate stats)."""
    holder = Holder(mem)
    eng = make_engine(list(sc.streams), max_batch_frames=8 if splits else 1, mask_frames_between=sc.fb)
    eng.enable_log(N_FRAMES)
    if engine == "B":
        eng.enable_pose_masks()
        if sc.occlusion:
            eng.enable_pose_mask_occlusion()
        if gate:
            eng.enable_pose_mask_depth_gate(sc.tf, sc.tb)
    k = i = 0
    while k < N_FRAMES:
        t = 1 if splits is None else min(splits[i % len(splits)], N_FRAMES - k)
        if sc.restart and k < sc.restart[0] < k + t:
            t = sc.restart[0] - k   # (a restart falls between two batches)
        i += 1
        if sc.restart and k == sc.restart[0]:
            d = E.default_object()
            for j, v in enumerate(sc.pose0(k, sc.restart[1])):
                d.p_mean0[j] = v
            eng.restart_objects([(sc.restart[1], d, None, None)], keep_mesh=True)
        if splits is None:
            if k in refused_before:
                # the last object hands a camera image to an engine without roft_engine_enable_flow: refused when the objects before it
                # have been scheduled -- history, flow count and gate image chosen
                poisoned = sc.frames(holder, k, engine)
                poisoned[-1] = dict(poisoned[-1], flow=None, image=np.zeros((pc.H, pc.W), np.uint8))
                with pytest.raises(L.RoftError):
                    eng.submit(poisoned)
            eng.submit(sc.frames(holder, k, engine))
        else:
            eng.submit_batch([sc.frames(holder, k + j, engine) for j in range(t)])
        eng.step()
        k += t
        if per_step:
            per_step(eng, k)
    out = _read_log(eng, N_FRAMES), [eng.mask(o) for o in range(sc.n_obj)], eng.stats(), eng.pose_mask_gate_stats()
    eng.close()
    return out


def _pair(sc, splits, mem="pageable"):
    """Engines A and B over the scenario, every object's mask compared after every step."""
    seen = {"A": [], "B": []}

    def keep(which):
        return lambda eng, k: seen[which].append([eng.mask(o) for o in range(sc.n_obj)])

    a = _run(sc, "A", splits, mem, per_step=keep("A"))
    b = _run(sc, "B", splits, mem, per_step=keep("B"))
    _assert_same(b[:3], a[:3], (splits, mem))
    assert len(seen["A"]) == len(seen["B"]) > 0
    for s, (ma, mb) in enumerate(zip(seen["A"], seen["B"])):
        for o in range(sc.n_obj):
            assert np.array_equal(ma[o], mb[o]), ("mask after step", s, "object", o, int((ma[o] != mb[o]).sum()))
    assert a[3] == dict(gated=0, emptied=0, pixels_front=0, pixels_behind=0)
    assert b[3] == sc.reference_stats(), (b[3], sc.reference_stats())
    assert (a[0]["npts"] > 0).any() and (a[0]["sel"] >= 0).any(), "the run tracks: flow points and outlier tests"
    return a, b


@pytest.fixture(scope="module", autouse=True)
def _conditions():
    """asserted on the CPU reference before any engine runs"""
    gc.check_conditions(4)


# ---- 2. engine parity, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mem", ["pageable", "device"])
@pytest.mark.parametrize("splits", [None, SPLITS], ids=["frame_by_frame", "splits_4_8_2"])
def test_engine_parity_with_gated_host_masks(splits, mem):
    sc = Scenario()
    a, b = _pair(sc, splits, mem)
    assert b[3]["gated"] == 9 and b[3]["pixels_front"] > 9 * 300 and b[3]["emptied"] == 0
    # the gate adds no launch and no event: what ungated pose masks cost against HOST masks (tests/test_pose_masks_gpu.py) -- one
    # launch more per delivering batch, three batches deliver
    assert b[2]["launches"] - a[2]["launches"] == 3
    assert b[2]["event_ops"] == a[2]["event_ops"]


@pytest.mark.parametrize("env", ["ROFT_ONE_STREAM=1", "ROFT_PREP_AHEAD=2", "ROFT_CTRL_INGEST=0"])
def test_engine_parity_under_the_scheduling_switches(env, monkeypatch):
    name, value = env.split("=")
    monkeypatch.setenv(name, value)
    _pair(Scenario(), SPLITS)
    _pair(Scenario(), None)


def test_behind_test_on_parity_and_counts():
    """the behind tolerance on: against the delivering frame's depth it would remove most of a delayed silhouette (the object has
    moved: background where it was); against the right frame it removes the few pixels the pose noise puts beside the object"""
    sc = Scenario(tb=float(gc.TB))
    a, b = _pair(sc, SPLITS)
    assert b[3]["pixels_behind"] > 0 and b[3]["pixels_front"] > 9 * 300


# ---- 4. the mode does something ------------------------------------------------------------------------------------------
def test_the_mode_changes_what_the_engine_computes():
    sc = Scenario()
    on = _run(sc, "B", SPLITS)
    off = _run(sc, "B", SPLITS, gate=False)
    assert off[3] == dict(gated=0, emptied=0, pixels_front=0, pixels_behind=0)
    assert on[3] == sc.reference_stats() and on[3]["pixels_front"] > 0
    assert any(not np.array_equal(x, y) for x, y in zip(on[1], off[1]))
    assert not np.array_equal(on[0]["npts"], off[0]["npts"])
    assert on[2]["launches"] == off[2]["launches"] and on[2]["event_ops"] == off[2]["event_ops"]


# ---- 5. edges ------------------------------------------------------------------------------------------------------------
def test_a_silhouette_the_gate_empties_is_ignored():
    """object 1's frame 6 lies behind a wall: its silhouette of frame 12 (gate frame 6) loses every pixel, and its mask goes on from
    the one before"""
    wall = np.full((pc.H, pc.W), np.float32(0.05))
    sc = Scenario(depth=lambda k, i: wall if (k, i) == (6, 1) else gc.depth(i, k))
    assert not sc.mask_a(12, 1).any() and sc.mask_a(6, 1).any() and sc.mask_a(12, 0).any()
    for splits in (None, SPLITS):
        a, b = _pair(sc, splits)
        assert b[3]["emptied"] == 1 and b[1][1].any()


def test_a_refused_submit_consumes_nothing():
    sc = Scenario()
    a = _run(sc, "A", None)
    b = _run(sc, "B", None, refused_before=(5, 6, 7, 12))
    _assert_same(b[:2] + (None,), a[:2] + (None,))
    assert b[3] == sc.reference_stats()


def test_a_delivered_mask_on_a_pose_frame_is_not_gated():
    st = gc.streams(3)[1]
    net = np.ascontiguousarray(st.mask_gt[0].numpy())
    sc = Scenario(delivered=lambda k, i: net if (k, i) == (6, 1) else None)
    assert gc.gate(gc.render_pose(1, np.ascontiguousarray(st.pose_meas[6], np.float64).tobytes()), gc.depth(1, 0))[1].sum() > 300
    a, b = _pair(sc, SPLITS)
    assert b[3]["gated"] == 8


def test_a_dropped_flow_frame_moves_the_gate_frame():
    """object 1 misses the flows of frames 1 and 7: its chases start on frames 1 and 7, not 0 and 6"""
    sc = Scenario(flow_ok=lambda k, i: not (i == 1 and k in (1, 7)))
    base = Scenario()
    for k in (6, 12):
        assert (sc.gated(k, 1)[0] != base.gated(k, 1)[0]).sum() >= 20, "the other frame's depth gives another mask"
        assert np.array_equal(sc.gated(k, 0)[0], base.gated(k, 0)[0])
    for splits in (None, SPLITS):
        _pair(sc, splits)


def test_all_buffered_flows_when_the_number_between_masks_is_unknown():
    sc = Scenario(fb=0)
    assert np.array_equal(sc.gated(12, 0)[0], Scenario().gated(12, 0)[0])   # six flows were buffered: the same gate frames
    R = sc.render(12, 0)   # (a count that is one too high -- the flow of the mask's own frame counted twice -- gates against frame 5)
    assert (gc.gate(R, gc.depth(0, 5))[0] != sc.gated(12, 0)[0]).sum() >= 20
    for splits in (None, SPLITS):
        _pair(sc, splits)


def test_a_restarted_slot_is_gated_like_a_new_engines_first_frame():
    sc = Scenario(restart=(8, 1))
    assert sc.draws(8, 1) and sc.gated(8, 1)[1].sum() > 100 and sc.gated(8, 1)[0].any()
    for splits in (None, SPLITS):
        a, b = _pair(sc, splits)
        assert b[3]["gated"] == 10


@pytest.mark.parametrize("splits", [None, SPLITS], ids=["frame_by_frame", "splits_4_8_2"])
def test_the_gate_with_occlusion_four_objects_in_one_scene(splits):
    sc = Scenario(n_obj=4, occlusion=True)
    hidden = sum(int(((sc.render(k, i) > 0) & ~(sc.gated(k, i)[0] | sc.gated(k, i)[1] | sc.gated(k, i)[2])).sum()) for k in gc.POSE_FRAMES for i in range(4))
    assert hidden > 1000, "the objects overlap: the resolve removes pixels before the gate does"
    a, b = _pair(sc, splits)
    assert b[3]["gated"] == 12 and b[3]["pixels_front"] > 0


def test_everything_on_flow_raw_depth_quality_and_the_gate():
    """camera images instead of flows, 16-bit depth, track quality, pose masks and the gate in one engine: D_g is the converted image"""
    n, scale = N_FRAMES, 0.001
    streams = [util.stream(1400 + i, n, scale=4, with_gray=True) for i in range(3)]
    grays = [[np.ascontiguousarray(st.gray[k].numpy()) for k in range(n)] for st in streams]
    raws = [[np.clip(np.rint(gc.depth(i, k) / scale), 0, 65535).astype(np.uint16) for k in range(n)] for i in range(3)]
    converted = lambda k, i: ops.depth_convert(raws[i][k], scale)
    assert not np.array_equal(converted(0, 0), gc.depth(0, 0)), "the converted image is not the float image it was made from"
    sc = Scenario(depth=converted)

    def run(engine):
        eng = make_engine(streams, max_batch_frames=8)
        eng.enable_flow()
        eng.enable_raw_depth(scale)
        eng.enable_log(40)
        eng.enable_quality()
        if engine == "B":
            eng.enable_pose_masks()
            eng.enable_pose_mask_depth_gate()
        k = 0
        for t in SPLITS:
            batch = []
            for j in range(t):
                kk = k + j
                batch.append([dict(depth=raws[i][kk], image=grays[i][kk], flow=None, pose=sc.pose(kk, i), dt=streams[i].dt,
                                   mask=sc.mask_a(kk, i) if engine == "A" else None) for i in range(3)])
            eng.submit_batch(batch)
            eng.step()
            k += t
        out = _read_log(eng, n), [eng.mask(o) for o in range(3)], eng.stats(), eng.quality(0, n), eng.pose_mask_gate_stats()
        eng.close()
        return out

    a, b = run("A"), run("B")
    _assert_same(b[:3], a[:3])
    assert a[3].tobytes() == b[3].tobytes()
    assert b[4] == sc.reference_stats() and b[4]["pixels_front"] > 9 * 300


def test_run_sequence_gates_the_silhouettes_of_a_directory(tmp_path, capsys):
    import importlib.util
    import json
    import os
    import shutil
    from roft_amd import io
    st = util.stream(1400, N_FRAMES, scale=4)
    root = str(tmp_path / "seq")
    mesh = io.write_sequence(root, st, "box", flow_set="analytic")
    shutil.rmtree(os.path.join(root, "masks"))
    spec = importlib.util.spec_from_file_location("run_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_sequence.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    common = ["--root", root, "--object", "box", "--mesh", mesh, "--flow-set", "analytic", "--masks-from-pose"]
    assert rs.main(common + ["--out", str(tmp_path / "g_"), "--pose-mask-depth-gate", "0.02,0.05"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["pose_masks"] == dict(silhouettes=3, frames=3)
    gs = report["pose_mask_gate"]
    assert gs["gated"] == 3 and gs["emptied"] == 0 and gs["front_tolerance"] == 0.02 and gs["behind_tolerance"] == 0.05
    assert rs.main(common + ["--out", str(tmp_path / "f_"), "--pose-mask-depth-gate", "0.02"]) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["pose_mask_gate"]["gated"] == 3 and report["pose_mask_gate"]["pixels_behind"] == 0
    with pytest.raises(SystemExit):
        rs.main(common[:-1] + ["--out", str(tmp_path / "x_"), "--pose-mask-depth-gate", "0.02"])   # not without --masks-from-pose


# ---- 6. refusals with a device -------------------------------------------------------------------------------------------
def test_refusals_with_a_device():
    lib = L.lib()
    streams = list(gc.streams(3))

    def code(eng, front=0.02, behind=0.0, null=False):
        g = L.PoseMaskGate(front, behind)
        rc = lib.roft_engine_enable_pose_mask_depth_gate(eng._h, None if null else C.byref(g))
        assert rc == 0 or len(lib.roft_last_error_string()) > 10
        return rc

    eng = make_engine(streams)
    assert code(eng) == -4 and b"roft_engine_enable_pose_masks" in lib.roft_last_error_string()   # pose masks are not enabled
    eng.enable_pose_masks()
    for front, behind in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.02, float("nan")), (0.02, float("inf"))):
        assert code(eng, front, behind) == -1, (front, behind)
    assert code(eng, null=True) == 0          # the defaults
    assert code(eng, 0.03, -1.0) == 0         # again, before the first frame: the last call holds
    assert eng.pose_mask_gate_stats() == dict(gated=0, emptied=0, pixels_front=0, pixels_behind=0)
    holder = Holder("pageable")
    sc = Scenario()
    eng.submit(sc.frames(holder, 0, "B"))
    assert code(eng) == -4                    # a frame is submitted
    eng.step()
    assert code(eng) == -4
    assert eng.pose_mask_gate_stats()["gated"] == 3
    eng.close()
