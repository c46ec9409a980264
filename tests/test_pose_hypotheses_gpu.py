"""Pose hypotheses on the GPU (roft_amd/csrc/k_hypotheses.hip through roft_pose_hypotheses_score and roft_engine_score_hypotheses;
include/roft_engine.h, section 3j).  Every comparison is bit for bit -- the eight integers, depth_err as a double -- against
tests/quality_ref.py, against ops.track_quality, and between the operator and the engine entry; the searches reproduce the traces
and poses of the CPU reference (tests/golden/relocalise_traces.json)."""
import numpy as np
import pytest

import mesh_zoo
import pose_error_util as pe
import quality_ref as qr
import relocalise_cases as rc
import util
from roft_amd import _lib as L
from roft_amd import engine as E
from roft_amd import ops, relocalise, synth
from test_quality_gpu import DMAX, POSES, SMALL_SHAPES, TOL, cameras, host_frame, scene

pytestmark = pytest.mark.gpu

NAN_POSE = np.array([0.01, np.nan, 0.5, 1.0, 0.0, 0.0, 0.0])


def row(pose):
    return np.concatenate([pose[0], pose[1]])


def five_poses():
    return np.array([row(POSES[k]) for k in POSES])


def reference(oracle, ocam, d, D, mask, mesh, poses, frame=0, dmax=DMAX):
    return [qr.quality(oracle, ocam, d, D, mask > 1, mesh, p[:3], p[3:], TOL, dmax, frame=frame) for p in poses]


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert qr.same(qr.as_dict(g), w if isinstance(w, dict) else qr.as_dict(w)), (what, i, qr.as_dict(g), w)


def assert_draws_nothing(rec, n_mask):
    g = qr.as_dict(rec)
    assert g == dict(frame=g["frame"], n_mask=n_mask, n_render=0, n_both=0, n_depth=0, n_front=0, n_behind=0, reserved=0, depth_err=qr.DBL_MAX), g


# ---- operator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_operator_poses_windows_nan_and_duplicate(oracle, shape):
    """the five kinds of pose, a NaN pose and a duplicated pose in one call; window_pixels 0 and 1 (strips); against the reference and
    against roft_track_quality"""
    W, H, d = shape
    dcam, ocam = cameras(oracle, W, H)
    mesh = mesh_zoo.box()
    _, mask, D = scene(oracle, ocam, d, mesh, *POSES["inside_rotated"], seed=21)
    poses = np.vstack([five_poses(), NAN_POSE, row(POSES["inside_rotated"])])
    want = reference(oracle, ocam, d, D, mask, mesh, five_poses())
    assert want[1]["n_front"] > 0 and want[1]["n_behind"] > 0 and want[2]["n_render"] > 0 and want[3]["n_render"] == 0 and want[4]["n_render"] == 0
    dmesh = ops.make_mesh(*mesh)
    single = [ops.track_quality(dcam, d, D, mask, dmesh, p[:3], p[3:], TOL, DMAX) for p in five_poses()]
    assert_same(single, want, "track_quality")
    for wp in (0, 1):
        got = ops.pose_hypotheses_score(dcam, d, D, mask, dmesh, poses, TOL, DMAX, window_pixels=wp)
        assert_same(got[:5], want, wp)
        assert got[:5].tobytes() == np.array(single).tobytes()
        assert_draws_nothing(got[5], want[0]["n_mask"])
        assert got[6].tobytes() == got[1].tobytes()
    for bad in ([np.inf, 0, 0.5, 1, 0, 0, 0], [0, 0, 0.5, 1, 0, -np.inf, 0], [0, 0, 0.5, np.nan, 0, 0, 0]):
        assert_draws_nothing(ops.pose_hypotheses_score(dcam, d, D, mask, dmesh, [bad], TOL, DMAX)[0], want[0]["n_mask"])


@pytest.fixture(scope="module")
def many(oracle):
    """300 poses around one scene at 64 x 64, divider 2, with their reference records (computed once)"""
    dcam, ocam = cameras(oracle, 64, 64)
    mesh = mesh_zoo.box()
    x, q = POSES["inside_rotated"]
    _, mask, D = scene(oracle, ocam, 2, mesh, x, q, seed=22)
    rng = np.random.default_rng(23)
    poses = np.zeros((300, 7))
    poses[:, :3] = x + rng.uniform(-0.03, 0.03, (300, 3))
    quats = q + rng.uniform(-0.15, 0.15, (300, 4))
    poses[:, 3:] = quats / np.linalg.norm(quats, axis=1)[:, None]
    want = reference(oracle, ocam, 2, D, mask, mesh, poses)
    assert len({(w["n_render"], w["n_both"], w["n_front"]) for w in want}) > 250
    return dict(dcam=dcam, mesh=ops.make_mesh(*mesh), keep=mesh, mask=mask, D=D, poses=poses, want=want)


@pytest.mark.parametrize("n", [1, 7, 70, 300])
def test_operator_n(many, n):
    """1, 7, 70 (more than one wave of hypotheses, were they packed) and 300 (more workgroups than CUs)"""
    m = many
    got = ops.pose_hypotheses_score(m["dcam"], 2, m["D"], m["mask"], m["mesh"], m["poses"][:n], TOL, DMAX)
    assert_same(got, m["want"][:n])


def test_operator_independence(many):
    """the record of a pose in a call of 70 = alone = in a permuted call = next to a NaN pose"""
    m = many
    score = lambda p: ops.pose_hypotheses_score(m["dcam"], 2, m["D"], m["mask"], m["mesh"], p, TOL, DMAX)
    P = m["poses"][:70]
    base = score(P)
    for i in (0, 33, 69):
        assert score(P[i:i + 1]).tobytes() == base[i:i + 1].tobytes()
    perm = np.random.default_rng(24).permutation(70)
    assert score(P[perm]).tobytes() == base[perm].tobytes()
    with_nan = np.insert(P, 10, NAN_POSE, axis=0)
    got = score(with_nan)
    assert np.delete(got, 10).tobytes() == base.tobytes()
    assert_draws_nothing(got[10], int(base["n_mask"][0]))


def test_operator_mesh_beyond_the_vertex_cache(oracle):
    """per-triangle projection path: the projected vertices of this mesh do not fit the LDS next to a window"""
    v, t = mesh_zoo.box(n=44)
    assert len(v) * 12 + 4 * 8192 > 160 * 1024 - 4096
    dcam, ocam = cameras(oracle, 128, 96)
    _, mask, D = scene(oracle, ocam, 4, (v, t), *POSES["inside_rotated"], seed=25)
    poses = five_poses()[:3]
    want = reference(oracle, ocam, 4, D, mask, (v, t), poses)
    assert want[1]["n_depth"] > 0
    for wp in (0, 1):
        assert_same(ops.pose_hypotheses_score(dcam, 4, D, mask, ops.make_mesh(v, t), poses, TOL, DMAX, window_pixels=wp), want, wp)


def test_operator_mesh_of_no_triangles(oracle):
    dcam, ocam = cameras(oracle, 64, 64)
    _, mask, D = scene(oracle, ocam, 2, mesh_zoo.box(), *POSES["inside"], seed=26)
    empty = L.Mesh(None, 0, None, 0)
    poses = np.vstack([five_poses(), NAN_POSE])
    got = ops.pose_hypotheses_score(dcam, 2, D, mask, empty, poses, TOL, DMAX)
    want = reference(oracle, ocam, 2, D, mask, None, five_poses())
    assert_same(got[:5], want)
    assert want[0]["n_mask"] > 0
    for g in got:
        assert_draws_nothing(g, want[0]["n_mask"])
    assert got[0].tobytes() == ops.track_quality(dcam, 2, D, mask, empty, *POSES["inside"], TOL, DMAX).tobytes()


@pytest.mark.parametrize("mask_kind", ["empty", "full", "outside"])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_operator_masks(oracle, shape, mask_kind):
    W, H, d = shape
    dcam, ocam = cameras(oracle, W, H)
    mesh = mesh_zoo.box()
    _, mask, D = scene(oracle, ocam, d, mesh, *POSES["inside"], seed=27, mask_kind=mask_kind)
    want = reference(oracle, ocam, d, D, mask, mesh, five_poses())
    assert want[0]["n_render"] > 0 and want[0]["n_mask"] == {"empty": 0, "full": W * H}.get(mask_kind, want[0]["n_mask"])
    if mask_kind == "outside":
        assert want[0]["n_mask"] >= 8 and want[0]["n_both"] == 0
    for wp in (0, 1):
        assert_same(ops.pose_hypotheses_score(dcam, d, D, mask, ops.make_mesh(*mesh), five_poses(), TOL, DMAX, window_pixels=wp), want, wp)


def test_operator_more_than_one_chunk(many):
    """65 536 poses are one launch; one more is a second chunk: the same bits in every position (zero-triangle mesh: a quick launch)"""
    m = many
    n = (1 << 16) + 3
    poses = np.tile(m["poses"][:1], (n, 1))
    got = ops.pose_hypotheses_score(m["dcam"], 2, m["D"], m["mask"], L.Mesh(None, 0, None, 0), poses, TOL, DMAX)
    assert got.shape == (n,) and (got == got[0]).all() and got[0]["n_mask"] == m["want"][0]["n_mask"] and got[0]["frame"] == 0


# ---- engine -----------------------------------------------------------------------------------------------------------------------
N, N_OBJ, D_ENGINE = 9, 2, 4


@pytest.fixture(scope="module")
def streams():
    sts = [util.stream(1400 + o, N, scale=4) for o in range(N_OBJ)]
    assert sts[0].camera.width == 160 and sts[0].camera.height == 120
    assert any(st.mask_delivery[k] >= 0 for st in sts for k in range(1, N)) and any(st.pose_valid[1:N].any() for st in sts)
    return sts


def neighbourhood(x, q):
    """the estimate itself, then its compass candidates at two step sizes"""
    return np.vstack([np.concatenate([x, q])[None], relocalise.compass_candidates(x, q, 0.008, np.radians(4.0))[1:],
                      relocalise.compass_candidates(x, q, 0.03, np.radians(15.0))[1:]])


def run_engine(streams, score_every_batch, raw_depth=False, quality=True):
    """one-frame batches; returns per-frame masks, final log rows, quality records and the engine (open)"""
    eng = pe.make_engine(streams, max_batch_frames=1)
    if raw_depth:
        eng.enable_raw_depth(0.001)
    eng.enable_log(N)
    if quality:
        eng.enable_quality(depth_tolerance=TOL)
    masks, scored = {}, {}
    for k in range(N):
        frames = [host_frame(st, k) for st in streams]
        if raw_depth:
            for f in frames:
                f["depth"] = np.clip(np.rint(f["depth"] / 0.001), 0, 65535).astype(np.uint16)
        eng.submit(frames)
        eng.step()
        if score_every_batch:
            for o in range(N_OBJ):
                est = eng.get_log(k, 1)[0][0, o]
                scored[(k, o)] = eng.score_hypotheses(o, neighbourhood(est[6:9], est[9:13]), TOL)
        for o in range(N_OBJ):
            masks[(k, o)] = eng.mask(o)
    outs = (L.ObjectOutput * (N * N_OBJ))()
    L.check(L.lib().roft_engine_get_log(eng._h, 0, N, outs))
    return dict(eng=eng, masks=masks, scored=scored, log=bytes(outs), rec=eng.quality(0, N) if quality else None)


@pytest.fixture(scope="module")
def scoring(streams):
    r = run_engine(streams, True)
    yield r
    r["eng"].close()


def engine_camera(eng):
    c = eng.cfg.cam
    return L.Camera(c.width, c.height, c.fx, c.fy, c.cx, c.cy)


def test_engine_equals_the_operator_and_the_reference(streams, scoring, oracle):
    eng = scoring["eng"]
    pose = eng.get_log(N - 1, 1)[0][0]
    for o, st in enumerate(streams):
        P = np.vstack([neighbourhood(pose[o, 6:9], pose[o, 9:13]), NAN_POSE])
        got = eng.score_hypotheses(o, P, TOL)
        assert (got["frame"] == N - 1).all()
        depth, mask = util.frame_inputs(st, N - 1)[0], eng.mask(o)
        want = ops.pose_hypotheses_score(engine_camera(eng), D_ENGINE, depth, np.where(mask != 0, 255, 0).astype(np.uint8), ops.make_mesh(*st.mesh), P,
                                         TOL, eng.cfg.depth_maximum)
        want["frame"] = N - 1
        assert got.tobytes() == want.tobytes()
        ref = reference(oracle, util.oracle_camera(oracle, st.camera), D_ENGINE, depth, np.where(mask != 0, 255, 0), st.mesh, P[:-1], frame=N - 1,
                        dmax=eng.cfg.depth_maximum)
        assert_same(got[:-1], ref)
        assert got["n_render"][0] > 0 and got["n_both"][0] > 0 and got["n_depth"][0] > 0
        assert len({g.tobytes() for g in got}) > 20            # the neighbours are scored differently


def test_engine_entry_for_the_estimate_is_the_engines_own_record(scoring):
    """track quality enabled: hypothesis 0 of every frame was the frame's estimate"""
    for (k, o), got in scoring["scored"].items():
        assert got[0].tobytes() == scoring["rec"][k, o].tobytes(), (k, o)
    assert (scoring["rec"]["n_depth"][1:] > 0).all()


def test_engine_scoring_changes_no_output(streams, scoring):
    plain = run_engine(streams, False)
    plain["eng"].close()
    assert plain["log"] == scoring["log"]
    assert plain["rec"].tobytes() == scoring["rec"].tobytes()
    for key, m in plain["masks"].items():
        assert np.array_equal(m, scoring["masks"][key]), key


def test_engine_needs_neither_log_nor_quality(streams):
    eng = pe.make_engine(streams, max_batch_frames=1)
    for k in range(2):
        eng.submit([host_frame(st, k) for st in streams])
        eng.step()
    P = neighbourhood(*POSES["inside"])[:5]
    got = eng.score_hypotheses(1, P, TOL)
    depth, mask = util.frame_inputs(streams[1], 1)[0], eng.mask(1)
    want = ops.pose_hypotheses_score(engine_camera(eng), D_ENGINE, depth, np.where(mask != 0, 255, 0).astype(np.uint8), ops.make_mesh(*streams[1].mesh),
                                     P, TOL, eng.cfg.depth_maximum)
    want["frame"] = 1
    eng.close()
    assert got.tobytes() == want.tobytes()


def test_engine_object_without_a_mesh_has_no_render(streams):
    """R = 0, as in section 3d: the records count the mask alone, and equal the operator's for a mesh of no triangles"""
    st0 = streams[0]
    cfg = E.default_config(st0.camera.width, st0.camera.height, st0.flow_type, max_objects=2)
    c = st0.camera
    cfg.cam.fx, cfg.cam.fy, cfg.cam.cx, cfg.cam.cy = c.fx, c.fy, c.cx, c.cy
    cfg.flow_grid, cfg.flow_scale = st0.flow_grid, st0.flow_scale
    cfg.outlier_rejection = 0                                         # (the outlier test needs a mesh)
    eng = E.ROFTFilterBatch(cfg)
    for o, st in enumerate(streams):
        d = E.default_object()
        m0 = synth.initial_pose_from_stream(st)
        for i in range(13):
            d.p_mean0[i] = m0[i]
        eng.add_object(d, *(st.mesh if o == 0 else (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))))
    for k in range(2):
        eng.submit([host_frame(st, k) for st in streams])
        eng.step()
    P = np.vstack([neighbourhood(*POSES["inside"])[:4], NAN_POSE])
    got = eng.score_hypotheses(1, P, TOL)
    mask = eng.mask(1)
    want = ops.pose_hypotheses_score(engine_camera(eng), D_ENGINE, util.frame_inputs(streams[1], 1)[0], np.where(mask != 0, 255, 0).astype(np.uint8),
                                     L.Mesh(None, 0, None, 0), P, TOL, eng.cfg.depth_maximum)
    want["frame"] = 1
    assert got.tobytes() == want.tobytes() and int((mask != 0).sum()) > 0
    for g in got:
        assert_draws_nothing(g, int((mask != 0).sum()))
    assert eng.score_hypotheses(0, P, TOL)["n_render"][0] > 0        # its neighbour has one
    eng.close()


def test_engine_raw_depth_scores_the_engines_product(streams):
    """Z16 frames, align 0: D is what roft_engine_get_depth returns"""
    r = run_engine(streams, False, raw_depth=True)
    eng = r["eng"]
    pose = eng.get_log(N - 1, 1)[0][0]
    for o, st in enumerate(streams):
        P = neighbourhood(pose[o, 6:9], pose[o, 9:13])
        got = eng.score_hypotheses(o, P, TOL)
        want = ops.pose_hypotheses_score(engine_camera(eng), D_ENGINE, eng.depth(o), np.where(eng.mask(o) != 0, 255, 0).astype(np.uint8),
                                         ops.make_mesh(*st.mesh), P, TOL, eng.cfg.depth_maximum)
        want["frame"] = N - 1
        assert got.tobytes() == want.tobytes() and got["n_depth"][0] > 0
        assert got[0].tobytes() == r["rec"][N - 1, o].tobytes()
    eng.close()


def test_engine_refusals(streams):
    lib = L.lib()
    P = neighbourhood(*POSES["inside"])[:3]
    out = (L.QualityRecord * 3)()
    call = lambda eng, obj=0, poses=P.ctypes.data, n=3, tol=0.01, o=out: lib.roft_engine_score_hypotheses(eng._h, obj, poses, n, tol, o)
    eng = pe.make_engine(streams, max_batch_frames=1)
    assert call(eng) == L.ERR_STATE                              # nothing stepped
    eng.submit([host_frame(st, 0) for st in streams])
    assert call(eng) == L.ERR_STATE                              # submitted, not stepped
    eng.step()
    assert call(eng) == 0
    for kw in (dict(obj=-1), dict(obj=N_OBJ), dict(n=-1), dict(n=(1 << 20) + 1), dict(tol=-1.0), dict(tol=float("nan")), dict(poses=None), dict(o=None)):
        assert call(eng, **kw) == L.ERR_INVALID, kw
    assert call(eng, n=0, poses=None, o=None) == 0
    eng.submit([host_frame(st, 1) for st in streams])
    assert call(eng) == L.ERR_STATE                              # a submitted batch that has not been stepped
    with pytest.raises(L.RoftError, match="error -4"):
        eng.mask(0)                                              # ... exactly where roft_get_mask refuses
    eng.step()
    d = E.default_object()
    eng.restart_objects([(1, d, None, None)], keep_mesh=True)
    assert call(eng, obj=1) == L.ERR_STATE and call(eng, obj=0) == 0   # the restarted slot before its next step; its neighbour
    with pytest.raises(L.RoftError, match="error -4"):
        eng.mask(1)
    eng.close()
    gl = pe.make_engine(streams, max_batch_frames=1, render_mode=L.RENDER_GL)
    gl.submit([host_frame(st, 0) for st in streams])
    gl.step()
    with pytest.raises(L.RoftError, match="error -1.*ROFT_RENDER_GL"):
        gl.score_hypotheses(0, P)
    gl.close()


# ---- search -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_compass_search_over_the_operator_reproduces_the_reference(oracle, name):
    mask, depth = rc.scene(oracle, name)
    dcam, _ = rc.cameras(oracle)
    dmesh = ops.make_mesh(*mesh_zoo.box())
    x, q, trace = relocalise.compass_search(lambda p: ops.pose_hypotheses_score(dcam, rc.D, depth, mask, dmesh, p, rc.TOL, rc.DMAX), *rc.start_pose(name))
    gold = rc.golden()[name]
    assert [list(t) for t in trace] == gold["trace"]
    assert [float.hex(float(v)) for v in x] == gold["x"] and [float.hex(float(v)) for v in q] == gold["q"]


def test_relocalise_on_the_engine_reproduces_a_cpu_run(streams, scoring, oracle):
    eng = scoring["eng"]
    pose = eng.get_log(N - 1, 1)[0][0]
    for o, st in enumerate(streams):
        x0 = pose[o, 6:9] + np.array([0.010, -0.008, 0.012])
        q0 = relocalise.quat_mul(rc.turn([1, 2, -1], 8.0), pose[o, 9:13])
        x, q, trace = eng.relocalise(o, x0, q0, depth_tolerance=TOL)
        score = rc.cpu_scorer(oracle, util.oracle_camera(oracle, st.camera), D_ENGINE, util.frame_inputs(st, N - 1)[0], eng.mask(o) != 0, st.mesh,
                              TOL, eng.cfg.depth_maximum, frame=N - 1)
        xr, qr_, trace_r = relocalise.compass_search(score, x0, q0)
        assert trace == trace_r and x.tobytes() == xr.tobytes() and q.tobytes() == qr_.tobytes()
        assert len(trace) > 3 and trace[-1][1] < trace[0][1]
