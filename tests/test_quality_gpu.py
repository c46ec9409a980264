"""Track quality on the GPU (roft_amd/csrc/k_quality.hip through roft_track_quality and the engine): every record bit for bit
against tests/quality_ref.py -- the seven counts as integers, depth_err as a double."""
import ctypes as C

import numpy as np
import pytest

import mesh_zoo
import pose_error_util as pe
import quality_ref as qr
import util
from roft_amd import _lib as L
from roft_amd import ops

pytestmark = pytest.mark.gpu

TOL, DMAX = 0.01, 2.0
Q0 = np.array([1.0, 0.0, 0.0, 0.0])
Q1 = np.array([0.9, 0.3, 0.2, 0.1]) / np.linalg.norm([0.9, 0.3, 0.2, 0.1])
POSES = {
    "inside": (np.array([0.01, -0.005, 0.5]), Q0),
    "inside_rotated": (np.array([-0.02, 0.01, 0.45]), Q1),
    "clipped_left_top": (np.array([-0.25, -0.18, 0.5]), Q0),
    "off_screen": (np.array([5.0, 0.0, 0.5]), Q0),
    "behind": (np.array([0.0, 0.0, -0.5]), Q0),
}
SMALL_SHAPES = [(128, 96, 4), (64, 64, 2), (64, 50, 4)]


def cameras(oracle, W, H):
    f = 0.9 * W
    return L.Camera(W, H, f, f, W / 2 - 0.5, H / 2 - 0.5), oracle.camera(W, H, f, f, W / 2 - 0.5, H / 2 - 0.5)


def scene(oracle, ocam, d, mesh, x, q, seed, mask_kind="random"):
    """A mask and a depth image for the pose: M a random subset of a rectangle around the silhouette plus pixels elsewhere (a few of
    value 1, which are not the object); D the render with millimetre noise, an occluder plane in front of a part of it, a band
    behind it, and invalid readings (0, NaN, >= depth_maximum, negative)."""
    H, W = ocam.height, ocam.width
    rng = np.random.default_rng(seed)
    tile = oracle.render_depth(oracle.make_mesh(*mesh), x, q, ocam, d)
    r = qr.upsample(tile, d, H, W)
    mask = np.zeros((H, W), np.uint8)
    if mask_kind == "random":
        vs, us = np.nonzero(r)
        if len(vs):
            v0, v1, u0, u1 = max(vs.min() - 3, 0), min(vs.max() + 4, H), max(us.min() - 3, 0), min(us.max() + 4, W)
        else:
            v0, v1, u0, u1 = H // 4, H // 2, W // 4, W // 2
        mask[v0:v1, u0:u1] = np.where(rng.random((v1 - v0, u1 - u0)) < 0.7, 255, 0)
        mask[rng.random((H, W)) < 0.02] = 255
        mask[rng.random((H, W)) < 0.01] = 1
    elif mask_kind == "full":
        mask[:] = 255
    elif mask_kind == "outside":   # only outside the render's window: the last pixel, a run across a 32-bit word boundary, the last rows
        mask[H - 1, W - 1] = 255
        mask[H - 1, 28:36] = 255
        mask[H - 2, 0] = 255
        mask[r != 0] = 0
    else:
        assert mask_kind == "empty"
    D = (r + rng.integers(-4, 5, (H, W)).astype(np.float32) * np.float32(0.001)).astype(np.float32)
    D[r == 0] = rng.uniform(0.3, 1.5, int((r == 0).sum())).astype(np.float32)
    D[:, : (9 * W) // 20] = np.float32(0.31)                # the occluder: in front of whatever lies in the left 45 % of the image
    D[H // 2: H // 2 + 3, :] += np.float32(0.05)            # a band behind
    bad = rng.random((H, W))
    D[bad < 0.03] = 0.0
    D[(bad >= 0.03) & (bad < 0.05)] = np.nan
    D[(bad >= 0.05) & (bad < 0.07)] = np.float32(DMAX)
    D[(bad >= 0.07) & (bad < 0.08)] = -0.5
    return tile, mask, D


def check(oracle, W, H, d, mesh, pose, seed, mask_kind="random", windows=(0,), expect=None):
    dcam, ocam = cameras(oracle, W, H)
    x, q = pose
    tile, mask, D = scene(oracle, ocam, d, mesh, x, q, seed, mask_kind)
    want = qr.quality_from_tile(tile, d, mask > 1, D, TOL, DMAX)
    for wp in windows:
        got = qr.as_dict(ops.track_quality(dcam, d, D, mask, ops.make_mesh(*mesh), x, q, TOL, DMAX, window_pixels=wp))
        print(W, H, d, mask_kind, wp, got, want)
        assert qr.same(got, want), (wp, got, want)
    if expect:
        expect(want, tile)
    return want, tile


def strips_of(tile, tile_w):
    """strips the kernel draws a window in when its LDS window is capped at one row of the target (window_pixels = 1)"""
    js, is_ = np.nonzero(tile)
    win_w, win_h = is_.max() - is_.min() + 1, js.max() - js.min() + 1
    rows = max(1, tile_w // win_w)
    return -(-win_h // rows)


@pytest.mark.parametrize("pose", list(POSES))
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_operator_poses_and_strips(oracle, shape, pose):
    """cached projection path (the box has 294 vertices); window_pixels 0 and 1 (one row of the target: strips) give the same bits"""
    W, H, d = shape

    def expect(want, tile):
        if pose in ("off_screen", "behind"):
            assert want["n_render"] == 0 and want["n_mask"] > 0 and want["depth_err"] == qr.DBL_MAX
        else:
            assert want["n_depth"] > 0 and want["n_both"] > want["n_depth"] and want["n_render"] > want["n_both"]
        if pose == "inside_rotated":
            assert strips_of(tile, W // d) >= 3   # (window_pixels = 1: the window of this pose is drawn in at least three strips)
        if pose in ("inside", "inside_rotated"):
            assert want["n_front"] > 0 and want["n_behind"] > 0
        if pose == "clipped_left_top":
            assert tile[0].any() and tile[:, 0].any()
        if H % d:
            assert want["n_mask"] > 0   # (rows H - H % d .. H - 1 lie outside the tile: they count for n_mask only)

    check(oracle, W, H, d, mesh_zoo.box(), POSES[pose], seed=11, windows=(0, 1), expect=expect)


@pytest.mark.parametrize("mask_kind", ["empty", "full", "outside"])
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "%dx%d_d%d" % s)
def test_operator_masks(oracle, shape, mask_kind):
    W, H, d = shape

    def expect(want, tile):
        assert want["n_render"] > 0
        if mask_kind == "empty":
            assert want["n_mask"] == 0 and want["n_both"] == 0
        if mask_kind == "full":
            assert want["n_mask"] == W * H and want["n_both"] == want["n_render"]
        if mask_kind == "outside":
            assert want["n_mask"] >= 8 and want["n_both"] == 0

    check(oracle, W, H, d, mesh_zoo.box(), POSES["inside"], seed=12, mask_kind=mask_kind, windows=(0, 1), expect=expect)


@pytest.mark.parametrize("name", ["box", "box_open", "box_reversed", "two_components"])
def test_operator_meshes(oracle, name):
    """closed (back faces culled), open (drawn whole), inside out, two components; cached projection path"""
    v, t, _ = mesh_zoo.zoo()[name]
    for pose in ("inside_rotated", "clipped_left_top"):
        check(oracle, 128, 96, 4, (v, t), POSES[pose], seed=13, windows=(0, 1))


def test_operator_mesh_beyond_the_vertex_cache(oracle):
    """per-triangle projection path: the projected vertices of this mesh do not fit the LDS next to a window"""
    v, t = mesh_zoo.box(n=44)
    assert len(v) * 12 + 4 * 8192 > 160 * 1024 - 4096
    want, _ = check(oracle, 128, 96, 4, (v, t), POSES["inside_rotated"], seed=14, windows=(0, 1))
    assert want["n_depth"] > 0


def test_operator_without_a_mesh(oracle):
    dcam, ocam = cameras(oracle, 64, 64)
    _, mask, D = scene(oracle, ocam, 2, mesh_zoo.box(), *POSES["inside"], seed=15)
    empty = L.Mesh(None, 0, None, 0)
    got = qr.as_dict(ops.track_quality(dcam, 2, D, mask, empty, *POSES["inside"], TOL, DMAX))
    want = qr.quality(oracle, ocam, 2, D, mask > 1, None, *POSES["inside"], TOL, DMAX)
    assert qr.same(got, want) and got["n_mask"] > 0 and got["n_render"] == 0


def test_operator_640x480(oracle):
    """the engine's full shape, once: 9 600 plane words, a window of ~ 90 x 115 tile pixels; cached projection path"""
    want, _ = check(oracle, 640, 480, 2, mesh_zoo.box(), POSES["inside_rotated"], seed=16, windows=(0, 320))
    assert want["n_depth"] > 1000 and want["n_front"] > 0 and want["n_behind"] > 0


# ---- engine ------------------------------------------------------------------------------------------------------------------
N, N_OBJ, D_ENGINE = 20, 3, 4


@pytest.fixture(scope="module")
def streams():
    sts = [util.stream(4200 + o, N, scale=2, device="cuda") for o in range(N_OBJ)]
    assert sts[0].camera.width == 320 and sts[0].camera.height == 240
    assert any(st.pose_valid[1:N].any() for st in sts)   # pose arrivals included
    return sts


def host_frame(st, k):
    depth, flow, mask, pose = util.frame_inputs(st, k)
    return dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST)


def raw_log(eng, first, n):
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, first, n, outs))
    return [(np.array(r.pose[:]).tobytes(), np.array(r.twist[:]).tobytes(), r.n_flow_points, r.outlier_selected, np.array(r.outlier_L[:]).tobytes())
            for r in outs]


def least_log(T):
    """frames that can be in flight: 6 one-frame batches, 5 batches of T frames otherwise"""
    return 6 if T == 1 else 5 * T


def run(streams, splits, dev=False, quality=True, every=1, log=None, n=N, per_frame=None):
    """The streams through an engine in batches of the sizes `splits` (cycled); HOST inputs, or DEVICE inputs (dev).  Returns
    (records [n, objects] or None, raw log rows, final masks).  per_frame(eng, k): called after every one-frame step."""
    T = max(splits)
    log = max(n, least_log(T)) if log is None else log
    src = [util.to_device(st) for st in streams] if dev else streams
    frame = util.device_frame if dev else host_frame
    eng = pe.make_engine(streams, max_batch_frames=T)
    eng.enable_log(log)
    if quality:
        eng.enable_quality(every=every, depth_tolerance=TOL)
    k = i = 0
    while k < n:
        t = min(splits[i % len(splits)], n - k)
        i += 1
        batch = [[frame(st, k + j) for st in src] for j in range(t)]
        if T == 1:
            eng.submit(batch[0])
        else:
            eng.submit_batch(batch)
        eng.step()
        k += t
        if per_frame:
            per_frame(eng, k - 1)
    first = max(0, n - log)
    rec = eng.quality(first, n - first) if quality else None
    out = (rec, raw_log(eng, first, n - first), [eng.mask(o) for o in range(len(streams))], eng)
    return out


@pytest.fixture(scope="module")
def base(streams, oracle):
    """One-frame submits: the per-frame masks, the log rows and the depths -- and the reference's records on them."""
    masks = {}

    def grab(eng, k):
        for o in range(N_OBJ):
            masks[(k, o)] = eng.mask(o)

    rec, log, final, eng = run(streams, [1], per_frame=grab)
    pose = eng.get_log(0, N)[0]
    dmax = eng.cfg.depth_maximum
    eng.close()
    want = []
    for k in range(N):
        for o, st in enumerate(streams):
            depth = util.frame_inputs(st, k)[0]
            want.append(qr.quality(oracle, util.oracle_camera(oracle, st.camera), D_ENGINE, depth, masks[(k, o)] != 0, st.mesh,
                                   pose[k, o, 6:9], pose[k, o, 9:13], TOL, dmax, frame=k))
    return dict(rec=rec, log=log, final=final, want=want)


def test_engine_records_equal_the_reference(base):
    rec = base["rec"].reshape(-1)
    assert len(rec) == N * N_OBJ
    for i, want in enumerate(base["want"]):
        assert qr.same(qr.as_dict(rec[i]), want), (i // N_OBJ, i % N_OBJ, qr.as_dict(rec[i]), want)
    # the run measured something: every count moves
    for f in ("n_mask", "n_render", "n_both", "n_depth"):
        assert (base["rec"][f][1:] > 0).all(), f
    iou = ops.quality_overlap(base["rec"])
    assert iou.shape == (N, N_OBJ) and np.nanmax(iou) > 0.5 and np.nanmax(iou) <= 1.0


@pytest.mark.parametrize("case", ["batches_of_8", "cuts_3_5_1_8_3", "device_inputs", "device_inputs_batches_of_8", "one_stream"])
def test_engine_same_records_in_every_batch_shape(streams, base, case, monkeypatch):
    if case == "one_stream":
        monkeypatch.setenv("ROFT_ONE_STREAM", "1")
    splits = {"batches_of_8": [8], "cuts_3_5_1_8_3": [3, 5, 1, 8, 3], "device_inputs": [1], "device_inputs_batches_of_8": [8], "one_stream": [8]}[case]
    rec, log, final, eng = run(streams, splits, dev=case.startswith("device"))
    eng.close()
    assert rec.tobytes() == base["rec"].tobytes()
    assert log == base["log"]
    for a, b in zip(final, base["final"]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("splits", [[1], [8]], ids=["T1", "T8"])
def test_engine_quality_changes_no_result(streams, base, splits):
    rec, log, final, eng = run(streams, splits, quality=False)
    with pytest.raises(L.RoftError, match="error -1"):
        eng.quality(0, 1)
    eng.close()
    assert log == base["log"]
    for a, b in zip(final, base["final"]):
        assert np.array_equal(a, b)


def test_engine_every_third_frame(streams, base):
    rec, _, _, eng = run(streams, [3, 5, 1, 8, 3], every=3)
    eng.close()
    none = qr.none_record()
    for k in range(N):
        for o in range(N_OBJ):
            got = qr.as_dict(rec[k, o])
            assert qr.same(got, qr.as_dict(base["rec"][k, o]) if k % 3 == 0 else none), (k, o, got)


def test_engine_raw_depth_scores_the_engines_product(streams, oracle):
    """16-bit depth in: the records are the reference's on eng.depth(obj), the float image the engine made on the device"""
    n, scale = 6, 0.001
    eng = pe.make_engine(streams, max_batch_frames=1)
    eng.enable_raw_depth(scale)
    eng.enable_log(n)
    eng.enable_quality(depth_tolerance=TOL)
    masks, depths, raws = {}, {}, []
    for k in range(n):
        frames = []
        for st in streams:
            f = host_frame(st, k)
            f["depth"] = np.clip(np.rint(f["depth"] / scale), 0, 65535).astype(np.uint16)
            raws.append(f["depth"])
            frames.append(f)
        eng.submit(frames)
        eng.step()
        for o in range(N_OBJ):
            masks[(k, o)], depths[(k, o)] = eng.mask(o), eng.depth(o)
    rec = eng.quality(0, n)
    pose = eng.get_log(0, n)[0]
    dmax = eng.cfg.depth_maximum
    eng.close()
    for k in range(n):
        for o, st in enumerate(streams):
            want = qr.quality(oracle, util.oracle_camera(oracle, st.camera), D_ENGINE, depths[(k, o)], masks[(k, o)] != 0, st.mesh,
                              pose[k, o, 6:9], pose[k, o, 9:13], TOL, dmax, frame=k)
            assert qr.same(qr.as_dict(rec[k, o]), want), (k, o)
    assert (rec["n_depth"][1:] > 0).all()


def test_engine_ring_of_the_least_capacity(streams, base):
    """batches of 2: five batches in flight x 2 frames = a log (and a quality ring) of 10 rows over 20 frames"""
    least = least_log(2)
    assert least == 10
    rec, log, _, eng = run(streams, [2], log=least)
    assert rec.tobytes() == base["rec"][N - least:].tobytes()
    # (pose, twist, flow points, decision: a frame without an outlier test leaves outlier_L of its log row as the row's last user
    #  left it, so in a ring that field is not a function of the frame)
    assert [r[:4] for r in log] == [r[:4] for r in base["log"][(N - least) * N_OBJ:]]
    assert eng.quality(N - 3, 3).tobytes() == base["rec"][N - 3:].tobytes()
    assert eng.quality(N - least, 0).shape == (0, N_OBJ)
    for first, n in ((N - least - 1, 2), (0, 1), (N - 2, 3), (N - least, least + 1), (-1, 1)):   # older, ahead, longer than the ring
        with pytest.raises(L.RoftError, match="error -1"):
            eng.quality(first, n)
        with pytest.raises(L.RoftError, match="error -1"):   # ... exactly the ranges the log's scorer refuses
            eng.score_log("add", 0, first, n, np.zeros((max(n, 0), 7)))
    eng.close()


def test_engine_refusals(streams):
    lib = L.lib()
    eng = pe.make_engine(streams, max_batch_frames=4)
    with pytest.raises(L.RoftError, match="error -4.*roft_engine_enable_log"):   # without a log
        eng.enable_quality()
    eng.enable_log(19)
    with pytest.raises(L.RoftError, match="error -1.*at least 20 frames"):       # 5 batches in flight x 4 frames
        eng.enable_quality()
    eng.enable_log(20)
    for bad in (L.QualityParams(0, 0.01), L.QualityParams(1, -1.0), L.QualityParams(1, float("nan"))):
        assert lib.roft_engine_enable_quality(eng._h, C.byref(bad)) == -1
    assert lib.roft_engine_enable_quality(eng._h, None) == 0                     # NULL: the defaults
    with pytest.raises(L.RoftError, match="error -4.*capacity"):                 # the ring's capacity is the log's
        eng.enable_log(24)
    eng.enable_log(20)
    with pytest.raises(L.RoftError, match="error -4"):                           # no launch so far
        eng.quality_kernel_ms()
    eng.submit_batch([[host_frame(st, k) for st in streams] for k in range(4)])
    eng.step()
    assert (eng.quality(0, 4)["frame"] == np.arange(4)[:, None]).all()
    assert 0.0 < eng.quality_kernel_ms() < 100.0
    with pytest.raises(L.RoftError, match="error -4.*before the first frame"):
        eng.enable_quality()
    eng.close()

    late = pe.make_engine(streams, max_batch_frames=1)
    late.enable_log(8)
    late.submit([host_frame(st, 0) for st in streams])
    late.step()
    with pytest.raises(L.RoftError, match="error -4.*before the first frame"):
        late.enable_quality()
    late.close()

    gl = pe.make_engine(streams, max_batch_frames=1, render_mode=L.RENDER_GL)
    gl.enable_log(8)
    with pytest.raises(L.RoftError, match="error -1.*ROFT_RENDER_GL"):
        gl.enable_quality()
    gl.close()


# ---- the sequence tool -------------------------------------------------------------------------------------------------------
def test_run_sequence_writes_one_quality_row_per_frame(tmp_path, capsys):
    """tools/run_sequence.py --quality FILE: the logs are those of a run without it, byte for byte, and FILE holds one row per frame
    whose counts hang together."""
    import importlib.util
    import os
    from roft_amd import io, synth
    n = 10
    st = util.stream(4290, n, scale=4)                      # 160 x 120
    root = str(tmp_path / "seq")
    mesh = io.write_sequence(root, st, "box", flow_set="analytic")
    spec = importlib.util.spec_from_file_location("run_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_sequence.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    m0 = synth.initial_pose_from_stream(st)
    common = ["--root", root, "--object", "box", "--mesh", mesh, "--flow-set", "analytic", "--mask-set", "gt", "--init-pose"] + ["%.17g" % v for v in m0[6:13]]
    qfile = str(tmp_path / "quality.txt")
    assert rs.main(common + ["--out", str(tmp_path / "a_")]) == 0
    assert rs.main(common + ["--out", str(tmp_path / "b_"), "--quality", qfile]) == 0
    capsys.readouterr()
    for name in ("pose_estimate", "velocity_estimate"):
        assert open(str(tmp_path / ("a_" + name)), "rb").read() == open(str(tmp_path / ("b_" + name)), "rb").read()
    lines = open(qfile).read().splitlines()
    assert lines[0].startswith("# frame n_mask n_render n_both n_depth n_front n_behind depth_err overlap") and len(lines) == n + 1
    rows = np.array([[float(v) for v in line.split()] for line in lines[1:]])
    assert np.array_equal(rows[:, 0], np.arange(n))
    assert (rows[:, 3] <= np.minimum(rows[:, 1], rows[:, 2])).all() and (rows[:, 4] <= rows[:, 3]).all() and (rows[:, 5] + rows[:, 6] <= rows[:, 4]).all()
    assert (rows[:, 2] > 0).all() and (rows[1:, 8] > 0).any()
