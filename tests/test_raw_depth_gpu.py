"""Raw sensor depth on the device (include/roft_engine.h section 3c; k_depth.hip, engine_submit.hip).

Operators: roft_depth_convert and roft_depth_align against the numpy restatement of the contract (tests/depth_ref.py), EQUAL bits.
Shapes: 37 x 5 (a tail, an odd row length), 64 x 48, 640 x 480 for the conversion; for the alignment the restatement's own cases
(48 x 40 -> 64 x 48: more than one workgroup column is not needed to go wrong, a partial 64 x 4 tile is) plus one 424 x 240 ->
640 x 480 frame with a 15 mm baseline.

Engine: an engine with enable_raw_depth behaves, bit for bit, as if inputs[].depth had been a HOST float image holding the
operator's output.  So every test runs the SAME engine twice on util.stream(..., scale=2) -- 320 x 240, two objects on one shared
scene, raw frames made by quantising its depth to millimetres -- once fed the floats, once the 16-bit frames, and asks for equal
logs (poses, twists, flow point counts, outlier decisions and likelihoods), equal masks and get_depth equal to the operator."""
import ctypes as C

import numpy as np
import pytest

from roft_amd import _lib as L
from roft_amd import ops

import depth_ref as D
import util
from pose_error_util import make_engine

pytestmark = pytest.mark.gpu

SCALE = 0.001
HO3D_SCALE = 0.00012498664727900177


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, "%d of %d pixels differ, first at %s: %r != %r" % (len(bad), got.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def gpu_align(case):
    return ops.depth_align(case["raw"], case["dcam"], case["ccam"], case["scale"], case["R"], case["t"])


# ---- operators: convert -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [SCALE, HO3D_SCALE], ids=["mm", "ho3d"])
@pytest.mark.parametrize("shape", [(5, 37), (48, 64), (480, 640), (1, 1), (3, 7)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_convert_equals_the_restatement(shape, scale):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    raw = rng.integers(0, 65536, shape, dtype=np.uint16)
    raw.reshape(-1)[:3] = [0, 1, 65535][:raw.size]
    raw.reshape(-1)[-1] = 65535 if raw.size > 3 else raw.reshape(-1)[-1]      # (the last reading: the tail's last thread)
    got = ops.depth_convert(raw, scale)
    same_bits(got, D.convert(raw, scale))
    assert not got[raw == 0].any()


# ---- operators: align -------------------------------------------------------------------------------------------------------------
def test_align_general_case():
    case = D.general_case()
    counts = {}
    want = D.run(case, counts)
    assert counts["multiply"] > 0 and counts["uncovered"] > 0 and counts["offscreen"] > 0
    same_bits(gpu_align(case), want)


@pytest.mark.parametrize("shape", [(37, 5), (64, 48)], ids=lambda s: "%dx%d" % s)
def test_align_identity_equals_convert(shape):
    case = D.identity_case(*shape)
    got = gpu_align(case)
    same_bits(got, ops.depth_convert(case["raw"], case["scale"]))
    same_bits(got, D.run(case))


def test_align_times_two():
    case = D.times_two_case()
    got = gpu_align(case)
    same_bits(got, D.run(case))
    same_bits(np.ascontiguousarray(got[1:49, 1:65]), np.repeat(np.repeat(D.convert(case["raw"], case["scale"]), 2, 0), 2, 1))


def test_align_behind_the_camera():
    case = D.general_case(t=(0.015, 0.002, -1.0))
    counts = {}
    want = D.run(case, counts)
    assert counts["behind"] > 0
    same_bits(gpu_align(case), want)


def test_align_span_cap():
    case = D.general_case(f_colour=60 * 40.0)
    counts = {}
    want = D.run(case, counts)
    assert counts["capped"] > 0
    same_bits(gpu_align(case), want)


def test_align_all_zero_frame():
    case = D.general_case()
    case["raw"] = np.zeros_like(case["raw"])
    got = gpu_align(case)
    assert got.shape == (48, 64) and not _bits(got).any()


def test_align_424x240_into_640x480_and_twice_the_same_bits():
    dcam = D.Cam(424, 240, 212.0, 212.0, 211.5, 119.5)
    ccam = D.Cam(640, 480, 610.0, 610.0, 319.5, 239.5)
    case = dict(raw=D.block_frame(424, 240, SCALE, seed=5), scale=SCALE, dcam=dcam, ccam=ccam, R=D.rot_y(0.3), t=np.array([0.015, 0.0, 0.0]))
    counts = {}
    want = D.run(case, counts)
    assert counts["multiply"] > 0 and counts["uncovered"] > 0 and counts["offscreen"] > 0
    got = gpu_align(case)
    same_bits(got, want)
    same_bits(gpu_align(case), got)          # an integer minimum: no order, no run changes a bit


# ---- engine -----------------------------------------------------------------------------------------------------------------------
W, H = 320, 240
_cache = {}


N_STREAM = 36      # one stream length for every test: the stream is generated once


def _stream(seed, n=N_STREAM):
    assert n <= N_STREAM
    return util.stream(seed, N_STREAM, scale=2, with_gray=True)


def _raw(st, k):
    """frame k's 16-bit frame: ONE array per stream and image, so that the objects of a shared scene name one host pointer"""
    key = ("raw", id(st))
    if key not in _cache:
        _cache[key] = [np.clip(np.rint(st.depth[i].numpy() / SCALE), 0, 65535).astype(np.uint16) for i in range(st.n_frames)]
    return _cache[key][st.image(k)]


DCAM_W, DCAM_H = 160, 120


def _depth_camera(st):
    """a 160 x 120 depth camera in front of the 320 x 240 engine: half the colour camera's focal lengths"""
    c = st.camera
    return D.Cam(DCAM_W, DCAM_H, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5)


ALIGN_R, ALIGN_T = D.rot_y(0.2), np.array([0.004, 0.001, -0.0005])


def _raw_small(st, k):
    key = ("small", id(st))
    if key not in _cache:
        _cache[key] = [np.ascontiguousarray(_raw(st, j)[::2, ::2]) for j in range(st.n_frames)]
    return _cache[key][st.image(k)]


def _float_depth(st, k, align):
    """what the specification says the engine must behave as if it had been handed: the operator's output, computed once"""
    key = ("float", id(st), align, k)
    if key not in _cache:
        _cache[key] = (ops.depth_align(_raw_small(st, k), _depth_camera(st), st.camera, SCALE, ALIGN_R, ALIGN_T) if align
                       else ops.depth_convert(_raw(st, k), SCALE))
    return _cache[key]


def _gray(st, k):
    key = ("gray", id(st))
    if key not in _cache:
        _cache[key] = [np.ascontiguousarray(st.gray[i].numpy()) for i in range(st.n_frames)]
    return _cache[key][st.image(k)]


def _labels(st, k):
    """the label image of the frame's delivered mask (value 3 where the object is), or None"""
    mi = st.mask_delivery[k]
    if mi < 0:
        return None
    key = ("labels", id(st), int(mi))
    if key not in _cache:
        _cache[key] = np.where(st.mask_gt[mi].numpy() > 0, 3, 0).astype(np.uint8)
    return _cache[key]


def _full_log(eng, n):
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, 0, n, outs))
    rows = [(np.array(r.pose[:]).tobytes(), np.array(r.twist[:]).tobytes(), r.n_flow_points, r.outlier_selected, np.array(r.outlier_L[:]).tobytes())
            for r in outs]
    return [rows[f * eng.n_objects:(f + 1) * eng.n_objects] for f in range(n)]


class Pinned:
    """copies of host arrays in the library's pinned, device-mapped pool (roft_host_alloc): handed over as ROFT_MEM_DEVICE"""

    def __init__(self):
        self.ptrs, self.by_id = [], {}

    def put(self, a):
        if a is None:
            return None
        if id(a) not in self.by_id:
            a = np.ascontiguousarray(a)
            p = L.lib().roft_host_alloc(a.nbytes)
            assert p, "roft_host_alloc failed"
            C.memmove(p, a.ctypes.data, a.nbytes)
            self.ptrs.append(p)
            self.by_id[id(a)] = (p, a)      # (the array is kept: its id stays its own)
        return self.by_id[id(a)][0]

    def free(self):
        for p in self.ptrs:
            L.lib().roft_host_free(p)
        self.ptrs, self.by_id = [], {}


def run(streams, n, raw, T=1, dev=False, align=False, forms=False, fail_at=None, depths_at=()):
    """streams: one per object (the same stream twice: a shared scene).  raw: feed the 16-bit frames to an engine with
    enable_raw_depth -- else the operator's floats as HOST images to a plain engine.  dev: every image of the raw run lives in
    pinned memory and is handed over as ROFT_MEM_DEVICE.  forms: masks as label images and flows as camera images as well.
    fail_at: the batch holding that frame is first submitted with a bad last entry (refused), then as it should be."""
    eng = make_engine(streams, max_batch_frames=T)
    if raw:
        if align:
            eng.enable_raw_depth(SCALE, cam=_depth_camera(streams[0]), R=ALIGN_R, t=ALIGN_T)
        else:
            eng.enable_raw_depth(SCALE)
    if forms:
        eng.enable_flow()
    eng.enable_log(n)
    pin = Pinned()
    flows = {}

    def frame(st, k, bad=False):
        _, flow, mask, pose = util.frame_inputs(st, k)
        if flow is not None:
            flow = flows.setdefault((id(st), k), flow)        # (one array per stream and frame)
        if mask is not None:
            mask = flows.setdefault((id(st), k, "mask"), mask)
        depth = (_raw_small(st, k) if align else _raw(st, k)) if raw else _float_depth(st, k, align)
        d = dict(depth=depth, flow=flow, mask=mask, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST)
        if forms:
            d.update(flow=None, mask=None, image=_gray(st, k))
            if _labels(st, k) is not None:
                d.update(labels=_labels(st, k), label=3)
        if bad:
            d["mem_kind"] = 7
        if dev:
            assert not forms
            d.update(depth=pin.put(d["depth"]), flow=pin.put(d["flow"]), mask=pin.put(d["mask"]), mem_kind=L.MEM_DEVICE if not bad else 7)
        return d

    depths = {}
    k = 0
    while k < n:
        t = min(T, n - k)
        if fail_at is not None and k <= fail_at < k + t:
            before = eng.depth_stats()
            bad = [[frame(st, k + j, bad=(j == t - 1 and o == len(streams) - 1)) for o, st in enumerate(streams)] for j in range(t)]
            with pytest.raises(L.RoftError, match="error -1.*mem_kind"):
                eng.submit_batch(bad) if T > 1 else eng.submit(bad[0])
            assert eng.depth_stats() == before
        batch = [[frame(st, k + j) for st in streams] for j in range(t)]
        if T == 1:
            eng.submit(batch[0])
        else:
            eng.submit_batch(batch)
        eng.step()
        k += t
        if k - 1 in depths_at:
            depths[k - 1] = [eng.depth(o) for o in range(len(streams))]
    out = dict(log=_full_log(eng, n), masks=[eng.mask(o) for o in range(len(streams))], stats=eng.stats(), dstats=eng.depth_stats(),
               depths=depths, retain=eng.retain_frames())
    eng.close()
    pin.free()
    return out


def same(a, b):
    assert len(a["log"]) == len(b["log"])
    for f, (ra, rb) in enumerate(zip(a["log"], b["log"])):
        assert ra == rb, "frame %d differs" % f
    for ma, mb in zip(a["masks"], b["masks"]):
        assert np.array_equal(ma, mb)


def _log_is_alive(r, n):
    """the run measured something: flow points on most frames, an outlier test decided at least twice"""
    npts = [row[0][2] for row in r["log"]]
    assert sum(1 for v in npts[1:] if v > 0) >= n - 3
    assert sum(1 for row in r["log"] if row[0][3] >= 0) >= 2


def _n_frames(T):
    """more frames than the retention window (roft_engine_retain_frames(): 14 and 28 for these engines, asserted below) plus a
    batch: staging slots are recycled under a live depth_prev"""
    return 24 if T == 1 else 36


@pytest.mark.parametrize("dev", [False, True], ids=["host", "pinned-device"])
@pytest.mark.parametrize("T", [1, 4], ids=["T1", "T4"])
def test_convert_only_equivalence(T, dev):
    n = _n_frames(T)
    st = _stream(3100, n)
    ref = run([st, st], n, raw=False, T=T)
    got = run([st, st], n, raw=True, T=T, dev=dev, depths_at=(n - 1, T - 1))
    assert n > got["retain"] + T and got["retain"] == ref["retain"]
    _log_is_alive(ref, n)
    same(got, ref)
    for k, per_obj in got["depths"].items():
        for dep in per_obj:
            same_bits(dep, _float_depth(st, k, False))
    # one product per distinct pointer and frame -- the two objects of the shared scene make one, not two; two bytes per pixel go up
    assert got["dstats"] == dict(images=n, image_bytes=0 if dev else n * W * H * 2, products=n)
    assert ref["dstats"] == dict(images=0, image_bytes=0, products=0)
    if not dev:
        assert ref["stats"]["h2d_bytes"] - got["stats"]["h2d_bytes"] == n * W * H * 2      # (a float frame is four)


def test_two_scenes_make_two_products_per_frame():
    n = 8
    a, b = _stream(3100, 20), _stream(3101, 20)
    got = run([a, a, b], n, raw=True, T=4)
    same(got, run([a, a, b], n, raw=False, T=4))
    assert got["dstats"] == dict(images=2 * n, image_bytes=2 * n * W * H * 2, products=2 * n)


@pytest.mark.parametrize("T", [1, 4], ids=["T1", "T4"])
def test_align_equivalence(T):
    n = 14
    st = _stream(3100, 20)
    ref = run([st, st], n, raw=False, T=T, align=True)
    got = run([st, st], n, raw=True, T=T, align=True, depths_at=(n - 1,))
    same(got, ref)
    assert any(row[0][2] > 0 for row in ref["log"]), "the aligned depth carries flow points"
    for dep in got["depths"][n - 1]:
        same_bits(dep, _float_depth(st, n - 1, True))
        assert np.count_nonzero(dep) > dep.size // 2
    assert got["dstats"] == dict(images=n, image_bytes=n * DCAM_W * DCAM_H * 2, products=n)


def test_raw_depth_label_images_and_camera_images_together():
    n = 14
    st = _stream(3100, 20)
    ref = run([st, st], n, raw=False, T=4, forms=True)
    got = run([st, st], n, raw=True, T=4, forms=True)
    same(got, ref)
    assert sum(1 for row in got["log"] if row[0][2] > 0) >= n - 3
    assert got["dstats"]["products"] == n


def test_a_refused_submit_consumes_nothing():
    n = 10
    st = _stream(3100, 20)
    clean = run([st, st], n, raw=True, T=4)
    same(run([st, st], n, raw=True, T=4, fail_at=5), clean)
    same(run([st, st], n, raw=True, T=1, fail_at=1), clean)
    assert clean["dstats"]["products"] == n


def test_refusals():
    st = _stream(3100, 20)
    cam = _depth_camera(st)
    eng = make_engine([st])
    lib = L.lib()

    def refused(code, **over):
        src = ops.depth_source(SCALE, cam)
        for key, v in over.items():
            setattr(src, key, v)
        rc = lib.roft_engine_enable_raw_depth(eng._h, C.byref(src))
        assert rc == code, (over, rc)
        assert lib.roft_last_error_string()

    nan_R = (C.c_float * 9)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1)
    inf_t = (C.c_float * 3)(float("inf"), 0, 0)
    assert lib.roft_engine_enable_raw_depth(eng._h, None) == -1
    refused(-1, type=0)
    refused(-1, type=9)
    refused(-1, scale=0.0)
    refused(-1, scale=-1.0)
    refused(-1, scale=float("nan"))
    refused(-1, scale=float("inf"))
    refused(-1, R=nan_R)
    refused(-1, t=inf_t)
    refused(-1, cam=L.Camera(160, 120, 0.0, 100.0, 80.0, 60.0))
    refused(-1, cam=L.Camera(160, 120, 100.0, float("nan"), 80.0, 60.0))
    refused(-1, cam=L.Camera(4096, 4096, 100.0, 100.0, 80.0, 60.0))
    refused(-1, align=0)                                        # not aligned on the device, but 160 x 120 is not the engine's size
    with pytest.raises(L.RoftError, match="error -4"):
        eng.depth(0)                                            # an engine without raw depth makes none
    eng.enable_raw_depth(SCALE)                                 # ... and the corrected call is accepted
    # a misaligned DEVICE image
    import torch
    dst = util.to_device(st)
    buf = torch.zeros(W * H + 8, dtype=torch.int16).cuda()
    buf[2:2 + W * H] = torch.from_numpy(_raw(st, 0).astype(np.int16).reshape(-1)).cuda()
    d = util.device_frame(dst, 0)
    d["depth"] = buf.data_ptr() + 2
    with pytest.raises(L.RoftError, match="error -1.*depth 4 B"):
        eng.submit([d])
    assert eng.depth_stats() == dict(images=0, image_bytes=0, products=0) and eng.stats()["frames"] == 0
    d["depth"] = buf.data_ptr() + 4
    eng.submit([d])
    eng.step()
    same_bits(eng.depth(0), _float_depth(st, 0, False))
    assert eng.depth_stats() == dict(images=1, image_bytes=0, products=1)
    # enabling after the first frame
    with pytest.raises(L.RoftError, match="error -4"):
        eng.enable_raw_depth(SCALE)
    eng.close()


# ---- the sequence tool ------------------------------------------------------------------------------------------------------------
def test_run_sequence_tracks_from_16_bit_pngs(tmp_path, capsys):
    """tools/run_sequence.py --raw-depth SCALE reads depth/<i>.png and makes no float copy: its logs equal, byte for byte, those
    of the run on depth/<i>.float files holding the same readings as floats."""
    import importlib.util
    import os
    from roft_amd import io, synth
    n = 14
    st = util.stream(3102, n, scale=4)                      # 160 x 120
    root = str(tmp_path / "seq")
    mesh = io.write_sequence(root, st, "box", flow_set="analytic")
    for k in range(n):
        raw = np.clip(np.rint(st.depth[k].numpy() / SCALE), 0, 65535).astype(np.uint16)
        io.write_png(os.path.join(root, "depth", "%d.png" % k), raw)
        io.write_depth(os.path.join(root, "depth", "%d.float" % k), D.convert(raw, SCALE))
    spec = importlib.util.spec_from_file_location("run_sequence", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "run_sequence.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    m0 = synth.initial_pose_from_stream(st)
    common = ["--root", root, "--object", "box", "--mesh", mesh, "--flow-set", "analytic", "--mask-set", "gt", "--init-pose"] + ["%.17g" % v for v in m0[6:13]]
    assert rs.main(common + ["--out", str(tmp_path / "a_")]) == 0
    assert rs.main(common + ["--out", str(tmp_path / "b_"), "--raw-depth", str(SCALE)]) == 0
    capsys.readouterr()
    for name in ("pose_estimate", "velocity_estimate"):
        a, b = open(str(tmp_path / ("a_" + name)), "rb").read(), open(str(tmp_path / ("b_" + name)), "rb").read()
        assert a == b and len(a.splitlines()) == n
    seq = io.Sequence(root, "box", flow_set="analytic", mask_set="gt", width=160, height=120)
    f = seq.frame(3, depth_raw=True)
    assert f["depth"].dtype == np.uint16 and f["depth"].shape == (120, 160) and np.array_equal(D.convert(f["depth"], SCALE), seq.frame(3)["depth"])
