"""Camera images on the engine (roft_engine_enable_flow, roft_frames_submit_images; k_opticalflow.hip, engine_submit.hip): an
object whose entries carry images behaves, bit for bit, as if inputs[].flow of frame k had been a HOST buffer holding
roft_optical_flow(G_{k-1}, G_k) when frames k - 1 and k both carried an image, and NULL otherwise.  So every test runs the SAME
engine twice on identical inputs -- once fed the flows of ops.optical_flow, once fed the images -- and asks for EQUAL bytes:
the log (poses, twists, n_flow_points, outlier decisions and likelihoods), the final masks, the produced flows.  No tolerance.

Shapes: util.stream(seed, n, scale=2, with_gray=True) is 320 x 240 -- 10 x 30 Lucas-Kanade tiles at level 0, 5 x 15 and 3 x 8
(a partial tile row) below; the stand-alone conversion also runs at 1 x 1, 5 x 3 and 97 x 61 (no multiple of anything)."""
import ctypes as C

import numpy as np
import pytest
import torch

from roft_amd import _lib as L
from roft_amd import io, ops

import util
from pose_error_util import make_engine

pytestmark = pytest.mark.gpu

F32, S16 = L.FLOW_F32C2, L.FLOW_S16C2
N1 = 20     # masks at 0, 6, 12, 18 and pose arrivals every 6 frames: two deliveries after the first, two re-sync replays with tests
_flows = {}


def _stream(seed, n, ft):
    return util.stream(seed, n, scale=2, flow_type=ft, with_gray=True)


def _gray(st, k):
    """frame k's gray image: ONE array object per stream and frame, so that the objects of a shared scene name one host pointer"""
    if not hasattr(st, "_gray_np"):
        st._gray_np = [np.ascontiguousarray(st.gray[i].numpy()) for i in range(st.n_frames)]
    return st._gray_np[st.image(k)]


def _rgb(st, k):
    if not hasattr(st, "_rgb_np"):
        st._rgb_np = {}
    if k not in st._rgb_np:
        g = _gray(st, k).astype(np.int32)
        st._rgb_np[k] = np.ascontiguousarray(np.stack([g, g // 2 + 40, (3 * g) // 4 + 11], -1).astype(np.uint8))
    return st._rgb_np[k]


def _image_gray(st, k, kind):
    return _gray(st, k) if kind == "img" else io.rgb_to_gray(_rgb(st, k))


def _ref_flow(st, k, prev_kind, kind, ft, of):
    key = (id(st), k, prev_kind, kind, ft, tuple(sorted(of.items())))
    if key not in _flows:
        _flows[key] = ops.optical_flow(_image_gray(st, k - 1, prev_kind), _image_gray(st, k, kind), flow_type=ft, **of)
    return _flows[key]


def _full_log(eng, n):
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, 0, n, outs))
    rows = [(np.array(r.pose[:]).tobytes(), np.array(r.twist[:]).tobytes(), r.n_flow_points, r.outlier_selected, np.array(r.outlier_L[:]).tobytes())
            for r in outs]
    return [rows[f * eng.n_objects:(f + 1) * eng.n_objects] for f in range(n)]


def run(objs, n, ft, as_flows=False, splits=None, dev=False, of=None, enable=True, fail_at=None, flows_at=()):
    """objs: [(stream, feed)], feed(k) in 'img' (gray camera image) | 'rgb' (RGB8 image) | 'flow' (the flow handed directly) |
    'none'.  as_flows: the reference run -- every image is replaced by the flow the specification names for it.
    Returns dict(log, masks, stats, fstats, flows={(k, obj): produced flow} for k in flows_at)."""
    of = of or {}
    eng = make_engine([st for st, _ in objs], max_batch_frames=max(splits) if splits else 1)
    if enable:
        eng.enable_flow(**of)
    eng.enable_log(n)
    kept = []
    dstreams = {id(st): util.to_device(st) for st, _ in objs} if dev else {}

    def put(a):
        if a is None or not dev:
            return a
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        kept.append(t)
        return t.data_ptr()

    def frame(st, feed, k, bad=False):
        if dev:
            d = util.device_frame(dstreams[id(st)], k)
            d["flow"] = None
        else:
            depth, _, mask, pose = util.frame_inputs(st, k)
            d = dict(depth=depth, mask=mask, pose=pose, dt=st.dt, mem_kind=L.MEM_HOST)
        kind = feed(k)
        prev = feed(k - 1) if k > 0 else "none"
        if kind == "flow":
            d["flow"] = put(_ref_flow(st, k, "img", "img", ft, of)) if k > 0 else None
        elif kind in ("img", "rgb"):
            if as_flows:
                d["flow"] = put(_ref_flow(st, k, prev, kind, ft, of)) if prev in ("img", "rgb") else None
            else:
                img = _gray(st, k) if kind == "img" else _rgb(st, k)
                if dev:
                    if not hasattr(st, "_dev_img"):
                        st._dev_img = {}
                    if (k, kind) not in st._dev_img:     # one device image per stream and frame: a shared scene names one address
                        st._dev_img[(k, kind)] = torch.from_numpy(img).cuda()
                    d["image"] = st._dev_img[(k, kind)].data_ptr()
                    d["image_type"] = L.IMAGE_GRAY8 if kind == "img" else L.IMAGE_RGB8
                else:
                    d["image"] = img
                if bad:
                    d["flow"] = put(np.zeros_like(_ref_flow(st, max(k, 1), "img", "img", ft, of)))
        return d

    flows = {}
    k = i = 0
    while k < n:
        t = min(splits[i % len(splits)] if splits else 1, n - k)
        i += 1
        if fail_at is not None and k <= fail_at < k + t:
            # image AND flow in the LAST object's entry of the batch's last frame: everything before it has been consumed when
            # the call is refused -- and must be handed back
            before = eng.flow_stats()
            bad = [[frame(st, feed, k + j, bad=(j == t - 1 and o == len(objs) - 1)) for o, (st, feed) in enumerate(objs)] for j in range(t)]
            with pytest.raises(L.RoftError, match="camera image AND a flow"):
                eng.submit_batch(bad)
            assert eng.flow_stats() == before
        batch = [[frame(st, feed, k + j) for st, feed in objs] for j in range(t)]
        if t == 1 and not splits:
            eng.submit(batch[0])
        else:
            eng.submit_batch(batch)
        eng.step()
        k += t
        if k - 1 in flows_at:
            for o in range(len(objs)):
                flows[(k - 1, o)] = eng.produced_flow(o)
    out = dict(log=_full_log(eng, n), masks=[eng.mask(o) for o in range(len(objs))], stats=eng.stats(), fstats=eng.flow_stats(), flows=flows)
    eng.close()
    del kept
    for st, _ in objs:
        if hasattr(st, "_dev_img"):
            del st._dev_img
    return out


def same(a, b, objs_a=None, objs_b=None):
    """logs and masks of run a (its objects objs_a, default all) equal those of run b (objs_b)"""
    na = len(a["masks"])
    objs_a = list(range(na)) if objs_a is None else objs_a
    objs_b = objs_a if objs_b is None else objs_b
    assert len(a["log"]) == len(b["log"])
    for f, (ra, rb) in enumerate(zip(a["log"], b["log"])):
        for oa, ob in zip(objs_a, objs_b):
            assert ra[oa] == rb[ob], "frame %d, objects %d / %d differ" % (f, oa, ob)
    for oa, ob in zip(objs_a, objs_b):
        assert np.array_equal(a["masks"][oa], b["masks"][ob])


def always(kind):
    return lambda k: kind


def _log_is_alive(r, n):
    """the run measured something: flow points on most frames, an outlier test decided at least twice"""
    npts = [row[0][2] for row in r["log"]]
    assert sum(1 for v in npts[1:] if v > 0) >= n - 3
    assert sum(1 for row in r["log"] if row[0][3] >= 0) >= 2


# ---- 1. one object, DEVICE gray images, single-frame submits -------------------------------------------------------------
@pytest.mark.parametrize("ft", [F32, S16], ids=["f32c2", "s16c2"])
def test_device_images_single_frames(ft):
    st = _stream(2100, N1, ft)
    assert sum(1 for k in range(1, N1) if st.mask_delivery[k] >= 0) >= 2 and sum(1 for k in range(N1) if st.pose_valid[k]) >= 2
    ref = run([(st, always("img"))], N1, ft, as_flows=True, dev=True)
    got = run([(st, always("img"))], N1, ft, dev=True)
    _log_is_alive(ref, N1)
    same(got, ref)
    assert got["fstats"] == dict(images=N1, image_bytes=0, pyramids=N1, pairs=N1 - 1)
    assert ref["fstats"] == dict(images=0, image_bytes=0, pyramids=0, pairs=0)


# ---- 2. the produced flow ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", [F32, S16], ids=["f32c2", "s16c2"])
@pytest.mark.parametrize("of", [dict(levels=1, radius=2, iterations=2), dict(levels=2, radius=1, iterations=5)], ids=["l1r2i2", "l2r1i5"])
def test_produced_flow_equals_the_operator(ft, of):
    st = _stream(2100, N1, ft)
    got = run([(st, always("img"))], 3, ft, of=of, flows_at=(1, 2))
    for k in (1, 2):
        want = ops.optical_flow(_gray(st, k - 1), _gray(st, k), flow_type=ft, **of)
        assert got["flows"][(k, 0)].dtype == want.dtype and np.array_equal(got["flows"][(k, 0)], want), k
    assert np.any(got["flows"][(1, 0)] != 0)


def test_no_produced_flow_on_the_first_frame():
    st = _stream(2100, N1, F32)
    eng = make_engine([st])
    eng.enable_flow()
    depth, _, mask, pose = util.frame_inputs(st, 0)
    eng.submit([dict(depth=depth, mask=mask, pose=pose, dt=st.dt, image=_gray(st, 0))])
    eng.step()
    with pytest.raises(L.RoftError, match="no flow"):
        eng.produced_flow(0)
    eng.close()


# ---- 3. HOST images, batches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ft", [F32, S16], ids=["f32c2", "s16c2"])
def test_host_images_in_batches(ft):
    n = 40
    st = _stream(2101, n, ft)
    objs = [(st, always("img"))]
    single = run(objs, n, ft)
    same(single, run(objs, n, ft, as_flows=True))
    same(run(objs, n, ft, splits=[8]), single)
    same(run(objs, n, ft, splits=[1, 3, 4, 2, 8]), single)
    assert single["fstats"] == dict(images=n, image_bytes=n * 320 * 240, pyramids=n, pairs=n - 1)


# ---- 4. a shared scene plus a stream of its own --------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_shared_scene_and_own_stream(dev):
    F = 14
    a, b = _stream(2102, F, F32), _stream(2103, F, F32)
    objs = [(a, always("img"))] * 3 + [(b, always("img"))]
    got = run(objs, F, F32, splits=[4], dev=dev)
    alone_a = run([(a, always("img"))], F, F32, dev=dev)
    alone_b = run([(b, always("img"))], F, F32, dev=dev)
    for o in range(3):
        same(got, alone_a, [o], [0])
    same(got, alone_b, [3], [0])
    fs = got["fstats"]
    # one pyramid per distinct image, one flow per distinct pair: NOT per pair's two images (4 (F - 1)), not per object (4 F, 4 (F - 1))
    assert (fs["images"], fs["pyramids"], fs["pairs"]) == (2 * F, 2 * F, 2 * (F - 1))
    assert fs["image_bytes"] == (0 if dev else 2 * F * 320 * 240)


# ---- 5. a gap ------------------------------------------------------------------------------------------------------------
def test_gap_starts_over():
    F, gap = 14, 5
    a, b = _stream(2102, F, F32), _stream(2103, F, F32)
    trio = lambda k: "none" if k == gap else "img"
    objs = [(a, trio)] * 3 + [(b, always("img"))]
    got = run(objs, F, F32, splits=[4])
    ref = run(objs, F, F32, splits=[4], as_flows=True)
    same(got, ref)
    for f in (gap, gap + 1):
        assert all(got["log"][f][o][2] <= 0 for o in range(3)), "no flow, no flow points"     # n_flow_points
    assert got["log"][gap + 2][0][2] > 0
    assert got["fstats"]["pairs"] == 2 * (F - 1) - 2


# ---- 6. colour -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (61, 97), (240, 320)], ids=lambda s: "%dx%d" % (s[1], s[0]))
def test_image_to_gray_equals_the_fixed_point_formula(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    rgb = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
    if shape == (240, 320):
        rgb[0, :8] = [[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    want = io.rgb_to_gray(rgb)
    assert np.array_equal(ops.image_to_gray(rgb, L.IMAGE_RGB8), want)
    assert np.array_equal(ops.image_to_gray(np.ascontiguousarray(rgb[..., ::-1]), L.IMAGE_BGR8), want)
    assert np.array_equal(ops.image_to_gray(want), want)          # a gray image passes through


def test_rgb_images_equal_their_gray_images():
    n = 14
    st = _stream(2104, n, F32)
    # the reference: the same engine fed the gray images of the colour frames
    gray_of_rgb = run([(st, always("rgb"))], n, F32, as_flows=True)
    got = run([(st, always("rgb"))], n, F32, splits=[4], flows_at=(3,))
    same(got, gray_of_rgb)
    assert np.array_equal(got["flows"][(3, 0)], ops.optical_flow(io.rgb_to_gray(_rgb(st, 2)), io.rgb_to_gray(_rgb(st, 3))))
    assert got["fstats"]["image_bytes"] == n * 3 * 320 * 240
    _log_is_alive(got, n)


# ---- 7. flows handed directly next to images -----------------------------------------------------------------------------
def test_mixed_flows_and_images():
    n = 14
    a, b = _stream(2102, n, S16), _stream(2103, n, S16)
    got = run([(a, always("flow")), (b, always("img"))], n, S16, splits=[3])
    ref = run([(a, always("flow")), (b, always("img"))], n, S16, splits=[3], as_flows=True)
    same(got, ref)
    assert got["fstats"]["pairs"] == n - 1
    # an object may change form from frame to frame: a direct flow where it brought no image
    swap = lambda k: "flow" if k in (4, 5, 9) else "img"
    same(run([(a, swap), (b, always("img"))], n, S16, splits=[3]), run([(a, swap), (b, always("img"))], n, S16, splits=[3], as_flows=True))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_a_refused_submit_consumes_nothing():
    n = 14
    a, b = _stream(2102, n, F32), _stream(2103, n, F32)
    objs = [(a, always("img")), (b, always("img"))]
    clean = run(objs, n, F32, splits=[4])
    same(run(objs, n, F32, splits=[4], fail_at=6), clean)      # refused in the middle of the run, then the corrected batch
    same(run(objs, n, F32, fail_at=1), clean)                  # ... and frame by frame, with a previous image to keep


def _first_frame(st, **extra):
    depth, _, mask, pose = util.frame_inputs(st, 0)
    d = dict(depth=depth, mask=mask, pose=pose, dt=st.dt)
    d.update(extra)
    return d


def test_refusals():
    st = _stream(2100, N1, F32)
    # images without enable_flow: ROFT_ERR_STATE, and the same engine takes the frame with a flow instead
    eng = make_engine([st])
    with pytest.raises(L.RoftError, match=r"error -4.*roft_engine_enable_flow"):
        eng.submit([_first_frame(st, image=_gray(st, 0))])
    eng.submit([_first_frame(st)])
    eng.step()
    # enable_flow after the first frame
    with pytest.raises(L.RoftError, match="error -4"):
        eng.enable_flow()
    eng.close()
    # a configuration the producer cannot serve
    eng = make_engine([st], flow_grid=4)
    with pytest.raises(L.RoftError, match="error -1.*flow_grid 1"):
        eng.enable_flow()
    eng.close()
    eng = make_engine([st])
    with pytest.raises(L.RoftError, match="error -1.*multiple of"):
        eng.enable_flow(levels=6)               # 320 is no multiple of 4 * 32
    with pytest.raises(L.RoftError, match="error -1"):
        eng.enable_flow(radius=9)
    eng.enable_flow()                           # ... and the corrected call is accepted
    # unknown image type; image and flow in one entry
    with pytest.raises(L.RoftError, match="error -1.*image_type"):
        eng.submit([_first_frame(st, image=_gray(st, 0), image_type=7)])
    with pytest.raises(L.RoftError, match="error -1.*camera image AND a flow"):
        eng.submit([_first_frame(st, image=_gray(st, 0), flow=np.zeros((240, 320, 2), np.float32))])
    assert eng.flow_stats() == dict(images=0, image_bytes=0, pyramids=0, pairs=0) and eng.stats()["frames"] == 0
    # a misaligned DEVICE image
    dst = util.to_device(st)
    img = torch.zeros(240 * 320 + 8, dtype=torch.uint8).cuda()
    d = util.device_frame(dst, 0)
    d["flow"] = None
    d.update(image=img.data_ptr() + 1, image_type=L.IMAGE_GRAY8)
    with pytest.raises(L.RoftError, match="error -1.*camera image 4 B"):
        eng.submit([d])
    d["image"] = img.data_ptr() + 4
    eng.submit([d])
    eng.step()
    eng.sync()
    assert eng.flow_stats() == dict(images=1, image_bytes=0, pyramids=1, pairs=0)
    eng.close()
