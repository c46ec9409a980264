"""Lens distortion on the engine (include/roft_engine.h section 3g), the equivalence that defines the feature: engine A has
roft_engine_enable_rectification and receives the sensor's (distorted) frames; engine B has not and receives the stand-alone
operator's products as HOST images.  The two run in lockstep and must agree bit for bit after every step -- states, masks, the
produced flow, the depth -- and in every log row at the end.

Shapes: 64 x 48 (util.stream at scale 10: the smallest the flow producer takes at levels = 2 next to a 4:3 camera), three objects of
which two share a scene, 12 frames with a mask and a pose every 4th (deliveries at frames 0, 4, 8), the lens
(-0.05, 0.01, 0.001, 0.0005, 0) onto slightly different intrinsics."""
import ctypes as C

import numpy as np
import pytest

import rectify_ref as R
import util
from pose_error_util import make_engine
from roft_amd import _lib as L
from roft_amd import ops

pytestmark = pytest.mark.gpu

N = 12
SCALE = 0.001
DIST = (-0.05, 0.01, 0.001, 0.0005, 0.0)
ALIGN_T = np.array([0.004, 0.001, -0.0005])
_cache = {}


def _streams():
    a, b = (util.stream(5200 + i, N, scale=10, with_gray=True, mask_period=4, pose_period=4) for i in range(2))
    assert (a.camera.width, a.camera.height) == (64, 48)
    return [a, a, b]


def _sensor(st):
    c = st.camera
    return R.lens(R.Cam(c.width, c.height, c.fx * 1.02, c.fy * 0.99, c.cx + 0.7, c.cy - 0.4), DIST)


def _frame_image(st, k, what):
    """ONE array per stream, frame and form, so that the objects of a shared scene name one host pointer"""
    key = (id(st), k, what)
    if key not in _cache:
        i = st.image(k)
        if what == "f32":
            v = np.ascontiguousarray(st.depth[i].numpy())
        elif what == "z16":
            v = np.clip(np.rint(st.depth[i].numpy() / SCALE), 0, 65535).astype(np.uint16)
        elif what == "z16-small":
            v = np.ascontiguousarray(_frame_image(st, k, "z16")[::2, ::2])
        elif what == "gray":
            v = np.ascontiguousarray(st.gray[i].numpy())
        elif what in ("rgb", "bgr"):
            g = _frame_image(st, k, "gray")
            v = np.ascontiguousarray(np.stack([g, 255 - g, g // 2 + 17], axis=2))
        else:
            mi = st.mask_delivery[k]
            if mi < 0:
                v = None
            elif what == "mask":
                v = np.ascontiguousarray(st.mask_gt[mi].numpy())
            elif what == "labels8":
                v = np.where(st.mask_gt[mi].numpy() > 0, 3, 0).astype(np.uint8)
            else:
                v = np.where(st.mask_gt[mi].numpy() > 0, 300, 7).astype(np.uint16)
        _cache[key] = v
    return _cache[key]


def _product(st, img, kind):
    """what the contract says engine A behaves as if it had been handed: the operator's product, computed once"""
    key = ("product", id(img), kind)
    if key not in _cache:
        _cache[key] = (ops.rectify(img, _sensor(st), st.camera, kind=kind), img)     # (the source is kept: its id stays its own)
    return _cache[key][0]


class Pinned:
    """copies of host arrays in the library's pinned, device-mapped pool (roft_host_alloc): handed over as ROFT_MEM_DEVICE"""

    def __init__(self):
        self.ptrs, self.by_id = [], {}

    def put(self, a):
        if id(a) not in self.by_id:
            p = L.lib().roft_host_alloc(a.nbytes)
            assert p, "roft_host_alloc failed"
            C.memmove(p, a.ctypes.data, a.nbytes)
            self.ptrs.append(p)
            self.by_id[id(a)] = (p, a)
        return self.by_id[id(a)][0]

    def free(self):
        for p in self.ptrs:
            L.lib().roft_host_free(p)


def _entries(streams, k, depth, masks, image, rectified, pin=None, kinds=None):
    """the frame dicts of frame k for the three objects: the sensor's frames (engine A) or their products (engine B).  kinds: a
    set that receives the distinct (image, kind) pairs engine A has to rectify."""
    out = []
    for st in streams:
        d = dict(pose=util.frame_inputs(st, k)[3], dt=st.dt, flow=None, mem_kind=L.MEM_HOST)

        def put(key, img, kind, extra=()):
            if kind is not None:
                if kinds is not None:
                    kinds.add((id(img), kind))
                if rectified:
                    img = _product(st, img, kind)
            d[key] = pin.put(img) if pin else img
            if pin:
                d.update(extra)

        if depth == "f32":
            put("depth", _frame_image(st, k, "f32"), L.RECTIFY_F32)
        elif depth == "z16":
            put("depth", _frame_image(st, k, "z16"), L.RECTIFY_U16)
        else:
            put("depth", _frame_image(st, k, "z16-small"), None)      # aligned on the device: not touched
        if image == "gray":
            put("image", _frame_image(st, k, "gray"), L.RECTIFY_GRAY8, dict(image_type=L.IMAGE_GRAY8))
        else:
            img = _frame_image(st, k, image)
            typ = L.IMAGE_RGB8 if image == "rgb" else L.IMAGE_BGR8
            if rectified:      # G_k = rectify(gray(image)): engine B sees a GRAY8 image
                key = ("gray-of", id(img), typ)
                if key not in _cache:
                    _cache[key] = ops.image_to_gray(img, typ)
                if kinds is not None:
                    kinds.add((id(img), "gray-of-%d" % typ))
                d["image"] = _product(st, _cache[key], L.RECTIFY_GRAY8)
            else:
                if kinds is not None:
                    kinds.add((id(img), "gray-of-%d" % typ))
                d["image"], d["image_type"] = (pin.put(img) if pin else img), typ
        m = _frame_image(st, k, masks) if masks != "pose" else None
        if m is not None and masks == "mask":
            put("mask", m, L.RECTIFY_U8)
        elif m is not None:
            put("labels", m, L.RECTIFY_U8 if masks == "labels8" else L.RECTIFY_U16,
                dict(label_type=L.LABEL_U8 if masks == "labels8" else L.LABEL_U16))
            d["label"] = 3 if masks == "labels8" else 300
        if pin:
            d["mem_kind"] = L.MEM_DEVICE
        out.append(d)
    return out


def _full_log(eng, n):
    outs = (L.ObjectOutput * (n * eng.n_objects))()
    L.check(L.lib().roft_engine_get_log(eng._h, 0, n, outs))
    return [(np.array(r.pose[:]).tobytes(), np.array(r.twist[:]).tobytes(), r.n_flow_points, r.outlier_selected, np.array(r.outlier_L[:]).tobytes())
            for r in outs]


def _flow(eng, o):
    try:
        return eng.produced_flow(o)
    except L.RoftError:
        return None


def _same_flow(a, b):
    """equal bytes (a produced flow may hold NaN: compared as bits)"""
    return (a is None and b is None) or (a is not None and b is not None and a.tobytes() == b.tobytes())


def run_pair(depth="f32", masks="mask", image="gray", T=1, dev=False, rectify_first=False, refuse_flow_at=None):
    streams = _streams()
    st0 = streams[0]
    engines = []
    for rect in (True, False):
        eng = make_engine(streams, max_batch_frames=T)
        if rect and rectify_first:
            eng.enable_rectification(_sensor(st0))
        eng.enable_flow(levels=2)
        if depth == "z16":
            eng.enable_raw_depth(SCALE)
        elif depth == "z16-align":
            c = st0.camera
            eng.enable_raw_depth(SCALE, cam=R.Cam(c.width // 2, c.height // 2, c.fx / 2, c.fy / 2, (c.cx + 0.5) / 2 - 0.5, (c.cy + 0.5) / 2 - 0.5), t=ALIGN_T)
        if masks == "pose":
            eng.enable_pose_masks()
            eng.enable_pose_mask_depth_gate()
        eng.enable_log(N)
        if rect and not rectify_first:
            eng.enable_rectification(DIST, cam=_sensor(st0).cam)
        engines.append(eng)
    A, B = engines
    pin = Pinned() if dev else None
    expected_products, expected_bytes, npix = 0, 0, st0.camera.width * st0.camera.height
    src_bytes = {L.RECTIFY_F32: 4, L.RECTIFY_U16: 2, L.RECTIFY_U8: 1, L.RECTIFY_GRAY8: 1}
    k = 0
    n_flows = 0
    try:
        while k < N:
            t = min(T, N - k)
            kinds_per_frame = [set() for _ in range(t)]
            batch_a = [_entries(streams, k + j, depth, masks, image, False, pin, kinds_per_frame[j]) for j in range(t)]
            batch_b = [_entries(streams, k + j, depth, masks, image, True) for j in range(t)]
            if refuse_flow_at is not None and k <= refuse_flow_at < k + t:
                before = A.rectify_stats(), A.flow_stats()
                bad = [[dict(d) for d in frame] for frame in batch_a]
                bad[-1][-1]["flow"] = np.zeros((st0.camera.height, st0.camera.width, 2), np.float32) if not dev else bad[-1][-1]["depth"]
                with pytest.raises(L.RoftError, match="error -1.*flow.*roft_engine_enable_rectification"):
                    A.submit_batch(bad) if T > 1 else A.submit(bad[0])
                assert (A.rectify_stats(), A.flow_stats()) == before, "a refused submit consumes nothing"
            for eng, batch in ((A, batch_a), (B, batch_b)):
                if T == 1:
                    eng.submit(batch[0])
                else:
                    eng.submit_batch(batch)
            assert A.rectify_kernel_ms() > 0.0
            with pytest.raises(L.RoftError, match="error -4"):
                B.rectify_kernel_ms()
            A.step()
            B.step()
            k += t
            for kinds in kinds_per_frame:
                expected_products += len(kinds)
                expected_bytes += sum(npix * (4 if isinstance(kd, str) else 2 * src_bytes[kd]) for _, kd in kinds)
            for o in range(len(streams)):
                for x, y in zip(A.state(o), B.state(o)):
                    assert x.tobytes() == y.tobytes(), "state of object %d differs after frame %d" % (o, k - 1)
                assert np.array_equal(A.mask(o), B.mask(o)), "mask of object %d differs after frame %d" % (o, k - 1)
                fa, fb = _flow(A, o), _flow(B, o)
                assert _same_flow(fa, fb), "flow of object %d differs after frame %d" % (o, k - 1)
                n_flows += fa is not None
                da = A.depth(o)
                st = streams[o]
                if depth == "f32":
                    want = _product(st, _frame_image(st, k - 1, "f32"), L.RECTIFY_F32)
                elif depth == "z16":
                    want = ops.depth_convert(_product(st, _frame_image(st, k - 1, "z16"), L.RECTIFY_U16), SCALE)
                    assert B.depth(o).tobytes() == da.tobytes()
                else:
                    want = B.depth(o)
                assert da.tobytes() == want.tobytes(), "depth of object %d differs after frame %d" % (o, k - 1)
        log_a, log_b = _full_log(A, N), _full_log(B, N)
        for i, (ra, rb) in enumerate(zip(log_a, log_b)):
            assert ra == rb, "log row of frame %d, object %d differs" % divmod(i, len(streams))
        assert n_flows >= len(streams) * ((N + T - 1) // T - 1), "every step but the first ends on a frame with a produced flow"
        assert sum(1 for r in log_a if r[2] > 0) >= len(streams) * (N - 4), "the runs measured something: flow points on most frames"
        stats = A.rectify_stats()
        assert stats["products"] == expected_products and stats["bytes"] == expected_bytes
        assert stats["sources"] == expected_products      # (no image is named under two kinds here)
        assert B.rectify_stats() == dict(sources=0, products=0, bytes=0)
        with pytest.raises(L.RoftError, match="error -4.*first frame"):
            A.enable_rectification(DIST)
        return dict(stats=stats, gate=A.pose_mask_gate_stats() if masks == "pose" else None, gate_b=B.pose_mask_gate_stats() if masks == "pose" else None)
    finally:
        A.close()
        B.close()
        if pin:
            pin.free()


@pytest.mark.parametrize("dev", [False, True], ids=["host", "pinned-device"])
@pytest.mark.parametrize("T", [1, 4], ids=["T1", "T4"])
def test_float_depth_masks_and_gray_images(T, dev):
    out = run_pair("f32", "mask", "gray", T=T, dev=dev)
    # per frame: two scenes x (depth, image), and two masks on each of the three delivering frames
    assert out["stats"]["products"] == N * 4 + 3 * 2


@pytest.mark.parametrize("masks,image", [("labels8", "rgb"), ("labels16", "bgr")])
def test_raw_depth_label_images_and_colour_images(masks, image):
    run_pair("z16", masks, image, T=4, refuse_flow_at=5)


def test_label_images_from_device_memory_single_frames():
    run_pair("z16", "labels16", "rgb", T=1, dev=True, rectify_first=True, refuse_flow_at=2)


def test_aligned_raw_depth_is_not_touched():
    out = run_pair("z16-align", "mask", "gray", T=4, rectify_first=True)
    assert out["stats"]["products"] == N * 2 + 3 * 2


def test_pose_masks_and_their_depth_gate_read_the_rectified_depth():
    out = run_pair("f32", "pose", "gray", T=4)
    assert out["gate"] == out["gate_b"] and out["gate"]["gated"] >= 2 * 3


def test_a_source_of_another_size_is_refused():
    st = _streams()[0]
    eng = make_engine([st])
    try:
        c = st.camera
        for cam in (R.Cam(c.width + 8, c.height, c.fx, c.fy, c.cx, c.cy), R.Cam(c.width, c.height - 2, c.fx, c.fy, c.cx, c.cy)):
            with pytest.raises(L.RoftError, match="error -1.*size of roft_config::cam"):
                eng.enable_rectification(DIST, cam=cam)
        with pytest.raises(L.RoftError, match="error -1.*k1"):
            eng.enable_rectification((np.nan, 0, 0, 0, 0))
        assert L.lib().roft_engine_enable_rectification(eng._h, None) == L.ERR_INVALID
        eng.enable_rectification(DIST)
        assert eng.rectify_stats() == dict(sources=0, products=0, bytes=0)
    finally:
        eng.close()


# ---- the tools ----------------------------------------------------------------------------------------------------------------------
def test_run_sequence_and_render_results_rectify_a_directory_of_distorted_frames(tmp_path, capsys):
    """tools/run_sequence.py --flow-on-engine nvof2 --lens ... on a directory of the sensor's frames writes, byte for byte, the logs
    of the run without --lens on a directory that holds the operators' products; tools/render_results.py --lens draws the same
    overlays over the distorted frames as without it over the rectified ones."""
    import importlib.util
    import json
    import os
    from roft_amd import io, synth
    n = 14
    st = util.stream(5210, n, scale=4, with_gray=True)      # 160 x 120
    c = st.camera
    sensor = R.lens(R.Cam(c.width, c.height, c.fx * 1.02, c.fy * 0.99, c.cx + 0.7, c.cy - 0.4), DIST)
    root_a, root_b = str(tmp_path / "sensor"), str(tmp_path / "rectified")
    mesh = io.write_sequence(root_a, st, "box")
    io.write_sequence(root_b, st, "box")
    for k in range(n):
        io.write_depth(os.path.join(root_b, "depth", "%d.float" % k), ops.rectify(st.depth[k].numpy(), sensor, c))
        g = ops.rectify(np.ascontiguousarray(st.gray[k].numpy()), sensor, c)
        io.write_png(os.path.join(root_b, "rgb", "%d.png" % k), np.repeat(g[..., None], 3, axis=2))
        name = os.path.join("masks", "gt", "box_%d.png" % k)
        if os.path.exists(os.path.join(root_a, name)):
            io.write_png(os.path.join(root_b, name), ops.rectify(io.read_mask_png(os.path.join(root_a, name)), sensor, c, nearest=True))
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    spec = importlib.util.spec_from_file_location("run_sequence", os.path.join(tools, "run_sequence.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    m0 = synth.initial_pose_from_stream(st)
    lens_args = ["--lens=" + ",".join("%.17g" % v for v in DIST), "--lens-camera=" + ",".join("%.17g" % v for v in sensor.cam[2:])]
    common = ["--object", "box", "--mesh", mesh, "--mask-set", "gt", "--flow-on-engine", "nvof2", "--init-pose"] + ["%.17g" % v for v in m0[6:13]]
    capsys.readouterr()
    assert rs.main(["--root", root_a, "--out", str(tmp_path / "a_"), "--render-overlay", str(tmp_path / "over_a")] + common + lens_args) == 0
    report = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert report["rectification"]["products"] >= 2 * n and report["rectification"]["sources"] == report["rectification"]["products"]
    assert rs.main(["--root", root_b, "--out", str(tmp_path / "b_"), "--render-overlay", str(tmp_path / "over_b")] + common) == 0
    assert "rectification" not in json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    for name in ("pose_estimate", "velocity_estimate"):
        a, b = open(str(tmp_path / ("a_" + name)), "rb").read(), open(str(tmp_path / ("b_" + name)), "rb").read()
        assert a == b and len(a.splitlines()) == n
    for k in range(n):
        a, b = io.read_png(str(tmp_path / "over_a" / ("%d.png" % k))), io.read_png(str(tmp_path / "over_b" / ("%d.png" % k)))
        assert np.array_equal(a, b), "overlay %d differs" % k
    assert not np.array_equal(io.read_png(os.path.join(root_a, "rgb", "5.png")), io.read_png(os.path.join(root_b, "rgb", "5.png")))
