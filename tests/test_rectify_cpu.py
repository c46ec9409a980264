"""Lens distortion (include/roft_engine.h section 3g) without a GPU: the numpy restatement tests/rectify_ref.py alone is sharp --
identity, integer shift, zoom, pixels outside the source, a map that is not finite -- the header declares the calls and the binding
has them, and the stand-alone operators refuse bad arguments before a device is looked for."""
import ctypes as C
import math

import numpy as np
import pytest

import abi_header
import rectify_ref as R
from roft_amd import _lib as L
from roft_amd import ops


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", [R.Cam(64, 48, 60.0, 61.0, 30.2, 24.9), R.Cam(640, 480, 615.3, 617.9, 312.7, 245.1),
                                 R.Cam(1280, 720, 1229.4, 1231.8, 651.3, 348.6)], ids=lambda c: "%dx%d" % (c.width, c.height))
def test_identity_returns_the_input(cam):
    """Zero coefficients, source = target: both samplers return the input bit for bit, although the MAP is not exactly (u, v) in
    float (an off-centre principal point, fx != fy)."""
    ln = R.lens(cam)
    sx, sy = R.rect_map(ln, cam)
    u, v = np.meshgrid(np.arange(cam.width, dtype=np.float32), np.arange(cam.height, dtype=np.float32))
    assert np.max(np.abs(sx - u)) < 0.01 and np.max(np.abs(sy - v)) < 0.01
    for kind in (R.GRAY8, R.RGB8, R.U8, R.U16, R.F32):
        img = R.image(cam, kind)
        assert np.array_equal(R.rectify(img, kind, ln, cam), img), kind


def test_integer_shift_returns_the_window():
    """Zero coefficients and a principal point moved by (+5, +3) into a source that is (W + 8) x (H + 6): the shifted window."""
    t = R.TARGET
    src = R.Cam(t.width + 8, t.height + 6, t.fx, t.fy, t.cx + 5, t.cy + 3)
    ln = R.lens(src)
    for kind in (R.GRAY8, R.RGB8, R.U8, R.U16, R.F32):
        img = R.image(src, kind)
        assert np.array_equal(R.rectify(img, kind, ln, t), img[3:3 + t.height, 5:5 + t.width]), kind


def test_zoom_takes_every_second_pixel():
    """A source of exactly twice the size and twice the intrinsics, nearest, on u16 data."""
    t = R.TARGET
    src = R.Cam(2 * t.width, 2 * t.height, 2 * t.fx, 2 * t.fy, 2 * t.cx, 2 * t.cy)
    img = R.image(src, R.U16)
    assert np.array_equal(R.nearest(img, R.lens(src), t), img[::2, ::2])


def test_pixels_outside_the_source_are_zero():
    """Source B under the barrel lens leaves between 20 % and 60 % of the target outside (39.9 %), source A under the pincushion
    lens at least 1 % (3.0 %): both branches of `inside` are taken, and what is outside is 0."""
    npix = R.TARGET.width * R.TARGET.height
    for src, dist, lo, hi in ((R.SOURCE_B, R.BARREL, 0.20, 0.60), (R.SOURCE_A, R.PINCUSHION, 0.01, 1.0)):
        ln = R.lens(src, dist)
        counts = {}
        img = np.maximum(R.image(src, R.U16), 1)             # no zero in the source: a zero in the product is "outside"
        out = R.nearest(img, ln, R.TARGET, counts)
        assert counts["nonfinite"] == 0
        assert lo * npix <= counts["outside"] <= hi * npix, counts
        assert np.count_nonzero(out == 0) == counts["outside"]
        inside, iy, ix = R.inside_nearest(ln, *R.rect_map(ln, R.TARGET))
        assert np.array_equal(out[inside], img[iy[inside], ix[inside]])
    assert abs(R.nearest(np.ones((32, 40), np.uint8), R.lens(R.SOURCE_B, R.BARREL), R.TARGET).mean() - (1 - 0.399)) < 0.001


def test_a_map_that_is_not_finite_gives_zero():
    """k1 = k2 = k3 = 3e38 makes most of the map infinite (76 % with source A).  Where it is not finite both samplers give 0.  Where it is
    finite it is far outside the source (|sx| > 1e30): NEAREST gives 0 there too, so its whole product is 0; BILINEAR edge-extends
    by the contract and returns the source's corner pixel on that side -- which is 0 for an image whose border is 0, so for
    such an image every output of both samplers is 0.  A target whose principal point is a pixel centre has x = 0 on a column:
    0 * inf, a NaN, on top of the infinities."""
    ln = R.lens(R.SOURCE_A, R.NONFINITE)
    sx, sy = R.rect_map(ln, R.TARGET)
    finite = np.isfinite(sx) & np.isfinite(sy)
    assert 0.5 < np.count_nonzero(~finite) / finite.size < 0.9 and np.isinf(sx).any() and not np.isnan(sx).any()
    assert np.all(np.abs(sx[finite]) > 1e30) and np.all(np.abs(sy[finite]) > 1e30)
    centred = R.TARGET._replace(cx=32.0, cy=24.0)
    nx, ny = R.rect_map(ln, centred)
    assert np.isnan(nx).any() and np.isnan(ny).any()
    for kind in (R.GRAY8, R.U16):
        assert not R.rectify(np.maximum(R.image(R.SOURCE_A, kind), 1), kind, ln, centred)[np.isnan(nx) | np.isnan(ny)].any()
    for kind in (R.U8, R.U16, R.F32):
        assert not R.nearest(np.maximum(R.image(R.SOURCE_A, kind), 1).astype(R.image(R.SOURCE_A, kind).dtype), ln, R.TARGET).any()
    for kind in (R.GRAY8, R.RGB8):
        img = np.maximum(R.image(R.SOURCE_A, kind), 1)
        out = R.bilinear(img, ln, R.TARGET)
        assert not out[~finite].any()
        corner = img[np.where(sy[finite] > 0, -1, 0), np.where(sx[finite] > 0, -1, 0)]
        assert np.array_equal(out[finite], corner)
        img[0], img[-1], img[:, 0], img[:, -1] = 0, 0, 0, 0
        assert not R.bilinear(img, ln, R.TARGET).any()


def test_float_map_is_close_to_the_double_map():
    """(recorded in the header for the large sizes, asserted here only at 64 x 48 with a loose bound)"""
    for src, dist in ((R.SOURCE_A, R.PINCUSHION), (R.SOURCE_B, R.BARREL)):
        ln = R.lens(src, dist)
        sx, sy = R.rect_map(ln, R.TARGET)
        dx, dy = R.rect_map_double(ln, R.TARGET)
        assert max(np.max(np.abs(sx - dx)), np.max(np.abs(sy - dy))) < 1e-4


# ---- header and binding -----------------------------------------------------------------------------------------------------------
NEW_CALLS = ("roft_default_lens", "roft_rectify_map", "roft_rectify", "roft_engine_enable_rectification", "roft_engine_get_rectify_stats",
             "roft_debug_rectify_kernel_ms")


def test_header_declares_and_binding_has_the_calls():
    declared = {p.name: p for p in abi_header.prototypes()}
    rows = {f.name: f for f in L.ABI}
    lib = L.lib()
    for name in NEW_CALLS:
        assert name in declared and name in rows and hasattr(lib, name), name
    assert {s.name for s in abi_header.structs()} >= {"roft_lens", "roft_engine_rectify_stats"}
    values, _ = abi_header.defines()
    assert [values["ROFT_RECTIFY_" + k] for k in ("GRAY8", "RGB8", "U8", "U16", "F32")] == [R.GRAY8, R.RGB8, R.U8, R.U16, R.F32]
    assert (L.RECTIFY_GRAY8, L.RECTIFY_RGB8, L.RECTIFY_U8, L.RECTIFY_U16, L.RECTIFY_F32) == (R.GRAY8, R.RGB8, R.U8, R.U16, R.F32)
    assert values["ROFT_ABI_VERSION"] == 2 and L.ABI_VERSION == 2 and lib.roft_abi_version() == 2
    assert "(3g)" in open(abi_header.HEADER).read()


def test_default_lens_is_the_identity():
    cam = L.Camera(64, 48, 60.0, 61.0, 30.2, 24.9)
    ln = L.Lens()
    ln.k1 = 5.0
    assert L.lib().roft_default_lens(C.byref(ln), C.byref(cam)) == 0
    assert (ln.cam.width, ln.cam.height, ln.cam.fx, ln.cam.fy, ln.cam.cx, ln.cam.cy) == (64, 48, 60.0, 61.0, 30.2, 24.9)
    assert (ln.k1, ln.k2, ln.p1, ln.p2, ln.k3) == (0.0,) * 5
    assert L.lib().roft_default_lens(None, C.byref(cam)) == L.ERR_INVALID and L.lib().roft_default_lens(C.byref(ln), None) == L.ERR_INVALID


# ---- refusals, before a device is looked for ----------------------------------------------------------------------------------------
def _cam(c=R.TARGET, **over):
    d = dict(c._asdict(), **over)
    return L.Camera(d["width"], d["height"], d["fx"], d["fy"], d["cx"], d["cy"])


def _lens(cam=None, dist=(0.0,) * 5):
    return L.Lens(cam if cam is not None else _cam(R.SOURCE_A), *dist)


BAD = [
    ("null src", dict(src=None), "null"),
    ("null lens", dict(lens=None), "null"),
    ("null target", dict(target=None), "null"),
    ("null out", dict(out=None), "null"),
    ("kind 0", dict(kind=0), "kind"),
    ("kind 6", dict(kind=6), "kind"),
    ("k1 nan", dict(lens=_lens(dist=(math.nan, 0, 0, 0, 0))), "k1"),
    ("k2 inf", dict(lens=_lens(dist=(0, math.inf, 0, 0, 0))), "k2"),
    ("p1 -inf", dict(lens=_lens(dist=(0, 0, -math.inf, 0, 0))), "p1"),
    ("p2 nan", dict(lens=_lens(dist=(0, 0, 0, math.nan, 0))), "p2"),
    ("k3 too large for a float", dict(lens=_lens(dist=(0, 0, 0, 0, 1e39))), "k3"),
    ("source fx nan", dict(lens=_lens(_cam(R.SOURCE_A, fx=math.nan))), "source camera.*finite"),
    ("source cy inf", dict(lens=_lens(_cam(R.SOURCE_A, cy=math.inf))), "source camera.*finite"),
    ("source fy 0", dict(lens=_lens(_cam(R.SOURCE_A, fy=0.0))), "source camera.*focal"),
    ("source fx negative", dict(lens=_lens(_cam(R.SOURCE_A, fx=-70.0))), "source camera.*focal"),
    ("source too large", dict(lens=_lens(_cam(R.SOURCE_A, width=4096, height=4096))), r"source camera.*2\^24"),
    ("source width 0", dict(lens=_lens(_cam(R.SOURCE_A, width=0))), "source camera.*at least 1"),
    ("target cx nan", dict(target=_cam(cx=math.nan)), "target camera.*finite"),
    ("target fx 0", dict(target=_cam(fx=0.0)), "target camera.*focal"),
    ("target too large", dict(target=_cam(width=8192, height=2048)), r"target camera.*2\^24"),
    ("target height 0", dict(target=_cam(height=0)), "target camera.*at least 1"),
]


@pytest.mark.parametrize("name,over,reason", BAD, ids=[b[0] for b in BAD])
def test_operators_refuse_before_a_device_is_looked_for(name, over, reason):
    """ROFT_ERR_INVALID with its reason, also on a machine without a GPU (where anything accepted would be ROFT_ERR_DEVICE).  The
    buffers are 16 bytes long: a call that got past its checks would not be allowed to touch them."""
    import re
    lib = L.lib()
    buf = np.zeros(16, np.uint8)
    a = dict(src=buf.ctypes.data, kind=L.RECTIFY_U8, lens=_lens(), target=_cam(), out=buf.ctypes.data)
    a.update(over)
    ref = lambda s: None if s is None else C.byref(s)
    assert lib.roft_rectify(a["src"], a["kind"], ref(a["lens"]), ref(a["target"]), a["out"]) == L.ERR_INVALID, name
    assert re.search(reason, lib.roft_last_error_string().decode()), (name, lib.roft_last_error_string())
    if "kind" not in over and "src" not in over:
        assert lib.roft_rectify_map(ref(a["lens"]), ref(a["target"]), a["out"]) == L.ERR_INVALID, name
        assert re.search(reason, lib.roft_last_error_string().decode()), (name, lib.roft_last_error_string())


def test_ops_kind_by_dtype():
    assert ops._rectify_kind(np.zeros((2, 2), np.uint8), False) == L.RECTIFY_GRAY8
    assert ops._rectify_kind(np.zeros((2, 2), np.uint8), True) == L.RECTIFY_U8
    assert ops._rectify_kind(np.zeros((2, 2, 3), np.uint8), False) == L.RECTIFY_RGB8
    assert ops._rectify_kind(np.zeros((2, 2), np.uint16), False) == L.RECTIFY_U16
    assert ops._rectify_kind(np.zeros((2, 2), np.float32), False) == L.RECTIFY_F32
    with pytest.raises(TypeError):
        ops._rectify_kind(np.zeros((2, 2), np.float64), False)
