"""numpy restatement of the lens-distortion contract (include/roft_engine.h section 3g), written from the contract's text: every
step is one float32 operation in the order the contract gives, so the GPU tests can ask the kernel for EQUAL bits.  Shared by
tests/test_rectify_cpu.py (the restatement's own properties: the test inputs are sharp), tests/test_rectify_gpu.py and
tests/test_rectify_engine_gpu.py."""
import collections

import numpy as np

F = np.float32

Cam = collections.namedtuple("Cam", "width height fx fy cx cy")
Lens = collections.namedtuple("Lens", "cam k1 k2 p1 p2 k3")

GRAY8, RGB8, U8, U16, F32 = 1, 2, 3, 4, 5     # ROFT_RECTIFY_*


def lens(cam, dist=(0.0, 0.0, 0.0, 0.0, 0.0)):
    return Lens(cam, *dist)


def rect_map(ln, tgt):
    """(sx, sy), each [H, W] float32: where in the source image target pixel (u, v) reads."""
    fx, fy, cx, cy = F(tgt.fx), F(tgt.fy), F(tgt.cx), F(tgt.cy)                    # the cameras' doubles -> float, once
    fxs, fys, cxs, cys = F(ln.cam.fx), F(ln.cam.fy), F(ln.cam.cx), F(ln.cam.cy)
    k1, k2, p1, p2, k3 = F(ln.k1), F(ln.k2), F(ln.p1), F(ln.p2), F(ln.k3)
    u = np.arange(tgt.width).astype(F)[None, :]
    v = np.arange(tgt.height).astype(F)[:, None]
    one, two = F(1), F(2)
    with np.errstate(all="ignore"):
        x = (u - cx) / fx
        y = (v - cy) / fy
        xx = x * x
        yy = y * y
        xy = x * y
        r2 = xx + yy
        rad = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        tx = (two * p1) * xy + p2 * (r2 + two * xx)
        ty = p1 * (r2 + two * yy) + (two * p2) * xy
        xd = x * rad + tx
        yd = y * rad + ty
        sx = xd * fxs + cxs
        sy = yd * fys + cys
    for a in (x, y, r2, rad, tx, ty, sx, sy):
        assert a.dtype == F
    shape = (tgt.height, tgt.width)
    return np.broadcast_to(sx, shape).copy(), np.broadcast_to(sy, shape).copy()


def rect_map_double(ln, tgt):
    """the same formula in double (from the float intrinsics and coefficients): what the float map is measured against"""
    fx, fy, cx, cy = (float(F(a)) for a in (tgt.fx, tgt.fy, tgt.cx, tgt.cy))
    fxs, fys, cxs, cys = (float(F(a)) for a in (ln.cam.fx, ln.cam.fy, ln.cam.cx, ln.cam.cy))
    k1, k2, p1, p2, k3 = (float(F(a)) for a in (ln.k1, ln.k2, ln.p1, ln.p2, ln.k3))
    x = ((np.arange(tgt.width, dtype=float) - cx) / fx)[None, :]
    y = ((np.arange(tgt.height, dtype=float) - cy) / fy)[:, None]
    r2 = x * x + y * y
    rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return xd * fxs + cxs, yd * fys + cys


def inside_nearest(ln, sx, sy):
    """(inside, jy, jx): the contract's float test, and the integer indices where it holds (0 elsewhere)"""
    Ws, Hs = ln.cam.width, ln.cam.height
    with np.errstate(all="ignore"):
        jx = np.floor(sx + F(0.5))
        jy = np.floor(sy + F(0.5))
        inside = (jx >= F(0)) & (jx <= F(Ws - 1)) & (jy >= F(0)) & (jy <= F(Hs - 1))
    assert jx.dtype == F
    ix = np.where(inside, jx, F(0)).astype(np.int64)
    iy = np.where(inside, jy, F(0)).astype(np.int64)
    return inside, iy, ix


def nearest(src, ln, tgt, counts=None):
    """depth (uint16 / float32), masks and label images (uint8 / uint16)"""
    src = np.asarray(src)
    assert src.shape == (ln.cam.height, ln.cam.width) and src.dtype in (np.uint8, np.uint16, np.float32)
    sx, sy = rect_map(ln, tgt)
    inside, iy, ix = inside_nearest(ln, sx, sy)
    if counts is not None:
        counts.update(outside=int(np.count_nonzero(~inside)), nonfinite=int(np.count_nonzero(~(np.isfinite(sx) & np.isfinite(sy)))))
    return np.where(inside, src[iy, ix], src.dtype.type(0)).astype(src.dtype)


def bilinear(src, ln, tgt):
    """8-bit images, [H, W] or [H, W, 3] (the channels independently)"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.shape[:2] == (ln.cam.height, ln.cam.width)
    if src.ndim == 3:
        return np.stack([bilinear(np.ascontiguousarray(src[:, :, c]), ln, tgt) for c in range(src.shape[2])], axis=2)
    Ws, Hs = ln.cam.width, ln.cam.height
    sx, sy = rect_map(ln, tgt)
    finite = np.isfinite(sx) & np.isfinite(sy)
    sx, sy = np.where(finite, sx, F(0)), np.where(finite, sy, F(0))
    one = F(1)
    x0, y0 = np.floor(sx), np.floor(sy)
    ax, ay = sx - x0, sy - y0
    c0 = np.clip(x0, F(0), F(Ws - 1)).astype(np.int64)          # clamped in float, then converted
    c1 = np.clip(x0 + one, F(0), F(Ws - 1)).astype(np.int64)
    r0 = np.clip(y0, F(0), F(Hs - 1)).astype(np.int64)
    r1 = np.clip(y0 + one, F(0), F(Hs - 1)).astype(np.int64)
    p = src.astype(F)
    top = (one - ax) * p[r0, c0] + ax * p[r0, c1]
    bot = (one - ax) * p[r1, c0] + ax * p[r1, c1]
    val = (one - ay) * top + ay * bot
    assert val.dtype == F and ax.dtype == F
    out = np.minimum(np.rint(val), F(255)).astype(np.uint8)
    out[~finite] = 0
    return out


def rectify(src, kind, ln, tgt):
    return bilinear(src, ln, tgt) if kind in (GRAY8, RGB8) else nearest(src, ln, tgt)


def gray(image, rgb=True):
    """OpenCV's 8-bit COLOR_BGR2GRAY (include/roft_engine.h section 3a); rgb: the first channel is red"""
    img = np.asarray(image).astype(np.uint32)
    r, b = (img[:, :, 0], img[:, :, 2]) if rgb else (img[:, :, 2], img[:, :, 0])
    return ((r * 4899 + img[:, :, 1] * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


# ---- the cases the test files use ---------------------------------------------------------------------------------------------
TARGET = Cam(64, 48, 60.0, 60.0, 31.5, 23.5)
SOURCE_A = Cam(80, 60, 70.0, 71.0, 40.2, 29.6)
SOURCE_B = Cam(40, 32, 52.0, 53.0, 19.7, 16.4)
BARREL = (-0.30, 0.10, 0.010, -0.005, 0.02)
PINCUSHION = (0.25, 0.05, -0.004, 0.006, 0.0)
NONFINITE = (3e38, 3e38, 0.0, 0.0, 3e38)      # k1 = k2 = k3 = 3e38: part of the map overflows to inf and inf - inf


def target(W, H):
    """the test target at another size: f = 60, the principal point in the middle"""
    return Cam(W, H, 60.0, 60.0, (W - 1) / 2.0, (H - 1) / 2.0)


def image(cam, kind, seed=0):
    """a seeded source image of `cam`'s size in the layout of `kind`: every value of the type's range can occur, 0 included"""
    rng = np.random.default_rng(1000 * seed + 10 * kind + cam.width)
    H, W = cam.height, cam.width
    if kind == RGB8:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind in (GRAY8, U8):
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind == U16:
        return rng.integers(0, 65536, (H, W), dtype=np.uint16)
    return rng.uniform(0.1, 3.0, (H, W)).astype(F)
