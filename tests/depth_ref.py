"""numpy restatement of the raw-depth contract (include/roft_engine.h section 3c), written from the contract's text: every step is
one float32 operation in the order the contract gives, so the GPU tests can ask the kernels for EQUAL bits.  Shared by
tests/test_raw_depth_cpu.py (the restatement's own properties: the test inputs are sharp) and tests/test_raw_depth_gpu.py."""
import collections

import numpy as np

MAX_SPAN = 16      # ROFT_DEPTH_ALIGN_MAX_SPAN
F = np.float32

Cam = collections.namedtuple("Cam", "width height fx fy cx cy")


def convert(raw, scale):
    """out = (float)d * scale: one float multiply, 0 stays 0."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint16
    return raw.astype(F) * F(scale)


def align(raw, scale, dcam, ccam, R=None, t=None, counts=None):
    """The frame `raw` of depth camera `dcam` registered to colour camera `ccam`, P_colour = R P_depth + t.  counts (a dict, optional)
    receives how often each branch of the contract was taken: behind (P_2 <= 0), nonfinite, offscreen (empty range after clipping),
    capped (span >= MAX_SPAN), and of the colour pixels: multiply (covered by more than one reading), uncovered."""
    raw = np.asarray(raw)
    assert raw.dtype == np.uint16 and raw.shape == (dcam.height, dcam.width)
    R = np.asarray(np.eye(3) if R is None else R, F).reshape(3, 3)
    t = np.asarray(np.zeros(3) if t is None else t, F).reshape(3)
    scale = F(scale)
    fxd, fyd, cxd, cyd = F(dcam.fx), F(dcam.fy), F(dcam.cx), F(dcam.cy)     # the cameras' doubles -> float, once
    fxc, fyc, cxc, cyc = F(ccam.fx), F(ccam.fy), F(ccam.cx), F(ccam.cy)
    Wc, Hc = ccam.width, ccam.height
    ys, xs = np.nonzero(raw)                                                 # d != 0
    d = raw[ys, xs].astype(np.uint32)
    z = d.astype(F) * scale
    keep = np.ones(d.shape, bool)
    uv = []
    with np.errstate(all="ignore"):
        for s in (F(-0.5), F(0.5)):
            px, py = xs.astype(F) + s, ys.astype(F) + s
            X = ((px - cxd) / fxd) * z
            Y = ((py - cyd) / fyd) * z
            P = [((R[i, 0] * X + R[i, 1] * Y) + R[i, 2] * z) + t[i] for i in range(3)]
            front = P[2] > F(0)
            keep &= front
            u = (P[0] / P[2]) * fxc + cxc
            v = (P[1] / P[2]) * fyc + cyc
            assert u.dtype == F and v.dtype == F and X.dtype == F and P[2].dtype == F
            uv.append((u, v))
        n_behind = int(np.count_nonzero(~keep))
        (u0, v0), (u1, v1) = uv
        finite = np.isfinite(u0) & np.isfinite(v0) & np.isfinite(u1) & np.isfinite(v1)
        n_nonfinite = int(np.count_nonzero(keep & ~finite))
        keep &= finite
        x0 = np.maximum(np.ceil(u0), F(0))
        x1 = np.minimum(np.ceil(u1) - F(1), F(Wc - 1))
        y0 = np.maximum(np.ceil(v0), F(0))
        y1 = np.minimum(np.ceil(v1) - F(1), F(Hc - 1))
        empty = (x1 < x0) | (y1 < y0)
        n_offscreen = int(np.count_nonzero(keep & empty))
        keep &= ~empty
        capped = ((x1 - x0) >= F(MAX_SPAN)) | ((y1 - y0) >= F(MAX_SPAN))
        n_capped = int(np.count_nonzero(keep & capped))
        keep &= ~capped
    x0, x1, y0, y1 = (a[keep].astype(np.int64) for a in (x0, x1, y0, y1))
    d = d[keep]
    NONE = np.uint32(0xFFFFFFFF)
    key = np.full(Wc * Hc, NONE, np.uint32)
    cover = np.zeros(Wc * Hc, np.int64)
    for dy in range(MAX_SPAN):
        rows = y0 + dy <= y1
        if not rows.any():
            break
        for dx in range(MAX_SPAN):
            m = rows & (x0 + dx <= x1)
            if not m.any():
                break
            idx = (y0[m] + dy) * Wc + (x0[m] + dx)
            assert idx.min() >= 0 and idx.max() < Wc * Hc
            np.minimum.at(key, idx, d[m])       # the MINIMUM RAW VALUE of all source pixels that cover the target
            np.add.at(cover, idx, 1)
    out = np.where(key == NONE, F(0), key.astype(F) * scale).astype(F).reshape(Hc, Wc)
    if counts is not None:
        counts.update(behind=n_behind, nonfinite=n_nonfinite, offscreen=n_offscreen, capped=n_capped,
                      multiply=int(np.count_nonzero(cover > 1)), uncovered=int(np.count_nonzero(cover == 0)), cover=cover.reshape(Hc, Wc))
    return out


# ---- the cases both test files use --------------------------------------------------------------------------------------------
def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])


def block_frame(W, H, scale=0.001, seed=7):
    """A 0.4 m block over a 1.0 m background with a few millimetres of seeded relief, a strip of missing readings, and the values
    0, 1 and 65535 present."""
    rng = np.random.default_rng(seed)
    raw = np.full((H, W), round(1.0 / scale), np.int64) + rng.integers(-3, 4, (H, W))
    raw[H // 4:H // 4 + H // 3, W // 3:W // 3 + W // 3] = round(0.4 / scale) + rng.integers(-2, 3, (H // 3, W // 3))
    raw[H - 4:H - 2, 2:W // 2] = 0
    raw = np.clip(raw, 0, 65535).astype(np.uint16)
    raw[1, 1], raw[1, 2], raw[2, 1] = 0, 1, 65535
    return raw


def general_case(t=(0.015, 0.002, -0.0005), f_colour=56.0, scale=0.001):
    """A 48 x 40 depth image into a 64 x 48 colour camera: focal lengths 40 and 56 (f_colour), a 1.5 degree rotation about y, a
    15 mm baseline.  Returns dict(raw, scale, dcam, ccam, R, t)."""
    dcam = Cam(48, 40, 40.0, 40.0, 23.5, 19.5)
    ccam = Cam(64, 48, f_colour, f_colour, 31.5, 23.5)
    return dict(raw=block_frame(48, 40, scale), scale=scale, dcam=dcam, ccam=ccam, R=rot_y(1.5), t=np.array(t))


def times_two_case(scale=0.001):
    """An exact x2 camera: fx 30 -> 60, cx 15.5 -> 32.5, cy 11.5 -> 24.5, so that the footprint edges fall on half-integers --
    reading (x, y) is replicated into the 2 x 2 block at (2 x + 1, 2 y + 1), no holes, no overlaps; the colour image is 66 x 50, so
    the blocks fill columns 1 .. 64 and rows 1 .. 48 and leave a border of one pixel that nobody covers."""
    dcam = Cam(32, 24, 30.0, 30.0, 15.5, 11.5)
    ccam = Cam(66, 50, 60.0, 60.0, 32.5, 24.5)
    raw = block_frame(32, 24, scale, seed=11)
    raw[raw == 0] = 500      # (no missing readings: every colour pixel is covered exactly once)
    return dict(raw=raw, scale=scale, dcam=dcam, ccam=ccam, R=np.eye(3), t=np.zeros(3))


def identity_case(W=37, H=5, scale=0.001):
    cam = Cam(W, H, 31.0, 29.0, (W - 1) / 2.0, (H - 1) / 2.0)
    rng = np.random.default_rng(W * 100 + H)
    raw = rng.integers(200, 3000, (H, W)).astype(np.uint16)
    raw[0, :3] = [0, 1, 65535]
    return dict(raw=raw, scale=scale, dcam=cam, ccam=cam, R=np.eye(3), t=np.zeros(3))


def run(case, counts=None):
    return align(case["raw"], case["scale"], case["dcam"], case["ccam"], case["R"], case["t"], counts)
