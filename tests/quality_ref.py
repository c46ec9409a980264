"""Reference of track quality, written from the text of include/roft_engine.h (section 3d), not from the kernel: the tile comes
from the oracle's render_depth (pinned bit for bit against the HIP rasteriser elsewhere), the counts are boolean arrays, the sum
of |e| is a pair of Python integers in units of 2^-32 and 2^-64."""
import sys

import numpy as np

DBL_MAX = sys.float_info.max
FIELDS = ("frame", "n_mask", "n_render", "n_both", "n_depth", "n_front", "n_behind", "reserved", "depth_err")


def term_integers(t):
    """(hi, lo) of one term t = |e| (a float32, or any non-negative double): t' = min(t, 256); hi = floor(t' 2^32); lo = the integer
    part of (t' 2^32 - hi) 2^32.  In doubles, as the header states it; both products are exact for t >= 2^-41."""
    ts = min(float(t), 256.0) * 4294967296.0
    hi = int(np.floor(ts))
    lo = int((ts - float(hi)) * 4294967296.0)
    return hi, lo


def value(hi, lo):
    """value(HI, LO) = (double)HI 2^-32 + (double)LO 2^-64: two conversions (round to nearest even: Python's int -> float), two exact
    multiplications, one addition."""
    return float(hi) * (1.0 / 4294967296.0) + float(lo) * (1.0 / 4294967296.0 / 4294967296.0)


def upsample(tile, d, H, W):
    """r of every image pixel: R[v // d][u // d] where v // d < h and u // d < w, else 0 (no render value)."""
    h, w = tile.shape
    r = np.zeros((H, W), np.float32)
    r[:h * d, :w * d] = np.repeat(np.repeat(tile, d, axis=0), d, axis=1)
    return r


def quality_from_tile(tile, d, mask_bits, depth, depth_tolerance, depth_maximum, frame=0, check_exact=None):
    """The record (a dict over FIELDS) from R, M (boolean [H, W]) and D (float32 [H, W]).  check_exact: a list that receives, for every
    sample, whether the fixed-point image of |e| equals |e|."""
    H, W = mask_bits.shape
    depth = np.asarray(depth, np.float32)
    tol = np.float32(depth_tolerance)
    r = upsample(np.asarray(tile, np.float32), d, H, W)
    M = np.asarray(mask_bits, bool)
    Rm = r != 0
    both = M & Rm
    with np.errstate(invalid="ignore"):
        valid = both & (depth > 0) & (depth.astype(np.float64) < float(depth_maximum))   # (NaN fails both)
    e = (depth[valid] - r[valid]).astype(np.float32)   # one float subtraction
    hi = lo = 0
    for t in np.abs(e):
        h_, l_ = term_integers(t)
        hi += h_
        lo += l_
        if check_exact is not None:
            check_exact.append(h_ * 2 ** 32 + l_ == int(float(t) * 2.0 ** 64) and float(t) * 2.0 ** 64 == int(float(t) * 2.0 ** 64))
    n_depth = int(valid.sum())
    return dict(frame=frame, n_mask=int(M.sum()), n_render=int(Rm.sum()), n_both=int(both.sum()), n_depth=n_depth,
                n_front=int((e < -tol).sum()), n_behind=int((e > tol).sum()), reserved=0,
                depth_err=value(hi, lo) / float(n_depth) if n_depth else DBL_MAX)


def quality(ob, cam, d, depth, mask_bits, mesh, x, q, depth_tolerance=0.01, depth_maximum=2.0, frame=0, check_exact=None):
    """ob: the oracle binding; cam: its camera; mesh: (verts, tris) or None (an object without a mesh: R = 0)."""
    H, W = np.asarray(mask_bits).shape
    if mesh is None or len(mesh[1]) == 0:
        tile = np.zeros((H // d, W // d), np.float32)
    else:
        tile = ob.render_depth(ob.make_mesh(*mesh), x, q, cam, d)
    return quality_from_tile(tile, d, mask_bits, depth, depth_tolerance, depth_maximum, frame, check_exact)


def none_record():
    rec = dict.fromkeys(FIELDS, 0)
    rec["frame"] = -1
    rec["depth_err"] = 0.0
    return rec


def as_dict(rec):
    """A numpy record (ops.QUALITY_DTYPE) or ctypes struct -> dict over FIELDS with Python numbers."""
    return {k: (float(rec[k]) if k == "depth_err" else int(rec[k])) for k in FIELDS}


def same(a, b):
    """Bit for bit: the eight integers, and depth_err as doubles."""
    return all(int(a[k]) == int(b[k]) for k in FIELDS[:-1]) and np.float64(a["depth_err"]).tobytes() == np.float64(b["depth_err"]).tobytes()
