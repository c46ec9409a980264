"""The forward-backward check of include/roft_engine.h section 3f restated in numpy: float32 throughout, every product and
every sum a separate rounded operation (numpy never fuses), in the header's order.  check(F, B, tol_abs, tol_rel) returns the
checked field; parts(...) also the two masks the tests ask about."""
import numpy as np

f32 = np.float32
INVALID_BITS = 0x7FC00000


def parts(F, B, tol_abs=0.5, tol_rel=0.01):
    """(inside, valid, e2) per pixel [H, W]: the `inside` rule alone, inside && threshold, and the squared error (NaN outside)"""
    F = np.ascontiguousarray(F, f32)
    B = np.ascontiguousarray(B, f32)
    H, W = F.shape[:2]
    tol_abs, tol_rel = f32(tol_abs), f32(tol_rel)
    xs = np.arange(W, dtype=np.int64).astype(f32)[None, :]
    ys = np.arange(H, dtype=np.int64).astype(f32)[:, None]
    fx, fy = F[..., 0], F[..., 1]
    with np.errstate(all="ignore"):
        xf = xs + fx
        yf = ys + fy
        inside = (xf >= f32(0)) & (xf <= f32(W - 1)) & (yf >= f32(0)) & (yf <= f32(H - 1))
        # outside pixels read nothing: give them a harmless target
        xg = np.where(inside, xf, f32(0)).astype(f32)
        yg = np.where(inside, yf, f32(0)).astype(f32)
        x0f, y0f = np.floor(xg), np.floor(yg)
        ax, ay = (xg - x0f).astype(f32), (yg - y0f).astype(f32)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        sx, sy = (f32(1) - ax).astype(f32), (f32(1) - ay).astype(f32)
        b = []
        for c in range(2):
            Bc = B[..., c]
            top = (sx * Bc[y0, x0]).astype(f32) + (ax * Bc[y0, x1]).astype(f32)
            bot = (sx * Bc[y1, x0]).astype(f32) + (ax * Bc[y1, x1]).astype(f32)
            b.append(((sy * top).astype(f32) + (ay * bot).astype(f32)).astype(f32))
        bx, by = b
        ex, ey = (fx + bx).astype(f32), (fy + by).astype(f32)
        e2 = ((ex * ex).astype(f32) + (ey * ey).astype(f32)).astype(f32)
        m2 = (((fx * fx).astype(f32) + (fy * fy).astype(f32)).astype(f32) + ((bx * bx).astype(f32) + (by * by).astype(f32)).astype(f32)).astype(f32)
        bound = ((tol_rel * m2).astype(f32) + tol_abs).astype(f32)
        valid = inside & (e2 <= bound)
    assert e2.dtype == f32 and bound.dtype == f32
    return inside, valid, np.where(inside, e2, f32(np.nan))


def check(F, B, tol_abs=0.5, tol_rel=0.01):
    _, valid, _ = parts(F, B, tol_abs, tol_rel)
    out = np.ascontiguousarray(F, f32).copy()
    out.view(np.uint32)[~valid] = INVALID_BITS
    return out


def invalid(flow):
    """pixels carrying the invalid pattern in both components"""
    return (np.ascontiguousarray(flow, f32).view(np.uint32) == INVALID_BITS).all(axis=2)
