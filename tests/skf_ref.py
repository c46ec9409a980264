"""Exact reference of the velocity filter's correction (SKFCorrection::correctStep) and the table of cases that aim at every
median route, storage path and branch of roft_amd/csrc/k_skf.hip.

The reference is the information form in extended precision,
    e = y - H x,   l_j = max(exp(-|n_j - m| / b) / (2 b), 1e-6) / max_j(.),
    P+ = (P^-1 + sum_j l_j H_j' R^-1 H_j)^-1,   x+ = x + P+ sum_j l_j H_j' R^-1 e_j,
with m the median (numpy.sort: an exact order statistic, the mean of the two middle values for even N) and b the mean
absolute deviation of the norms sqrt(e[k]^2 + e[N + k]^2) -- the reference's COLUMN-major pairing -- while n_j is the true norm of
point j.  Arithmetic: numpy.longdouble where it carries at least 63 mantissa bits (x86), else mpmath at 100 bits; no third way.
The 6 x 6 inverses are Gauss-Jordan with partial pivoting, polished by Newton steps X <- X (2 I - A X).

skf_exact(..., mutation=...) computes deliberately WRONG variants (a median rank off by one, exchanged noise variances, ...):
tests/test_skf_ref_cpu.py demands that each case moves by more than 1e3 x SKF_RTOL under the mutations it is meant to catch,
so a kernel that takes the wrong branch cannot hide below the bar of tests/test_skf_paths_gpu.py.
"""
import functools
from collections import namedtuple

import numpy as np

MUTATIONS = ("rank_lo", "rank_hi", "rank_dup", "rswap", "noclamp", "rowmajor", "bswap", "reweight")


# ---------------------------------------------------------------------------------------------
# arithmetic
# ---------------------------------------------------------------------------------------------
class _LongDouble:
    name = "longdouble"

    @staticmethod
    def arr(a):
        return np.asarray(a, dtype=np.longdouble)

    sqrt = staticmethod(np.sqrt)
    exp = staticmethod(np.exp)

    @staticmethod
    def f64(a):
        return np.asarray(a, dtype=np.float64)


class _MpMath:
    name = "mpmath"

    def __init__(self):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.prec = 100
        self._cv = np.frompyfunc(lambda v: v if isinstance(v, self.mp.mpf) else self.mp.mpf(float(v)), 1, 1)
        self.sqrt = np.frompyfunc(self.mp.sqrt, 1, 1)
        self.exp = np.frompyfunc(self.mp.exp, 1, 1)

    def arr(self, a):
        a = np.asarray(a)
        out = self._cv(a)
        return out if isinstance(out, np.ndarray) else np.array(out, dtype=object)

    @staticmethod
    def f64(a):
        return np.array([float(v) for v in np.asarray(a, dtype=object).ravel()], dtype=np.float64).reshape(np.shape(a))


@functools.lru_cache(maxsize=None)
def backend(name=None):
    """The arithmetic of the reference: "longdouble", "mpmath", or None = the best one this machine has."""
    if name is None:
        if np.finfo(np.longdouble).nmant >= 63:
            name = "longdouble"
        else:
            try:
                import mpmath  # noqa: F401
                name = "mpmath"
            except ImportError:
                raise RuntimeError("tests/skf_ref.py needs numpy.longdouble with >= 63 mantissa bits (this one has %d) or mpmath; "
                                   "neither is available, and a double-precision reference would pin nothing"
                                   % np.finfo(np.longdouble).nmant)
    if name == "longdouble":
        if np.finfo(np.longdouble).nmant < 63:
            raise RuntimeError("numpy.longdouble has only %d mantissa bits here" % np.finfo(np.longdouble).nmant)
        return _LongDouble()
    if name == "mpmath":
        return _MpMath()
    raise ValueError(name)


def _eye(B):
    return B.arr(np.eye(6))


def _inverse6(B, A):
    """Gauss-Jordan with partial pivoting + three Newton steps."""
    n = A.shape[0]
    M = np.concatenate([A.copy(), _eye(B)], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if p != k:
            M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for i in range(n):
            if i != k:
                M[i] = M[i] - M[i, k] * M[k]
    X = M[:, n:]
    two_i = 2 * _eye(B)
    for _ in range(3):
        X = X @ (two_i - A @ X)
    return X


def _is_spd(A):
    """Cholesky in the reference's arithmetic: every pivot positive (a NaN compares false)."""
    n = A.shape[0]
    Lc = A.copy()
    for k in range(n):
        d = Lc[k, k]
        if not (d > 0):
            return False
        for i in range(k + 1, n):
            f = Lc[i, k] / d
            Lc[i, k + 1:] = Lc[i, k + 1:] - f * Lc[k, k + 1:]
    return True


# ---------------------------------------------------------------------------------------------
# the correction
# ---------------------------------------------------------------------------------------------
def skf_exact(x_pred, P_pred, y, H, rdiag=(1.0, 1.0), reweight=True, mutation=None, backend_name=None, info=None):
    """(status, x+, P+) as float64 arrays rounded from the extended-precision result.  y: 2N, H: 2N x 6 (doubles, or arrays of
    the backend's own type from yh_from_points).  status 0 corrected, 1 N == 0, 3 P_pred or the information matrix not positive
    definite (belief unchanged).  `info`, if a dict, receives mi, b, weighted and n_clamped."""
    assert mutation is None or mutation in MUTATIONS, mutation
    B = backend(backend_name)
    x0, P0 = np.array(x_pred, dtype=np.float64).reshape(6), np.array(P_pred, dtype=np.float64).reshape(6, 6)
    y = B.arr(y).reshape(-1)
    H = B.arr(H).reshape(-1, 6)
    N = y.size // 2
    if N <= 0:
        return 1, x0, P0
    x, P = B.arr(x0), B.arr(P0)
    r = B.arr(np.array(rdiag, dtype=np.float64))
    if mutation == "rswap":
        r = r[::-1]
    if not _is_spd(P):
        return 3, x0, P0

    e = y - H @ x
    lik = B.arr(np.ones(N))
    if bool(reweight) != (mutation == "reweight"):
        if mutation == "rowmajor":
            a, c = e[0::2], e[1::2]
        else:
            a, c = e[:N], e[N:]      # Map<MatrixXd>(data, N, 2) is column major
        norms = np.sort(B.sqrt(a * a + c * c))
        lo, hi = (N // 2 - 1, N // 2) if N % 2 == 0 else (N // 2, N // 2)
        if mutation == "rank_lo":
            lo, hi = max(lo - 1, 0), max(hi - 1, 0)
        elif mutation == "rank_hi":
            lo, hi = min(lo + 1, N - 1), min(hi + 1, N - 1)
        elif mutation == "rank_dup":
            hi = lo
        mi = (norms[lo] + norms[hi]) / 2
        b = np.sum(np.abs(norms - mi)) / N
        weighted = bool(b > B.arr(1e-4))
        if mutation == "bswap":
            weighted = not weighted
        n_clamped = 0
        if weighted:
            nj = B.sqrt(e[0::2] * e[0::2] + e[1::2] * e[1::2])
            l = B.exp(-np.abs(nj - mi) / b) / (2 * b)
            floor = B.arr(1e-6)
            low = np.array(l < floor, dtype=bool)
            n_clamped = int(low.sum())
            if mutation != "noclamp":
                l = np.where(low, floor, l)
            lik = l / np.max(l)
        if info is not None:
            info.update(mi=float(mi), b=float(b), weighted=weighted, n_clamped=n_clamped)

    w = np.empty(2 * N, dtype=lik.dtype)
    w[0::2] = lik / r[0]
    w[1::2] = lik / r[1]
    Lam = _inverse6(B, P) + H.T @ (H * w[:, None])
    if not _is_spd(Lam):
        return 3, x0, P0
    Pp = _inverse6(B, Lam)
    Pp = (Pp + Pp.T) / 2
    xo = x + Pp @ (H.T @ (w * e))
    return 0, B.f64(xo), B.f64(Pp)


Camera = namedtuple("Camera", "width height fx fy cx cy")
CAM_VGA = Camera(640, 480, 614.0, 611.5, 320.0, 240.0)       # integer principal point: u = cx and v = cy are pixels
CAM_HD = Camera(1920, 1080, 1380.25, 1377.75, 960.0, 540.0)


def _h_rows(fx, fy, cx, cy, dt, u, v, z):
    """The literal expression of ImageOpticalFlowMeasurement.hpp:279-280 (h_rows() of k_skf.hip) in the type of its arguments."""
    uu, vv = u - cx, v - cy
    zero = 0 * z
    r0 = [(fx / z) * dt, zero, (-uu / z) * dt, (-uu * vv / fy) * dt, (fx + uu * uu / fx) * dt, (-vv * fx / fy) * dt]
    r1 = [zero, (fy / z) * dt, (-vv / z) * dt, (-(fy + vv * vv / fy)) * dt, (vv * uu / fx) * dt, (uu * fy / fx) * dt]
    n = z.shape[0]
    H = np.empty((2 * n, 6), dtype=z.dtype)
    for i in range(6):
        H[0::2, i] = r0[i]
        H[1::2, i] = r1[i]
    return H


def yh_from_points(cam, dt, uv, z, flow_xy, backend_name=None):
    """(y, H) of flow points in the backend's extended type: u, v integers, z and the flow float32 (widened exactly)."""
    B = backend(backend_name)
    uv = np.asarray(uv, np.int32).reshape(-1, 2)
    z = B.arr(np.asarray(z, np.float32).astype(np.float64))
    y = B.arr(np.asarray(flow_xy, np.float32).astype(np.float64).reshape(-1))
    c = [B.arr(np.float64(t)) for t in (cam.fx, cam.fy, cam.cx, cam.cy, dt)]
    H = _h_rows(c[0], c[1], c[2], c[3], c[4], B.arr(uv[:, 0].astype(np.float64)), B.arr(uv[:, 1].astype(np.float64)), z)
    return y, H


def yh_from_points_f64(cam, dt, uv, z, flow_xy):
    """The same literal divisions in IEEE double, operation for operation what expand_yh_kernel / ro_flow_measurement do."""
    uv = np.asarray(uv, np.int32).reshape(-1, 2)
    z = np.asarray(z, np.float32).astype(np.float64)
    y = np.asarray(flow_xy, np.float32).astype(np.float64).reshape(-1)
    H = _h_rows(np.float64(cam.fx), np.float64(cam.fy), np.float64(cam.cx), np.float64(cam.cy), np.float64(dt),
                uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64), z)
    return y, H


def skf_exact_points(cam, dt, x_pred, P_pred, uv, z, flow_xy, rdiag=(1.0, 1.0), reweight=True, backend_name=None, info=None):
    y, H = yh_from_points(cam, dt, uv, z, flow_xy, backend_name)
    return skf_exact(x_pred, P_pred, y, H, rdiag, reweight, backend_name=backend_name, info=info)


def deviation(x, P, x_ref, P_ref):
    """(dx, dP): max |x - x_ref| / max |x_ref| (absolute where x_ref == 0) and max |P - P_ref| / max |P_ref|."""
    sx = float(np.max(np.abs(x_ref)))
    dx = float(np.max(np.abs(x - x_ref))) / (sx if sx > 0 else 1.0)
    dP = float(np.max(np.abs(P - P_ref)) / np.max(np.abs(P_ref)))
    return dx, dP


def assert_close(x, P, x_ref, P_ref, tol, what=""):
    """x within tol x max |x_ref| + 1e-15 (the floor serves the all-zero case), P within tol x max |P_ref|."""
    ex = float(np.max(np.abs(x - x_ref)))
    eP = float(np.max(np.abs(P - P_ref)))
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(P)), what
    assert ex <= tol * float(np.max(np.abs(x_ref))) + 1e-15, (what, "x", ex, float(np.max(np.abs(x_ref))))
    assert eP <= tol * float(np.max(np.abs(P_ref))), (what, "P", eP, float(np.max(np.abs(P_ref))))


# ---------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name family x_pred P_pred y H rdiag reweight mutations")
DT = 1.0 / 30.0
P_GENERIC = np.eye(6) * (1e-3 + 0.1)     # the tracker's P + Q after the first prediction


def random_points(rng, n, cam=CAM_VGA):
    uv = np.stack([rng.integers(0, cam.width, n), rng.integers(0, cam.height, n)], axis=1).astype(np.int32)
    z = rng.uniform(0.3, 1.5, n).astype(np.float32)
    return uv, z


def _random_H(rng, n):
    uv, z = random_points(rng, n)
    return yh_from_points_f64(CAM_VGA, DT, uv, z, np.zeros((n, 2), np.float32))[1]


def _y_from_norms(rng, norms, cluster=None):
    """y (2N) whose column-major pairs (y[k], y[N + k]) have the prescribed norms, up to the rounding of r cos, r sin; the
    members of `cluster` (a boolean array) share ONE pair, so that their norms are bit-identical in any arithmetic.  The order
    of the values is shuffled: neighbours in rank are not neighbours in thread order."""
    n = norms.size
    th = rng.uniform(0.0, 2.0 * np.pi, n)
    if cluster is not None:
        th[cluster] = th[cluster][0]
    perm = rng.permutation(n)
    r, th = norms[perm], th[perm]
    return np.concatenate([r * np.cos(th), r * np.sin(th)])


def _generic_y(rng, H, x_true):
    """Flow of a rigid motion + Laplacian pixel noise + 5 % gross outliers (flow vectors that lost their pixel)."""
    n = H.shape[0] // 2
    y = H @ x_true + rng.laplace(0.0, 0.5, 2 * n)
    bad = rng.random(n) < 0.05
    y[0::2][bad] += rng.uniform(-20.0, 20.0, int(bad.sum()))
    y[1::2][bad] += rng.uniform(-20.0, 20.0, int(bad.sum()))
    return y


X_TRUE = np.array([0.05, -0.03, 0.08, 0.2, -0.15, 0.1])


def _prescribed(name, family, seed, norms, mutations, cluster=None, rdiag=(1.0, 1.0)):
    rng = np.random.default_rng(seed)
    H = _random_H(rng, norms.size)
    return Case(name, family, np.zeros(6), P_GENERIC.copy(), _y_from_norms(rng, norms, cluster), H, rdiag, True, tuple(mutations))


def _generic(name, family, seed, n, mutations, rdiag=(1.0, 1.0), reweight=True, x_pred=None, P_pred=None):
    rng = np.random.default_rng(seed)
    H = _random_H(rng, n)
    y = _generic_y(rng, H, X_TRUE)
    return Case(name, family, np.zeros(6) if x_pred is None else x_pred, P_GENERIC.copy() if P_pred is None else P_pred, y, H,
                rdiag, reweight, tuple(mutations))


def _with_cluster(rng, n_below, n_cluster, n_above, value=1.0):
    """Sorted norms: n_below in [0.2, 0.9] x value, n_cluster identical values, n_above in [1.3, 3] x value with the smallest AT
    1.3 x value and the largest below AT 0.9 x value: the neighbours of the cluster are distinct and clearly apart."""
    lo = np.sort(rng.uniform(0.2, 0.9, n_below)) * value
    hi = np.sort(rng.uniform(1.3, 3.0, n_above)) * value
    if n_below:
        lo[-1] = 0.9 * value
    if n_above:
        hi[0] = 1.3 * value
    norms = np.concatenate([lo, np.full(n_cluster, value), hi])
    cluster = np.zeros(norms.size, bool)
    cluster[n_below:n_below + n_cluster] = True
    return norms, cluster


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in a fixed order.  `mutations` are the wrong variants the case is there to catch."""
    out = []
    seed = 7000

    def nxt():
        nonlocal seed
        seed += 1
        return seed

    # -- fallback through duplicates: 300 identical norms at the median share a bucket under any monotone binning.  A rank off by
    #    one stays inside the cluster by construction, so these cases pin the route (and the pairing), the next family the rank.
    for n in (600, 601):
        s = nxt()
        norms, cl = _with_cluster(np.random.default_rng(s), 150, 300, n - 450)
        out.append(_prescribed("dup_%d" % n, "fallback_duplicates", s, norms, ("rowmajor",), cl))
    # -- fallback, rank N/2 just outside the cluster (cnt_le / min_gt)
    s = nxt()
    norms, cl = _with_cluster(np.random.default_rng(s), 100, 300, 400)      # cluster = ranks 100 .. 399 = N/2 - 1
    out.append(_prescribed("dup_ends_below_rank_800", "fallback_rank_edge", s, norms, ("rank_lo", "rank_hi", "rank_dup"), cl))
    s = nxt()
    norms, cl = _with_cluster(np.random.default_rng(s), 400, 300, 100)      # cluster = ranks 400 = N/2 .. 699
    out.append(_prescribed("dup_starts_at_rank_800", "fallback_rank_edge", s, norms, ("rank_lo", "rank_hi", "rank_dup"), cl))
    # -- gross outliers: 8 x mean ~ 2.4e7, every other value in bin 0.  b ~ 3e6 puts every likelihood below the clamp.
    s = nxt()
    norms = np.random.default_rng(s).uniform(0.5, 1.5, 1000)
    norms[:3] = 1e9
    out.append(_prescribed("outliers_1000", "gross_outliers", s, norms, ("noclamp",)))
    # -- the two middle ranks in different buckets, no overflow
    for n in (1000, 999):
        s = nxt()
        r = np.random.default_rng(s)
        norms = np.concatenate([r.uniform(0.1, 0.2, 500), r.uniform(5.0, 6.0, n - 500)])
        out.append(_prescribed("straddle_%d" % n, "straddle", s, norms, ("rank_hi", "rank_dup") if n % 2 == 0 else ("rank_hi",)))
    # -- small buckets, a tie across the middle ranks N/2 - 1, N/2
    for n in (5, 8, 64, 65):
        s = nxt()
        norms = np.sort(np.random.default_rng(s).uniform(0.5, 4.0, n))
        norms[n // 2 - 1] = norms[n // 2]
        cl = np.zeros(n, bool)
        cl[n // 2 - 1:n // 2 + 1] = True
        out.append(_prescribed("ties_%d" % n, "small_ties", s, norms, ("rank_lo", "rank_hi") if n % 2 == 0 else ("rank_hi",), cl))
    # -- all zero: top == 0, unweighted, x+ = x exactly
    s = nxt()
    H = _random_H(np.random.default_rng(s), 100)
    out.append(Case("all_zero_100", "all_zero", np.zeros(6), P_GENERIC.copy(), np.zeros(200), H, (1.0, 1.0), True, ()))
    # -- b on either side of 1e-4 (uniform spread s around 1: b = s / 2)
    for tag, spread in (("below", 1e-4), ("above", 4e-4)):
        s = nxt()
        norms = 1.0 + spread * np.random.default_rng(s).uniform(-1.0, 1.0, 500)
        out.append(_prescribed("scale_switch_%s" % tag, "scale_switch", s, norms, ("bswap",)))
    # -- clamp.  |n - m| > 20 b for a tenth of the points is impossible (b, the MEAN of |n - m|, would exceed 2 b): the two
    #    cases are a tenth of the points as far out as a tenth can be (~ 9.6 b) and 4 % of them beyond 20 b; b is in the
    #    hundreds so that exp(-d / b) / (2 b) is below 1e-6 for them in both.
    s = nxt()
    r = np.random.default_rng(s)
    norms = np.concatenate([r.uniform(950.0, 1050.0, 450), r.uniform(4.0e4, 4.2e4, 50)])
    out.append(_prescribed("clamp_tenth_500", "clamp", s, norms, ("noclamp",)))
    s = nxt()
    r = np.random.default_rng(s)
    norms = np.concatenate([r.uniform(950.0, 1050.0, 480), r.uniform(1.1e4, 1.2e4, 20)])
    out.append(_prescribed("clamp_20b_500", "clamp", s, norms, ("noclamp",)))
    # -- thread and storage edges (512 threads, 64 lanes, LDS up to N = 4096, global scratch above)
    for n in (3, 4, 63, 64, 65, 511, 512, 513, 4096, 4097):
        out.append(_generic("edge_%d" % n, "edges", nxt(), n, ("rank_hi",)))
    s = nxt()
    norms, cl = _with_cluster(np.random.default_rng(s), 1898, 300, 1899)
    out.append(_prescribed("edge_4097_dup", "edges", s, norms, ("rowmajor",), cl))
    s = nxt()
    norms, cl = _with_cluster(np.random.default_rng(s), 1749, 300, 2049)    # N = 4098, cluster = ranks 1749 .. 2048 = N/2 - 1
    out.append(_prescribed("edge_4098_dup_ends_below_rank", "edges", s, norms, ("rank_hi", "rank_dup"), cl))
    # -- unequal measurement noise
    for n in (700, 4097):
        out.append(_generic("unequal_r_%d" % n, "unequal_noise", nxt(), n, ("rswap",), rdiag=(0.25, 4.0)))
    # -- prior conditioning, x_pred != 0
    for cond in (1.0, 1e2, 1e4):
        s = nxt()
        r = np.random.default_rng(s)
        Q, _ = np.linalg.qr(r.normal(size=(6, 6)))
        lam = 1e-3 * cond ** (np.arange(6) / 5.0)
        Pp = (Q * lam) @ Q.T
        Pp = 0.5 * (Pp + Pp.T)
        xp = X_TRUE + 0.3 * r.normal(size=6) * np.abs(X_TRUE)
        out.append(_generic("prior_cond_%g" % cond, "prior_conditioning", s, 700, ("rank_hi",), x_pred=xp, P_pred=Pp))
    # -- no re-weighting
    for n in (700, 4097):
        out.append(_generic("no_reweight_%d" % n, "no_reweight", nxt(), n, ("reweight",), reweight=False))
    table = {c.name: c for c in out}
    assert len(table) == len(out)
    return table


def bad_priors():
    """P_pred that is not positive definite: a negative eigenvalue in a random basis, a zero pivot, a NaN on the diagonal."""
    rng = np.random.default_rng(21)
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    neg = (Q * np.array([0.3, 0.2, 0.1, 0.05, 0.02, -0.01])) @ Q.T
    neg = 0.5 * (neg + neg.T)
    zero = np.diag([0.0, 0.1, 0.1, 0.1, 0.1, 0.1])
    nan = np.eye(6) * 0.1
    nan[3, 3] = np.nan
    return {"negative_eigenvalue": neg, "zero_pivot": zero, "nan_diagonal": nan}


FAMILIES = ("fallback_duplicates", "fallback_rank_edge", "gross_outliers", "straddle", "small_ties", "all_zero", "scale_switch",
            "clamp", "edges", "unequal_noise", "prior_conditioning", "no_reweight")


@functools.lru_cache(maxsize=None)
def exact(name):
    """(status, x+, P+, info) of a case: computed once, shared by every test, never modified (the arrays are read-only)."""
    c = cases()[name]
    info = {}
    st, x, P = skf_exact(c.x_pred, c.P_pred, c.y, c.H, c.rdiag, c.reweight, info=info)
    x.setflags(write=False)
    P.setflags(write=False)
    return st, x, P, info
