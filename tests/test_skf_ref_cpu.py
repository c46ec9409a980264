"""The inputs of tests/test_skf_paths_gpu.py are sound and sharp -- checked without a GPU.

  * sound: the oracle's sequential 2-row recursion (oracle/ro_velocity.c) agrees with the exact information-form reference of
    tests/skf_ref.py within ORACLE_RTOL on every case of the table.  Measured here over the table: worst 1.1e-13
    (scale_switch_above, where exp(-d / b) is taken at d / b up to 5 000), every other case below 4e-14.  This pins the oracle's
    SKF independently of the HIP kernel.
  * sharp: every case moves by more than SHARP = 1e3 x SKF_RTOL when the reference is given the defect the case is there to
    catch (a median rank off by one, exchanged noise variances, no clamp, ...), so such a defect in the kernel cannot pass the
    1e-8 bar of the GPU test.  Smallest measured: 8.3e-5 (edge_4097, median one rank high).
  * aimed: a restatement of the kernel's bucket layout says which median route each case takes, and each family takes the
    one it was built for.
"""
import numpy as np
import pytest

import skf_ref as R

from test_parity_gpu import SKF_RTOL   # the project's stated bar (importing the module touches no GPU)

ORACLE_RTOL = 1e-12      # 60 x the worst deviation measured when the case families were designed (1.7e-14)
SHARP = 1e3 * SKF_RTOL

CASES = list(R.cases())


def test_reference_arithmetic_is_extended():
    B = R.backend()
    assert B.name in ("longdouble", "mpmath")
    one = B.arr(1.0)
    assert (one + B.arr(2.0 ** -60)) - one == B.arr(2.0 ** -60)     # 53 bits would lose it


def test_mpmath_fallback_agrees_with_longdouble():
    """Both arithmetics on one small weighted case (the mpmath path is what a machine without an 80-bit long double takes)."""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        assert R.backend().name == "longdouble"    # this machine has no fallback to test, and needs none
        return
    c = R.cases()["ties_64"]
    st0, x0, P0 = R.skf_exact(c.x_pred, c.P_pred, c.y, c.H, (0.25, 4.0), True)
    st1, x1, P1 = R.skf_exact(c.x_pred, c.P_pred, c.y, c.H, (0.25, 4.0), True, backend_name="mpmath")
    assert st0 == st1 == 0
    R.assert_close(x1, P1, x0, P0, 1e-15)


def test_table_covers_every_family():
    fam = {c.family for c in R.cases().values()}
    assert fam == set(R.FAMILIES)
    n = {c.y.size // 2 for c in R.cases().values()}
    assert n >= {3, 4, 5, 8, 63, 64, 65, 511, 512, 513, 600, 601, 999, 1000, 4096, 4097}
    assert any(c.rdiag == (0.25, 4.0) and c.y.size // 2 == 4097 for c in R.cases().values())
    assert all(c.H.shape == (c.y.size, 6) for c in R.cases().values())


@pytest.mark.parametrize("name", CASES)
def test_oracle_matches_exact(oracle, name):
    c = R.cases()[name]
    st, x, P, _ = R.exact(name)
    rc, xo, Po = oracle.skf_correct(c.x_pred, c.P_pred, c.y, c.H, c.rdiag, c.reweight)
    assert rc == st == 0
    print("SKFDEV oracle %-20s %-32s dx %.2e dP %.2e" % ((c.family, name) + R.deviation(xo, Po, x, P)))
    R.assert_close(xo, Po, x, P, ORACLE_RTOL, name)


def test_empty_measurement(oracle):
    c = R.cases()["edge_3"]
    st, x, P = R.skf_exact(c.x_pred + 1.0, c.P_pred, np.zeros(0), np.zeros((0, 6)))
    rc, xo, Po = oracle.skf_correct(c.x_pred + 1.0, c.P_pred, np.zeros(0), np.zeros((0, 6)))
    assert st == rc == 1
    assert np.array_equal(x, xo) and np.array_equal(P, Po) and np.array_equal(x, c.x_pred + 1.0) and np.array_equal(P, c.P_pred)


@pytest.mark.parametrize("name", CASES)
def test_mutation_sharpness(name):
    c = R.cases()[name]
    _, x, P, _ = R.exact(name)
    assert c.mutations or c.family == "all_zero"
    for m in c.mutations:
        _, xm, Pm = R.skf_exact(c.x_pred, c.P_pred, c.y, c.H, c.rdiag, c.reweight, mutation=m)
        d = max(R.deviation(xm, Pm, x, P))
        assert d > SHARP, (name, m, d)


def test_every_mutation_is_aimed_at():
    used = {m for c in R.cases().values() for m in c.mutations}
    assert used == set(R.MUTATIONS)


# ---------------------------------------------------------------------------------------------
# the cases are what the table says they are
# ---------------------------------------------------------------------------------------------
K_BINS, K_BUCKET_CAP, K_LDS_N = 1024, 256, 4096     # kBins, kBucketCap, kSkfLdsN of roft_amd/csrc/k_skf.hip


def _norms(c):
    n = c.y.size // 2
    e = c.y - c.H @ c.x_pred
    return np.sqrt(e[:n] ** 2 + e[n:] ** 2)


def _route(c):
    """The median route of bucket_select2 in k_skf.hip, restated: "zero", "bucket" (with the two buckets) or "radix"."""
    q = _norms(c)
    n = q.size
    top = 8.0 * (q.sum() / n)
    if not top > 0.0:
        return "zero", None
    b = np.clip((q * ((K_BINS - 1) / top)).astype(np.int64), 0, K_BINS - 1)
    order = np.sort(b)
    ra, rb = (n // 2 - 1, n // 2) if n % 2 == 0 else (n // 2, n // 2)
    ba, bb = order[ra], order[rb]
    if max(np.count_nonzero(b == ba), np.count_nonzero(b == bb)) > K_BUCKET_CAP:
        return "radix", (ba, bb)
    return "bucket", (ba, bb)


def test_cases_take_the_routes_they_aim_at():
    T = R.cases()
    route = {name: _route(c) for name, c in T.items()}
    for name, c in T.items():
        if c.family in ("fallback_duplicates", "fallback_rank_edge", "gross_outliers") or "dup" in name:
            assert route[name][0] == "radix", name
        if c.family in ("straddle", "small_ties"):
            assert route[name][0] == "bucket", name
    assert route["all_zero_100"][0] == "zero"
    assert route["outliers_1000"][1] == (0, 0)                                  # everything but the outliers in bin 0
    assert route["straddle_1000"][1][0] != route["straddle_1000"][1][1]       # the two middle ranks in different buckets
    assert route["edge_4097"][0] == "bucket" and route["edge_4096"][0] == "bucket"   # above the LDS capacity on both routes
    assert route["edge_4097_dup"][0] == "radix" and route["edge_4098_dup_ends_below_rank"][0] == "radix"
    assert T["edge_4097"].y.size // 2 > K_LDS_N >= T["edge_4096"].y.size // 2


@pytest.mark.parametrize("name,first,last", [
    ("dup_600", 150, 449), ("dup_601", 150, 449), ("dup_ends_below_rank_800", 100, 399), ("dup_starts_at_rank_800", 400, 699),
    ("edge_4097_dup", 1898, 2197), ("edge_4098_dup_ends_below_rank", 1749, 2048)])
def test_clusters_are_bit_identical_and_sit_at_their_ranks(name, first, last):
    c = R.cases()[name]
    q = np.sort(_norms(c))
    n = q.size
    assert np.all(q[first:last + 1] == q[first]) and last - first + 1 == 300 > K_BUCKET_CAP
    assert q[first - 1] < 0.95 * q[first] and q[last + 1] > 1.2 * q[last]       # distinct and clearly apart
    if "ends_below" in name:
        assert last == n // 2 - 1 and n % 2 == 0
    elif "starts_at" in name:
        assert first == n // 2 and n % 2 == 0
    else:
        assert first < n // 2 - 1 and n // 2 < last


def test_ties_straddle_the_middle_ranks():
    for n in (5, 8, 64, 65):
        q = np.sort(_norms(R.cases()["ties_%d" % n]))
        assert q[n // 2 - 1] == q[n // 2] and q[n // 2 - 2] < q[n // 2 - 1] and q[n // 2] < q[n // 2 + 1]


def test_branch_cases_sit_on_their_side():
    info = {name: R.exact(name)[3] for name in R.cases()}
    assert 0.4e-4 < info["scale_switch_below"]["b"] < 0.6e-4 and not info["scale_switch_below"]["weighted"]
    assert 1.8e-4 < info["scale_switch_above"]["b"] < 2.2e-4 and info["scale_switch_above"]["weighted"]
    assert info["all_zero_100"]["b"] == 0.0 and info["all_zero_100"]["mi"] == 0.0 and not info["all_zero_100"]["weighted"]
    assert info["outliers_1000"]["n_clamped"] == 1000
    # clamp: the far points, and only a minority, are below the floor; how far out they are in units of b
    for name, n_far, far_min, k_b in (("clamp_tenth_500", 50, 4.0e4, 9.0), ("clamp_20b_500", 20, 1.1e4, 20.0)):
        i = info[name]
        q = _norms(R.cases()[name])
        far = np.abs(q - i["mi"]) > k_b * i["b"]
        assert np.count_nonzero(far) == n_far and np.all(q[far] >= far_min * 0.999)
        assert n_far <= i["n_clamped"] < 100 and i["weighted"]
    # prior conditioning
    for cond in (1.0, 1e2, 1e4):
        c = R.cases()["prior_cond_%g" % cond]
        assert np.isclose(np.linalg.cond(c.P_pred), cond, rtol=1e-6) and np.any(c.x_pred != 0.0)


# ---------------------------------------------------------------------------------------------
# the point entry and the status
# ---------------------------------------------------------------------------------------------
def test_point_entry_uses_the_measurement_models_expression(oracle):
    """yh_from_points_f64 is, bit for bit, the (y, H) the oracle's flow measurement assembles; the extended one rounds to it."""
    cam = R.CAM_VGA
    rng = np.random.default_rng(11)
    mask = (rng.random((cam.height, cam.width)) < 0.01).astype(np.uint8) * 255
    mask[0, 0] = mask[0, -1] = mask[-1, 0] = mask[-1, -1] = mask[240, 320] = 255
    depth = rng.uniform(0.05, 1.9, mask.shape).astype(np.float32)
    flow = (3.0 * rng.standard_normal(mask.shape + (2,))).astype(np.float32)
    ocam = oracle.camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    n, uv, y0, H0 = oracle.flow_measurement(ocam, mask, depth, flow, R.DT, radius=1.0)
    assert n == np.count_nonzero(mask) > 1000
    z, fxy = depth[uv[:, 1], uv[:, 0]], flow[uv[:, 1], uv[:, 0]]
    y1, H1 = R.yh_from_points_f64(cam, R.DT, uv, z, fxy)
    assert np.array_equal(y0, y1) and np.array_equal(H0, H1)
    y2, H2 = R.yh_from_points(cam, R.DT, uv, z, fxy)
    assert np.array_equal(R.backend().f64(y2), y1)
    assert np.max(np.abs(R.backend().f64(H2) - H1) / np.maximum(np.abs(H1), 1e-300)) < 4e-16


@pytest.mark.parametrize("kind", ["negative_eigenvalue", "zero_pivot", "nan_diagonal"])
def test_reference_status_3_leaves_the_belief(kind):
    c = R.cases()["edge_65"]
    P = R.bad_priors()[kind]
    xp = R.X_TRUE.copy()
    st, x, Po = R.skf_exact(xp, P, c.y, c.H)
    assert st == 3
    assert np.array_equal(x.view(np.uint64), xp.view(np.uint64)) and np.array_equal(Po.view(np.uint64), P.view(np.uint64))
