"""CPU: the zone statistics' host restatement (PvAmdHostZoneStats, csrc/pv_zones.h) against the independent numpy restatement
(tests/_zone_ref.py) bit for bit, against exact references within derived error bounds, its edges and refusals, and the label
rasteriser PvAmdHostZoneRects.  The GPU pass is held to PvAmdHostZoneStats in tests/test_gpu_zone_stats.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _zone_ref as ref

SHAPES = [(70, 127), (24, 50)]  # gy spans two blocks, the second partial; gy < 64
PLANES, ZONES = 3, 5


def planted_map(gx, gy, seed):
    """seeded values over nine decades, 10 % NaN, one +inf, one -inf, a +-0.0 tie at the minimum of plane 0 (non-negative there)
    and a tie at the maximum of plane 1"""
    rng = np.random.default_rng(seed)
    m = (10.0 ** rng.uniform(-4.0, 5.0, (gx, gy, PLANES))).astype(np.float32)
    m[..., 1:] *= rng.choice(np.float32([-1.0, 1.0]), (gx, gy, PLANES - 1))
    m[rng.random((gx, gy, PLANES)) < 0.10] = np.nan
    flat = m.reshape(-1, PLANES)
    cells = rng.permutation(gx * gy)
    flat[cells[0], 0], flat[cells[1], 2] = np.inf, -np.inf
    a, b = sorted(cells[2:4])
    flat[a, 0], flat[b, 0] = -0.0, 0.0      # the tie: the smaller cell's bits (-0.0) must be reported where both are in one zone
    c, d = sorted(cells[4:6])
    flat[c, 1] = flat[d, 1] = np.float32(3.0e5)
    return m, (a, b, c, d, cells[0], cells[1])


def scattered_labels(gx, gy, seed, tie):
    rng = np.random.default_rng(seed + 1000)
    lab = rng.integers(0, ZONES + 1, (gx, gy)).astype(np.uint8)  # every block holds every label
    a, b, c, d, pinf, ninf = tie
    lab.reshape(-1)[[a, b]] = 2
    lab.reshape(-1)[[c, d]] = 4
    lab.reshape(-1)[[pinf, ninf]] = 1, 5
    return lab


def rect_labels(pvlib, gx, gy, tie):
    dx = 0.25
    rects = [(0.0, 0.0, gx * dx * 0.5, gy * dx * 0.6), (gx * dx * 0.4, gy * dx * 0.3, gx * dx, gy * dx), (1.0, 1.0, 1.0 + dx, 1.0 + dx),
             (0.0, gy * dx * 0.9, gx * dx * 0.3, gy * dx), (gx * dx * 0.8, 0.0, gx * dx, gy * dx * 0.2)]
    return pvlib.zone_labels_from_rects(dx, gx, gy, rects)


_CASES = {}


def case(pvlib, shape, style):
    key = (shape, style)
    if key not in _CASES:
        gx, gy = shape
        m, tie = planted_map(gx, gy, gx * 1000 + gy)
        lab = scattered_labels(gx, gy, gx, tie) if style == "scattered" else rect_labels(pvlib, gx, gy, tie)
        got = pvlib.host_zone_stats(m, lab, ZONES)
        for a in (m, lab, got):
            a.setflags(write=False)
        _CASES[key] = (m, lab, got, tie)
    return _CASES[key]


# (1) the host restatement against the numpy restatement, bit for bit
@pytest.mark.parametrize("style", ["scattered", "rects"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_equals_numpy_restatement(pvlib, shape, style):
    m, lab, got, tie = case(pvlib, shape, style)
    assert got.shape == (ZONES, PLANES) and got.dtype == pvlib.ZONE_STAT_DTYPE == ref.DTYPE
    want = ref.zone_stats(m, lab, ZONES)
    assert ref.same_records(got, want), ref.first_difference(got, want)
    size = np.array([(lab == z).sum() for z in range(1, ZONES + 1)])
    assert np.array_equal((got["n_finite"] + got["n_nan"] + got["n_posinf"] + got["n_neginf"]), np.repeat(size[:, None], PLANES, 1))
    assert got["n_nan"].sum() > 0
    if style == "scattered":  # the planted ties sit in zones 2 and 4, the infinities in zones 1 and 5
        a, b, c, d = tie[:4]
        assert got["n_posinf"].sum() == 1 and got[0, 0]["n_posinf"] == 1 and got["n_neginf"].sum() == 1 and got[4, 2]["n_neginf"] == 1
        assert got[1, 0]["argmin"] == a and np.signbit(got[1, 0]["min"]) and got[1, 0]["min"] == 0.0
        assert got[3, 1]["argmax"] == c and got[3, 1]["max"] == np.float32(3.0e5)


# (2) against exact references
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_within_the_error_bounds_of_exact_sums(pvlib, shape):
    """u = 2^-53.  A double sum of n terms in ANY order carries every term through at most n - 1 roundings:
        |sum - S| <= gamma_(n-1) sum|x|,  gamma_k = k u / (1 - k u);
    the reference math.fsum is S rounded once (<= u |S| <= u sum|x|), so against it the bound is
    (gamma_(n-1) + u) sum|x| = n u sum|x| (1 + O(n u)) -- the issue's n 2^-53 sum|x|, the O(n u) factor (1e-12 here) being far
    below the resolution the bound itself is evaluated with.
    m2: with the computed mean m' and the exact mean mu, |m' - mu| <= |sum - S| / n + u |m'| <= delta, delta = (the sum's
    bound) / n + |mean| 2^-52.  In exact arithmetic sum (x - m')^2 = M + n (mu - m')^2 (the cross term vanishes), M = the exact
    sum (x - mu)^2.  Computing it rounds the subtract, the product (the error of the subtract counts twice) and at most n - 1
    adds of non-negative terms: a factor within 1 +- gamma_(n+2).  Hence
        |m2 - M| <= gamma_(n+2) M + (1 + gamma_(n+2)) n delta^2  <=  (n + 8) 2^-52 M + n delta^2,
    the issue's bound: its first term is twice gamma_(n+2) M, which leaves (n + 14) u M for the gamma n delta^2 term and for
    rounding M itself to a double.  The constants are the issue's, unchanged.  Counts and extremes are exact."""
    m, lab, got, _ = case(pvlib, shape, "scattered")
    cell = np.arange(m.shape[0] * m.shape[1]).reshape(m.shape[:2])
    for z in range(1, ZONES + 1):
        for k in range(PLANES):
            r = got[z - 1, k]
            x = m[..., k]
            member = lab == z
            with np.errstate(invalid="ignore"):
                finite = member & np.isfinite(x)
            xs = [float(v) for v in x[finite]]
            n = len(xs)
            assert n > 50
            assert (r["n_finite"], r["n_nan"], r["n_posinf"], r["n_neginf"]) == (
                n, (member & np.isnan(x)).sum(), (member & (x == np.inf)).sum(), (member & (x == -np.inf)).sum())
            assert r["min"] == min(xs) and r["max"] == max(xs)
            assert r["argmin"] == cell[finite][np.flatnonzero(x[finite] == min(xs))[0]]
            assert r["argmax"] == cell[finite][np.flatnonzero(x[finite] == max(xs))[0]]
            exact, mag = math.fsum(xs), math.fsum(abs(v) for v in xs)
            sum_bound = n * 2.0 ** -53 * mag
            print(shape, z, k, "n", n, "sum err", abs(r["sum"] - exact), "bound", sum_bound)
            assert abs(r["sum"] - exact) <= sum_bound
            assert r["mean"] == r["sum"] / n
            fx = [Fraction(v) for v in xs]
            mu = sum(fx) / n
            m2_exact = sum((v - mu) ** 2 for v in fx)
            delta = sum_bound / n + abs(r["mean"]) * 2.0 ** -52
            m2_bound = Fraction((n + 8) * 2.0 ** -52) * m2_exact + Fraction(n * delta * delta)
            print(shape, z, k, "m2 err", float(abs(Fraction(float(r["m2"])) - m2_exact)), "bound", float(m2_bound))
            assert abs(Fraction(float(r["m2"])) - m2_exact) <= m2_bound
            assert r["std"] == math.sqrt(r["m2"] / n)


# (3) edges and refusals
def test_edges(pvlib):
    rng = np.random.default_rng(3)
    m = rng.standard_normal((9, 70, 2)).astype(np.float32)
    lab = np.zeros((9, 70), np.uint8)
    lab[2, 65] = 1          # one cell
    lab[4:6, 10:30] = 3     # all NaN; zone 2 of 3 is a gap: no cells
    m[4:6, 10:30] = np.nan
    got = pvlib.host_zone_stats(m, lab, 3)
    assert ref.same_records(got, ref.zone_stats(m, lab, 3))
    one, none, nans = got[0], got[1], got[2]
    for k in range(2):
        v = m[2, 65, k]
        assert (one[k]["n_finite"], one[k]["argmin"], one[k]["argmax"]) == (1, 2 * 70 + 65, 2 * 70 + 65)
        assert one[k]["min"] == v and one[k]["max"] == v and one[k]["sum"] == float(v) and one[k]["mean"] == float(v)
        assert one[k]["m2"] == 0.0 and one[k]["std"] == 0.0
    for r, n_nan in ((none, 0), (nans, 40)):
        assert (r["n_finite"] == 0).all() and (r["n_nan"] == n_nan).all() and (r["n_posinf"] == 0).all() and (r["n_neginf"] == 0).all()
        assert (r["sum"] == 0.0).all() and not np.signbit(r["sum"]).any()
        for f in ("mean", "m2", "std", "min", "max"):
            assert np.isnan(r[f]).all(), f
        assert (r["argmin"] == -1).all() and (r["argmax"] == -1).all()
    # n_zones None: the largest label
    assert ref.same_records(pvlib.host_zone_stats(m, lab), got)


def test_refusals(pvlib):
    m = np.zeros((4, 5, 1), np.float32)
    lab = np.zeros((4, 5), np.uint8)
    lab[1, 1] = 3
    with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: a label above nZones"):
        pvlib.host_zone_stats(m, lab, 2)
    pvlib.host_zone_stats(m, lab, 3)
    for n in (0, 65):
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: nZones is 1 .. 64"):
            pvlib.host_zone_stats(m, np.zeros((4, 5), np.uint8), n)
    assert pvlib.host_zone_stats(m, np.zeros((4, 5), np.uint8), 64).shape == (64, 1)


# (4) the rectangles
def test_zone_rects(pvlib):
    gx, gy, dx = 37, 70, np.float32(0.3)
    rects = np.float32([(1.0, 2.0, 6.0, 9.0),       # 1
                        (4.0, 5.0, 8.0, 12.5),      # 2 overlaps 1: the later one wins
                        (-3.0, 18.0, 2.05, 40.0),   # 3 partly off the grid on two sides
                        (9.0, 0.0, 9.0, 5.0),       # 4 empty (xmin == xmax)
                        (4.5, 6.0, 4.8, 6.3)])      # 5 inside 2
    got = pvlib.zone_labels_from_rects(dx, gx, gy, rects)
    cx = ((np.arange(gx, dtype=np.float32) + np.float32(0.5)) * dx)[:, None]
    cz = ((np.arange(gy, dtype=np.float32) + np.float32(0.5)) * dx)[None, :]
    assert cx.dtype == np.float32 and cz.dtype == np.float32
    want = np.zeros((gx, gy), np.uint8)
    for j, (x0, z0, x1, z1) in enumerate(rects):
        want[(x0 <= cx) & (cx < x1) & (z0 <= cz) & (cz < z1)] = j + 1
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert set(np.unique(got)) == {0, 1, 2, 3, 5}
    assert (got[:, -1] == 3).any() and (got[0] == 3).any()      # (clipped at the grid's edges)
    assert (want == 1).sum() < ((rects[0][0] <= cx) & (cx < rects[0][2]) & (rects[0][1] <= cz) & (cz < rects[0][3])).sum()
    assert np.array_equal(pvlib.zone_labels_from_rects(dx, gx, gy, []), np.zeros((gx, gy), np.uint8))
