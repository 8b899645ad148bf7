"""CPU: PvAmdHostLobes -- the directional-energy-lobes definition of include/planeverb_amd.h (PvAmdSetLobeWindows) applied to one
impulse response with its velocities -- and PvAmdLobeGains against the numpy restatement of tests/_lobes_ref.py, bit for bit
(tolerance 0), on the oracle's recorded pr / vx / vy of the 70^2 golden scenes and on hand-made series.  The only tolerance is
the derived sum bound of the header.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _lobes_ref as ref
from test_host_lateral import oracle_run

EDGES5 = (0.005, 0.02, 0.05, 0.08, 0.2)
WINDOWS = [None, EDGES5]
ALL_SCENES = ["g71_smallroom", "g71_shoebox", "g71_empty", "g71_hugeroom"]
FP = C.POINTER(C.c_float)


def host_map(pvlib, p, vx, vy, delay, fs, edges):
    """PvAmdHostLobes on every reached cell: float32 [gx, gy, 1 + 5 nW], NaN elsewhere"""
    T = p.shape[0]
    cubes = [np.ascontiguousarray(np.moveaxis(v, 0, -1)) for v in (p, vx, vy)]  # [gx, gy, T]
    e = np.asarray(() if edges is None else edges, np.float32)
    nf = 1 + 5 * ((e.size or 2) + 1)
    out = np.full(delay.shape + (nf,), np.nan, np.float32)
    rec = np.empty(nf, np.float32)
    f = pvlib.lib().PvAmdHostLobes
    ep = e.ctypes.data_as(FP) if e.size else None
    for x, y in np.argwhere(delay < ref.NO_ONSET):
        ptr = [c[x, y].ctypes.data_as(FP) for c in cubes]
        assert f(ptr[0], ptr[1], ptr[2], T, fs, int(delay[x, y]), ep, int(e.size), rec.ctypes.data_as(FP)) == 0
        out[x, y] = rec
    return out


_MAPS, _REFS = {}, {}


def scene_map(pvlib, oracle, name, edges):
    if (name, edges) not in _MAPS:
        p, vx, vy, delay, fs = oracle_run(oracle, name)
        _MAPS[name, edges] = host_map(pvlib, p, vx, vy, delay, fs, edges)
    return _MAPS[name, edges]


def scene_ref(oracle, name, edges):
    """the restatement on the oracle's cubes (computed once, left unchanged)"""
    if (name, edges) not in _REFS:
        p, vx, vy, delay, fs = oracle_run(oracle, name)
        _REFS[name, edges] = ref.lobes(p, vx, vy, delay, fs, edges)
        _REFS[name, edges].setflags(write=False)
    return _REFS[name, edges]


def test_edge_steps():
    assert ref.edge_steps(None, 1443) == [14, 115] and ref.edge_steps((), 1968) == [19, 157]
    assert ref.edge_steps(EDGES5, 1443) == [7, 28, 72, 115, 288]
    assert ref.edge_steps((0.02, 0.01), 1443) is None and ref.edge_steps((0.0100, 0.0101), 1443) is None
    assert ref.edge_steps((0.0006,), 1443) is None and ref.edge_steps((0.01,) * 8, 1443) is None


# 1. the oracle's recorded fields, every reached cell
@pytest.mark.parametrize("edges", WINDOWS, ids=["default", "five"])
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_hugeroom"])
def test_oracle_scenes(pvlib, oracle, name, edges):
    p, vx, vy, delay, fs = oracle_run(oracle, name)
    assert p.shape == (435, 70, 70) and fs == 1443
    got = scene_map(pvlib, oracle, name, edges)
    want = scene_ref(oracle, name, edges)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s %s: %d values differ, first at %s: %s vs %s" % (name, edges, bad.sum(), np.argwhere(bad)[0],
                                                                             got[bad][:4], want[bad][:4])
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached) and np.isfinite(got[reached]).all()
    onset = np.where(reached, delay, 0).astype(np.int64)
    assert np.array_equal(got[..., 0][reached], (435 - onset)[reached].astype(np.float32))
    if edges is not None:  # the last edge (288 steps) leaves the cells with onset >= 147 an empty last window: five +0.0f
        empty = reached & (435 - onset <= 288)
        print(name, "cells with an empty last window", empty.sum(), "largest onset", onset.max())
        assert (got[empty][:, -5:] == 0).all() and not np.signbit(got[empty][:, -5:]).any()
        assert (got[reached & ~empty][:, -5] > 0).all()


# 2. random responses
def check(pvlib, p, vx, vy, fs, onset, edges=None):
    got = pvlib.host_lobes(p, vx, vy, fs, onset, edges)
    want = ref.lobes_ir(p, vx, vy, fs, onset, edges)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert same_bits(got, want).all(), (fs, onset, len(p), edges, got, want)
    return got


def test_random_series(pvlib):
    rng = np.random.default_rng(20261019)
    for i in range(200):
        T = int(rng.integers(1, 401))
        fs = int(rng.choice([1443, 1968, 700, 4000]))
        ne = int(rng.integers(0, 8))
        steps = np.sort(rng.choice(np.arange(1, 300), ne, replace=False))
        edges = tuple(float(np.float32((s + 0.5) / fs)) for s in steps) or None
        if edges:
            assert ref.edge_steps(edges, fs) == [int(s) for s in steps]
        p, vx, vy = ((rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32) for _ in range(3))
        if i % 5 == 0:  # zeros: q == 0 samples, p == 0 samples, one velocity component missing
            vx[rng.random(T) < 0.3] = 0
            vy[rng.random(T) < 0.3] = 0
            p[rng.random(T) < 0.1] = 0
        onset = 0 if i % 7 == 0 else T - 1 if i % 7 == 1 else int(rng.integers(0, T))
        m = check(pvlib, p, vx, vy, fs, onset, edges)
        assert m[0] == T - onset


# 3. exact synthetic cases: consequences of the definition, so no tolerance
def synthetic(seed=3, T=400):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.05, 1.0, T) * rng.choice([-1.0, 1.0], T)).astype(np.float32)  # (squares far from subnormal)


@pytest.mark.parametrize("edges", WINDOWS, ids=["default", "five"])
def test_exact_cases(pvlib, edges):
    fs, onset = 1443, 5
    p = synthetic()
    zero = np.zeros_like(p)
    E, XP, XN, YP, YN = (slice(1 + c, None, 5) for c in range(5))

    def plus_zero(v):
        return (v == 0).all() and not np.signbit(v).any()

    m = check(pvlib, p, np.float32(0.37) * p, zero, fs, onset, edges)
    assert (m[E] > 0).all() and np.array_equal(m[XP].view(np.uint32), m[E].view(np.uint32))
    assert plus_zero(m[XN]) and plus_zero(m[YP]) and plus_zero(m[YN])
    m = check(pvlib, p, np.float32(-0.37) * p, zero, fs, onset, edges)
    assert np.array_equal(m[XN].view(np.uint32), m[E].view(np.uint32))
    assert plus_zero(m[XP]) and plus_zero(m[YP]) and plus_zero(m[YN])
    v = np.float32(0.25) * p
    m = check(pvlib, p, v, v, fs, onset, edges)
    two = np.float32(2)
    assert np.array_equal((two * m[XP]).view(np.uint32), m[E].view(np.uint32))
    assert np.array_equal((two * m[YP]).view(np.uint32), m[E].view(np.uint32))
    assert plus_zero(m[XN]) and plus_zero(m[YN])
    m = check(pvlib, p, zero, zero, fs, onset, edges)
    assert (m[E] > 0).all() and all(plus_zero(m[s]) for s in (XP, XN, YP, YN))
    # samples before the onset do not enter
    q = p.copy()
    q[:onset] = 100.0
    assert same_bits(check(pvlib, q, v, -v, fs, onset, edges), check(pvlib, p, v, -v, fs, onset, edges)).all()


def test_signs(pvlib):
    """the lobe is chosen by the signs of p and v together: a negative pressure with a negative velocity travels towards +"""
    p = np.float32([0.5, -0.5, 0.5, -0.5, 0.5, -0.5, 0.5, -0.5])
    vx = np.float32([0.25, -0.25, -0.25, 0.25, 0.25, 0.25, 0.0, 0.0])
    vy = np.float32([0.0, 0.0, 0.0, 0.0, 0.25, 0.25, -0.25, -0.25])
    m = check(pvlib, p, vx, vy, 1443, 0, (0.002, 0.003, 0.004))  # edges at 2, 4, 5 steps: windows of 2, 2, 1, 3 steps
    assert ref.edge_steps((0.002, 0.003, 0.004), 1443) == [2, 4, 5]
    assert list(m) == [8, 0.5, 0.5, 0, 0, 0, 0.5, 0, 0.5, 0, 0, 0.25, 0.125, 0, 0.125, 0, 0.75, 0, 0.125, 0.25, 0.375]


# 4. the derived sum bound, every reached cell and window of the four golden scenes
@pytest.mark.parametrize("name", ALL_SCENES)
def test_sum_bound(pvlib, oracle, name):
    p, vx, vy, delay, fs = oracle_run(oracle, name)
    got = scene_map(pvlib, oracle, name, None)
    reached = delay < ref.NO_ONSET
    n = ref.edge_steps(None, fs)
    total = got[..., 0][reached].astype(np.int64)
    lo = [0] + n
    hi = n + [1 << 30]
    worst = 0.0
    for w in range(3):
        N = np.clip(np.minimum(total, hi[w]) - lo[w], 0, None)
        r = got[reached][:, 1 + 5 * w:6 + 5 * w].astype(np.float64)
        E, four = r[:, 0], r[:, 1] + r[:, 2] + r[:, 3] + r[:, 4]
        bound = (N + 8) * 2.0 ** -23 * E
        assert (np.abs(four - E) <= bound).all(), (name, w, np.abs(four - E).max())
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.abs(four - E) / bound)))
    print(name, "largest |sum - E| / bound", worst)


# 5. the reach of the record, on the restatement alone: one direction in the direct window, all round in the late one
def largest_share(rec, w):
    r = rec[:, 1 + 5 * w:6 + 5 * w].astype(np.float64)
    return r[:, 1:].max(axis=1) / r[:, 0]


@pytest.mark.parametrize("name", ["g71_hugeroom", "g71_shoebox"])
def test_direct_window_is_directional_and_late_window_is_not(oracle, name):
    _, _, _, delay, _ = oracle_run(oracle, name)
    rec = scene_ref(oracle, name, None)[delay < ref.NO_ONSET]
    direct, late = np.median(largest_share(rec, 0)), np.median(largest_share(rec, 2))
    print(name, "median largest-lobe share: direct", direct, "late", late)
    assert direct > 0.8
    assert late < 0.45


def test_empty_scene_direct_window_points_away_from_the_listener(oracle):
    _, _, _, delay, _ = oracle_run(oracle, "g71_empty")
    rec = scene_ref(oracle, "g71_empty", None)
    lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]
    X, Y = np.meshgrid(np.arange(delay.shape[0]), np.arange(delay.shape[1]), indexing="ij")
    dX, dY = X - lx, Y - ly
    cone = (delay < ref.NO_ONSET) & (np.abs(dY) * 4 <= -dX) & (-dX >= 6)
    assert cone.sum() > 20
    share = rec[cone][:, 3].astype(np.float64) / rec[cone][:, 1].astype(np.float64)  # XN / E of window 0
    print("g71_empty, cells", cone.sum(), "XN / E min", share.min(), "median", np.median(share))
    assert (share >= 0.85).all()


# 6. refusals
def test_refusals(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = np.empty(1 + 5 * 9, np.float32)
    fp, op = p.ctypes.data_as(FP), out.ctypes.data_as(FP)
    nan, inf = float("nan"), float("inf")

    def call(edges, T=8, onset=0, ptrs=(fp, fp, fp), o=op, fs=1443):
        e = np.asarray(edges, np.float32)
        return L.PvAmdHostLobes(ptrs[0], ptrs[1], ptrs[2], T, fs, onset, e.ctypes.data_as(FP) if e.size else None, int(e.size), o)

    for edges in ((0.02, 0.01), (0.01, 0.05, 0.04),  # unsorted
                  (0.0100, 0.0101), (0.01, 0.01),    # two edges with the same step count (14)
                  (0.0006,), (0.0, 0.01), (-0.01,),  # below one step
                  (0.001,) * 8, tuple(0.001 * (i + 1) for i in range(8)),  # 8 edges
                  (nan,), (0.01, nan), (inf,), (-inf,), (0.01, inf), (1000.0,), (3.0e38,)):  # not finite, above 2^20 steps
        assert call(edges) == -1, edges
        assert pvlib.last_error().startswith("lobes: "), pvlib.last_error()
        assert ref.edge_steps(edges, 1443) is None
    for kw in (dict(onset=-1), dict(onset=8), dict(T=0), dict(T=-3), dict(ptrs=(None, fp, fp)), dict(ptrs=(fp, None, fp)),
               dict(ptrs=(fp, fp, None)), dict(o=None), dict(fs=0)):
        assert call((0.01,), **kw) == -1, kw
        assert pvlib.last_error().startswith("lobes: "), pvlib.last_error()
    assert call(tuple(0.001 * (i + 1) for i in range(7)), onset=7) == 0 and out[0] == 1
    assert call((), onset=3) == 0 and out[0] == 5  # (no edges: the default)
    assert L.PvAmdHostLobes(fp, fp, fp, 8, 1024, 0, np.float32([1024.0]).ctypes.data_as(FP), 1, op) == 0  # 2^20 steps
    assert L.PvAmdHostLobes(fp, fp, fp, 8, 1024, 0, np.float32([1025.0]).ctypes.data_as(FP), 1, op) == -1
    # the solver calls refuse a null handle
    steps = (C.c_int * 7)()
    for f in (lambda: L.PvAmdSetLobeWindows(None, None, 0), lambda: L.PvAmdSetLobeWindows(None, fp, 1),
              lambda: L.PvAmdGetLobeWindows(None, op, steps), lambda: L.PvAmdComputeLobes(None, None),
              lambda: L.PvAmdCopyLobes(None, op), lambda: L.PvAmdCopyLobesBlock(None, 0, 0, 1, 1, op),
              lambda: L.PvAmdGetLobes(None, 0.0, 0.0, 0.0, op)):
        assert f() == -1
        assert pvlib.last_error().startswith("lobes: "), pvlib.last_error()


# 7. PvAmdLobeGains
def record(windows):
    return np.concatenate([[np.float32(1)]] + [np.asarray(w, np.float32) for w in windows]).astype(np.float32)


def test_lobe_gains(pvlib):
    rng = np.random.default_rng(7)
    one = np.float32(1)
    # omni: exactly 1 wherever the lobe sum is positive
    for _ in range(50):
        nw = int(rng.integers(1, 9))
        r = record([np.concatenate([[1.0], rng.uniform(0, 1, 4) * 10.0 ** rng.uniform(-8, 3)]) for _ in range(nw)])
        g = pvlib.lobe_gains(r, rng.standard_normal(2), 0)
        assert g.shape == (nw,) and g.dtype == np.float32 and (g == one).all()
    # all the energy travels towards +x: it left the emitter towards -x
    r = record([[2.5, 2.5, 0, 0, 0]])
    assert pvlib.lobe_gains(r, (-1.0, 0.0), 1)[0] == one
    floor = np.float32(0.01)
    want = (np.float32(2.5) * (floor * floor)) / np.float32(2.5)
    assert pvlib.lobe_gains(r, (1.0, 0.0), 1)[0] == want and abs(float(want) - 1e-4) < 1e-10
    # random records and forwards, both patterns
    for i in range(500):
        nw = int(rng.integers(1, 9))
        r = record([np.concatenate([[1.0], rng.uniform(0, 1, 4) * 10.0 ** rng.uniform(-8, 3, 4)]) for _ in range(nw)])
        fwd = rng.standard_normal(2) * (1.0 if i % 3 else 0.3)
        if i % 4 == 0:
            fwd = fwd / np.hypot(*fwd)
        kind = i % 2
        got, want = pvlib.lobe_gains(r, fwd, kind), ref.lobe_gains(r, fwd, kind)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (r, fwd, kind, got, want)
    # a window without directional energy: 0 / 0
    g = pvlib.lobe_gains(record([[1, 0.5, 0, 0.5, 0], [3, 0, 0, 0, 0]]), (0.0, 1.0), 1)
    assert np.isfinite(g[0]) and np.isnan(g[1])
    assert np.isnan(ref.lobe_gains(record([[3, 0, 0, 0, 0]]), (0.0, 1.0), 1)[0])
    # refusals
    L = pvlib.lib()
    out = np.empty(9, np.float32)
    rp, op = record([[1, 1, 0, 0, 0]] * 9).ctypes.data_as(FP), out.ctypes.data_as(FP)
    for args in ((None, 1, 1.0, 0.0, 1, op), (rp, 1, 1.0, 0.0, 1, None), (rp, 0, 1.0, 0.0, 1, op), (rp, 9, 1.0, 0.0, 1, op),
                 (rp, -1, 1.0, 0.0, 0, op), (rp, 1, 1.0, 0.0, 2, op), (rp, 1, 1.0, 0.0, -1, op)):
        assert L.PvAmdLobeGains(*args) == -1, args
        assert pvlib.last_error().startswith("lobes: "), pvlib.last_error()
    assert L.PvAmdLobeGains(rp, 8, 1.0, 0.0, 1, op) == 0


# 8. exports
NEW_EXPORTS = ["PvAmdSetLobeWindows", "PvAmdGetLobeWindows", "PvAmdComputeLobes", "PvAmdCopyLobes", "PvAmdCopyLobesBlock",
               "PvAmdGetLobes", "PvAmdHostLobes", "PvAmdLobeGains"]


def test_exports_present_and_guarded(pvlib):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the exception-guard macro of pv_capi.cpp"""
    L = C.CDLL(pvlib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    for n in NEW_EXPORTS:
        assert hasattr(L, n), n
        assert n in pvlib.SYMBOLS
        assert re.search(r"^PVA_EXPORT\s+int\s+%s\s*\(" % n, hdr, re.M), n
        m = re.search(r"^int\s+%s\s*\([^;{}]*?\)\s*try\s*\{.*?^\}\s*PV_API_CATCH\(-1\)" % n, src, re.M | re.S)
        assert m, n
        assert "\n}\n" not in m.group(0), n  # (the match ends at this function's own guard)
    assert re.search(r"^#define\s+PVA_LOBES_MAX_EDGES\s+7\s*$", hdr, re.M)
    assert pvlib.LOBES_MAX_EDGES == ref.MAX_EDGES == 7 and pvlib.LOBE_NAMES == ref.NAMES
    assert tuple(np.float32(pvlib.LOBES_DEFAULT_EDGES)) == tuple(np.float32(ref.DEFAULT_EDGES))
