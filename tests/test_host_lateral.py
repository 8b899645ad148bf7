"""CPU: PvAmdHostLateralFraction -- the lateral-energy-fraction definition of include/planeverb_amd.h (PvAmdLateralFraction)
applied to one impulse response with its velocities -- against the numpy restatement of tests/_lateral_ref.py, bit for bit
(tolerance 0), on the oracle's recorded pr / vx / vy of the 70^2 golden scenes and on hand-made series.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
import _lateral_ref as ref

SCENES = ["g71_empty", "g71_smallroom", "g71_shoebox"]
_RUNS = {}


def oracle_run(oracle, name):
    """the oracle's recorded pr, vx, vy [T, gx, gy] of a golden scene at its golden listener, its analysis onsets and fs"""
    if name not in _RUNS:
        g = golden(name)
        size, res = float(g["size"]), int(g["res"])
        o = oracle.OracleGrid(size, size, res, g["boxes"])
        L = tuple(float(v) for v in g["listener"])
        o.fdtd(L)
        p, vx, vy = (h[:, :o.gx, :o.gy].copy() for h in o.history())
        _, delay, _ = o.analyze(np.float32(oracle.free_energy(size, size, res)), L)
        _RUNS[name] = (p, vx, vy, delay, int(o.fs))
        o.close()
    return _RUNS[name]


def host_map(pvlib, p, vx, vy, delay, fs):
    """PvAmdHostLateralFraction on every reached cell: float32 [gx, gy, 11], NaN elsewhere"""
    T = p.shape[0]
    cubes = [np.ascontiguousarray(np.moveaxis(v, 0, -1)) for v in (p, vx, vy)]  # [gx, gy, T]
    out = np.full(delay.shape + (11,), np.nan, np.float32)
    rec = pvlib.PvAmdLateralFraction()
    fp = C.POINTER(C.c_float)
    f = pvlib.lib().PvAmdHostLateralFraction
    for x, y in np.argwhere(delay < ref.NO_ONSET):
        ptr = [c[x, y].ctypes.data_as(fp) for c in cubes]
        assert f(ptr[0], ptr[1], ptr[2], T, fs, int(delay[x, y]), rec) == 0
        out[x, y] = rec.as_array()
    return out


_MAPS = {}


def scene_map(pvlib, oracle, name):
    if name not in _MAPS:
        p, vx, vy, delay, fs = oracle_run(oracle, name)
        _MAPS[name] = (host_map(pvlib, p, vx, vy, delay, fs), delay)
    return _MAPS[name]


# 1. the oracle's recorded fields, every reached cell
@pytest.mark.parametrize("name", SCENES)
def test_oracle_scenes(pvlib, oracle, name):
    p, vx, vy, delay, fs = oracle_run(oracle, name)
    assert p.shape == (435, 70, 70) and fs == 1443
    got, _ = scene_map(pvlib, oracle, name)
    want = ref.lateral_fraction(p, vx, vy, delay, fs)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d values differ, first at %s: %s vs %s" % (name, bad.sum(), np.argwhere(bad)[0], got[bad][:4],
                                                                          want[bad][:4])
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached)
    # no window of these scenes is cut off by T and no cell has a zero direct flux
    assert (got[..., 3][reached] == ref.n80(fs)).all() and np.isfinite(got[reached]).all()
    print(name, "reached", reached.sum(), "lf median / p90 / max", np.median(got[..., 0][reached]),
          np.percentile(got[..., 0][reached], 90), got[..., 0][reached].max())


# 2. hand-made series
def check(pvlib, p, vx, vy, fs, onset):
    got = pvlib.host_lateral_fraction(p, vx, vy, fs, onset)
    want = ref.lateral_fraction_ir(p, vx, vy, fs, onset)
    assert got.dtype == np.float32 and got.shape == (11,)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    return got


def series(seed, T):
    rng = np.random.default_rng(seed)
    return tuple((rng.standard_normal(T) * s).astype(np.float32) for s in (1e-2, 3e-5, 2e-5))


def test_window_lengths():
    assert (ref.n5(1443), ref.n80(1443)) == (7, 115)
    assert (ref.n5(1968), ref.n80(1968)) == (9, 157)


@pytest.mark.parametrize("fs", [1443, 1968])
def test_window_cut_off_by_the_record(pvlib, fs):
    """onset + n80 > T (n < n80), onset + n80 == T, onset with fewer than n5 steps left, onset = T - 1"""
    T = 300
    p, vx, vy = series(fs, T)
    a5, a80 = ref.n5(fs), ref.n80(fs)
    for onset, n in ((0, a80), (T - a80 - 1, a80), (T - a80, a80), (T - a80 + 1, a80 - 1), (T - 40, 40), (T - a5 - 1, a5 + 1),
                     (T - a5, a5), (T - 2, 2), (T - 1, 1)):
        m = check(pvlib, p, vx, vy, fs, onset)
        assert m[3] == n, (onset, m)
        assert np.isfinite(m[4:]).all() and m[4] > 0
        assert np.isfinite(m[:3]).all()  # (the flux of random series is not zero)
        if n <= a5:  # no step after the direct sound: the three moments are empty, lf = 0 / e80
            assert (m[8:] == 0).all() and m[5] == 0 and m[0] == 0
    m = check(pvlib, p, vx, vy, fs, T - 1)
    assert m[4] == p[T - 1] * p[T - 1] and m[6] == p[T - 1] * vx[T - 1] and m[7] == p[T - 1] * vy[T - 1]


def test_zero_flux(pvlib):
    """a response whose first n5 samples carry no flux: NaN lf and direction, finite sums"""
    fs, T, onset = 1443, 300, 20
    p, vx, vy = series(7, T)
    a5 = ref.n5(fs)
    for how in ("no velocity", "no pressure"):
        q, x, y = p.copy(), vx.copy(), vy.copy()
        if how == "no velocity":
            x[onset:onset + a5] = 0
            y[onset:onset + a5] = 0
        else:
            q[onset:onset + a5] = 0
        m = check(pvlib, q, x, y, fs, onset)
        assert np.isnan(m[:3]).all() and np.isnan(m[5]), (how, m)
        assert m[3] == ref.n80(fs) and (m[6:8] == 0).all() and np.isfinite(m[4:5]).all() and np.isfinite(m[8:]).all()
        assert m[4] > 0 and m[8] > 0 and m[10] > 0


def test_known_directions(pvlib):
    """a plane wave along +x, then sound from the side only: lf = the whole late velocity energy over e80; sound along the
    direction only: lf = 0; and the sign of the direction follows the flux"""
    fs, T, onset = 1443, 300, 10
    a5, a80 = ref.n5(fs), ref.n80(fs)
    p = np.zeros(T, np.float32)
    vx, vy = p.copy(), p.copy()
    p[onset:onset + a80] = 0.5
    vx[onset:onset + a5] = 0.25      # the direct sound travels along +x
    vy[onset + a5:onset + a80] = 0.5  # everything later moves along y
    m = check(pvlib, p, vx, vy, fs, onset)
    assert m[1] == 1 and m[2] == 0 and m[0] == np.float32(a80 - a5) / np.float32(a80)
    vx[onset + a5:onset + a80], vy[onset + a5:onset + a80] = 0.5, 0.0
    m = check(pvlib, p, vx, vy, fs, onset)
    assert m[1] == 1 and m[2] == 0 and m[0] == 0
    m = check(pvlib, p, -vx, vy, fs, onset)
    assert m[1] == -1 and m[0] == 0
    m = check(pvlib, p, vy, vx, fs, onset)  # the same along y
    assert m[1] == 0 and m[2] == 1 and m[0] == 0


def test_random_series(pvlib):
    rng = np.random.default_rng(20261018)
    for _ in range(150):
        T = int(rng.integers(1, 500))
        fs = int(rng.choice([1443, 1968, 700, 4000, 12]))
        p, vx, vy = ((rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32) for _ in range(3))
        check(pvlib, p, vx, vy, fs, int(rng.integers(0, T)))


# 3. sanity, on the float32 records of the oracle scenes (a float64 evaluation of the definition on the same fields gives
#    medians of 0.016 / 0.054 / 0.291: the margins are 2-3 x)
def test_sanity(pvlib, oracle):
    med = {}
    for name in SCENES:
        got, delay = scene_map(pvlib, oracle, name)
        reached = delay < ref.NO_ONSET
        med[name] = float(np.median(got[..., 0][reached]))
        d = got[..., 1:3][reached].astype(np.float64)
        ok = ~np.isnan(d).any(axis=-1)
        assert ok.any() and (np.abs((d[ok] ** 2).sum(axis=-1) - 1.0) < 1e-6).all(), name
    print(med)
    assert med["g71_empty"] < 0.05
    assert med["g71_shoebox"] > 0.15
    assert med["g71_empty"] < med["g71_smallroom"] < med["g71_shoebox"]


def test_bad_arguments(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = pvlib.PvAmdLateralFraction()
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, fp, fp, 8, 1443, 0, out), (fp, None, fp, 8, 1443, 0, out), (fp, fp, None, 8, 1443, 0, out),
                 (fp, fp, fp, 8, 1443, 0, None), (fp, fp, fp, 0, 1443, 0, out), (fp, fp, fp, -3, 1443, 0, out),
                 (fp, fp, fp, 8, 1443, -1, out), (fp, fp, fp, 8, 1443, 8, out)):
        assert L.PvAmdHostLateralFraction(*args) == -1
        assert pvlib.last_error().startswith("lateral fraction: ")
    assert L.PvAmdHostLateralFraction(fp, fp, fp, 8, 1443, 7, out) == 0
    # the solver calls refuse a null handle
    for call in (lambda: L.PvAmdComputeLateralFraction(None, None), lambda: L.PvAmdCopyLateralFraction(None, fp),
                 lambda: L.PvAmdCopyLateralFractionBlock(None, 0, 0, 1, 1, fp),
                 lambda: L.PvAmdGetLateralFraction(None, 0.0, 0.0, 0.0, out)):
        assert call() == -1
        assert pvlib.last_error().startswith("lateral fraction: "), pvlib.last_error()


NEW_EXPORTS = ["PvAmdComputeLateralFraction", "PvAmdCopyLateralFraction", "PvAmdCopyLateralFractionBlock", "PvAmdGetLateralFraction",
               "PvAmdHostLateralFraction"]


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
    assert pvlib.LATERAL_FRACTION_NAMES == ref.NAMES
    assert C.sizeof(pvlib.PvAmdLateralFraction) == 44
