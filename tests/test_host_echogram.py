"""CPU: PvAmdHostEchogram -- the directional-echogram definition of include/planeverb_amd.h (PvAmdSetEchogram) applied to one
impulse response with its velocities -- against the numpy restatement of tests/_echogram_ref.py, bit for bit (tolerance 0), on
the oracle's recorded pr / vx / vy of the 70^2 golden scenes and on hand-made series.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _echogram_ref as ref
from test_host_lateral import SCENES, oracle_run, scene_map as lateral_scene_map

SETTINGS = [(0.005, 16), (0.002, 32), (0.01, 24), (0.0007, 1)]
FP = C.POINTER(C.c_float)


def host_map(pvlib, p, vx, vy, delay, fs, slot_seconds, n_slots):
    """PvAmdHostEchogram on every reached cell: float32 [gx, gy, 1 + 3 n], NaN elsewhere"""
    T = p.shape[0]
    cubes = [np.ascontiguousarray(np.moveaxis(v, 0, -1)) for v in (p, vx, vy)]  # [gx, gy, T]
    out = np.full(delay.shape + (1 + 3 * n_slots,), np.nan, np.float32)
    rec = np.empty(1 + 3 * n_slots, np.float32)
    f = pvlib.lib().PvAmdHostEchogram
    for x, y in np.argwhere(delay < ref.NO_ONSET):
        ptr = [c[x, y].ctypes.data_as(FP) for c in cubes]
        assert f(ptr[0], ptr[1], ptr[2], T, fs, int(delay[x, y]), slot_seconds, n_slots, rec.ctypes.data_as(FP)) == 0
        out[x, y] = rec
    return out


_MAPS = {}


def scene_map(pvlib, oracle, name, setting):
    if (name, setting) not in _MAPS:
        p, vx, vy, delay, fs = oracle_run(oracle, name)
        _MAPS[name, setting] = (host_map(pvlib, p, vx, vy, delay, fs, *setting), delay)
    return _MAPS[name, setting]


def test_slot_steps():
    assert [ref.slot_steps(s, 1443) for s, _ in SETTINGS] == [7, 2, 14, 1]
    assert ref.slot_steps(0.005, 1968) == 9 and ref.slot_steps(0.0006, 1443) == 0


# 1. the oracle's recorded fields, every reached cell
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", SCENES)
def test_oracle_scenes(pvlib, oracle, name, setting):
    p, vx, vy, delay, fs = oracle_run(oracle, name)
    assert p.shape == (435, 70, 70) and fs == 1443
    got, _ = scene_map(pvlib, oracle, name, setting)
    want = ref.echogram(p, vx, vy, delay, fs, *setting)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s %s: %d values differ, first at %s: %s vs %s" % (name, setting, bad.sum(), np.argwhere(bad)[0],
                                                                             got[bad][:4], want[bad][:4])
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached) and np.isfinite(got[reached]).all()
    full = ref.slot_steps(setting[0], fs) * setting[1]
    cut = reached & (got[..., 0] < full)
    onset = np.where(reached, delay, 0).astype(np.int64)
    assert np.array_equal(cut, reached & (onset + full > 435))
    # a slot the record does not reach: onset + j ns >= T
    empty = int(((onset[reached][:, None] + ref.slot_steps(setting[0], fs) * np.arange(setting[1])[None, :]) >= 435).sum())
    print(name, setting, "reached", reached.sum(), "cut by T", cut.sum(), "slots not reached", empty)
    if setting == (0.01, 24):
        if name != "g71_shoebox":
            assert cut.sum() > 100  # (the cut-off path is exercised)
        e = got[..., 1::3]
        unreached_slots = (onset[..., None] + 14 * np.arange(24)) >= 435
        assert (e[reached & cut][unreached_slots[reached & cut]] == 0).all()
    else:
        assert cut.sum() == 0


# 2. slot 0 at 5 ms is the direct-sound flux of the lateral-fraction records: the same sums over k < n5 in the same order
@pytest.mark.parametrize("name", SCENES)
def test_slot_zero_is_the_lateral_flux(pvlib, oracle, name):
    got, delay = scene_map(pvlib, oracle, name, (0.005, 16))
    lat, _ = lateral_scene_map(pvlib, oracle, name)
    reached = delay < ref.NO_ONSET
    assert same_bits(got[..., 2][reached], lat[..., 6][reached]).all()
    assert same_bits(got[..., 3][reached], lat[..., 7][reached]).all()


# 3. hand-made series
def check(pvlib, p, vx, vy, fs, onset, slot_seconds, n_slots):
    got = pvlib.host_echogram(p, vx, vy, fs, onset, slot_seconds, n_slots)
    want = ref.echogram_ir(p, vx, vy, fs, onset, slot_seconds, n_slots)
    assert got.dtype == np.float32 and got.shape == (1 + 3 * n_slots,)
    assert same_bits(got, want).all(), (fs, onset, len(p), slot_seconds, n_slots, got, want)
    return got


def series(seed, T):
    rng = np.random.default_rng(seed)
    return tuple((rng.standard_normal(T) * s).astype(np.float32) for s in (1e-2, 3e-5, 2e-5))


@pytest.mark.parametrize("n_slots", [1, 5, 32])
@pytest.mark.parametrize("slot_seconds", [0.0007, 0.005])
def test_window_cut_off_by_the_record(pvlib, slot_seconds, n_slots):
    """onset at T - 1; the window ending exactly at T, one step before, one step after; ns = 1; 1 and 32 slots"""
    fs, T = 1443, 300
    ns = ref.slot_steps(slot_seconds, fs)
    w = ns * n_slots
    assert ns == (1 if slot_seconds == 0.0007 else 7) and w < T
    p, vx, vy = series(n_slots, T)
    for onset, n in ((0, w), (T - w - 1, w), (T - w, w), (T - w + 1, w - 1), (T - 1, 1)):
        if onset >= T:  # (a window of one step cannot end past T)
            assert w == 1
            continue
        m = check(pvlib, p, vx, vy, fs, onset, slot_seconds, n_slots)
        assert m[0] == min(n, w) and np.isfinite(m).all()
        filled = -(-int(m[0]) // ns)  # slots with at least one member
        assert (m[1:1 + 3 * filled:3] > 0).all() and (m[1 + 3 * filled:] == 0).all()
        assert not np.signbit(m[1 + 3 * filled:]).any()  # (+0.0f)
    m = check(pvlib, p, vx, vy, fs, T - 1, slot_seconds, n_slots)
    assert m[1] == p[T - 1] * p[T - 1] and m[2] == p[T - 1] * vx[T - 1] and m[3] == p[T - 1] * vy[T - 1]


def test_known_values(pvlib):
    """a constant p with vx only, then vy only: ix[j] = ns p vx exactly (small powers of two); a sign flip"""
    fs, T, onset, ns, n_slots = 1443, 300, 10, 7, 16
    p = np.full(T, 0.5, np.float32)
    vx = np.full(T, 0.25, np.float32)
    zero = np.zeros(T, np.float32)
    m = check(pvlib, p, vx, zero, fs, onset, 0.005, n_slots)
    assert m[0] == ns * n_slots
    assert (m[1::3] == ns * 0.25).all() and (m[2::3] == ns * 0.125).all() and (m[3::3] == 0).all()
    m = check(pvlib, p, zero, vx, fs, onset, 0.005, n_slots)
    assert (m[2::3] == 0).all() and (m[3::3] == ns * 0.125).all()
    m = check(pvlib, p, -vx, zero, fs, onset, 0.005, n_slots)
    assert (m[2::3] == -ns * 0.125).all()
    # the flux changes sign from slot 3 on; a slot that straddles nothing
    flip = vx.copy()
    flip[onset + 3 * ns:] *= -1
    m = check(pvlib, p, flip, zero, fs, onset, 0.005, n_slots)
    assert (m[2:2 + 9:3] == ns * 0.125).all() and (m[2 + 9::3] == -ns * 0.125).all()
    # and in the middle of slot 3: 3 steps forth, 4 back
    flip = vx.copy()
    flip[onset + 3 * ns + 3:] *= -1
    m = check(pvlib, p, flip, zero, fs, onset, 0.005, n_slots)
    assert m[2 + 9] == -0.125 and (m[2 + 12::3] == -ns * 0.125).all()
    # samples before the onset do not enter
    q = p.copy()
    q[:onset] = 100.0
    assert same_bits(check(pvlib, q, vx, zero, fs, onset, 0.005, n_slots), check(pvlib, p, vx, zero, fs, onset, 0.005, n_slots)).all()


def test_random_series(pvlib):
    rng = np.random.default_rng(20261018)
    for _ in range(150):
        T = int(rng.integers(1, 500))
        fs = int(rng.choice([1443, 1968, 700, 4000, 12]))
        n_slots = int(rng.integers(1, 33))
        ns = int(rng.integers(1, 40))
        slot_seconds = float(np.float32((ns + 0.5) / fs))
        assert ref.slot_steps(slot_seconds, fs) == ns
        p, vx, vy = ((rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32) for _ in range(3))
        check(pvlib, p, vx, vy, fs, int(rng.integers(0, T)), slot_seconds, n_slots)


# 4. sanity, on the float32 records of the oracle scenes at (0.005, 16)
def test_sanity(pvlib, oracle):
    cos_median = {}
    for name in SCENES:
        p, vx, vy, delay, fs = oracle_run(oracle, name)
        got, _ = scene_map(pvlib, oracle, name, (0.005, 16))
        reached = delay < ref.NO_ONSET
        # the slot energies add up to the energy of the window
        p64 = p.astype(np.float64)
        for x, y in np.argwhere(reached)[::7]:
            t0 = int(delay[x, y])
            n = int(got[x, y, 0])
            want = (p64[t0:t0 + n, x, y] ** 2).sum()
            assert abs(got[x, y, 1::3].astype(np.float64).sum() - want) <= 1e-5 * want, (name, x, y)
        # slot 0's flux points away from the listener
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]
        X, Y = np.meshgrid(np.arange(delay.shape[0]), np.arange(delay.shape[1]), indexing="ij")
        rx, ry = (X - lx).astype(np.float64), (Y - ly).astype(np.float64)
        far = reached & (np.hypot(rx, ry) > 3)
        fx, fy = got[..., 2].astype(np.float64), got[..., 3].astype(np.float64)
        with np.errstate(all="ignore"):
            cos = (fx * rx + fy * ry) / (np.hypot(fx, fy) * np.hypot(rx, ry))
        cos_median[name] = float(np.median(cos[far]))
        assert far.sum() > 1000
    print(cos_median)
    assert cos_median["g71_empty"] > 0.99 and cos_median["g71_shoebox"] > 0.99


# 5. bad arguments
def test_bad_arguments(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = np.empty(1 + 3 * 33, np.float32)
    fp, op = p.ctypes.data_as(FP), out.ctypes.data_as(FP)
    nan, inf = float("nan"), float("inf")
    for args in ((None, fp, fp, 8, 1443, 0, 0.005, 4, op), (fp, None, fp, 8, 1443, 0, 0.005, 4, op),
                 (fp, fp, None, 8, 1443, 0, 0.005, 4, op), (fp, fp, fp, 8, 1443, 0, 0.005, 4, None),
                 (fp, fp, fp, 0, 1443, 0, 0.005, 4, op), (fp, fp, fp, -3, 1443, 0, 0.005, 4, op),
                 (fp, fp, fp, 8, 1443, -1, 0.005, 4, op), (fp, fp, fp, 8, 1443, 8, 0.005, 4, op),
                 (fp, fp, fp, 8, 1443, 0, 0.005, 0, op), (fp, fp, fp, 8, 1443, 0, 0.005, -1, op),
                 (fp, fp, fp, 8, 1443, 0, 0.005, 33, op),
                 (fp, fp, fp, 8, 1443, 0, nan, 4, op), (fp, fp, fp, 8, 1443, 0, inf, 4, op), (fp, fp, fp, 8, 1443, 0, -inf, 4, op),
                 (fp, fp, fp, 8, 1443, 0, 0.0, 4, op), (fp, fp, fp, 8, 1443, 0, -0.005, 4, op),
                 (fp, fp, fp, 8, 1443, 0, 0.0006, 4, op),  # ns = 0
                 (fp, fp, fp, 8, 1443, 0, 1000.0, 4, op), (fp, fp, fp, 8, 1443, 0, 3.0e38, 4, op)):  # ns > 2^20
        assert L.PvAmdHostEchogram(*args) == -1, args
        assert pvlib.last_error().startswith("echogram: "), pvlib.last_error()
    assert L.PvAmdHostEchogram(fp, fp, fp, 8, 1443, 7, 0.005, 32, op) == 0
    assert L.PvAmdHostEchogram(fp, fp, fp, 8, 1024, 0, 1024.0, 1, op) == 0 and out[0] == 8  # ns = 2^20
    assert L.PvAmdHostEchogram(fp, fp, fp, 8, 1024, 0, 1025.0, 1, op) == -1
    # the solver calls refuse a null handle
    sec, steps = C.c_float(0.0), C.c_int(0)
    for call in (lambda: L.PvAmdSetEchogram(None, 0.005, 16), lambda: L.PvAmdSetEchogram(None, 0.005, 0),
                 lambda: L.PvAmdGetEchogramSlots(None, C.byref(sec), C.byref(steps)),
                 lambda: L.PvAmdComputeEchogram(None, None), lambda: L.PvAmdCopyEchogram(None, op),
                 lambda: L.PvAmdCopyEchogramBlock(None, 0, 0, 1, 1, op), lambda: L.PvAmdGetEchogram(None, 0.0, 0.0, 0.0, op)):
        assert call() == -1
        assert pvlib.last_error().startswith("echogram: "), pvlib.last_error()


# 6. exports
NEW_EXPORTS = ["PvAmdSetEchogram", "PvAmdGetEchogramSlots", "PvAmdComputeEchogram", "PvAmdCopyEchogram", "PvAmdCopyEchogramBlock",
               "PvAmdGetEchogram", "PvAmdHostEchogram"]


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
    assert re.search(r"^#define\s+PVA_ECHOGRAM_MAX_SLOTS\s+32\s*$", hdr, re.M)
    assert pvlib.ECHOGRAM_MAX_SLOTS == ref.MAX_SLOTS == 32
