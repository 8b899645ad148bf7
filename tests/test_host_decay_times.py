"""CPU: PvAmdHostDecayTimes -- the decay-time definition of include/planeverb_amd.h (PvAmdDecayTimes: EDT, T20, T30 off the
backward-integrated curve) applied to one impulse response -- against the numpy restatement of tests/_decay_ref.py, bit for bit
(tolerance 0), and against impulse responses whose decay time is known.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _decay_ref as ref

QNAN_BITS = 0x7fc00000


def check(pvlib, p, fs, onset):
    got = pvlib.host_decay_times(p, fs, onset)
    want = ref.decay_times_ir(p, fs, onset)
    assert got.dtype == np.float32 and got.shape == (8,)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    # (same_bits calls any two NaNs equal: the definition names the bit pattern of a time that is not given)
    assert (got[:3].view(np.uint32)[np.isnan(got[:3])] == QNAN_BITS).all(), got
    return got


def decaying_noise(rng, T, fs, rt, onset=0):
    """seeded noise under an exponential envelope that loses 60 dB in rt seconds, from step `onset` on"""
    env = 10.0 ** (-3.0 * np.maximum(np.arange(T) - onset, 0) / (rt * fs))
    return (rng.standard_normal(T) * env * 10.0 ** rng.uniform(-4, 1)).astype(np.float32)


def exponential(T, fs, rt, onset):
    """p(t) = (-1)^k 10^(-3 k / (rt fs)), k = t - onset >= 0: the backward-integrated curve falls 60 dB in rt seconds exactly"""
    p = np.zeros(T, np.float64)
    k = np.arange(T - onset)
    p[onset:] = (-1.0) ** k * 10.0 ** (-3.0 * k / (rt * fs))
    return p.astype(np.float32)


def test_random_impulse_responses(pvlib):
    rng = np.random.default_rng(20261018)
    seen = np.zeros(3, int)
    for _ in range(120):
        T = int(rng.integers(20, 601))
        fs = int(rng.choice([1443, 1968]))
        onset = int(rng.integers(0, T))
        m = check(pvlib, decaying_noise(rng, T, fs, float(rng.uniform(0.02, 0.5)), onset if rng.random() < 0.5 else 0), fs, onset)
        seen += ~np.isnan(m[:3])
    assert (seen > 10).all() and (seen < 120).all(), seen  # (both the complete and the incomplete branch, in every range)


@pytest.mark.parametrize("fs", [1443, 1968])
def test_onsets(pvlib, fs):
    """onset 0, mid-record, tEnd - 1, tEnd and T - 1"""
    rng = np.random.default_rng(fs)
    T = 435
    t_end = T - ref.tail_n(fs)
    p = decaying_noise(rng, T, fs, 0.04)
    p[200:] += decaying_noise(rng, T, fs, 0.03, 200)[200:]
    for onset in (0, 200, t_end - 1, t_end, T - 1):
        m = check(pvlib, p, fs, onset)
        assert np.isfinite(m[6]) and m[6] > 0
        if onset >= t_end:  # the onset lies in the tail
            assert np.isnan(m[:3]).all() and (m[3:6] == 0).all() and np.isnan(m[7])
        else:
            assert np.isfinite(m[7]) and m[7] <= 0 and m[3] >= 1
    assert np.isfinite(check(pvlib, p, fs, 0)[:3]).all() and np.isfinite(check(pvlib, p, fs, 200)[:3]).all()


def test_tail_length():
    assert (ref.tail_n(1443), ref.tail_n(1968)) == (14, 19)


@pytest.mark.parametrize("onset", [0, 100])
@pytest.mark.parametrize("rt,points", [(0.03, (8, 15, 22)), (0.05, (13, 24, 36)), (0.1, (25, 48, 72)), (0.15, (37, 72, 108))])
def test_known_decay_time(pvlib, rt, points, onset):
    """an exact exponential decay: EDT, T20 and T30 within 1e-3 relative of its decay time (the numpy prototype of the definition
    gives < 1e-5: 1e-3 leaves room for the float32 curve and catches any wrong range, sign, factor or fs), and the point counts
    exactly -- they pin the range limits"""
    m = check(pvlib, exponential(435, 1443, rt, onset), 1443, onset)
    print(rt, onset, m)
    assert tuple(m[3:6]) == points
    for v in m[:3]:
        assert abs(v / rt - 1.0) < 1e-3, m
    assert m[6] > 1.0 and m[7] < -35.0


def test_incomplete_ranges(pvlib):
    """a curve that has fallen only 20 dB when the tail begins (a fast decay, then a plateau held up by one late sample): EDT is a
    number, T20 and T30 are the quiet NaN, their n is still reported and depth says why"""
    fs, T = 1443, 435
    p = exponential(T, fs, 0.05, 0)
    total = float((p.astype(np.float64) ** 2).sum())
    p[T - 1] = np.sqrt(total / 99.0)  # E(T - 1) = E0 / 100
    m = check(pvlib, p, fs, 0)
    assert np.isfinite(m[0]) and 0.04 < m[0] < 0.06
    assert (m.view(np.uint32)[1:3] == QNAN_BITS).all()
    assert m[3] >= 8 and m[4] > 300 and m[5] == m[4]  # (every step of the plateau lies inside -5 .. -25 dB)
    assert abs(m[7] + 20.0) < 0.1, m


def test_one_step_interval(pvlib):
    """a range whose interval has exactly one step: NaN with n == 1 although the range is complete"""
    fs, T = 1443, 100
    p = np.zeros(T, np.float32)
    p[10], p[11], p[12] = 1.0, np.sqrt(0.25), 1e-3  # r = 1, 0.2 (one EDT step more, the only one below -5 dB), 8e-7
    m = check(pvlib, p, fs, 10)
    assert tuple(m[3:6]) == (2, 1, 1)
    assert np.isfinite(m[0]) and m[0] > 0 and np.isnan(m[1]) and np.isnan(m[2])
    assert m[7] < -35.0  # (complete: the curve is far below every lower limit before the tail)
    p[11] = 0.0  # EDT alone with the onset step
    m = check(pvlib, p, fs, 10)
    assert tuple(m[3:6]) == (1, 0, 0) and np.isnan(m[:3]).all()


def test_bad_arguments(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = pvlib.PvAmdDecayTimes()
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    assert L.PvAmdHostDecayTimes(None, 8, 1443, 0, out) == -1
    assert pvlib.last_error().startswith("decay times: ")
    assert L.PvAmdHostDecayTimes(fp, 8, 1443, 0, None) == -1
    assert L.PvAmdHostDecayTimes(fp, 0, 1443, 0, out) == -1
    assert L.PvAmdHostDecayTimes(fp, -3, 1443, 0, out) == -1
    assert L.PvAmdHostDecayTimes(fp, 8, 1443, -1, out) == -1
    assert L.PvAmdHostDecayTimes(fp, 8, 1443, 8, out) == -1
    assert L.PvAmdHostDecayTimes(fp, 8, 1443, 7, out) == 0
    # the solver calls refuse a null handle
    for call in (lambda: L.PvAmdComputeDecayTimes(None, None), lambda: L.PvAmdCopyDecayTimes(None, fp),
                 lambda: L.PvAmdCopyDecayTimesBlock(None, 0, 0, 1, 1, fp), lambda: L.PvAmdGetDecayTimes(None, 0.0, 0.0, 0.0, out)):
        assert call() == -1
        assert pvlib.last_error().startswith("decay times: "), pvlib.last_error()


NEW_EXPORTS = ["PvAmdComputeDecayTimes", "PvAmdCopyDecayTimes", "PvAmdCopyDecayTimesBlock", "PvAmdGetDecayTimes",
               "PvAmdHostDecayTimes"]


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
    assert pvlib.DECAY_TIME_NAMES == ref.NAMES
    assert C.sizeof(pvlib.PvAmdDecayTimes) == 32
