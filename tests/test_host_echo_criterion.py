"""CPU: PvAmdHostEchoCriterion -- the echo-criterion definition of include/planeverb_amd.h (PvAmdEchoCriterion) applied to one
impulse response -- against the numpy restatement of tests/_echo_ref.py, bit for bit (tolerance 0), and against closed forms on
hand-made series.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
import _echo_ref as ref
from _room_metrics_ref import threshold_onset

FP = C.POINTER(C.c_float)
S_EK, S_TK, S_EKL, S_TKL, S_TS, M_EK, M_TK, M_EKL, M_TKL, M_TS = range(10)


def check(pvlib, p, fs, onset):
    got = pvlib.host_echo_criterion(p, fs, onset)
    want = ref.echo_criterion_ir(p, fs, onset)
    assert got.dtype == np.float32 and got.shape == (10,)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    return got


def steps(seconds, fs):
    """a record's delay back in steps: (float)k / (float)fs is exact enough to round-trip for k < 2^24"""
    return int(round(float(seconds) * fs))


@pytest.mark.parametrize("name", ["g71_smallroom", "g96_smallroom_res375"])
def test_reference_impulse_responses(pvlib, name):
    """the reference's own impulse responses, each with its onset from the restated threshold scan"""
    g = golden(name)
    fs = int(pvlib.host_grid_info(float(g["size"]), float(g["size"]), int(g["res"])).fs)
    assert fs == (1443 if name == "g71_smallroom" else 1968)
    n = 0
    for ir in g["probe_ir"]:
        p = np.ascontiguousarray(ir[:, 0])
        onset = threshold_onset(p)
        if onset < 0:
            continue
        m = check(pvlib, p, fs, onset)
        assert np.isfinite(m).all() and m[S_EK] > 0 and m[M_EK] > 0 and m[S_TS] > 0 and m[M_TS] > 0
        n += 1
    assert n >= 4, n


def test_random_impulse_responses(pvlib):
    rng = np.random.default_rng(20261019)
    for _ in range(200):
        T = int(rng.integers(1, 601))
        fs = int(rng.choice([1443, 1968, 700, 4000, 112]))
        p = (rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32)
        check(pvlib, p, fs, int(rng.integers(0, T)))


def test_lags_and_limits():
    assert ref.lags(1443) == (12, 72, 20, 115)
    assert ref.lags(1968) == (17, 98, 27, 157)
    assert ref.lags(112)[0] == 1 and ref.lags(111)[0] == 0
    assert ref.SPEECH_EXPONENT == np.float32(0.6666667) and float(ref.SPEECH_EXPONENT).hex() == "0x1.5555560000000p-1"


def two_pulses(T, onset, e):
    p = np.zeros(T, np.float32)
    p[onset] = 1.0
    p[onset + e] = 1.0
    return p


@pytest.mark.parametrize("fs", [1443, 1968])
def test_two_unit_pulses(pvlib, fs):
    """p[onset] = p[onset + e] = 1: both weights are 1, c steps from 0 to e / 2 at k = e, so x = (e / 2) / nD on the plateau
    k = e .. e + nD - 1 and falls to 0 at k = e + nD.  kk is the plateau's first step; the late maximum sees the part of the
    plateau at or past nL.  The library's own nD and nL show in the values"""
    nDs, nLs, nDm, nLm = ref.lags(fs)
    T, onset = 600, 7
    for e in (1, 2, nDs - 1, nDs, nDs + 1, nDm, nDm + 3, 40, nLs - nDs, nLs - nDs + 1, nLs - 1, nLs, nLm - nDm, nLm - nDm + 1,
              nLm - 1, nLm, 300):
        m = check(pvlib, two_pulses(T, onset, e), fs, onset)
        half = np.float32(e) / np.float32(2.0)
        for o, nD, nL in ((0, nDs, nLs), (5, nDm, nLm)):
            assert m[o + 0] == half / np.float32(nD) and steps(m[o + 1], fs) == e, (fs, e, o, m)
            assert m[o + 1] == np.float32(e) / np.float32(fs)
            assert m[o + 4] == half / np.float32(fs)
            if e + nD <= nL:  # x is back at 0 from k = e + nD on: nothing past the limit
                assert m[o + 2] == 0 and m[o + 3] == 0 and not np.signbit(m[o + 2]), (fs, e, o, m)
            else:  # the first step of the plateau at or past nL
                assert m[o + 2] == m[o + 0] and steps(m[o + 3], fs) == max(e, nL), (fs, e, o, m)
    # x falls to 0 at k = e + nD: a later, smaller pair of steps cannot be hidden by the first plateau once it has ended, and
    # the first maximum is the one reported
    e = 30
    p = two_pulses(T, onset, e)
    m0 = check(pvlib, p, fs, onset)
    for o, nD in ((0, nDs), (5, nDm)):
        q = p[:onset + e + nD].copy()  # the record ends with the plateau's last step
        r = check(pvlib, q, fs, onset)
        assert r[o + 0] == m0[o + 0] and r[o + 1] == m0[o + 1]
    # samples before the onset do not enter
    q = p.copy()
    q[:onset] = 100.0
    assert same_bits(check(pvlib, q, fs, onset), m0).all()


@pytest.mark.parametrize("fs", [1443, 1968, 112])
def test_short_and_empty_responses(pvlib, fs):
    nDs, nLs, nDm, nLm = ref.lags(fs)
    rng = np.random.default_rng(fs)
    T = 400
    p = (rng.standard_normal(T) * 1e-2).astype(np.float32)
    assert p[T - 1] != 0
    # onset = T - 1: one step, c(0) = 0 / w = 0, every maximum stays +0 and both ts are 0
    m = check(pvlib, p, fs, T - 1)
    assert (m == 0).all() and not np.signbit(m).any()
    # N <= nL: the late maximum stays +0 / 0; N = nL + 1 is the first response that can have one
    for nD, nL, o in ((nDs, nLs, 0), (nDm, nLm, 5)):
        for N in (1, 2, nD, nD + 1, nL - 1, nL):
            if N < 1:
                continue
            m = check(pvlib, p, fs, T - N)
            assert m[o + 2] == 0 and m[o + 3] == 0 and not np.signbit(m[o + 2]), (fs, N, o, m)
            if N > 1:
                assert m[o + 0] > 0
        q = np.zeros(T, np.float32)  # a step of c exactly at k = nL, in a response of nL + 1 steps
        q[T - nL - 1] = 1.0
        q[T - 1] = 1.0
        m = check(pvlib, q, fs, T - nL - 1)
        assert m[o + 2] == (np.float32(nL) / np.float32(2.0)) / np.float32(nD) and steps(m[o + 3], fs) == nL
    # an all-zero response: A = 0, c = 0 / 0, no x ever wins, ts is NaN
    m = check(pvlib, np.zeros(T, np.float32), fs, 10)
    for o in (0, 5):
        assert (m[o:o + 4] == 0).all() and not np.signbit(m[o:o + 4]).any() and np.isnan(m[o + 4])
    # zeros up to a late first sample: NaN x until then
    q = np.zeros(T, np.float32)
    q[200:] = p[200:]
    m = check(pvlib, q, fs, 10)
    assert np.isfinite(m).all() and m[S_EK] > 0


def test_sampling_rate_limit(pvlib):
    L = pvlib.lib()
    p = np.ones(64, np.float32)
    out = pvlib.PvAmdEchoCriterion()
    fp = p.ctypes.data_as(FP)
    for fs in (111, 100, 1, 0, -5):
        assert L.PvAmdHostEchoCriterion(fp, 64, fs, 0, out) == -1, fs
        assert pvlib.last_error().startswith("echo: "), pvlib.last_error()
    assert L.PvAmdHostEchoCriterion(fp, 64, 112, 0, out) == 0
    with pytest.raises(pvlib.PlaneverbError, match="echo: "):
        pvlib.host_echo_criterion(p, 111, 0)
    check(pvlib, p, 112, 3)


def test_bad_arguments(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = pvlib.PvAmdEchoCriterion()
    fp = p.ctypes.data_as(FP)
    for args in ((None, 8, 1443, 0, out), (fp, 8, 1443, 0, None), (fp, 0, 1443, 0, out), (fp, -3, 1443, 0, out),
                 (fp, 8, 1443, -1, out), (fp, 8, 1443, 8, out)):
        assert L.PvAmdHostEchoCriterion(*args) == -1, args
        assert pvlib.last_error().startswith("echo: "), pvlib.last_error()
    assert L.PvAmdHostEchoCriterion(fp, 8, 1443, 7, out) == 0
    # the solver calls refuse a null handle
    for call in (lambda: L.PvAmdComputeEchoCriterion(None, None), lambda: L.PvAmdCopyEchoCriterion(None, fp),
                 lambda: L.PvAmdCopyEchoCriterionBlock(None, 0, 0, 1, 1, fp),
                 lambda: L.PvAmdGetEchoCriterion(None, 0.0, 0.0, 0.0, out)):
        assert call() == -1
        assert pvlib.last_error().startswith("echo: "), pvlib.last_error()


NEW_EXPORTS = ["PvAmdComputeEchoCriterion", "PvAmdCopyEchoCriterion", "PvAmdCopyEchoCriterionBlock", "PvAmdGetEchoCriterion",
               "PvAmdHostEchoCriterion"]


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
    assert pvlib.ECHO_CRITERION_NAMES == ref.NAMES
    assert C.sizeof(pvlib.PvAmdEchoCriterion) == 40
    assert re.search(r"^#define\s+PVA_ECHO_SPEECH_EXPONENT\s+0\.6666667f\b", hdr, re.M)
    assert re.search(r"^#define\s+PVA_ECHO_SPEECH_CRIT\s+1\.0f\s*$", hdr, re.M)
    assert re.search(r"^#define\s+PVA_ECHO_MUSIC_CRIT\s+1\.8f\s*$", hdr, re.M)
    assert (pvlib.ECHO_SPEECH_CRIT, pvlib.ECHO_MUSIC_CRIT) == (float(ref.SPEECH_CRIT), 1.8)
