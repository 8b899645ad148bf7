"""CPU: the spectrum definition of include/planeverb_amd.h on the host -- PvAmdHostSpectrumTables against numpy in double,
PvAmdHostSpectrum against the numpy restatement of tests/_spectrum_ref.py bit for bit (tolerance 0) and against the textbook
DFT within the sequential-summation bound, and the bin rule of PvAmdSetSpectrumBins.  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
import _spectrum_ref as ref

IRRATIONAL = [np.sqrt(2.0) * 100.0, np.pi * 10.0, np.e * 100.0, 61.7, 1.0 / 3.0]


def check_tables(pvlib, T, fs, hz):
    c, s = pvlib.host_spectrum_tables(T, fs, hz)
    assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (T, len(hz)) and s.shape == c.shape
    wc, ws = ref.tables_f64(T, fs, hz)
    for got, want in ((c, wc), (s, ws)):
        ulp = np.spacing(np.abs(want.astype(np.float32))).astype(np.float64)  # one float32 ulp at the value
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= ulp).all(), (T, fs, err.max(), np.argwhere(err > ulp)[:4])
    assert (c[0] == 1).all() and (s[0] == 0).all()
    return c, s


@pytest.mark.parametrize("T,fs,hz", [
    (435, 1443, [0.0, 1443 / 2.0, 1443 / 4.0] + IRRATIONAL),
    (435, 1443, [0, 30, 61.7, 100, 137.5, 200, 250, 275]),
    (3179, 10556, [0.5, 0.0, 10556 / 2.0, 10556 / 4.0] + IRRATIONAL),
])
def test_tables_against_numpy_in_double(pvlib, T, fs, hz):
    """every entry within one float32 ulp of the double value (libm and double-rounding differences); row 0 and the 0 Hz bin exact"""
    c, s = check_tables(pvlib, T, fs, hz)
    j0 = hz.index(0.0) if 0.0 in hz else hz.index(0)
    assert (c[:, j0] == 1).all() and (s[:, j0] == 0).all()


def check_ir(pvlib, p, fs, onset, hz, pulse):
    got = pvlib.host_spectrum(p, fs, onset, hz, pulse)
    c, s = pvlib.host_spectrum_tables(len(p), fs, hz)
    want = ref.spectrum_ir(p, onset, c, s, pulse)
    assert got.dtype == np.float32 and got.shape == (len(hz), 3)
    assert same_bits(got, want).all(), (fs, onset, len(p), len(hz), got, want)
    return got


BINS8 = [0, 30, 61.7, 100, 137.5, 200, 250, 275]


@pytest.mark.parametrize("name", ["g71_smallroom", "g96_smallroom_res375"])
def test_reference_impulse_responses(pvlib, name):
    """the reference's own impulse responses, each with its onset from the restated threshold scan, against the grid's pulse"""
    g = golden(name)
    size, res = float(g["size"]), int(g["res"])
    fs = int(pvlib.host_grid_info(size, size, res).fs)
    pulse = pvlib.host_pulse(size, size, res)
    n = 0
    for ir in g["probe_ir"]:
        p = np.ascontiguousarray(ir[:, 0])
        assert len(p) == len(pulse)
        onset = ref.threshold_onset(p)
        if onset < 0:
            continue
        m = check_ir(pvlib, p, fs, onset, BINS8, pulse)
        assert np.isfinite(m).all()
        n += 1
    assert n >= 4, n


def test_random_impulse_responses(pvlib):
    rng = np.random.default_rng(20261017)
    for i in range(200):
        T = int(rng.integers(1, 601))
        fs = int(rng.choice([1443, 1968, 700, 4000, 12]))
        n = (1, 7, 8, 9, 32)[i % 5]
        p = (rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32)
        pulse = (rng.standard_normal(T) * 10.0 ** rng.uniform(-3, 0)).astype(np.float32)
        hz = (rng.uniform(0, fs / 2.0, n)).astype(np.float32)
        hz = np.minimum(hz, np.float32(fs / 2.0))
        check_ir(pvlib, p, fs, int(rng.integers(0, T)), hz, pulse)


def test_edges(pvlib):
    """onset = T - 1 (one term per sum), an all-zero response, a zero source, a denormal response"""
    rng = np.random.default_rng(7)
    T, fs = 400, 1443
    p = (rng.standard_normal(T) * 1e-2).astype(np.float32)
    pulse = (rng.standard_normal(T) * 1e-1).astype(np.float32)
    c, s = pvlib.host_spectrum_tables(T, fs, BINS8)
    m = check_ir(pvlib, p, fs, T - 1, BINS8, pulse)
    assert same_bits(m[:, 0], p[T - 1] * c[T - 1]).all() and same_bits(m[:, 1], p[T - 1] * s[T - 1]).all()
    z = check_ir(pvlib, np.zeros(T, np.float32), fs, 17, BINS8, pulse)
    assert (z[:, :2] == 0).all() and np.isneginf(z[:, 2]).all()
    q = check_ir(pvlib, p, fs, 3, BINS8, np.zeros(T, np.float32))  # spow = 0: +inf as IEEE says
    assert np.isposinf(q[:, 2]).all()
    q = check_ir(pvlib, np.zeros(T, np.float32), fs, 3, BINS8, np.zeros(T, np.float32))  # 0 / 0
    assert np.isnan(q[:, 2]).all() and (q[:, :2] == 0).all()
    d = check_ir(pvlib, (p * np.float32(1e-36)).astype(np.float32), fs, 0, BINS8, pulse)  # denormal products are kept
    assert (d[:, 0] != 0).any()


def dft_case(pvlib, p, fs, onset, ks):
    T = len(p)
    hz = np.array([k * fs / T for k in ks], np.float32)
    got = pvlib.host_spectrum(p, fs, onset, hz, np.ones(T, np.float32))
    z = p.astype(np.float64)
    z[:onset] = 0
    X = np.fft.rfft(z)[list(ks)]  # X = re - i im
    bound = 2.0 * (T + 1) * 2.0 ** -24 * np.abs(z).sum()
    err = max(np.abs(got[:, 0].astype(np.float64) - X.real).max(), np.abs(got[:, 1].astype(np.float64) + X.imag).max())
    print("dft: T %d fs %d onset %d err %.3e bound %.3e" % (T, fs, onset, err, bound))
    assert err <= bound, (err, bound)


def test_against_the_textbook_dft(pvlib):
    """with bins at k fs / T, re - i im is the DFT of the onset-zeroed response.  Bound per component, derived: the sequential
    float32 sum of T terms has a first-order error of (T - 1) u sum|p(t) w(t)|, u = 2^-24, each product adds u |p w| and each
    rounded twiddle u |p|: (T + 1) u sum|p(t)| with |w| <= 1; the factor 2 is margin over the first order (it also covers the
    rounding of the frequency itself to float32, 2 pi k u sum|p| at worst: k <= 32 << T here, and none where fs / T is exact)"""
    g = golden("g71_smallroom")
    fs = int(pvlib.host_grid_info(float(g["size"]), float(g["size"]), int(g["res"])).fs)
    for ir in g["probe_ir"]:
        p = np.ascontiguousarray(ir[:, 0])
        onset = ref.threshold_onset(p)
        if onset >= 0:
            dft_case(pvlib, p, fs, onset, range(0, 32))
    rng = np.random.default_rng(3)
    p = rng.standard_normal(481).astype(np.float32)  # fs / T = 3 exactly: every bin up to fs / 2
    dft_case(pvlib, p, 1443, 0, range(0, 241, 8))
    dft_case(pvlib, p, 1443, 200, range(1, 241, 8))


def test_bin_rule(pvlib):
    """the refusals of PvAmdSetSpectrumBins, through the host calls that apply the same rule (pv_spectrum.h spectrumBinsError;
    PvAmdSetSpectrumBins checks the bins against its grid's fs before it touches a device -- a handle cannot exist without one,
    tests/test_gpu_spectrum.py makes the same calls on a solver)"""
    L = pvlib.lib()
    T, fs = 16, 1443
    c = np.zeros((T, 40), np.float32)
    s = np.zeros((T, 40), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def tables(hz, n=None):
        h = np.asarray(hz, np.float32)
        return L.PvAmdHostSpectrumTables(T, fs, fp(h) if h.size else None, len(h) if n is None else n, fp(c), fp(s))

    assert tables([100.0]) == 0
    assert tables([0.0, fs / 2.0]) == 0  # both ends are inside
    assert tables(np.full(32, 5.0)) == 0
    for bad, what in (([], "bins"), (np.full(33, 5.0), "bins"), ([float("nan")], "finite"), ([float("inf")], "finite"),
                      ([10.0, -1.0], "negative"), ([10.0, fs / 2.0 + 0.25], "fs / 2")):
        assert tables(bad) == -1, bad
        assert pvlib.last_error().startswith("spectrum:") and what in pvlib.last_error(), pvlib.last_error()
    assert tables([100.0], n=-1) == -1 and tables([100.0], n=0) == -1
    assert L.PvAmdHostSpectrumTables(T, fs, None, 1, fp(c), fp(s)) == -1
    assert L.PvAmdHostSpectrumTables(0, fs, fp(c), 1, fp(c), fp(s)) == -1
    p = np.ones(T, np.float32)
    out = np.zeros(96, np.float32)
    h = np.array([100.0, 800.0], np.float32)
    assert L.PvAmdHostSpectrum(fp(p), T, fs, 0, fp(h), 2, fp(p), fp(out)) == -1 and "fs / 2" in pvlib.last_error()
    assert L.PvAmdHostSpectrum(fp(p), T, fs, T, fp(h), 1, fp(p), fp(out)) == -1
    assert L.PvAmdHostSpectrum(fp(p), T, fs, 0, fp(h), 1, None, fp(out)) == -1
    assert L.PvAmdHostSpectrum(fp(p), T, fs, 0, fp(h), 1, fp(p), fp(out)) == 0
    # the solver calls refuse a null handle
    for r in (L.PvAmdSetSpectrumBins(None, fp(h), 1), L.PvAmdGetSpectrumBins(None, fp(out), 32), L.PvAmdGetSpectrumSource(None, fp(out)),
              L.PvAmdComputeSpectrum(None, None), L.PvAmdCopySpectrum(None, fp(out)), L.PvAmdCopySpectrumBlock(None, 0, 0, 1, 1, fp(out)),
              L.PvAmdGetSpectrum(None, 0.0, 0.0, 0.0, fp(out))):
        assert r == -1 and pvlib.last_error()


NEW_EXPORTS = ["PvAmdSetSpectrumBins", "PvAmdGetSpectrumBins", "PvAmdGetSpectrumSource", "PvAmdComputeSpectrum", "PvAmdCopySpectrum",
               "PvAmdCopySpectrumBlock", "PvAmdGetSpectrum", "PvAmdHostSpectrumTables", "PvAmdHostSpectrum"]


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
    assert re.search(r"^#define\s+PVA_SPECTRUM_MAX_BINS\s+32\b", hdr, re.M) and pvlib.SPECTRUM_MAX_BINS == 32
    assert b"0.4.1" in pvlib.lib().PvAmdVersion()
