"""CPU: PvAmdHostModulation / PvAmdHostModulationTable / PvAmdCombineMti -- the modulation transfer function and index of
include/planeverb_amd.h (PvAmdModulation) -- against the numpy restatement of tests/_modulation_ref.py, bit for bit (tolerance 0),
and against a response whose modulation transfer function is known.  No device compute."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _modulation_ref as ref
from test_host_bands import CENTRES, decaying_noise

QNAN_BITS = 0x7fc00000


def check(pvlib, p, fs, onset, coefs, hz=None):
    got = pvlib.host_modulation(p, fs, onset, coefs, hz)
    want = ref.modulation_ir(p, onset, coefs, pvlib.host_modulation_table(len(p), fs, hz))
    assert got.dtype == np.float32 and got.shape == (len(coefs), 15)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    return got


def test_random_impulse_responses(pvlib):
    """64 responses in 16 groups of four; a group shares T, fs, its bands and its modulation frequencies, so that the restatement,
    sequential in t, runs once per group with the four responses side by side.  The library is called once per response."""
    rng = np.random.default_rng(20261019)
    for i in range(16):
        T = int(rng.integers(20, 901)) if i else 900
        fs = int(rng.choice([1443, 1968, 5249]))
        onsets = [int(rng.integers(0, T)) for _ in range(4)]
        onsets[i % 4] = (0, T - 1, T - 3, T // 2)[i % 4]
        n = 1 + i % 8
        hz = rng.permutation(CENTRES[fs])[:n]
        coefs = pvlib.host_band_coefs(fs, hz, (1, 3)[i % 2])
        mod_hz = None if i % 3 == 0 else np.sort(rng.uniform(0.0, (20.0, fs / 2)[i % 3 - 1], 14)).astype(np.float32)
        tab = pvlib.host_modulation_table(T, fs, mod_hz)
        ps = np.stack([decaying_noise(rng, T, fs, float(rng.uniform(0.02, 0.5)), o if rng.random() < 0.5 else 0) for o in onsets], axis=1)
        want = ref.modulation(ps, np.array(onsets, np.float32), coefs, tab)
        for c, o in enumerate(onsets):
            got = pvlib.host_modulation(ps[:, c], fs, o, coefs, mod_hz)
            assert got.dtype == np.float32 and got.shape == (n, 15)
            assert same_bits(got, want[c]).all(), (T, fs, o, hz, got, want[c])
            assert np.isfinite(got).all() and (got >= 0).all() and (got[:, 14] <= 1).all(), got


def test_late_onset_and_silent_band(pvlib):
    """an onset that leaves three samples; a response without energy gives E == 0 and 15 quiet NaNs per band; a band that
    underflows (a 1e-8 Hz third octave: the first samples of its output square to +0) does the same, beside a band that does not"""
    fs, T = 1443, 435
    rng = np.random.default_rng(fs)
    coefs = pvlib.host_band_coefs(fs, [63.0, 250.0], 1)
    p = decaying_noise(rng, T, fs, 0.5)  # (36 dB down at T - 3: far above the underflow of e)
    for onset in (T - 3, T - 1, 0):
        m = check(pvlib, p, fs, onset, coefs)
        assert np.isfinite(m).all()
    m = check(pvlib, np.zeros(T, np.float32), fs, 10, coefs)
    assert (m.view(np.uint32) == QNAN_BITS).all()
    faint = pvlib.host_band_coefs(fs, [1e-8, 63.0], 3)
    m = check(pvlib, p, fs, T - 3, faint)
    assert (m[0].view(np.uint32) == QNAN_BITS).all() and np.isfinite(m[1]).all()


def test_zero_modulation_frequency_gives_one(pvlib):
    """F = 0: cos = 1 and sin = 0 at every step, so re = E bit for bit and im = +0; a = E / E = 1, b = 0, m = 1.0f exactly, ti = 1"""
    fs, T = 1443, 435
    rng = np.random.default_rng(7)
    coefs = pvlib.host_band_coefs(fs, [63.0, 125.0, 250.0], 1)
    hz = np.array(ref.DEFAULT_HZ, np.float32)
    hz[[0, 5, 13]] = 0.0
    for seed in range(4):
        p = decaying_noise(rng, T, fs, 0.1)
        m = check(pvlib, p, fs, 17 * seed, coefs, hz)
        assert (m[:, [0, 5, 13]].view(np.uint32) == np.float32(1).view(np.uint32)).all(), m
        assert (m[:, :14] <= 1).all() and (m[:, 14] > 3 / 14).all()
        m = check(pvlib, p, fs, 17 * seed, coefs, np.zeros(14, np.float32))
        assert (m.view(np.uint32) == np.float32(1).view(np.uint32)).all(), m  # (every ti is 1, and 14 / 14 = 1)
    assert ref.transfer_index(np.float32([1.0, 2.0, 0.0, 0.5]))[:3].tolist() == [1.0, 1.0, 0.0]
    assert ref.transfer_index(np.float32([0.5]))[0] == np.float32(0.5)


def test_table_against_double(pvlib):
    """every entry is the float32 rounding of cos / sin of the header's phase, evaluated in double by the same libm"""
    for T, fs, hz in ((435, 1443, None), (97, 5249, np.linspace(0.0, 5249 / 2, 14).astype(np.float32))):
        tab = pvlib.host_modulation_table(T, fs, hz)
        assert tab.shape == (T, 14, 2) and tab.dtype == np.float32
        assert np.array_equal(tab.view(np.uint32), ref.table64(T, fs, hz).view(np.uint32))
        assert (tab[0, :, 0] == 1).all() and (tab[0, :, 1] == 0).all()
    # the default is the IEC series
    assert np.array_equal(pvlib.host_modulation_table(50, 1443), pvlib.host_modulation_table(50, 1443, ref.DEFAULT_HZ))
    assert tuple(pvlib.MODULATION_DEFAULT_HZ) == ref.DEFAULT_HZ and pvlib.MODULATION_FREQS == ref.M


def test_refusals(pvlib):
    L = pvlib.lib()
    fp = C.POINTER(C.c_float)
    fs = 1443
    out = np.zeros(15 * 8, np.float32)
    o = out.ctypes.data_as(fp)
    tab = np.zeros(8 * 28, np.float32)
    tp = tab.ctypes.data_as(fp)
    p = np.ones(8, np.float32)
    pp = p.ctypes.data_as(fp)
    c = pvlib.host_band_coefs(fs, [63.0], 1)
    cp = c.ctypes.data_as(fp)

    def freqs(**kw):
        h = np.array(ref.DEFAULT_HZ, np.float32)
        for k, v in kw.items():
            h[int(k[1:])] = v
        return h

    ok = freqs(i0=0.0, i13=fs / 2)
    assert L.PvAmdHostModulationTable(8, fs, ok.ctypes.data_as(fp), tp) == 0
    assert L.PvAmdHostModulation(pp, 8, fs, 7, cp, 1, ok.ctypes.data_as(fp), o) == 0
    assert L.PvAmdHostModulation(pp, 8, fs, 0, cp, 1, None, o) == 0
    # the rule of the setter (pv_modulation.h modulationFreqsError), through the host calls that share it
    for bad, why in ((freqs(i3=np.nan), "not finite"), (freqs(i0=np.inf), "not finite"), (freqs(i13=-np.inf), "not finite"),
                     (freqs(i7=-0.5), "negative"), (freqs(i13=fs / 2 + 0.25), "above fs / 2")):
        before, tbefore = out.copy(), tab.copy()
        assert L.PvAmdHostModulationTable(8, fs, bad.ctypes.data_as(fp), tp) == -1
        assert pvlib.last_error().startswith("modulation: ") and why in pvlib.last_error(), pvlib.last_error()
        assert L.PvAmdHostModulation(pp, 8, fs, 0, cp, 1, bad.ctypes.data_as(fp), o) == -1
        assert pvlib.last_error().startswith("modulation: ") and why in pvlib.last_error(), pvlib.last_error()
        assert np.array_equal(out, before) and np.array_equal(tab, tbefore)
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: "):
            pvlib.host_modulation(p, fs, 0, c, bad)
    with pytest.raises(ValueError):
        pvlib.host_modulation(p, fs, 0, c, [1.0, 2.0])
    for call in (lambda: L.PvAmdHostModulation(None, 8, fs, 0, cp, 1, None, o), lambda: L.PvAmdHostModulation(pp, 8, fs, 0, None, 1, None, o),
                 lambda: L.PvAmdHostModulation(pp, 8, fs, 0, cp, 1, None, None), lambda: L.PvAmdHostModulation(pp, 0, fs, 0, cp, 1, None, o),
                 lambda: L.PvAmdHostModulation(pp, 8, fs, -1, cp, 1, None, o), lambda: L.PvAmdHostModulation(pp, 8, fs, 8, cp, 1, None, o),
                 lambda: L.PvAmdHostModulation(pp, 8, fs, 0, cp, 0, None, o), lambda: L.PvAmdHostModulation(pp, 8, fs, 0, cp, 9, None, o),
                 lambda: L.PvAmdHostModulation(pp, 8, 0, 0, cp, 1, None, o), lambda: L.PvAmdHostModulationTable(0, fs, None, tp),
                 lambda: L.PvAmdHostModulationTable(8, 0, None, tp), lambda: L.PvAmdHostModulationTable(8, fs, None, None),
                 lambda: L.PvAmdCombineMti(None, cp, cp, 2, o), lambda: L.PvAmdCombineMti(cp, None, cp, 2, o),
                 lambda: L.PvAmdCombineMti(cp, cp, None, 2, o), lambda: L.PvAmdCombineMti(cp, cp, cp, 2, None),
                 lambda: L.PvAmdCombineMti(cp, cp, cp, 0, o), lambda: L.PvAmdCombineMti(cp, cp, cp, 9, o)):
        assert call() == -1
        assert pvlib.last_error().startswith("modulation: "), pvlib.last_error()
    # the solver calls refuse a null handle
    for call in (lambda: L.PvAmdSetModulationFrequencies(None, ok.ctypes.data_as(fp)), lambda: L.PvAmdSetModulationFrequencies(None, None),
                 lambda: L.PvAmdGetModulationFrequencies(None, o), lambda: L.PvAmdComputeModulation(None, None),
                 lambda: L.PvAmdCopyModulation(None, o), lambda: L.PvAmdCopyModulationBlock(None, 0, 0, 1, 1, o),
                 lambda: L.PvAmdGetModulation(None, 0.0, 0.0, 0.0, o)):
        assert call() == -1
        assert pvlib.last_error().startswith("modulation: "), pvlib.last_error()


def test_combine_mti_against_a_hand_computation(pvlib):
    """three bands with the male-speech weights of IEC 60268-16 for 125, 250 and 500 Hz (alpha 0.085, 0.127, 0.230; beta 0.085,
    0.078), every product and sum written out in float32"""
    f = np.float32
    mti = [f(0.5), f(0.72), f(0.33)]
    alpha = [f(0.085), f(0.127), f(0.230)]
    beta = [f(0.085), f(0.078)]
    s = f(f(f(f(0) + f(alpha[0] * mti[0])) + f(alpha[1] * mti[1])) + f(alpha[2] * mti[2]))
    r = f(f(f(0) + f(beta[0] * np.sqrt(f(mti[0] * mti[1])))) + f(beta[1] * np.sqrt(f(mti[1] * mti[2]))))
    want = f(s - r)
    got = pvlib.combine_mti(mti, alpha, beta)
    assert isinstance(got, np.float32) and got.view(np.uint32) == want.view(np.uint32), (got, want)
    assert abs(float(got) - (0.0425 + 0.09144 + 0.0759 - 0.085 * 0.6 - 0.078 * math.sqrt(0.2376))) < 1e-6
    assert got == ref.combine_mti(mti, alpha, beta)
    # one band, and the clamp on both sides
    assert pvlib.combine_mti([0.4], [0.5]) == f(f(0.5) * f(0.4))
    assert pvlib.combine_mti([0.9, 0.9], [1.0, 1.0], [0.0]) == 1.0
    assert pvlib.combine_mti([0.5, 0.5], [0.1, 0.1], [1.0]) == 0.0
    assert np.isnan(pvlib.combine_mti([np.nan, 0.5], [0.5, 0.5], [0.1]))
    rng = np.random.default_rng(5)
    for n in range(1, 9):
        m, a, b = rng.uniform(0, 1, n), rng.uniform(0, 2.0 / n, n), rng.uniform(0, 0.1, n - 1)
        assert pvlib.combine_mti(m, a, b) == ref.combine_mti(m, a, b)
    with pytest.raises(ValueError):
        pvlib.combine_mti([0.5, 0.5], [0.5], [0.1])


NEW_EXPORTS = ["PvAmdSetModulationFrequencies", "PvAmdGetModulationFrequencies", "PvAmdComputeModulation", "PvAmdCopyModulation",
               "PvAmdCopyModulationBlock", "PvAmdGetModulation", "PvAmdHostModulation", "PvAmdHostModulationTable", "PvAmdCombineMti"]


def test_exports_present_and_guarded(pvlib, tmp_path):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the exception-guard macro of pv_capi.cpp; the record is a struct of fifteen floats; the header does not call the index STI"""
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
    assert "#define PVA_MODULATION_FREQS 14" in hdr and re.search(r"typedef struct PvAmdModulation \{[^}]*\} PvAmdModulation;", hdr)
    assert not [n for n in re.findall(r"^PVA_EXPORT\s+[\w\s\*]*?\b(\w+)\s*\(", hdr, re.M) if "sti" in n.lower()]
    assert "seven octave" in hdr and "partial index" in hdr.lower()
    import subprocess
    csrc = tmp_path / "size.c"
    csrc.write_text('#include "planeverb_amd.h"\ntypedef char fifteen_floats[sizeof(PvAmdModulation) == 60 ? 1 : -1];\n'
                    'int main(void) { PvAmdModulation m; m.mti = 0; m.m[13] = 0; (void)m; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(csrc)])


# ---- a known answer --------------------------------------------------------------------------------------------------

SANITY_FS, SANITY_T, SANITY_RT, SANITY_HZ = 48000, 36000, 0.6, 8000.0
# the largest |m(F) - theory| of PvAmdHostModulation over the 20 seeds and the 14 default modulation frequencies, measured on the
# CPU, and the bound: 1.5 x that
SANITY_MEASURED = 0.052836
SANITY_BOUND = 1.5 * SANITY_MEASURED


def sanity_deviation(pvlib, seed):
    """Gaussian noise under an exponential envelope that loses 60 dB in RT seconds, through one wide band (the 8 kHz octave at
    fs = 48 kHz: 5.7 kHz of noise bandwidth): the envelope of p^2 is exp(-13.8 t / RT), whose normalised Fourier transform has the
    magnitude 1 / sqrt(1 + (2 pi F RT / 13.8)^2) (Schroeder 1981).  Returns |m - theory| per modulation frequency"""
    fs, T, rt = SANITY_FS, SANITY_T, SANITY_RT
    rng = np.random.default_rng(1000 + seed)
    p = (rng.standard_normal(T) * 10.0 ** (-3.0 * np.arange(T) / (rt * fs))).astype(np.float32)
    coefs = pvlib.host_band_coefs(fs, [SANITY_HZ], 1)
    m = pvlib.host_modulation(p, fs, 0, coefs)[0, :14].astype(np.float64)
    F = np.array(ref.DEFAULT_HZ)
    theory = 1.0 / np.sqrt(1.0 + (2.0 * np.pi * F * rt / 13.8) ** 2)
    return np.abs(m - theory), m, theory


def test_decaying_noise_follows_the_schroeder_formula(pvlib):
    worst = 0.0
    for seed in range(20):
        dev, m, theory = sanity_deviation(pvlib, seed)
        worst = max(worst, float(dev.max()))
        assert (np.diff(theory) < 0).all() and theory[0] > 0.98 and theory[-1] < 0.35
    print("largest deviation over 20 seeds: %.6f (bound %.6f)" % (worst, SANITY_BOUND))
    assert worst <= SANITY_BOUND, (worst, SANITY_BOUND)
