"""CPU: PvAmdHostBandCoefs / PvAmdHostBandMetrics -- the band filters and the per-band record of include/planeverb_amd.h
(PvAmdBandMetrics) -- against the numpy restatement of tests/_bands_ref.py, bit for bit (tolerance 0), against a double-precision
design written here, and against a response whose per-band decay times are known.  No device compute."""
import cmath
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _bands_ref as ref

QNAN_BITS = 0x7fc00000


def check(pvlib, p, fs, onset, coefs):
    got = pvlib.host_band_metrics(p, fs, onset, coefs)
    want = ref.band_metrics_ir(p, fs, onset, coefs)
    assert got.dtype == np.float32 and got.shape == (len(coefs), 12)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    assert (got[:, :3].view(np.uint32)[np.isnan(got[:, :3])] == QNAN_BITS).all(), got
    return got


def decaying_noise(rng, T, fs, rt, onset=0):
    """seeded noise under an exponential envelope that loses 60 dB in rt seconds, from step `onset` on"""
    env = 10.0 ** (-3.0 * np.maximum(np.arange(T) - onset, 0) / (rt * fs))
    return (rng.standard_normal(T) * env * 10.0 ** rng.uniform(-4, 1)).astype(np.float32)


CENTRES = {1443: (31.5, 63.0, 125.0, 250.0, 40.0, 80.0, 160.0, 200.0), 1968: (31.5, 63.0, 125.0, 250.0, 500.0, 50.0, 100.0, 400.0),
           5249: (31.5, 63.0, 125.0, 250.0, 500.0, 1000.0, 800.0, 1250.0)}  # (every upper octave edge below fs / 2)


def test_random_impulse_responses(pvlib):
    """120 responses in 24 groups of five; a group shares T, fs and its bands, so that the restatement, sequential in t, runs once
    per group with the five responses side by side.  The library is called once per response."""
    rng = np.random.default_rng(20261018)
    seen = np.zeros(3, int)
    total = 0
    for i in range(24):
        T = int(rng.integers(20, 1501)) if i else 1500
        fs = int(rng.choice([1443, 1968, 5249]))
        t_end = T - ref.tail_n(fs)
        onsets = [int(rng.integers(0, T)) for _ in range(5)]
        onsets[i % 5] = (max(t_end - 1, 0), min(max(t_end, 0), T - 1), T - 1)[i % 3]
        n = 1 + i % 8
        fraction = (1, 3)[(i // 8) % 2] if i < 16 else int(rng.choice([1, 3]))
        hz = rng.permutation(CENTRES[fs])[:n]
        coefs = pvlib.host_band_coefs(fs, hz, fraction)
        ps = np.stack([decaying_noise(rng, T, fs, float(rng.uniform(0.02, 0.5)), o if rng.random() < 0.5 else 0) for o in onsets], axis=1)
        want = ref.band_metrics(ps, np.array(onsets, np.float32), fs, coefs)
        for c, o in enumerate(onsets):
            got = pvlib.host_band_metrics(ps[:, c], fs, o, coefs)
            assert got.dtype == np.float32 and got.shape == (n, 12)
            assert same_bits(got, want[c]).all(), (T, fs, o, hz, fraction, got, want[c])
            assert (got[:, :3].view(np.uint32)[np.isnan(got[:, :3])] == QNAN_BITS).all(), got
            seen += (~np.isnan(got[:, :3])).sum(axis=0)
            total += n
    assert (seen > 10).all() and (seen < total - 10).all(), (seen, total)  # (the complete and the incomplete branch of every range)


def test_onsets_and_empty_band(pvlib):
    """onset 0, mid-record, tEnd - 1, tEnd and T - 1; an all-zero response gives e0 = 0 and what IEEE then gives"""
    fs, T = 1443, 435
    rng = np.random.default_rng(fs)
    t_end = T - ref.tail_n(fs)
    coefs = pvlib.host_band_coefs(fs, [63.0, 250.0], 1)
    p = decaying_noise(rng, T, fs, 0.04)
    p[200:] += decaying_noise(rng, T, fs, 0.03, 200)[200:]
    for onset in (0, 200, t_end - 1, t_end, T - 1):
        m = check(pvlib, p, fs, onset, coefs)
        assert np.isfinite(m[:, 6]).all() and (m[:, 6] > 0).all()
        if onset >= t_end:
            assert np.isnan(m[:, :3]).all() and (m[:, 3:6] == 0).all() and np.isnan(m[:, 7]).all()
        else:
            assert np.isfinite(m[:, 7]).all() and (m[:, 7] <= 0).all() and (m[:, 3] >= 1).all()
    m = check(pvlib, np.zeros(T, np.float32), fs, 10, coefs)
    assert (m[:, 6] == 0).all() and np.isnan(m[:, :3]).all() and np.isnan(m[:, 7:]).all() and (m[:, 3:6] == 0).all()


# ---- the design ------------------------------------------------------------------------------------------------------

def design64(fs, fc, fraction):
    """the header's design in python floats (double): ten coefficients, f1, f2"""
    h = 1.0 / (2 * fraction)
    f1, f2 = fc * 2.0 ** -h, fc * 2.0 ** h
    W1, W2 = math.tan(math.pi * f1 / fs), math.tan(math.pi * f2 / fs)
    bw, w0sq = W2 - W1, W1 * W2
    p = cmath.exp(1j * 3 * math.pi / 4)
    root = cmath.sqrt((p * bw) ** 2 - 4 * w0sq)
    zs = sorted(((1 + s) / (1 - s) for s in ((p * bw + root) / 2, (p * bw - root) / 2)), key=lambda z: abs(cmath.phase(z)))
    zi = cmath.exp(-2j * math.atan(math.sqrt(w0sq)))
    out = []
    for z in zs:
        a1, a2 = -2 * z.real, abs(z) ** 2
        g = abs((1 + a1 * zi + a2 * zi * zi) / (1 - zi * zi))
        out += [g, 0.0, -g, a1, a2]
    return np.array(out), f1, f2


def response_db(c, f, fs):
    """magnitude of the two sections in series at f, evaluated in double"""
    zi = cmath.exp(-2j * math.pi * f / fs)
    H = 1.0
    for s in range(2):
        b0, b1, b2, a1, a2 = (float(v) for v in c[5 * s:5 * s + 5])
        H *= (b0 + b1 * zi + b2 * zi * zi) / (1 + a1 * zi + a2 * zi * zi)
    return 20 * math.log10(abs(H))


DESIGNS = [(fs, fr, fc) for fs in (1443, 1968, 5249) for fr in (1, 3) for fc in (31.5, 63.0, 125.0, 250.0, 500.0, 1000.0)
           if fc * 2.0 ** (1 / (2 * fr)) < fs / 2]


def test_coefficients_against_a_double_design(pvlib):
    """every float32 coefficient within 1e-6 relative of the double design (float32 rounding is 6e-8: 16 x), the sections in
    pole-angle order, and the float32 coefficients' response, evaluated in double: 0 dB at sqrt(f1 f2), -3.01 dB at both edges.

    Tolerance of the response: what the double design itself misses the target by at that point plus MARGIN = 0.01 dB for the
    float32 rounding.  The double design misses the edges and the pre-warped centre by less than 1e-9 dB (asserted), so there the
    tolerance IS the margin; sqrt(f1 f2) in Hz is not the pre-warped centre, and the design's own value there is taken as it is
    (below 0.05 dB down while f2 < fs / 8, 0.19 dB down for the 500 Hz octave at fs = 1443).  The margin's reasoning, for the narrowest band tested (third octave, 31.5 Hz, fs = 5249): pole radius
    1 - 0.0031, pole angle 0.0377, so at the centre |1 + a1 z^-1 + a2 z^-2| = |z - p| |z - p*| is about 0.0031 x 0.075 =
    2.3e-4; a1 (near -2) and a2 (near 1) move by at most 6e-8 + 3e-8 = 9e-8 when rounded, 4e-4 of that magnitude = 0.0035 dB
    per section, 0.007 dB for both; b0 / b2 add 1e-6 dB.  0.01 dB covers that; it is five times tighter than the 0.05 dB a design
    without pre-warping misses an edge by."""
    MARGIN = 0.01
    assert (5249, 3, 31.5) in DESIGNS
    for fs, fr, fc in DESIGNS:
        c64, f1, f2 = design64(fs, fc, fr)
        c32 = pvlib.host_band_coefs(fs, [fc], fr)[0]
        assert c32.dtype == np.float32 and c32.shape == (10,)
        assert c32[1] == 0 and c32[6] == 0 and c32[2] == -c32[0] and c32[7] == -c32[5]
        nz = c64 != 0
        assert (np.abs(c32[nz].astype(np.float64) - c64[nz]) <= 1e-6 * np.abs(c64[nz])).all(), (fs, fr, fc, c32, c64)
        ang = [math.acos(max(-1.0, min(1.0, -float(c32[5 * s + 3]) / (2 * math.sqrt(float(c32[5 * s + 4])))))) for s in range(2)]
        assert ang[0] < ang[1], (fs, fr, fc, ang)
        f0w = fs / math.pi * math.atan(math.sqrt(math.tan(math.pi * f1 / fs) * math.tan(math.pi * f2 / fs)))
        for f, target, exact in ((math.sqrt(f1 * f2), 0.0, False), (f0w, 0.0, True), (f1, -10 * math.log10(2.0), True),
                                 (f2, -10 * math.log10(2.0), True)):
            d64 = response_db(c64, f, fs)
            own = abs(d64 - target)
            if exact:  # (the design meets these three by construction)
                assert own < 1e-9, (fs, fr, fc, f, own)
            else:  # (sqrt(f1 f2) in Hz lies beside the pre-warped centre: up to 0.2 dB down for an octave next to fs / 2)
                assert d64 <= 1e-9 and own < 0.25 and (own < 0.05 or f2 > fs / 8), (fs, fr, fc, f, d64)
            got = response_db(c32, f, fs)
            assert abs(got - d64) <= MARGIN, (fs, fr, fc, f, got, d64)
            assert abs(got - target) <= own + MARGIN
    # several bands at once: the same sets, in the order given
    many = pvlib.host_band_coefs(1443, [250.0, 63.0, 125.0], 3)
    for j, fc in enumerate((250.0, 63.0, 125.0)):
        assert np.array_equal(many[j], pvlib.host_band_coefs(1443, [fc], 3)[0])


def test_a_design_without_prewarp_would_fail():
    """the check above has teeth: edges taken as pi f / fs instead of tan(pi f / fs) miss the upper -3.01 dB point of the 250 Hz
    octave at fs = 1443 by more than 0.05 dB"""
    fs, fc = 1443, 250.0
    _, f1, f2 = design64(fs, fc, 1)
    real_tan = math.tan
    try:
        math.tan = lambda x: x
        wrong, _, _ = design64(fs, fc, 1)
    finally:
        math.tan = real_tan
    assert abs(response_db(wrong, f2, fs) + 10 * math.log10(2.0)) > 0.05


# ---- known answers ---------------------------------------------------------------------------------------------------

def two_tones(fs, T, a63):
    t = np.arange(T)
    return (a63 * np.sin(2 * np.pi * 63.0 * t / fs) * 10.0 ** (-3.0 * t / (0.5 * fs)) +
            np.sin(2 * np.pi * 250.0 * t / fs) * 10.0 ** (-3.0 * t / (0.15 * fs)))


def prototype64(p, c, fs):
    """the definition in float64 (filter backwards from rest, backward integral, the three ranges, least squares): edt, t20, t30"""
    T = len(p)
    y = np.zeros(T)
    z = [0.0] * 4
    for t in range(T - 1, -1, -1):
        x = p[t]
        for s in range(2):
            b0, b1, b2, a1, a2 = c[5 * s:5 * s + 5]
            ys = b0 * x + z[2 * s]
            z[2 * s] = b1 * x - a1 * ys + z[2 * s + 1]
            z[2 * s + 1] = b2 * x - a2 * ys
            x = ys
        y[t] = x
    E = np.cumsum((y * y)[::-1])[::-1]
    r = E / E[0]
    L = 10 * np.log10(r)
    k = np.arange(T)
    out = []
    for hi, lo in ((1.0, 0.1), (10 ** -0.5, 10 ** -2.5), (10 ** -0.5, 10 ** -3.5)):
        m = (r <= hi) & (r >= lo) & (k < T - int(0.01 * fs))
        out.append(-60.0 / np.polyfit(k[m], L[m], 1)[0] / fs)
    return out


IDENTITY = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0])  # (no filter: the broadband curve)


def test_known_decay_times_per_band(pvlib):
    """a 63 Hz tone losing 60 dB in 0.5 s plus a 250 Hz tone losing 60 dB in 0.15 s, fs = 1443, T = 1500, onset 0: the 63 Hz and
    250 Hz octave bands report their own EDT and T20, the broadband T30 follows the slow tone.

    Bound per value: ten times the relative error of the float64 prototype above, capped at 2 %.  The prototype's figures, with
    the 63 Hz tone at 0.46 of the 250 Hz tone's amplitude:
        63 Hz band   EDT 3e-4, T20 4e-4          250 Hz band   EDT 0.6 %, T20 1.8 %          broadband T30 1.7 %
    The amplitude ratio is the one free choice, and the definition leaves little room for it: the 250 Hz octave filter passes
    63 Hz at -27.2 dB, and the slow tone's leak ends up holding the 250 Hz band's curve -- with EQUAL amplitudes the float64
    prototype's 250 Hz T20 is 8.9 % long (T30 36 %), a property of a 4th-order band-pass and not of the arithmetic.  Making the
    slow tone weaker pushes its leak below the T20 range, but also pushes the broadband knee, above which the fast tone rules,
    into the broadband T30 range (at 0.3 the broadband T30 is 5 % short).  0.46 is where both prototype errors are below the 2 %
    cap; the float32 library agrees with the prototype to 1e-5."""
    fs, T = 1443, 1500
    p = two_tones(fs, T, 0.46)
    p32 = p.astype(np.float32)
    coefs = pvlib.host_band_coefs(fs, [63.0, 250.0], 1)
    m = check(pvlib, p32, fs, 0, coefs)
    bb = pvlib.host_decay_times(p32, fs, 0)
    cases = []
    for j, (fc, rt) in enumerate(((63.0, 0.5), (250.0, 0.15))):
        proto = prototype64(p, design64(fs, fc, 1)[0], fs)
        cases += [("%g Hz edt" % fc, m[j, 0], proto[0], rt), ("%g Hz t20" % fc, m[j, 1], proto[1], rt)]
    cases.append(("broadband t30", bb[2], prototype64(p, IDENTITY, fs)[2], 0.5))
    for name, got, proto, rt in cases:
        perr = abs(proto / rt - 1.0)
        bound = min(10.0 * perr, 0.02)
        print("%-14s got %.6f prototype %.6f (error %.2e) bound %.2e" % (name, got, proto, perr, bound))
    for name, got, proto, rt in cases:
        assert abs(float(got) / rt - 1.0) <= min(10.0 * abs(proto / rt - 1.0), 0.02), (name, got, proto)
    # the band tells the two decays apart where the broadband record cannot
    assert m[1, 1] < 0.4 * m[0, 1] and bb[2] > 3 * m[1, 1]


# ---- refusals --------------------------------------------------------------------------------------------------------

def test_band_refusals(pvlib):
    L = pvlib.lib()
    fp = C.POINTER(C.c_float)
    out = np.zeros(90, np.float32)
    o = out.ctypes.data_as(fp)

    def coefs(hz, n, fraction, fs=1443, outp=o):
        h = np.asarray(hz, np.float32)
        return L.PvAmdHostBandCoefs(fs, h.ctypes.data_as(fp) if h.size else None, n, fraction, outp)

    assert coefs([63.0], 1, 1) == 0
    assert coefs([63.0] * 8, 8, 3) == 0
    for args, why in ((([], 1, 1), "null"), (([63.0], 0, 1), "0 .. 8 bands"), (([63.0] * 9, 9, 1), "0 .. 8 bands"),
                      (([63.0], -1, 1), "0 .. 8 bands"), (([63.0], 1, 2), "fraction"), (([63.0], 1, 0), "fraction"),
                      (([np.nan], 1, 1), "not finite"), (([np.inf], 1, 1), "not finite"), (([0.0], 1, 1), "lower edge"),
                      (([-63.0], 1, 1), "lower edge"), (([63.0, 600.0], 2, 1), "upper edge"),
                      (([511.0], 1, 1), "upper edge")):
        before = out.copy()
        assert coefs(*args) == -1, args
        assert pvlib.last_error().startswith("band metrics: ") and why in pvlib.last_error(), (args, pvlib.last_error())
        assert np.array_equal(out, before)
    assert coefs([63.0], 1, 1, outp=None) == -1
    assert coefs([509.0], 1, 1) == 0  # (f2 = 719.8 < 721.5 = fs / 2; 511 Hz above gives 722.7)
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_band_coefs(1443, [63.0], 5)

    p = np.ones(8, np.float32)
    pp = p.ctypes.data_as(fp)
    c = pvlib.host_band_coefs(1443, [63.0], 1)
    cp = c.ctypes.data_as(fp)
    assert L.PvAmdHostBandMetrics(pp, 8, 1443, 7, cp, 1, o) == 0
    for call in (lambda: L.PvAmdHostBandMetrics(None, 8, 1443, 0, cp, 1, o), lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, 0, None, 1, o),
                 lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, 0, cp, 1, None), lambda: L.PvAmdHostBandMetrics(pp, 0, 1443, 0, cp, 1, o),
                 lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, -1, cp, 1, o), lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, 8, cp, 1, o),
                 lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, 0, cp, 0, o), lambda: L.PvAmdHostBandMetrics(pp, 8, 1443, 0, cp, 9, o),
                 lambda: L.PvAmdHostBandMetrics(pp, 8, 0, 0, cp, 1, o)):
        assert call() == -1
        assert pvlib.last_error().startswith("band metrics: "), pvlib.last_error()
    # the solver calls refuse a null handle
    fr = C.c_int(0)
    for call in (lambda: L.PvAmdSetBands(None, cp, 1, 1), lambda: L.PvAmdGetBands(None, o, 8, C.byref(fr)),
                 lambda: L.PvAmdGetBandCoefs(None, o), lambda: L.PvAmdComputeBandMetrics(None, None),
                 lambda: L.PvAmdCopyBandMetrics(None, o), lambda: L.PvAmdCopyBandMetricsBlock(None, 0, 0, 1, 1, o),
                 lambda: L.PvAmdGetBandMetrics(None, 0.0, 0.0, 0.0, o)):
        assert call() == -1
        assert pvlib.last_error().startswith("band metrics: "), pvlib.last_error()


NEW_EXPORTS = ["PvAmdSetBands", "PvAmdGetBands", "PvAmdGetBandCoefs", "PvAmdComputeBandMetrics", "PvAmdCopyBandMetrics",
               "PvAmdCopyBandMetricsBlock", "PvAmdGetBandMetrics", "PvAmdHostBandCoefs", "PvAmdHostBandMetrics"]


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
    assert pvlib.BAND_METRIC_NAMES == ref.NAMES
    assert pvlib.BANDS_MAX == 8 and "#define PVA_BANDS_MAX 8" in hdr
