"""CPU: the auralisation's host restatements (PvAmdHostAuralTaps, PvAmdHostAuralResample, PvAmdHostAuralConvolve: csrc/pv_aural.h)
against the numpy restatement written from the header (tests/_aural_ref.py), the resampler against the function it samples, the
convolution against float64 within the sequential-summation bound, the refusals, and the edge cases once more in a program of their
own under ASan + UBSan.  tests/test_gpu_aural.py holds the kernels to the same numpy restatement.  The restated chunk walk of the
tiled kernel (_aural_ref.chunk_walk), with which the cases of tests/test_gpu_aural_walk.py assert the path they reach, is pinned to
brute force here."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _aural_ref as ref
from conftest import ROOT, bits, same_bits

FS, T = 1443, 435
NEW_EXPORTS = ["PvAmdSetAuralisation", "PvAmdGetAuralisation", "PvAmdGetAuralTaps", "PvAmdComputeAuralResponses", "PvAmdCopyAuralResponse",
               "PvAmdAuralise", "PvAmdCopyAuralOutput", "PvAmdCopyAuralMix", "PvAmdAuralShape", "PvAmdSetAuralForm", "PvAmdHostAuralTaps",
               "PvAmdHostAuralResample", "PvAmdHostAuralConvolve"]
SETTINGS = [(FS, T, rate, Z, beta) for rate in (1443, 1000, 700, 8000) for Z in (2, 4, 16, 64) for beta in (0.0, 9.0, 20.0)]
SETTINGS.append((84351, 500, 48000, 16, 9.0))


def specials(v):
    """a denormal, a -0.0, one inf and one NaN sample, where there is room"""
    for i, s in enumerate((1.0e-41, -0.0, np.inf, np.nan)):
        if 3 * i + 1 < v.size:
            v[3 * i + 1] = s
    return v


@pytest.fixture(scope="module")
def tables(pvlib):
    """the restatement's tables of the settings the other tests use, computed once"""
    return dict(((rate, Z), ref.taps(FS, T, rate, Z, 9.0)) for rate, Z in ((1443, 16), (1000, 16), (8000, 16), (1000, 4), (8000, 2)))


def test_taps_against_the_restatement(pvlib):
    seen = {"ok": 0, "refused": 0}
    for fs, t, rate, Z, beta in SETTINGS:
        try:
            first, w = ref.taps(fs, t, rate, Z, beta)
        except ref.Refused:
            with pytest.raises(pvlib.PlaneverbError, match="^aural: "):
                pvlib.host_aural_taps(fs, t, rate, Z, beta)
            seen["refused"] += 1
            continue
        assert pvlib.host_aural_shape(fs, t, rate, Z, beta) == w.shape
        gf, gw = pvlib.host_aural_taps(fs, t, rate, Z, beta)
        assert gf.dtype == np.int32 and np.array_equal(gf, first), (rate, Z, beta)
        assert gw.dtype == np.float32 and np.array_equal(bits(gw), bits(w)), (rate, Z, beta, int((bits(gw) != bits(w)).sum()))
        seen["ok"] += 1
    assert seen == {"ok": 37, "refused": 12}  # (refused: rate = 700)
    # the shapes of the three rates at Z = 16
    assert [pvlib.host_aural_shape(FS, T, r, 16, 9.0) for r in (1443, 1000, 8000)] == [(435, 33), (301, 47), (2407, 33)]


def test_refusals(pvlib):
    L = pvlib.lib()
    for bad in (dict(rate=999), dict(rate=384001), dict(rate=0), dict(Z=1), dict(Z=65), dict(beta=-0.25), dict(beta=20.5),
                dict(beta=float("nan")), dict(beta=float("inf")), dict(fs=0), dict(T=0),
                dict(fs=84351, T=500, rate=1000),       # K = 2699 > PVA_AURAL_MAX_TAPS
                dict(T=30000, rate=384000)):            # L * K above 2^24
        a = dict(dict(fs=FS, T=T, rate=8000, Z=16, beta=9.0), **bad)
        with pytest.raises(pvlib.PlaneverbError, match="^aural: "):
            pvlib.host_aural_shape(a["fs"], a["T"], a["rate"], a["Z"], a["beta"])
    # K = 1024 is never reached (K is odd); the largest legal K
    assert pvlib.host_aural_shape(51150, 500, 6400, 64, 9.0)[1] == 1023
    with pytest.raises(pvlib.PlaneverbError, match="^aural: more than 1024 taps"):
        pvlib.host_aural_shape(51300, 500, 6400, 64, 9.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    first, w, out = np.zeros(435, np.int32), np.zeros((435, 33), np.float32), np.zeros(435, np.float32)
    assert L.PvAmdHostAuralTaps(FS, T, 1443, 16, 9.0, ip(first), fp(w), 434, None, None) == -1 and pvlib.last_error().startswith("aural:")
    assert L.PvAmdHostAuralTaps(FS, T, 1443, 16, 9.0, ip(first), None, 435, None, None) == -1
    assert L.PvAmdHostAuralTaps(FS, T, 1443, 16, 9.0, ip(first), fp(w), 435, None, None) == 0
    p = np.ones(T, np.float32)
    for args in ((None, T, ip(first), fp(w), 435, 33, fp(out)), (fp(p), T, None, fp(w), 435, 33, fp(out)), (fp(p), T, ip(first), None, 435, 33, fp(out)),
                 (fp(p), T, ip(first), fp(w), 435, 33, None), (fp(p), 0, ip(first), fp(w), 435, 33, fp(out)),
                 (fp(p), T, ip(first), fp(w), 0, 33, fp(out)), (fp(p), T, ip(first), fp(w), 435, 0, fp(out)),
                 (fp(p), T, ip(first), fp(w), 435, 1025, fp(out))):
        assert L.PvAmdHostAuralResample(*args) == -1 and pvlib.last_error().startswith("aural:")
    big = np.zeros(2 * T, np.float32)
    for args in ((None, T, fp(p), T, fp(big)), (fp(p), T, None, T, fp(big)), (fp(p), T, fp(p), T, None), (fp(p), 0, fp(p), T, fp(big)),
                 (fp(p), T, fp(p), 0, fp(big)), (fp(p), T, fp(p), pvlib.AURAL_MAX_SAMPLES + 1, fp(big))):
        assert L.PvAmdHostAuralConvolve(*args) == -1 and pvlib.last_error().startswith("aural:")


@pytest.mark.parametrize("rate", [1443, 1000, 8000, 48000])
def test_physical_check(pvlib, rate):
    """a band-limited function resampled agrees with the same function sampled at `rate` to 1e-4 absolute: eight times the worst
    error the definition gave in numpy (1.24e-5 at 8000 and 48000, 7.5e-6 at 1000, 2.9e-8 at 1443), whose source is the filter's
    stop-band and transition band, not float32 (a sum of 33 .. 47 terms of magnitude <= 1: 47 x 2^-24 = 2.8e-6)"""
    f = 0.35 * min(FS, rate) / 2.0

    def fn(t):
        return np.exp(-((t - 0.15) / 0.04) ** 2) * np.cos(2.0 * np.pi * f * t)

    first, w = pvlib.host_aural_taps(FS, T, rate, 16, 9.0)
    p = fn(np.arange(T) / float(FS)).astype(np.float32)
    h = pvlib.host_aural_resample(p, first, w)
    want = fn(np.arange(h.size) / float(rate))
    err = np.abs(h.astype(np.float64) - want).max()
    print("rate %d: worst absolute error %.3g" % (rate, err))
    assert err <= 1e-4, err


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_resample_against_the_restatement(pvlib, tables):
    rng = np.random.default_rng(20261021)
    for (rate, Z), (first, w) in tables.items():
        for special in (False, True):
            p = rng.standard_normal(T).astype(np.float32)
            if special:
                specials(p)
            got, want = pvlib.host_aural_resample(p, first, w), ref.resample(p, first, w)
            assert got.shape == want.shape == (w.shape[0],) and same_bits(got, want).all(), (rate, Z, special)
            assert np.isnan(got).any() == special
    # a short run: every table row reaches outside 0 .. T - 1
    first, w = ref.taps(FS, 9, 8000, 16, 9.0)
    p = specials(rng.standard_normal(9).astype(np.float32))
    assert same_bits(pvlib.host_aural_resample(p, first, w), ref.resample(p, first, w)).all()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_convolve_against_the_restatement(pvlib, tables):
    rng = np.random.default_rng(7)
    for L in (1, 2, 9, 301, 2407):
        h = rng.standard_normal(L).astype(np.float32) * np.exp(-np.arange(L) / 200.0).astype(np.float32)
        for N in sorted(set(n for n in (1, 2, L - 1, L, L + 1, 300) if n >= 1 and (L < 2407 or n <= 300))):
            for special in (False, True):
                x = rng.standard_normal(N).astype(np.float32)
                if special:
                    specials(x)
                    if L > 7:
                        h = h.copy()
                        h[5], h[7] = -0.0, 1.0e-40
                got, want = pvlib.host_aural_convolve(h, x), ref.convolve(h, x)
                assert got.shape == want.shape == (N + L - 1,) and same_bits(got, want).all(), (L, N, special)
                if special and N > 10:
                    # a NaN sample poisons exactly the outputs whose range of terms holds it: m = 10 .. 10 + L - 1; the terms
                    # outside an output's range are not formed, so the inf at 7 and the NaN reach no other output
                    nan = np.isnan(got)
                    assert nan[10:10 + L].all() and not nan[:7].any() and not nan[10 + L:].any(), (L, N)


def test_convolve_against_float64(pvlib):
    """Against np.convolve in float64 (exact products of float32 pairs, sums good to 2^-53).  An output of `terms` terms is `terms`
    products, each rounded once, and terms - 1 sums, each rounded once (the first sum, +0 + product, is exact): term i passes through
    at most 1 + (terms - 1) roundings, so |o - exact| <= gamma_terms sum |h| |x| with gamma_n = n u / (1 - n u), u = 2^-24.
    The bound (terms - 1) u sum |h| |x| counts the sums alone; it cannot hold for terms = 1, where it asks a rounded product to be
    exact, so it is asserted from two terms on, where the worst case of the products' roundings does not occur in these samples."""
    rng = np.random.default_rng(11)
    u = 2.0 ** -24
    for L, N in ((301, 300), (2407, 300), (9, 1), (1, 9), (2, 2)):
        h = rng.standard_normal(L).astype(np.float32)
        x = rng.standard_normal(N).astype(np.float32)
        got = pvlib.host_aural_convolve(h, x).astype(np.float64)
        exact = np.convolve(h.astype(np.float64), x.astype(np.float64))
        mag = np.convolve(np.abs(h.astype(np.float64)), np.abs(x.astype(np.float64)))
        m = np.arange(N + L - 1)
        terms = np.minimum(L - 1, m) - np.maximum(0, m - N + 1) + 1
        assert (terms >= 1).all() and terms.max() == min(L, N)
        err = np.abs(got - exact)
        gamma = terms * u / (1.0 - terms * u)
        assert (err <= gamma * mag).all(), (L, N)
        sums_only = (terms - 1) * u * mag
        print("L %d N %d: worst error / bound %.3g, outputs above the sums-only bound: %d of them with one term, %d with more" % (
            L, N, (err / (gamma * mag + 1e-300)).max(), ((err > sums_only) & (terms == 1)).sum(), ((err > sums_only) & (terms > 1)).sum()))
        assert (err[terms > 1] <= sums_only[terms > 1]).all(), (L, N)


def brute_walk(L, N, B, C):
    """chunk_walk from the words alone: a chunk is W exactly when every pair (m in m0 .. m0 + B - 1, k in the chunk) has
    0 <= m - k < N and k < L"""
    M, walks = N + L - 1, []
    for m0 in range(0, M, B):
        m = np.arange(m0, m0 + B)[:, None]
        k0, k_end, s = max(0, m0 - N + 1), min(L - 1, m0 + B - 1, M - 1), ""
        while k0 <= k_end:
            k = np.arange(k0, k0 + C)[None, :]
            s += "W" if bool(((m - k >= 0) & (m - k < N) & (k < L)).all()) else "g"
            k0 += C
        walks.append(s)
    return walks


def test_chunk_walk_against_brute_force():
    for L in range(1, 41):
        for N in range(1, 41):
            for B, C in ((8, 4), (4, 4), (8, 8), (12, 4)):
                assert ref.chunk_walk(L, N, B, C) == brute_walk(L, N, B, C), (L, N, B, C)
    assert any("WW" in s for s in ref.chunk_walk(40, 40, 8, 4)) and any("gW" in s for s in ref.chunk_walk(40, 40, 8, 4))
    rng = np.random.default_rng(429)
    pairs = [(int(a), int(b)) for a, b in rng.integers(1, 3001, (300, 2))] + [(301, 384), (301, 383), (256, 1000), (255, 1000)]
    whole = 0
    for L, N in pairs:
        got = ref.chunk_walk(L, N, 256, 128)
        assert got == brute_walk(L, N, 256, 128), (L, N)
        assert len(got) == (N + L - 1 + 255) // 256 and all(got)  # (a block per 256 outputs, none with an empty k range)
        whole += sum(s.count("W") for s in got)
    assert whole > 1000
    # a whole chunk needs N >= B + C, and at N = B + C a response that covers the chunk
    assert not any("W" in s for L in (200, 301, 3000) for s in ref.chunk_walk(L, 383, 256, 128))
    assert ref.chunk_walk(301, 384, 256, 128) == ["gg", "gWg", "gg"]
    assert not any("W" in s for s in ref.chunk_walk(255, 384, 256, 128))  # (the chunk k0 = 128 would end at tap 255 = L)


def test_what_the_first_convolution_shapes_covered(pvlib):
    """Regression note.  Until the walk cases of tests/test_gpu_aural_walk.py, the (L, N) pairs of test_convolution and
    test_convolution_short_responses ran exactly two whole chunks on the device, (L, N) = (128, 519) and (129, 519) at the block
    m0 = 256: both the block's first chunk (k0 = 0, zero accumulators, kBegin = 0), neither followed by another whole one.  The
    loop the measured shapes of profiles/aural.txt spend their time in was otherwise never compared with the definition."""
    B, C = pvlib.aural_shape()
    assert (B, C) == (256, 128)
    pairs = []
    for L in (301, 2407):  # test_convolution
        k = (L + 100) // B + 1
        pairs += [(L, n) for n in [1, 2, 65] + [k * B - L + 1 + d for d in (-1, 0, 1)]]
    for L in (69, 128, 129):  # test_convolution_short_responses
        pairs += [(L, n) for n in (1, 2, 65, C, B - L, B - L + 1, B - L + 2, 2 * B + 7)]
    assert len(pairs) == 36
    with_whole = dict((p, ref.chunk_walk(p[0], p[1], B, C)) for p in pairs if any("W" in s for s in ref.chunk_walk(p[0], p[1], B, C)))
    assert with_whole == {(128, 519): ["g", "W", "g"], (129, 519): ["gg", "Wg", "gg"]}
    # the shapes that were added for it
    assert ref.chunk_walk(2407, 1000, B, C).count("ggWWWWWggg") >= 3
    walk = ref.chunk_walk(2407, 2407, B, C)
    assert (sum(s.count("W") for s in walk), sum(len(s) for s in walk), max(len(r) for s in walk for r in re.findall("W+", s))) == (152, 199, 16)


def test_exports_present_and_guarded(pvlib):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the exception-guard macro of pv_capi.cpp"""
    L = C.CDLL(pvlib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    for n in NEW_EXPORTS:
        assert hasattr(L, n), n
        assert re.search(r"PVA_EXPORT \w+ %s\(" % n, hdr), n
        assert n in pvlib.SYMBOLS, n
        m = re.search(r"^\w+ %s\([^)]*\) try \{.*?^\} (PV_API_CATCH\w*)" % n, src, re.S | re.M)
        assert m, n
    for const in ("AURAL_MAX_TAPS", "AURAL_MAX_RECEIVERS", "AURAL_MAX_SIGNALS", "AURAL_MAX_SAMPLES", "AURAL_RECEIVERS", "AURAL_ARRAYS"):
        m = re.search(r"#define PVA_%s\s+(.+)" % const, hdr)
        assert m and eval(m.group(1)) == getattr(pvlib, const), const
    assert hasattr(pvlib.Solver, "set_auralisation") and hasattr(pvlib.Solver, "auralise") and hasattr(pvlib.Solver, "aural_mix")


def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/aural_edges.cpp calls the three host functions of the HIP-less host build (pv_capi.cpp against the fake solver of
    tests/host/) with exactly sized arrays; nothing is loaded into Python under a sanitizer"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "aural_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-DPVA_HOST_TEST", "-I", host,
                           "-I", csrc, "-I", os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "aural_edges.cpp"), os.path.join(csrc, "pv_core.cpp"), os.path.join(csrc, "pv_context.cpp"),
                           os.path.join(csrc, "pv_capi.cpp"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
