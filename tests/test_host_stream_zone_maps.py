"""CPU: the accumulate passes of PvAmdSetZoneMaps as the host restates them -- PvAmdHostRoomSumsAdvance, PvAmdHostRoomMetricsFromSums
and PvAmdHostSpectrumAdvance, built from the step functions the kernel of csrc/pv_zone_maps.hip applies -- chained over partitions of
the run into passes, against the one-walk definitions PvAmdHostRoomMetrics and PvAmdHostSpectrum on the families of
tests/_adversarial.py (NaN and +-inf included); the new exports and their guards; and the edge cases in a stand-alone program under
ASan + UBSan (nothing is loaded into Python under a sanitizer).  The spectrum's level plane is spectrumLevel of the chained sums:
that function has no export of its own, so the stand-alone program holds it to spectrumOfIr's level; here re and im are compared."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _adversarial as adv
from conftest import ROOT

NAMES = ["PvAmdSetZoneMaps", "PvAmdGetZoneMaps"]
HOST_NAMES = ["PvAmdHostRoomSumsAdvance", "PvAmdHostRoomMetricsFromSums", "PvAmdHostSpectrumAdvance"]
FS = 1443
N50, N80 = int(np.float32(0.05) * np.float32(FS)), int(np.float32(0.08) * np.float32(FS))
TILE = (12, 40)


def onsets_of(T):
    return [0, T // 2, T - 1, T - N50 + 3, T - 5]  # the last two: within n50 of T


def histories(T):
    """(p [T, 12, 40], family [12, 40], onset [12, 40]): every family of _adversarial at every onset of onsets_of(T)"""
    A, B = TILE
    rng = np.random.default_rng(T)
    ons = np.array(onsets_of(T))
    onset = ons[(np.arange(A)[:, None] * 3 + np.arange(B)[None, :]) % len(ons)]
    t = np.arange(T)[:, None, None]
    base = (rng.standard_normal((T, A, B)) * np.exp(-0.01 * np.maximum(t - onset, 0))).astype(np.float32)
    base[t < onset] = 0
    base[onset, np.arange(A)[:, None], np.arange(B)[None, :]] = 0.5  # (the first recorded sample: non-zero)
    p, fam = adv.generate(base, 11 + T, TILE, onset=onset.astype(np.float32), fs=FS)
    return p, fam, onset


def cases(T):
    """one cell per (family, onset) where the draw has one: (p [T], onset, label)"""
    p, fam, onset = histories(T)
    out = []
    for f in range(len(adv.FAMILIES)):
        for on in sorted(set(onsets_of(T))):
            c = np.argwhere((fam == f) & (onset == on))
            if len(c):
                x, y = c[0]
                out.append((np.ascontiguousarray(p[:, x, y]), int(on), "%s, onset %d, T %d" % (adv.FAMILIES[f], on, T)))
    assert len({c[2].split(",")[0] for c in out}) == len(adv.FAMILIES)  # every family, NaN / inf included
    assert any(not np.isfinite(c[0]).all() for c in out)
    return out


def partitions(T, onset):
    """the ways the run is cut into accumulate passes [tA, tB)"""
    def steps(n):
        return [(a, a + n) for a in range(0, T, n)]  # (the last pass reaches past T where n does not divide it)
    cuts = sorted({0, onset, min(onset + N50, T), min(onset + N80, T), T})
    return {"96": steps(96), "64, short last": [(a, min(a + 64, T)) for a in range(0, T, 64)], "1": steps(1), "one pass": [(0, T)],
            "at the onset and the window ends": list(zip(cuts[:-1], cuts[1:]))}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


@pytest.mark.parametrize("T", [435, 160])
def test_room_sums_chain_equals_one_walk(pvlib, T):
    for p, onset, ctx in cases(T):
        want = pvlib.host_room_metrics(p, FS, onset)
        for name, passes in partitions(T, onset).items():
            assert passes[0][0] == 0 and passes[-1][1] >= T and all(a[1] == b[0] for a, b in zip(passes, passes[1:]))
            sums = np.full(6, 123.5, np.float32)  # (never read: the pass that holds the onset starts from +0.0)
            for tA, tB in passes:
                sums = pvlib.host_room_sums_advance(p, FS, onset, tA, tB, sums)
            got = pvlib.host_room_metrics_from_sums(sums, FS)
            assert same_bits(got, want), (ctx, name, got, want)


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("T", [435, 160])
def test_spectrum_chain_equals_one_walk(pvlib, T, n):
    hz = [20.0 + 37.5 * j for j in range(n)]
    c, s = pvlib.host_spectrum_tables(T, FS, hz)
    pulse = np.random.default_rng(3).standard_normal(T).astype(np.float32)
    for p, onset, ctx in cases(T):
        want = pvlib.host_spectrum(p, FS, onset, hz, pulse)
        for name, passes in partitions(T, onset).items():
            reim = np.full((n, 2), 123.5, np.float32)
            for tA, tB in passes:
                reim = pvlib.host_spectrum_advance(p, onset, tA, tB, c, s, reim)
            assert same_bits(reim, want[:, :2]), (ctx, name, n)


def test_passes_that_hold_nothing(pvlib):
    p = np.arange(1, 161, dtype=np.float32)
    c, s = pvlib.host_spectrum_tables(160, FS, [50.0, 100.0])
    junk6, junk4 = np.full(6, 7.0, np.float32), np.full((2, 2), 7.0, np.float32)
    for onset, tA, tB in ((70, 0, 64), (70, 0, 70), (70, 64, 64), (70, 160, 224), (70, 200, 200)):
        assert same_bits(pvlib.host_room_sums_advance(p, FS, onset, tA, tB, junk6), junk6), (onset, tA, tB)
        assert same_bits(pvlib.host_spectrum_advance(p, onset, tA, tB, c, s, junk4), junk4), (onset, tA, tB)
    lib = pvlib.lib()
    out = pvlib.PvAmdRoomMetrics()
    f6 = (C.c_float * 6)()
    for bad in ((None, 160, FS, 0, 0, 1, f6), (f6, 0, FS, 0, 0, 1, f6), (f6, 6, FS, 6, 0, 1, f6), (f6, 6, FS, -1, 0, 1, f6),
                (f6, 6, FS, 0, 2, 1, f6), (f6, 6, FS, 0, -1, 1, f6), (f6, 6, FS, 0, 0, 1, None)):
        assert lib.PvAmdHostRoomSumsAdvance(*bad) == -1 and pvlib.last_error().startswith("zone maps: PvAmdHostRoomSumsAdvance"), bad
    assert lib.PvAmdHostRoomMetricsFromSums(None, FS, out) == -1 and pvlib.last_error().startswith("zone maps: PvAmdHostRoomMetricsFromSums")
    assert lib.PvAmdHostSpectrumAdvance(f6, 6, 0, 0, 1, f6, f6, 33, f6) == -1 and pvlib.last_error().startswith("zone maps: PvAmdHostSpectrumAdvance")
    assert lib.PvAmdHostSpectrumAdvance(f6, 6, 0, 0, 1, None, f6, 1, f6) == -1


def test_exports_exist_and_are_guarded(pvlib):
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    L = C.CDLL(pvlib.LIB_PATH)
    for n in NAMES + HOST_NAMES:
        assert re.search(r"^PVA_EXPORT int %s\(" % n, hdr, re.M), n
        assert hasattr(L, n) and n in pvlib.SYMBOLS, n
        m = re.search(r"^int %s\([^)]*\) try \{(.*?)^\} PV_API_CATCH\(-1\)$" % n, src, re.M | re.S)
        assert m, n
        assert "\n}" not in m.group(1), n  # (the guard that closes it is its own)
    for n in NAMES:
        assert re.search(r"^PVA_EXPORT int %s\(PvAmdSolver\* s[,)]" % n, hdr, re.M), n
    assert re.search(r"^#define PVA_ZMAP_ROOM_METRICS 1u$", hdr, re.M) and re.search(r"^#define PVA_ZMAP_SPECTRUM +2u$", hdr, re.M)
    assert (pvlib.ZMAP_ROOM_METRICS, pvlib.ZMAP_SPECTRUM) == (1, 2)
    for m in ("set_zone_maps", "zone_maps"):
        assert callable(getattr(pvlib.Solver, m)), m
    lib = pvlib.lib()
    k = C.c_uint(7)
    assert lib.PvAmdSetZoneMaps(None, 1) == -1 and pvlib.last_error() == "zone maps: null solver handle"
    assert lib.PvAmdGetZoneMaps(None, C.byref(k)) == -1 and pvlib.last_error() == "zone maps: null solver handle"
    assert k.value == 7


def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/stream_zone_maps_edges.cpp includes csrc/pv_metrics.h and csrc/pv_spectrum.h and runs the edge cases -- onset >= tB,
    tA >= T, the empty pass, n = 32 -- and the chains, levels included, with exactly sized arrays"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "stream_zone_maps_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", csrc, "-Wall",
                           "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "stream_zone_maps_edges.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "stream_zone_maps_edges: 0 failure(s)" in r.stdout, r.stdout
