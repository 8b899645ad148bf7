"""CPU: the waterfall's host restatement (PvAmdHostWaterfall, csrc/pv_waterfall.h) against the numpy restatement written from the
header (tests/_waterfall_ref.py), the textbook sum, a synthetic mode, the setting's refusals, and the edge cases once more in a
program of their own under ASan + UBSan.  tests/test_gpu_waterfall.py holds the kernel to the same numpy restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _adversarial as adv
import _waterfall_ref as ref
from _room_metrics_ref import threshold_onset
from conftest import ROOT, golden, same_bits
from test_host_adversarial import FS as ADV_FS, T as ADV_T, block as adv_block, SEED as ADV_SEED, TILE as ADV_TILE


def bins_of(n, fs):
    return np.linspace(0.0, fs / 2.0, n).astype(np.float32) if n > 1 else np.array([61.7], np.float32)


def check_ir(pvlib, p, fs, onset, hz, seconds, m, pulse):
    """host_waterfall == the numpy restatement, bit for bit; returns the record's parts"""
    T, n = len(p), len(hz)
    got = pvlib.host_waterfall(p, fs, onset, hz, seconds, m, pulse)
    c, s = ref.tables(pvlib, T, fs, hz)
    ns = ref.slice_steps(seconds, fs)
    want = ref.parts(ref.waterfall_ir(p, onset, c, s, ns, m, pulse)[None], n, m)
    assert got["response"].shape == (1, n, 2) and got["level"].shape == (1, m, n)
    for k in ("onset", "slices", "response", "level"):
        assert got[k].dtype == np.float32
        assert same_bits(got[k], want[k]).all(), (k, fs, onset, T, n, m, ns)
    assert got["onset"][0] == onset and got["slices"][0] == min(m, (T - 1 - onset) // ns + 1)
    return got


# (n, m) of the parity cases: 1, 64, 65 and 130 bins (65 and 130 cross a wave's 64), 1 and 16 slices
SHAPES = [(1, 1), (64, 16), (65, 16), (130, 1), (130, 16)]


# (1) restatement parity
@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the numpy restatement overflows and divides as the definition says)
def test_parity_on_the_adversarial_families(pvlib):
    """every finite family of tests/_adversarial.py, several cells each; onsets as planted (T - 1 among them) and 0; a slice
    length that puts the last slices past T (-inf levels, a slice count below m)"""
    hist, delay = adv_block()
    p, fam = adv.generate(hist, ADV_SEED, ADV_TILE, delay, ADV_FS)
    rng = np.random.default_rng(11)
    pulse = (rng.standard_normal(ADV_T) * 0.1).astype(np.float32)
    seen_short = False
    for f in range(adv.N_FINITE):
        cells = np.argwhere(fam == f)[:2]
        assert len(cells) == 2, adv.FAMILIES[f]
        for i, (x, y) in enumerate(cells):
            n, m = SHAPES[(f + i) % len(SHAPES)]
            q = np.ascontiguousarray(p[:, x, y])
            for onset in (int(delay[x, y]), 0):
                got = check_ir(pvlib, q, ADV_FS, onset, bins_of(n, ADV_FS), 0.0105, m, pulse)  # ns = 15
                if got["slices"][0] < m:
                    seen_short = True
                    k = int(got["slices"][0])
                    assert np.isneginf(got["level"][0, k:]).all()
    assert seen_short
    x, y = 20, 20  # the planted onset T - 1: one term per sum, every slice but the first is empty
    assert delay[x, y] == ADV_T - 1
    got = check_ir(pvlib, np.ascontiguousarray(p[:, x, y]), ADV_FS, ADV_T - 1, bins_of(65, ADV_FS), 0.0105, 16, pulse)
    assert got["slices"][0] == 1


@pytest.mark.parametrize("name", ["g71_smallroom", "g96_smallroom_res375"])
def test_parity_on_the_reference_impulse_responses(pvlib, name):
    g = golden(name)
    size, res = float(g["size"]), int(g["res"])
    fs = int(pvlib.host_grid_info(size, size, res).fs)
    pulse = pvlib.host_pulse(size, size, res)
    done = 0
    for i, ir in enumerate(g["probe_ir"]):
        p = np.ascontiguousarray(ir[:, 0])
        onset = threshold_onset(p)
        if onset < 0:
            continue
        n, m = SHAPES[i % len(SHAPES)]
        got = check_ir(pvlib, p, fs, onset, bins_of(n, fs), 0.02, m, pulse)
        assert np.isfinite(got["response"]).all()
        check_ir(pvlib, p, fs, len(p) - 1, bins_of(n, fs), 0.02, m, pulse)
        done += 1
    assert done >= 4, done


# (2) textbook bound
def test_against_the_textbook_sum(pvlib):
    """every R[k][j], I[k][j] against the same sum in float64 over the same float32 tables and samples: within
    gamma_{N + 1} sum_t |p(t) w(t)|, N = T - t_k the terms of the slice, gamma_q = q u / (1 - q u), u = 2^-24 -- the bound of
    sequential summation (N - 1 additions and one rounded product per term), derived, not measured.  The slices' R, I are read
    back through slice 0 of a record whose onset is the slice's first step: the walk is the same walk"""
    rng = np.random.default_rng(5)
    T, fs, n = 435, 1443, 130
    hz = bins_of(n, fs)
    c, s = ref.tables(pvlib, T, fs, hz)
    pulse = np.ones(T, np.float32)
    u = 2.0 ** -24
    worst = 0.0
    for case in range(4):
        p = (rng.standard_normal(T) * 10.0 ** (-2.0 * np.arange(T) / T) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
        onset, ns = int(rng.integers(0, 40)), 24
        seconds = ns / fs + 1e-4
        assert ref.slice_steps(seconds, fs) == ns
        full = pvlib.host_waterfall(p, fs, onset, hz, seconds, 16, pulse)
        for k in range(16):
            tk = onset + k * ns
            rec = pvlib.host_waterfall(p, fs, tk, hz, seconds, 1, pulse)
            got = rec["response"][0]
            assert same_bits(rec["level"][0, 0], full["level"][0, k]).all()  # (the same sums: the same level)
            if k == 0:
                assert same_bits(got, full["response"][0]).all()
            N = T - tk
            gamma = (N + 1) * u / (1.0 - (N + 1) * u)
            pd = p[tk:].astype(np.float64)[:, None]
            for comp, w in ((0, c), (1, s)):
                terms = pd * w[tk:].astype(np.float64)
                err = np.abs(got[:, comp].astype(np.float64) - terms.sum(axis=0))
                bound = gamma * np.abs(terms).sum(axis=0)
                assert (err <= bound).all(), (case, k, comp, (err / np.maximum(bound, 1e-300)).max())
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    print("waterfall: worst error / bound = %.4f" % worst)


# (3) synthetic mode
@pytest.mark.parametrize("delta,jmode", [(0.01, 20), (0.02, 40), (0.005, 12)])
def test_a_decaying_mode_is_a_ridge(pvlib, delta, jmode):
    """p(t) = (float)(exp(-delta t) cos(2 pi f0 t / fs)) with f0 the bin jmode: the level at the mode's bin falls strictly from
    slice to slice, and the mode's bin is the loudest bin of every one of the 32 slices"""
    T, fs, n, ns, m = 435, 1443, 130, 8, 32
    hz = bins_of(n, fs)
    t = np.arange(T, dtype=np.float64)
    p = (np.exp(-delta * t) * np.cos(2.0 * np.pi * float(hz[jmode]) * t / fs)).astype(np.float32)
    pulse = np.zeros(T, np.float32)
    pulse[0] = 1.0  # (a flat source: spow = 1 at every bin)
    got = check_ir(pvlib, p, fs, 0, hz, (ns + 0.5) / fs, m, pulse)
    level = got["level"][0]
    assert got["slices"][0] == m and np.isfinite(level).all()
    assert (np.diff(level[:, jmode]) < 0).all(), level[:, jmode]
    assert (level.argmax(axis=1) == jmode).all(), level.argmax(axis=1)


# (4) the setting's refusals
def test_setting_rule(pvlib):
    """the refusals of PvAmdSetWaterfall through the host call that applies the same rule (pv_waterfall.h waterfallSettingError;
    PvAmdSetWaterfall checks the setting against its grid's fs before it touches a device)"""
    L = pvlib.lib()
    T, fs = 16, 1443
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    p = np.ones(T, np.float32)
    out = np.zeros(2 + 2 * 513 + 65 * 513, np.float32)

    def call(hz, seconds=0.01, m=4, n=None):
        h = np.asarray(hz, np.float32)
        return L.PvAmdHostWaterfall(fp(p), T, fs, 0, fp(h) if h.size else None, len(h) if n is None else n, seconds, m, fp(p), fp(out))

    assert call([100.0]) == 0
    assert call([0.0, fs / 2.0]) == 0  # both ends are inside
    assert call(np.full(512, 5.0), m=64) == 0  # the caps themselves
    assert call([100.0], seconds=1.0 / fs + 1e-6, m=1) == 0  # ns = 1
    for bad, what in (([], "bins"), (np.full(513, 5.0), "bins"), ([float("nan")], "finite"), ([float("inf")], "finite"),
                      ([10.0, -1.0], "negative"), ([10.0, fs / 2.0 + 0.25], "fs / 2")):
        assert call(bad) == -1, bad
        assert pvlib.last_error().startswith("waterfall:") and what in pvlib.last_error(), pvlib.last_error()
    assert call([100.0], n=-1) == -1 and call([100.0], n=0) == -1
    for m in (0, -1, 65):
        assert call([100.0], m=m) == -1 and "slices" in pvlib.last_error()
    for seconds in (0.0, 0.5 / fs, -1.0, float("nan"), float("inf"), ((1 << 20) + 1) / fs * 1.001):
        assert call([100.0], seconds=seconds) == -1 and "steps" in pvlib.last_error(), seconds
    assert call([100.0], seconds=(1 << 20) / fs) == 0  # ns = 2^20: every slice but the first past T
    assert L.PvAmdHostWaterfall(fp(p), T, fs, T, fp(p), 1, 0.01, 1, fp(p), fp(out)) == -1  # onset = T
    assert L.PvAmdHostWaterfall(fp(p), T, fs, -1, fp(p), 1, 0.01, 1, fp(p), fp(out)) == -1
    assert L.PvAmdHostWaterfall(None, T, fs, 0, fp(p), 1, 0.01, 1, fp(p), fp(out)) == -1
    assert L.PvAmdHostWaterfall(fp(p), T, fs, 0, fp(p), 1, 0.01, 1, None, fp(out)) == -1
    assert L.PvAmdHostWaterfall(fp(p), T, fs, 0, None, 1, 0.01, 1, fp(p), fp(out)) == -1
    # the solver calls refuse a null handle
    for r in (L.PvAmdSetWaterfall(None, fp(p), 1, 0.01, 1), L.PvAmdGetWaterfall(None, None, 0, None, None, None), L.PvAmdWaterfallFloats(None),
              L.PvAmdComputeWaterfall(None, fp(p), 1, None), L.PvAmdCopyWaterfall(None, fp(out), 1)):
        assert r == -1 and pvlib.last_error()


NEW_EXPORTS = ["PvAmdSetWaterfall", "PvAmdGetWaterfall", "PvAmdWaterfallFloats", "PvAmdComputeWaterfall", "PvAmdCopyWaterfall",
               "PvAmdHostWaterfall"]


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
    for name, v in (("BINS", 512), ("SLICES", 64), ("RECEIVERS", 256)):
        assert re.search(r"^#define\s+PVA_WATERFALL_MAX_%s\s+%d\b" % (name, v), hdr, re.M)
        assert getattr(pvlib, "WATERFALL_MAX_" + name) == v


# (5) the edge cases under ASan + UBSan, in a program of their own
def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/waterfall_edges.cpp calls PvAmdHostWaterfall of the HIP-less host build (pv_capi.cpp against the fake solver of
    tests/host/) with exactly sized arrays; nothing is loaded into Python under a sanitizer"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "waterfall_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-DPVA_HOST_TEST", "-I", host,
                           "-I", csrc, "-I", os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "waterfall_edges.cpp"), os.path.join(csrc, "pv_core.cpp"), os.path.join(csrc, "pv_context.cpp"),
                           os.path.join(csrc, "pv_capi.cpp"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "waterfall_edges: 0 failure(s)" in r.stdout, r.stdout
