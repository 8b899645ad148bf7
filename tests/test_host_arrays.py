"""CPU: the source arrays' host restatements (PvAmdHostArrayTaps, PvAmdHostArrayResponse: csrc/pv_arrays.h) against the numpy
restatement written from the header (tests/_arrays_ref.py), the float64 mix within the derived summation bound, the cancelling pair,
the identity array, the refusals, and the edge cases once more in a program of their own under ASan + UBSan.
tests/test_gpu_arrays.py holds the kernels to the same numpy restatement."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _adversarial as adv
import _arrays_ref as ref
from _room_metrics_ref import threshold_onset
from conftest import ROOT, bits, golden, same_bits
from test_host_adversarial import FS as ADV_FS, T as ADV_T, block as adv_block, SEED as ADV_SEED, TILE as ADV_TILE

FS, T = 1443, 435


def check_taps(pvlib, fs, T, gain, delay, interp):
    """host taps == restatement, bit for bit (or both refuse); returns the taps or None"""
    try:
        wd, ww = ref.taps(fs, T, gain, delay, interp)
    except ref.Refused:
        with pytest.raises(pvlib.PlaneverbError):
            pvlib.host_array_taps(fs, T, gain, delay, interp)
        assert pvlib.last_error().startswith("arrays:")
        return None
    gd, gw = pvlib.host_array_taps(fs, T, gain, delay, interp)
    assert list(gd) == list(wd), (gain, delay, interp)
    assert gw.dtype == np.float32 and np.array_equal(bits(gw), bits(ww)), (gain, delay, interp)
    return gd, gw


def delays_of(fs, T):
    """integer delays, mu near 0 and near 1, n = 0 with mu != 0, d just below T"""
    out = [0.0, 1.0 / fs, 7.0 / fs, (T - 1.0) / fs, (T - 3.0) / fs]
    for n in (0, 1, 2, 17, T - 3, T - 2, T - 1):
        for mu in (1e-7, 1e-4, 0.25, 0.5, 0.75, 1.0 - 1e-4, 1.0 - 1e-6):
            out.append((n + mu) / fs)
    out += [np.nextafter(np.float32(T / fs), np.float32(0)), T / fs, (T + 0.5) / fs, (T - 0.5) / fs, (T - 0.49) / fs]
    return [float(np.float32(d)) for d in out]


def test_taps_against_the_restatement(pvlib):
    seen = {"one": 0, "four": 0, "refused": 0, "past": 0}
    for interp in (ref.NEAREST, ref.LAGRANGE3):
        for gain in (1.0, -1.0, 0.37, -2.5e-3, 0.0, 3.0e20):
            for d in delays_of(FS, T):
                r = check_taps(pvlib, FS, T, gain, d, interp)
                if r is None:
                    seen["refused"] += 1
                    continue
                seen["one" if len(r[0]) == 1 else "four"] += 1
                seen["past"] += int(max(r[0]) >= T)
                assert min(r[0]) >= 0 and list(r[0]) == sorted(r[0])
    assert all(v > 0 for v in seen.values()), seen
    # n = 0 with mu != 0 is refused by LAGRANGE3 and rounds by NEAREST
    assert check_taps(pvlib, FS, T, 1.0, 0.4 / FS, ref.LAGRANGE3) is None
    assert list(check_taps(pvlib, FS, T, 1.0, 0.4 / FS, ref.NEAREST)[0]) == [0]
    # a delay that rounds to T is refused by NEAREST, kept (with taps past T - 1) by LAGRANGE3
    assert check_taps(pvlib, FS, T, 1.0, (T - 0.25) / FS, ref.NEAREST) is None
    assert list(check_taps(pvlib, FS, T, 1.0, (T - 0.25) / FS, ref.LAGRANGE3)[0]) == [T - 2, T - 1, T, T + 1]
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert check_taps(pvlib, FS, T, bad, 0.01, ref.LAGRANGE3) is None
        assert check_taps(pvlib, FS, T, 1.0, bad, ref.NEAREST) is None
    assert check_taps(pvlib, FS, T, 1.0, -1e-6, ref.NEAREST) is None
    assert check_taps(pvlib, FS, T, 1.0, 0.01, 2) is None


def test_lagrange_weights_sum_to_the_gain():
    """sum_j gain * L_j = gain within 4 ulp of double, before the rounding to float32 (the L_j are the Lagrange basis of four nodes:
    they sum to 1; each is three multiplications and a division of numbers of magnitude <= 3)"""
    rng = np.random.default_rng(3)
    for mu in list(rng.uniform(0.0, 1.0, 200)) + [1e-9, 1.0 - 1e-9, 0.5]:
        for gain in (1.0, -0.37, 123.5):
            s = sum(ref.lagrange_double(gain, float(mu)))
            g = float(np.float32(gain))
            assert abs(s - g) <= 4 * np.spacing(abs(g)), (mu, gain, s)


def random_members(rng, M, fs, T, far=False):
    out = []
    for i in range(M):
        kind = rng.integers(0, 4)
        if kind == 0:
            d = 0.0
        elif kind == 1:
            d = float(rng.integers(2, 40)) / fs  # (k / fs in float32 is k steps only nearly: n = k or k - 1)
        else:
            d = float(rng.uniform(1.01, (T - 2 if far else 60))) / fs
        out.append((float(rng.uniform(-1.5, 1.5)), float(np.float32(d))))
    if far:
        out[-1] = (0.8, float(np.float32((T - 1.5) / fs)))  # (taps T - 3 .. T: one past T - 1)
    return out


def check_response(pvlib, p, members, fs, interp, extra=None):
    """host response == restatement, bit for bit, onset included; within the summation bound of the float64 mix"""
    p = np.asarray(p, np.float32)
    T = p.shape[1]
    tm, td, tw = ref.expand(members, fs, T, interp)
    if extra is not None:  # (taps the tap rule never makes: below t = 0)
        tm, td, tw = (np.concatenate([a, np.asarray(b, a.dtype)]) for a, b in zip((tm, td, tw), extra))
    got, on = pvlib.host_array_response(p, tm, td, tw)
    want = ref.response(p, tm, td, tw)
    assert got.dtype == np.float32 and same_bits(got, want).all()
    assert bits(np.float32(on)) == bits(ref.onset(want))
    # gamma_{K + 1} sum |w p|: K products and K sums, each rounded once (u = 2^-24) -- the bound of sequential summation
    K, u = len(tm), 2.0 ** -24
    gamma = (K + 1) * u / (1.0 - (K + 1) * u)
    exact, mag = np.zeros(T), np.zeros(T)
    for m, d, w in zip(tm, td, tw):
        q = ref.shifted(p[m], int(d)).astype(np.float64) * float(w)
        exact += q
        mag += np.abs(q)
    if np.isfinite(mag).all() and mag.max() < 1e30 and (mag[mag > 0].min() if (mag > 0).any() else 1) > 1e-30:
        assert (np.abs(got.astype(np.float64) - exact) <= gamma * mag).all()
    return got, on


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_response_on_the_adversarial_families(pvlib):
    hist, delay = adv_block()
    p, fam = adv.generate(hist, ADV_SEED, ADV_TILE, delay, ADV_FS)
    rng = np.random.default_rng(17)
    for f in range(adv.N_FINITE):
        cells = np.argwhere(fam == f)
        assert len(cells) >= 2, adv.FAMILIES[f]
        for M in (1, 2, 17, 64):
            pick = cells[rng.integers(0, len(cells), M)]
            rows = np.stack([p[:, x, y] for x, y in pick])
            check_response(pvlib, rows, random_members(rng, M, ADV_FS, ADV_T, far=(M == 17)), ADV_FS, (f + M) % 2)
    # taps reaching below t = 0 (negative delays) and past T - 1, on one member
    rows = p[:, cells[0][0], cells[0][1]][None]
    check_response(pvlib, rows, [(1.0, 0.0)], ADV_FS, ref.NEAREST, extra=([0, 0, 0], [-1, -ADV_T, ADV_T + 5], [0.5, 2.0, 3.0]))


@pytest.mark.parametrize("name", ["g71_smallroom", "g96_smallroom_res375"])
def test_response_on_the_reference_impulse_responses(pvlib, name):
    g = golden(name)
    size, res = float(g["size"]), int(g["res"])
    fs = int(pvlib.host_grid_info(size, size, res).fs)
    rows = np.stack([np.ascontiguousarray(ir[:, 0]) for ir in g["probe_ir"]]).astype(np.float32)
    M0, T = rows.shape
    rng = np.random.default_rng(5)
    for M in (1, 2, 17, 64):
        sel = rows[rng.integers(0, M0, M)]
        for interp in (ref.NEAREST, ref.LAGRANGE3):
            check_response(pvlib, sel, random_members(rng, M, fs, T, far=(M == 2)), fs, interp)
    # the identity array: y == p, and the onset the reference's rule gives on p
    for p in rows:
        got, on = check_response(pvlib, p[None], [(1.0, 0.0)], fs, ref.LAGRANGE3)
        assert same_bits(got, p).all()
        t0 = threshold_onset(p)
        assert (on == ref.FLT_MAX) if t0 < 0 else (on == t0)
    # the cancelling pair: one cell, equal delays, gains +g and -g
    for d in (0.0, 3.0 / fs, 3.37 / fs):
        got, on = check_response(pvlib, np.stack([rows[0], rows[0]]), [(0.7, d), (-0.7, d)], fs, ref.LAGRANGE3)
        if len(ref.taps(fs, T, 0.7, d, ref.LAGRANGE3)[0]) == 1:  # (tap by tap the sums cancel exactly only where a member is one tap)
            assert (bits(got) == 0).all() and on == ref.FLT_MAX


def test_cancelling_pair_is_exactly_zero(pvlib):
    """y = (+0 + g p) + (-g p) = +0 at every step, also with four taps per member when the members alternate tap by tap"""
    rng = np.random.default_rng(9)
    p = (rng.standard_normal(T) * 0.3).astype(np.float32)
    for d in (0.0, 5.0 / FS):
        tm, td, tw = ref.expand([(0.9, d), (-0.9, d)], FS, T, ref.NEAREST)
        y, on = pvlib.host_array_response(np.stack([p, p]), tm, td, tw)
        assert (bits(y) == 0).all() and on == ref.FLT_MAX


def test_refusals(pvlib):
    L = pvlib.lib()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    d4, w4 = np.zeros(4, np.int32), np.zeros(4, np.float32)
    assert L.PvAmdHostArrayTaps(FS, T, 1.0, 0.0, 0, None, fp(w4)) == -1 and pvlib.last_error().startswith("arrays:")
    assert L.PvAmdHostArrayTaps(FS, T, 1.0, 0.0, 0, ip(d4), None) == -1
    assert L.PvAmdHostArrayTaps(0, T, 1.0, 0.0, 0, ip(d4), fp(w4)) == -1
    assert L.PvAmdHostArrayTaps(FS, 0, 1.0, 0.0, 0, ip(d4), fp(w4)) == -1
    assert L.PvAmdHostArrayTaps(FS, T, 1.0, 0.0, -1, ip(d4), fp(w4)) == -1 and "interp" in pvlib.last_error()
    p, out = np.ones((2, 8), np.float32), np.zeros(8, np.float32)
    tm, td, tw = np.array([0, 1], np.int32), np.array([0, 1], np.int32), np.ones(2, np.float32)
    assert L.PvAmdHostArrayResponse(fp(p), 2, 8, ip(tm), ip(td), fp(tw), 2, fp(out), None) == 0
    assert L.PvAmdHostArrayResponse(None, 2, 8, ip(tm), ip(td), fp(tw), 2, fp(out), None) == -1
    assert L.PvAmdHostArrayResponse(fp(p), 2, 8, ip(tm), ip(td), fp(tw), 2, None, None) == -1
    assert L.PvAmdHostArrayResponse(fp(p), 2, 8, None, ip(td), fp(tw), 2, fp(out), None) == -1
    assert L.PvAmdHostArrayResponse(fp(p), 0, 8, ip(tm), ip(td), fp(tw), 2, fp(out), None) == -1
    assert L.PvAmdHostArrayResponse(fp(p), 1, 8, ip(tm), ip(td), fp(tw), 2, fp(out), None) == -1 and "member" in pvlib.last_error()
    assert L.PvAmdHostArrayResponse(fp(p), 2, 8, None, None, None, 0, fp(out), None) == 0 and (out == 0).all()  # no taps: y = +0
    # the solver calls refuse a null handle
    for r in (L.PvAmdSetArrays(None, ip(tm), 1, fp(p), 0), L.PvAmdGetArrays(None, None, 0, None), L.PvAmdGetArrayTaps(None, 0, None, None, None, 0),
              L.PvAmdSetArrayRecords(None, 1, 0), L.PvAmdGetArrayRecordKinds(None, None, None), L.PvAmdArrayRecordFloats(None, 0, 1),
              L.PvAmdComputeArrays(None, None), L.PvAmdCopyArrayResponse(None, 0, fp(out)), L.PvAmdGetArrayOnsets(None, fp(out), 1),
              L.PvAmdGetArrayRecords(None, 0, 1, fp(out), 1)):
        assert r == -1 and pvlib.last_error()


NEW_EXPORTS = ["PvAmdSetArrays", "PvAmdGetArrays", "PvAmdGetArrayTaps", "PvAmdSetArrayRecords", "PvAmdGetArrayRecordKinds",
               "PvAmdArrayRecordFloats", "PvAmdComputeArrays", "PvAmdCopyArrayResponse", "PvAmdGetArrayOnsets", "PvAmdGetArrayRecords",
               "PvAmdHostArrayTaps", "PvAmdHostArrayResponse"]


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
    for name, v in (("ARRAYS_MAX", 256), ("ARRAY_MEMBERS_MAX", 64), ("ARRAY_NEAREST", 0), ("ARRAY_LAGRANGE3", 1)):
        assert re.search(r"^#define\s+PVA_%s\s+%d\b" % (name, v), hdr, re.M)
        assert getattr(pvlib, name) == v


def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/arrays_edges.cpp calls PvAmdHostArrayTaps / PvAmdHostArrayResponse of the HIP-less host build (pv_capi.cpp against
    the fake solver of tests/host/) with exactly sized arrays; nothing is loaded into Python under a sanitizer"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "arrays_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-DPVA_HOST_TEST", "-I", host,
                           "-I", csrc, "-I", os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "arrays_edges.cpp"), os.path.join(csrc, "pv_core.cpp"), os.path.join(csrc, "pv_context.cpp"),
                           os.path.join(csrc, "pv_capi.cpp"), "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "arrays_edges: 0 failure(s)" in r.stdout, r.stdout
