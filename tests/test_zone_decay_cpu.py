"""CPU: the zone decay's host restatement (PvAmdHostZoneDecay, csrc/pv_zone_decay.h) against the independent numpy restatement
(tests/_zone_decay_ref.py) bit for bit, its sums against exact references within a derived bound, a synthetic geometric decay
whose decay time it must give back, its edges, its refusals, the exports, and the edge cases once more in a stand-alone program
under ASan + UBSan.  The GPU pass is held to PvAmdHostZoneDecay in tests/test_gpu_zone_decay.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _zone_decay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 3), (7, 64), (9, 65), (4, 130)]  # gy below a block, one block, one cell more, two blocks and two cells
T, FS = 40, 400                                # tailN = 4
ZONES = 6                                      # labels 0 .. 5 scattered; zone 6 has no cell
ALIGNS = ["absolute", "onset"]
NEW_EXPORTS = ["PvAmdComputeZoneDecay", "PvAmdZoneDecayChunkSlots", "PvAmdHostZoneDecay"]


def planted(gx, gy):
    """a decaying random history (1.5 dB a step, so the ranges fill), LARGE values below every onset (they must not count),
    onsets 0 .. T - 1 with 0, T - 1 and 'none' planted, labels 0 .. 5 scattered"""
    rng = np.random.default_rng(gx * 1000 + gy)
    delay = rng.integers(0, T, (gx, gy)).astype(np.float32)
    early = rng.random((gx, gy)) < 0.6  # (most cells early: the curves span the ranges)
    delay[early] = rng.integers(0, 4, int(early.sum()))
    lab = rng.integers(0, ZONES, (gx, gy)).astype(np.uint8)
    delay[lab >= 3] %= 6  # (zones 3 .. 5 begin early everywhere: their ONSET curves keep slots before the tail)
    flat = delay.reshape(-1)
    cells = rng.permutation(gx * gy)
    flat[cells[0]], flat[cells[1]] = 0.0, T - 1
    flat[cells[2:2 + max(2, gx * gy // 8)]] = ref.NO_ONSET
    t = np.arange(T)[:, None, None]
    p = (rng.standard_normal((T, gx, gy)) * 10.0 ** (-0.075 * t)).astype(np.float32)
    p[t < np.where(delay == ref.NO_ONSET, T, delay)[None]] = np.float32(1.0e6)
    lab.reshape(-1)[cells[:2]] = 1, 2  # (the planted onsets 0 and T - 1)
    return p, delay, lab


_CASES = {}


def case(pvlib, shape, align):
    key = (shape, align)
    if key not in _CASES:
        p, delay, lab = planted(*shape)
        got = pvlib.host_zone_decay(p, delay, FS, lab, ZONES, align)
        for a in (p, delay, lab) + got:
            a.setflags(write=False)
        _CASES[key] = (p, delay, lab, got)
    return _CASES[key]


# (1) the host restatement against the numpy restatement, bit for bit
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_host_equals_numpy_restatement(pvlib, shape, align):
    p, delay, lab, (rec, etc, edc) = case(pvlib, shape, align)
    assert rec.shape == (ZONES,) and rec.dtype == pvlib.ZONE_DECAY_DTYPE == ref.DTYPE and rec.dtype.itemsize == 64
    assert etc.shape == edc.shape == (ZONES, T)
    wrec, wetc, wedc = ref.zone_decay(p, delay, FS, lab, ZONES, ALIGNS.index(align))
    assert ref.same_doubles(etc, wetc), np.argwhere(etc != wetc)[:4]
    assert ref.same_doubles(edc, wedc), np.argwhere(edc != wedc)[:4]
    assert ref.same_records(rec, wrec), ref.first_difference(rec, wrec)
    reached = delay != ref.NO_ONSET
    assert [int(r["n_cells"]) for r in rec] == [int(((lab == z) & reached).sum()) for z in range(1, ZONES + 1)]
    assert rec[ZONES - 1]["n_cells"] == 0 and rec["n_cells"][:5].min() >= (0 if shape == (5, 3) else 5)
    assert (delay == T - 1).any() and (delay == 0).any() and (~reached).any()
    if shape != (5, 3):
        assert np.isfinite(rec["edt"][2:5]).all() and (rec["n_t30"][2:5] > 2).all() and (rec["t_last"][2:5] <= 5).all()
        if align == "onset":  # zone 2 holds the onset T - 1: no slot holds every cell
            assert rec[1]["t_last"] == T - 1 and np.isnan(rec[1]["depth"]) and rec[1]["n_edt"] == 0


# (2) the sums against exact references
@pytest.mark.parametrize("align", ALIGNS)
def test_sums_within_the_error_bound_of_exact_sums(pvlib, align):
    """u = 2^-53.  Every term (double)p * (double)p is exact (24 x 24 bits) and non-negative.  A double sum of n terms in ANY
    order carries each term through at most n - 1 roundings: |etc - S| <= gamma_(n-1) S, gamma_k = k u / (1 - k u); the adds of
    +0.0 (cells without a sample, padding) are exact.  math.fsum is S rounded once (<= u S).  Together (gamma_(n-1) + u) S =
    n u S (1 + O(n u)), the O(n u) factor (1e-13 here) far below the resolution the bound is evaluated with.  n = the members with
    a sample in the slot."""
    shape = (4, 130)
    p, delay, lab, (rec, etc, edc) = case(pvlib, shape, align)
    reached = delay != ref.NO_ONSET
    t0 = np.where(reached, delay, 0).astype(int)
    worst = 0.0
    for z in range(1, ZONES):
        xs, ys = np.nonzero((lab == z) & reached)
        for j in range(T):
            terms = []
            for X, Y in zip(xs, ys):
                t = j if align == "absolute" else t0[X, Y] + j
                if t0[X, Y] <= t < T:
                    terms.append(float(p[t, X, Y]) ** 2)  # (exact)
            exact = math.fsum(terms)
            bound = len(terms) * 2.0 ** -53 * exact
            worst = max(worst, abs(etc[z - 1, j] - exact) / bound if bound else 0.0)
            assert abs(etc[z - 1, j] - exact) <= bound, (z, j, len(terms), etc[z - 1, j], exact)
        # edc: T - j further adds of non-negative terms
        for j in (0, T // 2):
            exact = math.fsum(float(v) for v in etc[z - 1, j:])
            assert abs(edc[z - 1, j] - exact) <= (T - j) * 2.0 ** -53 * exact
    print(align, "largest |etc - exact| / bound:", worst)


# (3) a geometric decay gives back its decay time
def test_fit_recovers_a_geometric_decay(pvlib):
    """Every member starts at t0 = 0 with p_s(t) = fl32(a_s g^t), g = 10^(-step / 20): step dB a slot, so the ideal curve is
    etc[j] = A q^j, q = g^2, edc[j] = A q^j (1 - q^(T - j)) / (1 - q), and the ideal level is the line -step j plus
        d(j) = 10 log10((1 - q^(T - j)) / (1 - q^T))   (the truncation at T; -D_t(j) <= d(j) <= 0, growing in size with j).
    True decay time: 60 / step / fs seconds.
    Roundings: p is a float32, so p^2 = a^2 q^t (1 + e)^2, |e| <= 2^-24 (the power itself is computed in double and rounded
    once more: |e| <= 2^-24 + 2^-52); the sums add at most (cells + T) roundings of 2^-53 each to a sum of non-negative terms.
    So edc[j] is its ideal value times (1 + e_j), |e_j| <= E = 2^-23 + 2^-47 + (cells + T) 2^-52 (with room), the ratio
    r(j) carries two of them and one division, and log10 is within an ulp or two of a value of size <= 2 dB / 10 -- D_r =
    10 log10((1 + E)^2 (1 + 2^-52)) + 4 * 35 * 2^-52 covers the level's error.
    Members of a range [lo, hi] (dB): a member has -step j + d(j) >= lo, and d <= 0, so j <= jmax = floor(-lo / step): on the
    members |level - line| <= D = D_t(jmax) + D_r.  Every j with -hi / step <= j and -step j - D >= lo IS a member, so
    n >= nmin = floor((-lo - D) / step) - ceil(-hi / step) + 1 - 1 (one off for a level within rounding of a limit).
    Members are contiguous in j (edc decreases strictly), so kbar is their mean and the fitted slope is
        sum (k - kbar) y_k / Sxx,  Sxx = n (n^2 - 1) / 12;
    a perturbation of the y_k by at most D moves it by at most D sum|k - kbar| / Sxx <= D (n^2 / 4) / Sxx = 3 D n / (n^2 - 1),
    decreasing in n.  The two sums Sy and Sky are accumulated in double: (n + 1) roundings over terms of size <= jmax * -lo,
    an error of the numerator of at most 2 (n + 2) 2^-53 n jmax (-lo), divided by Sxx: D_s.
    With rho = (3 D nmin / (nmin^2 - 1) + D_s) / step the value is within rho / (1 - rho) of the true time, relatively, plus two
    roundings of the final quotients."""
    gx, gy, Tn, fs, step = 3, 70, 120, 1000, 0.5
    tail = ref.tail_n(fs)
    assert tail == 10
    g = 10.0 ** (-step / 20.0)
    q = g * g
    rng = np.random.default_rng(5)
    amp = rng.uniform(0.5, 2.0, (gx, gy))
    p = (amp[None] * g ** np.arange(Tn, dtype=np.float64)[:, None, None]).astype(np.float32)
    delay = np.zeros((gx, gy), np.float32)
    lab = np.ones((gx, gy), np.uint8)
    true = 60.0 / step / fs
    for align in ALIGNS:
        rec, etc, edc = pvlib.host_zone_decay(p, delay, fs, lab, 1, align)
        r = rec[0]
        assert (r["n_cells"], r["t_first"], r["t_last"]) == (gx * gy, 0, 0)
        j_end = Tn - tail
        # all three ranges complete: the level at jEnd - 1 lies below -35 dB by the ideal curve (and the record agrees)
        assert -step * (j_end - 1) < -35.0 - 1.0 and r["depth"] < -35.0
        e = 2.0 ** -23 + 2.0 ** -47 + (gx * gy + Tn) * 2.0 ** -52
        d_r = 10.0 * math.log10((1.0 + e) ** 2 * (1.0 + 2.0 ** -52)) + 4 * 35 * 2.0 ** -52
        for name, cnt, hi, lo in (("edt", "n_edt", 0.0, -10.0), ("t20", "n_t20", -5.0, -25.0), ("t30", "n_t30", -5.0, -35.0)):
            jmax = math.floor(-lo / step)
            d_t = -10.0 * math.log10((1.0 - q ** (Tn - jmax)) / (1.0 - q ** Tn))
            assert d_t > 0.0
            d = d_t + d_r
            nmin = math.floor((-lo - d) / step) - math.ceil(-hi / step) + 1 - 1
            assert r[cnt] >= nmin >= 19, (name, r[cnt], nmin)
            d_s = 2 * (nmin + 2) * 2.0 ** -53 * nmin * jmax * -lo / (nmin * (nmin * nmin - 1) / 12.0)
            rho = (3.0 * d * nmin / (nmin * nmin - 1) + d_s) / step
            bound = true * (rho / (1.0 - rho) + 2.0 ** -51)
            print(align, name, "n", r[cnt], "value", r[name], "true", true, "error", abs(r[name] - true), "bound", bound)
            assert abs(r[name] - true) <= bound, (align, name)


# (4) edges
def test_edges(pvlib):
    gx, gy, Tn = 3, 66, 30  # tailN = 4: the tail begins at 26
    rng = np.random.default_rng(9)
    p = rng.standard_normal((Tn, gx, gy)).astype(np.float32)
    delay = np.full((gx, gy), ref.NO_ONSET, np.float32)
    lab = np.zeros((gx, gy), np.uint8)
    lab[0, :10] = 1                         # 1: every cell unreached
    lab[1, 60:66], delay[1, 60:66] = 2, 26  # 2: t_first at the tail's first step ...
    delay[1, 65] = 29                       #    ... and t_last = T - 1
    lab[2, 64], delay[2, 64] = 4, 0         # 4: one cell from step 0; 3: no cell at all
    p[:, 2, 64] = np.float32(0.25) ** np.arange(Tn)  # 12 dB a step: the EDT range holds its first point only
    for align in ALIGNS:
        rec, etc, edc = pvlib.host_zone_decay(p, delay, FS, lab, 4, align)
        wrec, wetc, wedc = ref.zone_decay(p, delay, FS, lab, 4, ALIGNS.index(align))
        assert ref.same_records(rec, wrec) and ref.same_doubles(etc, wetc) and ref.same_doubles(edc, wedc)
        for z in (0, 2):  # unreached, no cells
            r = rec[z]
            assert (r["n_cells"], r["t_first"], r["t_last"], r["n_edt"], r["n_t20"], r["n_t30"]) == (0, -1, -1, 0, 0, 0)
            assert r["e0"] == 0.0 and not np.signbit(r["e0"]) and all(np.isnan(r[f]) for f in ("edt", "t20", "t30", "depth"))
            assert (etc[z] == 0.0).all() and (edc[z] == 0.0).all()
        r = rec[1]  # ABSOLUTE: j0 = 26 = jEnd; ONSET: jEnd = 30 - 4 - 29 < 0
        assert (r["n_cells"], r["t_first"], r["t_last"], r["n_edt"], r["n_t20"], r["n_t30"]) == (6, 26, 29, 0, 0, 0)
        assert all(np.isnan(r[f]) for f in ("edt", "t20", "t30", "depth")) and r["e0"] > 0.0
        r = rec[3]
        assert r["n_edt"] == 1 and np.isnan(r["edt"]) and r["n_t20"] == 2 and r["t20"] > 0.0 and r["depth"] < -100.0
        for z in range(4):
            assert edc[z, 0].tobytes() == rec[z]["e0"].tobytes()          # E0 bit for bit, whatever t_first is
            assert (np.diff(edc[z]) <= 0.0).all() and edc[z, -1] == etc[z, -1]
    # the single cell: the two alignments coincide at t0 = 0, and etc is the squared sample
    assert np.array_equal(etc[3], p[:, 2, 64].astype(np.float64) ** 2)
    # n_zones None: the largest label
    assert ref.same_records(pvlib.host_zone_decay(p, delay, FS, lab)[0], pvlib.host_zone_decay(p, delay, FS, lab, 4)[0])


# (5) refusals and exports
def test_refusals(pvlib):
    p = np.zeros((6, 4, 5), np.float32)
    delay = np.zeros((4, 5), np.float32)
    lab = np.zeros((4, 5), np.uint8)
    lab[1, 1] = 3
    with pytest.raises(pvlib.PlaneverbError, match="^zone decay: a label above nZones"):
        pvlib.host_zone_decay(p, delay, FS, lab, 2)
    for n in (0, 65):
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: nZones is 1 .. 64"):
            pvlib.host_zone_decay(p, delay, FS, np.zeros((4, 5), np.uint8), n)
    with pytest.raises(pvlib.PlaneverbError, match="^zone decay: align is"):
        pvlib.host_zone_decay(p, delay, FS, lab, 3, 2)
    with pytest.raises(ValueError, match="^zone decay: align is one of"):
        pvlib.host_zone_decay(p, delay, FS, lab, 3, "late")
    for bad in (6.0, -1.0, np.nan):
        d = delay.copy()
        d[1, 1] = bad
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: an onset outside"):
            pvlib.host_zone_decay(p, d, FS, lab, 3)
        d[1, 1], d[0, 0] = 0.0, bad  # (an unlabelled cell's onset is not looked at)
        pvlib.host_zone_decay(p, d, FS, lab, 3)
    with pytest.raises(pvlib.PlaneverbError, match="^zone decay: PvAmdHostZoneDecay"):
        pvlib.host_zone_decay(p, delay, 0, lab, 3)
    with pytest.raises(ValueError):
        pvlib.host_zone_decay(p, delay[:3], FS, lab, 3)
    L = pvlib.lib()
    out = np.zeros(3, pvlib.ZONE_DECAY_DTYPE)
    assert L.PvAmdHostZoneDecay(None, None, 4, 5, 6, FS, None, 3, 0, out.ctypes.data_as(C.c_void_p), None, None) == -1
    assert pvlib.last_error().startswith("zone decay: ")
    rec, etc, edc = pvlib.host_zone_decay(p, delay, FS, lab, 64, "onset")
    assert rec.shape == (64,) and etc.shape == (64, 6)


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
    assert re.search(r"#define\s+PVA_ZONE_DECAY_ABSOLUTE\s+0\b", hdr) and re.search(r"#define\s+PVA_ZONE_DECAY_ONSET\s+1\b", hdr)
    assert (pvlib.PVA_ZONE_DECAY_ABSOLUTE, pvlib.PVA_ZONE_DECAY_ONSET) == (0, 1)
    assert pvlib.ZONE_DECAY_DTYPE.itemsize == 64 and pvlib.ZONE_DECAY_DTYPE.names == ref.DTYPE.names
    assert callable(pvlib.Solver.zone_decay) and callable(pvlib.host_zone_decay)


# (6) the edge cases under ASan + UBSan, in a program of their own
def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/zone_decay_edges.cpp includes csrc/pv_zone_decay.h and runs the edge cases with exactly sized arrays; nothing is
    loaded into Python under a sanitizer"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "zone_decay_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", csrc, "-Wall",
                           "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "zone_decay_edges.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "zone_decay_edges: 0 failure(s)" in r.stdout, r.stdout
