"""CPU: the zone band decay's host restatement (PvAmdHostZoneBandDecay, csrc/pv_zone_band_decay.h) against the independent numpy
restatement (tests/_zone_band_decay_ref.py) bit for bit, its tie to PvAmdHostZoneDecay through the identity filter, a single-cell
zone against an independently filtered response and against PvAmdHostBandMetrics, PvAmdHostZoneCurveClarity on hand-built curves,
the refusals, the exports, and the edge cases once more in a stand-alone program under ASan + UBSan.  The GPU pass is held to
PvAmdHostZoneBandDecay in tests/test_gpu_zone_band_decay.py.

The physical check the issue describes -- a zone of sinusoids at a band's centre under a geometric envelope, T20 within a DERIVED
bound -- is left out: the envelope, the ripple of the squared sinusoid under the backward sum and the start-up transient of the
filter can be bounded in closed form, but the float32 roundings of the recursive filter enter through its noise gain, for which no
closed bound was derived here; a tolerance read off the output would check nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _zone_band_decay_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 5), (3, 64), (3, 70), (2, 130)]  # gy below a block, one block, a block and six cells, two blocks and two cells
T, FS = 40, 400                                # tailN = 4, n50 = 20, n80 = 32
ZONES = 5                                      # labels 0 .. 3 scattered, zone 4 = one cell, zone 5 has no cell
ALIGNS = ["absolute", "onset"]
BANDS = {1: [50.0], 3: [25.0, 50.0, 100.0]}    # octave bands below fs / 2 = 200 Hz
NEW_EXPORTS = ["PvAmdComputeZoneBandDecay", "PvAmdZoneBandDecayChunk", "PvAmdHostZoneBandDecay", "PvAmdHostZoneCurveClarity"]


def planted(gx, gy):
    """a decaying random history, LARGE values below every onset (they must not count), random onsets with 0, T - 1 and 'none'
    planted, labels 0 .. 3 scattered, zone 4 one cell"""
    rng = np.random.default_rng(gx * 1000 + gy + 7)
    delay = rng.integers(0, T, (gx, gy)).astype(np.float32)
    early = rng.random((gx, gy)) < 0.6
    delay[early] = rng.integers(0, 4, int(early.sum()))
    lab = rng.integers(0, 4, (gx, gy)).astype(np.uint8)
    flat = delay.reshape(-1)
    cells = rng.permutation(gx * gy)
    flat[cells[0]], flat[cells[1]] = 0.0, T - 1
    flat[cells[2:2 + max(2, gx * gy // 8)]] = ref.NO_ONSET
    lab.reshape(-1)[cells[:2]] = 1, 2
    lab.reshape(-1)[cells[-1]], flat[cells[-1]] = 4, 3.0  # the one-cell zone
    t = np.arange(T)[:, None, None]
    p = (rng.standard_normal((T, gx, gy)) * 10.0 ** (-0.075 * t)).astype(np.float32)
    p[t < np.where(delay == ref.NO_ONSET, T, delay)[None]] = np.float32(1.0e6)
    return p, delay, lab


_CASES = {}


def case(pvlib, shape, nb, align):
    key = (shape, nb, align)
    if key not in _CASES:
        p, delay, lab = planted(*shape)
        coefs = pvlib.host_band_coefs(FS, BANDS[nb])
        got = pvlib.host_zone_band_decay(p, delay, FS, lab, coefs, ZONES, align)
        for a in (p, delay, lab, coefs) + got:
            a.setflags(write=False)
        _CASES[key] = (p, delay, lab, coefs, got)
    return _CASES[key]


# (1) the host restatement against the numpy restatement, bit for bit
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("shape,nb", [(s, 1) for s in SHAPES] + [((3, 70), 3)], ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "%db" % v)
def test_host_equals_numpy_restatement(pvlib, shape, nb, align):
    p, delay, lab, coefs, (rec, etc, edc) = case(pvlib, shape, nb, align)
    assert rec.shape == (ZONES, nb) and rec.dtype == pvlib.ZONE_BAND_DECAY_DTYPE == ref.DTYPE and rec.dtype.itemsize == 96
    assert etc.shape == edc.shape == (ZONES, nb, T)
    wrec, wetc, wedc = ref.zone_band_decay(p, delay, FS, lab, ZONES, coefs, ALIGNS.index(align))
    assert ref.same_doubles(etc, wetc), np.argwhere(etc != wetc)[:4]
    assert ref.same_doubles(edc, wedc), np.argwhere(edc != wedc)[:4]
    assert ref.same_records(rec, wrec), ref.first_difference(rec, wrec)
    reached = delay != ref.NO_ONSET
    for b in range(nb):  # the members do not depend on the band
        assert [int(r["n_cells"]) for r in rec[:, b]] == [int(((lab == z) & reached).sum()) for z in range(1, ZONES + 1)]
    assert (rec[3]["n_cells"] == 1).all() and (rec[4]["n_cells"] == 0).all() and (rec[4]["t_first"] == -1).all()
    empty = rec[4]
    assert all(np.isnan(empty[f]).all() for f in ("edt", "t20", "t30", "depth", "c50", "c80", "d50", "ts")) and (empty["e0"] == 0.0).all()
    assert (etc[4] == 0.0).all() and not np.signbit(etc[4]).any()
    some = rec["n_cells"] > 0
    assert np.isfinite(rec["c50"][some]).all() and np.isfinite(rec["ts"][some]).all() and some[:4].sum() >= nb * (2 if shape == (4, 5) else 4)
    if nb == 3:  # the bands differ
        assert not np.array_equal(etc[0, 0], etc[0, 1]) and not np.array_equal(etc[0, 1], etc[0, 2])


# (2) the identity filter ties the pass to the broadband restatement
@pytest.mark.parametrize("align", ALIGNS)
def test_identity_filter_gives_the_broadband_zone_decay(pvlib, align):
    """b0 = 1 and every other coefficient 0 in both sections: y = 1 * x + 0 = x in every step (the states stay +0.0f), so etc, edc
    and the shared fields of every record are PvAmdHostZoneDecay's, bit for bit -- in both of two 'bands'"""
    p, delay, lab = planted(3, 70)
    rec, etc, edc = pvlib.host_zone_band_decay(p, delay, FS, lab, np.stack([ref.IDENTITY, ref.IDENTITY]), ZONES, align)
    wrec, wetc, wedc = pvlib.host_zone_decay(p, delay, FS, lab, ZONES, align)
    for b in range(2):
        assert ref.same_doubles(etc[:, b], wetc) and ref.same_doubles(edc[:, b], wedc)
        for f in pvlib.ZONE_DECAY_DTYPE.names:
            assert ref.same_doubles(rec[f][:, b].astype(np.float64), wrec[f].astype(np.float64)), f
    # ... and PvAmdHostZoneCurveClarity on that broadband curve gives the records' clarity
    for z in range(ZONES):
        j0 = int(wrec[z]["t_first"]) if align == "absolute" and wrec[z]["n_cells"] else 0
        got = pvlib.host_zone_curve_clarity(wetc[z], FS, j0)
        assert ref.same_doubles(got, np.array([rec[z, 0][f] for f in ("c50", "c80", "d50", "ts")]))


# (3) a single-cell zone
def test_single_cell_zone_is_the_filtered_response_squared(pvlib):
    """etc of a one-cell zone is the exact double square of the independently filtered y(t) (a butterfly over one value and 63
    times +0.0 returns the value).  Its e0 against PvAmdHostBandMetrics' e0: that one squares in float32 and adds n = T - t0 terms
    sequentially in float32, so it lies within n * 2^-24, relatively, of the exact sum of the exact squares (one rounding per
    product and n - 1 roundings of partial sums that never exceed the total, first order in 2^-24) -- the bound the issue names;
    ours is that sum in double (n * 2^-53, absorbed) rounded to float."""
    p, delay, lab, coefs, (rec, etc, edc) = case(pvlib, (3, 70), 3, "absolute")
    (X,), (Y,) = np.nonzero(lab == 4)
    t0 = int(delay[X, Y])
    bm = pvlib.host_band_metrics(p[:, X, Y], FS, t0, coefs)
    for b in range(3):
        y = ref.filter_backwards(p[:, X, Y], t0, coefs[b]).astype(np.float64)
        assert np.array_equal(y.astype(np.float32), ref.filtered_history(p, delay, lab, coefs[b])[:, X, Y])  # (the two forms of the loop)
        assert np.array_equal(etc[3, b], y * y) and (etc[3, b, :t0] == 0.0).all() and (etc[3, b, t0:] > 0.0).any()
        for align in ALIGNS:
            r = case(pvlib, (3, 70), 3, align)[4][0][3, b]
            n = T - t0
            err = abs(float(np.float32(r["e0"])) - float(bm[b, 6]))
            print(align, b, "e0", r["e0"], "band metrics e0", bm[b, 6], "error / bound", err / (n * 2.0 ** -24 * r["e0"]))
            assert err <= n * 2.0 ** -24 * r["e0"]
    # ONSET: the same samples, moved to slot t - t0
    eo = case(pvlib, (3, 70), 3, "onset")[4][1]
    assert np.array_equal(eo[3, :, :T - t0], etc[3, :, t0:]) and (eo[3, :, T - t0:] == 0.0).all()


# (4) the clarity of hand-built curves
def test_curve_clarity_on_hand_built_curves(pvlib):
    fs = 100  # n50 = 5, n80 = 8
    e = np.zeros(12)
    e[2], e[9] = 3.0, 1.0  # j0 = 2: 3 inside both windows (slots 2 .. 6 and 2 .. 9), 1 at slot 9: late for 50 ms, early for 80 ms
    c50, c80, d50, ts = pvlib.host_zone_curve_clarity(e, fs, 2)
    assert c50 == ref.level10(3.0 / 1.0) and d50 == 0.75 and ts == ((7.0 * 1.0) / 4.0) / 100.0
    assert c80 == np.inf  # nothing at or after slot 10
    assert ref.same_doubles(np.array([c50, c80, d50, ts]), np.array(ref.clarity(e, fs, 2)))
    # t0 + n50 >= T: l50 = edc[T] = +0.0
    c50, c80, d50, ts = pvlib.host_zone_curve_clarity(e, fs, 8)
    assert c50 == np.inf and c80 == np.inf and d50 == 1.0 and ts == (1.0 / 1.0) / 100.0
    # the curve's first slot only: e50 = e80 = e0, nothing late
    one = np.zeros(30)
    one[0] = 2.5
    assert list(pvlib.host_zone_curve_clarity(one, fs, 0)) == [np.inf, np.inf, 1.0, 0.0]
    # all zero: 0 / 0 everywhere
    assert np.isnan(pvlib.host_zone_curve_clarity(np.zeros(20), fs, 0)).all()
    # a random curve against the restatement
    rng = np.random.default_rng(3)
    r = rng.random(50) * 10.0 ** (-0.1 * np.arange(50))
    for j0 in (0, 7, 49):
        assert ref.same_doubles(pvlib.host_zone_curve_clarity(r, 250, j0), np.array(ref.clarity(r, 250, j0)))
    for bad in ((r, 250, -1), (r, 250, 50), (r, 0, 0), (np.zeros(0), 250, 0)):
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: PvAmdHostZoneCurveClarity"):
            pvlib.host_zone_curve_clarity(*bad)
    assert pvlib.lib().PvAmdHostZoneCurveClarity(r.ctypes.data_as(C.POINTER(C.c_double)), 50, 250, 0, None) == -1


# (5) refusals and exports
def test_refusals(pvlib):
    p = np.zeros((6, 4, 5), np.float32)
    delay = np.zeros((4, 5), np.float32)
    lab = np.zeros((4, 5), np.uint8)
    lab[1, 1] = 3
    coefs = pvlib.host_band_coefs(FS, [50.0])
    with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: a label above nZones"):
        pvlib.host_zone_band_decay(p, delay, FS, lab, coefs, 2)
    for n in (0, 65):
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: nZones is 1 .. 64"):
            pvlib.host_zone_band_decay(p, delay, FS, np.zeros((4, 5), np.uint8), coefs, n)
    with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: align is"):
        pvlib.host_zone_band_decay(p, delay, FS, lab, coefs, 3, 2)
    for bad in (6.0, -1.0, np.nan):
        d = delay.copy()
        d[1, 1] = bad
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: an onset outside"):
            pvlib.host_zone_band_decay(p, d, FS, lab, coefs, 3)
        d[1, 1], d[0, 0] = 0.0, bad  # (an unlabelled cell's onset is not looked at)
        pvlib.host_zone_band_decay(p, d, FS, lab, coefs, 3)
    for nb in (0, 9):  # nBands outside 1 .. PVA_BANDS_MAX
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: PvAmdHostZoneBandDecay"):
            pvlib.host_zone_band_decay(p, delay, FS, lab, np.zeros((nb, 10), np.float32), 3)
    with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: PvAmdHostZoneBandDecay"):
        pvlib.host_zone_band_decay(p, delay, 0, lab, coefs, 3)
    with pytest.raises(ValueError):
        pvlib.host_zone_band_decay(p, delay[:3], FS, lab, coefs, 3)
    L = pvlib.lib()
    out = np.zeros(3, pvlib.ZONE_BAND_DECAY_DTYPE)
    fp, ub = C.POINTER(C.c_float), C.POINTER(C.c_ubyte)
    args = [p.ctypes.data_as(fp), delay.ctypes.data_as(fp), 4, 5, 6, FS, lab.ctypes.data_as(ub), 3, coefs.ctypes.data_as(fp), 1, 0,
            out.ctypes.data_as(C.c_void_p), None, None]
    assert L.PvAmdHostZoneBandDecay(*args) == 0  # (the curves are optional)
    for i in (0, 1, 6, 8, 11):  # null history, onsets, labels, coefficients, output
        a = list(args)
        a[i] = None
        assert L.PvAmdHostZoneBandDecay(*a) == -1, i
        assert pvlib.last_error().startswith("zone band decay: "), pvlib.last_error()
    rec, etc, edc = pvlib.host_zone_band_decay(p, delay, FS, lab, pvlib.host_band_coefs(FS, [20.0] * 8), 64, "onset")
    assert rec.shape == (64, 8) and etc.shape == (64, 8, 6)


def test_exports_present_and_guarded(pvlib):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the exception-guard macro of pv_capi.cpp; the out-of-scope lists no longer name what this adds"""
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
    assert pvlib.ZONE_BAND_DECAY_DTYPE.itemsize == 96 and pvlib.ZONE_BAND_DECAY_DTYPE.names == ref.DTYPE.names
    assert re.search(r"\}\s*PvAmdZoneBandDecay;\s*/\* 96 bytes \*/", hdr)
    assert callable(pvlib.Solver.zone_band_decay) and callable(pvlib.host_zone_band_decay) and callable(pvlib.host_zone_curve_clarity)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for text in (hdr, design):
        assert "per-band curves, clarity and centre time of a zone" not in re.sub(r"[\s*]+", " ", text)


def test_cli_flag_needs_zone_decay_and_bands():
    import contextlib
    import io

    from planeverb_amd import __main__ as cli
    for argv in (["x.pv", "--zone", "0,0,1,1", "--zone-decay", "onset", "--zone-band-decay"],
                 ["x.pv", "--zone", "0,0,1,1", "--bands", "250", "--zone-band-decay"]):
        err = io.StringIO()
        with pytest.raises(SystemExit), contextlib.redirect_stderr(err):
            cli.main(argv)
        assert "--zone-band-decay: needs --zone-decay and --bands" in err.getvalue()


# (6) the edge cases under ASan + UBSan, in a program of their own
def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/zone_band_decay_edges.cpp includes csrc/pv_zone_band_decay.h and runs the edge cases with exactly sized arrays;
    nothing is loaded into Python under a sanitizer"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "zone_band_decay_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", csrc, "-Wall",
                           "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "zone_band_decay_edges.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "zone_band_decay_edges: 0 failure(s)" in r.stdout, r.stdout
