"""GPU (-m gpu): the analysis passes at the run lengths of tests/_run_lengths.py -- runs shorter than a chunk of steps, than the
ring of chunks in flight, than the tail, the 50 / 80 ms limits, a slot, a window or a slice; runs that end exactly on a chunk's
edge; runs longer than the grid's own T.  Every kernel that reads a run's history walks it in chunks with a ring of loads in
flight, and a kernel that is wrong only when its last chunk is exactly full, when T < NB S, or when the tail is longer than the
run is wrong at none of the lengths the other test files use (100, 160, 200, 300, 435).

The grid is the 24 x 50 grid of tests/test_gpu_non_square.py (3 x 2 tiles of 12 x 40, 1086 air cells, its walls and listeners).
The expected values are those of the kinds' own tests: the host restatements (held to their numpy restatements at the same
lengths, without a device, in tests/test_host_run_lengths.py), the numpy restatements, the ring oracle, and a solver that keeps
its history for the sparse-emitter mode.  Every comparison is bit for bit, NaN by position; nothing here is timed."""
import numpy as np
import pytest

import _adversarial as adv
import _arrays_ref
import _run_lengths as rl
import _zone_decay_ref as zref
import test_gpu_analysis_maps as maps
import test_gpu_arrays as ga
import test_gpu_emitter_records as er
import test_gpu_injected_history as inj
import test_gpu_non_square as ns
import test_gpu_stream_zone_decay as szd
import test_gpu_waterfall as gw
import test_gpu_zone_band_decay as zbd
import test_gpu_zone_decay as zd
import test_gpu_zone_stats as zs
from _rect_ref import listeners_rect
from conftest import bits, same_bits
from test_gpu_layer import cell_of
from test_gpu_modulation import THIRDS8
from test_gpu_parity import fuse_opts
from test_gpu_query_records import check_against_maps, records
from test_gpu_spectrum import BINS

pytestmark = pytest.mark.gpu

SMALL = ns.SMALL
SEED = inj.SEED
LISTENER = ns.listeners(SMALL)[0]
NAMES = ["occlusion", "wetGain", "rt60", "lowpass", "dirX", "dirY", "srcDirX", "srcDirY"]


def lengths(which):
    return pytest.mark.parametrize("T", which, ids=rl.ident)


def make(pvlib, T, **opts):
    s = ns.solver(pvlib, SMALL, num_steps=T, **opts)
    assert s.fs == rl.FS and s.T == T
    if "steps_per_launch" not in opts:
        assert (s.info.stepsPerLaunch, s.info.tileRows, s.info.tileCols) == (rl.K, 12, 40)
    return s


def settings(s):
    """eight third-octave bands, 32 bins, sixteen 5 ms slots, the lobe windows at 10 and 80 ms: windows and slots past a short run"""
    s.set_bands(THIRDS8, 3)
    s.set_modulation_frequencies(None)
    s.set_spectrum_bins(BINS[32])
    s.set_echogram(*inj.SLOTS16)
    s.set_lobe_windows(maps.EDGES)
    return s


def reached_by_oracle(oracle, T):
    """the cells the first run of the oracle's chain reaches in T steps; an extended run reaches what the grid's own T reaches
    (every air cell: the front has passed the whole grid by step 63)"""
    w = ns.ref_chain(oracle, SMALL, steps=min(T, rl.GRID_T))[0]
    assert T <= rl.GRID_T or w["reached"] == w["air"]
    return w["reached"]


# ------------------------------------------------------------------------------------------------------------------------------
# (a) the nine per-cell kinds on the injected history, every reached cell, every length
# ------------------------------------------------------------------------------------------------------------------------------
@lengths(rl.ALL)
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_nine_kinds(pvlib, oracle, T):
    """the six pressure kinds against the host restatements, the three velocity kinds against the numpy restatements on
    impulse_response, on every reached cell of the adversarial history; records of cells without an onset are NaN.  No setter and
    no compute call refuses a short run: a window, slot or limit past the run's end is an empty sum (include/planeverb_amd.h)"""
    n = reached_by_oracle(oracle, T)
    with settings(make(pvlib, T)) as s:
        if n == 0:  # (one step: the pulse has not left the listener's cell, no cell has an onset)
            s.run(LISTENER)
            _, _, delay = adv.inject(s, SEED)
            assert not (delay < adv.NO_ONSET).any()
            for k in maps.KINDS:
                assert maps.compute(s, k) > 0
                assert np.isnan(maps.whole(s, k)).all(), k["name"]
            return
        r = inj.analyse(pvlib, s, LISTENER, "T = %d" % T, inj.SLOTS16, maps.EDGES, every_cell=True)
        reached = r["delay"] < adv.NO_ONSET
        assert reached.sum() == n, (reached.sum(), n)
        per_family = [int(((r["fam"] == f) & reached).sum()) for f in range(len(adv.FAMILIES))]
        print("run lengths: T = %d, %d cells reached, per family %s" % (T, n, per_family))
        assert T < rl.TAIL - 1 or min(per_family) >= 2, per_family
        assert r["maps"]["band_metrics"].shape[2:] == (8, 12) and r["maps"]["spectrum"].shape[2:] == (32, 3)
        assert r["maps"]["echogram"].shape[2:] == (49,) and r["maps"]["lobes"].shape[2:] == (16,)


# ------------------------------------------------------------------------------------------------------------------------------
# (b) the core outputs against the ring oracle, every length the oracle takes
# ------------------------------------------------------------------------------------------------------------------------------
CORE_FORMS = {"default": dict(), "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}


@pytest.mark.parametrize("form", list(CORE_FORMS))
@lengths(rl.WITHIN)
def test_core_outputs(pvlib, oracle, T, form):
    """the final fields, recorded planes, impulse responses beside the edges, all eight members of every cell and the onset map
    after each of the two chained listeners: at short T most cells of the second run have no onset and carry the first run's
    record.  'graph' steps in launches of K steps (the small-grid kernel of the default takes a run in one launch)"""
    chain = ns.ref_chain(oracle, SMALL, steps=T)
    with make(pvlib, T, **CORE_FORMS[form]) as s:
        ns.check_efree(s, oracle, SMALL)
        if chain[0]["reached"]:
            ns.run_chain(s, SMALL, chain, "run length %d %s" % (T, form))
        else:  # (one step: run_chain insists on a reached cell)
            assert T == 1
            for k, (L, w) in enumerate(zip(ns.listeners(SMALL), chain)):
                s.run(L)
                ns.check(s, w, "run length 1 %s run %d" % (form, k))
                assert w["reached"] == 0 and not (s.results()[1] < adv.NO_ONSET).any()
        # (the oracle's own figures: up to 73 steps the second run leaves cells of the first without an onset -- 351 of them at 27)
        carried = int(((chain[0]["d"] < 1e30) & ~(chain[1]["d"] < 1e30)).sum())
        assert (carried > 0) == (2 <= T < rl.HALF_RING - 1), (T, carried)


# ------------------------------------------------------------------------------------------------------------------------------
# (c) the zone reductions around S, tailN, the 64-slot chunk and the 256-thread row group
# ------------------------------------------------------------------------------------------------------------------------------
def injected(pvlib, s):
    """run, inject: (p [T, gx, gy], family [gx, gy], onset map, reached)"""
    s.run(LISTENER)
    new, fam, delay = adv.inject(s, SEED)
    return np.ascontiguousarray(new[:, :s.gx, :s.gy]), fam[:s.gx, :s.gy], delay, delay < adv.NO_ONSET


def five_zones(fam, reached):
    """1 .. 3 scattered over the finite cells, every poisoned cell in zone 1, 4 = a block around the listener, 5 = no cell"""
    lab = np.random.default_rng(SEED).integers(0, 4, fam.shape).astype(np.uint8)
    lc = listeners_rect(*SMALL)[0]
    lab[lc[0] - 2:lc[0] + 3, lc[1] - 2:lc[1] + 4] = 4
    lab[fam == adv.NONFINITE] = 1
    assert ((lab == 4) & reached).any()
    return lab


@lengths(rl.ZONES)
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_zone_reductions(pvlib, T):
    """the zone decay in both alignments, the zone band decay, and the zone statistics of decay_times and room_metrics against
    their host restatements on the injected planes"""
    with make(pvlib, T) as s:
        s.set_bands(zbd.OCTAVES[:2])
        p, fam, delay, reached = injected(pvlib, s)
        lab = five_zones(fam, reached)
        s.set_zones(lab, 5)
        ctx = "T = %d" % T
        got, _, _ = zd.check(pvlib, s, lab, 5, ctx, p=p)
        poisoned = bool(((fam == adv.NONFINITE) & reached).any())
        assert poisoned == (T >= rl.S)  # (the first poisoned cell is reached at step 7)
        for rec, etc, edc in got.values():
            assert etc.shape == (5, T) and rec["n_cells"][4] == 0 and rec["t_first"][4] == -1 and (etc[4] == 0.0).all()
            assert np.isfinite(etc[1:]).all() and np.isfinite(etc[0]).all() == (not poisoned)
            assert rec["n_cells"][3] > 0 and (etc[3] > 0).any()
        zbd.check(pvlib, s, lab, 5, ctx, p=p)
        for name in ("decay_times", "room_metrics"):
            k = maps.BY_NAME[name]
            assert maps.compute(s, k) > 0
            st, m = zs.check(pvlib, s, k, lab, 5, ctx)
            assert np.array_equal(np.isnan(m).all(axis=-1), ~reached)
            flat = st.reshape(5, -1)
            assert (flat["n_finite"][4] == 0).all() and (flat["n_nan"][4] == 0).all() and flat["n_finite"][3].max() > 0


# ------------------------------------------------------------------------------------------------------------------------------
# (d) waterfalls and source arrays
# ------------------------------------------------------------------------------------------------------------------------------
def pick_cells(fam, reached, per_family):
    cells = []
    for f in range(len(adv.FAMILIES)):
        idx = np.argwhere((fam == f) & reached)
        cells += [tuple(int(v) for v in idx[i]) for i in sorted(set(np.linspace(0, len(idx) - 1, per_family).astype(int)))] if len(idx) else []
    return cells


@lengths(rl.RECEIVERS)
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_waterfalls(pvlib, T):
    """receivers on reached cells of every family of the injected history (and one cell without an onset), one bin and one slice,
    then 65 bins and sixteen 15-step slices -- slices past T wherever T < 240 -- against the host restatement"""
    with make(pvlib, T) as s:
        p, fam, delay, reached = injected(pvlib, s)
        cells = pick_cells(fam, reached, 2)
        silent = tuple(int(v) for v in np.argwhere(~reached)[0])
        pulse = s.pulse()
        assert len(pulse) == T
        assert len(cells) == (2 * len(adv.FAMILIES) if T > 1 else 0)  # (one step: no cell has an onset)
        for n, m in ((1, 1), (65, 16)):
            hz = gw.bins_of(n, s.fs)
            s.set_waterfall(hz, 0.0105, m)
            assert s.waterfall_setting()[2] == 15
            assert s.compute_waterfall(gw.positions(cells + [silent])) > 0
            got = s.waterfall()
            assert got["level"].shape == (len(cells) + 1, m, n)
            for i, c in enumerate(cells):
                want = pvlib.host_waterfall(np.ascontiguousarray(p[:, c[0], c[1]]), s.fs, int(delay[c]), hz, 0.0105, m, pulse)
                for k in gw.KEYS:
                    assert same_bits(got[k][i], want[k][0]).all(), (T, n, m, adv.describe(fam, c), k)
                assert got["slices"][i] == min(m, (T - 1 - int(delay[c])) // 15 + 1)
            for k in gw.KEYS:
                assert np.isnan(got[k][-1]).all(), k


@lengths(rl.RECEIVERS)
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_source_arrays(pvlib, T):
    """arrays on reached finite cells of the injected history, both interpolations, against the numpy restatement of the mix and
    the six host kinds on it: the identity, a cancelling pair, fractional delays, a member delayed by 0.6 T, one whose largest tap
    passes T - 1 (where the tap rule takes them: it refuses a delay of T steps or more, and the refusal is asserted)"""
    with make(pvlib, T) as s:
        ga.configure(pvlib, s)
        p, fam, delay, reached = injected(pvlib, s)
        hist = ga.history(s)
        finite = np.isfinite(hist).all(axis=0)[:s.gx, :s.gy]
        cells = [c for c in pick_cells(fam, reached & finite, 2)]
        if not cells:  # (one step: no cell has an onset; the mix of silent members is silence)
            assert T == 1
            cells = [listeners_rect(*SMALL)[0], (3, 30)]
        c = lambda i: cells[i % len(cells)]  # noqa: E731
        dl = lambda k: float(np.float32(k / s.fs))  # noqa: E731
        with pytest.raises(pvlib.PlaneverbError, match="^arrays:"):
            s.set_arrays(ga.members_at([[(c(0), 1.0, dl(T + 0.5))]]))
        for interp in (pvlib.ARRAY_LAGRANGE3, pvlib.ARRAY_NEAREST):
            arrays = [[(c(0), 1.0, 0.0)], [(c(1), 0.7, 0.0), (c(1), -0.7, 0.0)], [(c(2), 0.8, 0.0), (c(3), -0.5, dl(7.3) if T > 9 else 0.0)],
                      [(c(i), 0.1 * (i + 1), (0.0, dl(min(5, T - 1)))[i % 2]) for i in range(min(len(cells), 17))]]
            for gain, d in ((0.9, dl(0.6 * T)), (0.5, dl(T - 1.5))):
                try:
                    _arrays_ref.taps(s.fs, T, gain, d, interp)
                    arrays.append([(c(4), 1.0, 0.0), (c(5), gain, d)])
                except _arrays_ref.Refused:
                    with pytest.raises(pvlib.PlaneverbError, match="^arrays:"):
                        s.set_arrays(ga.members_at([[(c(5), gain, d)]]), interp)
            assert len(arrays) == 6 or T < 4
            s.set_arrays(ga.members_at(arrays), interp)
            assert s.compute_arrays() > 0
            want = ga.restate(s, hist, arrays, interp)
            ga.check(pvlib, s, want, "T = %d interp=%d" % (T, interp))
            assert not (bits(want[1][0]) != 0).any() and want[1][1] == _arrays_ref.FLT_MAX  # (the cancelling pair)
            if len(arrays) == 6 and interp == pvlib.ARRAY_LAGRANGE3:
                assert max(s.array_taps(5)[1]) >= T  # (a tap past T - 1)


# ------------------------------------------------------------------------------------------------------------------------------
# (e) in-run records and the sparse-emitter mode against a solver that keeps its history
# ------------------------------------------------------------------------------------------------------------------------------
CELLS = [(12, 19), (13, 19), (12, 21), (10, 22), (12, 40), (11, 39), (2, 45), (22, 30)]  # the listener's cell, its neighbours, tile edges, far corners
_FULL = {}


def full_history(pvlib, T):
    """the solver that keeps its history, once per length: whole maps, traces, zone curves, array responses and records"""
    if T not in _FULL:
        with er.configure(make(pvlib, T)) as s:
            ga.configure(pvlib, s)
            air = s.material()[0][:s.gx, :s.gy] != 0
            cells = [c for c in CELLS if air[c]]
            assert len(cells) >= 6
            lab = np.random.default_rng(SEED).integers(0, 4, (s.gx, s.gy)).astype(np.uint8)
            lab[10:15, 17:23] = 4
            s.set_zones(lab, 5)
            pos = [cell_of(*c) for c in cells]
            s.set_record_queries(pos)
            s.set_query_records(pvlib.QREC_ALL)
            s.run(LISTENER)
            res, delay = s.results()
            # the in-run records of the full-history solver are the whole maps at the queried cells
            recs = records(s, pvlib, pvlib.QREC_ALL)
            check_against_maps(pvlib, s, ns.metres(SMALL), pos, pvlib.QREC_ALL, recs, "record queries T = %d" % T)
            w = {"delay": delay, "res": res, "cells": cells, "lab": lab, "T": T}
            for sp, k in er.selected(pvlib, pvlib.QREC_ALL, pvlib.QSPEC_ALL):
                w[(sp, k)] = er.whole_maps(pvlib)[(sp, k)](s)
            w["ir"] = dict((c, s.impulse_response(*c)) for c in cells)
            w["curves"] = s.zone_decay("absolute", curves=True)
            arrays = arrays_of(cells, s.fs, T)
            s.set_arrays(ga.members_at(arrays))
            s.compute_arrays()
            w["arrays"] = arrays
            w["array_y"] = [(s.array_response(i), s.array_onsets()[i]) for i in range(len(arrays))]
            w["array_rec"] = dict(((sp, k), s.array_records(k, spectral=sp)) for sp, k, _ in ga.kinds_of(pvlib))
        _FULL[T] = w
    return _FULL[T]


def arrays_of(cells, fs, T):
    dl = lambda k: float(np.float32(k / fs))  # noqa: E731
    arrays = [[(cells[0], 1.0, 0.0)], [(cells[1], 0.7, 0.0), (cells[1], -0.7, 0.0)], [(cells[2], 0.8, 0.0), (cells[3], -0.5, 0.0)]]
    if T >= 4:
        arrays += [[(cells[0], 0.5, dl(1.6)), (cells[4], 1.0, 0.0)], [(cells[1], 1.0, dl(0.6 * T))], [(cells[2], 1.0, 0.0), (cells[3], 0.5, dl(T - 1.5))]]
    return arrays


@pytest.mark.parametrize("fuse", [0, 1])
@lengths(rl.IN_RUN)
def test_sparse_emitter_mode(pvlib, T, fuse):
    """emitter records of all nine kinds, the emitters' traces, the zones' decay curves, the array responses, onsets and records
    of a sparse-emitter solver against the solver that keeps its history.  The accumulate passes take halfRing = min(roundUp(T, K),
    8 K) steps each (K = 12 with fuse 0: one pass up to 96 steps, three at 193; K = 8 with fuse 1); timings() does not count
    the passes, so their number is not asserted"""
    ref = full_history(pvlib, T)
    cells = ref["cells"]
    with er.configure(make(pvlib, T, streaming_analysis=1, **fuse_opts(fuse))) as st:
        assert st.info.streamFuse == fuse and st.info.stepsPerLaunch == (8 if fuse else rl.K)
        ga.configure(pvlib, st)
        st.set_emitters([cell_of(*c) for c in cells])
        assert [tuple(c) for c in st.emitter_cells()] == cells
        st.set_emitter_records(pvlib.QREC_ALL, pvlib.QSPEC_ALL)
        st.set_zones(ref["lab"], 5)
        st.set_zone_curves(True)
        st.set_arrays(ga.members_at(ref["arrays"]))
        st.run(LISTENER)
        ctx = "T = %d fuse %d" % (T, fuse)
        er.check(pvlib, st, ref, pvlib.QREC_ALL, pvlib.QSPEC_ALL, ctx)
        for i, c in enumerate(cells):
            tr = st.emitter_trace(i)
            assert tr.shape == (T,) and same_bits(tr, ref["ir"][c][:, 0]).all(), (ctx, c)
        szd.same_curves(szd.curves(st), ref["curves"], ctx)
        assert st.compute_arrays() > 0
        for i, (y, on) in enumerate(ref["array_y"]):
            assert same_bits(st.array_response(i), y).all(), (ctx, i)
        assert np.array_equal(bits(st.array_onsets()), bits(np.array([on for _, on in ref["array_y"]], np.float32)))
        for sp, k, _ in ga.kinds_of(pvlib):
            assert same_bits(st.array_records(k, spectral=sp), ref["array_rec"][(sp, k)]).all(), (ctx, sp, k)
        on = np.array([ref["delay"][c] < er.NO_ONSET for c in cells])
        assert on.any() == (T >= 2) and (on.all() == (T >= rl.HALF_RING - 1))


# ------------------------------------------------------------------------------------------------------------------------------
# (f) extended runs: num_steps above the grid's own T
# ------------------------------------------------------------------------------------------------------------------------------
_OWN = {}


def own_length(pvlib):
    if not _OWN:
        with make(pvlib, rl.GRID_T) as s:
            s.run(LISTENER)
            _OWN.update(hist=adv.history(s), res=s.results()[0], delay=s.results()[1], pulse=s.pulse())
    return _OWN


@lengths(rl.EXTENDED)
def test_extended_runs(pvlib, T):
    """No oracle exists here: the ring (tests/_rect_ref.RectRing) refuses more steps than the grid's own T.  What an extended run
    must keep of the grid's own: the recorded planes 0 .. T_grid - 1, the pulse table (zero from T_grid on: nothing is injected
    after it), the onset map (every onset lies below T_grid), and every member of the results but rt60 -- occlusion, lowpass and the
    four direction members read [onset, onset + nDry), wetGain reads nWet steps behind them, and on this grid every such window
    ends below T_grid; rt60 regresses up to T - nCut and so depends on T.  test_nine_kinds holds the nine kinds to their
    restatements on an extended history"""
    own = own_length(pvlib)
    with make(pvlib, T) as s:
        s.run(LISTENER)
        pulse = s.pulse()
        assert pulse.shape == (T,) and same_bits(pulse[:rl.GRID_T], own["pulse"]).all() and not pulse[rl.GRID_T:].any()
        assert np.abs(own["pulse"]).max() > 0
        hist = adv.history(s)
        assert hist.shape == (T,) + own["hist"].shape[1:]
        bad = ~same_bits(hist[:rl.GRID_T], own["hist"])
        assert not bad.any(), "T = %d: %d recorded samples differ from the grid's own run, first at %s" % (T, bad.sum(), np.argwhere(bad)[0])
        assert np.abs(hist[rl.GRID_T:]).max() > 0  # (the field goes on ringing)
        res, delay = s.results()
        assert same_bits(delay, own["delay"]).all()
        reached = delay < adv.NO_ONSET
        assert delay[reached].max() + rl.TAIL + 1 + rl.N80 <= rl.GRID_T
        for k, name in enumerate(NAMES):
            if name != "rt60":
                assert same_bits(res[..., k], own["res"][..., k]).all(), (T, name)
        assert not same_bits(res[..., 2], own["res"][..., 2]).all()
