"""GPU (-m gpu): the analysis records valid_mask leaves out of compare_maps, against the oracle on the SAME grid, every cell, all
eight members, bit for bit (same_bits: NaN == NaN, +inf != NaN).

* Late-onset cells: reached cells whose dry, wet or decay window runs past the end of the impulse response.  Only grids above ~250
  cells have them at 275 Hz (onsets 406 ... 434 of T = 435).  Samples past T count as zero (the oracle's PR / VX / VY; the device's
  min(onset + N, T) clamps), RT60 is +inf for a regression length <= -2 and NaN for -1 ... 1 (tests/test_oracle_edges.py pins
  that rule in float64).
* Carried records: a cell without an onset keeps the previous run's members 0-3 and 6-7 (Analyzer.cpp:160-165) and its
  listener direction is walked from that stale occlusion; the reference is the oracle chain (OracleGrid.analyze(prev=...)).

Every case asserts a floor on its late-onset / carried cell counts (measured with the oracle), so coverage cannot vanish silently.
The oracle runs on the host: ~4 s and 1.4 GB per 520^2 run, ~15 s and ~5.7 GB for the 1040^2 grid of the windowed cases.
"""
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits, valid_mask
from test_gpu_parity import NAMES, fuse_opts, random_scene

pytestmark = pytest.mark.gpu

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
EFREE = np.float32(0.0447895788)  # open grids of Mode A at 275 Hz (test_gpu_parity.test_free_grid_energy)


def cell(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def open_size(n):
    return float((n + 0.5) * DX)


def late_mask(delay, T, fs):
    return (delay < 1e30) & ~valid_mask(delay, T, fs)


def compare_all_cells(res, delay, rres, rdelay, ctx="", T=435, fs=1443):
    """all eight members of every cell and the onset map, no mask (T, fs: the grid's, for the message only)"""
    assert res.shape == rres.shape and delay.shape == rdelay.shape, ctx
    bad = ~same_bits(delay, rdelay)
    assert not bad.any(), "%s delay: %d cells differ, first %s" % (ctx, int(bad.sum()), np.argwhere(bad)[0])
    late = late_mask(rdelay, T, fs)
    for k, nm in enumerate(NAMES):
        bad = ~same_bits(res[..., k], rres[..., k])
        if bad.any():
            c = tuple(np.argwhere(bad)[0])
            raise AssertionError("%s %s: %d cells differ (%d of them late-onset, %d without an onset); first %s: %r vs %r" % (
                ctx, nm, int(bad.sum()), int((bad & late).sum()), int((bad & (rdelay > 1e30)).sum()), c, res[c + (k,)],
                rres[c + (k,)]))


# ------------------------------------------------------------------------------------------------------------------------------
# oracle chains, computed once per module: key -> list of (records, delay, late cells, carried cells) after each run
# ------------------------------------------------------------------------------------------------------------------------------
_CHAINS = {}


def oracle_chain(oracle, key, size, res, boxes, listeners, efree=None):
    if key in _CHAINS:
        return _CHAINS[key]
    o = oracle.OracleGrid(size, size, res, boxes)
    ef = oracle.free_energy(size, size, res) if efree is None else efree
    out, prev, ever = [], None, None
    for L in listeners:
        o.fdtd(L)
        r, d, _ = o.analyze(ef, L, prev=prev)
        on = d < 1e30
        carried = 0 if ever is None else int((~on & ever).sum())
        ever = on if ever is None else (ever | on)
        out.append((r, d, int(late_mask(d, o.T, o.fs).sum()), carried))
        prev = r
    o.close()
    _CHAINS[key] = out
    return out


N_OPEN = 520
OPEN_SEQ = [cell(260, 260), cell(15, 500), cell(260, 260)]  # centre, near a corner, back


def open_chain(oracle):
    return oracle_chain(oracle, "open520", open_size(N_OPEN), 275, None, OPEN_SEQ, EFREE)


def open_60_400(oracle):
    return oracle_chain(oracle, "open520_60_400", open_size(N_OPEN), 275, None, [cell(60, 400)], EFREE)


N_WIN = 1040
WIN_SEQ = [cell(300, 700), cell(1000, 40)]  # the second listener lies outside the first run's history window


def window_chain(oracle):
    return oracle_chain(oracle, "open1040", open_size(N_WIN), 275, None, WIN_SEQ, EFREE)


N_SMALL = 254
SMALL_SEQ = [cell(20, 20), cell(230, 230)]


def small_chain(oracle):
    return oracle_chain(oracle, "open254", open_size(N_SMALL), 275, None, SMALL_SEQ, EFREE)


FLOOR_SEQ = [(3.0, 0.0, 3.0), (22.0, 0.0, 22.0), (12.5, 0.0, 5.0), (3.0, 0.0, 3.0), (20.0, 0.0, 12.0)]


def floor_chain(oracle, pvlib):
    return oracle_chain(oracle, "floor375", 25.0, 375, pvlib.load_pv(os.path.join(SCENES, "FloorPlanScene.pv")), FLOOR_SEQ)


def run_and_compare(s, listeners, chain, ctx):
    """one solver runs the whole sequence; every map after every run"""
    for i, (L, (r, d, _, _)) in enumerate(zip(listeners, chain)):
        s.run(L)
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "%s run %d" % (ctx, i), s.T, s.fs)


# ------------------------------------------------------------------------------------------------------------------------------
# a. open 520^2: every form of the analysis on grids whose history window is the whole grid
# ------------------------------------------------------------------------------------------------------------------------------
OPTS_A = [dict(), dict(rt60_lanes=16), dict(rt60_lanes=4), dict(rt60_lanes=1), dict(dense_history=1), "near_box_0",
          dict(lazy_far_cells=1), dict(lazy_far_cells=0)]


@pytest.mark.parametrize("opts", OPTS_A, ids=lambda o: o if isinstance(o, str) else ",".join("%s=%s" % kv for kv in o.items()) or "default")
def test_late_onset_open_520(pvlib, oracle, monkeypatch, opts):
    """listener at the centre (15 680 late-onset cells: 14 436 with RT60 = +inf, 1 244 NaN) and at cell (60, 400) (12 384)"""
    centre = open_chain(oracle)[0]
    side = open_60_400(oracle)[0]
    assert centre[2] >= 15000 and side[2] >= 10000
    assert np.isposinf(centre[0][..., 2]).sum() >= 14000 and np.isnan(centre[0][..., 2]).sum() >= 1200
    if opts == "near_box_0":
        monkeypatch.setenv("PLANEVERB_AMD_NEAR_BOX", "0")
        opts = {}
    size = open_size(N_OPEN)
    for L, (r, d, _, _) in ((OPEN_SEQ[0], centre), (cell(60, 400), side)):
        with pvlib.Solver(size, size, 275, **opts) as s:
            assert (s.gx, s.gy, s.T) == (N_OPEN, N_OPEN, 435) and np.float32(s.efree) == EFREE
            s.run(L)
            got, gd = s.results()
            compare_all_cells(got, gd, r, d, "520^2 %r listener %r" % (opts, L))


def _late_emitters(r, d, T, fs):
    """emitters (metres) at late-band cells with regression lengths -28, -2, -1, 0, 1, 2, plus ordinary and unreached cells"""
    n_dry, n_cut = int(np.float32(0.01) * np.float32(fs)), int(np.float32(0.01) * np.float32(fs))
    picks = []
    for rn in (-28, -2, -1, 0, 1, 2):
        onset = (T - n_cut) - (n_dry + 1) - rn
        cand = np.argwhere(d == onset)
        assert len(cand) > 0, rn
        picks += [tuple(cand[0]), tuple(cand[len(cand) // 2])]
    for onset in (3, 120, 300):
        picks.append(tuple(np.argwhere(d == onset)[0]))
    picks.append(tuple(np.argwhere(d > 1e30)[0]))
    cells = np.array(picks)
    return [cell(int(x), int(y)) for x, y in cells], cells


def test_late_onset_outputs_get_output_and_queries(pvlib, oracle):
    """f. the user-facing path: PvAmdGetOutput and the output queries for emitters in the late band equal the oracle's records bit
    for bit, +inf and NaN RT60 included"""
    r, d, _, _ = open_chain(oracle)[0]
    E, cells = _late_emitters(r, d, 435, 1443)
    want = r[cells[:, 0], cells[:, 1]]
    assert np.isposinf(want[:, 2]).sum() >= 4 and np.isnan(want[:, 2]).sum() >= 6
    size = open_size(N_OPEN)
    with pvlib.Solver(size, size, 275) as s:
        s.set_output_queries(E)
        s.run(OPEN_SEQ[0])
        q = s.queried_outputs()
        for i, e in enumerate(E):
            assert same_bits(s.get_output(e).as_array(), want[i]).all(), "get_output %s: %r vs %r" % (cells[i], s.get_output(e).as_array(), want[i])
            assert same_bits(q[i], want[i]).all(), "query %s: %r vs %r" % (cells[i], q[i], want[i])


# ------------------------------------------------------------------------------------------------------------------------------
# b. a history window smaller than the grid
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(), dict(lazy_far_cells=0), dict(dense_history=1)],
                         ids=["default", "lazy_far_cells=0", "dense_history=1"])
def test_late_onset_windowed_history_1040(pvlib, oracle, opts):
    """open 1040^2, listener at cell (300, 700): the (2 (T + 2 + K) + 1)-cell history window plus a tile is smaller than the grid, so
    the map has far cells (outside the window) and a window edge.  The oracle on this grid holds T x 1041^2 x 3 floats of history
    (~5.7 GB of host memory) and takes ~15 s."""
    r, d, nlate, _ = window_chain(oracle)[0]
    assert nlate >= 10000
    size = open_size(N_WIN)
    with pvlib.Solver(size, size, 275, **opts) as s:
        assert (s.gx, s.gy, s.T) == (N_WIN, N_WIN, 435) and np.float32(s.efree) == EFREE
        if not opts.get("dense_history"):
            assert s.info.histRows < s.gx, (s.info.histRows, s.gx)
        s.run(WIN_SEQ[0])
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "1040^2 %r" % (opts,))


# ------------------------------------------------------------------------------------------------------------------------------
# c. launch-bound grids: the resident kernel, the replayed graph, the fused analysis
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["default", "resident", "graph", "fused"])
def test_late_onset_launch_bound_254(pvlib, request, oracle, form):
    """open 254^2, listener at cell (20, 20): 1 968 late-onset cells"""
    r, d, nlate, _ = small_chain(oracle)[0]
    assert nlate >= 1900
    opts = {"default": {}, "resident": dict(resident_kernel=1, steps_per_launch=12, tile_rows=12),
            "graph": dict(resident_kernel=2), "fused": dict(fused_analysis=1)}[form]
    lib = request.getfixturevalue("pvlib_exp") if form == "fused" else pvlib
    size = open_size(N_SMALL)
    with lib.Solver(size, size, 275, **opts) as s:
        if form == "resident":
            assert s.info.residentKernel == 1
        if form == "graph":
            assert s.info.residentKernel == 0
        s.run(SMALL_SEQ[0])
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "254^2 " + form)


# ------------------------------------------------------------------------------------------------------------------------------
# d. walls
# ------------------------------------------------------------------------------------------------------------------------------
def test_late_onset_behind_walls_180m(pvlib, oracle):
    """random_scene (120 walls) in a 180 m grid (504^2): late-onset cells in the shadows of the walls and at the reached region's
    frontier (seed 11: 13 404 of them, finite history; the oracle's FreeGrid run on this size adds ~4 s)"""
    size = 180.0
    rng = np.random.default_rng(11)
    boxes = random_scene(rng, size, 120)
    L = (rng.uniform(60, 120), 0.0, rng.uniform(60, 120))
    r, d, nlate, _ = oracle_chain(oracle, "walls180", size, 275, boxes, [L])[0]
    assert nlate >= 10000
    with pvlib.Solver(size, size, 275) as s:
        assert np.float32(s.efree) == np.float32(oracle.free_energy(size, size, 275))  # (the centre-cell quirk of 40 m: not EFREE)
        for b in boxes:
            s.add_geometry(b)
        s.run(L)
        got, gd = s.results()
        assert np.isfinite(s.fields()[0]).all()
        compare_all_cells(got, gd, r, d, "walls")


# ------------------------------------------------------------------------------------------------------------------------------
# e. sparse-emitter mode
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [1, 0])
def test_late_onset_sparse_emitter_mode_520(pvlib, oracle, fuse):
    """streaming_analysis = 1: the forward outputs (onset, occlusion, lowpass, both directions) of every cell, and wet gain / RT60
    at registered emitters in the late band (regression lengths -28, -2, -1, 0, 1, 2) and elsewhere; zero wet gain / RT60 at every
    other cell"""
    r, d, _, _ = open_chain(oracle)[0]
    E, cells = _late_emitters(r, d, 435, 1443)
    size = open_size(N_OPEN)
    with pvlib.Solver(size, size, 275, streaming_analysis=1, **fuse_opts(fuse)) as s:
        assert s.info.streamFuse == fuse
        s.set_emitters(E)
        s.run(OPEN_SEQ[0])
        got, gd = s.results()
        em = np.zeros(gd.shape, bool)
        em[cells[:, 0], cells[:, 1]] = True
        want = r.copy()
        want[..., 1][~em] = 0
        want[..., 2][~em] = 0
        compare_all_cells(got, gd, want, d, "streaming fuse %d" % fuse)
        for i, e in enumerate(E):
            assert same_bits(s.get_output(e).as_array(), r[cells[i, 0], cells[i, 1]]).all(), "emitter %s" % cells[i]


# ------------------------------------------------------------------------------------------------------------------------------
# g. carried records: sequences on one solver and on two solvers taking turns, against the oracle chain
# ------------------------------------------------------------------------------------------------------------------------------
def _taking_turns(lib, size, res, listeners, chain, ctx, prepare=None, **opts):
    """PvAmdRunAsyncAfter: iterations alternate between two solvers, each enqueued while the previous one is in flight
    (Solver::run's carryFrom copies the other solver's records into cells without an onset)"""
    with lib.Solver(size, size, res, **opts) as a, lib.Solver(size, size, res, **opts) as b:
        for s in (a, b):
            if prepare:
                prepare(s)
        pair, prev, pending = (a, b), None, []

        def collect_oldest():
            t, j = pending.pop(0)
            t.sync()
            got, gd = t.results()
            compare_all_cells(got, gd, chain[j][0], chain[j][1], "%s iteration %d" % (ctx, j), t.T, t.fs)

        for i, L in enumerate(listeners):
            s = pair[i & 1]
            if prev is None:
                s.run_async(L)
            else:
                s.run_async_after(prev, L)  # (prev's run is still in flight)
            prev = s
            pending.append((s, i))
            if len(pending) == 2:
                collect_oldest()
        while pending:
            collect_oldest()


@pytest.mark.parametrize("turns", [False, True], ids=["one_solver", "two_solvers"])
def test_carried_records_open_520(pvlib, oracle, turns):
    """open 520^2: centre, near a corner, back to the centre"""
    chain = open_chain(oracle)
    assert chain[1][3] >= 170000 and chain[2][3] >= 6000 and chain[0][2] >= 15000
    size = open_size(N_OPEN)
    if turns:
        _taking_turns(pvlib, size, 275, OPEN_SEQ, chain, "520^2 turns")
    else:
        with pvlib.Solver(size, size, 275) as s:
            run_and_compare(s, OPEN_SEQ, chain, "520^2 chain")


@pytest.mark.parametrize("turns", [False, True], ids=["one_solver", "two_solvers"])
def test_carried_records_windowed_1040(pvlib, oracle, turns):
    """open 1040^2 (history window smaller than the grid; ~5.7 GB of host memory for the oracle): the second listener lies outside
    the first run's window, so the first run's records outside the second run's window are carried too"""
    chain = window_chain(oracle)
    assert chain[0][2] >= 10000 and chain[1][3] >= 100000
    size = open_size(N_WIN)
    if turns:
        _taking_turns(pvlib, size, 275, WIN_SEQ, chain, "1040^2 turns")
    else:
        with pvlib.Solver(size, size, 275) as s:
            run_and_compare(s, WIN_SEQ, chain, "1040^2 chain")


@pytest.mark.parametrize("form", ["one_solver", "two_solvers", "fused_two_solvers"])
def test_carried_records_floor_plan(pvlib, request, oracle, form):
    """FloorPlanScene at 375 Hz, the listener moving between closed rooms: each room keeps the records of the last run that reached
    it"""
    chain = floor_chain(oracle, pvlib)
    assert max(c[3] for c in chain) >= 900
    scene = os.path.join(SCENES, "FloorPlanScene.pv")
    if form == "one_solver":
        with pvlib.Solver(25.0, 25.0, 375) as s:
            s.load_scene(scene)
            run_and_compare(s, FLOOR_SEQ, chain, "floor plan")
    else:
        lib = request.getfixturevalue("pvlib_exp") if form.startswith("fused") else pvlib
        opts = dict(fused_analysis=1) if form.startswith("fused") else {}
        _taking_turns(lib, 25.0, 375, FLOOR_SEQ, chain, "floor plan " + form, prepare=lambda s: s.load_scene(scene), **opts)


@pytest.mark.parametrize("form", ["one_solver", "two_solvers", "fused_one_solver", "fused_two_solvers"])
def test_carried_records_launch_bound_254(pvlib, request, oracle, form):
    """open 254^2, listener near one corner, then near the other: 1 968 late-onset cells in the first run, carried cells in the
    second, and cells at the second run's frontier whose listener direction depends on the stale occlusion
    (tests/test_oracle_edges.py)"""
    chain = small_chain(oracle)
    assert chain[0][2] >= 1900 and chain[1][3] >= 1000
    lib = request.getfixturevalue("pvlib_exp") if form.startswith("fused") else pvlib
    opts = dict(fused_analysis=1) if form.startswith("fused") else {}
    size = open_size(N_SMALL)
    if form.endswith("two_solvers"):
        _taking_turns(lib, size, 275, SMALL_SEQ, chain, "254^2 " + form, **opts)
    else:
        with lib.Solver(size, size, 275, **opts) as s:
            run_and_compare(s, SMALL_SEQ, chain, "254^2 " + form)
