"""GPU (-m gpu): per-cell directional energy lobes (PvAmdComputeLobes; pv_lobes.hip).

The expected values come from the numpy restatement (tests/_lobes_ref.py, written from the definition in
include/planeverb_amd.h) fed with pressure AND velocity from somewhere else than the pass under test: the oracle's recorded
pr / vx / vy cubes on the 70^2 presets, and the solver's own impulse_response(cx, cy) (pv_ir_kernel: one cell on one lane, from
the tile's first recorded sample) everywhere else, with the run's own onset map (results()[1]).  Tolerance 0: conftest.same_bits,
NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _lobes_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_lateral import check_cells, preset_solver
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history
from test_host_lateral import oracle_run
from test_host_lobes import EDGES5, WINDOWS, scene_ref

pytestmark = pytest.mark.gpu


def floats(edges):
    return 1 + 5 * (len(edges or ref.DEFAULT_EDGES) + 1)


def responses(s, cells):
    """impulse_response of the given result cells [(x, y)]: float32 [T, len(cells), 3]"""
    return np.stack([s.impulse_response(int(x), int(y)) for x, y in cells], axis=1)


def expected_at(s, cells, delay, edges=None, irs=None):
    """the restatement on impulse_response of the given result cells: float32 [len(cells), 1 + 5 nW]"""
    irs = responses(s, cells) if irs is None else irs
    d = np.array([delay[x, y] for x, y in cells], np.float32)
    return ref.lobes(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs, edges)


def expected_map(s, delay, edges=None):
    """the same for every reached cell of the map: float32 [gx, gy, 1 + 5 nW], NaN without an onset"""
    out = np.full(delay.shape + (floats(edges),), np.nan, np.float32)
    cells = np.argwhere(delay < ref.NO_ONSET)
    if len(cells):
        out[cells[:, 0], cells[:, 1]] = expected_at(s, cells, delay, edges)
    return out


def check_nan_pattern(got, reached, ctx):
    """NaN records on exactly the unreached cells; every value of a reached cell is a number, window 0 has energy"""
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached), ctx
    assert np.array_equal(np.isnan(got).any(axis=-1), ~reached), ctx
    assert np.isfinite(got[reached]).all(), ctx
    assert (got[..., 0][reached] >= 1).all() and (got[..., 1][reached] > 0).all(), ctx


def check_map(got, want, delay, T, ctx):
    reached = delay < ref.NO_ONSET
    check_cells(got, want, ctx)
    check_nan_pattern(got, reached, ctx)
    onset = np.where(reached, delay, 0).astype(np.int64)
    assert np.array_equal(got[..., 0][reached], (T - onset)[reached].astype(np.float32)), ctx  # n == T - onset


def sample(rng, mask, n):
    idx = np.argwhere(mask)
    return idx[rng.choice(len(idx), min(len(idx), n), replace=False)]


_PRESET = {}


def preset_run(pvlib, name, edges=None):
    """plain run of a preset scene at its golden listener: (records, delay, (gx, T, fs)); one run serves both window settings"""
    if (name, edges) not in _PRESET:
        g = golden(name)
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            delay, shape = s.results()[1], (s.gx, s.T, s.fs)
            for e in WINDOWS:
                s.set_lobe_windows(e)
                sec, steps = s.lobe_windows()
                assert list(steps) == ref.edge_steps(e, s.fs) and same_bits(sec, np.float32(e or ref.DEFAULT_EDGES)).all()
                assert s.compute_lobes() > 0
                _PRESET[name, e] = (s.lobes(), delay, shape)
    return _PRESET[name, edges]


# 1. the 70^2 presets (T = 435: the resident path) against the oracle's recorded pr / vx / vy, every cell
@pytest.mark.parametrize("edges", WINDOWS, ids=["default", "five"])
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty", "g71_hugeroom"])
def test_preset_grid(pvlib, oracle, name, edges):
    got, delay, (gx, T, fs) = preset_run(pvlib, name, edges)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, floats(edges))
    _, _, _, odelay, ofs = oracle_run(oracle, name)
    assert ofs == fs and same_bits(delay, odelay).all()
    assert (delay < ref.NO_ONSET).sum() > 1000
    check_map(got, scene_ref(oracle, name, edges), delay, T, "%s %s" % (name, edges))


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; neighbours across
#    tile edges, across the window edge and in tiles recorded from a later launch; responses that end inside window 0, inside
#    window 1, and after one step
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        onset = np.where(reached, delay, 0).astype(np.int64)
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False

        rxi, wi, K = s.info.tileRows, s.info.tileCols, s.info.stepsPerLaunch
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]  # (the listener's cell)
        first_row, first_col = (X % rxi == 0), (Y % wi == 0)
        # Neighbour tiles recorded from a later launch: as tests/test_gpu_lateral.py finds them
        assert rxi >= K and wi >= K
        hist = history(s)
        nz = hist != 0
        tnz_cell = np.where(nz.any(axis=0), nz.argmax(axis=0), 10 ** 6)
        ntx, nty = -(-s.gx // rxi), -(-s.gy // wi)
        tnz = np.full((ntx, nty), 10 ** 6)
        ti, tj = X // rxi, Y // wi
        np.minimum.at(tnz, (ti, tj), tnz_cell)
        later_x = first_row & (ti < lx // rxi) & (ti > 0) & (tnz[np.maximum(ti - 1, 0), tj] >= tnz[ti, tj] + K)
        later_y = first_col & (tj < ly // wi) & (tj > 0) & (tnz[ti, np.maximum(tj - 1, 0)] >= tnz[ti, tj] + K)
        n0, n1 = ref.edge_steps(None, s.fs)
        assert (n0, n1) == (14, 115)
        N = s.T - onset
        band = (np.abs(X - lx) <= 60) & (np.abs(Y - ly) <= 60)
        classes = {"tile edge": reached & band & (first_row | first_col),
                   "ends inside window 0": reached & (N <= n0), "ends inside window 1": reached & (N > n0) & (N <= n1),
                   "N = 1": reached & (N == 1)}
        if where == "corner":  # (no tile lies above or left of the listener's: the upstream neighbour lies outside the window)
            classes["upstream neighbour outside the window"] = reached & ((X == 0) | (Y == 0))
        else:
            classes["upstream neighbour in another tile"] = reached & ~band & (first_row | first_col)
            classes["later neighbour tile"] = reached & (later_x | later_y)
        rng = np.random.default_rng(400)
        pick = np.zeros(delay.shape, bool)
        for name, m in classes.items():
            assert m.any(), (where, name)
            sel = sample(rng, m, 60)
            pick[sel[:, 0], sel[:, 1]] = True
        sel = sample(rng, reached, 100)
        pick[sel[:, 0], sel[:, 1]] = True
        cells = np.argwhere(pick)
        print(where, "tile", (rxi, wi, K), "sample", len(cells), dict((k, int((v & pick).sum())) for k, v in classes.items()))
        assert len(cells) >= 300
        irs = responses(s, cells)
        for edges in (None, (0.005, 0.02, 0.05)):
            s.set_lobe_windows(edges)
            s.compute_lobes()
            got = s.lobes()
            assert np.isnan(got[outside]).all()
            check_nan_pattern(got, reached, where)
            assert np.array_equal(got[..., 0][reached], N[reached].astype(np.float32))
            check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay, edges, irs), "%s %s" % (where, edges))
            if edges is None:  # the windows the response does not reach hold five +0.0f
                for m, first_empty in ((classes["ends inside window 0"], 6), (classes["ends inside window 1"], 11)):
                    tail = got[m][:, first_empty:]
                    assert (tail == 0).all() and not np.signbit(tail).any()


# 3. the same bits on every stepping path
FORMS = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
         "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}


@pytest.mark.parametrize("form", list(FORMS))
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay, _ = preset_run(pvlib, "g71_smallroom", EDGES5)
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g, **FORMS[form]) as s:
        s.set_lobe_windows(EDGES5)  # (set before the run: a run does not touch the setting)
        s.run_async(g["listener"])
        s.sync()
        s.compute_lobes()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.lobes(), want).all(), form


def test_non_square_grid(pvlib):
    """95 x 70 cells: the three paths give the same bits, and those are the restatement's on impulse_response"""
    L = cell_of(40, 22)
    maps = {}
    for form, opts in FORMS.items():
        with pvlib.Solver(open_size(95), open_size(70), 275, **opts) as s:
            assert (s.gx, s.gy, s.T) == (95, 70, 435)
            s.load_scene(SMALLROOM)
            s.run(L)
            s.compute_lobes()
            maps[form] = (s.lobes(), s.results()[1])
            if form == "resident":
                got, delay = maps[form]
                assert got.shape == (95, 70, 16)
                reached = delay < ref.NO_ONSET
                assert reached.sum() > 3000
                check_nan_pattern(got, reached, "95 x 70")
                cells = sample(np.random.default_rng(95), reached, 300)
                check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay), "95 x 70")
    for form in ("small_grid", "graph"):
        assert same_bits(maps[form][1], maps["resident"][1]).all(), form
        assert same_bits(maps[form][0], maps["resident"][0]).all(), form


# 4. batch members, and a second run that reaches fewer cells: nothing is carried over
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with preset_solver(pvlib, g) as s:
        s.run(L[1])
        s.compute_lobes()  # (no windows were ever set: the default)
        plain.append(s.lobes())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [preset_solver(pvlib, g) for _ in L]
    try:
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_lobes()
            assert same_bits(s.lobes(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with preset_solver(pvlib, g) as s:
        s.run(L[0])
        s.compute_lobes()
        first, first_reached = s.lobes(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_lobes()
        got, delay = s.lobes(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected_map(s, delay), delay, s.T, "walled-in second run")
    # the second of two iterations in flight on two solvers reads its own run
    with preset_solver(pvlib, g) as a, preset_solver(pvlib, g) as b:
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_lobes()  # (waits for the run in flight)
        got = b.lobes()
        assert same_bits(got, plain[0]).all()
        a.sync()


# 5. few live groups in a big window: a closed room in a 1024-cell grid (waves without a live lane, waves with one)
def test_few_groups_in_a_big_window(pvlib):
    n = 1024
    size = open_size(n)
    with pvlib.Solver(size, size, 275, num_steps=435) as s:
        assert s.gx == n and s.T == 435
        s.load_scene(SHOEBOX)
        s.run((5.0, 0.0, 4.0))
        s.compute_lobes()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.lobes_block(r0, c0, r1 - r0, c1 - c0)
        assert got.shape == (r1 - r0, c1 - c0, 16)
        check_nan_pattern(got, reached[rows, cols], "1024 block")
        rxi, wi = s.info.tileRows, s.info.tileCols
        idx = np.argwhere(reached)
        edge = idx[(idx[:, 0] % rxi == 0) | (idx[:, 1] % wi == 0)]
        rng = np.random.default_rng(1024)
        cells = np.unique(np.concatenate([edge[rng.choice(len(edge), min(len(edge), 100), replace=False)],
                                          idx[rng.choice(len(idx), 250, replace=False)]]), axis=0)
        assert len(cells) >= 300 and len(edge) > 0
        check_cells(got[cells[:, 0] - r0, cells[:, 1] - c0], expected_at(s, cells, delay), "1024 block")
        whole = s.lobes()
        assert same_bits(whole[rows, cols], got).all()
        whole[rows, cols] = np.nan
        assert np.isnan(whole).all()


# 6. split-field edge layers: the cells inside the layers get records like any other cell (the undamped recurrence, which is
#    what impulse_response returns there too)
def test_split_layer(pvlib):
    n = 160
    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        s.set_edge_layer_split((24, 24, 24, 24))
        s.run(cell_of(n // 2, n // 3 + 6))
        s.compute_lobes()
        got, delay = s.lobes(), s.results()[1]
        reached = delay < ref.NO_ONSET
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached)
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()
        layer = np.ones(delay.shape, bool)
        layer[24:-24, 24:-24] = False
        rng = np.random.default_rng(160)
        picks = [sample(rng, m, 200) for m in (reached & layer, reached & ~layer)]
        assert len(picks[0]) == 200 and len(picks[1]) == 200
        cells = np.concatenate(picks)
        check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay), "split layer")


# 7. a resolution with other window lengths: fs 1968, edges at 19 and 157 steps
def test_other_resolution(pvlib):
    got, delay, (gx, T, fs) = preset_run(pvlib, "g96_smallroom_res375")
    assert gx == 95 and got.shape == (95, 95, 16) and fs == 1968 and ref.edge_steps(None, fs) == [19, 157]
    reached = delay < ref.NO_ONSET
    check_nan_pattern(got, reached, "res 375")
    g = golden("g96_smallroom_res375")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        assert same_bits(s.results()[1], delay).all()
        assert len(np.argwhere(reached)) > 3000
        cells = sample(np.random.default_rng(96), reached, 1200)
        want = expected_at(s, cells, delay)
    check_cells(got[cells[:, 0], cells[:, 1]], want, "res 375")


# 8. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.compute_lobes()
        m = s.lobes()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.lobes_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.lobes_at(e)).all() and s.lobes_at(e).shape == (16,)
        # the wet-path weights of an emitter at that cell: finite energy ratios between the floor and 1
        rec = s.lobes_at(g["emitters"][0])
        for fwd in ((1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (0.6, -0.8)):
            gains = pvlib.lobe_gains(rec, fwd, pvlib.LOBE_PATTERN_CARDIOID)
            assert same_bits(gains, ref.lobe_gains(rec, fwd, 1)).all()
            assert gains.shape == (3,) and ((gains >= 1e-4 * 0.99) & (gains <= 1)).all()


# 9. lifetime: -1 before compute and after a run, a geometry, boundary or layer change or a set_lobe_windows; independent of the
#    seven other record kinds
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        reads = (s.lobes, lambda: s.lobes_at(g["emitters"][0]), lambda: s.lobes_block(0, 0, 2, 2))

        def refused():
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match="^lobes: "):
                    call()

        def others():
            s.compute_room_metrics()
            s.compute_spectrum()
            s.compute_decay_times()
            s.compute_lateral_fraction()
            s.compute_band_metrics()
            s.compute_echogram()
            s.compute_echo_criterion()
            return (s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics(), s.echogram(),
                    s.echo_criterion())

        def read_others():
            return (s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics(), s.echogram(),
                    s.echo_criterion())

        refused()  # (not computed yet)
        s.set_spectrum_bins([50.0, 100.0])
        s.set_bands([125.0])
        s.set_echogram(0.005, 16)
        before = others()
        refused()
        s.compute_lobes()
        first = s.lobes()
        assert same_bits(first, want).all()
        for a, b in zip(read_others(), before):
            assert same_bits(a, b).all()  # (still valid)
        others()
        assert same_bits(s.lobes(), first).all()  # (computing the seven other kinds leaves these bits alone)
        s.set_echogram(0.002, 8)  # (another kind's setting)
        assert same_bits(s.lobes(), first).all()
        s.set_lobe_windows(None)  # (even the same windows)
        refused()
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        for a, b in zip(read_others(), before):
            assert same_bits(a, b).all()  # (set_lobe_windows invalidated this kind only)
        for bad in ((0.02, 0.01), (0.0100, 0.0101), (0.0006,), (0.001,) * 8, (float("nan"),), (float("inf"),), (1000.0,)):
            with pytest.raises(pvlib.PlaneverbError, match="^lobes: "):
                s.set_lobe_windows(bad)
        assert list(s.lobe_windows()[1]) == [14, 115]  # (nothing changed)
        s.compute_lobes()
        assert same_bits(s.lobes(), first).all()
        s.set_lobe_windows(EDGES5)  # (another nW: the storage is allocated again)
        refused()
        s.compute_lobes()
        assert same_bits(s.lobes(), preset_run(pvlib, "g71_smallroom", EDGES5)[0]).all()
        s.set_lobe_windows(())
        s.compute_lobes()
        assert same_bits(s.lobes(), first).all()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_lobes()  # (the last completed run is still the first one)
        assert same_bits(s.lobes(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_lobes()
        second = s.lobes()
        assert not same_bits(second, first).all()
        assert np.array_equal(np.isnan(second).all(axis=-1), ~(s.results()[1] < ref.NO_ONSET))
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_lobes()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


#    refusals: a "lobes: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: .*history"):
            s.compute_lobes()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: .*onset map"):
            s.compute_lobes()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_lobe_windows((0.01,)), s.lobe_windows, s.compute_lobes, s.lobes, lambda: s.lobes_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="^lobes: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: no completed run"):
            s.compute_lobes()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: "):
            s.lobes()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: no completed run"):
            s.compute_lobes()
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^lobes: block outside the map"):
            s.lobes_block(0, 0, s.gx + 1, 1)
        assert s.compute_lobes() > 0
        assert np.isfinite(s.lobes_at(E)).all()


# 10. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(*more):
        return json.loads(subprocess.run(cmd + list(more), capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                         timeout=300).stdout)

    outs = {None: run("--lobes"), (0.005, 0.02, 0.08): run("--lobes", "0.005,0.02,0.08")}
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        for edges, out in outs.items():
            s.set_lobe_windows(edges)
            s.compute_lobes()
            for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), out["emitters"]):
                m = s.lobes_at(e)
                lo = rec["lobes"]
                assert "rt60" in rec and list(lo) == ["n", "windows"] and len(lo["windows"]) == len(edges or (0, 0)) + 1
                assert all(list(w) == list(pvlib.LOBE_NAMES) for w in lo["windows"])
                got = np.float32([lo["n"]] + [w[k] for w in lo["windows"] for k in pvlib.LOBE_NAMES])
                assert same_bits(got, m).all(), (got, m)
