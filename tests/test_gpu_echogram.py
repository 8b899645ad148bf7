"""GPU (-m gpu): per-cell directional echogram (PvAmdComputeEchogram; pv_echogram.hip).

The expected values come from the numpy restatement (tests/_echogram_ref.py, written from the definition in
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

import _echogram_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_lateral import check_cells, preset_solver
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history
from test_host_lateral import oracle_run

pytestmark = pytest.mark.gpu

SETTINGS = [(0.005, 16), (0.002, 32), (0.01, 24)]


def responses(s, cells):
    """impulse_response of the given result cells [(x, y)]: float32 [T, len(cells), 3]"""
    return np.stack([s.impulse_response(int(x), int(y)) for x, y in cells], axis=1)


def expected_at(s, cells, delay, setting, irs=None):
    """the restatement on impulse_response of the given result cells: float32 [len(cells), 1 + 3 n]"""
    irs = responses(s, cells) if irs is None else irs
    d = np.array([delay[x, y] for x, y in cells], np.float32)
    return ref.echogram(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs, *setting)


def expected_map(s, delay, setting):
    """the same for every reached cell of the map: float32 [gx, gy, 1 + 3 n], NaN without an onset"""
    out = np.full(delay.shape + (1 + 3 * setting[1],), np.nan, np.float32)
    cells = np.argwhere(delay < ref.NO_ONSET)
    if len(cells):
        out[cells[:, 0], cells[:, 1]] = expected_at(s, cells, delay, setting)
    return out


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    check_cells(got, want, ctx)
    # NaN records on exactly the unreached cells; n and every slot value of a reached cell are numbers, slot 0 has energy
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached), ctx
    assert np.array_equal(np.isnan(got).any(axis=-1), ~reached), ctx
    assert np.isfinite(got[reached]).all(), ctx
    assert (got[..., 0][reached] >= 1).all() and (got[..., 1][reached] > 0).all(), ctx


_PRESET = {}
_SHOEBOX = {}  # impulse_response of every reached cell of g71_shoebox: one set serves the three settings


def preset_run(pvlib, name, setting=(0.005, 16)):
    """plain run of a 70^2 preset scene at its golden listener: (records, delay, (gx, T, fs))"""
    if (name, setting) not in _PRESET:
        g = golden(name)
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            delay, shape = s.results()[1], (s.gx, s.T, s.fs)
            for st in SETTINGS:  # (one run serves every setting)
                s.set_echogram(*st)
                assert s.echogram_slots() == (st[1], np.float32(st[0]), ref.slot_steps(st[0], s.fs))
                assert s.compute_echogram() > 0
                _PRESET[name, st] = (s.echogram(), delay, shape)
    return _PRESET[name, setting]


# 1. the 70^2 presets (T = 435: the resident path) against the oracle's recorded pr / vx / vy
@pytest.mark.parametrize("setting", SETTINGS)
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, oracle, name, setting):
    got, delay, (gx, T, fs) = preset_run(pvlib, name, setting)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, 1 + 3 * setting[1])
    p, vx, vy, odelay, ofs = oracle_run(oracle, name)
    assert ofs == fs and same_bits(delay, odelay).all()
    want = ref.echogram(p, vx, vy, delay, fs, *setting)
    check_map(got, want, delay, "%s %s" % (name, setting))
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    full = ref.slot_steps(setting[0], fs) * setting[1]
    cut = reached & (np.where(reached, delay, 0).astype(np.int64) + full > T)
    assert np.array_equal(reached & (got[..., 0] < full), cut)
    if setting == (0.01, 24):
        assert full == 336 and (cut.sum() > 100 or name == "g71_shoebox")
    else:
        assert not cut.any()
    if name == "g71_shoebox":
        # the same with vx, vy of impulse_response, every reached cell: the two expectations agree with each other too
        cells = np.argwhere(reached)
        if "irs" not in _SHOEBOX:
            g = golden(name)
            with preset_solver(pvlib, g) as s:
                s.run(g["listener"])
                assert same_bits(s.results()[1], delay).all()
                _SHOEBOX["irs"] = responses(s, cells)
        irs = _SHOEBOX["irs"]
        want_ir = np.full(want.shape, np.nan, np.float32)
        want_ir[cells[:, 0], cells[:, 1]] = ref.echogram(irs[..., 0], irs[..., 1], irs[..., 2], delay[reached], fs, *setting)
        check_cells(want_ir, want, name + ": impulse_response against the oracle")
        check_map(got, want_ir, delay, name + ": impulse_response")


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; neighbours across
#    tile edges, across the window edge and in tiles recorded from a later launch; windows cut off by T
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    settings = [(0.005, 16), (0.02, 5)]
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
        edge = (X == 0) | (Y == 0)
        fulls = [ref.slot_steps(st[0], s.fs) * st[1] for st in settings]
        assert fulls == [112, 140]
        cut = onset + min(fulls) > s.T  # cut off by T at both settings
        band = (np.abs(X - lx) <= 60) & (np.abs(Y - ly) <= 60)
        classes = {"tile edge in the band": reached & band & (first_row | first_col), "cut off by T": reached & cut}
        if where == "corner":  # (no tile lies above or left of the listener's)
            classes["window edge"] = reached & edge
        else:
            classes["later neighbour tile"] = reached & (later_x | later_y)
        rng = np.random.default_rng(400)
        pick = np.zeros(delay.shape, bool)
        pick |= classes["tile edge in the band"]
        for name, m in classes.items():
            assert m.any(), (where, name)
            idx = np.argwhere(m)
            sel = idx[rng.choice(len(idx), min(len(idx), 120), replace=False)]
            pick[sel[:, 0], sel[:, 1]] = True
        idx = np.argwhere(reached)
        sel = idx[rng.choice(len(idx), 100, replace=False)]
        pick[sel[:, 0], sel[:, 1]] = True
        cells = np.argwhere(pick)
        print(where, "tile", (rxi, wi, K), "sample", len(cells), dict((k, int((v & pick).sum())) for k, v in classes.items()))
        assert len(cells) >= 300 and (classes["cut off by T"] & pick).sum() >= 20
        irs = responses(s, cells)
        for st, full in zip(settings, fulls):
            s.set_echogram(*st)
            s.compute_echogram()
            got = s.echogram()
            assert np.isnan(got[outside]).all()
            assert np.array_equal(np.isnan(got).all(axis=-1), ~reached) and np.array_equal(np.isnan(got).any(axis=-1), ~reached)
            check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay, st, irs), "%s %s" % (where, st))
            n = got[..., 0]
            c = onset + full > s.T
            assert (n[reached & c] < full).all() and (n[reached & ~c] == full).all()


# 3. the same bits on every stepping path
@pytest.mark.parametrize("form", ["resident", "small_grid", "graph"])
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay, _ = preset_run(pvlib, "g71_smallroom")
    g = golden("g71_smallroom")
    opts = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
            "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}[form]
    with preset_solver(pvlib, g, **opts) as s:
        s.set_echogram(0.005, 16)  # (set before the run: a run does not touch the setting)
        s.run_async(g["listener"])
        s.sync()
        s.compute_echogram()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.echogram(), want).all(), form


# 4. batch members, and a second run that reaches fewer cells: nothing is carried over
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    st = (0.005, 16)
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with preset_solver(pvlib, g) as s:
        s.run(L[1])
        s.set_echogram(*st)
        s.compute_echogram()
        plain.append(s.echogram())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [preset_solver(pvlib, g) for _ in L]
    try:
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.set_echogram(*st)
            s.compute_echogram()
            assert same_bits(s.echogram(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with preset_solver(pvlib, g) as s:
        s.set_echogram(*st)
        s.run(L[0])
        s.compute_echogram()
        first, first_reached = s.echogram(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_echogram()
        got, delay = s.echogram(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected_map(s, delay, st), delay, "walled-in second run")
    # the second of two iterations in flight on two solvers reads its own run
    with preset_solver(pvlib, g) as a, preset_solver(pvlib, g) as b:
        b.set_echogram(*st)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_echogram()  # (waits for the run in flight)
        got = b.echogram()
        assert same_bits(got, plain[0]).all()
        a.sync()


# 5. few live groups in a big window: a closed room in a 1024-cell grid (waves without a live lane, waves with one)
def test_few_groups_in_a_big_window(pvlib):
    n = 1024
    size = open_size(n)
    st = (0.005, 16)
    with pvlib.Solver(size, size, 275, num_steps=435) as s:
        assert s.gx == n and s.T == 435
        s.load_scene(SHOEBOX)
        s.run((5.0, 0.0, 4.0))
        s.set_echogram(*st)
        s.compute_echogram()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.echogram_block(r0, c0, r1 - r0, c1 - c0)
        assert got.shape == (r1 - r0, c1 - c0, 49)
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached[rows, cols])
        assert np.array_equal(np.isnan(got).any(axis=-1), ~reached[rows, cols])
        rxi, wi = s.info.tileRows, s.info.tileCols
        idx = np.argwhere(reached)
        edge = idx[(idx[:, 0] % rxi == 0) | (idx[:, 1] % wi == 0)]
        rng = np.random.default_rng(1024)
        cells = np.unique(np.concatenate([edge[rng.choice(len(edge), min(len(edge), 150), replace=False)],
                                          idx[rng.choice(len(idx), 250, replace=False)]]), axis=0)
        assert len(cells) >= 300 and len(edge) > 0
        check_cells(got[cells[:, 0] - r0, cells[:, 1] - c0], expected_at(s, cells, delay, st), "1024 block")
        whole = s.echogram()
        assert same_bits(whole[rows, cols], got).all()
        whole[rows, cols] = np.nan
        assert np.isnan(whole).all()


# 6. split-field edge layers: the cells inside the layers get records like any other cell (the undamped recurrence, which is
#    what impulse_response returns there too)
def test_split_layer(pvlib):
    n = 160
    st = (0.005, 16)
    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        s.set_edge_layer_split((24, 24, 24, 24))
        s.run(cell_of(n // 2, n // 3 + 6))
        s.set_echogram(*st)
        s.compute_echogram()
        got, delay = s.echogram(), s.results()[1]
        reached = delay < ref.NO_ONSET
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached)
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()
        layer = np.ones(delay.shape, bool)
        layer[24:-24, 24:-24] = False
        rng = np.random.default_rng(160)
        picks = []
        for m in (reached & layer, reached & ~layer):
            idx = np.argwhere(m)
            picks.append(idx[rng.choice(len(idx), min(len(idx), 200), replace=False)])
        assert len(picks[0]) == 200
        cells = np.concatenate(picks)
        check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay, st), "split layer")


# 7. setting changes: another nSlots reallocates, reads are refused until recomputed, the first setting gives the first bits again
def test_setting_changes(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        assert s.echogram_slots() == (0, 0.0, 0)
        s.run(g["listener"])
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        first = s.echogram()
        assert same_bits(first, preset_run(pvlib, "g71_smallroom", (0.005, 16))[0]).all()
        for bad in ((0.005, 33), (0.005, -1), (0.0006, 4), (float("nan"), 4), (float("inf"), 4), (-0.005, 4), (1000.0, 4)):
            with pytest.raises(pvlib.PlaneverbError, match="echogram: "):
                s.set_echogram(*bad)
        assert s.echogram_slots()[::2] == (16, 7) and same_bits(s.echogram(), first).all()  # (nothing changed)
        s.set_echogram(0.002, 32)
        assert s.echogram_slots()[::2] == (32, 2)
        for call in (s.echogram, lambda: s.echogram_at(g["emitters"][0]), lambda: s.echogram_block(0, 0, 2, 2)):
            with pytest.raises(pvlib.PlaneverbError, match="echogram: not computed"):
                call()
        s.compute_echogram()
        second = s.echogram()
        assert second.shape == (70, 70, 97)
        assert same_bits(second, preset_run(pvlib, "g71_smallroom", (0.002, 32))[0]).all()
        s.set_echogram(0.01, 1)  # (fewer planes than allocated)
        s.compute_echogram()
        one = s.echogram()
        assert one.shape == (70, 70, 4)
        assert same_bits(one[..., 1:], preset_run(pvlib, "g71_smallroom", (0.01, 24))[0][..., 1:4]).all()  # (slot 0 is slot 0)
        assert np.array_equal(np.isnan(one[..., 0]), np.isnan(first[..., 0])) and (one[..., 0][~np.isnan(one[..., 0])] <= 14).all()
        s.set_echogram(0.005, 16)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: not computed"):
            s.echogram()
        s.compute_echogram()
        assert same_bits(s.echogram(), first).all()
        s.set_echogram(0.005, 0)
        assert s.echogram_slots() == (0, 0.0, 0)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: no slots set"):
            s.compute_echogram()
        with pytest.raises(pvlib.PlaneverbError, match="echogram: no slots set"):
            s.echogram_at(g["emitters"][0])
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        assert same_bits(s.echogram(), first).all()


# 8. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        m = s.echogram()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.echogram_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.echogram_at(e)).all() and s.echogram_at(e).shape == (49,)


# 9. lifetime: -1 before compute and after a run, a geometry, boundary or layer change or a set_echogram; independent of the
#    other five record kinds
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.set_echogram(0.005, 16)
        reads = (s.echogram, lambda: s.echogram_at(g["emitters"][0]), lambda: s.echogram_block(0, 0, 2, 2))

        def refused():
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match="echogram: "):
                    call()

        def others():
            s.compute_room_metrics()
            s.compute_spectrum()
            s.compute_decay_times()
            s.compute_lateral_fraction()
            s.compute_band_metrics()
            return s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics()

        refused()  # (not computed yet)
        s.set_spectrum_bins([50.0, 100.0])
        s.set_bands([125.0])
        before = others()
        refused()
        s.compute_echogram()
        first = s.echogram()
        assert same_bits(first, want).all()
        for a, b in zip((s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics()), before):
            assert same_bits(a, b).all()  # (still valid)
        others()
        assert same_bits(s.echogram(), first).all()  # (and the reverse)
        s.set_echogram(0.005, 16)  # (even the same setting)
        refused()
        assert same_bits(s.lateral_fraction(), before[3]).all()
        s.compute_echogram()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_echogram()  # (the last completed run is still the first one)
        assert same_bits(s.echogram(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_echogram()
        second = s.echogram()
        assert not same_bits(second, first).all()
        assert np.array_equal(np.isnan(second).all(axis=-1), ~(s.results()[1] < ref.NO_ONSET))
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_echogram()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


# 10. refusals: an "echogram: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.set_echogram(0.005, 16)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: .*history"):
            s.compute_echogram()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_echogram(0.005, 16)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: .*onset map"):
            s.compute_echogram()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_echogram(0.005, 16), s.echogram_slots, s.compute_echogram, s.echogram, lambda: s.echogram_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="echogram: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: no slots set"):
            s.compute_echogram()
        s.set_echogram(0.005, 16)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: no completed run"):
            s.compute_echogram()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="echogram: "):
            s.echogram()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="echogram: no completed run"):
            s.compute_echogram()
        s.run(L)
        assert s.compute_echogram() > 0
        assert np.isfinite(s.echogram_at(E)).all()


# 11. slot 0 at 5 ms is the direct-sound flux of the lateral-fraction records of the same run
def test_slot_zero_is_the_lateral_flux(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        s.compute_lateral_fraction()
        e, lat = s.echogram(), s.lateral_fraction()
        assert same_bits(e, preset_run(pvlib, "g71_smallroom")[0]).all()
        assert np.isfinite(e[..., 2]).sum() > 1000
        assert same_bits(e[..., 2], lat[..., 6]).all() and same_bits(e[..., 3], lat[..., 7]).all()


# 12. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    withe = json.loads(subprocess.run(cmd + ["--echogram", "0.005,16"], capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                      timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.set_echogram(0.005, 16)
        s.compute_echogram()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withe["emitters"]):
            m = s.echogram_at(e)
            eg = rec["echogram"]
            assert "rt60" in rec and list(eg) == ["slotSteps", "n", "e", "ix", "iy"] and eg["slotSteps"] == 7
            assert len(eg["e"]) == len(eg["ix"]) == len(eg["iy"]) == 16
            got = np.empty(49, np.float32)
            got[0], got[1::3], got[2::3], got[3::3] = eg["n"], eg["e"], eg["ix"], eg["iy"]
            assert same_bits(got, m).all(), (got, m)
