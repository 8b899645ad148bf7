"""GPU (-m gpu): per-cell echo criterion, speech and music (PvAmdComputeEchoCriterion; pv_echo.hip).

The expected values come from the numpy restatement (tests/_echo_ref.py, written from the definition in
include/planeverb_amd.h; it keeps c per step, the kernel recomputes the lagged one) fed with pressure from somewhere else than the
pass under test: the oracle's recorded pressure cube on the 70^2 presets, and the solver's own history_plane(t) everywhere else,
with the run's own onset map (results()[1]).  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _echo_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_lateral import check_cells, preset_solver
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history
from test_host_lateral import oracle_run

pytestmark = pytest.mark.gpu

S_EK, S_TK, S_EKL, S_TKL, S_TS, M_EK, M_TK, M_EKL, M_TKL, M_TS = range(10)


def expected_at(hist, cells, delay, fs):
    """the restatement on the recorded pressure hist [T, rows, cols] of the given cells [(x, y)] of it: float32 [len(cells), 10]"""
    cells = np.asarray(cells)
    return ref.echo_criterion(np.ascontiguousarray(hist[:, cells[:, 0], cells[:, 1]]), delay[cells[:, 0], cells[:, 1]], fs)


def expected_map(s, delay):
    """the same for every reached cell of the map: float32 [gx, gy, 10], NaN without an onset"""
    out = np.full(delay.shape + (10,), np.nan, np.float32)
    cells = np.argwhere(delay < ref.NO_ONSET)
    if len(cells):
        out[cells[:, 0], cells[:, 1]] = expected_at(history(s), cells, delay, s.fs)
    return out


def check_nan_pattern(got, reached, ctx):
    """ten NaNs on exactly the unreached cells; the maxima and their delays of a reached cell are numbers"""
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached), ctx
    for v in (S_EK, S_TK, S_EKL, S_TKL, M_EK, M_TK, M_EKL, M_TKL):
        assert np.isfinite(got[..., v][reached]).all(), (ctx, v)


def check_map(got, want, delay, ctx):
    check_cells(got, want, ctx)
    check_nan_pattern(got, delay < ref.NO_ONSET, ctx)


_PRESET = {}


def preset_run(pvlib, name):
    """plain run of a preset scene at its golden listener: (records, delay, (gx, T, fs))"""
    if name not in _PRESET:
        g = golden(name)
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            assert s.compute_echo_criterion() > 0
            _PRESET[name] = (s.echo_criterion(), s.results()[1], (s.gx, s.T, s.fs))
    return _PRESET[name]


# 1. the 70^2 presets (T = 435: the resident path) against the oracle's recorded pressure, every reached cell
@pytest.mark.parametrize("name", ["g71_hugeroom", "g71_empty", "g71_smallroom", "g71_shoebox"])
def test_preset_grid(pvlib, oracle, name):
    got, delay, (gx, T, fs) = preset_run(pvlib, name)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, 10) and ref.lags(fs) == (12, 72, 20, 115)
    p, _, _, odelay, ofs = oracle_run(oracle, name)
    assert ofs == fs and p.shape == (435, 70, 70) and same_bits(delay, odelay).all()
    want = ref.echo_criterion(p, delay, fs)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    # what the reference alone says of these scenes (the test's reach, not a measurement of the kernel)
    speech, music = want[..., S_EK][reached], want[..., M_EK][reached]
    print(name, "reached", reached.sum(), "speech max %.4f over %d" % (speech.max(), (speech > ref.SPEECH_CRIT).sum()),
          "music max %.4f over %d" % (music.max(), (music > ref.MUSIC_CRIT).sum()))
    assert not np.isnan(want[reached]).any() and (want[..., S_EKL][reached] > 0).all()
    if name == "g71_hugeroom":
        assert (speech > ref.SPEECH_CRIT).sum() >= 500 and (music > ref.MUSIC_CRIT).sum() >= 5
    if name == "g71_empty":
        assert not (speech > ref.SPEECH_CRIT).any() and not (music > ref.MUSIC_CRIT).any()
    check_map(got, want, delay, name)


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; tile-edge cells,
#    cells whose lagged planes lie before their tile's first recorded launch, responses shorter than the limits and the lags
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        s.compute_echo_criterion()
        got, delay = s.echo_criterion(), s.results()[1]
        nDs, nLs, nDm, nLm = ref.lags(s.fs)
        assert (nDs, nLs, nDm, nLm) == (12, 72, 20, 115)
        reached = delay < ref.NO_ONSET
        check_nan_pattern(got, reached, where)
        onset = np.where(reached, delay, 0).astype(np.int64)
        N = s.T - onset
        xs, ys = np.nonzero(reached)
        outside = np.ones(delay.shape, bool)
        outside[max(xs.min() - 2, 0):xs.max() + 3, max(ys.min() - 2, 0):ys.max() + 3] = False
        assert np.isnan(got[outside]).all()

        rxi, wi, K = s.info.tileRows, s.info.tileCols, s.info.stepsPerLaunch
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        hist = history(s)
        # the first step at which a tile holds a non-zero sample: its history is recorded from the launch of that step at the
        # latest, so a cell whose onset is less than K + nDm steps later reads lagged planes from before that launch
        nz = hist != 0
        tnz_cell = np.where(nz.any(axis=0), nz.argmax(axis=0), 10 ** 6)
        ntx, nty = -(-s.gx // rxi), -(-s.gy // wi)
        tnz = np.full((ntx, nty), 10 ** 6)
        ti, tj = X // rxi, Y // wi
        np.minimum.at(tnz, (ti, tj), tnz_cell)
        early = onset - nDm < tnz[ti, tj] + K
        classes = {"tile edge": reached & ((X % rxi == 0) | (Y % wi == 0) | (X % rxi == rxi - 1) | (Y % wi == wi - 1)),
                   "lagged planes before the tile's first launch": reached & early & (onset >= nDm),
                   "N <= nL (speech)": reached & (N <= nLs), "N <= nL (music)": reached & (N <= nLm) & (N > nLs),
                   "N <= nD": reached & (N <= nDm), "N = 1": reached & (N == 1)}
        rng = np.random.default_rng(400)
        pick = np.zeros(delay.shape, bool)
        for name, m in classes.items():
            assert m.any(), (where, name)
            idx = np.argwhere(m)
            sel = idx[rng.choice(len(idx), min(len(idx), 80), replace=False)]
            pick[sel[:, 0], sel[:, 1]] = True
        idx = np.argwhere(reached)
        sel = idx[rng.choice(len(idx), 150, replace=False)]
        pick[sel[:, 0], sel[:, 1]] = True
        cells = np.argwhere(pick)
        print(where, "tile", (rxi, wi, K), "sample", len(cells), dict((k, int((v & pick).sum())) for k, v in classes.items()))
        assert len(cells) >= 300
        check_cells(got[cells[:, 0], cells[:, 1]], expected_at(hist, cells, delay, s.fs), where)
        # a response no longer than the limit has no late maximum; one of a single step has none at all
        assert (got[..., S_EKL][reached & (N <= nLs)] == 0).all() and (got[..., S_TKL][reached & (N <= nLs)] == 0).all()
        assert (got[..., M_EKL][reached & (N <= nLm)] == 0).all() and (got[..., M_TKL][reached & (N <= nLm)] == 0).all()
        assert (got[reached & (N == 1)] == 0).all()


# 3. the same bits on every stepping path
@pytest.mark.parametrize("form", ["resident", "small_grid", "graph"])
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay, _ = preset_run(pvlib, "g71_smallroom")
    g = golden("g71_smallroom")
    opts = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
            "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}[form]
    with preset_solver(pvlib, g, **opts) as s:
        s.run_async(g["listener"])
        s.sync()
        s.compute_echo_criterion()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.echo_criterion(), want).all(), form


# 4. batch members, and a second run that reaches fewer cells: nothing is carried over
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with preset_solver(pvlib, g) as s:
        s.run(L[1])
        s.compute_echo_criterion()
        plain.append(s.echo_criterion())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [preset_solver(pvlib, g) for _ in L]
    try:
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_echo_criterion()
            assert same_bits(s.echo_criterion(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with preset_solver(pvlib, g) as s:
        s.run(L[0])
        s.compute_echo_criterion()
        first, first_reached = s.echo_criterion(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_echo_criterion()
        got, delay = s.echo_criterion(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected_map(s, delay), delay, "walled-in second run")
    # the second of two iterations in flight on two solvers reads its own run
    with preset_solver(pvlib, g) as a, preset_solver(pvlib, g) as b:
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_echo_criterion()  # (waits for the run in flight)
        got = b.echo_criterion()
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
        s.compute_echo_criterion()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.echo_criterion_block(r0, c0, r1 - r0, c1 - c0)
        assert got.shape == (r1 - r0, c1 - c0, 10)
        check_nan_pattern(got, reached[rows, cols], "1024 block")
        rxi, wi = s.info.tileRows, s.info.tileCols
        idx = np.argwhere(reached)
        edge = idx[(idx[:, 0] % rxi == 0) | (idx[:, 1] % wi == 0)]
        rng = np.random.default_rng(1024)
        cells = np.unique(np.concatenate([edge[rng.choice(len(edge), min(len(edge), 150), replace=False)],
                                          idx[rng.choice(len(idx), 250, replace=False)]]), axis=0)
        assert len(cells) >= 300 and len(edge) > 0
        local = cells - np.array([r0, c0])
        want = expected_at(history(s, rows, cols), local, delay[rows, cols], s.fs)
        check_cells(got[local[:, 0], local[:, 1]], want, "1024 block")
        assert (want[:, S_EKL] > 0).all()
        whole = s.echo_criterion()
        assert same_bits(whole[rows, cols], got).all()
        whole[rows, cols] = np.nan
        assert np.isnan(whole).all()


# 6. split-field edge layers: the cells inside the layers get records like any other cell
def test_split_layer(pvlib):
    n = 160
    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        s.set_edge_layer_split((24, 24, 24, 24))
        s.run(cell_of(n // 2, n // 3 + 6))
        s.compute_echo_criterion()
        got, delay = s.echo_criterion(), s.results()[1]
        reached = delay < ref.NO_ONSET
        check_nan_pattern(got, reached, "split layer")
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
        check_cells(got[cells[:, 0], cells[:, 1]], expected_at(history(s), cells, delay, s.fs), "split layer")


# 7. a resolution with other lags: fs 1968, nD 17 and 27
def test_other_resolution(pvlib):
    got, delay, (gx, T, fs) = preset_run(pvlib, "g96_smallroom_res375")
    assert gx == 95 and got.shape == (95, 95, 10) and fs == 1968 and ref.lags(fs) == (17, 98, 27, 157)
    reached = delay < ref.NO_ONSET
    check_nan_pattern(got, reached, "res 375")
    g = golden("g96_smallroom_res375")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        assert same_bits(s.results()[1], delay).all()
        hist = history(s)
    idx = np.argwhere(reached)
    assert len(idx) > 3000
    cells = idx[np.random.default_rng(96).choice(len(idx), 1200, replace=False)]
    want = expected_at(hist, cells, delay, fs)
    check_cells(got[cells[:, 0], cells[:, 1]], want, "res 375")
    assert (want[:, S_EK] > 0).all() and (want[:, M_EK] > 0).all()


# 8. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.compute_echo_criterion()
        m = s.echo_criterion()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.echo_criterion_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.echo_criterion_at(e)).all() and s.echo_criterion_at(e).shape == (10,)


#    lifetime: -1 before compute and after a run or a geometry, boundary or layer change; independent of the six other kinds
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        reads = (s.echo_criterion, lambda: s.echo_criterion_at(g["emitters"][0]), lambda: s.echo_criterion_block(0, 0, 2, 2))

        def refused():
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match="^echo: "):
                    call()

        def others():
            s.compute_room_metrics()
            s.compute_spectrum()
            s.compute_decay_times()
            s.compute_lateral_fraction()
            s.compute_band_metrics()
            s.compute_echogram()
            return s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics(), s.echogram()

        refused()  # (not computed yet)
        s.set_spectrum_bins([50.0, 100.0])
        s.set_bands([125.0])
        s.set_echogram(0.005, 16)
        before = others()
        refused()
        s.compute_echo_criterion()
        first = s.echo_criterion()
        assert same_bits(first, want).all()
        for a, b in zip((s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction(), s.band_metrics(), s.echogram()), before):
            assert same_bits(a, b).all()  # (still valid)
        others()
        assert same_bits(s.echo_criterion(), first).all()  # (and the reverse)
        s.set_echogram(0.002, 8)  # (another kind's setting)
        assert same_bits(s.echo_criterion(), first).all()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_echo_criterion()  # (the last completed run is still the first one)
        assert same_bits(s.echo_criterion(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_echo_criterion()
        second = s.echo_criterion()
        assert not same_bits(second, first).all()
        assert np.array_equal(np.isnan(second).all(axis=-1), ~(s.results()[1] < ref.NO_ONSET))
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_echo_criterion()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


#    refusals: an "echo: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^echo: .*history"):
            s.compute_echo_criterion()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^echo: .*onset map"):
            s.compute_echo_criterion()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (s.compute_echo_criterion, s.echo_criterion, lambda: s.echo_criterion_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="^echo: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^echo: no completed run"):
            s.compute_echo_criterion()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="^echo: "):
            s.echo_criterion()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="^echo: no completed run"):
            s.compute_echo_criterion()
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^echo: block outside the map"):
            s.echo_criterion_block(0, 0, s.gx + 1, 1)
        assert s.compute_echo_criterion() > 0
        assert np.isfinite(s.echo_criterion_at(E)).all()


# 9. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    withe = json.loads(subprocess.run(cmd + ["--echo-criterion"], capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                      timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.compute_echo_criterion()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withe["emitters"]):
            m = s.echo_criterion_at(e)
            assert "rt60" in rec and list(rec["echoCriterion"]) == list(pvlib.ECHO_CRITERION_NAMES)
            got = np.array([rec["echoCriterion"][n] for n in pvlib.ECHO_CRITERION_NAMES], np.float32)
            assert same_bits(got, m).all(), (got, m)
