"""GPU (-m gpu): per-cell, per-band decay times and clarity (PvAmdSetBands / PvAmdComputeBandMetrics; pv_bands.hip).

The expected values always come from the numpy restatement (tests/_bands_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t), its own onset map
(results()[1]) and the coefficients the solver itself reports (band_coefs()).  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _bands_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history

pytestmark = pytest.mark.gpu

OCTAVES = [63.0, 125.0, 250.0]


def expected(s):
    return ref.band_metrics(history(s), s.results()[1], s.fs, s.band_coefs())


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    assert got.shape == want.shape and got.dtype == np.float32 and got.shape[-1] == 12
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:4], want[bad][:4])
    # NaN records on exactly the unreached cells: the three counts of a reached cell are numbers
    assert np.array_equal(np.isnan(got).all(axis=(-1, -2)), ~reached), ctx
    assert np.isfinite(got[..., 3:6][reached]).all(), ctx


def solver_of(pvlib, g, **opts):
    s = pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"]), **opts)
    for b in g["boxes"]:
        s.add_geometry(b)
    return s


_PRESET = {}


def preset_run(pvlib, name):
    """plain run of a 70^2 preset scene at its golden listener with the three octaves: (records, delay, restatement, (gx, T, fs))"""
    if name not in _PRESET:
        g = golden(name)
        with solver_of(pvlib, g) as s:
            s.set_bands(OCTAVES)
            s.run(g["listener"])
            assert s.compute_band_metrics() > 0
            assert same_bits(s.band_coefs(), pvlib.host_band_coefs(s.fs, OCTAVES, 1)).all()
            _PRESET[name] = (s.band_metrics(), s.results()[1], expected(s), (s.gx, s.T, s.fs))
    return _PRESET[name]


# how many reached cells have a complete range with n >= 2, [band 63 / 125 / 250][edt, t20, t30]: the restatement on the oracle's
# history of these scenes (oracle/pvoracle.py, the same bits as the device's), computed on the CPU
PRESET_COUNTS = {"g71_smallroom": (4673, [[4673, 4615, 3799], [4673, 4456, 2724], [4673, 3802, 1278]]),
                 "g71_shoebox": (1944, [[1944, 1887, 687], [1944, 1602, 262], [1944, 824, 20]]),
                 "g71_empty": (4900, [[4900, 4900, 4900], [4900, 4900, 4900], [4900, 4900, 4832]])}


# 1. the 70^2 presets (T = 435: the resident path); n = 3: two register blocks, the second one padded
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    got, delay, want, (gx, T, fs) = preset_run(pvlib, name)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, 3, 12)
    check_map(got, want, delay, name)
    reached = delay < ref.NO_ONSET
    valid = ~np.isnan(got[..., :3]) & reached[..., None, None]
    counts = valid.sum(axis=(0, 1))
    print(name, "reached", reached.sum(), "valid [band][edt, t20, t30]", counts.tolist())
    n_reached, table = PRESET_COUNTS[name]
    assert reached.sum() == n_reached and counts.tolist() == table
    # the complete AND the incomplete branch of T20 and T30 occur in a band of this scene (g71_empty: of T30, in the 250 Hz band);
    # every reached cell of the presets has an EDT in every octave (the oracle's count of incomplete EDT ranges is 0: that branch
    # is held by the windowed runs below, whose onsets in the tail leave EDT incomplete)
    for j in ((1, 2) if name != "g71_empty" else (2,)):
        assert ((counts[:, j] > 0) & (counts[:, j] < n_reached)).any()
    # (no band of the presets is empty at a reached cell, and every reached cell has a late part after 50 ms: the oracle's counts)
    assert (got[..., 6][reached] > 0).all() and np.isfinite(got[..., 8][reached]).all() and not np.isnan(got[..., 9][reached]).any()
    assert (got[..., 10][reached] >= 0).all() and (got[..., 10][reached] <= 1).all() and (got[..., 11][reached] >= 0).all()


# 2. more than one register block, a padded last block, n not a multiple of the block: five and eight third octaves
@pytest.mark.parametrize("hz", [[50.0, 63.0, 80.0, 100.0, 125.0], [31.5, 40.0, 63.0, 100.0, 160.0, 250.0, 400.0, 500.0]])
def test_five_and_eight_third_octaves(pvlib, hz):
    g = golden("g71_smallroom")
    with solver_of(pvlib, g) as s:
        s.set_bands(hz, 3)
        assert np.array_equal(s.bands()[0], np.array(hz, np.float32)) and s.bands()[1] == 3
        s.run(g["listener"])
        s.compute_band_metrics()
        got, delay = s.band_metrics(), s.results()[1]
        assert got.shape == (70, 70, len(hz), 12)
        check_map(got, expected(s), delay, "%d third octaves" % len(hz))
        # an octave set afterwards: other records, the ones of the preset run
        s.set_bands(OCTAVES, 1)
        s.compute_band_metrics()
        assert same_bits(s.band_metrics(), preset_run(pvlib, "g71_smallroom")[0]).all()


# 3. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; onsets in the tail
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.set_bands(OCTAVES)
        s.run(L400[where])
        s.compute_band_metrics()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        got = s.band_metrics()
        want = ref.band_metrics(history(s, rows, cols), delay[rows, cols], s.fs, s.band_coefs())
        check_map(got[rows, cols], want, delay[rows, cols], where)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False
        assert np.isnan(got[outside]).all()
        tail = reached & (delay >= s.T - ref.tail_n(s.fs))  # onset at or after tEnd: every range incomplete, EDT included
        assert tail.any() and (reached & (delay < 8)).any()
        assert np.isnan(got[..., :3][tail]).all() and (got[..., 3:6][tail] == 0).all() and np.isnan(got[..., 7][tail]).all()
        assert np.isfinite(got[..., 6][tail]).all()
        assert np.isfinite(got[..., 0][reached & ~tail]).any()


# 4. the same bits on every stepping path
@pytest.mark.parametrize("form", ["resident", "small_grid", "graph"])
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay, _, _ = preset_run(pvlib, "g71_smallroom")
    g = golden("g71_smallroom")
    opts = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
            "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}[form]
    with solver_of(pvlib, g, **opts) as s:
        s.set_bands(OCTAVES)
        s.run_async(g["listener"])
        s.sync()
        s.compute_band_metrics()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.band_metrics(), want).all(), form


# 5. batch members, a second run that reaches fewer cells (nothing is carried over), two solvers in flight
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with solver_of(pvlib, g) as s:
        s.set_bands(OCTAVES)
        s.run(L[1])
        s.compute_band_metrics()
        plain.append(s.band_metrics())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [solver_of(pvlib, g) for _ in L]
    try:
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.set_bands(OCTAVES)  # (after the run: the bands belong to the pass, not to the run)
            s.compute_band_metrics()
            assert same_bits(s.band_metrics(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with solver_of(pvlib, g) as s:
        s.set_bands(OCTAVES)
        s.run(L[0])
        s.compute_band_metrics()
        first, first_reached = s.band_metrics(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_band_metrics()
        got, delay = s.band_metrics(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[..., 6][only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected(s), delay, "walled-in second run")
    # the second of two iterations in flight on two solvers
    with solver_of(pvlib, g) as a, solver_of(pvlib, g) as b:
        b.set_bands(OCTAVES)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_band_metrics()  # (waits for the run in flight)
        assert same_bits(b.band_metrics(), plain[0]).all()
        a.sync()


# 6. few live groups in a big window: a closed room in a 1024-cell grid (waves without a live lane, waves with one)
def test_few_groups_in_a_big_window(pvlib):
    n = 1024
    size = open_size(n)
    with pvlib.Solver(size, size, 275, num_steps=435) as s:
        assert s.gx == n and s.T == 435
        s.load_scene(SHOEBOX)
        s.set_bands(OCTAVES)
        s.run((5.0, 0.0, 4.0))
        s.compute_band_metrics()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.band_metrics_block(r0, c0, r1 - r0, c1 - c0)
        want = ref.band_metrics(history(s, rows, cols), delay[rows, cols], s.fs, s.band_coefs())
        check_map(got, want, delay[rows, cols], "1024 block")
        whole = s.band_metrics()
        assert same_bits(whole[rows, cols], got).all()
        whole[rows, cols] = np.nan
        assert np.isnan(whole).all()


# 7. split-field edge layers: the cells inside the layers get records like any other cell
def test_split_layer(pvlib):
    n = 160
    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        s.set_edge_layer_split((24, 24, 24, 24))
        s.set_bands([63.0, 250.0])
        s.run(cell_of(n // 2, n // 3 + 6))
        s.compute_band_metrics()
        got, delay = s.band_metrics(), s.results()[1]
        reached = delay < ref.NO_ONSET
        assert same_bits(got, expected(s)).all()
        assert np.array_equal(np.isnan(got).all(axis=(-1, -2)), ~reached)
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()


# 8. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with solver_of(pvlib, g) as s:
        s.set_bands(OCTAVES)
        s.run(g["listener"])
        s.compute_band_metrics()
        m = s.band_metrics()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.band_metrics_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.band_metrics_at(e)).all() and s.band_metrics_at(e).shape == (3, 12)


# 9. lifetime: -1 before compute and after a run, a geometry, boundary, layer or BAND change; independent of the other four passes
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with solver_of(pvlib, g) as s:
        s.run(g["listener"])
        reads = (s.band_metrics, lambda: s.band_metrics_at(g["emitters"][0]), lambda: s.band_metrics_block(0, 0, 2, 2))

        def refused(why="band metrics: "):
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match=why):
                    call()

        refused("band metrics: no bands set")
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: no bands set"):
            s.compute_band_metrics()
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: no bands set"):
            s.band_coefs()
        assert len(s.bands()[0]) == 0
        s.set_bands(OCTAVES)
        refused("band metrics: not computed")
        s.set_spectrum_bins([50.0, 100.0])
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        s.compute_lateral_fraction()
        others = lambda: (s.room_metrics(), s.spectrum(), s.decay_times(), s.lateral_fraction())  # noqa: E731
        before = others()
        refused()
        s.compute_band_metrics()
        first = s.band_metrics()
        assert same_bits(first, want).all()
        assert all(same_bits(a, b).all() for a, b in zip(others(), before))  # (the other four are still valid)
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        s.compute_lateral_fraction()
        assert same_bits(s.band_metrics(), first).all()  # (and the reverse)
        # a change of bands invalidates, even to the same bands; the other four stay
        s.set_bands(OCTAVES)
        refused("band metrics: not computed")
        assert all(same_bits(a, b).all() for a, b in zip(others(), before))
        s.set_bands([125.0], 3)
        refused("band metrics: not computed")
        s.compute_band_metrics()
        assert s.band_metrics().shape == (70, 70, 1, 12)
        # a refused change leaves bands and records alone
        for bad in ([63.0, 800.0], [float("nan")], [0.0], [63.0] * 9):
            with pytest.raises(pvlib.PlaneverbError, match="band metrics: "):
                s.set_bands(bad, 3)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: fraction"):
            s.set_bands([63.0], 2)
        assert s.bands()[0].tolist() == [125.0] and s.bands()[1] == 3 and s.band_metrics().shape == (70, 70, 1, 12)
        s.set_bands([])
        refused("band metrics: no bands set")
        s.set_bands(OCTAVES)
        s.compute_band_metrics()
        assert same_bits(s.band_metrics(), first).all()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_band_metrics()  # (the last completed run is still the first one)
        assert same_bits(s.band_metrics(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_band_metrics()
        second = s.band_metrics()
        check_map(second, expected(s), s.results()[1], "second run")
        assert not same_bits(second, first).all()
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_band_metrics()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


# 10. refusals: a "band metrics: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.set_bands(OCTAVES)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*history"):
            s.compute_band_metrics()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_bands(OCTAVES)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*onset map"):
            s.compute_band_metrics()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_bands(OCTAVES), s.compute_band_metrics, s.band_metrics, lambda: s.band_metrics_at(E), s.band_coefs):
            with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: no bands set"):
            s.compute_band_metrics()
        s.set_bands(OCTAVES)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: no completed run"):
            s.compute_band_metrics()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: "):
            s.band_metrics()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: no completed run"):
            s.compute_band_metrics()
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: block outside the map"):
            s.band_metrics_block(0, 0, s.gx + 1, 1)
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*upper edge"):
            s.set_bands([600.0])
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*lower edge"):
            s.set_bands([-1.0])
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: .*not finite"):
            s.set_bands([float("inf")])
        with pytest.raises(pvlib.PlaneverbError, match="band metrics: 0 .. 8 bands"):
            s.set_bands([63.0] * 9)
        s.run(L)
        assert s.compute_band_metrics() > 0
        assert np.isfinite(s.band_metrics_at(E)[:, 3:7]).all()


# 11. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = json.loads(subprocess.run(cmd + ["--bands", "63,125,250", "--band-fraction", "3"], capture_output=True, text=True, check=True,
                                    cwd=ROOT, env=env, timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_bands(OCTAVES, 3)
        s.run((5.0, 0.0, 4.0))
        s.compute_band_metrics()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), out["emitters"]):
            m = s.band_metrics_at(e)
            assert "rt60" in rec and len(rec["bandMetrics"]) == 3
            for j, band in enumerate(rec["bandMetrics"]):
                assert band["hz"] == OCTAVES[j] and band["fraction"] == 3
                assert [k for k in band if k not in ("hz", "fraction")] == list(pvlib.BAND_METRIC_NAMES)
                got = np.array([band[n] for n in pvlib.BAND_METRIC_NAMES], np.float32)
                assert same_bits(got, m[j]).all(), (got, m[j])
