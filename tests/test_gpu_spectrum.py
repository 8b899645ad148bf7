"""GPU (-m gpu): per-cell transfer functions at chosen frequencies (PvAmdComputeSpectrum; pv_spectrum.hip).

The expected values always come from the numpy restatement (tests/_spectrum_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t), its own onset map
(results()[1]), its pulse() and the tables of host_spectrum_tables.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _spectrum_ref as ref
from conftest import ROOT, SCENES, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of, walls

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
SHOEBOX = os.path.join(SCENES, "Shoebox.pv")
BINS8 = [0, 30, 61.7, 100, 137.5, 200, 250, 275]
BINS = {1: [137.5], 8: BINS8, 9: BINS8 + [300.0], 32: [float(v) for v in np.linspace(0.0, 1443 / 2.0, 32)]}


def history(s, rows=None, cols=None):
    """float32 [T, gx, gy] (or the block rows x cols of it): the recorded pressure of the result cells"""
    rows = slice(0, s.gx) if rows is None else rows
    cols = slice(0, s.gy) if cols is None else cols
    return np.stack([s.history_plane(t)[rows, cols] for t in range(s.T)])


def expected(pvlib, s, hist=None, delay=None):
    hz = s.spectrum_bins()
    c, sn = pvlib.host_spectrum_tables(s.T, s.fs, hz)
    return ref.spectrum(history(s) if hist is None else hist, s.results()[1] if delay is None else delay, c, sn, s.pulse())


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    assert got.shape == want.shape and got.dtype == np.float32
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:4], want[bad][:4])
    # NaN on exactly the unreached cells: the two sums of a reached cell are finite numbers
    assert np.array_equal(np.isnan(got[..., :2]).all(axis=(-1, -2)), ~reached), ctx
    assert not np.isnan(got[..., :2][reached]).any(), ctx


def load(s, g):
    for b in g["boxes"]:
        s.add_geometry(b)


_PRESET = {}


def smallroom_run(pvlib):
    """plain run of g71_smallroom at its golden listener with BINS8: (records, delay)"""
    if "v" not in _PRESET:
        g = golden("g71_smallroom")
        with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
            load(s, g)
            s.run(g["listener"])
            s.set_spectrum_bins(BINS8)
            s.compute_spectrum()
            _PRESET["v"] = (s.spectrum(), s.results()[1])
    return _PRESET["v"]


# 1. the 70^2 presets (T = 435: the resident path); on g71_smallroom also one bin, one past a block of 8, and the maximum
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    g = golden(name)
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        assert (s.gx, s.T, s.fs) == (70, 435, 1443)
        load(s, g)
        s.run(g["listener"])
        hist, delay = history(s), s.results()[1]
        reached = delay < ref.NO_ONSET
        assert reached.sum() > 1000
        for n in ((8, 1, 9, 32) if name == "g71_smallroom" else (8,)):
            s.set_spectrum_bins(BINS[n])
            assert same_bits(s.spectrum_bins(), np.array(BINS[n], np.float32)).all()
            assert s.compute_spectrum() > 0
            got = s.spectrum()
            assert got.shape == (70, 70, n, 3)
            check_map(got, expected(pvlib, s, hist, delay), delay, "%s n=%d" % (name, n))
            if n == 8:
                assert np.isfinite(got[reached]).all()
                assert (np.abs(got[..., 1:, 1][reached]) > 0).any()  # (not degenerate: imaginary parts away from 0 Hz)
                if name == "g71_smallroom":
                    assert same_bits(got, smallroom_run(pvlib)[0]).all()


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0
N400 = 400
L400 = {"centre": cell_of(200, 200), "corner": cell_of(3, 3), "offset": cell_of(250, 130)}


@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        s.set_spectrum_bins(BINS[9])
        s.compute_spectrum()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        got = s.spectrum()
        check_map(got[rows, cols], expected(pvlib, s, history(s, rows, cols), delay[rows, cols]), delay[rows, cols], where)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False
        assert np.isnan(got[outside]).all()
        assert (reached & (delay >= s.T - 4)).any() and (reached & (delay < 8)).any()  # late-onset cells and early ones


# 3. the same bits on every stepping path
@pytest.mark.parametrize("form", ["resident", "small_grid", "graph"])
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay = smallroom_run(pvlib)
    g = golden("g71_smallroom")
    opts = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
            "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}[form]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"]), **opts) as s:
        load(s, g)
        s.set_spectrum_bins(BINS8)  # (before the first run)
        s.run_async(g["listener"])
        s.sync()
        s.compute_spectrum()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.spectrum(), want).all(), form


def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    size, res = float(g["size"]), int(g["res"])
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [smallroom_run(pvlib)[0]]
    with pvlib.Solver(size, size, res) as s:
        load(s, g)
        s.run(L[1])
        s.set_spectrum_bins(BINS8)
        s.compute_spectrum()
        plain.append(s.spectrum())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [pvlib.Solver(size, size, res) for _ in L]
    try:
        for s in solvers:
            load(s, g)
            s.set_spectrum_bins(BINS8)
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_spectrum()
            assert same_bits(s.spectrum(), w).all()
    finally:
        for s in solvers:
            s.close()
    # the second of two iterations in flight on two solvers: its no-onset cells carry the first one's RESULTS, not its records
    with pvlib.Solver(size, size, res) as a, pvlib.Solver(size, size, res) as b:
        for s in (a, b):
            load(s, g)
        b.set_spectrum_bins(BINS8)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_spectrum()  # (waits for the run in flight)
        got = b.spectrum()
        assert same_bits(got, plain[0]).all()
        check_map(got, expected(pvlib, b), b.results()[1], "carried")
        a.sync()


# 4. few live groups in a big window: a closed room in a 1024-cell grid
def test_few_groups_in_a_big_window(pvlib):
    n = 1024
    size = open_size(n)
    with pvlib.Solver(size, size, 275, num_steps=435) as s:
        assert s.gx == n and s.T == 435
        s.load_scene(SHOEBOX)
        s.run((5.0, 0.0, 4.0))
        s.set_spectrum_bins(BINS8)
        s.compute_spectrum()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.spectrum_block(r0, c0, r1 - r0, c1 - c0)
        check_map(got, expected(pvlib, s, history(s, rows, cols), delay[rows, cols]), delay[rows, cols], "1024 block")
        whole = s.spectrum()
        assert same_bits(whole[rows, cols], got).all()
        whole[rows, cols] = np.nan
        assert np.isnan(whole).all()


# 5. split-field edge layers: the cells inside the layers get records like any other cell
def test_split_layer(pvlib):
    n = 160
    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        s.set_edge_layer_split((24, 24, 24, 24))
        s.run(cell_of(n // 2, n // 3 + 6))
        s.set_spectrum_bins(BINS8)
        s.compute_spectrum()
        got, delay = s.spectrum(), s.results()[1]
        check_map(got, expected(pvlib, s), delay, "split layer")
        reached = delay < ref.NO_ONSET
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()


def cell_and_valid(pvlib, g, e):
    """(result cx, result cy, valid) of PvAmdHostCells: the cell PvAmdGetOutput reads"""
    _, rc = pvlib.host_cells(float(g["size"]), float(g["size"]), int(g["res"]), e[0], e[2])
    return (rc[0], rc[1], True) if rc is not None else (-1, -1, False)


# 6. the point query reads the cell get_output reads; the source values are the restatement's on pulse()
def test_point_query_and_source(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        load(s, g)
        s.run(g["listener"])
        s.set_spectrum_bins(BINS[9])
        c, sn = pvlib.host_spectrum_tables(s.T, s.fs, s.spectrum_bins())
        src = s.spectrum_source()
        assert src.shape == (9, 3) and same_bits(src, ref.source(s.pulse(), c, sn)).all()
        assert (src[:, 2] > 0).all()
        s.compute_spectrum()
        m = s.spectrum()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.spectrum_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.spectrum_at(e)).all() and s.spectrum_at(e).shape == (9, 3)


# 7. lifetime: valid until the next run, geometry, boundary, layer or bin change; independent of the room metrics
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        load(s, g)
        s.run(g["listener"])
        s.set_spectrum_bins(BINS8)
        s.compute_room_metrics()
        metrics = s.room_metrics()
        s.compute_spectrum()
        first = s.spectrum()
        assert same_bits(first, smallroom_run(pvlib)[0]).all()
        assert same_bits(s.room_metrics(), metrics).all()  # (still valid)
        s.compute_room_metrics()
        assert same_bits(s.spectrum(), first).all()  # (and the reverse)
        # a bin change
        s.set_spectrum_bins(BINS[9])
        for call in (s.spectrum, lambda: s.spectrum_at(g["emitters"][0]), lambda: s.spectrum_block(0, 0, 2, 2)):
            with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
                call()
        assert same_bits(s.room_metrics(), metrics).all()
        s.compute_spectrum()  # (the device planes are allocated again: nine bins)
        assert same_bits(s.spectrum()[:, :, :8], first).all()
        s.set_spectrum_bins(BINS8)
        s.compute_spectrum()
        assert same_bits(s.spectrum(), first).all()
        # refused bins change nothing
        for bad in ([float("nan")], [-1.0], [s.fs / 2.0 + 1.0], [1.0] * 33):
            with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
                s.set_spectrum_bins(bad)
        assert same_bits(s.spectrum_bins(), np.array(BINS8, np.float32)).all() and same_bits(s.spectrum(), first).all()
        # geometry
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
            s.spectrum()
        s.compute_spectrum()  # (the last completed run is still the first one)
        assert same_bits(s.spectrum(), first).all()
        # a new run
        s.run((7.0, 0.0, 9.5))
        with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
            s.spectrum()
        s.compute_spectrum()
        second = s.spectrum()
        check_map(second, expected(pvlib, s), s.results()[1], "second run")
        assert not same_bits(second, first).all()
        s.set_grid_boundary((1, 0, 0, 0))
        with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
            s.spectrum()
        s.compute_spectrum()
        s.set_edge_layer((8, 8, 8, 8))
        with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
            s.spectrum()
        s.remove_geometry(gid)
        # clearing the bins
        s.set_spectrum_bins([])
        assert len(s.spectrum_bins()) == 0
        with pytest.raises(pvlib.PlaneverbError, match="no bins"):
            s.compute_spectrum()


# 8. refusals: an error message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.set_spectrum_bins(BINS8)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: .*history"):
            s.compute_spectrum()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_spectrum_bins(BINS8)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: .*onset map"):
            s.compute_spectrum()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_spectrum_bins(BINS8), s.compute_spectrum, lambda: s.spectrum_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: no bins"):
            s.compute_spectrum()
        s.set_spectrum_bins(BINS8)
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: no completed run"):
            s.compute_spectrum()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="spectrum"):
            s.spectrum()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: no completed run"):
            s.compute_spectrum()
        s.run(L)
        s.set_spectrum_bins([])
        with pytest.raises(pvlib.PlaneverbError, match="spectrum: no bins"):
            s.compute_spectrum()
        s.set_spectrum_bins(BINS8)
        assert s.compute_spectrum() > 0
        assert np.isfinite(s.spectrum_at(E)).all()


# 9. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    plain = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout)
    withs = json.loads(subprocess.run(cmd + ["--spectrum", "50,100,200"], capture_output=True, text=True, check=True, cwd=ROOT,
                                      env=env, timeout=300).stdout)
    assert all("spectrum" not in e for e in plain["emitters"]) and "spectrum" not in plain
    assert sorted(plain) == sorted(withs)
    assert [sorted(e) for e in plain["emitters"]] == [sorted(k for k in e if k != "spectrum") for e in withs["emitters"]]
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.set_spectrum_bins([50, 100, 200])
        s.compute_spectrum()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withs["emitters"]):
            m = s.spectrum_at(e)
            assert list(rec["spectrum"]) == ["hz", "re", "im", "levelDb"] and rec["spectrum"]["hz"] == [50.0, 100.0, 200.0]
            got = np.array([rec["spectrum"][k] for k in ("re", "im", "levelDb")], np.float32).T
            assert same_bits(got, m).all(), (got, m)
