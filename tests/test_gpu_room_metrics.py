"""GPU (-m gpu): per-cell room metrics (PvAmdComputeRoomMetrics: C50, C80, D50, Ts and their six sums; pv_metrics.hip).

The expected values always come from the numpy restatement (tests/_room_metrics_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t) and its own onset map
(results()[1]).  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _room_metrics_ref as ref
from conftest import ROOT, SCENES, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of, walls

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
SHOEBOX = os.path.join(SCENES, "Shoebox.pv")


def history(s, rows=None, cols=None):
    """float32 [T, gx, gy] (or the block rows x cols of it): the recorded pressure of the result cells"""
    rows = slice(0, s.gx) if rows is None else rows
    cols = slice(0, s.gy) if cols is None else cols
    return np.stack([s.history_plane(t)[rows, cols] for t in range(s.T)])


def expected(s):
    return ref.room_metrics(history(s), s.results()[1], s.fs)


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    assert got.shape == want.shape and got.dtype == np.float32
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:4], want[bad][:4])
    # NaN on exactly the unreached cells: the six sums of a reached cell are finite numbers
    assert np.array_equal(np.isnan(got[..., 4:]).all(axis=-1), ~reached), ctx
    assert not np.isnan(got[..., 4:][reached]).any(), ctx


_PRESET = {}


def preset_run(pvlib, name):
    """plain run of a 70^2 preset scene at its golden listener: (metrics, delay); the restatement is checked by test_preset_grid"""
    if name not in _PRESET:
        g = golden(name)
        with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
            for b in g["boxes"]:
                s.add_geometry(b)
            s.run(g["listener"])
            ms = s.compute_room_metrics()
            assert ms > 0
            _PRESET[name] = (s.room_metrics(), s.results()[1], expected(s), (s.gx, s.T, s.fs))
    return _PRESET[name]


# 1. the 70^2 presets (T = 435: the resident / small-grid path)
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    got, delay, want, (gx, T, fs) = preset_run(pvlib, name)
    assert (gx, T, fs) == (70, 435, 1443)
    check_map(got, want, delay, name)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    # not degenerate: the largest onset + n80 < T, so every reached cell has non-empty late windows
    assert delay[reached].max() + ref.n80(fs) < T
    assert np.isfinite(got[..., 0][reached]).all() and np.isfinite(got[..., 1][reached]).all()
    assert (got[..., 4][reached] > 0).all()


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
        s.compute_room_metrics()
        got, delay = s.room_metrics(), s.results()[1]
        check_map(got, expected(s), delay, where)
        reached = delay < ref.NO_ONSET
        late = reached & (delay < s.T - ref.n50(s.fs))
        empty = reached & ~late
        assert late.any() and empty.any()
        assert np.isfinite(got[..., 0][late]).all()
        assert np.isposinf(got[..., 0][empty]).all() and (got[..., 2][empty] == 1).all()


# 3. the same bits on every stepping path
@pytest.mark.parametrize("form", ["resident", "small_grid", "graph"])
def test_same_bits_on_every_path(pvlib, form):
    want, wdelay, _, _ = preset_run(pvlib, "g71_smallroom")
    g = golden("g71_smallroom")
    opts = {"resident": dict(resident_kernel=1), "small_grid": dict(resident_kernel=2, small_grid_kernel=1),
            "graph": dict(resident_kernel=2, small_grid_kernel=2, use_graph=1)}[form]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"]), **opts) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run_async(g["listener"])
        s.sync()
        s.compute_room_metrics()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.room_metrics(), want).all(), form


def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    size, res = float(g["size"]), int(g["res"])
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = []
    for l in L:
        with pvlib.Solver(size, size, res) as s:
            for b in g["boxes"]:
                s.add_geometry(b)
            s.run(l)
            s.compute_room_metrics()
            plain.append(s.room_metrics())
    assert same_bits(plain[0], preset_run(pvlib, "g71_smallroom")[0]).all()
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [pvlib.Solver(size, size, res) for _ in L]
    try:
        for s in solvers:
            for b in g["boxes"]:
                s.add_geometry(b)
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_room_metrics()
            assert same_bits(s.room_metrics(), w).all()
    finally:
        for s in solvers:
            s.close()
    # the second of two iterations in flight on two solvers: its no-onset cells carry the first one's RESULTS, not its metrics
    with pvlib.Solver(size, size, res) as a, pvlib.Solver(size, size, res) as b:
        for s in (a, b):
            for bx in g["boxes"]:
                s.add_geometry(bx)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_room_metrics()  # (waits for the run in flight)
        got = b.room_metrics()
        assert same_bits(got, plain[0]).all()
        check_map(got, expected(b), b.results()[1], "carried")
        a.sync()


# 4. few live groups in a big window: a closed room in a 1024-cell grid
def test_few_groups_in_a_big_window(pvlib):
    n = 1024
    size = open_size(n)
    with pvlib.Solver(size, size, 275, num_steps=435) as s:
        assert s.gx == n and s.T == 435
        s.load_scene(SHOEBOX)
        s.run((5.0, 0.0, 4.0))
        s.compute_room_metrics()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.room_metrics_block(r0, c0, r1 - r0, c1 - c0)
        want = ref.room_metrics(history(s, rows, cols), delay[rows, cols], s.fs)
        check_map(got, want, delay[rows, cols], "1024 block")
        assert np.isfinite(got[..., 0][reached[rows, cols]]).all()
        whole = s.room_metrics()
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
        s.compute_room_metrics()
        got, delay = s.room_metrics(), s.results()[1]
        check_map(got, expected(s), delay, "split layer")
        reached = delay < ref.NO_ONSET
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()


# 6. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        s.compute_room_metrics()
        m = s.room_metrics()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.room_metrics_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.room_metrics_at(e)).all() and s.room_metrics_at(e).shape == (10,)


def cell_and_valid(pvlib, g, e):
    """(result cx, result cy, valid) of PvAmdHostCells: the cell PvAmdGetOutput reads"""
    _, rc = pvlib.host_cells(float(g["size"]), float(g["size"]), int(g["res"]), e[0], e[2])
    return (rc[0], rc[1], True) if rc is not None else (-1, -1, False)


# 7. lifetime: valid until the next run or geometry change
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        s.compute_room_metrics()
        first = s.room_metrics()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        for call in (s.room_metrics, lambda: s.room_metrics_at(g["emitters"][0]), lambda: s.room_metrics_block(0, 0, 2, 2)):
            with pytest.raises(pvlib.PlaneverbError, match="room metrics"):
                call()
        s.compute_room_metrics()  # (the last completed run is still the first one)
        assert same_bits(s.room_metrics(), first).all()
        s.run((7.0, 0.0, 9.5))
        with pytest.raises(pvlib.PlaneverbError, match="room metrics"):
            s.room_metrics()
        s.compute_room_metrics()
        second = s.room_metrics()
        check_map(second, expected(s), s.results()[1], "second run")
        assert not same_bits(second, first).all()
        s.set_grid_boundary((1, 0, 0, 0))
        with pytest.raises(pvlib.PlaneverbError):
            s.room_metrics()
        s.compute_room_metrics()
        s.set_edge_layer((8, 8, 8, 8))
        with pytest.raises(pvlib.PlaneverbError):
            s.room_metrics()
        s.remove_geometry(gid)


# 8. refusals: an error message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="history"):
            s.compute_room_metrics()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="onset map"):
            s.compute_room_metrics()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            s.compute_room_metrics()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            s.room_metrics_at(E)
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="no completed run"):
            s.compute_room_metrics()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="room metrics"):
            s.room_metrics()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="no completed run"):
            s.compute_room_metrics()
        s.run(L)
        assert s.compute_room_metrics() > 0
        assert np.isfinite(s.room_metrics_at(E)).all()


# 9. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    plain = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout)
    withm = json.loads(subprocess.run(cmd + ["--room-metrics"], capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                      timeout=300).stdout)
    assert all("roomMetrics" not in e for e in plain["emitters"]) and "roomMetrics" not in plain
    assert [sorted(e) for e in plain["emitters"]] == [sorted(k for k in e if k != "roomMetrics") for e in withm["emitters"]]
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.compute_room_metrics()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withm["emitters"]):
            m = s.room_metrics_at(e)
            assert list(rec["roomMetrics"]) == list(pvlib.ROOM_METRIC_NAMES)
            got = np.array([rec["roomMetrics"][n] for n in pvlib.ROOM_METRIC_NAMES], np.float32)
            assert same_bits(got, m).all(), (got, m)
