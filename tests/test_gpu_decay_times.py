"""GPU (-m gpu): per-cell decay times (PvAmdComputeDecayTimes: EDT, T20, T30, their point counts, E0 and the curve's depth;
pv_decay.hip).

The expected values always come from the numpy restatement (tests/_decay_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t) and its own onset map
(results()[1]).  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _decay_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history

pytestmark = pytest.mark.gpu


def expected(s):
    return ref.decay_times(history(s), s.results()[1], s.fs)


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    assert got.shape == want.shape and got.dtype == np.float32
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:4], want[bad][:4])
    # NaN records on exactly the unreached cells: the three counts and E0 of a reached cell are numbers
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached), ctx
    assert np.isfinite(got[..., 3:7][reached]).all() and (got[..., 6][reached] > 0).all(), ctx


_PRESET = {}


def preset_run(pvlib, name):
    """plain run of a 70^2 preset scene at its golden listener: (records, delay, restatement, (gx, T, fs))"""
    if name not in _PRESET:
        g = golden(name)
        with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
            for b in g["boxes"]:
                s.add_geometry(b)
            s.run(g["listener"])
            assert s.compute_decay_times() > 0
            _PRESET[name] = (s.decay_times(), s.results()[1], expected(s), (s.gx, s.T, s.fs))
    return _PRESET[name]


# 1. the 70^2 presets (T = 435: the resident path); both branches of every range are present
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    got, delay, want, (gx, T, fs) = preset_run(pvlib, name)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, 8)
    check_map(got, want, delay, name)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    valid = ~np.isnan(got[..., :3]) & reached[..., None]
    print(name, "reached", reached.sum(), "valid edt/t20/t30", valid.sum(axis=(0, 1)), "fit points min/median",
          got[..., 3:6][valid].min(), np.median(got[..., 3:6][valid]))
    assert valid[..., 0][reached].all()  # (every reached cell of the presets has an EDT)
    if name == "g71_smallroom":
        assert valid[..., 2].sum() >= 1000 and (reached & ~valid[..., 2]).sum() >= 100
    elif name == "g71_shoebox":
        assert valid[..., 1].sum() >= 500 and (reached & ~valid[..., 1]).sum() >= 500
    else:
        assert valid[reached].all()
    assert (got[..., 3:6][valid] >= 2).all() and (got[..., 7][reached] < 0).all()
    assert (np.isfinite(got[..., :3][valid]) & (got[..., :3][valid] > 0)).all()  # (no time of the presets is non-positive or infinite)


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; onsets in the tail
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        s.compute_decay_times()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        got = s.decay_times()
        check_map(got[rows, cols], ref.decay_times(history(s, rows, cols), delay[rows, cols], s.fs), delay[rows, cols], where)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False
        assert np.isnan(got[outside]).all()
        tail = reached & (delay >= s.T - ref.tail_n(s.fs))  # onset at or after tEnd
        assert tail.any() and (reached & (delay < 8)).any()
        assert np.isnan(got[..., :3][tail]).all() and (got[..., 3:6][tail] == 0).all() and np.isnan(got[..., 7][tail]).all()
        assert np.isfinite(got[..., 6][tail]).all()


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
        s.compute_decay_times()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.decay_times(), want).all(), form


# 4. batch members, and a second run that reaches fewer cells: nothing is carried over
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    size, res = float(g["size"]), int(g["res"])
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with pvlib.Solver(size, size, res) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(L[1])
        s.compute_decay_times()
        plain.append(s.decay_times())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [pvlib.Solver(size, size, res) for _ in L]
    try:
        for s in solvers:
            for b in g["boxes"]:
                s.add_geometry(b)
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_decay_times()
            assert same_bits(s.decay_times(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with pvlib.Solver(size, size, res) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(L[0])
        s.compute_decay_times()
        first, first_reached = s.decay_times(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_decay_times()
        got, delay = s.decay_times(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[..., 6][only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected(s), delay, "walled-in second run")
    # the second of two iterations in flight on two solvers: its no-onset cells carry the first one's RESULTS, not its records
    with pvlib.Solver(size, size, res) as a, pvlib.Solver(size, size, res) as b:
        for s in (a, b):
            for bx in g["boxes"]:
                s.add_geometry(bx)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_decay_times()  # (waits for the run in flight)
        got = b.decay_times()
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
        s.compute_decay_times()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.decay_times_block(r0, c0, r1 - r0, c1 - c0)
        check_map(got, ref.decay_times(history(s, rows, cols), delay[rows, cols], s.fs), delay[rows, cols], "1024 block")
        whole = s.decay_times()
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
        s.compute_decay_times()
        got, delay = s.decay_times(), s.results()[1]
        reached = delay < ref.NO_ONSET
        want = expected(s)
        assert same_bits(got, want).all()
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached)
        assert reached[:24].any() and reached[-24:].any() and reached[:, :24].any() and reached[:, -24:].any()


# 7. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        s.compute_decay_times()
        m = s.decay_times()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.decay_times_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.decay_times_at(e)).all() and s.decay_times_at(e).shape == (8,)


# 8. lifetime: -1 before compute and after a run, a geometry, boundary or layer change; independent of metrics and spectrum
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        reads = (s.decay_times, lambda: s.decay_times_at(g["emitters"][0]), lambda: s.decay_times_block(0, 0, 2, 2))

        def refused():
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match="decay times: "):
                    call()

        refused()  # (not computed yet)
        s.set_spectrum_bins([50.0, 100.0])
        s.compute_room_metrics()
        s.compute_spectrum()
        metrics, spectrum = s.room_metrics(), s.spectrum()
        refused()
        s.compute_decay_times()
        first = s.decay_times()
        assert same_bits(first, want).all()
        assert same_bits(s.room_metrics(), metrics).all() and same_bits(s.spectrum(), spectrum).all()  # (still valid)
        s.compute_room_metrics()
        s.compute_spectrum()
        assert same_bits(s.decay_times(), first).all()  # (and the reverse)
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_decay_times()  # (the last completed run is still the first one)
        assert same_bits(s.decay_times(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_decay_times()
        second = s.decay_times()
        check_map(second, expected(s), s.results()[1], "second run")
        assert not same_bits(second, first).all()
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_decay_times()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


# 9. refusals: a "decay times: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="decay times: .*history"):
            s.compute_decay_times()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="decay times: .*onset map"):
            s.compute_decay_times()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (s.compute_decay_times, s.decay_times, lambda: s.decay_times_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="decay times: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="decay times: no completed run"):
            s.compute_decay_times()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="decay times: "):
            s.decay_times()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="decay times: no completed run"):
            s.compute_decay_times()
        s.run(L)
        assert s.compute_decay_times() > 0
        assert np.isfinite(s.decay_times_at(E)[3:7]).all()


# 10. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    withd = json.loads(subprocess.run(cmd + ["--decay-times"], capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                      timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.compute_decay_times()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withd["emitters"]):
            m = s.decay_times_at(e)
            assert "rt60" in rec and list(rec["decayTimes"]) == list(pvlib.DECAY_TIME_NAMES)
            got = np.array([rec["decayTimes"][n] for n in pvlib.DECAY_TIME_NAMES], np.float32)
            assert same_bits(got, m).all(), (got, m)
