"""GPU (-m gpu): per-cell early lateral energy fraction and early-sound direction (PvAmdComputeLateralFraction; pv_lateral.hip).

The expected values come from the numpy restatement (tests/_lateral_ref.py, written from the definition in
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

import _lateral_ref as ref
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of, walls
from test_gpu_room_metrics import L400, N400, SHOEBOX, SMALLROOM, cell_and_valid, history
from test_host_lateral import oracle_run

pytestmark = pytest.mark.gpu


def expected_at(s, cells, delay):
    """the restatement on impulse_response of the given result cells [(x, y)]: float32 [len(cells), 11]"""
    irs = np.stack([s.impulse_response(int(x), int(y)) for x, y in cells], axis=1)  # [T, N, 3]
    d = np.array([delay[x, y] for x, y in cells], np.float32)
    return ref.lateral_fraction(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs)


def expected_map(s, delay):
    """the same for every reached cell of the map: float32 [gx, gy, 11], NaN without an onset"""
    out = np.full(delay.shape + (11,), np.nan, np.float32)
    cells = np.argwhere(delay < ref.NO_ONSET)
    if len(cells):
        out[cells[:, 0], cells[:, 1]] = expected_at(s, cells, delay)
    return out


def check_cells(got, want, ctx):
    assert got.shape == want.shape and got.dtype == np.float32
    bad = ~same_bits(got, want)
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, np.argwhere(bad)[0], got[bad][:4], want[bad][:4])


def check_map(got, want, delay, ctx):
    reached = delay < ref.NO_ONSET
    check_cells(got, want, ctx)
    # NaN records on exactly the unreached cells: n, e80 and the five sums of a reached cell are numbers
    assert np.array_equal(np.isnan(got).all(axis=-1), ~reached), ctx
    assert np.isfinite(got[..., 3:5][reached]).all() and np.isfinite(got[..., 6:][reached]).all(), ctx
    assert (got[..., 3][reached] >= 1).all() and (got[..., 4][reached] > 0).all(), ctx


def preset_solver(pvlib, g, **opts):
    s = pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"]), **opts)
    for b in g["boxes"]:
        s.add_geometry(b)
    return s


_PRESET = {}


def preset_run(pvlib, name):
    """plain run of a 70^2 preset scene at its golden listener: (records, delay, (gx, T, fs))"""
    if name not in _PRESET:
        g = golden(name)
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            assert s.compute_lateral_fraction() > 0
            _PRESET[name] = (s.lateral_fraction(), s.results()[1], (s.gx, s.T, s.fs))
    return _PRESET[name]


# 1. the 70^2 presets (T = 435: the resident path) against the oracle's recorded pr / vx / vy
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, oracle, name):
    got, delay, (gx, T, fs) = preset_run(pvlib, name)
    assert (gx, T, fs) == (70, 435, 1443) and got.shape == (70, 70, 11)
    p, vx, vy, odelay, ofs = oracle_run(oracle, name)
    assert ofs == fs and same_bits(delay, odelay).all()
    want = ref.lateral_fraction(p, vx, vy, delay, fs)
    check_map(got, want, delay, name)
    reached = delay < ref.NO_ONSET
    assert reached.sum() > 1000
    lf = got[..., 0][reached]
    print(name, "reached", reached.sum(), "lf median / p90 / max", np.median(lf), np.percentile(lf, 90), lf.max())
    assert (got[..., 3][reached] == ref.n80(fs)).all() and np.isfinite(got[reached]).all()
    if name == "g71_shoebox":
        # the same with vx, vy of impulse_response, every reached cell: the two expectations agree with each other too
        g = golden(name)
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            want_ir = expected_map(s, delay)
        check_cells(want_ir, want, name + ": impulse_response against the oracle")
        check_map(got, want_ir, delay, name + ": impulse_response")


# 2. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0; neighbours across
#    tile edges, across the window edge and in tiles recorded from a later launch; windows cut off by T
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        s.compute_lateral_fraction()
        got, delay = s.lateral_fraction(), s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False
        assert np.isnan(got[outside]).all()
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached)

        rxi, wi, K = s.info.tileRows, s.info.tileCols, s.info.stepsPerLaunch
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]  # (the listener's cell)
        first_row, first_col = (X % rxi == 0), (Y % wi == 0)
        # Neighbour tiles recorded from a later launch: first-row / first-column cells of tiles that lie above / left of the
        # listener's tile, so that the neighbour tile is a whole tile (rxi, wi >= K steps) further from the listener, AND whose
        # neighbour tile's first non-zero step tnz is at least K later than their own (a tile is recorded from the launch in which
        # the pulse first reached it: tileFirst <= tnz < tileFirst + K)
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
        # the window is tile-aligned and holds every cell the pulse can reach: its first row / column can hold reached cells
        # only where the grid's edge clips it, i.e. at X = 0 / Y = 0 (the corner listener)
        edge = (X == 0) | (Y == 0)
        cut = delay + ref.n80(s.fs) > s.T  # n < n80
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
        want = expected_at(s, cells, delay)
        check_cells(got[cells[:, 0], cells[:, 1]], want, where)
        n = got[..., 3]
        assert (n[reached & cut] < ref.n80(s.fs)).all() and (n[reached & ~cut] == ref.n80(s.fs)).all()


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
        s.compute_lateral_fraction()
        assert same_bits(s.results()[1], wdelay).all()
        assert same_bits(s.lateral_fraction(), want).all(), form


# 4. batch members, and a second run that reaches fewer cells: nothing is carried over
def test_batch_members_and_carried_runs(pvlib):
    g = golden("g71_smallroom")
    size, res = float(g["size"]), int(g["res"])
    L = [tuple(g["listener"]), (7.0, 0.0, 9.5)]
    plain = [preset_run(pvlib, "g71_smallroom")[0]]
    with preset_solver(pvlib, g) as s:
        s.run(L[1])
        s.compute_lateral_fraction()
        plain.append(s.lateral_fraction())
    assert not same_bits(plain[0], plain[1]).all()
    solvers = [preset_solver(pvlib, g) for _ in L]
    try:
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            s.compute_lateral_fraction()
            assert same_bits(s.lateral_fraction(), w).all()
    finally:
        for s in solvers:
            s.close()
    # a walled-in listener after an open one on the same solver: the cells only the first run reached hold NaN
    with preset_solver(pvlib, g) as s:
        s.run(L[0])
        s.compute_lateral_fraction()
        first, first_reached = s.lateral_fraction(), s.results()[1] < ref.NO_ONSET
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)
        s.run(L[1])
        s.compute_lateral_fraction()
        got, delay = s.lateral_fraction(), s.results()[1]
        reached = delay < ref.NO_ONSET
        only_first = first_reached & ~reached
        assert 4 <= reached.sum() < 200 and only_first.sum() > 1000
        assert not np.isnan(first[..., 4][only_first]).any() and np.isnan(got[only_first]).all()
        check_map(got, expected_map(s, delay), delay, "walled-in second run")
    # the second of two iterations in flight on two solvers reads its own run
    with preset_solver(pvlib, g) as a, preset_solver(pvlib, g) as b:
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.compute_lateral_fraction()  # (waits for the run in flight)
        got = b.lateral_fraction()
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
        s.compute_lateral_fraction()
        delay = s.results()[1]
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert 1000 < reached.sum() < 20000
        r0, r1, c0, c1 = max(xs.min() - 3, 0), xs.max() + 4, max(ys.min() - 3, 0), ys.max() + 4
        rows, cols = slice(r0, r1), slice(c0, c1)
        got = s.lateral_fraction_block(r0, c0, r1 - r0, c1 - c0)
        assert np.array_equal(np.isnan(got).all(axis=-1), ~reached[rows, cols])
        rxi, wi = s.info.tileRows, s.info.tileCols
        idx = np.argwhere(reached)
        edge = idx[(idx[:, 0] % rxi == 0) | (idx[:, 1] % wi == 0)]
        rng = np.random.default_rng(1024)
        cells = np.unique(np.concatenate([edge[rng.choice(len(edge), min(len(edge), 150), replace=False)],
                                          idx[rng.choice(len(idx), 250, replace=False)]]), axis=0)
        assert len(cells) >= 300 and len(edge) > 0
        check_cells(got[cells[:, 0] - r0, cells[:, 1] - c0], expected_at(s, cells, delay), "1024 block")
        whole = s.lateral_fraction()
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
        s.compute_lateral_fraction()
        got, delay = s.lateral_fraction(), s.results()[1]
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
        check_cells(got[cells[:, 0], cells[:, 1]], expected_at(s, cells, delay), "split layer")


# 7. the point query reads the cell get_output reads
def test_point_query(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        s.compute_lateral_fraction()
        m = s.lateral_fraction()
        res, _ = s.results()
        emitters = [tuple(e) for e in g["emitters"]] + [cell_of(0, 0), cell_of(69, 69), cell_of(69, 0), (7.3, 1.0, 3.1)]
        for e in emitters:
            rcx, rcy, valid = cell_and_valid(pvlib, g, e)
            assert valid
            assert same_bits(s.get_output(e).as_array(), res[rcx, rcy]).all()
            assert same_bits(s.lateral_fraction_at(e), m[rcx, rcy]).all(), e
        for e in (cell_of(70, 10), cell_of(10, 70), (-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)):
            assert not cell_and_valid(pvlib, g, e)[2]
            assert np.isnan(s.lateral_fraction_at(e)).all() and s.lateral_fraction_at(e).shape == (11,)


# 8. lifetime: -1 before compute and after a run, a geometry, boundary or layer change; independent of the other records
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib, "g71_smallroom")[0]
    with preset_solver(pvlib, g) as s:
        s.run(g["listener"])
        reads = (s.lateral_fraction, lambda: s.lateral_fraction_at(g["emitters"][0]), lambda: s.lateral_fraction_block(0, 0, 2, 2))

        def refused():
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: "):
                    call()

        refused()  # (not computed yet)
        s.set_spectrum_bins([50.0, 100.0])
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        metrics, spectrum, decay = s.room_metrics(), s.spectrum(), s.decay_times()
        refused()
        s.compute_lateral_fraction()
        first = s.lateral_fraction()
        assert same_bits(first, want).all()
        assert same_bits(s.room_metrics(), metrics).all() and same_bits(s.spectrum(), spectrum).all()  # (still valid)
        assert same_bits(s.decay_times(), decay).all()
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        assert same_bits(s.lateral_fraction(), first).all()  # (and the reverse)
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused()
        s.compute_lateral_fraction()  # (the last completed run is still the first one)
        assert same_bits(s.lateral_fraction(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused()
        s.compute_lateral_fraction()
        second = s.lateral_fraction()
        assert not same_bits(second, first).all()
        assert np.array_equal(np.isnan(second).all(axis=-1), ~(s.results()[1] < ref.NO_ONSET))
        s.set_grid_boundary((1, 0, 0, 0))
        refused()
        s.compute_lateral_fraction()
        s.set_edge_layer((8, 8, 8, 8))
        refused()
        s.remove_geometry(gid)


# 9. refusals: a "lateral fraction: ..." message each, and the solver goes on working
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: .*history"):
            s.compute_lateral_fraction()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: .*onset map"):
            s.compute_lateral_fraction()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (s.compute_lateral_fraction, s.lateral_fraction, lambda: s.lateral_fraction_at(E)):
            with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: no completed run"):
            s.compute_lateral_fraction()
        assert pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: "):
            s.lateral_fraction()
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="lateral fraction: no completed run"):
            s.compute_lateral_fraction()
        s.run(L)
        assert s.compute_lateral_fraction() > 0
        assert np.isfinite(s.lateral_fraction_at(E)).all()


# 10. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    withl = json.loads(subprocess.run(cmd + ["--lateral-fraction"], capture_output=True, text=True, check=True, cwd=ROOT, env=env,
                                      timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.compute_lateral_fraction()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), withl["emitters"]):
            m = s.lateral_fraction_at(e)
            assert "rt60" in rec and list(rec["lateralFraction"]) == list(pvlib.LATERAL_FRACTION_NAMES)
            got = np.array([rec["lateralFraction"][n] for n in pvlib.LATERAL_FRACTION_NAMES], np.float32)
            assert same_bits(got, m).all(), (got, m)
