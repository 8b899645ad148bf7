"""GPU (-m gpu): in-run analysis records of the registered output queries (PvAmdSetQueryRecords; pv_query_records.hip).

Reference A, for every query: the whole-map record of the same cell -- the same listener run, compute_<kind>(), the map at the
query's cell (NaNs for a position off the map).  Reference B, for at least 8 reached queries per test that has them: the host
restatement (api.host_<kind>) of the definition applied to impulse_response(cx, cy) with the run's own onset.  Tolerance 0:
conftest.same_bits, NaN == NaN."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_lateral import preset_solver
from test_gpu_layer import cell_of
from test_gpu_lobes import FORMS
from test_gpu_room_metrics import L400, N400, SMALLROOM, history
from test_host_lobes import EDGES5

pytestmark = pytest.mark.gpu

NO_ONSET = 1e30
ECHOGRAM = (0.005, 16)
BOXES4 = ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5))
L_IN = (7.0, 0.0, 9.5)  # inside BOXES4


def kinds_of(pvlib):
    """kind bit -> (compute + map of the whole-map pass, host restatement of one response ir[T, 3] with its onset)"""
    return {
        pvlib.QREC_ROOM_METRICS: (lambda s: (s.compute_room_metrics(), s.room_metrics())[1],
                                  lambda s, ir, t0: pvlib.host_room_metrics(ir[:, 0], s.fs, t0)),
        pvlib.QREC_DECAY_TIMES: (lambda s: (s.compute_decay_times(), s.decay_times())[1],
                                 lambda s, ir, t0: pvlib.host_decay_times(ir[:, 0], s.fs, t0)),
        pvlib.QREC_LATERAL: (lambda s: (s.compute_lateral_fraction(), s.lateral_fraction())[1],
                             lambda s, ir, t0: pvlib.host_lateral_fraction(ir[:, 0], ir[:, 1], ir[:, 2], s.fs, t0)),
        pvlib.QREC_ECHOGRAM: (lambda s: (s.compute_echogram(), s.echogram())[1],
                              lambda s, ir, t0: pvlib.host_echogram(ir[:, 0], ir[:, 1], ir[:, 2], s.fs, t0, s.echogram_slots()[1],
                                                                    s.echogram_slots()[0])),
        pvlib.QREC_ECHO_CRITERION: (lambda s: (s.compute_echo_criterion(), s.echo_criterion())[1],
                                    lambda s, ir, t0: pvlib.host_echo_criterion(ir[:, 0], s.fs, t0)),
        pvlib.QREC_LOBES: (lambda s: (s.compute_lobes(), s.lobes())[1],
                           lambda s, ir, t0: pvlib.host_lobes(ir[:, 0], ir[:, 1], ir[:, 2], s.fs, t0, list(s.lobe_windows()[0]))),
    }


def bits(pvlib, kinds):
    return [k for k in kinds_of(pvlib) if kinds & k]


def cells_of(pvlib, size, positions):
    """the result cell PvAmdGetOutput reads for each position, None off the map"""
    return [pvlib.host_cells(size[0], size[1], 275, p[0], p[2])[1] for p in positions]


def records(s, pvlib, kinds):
    return dict((k, s.queried_records(k)) for k in bits(pvlib, kinds))


def check_against_maps(pvlib, s, size, positions, kinds, recs, ctx, host=8):
    """references A and B for the run the solver has just completed (no run in between: the whole-map passes read the same run)"""
    cells = cells_of(pvlib, size, positions)
    delay = s.results()[1]
    reached = [i for i, c in enumerate(cells) if c is not None and delay[c] < NO_ONSET]
    irs = dict((i, s.impulse_response(*cells[i])) for i in reached[:host])
    for k in bits(pvlib, kinds):
        whole, restate = kinds_of(pvlib)[k]
        m = whole(s)
        got = recs[k]
        assert got.shape == (len(positions), m.shape[-1]) and got.dtype == np.float32, (ctx, k)
        want = np.stack([m[c] if c is not None else np.full(m.shape[-1], np.nan, np.float32) for c in cells]) if cells else got
        bad = ~same_bits(got, want)
        assert not bad.any(), "%s kind %d: %d values differ from the whole-map records, first at %s" % (
            ctx, k, bad.sum(), np.argwhere(bad)[0])
        for i, c in enumerate(cells):  # NaN exactly where the position is off the map or its cell has no onset
            assert np.isnan(got[i]).all() == (i not in reached), (ctx, k, i)
        for i, ir in irs.items():
            assert same_bits(got[i], restate(s, ir, int(delay[cells[i]]))).all(), (ctx, k, i, cells[i])
    # the in-run records are still readable behind the whole-map passes, with the same bits
    for k, r in records(s, pvlib, kinds).items():
        assert same_bits(r, recs[k]).all(), (ctx, k)
    return reached


def run_with(s, pvlib, L, positions, kinds):
    s.set_output_queries(positions)
    s.set_query_records(kinds)
    assert s.query_record_kinds() == kinds
    s.run(L)
    return records(s, pvlib, kinds)


def pick(rng, mask, n):
    idx = np.argwhere(mask)
    return [tuple(int(v) for v in c) for c in idx[rng.choice(len(idx), min(len(idx), n), replace=False)]]


# ---- the 71^2 preset: one query set for tests 1, 2, 3 and 5
_G71 = {}


def g71_queries(pvlib, n=64):
    """n positions on g71_smallroom by class, from a plain run's delay map: (positions, classes {name: [query index]})"""
    if "q" not in _G71:
        g = golden("g71_smallroom")
        with preset_solver(pvlib, g) as s:
            s.run(g["listener"])
            delay = s.results()[1]
            rxi, wi = s.info.tileRows, s.info.tileCols
        reached = delay < NO_ONSET
        X, Y = np.meshgrid(np.arange(delay.shape[0]), np.arange(delay.shape[1]), indexing="ij")
        rng = np.random.default_rng(71)
        lcell = tuple(int(v) for v in np.unravel_index(np.argmin(delay), delay.shape))
        edge = reached & (((X % rxi == 0) & (X > 0)) | ((Y % wi == 0) & (Y > 0)))
        cells, classes = [], {}

        def add(name, cs):
            classes[name] = list(range(len(cells), len(cells) + len(cs)))
            cells.extend(cs)

        add("listener", [lcell])
        if edge.any():  # (a grid of more than one tile)
            add("tile edge", pick(rng, edge, 8))
        add("no onset", pick(rng, ~reached, 4))
        add("random", pick(rng, reached, 64 - len(cells) - 4))
        pos = [cell_of(*c) for c in cells]
        classes["off the map"] = [len(pos), len(pos) + 1]
        pos += [cell_of(70, 10), (3.0, 0.0, 30.0)]
        classes["duplicate"] = [len(pos), len(pos) + 1]
        pos += [pos[0], pos[classes["random"][0]]]
        assert len(pos) == 64 and all(classes.values()), classes
        onsets = np.array([delay[c] for c in cells if delay[c] < NO_ONSET])
        assert onsets.max() - onsets.min() > 100  # (the onsets differ widely across the wave)
        _G71["q"] = (pos, classes)
    pos, classes = _G71["q"]
    return pos[:n], classes


def g71_records(pvlib):
    """test 1's run: all six kinds, 64 queries, echogram (0.005, 16), lobe windows EDGES5; checked where it is made"""
    if "r" not in _G71:
        g = golden("g71_smallroom")
        pos, classes = g71_queries(pvlib)
        size = (float(g["size"]), float(g["size"]))
        with preset_solver(pvlib, g) as s:
            s.set_echogram(*ECHOGRAM)
            s.set_lobe_windows(EDGES5)
            recs = run_with(s, pvlib, g["listener"], pos, pvlib.QREC_ALL)
            assert (s.gx, s.T) == (70, 435)
            reached = check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, recs, "g71")
            assert set(range(64)) - set(classes["no onset"] + classes["off the map"]) == set(reached)
            for k, r in recs.items():
                for i, j in zip(classes["duplicate"], (0, classes["random"][0])):
                    assert same_bits(r[i], r[j]).all()
            s.set_lobe_windows(None)  # the default windows as well
            dflt = run_with(s, pvlib, g["listener"], pos, pvlib.QREC_LOBES)
            assert dflt[pvlib.QREC_LOBES].shape == (64, 16)
            check_against_maps(pvlib, s, size, pos, pvlib.QREC_LOBES, dflt, "g71, default windows")
        _G71["r"] = recs
    return _G71["r"]


def g71_solver(pvlib, **opts):
    s = preset_solver(pvlib, golden("g71_smallroom"), **opts)
    s.set_echogram(*ECHOGRAM)
    s.set_lobe_windows(EDGES5)
    return s


# 1. the preset grid: a full wave of queries, all six kinds at once
def test_preset_grid(pvlib):
    recs = g71_records(pvlib)
    assert [recs[k].shape[1] for k in sorted(recs)] == [10, 8, 11, 49, 10, 31]


# 2. every kind alone, and subsets: the same bits as in test 1, and an unselected kind's read is refused
def test_every_kind_alone_and_subsets(pvlib):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    with g71_solver(pvlib) as s:
        for kinds in list(want) + [pvlib.QREC_ROOM_METRICS | pvlib.QREC_LOBES, pvlib.QREC_ALL]:
            recs = run_with(s, pvlib, g["listener"], pos, kinds)
            assert sorted(recs) == bits(pvlib, kinds)
            for k in want:
                if kinds & k:
                    assert same_bits(recs[k], want[k]).all(), (kinds, k)
                else:
                    with pytest.raises(pvlib.PlaneverbError, match="^query records: .*not selected"):
                        s.queried_records(k)


# 3. query counts: none, one, 63 (one dead lane)
@pytest.mark.parametrize("n", [0, 1, 63])
def test_query_counts(pvlib, n):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib, n)
    with g71_solver(pvlib) as s:
        recs = run_with(s, pvlib, g["listener"], pos, pvlib.QREC_ALL)
        for k, r in recs.items():
            assert r.shape == (n, want[k].shape[1]) and same_bits(r, want[k][:n]).all(), (n, k)
        assert s.queried_outputs().shape == (n, 8)


# 4. a history window smaller than the grid
@pytest.mark.parametrize("where", ["corner", "offset"])
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        delay = s.results()[1]
        reached = delay < NO_ONSET
        onset = np.where(reached, delay, 0).astype(np.int64)
        rxi, wi, K = s.info.tileRows, s.info.tileCols, s.info.stepsPerLaunch
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]
        first_row, first_col = (X % rxi == 0), (Y % wi == 0)
        n0, n1 = 14, 115  # the default lobe windows at fs 1443
        N = s.T - onset
        classes = {"listener": reached & (X == lx) & (Y == ly),
                   "ends inside window 0": reached & (N <= n0) & (N > 1), "ends inside window 1": reached & (N > n0) & (N <= n1),
                   "N = 1": reached & (N == 1), "no onset": ~reached & (np.abs(X - lx) < 100) & (np.abs(Y - ly) < 100),
                   "outside the window": ~reached & ((np.abs(X - lx) > s.T + 40) | (np.abs(Y - ly) > s.T + 40))}
        if where == "corner":  # (no tile lies above or left of the listener's: the upstream neighbour lies outside the window)
            classes["upstream neighbour outside the window"] = reached & ((X == 0) | (Y == 0))
        else:
            # neighbour tiles recorded from a later launch: as tests/test_gpu_lobes.py finds them
            assert rxi >= K and wi >= K
            nz = history(s) != 0
            tnz_cell = np.where(nz.any(axis=0), nz.argmax(axis=0), 10 ** 6)
            tnz = np.full((-(-s.gx // rxi), -(-s.gy // wi)), 10 ** 6)
            ti, tj = X // rxi, Y // wi
            np.minimum.at(tnz, (ti, tj), tnz_cell)
            later_x = first_row & (ti < lx // rxi) & (ti > 0) & (tnz[np.maximum(ti - 1, 0), tj] >= tnz[ti, tj] + K)
            later_y = first_col & (tj < ly // wi) & (tj > 0) & (tnz[ti, np.maximum(tj - 1, 0)] >= tnz[ti, tj] + K)
            classes["upstream neighbour in another tile"] = reached & (first_row & (X > 0) | first_col & (Y > 0))
            classes["later neighbour tile"] = reached & (later_x | later_y)
        rng = np.random.default_rng(400)
        cells = []
        for name, m in classes.items():
            assert m.any(), (where, name)
            cells += pick(rng, m, 5)
        cells += pick(rng, reached, 61 - len(cells))
        pos = [cell_of(*c) for c in cells] + [cell_of(N400, 7), (-0.5, 0.0, 3.0), cell_of(*cells[0])]
        assert len(pos) == 64
        s.set_echogram(*ECHOGRAM)
        recs = run_with(s, pvlib, L400[where], pos, pvlib.QREC_ALL)
        assert same_bits(s.results()[1], delay).all()
        got = check_against_maps(pvlib, s, (size, size), pos, pvlib.QREC_ALL, recs, where, host=64)
        assert len(got) >= 40
        lobes = recs[pvlib.QREC_LOBES]
        n1s = [i for i, c in enumerate(cells) if classes["N = 1"][c]]
        assert n1s and all(lobes[i, 0] == 1 and (lobes[i, 6:] == 0).all() for i in n1s)


# 5. every stepping path gives the bits of test 1; a walled-in listener on the resident-window path
@pytest.mark.parametrize("form", list(FORMS))
def test_same_bits_on_every_path(pvlib, form):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    with g71_solver(pvlib, **FORMS[form]) as s:
        s.set_output_queries(pos)
        s.set_query_records(pvlib.QREC_ALL)
        s.run_async(g["listener"])
        s.sync()
        for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
            assert same_bits(r, want[k]).all(), (form, k)


def test_resident_window_path(pvlib):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    with g71_solver(pvlib, steps_per_launch=12, tile_rows=36, use_graph=2) as s:
        for b in BOXES4:
            s.add_geometry(b)
        s.run(L_IN)
        assert s.last_run_resident_window()
        delay = s.results()[1]
        reached = delay < NO_ONSET
        assert 4 <= reached.sum() < 200
        rng = np.random.default_rng(5)
        cells = pick(rng, reached, 40) + pick(rng, ~reached, 24)
        pos = [cell_of(*c) for c in cells]
        recs = run_with(s, pvlib, L_IN, pos, pvlib.QREC_ALL)
        assert s.last_run_resident_window()
        got = check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, recs, "window path")
        assert got == list(range(min(40, int(reached.sum()))))  # (inside the enclosure: records; outside: NaN)


# 6. non-square
def test_non_square_grid(pvlib):
    size = (open_size(95), open_size(70))
    L = cell_of(40, 22)
    with pvlib.Solver(size[0], size[1], 275) as s:
        assert (s.gx, s.gy, s.T) == (95, 70, 435)
        s.load_scene(SMALLROOM)
        s.run(L)
        delay = s.results()[1]
        reached = delay < NO_ONSET
        rng = np.random.default_rng(95)
        cells = pick(rng, reached, 56) + pick(rng, ~reached, 4) + [(94, 69), (94, 0), (0, 69)]
        pos = [cell_of(*c) for c in cells] + [cell_of(95, 10)]
        s.set_echogram(*ECHOGRAM)
        recs = run_with(s, pvlib, L, pos, pvlib.QREC_ALL)
        assert len(check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, recs, "95 x 70")) >= 56


# 7. runs in flight
def test_runs_in_flight(pvlib):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    L = [tuple(g["listener"]), L_IN]
    pos, _ = g71_queries(pvlib)
    sets = [pos, pos[40:10:-1]]
    plain = []
    for l, q in zip(L, sets):
        with g71_solver(pvlib) as s:
            plain.append(run_with(s, pvlib, l, q, pvlib.QREC_ALL))
    assert same_bits(plain[0][1], g71_records(pvlib)[1]).all()
    # a batch of two solvers with different listeners and different query sets
    solvers = [g71_solver(pvlib) for _ in L]
    try:
        for s, q in zip(solvers, sets):
            s.set_output_queries(q)
            s.set_query_records(pvlib.QREC_ALL)
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
                assert same_bits(r, w[k]).all(), ("batch", k)
    finally:
        for s in solvers:
            s.close()
    # two iterations in flight on two solvers
    with g71_solver(pvlib) as a, g71_solver(pvlib) as b:
        for s, q in ((a, sets[1]), (b, sets[0])):
            s.set_output_queries(q)
            s.set_query_records(pvlib.QREC_ALL)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.sync()
        a.sync()
        for s, w in ((a, plain[1]), (b, plain[0])):
            for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
                assert same_bits(r, w[k]).all(), ("pipelined", k)
    # a second run on the same solver that reaches fewer cells: a query only the first run reached gives NaN
    with g71_solver(pvlib) as s:
        first = run_with(s, pvlib, L[0], pos, pvlib.QREC_ALL)
        for b in BOXES4:
            s.add_geometry(b)
        s.run(L[1])
        second = records(s, pvlib, pvlib.QREC_ALL)
        reached = check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, second, "walled-in second run")
        lost = [i for i in range(64) if not np.isnan(first[1][i]).any() and i not in reached]
        assert len(lost) > 30
        for k, r in second.items():
            assert np.isnan(r[lost]).all(), k


# 8. settings and lifetime
def test_settings_and_lifetime(pvlib):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    K = pvlib.QREC_LOBES
    with g71_solver(pvlib) as s:
        recs = run_with(s, pvlib, g["listener"], pos, pvlib.QREC_ALL)
        s.compute_lobes()
        whole = s.lobes()
        assert same_bits(s.queried_records(K), want[K]).all() and same_bits(s.queried_records(K), recs[K]).all()
        assert same_bits(s.lobes(), whole).all()  # (reading the in-run records does not disturb the whole-map ones)
        # a lobe-window change: the record size follows, the old read is refused until the next run
        assert s.query_record_floats(K) == 31
        s.set_lobe_windows(None)
        assert s.query_record_floats(K) == 16
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            s.queried_records(K)
        s.run(g["listener"])
        assert s.queried_records(K).shape == (64, 16)
        s.compute_lobes()
        cells = cells_of(pvlib, (float(g["size"]),) * 2, pos)
        m = s.lobes()
        assert all(same_bits(r, m[c]).all() for r, c in zip(s.queried_records(K), cells) if c is not None)
        # the echogram slots cannot go while the kind is selected
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            s.set_echogram(0.0, 0)
        assert s.echogram_slots()[0] == 16 and s.query_record_floats(pvlib.QREC_ECHOGRAM) == 49
        # changing the queries: refused until the next run
        s.set_output_queries(pos[:5])
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            s.queried_records(pvlib.QREC_ROOM_METRICS)
        s.run(g["listener"])
        assert same_bits(s.queried_records(pvlib.QREC_ROOM_METRICS), want[pvlib.QREC_ROOM_METRICS][:5]).all()
        # no kinds: nothing is recorded, every read is refused
        s.set_query_records(0)
        assert s.query_record_kinds() == 0
        s.run(g["listener"])
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            s.queried_records(pvlib.QREC_ROOM_METRICS)
        s.set_echogram(0.0, 0)  # (allowed again)
        assert same_bits(s.queried_outputs(), s.queried_outputs()).all()


# 9. refusals: a "query records: ..." message each
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*unknown"):
            s.set_query_records(64)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*echogram"):
            s.set_query_records(pvlib.QREC_ECHOGRAM)
        assert s.query_record_kinds() == 0
        s.set_output_queries([E])
        s.set_query_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            s.queried_records(pvlib.QREC_ROOM_METRICS)  # (no run yet)
        s.run(L)
        assert np.isfinite(s.queried_records(pvlib.QREC_ROOM_METRICS)).all()
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*history"):
            s.set_query_records(pvlib.QREC_ROOM_METRICS)
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*onset map"):
            s.set_query_records(pvlib.QREC_ROOM_METRICS)


# 10. the command line: the same bytes with and without --in-run-records (the two measured durations aside: no two runs share them)
def test_cli(pvlib):
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4", "--emitter", "5,0,6", "--emitter", "12,0,9",
           "--emitter", "40,0,3", "--room-metrics", "--decay-times", "--lateral-fraction", "--echogram", "0.005,16",
           "--echo-criterion", "--lobes", "0.005,0.02,0.08"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(*more):
        out = subprocess.run(cmd + list(more), capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout
        assert len(re.findall(r'"(?:fdtd_ms|analysis_ms)": [0-9.e+-]+,', out)) == 2
        return re.sub(r'("(?:fdtd_ms|analysis_ms)"): [0-9.e+-]+,', r"\1: 0,", out)

    a, b = run(), run("--in-run-records")
    assert a == b
    rec = json.loads(b)["emitters"]
    assert len(rec) == 3 and all(k in rec[0] for k in ("roomMetrics", "decayTimes", "lateralFraction", "echogram", "echoCriterion",
                                                        "lobes"))
    assert np.isfinite(rec[0]["roomMetrics"]["c50"]) and np.isnan(rec[2]["roomMetrics"]["c50"])
