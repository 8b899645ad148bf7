"""GPU (-m gpu): record queries -- more than one wave of in-run analysis records per kind (PvAmdSetRecordQueries; the second grid
dimension of pv_query_records_kernel).

The references are those of test_gpu_query_records.py, whose helpers are used: A, for every query, the whole-map record of the
same cell on the same run (NaNs for a position off the map); B, for at least 8 reached queries per test, the host restatement
applied to the cell's impulse response.  Tolerance 0 (conftest.same_bits, NaN == NaN)."""
import numpy as np
import pytest

from conftest import golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of
from test_gpu_query_records import (ECHOGRAM, NO_ONSET, check_against_maps, g71_queries, g71_solver, pick, records)
from test_gpu_room_metrics import L400, N400, SMALLROOM

pytestmark = pytest.mark.gpu


def run_records(s, pvlib, L, positions, kinds):
    s.set_record_queries(positions)
    s.set_query_records(kinds)
    s.run(L)
    return records(s, pvlib, kinds)


def g71_positions(pvlib, n):
    """n > 64 positions on g71_smallroom: the 64 of test_gpu_query_records.py (listener cell, tile edges, 4 cells without an
    onset, 2 off the map, duplicates), query 0 again at index 64, 2 more off the map and 2 more without an onset behind it, the
    rest reached cells drawn at random (with repeats once the map runs out: 1024 < 4900 cells, so there are none)"""
    base, classes = g71_queries(pvlib)
    g = golden("g71_smallroom")
    with g71_solver(pvlib) as s:
        s.run(g["listener"])
        delay = s.results()[1]
    reached = delay < NO_ONSET
    rng = np.random.default_rng(n)
    pos = list(base) + [base[0]]
    nan = set(classes["no onset"] + classes["off the map"])
    if n >= len(pos) + 4:
        nan |= set(range(len(pos), len(pos) + 4))
        pos += [cell_of(70, 33), (-2.0, 0.0, 5.0)] + [cell_of(*c) for c in pick(rng, ~reached, 2)]
    pos += [cell_of(*c) for c in pick(rng, reached, n - len(pos))]
    assert len(pos) == n
    return pos, nan


# 1. 65: a second group with one live lane; 128: two full groups; 150: a partial last group; 1024: the cap, 16 groups
@pytest.mark.parametrize("n", [65, 128, 150, 1024])
def test_more_than_one_wave(pvlib, n):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    pos, nan = g71_positions(pvlib, n)
    with g71_solver(pvlib) as s:
        assert (s.gx, s.T) == (70, 435)
        recs = run_records(s, pvlib, g["listener"], pos, pvlib.QREC_ALL)
        assert [recs[k].shape for k in sorted(recs)] == [(n, f) for f in (10, 8, 11, 49, 10, 31)]
        reached = check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, recs, "n = %d" % n)
        assert set(range(n)) - nan == set(reached) and len(nan) >= (10 if n >= 69 else 6)
        for k, r in recs.items():
            assert same_bits(r[64], r[0]).all() and not np.isnan(r[0]).any(), k  # (the same cell in two groups)
        # the first 64 records are those of the same 64 positions as output queries, on a second run
        s.set_record_queries([])
        s.set_output_queries(pos[:64])
        s.run(g["listener"])
        for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
            assert r.shape[0] == 64 and same_bits(r, recs[k][:64]).all(), (n, k)


# 2. a history window smaller than the grid, two groups
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
        rxi, wi = s.info.tileRows, s.info.tileCols
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]
        far = np.maximum(np.abs(X - lx), np.abs(Y - ly))
        classes = {"inside, no onset": ~reached & (far < 100),
                   "tile-rounded margin": ~reached & (far > s.T) & (far <= s.T + max(rxi, wi)),
                   "outside the window": ~reached & (far > s.T + 40)}
        rng = np.random.default_rng(401)
        cells = []
        for name, m in classes.items():
            assert m.any(), (where, name)
            cells += pick(rng, m, 8)
        cells += pick(rng, reached, 97 - len(cells))
        pos = [cell_of(*c) for c in cells] + [cell_of(N400, 7), (-0.5, 0.0, 3.0)]
        pos.insert(70, pos[30])  # (a reached cell in both groups)
        assert len(pos) == 100
        s.set_echogram(*ECHOGRAM)
        recs = run_records(s, pvlib, L400[where], pos, pvlib.QREC_ALL)
        assert same_bits(s.results()[1], delay).all()
        got = check_against_maps(pvlib, s, (size, size), pos, pvlib.QREC_ALL, recs, where, host=12)
        assert len(got) == 100 - 2 - sum(1 for c in cells if not reached[c]) >= 70 and 70 in got and 30 in got


# 3. non-square, 70 queries
def test_non_square_grid(pvlib):
    size = (open_size(95), open_size(70))
    L = cell_of(40, 22)
    with pvlib.Solver(size[0], size[1], 275) as s:
        assert (s.gx, s.gy, s.T) == (95, 70, 435)
        s.load_scene(SMALLROOM)
        s.run(L)
        reached = s.results()[1] < NO_ONSET
        rng = np.random.default_rng(96)
        cells = pick(rng, reached, 62) + pick(rng, ~reached, 4) + [(94, 69), (94, 0), (0, 69)]
        pos = [cell_of(*c) for c in cells] + [cell_of(95, 10)]
        assert len(pos) == 70
        s.set_echogram(*ECHOGRAM)
        recs = run_records(s, pvlib, L, pos, pvlib.QREC_ALL)
        assert len(check_against_maps(pvlib, s, size, pos, pvlib.QREC_ALL, recs, "95 x 70")) >= 62


# 4. both tables at once; back to the output queries; the stamp
def test_coexistence_and_stamp(pvlib):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    outq, _ = g71_queries(pvlib)
    recq, _ = g71_positions(pvlib, 150)
    recq = recq[::-1]
    with g71_solver(pvlib) as s:
        s.set_output_queries(outq)
        s.set_query_records(pvlib.QREC_ALL)
        s.run(g["listener"])
        old_out = s.queried_outputs()
        old = records(s, pvlib, pvlib.QREC_ALL)
        assert old[1].shape == (64, 10)
        # both tables: the outputs are the output queries', the records the record queries'
        s.set_record_queries(recq)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: no completed run"):
            s.queried_records(pvlib.QREC_ROOM_METRICS)  # (the table changed)
        s.run(g["listener"])
        assert s.queried_outputs().shape == (64, 8) and same_bits(s.queried_outputs(), old_out).all()
        recs = records(s, pvlib, pvlib.QREC_ALL)
        check_against_maps(pvlib, s, size, recq, pvlib.QREC_ALL, recs, "both tables")
        # changing the OUTPUT queries leaves the record queries' records readable; changing the record table does not
        s.set_output_queries(outq[:10])
        assert same_bits(s.queried_records(pvlib.QREC_LOBES), recs[pvlib.QREC_LOBES]).all()
        s.set_output_queries(outq)
        s.set_record_queries(recq[:70])
        with pytest.raises(pvlib.PlaneverbError, match="^query records: no completed run"):
            s.queried_records(pvlib.QREC_LOBES)
        s.run(g["listener"])
        for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
            assert r.shape[0] == 70 and same_bits(r, recs[k][:70]).all(), k
        # no record queries: the behaviour of before, bit for bit
        s.set_record_queries([])
        with pytest.raises(pvlib.PlaneverbError, match="^query records: no completed run"):
            s.queried_records(pvlib.QREC_ROOM_METRICS)
        s.run(g["listener"])
        assert same_bits(s.queried_outputs(), old_out).all()
        for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
            assert same_bits(r, old[k]).all(), k
        # the record table registered first, the kinds afterwards: the block is sized for the table
        s.set_query_records(0)
        s.set_record_queries(recq)
        s.set_query_records(pvlib.QREC_ALL)
        s.run(g["listener"])
        for k, r in records(s, pvlib, pvlib.QREC_ALL).items():
            assert same_bits(r, recs[k]).all(), k


# 5. refusals, a "query records: ..." message each
def test_refusals(pvlib):
    E = (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_record_queries([E] * 3)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*1024"):
            s.set_record_queries([E] * (pvlib.RECORD_QUERIES_MAX + 1))
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            pvlib._check(pvlib.lib().PvAmdSetRecordQueries(s._h, None, 2))
        with pytest.raises(pvlib.PlaneverbError, match="^query records: "):
            pvlib._check(pvlib.lib().PvAmdSetRecordQueries(s._h, None, -1))
        # (nothing changed: three record queries)
        s.set_query_records(pvlib.QREC_ROOM_METRICS)
        s.run((5.0, 0.0, 4.0))
        r = s.queried_records(pvlib.QREC_ROOM_METRICS)
        assert r.shape == (3, 10) and np.isfinite(r).all() and same_bits(r[0], r[2]).all()
    with pvlib.Solver(25.0, 25.0, 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*slab"):
            s.set_record_queries([E])
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*history"):
            s.set_record_queries([E])
