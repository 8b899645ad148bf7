"""Reach-bounded runs (PVA_OPT_REACH_BOUND, csrc/pv_solver.cpp Solver::setReachArgs): a run's launches advance only the tiles
the pulse can have reached, the rest of both buffer sets is kept at zero.  Every case compares with full sweeps
(reach_bound=0) bit for bit: final pr / vx / vy, result and onset maps, queried outputs."""
import os

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE = os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv")
DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
LISTENERS = [(5, 4), (8, 8), (12, 6), (15, 15), (20, 5), (5, 20), (20, 20), (12.5, 18)]  # bench.py's


def size(n):
    return float((n + 0.5) * DX)


def cell(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def run(s, listener, emitters):
    s.set_output_queries(emitters)
    s.run(listener)
    return s.queried_outputs()


def check_same(a, b, ctx, full_maps=False):
    """a, b: solvers that just ran the same listener"""
    for name, x, y in zip(("pr", "vx", "vy"), a.fields(), b.fields()):
        bad = ~same_bits(x, y)
        assert not bad.any(), "%s: %s differs in %d cells, first %s" % (ctx, name, bad.sum(), np.argwhere(bad)[:3].tolist())
    if full_maps:
        (ra, da), (rb, db) = a.results(), b.results()
        assert same_bits(da, db).all(), "%s: onset map" % ctx
        for m in range(8):
            assert same_bits(ra[..., m], rb[..., m]).all(), "%s: result member %d" % (ctx, m)
    else:  # the history window's block (the cells the analysis looked at); the far cells are the same code either way
        wa, wb = a.info.histRows, a.info.histPitch
        assert (wa, wb) == (b.info.histRows, b.info.histPitch)
        x, _, z = a._last_listener
        cx, cy = int(np.float32(x) / DX), int(np.float32(z) / DX)
        r0, c0 = max(0, cx - 450), max(0, cy - 450)
        nr, nc = min(a.gx - r0, 900), min(a.gy - c0, 900)
        (ra, da), (rb, db) = a.results_block(r0, c0, nr, nc), b.results_block(r0, c0, nr, nc)
        assert same_bits(da, db).all(), "%s: onsets of the window block" % ctx
        assert same_bits(ra, rb).all(), "%s: records of the window block" % ctx


def pair_run(a, b, listener, emitters, ctx, full_maps=False):
    oa, ob = run(a, listener, emitters), run(b, listener, emitters)
    assert same_bits(oa, ob).all(), "%s: queried outputs %s vs %s" % (ctx, oa, ob)
    a._last_listener = b._last_listener = listener
    check_same(a, b, ctx, full_maps)


def test_hugeroom_4096_bench_listeners(pvlib):
    """config 4 of the bench: HugeRoom.pv at 4096^2, every bench listener in turn (each run clears the previous one's rectangle)"""
    with pvlib.Solver(size(4096), size(4096), 275) as a, pvlib.Solver(size(4096), size(4096), 275, reach_bound=0) as b:
        a.load_scene(HUGE)
        b.load_scene(HUGE)
        for i, (x, z) in enumerate(LISTENERS):
            pair_run(a, b, (x, 0.0, z), [(x, 0.0, z + 2.0), (5.0, 0.0, 6.0)], "listener %d" % i, full_maps=(i == 0))


def test_open_field_4096_positions_and_far_listener(pvlib):
    """open 4096^2 grid: listener at the centre, a corner, an edge, on a tile boundary (36 x 40-cell tiles), then A, far B, A"""
    n = 4096
    centre, corner, edge, boundary = (n // 2, n // 2), (0, 0), (0, n // 3), (36 * 40, 40 * 37)
    with pvlib.Solver(size(n), size(n), 275) as a, pvlib.Solver(size(n), size(n), 275, reach_bound=0) as b:
        assert a.info.stepsPerLaunch == 12 and a.info.tileRows == 36
        for k, (cx, cy) in enumerate([centre, corner, edge, boundary, (n, n), centre, (n - 5, 7), centre]):
            em = [cell(min(cx + 16, n - 1), cy), cell(cx, min(cy + 16, n - 1))]
            pair_run(a, b, cell(min(cx, n - 1), min(cy, n - 1)), em, "run %d at %s" % (k, (cx, cy)), full_maps=(k == 1))


def test_2048_without_graph(pvlib):
    """2048^2 (the (10, 36) tile): the reach-bounded plain launches (use_graph=2) against full sweeps and against the graph"""
    with pvlib.Solver(size(2048), size(2048), 275, use_graph=2) as a, \
            pvlib.Solver(size(2048), size(2048), 275, use_graph=2, reach_bound=0) as b, \
            pvlib.Solver(size(2048), size(2048), 275) as g:
        assert a.info.stepsPerLaunch == 10 and a.info.tileRows == 36
        for s in (a, b, g):
            s.load_scene(HUGE)
        for i, (x, z) in enumerate(LISTENERS[:3]):
            lst, em = (x, 0.0, z), [(x, 0.0, z + 2.0), (5.0, 0.0, 6.0)]
            pair_run(a, b, lst, em, "listener %d, full sweeps" % i, full_maps=(i == 0))
            og = run(g, lst, em)
            assert same_bits(og, a.queried_outputs()).all(), "listener %d: graph" % i
            g._last_listener = lst
            check_same(a, g, "listener %d, graph" % i)


def test_grid_smaller_than_reach(pvlib):
    """a 600^2 grid: the reach covers the whole grid after a few launches (the window saturates)"""
    opts = dict(use_graph=2, resident_kernel=2)
    with pvlib.Solver(size(600), size(600), 275, **opts) as a, \
            pvlib.Solver(size(600), size(600), 275, reach_bound=0, **opts) as b:
        for k, (cx, cy) in enumerate([(300, 300), (2, 590), (300, 300)]):
            pair_run(a, b, cell(cx, cy), [cell(cx + 3, cy), cell(10, 10)], "run %d" % k, full_maps=True)


def test_set_fields_and_raw_steps_between_runs(pvlib):
    """run, then set_fields(random) + run_steps, then a run: equals a fresh solver's run"""
    n = 4096
    rng = np.random.default_rng(7)
    with pvlib.Solver(size(n), size(n), 275) as a:
        a.load_scene(HUGE)
        run(a, (8.0, 0.0, 8.0), [(8.0, 0.0, 10.0)])
        a.set_fields(*[(rng.random((a.gx + 1, a.gy + 1), np.float32) - np.float32(0.5)) for _ in range(3)])
        a.run_steps(24)
        with pvlib.Solver(size(n), size(n), 275) as f:
            f.load_scene(HUGE)
            pair_run(a, f, (15.0, 0.0, 15.0), [(15.0, 0.0, 17.0), (5.0, 0.0, 6.0)], "after raw stepping")


def test_geometry_change_between_runs(pvlib):
    n = 4096
    with pvlib.Solver(size(n), size(n), 275) as a, pvlib.Solver(size(n), size(n), 275, reach_bound=0) as b:
        lst, em = cell(1000, 1000), [cell(1010, 1000), cell(1000, 1200)]
        pair_run(a, b, lst, em, "empty grid")
        box = (cell(1040, 980)[0], cell(1040, 980)[2], 2.0, 3.0, 0.3)  # (x, z, width, depth, absorption)
        for s in (a, b):
            s.add_geometry(box)
        pair_run(a, b, lst, em, "with a box")


def test_two_solvers_in_flight(pvlib):
    n = 4096
    with pvlib.Solver(size(n), size(n), 275) as a1, pvlib.Solver(size(n), size(n), 275) as a2, \
            pvlib.Solver(size(n), size(n), 275, reach_bound=0) as b:
        for s in (a1, a2, b):
            s.load_scene(HUGE)
        for step in range(3):
            l1, l2 = LISTENERS[2 * step], LISTENERS[2 * step + 1]
            e1, e2 = [(l1[0], 0.0, l1[1] + 2.0)], [(l2[0], 0.0, l2[1] + 2.0)]
            a1.set_output_queries(e1)
            a2.set_output_queries(e2)
            a1.run_async((l1[0], 0.0, l1[1]))
            a2.run_async((l2[0], 0.0, l2[1]))
            a1.sync()
            a2.sync()
            for s, (x, z), e in ((a1, l1, e1), (a2, l2, e2)):
                ob = run(b, (x, 0.0, z), e)
                assert same_bits(s.queried_outputs(), ob).all(), "step %d" % step
                s._last_listener = b._last_listener = (x, 0.0, z)
                check_same(s, b, "step %d, listener %s" % (step, (x, z)))


def test_short_bake(pvlib):
    """a baked probe table (Solver runs through the bake's own schedule) equals the one baked with full sweeps"""
    n = 3100  # (> 4096 tiles: the plain launches, no graph)
    lattice = (5, 10.0, 10.0, 10.0, 10.0, 2, 2)
    with pvlib.Solver(size(n), size(n), 275, num_steps=200) as a, \
            pvlib.Solver(size(n), size(n), 275, num_steps=200, reach_bound=0) as b:
        ba, bb = pvlib.Bake(a, *lattice), pvlib.Bake(b, *lattice)
        ba.run([a])
        bb.run([b])
        for k in range(4):
            (sa, ra), (sb, rb) = ba.probe(k), bb.probe(k)
            assert (sa == sb).all(), (k, sa, sb)
            assert same_bits(ra, rb).all(), "probe %d" % k
        ba.close()
        bb.close()
