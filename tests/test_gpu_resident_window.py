"""Resident-window runs (PVA_OPT_RESIDENT_WINDOW, csrc/pv_solver.cpp Solver::windowFor / enqueueWindowRun): a run whose listener
is walled in steps only the tile window around its air component, in one launch of the resident kernel.  Every case compares
with the reach-bounded launches (resident_window=0) bit for bit -- final pr / vx / vy of the whole grid, result and onset maps,
queried outputs -- and asserts which path the runs took: a case that silently fell back would prove nothing.  The comparisons with
the oracle (grids of 226^2 ... 280^2 that reach the path through an explicit (12, 36) tile) are in test_gpu_resident_window_small.py."""
import os

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE = os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g71_hugeroom_cfg4.npz")
DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
LISTENERS = [(5, 4), (8, 8), (12, 6), (15, 15), (20, 5), (5, 20), (20, 20), (12.5, 18)]  # bench.py's
N = 4096


def size(n):
    return float((n + 0.5) * DX)


def cell(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def run(s, listener, emitters):
    s.set_output_queries(emitters)
    s.run(listener)
    s._last_listener = listener
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
        x, _, z = a._last_listener
        cx, cy = int(np.float32(x) / DX), int(np.float32(z) / DX)
        r0, c0 = max(0, cx - 450), max(0, cy - 450)
        nr, nc = min(a.gx - r0, 900), min(a.gy - c0, 900)
        (ra, da), (rb, db) = a.results_block(r0, c0, nr, nc), b.results_block(r0, c0, nr, nc)
        assert same_bits(da, db).all(), "%s: onsets of the window block" % ctx
        assert same_bits(ra, rb).all(), "%s: records of the window block" % ctx


def pair_run(a, b, listener, emitters, ctx, window, full_maps=False):
    """a: the solver under test (window = the path its run must take), b: the comparison solver (never the window path)"""
    oa, ob = run(a, listener, emitters), run(b, listener, emitters)
    assert a.last_run_resident_window() == window, "%s: window path %s" % (ctx, "not taken" if window else "taken")
    assert not b.last_run_resident_window(), ctx
    assert same_bits(oa, ob).all(), "%s: queried outputs %s vs %s" % (ctx, oa, ob)
    check_same(a, b, ctx, full_maps)


def room(s, cx, cy, h=60, w=70, t=3):
    """a closed room of h x w air cells behind t-cell walls whose first air cell is (cx, cy); returns the ids of its four walls"""
    d = float(DX)

    def box(r0, c0, r1, c1):  # cells [r0, r1) x [c0, c1): (centre x, centre z, width, depth, absorption)
        return s.add_geometry(((r0 + r1) * 0.5 * d, (c0 + c1) * 0.5 * d, (r1 - r0) * d - 0.2 * d, (c1 - c0) * d - 0.2 * d, 0.4))

    # (every wall runs through both of its corners: whatever the rasteriser does with a box's last row / column, the walls overlap)
    return [box(cx - t, cy - t, cx, cy + w + t), box(cx + h, cy - t, cx + h + t, cy + w + t),
            box(cx - t, cy - t, cx + h + t, cy), box(cx - t, cy + w, cx + h + t, cy + w + t)]


def test_hugeroom_4096_bench_listeners_and_golden(pvlib):
    """config 4 of the bench: every bench listener in turn on one solver, every run on the window path; against the reach-bounded
    launches, against full sweeps, and the records against the reference's 71^2 run of the same room (what bench.py verifies)"""
    g = np.load(GOLDEN)
    assert [tuple(l) for l in g["listeners"][:, [0, 2]].tolist()] == [tuple(map(float, l)) for l in LISTENERS]
    with pvlib.Solver(size(N), size(N), 275) as a, pvlib.Solver(size(N), size(N), 275, resident_window=0) as b, \
            pvlib.Solver(size(N), size(N), 275, reach_bound=0) as f:
        for s in (a, b, f):
            s.load_scene(HUGE)
        for i, (x, z) in enumerate(LISTENERS):
            lst, em = (float(x), 0.0, float(z)), [(float(x), 0.0, z + 2.0), (5.0, 0.0, 6.0)]
            pair_run(a, b, lst, em, "listener %d" % i, True, full_maps=(i == 0))
            assert a.timings().stepLaunches == 37
            assert same_bits(a.queried_outputs(), g["emitter_out"][i]).all(), "listener %d: golden records" % i
            if i in (0, 5):
                of = run(f, lst, em)
                assert not f.last_run_resident_window()
                assert same_bits(a.queried_outputs(), of).all(), "listener %d: full sweeps" % i
                check_same(a, f, "listener %d, full sweeps" % i, full_maps=(i == 0))


def test_open_field_and_listener_in_a_wall(pvlib):
    with pvlib.Solver(size(N), size(N), 275) as a, pvlib.Solver(size(N), size(N), 275, resident_window=0) as b:
        pair_run(a, b, cell(2000, 2100), [cell(2016, 2100), cell(2000, 2116)], "open field", False)
        for s in (a, b):
            s.load_scene(HUGE)
        wall = (12.41, 0.0, 12.29)  # the centre of HugeRoom.pv's inner box
        pair_run(a, b, wall, [(12.0, 0.0, 6.0), (5.0, 0.0, 6.0)], "listener inside a wall", False)
        pair_run(a, b, (8.0, 0.0, 8.0), [(8.0, 0.0, 10.0)], "back in the room", True)


def test_mixed_sequences_on_one_solver(pvlib):
    """window run -> open-field run -> window run; set_fields + run_steps between two window runs"""
    rng = np.random.default_rng(5)
    with pvlib.Solver(size(N), size(N), 275) as a, pvlib.Solver(size(N), size(N), 275, resident_window=0) as b:
        for s in (a, b):
            s.load_scene(HUGE)
        em = [(12.0, 0.0, 6.0), (5.0, 0.0, 6.0)]
        pair_run(a, b, (5.0, 0.0, 4.0), em, "window run 1", True)
        pair_run(a, b, cell(1500, 1600), [cell(1510, 1600)], "open-field run", False)
        pair_run(a, b, (20.0, 0.0, 20.0), em, "window run 2", True)
        fields = [(rng.random((a.gx + 1, a.gy + 1), np.float32) - np.float32(0.5)) for _ in range(3)]
        for s in (a, b):
            s.set_fields(*fields)
            s.run_steps(24)
        pair_run(a, b, (15.0, 0.0, 15.0), em, "window run after raw stepping", True, full_maps=True)


def test_geometry_changes(pvlib):
    """a box added inside the room (the component changes: new fill), then a wall removed: the room opens, path not taken"""
    with pvlib.Solver(size(N), size(N), 275) as a, pvlib.Solver(size(N), size(N), 275, resident_window=0) as b:
        walls = [room(s, 1000, 1100) for s in (a, b)]
        lst, em = cell(1010, 1110), [cell(1030, 1120), cell(1050, 1160)]
        pair_run(a, b, lst, em, "closed room", True)
        d = float(DX)
        for s in (a, b):
            s.add_geometry((1035.0 * d, 1130.0 * d, 6.0 * d, 9.0 * d, 0.2))
        pair_run(a, b, lst, em, "a box inside the room", True)
        for s, w in zip((a, b), walls):
            s.remove_geometry(w[3])
        pair_run(a, b, lst, em, "the room opened", False)
        pair_run(a, b, lst, em, "the room opened, again (cached answer)", False)


def test_window_at_the_origin_and_across_three_tile_rows(pvlib):
    with pvlib.Solver(size(N), size(N), 275) as a, pvlib.Solver(size(N), size(N), 275, resident_window=0) as b:
        for s in (a, b):
            d = float(DX)  # air cells from row / column 0, walls on the two far sides: the window's ring is clipped at the grid's edge
            s.add_geometry((31.5 * d, 25.0 * d, 2.8 * d, 58.0 * d, 0.4))  # rows 30 .. 32 from beyond column 0 to column 53
            s.add_geometry((16.0 * d, 51.5 * d, 38.0 * d, 2.8 * d, 0.4))  # columns 50 .. 52 from beyond row 0 through the other wall
            room(s, 3590, 2010, h=80, w=60)  # rows 3589 .. 3670: tile rows 99, 100, 101
        pair_run(a, b, cell(4, 6), [cell(20, 30), cell(10, 45)], "room in the corner", True)
        pair_run(a, b, cell(3600, 2040), [cell(3660, 2015), cell(3595, 2065)], "room across three tile rows", True, full_maps=True)


def test_two_solvers_in_flight(pvlib):
    """the bench's shape: two window runs side by side, both holding a reservation of the device's resident budget"""
    with pvlib.Solver(size(N), size(N), 275) as a1, pvlib.Solver(size(N), size(N), 275) as a2, \
            pvlib.Solver(size(N), size(N), 275, resident_window=0) as b:
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
            assert a1.last_run_resident_window() and a2.last_run_resident_window(), "step %d: both on the window path" % step
            for s, (x, z), e in ((a1, l1, e1), (a2, l2, e2)):
                ob = run(b, (x, 0.0, z), e)
                assert same_bits(s.queried_outputs(), ob).all(), "step %d" % step
                s._last_listener = (x, 0.0, z)
                check_same(s, b, "step %d, listener %s" % (step, (x, z)))


def test_short_bake(pvlib):
    """a baked probe table over probes inside the room equals the one baked without the window path"""
    lattice = (5, 5.0, 5.0, 12.0, 12.0, 2, 2)
    with pvlib.Solver(size(N), size(N), 275, num_steps=200) as a, \
            pvlib.Solver(size(N), size(N), 275, num_steps=200, resident_window=0) as b:
        for s in (a, b):
            s.load_scene(HUGE)
        ba, bb = pvlib.Bake(a, *lattice), pvlib.Bake(b, *lattice)
        ba.run([a])
        bb.run([b])
        assert a.last_run_resident_window() and not b.last_run_resident_window()
        for k in range(4):
            (sa, ra), (sb, rb) = ba.probe(k), bb.probe(k)
            assert (sa == sb).all(), (k, sa, sb)
            assert same_bits(ra, rb).all(), "probe %d" % k
        ba.close()
        bb.close()
