"""GPU (-m gpu): the two things a resident-window run decides per run besides its window (csrc/pv_solver.cpp enqueueRun):

  * the hand-off between epochs: through ONE XCD's L2 when the window's 3 x tile rows x tile columns blocks are at most 32 and the
    solver's XCD has room (Solver.last_run_one_xcd()), else the placement-independent one;
  * the clear in front of the launch: none when the window is the previous run's (csrc/pv_core.cpp planClear, whose table
    tests/test_host_window_clear.py checks without a device).

Scenes, references and comparisons are those of tests/test_gpu_resident_window_small.py: 226^2 ... 280^2 grids on the explicit
(12, 36) tile, every bit of the fields, the recorded planes HIST_TS, all maps and the carried records against oracle.OracleGrid, or
against a resident_window=0 solver where the oracle has no such run (other step counts).  Every run asserts both decisions' visible
half: which path it took and which hand-off.
"""
import numpy as np
import pytest

from test_gpu_resident_window_small import (G226, G280, IN_A, IN_A2, IN_B, IN_C, IN_D, IN_D2, OPTS, ROOM_C, ROOM_D, TWO_ROOMS, cell, check,
                                            check_pair, open_listeners, oracle_chain, pair_seq, room, solver, two_rooms)

pytestmark = pytest.mark.gpu

assert OPTS == dict(steps_per_launch=12, tile_rows=36, use_graph=2)
BOXES = np.array(TWO_ROOMS, np.float32)


def run(s, L, ctx, window=True, one_xcd=True):
    s.run(L)
    took(s, ctx, window, one_xcd)


def took(s, ctx, window=True, one_xcd=True):
    assert s.last_run_resident_window() == window, "%s: window path %s" % (ctx, "not taken" if window else "taken")
    assert s.last_run_one_xcd() == one_xcd, "%s: one-XCD hand-off %s" % (ctx, "not taken" if one_xcd else "taken")


def test_two_rooms(pvlib, oracle):
    """rooms A (3 x 2 tiles) and B (2 x 3 tiles): 18 blocks each, one XCD"""
    chain = oracle_chain(oracle, "two_rooms", G280, BOXES, [(None, IN_A), (None, IN_B), (None, IN_A2)])
    with two_rooms(pvlib) as s:
        assert s.last_run_one_xcd() is False and s.last_run_resident_window() is False  # (a fresh solver: no run yet)
        for k, L in enumerate((IN_A, IN_B, IN_A2)):
            run(s, L, "run %d" % k)
            check(s, chain[k], "two rooms, one XCD, run %d" % k)


def test_open_grid_is_too_large_for_one_xcd(pvlib, oracle):
    """7 x 6 tiles = 126 blocks: the window path with the placement-independent hand-off"""
    L = cell(*open_listeners(G226)["centre"])
    chain = oracle_chain(oracle, ("open", "226", "centre"), G226, None, [(None, L), (None, L)])
    with solver(pvlib, G226) as s:
        run(s, L, "open 226^2", one_xcd=False)
        check(s, chain[0], "open 226^2")


@pytest.mark.parametrize("steps", [1, 11, 12, 13])
def test_short_runs(pvlib, steps):
    """one epoch, a short last epoch, and the claim counter behind 3 and 6 flag words: room C is one tile (3 blocks), room D two
    tiles side by side (6 blocks in two history tiles); against the reach-bounded launches"""
    def scene(**opts):
        s = two_rooms(pvlib, num_steps=steps, **opts)
        for b in room(*ROOM_C, 0.6) + room(*ROOM_D, 0.3):
            s.add_geometry(b)
        return s
    with scene() as a, scene(resident_window=0) as b:
        for ctx, L in (("room C", IN_C), ("room D", IN_D), ("room D, no clear", IN_D2), ("room C again", cell(223, 69))):
            ctx = "T = %d, %s" % (steps, ctx)
            pair_seq(a, b, [(ctx, L, True)], planes=sorted({0, steps // 2, steps - 1}))
            took(a, ctx)
            took(b, ctx + " (comparison)", window=False, one_xcd=False)


def test_two_solvers_in_flight(pvlib, oracle):
    """two solvers of one device run at once, each in its own room on its own XCD"""
    twice_a = oracle_chain(oracle, "two_rooms_a_twice", G280, BOXES, [(None, IN_A), (None, IN_A)])
    twice_b = oracle_chain(oracle, "two_rooms_b_twice", G280, BOXES, [(None, IN_B), (None, IN_B)])
    with two_rooms(pvlib) as a, two_rooms(pvlib) as b:
        for rep in range(2):  # (the second pair: neither solver clears)
            a.run_async(IN_A)
            b.run_async(IN_B)
            a.sync()
            b.sync()
            took(a, "solver a, pair %d" % rep)
            took(b, "solver b, pair %d" % rep)
            assert pvlib.lib().PvAmdLastRunOneXcd(a._h) == 1 and pvlib.lib().PvAmdLastRunOneXcd(b._h) == 1
            check(a, twice_a[rep], "solver a in room A, pair %d" % rep)
            check(b, twice_b[rep], "solver b in room B, pair %d" % rep)


@pytest.mark.parametrize("env", [{"PLANEVERB_AMD_RESIDENT_XCD": "0"}, {"PLANEVERB_AMD_RESIDENT_XCD_TARGET": "9"}], ids=["off", "no_such_xcd"])
def test_hand_off_switches(pvlib, oracle, monkeypatch, env):
    """PLANEVERB_AMD_RESIDENT_XCD=0: never the one-XCD hand-off.  ..._XCD_TARGET=9: an XCD that does not exist -- no block claims a
    tile, the host sees it and repeats the launch placement-independent, and the solver stays there: that launch is the stencil-only
    one of the solver's creation, so every run of the caller's is placement-independent.  The same vectors either way."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    chain = oracle_chain(oracle, "two_rooms", G280, BOXES, [(None, IN_A), (None, IN_B), (None, IN_A2)])
    with two_rooms(pvlib) as s:
        for k, L in enumerate((IN_A, IN_B, IN_A2)):
            run(s, L, "%r run %d" % (env, k), one_xcd=False)
            check(s, chain[k], "%r run %d" % (env, k))


def test_unchanged_window_is_not_cleared(pvlib, oracle):
    """A; A from another cell: no clear; B: the rectangle of A; A: the rectangle of B; set_fields of random planes, then A: all planes"""
    seq = [IN_A, IN_A2, IN_B, IN_A, IN_A2]
    chain = oracle_chain(oracle, "unchanged_window", G280, BOXES, [(None, L) for L in seq])
    assert [c["reached"] for c in chain] == [3111, 3111, 4131, 3111, 3111] and [c["carried"] for c in chain] == [0, 0, 3111, 4131, 4131]
    rng = np.random.default_rng(7)
    with two_rooms(pvlib) as s:
        for k, L in enumerate(seq):
            if k == 4:
                s.set_fields(*(rng.standard_normal((s.gx + 1, s.gy + 1)).astype(np.float32) for _ in range(3)))
            run(s, L, "run %d" % k)
            check(s, chain[k], "unchanged window, run %d" % k)


def test_one_epoch_leaves_no_stale_buffer_set(pvlib):
    """T = 11 is one epoch: a run publishes into buffer set 1 only and never reads.  Room A twice (the second run clears nothing),
    then a listener inside A's wall -- reach-bounded launches that start from the cleared rectangle of A: the final fields are zero
    inside A in the buffer set those launches end in -- and room A again"""
    with two_rooms(pvlib, num_steps=11) as a, two_rooms(pvlib, num_steps=11, resident_window=0) as b:
        seq = [("room A", IN_A, True), ("room A, no clear", cell(45, 65), True), ("inside A's wall", cell(28, 60), False),
               ("room A again", IN_A, True)]
        for ctx, L, window in seq:
            pair_seq(a, b, [(ctx, L, window)], planes=(0, 5, 10))
            took(a, ctx, window=window, one_xcd=window)
            if not window:
                assert not any(f[29:82, 49:112].any() for f in a.fields()), "fields inside room A after a run that never reached it"
