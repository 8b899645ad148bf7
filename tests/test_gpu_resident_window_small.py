"""GPU (-m gpu): resident-window runs (csrc/pv_solver.cpp Solver::windowFor / enqueueWindowRun / residentArgs, csrc/pv_resident.hip
ResidentArgs::window) against the oracle, on grids small enough for it.

tests/test_gpu_resident_window.py reaches the path through the default (12, 36) tile, i.e. on 4096^2 grids, where the only reference
is the library's other paths.  The path is not tied to large grids: steps_per_launch=12, tile_rows=36 (an explicit tile: neither
the whole-grid resident kernel nor the small-grid kernel) with use_graph=2 (no graph: the reach-bounded launches) plans
StepPath::Window on any grid (tests/test_host_run_plan.py pins that without a device), and findEnclosure treats the grid's edges as
ordinary faces, so an OPEN grid of few enough tiles is its own enclosure.  Every case here runs that configuration on a grid of
226 ... 280 cells and compares every bit -- final pr / vx / vy (ghost row and column included), recorded planes, the onset map
and all eight members of every cell -- with oracle.OracleGrid (tests/_boundary_ref.RingOracle for other grid boundaries), or with
a resident_window=0 solver where no oracle exists.  Every case asserts which path each run took.

The oracle restates the reference, which is self-consistent on SQUARE grids only (its rasteriser, solver and analyzer
use three different strides), so the far-edge geometries are spread over three square grids:

  252^2: 253 = 7 * 36 + 1 array rows: the ghost row is the first row of an eighth tile row that holds nothing else (and 253 =
         6 * 40 + 13 array columns); 8 x 7 tiles.
  280^2: 281 = 7 * 40 + 1 array columns: the ghost column is the first column of an eighth tile column that holds nothing else (and
         281 = 7 * 36 + 29 array rows: the last tile row's third 12-row block holds 5 rows); 8 x 8 = 64 tiles, 192 resident blocks.
  226^2: 227 = 6 * 36 + 11 array rows and 5 * 40 + 27 array columns: of the last tile row's three 12-row blocks the first is partly,
         the other two wholly outside the grid; 7 x 6 tiles.

The non-square 252 x 280 grid, where BOTH ghost lines have a tile row / column of their own, is compared with the reach-bounded
launches of the library (test_non_square_grid).
"""
import numpy as np
import pytest

import _room_metrics_ref as metrics_ref
from _boundary_ref import RingOracle, half_cell_box
from _round_shapes_ref import CONVEX, DISC, POLYGON, WALL_PATH, compose as compose_shapes
from _shapes_ref import obb_vertices
from conftest import same_bits
from test_gpu_analysis_edges import DX, EFREE, N_OPEN, OPEN_SEQ, compare_all_cells, open_chain, open_size
from test_gpu_boundary import MIXED, RIGID, check
from test_gpu_layer import check as check_layer, ref_run as layer_ref_run
from test_gpu_room_metrics import check_map, history
from test_gpu_shapes import load_material
from test_gpu_split_layer import ref_run as split_ref_run

pytestmark = pytest.mark.gpu

OPTS = dict(steps_per_launch=12, tile_rows=36, use_graph=2)
G252, G280, G226 = (252, 252), (280, 280), (226, 226)
GRIDS = {"252": G252, "280": G280, "226": G226}
ABSORBING = (0.0, 0.0, 0.0, 0.0)
HIST_TS = (0, 17, 434)  # the first step, one of the second epoch (12 ... 23), the last
D = float(DX)


def metres(grid):
    return open_size(grid[0]), open_size(grid[1])


def cell(cx, cy):
    return ((cx + 0.5) * D, 0.0, (cy + 0.5) * D)


def solver(pvlib, grid, **opts):
    s = pvlib.Solver(*metres(grid), 275, **OPTS, **opts)
    assert (s.gx, s.gy, s.T) == (grid[0], grid[1], opts.get("num_steps", 435)), (s.gx, s.gy, s.T)
    assert s.info.stepsPerLaunch == 12 and s.info.tileRows == 36 and s.info.residentKernel == 0
    return s


def run_window(s, L, ctx, taken=True):
    s.run(L)
    assert s.last_run_resident_window() == taken, "%s: window path %s" % (ctx, "not taken" if taken else "taken")


def room(r0, c0, h, w, R, t=3):
    """walls t cells thick around the air cells [r0, r0 + h) x [c0, c0 + w); every wall runs through both of its corners"""
    return [half_cell_box(DX, r0 - t, r0, c0 - t, c0 + w + t, R), half_cell_box(DX, r0 + h, r0 + h + t, c0 - t, c0 + w + t, R),
            half_cell_box(DX, r0 - t, r0 + h + t, c0 - t, c0, R), half_cell_box(DX, r0 - t, r0 + h + t, c0 + w, c0 + w + t, R)]


def corner_room(grid, r0, c0, R, t=3):
    """air cells [r0, gx) x [c0, gy) behind walls on the two near sides only: the far walls are the grid's xmax and ymax edges, so
    the component touches the last row and column and its window the ghost row and column"""
    gx, gy = grid
    return [half_cell_box(DX, r0 - t, r0, c0 - t, gy + 1, R), half_cell_box(DX, r0 - t, gx + 1, c0 - t, c0, R)]


# ------------------------------------------------------------------------------------------------------------------------------
# references, computed once per module
# ------------------------------------------------------------------------------------------------------------------------------
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def efree_of(oracle, grid):
    return memo(("efree", grid), lambda: np.float32(oracle.free_energy(*metres(grid), 275)))


def oracle_chain(oracle, key, grid, boxes, steps):
    """the oracle chain (prev=) over steps = [(material or None, listener)] on one grid with `boxes`: per run the dict
    test_gpu_boundary.check takes -- final fields, recorded planes HIST_TS, records, onsets -- plus `carried`, the cells without an
    onset in this run that had one in an earlier run.  (None: the material stays; the same listener again: only the analysis.)"""
    def make():
        o = oracle.OracleGrid(*metres(grid), 275, boxes)
        assert (o.gx, o.gy, o.T) == (grid[0], grid[1], 435)
        ef = efree_of(oracle, grid)
        out, prev, ever, last = [], None, None, None
        for mat, L in steps:
            if mat is not None:
                load_material(o, *mat)
            if mat is not None or L != last:
                f = o.fdtd(L, want_fields=True).copy()
                hist = {t: o.history()[0][t].copy() for t in HIST_TS}
                last = L
            r, d, _ = o.analyze(ef, L, prev=prev)
            on = d < 1e30
            carried = 0 if ever is None else int((~on & ever).sum())
            ever = on if ever is None else (ever | on)
            out.append(dict(f=f, hist=hist, ir={}, r=r, d=d, carried=carried, reached=int(on.sum())))
            prev = r
        o.close()
        return out
    return memo(("chain", key), make)


def ring_chain(oracle, key, grid, steps):
    """the same over steps = [(boxes, R4, listener)] with the ring oracle (grid edges of any absorption)"""
    def make():
        out, prev = [], None
        for boxes, R4, L in steps:
            ring = RingOracle(oracle, open_size(grid[0]), 275, np.array(boxes, np.float32) if boxes else None, R4, efree=efree_of(oracle, grid))
            f = ring.fdtd(L).copy()
            hist = {t: ring.history()[0][t].copy() for t in HIST_TS}
            r, d = ring.analyze(prev)
            ring.close()
            out.append(dict(f=f, hist=hist, ir={}, r=r, d=d, reached=int((d < 1e30).sum())))
            prev = r
        return out
    return memo(("ring", key), make)


def check_pair(a, b, ctx, planes=()):
    """a, b: solvers that just ran the same listener; fields, recorded planes, records and onsets of every cell"""
    for name, x, y in zip(("pr", "vx", "vy"), a.fields(), b.fields()):
        bad = ~same_bits(x, y)
        assert not bad.any(), "%s: %s differs in %d cells, first %s" % (ctx, name, bad.sum(), np.argwhere(bad)[:3].tolist())
    for t in planes:
        assert same_bits(a.history_plane(t), b.history_plane(t)).all(), "%s: recorded pr, step %d" % (ctx, t)
    (ra, da), (rb, db) = a.results(), b.results()
    compare_all_cells(ra, da, rb, db, ctx, a.T, a.fs)


# ------------------------------------------------------------------------------------------------------------------------------
# a. an open grid is the window
# ------------------------------------------------------------------------------------------------------------------------------
def open_listeners(grid):
    gx, gy = grid
    return {"centre": (gx // 2, gy // 2), "first_cell": (0, 0), "last_cell": (gx - 1, gy - 1),
            "tile_boundary": (36, 40),      # the first row / column of tile (1, 1)
            "block_boundary": (48, 57)}     # the first row of the second 12-row block of tile row 1; no tile boundary


@pytest.mark.parametrize("where", list(open_listeners(G280)))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_open_grid_is_the_window(pvlib, oracle, grid, where):
    """no geometry: the air component is the whole grid, the window every tile.  Two runs on one solver (the second re-uses flag
    words, planes and maps; its unreached cells carry the first run's records)"""
    g = GRIDS[grid]
    L = cell(*open_listeners(g)[where])
    chain = oracle_chain(oracle, ("open", grid, where), g, None, [(None, L), (None, L)])
    assert chain[0]["reached"] > 20000
    with solver(pvlib, g) as s:
        assert np.float32(s.efree) == efree_of(oracle, g)
        for rep in range(2):
            run_window(s, L, "%s %s run %d" % (grid, where, rep))
            check(s, chain[rep], "open %s, listener %s, run %d" % (grid, where, rep))


# ------------------------------------------------------------------------------------------------------------------------------
# b. grid boundaries: the window's last blocks hold the ghost row / column, whose faces carry the boundary's admittance
# ------------------------------------------------------------------------------------------------------------------------------
def corner_case(grid):
    """(boxes of the corner room, a listener inside, another one inside): the room starts in tile (4, 4)"""
    g = GRIDS[grid]
    return corner_room(g, 150, 170, 0.4), cell(g[0] - 20, 200), cell(170, g[1] - 3)


@pytest.mark.parametrize("R4", [RIGID, MIXED, ABSORBING], ids=["rigid", "mixed", "absorbing"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_grid_boundaries(pvlib, oracle, grid, R4):
    """run 1: the open grid (the window touches all four edges); run 2: a room whose far walls are the grid's xmax and ymax edges
    (a window that starts at tile (4, 4) and ends with the grid); run 3: the boundary changes under the cached enclosure"""
    g = GRIDS[grid]
    boxes, L2, L3 = corner_case(grid)
    R4b = MIXED if R4 != MIXED else RIGID
    chain = ring_chain(oracle, ("edges", grid, R4), g, [(None, R4, cell(g[0] // 2, g[1] // 2)), (boxes, R4, L2), (boxes, R4b, L3)])
    room_cells = (g[0] - 150) * (g[1] - 170)
    assert chain[0]["reached"] > 20000 and chain[1]["reached"] == room_cells == chain[2]["reached"]
    with solver(pvlib, g) as s:
        s.set_grid_boundary(R4)
        run_window(s, cell(g[0] // 2, g[1] // 2), "open")
        check(s, chain[0], "%s %s open" % (grid, R4))
        for b in boxes:
            s.add_geometry(b)
        run_window(s, L2, "corner room")
        check(s, chain[1], "%s %s corner room" % (grid, R4))
        s.set_grid_boundary(R4b)
        run_window(s, L3, "corner room, boundary changed")
        check(s, chain[2], "%s %s -> %s corner room" % (grid, R4, R4b))


def pair_seq(a, b, seq, planes=HIST_TS):
    """a: the solver under test, b: the resident_window=0 solver; seq = [(context, listener, whether a's run takes the path)]"""
    for ctx, L, taken in seq:
        run_window(a, L, ctx, taken=taken)
        run_window(b, L, ctx + " (comparison)", taken=False)
        check_pair(a, b, ctx, planes=planes)


def test_non_square_grid(pvlib):
    """252 x 280: 253 x 281 array cells = 7 x 7 full tiles, the ghost row AND the ghost column in a tile row / column of their own
    (8 x 8 tiles); against the reach-bounded launches, since the oracle is defined on square grids only"""
    g = (252, 280)
    with solver(pvlib, g) as a, solver(pvlib, g, resident_window=0) as b:
        for s in (a, b):
            s.set_grid_boundary(MIXED)
        pair_seq(a, b, [("open, centre", cell(126, 140), True), ("open, last cell", cell(251, 279), True)])
        for s in (a, b):
            for bx in corner_room(g, 150, 170, 0.4):
                s.add_geometry(bx)
        pair_seq(a, b, [("corner room", cell(240, 200), True), ("outside the corner room", cell(100, 100), True),
                        ("corner room again", cell(170, 277), True)])


# ------------------------------------------------------------------------------------------------------------------------------
# c. a room closed only by shapes: the host's copy of beta (what findEnclosure walks) against the device's rasteriser
# ------------------------------------------------------------------------------------------------------------------------------
def m_(cells):
    """cell units -> metres"""
    return (np.asarray(cells, np.float64) * D).astype(np.float32)


def shape_room(box_end):
    """the four sides of a room of about 100 x 120 cells on the 226^2 grid, as _round_shapes_ref shapes [(shape, absorption)]:
    low x: an oriented box 3 cells thick, 4.6 degrees off the y axis, from column 40 to column box_end; high x: the arc of a disc
    of 400 cells radius whose centre lies outside the grid; low y: a wall path of two segments; high y: a U-shaped polygon
    whose 6-cell base faces the room.  box_end = 180: the box runs through the polygon; 169: it ends one cell short of it."""
    mid, half = 0.5 * (40 + box_end), 0.5 * (box_end - 40)
    box = obb_vertices(*m_([60.0 + 0.08 * (mid - 110.0), mid]), *m_([2 * half, 3.0]), 0.08, 1.0)
    path = m_([(50.0, 50.0), (110.0, 46.0), (175.0, 52.0)])
    u = m_([(45, 170), (180, 170), (180, 190), (150, 190), (150, 176), (80, 176), (80, 190), (45, 190)])
    return {"box": ((CONVEX, box, 0.0), 0.35), "path": ((WALL_PATH, path, float(1.5 * D)), 0.5),
            "disc": ((DISC, m_([(560.0, 110.0)]), float(400 * D)), 0.65), "u": ((POLYGON, u, 0.0), 0.8)}


INNER_BOX = half_cell_box(DX, 100, 110, 100, 120, 0.2)  # an AABB of another absorption inside the room
IN_SHAPES = cell(120, 80)


def test_room_closed_by_shapes(pvlib, oracle):
    """closed; the box updated so that a one-cell gap opens beside the polygon (the air component becomes most of the grid); closed
    again.  A cell of the host's beta that disagrees with the device's material along a rim would end the fill, or the energy, at
    the wrong place"""
    g = G226
    with solver(pvlib, g) as s:
        s.add_geometry(INNER_BOX)
        base = s.material()
        o = oracle.OracleGrid(*metres(g), 275, np.array([INNER_BOX], np.float32))
        assert np.array_equal(base[0] != 0, o.material()[0] != 0) and (base[0] == 0).sum() == 200 + 2 * 227 - 1
        o.close()
        closed, gap = shape_room(180), shape_room(169)
        order = ["box", "path", "disc", "u"]
        ids = {}
        (_, v, _), a = closed["box"]
        ids["box"] = s.add_shape(v, a)
        (_, pts, r), a = closed["path"]
        ids["path"] = s.add_wall_path(pts, r, a)
        (_, c, r), a = closed["disc"]
        ids["disc"] = s.add_disc(c[0][0], c[0][1], r, a)
        (_, v, _), a = closed["u"]
        ids["u"] = s.add_polygon(v, a)
        # (an updated shape becomes the newest: it wins the cells it shares with the others)
        steps = [[closed[k] for k in order], [closed[k] for k in order[1:]] + [gap["box"]], [closed[k] for k in order[1:]] + [closed["box"]]]
        mats = [compose_shapes(base[0], base[1], st, g[0], g[1], s.dx) for st in steps]
        chain = oracle_chain(oracle, "shape_room", g, None, [(m, IN_SHAPES) for m in mats])
        # measured with the oracle: 11 829 cells reached in the closed room, 31 089 with the gap, 19 260 of which carry their records
        # through the third run; the gap is column 169 of rows 63 .. 65, one cell wide (the component: 35 001 cells in 5 x 6 tiles)
        assert [c["reached"] for c in chain] == [11829, 31089, 11829] and chain[2]["carried"] == 19260
        assert np.argwhere((mats[0][0] == 0) & (mats[1][0] != 0)).tolist() == [[63, 169], [64, 169], [65, 169]]
        for k, box in enumerate((None, gap["box"], closed["box"])):
            if box is not None:
                s.update_shape(ids["box"], box[0][1], box[1])
            b, R = s.material()
            assert np.array_equal(b, mats[k][0]), "step %d: beta differs in %d cells" % (k, (b != mats[k][0]).sum())
            assert np.array_equal(R.view(np.uint32), mats[k][1].view(np.uint32)), "step %d: R" % k
            run_window(s, IN_SHAPES, "shape room, step %d" % k)
            check(s, chain[k], "shape room, step %d" % k)


# ------------------------------------------------------------------------------------------------------------------------------
# d. two rooms, carried records;  e. step counts;  f. room metrics;  h. refusals -- all in the two-room scene on 280^2
# ------------------------------------------------------------------------------------------------------------------------------
ROOM_A = (30, 50, 51, 61)    # air rows 30 .. 80, ring 29 .. 81: tile rows 0, 1, 2; columns 50 .. 110, ring 49 .. 111: tile columns 1, 2
ROOM_B = (150, 170, 51, 81)  # air rows 150 .. 200: tile rows 4, 5; columns 170 .. 250: tile columns 4, 5, 6
TWO_ROOMS = room(*ROOM_A, 0.4) + room(*ROOM_B, 0.8)
IN_A, IN_B, IN_A2 = cell(40, 60), cell(160, 200), cell(72, 100)


def two_rooms(pvlib, **opts):
    s = solver(pvlib, G280, **opts)
    for b in TWO_ROOMS:
        s.add_geometry(b)
    return s


def test_two_rooms_carry_their_records(pvlib, oracle):
    """listener in room A, in room B, in room A again: the cells of the other room carry their records through each run"""
    chain = oracle_chain(oracle, "two_rooms", G280, np.array(TWO_ROOMS, np.float32), [(None, IN_A), (None, IN_B), (None, IN_A2)])
    # (measured with the oracle: 3111 = 51 x 61 cells reached in A, 4131 = 51 x 81 in B; run 2 carries A's, run 3 B's)
    assert [c["reached"] for c in chain] == [3111, 4131, 3111] and [c["carried"] for c in chain] == [0, 3111, 4131]
    with two_rooms(pvlib) as s:
        b, _ = s.material()
        o = oracle.OracleGrid(*metres(G280), 275, np.array(TWO_ROOMS, np.float32))
        assert np.array_equal(b != 0, o.material()[0] != 0)
        o.close()
        for k, L in enumerate((IN_A, IN_B, IN_A2)):
            run_window(s, L, "run %d" % k)
            check(s, chain[k], "two rooms, run %d" % k)


ROOM_C = (222, 50, 19, 21)  # air rows 222 .. 240 and columns 50 .. 70: inside tile (6, 1), so its window fits any history window
IN_C = cell(230, 60)
ROOM_D = (222, 100, 19, 41)  # air rows 222 .. 240, columns 100 .. 140: tiles (6, 2) and (6, 3) -- six blocks in two history tiles
IN_D, IN_D2 = cell(230, 118), cell(225, 121)


@pytest.mark.parametrize("steps", [1, 11, 12, 13, 200])
def test_step_counts(pvlib, steps):
    """a last epoch of fewer than 12 steps, and runs of one epoch or less; against the reach-bounded launches (the oracle's T is its
    grid's).  The history window of a short run is a few tiles around the listener (2 x 2 for T = 1): room A's window, three tile
    rows high, sticks out of it -- the refusal of windowFor that test_enclosure_and_history_window_1040 meets on a large grid -- so
    the short runs have a one-tile and a two-tile room of their own, and T = 1 asserts the refusal in room A"""
    def scene(**opts):
        s = two_rooms(pvlib, num_steps=steps, **opts)
        for b in room(*ROOM_C, 0.6) + room(*ROOM_D, 0.3):
            s.add_geometry(b)
        return s
    with scene() as a, scene(resident_window=0) as b:
        seq = [("room C", IN_C, True), ("room D: two tiles", IN_D, True), ("room D, from its other tile", IN_D2, True)]
        if steps == 1:
            seq.append(("room A: taller than the history window", IN_A, False))
        if steps == 200:
            seq += [("room A", IN_A, True), ("room B", IN_B, True)]
        seq.append(("room C again", cell(223, 69), True))
        pair_seq(a, b, [("T = %d, %s" % (steps, c), L, t) for c, L, t in seq], planes=sorted({0, steps // 2, steps - 1}))
        assert steps == 1 or (a.history_plane(steps - 1) != 0).any()


def test_room_metrics_on_the_window_path(pvlib):
    with two_rooms(pvlib) as a, two_rooms(pvlib, resident_window=0) as b:
        run_window(a, IN_A, "room A")
        run_window(b, IN_A, "comparison", taken=False)
        for s in (a, b):
            s.compute_room_metrics()
        got, delay = a.room_metrics(), a.results()[1]
        assert (delay < metrics_ref.NO_ONSET).sum() == 3111
        check_map(got, metrics_ref.room_metrics(history(a), delay, a.fs), delay, "window run")
        assert same_bits(got, b.room_metrics()).all(), "metrics of a window run vs a reach-bounded run"


def test_refusal_too_many_tiles(pvlib, oracle):
    """an open 520^2 grid is more tiles than any window holds: reach-bounded launches, the same records and onsets (the chain of
    test_gpu_analysis_edges.open_chain keeps no fields, so the final pr / vx / vy are not compared here)"""
    r, d, _, _ = open_chain(oracle)[0]
    with pvlib.Solver(open_size(N_OPEN), open_size(N_OPEN), 275, **OPTS) as s:
        assert (s.gx, s.gy, s.info.stepsPerLaunch, s.info.tileRows) == (N_OPEN, N_OPEN, 12, 36) and np.float32(s.efree) == EFREE
        run_window(s, OPEN_SEQ[0], "520^2", taken=False)
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "open 520^2")


def test_refusal_listener_in_a_wall_or_outside(pvlib):
    with two_rooms(pvlib) as a, two_rooms(pvlib, resident_window=0) as b:
        seq = [("room A", IN_A, True), ("inside A's wall", cell(28, 60), False), ("outside the grid", (-7.0, 0.0, 30.0), False),
               ("room B", IN_B, True), ("beyond xmax", cell(G280[0] + 5, 100), False), ("room A again", IN_A2, True)]
        pair_seq(a, b, seq)


# ------------------------------------------------------------------------------------------------------------------------------
# i. an enclosure that sticks out of the history window (1040^2: the smallest size class whose history window is not the grid)
# ------------------------------------------------------------------------------------------------------------------------------
def test_enclosure_and_history_window_1040(pvlib):
    """a corridor 30 cells wide and 1000 long (2 x 26 tiles: within the tile cap) with the listener at one end reaches past the
    history window around the listener: not taken; a corridor 30 x 400 with the listener in its middle: taken; both orders"""
    n = 1040
    with pvlib.Solver(open_size(n), open_size(n), 275, **OPTS) as a, \
            pvlib.Solver(open_size(n), open_size(n), 275, resident_window=0, **OPTS) as b:
        for s in (a, b):
            assert (s.gx, s.gy, s.info.stepsPerLaunch, s.info.tileRows) == (n, n, 12, 36) and s.info.histRows < s.gx
            for bx in room(100, 20, 30, 1000, 0.4) + room(300, 300, 30, 400, 0.7):
                s.add_geometry(bx)
        end, middle = cell(115, 30), cell(315, 500)
        pair_seq(a, b, [("long corridor, listener at its end", end, False), ("short corridor, listener in the middle", middle, True),
                        ("long corridor again", end, False), ("short corridor, near its end", cell(302, 690), True)], planes=(0, 434))


# ------------------------------------------------------------------------------------------------------------------------------
# g. edge layers keep a run off the path
# ------------------------------------------------------------------------------------------------------------------------------
def test_edge_layers_keep_the_run_off_the_path(pvlib, oracle):
    """226^2 with a closed room: a graded layer, then the split-field layer (planRun: layerActive), against the layer restatements;
    the layer removed: the path again, against the oracle.  The cells outside the room carry their records all the way"""
    n, w4 = G226[0], (8, 12, 0, 16)
    boxes = np.array(room(60, 70, 50, 60, 0.4), np.float32)
    L, L2 = cell(80, 100), cell(100, 75)
    first = oracle_chain(oracle, "layer_room", G226, boxes, [(None, L)])[0]
    graded = layer_ref_run(oracle, "rw_small", n, boxes, w4, L2, prev=first["r"])
    split = split_ref_run(oracle, "rw_small", n, boxes, w4, L, prev=graded["r"])
    with solver(pvlib, G226) as s:
        for b in boxes:
            s.add_geometry(b)
        run_window(s, L, "no layer")
        check(s, first, "room, no layer")
        s.set_edge_layer(w4)
        run_window(s, L2, "graded layer", taken=False)
        check_layer(s, graded, "room, graded layer", w4)
        s.set_edge_layer_split(w4)
        run_window(s, L, "split layer", taken=False)
        check_layer(s, split, "room, split layer", w4)
        s.set_edge_layer((0, 0, 0, 0))
        run_window(s, L2, "layer removed")
        o = oracle.OracleGrid(*metres(G226), 275, boxes)
        f = o.fdtd(L2, want_fields=True)
        r, d, _ = o.analyze(efree_of(oracle, G226), L2, prev=split["r"])
        check(s, dict(f=f, hist={t: o.history()[0][t] for t in HIST_TS}, ir={}, r=r, d=d), "room, layer removed")
        o.close()
