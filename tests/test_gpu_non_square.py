"""GPU (-m gpu): grids with gx != gy against an independent reference, on every stepping path and analysis kind.

A swap of gx and gy -- in an index x * (gy + 1) + y, a tile count, a reached-cell bounding box, a block copy, the validity test of a
point query, the per-axis clip of the history window -- is invisible on a square grid, and the pinned oracle cannot run a
non-square one.  The reference here is tests/_rect_ref.RectRing: the rectangle enclosed by a one-cell ring of walls
inside a SQUARE oracle grid (tests/test_host_rect_ref.py pins it, without a device, to the numpy restatement that steps with stride
gy + 1).  Every grid comes in both orientations, with a scene that is not symmetric under transposition (walls_rect), two chained
listeners (the carry rule) and, unless a case says otherwise, every cell compared bit for bit modulo the sign of zero
(test_gpu_boundary.check: final pr / vx / vy with the ghost row and column, recorded planes, impulse responses next to each edge,
the onset map and all eight members).  Every case asserts which path its runs took.

  24 x 50            the small-grid kernel (<= 1536 array cells)
  70 x 127           the resident kernel within one XCD (6 x 4 and 11 x 2 tiles of (12, 12))
  127 x 191          the resident kernel across XCDs (11 x 5 and 16 x 4 tiles)
  30 x 150           one axis shorter than one (36, 40) tile: the ghost line lies inside the only tile of that axis
  252 x 280          the (12, 36) tile path: the resident window, launches, graph, edge tiles, two kernels, sparse-emitter mode
  420 x 200, T = 160 the history window (2 (T + 2 + K) + 1 = 349 cells) clipped along one axis only
  200 x 440, T = 160 the same where the clip along y shows in histPitch (11 tile columns of 40 round up to the pitch of 10)
  126 x 150          slab groups of two and three slabs on the (8, 24) tile (three slabs need six tile rows: 121 array rows)
"""
import numpy as np
import pytest

import _bands_ref
import _decay_ref
import _echo_ref
import _echogram_ref
import _lateral_ref
import _room_metrics_ref
import _spectrum_ref
import test_gpu_bands as k_bands
import test_gpu_decay_times as k_decay
import test_gpu_echo_criterion as k_echo
import test_gpu_echogram as k_echogram
import test_gpu_lateral as k_lateral
import test_gpu_room_metrics as k_room
import test_gpu_spectrum as k_spectrum
from _layer_ref import layer_fdtd
from _rect_ref import RectRing, free_energy, listeners_rect, size_of, walls_rect
from _round_shapes_ref import CAPSULE, CONVEX, DISC, POLYGON, compose as compose_round
from _shapes_ref import compose as compose_convex, obb_vertices
from _split_layer_ref import split_fdtd
from conftest import same_bits
from test_gpu_analysis_edges import DX, EFREE, compare_all_cells
from test_gpu_bake import check_against_fresh
from test_gpu_boundary import MIXED, check, edge_cells
from test_gpu_parity import fuse_opts
from test_gpu_resident_window_small import OPTS as WINDOW_OPTS

pytestmark = pytest.mark.gpu

ABSORBING = (0.0, 0.0, 0.0, 0.0)
SMALL, XCD, CROSS, THIN, TILE = (24, 50), (70, 127), (127, 191), (30, 150), (252, 280)
CLIP, CLIP_Y, SLAB = (420, 200), (200, 440), (126, 150)
T_CLIP = 160


def both(g):
    return [g, g[::-1]]


ALL_GRIDS = [g for pair in (SMALL, XCD, CROSS, THIN, TILE, CLIP, CLIP_Y, SLAB) for g in both(pair)]


def gid(g):
    return "%dx%d" % g if isinstance(g, tuple) and len(g) == 2 and isinstance(g[0], int) else None


def metres(g):
    return size_of(g[0], DX), size_of(g[1], DX)


def cell(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def listeners(g):
    return [cell(*c) for c in listeners_rect(*g)]


def tiles(s):
    """(tile rows, tile columns) of the solver's cell array"""
    i = s.info
    return -(-(s.gx + 1) // i.tileRows), -(-(s.gy + 1) // i.tileCols)


def info_now(pvlib, s):
    """PvAmdGetInfo again (Solver.info is read at creation: an edge layer set later changes residentKernel)"""
    i = pvlib.PvAmdInfo()
    assert pvlib.lib().PvAmdGetInfo(s._h, i) == 0
    return i


# ------------------------------------------------------------------------------------------------------------------------------
# references, computed once per module
# ------------------------------------------------------------------------------------------------------------------------------
_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def efree_of(oracle, g):
    """the free-field energy restated from the cells the library reads: EFREE where the source stays on the centre cell"""
    return memo(("efree", g), lambda: free_energy(oracle, g[0], g[1], 275)[0])


def hist_ts(T):
    return sorted({0, min(17, T - 1), min(200, T - 1), T - 1})


def record(ring, prev, cells, keep_cube=False):
    """what test_gpu_boundary.check takes, of the ring's last run"""
    pr, vx, vy = ring.history()
    w = dict(hist={t: pr[t].copy() for t in hist_ts(ring.T)})
    w["ir"] = {c: np.stack([pr[:, c[0], c[1]], vx[:, c[0], c[1]], vy[:, c[0], c[1]]], 1).copy() for c in cells}
    w["r"], w["d"] = ring.analyze(prev)
    w["reached"] = int((w["d"] < 1e30).sum())
    if keep_cube:
        w["cube"] = tuple(h[:, :ring.gx, :ring.gy].copy() for h in (pr, vx, vy))
    return w


def ref_chain(oracle, g, R4=ABSORBING, steps=None, seq=None, material=None, keep_cube=False):
    """the ring rectangle's results after each run of a chain of listeners (prev=: the carry rule) on grid g with walls_rect"""
    seq = listeners(g) if seq is None else seq

    def make():
        ring = RectRing(oracle, g[0], g[1], 275, walls_rect(DX, *g), R4, efree_of(oracle, g), steps=steps)
        if material is not None:
            ring.load_material(*material[1])
        air = int((ring.material()[0][:g[0], :g[1]] != 0).sum())
        out, prev = [], None
        for L in seq:
            f = ring.fdtd(L).copy()
            w = record(ring, prev, edge_cells(*g), keep_cube)
            w["f"], w["air"] = f, air
            prev = w["r"]
            out.append(w)
        ring.close()
        return out
    return memo(("chain", g, tuple(R4), steps, tuple(seq), None if material is None else material[0], keep_cube), make)


def solver(pvlib, g, R4=None, walls=True, **opts):
    s = pvlib.Solver(*metres(g), 275, **opts)
    assert (s.gx, s.gy, s.T) == (g[0], g[1], opts.get("num_steps", 435)), (s.gx, s.gy, s.T)
    if walls:
        for b in walls_rect(DX, *g):
            s.add_geometry(b)
    if R4 is not None:
        s.set_grid_boundary(R4)
    return s


def run_chain(s, g, chain, ctx, took=None, seq=None):
    """every listener of the chain on one solver; every cell of every run"""
    for k, (L, w) in enumerate(zip(listeners(g) if seq is None else seq, chain)):
        s.run(L)
        if took is not None:
            took(s, "%s run %d" % (ctx, k))
        check(s, w, "%s %dx%d run %d" % (ctx, g[0], g[1], k))
        assert 0 < w["reached"] <= w["air"]
        print("non-square: %s %dx%d run %d: tiles %dx%d of (%d, %d), %d cells compared, %d of %d air cells reached" % (
            ctx, g[0], g[1], k, *tiles(s), s.info.tileRows, s.info.tileCols, g[0] * g[1], w["reached"], w["air"]))


def took(resident=None, window=False, one_xcd=False):
    def f(s, ctx):
        if resident is not None:
            assert s.info.residentKernel == resident, "%s: residentKernel %d" % (ctx, s.info.residentKernel)
        assert s.last_run_resident_window() == window, "%s: window path %s" % (ctx, "not taken" if window else "taken")
        assert s.last_run_one_xcd() == one_xcd, "%s: one-XCD hand-off %s" % (ctx, "not taken" if one_xcd else "taken")
    return f


def check_efree(s, oracle, g):
    want = efree_of(oracle, g)
    assert np.float32(s.efree).view(np.uint32) == np.float32(want).view(np.uint32), (g, s.efree, want)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the small-grid kernel: 24 x 50 (25 x 51 = 1275 array cells)
# ------------------------------------------------------------------------------------------------------------------------------
# (no accessor tells the small-grid kernel from the graph: "small" forces it as test_same_bits_on_every_path does; the default
# resolves to it -- planRun, tests/test_host_run_plan.py -- and "resident" asks for the resident kernel by name)
SMALL_FORMS = {"default": (dict(), None, False), "small": (dict(resident_kernel=2, small_grid_kernel=1), 0, False),
               "resident": (dict(resident_kernel=1), 1, True),
               "graph": (dict(resident_kernel=2, small_grid_kernel=2, use_graph=1), 0, False)}


@pytest.mark.parametrize("form", list(SMALL_FORMS))
@pytest.mark.parametrize("g", both(SMALL), ids=gid)
def test_small_grid_kernel(pvlib, oracle, g, form):
    opts, resident, one_xcd = SMALL_FORMS[form]
    chain = ref_chain(oracle, g)
    with solver(pvlib, g, **opts) as s:
        assert (s.gx + 1) * (s.gy + 1) <= 1536
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "small " + form, took(resident, one_xcd=one_xcd))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the resident kernel within one XCD: 70 x 127 (6 x 4 tiles), 127 x 70 (11 x 2)
# ------------------------------------------------------------------------------------------------------------------------------
OFF = dict(resident_kernel=2, small_grid_kernel=2)
XCD_FORMS = {"default": (dict(), ABSORBING, 1, True), "mixed": (dict(), MIXED, 1, True),
             "graph": (dict(use_graph=1, **OFF), ABSORBING, 0, False), "graph_mixed": (dict(use_graph=1, **OFF), MIXED, 0, False),
             "launches_reach": (dict(use_graph=2, reach_bound=1, **OFF), ABSORBING, 0, False),
             "launches_full": (dict(use_graph=2, reach_bound=0, **OFF), ABSORBING, 0, False),
             "launches_reach_mixed": (dict(use_graph=2, reach_bound=1, **OFF), MIXED, 0, False)}


@pytest.mark.parametrize("form", list(XCD_FORMS))
@pytest.mark.parametrize("g", both(XCD), ids=gid)
def test_resident_kernel_one_xcd(pvlib, oracle, g, form):
    opts, R4, resident, one_xcd = XCD_FORMS[form]
    chain = ref_chain(oracle, g, R4)
    with solver(pvlib, g, R4, **opts) as s:
        assert (s.info.tileRows, s.info.tileCols) == (12, 40) and tiles(s) == {XCD: (6, 4), XCD[::-1]: (11, 2)}[g]
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "70 x 127 " + form, took(resident, one_xcd=one_xcd))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. the resident kernel across XCDs: 127 x 191 (11 x 5 tiles), 191 x 127 (16 x 4)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", both(CROSS), ids=gid)
def test_resident_kernel_across_xcds(pvlib, oracle, g):
    chain = ref_chain(oracle, g)
    with solver(pvlib, g) as s:
        assert tiles(s) == {CROSS: (11, 5), CROSS[::-1]: (16, 4)}[g] and tiles(s)[0] * tiles(s)[1] > 32
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "127 x 191", took(1, one_xcd=False))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. one axis shorter than one (36, 40) tile: 30 x 150 (1 x 4 tiles), 150 x 30 (5 x 1)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [2, 0], ids=["launches", "graph"])
@pytest.mark.parametrize("g", both(THIN), ids=gid)
def test_axis_shorter_than_a_tile(pvlib, oracle, g, graph):
    """use_graph=2: the open grid is its own enclosure of 4 or 5 tiles -- the resident window, 12 or 15 blocks on one XCD;
    use_graph=0: the replayed graph"""
    chain = ref_chain(oracle, g)
    with solver(pvlib, g, steps_per_launch=12, tile_rows=36, use_graph=graph) as s:
        assert (s.info.tileRows, s.info.tileCols) == (36, 40) and tiles(s) == {THIN: (1, 4), THIN[::-1]: (5, 1)}[g]
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "30 x 150 use_graph=%d" % graph, took(0, window=graph == 2, one_xcd=graph == 2))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the (12, 36) tile path: 252 x 280 (8 x 8 tiles: both ghost lines in a tile row / column of their own) and 280 x 252 (8 x 7:
#    neither)
# ------------------------------------------------------------------------------------------------------------------------------
T36 = dict(steps_per_launch=12, tile_rows=36)
TILE_FORMS = {"window": (WINDOW_OPTS, ABSORBING, True), "window_mixed": (WINDOW_OPTS, MIXED, True),
              "launches_reach": (dict(resident_window=0, **WINDOW_OPTS), ABSORBING, False),
              "launches_reach_mixed": (dict(resident_window=0, **WINDOW_OPTS), MIXED, False),
              "launches_full": (dict(reach_bound=0, **WINDOW_OPTS), ABSORBING, False),
              "graph": (dict(use_graph=1, **T36), ABSORBING, False), "graph_mixed": (dict(use_graph=1, **T36), MIXED, False),
              "edge_tiles_0": (dict(edge_tiles=0, **T36), ABSORBING, False), "edge_tiles_1": (dict(edge_tiles=1, **T36), ABSORBING, False),
              "edge_tiles_1_mixed": (dict(edge_tiles=1, **T36), MIXED, False),
              "two_kernel": (dict(merged_launch=0), ABSORBING, False), "two_kernel_mixed": (dict(merged_launch=0), MIXED, False)}


@pytest.mark.parametrize("form", list(TILE_FORMS))
@pytest.mark.parametrize("g", both(TILE), ids=gid)
def test_tile_path(pvlib, oracle, g, form):
    opts, R4, window = TILE_FORMS[form]
    chain = ref_chain(oracle, g, R4)
    with solver(pvlib, g, R4, **opts) as s:
        if "steps_per_launch" in opts:
            assert (s.info.stepsPerLaunch, s.info.tileRows, s.info.tileCols) == (12, 36, 40)
            assert tiles(s) == {TILE: (8, 8), TILE[::-1]: (8, 7)}[g]
        check_efree(s, oracle, g)
        # (8 x 8 or 8 x 7 tiles = 192 or 168 blocks of the resident window: more than one XCD holds)
        run_chain(s, g, chain, "252 x 280 " + form, took(0, window=window, one_xcd=False))


@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R4", [ABSORBING, MIXED], ids=["absorbing", "mixed"])
@pytest.mark.parametrize("g", both(TILE), ids=gid)
def test_sparse_emitter_mode(pvlib, oracle, g, R4, fuse):
    """streaming_analysis=1: the forward outputs of every cell; wet gain and RT60 at the emitters only -- one beside each edge"""
    gx, gy = g
    L = listeners(g)[0]
    w = ref_chain(oracle, g, R4)[0]
    r, d = w["r"], w["d"]
    on = d < 1e30
    lc = listeners_rect(gx, gy)[0]
    cells = [(lc[0], lc[1] - 10), (10, 10)]
    for x, y in ((0, None), (gx - 1, None), (None, 0), (None, gy - 1)):
        line = on[x, :] if y is None else on[:, y]
        k = int(np.flatnonzero(line)[line.sum() // 2])
        cells.append((x, k) if y is None else (k, y))
    cells = np.array(cells)
    assert on[cells[:, 0], cells[:, 1]].all()
    E = np.array([cell(cx, cy) for cx, cy in cells], np.float32)
    with solver(pvlib, g, R4, streaming_analysis=1, **fuse_opts(fuse)) as s:
        assert s.info.streamFuse == fuse and s.info.residentKernel == 0
        s.set_emitters(E)
        s.run(L)
        got, gd = s.results()
        em = np.zeros(gd.shape, bool)
        em[cells[:, 0], cells[:, 1]] = True
        want = r.copy()
        want[..., 1][~em] = 0
        want[..., 2][~em] = 0
        compare_all_cells(got, gd, want, d, "sparse-emitter %dx%d fuse %d %s" % (gx, gy, fuse, R4), s.T, s.fs)
        for i, e in enumerate(E):
            assert same_bits(s.get_output(e).as_array(), r[cells[i, 0], cells[i, 1]]).all(), "emitter %s" % cells[i]


# ------------------------------------------------------------------------------------------------------------------------------
# 6. the history window clipped along one axis only (Solver::init: wtx, wty), T = 160
# ------------------------------------------------------------------------------------------------------------------------------
def clipped_axes(s):
    """(x clipped, y clipped) as histRows / histPitch show them"""
    ntx, nty = tiles(s)
    return s.info.histRows < ntx * s.info.tileRows, s.info.histPitch < -(-nty * s.info.tileCols // 64) * 64


@pytest.mark.parametrize("graph", [0, 2], ids=["default", "launches"])
@pytest.mark.parametrize("g", both(CLIP) + both(CLIP_Y), ids=gid)
def test_history_window_clipped_along_one_axis(pvlib, oracle, g, graph):
    """2 (T + 2 + K) + 1 = 349 cells: narrower than 421 or 441 array cells, wider than 201.  The listeners of the chain lie
    beside the middle of the long axis and near its far end, so the window moves along the clipped axis between the runs"""
    chain = ref_chain(oracle, g, steps=T_CLIP)
    with solver(pvlib, g, num_steps=T_CLIP, use_graph=graph) as s:
        i = s.info
        assert (i.stepsPerLaunch, i.tileRows, i.tileCols) == (12, 12, 40)
        reach = 2 * (T_CLIP + 2 + 12) + 1
        long_x = g[0] > g[1]
        ntx, nty = tiles(s)
        if long_x:
            assert clipped_axes(s) == (True, False) and i.histRows == (-(-reach // 12) + 1) * 12 < s.gx + 1
        else:
            # (420: 11 tile columns clipped to 10, 440 and 400 columns, both round up to a pitch of 448: histPitch cannot show it)
            assert i.histRows == ntx * 12 and i.histPitch == -(-(-(-reach // 40) + 1) * 40 // 64) * 64 == 448
            assert clipped_axes(s) == (False, g[1] == 440) and nty * 40 > (-(-reach // 40) + 1) * 40
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "clipped window use_graph=%d" % graph, took(0))


# ------------------------------------------------------------------------------------------------------------------------------
# 7. slab groups on one device
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nslabs", [2, 3])
@pytest.mark.parametrize("g", both(SLAB), ids=gid)
def test_slab_groups(pvlib, oracle, g, nslabs):
    with pvlib.Solver(*metres(g), 275, slabs=[0] * nslabs, steps_per_launch=8, tile_rows=24) as s:
        assert (s.gx, s.gy) == g and (s.info.stepsPerLaunch, s.info.tileRows, s.info.tileCols) == (8, 24, 48)
        si = s.slab_info()
        assert si.nslabs == nslabs and sum(si.rows[:nslabs]) == g[0] + 1
        L = cell(si.row0[1] - 2, g[1] // 3 + 3)  # two rows from the first slab boundary
        seq = [L, listeners(g)[1]]
        chain = ref_chain(oracle, g, MIXED, seq=seq)
        for b in walls_rect(DX, *g):
            s.add_geometry(b)
        s.set_grid_boundary(MIXED)
        check_efree(s, oracle, g)
        run_chain(s, g, chain, "%d slabs" % nslabs, seq=seq)


# ------------------------------------------------------------------------------------------------------------------------------
# 8. edge layers: the references are the numpy restatements on the rectangle (duck()), analysed through the square grid
# ------------------------------------------------------------------------------------------------------------------------------
W4 = (24, 0, 7, 40)
SPLIT_R0 = 1e-4


def layer_cells(g):
    gx, gy = g
    return sorted(set(edge_cells(gx, gy) + [(W4[0] - 1, gy // 3), (W4[0], gy // 3), (gx // 3, 3), (gx // 3, W4[2]), (gx // 3, gy - W4[3]),
                                             (gx // 3, gy - 5), (3, 3)]))


def layer_ref(oracle, pvlib, g, model):
    def make():
        ring = RectRing(oracle, g[0], g[1], 275, walls_rect(DX, *g), ABSORBING, efree_of(oracle, g))
        L = listeners(g)[0]
        tabs = pvlib.edge_layer_tables(*metres(g), 275, W4, r0=SPLIT_R0 if model == "split" else None)
        assert tabs["apx"].shape == (g[0] + 1,) and tabs["apy"].shape == (g[1] + 1,)
        if model == "split":
            f, hist, resp, _ = split_fdtd(ring.duck(), L, tabs, cells=layer_cells(g))
        else:
            f, hist, resp = layer_fdtd(ring.duck(), L, tabs, cells=layer_cells(g))
        w = dict(f=f, hist={t: hist[0][t].copy() for t in hist_ts(ring.T)}, ir=resp)
        w["r"], w["d"] = ring.analyze_history(hist, L)
        ring.close()
        return w
    return memo(("layer", g, model), make)


def exact_velocity(g):
    """test_gpu_layer.exact_velocity for a gx x gy grid: the cells whose velocity faces carry no damping"""
    m = np.zeros((g[0] + 1, g[1] + 1), bool)
    m[W4[0]:g[0] - W4[1] + 1, W4[2]:g[1] - W4[3] + 1] = True
    return m


def check_layer(s, w, ctx, g):
    """test_gpu_layer.check with the layer mask of a non-square grid: the library records the pressure only and re-derives the
    velocities with the undamped recurrence, so the velocity members of layer cells are not the damped stencil's"""
    for k, (got, want) in enumerate(zip(s.fields(), w["f"])):
        bad = ~same_bits(got, want)
        assert not bad.any(), "%s field %s: %d cells differ, first %s" % (ctx, "pr vx vy".split()[k], bad.sum(), np.argwhere(bad)[0])
    for t, plane in w["hist"].items():
        assert same_bits(s.history_plane(t), plane).all(), "%s recorded pr, step %d" % (ctx, t)
    ev = exact_velocity(g)
    for c, ir in w["ir"].items():
        cols = slice(None) if ev[c] else slice(0, 1)
        assert same_bits(s.impulse_response(*c)[:, cols], ir[:, cols]).all(), "%s impulse response at %s" % (ctx, c)
    got, gd = s.results()
    want = w["r"].copy()
    lay = ~ev[:g[0], :g[1]]
    want[lay, 6:8] = got[lay, 6:8]
    compare_all_cells(got, gd, want, w["d"], ctx, s.T, s.fs)
    assert ev[:g[0], :g[1]].sum() > 0 and lay.sum() > 0


@pytest.mark.parametrize("model", ["graded", "split"])
@pytest.mark.parametrize("g", both(XCD) + [TILE], ids=gid)
def test_edge_layers(pvlib, oracle, g, model):
    """70 x 127 and 127 x 70: the preset tile, where a layer resolves the resident kernel off; 252 x 280: the (12, 36) tile, where it
    keeps the run off the window path"""
    w = layer_ref(oracle, pvlib, g, model)
    opts = WINDOW_OPTS if g == TILE else {}
    with solver(pvlib, g, **opts) as s:
        if model == "split":
            s.set_edge_layer_split(W4, SPLIT_R0)
            assert s.edge_layer_model() == ("split", SPLIT_R0)
        else:
            s.set_edge_layer(W4)
        assert list(s.edge_layer()) == list(W4) and info_now(pvlib, s).residentKernel == 0
        for rep in range(2):
            s.run(listeners(g)[0])
            assert not s.last_run_resident_window() and not s.last_run_one_xcd()
            check_layer(s, w, "%s layer %dx%d run %d" % (model, g[0], g[1], rep), g)


# ------------------------------------------------------------------------------------------------------------------------------
# 9. rasterised shapes
# ------------------------------------------------------------------------------------------------------------------------------
def shapes():
    """[((kind, points, radius), absorption)] in metres, oldest first.  70 cells are 24.96 m, 127 cells 45.29 m:
    box:     crosses the far y edge of 70 x 127; outside 127 x 70
    disc:    crosses the far x edge of 70 x 127; inside 127 x 70
    capsule: around y = 25 m, beyond the short side: inside 70 x 127, partly outside 127 x 70 (it crosses that grid's far y edge)
    polygon: an L around x = 45 m: crosses the far x edge of 127 x 70; outside 70 x 127"""
    box = obb_vertices(12.0, 44.5, 6.0, 2.5, 1.0, 0.2)
    ell = np.array([(42.0, 8.0), (47.0, 8.0), (47.0, 10.0), (44.0, 10.0), (44.0, 14.0), (42.0, 14.0)], np.float32)
    return [((CONVEX, box, 0.0), 0.35), ((DISC, np.array([(24.5, 15.0)], np.float32), 2.0), 0.65),
            ((CAPSULE, np.array([(15.0, 24.0), (20.0, 26.5)], np.float32), 0.7), 0.5), ((POLYGON, ell, 0.0), 0.8)]


@pytest.mark.parametrize("g", both(XCD), ids=gid)
def test_shapes(pvlib, oracle, g):
    gx, gy = g
    sh = shapes()
    with solver(pvlib, g) as s:
        base = s.material()
        s.add_oriented_box(12.0, 44.5, 6.0, 2.5, 1.0, 0.2, sh[0][1])
        s.add_disc(24.5, 15.0, 2.0, sh[1][1])
        s.add_capsule((15.0, 24.0), (20.0, 26.5), 0.7, sh[2][1])
        s.add_polygon(sh[3][0][1], sh[3][1])
        first = compose_convex(base[0], base[1], [(sh[0][0][1], sh[0][1])], gx, gy, s.dx)
        assert same_bits(first[1], compose_round(base[0], base[1], sh[:1], gx, gy, s.dx)[1]).all()
        b, R = compose_round(first[0], first[1], sh[1:], gx, gy, s.dx)
        covered = [int(((compose_round(base[0], base[1], [x], gx, gy, s.dx)[0] == 0) & (base[0] != 0)).sum()) for x in sh]
        assert all(covered[:3]) if g == XCD else all(covered[1:]), covered  # (each grid has three of the four shapes)
        assert (b[gx - 1, :gy] != base[0][gx - 1, :gy]).any() and (b[:gx, gy - 1] != base[0][:gx, gy - 1]).any(), "a shape on each far edge"
        gb, gR = s.material()
        assert np.array_equal(gb, b), "beta differs in %d cells, first %s" % ((gb != b).sum(), np.argwhere(gb != b)[:3].tolist())
        assert np.array_equal(gR.view(np.uint32), R.view(np.uint32)), "R"
        for cx, cy in listeners_rect(gx, gy):
            assert b[cx, cy] == 1
        chain = ref_chain(oracle, g, material=("shapes", (b, R)))
        for k, (L, w) in enumerate(zip(listeners(g), chain)):
            s.run(L)
            took(1, one_xcd=True)(s, "shapes run %d" % k)
            check(s, w, "shapes %dx%d run %d" % (gx, gy, k))
            assert 0 < w["reached"] <= w["air"]


# ------------------------------------------------------------------------------------------------------------------------------
# 10. a bake
# ------------------------------------------------------------------------------------------------------------------------------
def test_bake(pvlib):
    """a 3 x 5 lattice of probes on 70 x 127 whose last two rows lie beyond the short side; every probe against a plain run"""
    g = XCD

    def make():
        return solver(pvlib, g)

    with make() as s:
        b = pvlib.Bake(s, 2, 2.0, 3.0, 9.0, 9.5, 3, 5)
        try:
            b.run([s])
            i = b.info()
            assert (i["gx"], i["gy"], i["nx"], i["nz"]) == (70, 127, 3, 5) and i["probesBaked"] == 15 and i["probesInvalid"] == 0
            states = check_against_fresh(pvlib, b, make)
            assert states == [1] * 15
        finally:
            b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 11. the seven analysis kinds
# ------------------------------------------------------------------------------------------------------------------------------
BINS, BANDS, SLOTS = [63.0, 125.0, 250.0], [125.0, 250.0], (0.005, 16)


class Kind:
    def __init__(self, name, mod, ref, setup=None):
        self.name, self.mod, self.ref, self.setup = name, mod, ref, setup or (lambda s: None)

    def compute(self, s):
        assert getattr(s, "compute_" + self.name)() > 0

    def map(self, s):
        return getattr(s, self.name)()

    def block(self, s, *a):
        return getattr(s, self.name + "_block")(*a)

    def at(self, s, pos):
        return getattr(s, self.name + "_at")(pos)


def _spectrum(pvlib, s, p, vx, vy, d):
    c, sn = pvlib.host_spectrum_tables(s.T, s.fs, s.spectrum_bins())
    return _spectrum_ref.spectrum(p, d, c, sn, s.pulse())


KINDS = [Kind("room_metrics", k_room, lambda pvlib, s, p, vx, vy, d: _room_metrics_ref.room_metrics(p, d, s.fs)),
         Kind("spectrum", k_spectrum, _spectrum, lambda s: s.set_spectrum_bins(BINS)),
         Kind("decay_times", k_decay, lambda pvlib, s, p, vx, vy, d: _decay_ref.decay_times(p, d, s.fs)),
         Kind("lateral_fraction", k_lateral, lambda pvlib, s, p, vx, vy, d: _lateral_ref.lateral_fraction(p, vx, vy, d, s.fs)),
         Kind("band_metrics", k_bands, lambda pvlib, s, p, vx, vy, d: _bands_ref.band_metrics(p, d, s.fs, s.band_coefs()),
              lambda s: s.set_bands(BANDS)),
         Kind("echogram", k_echogram, lambda pvlib, s, p, vx, vy, d: _echogram_ref.echogram(p, vx, vy, d, s.fs, *SLOTS),
              lambda s: s.set_echogram(*SLOTS)),
         Kind("echo_criterion", k_echo, lambda pvlib, s, p, vx, vy, d: _echo_ref.echo_criterion(p, d, s.fs))]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.name)
@pytest.mark.parametrize("g", both(XCD), ids=gid)
def test_analysis_kinds(pvlib, oracle, g, kind):
    """the whole map against the kind's numpy restatement fed with the RING's recorded cube (so a map transposed, or built from a
    history read with the wrong stride, cannot agree with itself), block reads along both far edges, point queries in the corners
    and at two cells that lie inside one orientation only"""
    gx, gy = g
    w = ref_chain(oracle, g, keep_cube=True)[0]
    p, vx, vy = w["cube"]
    with solver(pvlib, g) as s:
        kind.setup(s)
        s.run(listeners(g)[0])
        took(1, one_xcd=True)(s, kind.name)
        res, delay = s.results()
        assert same_bits(delay, w["d"]).all(), "onset map"
        kind.compute(s)
        got = kind.map(s)
        assert got.shape[:2] == (gx, gy)
        want = kind.ref(pvlib, s, p, vx, vy, delay)
        kind.mod.check_map(got, want, delay, "%s %dx%d" % (kind.name, gx, gy))
        reached = delay < 1e30
        tail = got.reshape(gx, gy, -1)
        assert np.array_equal(np.isnan(tail).all(axis=-1), ~reached) and reached.sum() == w["air"] and (~reached).sum() > 50
        # blocks along the far edges; a block of the transposed shape does not fit
        assert same_bits(kind.block(s, gx - 5, 0, 5, gy), got[gx - 5:]).all()
        assert same_bits(kind.block(s, 0, gy - 5, gx, 5), got[:, gy - 5:]).all()
        for bad in ((0, 0, gy, gx), (gx - 5, 0, 6, gy), (0, gy - 5, gx, 6)):
            with pytest.raises(pvlib.PlaneverbError):
                kind.block(s, *bad)
        with pytest.raises(pvlib.PlaneverbError):
            s.results_block(0, 0, gy, gx)
        rb, db = s.results_block(gx - 5, 0, 5, gy)
        assert same_bits(rb, res[gx - 5:]).all() and same_bits(db, delay[gx - 5:]).all()
        # point queries
        for c in ((gx - 1, gy - 1), (gx - 1, 0), (0, gy - 1), (100, 10), (10, 100)):
            inside = c[0] < gx and c[1] < gy
            assert inside == (c != ((100, 10) if g == XCD else (10, 100)))
            assert (pvlib.host_cells(*metres(g), 275, *cell(*c)[::2])[1] == c) == inside
            at, out = kind.at(s, cell(*c)), s.get_output(cell(*c)).as_array()
            if inside:
                assert same_bits(at, got[c]).all() and same_bits(out, res[c]).all(), c
                assert reached[c] and not np.isnan(at).all(), c
            else:
                assert np.isnan(at).all() and at.shape == got[0, 0].shape, c
                assert out[0] == -1 and not out[1:].any(), c


def sample_cells(delay, tile_rows, tile_cols, n=320):
    """reached cells: the first and last row / column of tiles (tile-edge cells), then a spread of the rest"""
    gx, gy = delay.shape
    on = delay < 1e30
    xs = sorted({x for k in range(1, gx // tile_rows + 1) for x in (k * tile_rows - 1, k * tile_rows) if x < gx})
    ys = sorted({y for k in range(1, gy // tile_cols + 1) for y in (k * tile_cols - 1, k * tile_cols) if y < gy})
    rng = np.random.default_rng(5)
    edge = [(x, int(rng.integers(gy))) for x in xs for _ in range(3)] + [(int(rng.integers(gx)), y) for y in ys for _ in range(6)]
    corner = [(x, y) for x in xs[:6] for y in ys[:3]]
    reached = np.argwhere(on)
    rest = [tuple(int(v) for v in reached[k]) for k in rng.choice(len(reached), 2 * n, replace=False)]
    cells = [c for c in dict.fromkeys(corner + edge) if on[c]][:n // 2]
    cells = list(dict.fromkeys(cells + rest))[:n]
    n_edge = sum(1 for c in cells if c[0] in xs or c[1] in ys)
    assert len(cells) >= 300 and n_edge >= 60, (len(cells), n_edge)
    return np.array(cells)


@pytest.mark.parametrize("g", both(CLIP), ids=gid)
def test_analysis_kinds_clipped_window(pvlib, g):
    """420 x 200 and 200 x 420, T = 160: >= 300 reached cells per kind, tile-edge cells among them, against the restatement fed with
    the solver's own recorded planes (what each kind's test_window_smaller_than_the_grid does; the stepping on these grids is
    test_history_window_clipped_along_one_axis).  The second listener of the chain, near the far end of the clipped axis"""
    gx, gy = g
    with solver(pvlib, g, num_steps=T_CLIP) as s:
        for k in KINDS:
            k.setup(s)
        s.run(listeners(g)[1])
        res, delay = s.results()
        cells = sample_cells(delay, s.info.tileRows, s.info.tileCols)
        cx, cy = cells[:, 0], cells[:, 1]
        irs = np.stack([s.impulse_response(int(x), int(y)) for x, y in cells], axis=1)  # [T, N, 3]
        planes = np.stack([s.history_plane(t)[cx, cy] for t in range(s.T)])
        assert same_bits(planes, irs[..., 0]).all()
        d = delay[cx, cy]
        for k in KINDS:
            k.compute(s)
            got = k.map(s)
            want = k.ref(pvlib, s, planes, irs[..., 1], irs[..., 2], d)
            bad = ~same_bits(got[cx, cy], want)
            assert not bad.any(), "%s %dx%d: %d values differ, first cell %s" % (k.name, gx, gy, bad.sum(), cells[np.argwhere(bad)[0][0]])
            flat = got.reshape(gx, gy, -1)
            assert np.array_equal(np.isnan(flat).all(axis=-1), ~(delay < 1e30)), k.name
            assert same_bits(k.block(s, gx - 5, 0, 5, gy), got[gx - 5:]).all(), k.name
            assert same_bits(k.block(s, 0, gy - 5, gx, 5), got[:, gy - 5:]).all(), k.name
