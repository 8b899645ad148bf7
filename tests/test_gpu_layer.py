"""GPU (-m gpu): graded absorbing edge layers (PvAmdSetEdgeLayer, PlaneverbSetEdgeLayer).

The oracle is tests/_layer_ref.py: the numpy float32 restatement of the stencil with the library's own tables
(PvAmdHostEdgeLayerTables, pinned to the documented formula and, at width 0, to the pinned oracle by tests/test_host_layer.py),
analysed by the pinned oracle's unchanged analysis.  Every case compares every cell: final fields (ghost row and column
included), recorded planes, impulse responses inside and next to the layers, the onset map and all eight members, bit for bit
modulo the sign of zero (compare_all_cells).
"""
import numpy as np
import pytest

from _boundary_ref import half_cell_box
from _layer_ref import analyze, layer_fdtd
from conftest import same_bits
from test_gpu_analysis_edges import DX, compare_all_cells, open_size

pytestmark = pytest.mark.gpu

_REF = {}
_EFREE = {}


def efree_of(oracle, size, res=275):
    if (size, res) not in _EFREE:
        _EFREE[(size, res)] = np.float32(oracle.free_energy(size, size, res))
    return _EFREE[(size, res)]


def cell_of(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def probe_cells(n, w4):
    """cells inside each layer, on its inner boundary and next to it, corners and the ghost row / column"""
    out = [(0, 0), (n - 1, n - 1), (n, n // 2), (n // 2, n)]
    for k, w in enumerate(w4):
        for d in ([0, w - 1, w, w + 1] if w else [0, 1]):
            x = d if k in (0, 2) else n - 1 - d
            out.append((x, n // 3) if k < 2 else (n // 3, x))
    return sorted(set(out))


def walls(n):
    """an interior wall, a wall inside the x = 0 layer and one across the y = gy layer"""
    return np.array([half_cell_box(DX, n // 3, n // 3 + 2, 30, n - 30, 0.3),
                     half_cell_box(DX, 4, 10, n // 2, n // 2 + 9, 0.6),
                     half_cell_box(DX, 2 * n // 3, 2 * n // 3 + 7, n - 12, n + 1, 0.1)], np.float32)


def ref_run(oracle, key, n, boxes, w4, L, R4=None, hist_ts=(0, 100, 434), prev=None):
    """the restatement's results of one run: dict(f, hist {t: pr}, ir {cell: [T, 3]}, r, d)"""
    from planeverb_amd import api
    k = (key, n, tuple(w4), tuple(L), None if R4 is None else tuple(R4), None if prev is None else prev.tobytes()[:64] + bytes([len(prev)]))
    if k in _REF:
        return _REF[k]
    size = open_size(n)
    o = oracle.OracleGrid(size, size, 275, boxes)
    assert o.gx == n
    tabs = api.edge_layer_tables(size, size, 275, w4)
    cells = probe_cells(n, w4)
    f, hist, resp = layer_fdtd(o, L, tabs, R4=R4, cells=cells)
    w = dict(f=f, hist={t: hist[0][t].copy() for t in hist_ts}, ir=resp)
    w["r"], w["d"] = analyze(o, hist, efree_of(oracle, size), L, prev=prev)
    o.close()
    _REF[k] = w
    return w


def exact_velocity(n, w4):
    """cells whose velocity faces x and y carry no damping: the library records the pressure only and re-derives vx / vy with the
    undamped recurrence (pv_analysis_dev.h), so the impulse-response velocities and the source direction (srcDirX / srcDirY)
    of the cells inside a layer are not the damped stencil's (include/planeverb_amd.h PvAmdSetEdgeLayer)"""
    m = np.zeros((n + 1, n + 1), bool)
    m[w4[0]:n - w4[1] + 1, w4[2]:n - w4[3] + 1] = True
    return m


def check(s, w, ctx, w4):
    for k, (got, want) in enumerate(zip(s.fields(), w["f"])):
        bad = ~same_bits(got, want)
        assert not bad.any(), "%s field %s: %d cells differ, first %s" % (ctx, "pr vx vy".split()[k], bad.sum(), np.argwhere(bad)[0])
    for t, plane in w["hist"].items():
        assert same_bits(s.history_plane(t), plane).all(), "%s recorded pr, step %d" % (ctx, t)
    n = s.gx
    ev = exact_velocity(n, w4)
    for c, ir in w["ir"].items():
        got = s.impulse_response(*c)
        cols = slice(None) if ev[c] else slice(0, 1)
        assert same_bits(got[:, cols], ir[:, cols]).all(), "%s impulse response at %s" % (ctx, c)
    got, gd = s.results()
    want = w["r"].copy()
    lay = ~ev[:n, :n]
    want[lay, 6:8] = got[lay, 6:8]  # (velocity-derived members of layer cells: see exact_velocity)
    compare_all_cells(got, gd, want, w["d"], ctx, s.T, s.fs)
    assert ev[:n, :n].sum() > 0


def solver(pvlib, n, boxes, w4, R4=None, **opts):
    s = pvlib.Solver(open_size(n), open_size(n), 275, **opts)
    for b in (boxes if boxes is not None else []):
        s.add_geometry(b)
    if R4 is not None:
        s.set_grid_boundary(R4)
    s.set_edge_layer(w4)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's preset grids: the resident / small-grid kernel resolves off
# ------------------------------------------------------------------------------------------------------------------------------
PRESETS = [(70, (24, 24, 24, 24)), (127, (24, 0, 7, 40)), (254, (24, 24, 24, 24))]


@pytest.mark.parametrize("n,w4", PRESETS, ids=[str(p[0]) for p in PRESETS])
def test_presets(pvlib, oracle, n, w4):
    L = cell_of(n // 2, n // 3 + 6)
    w = ref_run(oracle, "preset", n, walls(n), w4, L)
    with solver(pvlib, n, walls(n), w4) as s:
        assert s.info.residentKernel == 0
        assert list(s.edge_layer()) == list(w4)
        for rep in range(2):
            s.run(L)
            check(s, w, "%d^2 run %d" % (n, rep), w4)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. 520^2 on the tile path: graph replay and plain launches, reach bound on and off; walls and the listener inside a layer
# ------------------------------------------------------------------------------------------------------------------------------
N520 = 520
W520 = (24, 0, 7, 40)
L520_IN = cell_of(10, 300)   # inside the x = 0 layer, in a layer tile
L520 = cell_of(300, 200)


@pytest.mark.parametrize("form", ["graph", "plain_reach", "plain_full"])
@pytest.mark.parametrize("where", ["listener_in_layer", "open"])
def test_tile_path_520(pvlib, oracle, form, where):
    L = L520_IN if where == "listener_in_layer" else L520
    w = ref_run(oracle, "520", N520, walls(N520), W520, L)
    opts = {"graph": dict(), "plain_reach": dict(use_graph=2), "plain_full": dict(use_graph=2, reach_bound=0)}[form]
    with solver(pvlib, N520, walls(N520), W520, **opts) as s:
        assert s.info.residentKernel == 0
        s.run(L)
        check(s, w, "520^2 %s %s" % (form, where), W520)


def test_reach_bound_on_off_identical(pvlib):
    outs = []
    for rb in (1, 0):
        with solver(pvlib, N520, None, (24, 24, 24, 24), use_graph=2, reach_bound=rb) as s:
            s.run(L520)
            outs.append((s.fields(), s.results()))
    for a, b in zip(outs[0][0], outs[1][0]):
        assert same_bits(a, b).all()
    assert same_bits(outs[0][1][0], outs[1][1][0]).all() and same_bits(outs[0][1][1], outs[1][1][1]).all()


def test_layer_in_front_of_rigid_edges(pvlib, oracle):
    n, w4, R4 = 254, (16, 24, 0, 32), (1.0, 1.0, 1.0, 1.0)
    L = cell_of(100, 120)
    w = ref_run(oracle, "rigid", n, walls(n), w4, L, R4=R4)
    with solver(pvlib, n, walls(n), w4, R4=R4) as s:
        s.run(L)
        check(s, w, "254^2 layer + rigid edges", w4)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. changing and removing the layer between runs
# ------------------------------------------------------------------------------------------------------------------------------
def test_change_and_remove_between_runs(pvlib, oracle):
    n = 127
    L1, L2 = cell_of(60, 40), cell_of(30, 90)
    first = ref_run(oracle, "chg", n, walls(n), (24, 24, 24, 24), L1)
    second = ref_run(oracle, "chg", n, walls(n), (8, 30, 0, 16), L2, prev=first["r"])
    with solver(pvlib, n, walls(n), (24, 24, 24, 24)) as s, solver(pvlib, n, walls(n), (0, 0, 0, 0)) as fresh:
        s.run(L1)
        check(s, first, "change: run 1", (24, 24, 24, 24))
        s.set_edge_layer((8, 30, 0, 16))  # the carry rule: cells without an onset keep run 1's records
        s.run(L2)
        check(s, second, "change: run 2", (8, 30, 0, 16))
        s.set_edge_layer((0, 0, 0, 0))
        assert s.info.residentKernel == fresh.info.residentKernel
        s.run(L1)
        fresh.run(L1)
        for a, b in zip(s.fields(), fresh.fields()):
            assert same_bits(a, b).all()
        rs, ds = s.results()
        rf, df = fresh.results()
        on = df < 1e30
        assert same_bits(ds, df).all() and same_bits(rs[on], rf[on]).all() and on.sum() > 1000


# ------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.set_edge_layer((4, 4, 4, 4))
        for bad in ((-1, 0, 0, 0), (65, 0, 0, 0), (31, 32, 0, 0)):
            with pytest.raises(pvlib.PlaneverbError):
                s.set_edge_layer(bad)
            assert list(s.edge_layer()) == [4, 4, 4, 4]
        with pytest.raises(ValueError):
            s.set_edge_layer((1, 2))
    with pvlib.Solver(open_size(N520), open_size(N520), 275, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="sparse-emitter"):
            s.set_edge_layer((8, 8, 8, 8))
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            s.set_edge_layer((8, 8, 8, 8))
    efree = pvlib.compute_efree(open_size(512), open_size(512), 275)
    rank = pvlib.SlabRank(open_size(512), open_size(512), 275, 0, 0, 2, efree)
    try:
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            rank.solver.set_edge_layer((8, 8, 8, 8))
    finally:
        rank.close()
    with pvlib.Solver(open_size(N520), open_size(N520), 275, steps_per_launch=12, tile_rows=36, edge_tiles=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="edge tiles"):
            s.set_edge_layer((8, 8, 8, 8))


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the live module and 6. bakes
# ------------------------------------------------------------------------------------------------------------------------------
D70 = np.float32(343.21) / np.float32(275) / np.float32(3.5)


def _batch_output(pvlib, w4, L, E):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        for b in walls(70):
            s.add_geometry(b)
        s.set_edge_layer(w4)
        s.run(L)
        return s.get_output(E).as_array()


def _settle(pvlib):
    n = pvlib.IterationCount()
    assert pvlib.WaitIterations(n + 4, 60000) >= n + 4


def test_live_module(pvlib):
    L, E = cell_of(35, 30), cell_of(25, 45)
    plain = _batch_output(pvlib, (0, 0, 0, 0), L, E)
    layered = _batch_output(pvlib, (24, 24, 24, 24), L, E)
    assert not same_bits(plain, layered).all()
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, pvlib.pv_AbsorbingBoundary, ".", 0, pvlib.pv_GPU))
    try:
        for b in walls(70):
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(L)
        eid = pvlib.Emit(E)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), plain).all()
        pvlib.SetEdgeLayer(24, 24, 24, 24)  # while running: applied at an iteration boundary
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), layered).all()
        pvlib.SetEdgeLayer(40, 40, 0, 0)  # refused (70 - 80 cells): nothing changes
        assert "interior" in pvlib.last_error()
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), layered).all()
        pvlib.SetEdgeLayer(0, 0, 0, 0)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), plain).all()
    finally:
        pvlib.Exit()


def test_bakes_carry_the_layer(pvlib):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 2, 2)
    with pvlib.Solver(25.0, 25.0, 275) as plain, pvlib.Solver(25.0, 25.0, 275) as zero, \
            pvlib.Solver(25.0, 25.0, 275) as layered:
        zero.set_edge_layer((0, 0, 0, 0))
        layered.set_edge_layer((24, 24, 24, 24))
        bp, bz, bl = (pvlib.Bake(s, *lattice) for s in (plain, zero, layered))
        try:
            assert bp.info()["materialHash"] == bz.info()["materialHash"]
            assert bl.info()["materialHash"] != bp.info()["materialHash"]
            with pytest.raises(pvlib.PlaneverbError, match="material"):
                bl.run([plain])
            bl.run([layered])
            assert bl.info()["probesBaked"] == 4
        finally:
            for b in (bp, bz, bl):
                b.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the physics bar on the device: the library's recorded responses against the open field (tests/test_host_layer.py)
# ------------------------------------------------------------------------------------------------------------------------------
def test_physics_bar_on_device(pvlib, oracle):
    from test_host_layer import BAR_DB, LC, N, PAD, cell as hcell, size_of
    from _layer_ref import unit_tables
    w = pvlib.EDGE_LAYER_DEFAULT_WIDTH
    big = oracle.OracleGrid(size_of(N + 2 * PAD), size_of(N + 2 * PAD), 275, with_history=False)
    Lb = hcell(LC + PAD, LC + PAD)
    _, truth, _ = layer_fdtd(big, Lb, unit_tables(big.gx, big.gy), win=(PAD, PAD, N + 1, N + 1))
    big.close()
    inner = np.s_[w:N - w, w:N - w]
    err = {}
    for w4 in ((0, 0, 0, 0), (w, w, w, w)):
        with pvlib.Solver(size_of(N), size_of(N), 275) as s:
            s.set_edge_layer(w4)
            s.run(hcell(LC, LC))
            err[w4[0]] = sum(((s.history_plane(t)[inner] - truth[0][t][inner].astype(np.float64)) ** 2).sum()
                             for t in range(s.T))
    db = 10 * np.log10(err[0] / err[w])
    assert db >= BAR_DB, "device: %.2f dB" % db
