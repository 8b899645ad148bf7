"""GPU (-m gpu): split-field edge layers (PvAmdSetEdgeLayerSplit, PlaneverbSetEdgeLayerSplit).

The oracle is tests/_split_layer_ref.py: the numpy float32 restatement of the split stencil with the library's own tables
(PvAmdHostEdgeLayerTablesR0, pinned to the documented formula and, at width 0, to the pinned oracle by
tests/test_host_split_layer.py), analysed by the pinned oracle's unchanged analysis.  Every case compares every cell as
tests/test_gpu_layer.py does (check): final fields with the ghost row and column, recorded planes, impulse responses inside,
on and next to the layers, the onset map and all eight members, bit for bit modulo the sign of zero.
"""
import math

import numpy as np
import pytest

from _split_layer_ref import analyze, split_fdtd
from conftest import same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import L520, L520_IN, N520, W520, cell_of, check, efree_of, probe_cells, walls

pytestmark = pytest.mark.gpu

R0 = 1e-4  # (api.EDGE_LAYER_SPLIT_R0, checked below)
_REF = {}


def ref_run(oracle, key, n, boxes, w4, L, R4=None, hist_ts=(0, 100, 434), prev=None, r0=R0):
    """the restatement's results of one run: dict(f, hist {t: pr}, ir {cell: [T, 3]}, r, d)"""
    from planeverb_amd import api
    k = (key, n, tuple(w4), tuple(L), None if R4 is None else tuple(R4), r0,
         None if prev is None else prev.tobytes()[:64] + bytes([len(prev)]))
    if k in _REF:
        return _REF[k]
    size = open_size(n)
    o = oracle.OracleGrid(size, size, 275, boxes)
    assert o.gx == n
    tabs = api.edge_layer_tables(size, size, 275, w4, r0=r0)
    f, hist, resp, _ = split_fdtd(o, L, tabs, R4=R4, cells=probe_cells(n, w4))
    w = dict(f=f, hist={t: hist[0][t].copy() for t in hist_ts}, ir=resp)
    w["r"], w["d"] = analyze(o, hist, efree_of(oracle, size), L, prev=prev)
    o.close()
    _REF[k] = w
    return w


def solver(pvlib, n, boxes, w4, R4=None, r0=R0, **opts):
    s = pvlib.Solver(open_size(n), open_size(n), 275, **opts)
    for b in (boxes if boxes is not None else []):
        s.add_geometry(b)
    if R4 is not None:
        s.set_grid_boundary(R4)
    s.set_edge_layer_split(w4, r0)
    return s


def same_run(a, b, ctx):
    """two solvers' last runs: fields, onsets and the records of every cell with an onset, bit for bit"""
    for k, (x, y) in enumerate(zip(a.fields(), b.fields())):
        assert same_bits(x, y).all(), "%s field %d" % (ctx, k)
    ra, da = a.results()
    rb, db = b.results()
    on = db < 1e30
    assert same_bits(da, db).all() and same_bits(ra[on], rb[on]).all() and on.sum() > 1000, ctx


# ------------------------------------------------------------------------------------------------------------------------------
# 1. the reference's preset grids: the resident / small-grid kernel resolves off
# ------------------------------------------------------------------------------------------------------------------------------
PRESETS = [(70, (24, 24, 24, 24)), (127, (24, 0, 7, 40)), (254, (24, 24, 24, 24))]


@pytest.mark.parametrize("n,w4", PRESETS, ids=[str(p[0]) for p in PRESETS])
def test_presets(pvlib, oracle, n, w4):
    assert pvlib.EDGE_LAYER_SPLIT_R0 == R0
    L = cell_of(n // 2, n // 3 + 6)
    w = ref_run(oracle, "preset", n, walls(n), w4, L)
    with solver(pvlib, n, walls(n), w4) as s:
        assert s.info.residentKernel == 0
        assert list(s.edge_layer()) == list(w4) and s.edge_layer_model() == ("split", R0)
        for rep in range(2):
            s.run(L)
            check(s, w, "split %d^2 run %d" % (n, rep), w4)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. 520^2 on the tile path: graph replay and plain launches, reach bound on and off; the listener inside a layer and in the open
# ------------------------------------------------------------------------------------------------------------------------------
FORMS = {"graph": dict(), "plain_reach": dict(use_graph=2), "plain_full": dict(use_graph=2, reach_bound=0)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("where", ["listener_in_layer", "open"])
def test_tile_path_520(pvlib, oracle, form, where):
    L = L520_IN if where == "listener_in_layer" else L520
    w = ref_run(oracle, "520", N520, walls(N520), W520, L)
    with solver(pvlib, N520, walls(N520), W520, **FORMS[form]) as s:
        assert s.info.residentKernel == 0
        s.run(L)
        check(s, w, "split 520^2 %s %s" % (form, where), W520)


def test_layer_in_front_of_rigid_edges(pvlib, oracle):
    n, w4, R4 = 254, (16, 24, 0, 32), (1.0, 1.0, 1.0, 1.0)
    L = cell_of(100, 120)
    w = ref_run(oracle, "rigid", n, walls(n), w4, L, R4=R4)
    with solver(pvlib, n, walls(n), w4, R4=R4) as s:
        s.run(L)
        check(s, w, "split 254^2 layer + rigid edges", w4)


def test_other_r0(pvlib, oracle):
    n, w4, r0 = 127, (12, 20, 8, 16), 1e-2
    L = cell_of(40, 70)
    w = ref_run(oracle, "r0", n, walls(n), w4, L, r0=r0)
    with solver(pvlib, n, walls(n), w4, r0=r0) as s:
        assert s.edge_layer_model() == ("split", r0)
        s.run(L)
        check(s, w, "split 127^2 r0 1e-2", w4)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. no stale x part: consecutive runs, model changes, set_fields + run_steps
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,opts", [(127, dict()), (N520, dict(use_graph=2))], ids=["127_graph", "520_plain_reach"])
def test_consecutive_runs_match_fresh_solvers(pvlib, n, opts):
    w4 = (24, 24, 24, 24)
    L1, L2 = cell_of(12, n // 2), cell_of(n // 2, n - 30)  # (the first inside the x = 0 layer)
    with solver(pvlib, n, walls(n), w4, **opts) as s:
        for L in (L1, L2, L1):
            s.run(L)
            with solver(pvlib, n, walls(n), w4, **opts) as fresh:
                fresh.run(L)
                same_run(s, fresh, "split %d^2 consecutive run at %s" % (n, L))


def test_model_changes_match_fresh_solvers(pvlib):
    n, w4 = 127, (24, 0, 7, 40)
    L = cell_of(60, 50)
    steps = [("none", (0, 0, 0, 0)), ("split", w4), ("unsplit", w4), ("split", w4), ("split", (8, 8, 30, 0))]

    def apply(s, model, widths):
        if model == "unsplit":
            s.set_edge_layer(widths)
        elif model == "split":
            s.set_edge_layer_split(widths)
        else:
            s.set_edge_layer(widths)

    with pvlib.Solver(open_size(n), open_size(n), 275) as s:
        for b in walls(n):
            s.add_geometry(b)
        for model, widths in steps:
            apply(s, model, widths)
            assert s.edge_layer_model() == (("split", R0) if model == "split" else ("unsplit", 0.1))
            s.run(L)
            with pvlib.Solver(open_size(n), open_size(n), 275) as fresh:
                for b in walls(n):
                    fresh.add_geometry(b)
                apply(fresh, model, widths)
                assert fresh.info.residentKernel == s.info.residentKernel
                fresh.run(L)
                same_run(s, fresh, "model %s %s" % (model, widths))


def test_set_fields_and_run_steps(pvlib, oracle):
    from planeverb_amd import api
    n, w4 = 127, (24, 16, 8, 24)
    size = open_size(n)
    rng = np.random.default_rng(7)
    xx, yy = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    bump = np.exp(-(((xx - 20) ** 2 + (yy - 60) ** 2) / 200.0)).astype(np.float32)  # (reaching into the x = 0 layer)
    f0 = [bump, (0.1 * rng.standard_normal((n + 1, n + 1)) * bump).astype(np.float32),
          (0.1 * rng.standard_normal((n + 1, n + 1)) * bump).astype(np.float32)]
    for f in f0:  # (a state of the grid's cells: the ghost row and column hold zeros, as every run leaves them)
        f[n, :] = 0
        f[:, n] = 0
    o = oracle.OracleGrid(size, size, 275, walls(n))
    tabs = api.edge_layer_tables(size, size, 275, w4, r0=R0)
    want, _, _, _ = split_fdtd(o, cell_of(60, 60), tabs, steps=74, record=False, fields0=f0, with_pulse=False)
    o.close()
    with solver(pvlib, n, walls(n), w4) as s:
        s.run(cell_of(15, 60))  # (leaves a non-zero x part in the layers: set_fields must clear it)
        s.set_fields(*f0)
        s.run_steps(37)
        s.run_steps(37)  # (the x part carries over from the first call)
        for k, (got, ref) in enumerate(zip(s.fields(), want)):
            bad = ~same_bits(got, ref)
            assert not bad.any(), "run_steps field %d: %d cells differ, first %s" % (k, bad.sum(), np.argwhere(bad)[0])
        s.set_fields(*f0)
        s.run_steps(74)
        for got, ref in zip(s.fields(), want):
            assert same_bits(got, ref).all()


# ------------------------------------------------------------------------------------------------------------------------------
# 4. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.set_edge_layer_split((4, 4, 4, 4), 1e-3)
        for bad in ((-1, 0, 0, 0), (65, 0, 0, 0), (31, 32, 0, 0)):
            with pytest.raises(pvlib.PlaneverbError):
                s.set_edge_layer_split(bad)
            assert list(s.edge_layer()) == [4, 4, 4, 4] and s.edge_layer_model() == ("split", 1e-3)
        for r0 in (0.0, 1.0, -0.5, 2.0, math.nan, math.inf):
            with pytest.raises(pvlib.PlaneverbError, match="r0"):
                s.set_edge_layer_split((8, 8, 8, 8), r0)
            assert list(s.edge_layer()) == [4, 4, 4, 4] and s.edge_layer_model() == ("split", 1e-3)
        with pytest.raises(ValueError):
            s.set_edge_layer_split((1, 2))
        s.set_edge_layer((4, 4, 4, 4))
        assert s.edge_layer_model() == ("unsplit", 0.1)
    with pvlib.Solver(open_size(N520), open_size(N520), 275, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="sparse-emitter"):
            s.set_edge_layer_split((8, 8, 8, 8))
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            s.set_edge_layer_split((8, 8, 8, 8))
    efree = pvlib.compute_efree(open_size(512), open_size(512), 275)
    rank = pvlib.SlabRank(open_size(512), open_size(512), 275, 0, 0, 2, efree)
    try:
        with pytest.raises(pvlib.PlaneverbError, match="slab"):
            rank.solver.set_edge_layer_split((8, 8, 8, 8))
    finally:
        rank.close()
    with pvlib.Solver(open_size(N520), open_size(N520), 275, steps_per_launch=12, tile_rows=36, edge_tiles=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="edge tiles"):
            s.set_edge_layer_split((8, 8, 8, 8))


def test_batched_runs_refuse_a_split_layer(pvlib):
    with pvlib.Solver(open_size(N520), open_size(N520), 275) as a, pvlib.Solver(open_size(N520), open_size(N520), 275) as b:
        a.set_edge_layer_split((8, 8, 8, 8))
        with pytest.raises(pvlib.PlaneverbError, match="edge layers"):
            pvlib.run_batch([a, b], [L520, L520])


# ------------------------------------------------------------------------------------------------------------------------------
# 5. the live module and 6. bakes
# ------------------------------------------------------------------------------------------------------------------------------
def _batch_output(pvlib, model, w4, L, E):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        for b in walls(70):
            s.add_geometry(b)
        (s.set_edge_layer_split if model == "split" else s.set_edge_layer)(w4)
        s.run(L)
        return s.get_output(E).as_array()


def _settle(pvlib):
    n = pvlib.IterationCount()
    assert pvlib.WaitIterations(n + 4, 60000) >= n + 4


def test_live_module(pvlib):
    L, E = cell_of(35, 30), cell_of(25, 45)
    w4 = (24, 24, 24, 24)
    plain = _batch_output(pvlib, "unsplit", (0, 0, 0, 0), L, E)
    unsplit = _batch_output(pvlib, "unsplit", w4, L, E)
    split = _batch_output(pvlib, "split", w4, L, E)
    assert not same_bits(split, unsplit).all() and not same_bits(split, plain).all()
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, pvlib.pv_AbsorbingBoundary, ".", 0, pvlib.pv_GPU))
    try:
        for b in walls(70):
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(L)
        eid = pvlib.Emit(E)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), plain).all()
        pvlib.SetEdgeLayerSplit(*w4)  # while running: applied at an iteration boundary
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), split).all()
        pvlib.SetEdgeLayerSplit(40, 40, 0, 0)  # refused (70 - 80 cells): nothing changes
        assert "interior" in pvlib.last_error() and "Split" in pvlib.last_error()
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), split).all()
        pvlib.SetEdgeLayer(*w4)  # back to the unsplit model
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), unsplit).all()
        pvlib.SetEdgeLayerSplit(*w4)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), split).all()
        pvlib.SetEdgeLayer(0, 0, 0, 0)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), plain).all()
    finally:
        pvlib.Exit()


def test_bakes_carry_the_model(pvlib):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 2, 2)
    w4 = (24, 24, 24, 24)
    solvers = [pvlib.Solver(25.0, 25.0, 275) for _ in range(5)]
    free, unsplit, split, split2, split0 = solvers
    bakes = []
    try:
        unsplit.set_edge_layer(w4)
        split.set_edge_layer_split(w4)
        split2.set_edge_layer_split(w4, 1e-3)
        split0.set_edge_layer_split((0, 0, 0, 0))  # (no layer: the layer-free hash)
        bakes = [pvlib.Bake(s, *lattice) for s in solvers]
        h = [b.info()["materialHash"] for b in bakes]
        assert h[4] == h[0]
        assert len({h[0], h[1], h[2], h[3]}) == 4
        with pytest.raises(pvlib.PlaneverbError, match="material"):
            bakes[2].run([unsplit])
        bakes[2].run([split])
        assert bakes[2].info()["probesBaked"] == 4
    finally:
        for b in bakes:
            b.close()
        for s in solvers:
            s.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 7. the physics bar on the device: the library's recorded pressure against the open field (tests/test_host_split_layer.py)
# ------------------------------------------------------------------------------------------------------------------------------
def test_physics_bar_on_device(pvlib, oracle):
    from test_host_layer import LC, N, PAD, cell as hcell, size_of
    from test_host_split_layer import BAR_DB_24, BAR_OVER_UNSPLIT_DB
    from _layer_ref import layer_fdtd, unit_tables
    w = pvlib.EDGE_LAYER_DEFAULT_WIDTH
    big = oracle.OracleGrid(size_of(N + 2 * PAD), size_of(N + 2 * PAD), 275, with_history=False)
    Lb = hcell(LC + PAD, LC + PAD)
    _, truth, _ = layer_fdtd(big, Lb, unit_tables(big.gx, big.gy), win=(PAD, PAD, N + 1, N + 1))
    big.close()
    inner = np.s_[w:N - w, w:N - w]
    err = {}
    for model, w4 in (("plain", (0, 0, 0, 0)), ("unsplit", (w,) * 4), ("split", (w,) * 4)):
        with pvlib.Solver(size_of(N), size_of(N), 275) as s:
            (s.set_edge_layer_split if model == "split" else s.set_edge_layer)(w4)
            s.run(hcell(LC, LC))
            err[model] = sum(((s.history_plane(t)[inner] - truth[0][t][inner].astype(np.float64)) ** 2).sum()
                             for t in range(s.T))
    db = 10 * np.log10(err["plain"] / err["split"])
    assert db >= BAR_DB_24, "device: %.2f dB" % db
    assert 10 * np.log10(err["unsplit"] / err["split"]) >= BAR_OVER_UNSPLIT_DB
