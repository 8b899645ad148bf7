"""GPU (-m gpu): grid edges of any absorption (PvAmdSetGridBoundary, PlaneverbInit's gridBoundaryType, PlaneverbSetGridBoundary).

The reference steps absorbing edges only, so the oracle is the ring grid of tests/_boundary_ref.py: the pinned oracle on a grid
two cells larger whose one-cell ring of walls has the edge absorptions (tests/test_host_boundary.py pins it to the plain grid for
R = 0).  Every case compares every cell: final fields (ghost row and column included), recorded planes, impulse responses next to
each edge, the onset map and all eight members, bit for bit modulo the sign of zero (compare_all_cells: late-onset cells too).
"""
import numpy as np
import pytest

from _boundary_ref import RingOracle, half_cell_box
from conftest import same_bits
from test_gpu_analysis_edges import DX, compare_all_cells, open_size
from test_gpu_parity import fuse_opts

pytestmark = pytest.mark.gpu

RIGID, MIXED = (1.0, 1.0, 1.0, 1.0), (0.0, 1.0, 0.5, 0.25)
R4S = [RIGID, MIXED]
R4_IDS = ["rigid", "mixed"]

_EFREE = {}
_RING = {}


def efree_of(oracle, size, res):
    if (size, res) not in _EFREE:
        _EFREE[(size, res)] = np.float32(oracle.free_energy(size, size, res))
    return _EFREE[(size, res)]


def cell_of(dx, cx, cy):
    return ((cx + 0.5) * float(dx), 0.0, (cy + 0.5) * float(dx))


def edge_cells(gx, gy):
    """cells next to each edge, a corner and the ghost row / column"""
    return [(0, gy // 2), (gx - 1, gy // 3), (gx // 2, 0), (gx // 3, gy - 1), (0, 0), (gx - 1, gy - 1), (gx, gy // 2),
            (gx // 2, gy)]


def walls(dx, n):
    """interior walls plus one wall on the x = 0 edge and one on the y = gy edge (half-cell edges: tests/_boundary_ref.py)"""
    return np.array([half_cell_box(dx, n // 3, n // 3 + 2, 3, n - 12, 0.3),
                     half_cell_box(dx, 5, n // 4, 2 * n // 3, 2 * n // 3 + 1, 0.9),
                     half_cell_box(dx, 0, 3, n // 2, n // 2 + 9, 0.6),
                     half_cell_box(dx, 2 * n // 3, 2 * n // 3 + 7, n - 3, n + 1, 0.1)], np.float32)


def ring_run(oracle, key, size, res, boxes, R4, listeners, hist_ts=(), ir=True, prev=None, efree=None):
    """the ring oracle's results after each run of `listeners` on one grid: dict(f, hist {t: pr}, ir {cell: [T, 3]}, r, d)"""
    k = (key, tuple(R4), tuple(map(tuple, listeners)), None if prev is None else id(prev))
    if k in _RING:
        return _RING[k]
    ring = RingOracle(oracle, size, res, boxes, R4, efree=efree_of(oracle, size, res) if efree is None else efree)
    out = []
    for L in listeners:
        f = ring.fdtd(L)
        pr, vx, vy = ring.history()
        w = dict(f=f.copy(), hist={t: pr[t].copy() for t in hist_ts})
        w["ir"] = {c: np.stack([pr[:, c[0], c[1]], vx[:, c[0], c[1]], vy[:, c[0], c[1]]], 1).copy()
                   for c in (edge_cells(ring.gx, ring.gy) if ir else [])}
        w["r"], w["d"] = ring.analyze(prev)
        prev = w["r"]
        out.append(w)
    ring.close()
    _RING[k] = out
    return out


def check(s, w, ctx, fields=True):
    if fields:
        for k, (got, want) in enumerate(zip(s.fields(), w["f"])):
            bad = ~same_bits(got, want)
            assert not bad.any(), "%s field %s: %d cells differ, first %s" % (ctx, "pr vx vy".split()[k], bad.sum(), np.argwhere(bad)[0])
    for t, plane in w["hist"].items():
        assert same_bits(s.history_plane(t), plane).all(), "%s recorded pr, step %d" % (ctx, t)
    for c, ir in w["ir"].items():
        assert same_bits(s.impulse_response(*c), ir).all(), "%s impulse response at %s" % (ctx, c)
    got, gd = s.results()
    compare_all_cells(got, gd, w["r"], w["d"], ctx, s.T, s.fs)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. 70^2 through the resident kernel
# ------------------------------------------------------------------------------------------------------------------------------
D70 = np.float32(343.21) / np.float32(275) / np.float32(3.5)
L70 = cell_of(D70, 10, 50)


def case70(oracle, R4):
    return ring_run(oracle, "70", 25.0, 275, walls(D70, 70), R4, [L70], hist_ts=(0, 50, 200, 434))[0]


@pytest.mark.parametrize("R4", R4S, ids=R4_IDS)
def test_resident_70(pvlib, oracle, R4):
    w = case70(oracle, R4)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        assert s.info.residentKernel == 1
        for b in walls(D70, 70):
            s.add_geometry(b)
        s.set_grid_boundary(R4)
        for rep in range(2):  # (the second run re-uses flags, planes and maps)
            s.run(L70)
            check(s, w, "70^2 resident %s run %d" % (R4, rep))
        assert np.float32(s.efree) == efree_of(oracle, 25.0, 275)  # the free field stays the open grid's


# ------------------------------------------------------------------------------------------------------------------------------
# 2. >= 520^2 through the merged tile kernel, edge tiles off / on, and the two-kernel launch
# ------------------------------------------------------------------------------------------------------------------------------
N520 = 520
S520 = open_size(N520)
L520 = cell_of(DX, 40, 470)
FORMS = {"merged": dict(), "edge_tiles_0": dict(steps_per_launch=12, tile_rows=36, edge_tiles=0),
         "edge_tiles_1": dict(steps_per_launch=12, tile_rows=36, edge_tiles=1), "two_kernel": dict(merged_launch=0)}


def case520(oracle, scene, R4):
    boxes = walls(DX, N520) if scene == "walled" else None
    return ring_run(oracle, "520" + scene, S520, 275, boxes, R4, [L520], ir=False)[0]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("R4", R4S, ids=R4_IDS)
@pytest.mark.parametrize("scene", ["walled", "open"])
def test_tile_kernels_520(pvlib, oracle, scene, R4, form):
    """edge tiles (class 2) hold the absorbing pattern only: along a non-absorbing side they must fall to the general arm"""
    w = case520(oracle, scene, R4)
    with pvlib.Solver(S520, S520, 275, **FORMS[form]) as s:
        assert s.info.residentKernel == 0
        if scene == "walled":
            for b in walls(DX, N520):
                s.add_geometry(b)
        s.set_grid_boundary(R4)
        s.run(L520)
        check(s, w, "520^2 %s %s %s" % (scene, form, R4))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. 254^2 in the forms of test_late_onset_launch_bound_254
# ------------------------------------------------------------------------------------------------------------------------------
S254 = open_size(254)
L254 = cell_of(DX, 20, 20)


@pytest.mark.parametrize("form", ["default", "resident", "graph", "fused"])
@pytest.mark.parametrize("R4", R4S, ids=R4_IDS)
def test_launch_bound_254(pvlib, request, oracle, R4, form):
    w = ring_run(oracle, "254", S254, 275, None, R4, [L254], hist_ts=(0, 100, 434))[0]
    opts = {"default": {}, "resident": dict(resident_kernel=1, steps_per_launch=12, tile_rows=12),
            "graph": dict(resident_kernel=2), "fused": dict(fused_analysis=1)}[form]
    lib = request.getfixturevalue("pvlib_exp") if form == "fused" else pvlib
    with lib.Solver(S254, S254, 275, **opts) as s:
        if form == "resident":
            assert s.info.residentKernel == 1
        if form == "graph":
            assert s.info.residentKernel == 0
        s.set_grid_boundary(R4)
        s.run(L254)
        check(s, w, "254^2 %s %s" % (form, R4))


# ------------------------------------------------------------------------------------------------------------------------------
# 4. sparse-emitter mode, 520^2
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R4", R4S, ids=R4_IDS)
def test_sparse_emitter_mode_520(pvlib, oracle, R4, fuse):
    w = case520(oracle, "open", R4)
    r, d = w["r"], w["d"]
    on = d < 1e30
    cells = [(40, 460), (10, 10)]  # the listener's neighbourhood, and a reached cell next to each side the wave reaches
    for line in (np.s_[0, :], np.s_[N520 - 1, :], np.s_[:, 0], np.s_[:, N520 - 1]):
        idx = np.argwhere(on[line]).ravel()
        if idx.size:
            k = int(idx[idx.size // 2])
            cells.append((0 if line[0] == 0 else N520 - 1, k) if isinstance(line[0], int) else (k, 0 if line[1] == 0 else N520 - 1))
    cells = np.array(cells)
    assert len(cells) >= 4 and on[cells[:, 0], cells[:, 1]].sum() >= 3
    E = np.array([cell_of(DX, cx, cy) for cx, cy in cells], np.float32)
    with pvlib.Solver(S520, S520, 275, streaming_analysis=1, **fuse_opts(fuse)) as s:
        assert s.info.streamFuse == fuse
        s.set_grid_boundary(R4)
        s.set_emitters(E)
        s.run(L520)
        got, gd = s.results()
        em = np.zeros(gd.shape, bool)
        em[cells[:, 0], cells[:, 1]] = True
        want = r.copy()
        want[..., 1][~em] = 0
        want[..., 2][~em] = 0
        compare_all_cells(got, gd, want, d, "sparse-emitter fuse %d %s" % (fuse, R4))
        for i, e in enumerate(E):
            assert same_bits(s.get_output(e).as_array(), r[cells[i, 0], cells[i, 1]]).all(), "emitter %s" % cells[i]


# ------------------------------------------------------------------------------------------------------------------------------
# 5. slab groups on one device
# ------------------------------------------------------------------------------------------------------------------------------
S512 = open_size(512)


@pytest.mark.parametrize("R4", R4S, ids=R4_IDS)
@pytest.mark.parametrize("nslabs", [2, 3])
def test_slab_groups_512(pvlib, oracle, nslabs, R4):
    boxes = walls(DX, 512)
    with pvlib.Solver(S512, S512, 275, slabs=[0] * nslabs) as s:
        row0 = s.slab_info().row0[1]
        L = cell_of(DX, row0 - 2, 300)  # next to the first slab boundary
        w = ring_run(oracle, "512", S512, 275, boxes, R4, [L], ir=False)[0]
        for b in boxes:
            s.add_geometry(b)
        s.set_grid_boundary(R4)
        assert same_bits(s.grid_boundary(), np.float32(R4)).all()
        s.run(L)
        check(s, w, "%d slabs %s" % (nslabs, R4))


# ------------------------------------------------------------------------------------------------------------------------------
# 6. invariance, 7. a change between two runs, 8. refusals
# ------------------------------------------------------------------------------------------------------------------------------
def test_absorbing_is_untouched_and_round_trip(pvlib):
    L2 = cell_of(D70, 40, 20)
    with pvlib.Solver(25.0, 25.0, 275) as a, pvlib.Solver(25.0, 25.0, 275) as b, pvlib.Solver(25.0, 25.0, 275) as c:
        for s in (a, b, c):
            for bx in walls(D70, 70):
                s.add_geometry(bx)
        assert same_bits(a.grid_boundary(), np.zeros(4, np.float32)).all()
        b.set_grid_boundary((0, 0, 0, 0))
        a.run(L70)
        b.run(L70)
        for fa, fb in zip(a.fields(), b.fields()):
            assert same_bits(fa, fb).all()
        ra, da = a.results()
        rb, db = b.results()
        assert same_bits(ra, rb).all() and same_bits(da, db).all()
        # R = 1, then back to 0: the fields and every reached cell equal a fresh absorbing run (unreached cells carry)
        c.set_grid_boundary(RIGID)
        c.run(L70)
        c.set_grid_boundary((0, 0, 0, 0))
        c.run(L2)
        a.run(L2)
        for fa, fc in zip(a.fields(), c.fields()):
            assert same_bits(fa, fc).all()
        ra, da = a.results()
        rc, dc = c.results()
        on = da < 1e30
        assert same_bits(da, dc).all() and same_bits(ra[on], rc[on]).all() and on.sum() > 1000
        v = np.array([0.1, -0.5, 2.0, 1.0], np.float32)
        c.set_grid_boundary(v)
        assert same_bits(c.grid_boundary(), v).all()


def test_change_between_runs_follows_the_carry_rule(pvlib, oracle):
    """run 1 absorbing; run 2 with mixed edges, another listener and a new block of wall cells, which have no onset and so keep
    run 1's records (the carry rule, checked with the ring oracle's analyze(prev=...))"""
    L2 = cell_of(D70, 60, 12)
    block = half_cell_box(D70, 50, 56, 50, 56, 0.5)
    boxes2 = np.concatenate([walls(D70, 70), np.array([block], np.float32)])
    first = case70(oracle, (0.0, 0.0, 0.0, 0.0))
    second = ring_run(oracle, "70block", 25.0, 275, boxes2, MIXED, [L2], ir=False, prev=first["r"])[0]
    fresh = ring_run(oracle, "70block", 25.0, 275, boxes2, MIXED, [L2], ir=False)[0]
    assert (~same_bits(second["r"], fresh["r"])).any(), "no carried cell: the case shows nothing"
    for opts in (dict(), dict(resident_kernel=2)):
        with pvlib.Solver(25.0, 25.0, 275, **opts) as s:
            for b in walls(D70, 70):
                s.add_geometry(b)
            s.run(L70)
            check(s, first, "carry %s run 1" % opts)
            s.set_grid_boundary(MIXED)
            s.add_geometry(block)
            s.run(L2)
            check(s, second, "carry %s run 2" % opts)


def test_refusals(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.set_grid_boundary(MIXED)
        for bad in (np.nan, np.inf, -np.inf):
            with pytest.raises(pvlib.PlaneverbError, match="finite"):
                s.set_grid_boundary((0.0, 0.0, bad, 0.0))
            assert same_bits(s.grid_boundary(), np.float32(MIXED)).all()
        with pytest.raises(ValueError):
            s.set_grid_boundary((1.0, 1.0))
    efree = pvlib.compute_efree(S512, S512, 275)
    rank = pvlib.SlabRank(S512, S512, 275, 0, 0, 2, efree)
    try:
        with pytest.raises(pvlib.PlaneverbError, match="slab rank"):
            rank.solver.set_grid_boundary((0.0, 1.0, 0.0, 0.0))
        rank.solver.set_grid_boundary((0.0, 0.0, 0.0, 0.0))
        assert same_bits(rank.solver.grid_boundary(), np.zeros(4, np.float32)).all()
    finally:
        rank.close()


# ------------------------------------------------------------------------------------------------------------------------------
# 9. the live module
# ------------------------------------------------------------------------------------------------------------------------------
def _batch_output(pvlib, R4, L, E):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        for b in walls(D70, 70):
            s.add_geometry(b)
        s.set_grid_boundary(R4)
        s.run(L)
        return s.get_output(E).as_array()


def _settle(pvlib):
    n = pvlib.IterationCount()
    assert pvlib.WaitIterations(n + 4, 60000) >= n + 4


def test_live_module(pvlib):
    E = cell_of(D70, 20, 40)
    rigid = _batch_output(pvlib, RIGID, L70, E)
    absorbing = _batch_output(pvlib, (0, 0, 0, 0), L70, E)
    mixed = _batch_output(pvlib, MIXED, L70, E)
    assert not same_bits(rigid, absorbing).all() and not same_bits(mixed, absorbing).all()
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, pvlib.pv_ReflectingBoundary, ".", 0, pvlib.pv_GPU))
    try:
        for b in walls(D70, 70):
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(L70)
        eid = pvlib.Emit(E)
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), rigid).all()
        pvlib.SetGridBoundary(*MIXED)  # while running: applied at an iteration boundary
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), mixed).all()
        pvlib.SetGridBoundary(0.0, np.nan, 0.0, 0.0)  # refused: nothing changes
        _settle(pvlib)
        assert same_bits(pvlib.GetOutput(eid).as_array(), mixed).all()
    finally:
        pvlib.Exit()
    for bt in (pvlib.pv_AbsorbingBoundary, 7):  # any other value: absorbing, as before (with a warning)
        pvlib.Init(pvlib.Config((25.0, 25.0), 275, bt, ".", 0, pvlib.pv_GPU))
        try:
            for b in walls(D70, 70):
                pvlib.AddGeometry(b)
            pvlib.SetListenerPosition(L70)
            eid = pvlib.Emit(E)
            _settle(pvlib)
            assert same_bits(pvlib.GetOutput(eid).as_array(), absorbing).all(), bt
        finally:
            pvlib.Exit()


# ------------------------------------------------------------------------------------------------------------------------------
# 10. bakes
# ------------------------------------------------------------------------------------------------------------------------------
def test_bakes_carry_the_boundary(pvlib):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 2, 2)
    with pvlib.Solver(25.0, 25.0, 275) as plain, pvlib.Solver(25.0, 25.0, 275) as zero, \
            pvlib.Solver(25.0, 25.0, 275) as rigid:
        zero.set_grid_boundary((0.0, 0.0, 0.0, 0.0))
        rigid.set_grid_boundary(RIGID)
        bp, bz, br = (pvlib.Bake(s, *lattice) for s in (plain, zero, rigid))
        try:
            assert bp.info()["materialHash"] == bz.info()["materialHash"]
            assert br.info()["materialHash"] != bp.info()["materialHash"]
            with pytest.raises(pvlib.PlaneverbError, match="material"):
                br.run([plain])
            with pytest.raises(pvlib.PlaneverbError, match="material"):
                bp.run([rigid])
            br.run([rigid])
            bp.run([plain])
            with pytest.raises(pvlib.PlaneverbError):
                br.merge(bp)
            assert br.info()["probesBaked"] == 4
        finally:
            for b in (bp, bz, br):
                b.close()
