"""CPU: the rectangular ring reference of tests/_rect_ref.py, which tests/test_gpu_non_square.py compares the library with.

The pinned oracle is no reference on a grid with gx != gy, so the non-square reference is a ring rectangle inside a
SQUARE oracle grid.  Pinned here, without a device:
  * two independent restatements agree on non-square grids: the ring rectangle (the oracle's C stencil on a square array) and
    tests/_layer_ref.layer_fdtd with unit tables (numpy, stride gy + 1), final fields and every recorded plane;
  * the ring interior's material is the library's host rasteriser's on every grid the GPU file uses;
  * the free-field energy of a non-square grid, restated from the cells the library reads, is the square grids' EFREE wherever
    the short side is >= 30 cells;
  * the scene is not symmetric under transposition, so the two orientations of a grid are two cases;
  * the library's cell lookup tells a 70 x 127 grid from a 127 x 70 one.
"""
import numpy as np
import pytest

from _layer_ref import courant_of, edge_layer_tables, layer_fdtd, unit_tables
from _rect_ref import RectRing, free_cells, free_energy, free_samples, listeners_rect, size_of, walls_rect
from conftest import bits, same_bits

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
EFREE = np.float32(0.0447895788)  # open square grids at 275 Hz (tests/test_gpu_analysis_edges.EFREE)
ABSORBING, UNEVEN = (0.0, 0.0, 0.0, 0.0), (0.9, 0.2, 0.6, 1.0)
# every grid of tests/test_gpu_non_square.py (GRIDS there; test_the_gpu_file_uses_these_grids pins the two lists together)
GPU_GRIDS = [(24, 50), (50, 24), (70, 127), (127, 70), (127, 191), (191, 127), (30, 150), (150, 30), (252, 280), (280, 252),
             (420, 200), (200, 420), (200, 440), (440, 200), (126, 150), (150, 126)]


def cell(cx, cy):
    return ((cx + 0.5) * float(DX), 0.0, (cy + 0.5) * float(DX))


def test_the_gpu_file_uses_these_grids():
    import test_gpu_non_square as gpu
    assert sorted(gpu.ALL_GRIDS) == sorted(GPU_GRIDS) and gpu.EFREE == EFREE


def two_walls(gx, gy):
    """two walls, one of them running into the ghost column"""
    return walls_rect(DX, gx, gy)[[0, 2]]


@pytest.mark.parametrize("R4", [ABSORBING, UNEVEN], ids=["absorbing", "uneven"])
@pytest.mark.parametrize("grid", [(70, 100), (100, 70), (40, 113)], ids=lambda g: "%dx%d" % g)
def test_ring_rectangle_equals_the_stride_gy_restatement(oracle, grid, R4):
    gx, gy = grid
    L = cell(*listeners_rect(gx, gy)[0])
    ring = RectRing(oracle, gx, gy, 275, two_walls(gx, gy), R4, EFREE)
    try:
        f = ring.fdtd(L).copy()
        hist = [h.copy() for h in ring.history()]
        duck = ring.duck()
        assert (duck.gx, duck.gy, duck.T) == (gx, gy, 435) and duck.material()[0].shape == (gx + 1, gy + 1)
        f2, hist2, _ = layer_fdtd(duck, L, unit_tables(gx, gy), R4=R4)
        for name, a, b in zip(("pr", "vx", "vy"), f, f2):
            assert same_bits(a, b).all(), "%s: %d cells differ" % (name, (~same_bits(a, b)).sum())
        assert hist[0].shape == (435, gx + 1, gy + 1)
        for name, a, b in zip(("pr", "vx", "vy"), hist, hist2):
            assert same_bits(a, b).all(), "recorded %s" % name
        nz = hist[0] != 0  # (same_bits: modulo the sign of zero -- a wall cell holds beta * negative = -0 in one, +0 in the other)
        assert np.array_equal(nz, hist2[0] != 0) and np.array_equal(bits(hist[0][nz]), bits(hist2[0][nz]))
        assert (f[0] != 0).sum() > gx * gy // 2
        # the restated history analysed through the square grid gives the ring's own records
        r, d = ring.analyze()
        r2, d2 = ring.analyze_history(hist2, L)
        assert same_bits(d, d2).all() and same_bits(r, r2).all()
        air = ring.material()[0][:gx, :gy] != 0
        assert (d[air] < 1e30).all() and not np.isnan(r[air]).any() and (d[~air] > 1e30).all()
    finally:
        ring.close()


def test_a_shorter_run_is_the_first_steps_of_the_whole_run(oracle):
    """steps=: what a solver created with num_steps computes -- the grid's own pulse table, cut"""
    gx, gy, L = 40, 70, cell(20, 26)
    whole = RectRing(oracle, gx, gy, 275, two_walls(gx, gy), UNEVEN, EFREE)
    short = RectRing(oracle, gx, gy, 275, two_walls(gx, gy), UNEVEN, EFREE, steps=160)
    try:
        whole.fdtd(L)
        f = short.fdtd(L)
        assert short.T == 160 and short.history()[0].shape[0] == 160
        for a, b in zip(whole.history(), short.history()):
            assert np.array_equal(bits(a[:160]), bits(b))
        f2, _, _ = layer_fdtd(short.duck(), L, unit_tables(gx, gy), R4=UNEVEN)
        assert same_bits(f, f2).all()
    finally:
        whole.close()
        short.close()


@pytest.mark.parametrize("grid", GPU_GRIDS, ids=lambda g: "%dx%d" % g)
def test_ring_material_is_the_host_rasterisers(pvlib, oracle, grid):
    gx, gy = grid
    boxes = walls_rect(DX, gx, gy)
    beta, R = pvlib.host_rasterize(size_of(gx, DX), size_of(gy, DX), 275, boxes)
    assert beta.shape == (gx + 1, gy + 1)
    ring = RectRing(oracle, gx, gy, 275, boxes, UNEVEN, EFREE)  # (asserts beta with the ghost lines, and R on wall cells)
    try:
        b, Rr = ring.material()
        assert np.array_equal(b, beta) and (b[gx, :] == 0).all() and (b[:, gy] == 0).all()
        wall = beta[:gx, :gy] == 0
        assert np.array_equal(bits(Rr[:gx, :gy][wall]), bits(R[:gx, :gy][wall]))
        # the four walls: on the x = 0 edge, in the ghost column, in the ghost row; four absorptions
        assert (beta[0, :gy] == 0).any() and (beta[:gx, gy - 1] == 0).any() and (beta[gx - 1, :gy] == 0).any()
        assert sorted(set(np.float32(R[:gx, :gy][wall]).tolist())) == sorted(np.float32([0.1, 0.3, 0.6, 0.8]).tolist())
        for cx, cy in listeners_rect(gx, gy):
            assert beta[cx, cy] == 1 and 0 <= cx < gx and 0 <= cy < gy
            ring.shifted(cell(cx, cy))
            assert ring.o.listener_cell(*cell(cx, cy)[::2]) == (cx, cy)
    finally:
        ring.close()


# the reference passes the centre cell in metres and truncates it again ((int)((n * dx) / dx), FreeGrid.cpp:84, FDTD.cpp:97-98), which
# in float32 gives n - 1 for some n (62 for 63, 125 for 126: the "centre-cell quirk" of tests/test_gpu_analysis_edges.py, which is
# why a 127^2 or a 504^2 grid does not have EFREE either).  The library does the same per axis, so a non-square grid can have the
# source moved along one axis only: values no square grid has.
MOVED = {(70, 127): (0, 1), (127, 70): (1, 0), (127, 191): (1, 0), (191, 127): (0, 1), (252, 280): (1, 0), (280, 252): (0, 1),
         (126, 150): (1, 0), (150, 126): (0, 1)}
E_MOVED = {(0, 1): np.float32(0.042323366), (1, 0): np.float32(0.02950587), (1, 1): np.float32(0.028847147)}


@pytest.mark.parametrize("grid", GPU_GRIDS + [(30, 31), (31, 30), (127, 127)], ids=lambda g: "%dx%d" % g)
def test_free_field_energy(oracle, grid):
    """the pulse moves one cell per step and the sum covers 18 samples, so no edge of a grid whose short side is >= 30 cells
    can reach the cell that is read: the value depends only on where the read cell lies relative to the source.  With the source
    on the centre cell that is the square grids' EFREE, bit for bit; with the source moved by the re-truncation it is one of
    three other values, the same on every such grid."""
    gx, gy = grid
    assert free_samples(1443) == 18
    src, (ex, ey), r = free_cells(gx, gy, DX)
    moved = (gx // 2 - src[0], gy // 2 - src[1])
    assert moved == MOVED.get(grid, (1, 1) if grid == (127, 127) else (0, 0)), (grid, src)
    assert (ex, ey) == (gx // 2 + 2, gy // 2) and r == np.float32(np.float32(2) * DX)
    e, n = free_energy(oracle, gx, gy, 275)
    assert n == 18 and np.isfinite(e) and e > 0
    if min(grid) >= 30:
        want = EFREE if moved == (0, 0) else E_MOVED[moved]
        assert bits(e) == bits(want), (grid, e, want)


def test_square_free_field_energy_is_the_oracles(oracle):
    """the restatement on square grids against pvo_free_energy itself: source on the centre cell (70, 254) and moved (127)"""
    for n, moved in ((70, False), (254, False), (127, True)):
        e, _ = free_energy(oracle, n, n, 275)
        assert bits(e) == bits(np.float32(oracle.free_energy(size_of(n, DX), size_of(n, DX), 275))), n
        assert (bits(e) == bits(EFREE)) == (not moved) and (bits(e) == bits(E_MOVED[(1, 1)])) == moved, n


@pytest.mark.parametrize("grid", [(70, 127), (24, 50)], ids=lambda g: "%dx%d" % g)
def test_the_scene_is_not_transposition_symmetric(oracle, grid):
    gx, gy = grid
    out = []
    for a, b in ((gx, gy), (gy, gx)):
        ring = RectRing(oracle, a, b, 275, walls_rect(DX, a, b), ABSORBING, EFREE)
        f = ring.fdtd(cell(*listeners_rect(a, b)[0])).copy()
        r, d = ring.analyze()
        out.append((f, r, d, ring.material()[0]))
        ring.close()
    (f1, r1, d1, m1), (f2, r2, d2, m2) = out
    assert f1[0].shape == f2[0].T.shape
    assert (m1 != m2.T).any(), "material"
    assert (~same_bits(f1[0], f2[0].T)).sum() > gx * gy // 4, "pressure"
    assert (~same_bits(f1[1], f2[2].T)).sum() > gx * gy // 4, "vx against the transposed vy"
    assert (~same_bits(d1, d2.T)).sum() > gx * gy // 8, "onsets"
    assert (~same_bits(r1[..., 0], r2[..., 0].transpose(1, 0))).sum() > gx * gy // 4, "occlusion"


@pytest.mark.parametrize("r0", [None, 1e-4], ids=["graded", "split"])
@pytest.mark.parametrize("grid", [(70, 127), (127, 70), (252, 280)], ids=lambda g: "%dx%d" % g)
def test_edge_layer_tables_of_a_non_square_grid(pvlib, oracle, grid, r0):
    """the library's tables (which the GPU file hands to the restated stencils) against the documented formula, per axis"""
    gx, gy = grid
    w4 = (24, 0, 7, 40)
    got = pvlib.edge_layer_tables(size_of(gx, DX), size_of(gy, DX), 275, w4, r0=r0)
    o = oracle.OracleGrid(25.0, 25.0, 275, with_history=False)
    want = edge_layer_tables(gx, gy, courant_of(o), w4) if r0 is None else edge_layer_tables(gx, gy, courant_of(o), w4, R0=r0)
    o.close()
    for k, v in want.items():
        assert got[k].shape == v.shape == ((gx + 1,) if k.endswith("x") else (gy + 1,)), k
        assert np.array_equal(bits(got[k]), bits(v)), k


def test_cell_lookup_tells_the_orientations_apart(pvlib):
    tall, wide = (size_of(70, DX), size_of(127, DX)), (size_of(127, DX), size_of(70, DX))
    for (sx, sy), (gx, gy) in ((tall, (70, 127)), (wide, (127, 70))):
        i = pvlib.host_grid_info(sx, sy, 275)
        assert (i.gx, i.gy) == (gx, gy)
        for c in ((100, 10), (10, 100), (gx - 1, gy - 1), (gx - 1, 0), (0, gy - 1), (gx, 3), (3, gy)):
            lc, rc = pvlib.host_cells(sx, sy, 275, *cell(*c)[::2])
            assert lc == c
            assert rc == (c if (c[0] < gx and c[1] < gy) else None), (gx, gy, c, rc)
    assert pvlib.host_cells(*tall, 275, *cell(100, 10)[::2])[1] is None
    assert pvlib.host_cells(*wide, 275, *cell(100, 10)[::2])[1] == (100, 10)
    assert pvlib.host_cells(*tall, 275, *cell(10, 100)[::2])[1] == (10, 100)
    assert pvlib.host_cells(*wide, 275, *cell(10, 100)[::2])[1] is None
