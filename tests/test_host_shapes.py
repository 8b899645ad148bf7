"""CPU: the shape model of include/planeverb_amd.h -- oriented-box vertices, refusals, counter-clockwise ordering and the
cell-centre coverage rule -- against the numpy float32 restatement in _shapes_ref.py, bit for bit."""
import numpy as np
import pytest

from _shapes_ref import F, coverage, obb_vertices, random_convex


def test_oriented_box_vertices_match_numpy(pvlib):
    rng = np.random.default_rng(7)
    for k in range(600):
        px, py = rng.uniform(-5, 60, 2)
        w, h = rng.uniform(0.01, 30, 2)
        ang = rng.uniform(0, 2 * np.pi)
        scale = [1.0, 1e-3, 7.5, 1e4][k % 4]  # unit and non-unit axes
        ax, ay = scale * np.cos(ang), scale * np.sin(ang)
        if k % 50 == 0:
            ax, ay = (0.0, 3.0) if k % 100 else (-2.0, 0.0)  # axis-aligned
        got = pvlib.host_oriented_box_vertices(px, py, w, h, ax, ay)
        want = obb_vertices(px, py, w, h, ax, ay)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, got, want)
        # counter-clockwise, and the library keeps it as it is
        assert np.array_equal(pvlib.host_shape(got), got)


@pytest.mark.parametrize("args", [
    (1.0, 1.0, 2.0, 1.0, 0.0, 0.0),             # zero axis
    (1.0, 1.0, 2.0, 1.0, -0.0, 0.0),
    (float("nan"), 1.0, 2.0, 1.0, 1.0, 0.0),    # non-finite inputs
    (1.0, 1.0, float("inf"), 1.0, 1.0, 0.0),
    (1.0, 1.0, 2.0, 1.0, float("inf"), 0.0),
])
def test_oriented_box_refusals(pvlib, args):
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_oriented_box_vertices(*args)
    assert pvlib.last_error()


@pytest.mark.parametrize("name,xy,absorption", [
    ("two vertices", [(0, 0), (1, 0)], 0.5),
    ("nine vertices", [(np.cos(a), np.sin(a)) for a in np.linspace(0, 2 * np.pi, 9, endpoint=False)], 0.5),
    ("collinear", [(0, 0), (1, 1), (2, 2), (3, 3)], 0.5),
    ("repeated point", [(1, 1), (1, 1), (1, 1)], 0.5),
    ("non-convex", [(0, 0), (4, 0), (1, 1), (0, 4)], 0.5),
    ("bow tie", [(0, 0), (2, 2), (2, 0), (0, 2)], 0.5),
    ("pentagram", [(np.cos(a), np.sin(a)) for a in np.arange(5) * 4 * np.pi / 5], 0.5),
    ("nan coordinate", [(0, 0), (1, 0), (0, float("nan"))], 0.5),
    ("inf coordinate", [(0, 0), (float("inf"), 0), (0, 1)], 0.5),
    ("nan absorption", [(0, 0), (1, 0), (0, 1)], float("nan")),
    ("inf absorption", [(0, 0), (1, 0), (0, 1)], float("inf")),
])
def test_shape_refusals(pvlib, name, xy, absorption):
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_shape(xy, absorption)
    assert pvlib.last_error(), name
    # the refusal is the library's, not the binding's: the coverage helper refuses the same list
    if not np.isfinite(absorption):
        return
    a = np.ascontiguousarray(xy, np.float32).reshape(-1)
    cover = np.empty((71, 71), np.uint8)
    assert pvlib.lib().PvAmdHostShapeCoverage(F(25.0), F(25.0), 275, pvlib._f(a), a.size // 2,
                                              cover.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_ubyte))) == -1


def test_clockwise_list_is_reversed(pvlib):
    cw = np.array([(0, 0), (0, 3), (2, 4), (5, 1), (3, -1)], np.float32)
    got = pvlib.host_shape(cw)
    assert np.array_equal(got, cw[::-1])
    ccw = cw[::-1].copy()
    assert np.array_equal(pvlib.host_shape(ccw), ccw)
    # triangle, both orders: the same covered cells
    tri = np.array([(3.0, 3.0), (20.0, 5.0), (9.0, 21.0)], np.float32)
    a = pvlib.host_shape_coverage(25.0, 25.0, 275, tri)
    b = pvlib.host_shape_coverage(25.0, 25.0, 275, tri[::-1].copy())
    assert np.array_equal(a, b) and a.sum() > 100


def test_collinear_middle_vertex_is_accepted(pvlib):
    sq = [(0, 0), (1, 0), (2, 0), (2, 2), (0, 2)]
    assert pvlib.host_shape(sq).shape == (5, 2)


def test_coverage_matches_numpy(pvlib):
    """random oriented boxes, convex polygons, slivers and shapes partly or wholly outside the grid, on two grids"""
    rng = np.random.default_rng(11)
    for size, res in ((25.0, 275), (13.0, 700)):
        g = pvlib.host_grid_info(size, size, res)
        shapes = []
        for k in range(60):
            kind = k % 5
            c = rng.uniform(-0.2 * size, 1.2 * size, 2)
            if kind == 0:
                ang = rng.uniform(0, 2 * np.pi)
                shapes.append(obb_vertices(c[0], c[1], rng.uniform(0.1, size), rng.uniform(0.05, 3), np.cos(ang) * 3, np.sin(ang) * 3))
            elif kind == 1:
                shapes.append(random_convex(rng, c[0], c[1], rng.uniform(0.2, size / 2), int(rng.integers(3, 9))))
            elif kind == 2:  # sliver triangle
                d = rng.uniform(-1, 1, 2) * size
                shapes.append(np.array([c, c + d, c + d * 1.0001 + 0.01], np.float32))
            elif kind == 3:  # wholly outside
                shapes.append(obb_vertices(-3 * size, c[1], 2, 2, 1, 1))
            else:  # straddles the ghost row / column
                shapes.append(obb_vertices(size * 0.98, size * 0.98, 2, 2, 1, 0.3))
        n_cov = 0
        for xy in shapes:
            want = coverage(xy, g.gx, g.gy, g.dx)
            try:
                got = pvlib.host_shape_coverage(size, size, res, xy)
            except pvlib.PlaneverbError:  # (a sliver rounded to zero area)
                continue
            assert np.array_equal(got, want), (size, res, xy, int((got != want).sum()))
            assert not got[g.gx, :].any() and not got[:, g.gy].any()
            n_cov += int(got.sum())
        assert n_cov > 1000


def test_live_shape_calls_without_a_module(pvlib):
    """Part 1 extensions return the reference's sentinels when the module is not initialised"""
    assert pvlib.AddOrientedGeometry((1, 1, 2, 1, 1, 0, 0.5)) == -1
    assert pvlib.AddPolygonGeometry([(0, 0), (1, 0), (0, 1)], 0.5) == -1
    pvlib.UpdateOrientedGeometry(0, (1, 1, 2, 1, 1, 0, 0.5))
    pvlib.UpdatePolygonGeometry(0, [(0, 0), (1, 0), (0, 1)], 0.5)
    pvlib.RemoveOrientedGeometry(0)
    pvlib.RemovePolygonGeometry(0)
