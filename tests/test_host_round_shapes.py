"""CPU: discs, capsules, wall paths and simple polygons (include/planeverb_amd.h, "Round and concave shapes") -- the host
coverage function against the numpy float32 restatement in _round_shapes_ref.py, bit for bit (boolean maps, tolerance zero),
the refusals, and the live-module calls' allocation-failure sweep in the HIP-less build."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_analysis_edges import DX, open_size
from _round_shapes_ref import (CAPSULE, DISC, POLYGON, WALL_PATH, coverage, random_path, random_simple_polygon)

F = np.float32
GRIDS = (70, 254, 520)


def centre(i):
    return float((F(i) + F(0.5)) * F(DX))


def check(pvlib, n, shape):
    size = open_size(n)
    g = pvlib.host_grid_info(size, size, 275)
    assert (g.gx, g.gy) == (n, n)
    kind, pts, r = shape
    got = pvlib.host_coverage(size, size, 275, kind, pts, r)
    want = coverage(shape, g.gx, g.gy, g.dx)
    assert np.array_equal(got, want), (n, shape, int((got != want).sum()), np.argwhere(got != want)[:4])
    assert not got[g.gx, :].any() and not got[:, g.gy].any()
    return int(got.sum())


@pytest.mark.parametrize("n", GRIDS)
def test_disc_and_capsule_coverage_matches_numpy(pvlib, n):
    rng = np.random.default_rng(100 + n)
    size, dx = open_size(n), float(DX)
    covered = empty = 0
    for k in range(80):
        c = rng.uniform(-0.2 * size, 1.2 * size, 2)
        r = [rng.uniform(0.05, 0.5) * dx, rng.uniform(0.5, 3.0) * dx, rng.uniform(0.02, 0.3) * size][k % 3]
        if k % 8 == 7:  # wholly outside
            c = np.array([-3.0 * size, c[1]])
        if k % 8 == 5:  # the centre exactly on a cell centre
            c = np.array([centre(int(rng.integers(0, n))), centre(int(rng.integers(0, n)))])
        got = check(pvlib, n, (DISC, c, r))
        covered += got
        empty += got == 0
        d = rng.uniform(-0.4, 0.4, 2) * size * (0.05 if k % 2 else 1.0)
        b = c + d
        if k % 8 == 5:  # both end points exactly on cell centres
            b = np.array([centre(int(rng.integers(0, n))), centre(int(rng.integers(0, n)))])
        if k % 16 == 3:  # a == b: the disc's bits
            b = c
            assert np.array_equal(pvlib.host_coverage(size, size, 275, CAPSULE, [c, b], r),
                                  pvlib.host_coverage(size, size, 275, DISC, c, r))
        covered += check(pvlib, n, (CAPSULE, [c, b], r))
    assert covered > 500 and empty > 0  # (radii below half a cell: an empty coverage is valid)


@pytest.mark.parametrize("n", GRIDS)
def test_wall_path_coverage_matches_numpy_and_is_the_union_of_its_capsules(pvlib, n):
    rng = np.random.default_rng(200 + n)
    size, dx = open_size(n), float(DX)
    covered = 0
    for k in range(30):
        m = [2, 3, 5, 17, 40, 64][k % 6]
        pts = random_path(rng, size, m, size * (0.3 if m < 10 else 0.08))
        if k % 5 == 1:  # points exactly on cell centres, one of them repeated (a zero-length segment)
            idx = rng.integers(0, n, (m, 2))
            pts = np.array([[centre(i), centre(j)] for i, j in idx], np.float32)
            pts[m // 2] = pts[m // 2 - 1]
        if k % 5 == 3:  # runs out of the grid
            pts = pts + F(0.7 * size)
        r = [rng.uniform(0.1, 0.5), rng.uniform(0.5, 2.5)][k % 2] * dx
        covered += check(pvlib, n, (WALL_PATH, pts, r))
        got = pvlib.host_coverage(size, size, 275, WALL_PATH, pts, r)
        union = np.zeros_like(got)
        for i in range(m - 1):
            union |= pvlib.host_coverage(size, size, 275, CAPSULE, pts[i:i + 2], r)
        assert np.array_equal(got, union), (n, k)
    assert covered > 500


def l_room(x0, y0, s):
    return np.array([(x0, y0), (x0 + 2 * s, y0), (x0 + 2 * s, y0 + s), (x0 + s, y0 + s), (x0 + s, y0 + 2 * s), (x0, y0 + 2 * s)],
                    np.float32)


@pytest.mark.parametrize("n", GRIDS)
def test_polygon_coverage_matches_numpy(pvlib, n):
    rng = np.random.default_rng(300 + n)
    size = open_size(n)
    covered = 0
    for k in range(40):
        m = [3, 4, 6, 9, 20, 37, 64][k % 7]
        c = rng.uniform(-0.1 * size, 1.1 * size, 2)
        xy = random_simple_polygon(rng, c[0], c[1], rng.uniform(0.05, 0.6) * size, m)
        if k % 10 == 9:
            xy = xy - F(3 * size)  # wholly outside
        covered += check(pvlib, n, (POLYGON, xy, 0.0))
    # collinear runs, and vertices at the height of cell centres (and on cell centres)
    a, b, c3 = centre(n // 5), centre(n // 2), centre(4 * n // 5)
    mid = centre((n // 5 + n // 2) // 2)
    for xy in ([(a, a), (mid, a), (b, a), (c3, a), (c3, b), (b, b), (b, c3), (a, c3), (a, b)],   # an L with collinear runs
               l_room(a, a, b - a), l_room(a, a, b - a)[::-1],
               [(a, a), (c3, a), (c3, c3), (b, mid), (a, c3)],                                     # a notch whose tip is a cell centre
               [(a, b), (b, a), (c3, b), (b, c3)]):                                               # a diamond through cell centres
        covered += check(pvlib, n, (POLYGON, np.array(xy, np.float32), 0.0))
    assert covered > 2000


def test_either_winding_covers_the_same_cells(pvlib):
    rng = np.random.default_rng(5)
    size = open_size(254)
    xy = random_simple_polygon(rng, size / 2, size / 2, size / 3, 23)
    a = pvlib.host_coverage(size, size, 275, POLYGON, xy)
    b = pvlib.host_coverage(size, size, 275, POLYGON, xy[::-1].copy())
    assert np.array_equal(a, b) and a.sum() > 1000


NAN, INF = float("nan"), float("inf")
REFUSALS = [
    ("disc nan centre", DISC, [(NAN, 1)], 1.0),
    ("disc inf centre", DISC, [(1, INF)], 1.0),
    ("disc zero radius", DISC, [(1, 1)], 0.0),
    ("disc negative radius", DISC, [(1, 1)], -1.0),
    ("disc nan radius", DISC, [(1, 1)], NAN),
    ("disc inf radius", DISC, [(1, 1)], INF),
    ("capsule nan end", CAPSULE, [(1, 1), (NAN, 2)], 1.0),
    ("capsule zero radius", CAPSULE, [(1, 1), (3, 2)], 0.0),
    ("capsule inf radius", CAPSULE, [(1, 1), (3, 2)], INF),
    ("path of one point", WALL_PATH, [(1, 1)], 1.0),
    ("path of no point", WALL_PATH, np.zeros((0, 2)), 1.0),
    ("path of 65 points", WALL_PATH, [(0.1 * i, 1) for i in range(65)], 1.0),
    ("path nan point", WALL_PATH, [(1, 1), (2, 2), (NAN, 3)], 1.0),
    ("path negative radius", WALL_PATH, [(1, 1), (2, 2), (4, 3)], -0.5),
    ("polygon of two", POLYGON, [(0, 0), (1, 0)], 0.0),
    ("polygon of 65", POLYGON, [(np.cos(a), np.sin(a)) for a in np.linspace(0, 2 * np.pi, 65, endpoint=False)], 0.0),
    ("polygon zero area", POLYGON, [(0, 0), (1, 1), (2, 2), (3, 3)], 0.0),
    ("polygon repeated point", POLYGON, [(1, 1), (1, 1), (1, 1)], 0.0),
    ("polygon nan", POLYGON, [(0, 0), (1, 0), (0, NAN)], 0.0),
    ("polygon inf", POLYGON, [(0, 0), (INF, 0), (0, 1)], 0.0),
    ("bow tie", POLYGON, [(0, 0), (2, 2), (2, 0), (0, 2)], 0.0),
    ("pentagram", POLYGON, [(np.cos(a), np.sin(a)) for a in np.arange(5) * 4 * np.pi / 5], 0.0),
    ("touches itself at a vertex", POLYGON, [(0, 0), (4, 0), (4, 4), (2, 0), (0, 4)], 0.0),
    ("figure eight sharing a vertex", POLYGON, [(0, 0), (2, 2), (4, 0), (4, 4), (2, 2), (0, 4)], 0.0),
    ("spike folding back", POLYGON, [(0, 0), (4, 0), (4, 4), (4, 1), (0, 4)], 0.0),
    ("zero-length edge", POLYGON, [(0, 0), (4, 0), (4, 0), (4, 4), (0, 4)], 0.0),
]


@pytest.mark.parametrize("name,kind,pts,r", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals(pvlib, name, kind, pts, r):
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_coverage(25.0, 25.0, 275, kind, np.asarray(pts, np.float32), r)
    assert pvlib.last_error(), name


def test_accepted_edge_cases(pvlib):
    # concave, collinear runs, 64 vertices, a 64-point path, a tiny radius: all valid
    pvlib.host_coverage(25.0, 25.0, 275, POLYGON, [(0, 0), (4, 0), (1, 1), (0, 4)])
    pvlib.host_coverage(25.0, 25.0, 275, POLYGON, [(0, 0), (1, 0), (2, 0), (2, 2), (1, 2), (0, 2)])
    pvlib.host_coverage(25.0, 25.0, 275, POLYGON, [(5 + 4 * np.cos(a), 5 + 4 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 64, endpoint=False)])
    pvlib.host_coverage(25.0, 25.0, 275, WALL_PATH, [(0.3 * i, 2 + (i % 2)) for i in range(64)], 0.2)
    assert pvlib.host_coverage(25.0, 25.0, 275, DISC, [(5.0, 5.0)], 1e-3).sum() == 0
    assert pvlib.POLY_MAX_VERTS == 64


def test_live_round_shape_calls_without_a_module(pvlib):
    """Part 1 extensions return the reference's sentinels when the module is not initialised"""
    assert pvlib.AddDiscGeometry(5, 5, 1, 0.5) == -1
    assert pvlib.AddWallPathGeometry([(1, 1), (4, 1), (4, 5)], 0.3, 0.5) == -1
    assert pvlib.AddConcavePolygonGeometry(l_room(2, 2, 3), 0.5) == -1
    pvlib.UpdateDiscGeometry(0, 5, 5, 1, 0.5)
    pvlib.UpdateWallPathGeometry(0, [(1, 1), (4, 1)], 0.3, 0.5)
    pvlib.UpdateConcavePolygonGeometry(0, l_room(2, 2, 3), 0.5)
    pvlib.RemoveDiscGeometry(0)
    pvlib.RemoveWallPathGeometry(0)
    pvlib.RemoveConcavePolygonGeometry(0)


def test_live_round_shape_calls_under_allocation_failure(tmp_path):
    """tests/host/alloc_fault_round.cpp: every allocation of every new live-module call fails once, in the HIP-less build of
    the live module (the flags of tests/host/Makefile), under ASan + UBSan"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "alloc_fault_round")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-DPVA_HOST_TEST",
                           "-I", host, "-I", csrc, "-I", os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "alloc_fault_round.cpp"), os.path.join(csrc, "pv_core.cpp"),
                           os.path.join(csrc, "pv_context.cpp"), os.path.join(csrc, "pv_capi.cpp"), "-lpthread"])
    for pipeline in ("1", "2"):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", PLANEVERB_AMD_LIVE_PIPELINE=pipeline)
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
        assert "alloc_fault_round: 0 failure(s)" in r.stdout, r.stdout
