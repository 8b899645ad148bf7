"""CPU: triangle meshes (include/planeverb_amd.h, "Triangle meshes") -- the library's host restatement of slice and coverage
(PvAmdHostMeshSection, PvAmdHostMeshCoverage: the marks-and-scan form the kernels use) against the naive numpy float32
restatement in _mesh_ref.py, bit for bit (tolerance zero), and every refusal."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_analysis_edges import DX, open_size
from _mesh_ref import (SHELL, SOLID, box, comb, coverage, even_endpoints, rotated_box, rotation, section, snap, tetrahedron, torus,
                       uv_sphere)

F = np.float32
N = 70
SIZE = open_size(N)
dx = float(DX)


def generators(rng, size):
    """closed meshes that stick out of the grid on every side between them, some vertices snapped onto the slice plane (h = 0.4)
    and onto cell-centre lines"""
    h = 0.4
    c = size / 2
    out = [("box", box((3.0, -1.0, 4.0), (9.0, 2.0, 11.0))),
           ("box out left and bottom", box((-5.0, -1.0, -3.0), (6.0, 2.0, 5.0))),
           ("box out right and top", box((size - 4.0, -1.0, size - 6.0), (size + 9.0, 2.0, size + 3.0))),
           ("box over the whole grid", box((-2.0, -1.0, -2.0), (size + 2.0, 2.0, size + 2.0))),
           ("rotated box", rotated_box(rng, (c, 0.3, c), (5.0, 3.0, 2.0))),
           ("sphere", uv_sphere((c - 2.0, 0.1, c + 1.0), 6.0, 12, 16)),
           ("sphere out of the grid", uv_sphere((1.0, 0.0, size - 1.0), 5.0, 9, 11)),
           ("torus", torus((c, 0.5, c), 7.0, 2.5, 24, 12)),
           ("tilted torus", torus((c + 3.0, 0.0, c - 2.0), 6.0, 2.0, 20, 10, rotation(rng))),
           ("tetrahedron", tetrahedron((2.0, -1.0, 3.0), (14.0, -0.5, 5.0), (6.0, -0.8, 15.0), (8.0, 4.0, 8.0))),
           ("comb", comb(1.0, 5.0, 30, 0.55, 0.3, 8.0))]
    snapped = []
    for name, (v, t) in out[4:10]:
        snapped.append((name + ", snapped", (snap(v, dx, h, rng), t)))
    return h, out + snapped


@pytest.mark.parametrize("mode,radius", [(SOLID, 0.0), (SHELL, 0.3), (SHELL, 0.04)])
def test_host_coverage_and_section_match_numpy(pvlib, mode, radius):
    rng = np.random.default_rng(7)
    g = pvlib.host_grid_info(SIZE, SIZE, 275)
    assert (g.gx, g.gy) == (N, N)
    h, meshes = generators(rng, SIZE)
    covered = 0
    for name, (v, t) in meshes:
        for hh, m12 in ((h, None), (-0.2, None), (h, np.hstack([rotation(rng) * 0.8, [[1.5], [0.1], [-2.0]]]).astype(np.float32))):
            seg, valid = pvlib.host_mesh_section(v, t, hh, m12)
            wseg, wvalid = section(v, t, hh, m12)
            assert np.array_equal(valid, wvalid), name
            assert np.array_equal(seg.view(np.uint32), wseg.view(np.uint32)), name
            assert even_endpoints(seg, valid), name  # (closed meshes: the section is closed, bit for bit)
            got = pvlib.host_mesh_coverage(SIZE, SIZE, 275, v, t, hh, mode, radius, m12)
            want = coverage((v, t, mode, radius, m12), hh, g.gx, g.gy, g.dx)
            assert np.array_equal(got, want), (name, hh, int((got != want).sum()), np.argwhere(got != want)[:4])
            assert not got[g.gx, :].any() and not got[:, g.gy].any()
            covered += int(got.sum())
    assert covered > 500  # (something is covered; a radius of a tenth of a cell covers little)


def test_identity_transform_is_no_transform(pvlib):
    v, t = uv_sphere((12.0, 0.2, 11.0), 6.0, 10, 14)
    eye = np.eye(3, 4, dtype=np.float32)
    a, va = pvlib.host_mesh_section(v, t, 0.3, None)
    b, vb = pvlib.host_mesh_section(v, t, 0.3, eye)
    assert np.array_equal(va, vb) and np.array_equal(a, b)


def test_box_mesh_covers_what_the_polygon_rule_gives_its_rectangle(pvlib):
    rng = np.random.default_rng(3)
    for k in range(20):
        x0, z0 = rng.uniform(-3.0, SIZE - 2.0, 2)
        x1, z1 = x0 + rng.uniform(0.1, 12.0), z0 + rng.uniform(0.1, 12.0)
        if k % 4 == 0:  # edges exactly on cell-centre lines
            x0, z0 = [float((F(int(q / dx)) + F(0.5)) * F(DX)) for q in (abs(x0), abs(z0))]
        v, t = box((x0, -1.0, z0), (x1, 1.0, z1))
        got = pvlib.host_mesh_coverage(SIZE, SIZE, 275, v, t, 0.0, SOLID)
        rect = np.array([(x0, z0), (x1, z0), (x1, z1), (x0, z1)], np.float32)
        want = pvlib.host_coverage(SIZE, SIZE, 275, pvlib.SHAPE_POLYGON, rect)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:4])


def test_torus_section_is_an_annulus(pvlib):
    c = SIZE / 2
    v, t = torus((c, 0.0, c), 7.0, 2.0, 32, 12)
    got = pvlib.host_mesh_coverage(SIZE, SIZE, 275, v, t, 0.1, SOLID)
    xs, ys = np.nonzero(got)
    inside = got[xs.min():xs.max() + 1, ys.min():ys.max() + 1]
    ci = int(c / dx)
    assert got[ci, ci] == 0 and (inside == 0).sum() > 100       # the hole
    assert got[int((c + 7.0) / dx), ci] == 1 and got[ci, int((c - 7.0) / dx)] == 1
    # the hole is enclosed: a row through the centre goes covered, uncovered, covered
    row = got[:, ci]
    runs = np.flatnonzero(np.diff(np.concatenate([[0], row, [0]]).astype(np.int8)))
    assert len(runs) == 4


def test_refusals(pvlib):
    v, t = box((3.0, -1.0, 4.0), (9.0, 2.0, 11.0))
    nan, inf = float("nan"), float("inf")
    cov = lambda vv=v, tt=t, h=0.0, mode=SOLID, r=0.0, m=None: pvlib.host_mesh_coverage(SIZE, SIZE, 275, vv, tt, h, mode, r, m)
    assert cov().sum() > 0

    def bad_vertex(val):
        w = v.copy()
        w[3, 2] = val
        return w

    def bad_m(val):
        m = np.eye(3, 4, dtype=np.float32)
        m[1, 3] = val
        return m

    open_mesh = t[:-1]                       # one triangle missing: two... three edges belong to one triangle only
    fin = np.vstack([t, [[0, 1, 6]]])        # an extra triangle: edge (0, 1) is shared by three
    dup = t.copy()
    dup[0] = (0, 1, 1)
    oob = t.copy()
    oob[2, 1] = 8
    neg = t.copy()
    neg[2, 1] = -1
    cases = {
        "nan vertex": lambda: cov(vv=bad_vertex(nan)), "inf vertex": lambda: cov(vv=bad_vertex(inf)),
        "nan transform": lambda: cov(m=bad_m(nan)), "inf transform": lambda: cov(m=bad_m(-inf)),
        "nan h": lambda: cov(h=nan), "inf h": lambda: cov(h=inf),
        "shell r = 0": lambda: cov(mode=SHELL, r=0.0), "shell r < 0": lambda: cov(mode=SHELL, r=-1.0),
        "shell r nan": lambda: cov(mode=SHELL, r=nan), "shell r inf": lambda: cov(mode=SHELL, r=inf),
        "shell r*r = 0": lambda: cov(mode=SHELL, r=1e-30), "shell r*r = inf": lambda: cov(mode=SHELL, r=1e30),
        "index = nv": lambda: cov(tt=oob), "index < 0": lambda: cov(tt=neg),
        "no triangle": lambda: cov(tt=np.zeros((0, 3), np.int32)),
        "two equal indices": lambda: cov(tt=dup),
        "open mesh, solid": lambda: cov(tt=open_mesh), "edge shared by three, solid": lambda: cov(tt=fin),
        "unknown mode": lambda: cov(mode=2),
    }
    for name, f in cases.items():
        with pytest.raises(pvlib.PlaneverbError):
            f()
        assert pvlib.last_error(), name
    # the same open mesh is a valid shell
    got = cov(tt=open_mesh, mode=SHELL, r=0.3)
    want = coverage((v, open_mesh, SHELL, 0.3, None), 0.0, N, N, DX)
    assert np.array_equal(got, want) and got.sum() > 0
    # over the per-mesh limit (the count is checked before the arrays are read)
    big = np.zeros(((1 << 20) + 1, 3), np.int32)
    with pytest.raises(pvlib.PlaneverbError):
        cov(tt=big)
    assert "1 << 20" in pvlib.last_error()
    # the section restatement refuses what it cannot index
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_mesh_section(v, oob, 0.0)
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.host_mesh_section(bad_vertex(nan), t, 0.0)


def test_exports_are_declared_bound_and_guarded(pvlib):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the catch family"""
    names = ["PvAmdAddMesh", "PvAmdUpdateMesh", "PvAmdSetMeshTransform", "PvAmdRemoveMesh", "PvAmdSetSliceHeight",
             "PvAmdGetSliceHeight", "PvAmdMeshTriangles", "PvAmdCopyMeshSection", "PvAmdHostMeshSection", "PvAmdHostMeshCoverage"]
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    for n in names:
        assert hasattr(pvlib.lib(), n) and n in pvlib.SYMBOLS, n
        assert re.search(r"PVA_EXPORT\s+\w+\s+%s\s*\(" % n, hdr), n
        assert re.search(r"^\w+\s+%s\s*\([^;{}]*?\)\s*try\s*\{.*?\}\s*PV_API_CATCH\(" % n, src, re.M | re.S), n
