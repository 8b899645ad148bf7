"""GPU (-m gpu): discs, capsules, wall paths and simple polygons in the shape layer (include/planeverb_amd.h, "Round and
concave shapes"), tolerance zero throughout.

* Material: PvAmdCopyMaterial after add / update / remove equals the numpy restatement (_round_shapes_ref.py) composed over the
  AABB layer and over convex shapes: the sequence rule, removal, kind changes, shapes across many 64-cell bins.
* Runs: the composed material goes into the oracle's b / R planes (as test_gpu_shapes.py) and every member of every cell and
  the onset map are compared: a disc pillar, an L-shaped room and a bent wall path with a door gap, at 96^2 (resident kernel)
  and 520^2 (tile path: graph and plain launches, reach bound on and off).
* A concave polygon against its convex decomposition, the live module, a split-field layer in front of rigid edges, slabs.
"""
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from _round_shapes_ref import (CAPSULE, CONVEX, DISC, POLYGON, WALL_PATH, centres, compose, coverage, random_path,
                               random_simple_polygon)
from _shapes_ref import obb_vertices, random_convex
from _split_layer_ref import analyze, split_fdtd
from test_gpu_analysis_edges import DX, EFREE, cell, compare_all_cells, open_size
from test_gpu_layer import check as layer_check, efree_of, probe_cells
from test_gpu_parity import random_scene
from test_gpu_shapes import Model, load_material, oracle_runs

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
F = np.float32


def add(s, shape, a):
    kind, pts, r = shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if kind == DISC:
        return s.add_disc(pts[0, 0], pts[0, 1], r, a)
    if kind == CAPSULE:
        return s.add_capsule(pts[0], pts[1], r, a)
    if kind == WALL_PATH:
        return s.add_wall_path(pts, r, a)
    if kind == POLYGON:
        return s.add_polygon(pts, a)
    return s.add_shape(pts, a)


def update(s, sid, shape, a):
    kind, pts, r = shape
    pts = np.asarray(pts, np.float32).reshape(-1, 2)
    if kind == DISC:
        s.update_disc(sid, pts[0, 0], pts[0, 1], r, a)
    elif kind == CAPSULE:
        s.update_capsule(sid, pts[0], pts[1], r, a)
    elif kind == WALL_PATH:
        s.update_wall_path(sid, pts, r, a)
    elif kind == POLYGON:
        s.update_polygon(sid, pts, a)
    else:
        s.update_shape(sid, pts, a)


def random_shape(rng, size, k):
    c = rng.uniform(-0.1 * size, 1.1 * size, 2)
    kind = k % 6
    if kind == 0:
        return (DISC, [c], rng.choice([rng.uniform(0.1, 0.5) * float(DX), rng.uniform(0.3, size / 6)]))
    if kind == 1:
        return (CAPSULE, [c, c + rng.uniform(-0.4, 0.4, 2) * size], rng.uniform(0.1, 1.0))
    if kind == 2:
        m = int(rng.choice([3, 6, 17, 40]))
        return (WALL_PATH, random_path(rng, size, m, size * 0.12), rng.uniform(0.15, 0.6))
    if kind == 3:
        return (POLYGON, random_simple_polygon(rng, c[0], c[1], rng.uniform(0.05, 0.35) * size, int(rng.choice([5, 8, 9, 30, 64]))), 0.0)
    if kind == 4:
        return (CONVEX, random_convex(rng, c[0], c[1], rng.uniform(0.5, size / 5), int(rng.integers(3, 9))), 0.0)
    ang = rng.uniform(0, 2 * np.pi)
    return (CONVEX, obb_vertices(c[0], c[1], rng.uniform(0.5, size / 2), rng.uniform(0.2, 1.5), np.cos(ang), np.sin(ang)), 0.0)


def absorption(rng):
    return float(rng.choice([0.969536, 0.5, 0.0, 0.999, rng.uniform(0.05, 0.95)]))


def check_material(s, base, model, ctx=""):
    want_b, want_R = compose(base[0], base[1], model.ordered(), s.gx, s.gy, s.dx)
    b, R = s.material()
    assert np.array_equal(b, want_b), "%s beta: %d cells differ, first %s" % (ctx, int((b != want_b).sum()), np.argwhere(b != want_b)[:3])
    assert np.array_equal(R.view(np.uint32), want_R.view(np.uint32)), "%s R differs" % ctx
    return want_b, want_R


# ------------------------------------------------------------------------------------------------------------------------------
# material
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,n_ops", [(275, 60), (1000, 60)])  # 70^2 (two bins a side) and 254^2
def test_material_through_random_add_update_remove(pvlib, res, n_ops):
    rng = np.random.default_rng(res)
    size = 25.0
    with pvlib.Solver(size, size, res) as s:
        s.load_scene(SMALLROOM)
        base = s.material()
        model = Model()
        for step in range(n_ops):
            op = rng.random()
            if op < 0.5 or not model.live:
                sh, a = random_shape(rng, size, step), absorption(rng)
                assert add(s, sh, a) == model.add(sh, a)
            elif op < 0.8:  # (an update may change the kind)
                sid = int(rng.choice(list(model.live)))
                sh, a = random_shape(rng, size, int(rng.integers(0, 6))), absorption(rng)
                update(s, sid, sh, a)
                model.update(sid, sh, a)
            else:
                sid = int(rng.choice(list(model.live)))
                s.remove_shape(sid)
                model.remove(sid)
            if step % 5 == 4:
                check_material(s, base, model, "step %d" % step)
            if step % 20 == 19:
                s.run((5.0, 0.0, 4.0))  # (so the changes reach the device in several batches; what the kernel wrote is checked by the oracle runs below)
        want_b, _ = check_material(s, base, model, "end")
        # the b / by of the impulse-response cells: the material during the run
        s.run((12.5, 0.0, 12.5))
        xs, ys = np.nonzero(want_b[:s.gx, :s.gy] != base[0][:s.gx, :s.gy])
        for cx, cy in list(zip(xs[:6], ys[:6])) + [(3, 3)]:
            cells = s.impulse_response_cells(int(cx), int(cy))
            assert (cells["b"] == want_b[cx, cy]).all() and (cells["by"][want_b[cx, cy] == 0] == 0).all(), (cx, cy)
        # refusals leave the table as it was
        for bad in (lambda: s.add_disc(5, 5, 0.0, 0.5), lambda: s.add_disc(5, float("nan"), 1.0, 0.5),
                    lambda: s.add_capsule((1, 1), (2, 2), -1.0, 0.5), lambda: s.add_wall_path([(1, 1)], 0.5, 0.5),
                    lambda: s.add_polygon([(0, 0), (2, 2), (2, 0), (0, 2)], 0.5), lambda: s.add_polygon([(0, 0), (1, 1), (2, 2)], 0.5),
                    lambda: s.add_polygon([(0, 0), (1, 0), (1, 1)], float("inf")), lambda: s.add_polygon([(0, 0), (1, 0), (1, 1)], float("nan")),
                    lambda: s.add_disc(5, 5, 1.0, float("nan")), lambda: s.add_disc(5, 5, 1.0, float("inf")),
                    lambda: s.add_capsule((1, 1), (4, 2), 0.5, float("nan")), lambda: s.add_capsule((1, 1), (4, 2), 0.5, float("-inf")),
                    lambda: s.add_wall_path([(1, 1), (4, 2), (5, 6)], 0.5, float("nan")),
                    lambda: s.add_wall_path([(1, 1), (4, 2), (5, 6)], 0.5, float("inf")),
                    lambda: s.update_disc(next(iter(model.live)), 5, 5, 1.0, float("nan")),
                    lambda: s.update_disc(next(iter(model.live)), 5, 5, 1.0, float("inf")),
                    lambda: s.update_capsule(next(iter(model.live)), (1, 1), (4, 2), 0.5, float("nan")),
                    lambda: s.update_capsule(next(iter(model.live)), (1, 1), (4, 2), 0.5, float("inf")),
                    lambda: s.update_wall_path(next(iter(model.live)), [(1, 1), (4, 2), (5, 6)], 0.5, float("nan")),
                    lambda: s.update_wall_path(next(iter(model.live)), [(1, 1), (4, 2), (5, 6)], 0.5, float("inf")),
                    lambda: s.update_polygon(next(iter(model.live)), [(0, 0), (1, 0), (1, 1)], float("nan")),
                    lambda: s.add_disc(5, 5, float("inf"), 0.5), lambda: s.add_wall_path([(1, 1), (float("inf"), 2)], 0.5, 0.5),
                    lambda: s.update_disc(next(iter(model.live)), 5, 5, -2.0, 0.5), lambda: s.update_polygon(999, [(0, 0), (1, 0), (1, 1)], 0.5)):
            with pytest.raises(pvlib.PlaneverbError):
                bad()
        check_material(s, base, model, "after refusals")
        assert add(s, (DISC, [(3.0, 3.0)], 0.6), 0.5) == model.add((DISC, [(3.0, 3.0)], 0.6), 0.5)  # (the id table too)
        check_material(s, base, model, "after refusals and one more shape")
        # removing everything brings back the AABB layer
        for sid in list(model.live):
            s.remove_shape(sid)
            model.remove(sid)
        b, R = s.material()
        assert np.array_equal(b, base[0]) and np.array_equal(R.view(np.uint32), base[1].view(np.uint32))


def test_sequence_rule_and_many_bins_520(pvlib, oracle):
    """a disc over a polygon over a convex box, in every order of updates; shapes that straddle the whole grid's bins"""
    size = open_size(520)
    rng = np.random.default_rng(520)
    with pvlib.Solver(size, size, 275) as s:
        boxes = random_scene(rng, size, 20)
        for bx in boxes:
            s.add_geometry(bx)
        base = s.material()
        model = Model()
        c = size / 2
        shapes = [((POLYGON, random_simple_polygon(rng, c, c, size * 0.45, 64), 0.0), 0.2),
                  ((DISC, [(c + 3.0, c)], size * 0.2), 0.5),
                  ((CONVEX, obb_vertices(c, c, size * 0.9, 4.0, 1.0, 0.7), 0.0), 0.7),
                  ((WALL_PATH, [(2.0, 2.0), (size - 2, 3.0), (size - 3, size - 2), (4.0, size - 4), (c, c)], 0.9), 0.9),
                  ((CAPSULE, [(-5.0, c / 2), (size + 5, c * 1.5)], 1.3), 0.35)]
        ids = []
        for sh, a in shapes:
            ids.append(add(s, sh, a))
            assert ids[-1] == model.add(sh, a)
        check_material(s, base, model, "added")
        for order in ([0, 1, 2, 3, 4], [4, 3, 2, 1, 0], [2, 0, 4, 1, 3]):
            for k in order:  # (an update with the same geometry moves the shape to the top)
                update(s, ids[k], *shapes[k])
                model.update(ids[k], *shapes[k])
            check_material(s, base, model, "order %s" % order)
        s.remove_shape(ids[1])
        model.remove(ids[1])
        mat = check_material(s, base, model, "disc removed")
        # what the kernel wrote (PvAmdCopyMaterial is the host mirror): a whole run on it against the oracle on the composed
        # material, from an air cell between the 64-vertex polygon's spikes and the wall path
        air = np.argwhere(mat[0][:s.gx, :s.gy] != 0)
        lx, ly = air[np.argmin(np.abs(air - [150, 200]).sum(1))]
        Lst = cell(int(lx), int(ly))
        (r, d), = oracle_runs(oracle, size, 275, boxes, [mat], [Lst], EFREE)
        s.run(Lst)
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "520^2 after the update orders", s.T, s.fs)


# ------------------------------------------------------------------------------------------------------------------------------
# whole runs against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def scenes(size):
    """(name, boxes or None, shapes [(shape, absorption)], listener, scale) in units of the grid size"""
    u = size / 25.0
    pillar = [((DISC, [(12.0 * u, 12.5 * u)], 1.6 * u), 0.8), ((DISC, [(9.0 * u, 15.0 * u)], 0.3 * float(DX)), 0.8)]
    # an L-shaped room: the walls are a concave ring (outer L minus nothing: the ring is drawn as a thick wall path around
    # the L outline, closed) plus a concave L-shaped block of furniture inside
    L_out = np.array([(5, 5), (20, 5), (20, 12), (12, 12), (12, 20), (5, 20)], np.float32) * F(u)
    l_room = [((WALL_PATH, np.vstack([L_out, L_out[:1]]), 0.35 * u), 0.9),
              ((POLYGON, np.array([(7, 7), (11, 7), (11, 8.5), (8.5, 8.5), (8.5, 11), (7, 11)], np.float32) * F(u), 0.0), 0.6)]
    # a bent wall with a door gap: two paths that leave 1.5 u open
    bent = [((WALL_PATH, np.array([(4, 14), (10, 14), (13, 11)], np.float32) * F(u), 0.3 * u), 0.85),
            ((WALL_PATH, np.array([(14.2, 9.8), (17, 7), (22, 7)], np.float32) * F(u), 0.3 * u), 0.85)]
    # point lists longer than 8, which the kernel reads from the pooled table (three of them, so two start at a non-zero
    # offset): a zigzag wall of 17 points, a 64-vertex gear and a 33-point arc around the listener that opens towards the gear
    zig = np.array([(4.0 + i, 18.0 + 0.8 * (i % 2)) for i in range(17)], np.float32) * F(u)
    ga = 2 * np.pi * np.arange(64) / 64
    gr = np.where(np.arange(64) % 2 == 0, 3.2, 2.0)
    gear = np.stack([14.0 + gr * np.cos(ga), 13.0 + gr * np.sin(ga)], 1).astype(np.float32) * F(u)
    aa = np.deg2rad(np.linspace(25.0, 335.0, 33))
    arc = np.stack([8.0 + 3.5 * np.cos(aa), 10.0 + 3.5 * np.sin(aa)], 1).astype(np.float32) * F(u)
    pooled = [((WALL_PATH, zig, 0.3 * u), 0.9), ((POLYGON, gear, 0.0), 0.6), ((WALL_PATH, arc, 0.25 * u), 0.8)]
    return [("disc pillar", pillar, (5.0 * u, 0.0, 12.5 * u)), ("L room", l_room, (9.5 * u, 0.0, 15.0 * u)),
            ("bent wall", bent, (8.0 * u, 0.0, 8.0 * u)), ("pooled point lists", pooled, (8.0 * u, 0.0, 10.0 * u))]


def run_scene(pvlib, oracle, size, res, boxes, shapes, L, ctx, efree=None, **opts):
    with pvlib.Solver(size, size, res, **opts) as s:
        for bx in (boxes if boxes is not None else []):
            s.add_geometry(bx)
        base = s.material()
        model = Model()
        for sh, a in shapes:
            assert add(s, sh, a) == model.add(sh, a)
        mat = check_material(s, base, model, ctx)
        assert (mat[0] != base[0]).sum() > 20, ctx
        (r, d), = oracle_runs(oracle, size, res, boxes, [mat], [L], efree)
        s.run(L)
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, ctx, s.T, s.fs)
        return s.info


@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["disc_pillar", "l_room", "bent_wall", "pooled_point_lists"])
def test_oracle_resident_96(pvlib, oracle, which):
    name, shapes, L = scenes(25.0)[which]
    info = run_scene(pvlib, oracle, 25.0, 375, pvlib.load_pv(SMALLROOM) if which == 0 else None, shapes, L, "96^2 " + name)
    assert info.residentKernel == 1


FORMS = {"graph": dict(), "plain_reach": dict(use_graph=2), "plain_full": dict(use_graph=2, reach_bound=0)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("which", [0, 1, 2, 3], ids=["disc_pillar", "l_room", "bent_wall", "pooled_point_lists"])
def test_oracle_tile_path_520(pvlib, oracle, which, form):
    size = open_size(520)
    name, shapes, L = scenes(size)[which]
    rng = np.random.default_rng(which)
    boxes = random_scene(rng, size, 12) if which == 0 else None
    info = run_scene(pvlib, oracle, size, 275, boxes, shapes, L, "520^2 %s %s" % (name, form), EFREE, **FORMS[form])
    assert info.residentKernel == 0


# ------------------------------------------------------------------------------------------------------------------------------
# a concave polygon and its convex decomposition
# ------------------------------------------------------------------------------------------------------------------------------
def test_concave_polygon_equals_its_convex_decomposition(pvlib):
    size, res = 25.0, 1000
    # a U-shaped footprint, slightly rotated so that no edge runs along a row of cell centres
    ang = 0.3113
    rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
    U = np.array([(0, 0), (12, 0), (12, 9), (9, 9), (9, 3), (3, 3), (3, 9), (0, 9)], np.float64)
    place = lambda p: (np.asarray(p, np.float64) @ rot.T + [7.953, 4.871]).astype(np.float32)
    concave = place(U)
    pieces = [place([U[0], U[1], U[5]]), place([U[1], U[4], U[5]]),   # the base, cut along the diagonal (3,3)-(12,0)
              place([U[1], U[2], U[3], U[4]]), place([U[0], U[5], U[6], U[7]])]
    with pvlib.Solver(size, size, res) as a, pvlib.Solver(size, size, res) as b:
        # the coordinates are chosen so that no cell centre lies exactly on an internal cut (nor on any other edge): assert it
        X, Y = centres(a.gx, a.gy, a.dx)
        for p in pieces:
            q = p.astype(np.float64)
            for i in range(len(q)):
                (ax, ay), (bx, by) = q[i], q[(i + 1) % len(q)]
                on = (bx - ax) * (Y.astype(np.float64) - ay) - (by - ay) * (X.astype(np.float64) - ax)
                assert (on != 0).all()
                # (nor within the float32 rounding of either rule, where the two could differ: 16 ulp of a coordinate below
                # 32 m, the bound pv_core.cpp's shapeCellBounds gives the edge function)
                assert np.abs(on).min() / np.hypot(bx - ax, by - ay) > 16 * 2.0 ** -19
        a.add_polygon(concave, 0.5)
        for p in pieces:
            b.add_shape(p, 0.5)
        (ba, Ra), (bb, Rb) = a.material(), b.material()
        assert np.array_equal(ba, bb) and np.array_equal(Ra.view(np.uint32), Rb.view(np.uint32))
        assert (ba[:a.gx, :a.gy] == 0).sum() > 3000


# ------------------------------------------------------------------------------------------------------------------------------
# a split-field layer in front of rigid grid edges, with a disc
# ------------------------------------------------------------------------------------------------------------------------------
def test_split_layer_and_rigid_edges_with_a_disc(pvlib, oracle):
    n, w4, R4, r0 = 254, (16, 24, 0, 32), (1.0, 1.0, 1.0, 1.0), 1e-4
    size = open_size(n)
    L = cell(100, 120)
    at = lambda cx, cy: np.array([[cell(cx, cy)[0], cell(cx, cy)[2]]], np.float32)
    discs = [((DISC, at(130, 118), 9.5 * float(DX)), 0.7),   # a pillar next to the listener
             ((DISC, at(8, 60), 6.0 * float(DX)), 0.4)]      # inside the x = 0 layer
    with pvlib.Solver(size, size, 275) as s:
        s.set_grid_boundary(R4)
        s.set_edge_layer_split(w4, r0)
        base = s.material()
        model = Model()
        for sh, a in discs:
            assert add(s, sh, a) == model.add(sh, a)
        mat = check_material(s, base, model, "split layer")
        o = oracle.OracleGrid(size, size, 275, None)
        load_material(o, *mat)
        tabs = pvlib.edge_layer_tables(size, size, 275, w4, r0=r0)
        f, hist, resp, _ = split_fdtd(o, L, tabs, R4=R4, cells=probe_cells(n, w4))
        w = dict(f=f, hist={t: hist[0][t].copy() for t in (0, 100, 434)}, ir=resp)
        w["r"], w["d"] = analyze(o, hist, efree_of(oracle, size), L)
        o.close()
        s.run(L)
        layer_check(s, w, "split layer + rigid edges + discs", w4)


# ------------------------------------------------------------------------------------------------------------------------------
# slabs
# ------------------------------------------------------------------------------------------------------------------------------
def test_slab_group_takes_round_shapes_and_matches_one_solver(pvlib):
    size = open_size(600)
    rng = np.random.default_rng(6)
    boxes = random_scene(rng, size, 20)
    c = size / 2
    L = [cell(300, 300), cell(60, 520)]
    res = []
    for slabs in (None, [0, 0]):
        with pvlib.Solver(size, size, 275, slabs=slabs) as s:
            for bx in boxes:
                s.add_geometry(bx)
            d = s.add_disc(c + 20.0, c, 14.0, 0.6)  # (across the slab boundary)
            p = s.add_wall_path([(10.0, 20.0), (c, 40.0), (size - 10, 30.0)], 0.8, 0.8)
            g = s.add_polygon(random_simple_polygon(np.random.default_rng(1), c, c * 1.5, 30.0, 40), 0.3)
            out = [s.material()]
            s.run(L[0])
            out.append(s.results())
            s.update_disc(d, c - 30.0, c + 10.0, 9.0, 0.6)
            s.remove_shape(p)
            s.run(L[1])
            out.append(s.results())
            res.append(out)
            assert g == 2
    (m1, a1, b1), (m2, a2, b2) = res
    assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])
    for (r1, d1), (r2, d2) in ((a1, a2), (b1, b2)):
        assert same_bits(d1, d2).all() and same_bits(r1, r2).all()


def test_slab_rank_refuses_round_shapes(pvlib):
    h = pvlib.lib().PvAmdCreateSlabRank(25.0, 25.0, 275, 0, 0, 2)
    assert h
    try:
        xy = np.array([1, 1, 5, 1, 5, 5, 3, 2, 1, 5], np.float32)
        for rc in (pvlib.lib().PvAmdAddDisc(h, 5, 5, 2, 0.5), pvlib.lib().PvAmdAddCapsule(h, 5, 5, 9, 9, 1, 0.5),
                   pvlib.lib().PvAmdAddWallPath(h, pvlib._f(xy), 5, 0.5, 0.5), pvlib.lib().PvAmdAddPolygon(h, pvlib._f(xy), 5, 0.5)):
            assert rc == -1 and "slab rank" in pvlib.last_error()
    finally:
        pvlib.lib().PvAmdDestroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# live module: a pillar is added, moved and removed between iterations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["1", "2"])
def test_live_disc_added_moved_removed(pvlib, monkeypatch, pipeline):
    monkeypatch.setenv("PLANEVERB_AMD_LIVE_PIPELINE", pipeline)
    boxes = pvlib.load_pv(SMALLROOM)
    Lst = (5.0, 0.0, 4.0)
    E = [(12.0, 0.0, 20.0), (20.0, 0.0, 5.0), (3.0, 0.0, 22.0)]
    # every state leaves every emitter reachable, so its records do not depend on the iterations before it
    states = [None, ("disc", 9.0, 8.0, 1.5), ("disc", 10.0, 9.0, 1.5), ("disc", 12.5, 9.5, 2.0), None,
              ("path", [(8.0, 14.0), (12.0, 10.0), (16.0, 10.0)], 0.4), ("poly", [(8, 7), (12, 7), (12, 8), (9, 8), (9, 11), (8, 11)])]
    remove = {"disc": pvlib.RemoveDiscGeometry, "path": pvlib.RemoveWallPathGeometry, "poly": pvlib.RemoveConcavePolygonGeometry}
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, 0, ".", 0, pvlib.pv_GPU))
    try:
        for b in boxes:
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(Lst)
        eids = [pvlib.Emit(e) for e in E]
        sid = kind = None
        for k, st in enumerate(states):
            if sid is not None and (st is None or st[0] != kind):
                remove[kind](sid)
                sid = kind = None
            if st is not None:
                if st[0] == "path":
                    sid = pvlib.AddWallPathGeometry(st[1], st[2], 0.7)
                elif st[0] == "poly":
                    sid = pvlib.AddConcavePolygonGeometry(st[1], 0.7)
                elif sid is None:
                    sid = pvlib.AddDiscGeometry(st[1], st[2], st[3], 0.7)
                else:
                    pvlib.UpdateDiscGeometry(sid, st[1], st[2], st[3], 0.7)
                kind = st[0]
                assert sid == 0
            target = pvlib.IterationCount() + 4
            assert pvlib.WaitIterations(target, 120000) >= target
            got = [pvlib.GetOutput(eid).as_array() for eid in eids]
            with pvlib.Solver(25.0, 25.0, 275) as fresh:  # a fresh solver with the same geometry
                for b in boxes:
                    fresh.add_geometry(b)
                if st is not None:
                    if st[0] == "path":
                        fresh.add_wall_path(st[1], st[2], 0.7)
                    elif st[0] == "poly":
                        fresh.add_polygon(st[1], 0.7)
                    else:
                        fresh.add_disc(st[1], st[2], st[3], 0.7)
                fresh.run(Lst)
                for g, e in zip(got, E):
                    want = fresh.get_output(e).as_array()
                    assert np.isfinite(want[0]) and want[0] >= 0, (k, e, want)
                    assert same_bits(g, want).all(), (pipeline, k, e, g, want)
        assert pvlib.IsRunning()
    finally:
        pvlib.Exit()
