"""GPU (-m gpu): triangle meshes, sliced at the solver's height and rasterised on the device (include/planeverb_amd.h, "Triangle
meshes"), tolerance zero throughout.

* Material: PvAmdCopyMaterial equals the numpy restatement (_mesh_ref.py) composed over SmallRoomScene's AABBs and under shapes,
  for every generator, for a 10 000-triangle sphere (many blocks), a comb (hundreds of crossings in the same rows and words), one
  triangle across every row, and through a random sequence of add / update / transform / height change / remove with runs in
  between; 70^2 (three coverage words per column, the last one partial) and 254^2.
* The section the device sliced against the restatement.
* Runs: a box mesh and the polygon rectangle give bit-identical outputs and onsets at 96^2 (resident kernel) and 520^2 (tile
  path); the composed material of a sphere and a torus goes through the oracle; one run in sparse-emitter mode.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from _mesh_ref import (SHELL, SOLID, Model, box, comb, compose, coverage, rotated_box, rotation, section, snap, tetrahedron, torus,
                       uv_sphere)
from _round_shapes_ref import DISC, POLYGON, compose as compose_shapes
from test_gpu_analysis_edges import DX, EFREE, cell, compare_all_cells, open_size
from test_gpu_shapes import oracle_runs

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
F = np.float32
dx = float(DX)


def add(s, mesh, a):
    v, t, mode, r, m12 = mesh
    mid = s.add_mesh(v, t, a, mode, r)
    if m12 is not None:
        s.set_mesh_transform(mid, m12)
    return mid


def check_material(s, base, model, h, shapes=(), ctx=""):
    """AABB layer < meshes (most recent on top) < shapes"""
    b, R = compose(base[0], base[1], model.ordered(), h, s.gx, s.gy, s.dx)
    want_b, want_R = compose_shapes(b, R, list(shapes), s.gx, s.gy, s.dx)
    got_b, got_R = s.material()
    bad = got_b != want_b
    assert not bad.any(), "%s beta: %d cells differ, first %s" % (ctx, int(bad.sum()), np.argwhere(bad)[:3])
    assert np.array_equal(got_R.view(np.uint32), want_R.view(np.uint32)), "%s R differs" % ctx
    return want_b, want_R


def random_mesh(rng, size, k):
    c = rng.uniform(0.0, size, 2)
    y = rng.uniform(-0.5, 0.5)
    kind = k % 5
    if kind == 0:
        v, t = rotated_box(rng, (c[0], y, c[1]), rng.uniform(0.5, size / 5, 3))
    elif kind == 1:
        v, t = uv_sphere((c[0], y, c[1]), rng.uniform(1.0, size / 5), int(rng.integers(4, 12)), int(rng.integers(5, 16)))
    elif kind == 2:
        R = rng.uniform(2.0, size / 4)
        v, t = torus((c[0], y, c[1]), R, R * rng.uniform(0.15, 0.45), 18, 9, rotation(rng) if rng.random() < 0.5 else None)
    elif kind == 3:
        p = rng.uniform(-2.0, size + 2.0, (4, 3))
        p[:3, 1], p[3, 1] = rng.uniform(-2.0, -1.2, 3), rng.uniform(1.2, 6.0)
        v, t = tetrahedron(*p)
    else:
        v, t = comb(c[0] - 4.0, c[1] - 2.0, int(rng.integers(3, 12)), 0.9, 0.45, rng.uniform(1.0, 6.0))
    if rng.random() < 0.3:
        v = snap(v, dx, 0.0, rng)
    shell = rng.random() < 0.4
    return (v, t, SHELL if shell else SOLID, float(rng.uniform(0.1, 0.7)) if shell else 0.0, None)


def random_transform(rng, size):
    m = np.hstack([rotation(rng) * rng.uniform(0.6, 1.3), rng.uniform(-0.2, 0.2, (3, 1)) * [[size], [2.0], [size]]])
    return m.astype(np.float32).reshape(12)


def absorption(rng):
    return float(rng.choice([0.969536, 0.5, 0.0, 0.999, rng.uniform(0.05, 0.95)]))


# ------------------------------------------------------------------------------------------------------------------------------
# material
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res,n_ops", [(275, 60), (1000, 40)])  # 70^2 and 254^2
def test_material_through_random_add_update_transform_height_remove(pvlib, res, n_ops):
    rng = np.random.default_rng(res + 1)
    size = 25.0
    with pvlib.Solver(size, size, res) as s:
        s.load_scene(SMALLROOM)
        base = s.material()
        assert s.slice_height == 0.0
        shapes = [((DISC, [(9.0, 16.0)], 1.4), 0.8), ((POLYGON, [(14, 3), (22, 4), (21, 9), (17, 6), (15, 10)], 0.0), 0.3)]
        model, h = Model(), 0.0
        for step in range(n_ops):
            op = rng.random()
            if op < 0.35 or not model.live or (len(model.live) < 2 and op < 0.6):
                if len(model.live) >= 6:
                    continue
                mesh, a = random_mesh(rng, size, step), absorption(rng)
                assert s.add_mesh(mesh[0], mesh[1], a, mesh[2], mesh[3]) == model.add(mesh, a)
            elif op < 0.5:
                mid = int(rng.choice(list(model.live)))
                mesh, a = random_mesh(rng, size, int(rng.integers(0, 5))), absorption(rng)
                s.update_mesh(mid, mesh[0], mesh[1], a, mesh[2], mesh[3])
                model.update(mid, mesh, a)
            elif op < 0.7:
                mid = int(rng.choice(list(model.live)))
                m = random_transform(rng, size)
                s.set_mesh_transform(mid, m)
                model.transform(mid, m)
            elif op < 0.85:
                h = float(F(rng.uniform(-0.8, 0.8)))
                s.set_slice_height(h)
                assert s.slice_height == h
            else:
                mid = int(rng.choice(list(model.live)))
                s.remove_mesh(mid)
                model.remove(mid)
            if step == 7:  # the shape layer goes on top, and stays there
                s.add_disc(9.0, 16.0, 1.4, 0.8)
                s.add_polygon(shapes[1][0][1], 0.3)
            if step % 4 == 3:
                check_material(s, base, model, h, shapes if step >= 7 else (), "step %d" % step)
            if step % 15 == 14:
                s.run((5.0, 0.0, 4.0))  # (so the changes reach the device in several batches)
        want_b, _ = check_material(s, base, model, h, shapes, "end")
        # the b / by of the impulse-response cells: the material during the run
        s.run((12.5, 0.0, 12.5))
        xs, ys = np.nonzero(want_b[:s.gx, :s.gy] != base[0][:s.gx, :s.gy])
        for cx, cy in list(zip(xs[:6], ys[:6])) + [(3, 3)]:
            cells = s.impulse_response_cells(int(cx), int(cy))
            assert (cells["b"] == want_b[cx, cy]).all() and (cells["by"][want_b[cx, cy] == 0] == 0).all(), (cx, cy)
        # refusals leave the tables as they were
        v, t = box((3.0, -1.0, 4.0), (9.0, 2.0, 11.0))
        nanv = v.copy()
        nanv[0, 0] = np.nan
        if not model.live:
            mesh = (v, t, SOLID, 0.0, None)
            assert add(s, mesh, 0.5) == model.add(mesh, 0.5)
        live = next(iter(model.live))
        for bad in (lambda: s.add_mesh(nanv, t, 0.5), lambda: s.add_mesh(v, t[:-1], 0.5), lambda: s.add_mesh(v, t, float("nan")),
                    lambda: s.add_mesh(v, t, 0.5, SHELL, 0.0), lambda: s.add_mesh(v, t, 0.5, SHELL, float("inf")),
                    lambda: s.add_mesh(v, t + 1, 0.5), lambda: s.add_mesh(v, t[:0], 0.5), lambda: s.add_mesh(v, t, 0.5, 3),
                    lambda: s.update_mesh(live, v, t[:-1], 0.5), lambda: s.update_mesh(999, v, t, 0.5),
                    lambda: s.set_mesh_transform(live, np.full(12, np.inf, np.float32)), lambda: s.set_mesh_transform(77, np.eye(3, 4)),
                    lambda: s.set_slice_height(float("nan")), lambda: s.set_slice_height(float("inf")), lambda: s.remove_mesh(63)):
            with pytest.raises(pvlib.PlaneverbError):
                bad()
        assert s.slice_height == h
        check_material(s, base, model, h, shapes, "after refusals")
        mesh = (v, t[:-1], SHELL, 0.3, None)  # (the open mesh is a valid shell; the id table is as the model's)
        assert add(s, mesh, 0.5) == model.add(mesh, 0.5)
        check_material(s, base, model, h, shapes, "after refusals and one more mesh")
        # removing every mesh brings back the AABB layer under the shapes
        for mid in list(model.live):
            s.remove_mesh(mid)
            model.remove(mid)
        check_material(s, base, model, h, shapes, "no mesh left")


def special_meshes(size):
    c = size / 2
    big = uv_sphere((c, 0.3, c), 0.42 * size, 72, 70)  # 2 * 70 * 71 = 9940 triangles
    assert 9900 <= len(big[1]) <= 10100
    # teeth thinner than a cell, 0.13 m apart: ~300 crossings in each of the rows they span, several marks per coverage word
    teeth = comb(0.7, 2.0, 150, 0.13, 0.05, size - 4.0)
    # faces that span every row of the grid (and stick out at both ends)
    spike = tetrahedron((3.0, -1.0, -4.0), (size - 2.0, -1.0, size + 5.0), (9.0, -1.0, size + 6.0), (c, 0.6, c))
    return [("10 000-triangle sphere", (big[0], big[1], SOLID, 0.0, None), 0.1),
            ("10 000-triangle sphere, shell", (big[0], big[1], SHELL, 0.25, None), 0.1),
            ("comb", (teeth[0], teeth[1], SOLID, 0.0, None), 0.0), ("comb, shell", (teeth[0], teeth[1], SHELL, 0.04, None), 0.0),
            ("tall tetrahedron", (spike[0], spike[1], SOLID, 0.0, None), 0.2),
            ("one triangle across every row", (np.array([(1.0, -1.0, -3.0), (size - 1.0, -1.0, size + 4.0), (c, 2.0, c)], np.float32),
                                               np.array([(0, 1, 2)], np.int32), SHELL, 0.3, None), 0.5)]


@pytest.mark.parametrize("res", [275, 1000])
def test_generators_many_blocks_contended_words_and_long_segments(pvlib, res):
    size = 25.0
    rng = np.random.default_rng(11)
    c = size / 2
    meshes = [(name, m, 0.0) for name, m in [
        ("box out of the grid", (*box((-5.0, -1.0, -3.0), (6.0, 2.0, 5.0)), SOLID, 0.0, None)),
        ("box over the whole grid", (*box((-2.0, -1.0, -2.0), (size + 2.0, 2.0, size + 2.0)), SOLID, 0.0, None)),
        ("rotated box", (*rotated_box(rng, (c, 0.3, c), (5.0, 3.0, 2.0)), SOLID, 0.0, None)),
        ("torus", (*torus((c, 0.2, c), 7.0, 2.5, 24, 12), SOLID, 0.0, None)),
        ("tilted torus, shell", (*torus((c + 3.0, 0.0, c - 2.0), 6.0, 2.0, 20, 10, rotation(rng)), SHELL, 0.2, None)),
        ("sphere out of the corner", (*uv_sphere((1.0, 0.0, size - 1.0), 5.0, 9, 11), SOLID, 0.0, None))]] + special_meshes(size)
    with pvlib.Solver(size, size, res) as s:
        s.load_scene(SMALLROOM)
        base = s.material()
        mid = None
        for name, mesh, h in meshes:
            s.set_slice_height(h)
            for variant in (mesh, mesh[:4] + (random_transform(rng, size),), (snap(mesh[0], s.dx, h, rng),) + mesh[1:]):
                if mid is None:
                    mid = s.add_mesh(variant[0], variant[1], 0.7, variant[2], variant[3])
                    s.set_mesh_transform(mid, np.eye(3, 4) if variant[4] is None else variant[4])
                else:  # (one slot throughout: every update re-derives where the mesh was)
                    s.update_mesh(mid, variant[0], variant[1], 0.7, variant[2], variant[3])
                    s.set_mesh_transform(mid, np.eye(3, 4) if variant[4] is None else variant[4])
                model = Model()
                model.add(variant[:4] + (np.eye(3, 4, dtype=np.float32).reshape(12) if variant[4] is None else variant[4],), 0.7)
                want_b, _ = check_material(s, base, model, h, (), "%s at %d" % (name, res))
                seg, valid = s.mesh_section(mid)
                wseg, wvalid = section(variant[0], variant[1], h, model.ordered()[0][0][4])
                assert np.array_equal(valid, wvalid) and np.array_equal(seg.view(np.uint32), wseg.view(np.uint32)), name
            assert (want_b != base[0]).any() or "comb" in name, name


def test_torus_has_a_hole_and_section_without_transform(pvlib):
    size = 25.0
    v, t = torus((12.5, 0.0, 12.5), 7.0, 2.0, 32, 12)
    with pvlib.Solver(size, size, 275) as s:
        mid = s.add_mesh(v, t, 0.4)
        b, R = s.material()
        ci = int(12.5 / s.dx)
        assert b[ci, ci] == 1 and b[int(19.5 / s.dx), ci] == 0 and b[int(5.5 / s.dx), ci] == 0
        assert np.array_equal(b[:s.gx, :s.gy] == 0, coverage((v, t, SOLID, 0.0, None), 0.0, s.gx, s.gy, s.dx)[:s.gx, :s.gy] == 1)
        seg, valid = s.mesh_section(mid)  # (no transform call: the vertices as they are)
        hseg, hvalid = pvlib.host_mesh_section(v, t, 0.0)
        assert np.array_equal(valid, hvalid) and np.array_equal(seg.view(np.uint32), hseg.view(np.uint32)) and valid.sum() > 60
        # above the torus nothing is cut
        s.set_slice_height(2.5)
        b, _ = s.material()
        assert (b[:s.gx, :s.gy] == 1).all() and s.mesh_section(mid)[1].sum() == 0


def test_slabs_refuse_meshes(pvlib):
    v, t = box((3.0, -1.0, 4.0), (9.0, 2.0, 11.0))
    tp = t.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    h = pvlib.lib().PvAmdCreateSlabRank(25.0, 25.0, 275, 0, 0, 2)
    assert h
    try:
        assert pvlib.lib().PvAmdAddMesh(h, pvlib._f(v), 8, tp, 12, 0.5, 0, 0.0) == -1 and "slab" in pvlib.last_error()
        assert pvlib.lib().PvAmdSetSliceHeight(h, 1.0) == -1
    finally:
        pvlib.lib().PvAmdDestroy(h)
    with pvlib.Solver(open_size(600), open_size(600), 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError):
            s.add_mesh(v, t, 0.5)
        assert "slab" in pvlib.last_error()


# ------------------------------------------------------------------------------------------------------------------------------
# runs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,res,resident", [(95, 375, 1), (520, 275, 0)])  # cell arrays of 96^2 and 521^2
def test_box_mesh_and_polygon_rectangle_run_bit_identically(pvlib, n, res, resident):
    size = 25.0 if n == 95 else open_size(520)
    u = size / 25.0
    rect = np.array([(8.0, 9.0), (13.5, 9.0), (13.5, 12.25), (8.0, 12.25)], np.float32) * F(u)
    (x0, z0), (x1, z1) = rect[0], rect[2]
    L = (5.0 * u, 0.0, 4.0 * u)
    out = []
    for as_mesh in (True, False):
        with pvlib.Solver(size, size, res) as s:
            assert (s.gx, s.gy) == (n, n)
            if n == 95:
                s.load_scene(SMALLROOM)
            if as_mesh:
                s.set_slice_height(0.25)
                s.add_mesh(*box((x0, -1.0, z0), (x1, 1.5, z1)), 0.6)
            else:
                s.add_polygon(rect, 0.6)
            mat = s.material()
            s.run(L)
            out.append((mat, s.results(), s.info.residentKernel))
    (ma, (ra, da), ka), (mb, (rb, db), kb) = out
    assert ka == kb == resident
    assert np.array_equal(ma[0], mb[0]) and np.array_equal(ma[1].view(np.uint32), mb[1].view(np.uint32))
    assert (ma[0][:n, :n] == 0).sum() > 100
    assert same_bits(da, db).all() and same_bits(ra, rb).all()


def test_oracle_sphere_and_torus(pvlib, oracle):
    size, res = 25.0, 275
    boxes = pvlib.load_pv(SMALLROOM)
    L = (5.0, 0.0, 4.0)
    with pvlib.Solver(size, size, res) as s:
        for bx in boxes:
            s.add_geometry(bx)
        base = s.material()
        model = Model()
        s.set_slice_height(0.35)
        for mesh, a in (((*uv_sphere((11.0, 0.0, 9.0), 2.2, 10, 14), SOLID, 0.0, None), 0.7),
                        ((*torus((15.0, 0.4, 16.0), 4.0, 1.2, 24, 10), SOLID, 0.0, None), 0.4),
                        ((*uv_sphere((19.0, 0.5, 6.0), 2.5, 8, 12), SHELL, 0.3, None), 0.9)):
            assert add(s, mesh, a) == model.add(mesh, a)
        mat = check_material(s, base, model, 0.35, (), "oracle scene")
        assert (mat[0] != base[0]).sum() > 40
        (r, d), = oracle_runs(oracle, size, res, boxes, [mat], [L])
        s.run(L)
        got, gd = s.results()
        compare_all_cells(got, gd, r, d, "sphere and torus", s.T, s.fs)


def test_oracle_sparse_emitter_mode(pvlib, oracle):
    boxes = pvlib.load_pv(SMALLROOM)
    L = (5.0, 0.0, 4.0)
    E = [(12.0, 0.0, 20.0), (20.0, 0.0, 5.0), (3.0, 0.0, 22.0)]
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        for bx in boxes:
            s.add_geometry(bx)
        base = s.material()
        model = Model()
        mesh = (*torus((14.0, 0.1, 12.0), 4.5, 1.3, 24, 10), SOLID, 0.0, None)
        assert add(s, mesh, 0.6) == model.add(mesh, 0.6)
        mat = check_material(s, base, model, 0.0, (), "streaming")
        (r, d), = oracle_runs(oracle, 25.0, 275, boxes, [mat], [L])
        s.set_emitters(E)
        s.run(L)
        got, gd = s.results()
        assert same_bits(gd, d).all()
        for k in (0, 3, 4, 5, 6, 7):  # the forward outputs of every cell
            assert same_bits(got[..., k], r[..., k]).all(), k
        o = oracle.OracleGrid(25.0, 25.0, 275)
        for e in E:
            assert same_bits(s.get_output(e).as_array(), r.reshape(-1, 8)[o.result_index(e)]).all(), e
        o.close()


# ------------------------------------------------------------------------------------------------------------------------------
# live module: a mesh is added, moved, sliced at another height and removed between iterations
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["1", "2"])
def test_live_mesh_added_moved_height_changed_removed(pvlib, monkeypatch, pipeline):
    monkeypatch.setenv("PLANEVERB_AMD_LIVE_PIPELINE", pipeline)
    boxes = pvlib.load_pv(SMALLROOM)
    Lst = (5.0, 0.0, 4.0)
    E = [(12.0, 0.0, 20.0), (20.0, 0.0, 5.0), (3.0, 0.0, 22.0)]
    # a cone standing on y = -0.5: the higher the slice, the smaller the pillar
    n = 16
    ring = [(1.8 * np.cos(2 * np.pi * k / n), -0.5, 1.8 * np.sin(2 * np.pi * k / n)) for k in range(n)]
    v = np.array(ring + [(0.0, -0.5, 0.0), (0.0, 2.5, 0.0)], np.float32) + np.array([9.0, 0.0, 8.0], np.float32)
    t = np.array([(k, (k + 1) % n, n) for k in range(n)] + [((k + 1) % n, k, n + 1) for k in range(n)], np.int32)
    move = lambda x, z: np.array([1, 0, 0, x, 0, 1, 0, 0, 0, 0, 1, z], np.float32)
    # (mesh present, transform or None, height); every state leaves every emitter reachable
    states = [(False, None, 0.0), (True, None, 0.0), (True, move(1.5, 1.0), 0.0), (True, move(1.5, 1.0), 1.5), (True, move(3.0, 2.0), 0.75),
              (False, None, 0.75), (True, None, 0.75)]
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, 0, ".", 0, pvlib.pv_GPU))
    try:
        for b in boxes:
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(Lst)
        eids = [pvlib.Emit(e) for e in E]
        mid, cur_m, cur_h = None, None, 0.0
        for k, (present, m, h) in enumerate(states):
            if mid is not None and not present:
                pvlib.RemoveMeshGeometry(mid)
                mid, cur_m = None, None
            if present and mid is None:
                mid = pvlib.AddMeshGeometry(v, t, 0.7)
                assert mid == 0
                cur_m = None
            if present and m is not None and (cur_m is None or not np.array_equal(m, cur_m)):
                pvlib.SetMeshGeometryTransform(mid, m)
                cur_m = m
            if h != cur_h:
                pvlib.SetSliceHeight(h)
                cur_h = h
            target = pvlib.IterationCount() + 4
            assert pvlib.WaitIterations(target, 120000) >= target
            got = [pvlib.GetOutput(eid).as_array() for eid in eids]
            with pvlib.Solver(25.0, 25.0, 275) as fresh:  # a fresh solver with the same geometry
                for b in boxes:
                    fresh.add_geometry(b)
                fresh.set_slice_height(h)
                if present:
                    fm = fresh.add_mesh(v, t, 0.7)
                    if m is not None:
                        fresh.set_mesh_transform(fm, m)
                    b_, _ = fresh.material()
                    want_b, _ = compose(*base_of(pvlib, boxes), [((v, t, SOLID, 0.0, m), 0.7)], h, fresh.gx, fresh.gy, fresh.dx)
                    assert np.array_equal(b_, want_b) and (want_b != base_of(pvlib, boxes)[0]).sum() > 3, k
                fresh.run(Lst)
                for g, e in zip(got, E):
                    want = fresh.get_output(e).as_array()
                    assert np.isfinite(want[0]) and want[0] >= 0, (k, e, want)
                    assert same_bits(g, want).all(), (pipeline, k, e, g, want)
        assert pvlib.IsRunning()
        # refusals at the call: nothing is queued, the id table is unchanged
        assert pvlib.AddMeshGeometry(v, t[:-1], 0.7) == -1 and "closed" in pvlib.last_error()
        assert pvlib.AddMeshGeometry(v, t, float("nan")) == -1
        assert pvlib.AddMeshGeometry(v, t, 0.7) == 1
    finally:
        pvlib.Exit()


_BASE = {}


def base_of(pvlib, boxes):
    if "m" not in _BASE:
        with pvlib.Solver(25.0, 25.0, 275) as s:
            for b in boxes:
                s.add_geometry(b)
            _BASE["m"] = s.material()
    return _BASE["m"]
