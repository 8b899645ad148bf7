"""GPU (-m gpu): oriented boxes and convex polygons (include/planeverb_amd.h, "Shapes").

* Material: PvAmdCopyMaterial and the b / by of PvAmdGetImpulseResponseCells equal the numpy restatement of the coverage and
  composition rules (_shapes_ref.py) over AABB scenes, through random add / update / remove sequences, and removing every
  shape gives back the AABB-only material and runs bit-identical to a solver that never had a shape.
* Runs: the composed material is loaded into the oracle's b / R planes and every member of every cell is compared, chained
  with prev= as in test_gpu_analysis_edges.py, for the resident, merged, windowed, sparse-emitter, batched and slab forms.
* Live module: a door swings on its hinge, one PlaneverbUpdateOrientedGeometry per iteration, one and two solvers in flight.
"""
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from _shapes_ref import compose, obb_vertices, random_convex
from test_gpu_analysis_edges import EFREE, cell, compare_all_cells, open_size
from test_gpu_parity import random_scene

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")


def load_material(o, b, R):
    """overwrite the oracle grid's material planes (its FDTD reads them on every run)"""
    n = o.ncell
    np.ctypeslib.as_array(o._g.contents.b, (n,))[:] = np.asarray(b, np.int16).reshape(-1)
    np.ctypeslib.as_array(o._g.contents.R, (n,))[:] = np.asarray(R, np.float32).reshape(-1)


def random_shapes(rng, size, n):
    """oriented boxes, convex polygons, slivers, shapes partly or wholly outside the grid; (vertices, absorption)"""
    out = []
    for k in range(n):
        c = rng.uniform(-0.1 * size, 1.1 * size, 2)
        a = float(rng.choice([0.969536, 0.5, 0.0, 0.999, rng.uniform(0.05, 0.95)]))
        kind = k % 4
        if kind == 0:
            ang = rng.uniform(0, 2 * np.pi)
            xy = obb_vertices(c[0], c[1], rng.uniform(0.5, size / 3), rng.uniform(0.2, 1.5), np.cos(ang), np.sin(ang))
        elif kind == 1:
            xy = random_convex(rng, c[0], c[1], rng.uniform(0.5, size / 5), int(rng.integers(3, 9)))
        elif kind == 2:
            d = rng.uniform(-0.3, 0.3, 2) * size
            xy = np.array([c, c + d, c + d * 1.02 + rng.uniform(0.05, 0.3, 2)], np.float32)
        else:
            xy = obb_vertices(c[0] + rng.choice([-1, 1]) * size, c[1], size / 2, 2.0, 1.0, 0.4)
        out.append((np.asarray(xy, np.float32), a))
    return out


class Model:
    """the shape table as the library keeps it: ids recycled LIFO, sequence order = order of the last add / update"""

    def __init__(self):
        self.live, self.free, self.seq = {}, [], 0

    def add(self, xy, a):
        sid = self.free.pop() if self.free else len(self.live) + len(self.free)
        self.live[sid] = (xy, a, self.seq)
        self.seq += 1
        return sid

    def update(self, sid, xy, a):
        self.live[sid] = (xy, a, self.seq)
        self.seq += 1

    def remove(self, sid):
        del self.live[sid]
        self.free.append(sid)

    def ordered(self):
        return [(xy, a) for xy, a, _ in sorted(self.live.values(), key=lambda v: v[2])]


def check_material(s, base, model, ctx=""):
    want_b, want_R = compose(base[0], base[1], model.ordered(), s.gx, s.gy, s.dx)
    b, R = s.material()
    assert np.array_equal(b, want_b), "%s beta: %d cells differ" % (ctx, int((b != want_b).sum()))
    assert np.array_equal(R.view(np.uint32), want_R.view(np.uint32)), "%s R differs" % ctx
    return want_b, want_R


def add_all(s, model, shapes):
    for xy, a in shapes:
        try:
            sid = s.add_shape(xy, a)
        except Exception:  # (a sliver whose area rounded to zero: refused on both sides)
            continue
        assert sid == model.add(xy, a)


# ------------------------------------------------------------------------------------------------------------------------------
# material
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,res", [("SmallRoomScene.pv", 275), ("FloorPlanScene.pv", 375), ("HugeRoom.pv", 1000)])
def test_material_composition(pvlib, scene, res):
    rng = np.random.default_rng(sum(map(ord, scene)) + res)
    with pvlib.Solver(25.0, 25.0, res) as s:
        s.load_scene(os.path.join(SCENES, scene))
        base = s.material()
        model = Model()
        add_all(s, model, random_shapes(rng, 25.0, 40))
        want_b, _ = check_material(s, base, model, scene)
        # the b / by of the impulse-response cells: the material during the run
        s.run((12.5, 0.0, 12.5))
        xs, ys = np.nonzero(want_b[:s.gx, :s.gy] != base[0][:s.gx, :s.gy])
        pick = list(zip(xs[:6], ys[:6])) + [(3, 3), (s.gx // 2, s.gy // 2)]
        for cx, cy in pick:
            cells = s.impulse_response_cells(int(cx), int(cy))
            assert (cells["b"] == want_b[cx, cy]).all() and (cells["by"][want_b[cx, cy] == 0] == 0).all(), (cx, cy)


def test_random_add_update_remove_sequences(pvlib):
    rng = np.random.default_rng(5)
    size = 25.0
    with pvlib.Solver(size, size, 375) as s:
        s.load_scene(SMALLROOM)
        base = s.material()
        model = Model()
        for step in range(12):
            for _ in range(int(rng.integers(1, 8))):
                op = rng.random()
                if op < 0.45 or not model.live:
                    (xy, a), = random_shapes(rng, size, 1) if rng.random() < 0.5 else [random_shapes(rng, size, 2)[1]]
                    add_all(s, model, [(xy, a)])
                elif op < 0.75:
                    sid = int(rng.choice(list(model.live)))
                    ang = rng.uniform(0, 2 * np.pi)
                    c = rng.uniform(0, size, 2)
                    if rng.random() < 0.5:
                        s.update_oriented_box(sid, c[0], c[1], 6.0, 0.5, np.cos(ang) * 2, np.sin(ang) * 2, 0.3)
                        model.update(sid, obb_vertices(c[0], c[1], 6.0, 0.5, np.cos(ang) * 2, np.sin(ang) * 2), 0.3)
                    else:
                        xy = random_convex(rng, c[0], c[1], 2.0, 5)
                        s.update_shape(sid, xy, 0.7)
                        model.update(sid, xy, 0.7)
                else:
                    sid = int(rng.choice(list(model.live)))
                    s.remove_shape(sid)
                    model.remove(sid)
            check_material(s, base, model, "step %d" % step)
            if step % 4 == 3:
                s.run((5.0, 0.0, 4.0))  # (applied on the device between runs as well)
        # an AABB change under the shapes keeps the shapes on top
        gid = s.add_geometry((12.5, 12.5, 10.0, 1.0, 0.25))
        base2 = pvlib.host_rasterize(size, size, 375, np.vstack([pvlib.load_pv(SMALLROOM), [[12.5, 12.5, 10.0, 1.0, 0.25]]]))
        check_material(s, base2, model, "after an AABB")
        s.remove_geometry(gid)
        # refusals leave the table as it was
        with pytest.raises(pvlib.PlaneverbError):
            s.add_shape([(0, 0), (1, 1), (2, 2)], 0.5)
        with pytest.raises(pvlib.PlaneverbError):
            s.remove_shape(999)


def test_remove_every_shape_restores_the_aabb_path(pvlib):
    L = (5.0, 0.0, 4.0)
    with pvlib.Solver(25.0, 25.0, 275) as s, pvlib.Solver(25.0, 25.0, 275) as ref:
        for x in (s, ref):
            x.load_scene(SMALLROOM)
        base = ref.material()
        ids = [s.add_oriented_box(8.0 + i, 9.0, 5.0, 0.4, 1.0, 0.3 * i, 0.5) for i in range(5)]
        s.run(L)
        for i in ids:
            s.remove_shape(i)
        b, R = s.material()
        assert np.array_equal(b, base[0]) and np.array_equal(R.view(np.uint32), base[1].view(np.uint32))
        s.run(L)
        ref.run(L)
        (r1, d1), (r2, d2) = s.results(), ref.results()
        assert same_bits(d1, d2).all() and same_bits(r1, r2).all()
        E = (12.0, 0.0, 20.0)
        assert same_bits(s.get_output(E).as_array(), ref.get_output(E).as_array()).all()


# ------------------------------------------------------------------------------------------------------------------------------
# runs against the oracle
# ------------------------------------------------------------------------------------------------------------------------------
def oracle_runs(oracle, size, res, boxes, materials, listeners, efree=None):
    """the oracle chain over (material, listener) pairs: [(records, delay)]"""
    o = oracle.OracleGrid(size, size, res, boxes)
    ef = oracle.free_energy(size, size, res) if efree is None else efree
    out, prev = [], None
    for (b, R), L in zip(materials, listeners):
        load_material(o, b, R)
        o.fdtd(L)
        r, d, _ = o.analyze(ef, L, prev=prev)
        out.append((r, d))
        prev = r
    o.close()
    return out


def accepted(pvlib, shapes):
    """the shapes the library accepts (a sliver can round to zero area)"""
    out = []
    for xy, a in shapes:
        try:
            pvlib.host_shape(xy, a)
            out.append((xy, a))
        except pvlib.PlaneverbError:
            pass
    return out


def run_case(pvlib, oracle, size, res, boxes, shape_steps, listeners, ctx, efree=None, **opts):
    """shape_steps[i]: shapes present during run i (each step replaces the previous set); one solver runs them all"""
    shape_steps = [accepted(pvlib, st) for st in shape_steps]
    with pvlib.Solver(size, size, res, **opts) as s:
        for bx in (boxes if boxes is not None else []):
            s.add_geometry(bx)
        base = s.material()
        mats, ids = [], []
        for k, (shapes, L) in enumerate(zip(shape_steps, listeners)):
            for i in ids:
                s.remove_shape(i)
            model = Model()
            ids = []
            for xy, a in shapes:
                ids.append(s.add_shape(xy, a))
                model.add(xy, a)
            mats.append(check_material(s, base, model, "%s step %d" % (ctx, k)))
        chain = oracle_runs(oracle, size, res, boxes, mats, listeners, efree)
        # (second pass: run with each step's shapes)
        for i in ids:
            s.remove_shape(i)
        ids = []
        for k, (shapes, L) in enumerate(zip(shape_steps, listeners)):
            for i in ids:
                s.remove_shape(i)
            ids = [s.add_shape(xy, a) for xy, a in shapes]
            s.run(L)
            got, gd = s.results()
            compare_all_cells(got, gd, chain[k][0], chain[k][1], "%s run %d" % (ctx, k), s.T, s.fs)
    return chain


def room_with_doorway():
    """a 10 m room inside a 25 m grid, its right wall with a 2 m doorway at z = 11 ... 13"""
    return np.array([[12.5, 5.0, 10.8, 0.8, 0.9], [12.5, 15.0, 10.8, 0.8, 0.9], [7.5, 10.0, 0.8, 10.8, 0.9],
                     [17.5, 7.6, 0.8, 5.6, 0.9], [17.5, 14.0, 0.8, 2.8, 0.9]], np.float32)


def test_rotated_wall_closes_and_opens_a_room(pvlib, oracle):
    """air components change: a wall at 45 degrees seals the doorway, then goes away (run 3 carries the unreached cells)"""
    plug = (obb_vertices(17.5, 11.5, 5.0, 1.5, 1.0, 1.0), 0.8)
    L = (10.0, 0.0, 10.0)
    chain = run_case(pvlib, oracle, 25.0, 275, room_with_doorway(), [[], [plug], []], [L, L, (11.0, 0.0, 9.0)], "room")
    # the sealed room: the outside is unreached in run 2
    assert (chain[1][1] > 1e30).sum() > (chain[0][1] > 1e30).sum()


@pytest.mark.parametrize("res", [375, 500])  # 96^2 and 127^2: the resident kernel
def test_oracle_resident_presets(pvlib, oracle, res):
    rng = np.random.default_rng(res)
    boxes = pvlib.load_pv(SMALLROOM)
    steps = [random_shapes(rng, 25.0, 8), random_shapes(rng, 25.0, 8)]
    run_case(pvlib, oracle, 25.0, res, boxes, steps, [(5.0, 0.0, 4.0), (20.0, 0.0, 20.0)], "resident %d" % res)


def test_oracle_merged_512(pvlib, oracle):
    rng = np.random.default_rng(512)
    size = open_size(512)
    boxes = random_scene(rng, size, 40)
    steps = [random_shapes(rng, size, 30), random_shapes(rng, size, 30)]
    run_case(pvlib, oracle, size, 275, boxes, steps, [cell(256, 256), cell(40, 470)], "merged 512", EFREE)


def test_oracle_windowed_1040(pvlib, oracle):
    """a history window smaller than the grid: the second listener lies outside the first run's window"""
    rng = np.random.default_rng(1040)
    size = open_size(1040)
    near = [(obb_vertices(c[0], c[1], 8.0, 0.6, 1.0, 0.6), 0.7) for c in ((95.0, 230.0), (330.0, 20.0), (110.0, 240.0))]
    steps = [near + random_shapes(rng, size, 10), near[1:]]
    run_case(pvlib, oracle, size, 275, None, steps, [cell(300, 700), cell(1000, 40)], "window 1040", EFREE)


def test_oracle_sparse_emitter_mode(pvlib, oracle):
    rng = np.random.default_rng(3)
    boxes = pvlib.load_pv(SMALLROOM)
    shapes = random_shapes(rng, 25.0, 10)
    L = (5.0, 0.0, 4.0)
    E = [(12.0, 0.0, 20.0), (20.0, 0.0, 5.0), (3.0, 0.0, 22.0)]
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        for bx in boxes:
            s.add_geometry(bx)
        base = s.material()
        model = Model()
        add_all(s, model, shapes)
        mat = check_material(s, base, model, "streaming")
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


def test_oracle_batch_two_shape_sets(pvlib, oracle):
    rng = np.random.default_rng(9)
    boxes = pvlib.load_pv(SMALLROOM)
    sets = [random_shapes(rng, 25.0, 6), random_shapes(rng, 25.0, 9)]
    L = [(5.0, 0.0, 4.0), (20.0, 0.0, 18.0)]
    solvers = [pvlib.Solver(25.0, 25.0, 275) for _ in range(2)]
    try:
        mats = []
        for s, shapes in zip(solvers, sets):
            for bx in boxes:
                s.add_geometry(bx)
            base = s.material()
            model = Model()
            add_all(s, model, shapes)
            mats.append(check_material(s, base, model, "batch"))
        pvlib.run_batch(solvers, L)
        for k, s in enumerate(solvers):
            (r, d), = oracle_runs(oracle, 25.0, 275, boxes, [mats[k]], [L[k]])
            got, gd = s.results()
            compare_all_cells(got, gd, r, d, "batch member %d" % k, s.T, s.fs)
    finally:
        for s in solvers:
            s.close()


@pytest.mark.parametrize("nslabs", [2, 4])
def test_slabs_bit_identical_to_one_solver(pvlib, nslabs):
    rng = np.random.default_rng(nslabs)
    size = open_size(600)
    boxes = random_scene(rng, size, 30)
    shapes = random_shapes(rng, size, 25)
    # (a wall across every slab boundary)
    shapes.append((obb_vertices(size / 2, size / 2, size * 0.9, 1.0, 0.2, 1.0), 0.6))
    L = [cell(300, 300), cell(60, 520)]
    res = []
    for slabs in (None, [0] * nslabs):
        with pvlib.Solver(size, size, 275, slabs=slabs) as s:
            for bx in boxes:
                s.add_geometry(bx)
            ids = [s.add_shape(xy, a) for xy, a in shapes]
            out = [s.material()]
            s.run(L[0])
            out.append(s.results())
            s.update_oriented_box(ids[-1], size / 2, size / 2, size * 0.9, 1.0, 1.0, 0.2, 0.6)
            s.remove_shape(ids[0])
            s.run(L[1])
            out.append(s.results())
            res.append(out)
    (m1, a1, b1), (m2, a2, b2) = res
    assert np.array_equal(m1[0], m2[0]) and np.array_equal(m1[1], m2[1])
    for (r1, d1), (r2, d2) in ((a1, a2), (b1, b2)):
        assert same_bits(d1, d2).all() and same_bits(r1, r2).all()


def test_slab_rank_refuses_shapes(pvlib):
    h = pvlib.lib().PvAmdCreateSlabRank(25.0, 25.0, 275, 0, 0, 2)
    assert h
    try:
        assert pvlib.lib().PvAmdAddOrientedBox(h, 5, 5, 2, 1, 1, 0, 0.5) == -1
        assert "slab rank" in pvlib.last_error()
    finally:
        pvlib.lib().PvAmdDestroy(h)


# ------------------------------------------------------------------------------------------------------------------------------
# live module
# ------------------------------------------------------------------------------------------------------------------------------
def door(theta):
    """a 2.8 m door hinged at (17.5, 10.1), closed along +z (theta = 0), opening outwards to theta = 90 degrees"""
    L, T = 2.8, 0.5
    ux, uy = float(np.sin(theta)), float(np.cos(theta))
    return (17.5 + ux * L / 2, 10.1 + uy * L / 2, L, T, ux, uy, 0.6)


@pytest.mark.parametrize("pipeline", ["1", "2"])
def test_live_door_swings(pvlib, oracle, monkeypatch, pipeline):
    monkeypatch.setenv("PLANEVERB_AMD_LIVE_PIPELINE", pipeline)
    boxes = room_with_doorway()
    Lst = (10.0, 0.0, 10.0)
    E = [(12.0, 0.0, 12.0), (21.0, 0.0, 12.0), (21.0, 0.0, 21.0)]
    # open to closed: in the first state every emitter cell is reached, so its records do not depend on the iterations the
    # module ran before the geometry arrived (the empty grid); from there on the oracle chain carries the unreached cells
    angles = np.linspace(np.pi / 2, 0, 9)
    o = oracle.OracleGrid(25.0, 25.0, 275, boxes)
    base = o.material()
    ef = oracle.free_energy(25.0, 25.0, 275)
    pvlib.Init(pvlib.Config((25.0, 25.0), 275, 0, ".", 0, pvlib.pv_GPU))
    try:
        for b in boxes:
            pvlib.AddGeometry(b)
        pvlib.SetListenerPosition(Lst)
        eids = [pvlib.Emit(e) for e in E]
        sid = pvlib.AddOrientedGeometry(door(angles[0]))
        assert sid == 0
        prev = None
        for k, th in enumerate(angles):
            if k:
                pvlib.UpdateOrientedGeometry(sid, door(th))
            target = pvlib.IterationCount() + 4
            assert pvlib.WaitIterations(target, 120000) >= target
            px, py, w, h, ax, ay, a = door(th)
            b, R = compose(base[0], base[1], [(obb_vertices(px, py, w, h, ax, ay), a)], o.gx, o.gy, o.dx)
            load_material(o, b, R)
            o.fdtd(Lst)
            r, d, _ = o.analyze(ef, Lst, prev=prev)
            prev = r
            for eid, e in zip(eids, E):
                want = r.reshape(-1, 8)[o.result_index(e)]
                assert same_bits(pvlib.GetOutput(eid).as_array(), want).all(), (pipeline, k, e)
        assert pvlib.IsRunning()
    finally:
        pvlib.Exit()
        o.close()
