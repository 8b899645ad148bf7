"""GPU (-m gpu): baked probe tables (include/planeverb_amd.h Part 4) against the runs they come from.

* every baked block equals what a FRESH solver's run at that probe holds on the block's nodes (all 8 members and the onset, bit for
  bit), the reached flags agree, and no reached lattice node lies outside the block -- in the resident kernel (the reference's
  preset grid), the replayed graph, a merged-kernel grid whose history window is smaller than the grid, a scene with oriented
  boxes; probes inside a wall or outside the grid are invalid (state 2);
* a solver that carried records from an earlier run bakes the same file as fresh solvers;
* one solver, two solvers and two merged rank halves save byte-identical files;
* a query at a probe position and a reached lattice node equals PvAmdGetOutput of that probe's run;
* PvAmdBakeQueryDevice equals PvAmdBakeQuery bit for bit;
* refusals: sparse-emitter mode, slab groups, another grid or T, a material changed after PvAmdBakeCreate.
"""
import os

import numpy as np
import pytest

from conftest import SCENES, same_bits
from test_gpu_analysis_edges import DX, open_size

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")


def probe_pos(b, k):
    i = b.info()
    x = np.float32(i["x0"]) + np.float32(k % i["nx"]) * np.float32(i["sx"])
    z = np.float32(i["z0"]) + np.float32(k // i["nx"]) * np.float32(i["sz"])
    return (float(x), 0.0, float(z))


def check_against_fresh(pvlib, bake, make, expect_invalid=()):
    """every probe of `bake` against a fresh solver's run (make() -> configured solver)"""
    info = bake.info()
    d = info["stride"]
    states = []
    for k in range(info["nx"] * info["nz"]):
        st, rec = bake.probe(k)
        states.append(int(st[0]))
        if k in expect_invalid:
            assert st[0] == 2 and st[3] == 0, (k, st)
        if st[0] != 1:
            continue
        with make() as s:
            s.run(probe_pos(bake, k))
            res, delay = s.results()
        lat_res, lat_delay = res[::d, ::d], delay[::d, ::d]
        reached = lat_delay < FLT_MAX
        i0, j0, ni, nj = (int(v) for v in st[1:])
        inside = np.zeros_like(reached)
        inside[i0:i0 + ni, j0:j0 + nj] = True
        assert not (reached & ~inside).any(), "probe %d: reached nodes outside the block" % k
        if ni == 0:
            continue
        blk_res, blk_delay = lat_res[i0:i0 + ni, j0:j0 + nj], lat_delay[i0:i0 + ni, j0:j0 + nj]
        r = blk_delay < FLT_MAX
        assert r.any() and np.array_equal(rec[..., 8] < FLT_MAX, r), "probe %d: reached flags" % k
        assert same_bits(rec[..., 8][r], blk_delay[r]).all(), "probe %d: onsets" % k
        for m in range(8):
            bad = ~same_bits(rec[..., m][r], blk_res[..., m][r])
            assert not bad.any(), "probe %d member %d: %d nodes differ" % (k, m, bad.sum())
        assert not rec[~r][:, :8].any() and (rec[~r][:, 8] == FLT_MAX).all()
    assert 1 in states, states
    return states


def _bake(pvlib, solvers, lattice, **kw):
    b = pvlib.Bake(solvers[0], *lattice)
    b.run(solvers, **kw)
    return b


def test_smallroom_resident_with_invalid_probes(pvlib):
    # 25 m SmallRoomScene at 275 Hz (the resident kernel); the last column of probes lies outside the grid
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 6, 5)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        b = _bake(pvlib, [s], lattice)
        beta, _ = s.material()

    def make():
        t = pvlib.Solver(25.0, 25.0, 275)
        t.load_scene(SMALLROOM)
        return t

    gx = b.info()["gx"]
    invalid = set()
    for k in range(30):
        x, _, z = probe_pos(b, k)
        cx, cy = int(np.float32(x) / np.float32(b.info()["dx"])), int(np.float32(z) / np.float32(b.info()["dx"]))
        if cx >= gx or cy >= gx or beta[cx, cy] == 0:
            invalid.add(k)
    assert invalid
    check_against_fresh(pvlib, b, make, invalid)
    assert b.info()["probesInvalid"] == len(invalid)


def test_replayed_graph_grid_with_wall_probe(pvlib):
    size = open_size(300)
    wall = (5.0, 5.0, 1.0, 1.0, 0.5)  # centred on probe (1, 1)
    lattice = (4, 3.0, 3.0, 2.0, 2.0, 3, 3)

    def make():
        t = pvlib.Solver(size, size, 275, resident_kernel=2)
        t.add_geometry(wall)
        return t

    with make() as s:
        b = _bake(pvlib, [s], lattice)
    check_against_fresh(pvlib, b, make, expect_invalid={4})


def test_merged_kernel_window_smaller_than_grid(pvlib):
    size = open_size(520)
    lattice = (5, 10.0, 10.0, 10.0, 10.0, 3, 3)

    def make():
        return pvlib.Solver(size, size, 275, num_steps=200)

    with make() as s:
        assert s.info.histRows < s.gx
        b = _bake(pvlib, [s], lattice)
    check_against_fresh(pvlib, b, make)


def test_oriented_boxes(pvlib):
    lattice = (3, 4.0, 4.0, 4.0, 4.0, 4, 4)

    def make():
        t = pvlib.Solver(25.0, 25.0, 275)
        t.load_scene(SMALLROOM)
        t.add_oriented_box(12.0, 8.0, 6.0, 0.5, 1.0, 0.6, 0.3)
        t.add_oriented_box(7.0, 16.0, 4.0, 0.4, -0.3, 1.0, 0.9)
        return t

    with make() as s:
        b = _bake(pvlib, [s], lattice)
    check_against_fresh(pvlib, b, make)


def test_no_carried_records_and_dealing(pvlib, tmp_path):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 4, 4)
    paths = {}
    with pvlib.Solver(25.0, 25.0, 275) as a, pvlib.Solver(25.0, 25.0, 275) as c:
        for s in (a, c):
            s.load_scene(SMALLROOM)
        b = _bake(pvlib, [a], lattice)
        paths["fresh"] = str(tmp_path / "fresh.pvbake")
        b.save(paths["fresh"])
        # c first runs a listener elsewhere (its map then carries those records), then bakes
        c.run((20.0, 0.0, 20.0))
        b2 = _bake(pvlib, [c], lattice)
        paths["carried"] = str(tmp_path / "carried.pvbake")
        b2.save(paths["carried"])
        # two solvers, two rank halves merged
        b3 = _bake(pvlib, [a, c], lattice)
        paths["two"] = str(tmp_path / "two.pvbake")
        b3.save(paths["two"])
        h0 = _bake(pvlib, [a], lattice, rank=0, world=2)
        h1 = _bake(pvlib, [c, a], lattice, rank=1, world=2)
        h0.merge(h1)
        paths["merged"] = str(tmp_path / "merged.pvbake")
        h0.save(paths["merged"])
    want = open(paths["fresh"], "rb").read()
    for k in ("carried", "two", "merged"):
        assert open(paths[k], "rb").read() == want, k


def test_anchor_query_equals_get_output(pvlib):
    lattice = (3, 3.125, 3.125, 4.5, 4.5, 3, 3)  # multiples of 1/8 m
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        b = _bake(pvlib, [s], lattice)
        d = b.info()["stride"]
        checked = 0
        for k in range(9):
            st, rec = b.probe(k)
            if st[0] != 1 or st[3] == 0:
                continue
            L = probe_pos(b, k)
            s.run(L)
            idx = np.argwhere(rec[..., 8] < FLT_MAX)
            rng = np.random.default_rng(k)
            for ii, jj in idx[rng.choice(len(idx), min(20, len(idx)), replace=False)]:
                r, c = (int(st[1]) + ii) * d, (int(st[2]) + jj) * d
                E = (float((np.float32(r) + np.float32(0.5)) * DX), 0.0, float((np.float32(c) + np.float32(0.5)) * DX))
                got = b.query([L], [E])[0]
                want = s.get_output(E).as_array()
                assert same_bits(got, want).all(), (k, r, c, got, want)
                checked += 1
        assert checked >= 20


def test_device_query_equals_host_query(pvlib):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 4, 4)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        b = _bake(pvlib, [s], lattice)
    rng = np.random.default_rng(5)
    n = 1_000_000
    L = np.zeros((n, 3), np.float32)
    E = np.zeros((n, 3), np.float32)
    L[:, 0], L[:, 2] = rng.uniform(-2, 27, n), rng.uniform(-2, 27, n)
    E[:, 0], E[:, 2] = rng.uniform(-1, 26, n), rng.uniform(-1, 26, n)
    host = b.query(L, E)
    dev = b.query_device(L, E, 0)
    bad = ~same_bits(host, dev).all(axis=1)
    assert not bad.any(), (bad.sum(), host[bad][0], dev[bad][0])
    assert (host[:, 0] != -1).sum() > n // 4
    assert same_bits(b.query_device(L[:1000], E[:1000], 0), host[:1000]).all()  # cached upload


def test_refusals(pvlib):
    lattice = (2, 2.5, 2.5, 5.0, 5.0, 2, 2)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        b = pvlib.Bake(s, *lattice)
        with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as t:
            t.load_scene(SMALLROOM)
            with pytest.raises(pvlib.PlaneverbError, match="sparse-emitter"):
                b.run([t])
        with pvlib.Solver(25.0, 25.0, 275, slabs=[0, 0]) as t:
            with pytest.raises(pvlib.PlaneverbError, match="slab"):
                b.run([t])
        for kw in (dict(num_steps=300), dict()):
            with pvlib.Solver(25.0, 25.0, 300 if not kw else 275, **kw) as t:
                t.load_scene(SMALLROOM)
                with pytest.raises(pvlib.PlaneverbError, match="another grid"):
                    b.run([t])
        s.add_geometry((12.0, 12.0, 1.0, 1.0, 0.5))
        with pytest.raises(pvlib.PlaneverbError, match="material"):
            b.run([s])
        assert b.info()["probesBaked"] == 0
