"""GPU (-m gpu): the zones' ABSOLUTE ensemble decay curves of a sparse-emitter solver (PvAmdSetZoneCurves), accumulated inside the
run off the ring of pressure planes (csrc/pv_zone_decay.hip: the rows kernel over the ring source).

The reference is always a SECOND solver that keeps its history -- the same scene, listener and labels, zone_decay("absolute",
curves=True) -- never the sparse-emitter solver itself.  Tolerance 0: all 64 bytes of every record, etc and edc bit for bit,
NaN == NaN by position."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _zone_decay_ref as zref
import test_gpu_emitter_records as er
from conftest import ROOT, same_bits
from test_gpu_layer import cell_of
from test_gpu_non_square import ABSORBING, MIXED, TILE, both, gid, listeners, solver as rect_solver
from test_gpu_parity import fuse_opts
from test_gpu_room_metrics import SMALLROOM
from test_gpu_zone_stats import five_zones

pytestmark = pytest.mark.gpu

L_ROOM = er.L_ROOM
L_OPEN = (10.0, 0.0, 14.0)

_REF = {}


def reference(key, make, runs, labels, n_zones):
    """(records, etc, edc, res, delay) of the full-history solver make() returns after the listeners `runs`, one after the
    other, under the labels; once per key, read-only"""
    if key not in _REF:
        with make() as s:
            s.set_zones(labels, n_zones)
            for L in runs:
                s.run(L)
            w = s.zone_decay("absolute", curves=True) + s.results()
        for v in w:
            v.setflags(write=False)
        _REF[key] = w
    return _REF[key]


def same_curves(got, want, ctx):
    (r, e, d), (wr, we, wd) = got, want[:3]
    assert r.shape == wr.shape and e.shape == d.shape == we.shape
    bad = e.view(np.uint64) != we.view(np.uint64)
    print("%s: %d zones x %d slots, %d etc values differ" % (ctx, e.shape[0], e.shape[1], bad.sum()))
    assert zref.same_doubles(e, we), "%s etc: first at (zone, slot) %s" % (ctx, np.argwhere(bad)[:4].tolist())
    assert zref.same_doubles(d, wd), "%s edc" % ctx
    assert zref.same_records(r, wr), "%s: %s" % (ctx, zref.first_difference(r, wr))


def curves(st):
    got = st.zone_decay("absolute", curves=True)
    assert zref.same_records(st.zone_decay("absolute"), got[0])  # (without the curves: the same records)
    return got


def smallroom(pvlib, **opts):
    return er.smallroom(pvlib, **opts)


# 1. SmallRoom 70^2, T = 435: several passes, the last one short (three groups and three slots at K = 12); zones across tile
# boundaries and the Y = 64 block boundary, with wall cells, one cell, no cell, and the whole grid
@pytest.mark.parametrize("fuse", [1, 0])
def test_five_zones(pvlib, fuse):
    with smallroom(pvlib, streaming_analysis=1, **fuse_opts(fuse)) as st:
        assert st.info.streamFuse == fuse and (st.gx, st.gy, st.T) == (70, 70, 435)
        lab = five_zones(st)
        want = reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5)
        st.set_zones(lab, 5)
        assert not st.zone_curves()
        st.set_zone_curves(True)
        assert st.zone_curves()
        st.run(L_ROOM)
        got = curves(st)
        same_curves(got, want, "fuse %d" % fuse)
        r, e, _ = got
        assert r["n_cells"][2] == 1 and r["n_cells"][3] == 0 and r["n_cells"][4] > 1000 and (e[3] == 0.0).all()
        assert r["t_first"][2] == r["t_last"][2] > 0 and (e[2, :r["t_first"][2]] == 0.0).all() and (e[2, r["t_first"][2]:] > 0).any()
        beta = st.material()[0][:st.gx, :st.gy]
        assert ((beta == 0) & (lab == 5)).any() or ((beta == 0) & (lab == 1)).any()  # (wall cells inside a zone: never members)
        ms = st.zone_decay("absolute", with_ms=True)[1]
        assert ms > 0


# 2. an open grid of 254^2 at 1000 Hz, T about 1580, fused air tiles: a zone inside tiles that would otherwise be fused, and one far
# from the listener whose onsets fall in a later pass and differ inside one 64-block; the ring wraps a dozen times
def test_open_fused_tiles(pvlib):
    with pvlib.Solver(25.0, 25.0, 1000, streaming_analysis=1, **fuse_opts(1)) as st:
        assert st.info.streamFuse == 1 and st.gx == 254 and 1500 < st.T < 1700
        rxi, wi = st.info.tileRows, st.info.tileCols
        lab = np.zeros((st.gx, st.gy), np.uint8)
        assert (rxi, wi) == (24, 48)
        lab[2 * rxi + 3:3 * rxi + 9, 2 * wi + 5:2 * wi + 31] = 1  # near: air tiles (2, 2) and (3, 2), across a tile-row boundary
        lab[228:251, 197:250] = 2                                 # far: inside the block Y = 192 .. 255, across a tile-column boundary
        flags, box = pvlib.host_zone_tiles(lab, rxi, wi)
        assert flags.sum() == 2 + 4 and box == (2 * rxi + 3, 250, (2 * wi + 5) // 64, 3)
        want = reference("open1000", lambda: pvlib.Solver(25.0, 25.0, 1000), [L_OPEN], lab, 2)
        st.set_zones(lab, 2)
        st.set_zone_curves(True)
        st.run(L_OPEN)
        got = curves(st)
        same_curves(got, want, "254^2")
        r = got[0]
        half = 8 * 8  # (steps per accumulate pass: eight launches of the K = 8 of fuse_opts)
        assert r["n_cells"][0] == (rxi + 6) * 26 and r["n_cells"][1] == 23 * 53
        assert r["t_first"][1] // half > r["t_last"][0] // half          # the far zone's onsets: a later pass
        assert r["t_last"][1] - r["t_first"][1] > 16                      # ... and membership changes inside a 16-slot group
        assert st.T > 12 * 2 * half                                       # the ring wraps many times


# 3. non-square grids in both orientations: a zone on grid row 0, one on grid column 0, an all-wall zone
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R4", [ABSORBING, MIXED], ids=["absorbing", "mixed"])
@pytest.mark.parametrize("g", both(TILE), ids=gid)
def test_non_square(pvlib, g, R4, fuse):
    gx, gy = g
    L = listeners(g)[0]
    with rect_solver(pvlib, g, R4, streaming_analysis=1, **fuse_opts(fuse)) as st:
        assert st.info.streamFuse == fuse
        wall = st.material()[0][:gx, :gy] == 0
        lab = np.zeros(g, np.uint8)
        lab[0, :] = 1
        lab[1:, 0] = 2
        inner = wall.copy()
        inner[0, :] = inner[:, 0] = False
        assert inner.sum() > 10
        lab[inner] = 3
        want = reference(("rect", g, R4), lambda: rect_solver(pvlib, g, R4), [L], lab, 3)
        st.set_zones(lab, 3)
        st.set_zone_curves(True)
        st.run(L)
        got = curves(st)
        same_curves(got, want, "%dx%d %s fuse %d" % (gx, gy, R4, fuse))
        r, e, d = got
        assert r["n_cells"][0] > 0 and r["n_cells"][1] > 0
        assert (r["n_cells"][2], r["t_first"][2], r["t_last"][2]) == (0, -1, -1) and np.isnan(r["edt"][2]) and (e[2] == 0.0).all()


# 3b. 64 one-row zones: every lane of the wave keeps a zone's accumulators
def test_sixty_four_row_zones(pvlib):
    with smallroom(pvlib, streaming_analysis=1) as st:
        lab = np.zeros((st.gx, st.gy), np.uint8)
        for z in range(64):
            lab[3 + z, 1 + (z % 5):st.gy - (z % 3)] = z + 1
        want = reference("smallroom 64 rows", lambda: smallroom(pvlib), [L_ROOM], lab, 64)
        st.set_zones(lab, 64)
        st.set_zone_curves(True)
        st.run(L_ROOM)
        got = curves(st)
        same_curves(got, want, "64 zones")
        assert (got[0]["n_cells"] > 0).sum() > 40


# 4. together with emitters: both features use the tile plane, and either one's change must not drop the other's tiles
def test_with_emitters(pvlib):
    tk, sk = pvlib.QREC_DECAY_TIMES, pvlib.QSPEC_BAND_METRICS
    make = lambda: er.configure(smallroom(pvlib))
    eref = er.reference(pvlib, "smallroom zones", make, L_ROOM, tk, sk)
    cells = [(20, 16), (14, 11), (24, 30)]
    pos = [cell_of(*c) for c in cells]
    with er.configure(smallroom(pvlib, streaming_analysis=1, **fuse_opts(1))) as st:
        lab = five_zones(st)
        lab[lab == 5] = 0  # (not the whole grid: tiles without a labelled cell stay fused)
        want = reference("smallroom four", lambda: smallroom(pvlib), [L_ROOM], lab, 5)
        st.set_emitters(pos)
        st.set_emitter_records(tk, sk)
        st.set_zones(lab, 5)
        st.set_zone_curves(True)
        st.run(L_ROOM)
        er.check(pvlib, st, eref, tk, sk, "emitters and curves")
        same_curves(curves(st), want, "emitters and curves")
        st.set_emitters([])  # rewrites the tile plane: the zones' tiles must survive
        st.run(L_ROOM)
        same_curves(curves(st), want, "emitters cleared")
        st.set_zone_curves(False)  # ... and the emitters' tiles survive this
        st.set_emitters(pos)
        st.run(L_ROOM)
        er.check(pvlib, st, eref, tk, sk, "curves disabled")
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*history"):
            st.zone_decay()
        st.set_zone_curves(True)  # the reverse order: emitters first, then the zones' tiles on top
        st.run(L_ROOM)
        er.check(pvlib, st, eref, tk, sk, "curves enabled again")
        same_curves(curves(st), want, "curves enabled again")


# 5. state between runs: a second listener, and labels changed between runs
def test_state_between_runs(pvlib):
    L2 = cell_of(22, 19)
    with smallroom(pvlib, streaming_analysis=1) as st:
        lab = five_zones(st)
        lab2 = np.zeros_like(lab)
        lab2[5:40, 10:66] = 1
        lab2[41:69, 0:20] = 2
        first = reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5)
        second = reference("smallroom five, L2", lambda: smallroom(pvlib), [L_ROOM, L2], lab, 5)
        third = reference("smallroom two, L2 twice", lambda: smallroom(pvlib), [L_ROOM, L2, L2], lab2, 2)
        st.set_zones(lab, 5)
        st.set_zone_curves(True)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: no completed run"):
            st.zone_decay()
        st.run(L_ROOM)
        same_curves(curves(st), first, "first run")
        st.run_async(L2)  # (the call waits for the run in flight)
        same_curves(curves(st), second, "second listener")
        assert not zref.same_doubles(second[1], first[1])
        st.set_zones(lab2, 2)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: the last run was enqueued before"):
            st.zone_decay()
        st.run(L2)
        same_curves(curves(st), third, "new labels")


# 6. the run is otherwise untouched: result map, onset map and get_output with and without the curves
def test_results_unchanged(pvlib):
    g = TILE
    L = listeners(g)[0]
    pos = [cell_of(100, 120), cell_of(30, 200)]
    with rect_solver(pvlib, g, MIXED, streaming_analysis=1, **fuse_opts(1)) as st:
        lab = np.zeros(g, np.uint8)
        lab[60:130, 50:170] = 1
        lab[200:240, 10:60] = 2
        st.set_emitters(pos)
        st.run(L)
        plain = st.results() + tuple(st.get_output(p).as_array() for p in pos)
        st.set_zones(lab, 2)  # (labels alone change nothing)
        st.run(L)
        for a, b in zip(plain, st.results() + tuple(st.get_output(p).as_array() for p in pos)):
            assert same_bits(a, b).all()
        st.set_zone_curves(True)
        st.run(L)
        with_curves = st.results() + tuple(st.get_output(p).as_array() for p in pos)
        for a, b in zip(plain, with_curves):
            assert same_bits(a, b).all()
        assert (plain[1] < 1e30).sum() > 1000
        assert (st.zone_decay()["n_cells"] > 0).all()


# 7. refusals, each by its prefix and key word; the command line
def test_refusals(pvlib):
    with smallroom(pvlib) as s:  # a solver that keeps its history
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        with pytest.raises(pvlib.PlaneverbError, match="^zone curves: sparse-emitter solvers only"):
            s.set_zone_curves(True)
        assert not s.zone_curves()
    with pvlib.Solver(25.0, 25.0, 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^zone curves: .*slab"):
            s.set_zone_curves(True)
    with smallroom(pvlib, streaming_analysis=1, skip_analysis=1) as s:
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*onset map"):
            s.zone_decay()
    with smallroom(pvlib, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^zone curves: no zones set \\(PvAmdSetZones\\)"):
            s.set_zone_curves(True)
        s.set_zone_curves(False)  # (nothing to stop: fine)
        lab = five_zones(s)
        s.set_zones(lab, 5)
        got, n = s.zones()
        assert n == 5 and np.array_equal(got, lab)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*history.*PvAmdSetZoneCurves"):
            s.zone_decay()
        s.run(L_ROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*history.*PvAmdSetZoneCurves"):
            s.zone_decay()
        s.set_zone_curves(True)
        s.set_zone_curves(True)  # (twice: nothing changes)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: the last run was enqueued before the zone curves were enabled"):
            s.zone_decay()
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: onset-synchronised curves need the full pressure history"):
            s.zone_decay("onset")
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: the zones cannot be cleared while the zone curves are enabled"):
            s.set_zones(None)
        assert s.zones()[1] == 5 and s.zone_curves()
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: .*history"):
            s.zone_stats("decay_times")
        s.set_bands([125.0], 1)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: .*history"):
            s.zone_band_decay()
        # ... and the solver works afterwards
        s.run(L_ROOM)
        same_curves(curves(s), reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5), "after the refusals")
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: onset-synchronised"):
            s.zone_decay("onset")
        s.set_zone_curves(False)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*history"):
            s.zone_decay()
        s.set_zones(None)  # (allowed again)
        assert s.zones() == (None, 0)
    lib = pvlib.lib()
    on = pvlib.C.c_int(7)
    assert lib.PvAmdSetZoneCurves(None, 1) == -1 and pvlib.last_error() == "zone curves: null solver handle"
    assert lib.PvAmdGetZoneCurves(None, pvlib.C.byref(on)) == -1 and pvlib.last_error() == "zone curves: null solver handle"
    assert on.value == 7


def test_cli(pvlib):
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4", "--emitter", "5,0,6", "--zone", "2,2,9,8",
           "--zone", "12,3,20,20", "--zone-decay", "absolute", "--zone-decay-curves"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def zones(*more):
        out = subprocess.run(cmd + list(more), capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout
        return json.loads(out)["zones"]

    a, b = zones(), zones("--sparse-emitters")
    assert len(a) == len(b) == 2 and a[0]["zoneDecay"]["nCells"] > 100 and len(a[0]["zoneDecay"]["etc"]) == 435
    assert json.dumps(a) == json.dumps(b)
    bad = subprocess.run(cmd[:-1] + ["--sparse-emitters", "--zone-decay", "onset"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert bad.returncode != 0 and "--zone-decay absolute" in bad.stderr
