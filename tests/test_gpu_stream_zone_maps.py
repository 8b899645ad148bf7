"""GPU (-m gpu): the room-metrics and spectrum maps of the zones of a sparse-emitter solver (PvAmdSetZoneMaps), accumulated inside the
run off the ring of pressure planes (csrc/pv_zone_maps.hip) in the kinds' own maps.

The reference is always a SECOND solver that keeps its history -- the same scene, listener, labels and bins, compute_room_metrics()
/ compute_spectrum() and zone_stats -- never the sparse-emitter solver itself.  Tolerance 0: every float of every labelled cell's
record by bit pattern (NaN == NaN by position), every unlabelled cell NaN, all 64 bytes of every PvAmdZoneStat."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_emitter_records as er
import test_gpu_stream_zone_decay as zd
from conftest import ROOT
from test_gpu_layer import cell_of
from test_gpu_non_square import ABSORBING, MIXED, TILE, both, gid, listeners, solver as rect_solver
from test_gpu_parity import fuse_opts
from test_gpu_room_metrics import SMALLROOM
from test_gpu_zone_stats import five_zones

pytestmark = pytest.mark.gpu

L_ROOM, L_OPEN = zd.L_ROOM, zd.L_OPEN
BINS3 = [50.0, 100.0, 137.5]
BINS17 = [20.0 + 11.5 * j for j in range(17)]  # (two register blocks: 16 + 1)
NO_ONSET = 1e30

_REF = {}


def reference(key, make, runs, labels, n_zones, bins):
    """{"rm", "sp": the maps [gx, gy, ..]; "zrm", "zsp": the zone statistics; "res", "delay"} of the full-history solver make() returns
    after the listeners `runs`, one after the other (a callable among them: applied to the solver, e.g. more geometry), under the
    labels and bins; once per key, read-only"""
    if key not in _REF:
        with make() as s:
            s.set_zones(labels, n_zones)
            s.set_spectrum_bins(bins)
            for L in runs:
                L(s) if callable(L) else s.run(L)
            s.compute_room_metrics()
            s.compute_spectrum()
            res, delay = s.results()
            w = dict(rm=s.room_metrics(), sp=s.spectrum(), zrm=s.zone_stats("room_metrics"), zsp=s.zone_stats("spectrum"), res=res, delay=delay)
        for v in w.values():
            v.setflags(write=False)
        _REF[key] = w
    return _REF[key]


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def same_map(got, want, lab, ctx):
    assert got.shape == want.shape, ctx
    on = lab != 0
    g, w = got.reshape(lab.shape + (-1,)), want.reshape(lab.shape + (-1,))
    bad = ~bits_equal(g[on], w[on])
    print("%s: %d labelled cells x %d floats, %d differ; %d unlabelled cells" % (ctx, on.sum(), g.shape[-1], bad.sum(), (~on).sum()))
    assert not bad.any(), "%s: first at (labelled cell, float) %s: %s / %s" % (
        ctx, np.argwhere(bad)[:4].tolist(), g[on][bad][:4], w[on][bad][:4])
    assert np.isnan(g[~on]).all(), "%s: an unlabelled cell is not NaN" % ctx


def same_stats(got, want, ctx):
    assert got.shape == want.shape and got.dtype == want.dtype, ctx
    assert got.tobytes() == want.tobytes(), "%s: zone statistics differ at %s" % (
        ctx, np.argwhere(got.reshape(-1).view(np.uint8).reshape(-1, 64) != want.reshape(-1).view(np.uint8).reshape(-1, 64))[:4].tolist())


def check(pvlib, st, want, lab, kinds, ctx):
    assert st.zone_maps() == kinds
    if kinds & pvlib.ZMAP_ROOM_METRICS:
        same_map(st.room_metrics(), want["rm"], lab, ctx + " room metrics")
        same_stats(st.zone_stats("room_metrics"), want["zrm"], ctx + " room metrics")
    if kinds & pvlib.ZMAP_SPECTRUM:
        same_map(st.spectrum(), want["sp"], lab, ctx + " spectrum")
        same_stats(st.zone_stats("spectrum"), want["zsp"], ctx + " spectrum")


def smallroom(pvlib, **opts):
    return er.smallroom(pvlib, **opts)


def both_kinds(pvlib):
    return pvlib.ZMAP_ROOM_METRICS | pvlib.ZMAP_SPECTRUM


# 1. SmallRoom 70^2, T = 435: several wraps of the ring, the last pass short; the five zones of the zone statistics' test
@pytest.mark.parametrize("kinds", [1, 2, 3], ids=["room_metrics", "spectrum", "both"])
@pytest.mark.parametrize("fuse", [1, 0])
def test_five_zones(pvlib, fuse, kinds):
    with smallroom(pvlib, streaming_analysis=1, **fuse_opts(fuse)) as st:
        assert st.info.streamFuse == fuse and (st.gx, st.gy, st.T) == (70, 70, 435)
        lab = five_zones(st)
        want = reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5, BINS3)
        st.set_zones(lab, 5)
        st.set_spectrum_bins(BINS3)
        assert st.zone_maps() == 0
        st.set_zone_maps(kinds)
        st.run(L_ROOM)
        check(pvlib, st, want, lab, kinds, "fuse %d" % fuse)
        beta = st.material()[0][:st.gx, :st.gy]
        assert ((beta == 0) & (lab != 0)).any() and np.isnan(want["rm"][(beta == 0)]).all()  # (wall cells inside a zone: NaN records)
        assert np.isfinite(want["rm"][..., 0]).sum() > 1000
        # the other read-backs serve the same map
        if kinds & pvlib.ZMAP_ROOM_METRICS:
            assert bits_equal(st.room_metrics_block(8, 30, 5, 9), want["rm"][8:13, 30:39]).all()
            assert bits_equal(st.room_metrics_at(cell_of(20, 40)), want["rm"][20, 40]).all()
        if kinds & pvlib.ZMAP_SPECTRUM:
            assert bits_equal(st.spectrum_block(8, 30, 5, 9), want["sp"][8:13, 30:39]).all()
            assert bits_equal(st.spectrum_at(cell_of(20, 40)), want["sp"][20, 40]).all()


# 2. an open grid of 254^2 at 1000 Hz, T about 1580, fused air tiles: a zone inside tiles that would otherwise be fused, across a
# tile-row boundary, and one far from the listener whose onsets fall in a later pass and differ inside one row; 17 bins
def test_open_fused_tiles(pvlib):
    with pvlib.Solver(25.0, 25.0, 1000, streaming_analysis=1, **fuse_opts(1)) as st:
        assert st.info.streamFuse == 1 and st.gx == 254 and 1500 < st.T < 1700
        rxi, wi = st.info.tileRows, st.info.tileCols
        assert (rxi, wi) == (24, 48)
        lab = np.zeros((st.gx, st.gy), np.uint8)
        lab[2 * rxi + 3:3 * rxi + 9, 2 * wi + 5:2 * wi + 31] = 1
        lab[228:251, 197:250] = 2
        want = reference("open1000", lambda: pvlib.Solver(25.0, 25.0, 1000), [L_OPEN], lab, 2, BINS17)
        half = 8 * 8  # (steps per accumulate pass: eight launches of the K = 8 of fuse_opts)
        d = want["delay"]
        assert (d[lab != 0] < NO_ONSET).all()
        assert d[lab == 2].min() // half > d[lab == 1].max() // half          # the far zone's first onset: a later pass
        assert (d[lab == 2].reshape(23, 53).max(1) > d[lab == 2].reshape(23, 53).min(1)).all()  # ... and they differ inside every row
        st.set_zones(lab, 2)
        st.set_spectrum_bins(BINS17)
        st.set_zone_maps(both_kinds(pvlib))
        st.run(L_OPEN)
        check(pvlib, st, want, lab, both_kinds(pvlib), "254^2")


# 3. late onsets: a run cut short, so that labelled cells have an empty late window (l50 == 0, c50 = +inf, d50 = 1) and onsets in the
# last accumulate pass
def test_late_onsets(pvlib):
    T = 290
    with pvlib.Solver(25.0, 25.0, 1000, streaming_analysis=1, num_steps=T, **fuse_opts(1)) as st:
        assert st.T == T and st.info.streamFuse == 1
        lab = np.zeros((st.gx, st.gy), np.uint8)
        lab[95:110, 135:150] = 1   # around the listener: both windows filled
        lab[228:254, 0:40] = 2     # the far corner: reached late or not at all
        want = reference("open1000 short", lambda: pvlib.Solver(25.0, 25.0, 1000, num_steps=T), [L_OPEN], lab, 2, BINS3)
        half = 8 * 8
        last = (T - 1) // half * half
        rm, d = want["rm"], want["delay"]
        on = lab != 0
        empty = on & (rm[..., 5] == 0) & np.isposinf(rm[..., 0]) & (rm[..., 2] == 1)
        assert empty.any() and (on & (d >= last) & (d < T)).any() and (on & (d >= NO_ONSET)).any() and (on & (rm[..., 5] > 0)).any()
        st.set_zones(lab, 2)
        st.set_spectrum_bins(BINS3)
        st.set_zone_maps(both_kinds(pvlib))
        st.run(L_OPEN)
        check(pvlib, st, want, lab, both_kinds(pvlib), "T = %d" % T)


# 4. the 252 x 280 and 280 x 252 tile forms with absorbing and mixed edges: zones on grid row 0 and grid column 0, an all-wall zone
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
        want = reference(("rect", g, R4), lambda: rect_solver(pvlib, g, R4), [L], lab, 3, BINS3)
        st.set_zones(lab, 3)
        st.set_spectrum_bins(BINS3)
        st.set_zone_maps(both_kinds(pvlib))
        st.run(L)
        ctx = "%dx%d %s fuse %d" % (gx, gy, R4, fuse)
        check(pvlib, st, want, lab, both_kinds(pvlib), ctx)
        assert np.isnan(st.room_metrics()[lab == 3]).all() and np.isnan(st.spectrum()[lab == 3]).all()
        z = st.zone_stats("room_metrics")
        assert (z["n_nan"][2] == inner.sum()).all() and (z["n_finite"][2] == 0).all() and (z["n_finite"][0] > 0).any()


# 5. state between runs on ONE solver: cells reached in the first run and not in the second, then new labels, then new bins
def test_state_between_runs(pvlib):
    L2 = (7.0, 0.0, 9.5)

    def walls(s):  # four walls around L2: the second listener is walled in
        for b in ((5.8, 9.5, 0.8, 3.4, 0.5), (8.2, 9.5, 0.8, 3.4, 0.5), (7.0, 8.2, 3.2, 0.8, 0.5), (7.0, 10.8, 3.2, 0.8, 0.5)):
            s.add_geometry(b)

    with smallroom(pvlib, streaming_analysis=1) as st:
        lab = five_zones(st)
        lab2 = np.zeros_like(lab)
        lab2[5:40, 10:66] = 1
        lab2[41:69, 0:20] = 2
        bins2 = [31.5, 63.0, 125.0, 250.0]
        first = reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5, BINS3)
        second = reference("smallroom five, walled L2", lambda: smallroom(pvlib), [L_ROOM, walls, L2], lab, 5, BINS3)
        third = reference("smallroom two, walled", lambda: smallroom(pvlib), [L_ROOM, walls, L2, L_ROOM], lab2, 2, BINS3)
        fourth = reference("smallroom two, walled, bins2", lambda: smallroom(pvlib), [walls, L_ROOM], lab2, 2, bins2)
        lost = (first["delay"] < NO_ONSET) & (second["delay"] >= NO_ONSET) & (lab != 0)
        assert 4 <= (second["delay"] < NO_ONSET).sum() < 200 and lost.sum() > 1000
        assert np.isnan(second["rm"][lost]).all() and np.isfinite(first["rm"][lost][:, 4:]).all()
        st.set_zones(lab, 5)
        st.set_spectrum_bins(BINS3)
        st.set_zone_maps(both_kinds(pvlib))
        st.run(L_ROOM)
        check(pvlib, st, first, lab, both_kinds(pvlib), "first run")
        walls(st)
        st.run_async(L2)  # (the read-backs wait for the run in flight)
        check(pvlib, st, second, lab, both_kinds(pvlib), "walled-in listener")
        assert np.isnan(st.room_metrics()[lost]).all() and np.isnan(st.spectrum()[lost]).all()
        st.set_zones(lab2, 2)
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: the last run was enqueued before"):
            st.room_metrics()
        st.run(L_ROOM)
        check(pvlib, st, third, lab2, both_kinds(pvlib), "new labels")
        assert ((lab != 0) & (lab2 == 0)).any() and np.isnan(st.room_metrics()[lab2 == 0]).all()
        st.set_spectrum_bins(bins2)
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: the last run was enqueued before"):
            st.spectrum()
        same_map(st.room_metrics(), third["rm"], lab2, "new bins: the room metrics stay")
        st.run(L_ROOM)
        check(pvlib, st, fourth, lab2, both_kinds(pvlib), "new bins")


# 6. together with the zone curves and registered emitters with their records: each equals its reference, and selecting or
# deselecting either side drops nobody's tiles
def test_with_curves_and_emitters(pvlib):
    tk, sk = pvlib.QREC_DECAY_TIMES, pvlib.QSPEC_BAND_METRICS
    eref = er.reference(pvlib, "smallroom zones", lambda: er.configure(smallroom(pvlib)), L_ROOM, tk, sk)
    pos = [cell_of(*c) for c in [(20, 16), (14, 11), (24, 30)]]
    with er.configure(smallroom(pvlib, streaming_analysis=1, **fuse_opts(1))) as st:
        lab = five_zones(st)
        lab[lab == 5] = 0  # (not the whole grid: tiles without a labelled cell stay fused)
        bins = list(st.spectrum_bins())  # (er.configure's)
        want = reference("smallroom four", lambda: smallroom(pvlib), [L_ROOM], lab, 5, bins)
        cwant = zd.reference("smallroom four", lambda: smallroom(pvlib), [L_ROOM], lab, 5)
        K = both_kinds(pvlib)
        st.set_emitters(pos)
        st.set_emitter_records(tk, sk)
        st.set_zones(lab, 5)
        st.set_zone_curves(True)
        st.set_zone_maps(K)
        st.run(L_ROOM)
        er.check(pvlib, st, eref, tk, sk, "all three")
        zd.same_curves(zd.curves(st), cwant, "all three")
        check(pvlib, st, want, lab, K, "all three")
        st.set_zone_curves(False)  # the maps' tiles survive
        st.set_emitters([])
        st.run(L_ROOM)
        check(pvlib, st, want, lab, K, "curves off, emitters cleared")
        st.set_zone_curves(True)
        st.set_zone_maps(0)        # ... and the curves' tiles survive this
        assert st.zone_maps() == 0
        st.set_emitters(pos)
        st.run(L_ROOM)
        zd.same_curves(zd.curves(st), cwant, "maps off")
        er.check(pvlib, st, eref, tk, sk, "maps off")
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: not computed"):
            st.room_metrics()
        st.set_zone_maps(pvlib.ZMAP_SPECTRUM)  # the reverse order: curves first, then a map kind on top
        st.run(L_ROOM)
        zd.same_curves(zd.curves(st), cwant, "spectrum on top")
        check(pvlib, st, want, lab, pvlib.ZMAP_SPECTRUM, "spectrum on top")
        st.set_zone_curves(False)
        st.set_zone_maps(K)
        st.run(L_ROOM)
        check(pvlib, st, want, lab, K, "both kinds, curves off")
        er.check(pvlib, st, eref, tk, sk, "both kinds, curves off")


# 7. the run is otherwise untouched: result map, onset map and get_output with and without a kind selected
def test_results_unchanged(pvlib):
    g = TILE
    L = listeners(g)[0]
    pos = [cell_of(100, 120), cell_of(30, 200)]
    with rect_solver(pvlib, g, MIXED, streaming_analysis=1, **fuse_opts(1)) as st:
        lab = np.zeros(g, np.uint8)
        lab[60:130, 50:170] = 1
        lab[200:240, 10:60] = 2
        st.set_emitters(pos)
        st.set_zones(lab, 2)
        st.set_spectrum_bins(BINS3)
        st.run(L)
        plain = st.results() + tuple(st.get_output(p).as_array() for p in pos)
        st.set_zone_maps(both_kinds(pvlib))
        st.run(L)
        for a, b in zip(plain, st.results() + tuple(st.get_output(p).as_array() for p in pos)):
            assert bits_equal(a, b).all()
        assert (plain[1] < NO_ONSET).sum() > 1000 and np.isfinite(st.room_metrics()[lab != 0][:, 4:]).any()


# 8. refusals, each by its prefix and key word
def test_refusals(pvlib):
    RM, SP = pvlib.ZMAP_ROOM_METRICS, pvlib.ZMAP_SPECTRUM
    lib = pvlib.lib()
    k = pvlib.C.c_uint(7)
    assert lib.PvAmdSetZoneMaps(None, 1) == -1 and pvlib.last_error() == "zone maps: null solver handle"
    assert lib.PvAmdGetZoneMaps(None, pvlib.C.byref(k)) == -1 and pvlib.last_error() == "zone maps: null solver handle" and k.value == 7
    with smallroom(pvlib) as s:  # a solver that keeps its history
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: sparse-emitter solvers only.*PvAmdCompute"):
            s.set_zone_maps(RM)
        assert s.zone_maps() == 0
    with pvlib.Solver(25.0, 25.0, 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: .*slab"):
            s.set_zone_maps(RM)
    with smallroom(pvlib, streaming_analysis=1, skip_analysis=1) as s:
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: .*onset map"):
            s.set_zone_maps(RM)
    with smallroom(pvlib, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: kinds is a combination"):
            s.set_zone_maps(4)
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: no zones set \\(PvAmdSetZones\\)"):
            s.set_zone_maps(RM)
        s.set_zone_maps(0)  # (nothing to deselect: fine)
        lab = five_zones(s)
        s.set_zones(lab, 5)
        with pytest.raises(pvlib.PlaneverbError, match="^zone maps: PVA_ZMAP_SPECTRUM: no bins set"):
            s.set_zone_maps(RM | SP)
        assert s.zone_maps() == 0
        # nothing selected: today's refusals
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: not computed for the last run"):
            s.room_metrics()
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: the full pressure history is not kept"):
            s.zone_stats("room_metrics")
        s.run(L_ROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: not computed for the last run"):
            s.room_metrics()
        s.set_zone_maps(RM)
        s.set_zone_maps(RM)  # (twice: nothing changes)
        # the stamps: selected after the last run was enqueued
        for call in (s.room_metrics, lambda: s.room_metrics_block(0, 0, 2, 2), lambda: s.room_metrics_at(cell_of(20, 16))):
            with pytest.raises(pvlib.PlaneverbError, match="^room metrics: the last run was enqueued before the kind was selected"):
                call()
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: room metrics: the last run was enqueued before"):
            s.zone_stats("room_metrics")
        # the compute calls keep refusing, naming the history; so do the other kinds and their statistics
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: the full pressure history is not kept"):
            s.compute_room_metrics()
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: no bins set"):
            s.spectrum()
        s.set_spectrum_bins(BINS3)
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: the full pressure history is not kept"):
            s.compute_spectrum()
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: not computed for the last run"):
            s.spectrum()  # (not selected)
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: .*history"):
            s.zone_stats("spectrum")
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: .*history"):
            s.zone_stats("decay_times")
        with pytest.raises(pvlib.PlaneverbError, match="^decay times: .*history"):
            s.compute_decay_times()
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: the zones cannot be cleared while a zone map kind is selected"):
            s.set_zones(None)
        s.set_zone_maps(RM | SP)
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: the bins cannot be cleared while PVA_ZMAP_SPECTRUM is selected"):
            s.set_spectrum_bins([])
        assert s.zone_maps() == RM | SP and len(s.spectrum_bins()) == 3 and s.zones()[1] == 5
        # ... and the solver works afterwards; then new labels and new bins refuse the old maps
        want = reference("smallroom five", lambda: smallroom(pvlib), [L_ROOM], lab, 5, BINS3)
        s.run(L_ROOM)
        check(pvlib, s, want, lab, RM | SP, "after the refusals")
        s.set_zones(lab, 5)
        with pytest.raises(pvlib.PlaneverbError, match="^spectrum: the last run was enqueued before"):
            s.spectrum()
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: the last run was enqueued before"):
            s.room_metrics()
        s.run(L_ROOM)
        s.set_spectrum_bins(BINS3)
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: spectrum: the last run was enqueued before"):
            s.zone_stats("spectrum")
        same_map(s.room_metrics(), want["rm"], lab, "new bins: the room metrics stay")
        s.set_zone_maps(0)
        with pytest.raises(pvlib.PlaneverbError, match="^room metrics: not computed for the last run"):
            s.room_metrics()
        s.set_spectrum_bins([])
        s.set_zones(None)  # (allowed again)
        assert s.zones() == (None, 0)


# 9. the command line: the zone tables of a sparse-emitter run are those of a run that keeps its history
def test_cli(pvlib):
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4", "--emitter", "5,0,6", "--zone", "2,2,9,8",
           "--room-metrics", "--spectrum", "50,100"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def zones(*more):
        out = subprocess.run(cmd + list(more), capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout
        return json.loads(out)["zones"]

    a, b = zones(), zones("--sparse-emitters")
    assert len(a) == len(b) == 1 and a[0]["roomMetrics"]["c50"]["n"] > 100 and len(a[0]["spectrum"]) == 6
    assert json.dumps(a) == json.dumps(b)
