"""GPU (-m gpu): per-zone ensemble decay curves and decay times (PvAmdComputeZoneDecay, csrc/pv_zone_decay.hip).

Every comparison is bit for bit -- etc, edc and all 64 bytes of a record, NaNs by position -- against the host restatement
api.host_zone_decay fed the SAME solver's recorded planes (history_plane(t)[:gx, :gy] for all t) and its own onset map; the host
restatement itself is held to an independent numpy restatement and to exact sums in tests/test_zone_decay_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import _zone_decay_ref as ref
import test_gpu_analysis_maps as maps
import test_gpu_non_square as ns
from conftest import golden
from test_gpu_analysis_edges import open_size
from test_gpu_analysis_maps import BY_NAME, LISTENER, compute, identical, whole
from test_gpu_lateral import preset_solver
from test_gpu_query_records import BOXES4, L_IN
from test_gpu_room_metrics import L400, N400, SMALLROOM
from test_gpu_zone_stats import five_zones, scattered

pytestmark = pytest.mark.gpu

ALIGNS = ["absolute", "onset"]


def history(s):
    return np.stack([s.history_plane(t)[:s.gx, :s.gy] for t in range(s.T)])


def check(pvlib, s, labels, n_zones, ctx, aligns=ALIGNS, p=None):
    """zone_decay of the last run against the host restatement of its planes and onsets; {align: (records, etc, edc)}, p, delay"""
    p = history(s) if p is None else p
    delay = s.results()[1]
    out = {}
    for align in aligns:
        rec, etc, edc = s.zone_decay(align, curves=True)
        wrec, wetc, wedc = pvlib.host_zone_decay(p, delay, s.fs, labels, n_zones, align)
        assert rec.shape == (n_zones,) and rec.dtype == pvlib.ZONE_DECAY_DTYPE and etc.shape == edc.shape == (n_zones, s.T)
        assert ref.same_doubles(etc, wetc), "%s %s etc: %s" % (ctx, align, np.argwhere(etc != wetc)[:4])
        assert ref.same_doubles(edc, wedc), "%s %s edc: %s" % (ctx, align, np.argwhere(edc != wedc)[:4])
        assert ref.same_records(rec, wrec), "%s %s: %s" % (ctx, align, ref.first_difference(rec, wrec))
        assert ref.same_records(s.zone_decay(align), rec)  # (without the curves: the same records)
        reached = delay < ref.NO_ONSET
        assert [int(n) for n in rec["n_cells"]] == [int(((labels == z) & reached).sum()) for z in range(1, n_zones + 1)]
        out[align] = (rec, etc, edc)
    return out, p, delay


# (a) the solver of test_gpu_analysis_maps (25 m, 275 Hz, 160 steps, the box) with the five zones of test_gpu_zone_stats: across
# tile boundaries and the Y = 64 block boundary, around wall cells, one cell, no cell
def test_five_zones(pvlib):
    with maps.make_solver(pvlib) as s:
        assert (s.gx, s.gy) == (70, 70) and (s.info.tileRows, s.info.tileCols) == (12, 40) and s.T == 160
        s.run(LISTENER)
        lab = five_zones(s)
        s.set_zones(lab, 5)
        got, p, delay = check(pvlib, s, lab, 5, "25 m")
        (ra, ea, da), (ro, eo, do) = got["absolute"], got["onset"]
        assert ra["n_cells"][0] == 22 * 39 - 2 * 10 and ra["n_cells"][1] == 12 * 12 - 64 and ra["n_cells"][4] > 1000
        assert np.isfinite(ra["e0"]).all() and (ra["e0"][[0, 1, 2, 4]] > 0).all()
        # the single cell (50, 66)
        t0 = int(delay[50, 66])
        assert 0 < t0 < s.T - 1
        for r in (ra[2], ro[2]):
            assert (r["n_cells"], r["t_first"], r["t_last"]) == (1, t0, t0)
        sq = p[:, 50, 66].astype(np.float64) ** 2
        assert np.array_equal(ea[2, t0:], sq[t0:]) and (ea[2, :t0] == 0.0).all() and (sq[t0:] > 0).any()
        assert np.array_equal(eo[2, :s.T - t0], ea[2, t0:]) and (eo[2, s.T - t0:] == 0.0).all()  # the ABSOLUTE curve shifted by t0
        # the empty zone
        for r, e, d in ((ra[3], ea[3], da[3]), (ro[3], eo[3], do[3])):
            assert (r["n_cells"], r["t_first"], r["t_last"], r["n_edt"], r["n_t20"], r["n_t30"]) == (0, -1, -1, 0, 0, 0)
            assert r["e0"] == 0.0 and np.isnan(r["edt"]) and np.isnan(r["depth"]) and (e == 0.0).all() and (d == 0.0).all()
        # both alignments hold the same energy: every sample sits in exactly one slot
        assert np.allclose(ea.sum(axis=1), eo.sum(axis=1), rtol=1e-12)


# (b) grid shapes: the resident kernel across XCDs with a last block of 63 columns; gy < 64
@pytest.mark.parametrize("g", [ns.CROSS, ns.SMALL], ids=ns.gid)
def test_grid_shapes(pvlib, g):
    with ns.solver(pvlib, g) as s:
        assert (s.gx, s.gy) == g
        lab = scattered(s.gx, s.gy, 3, g[0])
        lab[s.gx // 3:2 * s.gx // 3, s.gy // 4:] = 4  # a block that reaches the last column
        s.set_zones(lab)
        s.run(ns.listeners(g)[0])
        got, _, _ = check(pvlib, s, lab, 4, "%d x %d" % g)
        assert (got["absolute"][0]["n_cells"] > 0).all() and (got["absolute"][0]["e0"] > 0).all()


# (c) a walled-in run on the resident-window path: a zone wholly outside the window is empty
def test_resident_window(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g, steps_per_launch=12, tile_rows=36, use_graph=2) as s:
        for b in BOXES4:
            s.add_geometry(b)
        lab = scattered(s.gx, s.gy, 2, 71)
        lab[:, :20] = 3  # far from the walled-in listener
        s.set_zones(lab, 3)
        s.run(L_IN)
        assert s.last_run_resident_window()
        got, _, delay = check(pvlib, s, lab, 3, "window path")
        for rec, etc, edc in got.values():
            assert rec[2]["n_cells"] == 0 and rec[2]["t_first"] == -1 and (etc[2] == 0.0).all() and rec["n_cells"][0] > 0
        assert (delay[:, :20] == ref.NO_ONSET).all()
        assert s.last_run_resident_window()


# (d) a history window smaller than the grid
@pytest.mark.parametrize("where", ["corner", "offset"])
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        lab = scattered(s.gx, s.gy, 3, 400)
        lab[120:300, 100:390] = 4  # a block partly inside either window
        s.set_zones(lab, 4)
        s.run(L400[where])
        got, _, delay = check(pvlib, s, lab, 4, "400^2 " + where)
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert xs.max() - xs.min() < 2 * s.T + 3 < N400  # (the window is smaller than the grid)
        rec = got["absolute"][0]
        for z in range(1, 5):  # every zone has cells without an onset, the scattered ones reached cells too
            assert (z == 4 or 0 < rec["n_cells"][z - 1]) and rec["n_cells"][z - 1] < (lab == z).sum() - 1000


# (e) a T that is no multiple of the kernel's slot group (16): the 275 Hz preset's own 435 steps
def test_ragged_last_slot_group(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        assert s.T == 435 and s.T % 16 != 0
        s.load_scene(SMALLROOM)
        lab = scattered(s.gx, s.gy, 4, 435)
        s.set_zones(lab, 4)
        s.run((5.0, 0.0, 4.0))
        got, _, _ = check(pvlib, s, lab, 4, "T = 435")
        rec = got["absolute"][0]
        assert (rec["n_edt"] > 2).all() and (got["absolute"][1][:, -1] > 0).all()  # (the last slot is written)


# (f) the slots dealt in several chunks: the scratch holds one double per slot in flight, zone and result row -- 64 zones x 400
# rows x 8 bytes = 204 800 bytes a slot, 200 slots = 41 MB against the 32 MiB bound: 160 slots (163 fit; whole groups of 16) + 40
def test_slots_in_chunks(pvlib):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=200) as s:
        assert s.gx == N400 and s.T == 200
        lab = np.broadcast_to((1 + (np.arange(N400) // 6) % 64).astype(np.uint8)[:, None], (N400, N400)).copy()
        lab[:, 300:] = 0
        s.set_zones(lab, 64)
        per_slot = 64 * s.gx * 8
        assert per_slot * s.T > (32 << 20) > per_slot * 16
        assert s.zone_decay_chunk_slots() == (32 << 20) // per_slot // 16 * 16 == 160 < s.T  # more than one chunk
        s.run(L400["offset"])
        got, _, _ = check(pvlib, s, lab, 64, "chunks", aligns=["absolute"])
        rec, etc, _ = got["absolute"]
        assert (rec["n_cells"] > 0).sum() > 10 and (etc[:, 160:] > 0).any() and (etc[:, :160] > 0).any()


# the command line: a zoneDecay table per --zone (in this process: main() is the whole tool)
def test_command_line_zone_decay(pvlib, capsys):
    import json

    from planeverb_amd.__main__ import main
    rects = [(2.0, 2.0, 9.0, 8.0), (6.0, 5.0, 30.0, 20.0), (23.0, 23.0, 24.0, 24.0)]
    argv = [SMALLROOM, "--listener", "5,0,4", "--zone-decay", "onset", "--zone-decay-curves"]
    for r in rects:
        argv += ["--zone", ",".join("%g" % v for v in r)]
    assert main(argv) == 0
    out = json.loads(capsys.readouterr().out)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        lab = pvlib.zone_labels_from_rects(s.dx, s.gx, s.gy, rects)
        s.set_zones(lab, 3)
        rec, etc, edc = s.zone_decay("onset", curves=True)
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))  # noqa: E731
    assert len(out["zones"]) == 3
    for t, r, e, d in zip(out["zones"], rec, etc, edc):
        z = t["zoneDecay"]
        assert z["align"] == "onset" and (z["nCells"], z["tFirst"], z["tLast"]) == (r["n_cells"], r["t_first"], r["t_last"])
        assert (z["nEdt"], z["nT20"], z["nT30"]) == (r["n_edt"], r["n_t20"], r["n_t30"])
        assert all(same(z[k], r[f]) for k, f in (("edt", "edt"), ("t20", "t20"), ("t30", "t30"), ("depth", "depth")))
        assert z["etc"] == [float(v) for v in e] and z["edc"] == [float(v) for v in d]
    assert out["zones"][0]["zoneDecay"]["nCells"] > 100
    with pytest.raises(SystemExit):
        main([SMALLROOM, "--zone-decay", "absolute"])  # needs --zone


# (g) the contract: refusals, nothing cached, nothing touched
def test_contract(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with maps.make_solver(pvlib) as s:
        lab = five_zones(s)
        s.set_zones(lab, 5)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: no completed run"):
            s.zone_decay()
        s.run(LISTENER)
        s.set_zones(None)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: no zones set"):
            s.zone_decay()
        s.set_zones(lab, 5)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: align is"):
            s.zone_decay(2)
        out = np.zeros(5, pvlib.ZONE_DECAY_DTYPE)
        assert pvlib.lib().PvAmdComputeZoneDecay(s._h, 0, out.ctypes.data_as(C.c_void_p), 4, None, None, None) == -1
        assert pvlib.last_error().startswith("zone decay: PvAmdComputeZoneDecay: the output holds fewer")
        assert pvlib.lib().PvAmdComputeZoneDecay(s._h, 0, None, 5, None, None, None) == -1
        assert pvlib.last_error().startswith("zone decay: ")
        # every computed map stays valid and unchanged; the call gives the same bytes twice and reports a device time
        kinds = [BY_NAME[n] for n in ("room_metrics", "decay_times", "band_metrics")]
        for k in kinds:
            compute(s, k)
        before = [whole(s, k) for k in kinds]
        results = [r.copy() for r in s.results()]
        first, ms = s.zone_decay("onset", with_ms=True)
        assert ms > 0
        assert ref.same_records(s.zone_decay("onset"), first)
        for k, b in zip(kinds, before):
            assert identical(whole(s, k), b), k["name"]
        stats = s.zone_stats("decay_times")
        # the next run's outputs are unchanged by a call in between
        s.run(LISTENER)
        for a, b in zip(s.results(), results):
            assert identical(a, b)
        assert ref.same_records(s.zone_decay("onset"), first)  # (the same listener: the same history)
        compute(s, kinds[1])
        assert ref.same_records(s.zone_stats("decay_times"), stats)
        # waits for a run in flight: a second box changes the history, and the call sees the new run
        gid = s.add_geometry((20.0, 5.0, 2.0, 2.0, 0.5))
        s.run_async(LISTENER)
        moved = s.zone_decay("onset")
        assert not ref.same_records(moved, first)
        check(pvlib, s, lab, 5, "after run_async")
        s.remove_geometry(gid)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*history"):
            s.zone_decay()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*onset map"):
            s.zone_decay()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^zone decay: .*slab"):
            s.zone_decay()
        s.run(L)
        assert s.get_output(E).occlusion > 0
