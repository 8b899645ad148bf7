"""GPU (-m gpu): per-zone ensemble decay curves per band (PvAmdComputeZoneBandDecay, csrc/pv_zone_band_decay.hip).

Every comparison is bit for bit -- etc, edc and all 96 bytes of a record, NaNs by position -- against the host restatement
api.host_zone_band_decay fed the SAME solver's recorded planes (history_plane(t)[:gx, :gy] for all t), its own onset map and the
coefficients it reports (band_coefs); the host restatement itself is held to an independent numpy restatement in
tests/test_zone_band_decay_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import _adversarial as adv
import _zone_band_decay_ref as ref
import test_gpu_analysis_maps as maps
import test_gpu_non_square as ns
from conftest import golden
from test_gpu_analysis_edges import open_size
from test_gpu_analysis_maps import KINDS, LISTENER, compute, identical, whole
from test_gpu_lateral import preset_solver
from test_gpu_query_records import BOXES4, L_IN
from test_gpu_room_metrics import L400, N400, SMALLROOM
from test_gpu_zone_stats import five_zones, scattered

pytestmark = pytest.mark.gpu

ALIGNS = ["absolute", "onset"]
OCTAVES = [125.0, 250.0, 500.0]  # below fs / 2 at the 275 Hz grids' fs = 1443


def history(s):
    return np.stack([s.history_plane(t)[:s.gx, :s.gy] for t in range(s.T)])


def check(pvlib, s, labels, n_zones, ctx, aligns=ALIGNS, p=None):
    """zone_band_decay of the last run against the host restatement of its planes, onsets and coefficients;
    {align: (records, etc, edc)}, p, delay"""
    p = history(s) if p is None else p
    delay = s.results()[1]
    coefs = s.band_coefs()
    nb = coefs.shape[0]
    out = {}
    for align in aligns:
        rec, etc, edc = s.zone_band_decay(align, curves=True)
        wrec, wetc, wedc = pvlib.host_zone_band_decay(p, delay, s.fs, labels, coefs, n_zones, align)
        assert rec.shape == (n_zones, nb) and rec.dtype == pvlib.ZONE_BAND_DECAY_DTYPE and etc.shape == edc.shape == (n_zones, nb, s.T)
        assert ref.same_doubles(etc, wetc), "%s %s etc: %s" % (ctx, align, np.argwhere(etc != wetc)[:4])
        assert ref.same_doubles(edc, wedc), "%s %s edc: %s" % (ctx, align, np.argwhere(edc != wedc)[:4])
        assert ref.same_records(rec, wrec), "%s %s: %s" % (ctx, align, ref.first_difference(rec, wrec))
        assert ref.same_records(s.zone_band_decay(align), rec)  # (without the curves: the same records)
        reached = delay < ref.NO_ONSET
        for b in range(nb):
            assert [int(n) for n in rec["n_cells"][:, b]] == [int(((labels == z) & reached).sum()) for z in range(1, n_zones + 1)]
        out[align] = (rec, etc, edc)
    return out, p, delay


# (a) the solver of test_gpu_analysis_maps (25 m, 275 Hz, 160 steps, the box) with the five zones of test_gpu_zone_stats and THREE
# bands: a wave carries two, so the last band group is short
def test_five_zones_three_bands(pvlib):
    with maps.make_solver(pvlib) as s:
        assert (s.gx, s.gy) == (70, 70) and (s.info.tileRows, s.info.tileCols) == (12, 40) and s.T == 160
        s.set_bands(OCTAVES)
        s.run(LISTENER)
        lab = five_zones(s)
        s.set_zones(lab, 5)
        assert s.zone_band_decay_chunk() == (1, s.T, 3)
        got, p, delay = check(pvlib, s, lab, 5, "25 m")
        (ra, ea, da), (ro, eo, do) = got["absolute"], got["onset"]
        assert (ra["n_cells"][0] == 22 * 39 - 2 * 10).all() and (ra["n_cells"][4] > 1000).all()
        assert np.isfinite(ra["e0"]).all() and (ra["e0"][[0, 1, 2, 4]] > 0).all()
        assert not np.array_equal(ea[0, 0], ea[0, 1]) and not np.array_equal(ea[0, 1], ea[0, 2])
        # the single cell (50, 66): the squares of the band-metrics filter's output at that cell
        t0 = int(delay[50, 66])
        assert 0 < t0 < s.T - 1
        coefs = s.band_coefs()
        for b in range(3):
            for r in (ra[2, b], ro[2, b]):
                assert (r["n_cells"], r["t_first"], r["t_last"]) == (1, t0, t0)
            y = ref.filter_backwards(p[:, 50, 66], t0, coefs[b]).astype(np.float64)
            assert np.array_equal(ea[2, b], y * y) and (ea[2, b, :t0] == 0.0).all() and (ea[2, b, t0:] > 0).any()
            assert np.array_equal(eo[2, b, :s.T - t0], ea[2, b, t0:]) and (eo[2, b, s.T - t0:] == 0.0).all()
            # ... whose float32 sum is host_band_metrics' e0, within n 2^-24 (tests/test_zone_band_decay_cpu.py has the bound)
            e0 = pvlib.host_band_metrics(p[:, 50, 66], s.fs, t0, coefs)[b, 6]
            assert abs(float(np.float32(ra[2, b]["e0"])) - float(e0)) <= (s.T - t0) * 2.0 ** -24 * ra[2, b]["e0"]
        # the empty zone, in every band
        for r, e, d in ((ra[3], ea[3], da[3]), (ro[3], eo[3], do[3])):
            assert (r["n_cells"] == 0).all() and (r["t_first"] == -1).all() and (r["n_edt"] == 0).all() and (r["e0"] == 0.0).all()
            assert np.isnan(r["edt"]).all() and np.isnan(r["c50"]).all() and np.isnan(r["ts"]).all() and (e == 0.0).all() and (d == 0.0).all()
        # both alignments hold the same energy: every sample sits in exactly one slot
        assert np.allclose(ea.sum(axis=2), eo.sum(axis=2), rtol=1e-12)


# (b) T = 435 = 27 groups of 16 slots + 3, two bands
def test_ragged_last_slot_group(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        assert s.T == 435 and s.T % 16 == 3
        s.load_scene(SMALLROOM)
        s.set_bands(OCTAVES[:2])
        lab = five_zones(s)
        s.set_zones(lab, 5)
        s.run((5.0, 0.0, 4.0))
        got, _, _ = check(pvlib, s, lab, 5, "T = 435")
        rec, etc, _ = got["absolute"]
        assert (rec["n_cells"][[0, 4]] > 0).all() and (etc[4, :, -1] > 0).all()  # (the last slot is written)


# (c) grid shapes: a last block of 63 columns; gy < 64
@pytest.mark.parametrize("g", [ns.CROSS, ns.SMALL], ids=ns.gid)
def test_grid_shapes(pvlib, g):
    with ns.solver(pvlib, g) as s:
        assert (s.gx, s.gy) == g
        s.set_bands(OCTAVES[1:])
        lab = scattered(s.gx, s.gy, 3, g[0])
        lab[s.gx // 3:2 * s.gx // 3, s.gy // 4:] = 4  # a block that reaches the last column
        s.set_zones(lab)
        s.run(ns.listeners(g)[0])
        got, _, _ = check(pvlib, s, lab, 4, "%d x %d" % g)
        assert (got["absolute"][0]["n_cells"] > 0).all() and (got["absolute"][0]["e0"] > 0).all()


# (d) a walled-in run on the resident-window path: a zone wholly outside the window is empty in every band
def test_resident_window(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g, steps_per_launch=12, tile_rows=36, use_graph=2) as s:
        for b in BOXES4:
            s.add_geometry(b)
        s.set_bands(OCTAVES)
        lab = scattered(s.gx, s.gy, 2, 71)
        lab[:, :20] = 3  # far from the walled-in listener
        s.set_zones(lab, 3)
        s.run(L_IN)
        assert s.last_run_resident_window()
        got, _, delay = check(pvlib, s, lab, 3, "window path")
        for rec, etc, edc in got.values():
            assert (rec[2]["n_cells"] == 0).all() and (rec[2]["t_first"] == -1).all() and (etc[2] == 0.0).all() and (rec["n_cells"][0] > 0).all()
        assert (delay[:, :20] == ref.NO_ONSET).all()
        assert s.last_run_resident_window()


# (e) a history window smaller than the grid
@pytest.mark.parametrize("where", ["corner", "offset"])
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.set_bands(OCTAVES[:2])
        lab = scattered(s.gx, s.gy, 3, 400)
        lab[120:300, 100:390] = 4  # a block partly inside either window
        s.set_zones(lab, 4)
        s.run(L400[where])
        got, _, delay = check(pvlib, s, lab, 4, "400^2 " + where)
        reached = delay < ref.NO_ONSET
        xs, ys = np.nonzero(reached)
        assert xs.max() - xs.min() < 2 * s.T + 3 < N400  # (the window is smaller than the grid)
        rec = got["absolute"][0]
        for z in range(1, 5):
            assert (z == 4 or 0 < rec["n_cells"][z - 1, 0]) and rec["n_cells"][z - 1, 0] < (lab == z).sum() - 1000


# (f) the (zone, band) pairs dealt in several chunks.  The scratch rule: a pair takes gx rows of T doubles, and a chunk holds all
# bands of as many whole zones as stay within 32 MiB.  The smallest solver here is the 70-row grid; at its own 435 steps a pair takes
# 70 * 435 * 8 = 243 600 bytes and 137 pairs fit.  Zones and bands are bounded by 64 and 8, and the host restatement's time grows
# with the bands, so: 64 zones and 3 bands = 192 pairs, 45 whole zones a chunk (137 // 3), two chunks (45 + 19 zones)
def test_pairs_in_chunks(pvlib):
    with pvlib.Solver(25.0, 25.0, 275) as s:
        assert (s.gx, s.T) == (70, 435)
        s.load_scene(SMALLROOM)
        s.set_bands(OCTAVES)
        lab = (1 + (np.arange(s.gx * s.gy) * 7) % 64).astype(np.uint8).reshape(s.gx, s.gy)  # every block holds many zones
        s.set_zones(lab, 64)
        pair = s.gx * s.T * 8
        assert (32 << 20) // pair == 137 and 137 // 3 == 45
        chunks, slots, bands = s.zone_band_decay_chunk()
        assert chunks == 2 and slots == s.T and bands == 3  # more than one chunk; time is never cut
        s.run((5.0, 0.0, 4.0))
        got, _, _ = check(pvlib, s, lab, 64, "chunks", aligns=["onset"])
        rec, etc, _ = got["onset"]
        assert (rec["n_cells"] > 0).all() and (etc[:45].sum(axis=2) > 0).all() and (etc[45:].sum(axis=2) > 0).all()
        # the first chunk's zones alone take one chunk: the same bits
        s.set_zones(np.where(lab <= 45, lab, 0).astype(np.uint8), 45)
        assert s.zone_band_decay_chunk() == (1, s.T, 3)
        one = s.zone_band_decay("onset", curves=True)
        assert ref.same_records(one[0], rec[:45]) and ref.same_doubles(one[1], etc[:45])


# (g) injected histories: the families of tests/_adversarial.py (denormal squares, signed zeros, squares that overflow float but
# not double, NaN and inf samples), nothing ahead of the wave front
def test_injected_histories(pvlib):
    with maps.make_solver(pvlib) as s:
        s.set_bands(OCTAVES[:2])
        s.run(LISTENER)
        new, fam, delay = adv.inject(s, 20261020)
        p = np.ascontiguousarray(new[:, :s.gx, :s.gy])
        fam = fam[:s.gx, :s.gy]
        reached = delay < ref.NO_ONSET
        # one zone per family (1 .. 11), and zone 12: one cell that holds an inf AND a NaN
        lab = np.where(reached & (fam >= 0), fam + 1, 0).astype(np.uint8)
        x, y = [int(v) for v in np.argwhere(reached & (fam == adv.FAMILIES.index("control")))[0]]
        t0 = int(delay[x, y])
        plane = new[t0 + 1].copy()
        plane[x, y] = np.inf
        s.set_history_plane(t0 + 1, plane)
        plane = new[s.T - 1].copy()
        plane[x, y] = np.nan
        s.set_history_plane(s.T - 1, plane)
        p[t0 + 1, x, y], p[s.T - 1, x, y] = np.inf, np.nan
        lab[x, y] = 12
        s.set_zones(lab, 12)
        got, _, _ = check(pvlib, s, lab, 12, "injected", p=p)
        for rec, etc, edc in got.values():
            finite_zones = [z for z in range(10) if z != adv.FAMILIES.index("loud")]
            assert np.isfinite(etc[finite_zones]).all()          # the other cells' zones are unaffected
            assert np.isnan(etc[11]).any()                        # the poisoned cell's own zone
            assert np.isfinite(etc[adv.FAMILIES.index("loud")]).all() and (etc[adv.FAMILIES.index("loud")] > 1e38).any()  # no float overflow
            assert (etc[adv.FAMILIES.index("quiet")] > 0).any() and (etc[adv.FAMILIES.index("quiet")] < 1e-30).all()      # no flush to zero
            assert (etc[adv.FAMILIES.index("silent")] == 0.0).all() and not np.signbit(etc[adv.FAMILIES.index("silent")]).any()


# (h) the contract: refusals, nothing cached, nothing touched
def test_contract(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with maps.make_solver(pvlib) as s:
        lab = five_zones(s)
        s.set_zones(lab, 5)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: no completed run"):
            s.zone_band_decay()
        s.set_record_queries([E, (12.0, 0.0, 9.0)])
        s.set_query_records(pvlib.QREC_DECAY_TIMES)
        s.run(LISTENER)
        s.set_zones(None)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: no zones set"):
            s.zone_band_decay()
        s.set_zones(lab, 5)
        bands = s.bands()
        s.set_bands([])
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: no bands set"):
            s.zone_band_decay()
        assert s.zone_band_decay_chunk()[0] == 0
        s.set_bands(*bands)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: align is"):
            s.zone_band_decay(2)
        out = np.zeros(10, pvlib.ZONE_BAND_DECAY_DTYPE)
        assert pvlib.lib().PvAmdComputeZoneBandDecay(s._h, 0, out.ctypes.data_as(C.c_void_p), 9, None, None, None) == -1
        assert pvlib.last_error().startswith("zone band decay: PvAmdComputeZoneBandDecay: the output holds fewer")
        assert pvlib.lib().PvAmdComputeZoneBandDecay(s._h, 0, None, 10, None, None, None) == -1
        assert pvlib.last_error().startswith("zone band decay: ")
        # all nine maps stay valid and unchanged, the broadband zone decay and the run's queried records too; the call gives the
        # same bytes twice and reports a device time
        for k in KINDS:
            compute(s, k)
        before = [whole(s, k) for k in KINDS]
        zd_before = s.zone_decay("onset", curves=True)
        records = s.queried_records(pvlib.QREC_DECAY_TIMES).copy()
        first, ms = s.zone_band_decay("onset", with_ms=True)
        assert ms > 0 and first.shape == (5, 2)
        assert ref.same_records(s.zone_band_decay("onset"), first)
        for k, b in zip(KINDS, before):
            assert identical(whole(s, k), b), k["name"]  # (a read is refused where a kind is no longer valid)
        zd_after = s.zone_decay("onset", curves=True)
        assert zd_after[0].tobytes() == zd_before[0].tobytes()
        assert ref.same_doubles(zd_after[1], zd_before[1]) and ref.same_doubles(zd_after[2], zd_before[2])
        assert identical(s.queried_records(pvlib.QREC_DECAY_TIMES), records)
        # the bands are read at the call: other bands, the other bands' result
        s.set_bands([250.0, 500.0, 125.0])
        moved = s.zone_band_decay("onset")
        assert moved.shape == (5, 3) and ref.same_records(moved[:, 2], first[:, 0]) and ref.same_records(moved[:, 0], first[:, 1])
        check(pvlib, s, lab, 5, "other bands", aligns=["onset"])
        s.set_bands(*bands)
        # waits for a run in flight
        s.add_geometry((20.0, 5.0, 2.0, 2.0, 0.5))
        s.run_async(LISTENER)
        assert not ref.same_records(s.zone_band_decay("onset"), first)
        check(pvlib, s, lab, 5, "after run_async", aligns=["absolute"])
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: .*history"):
            s.zone_band_decay()
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_zones(np.ones((s.gx, s.gy), np.uint8), 1)
        s.set_bands(OCTAVES[:1])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^zone band decay: .*onset map"):
            s.zone_band_decay()


# the command line: a zoneBandDecay list per --zone (in this process: main() is the whole tool)
def test_command_line_zone_band_decay(pvlib, capsys):
    import json

    from planeverb_amd.__main__ import main
    rects = [(2.0, 2.0, 9.0, 8.0), (23.0, 23.0, 24.0, 24.0)]
    argv = [SMALLROOM, "--listener", "5,0,4", "--zone-decay", "onset", "--zone-decay-curves", "--bands", "125,250"]
    for r in rects:
        argv += ["--zone", ",".join("%g" % v for v in r)]
    assert main(argv) == 0
    plain = capsys.readouterr().out
    assert "zoneBandDecay" not in plain
    assert main(argv + ["--zone-band-decay"]) == 0
    out = json.loads(capsys.readouterr().out)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_bands([125.0, 250.0])
        s.run((5.0, 0.0, 4.0))
        s.set_zones(pvlib.zone_labels_from_rects(s.dx, s.gx, s.gy, rects), 2)
        rec, etc, edc = s.zone_band_decay("onset", curves=True)
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))  # noqa: E731
    for t, rz, ez, dz in zip(out["zones"], rec, etc, edc):
        assert [b["hz"] for b in t["zoneBandDecay"]] == [125.0, 250.0]
        for b, r, e, d in zip(t["zoneBandDecay"], rz, ez, dz):
            assert all(same(b[k], r[k]) for k in ("edt", "t20", "t30", "depth", "c50", "c80", "d50", "ts"))
            assert b["etc"] == [float(v) for v in e] and b["edc"] == [float(v) for v in d]
        del t["zoneBandDecay"]
    was = json.loads(plain)  # without the flag: what it was (the two runs' timings aside)
    assert json.dumps(out["zones"]) == json.dumps(was["zones"]) and list(out) == list(was)
