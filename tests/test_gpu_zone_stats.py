"""GPU (-m gpu): zone statistics of the per-cell analysis maps (PvAmdComputeZoneStats, csrc/pv_zones.hip).

Every comparison is bit for bit -- all struct bytes, NaNs by position (_zone_ref.same_records) -- against the host restatement
api.host_zone_stats applied to the WHOLE map as Solver.<kind>() returns it; the host restatement itself is held to an independent
numpy restatement and to exact sums in tests/test_zone_stats_cpu.py."""
import numpy as np
import pytest

import _zone_ref as ref
import test_gpu_analysis_maps as maps
import test_gpu_non_square as ns
from conftest import golden
from test_gpu_analysis_edges import open_size
from test_gpu_analysis_maps import BY_NAME, IDS, KINDS, LISTENER, compute, identical, whole
from test_gpu_lateral import preset_solver
from test_gpu_modulation import THIRDS8
from test_gpu_query_records import BOXES4, L_IN
from test_gpu_room_metrics import L400, N400, SMALLROOM

pytestmark = pytest.mark.gpu


def check(pvlib, s, k, labels, n_zones, ctx):
    """zone_stats of kind k (computed) against the host restatement of its whole map; returns (records, map)"""
    m = whole(s, k)
    got = s.zone_stats(k["name"])
    want = pvlib.host_zone_stats(m, labels, n_zones)
    assert got.shape == (n_zones,) + k["width"] and got.dtype == pvlib.ZONE_STAT_DTYPE
    assert ref.same_records(got, want), "%s %s: %s" % (ctx, k["name"], ref.first_difference(got, want))
    size = np.array([(labels == z).sum() for z in range(1, n_zones + 1)]).reshape((n_zones,) + (1,) * len(k["width"]))
    assert np.array_equal(got["n_finite"] + got["n_nan"] + got["n_posinf"] + got["n_neginf"], np.broadcast_to(size, got.shape))
    return got, m


def scattered(gx, gy, n_zones, seed):
    return np.random.default_rng(seed).integers(0, n_zones + 1, (gx, gy)).astype(np.uint8)


# (a) all nine kinds on the solver of test_gpu_analysis_maps: 25 m, 275 Hz, 160 steps, the box
def five_zones(s):
    lab = np.full((s.gx, s.gy), 5, np.uint8)  # 5: the whole grid, where no other zone lies
    lab[8:30, 30:69] = 1                      # 1: across tile boundaries (12 x 40 tiles) and the Y = 64 block boundary
    lab[28:40, 28:40] = 2                     # 2: holds the box's cells (30 .. 37 of both axes: NaN)
    lab[50, 66] = 3                           # 3: one cell; 4: empty
    return lab


@pytest.fixture(scope="module")
def solver(pvlib):
    with maps.make_solver(pvlib) as s:
        assert (s.gx, s.gy) == (70, 70) and (s.info.tileRows, s.info.tileCols) == (12, 40)
        s.run(LISTENER)
        s.set_zones(five_zones(s), 5)
        yield s


@pytest.mark.parametrize("name", IDS)
def test_every_kind(pvlib, solver, name):
    s, k = solver, BY_NAME[name]
    lab, n = s.zones()
    assert n == 5 and np.array_equal(lab, five_zones(s))
    compute(s, k)
    assert s.zone_stats(KINDS.index(k)).tobytes() == s.zone_stats(name).tobytes()  # (by constant, by name)
    got, m = check(pvlib, s, k, lab, 5, "25 m")
    flat = got.reshape(5, -1)
    fin, nan = flat["n_finite"].max(axis=1), flat["n_nan"].min(axis=1)  # per zone: the fullest plane, the fewest NaNs
    assert fin[0] > 0 and nan[1] >= 64 and fin[1] > 0  # (the box's 8 x 8 cells)
    assert ((flat["n_finite"] + flat["n_nan"] + flat["n_posinf"] + flat["n_neginf"])[2] == 1).all()
    assert fin[3] == 0 and nan[3] == 0 and (flat["argmin"][3] == -1).all() and np.isnan(flat["mean"][3]).all()
    assert (flat["sum"][3] == 0.0).all() and fin[4] > 1000


# (b) grid shapes: the resident kernel across XCDs with a last block of 63 columns; gy < 64
@pytest.mark.parametrize("g", [ns.CROSS, ns.SMALL], ids=ns.gid)
def test_grid_shapes(pvlib, g):
    with ns.solver(pvlib, g) as s:
        assert (s.gx, s.gy) == g
        s.set_bands([125.0, 250.0])
        lab = scattered(s.gx, s.gy, 3, g[0])
        lab[s.gx // 3:2 * s.gx // 3, s.gy // 4:] = 4  # a block that reaches the last column
        s.set_zones(lab)
        assert s.zones()[1] == 4
        s.run(ns.listeners(g)[0])
        for name in ("decay_times", "band_metrics"):
            k = dict(BY_NAME[name])
            compute(s, k)
            got, _ = check(pvlib, s, k, lab, 4, "%d x %d" % g)
            assert (got["n_finite"].reshape(4, -1).max(axis=1) > 0).all() and (got["n_nan"].reshape(4, -1).max(axis=1) > 0).all()


# (c) a history window smaller than the grid: zones reach outside it, their outside cells count as NaN
def test_resident_window(pvlib):
    g = golden("g71_smallroom")
    with preset_solver(pvlib, g, steps_per_launch=12, tile_rows=36, use_graph=2) as s:
        for b in BOXES4:
            s.add_geometry(b)
        s.set_bands([125.0, 250.0])
        lab = scattered(s.gx, s.gy, 2, 71)
        lab[:, :20] = 3  # far from the walled-in listener
        s.set_zones(lab, 3)
        s.run(L_IN)
        assert s.last_run_resident_window()
        for name in ("room_metrics", "band_metrics"):
            k = BY_NAME[name]
            compute(s, k)
            got, m = check(pvlib, s, k, lab, 3, "window path")
            assert np.isnan(m[:, :20]).all() and np.isfinite(m).any()
            first = got.reshape(3, -1)[:, 0]
            assert first["n_finite"][2] == 0 and first["n_nan"][2] == 20 * s.gx and first["n_finite"][0] > 0
        assert s.last_run_resident_window()


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
        k = BY_NAME["room_metrics"]
        compute(s, k)
        got, m = check(pvlib, s, k, lab, 4, "400^2 " + where)
        reached = ~np.isnan(m).all(axis=-1)
        xs, ys = np.nonzero(reached)
        assert xs.max() - xs.min() < 2 * s.T + 3 < N400  # (the window is smaller than the grid)
        first = got[:, 0]
        outside = np.ones(m.shape[:2], bool)
        outside[xs.min():xs.max() + 1, ys.min():ys.max() + 1] = False
        assert (got["n_finite"][:3].max(axis=1) > 0).all()
        for z in range(1, 5):  # every zone has cells outside the window: they are NaN in every plane
            assert (lab[outside] == z).sum() > 1000 and (first["n_nan"][z - 1] >= (lab[outside] == z).sum())


# the planes of a map in several chunks: 64 zones x 400 rows x 48 bytes of scratch per plane, 96 planes -- 118 MB against the
# 32 MiB the scratch is kept within, so the planes are dealt 27 at a time
def test_planes_in_chunks(pvlib):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        s.load_scene(SMALLROOM)
        s.set_bands(THIRDS8, 3)
        lab = np.broadcast_to((1 + (np.arange(N400) // 6) % 64).astype(np.uint8)[:, None], (N400, N400)).copy()
        lab[:, 300:] = 0
        s.set_zones(lab, 64)
        s.run(L400["offset"])
        k = dict(BY_NAME["band_metrics"], width=(8, 12))
        compute(s, k)
        planes = 8 * 12
        assert 64 * s.gx * 48 * planes > 3 * (32 << 20) and 64 * s.gx * 48 < (32 << 20)
        got, _ = check(pvlib, s, k, lab, 64, "chunks")
        assert (got["n_finite"].reshape(64, -1).max(axis=1) > 0).sum() > 10


# the command line: a table per --zone (in this process: main() is the whole tool)
def test_command_line_zone_tables(pvlib, capsys):
    import json

    from planeverb_amd.__main__ import main
    rects = [(2.0, 2.0, 9.0, 8.0), (6.0, 5.0, 30.0, 20.0)]  # overlapping, the second partly off the 25 m grid
    argv = [SMALLROOM, "--listener", "5,0,4", "--room-metrics", "--bands", "125,250"]
    for r in rects:
        argv += ["--zone", ",".join("%g" % v for v in r)]
    assert main(argv) == 0
    out = json.loads(capsys.readouterr().out)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_bands([125.0, 250.0])
        s.run((5.0, 0.0, 4.0))
        s.compute_room_metrics()
        s.compute_band_metrics()
        lab = pvlib.zone_labels_from_rects(s.dx, s.gx, s.gy, rects)
        want = {"roomMetrics": (pvlib.host_zone_stats(s.room_metrics(), lab, 2), list(pvlib.ROOM_METRIC_NAMES)),
                "bandMetrics": (pvlib.host_zone_stats(s.band_metrics(), lab, 2).reshape(2, -1),
                                ["%gHz.%s" % (hz, n) for hz in (125.0, 250.0) for n in pvlib.BAND_METRIC_NAMES])}
    assert len(out["zones"]) == 2
    for j, t in enumerate(out["zones"]):
        assert t["rect"] == list(rects[j]) and t["cells"] == (lab == j + 1).sum() > 0
        for key, (recs, names) in want.items():
            assert list(t[key]) == names
            for n, r in zip(names, recs[j]):
                row = t[key][n]
                assert row["n"] == r["n_finite"]
                for f in ("mean", "std", "min", "max"):
                    assert row[f] == r[f] or (np.isnan(row[f]) and np.isnan(r[f])), (key, n, f)


# (d) the contract
def test_contract(pvlib):
    with maps.make_solver(pvlib) as s:
        room, decay, bands = BY_NAME["room_metrics"], BY_NAME["decay_times"], BY_NAME["band_metrics"]
        s.run(LISTENER)
        compute(s, room)
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: no zones set"):
            s.zone_stats("room_metrics")
        assert s.zones() == (None, 0)
        lab = five_zones(s)
        bad = lab.copy()
        bad[0, 0] = 6
        for labels, n, why in ((bad, 5, "a label above nZones"), (lab, 0, "nZones is 1 .. 64"), (lab, 65, "nZones is 1 .. 64")):
            with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: " + why):
                s.set_zones(labels, n)
            assert s.zones() == (None, 0)
        s.set_zones(lab, 5)
        # refused before the kind is computed, and after a new run until it is computed again
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: decay times: not computed"):
            s.zone_stats("decay_times")
        first, _ = check(pvlib, s, room, lab, 5, "contract")
        s.run(LISTENER)
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: room metrics: not computed"):
            s.zone_stats(pvlib.PVA_MAP_ROOM_METRICS)
        assert s.zones()[1] == 5  # (the labels survive the run)
        for k in (room, decay, bands):
            compute(s, k)
        before = [whole(s, k) for k in (room, decay, bands)]
        again = s.zone_stats("room_metrics")
        assert ref.same_records(again, first)  # (the same listener: the same map)
        assert s.zone_stats("room_metrics").tobytes() == again.tobytes()  # twice: identical bytes
        for k, b in zip((room, decay, bands), before):  # the map and two other kinds' maps are untouched
            assert identical(whole(s, k), b), k["name"]
        # new labels take effect on the next call
        other = np.roll(lab, 7, axis=0)
        s.set_zones(other, 5)
        moved, _ = check(pvlib, s, room, other, 5, "new labels")
        assert not ref.same_records(moved, again)
        assert ref.same_records(pvlib.host_zone_stats(before[0], lab, 5), again)
        # a geometry change invalidates the kind, not the labels
        gid = s.add_geometry((20.0, 5.0, 2.0, 2.0, 0.5))
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: room metrics: not computed"):
            s.zone_stats("room_metrics")
        s.remove_geometry(gid)
        assert np.array_equal(s.zones()[0], other)
        # a kind without its setting; an unknown kind
        s.set_spectrum_bins([])
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: "):
            s.zone_stats("spectrum")
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: kind"):
            s.zone_stats(9)
        # set_zones waits for a run in flight.  A run's timings -- its count of reached cells among them -- are taken when the run
        # is waited for and by nothing else, so they tell whether that has happened: after run_async they are still the earlier
        # run's, after set_zones they are the new run's
        s.run(LISTENER)
        reached = s.timings().reachedCells
        assert reached == s.gx * s.gy - 64  # (every cell but the box's)
        gid = s.add_geometry((20.0, 5.0, 2.0, 2.0, 0.5))  # (a second box: fewer cells to reach)
        s.run_async(LISTENER)
        assert s.timings().reachedCells == reached
        s.set_zones(lab, 5)
        assert 0 < s.timings().reachedCells < reached
        compute(s, room)
        check(pvlib, s, room, lab, 5, "after run_async")
        s.remove_geometry(gid)
        # cleared
        s.set_zones(None)
        with pytest.raises(pvlib.PlaneverbError, match="^zone statistics: no zones set"):
            s.zone_stats("room_metrics")
