"""GPU (-m gpu): the nine per-cell analysis passes, the zone decay and the zone statistics on histories the stencil never produces.

Solver.set_history_plane (PvAmdSetHistoryPlane, the inverse of history_plane) replaces the history a run recorded by the
adversarial one of tests/_adversarial.py -- ten finite families and one with NaN / inf samples, dealt by a hash of the cell so
that the lanes of a wave hold different ones -- and every kind is computed on it.  Expected values are what the kinds' own GPU
tests use, fed the injected planes and the run's own onset map: the host restatements api.host_* on every reached cell (held to
their numpy restatements on the same families, without a device, in tests/test_host_adversarial.py), and for the three velocity
kinds the numpy restatements on impulse_response(cx, cy).  Every comparison is bit for bit, NaNs by position.

The contract: a cell whose own samples are all finite (for the velocity kinds: and those of its (X - 1, Y) and (X, Y - 1)
neighbours) has the expected record whatever its neighbours in the wave hold -- all ten finite families, and the clean neighbours of
the poisoned cells.  Cells with non-finite samples are compared the same way, except for the kinds in UNSPECIFIED, whose records
of such cells include/planeverb_amd.h leaves unspecified."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _adversarial as adv
import _echogram_ref
import _lateral_ref
import _lobes_ref
import test_gpu_analysis_maps as maps
import test_gpu_non_square as ns
import test_gpu_zone_decay as zd
import test_gpu_zone_stats as zs
from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_analysis_maps import LISTENER, compute, identical, whole
from test_gpu_echogram import responses
from test_gpu_lateral import preset_solver
from test_gpu_modulation import THIRDS8
from test_gpu_query_records import BOXES4, L_IN
from test_gpu_room_metrics import L400, N400, SMALLROOM
from test_gpu_spectrum import BINS

pytestmark = pytest.mark.gpu

SEED = 20261019
SLOTS16 = (0.005, 16)
UNSPECIFIED = set()  # kinds whose records of cells with non-finite samples the header leaves unspecified
VELOCITY_KINDS = ("lateral_fraction", "echogram", "lobes")
WORKER = os.path.join(ROOT, "tests", "_injected_worker.py")


def first_scene(pvlib, nbins=32):
    """the solver of test_gpu_analysis_maps (70^2, tile 12 x 40, T = 160, one box) with eight bands, nbins bins and 16 slots"""
    s = maps.make_solver(pvlib)
    s.set_bands(THIRDS8, 3)
    s.set_spectrum_bins(BINS[nbins] if nbins in BINS else maps.BINS)
    s.set_echogram(*SLOTS16)
    return s


def per_cell(bad, nd):
    return bad.reshape(bad.shape[:nd] + (-1,)).any(axis=-1)


def compare(ctx, name, got, want, must, fam, cells=None):
    """got / want: [gx, gy, *width], or [N, *width] for the result cells `cells`; must: the cells that have to agree whatever the
    kind; a failure names the kind, the cell and the cell's family"""
    assert got.shape == want.shape and got.dtype == np.float32, (ctx, name, got.shape, want.shape)
    bad = per_cell(~same_bits(got, want), must.ndim)
    for which, sel in (("finite", bad & must), ("non-finite", bad & ~must)):
        if not sel.any() or (which == "non-finite" and name in UNSPECIFIED):
            continue
        i = tuple(np.argwhere(sel)[0])
        cell = i if cells is None else tuple(cells[i[0]])
        d = ~same_bits(got[i], want[i])
        raise AssertionError("%s, %s: %d cells with %s samples differ, first at %s: got %s, expected %s" % (
            ctx, name, sel.sum(), which, adv.describe(fam, cell), got[i][d][:4], want[i][d][:4]))


def velocity_cells(fam, reached, tile, n=520):
    """>= 400 reached cells: some of every family, >= 100 on a tile's first row or column, the four neighbours of poisoned cells"""
    rng = np.random.default_rng(SEED)
    gx, gy = fam.shape
    X, Y = np.meshgrid(np.arange(gx), np.arange(gy), indexing="ij")
    picks = []

    def some(mask, k):
        idx = np.argwhere(mask & reached)
        picks.extend(map(tuple, idx[rng.choice(len(idx), min(len(idx), k), replace=False)]))

    for f in range(len(adv.FAMILIES)):
        some(fam == f, 24)
    for x, y in picks[-24:]:  # (the last family: the poisoned cells)
        picks.extend((x + a, y + b) for a, b in ((1, 0), (0, 1), (-1, 0), (0, -1))
                     if 0 <= x + a < gx and 0 <= y + b < gy and reached[x + a, y + b])
    edge = (X % tile[0] == 0) | (Y % tile[1] == 0)
    some(edge, 130)
    some(np.ones_like(reached), n)
    cells = np.array(list(dict.fromkeys((int(x), int(y)) for x, y in picks))[:n])
    assert len(cells) >= 400 and edge[cells[:, 0], cells[:, 1]].sum() >= 100, (len(cells), edge[cells[:, 0], cells[:, 1]].sum())
    assert set(fam[cells[:, 0], cells[:, 1]]) == set(range(len(adv.FAMILIES)))
    return cells


def analyse(pvlib, s, listener, ctx, slots, edges, every_cell=False):
    """run, inject, read back, compute the nine kinds and hold each to its expected values; what the scene's other checks need"""
    s.run(listener)
    new, fam, delay = adv.inject(s, SEED)
    assert identical(adv.history(s), new), ctx + ": history_plane after the injection"
    gx, gy = s.gx, s.gy
    p = np.ascontiguousarray(new[:, :gx, :gy])
    finite = adv.finite_cells(new)
    clean_v, finite, fam = adv.clean_for_velocity(finite)[:gx, :gy], finite[:gx, :gy], fam[:gx, :gy]
    reached = delay < adv.NO_ONSET
    small = reached.sum() < 400  # (the walled-in room of the resident-window scene: a few dozen cells, all of them checked)
    for f, name in enumerate(adv.FAMILIES):
        assert small or ((fam == f) & reached).sum() >= 3, (ctx, name)
    assert np.array_equal(finite | ~reached, (fam != adv.NONFINITE) | ~reached)
    got = {}
    for k in maps.KINDS:
        assert compute(s, k) > 0
        got[k["name"]] = whole(s, k)
        assert np.isnan(got[k["name"]][~reached]).all(), (ctx, k["name"])
    want = adv.host_expected(pvlib, p, delay, s.fs, s.band_coefs(), s.modulation_frequencies(), s.spectrum_bins(), s.pulse())
    for name in adv.PRESSURE_KINDS:
        compare(ctx, name, got[name], want[name], finite | ~reached, fam)
    cells = np.argwhere(reached) if every_cell or small else velocity_cells(fam, reached, (s.info.tileRows, s.info.tileCols))
    cx, cy = cells[:, 0], cells[:, 1]
    irs = responses(s, cells)
    assert same_bits(irs[..., 0], p[:, cx, cy]).all(), ctx + ": impulse_response reads the injected planes"
    d = delay[cx, cy]
    with np.errstate(all="ignore"):
        vel = {"lateral_fraction": _lateral_ref.lateral_fraction(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs),
               "echogram": _echogram_ref.echogram(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs, *slots),
               "lobes": _lobes_ref.lobes(irs[..., 0], irs[..., 1], irs[..., 2], d, s.fs, edges)}
    for name in VELOCITY_KINDS:
        compare(ctx, name, got[name][cx, cy], vel[name], clean_v[cx, cy], fam, cells)
    return dict(p=p, fam=fam, delay=delay, maps=got, finite=finite)


# 1. the first scene: all nine kinds on every reached cell, the zone decay in both alignments and the zone statistics of every kind
@pytest.fixture(scope="module")
def first(pvlib):
    with first_scene(pvlib) as s:
        assert (s.gx, s.gy, s.T) == (70, 70, 160) and (s.info.tileRows, s.info.tileCols) == (12, 40)
        r = analyse(pvlib, s, LISTENER, "70^2", SLOTS16, maps.EDGES, every_cell=True)
        yield s, r


def test_first_scene_every_kind(first):
    s, r = first
    e0 = r["maps"]["decay_times"][..., 6]
    on = r["delay"] < adv.NO_ONSET
    assert (e0[(r["fam"] == 2) & on] == 0).all() and np.isinf(e0[(r["fam"] == 7) & (r["delay"] < s.T - 1)]).all()
    assert np.isfinite(e0[(r["fam"] == 9) & on]).all()


def test_first_scene_zone_decay(pvlib, first):
    s, r = first
    lab = zs.five_zones(s)
    s.set_zones(lab, 5)
    got, _, _ = zd.check(pvlib, s, lab, 5, "70^2 injected", p=r["p"])
    assert not np.isfinite(got["absolute"][1]).all()  # (a zone holds cells with non-finite samples)


@pytest.mark.parametrize("name", maps.IDS)
def test_first_scene_zone_stats(pvlib, first, name):
    s, r = first
    lab = zs.five_zones(s)
    s.set_zones(lab, 5)
    k = dict(maps.BY_NAME[name], width=r["maps"][name].shape[2:])  # (this scene's settings: eight bands, 32 bins, 16 slots)
    got, m = zs.check(pvlib, s, k, lab, 5, "70^2 injected")
    assert identical(m, r["maps"][name])
    assert got["n_finite"].sum() > 0 and got["n_nan"].sum() > 0


# 2. the other scenes, all nine kinds under the base settings
def scene_preset(pvlib):
    g = golden("g71_smallroom")
    s = preset_solver(pvlib, g)
    return s, g["listener"], lambda: s.T == 435


def scene_window_path(pvlib):
    s = preset_solver(pvlib, golden("g71_smallroom"), steps_per_launch=12, tile_rows=36, use_graph=2)
    for b in BOXES4:
        s.add_geometry(b)
    return s, L_IN, s.last_run_resident_window


def scene_offset_window(pvlib):
    size = open_size(N400)
    s = pvlib.Solver(size, size, 275, num_steps=160)
    s.load_scene(SMALLROOM)
    s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
    return s, L400["offset"], lambda: s.gx == N400 and 2 * s.T + 3 < N400


def scene_grid(g):
    def make(pvlib):
        s = ns.solver(pvlib, g)
        return s, ns.listeners(g)[0], lambda: (s.gx, s.gy) == g
    return make


SCENES = {"preset_T435": scene_preset, "resident_window": scene_window_path, "offset_window": scene_offset_window,
          "127x191": scene_grid(ns.CROSS), "24x50": scene_grid(ns.SMALL)}


@pytest.mark.parametrize("scene", list(SCENES))
def test_other_scenes(pvlib, scene):
    s, listener, took = SCENES[scene](pvlib)
    with s:
        maps.base_settings(s)
        r = analyse(pvlib, s, listener, scene, maps.SLOTS, maps.EDGES)
        assert took(), scene
        n = (r["delay"] < adv.NO_ONSET).sum()
        assert n >= 400 or (scene == "resident_window" and n >= 12), n


# 3. nothing of an injection survives into the next run
def test_next_run_is_clean(pvlib, first):
    s, _ = first
    s.run(LISTENER)
    with first_scene(pvlib) as f:
        f.run(LISTENER)
        for a, b in zip(s.results(), f.results()):
            assert identical(a, b)
        for t in range(s.T):
            assert identical(s.history_plane(t), f.history_plane(t)), t
        for k in (maps.BY_NAME["decay_times"], maps.BY_NAME["spectrum"]):
            compute(s, k), compute(f, k)
            assert identical(whole(s, k), whole(f, k)), k["name"]


# 4. what is stored is set, what is not is ignored; the contract around the call
def test_stored_cells_and_contract(pvlib):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        plane = np.full((s.gx + 1, s.gy + 1), 7.0, np.float32)
        with pytest.raises(pvlib.PlaneverbError, match="^set history plane: no completed run"):
            s.set_history_plane(0, plane)
        maps.base_settings(s)
        s.set_record_queries([L400["offset"]])
        s.set_query_records(pvlib.QREC_DECAY_TIMES)
        s.run(L400["offset"])
        results = [a.copy() for a in s.results()]
        records = s.queried_records(pvlib.QREC_DECAY_TIMES).copy()
        K = s.info.stepsPerLaunch
        stored = {}
        for t in (0, K, 100, s.T - 1):
            rec = s.history_plane(t)
            s.set_history_plane(t, plane)
            back = s.history_plane(t)
            stored[t] = back == 7.0
            assert ((back == 7.0) | (back == 0.0)).all() and stored[t][rec != 0].all(), t
        assert 0 < stored[0].sum() < stored[100].sum() <= stored[s.T - 1].sum() < plane.size  # (tiles join; the window is smaller)
        assert (stored[0] <= stored[K]).all() and (stored[K] <= stored[100]).all() and (stored[100] <= stored[s.T - 1]).all()
        xs, ys = np.nonzero(stored[s.T - 1])
        assert xs.min() > 0 and xs.min() % s.info.tileRows == 0  # (whole tiles, an origin other than tile 0)        # every map is "not computed" after a call; the run's results and in-run records are untouched
        for k in maps.KINDS:
            compute(s, k)
        s.set_history_plane(5, plane)
        for k in maps.KINDS:
            maps.refused(pvlib, s, k, "not computed")
        for a, b in zip(s.results(), results):
            assert identical(a, b)
        assert identical(s.queried_records(pvlib.QREC_DECAY_TIMES), records)
        # refusals
        for t in (-1, s.T):
            with pytest.raises(pvlib.PlaneverbError, match="^set history plane: step outside"):
                s.set_history_plane(t, plane)
        assert pvlib.lib().PvAmdSetHistoryPlane(s._h, 0, None) == -1 and pvlib.last_error().startswith("set history plane: ")
        assert pvlib.lib().PvAmdSetHistoryPlane(None, 0, None) == -1 and pvlib.last_error().startswith("set history plane: ")
        with pytest.raises(ValueError):
            s.set_history_plane(0, plane[:-1])
        # waits for a run in flight: the plane lands in the new run's history
        s.run_async(L400["corner"])
        s.set_history_plane(s.T - 1, plane)
        back = s.history_plane(s.T - 1)
        assert (back == 7.0).any() and not np.array_equal(back == 7.0, stored[s.T - 1])
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters([(5.0, 0.0, 6.0)])
        s.run((5.0, 0.0, 4.0))
        with pytest.raises(pvlib.PlaneverbError, match="^set history plane: .*history"):
            s.set_history_plane(0, np.zeros((s.gx + 1, s.gy + 1), np.float32))
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run((5.0, 0.0, 4.0))
        with pytest.raises(pvlib.PlaneverbError, match="^set history plane: .*slab"):
            s.set_history_plane(0, np.zeros((s.gx + 1, s.gy + 1), np.float32))


# 5. the two forms the library ships and no other test selects: a child process per setting, its map against this process's
FORMS = {"decay_two_launches": ({"PLANEVERB_AMD_DECAY_LAUNCHES": "2"}, "decay_times", 32),
         "spectrum_block_8": ({"PLANEVERB_AMD_SPECTRUM_BLOCK": "8"}, "spectrum", 32),
         "spectrum_block_16": ({"PLANEVERB_AMD_SPECTRUM_BLOCK": "16"}, "spectrum", 3)}


@pytest.mark.parametrize("form", list(FORMS))
def test_unselected_forms(pvlib, tmp_path, form):
    env, kind, nbins = FORMS[form]
    assert "PLANEVERB_AMD_DECAY_LAUNCHES" not in os.environ and "PLANEVERB_AMD_SPECTRUM_BLOCK" not in os.environ
    out = str(tmp_path / "map.npy")
    r = subprocess.run([sys.executable, WORKER, kind, str(nbins), out], env=dict(os.environ, **env), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    with first_scene(pvlib, nbins) as s:
        s.run(LISTENER)
        adv.inject(s, SEED)
        compute(s, maps.BY_NAME[kind])
        mine = whole(s, maps.BY_NAME[kind])
    theirs = np.load(out)
    assert mine.shape[2] == (8 if kind == "decay_times" else nbins) and not np.isfinite(mine).all() and np.isfinite(mine).any()
    assert identical(theirs, mine), form
