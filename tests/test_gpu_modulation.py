"""GPU (-m gpu): per-cell, per-band modulation transfer function and modulation transfer index (PvAmdComputeModulation;
pv_modulation.hip).

The expected values come from the host restatement (api.host_modulation: PvAmdHostModulation, itself held bit for bit to the numpy
restatement by tests/test_host_modulation.py) applied to something else than the pass under test: the solver's own
impulse_response(cx, cy) (pv_ir_kernel: one cell on one lane), with the run's own onset map (results()[1]), the coefficients the
solver reports (band_coefs()) and the modulation frequencies it reports.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import N_OPEN, OPEN_SEQ, open_size
from test_gpu_bands import solver_of
from test_gpu_layer import cell_of
from test_gpu_lobes import FORMS
from test_gpu_room_metrics import L400, N400, SMALLROOM

pytestmark = pytest.mark.gpu

NO_ONSET = np.float32(3.0e38)
BANDS = [63.0, 125.0]
ONE_BITS = np.float32(1).view(np.uint32)
THIRDS8 = [31.5, 40.0, 63.0, 100.0, 160.0, 250.0, 400.0, 500.0]


def expected_at(pvlib, s, cells, delay):
    """the host restatement on impulse_response of the given result cells: float32 [len(cells), n, 15], NaN without an onset"""
    coefs, hz = s.band_coefs(), s.modulation_frequencies()
    out = np.full((len(cells), len(coefs), 15), np.nan, np.float32)
    for i, (x, y) in enumerate(cells):
        if delay[x, y] < NO_ONSET:
            out[i] = pvlib.host_modulation(s.impulse_response(int(x), int(y))[:, 0], s.fs, int(delay[x, y]), coefs, hz)
    return out


def check_cells(pvlib, s, got, cells, delay, ctx):
    cells = np.asarray(cells).reshape(-1, 2)
    want = expected_at(pvlib, s, cells, delay)
    mine = got[cells[:, 0], cells[:, 1]]
    bad = ~same_bits(mine, want)
    assert not bad.any(), "%s: %d of %d values differ, first at cell %s: %s vs %s" % (
        ctx, bad.sum(), bad.size, cells[np.argwhere(bad)[0][0]], mine[bad][:4], want[bad][:4])


def check_nan_pattern(got, delay, ctx):
    """NaN records on exactly the cells without an onset (a band of a reached cell is all NaN or all numbers: E == 0 or not)"""
    reached = delay < NO_ONSET
    assert got.dtype == np.float32 and got.shape[-1] == 15
    assert np.isnan(got[~reached]).all(), ctx
    nan = np.isnan(got)
    assert np.array_equal(nan.all(axis=-1), nan.any(axis=-1)), ctx
    return reached


def sample(rng, mask, n):
    idx = np.argwhere(mask)
    return idx[rng.choice(len(idx), min(len(idx), n), replace=False)]


_PRESET = {}


def preset_run(pvlib):
    """plain run of g71_smallroom at its golden listener with two octaves and the default modulation frequencies"""
    if not _PRESET:
        g = golden("g71_smallroom")
        with solver_of(pvlib, g) as s:
            s.set_bands(BANDS)
            s.run(g["listener"])
            assert s.compute_modulation() > 0
            delay = s.results()[1]
            got = s.modulation()
            reached = delay < NO_ONSET
            rxi, wi = s.info.tileRows, s.info.tileCols
            X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
            offset = ((X // rxi * -(-s.gy // wi) + Y // wi) * rxi + X % rxi) * wi + Y % wi  # (the window is the whole grid)
            wave = offset // 64  # (64 consecutive plane offsets: a wave of the pass; it may straddle two tiles)
            spread = dict((w, np.ptp(delay[(wave == w) & reached])) for w in np.unique(wave[reached]))
            widest = max(spread, key=spread.get)
            rng = np.random.default_rng(71)
            classes = {"listener": np.argwhere(delay == delay.min())[:1],
                       "tile edges": sample(rng, reached & ((X % rxi == 0) | (X % rxi == rxi - 1) | (Y % wi == 0) | (Y % wi == wi - 1)), 16),
                       "latest onset": np.argwhere(reached & (delay == delay[reached].max()))[:1],
                       "frozen lanes": np.argwhere((wave == widest) & reached),
                       "no onset": np.argwhere(~reached)[:2],
                       "anywhere": sample(rng, reached, 16)}
            cells = np.concatenate(list(classes.values()))
            _PRESET["run"] = dict(got=got, delay=delay, spread=spread[widest], cells=cells, want=expected_at(pvlib, s, cells, delay),
                                  shape=(s.gx, s.T, s.fs), hz=s.modulation_frequencies(),
                                  counts=dict((k, len(v)) for k, v in classes.items()))
    return _PRESET["run"]


# 1. the 70^2 preset (T = 435: the resident path)
def test_preset_grid(pvlib):
    r = preset_run(pvlib)
    got, delay, cells = r["got"], r["delay"], r["cells"]
    assert r["shape"] == (70, 435, 1443) and got.shape == (70, 70, 2, 15)
    assert same_bits(r["hz"], np.float32(pvlib.MODULATION_DEFAULT_HZ)).all()
    reached = check_nan_pattern(got, delay, "g71_smallroom")
    assert reached.sum() == 4673 and np.array_equal(np.isnan(got).all(axis=(-1, -2)), ~reached)
    assert not np.isnan(got[reached]).any()  # (no octave of this scene is silent at a reached cell)
    print("cells", r["counts"], "onset spread of the widest wave", r["spread"])
    assert len(cells) >= 32 and r["spread"] > 100 and r["counts"]["frozen lanes"] >= 8 and r["counts"]["no onset"] == 2
    mine = got[cells[:, 0], cells[:, 1]]
    bad = ~same_bits(mine, r["want"])
    assert not bad.any(), (bad.sum(), cells[np.argwhere(bad)[0][0]], mine[bad][:4], r["want"][bad][:4])
    m, mti = got[reached][..., :14], got[reached][..., 14]
    assert (m >= 0).all() and (m <= 1.0001).all() and (mti >= 0).all() and (mti <= 1).all()
    assert m[..., 0].mean() > m[..., 13].mean()  # (a room smears fast modulations more than slow ones)


# 2. onsets that leave fewer steps than one chunk of the walk, and a band that is silent there
def test_late_onsets_and_a_silent_band(pvlib):
    size = open_size(N_OPEN)
    with pvlib.Solver(size, size, 275) as s:
        assert s.gx == N_OPEN and s.T == 435
        s.set_bands([1e-8, 63.0], 3)  # (the 1e-8 Hz third octave: gains of 5e-12 per section, so few samples square to +0)
        s.run(OPEN_SEQ[0])
        s.compute_modulation()
        got, delay = s.modulation(), s.results()[1]
        reached = check_nan_pattern(got, delay, "open 520")
        left = np.where(reached, s.T - delay, 0)
        short = reached & (left < 8)
        assert short.sum() > 1000 and (reached & (left == 1)).any() and (~reached).any()
        rng = np.random.default_rng(520)
        cells = np.concatenate([sample(rng, reached & (left == k), 6) for k in range(1, 8)] + [sample(rng, reached & (left > 100), 8),
                                                                                                np.argwhere(~reached)[:1]])
        check_cells(pvlib, s, got, cells, delay, "open 520")
        silent = np.isnan(got[..., 0, :]).all(axis=-1) & reached
        print("late-onset cells", int(short.sum()), "of them silent in band 0:", int((silent & short).sum()), "silent at all", int(silent.sum()))
        assert (silent & short).sum() > 100 and not np.isnan(got[..., 1, :][reached]).any()
        assert (got[..., 0, :].view(np.uint32)[silent] == 0x7fc00000).all()
        assert np.isfinite(got[..., 0, :][reached & (left > 300)]).any()  # (over hundreds of steps the band's output grows out of the underflow)


# 3. band counts, custom modulation frequencies with 0 Hz and fs / 2, and the default restored
@pytest.mark.parametrize("hz,fraction", [([125.0], 1), ([63.0, 125.0, 250.0], 1), (THIRDS8, 3)], ids=["1", "3", "8"])
def test_band_counts_and_custom_frequencies(pvlib, hz, fraction):
    g = golden("g71_smallroom")
    with solver_of(pvlib, g) as s:
        s.set_bands(hz, fraction)
        F = np.array(pvlib.MODULATION_DEFAULT_HZ, np.float32)
        F[0], F[6], F[13] = 0.0, 33.3, s.fs / 2
        s.set_modulation_frequencies(F)
        assert same_bits(s.modulation_frequencies(), F).all()
        s.run(g["listener"])
        s.compute_modulation()
        got, delay = s.modulation(), s.results()[1]
        assert got.shape == (70, 70, len(hz), 15)
        reached = check_nan_pattern(got, delay, "%d bands" % len(hz))
        cells = sample(np.random.default_rng(len(hz)), reached, 24)
        check_cells(pvlib, s, got, cells, delay, "%d bands, custom frequencies" % len(hz))
        live = reached[..., None] & ~np.isnan(got[..., 14])
        assert live.sum() > 4000 * len(hz) and (got[..., 0].view(np.uint32)[live] == ONE_BITS).all()  # m(0 Hz) == 1.0f exactly
        s.set_modulation_frequencies(None)
        assert same_bits(s.modulation_frequencies(), np.float32(pvlib.MODULATION_DEFAULT_HZ)).all()
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: not computed"):
            s.modulation()
        s.compute_modulation()
        again = s.modulation()
        check_cells(pvlib, s, again, cells[:8], delay, "%d bands, default frequencies" % len(hz))
        if hz == BANDS + [250.0]:
            assert same_bits(again[..., :2, :], preset_run(pvlib)["got"]).all()  # (a band's record does not depend on the others)


# 4. a history window smaller than the grid: clipped on two sides, and with a tile origin other than tile 0
@pytest.mark.parametrize("where", ["corner", "offset"])
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.set_bands(BANDS)
        s.run(L400[where])
        s.compute_modulation()
        got, delay = s.modulation(), s.results()[1]
        reached = check_nan_pattern(got, delay, where)
        xs, ys = np.nonzero(reached)
        rows, cols = slice(max(xs.min() - 2, 0), xs.max() + 3), slice(max(ys.min() - 2, 0), ys.max() + 3)
        outside = np.ones(delay.shape, bool)
        outside[rows, cols] = False
        assert outside.any() and np.isnan(got[outside]).all()
        rxi, wi = s.info.tileRows, s.info.tileCols
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        rng = np.random.default_rng(400)
        cells = np.concatenate([sample(rng, reached & ((X % rxi == 0) | (Y % wi == 0)), 12), sample(rng, reached & (delay >= s.T - 8), 8),
                                sample(rng, reached, 16), np.argwhere(~reached & ~outside)[:1]])
        assert len(cells) >= 32
        check_cells(pvlib, s, got, cells, delay, where)
        assert same_bits(s.modulation_block(rows.start, cols.start, 5, 7), got[rows.start:rows.start + 5, cols.start:cols.start + 7]).all()


# 5. a non-square grid
def test_non_square_grid(pvlib):
    with pvlib.Solver(open_size(70), open_size(127), 275) as s:
        assert (s.gx, s.gy, s.T) == (70, 127, 435)
        s.load_scene(SMALLROOM)
        s.set_bands(BANDS)
        s.run(cell_of(22, 40))
        s.compute_modulation()
        got, delay = s.modulation(), s.results()[1]
        assert got.shape == (70, 127, 2, 15)
        reached = check_nan_pattern(got, delay, "70 x 127")
        assert reached.sum() > 3000
        cells = np.concatenate([sample(np.random.default_rng(127), reached, 36), sample(np.random.default_rng(70), reached & (np.arange(127) >= 64), 12)])
        check_cells(pvlib, s, got, cells, delay, "70 x 127")
        e = cell_of(30, 100)
        assert same_bits(s.modulation_at(e), got[30, 100]).all()
        assert np.isnan(s.modulation_at(cell_of(70, 10))).all() and s.modulation_at(cell_of(70, 10)).shape == (2, 15)


# 6. the same bits on every stepping path
@pytest.mark.parametrize("form", list(FORMS))
def test_same_bits_on_every_path(pvlib, form):
    r = preset_run(pvlib)
    g = golden("g71_smallroom")
    with solver_of(pvlib, g, **FORMS[form]) as s:
        s.set_bands(BANDS)
        s.run_async(g["listener"])
        s.sync()
        s.compute_modulation()
        assert same_bits(s.results()[1], r["delay"]).all()
        assert same_bits(s.modulation(), r["got"]).all(), form


# 7. lifetime and refusals
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    want = preset_run(pvlib)["got"]
    with solver_of(pvlib, g) as s:
        reads = (s.modulation, lambda: s.modulation_at(g["emitters"][0]), lambda: s.modulation_block(0, 0, 2, 2))

        def refused(why="^modulation: "):
            for call in reads:
                with pytest.raises(pvlib.PlaneverbError, match=why):
                    call()

        with pytest.raises(pvlib.PlaneverbError, match="^modulation: no bands set"):
            s.compute_modulation()
        refused("^modulation: no bands set")
        s.set_bands(BANDS)
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: no completed run"):
            s.compute_modulation()
        s.run(g["listener"])
        refused("^modulation: not computed")
        s.set_spectrum_bins([50.0, 100.0])
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        s.compute_band_metrics()
        s.compute_lobes()
        others = lambda: (s.room_metrics(), s.spectrum(), s.decay_times(), s.band_metrics(), s.lobes())  # noqa: E731
        before = others()
        refused("^modulation: not computed")
        s.compute_modulation()
        first = s.modulation()
        assert same_bits(first, want).all()
        assert all(same_bits(a, b).all() for a, b in zip(others(), before))  # (the other kinds are still valid)
        s.compute_room_metrics()
        s.compute_spectrum()
        s.compute_decay_times()
        s.compute_band_metrics()
        s.compute_lobes()
        assert same_bits(s.modulation(), first).all()  # (and the reverse)
        # a change of bands invalidates this kind too, even to the same bands
        s.set_bands(BANDS)
        refused("^modulation: not computed")
        s.compute_modulation()
        assert same_bits(s.modulation(), first).all()
        # a change of the modulation frequencies invalidates, even to the same ones; the band metrics stay
        s.compute_band_metrics()
        bm = s.band_metrics()
        s.set_modulation_frequencies(pvlib.MODULATION_DEFAULT_HZ)
        refused("^modulation: not computed")
        assert same_bits(s.band_metrics(), bm).all()
        s.compute_modulation()
        assert same_bits(s.modulation(), first).all()
        # a refused change leaves frequencies and records alone
        for bad in ([float("nan")] + [1.0] * 13, [-1.0] + [1.0] * 13, [1.0] * 13 + [s.fs / 2 + 1.0], [float("inf")] * 14):
            with pytest.raises(pvlib.PlaneverbError, match="^modulation: "):
                s.set_modulation_frequencies(bad)
        assert same_bits(s.modulation_frequencies(), np.float32(pvlib.MODULATION_DEFAULT_HZ)).all() and same_bits(s.modulation(), first).all()
        s.set_bands([125.0], 3)
        refused("^modulation: not computed")
        s.compute_modulation()
        assert s.modulation().shape == (70, 70, 1, 15)
        s.set_bands([])
        refused("^modulation: no bands set")
        s.set_bands(BANDS)
        s.compute_modulation()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        refused("^modulation: not computed")
        s.compute_modulation()  # (the last completed run is still the first one)
        assert same_bits(s.modulation(), first).all()
        s.run((7.0, 0.0, 9.5))
        refused("^modulation: not computed")
        s.compute_modulation()
        second, delay = s.modulation(), s.results()[1]
        assert not same_bits(second, first).all()
        check_cells(pvlib, s, second, sample(np.random.default_rng(2), delay < NO_ONSET, 8), delay, "second run")
        s.set_grid_boundary((1, 0, 0, 0))
        refused("^modulation: not computed")
        s.remove_geometry(gid)
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: block outside the map"):
            s.modulation_block(0, 0, s.gx + 1, 1)


def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:  # (a sparse-emitter solver keeps no history)
        s.load_scene(SMALLROOM)
        s.set_emitters([E])
        s.set_bands(BANDS)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: .*history"):
            s.compute_modulation()
        assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_bands(BANDS)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="^modulation: .*onset map"):
            s.compute_modulation()
        assert pvlib.last_error()
        s.run(L)
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (s.set_modulation_frequencies, s.compute_modulation, s.modulation_frequencies):
            with pytest.raises(pvlib.PlaneverbError, match="^modulation: .*slab"):
                call()
            assert pvlib.last_error()
        s.run(L)
        assert s.get_output(E).occlusion > 0


# 8. the command line
def test_cli(pvlib):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + [x for e in E for x in ("--emitter", e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = json.loads(subprocess.run(cmd + ["--bands", "63,125", "--modulation"], capture_output=True, text=True, check=True, cwd=ROOT,
                                    env=env, timeout=300).stdout)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_bands(BANDS)
        s.run((5.0, 0.0, 4.0))
        s.compute_modulation()
        for e, rec in zip(((5.0, 0.0, 6.0), (12.0, 0.0, 9.0)), out["emitters"]):
            m = s.modulation_at(e)
            assert "rt60" in rec and len(rec["bandMetrics"]) == 2 and len(rec["modulation"]["bands"]) == 2
            assert same_bits(np.float32(rec["modulation"]["hz"]), np.float32(pvlib.MODULATION_DEFAULT_HZ)).all()
            for j, band in enumerate(rec["modulation"]["bands"]):
                assert band["hz"] == BANDS[j] and band["fraction"] == 1 and len(band["m"]) == 14
                got = np.array(band["m"] + [band["mti"]], np.float32)
                assert same_bits(got, m[j]).all(), (got, m[j])
    r = subprocess.run(cmd + ["--modulation"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode != 0 and "--bands" in r.stderr
