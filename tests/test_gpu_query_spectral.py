"""GPU (-m gpu): in-run frequency-resolved records of the registered queries -- band metrics, modulation, spectrum
(PvAmdSetQuerySpectralRecords; pv_query_spectral.hip).

Reference A, for every query: the whole-map record of the same cell -- the same listener run, compute_<kind>(), the map at the
query's cell (NaNs for a position off the map).  Reference B, for at least 8 reached queries per test that has them: the host
restatement (api.host_band_metrics, host_modulation, host_spectrum) of the definition applied to impulse_response(cx, cy) with
the run's own onset.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_bands import OCTAVES
from test_gpu_lateral import preset_solver
from test_gpu_layer import cell_of
from test_gpu_lobes import FORMS
from test_gpu_modulation import THIRDS8
from test_gpu_query_records import BOXES4, L_IN, NO_ONSET, cells_of, g71_queries, g71_solver, pick
from test_gpu_query_records import records as old_records
from test_gpu_record_queries import g71_positions
from test_gpu_room_metrics import L400, N400, SMALLROOM
from test_gpu_spectrum import BINS

pytestmark = pytest.mark.gpu

PER = {1: 12, 2: 15, 4: 3}
MOD_HZ = [0.5, 0.7, 1.1, 1.3, 1.7, 2.3, 2.9, 3.7, 4.1, 5.3, 6.1, 7.9, 11.0, 13.0]


def kinds_of(pvlib):
    """kind bit -> (compute + map [gx, gy, n, per] of the whole-map pass, host restatement [n, per] of one response with its onset)"""
    return {
        pvlib.QSPEC_BAND_METRICS: (lambda s: (s.compute_band_metrics(), s.band_metrics())[1],
                                   lambda s, ir, t0: pvlib.host_band_metrics(ir[:, 0], s.fs, t0, s.band_coefs())),
        pvlib.QSPEC_MODULATION: (lambda s: (s.compute_modulation(), s.modulation())[1],
                                 lambda s, ir, t0: pvlib.host_modulation(ir[:, 0], s.fs, t0, s.band_coefs(), s.modulation_frequencies())),
        pvlib.QSPEC_SPECTRUM: (lambda s: (s.compute_spectrum(), s.spectrum())[1],
                               lambda s, ir, t0: pvlib.host_spectrum(ir[:, 0], s.fs, t0, s.spectrum_bins(), s.pulse()[:len(ir)])),
    }


def bits(pvlib, kinds):
    return [k for k in kinds_of(pvlib) if kinds & k]


def records(s, pvlib, kinds):
    return dict((k, s.queried_spectral_records(k)) for k in bits(pvlib, kinds))


def check_against_maps(pvlib, s, size, positions, kinds, recs, ctx, host=8):
    """references A and B for the run the solver has just completed (no run in between: the whole-map passes read the same run)"""
    cells = cells_of(pvlib, size, positions)
    delay = s.results()[1]
    reached = [i for i, c in enumerate(cells) if c is not None and delay[c] < NO_ONSET]
    irs = dict((i, s.impulse_response(*cells[i])) for i in reached[:host])
    assert len(irs) >= min(8, len(reached)), ctx
    for k in bits(pvlib, kinds):
        whole, restate = kinds_of(pvlib)[k]
        m = whole(s)
        got = recs[k]
        assert got.shape == (len(positions),) + m.shape[2:] and got.shape[2] == PER[k] and got.dtype == np.float32, (ctx, k, got.shape)
        want = np.stack([m[c] if c is not None else np.full(m.shape[2:], np.nan, np.float32) for c in cells])
        bad = ~same_bits(got, want)
        assert not bad.any(), "%s kind %d: %d values differ from the whole-map records, first at %s" % (
            ctx, k, bad.sum(), np.argwhere(bad)[0])
        for i in range(len(cells)):  # NaN exactly where the position is off the map or its cell has no onset
            assert np.isnan(got[i]).all() == (i not in reached), (ctx, k, i)
        for i, ir in irs.items():
            assert same_bits(got[i], restate(s, ir, int(delay[cells[i]]))).all(), (ctx, k, i, cells[i])
    # the in-run records are still readable behind the whole-map passes, with the same bits
    for k, r in records(s, pvlib, kinds).items():
        assert same_bits(r, recs[k]).all(), (ctx, k)
    return reached


def settings(s, bands=OCTAVES, fraction=1, bins=BINS[9], mod=None):
    s.set_bands(bands, fraction)
    s.set_spectrum_bins(bins)
    if mod is not None:
        s.set_modulation_frequencies(mod)
    return s


def run_with(s, pvlib, L, positions, kinds):
    s.set_output_queries(positions)
    s.set_query_spectral_records(kinds)
    assert s.query_spectral_kinds() == kinds
    s.run(L)
    return records(s, pvlib, kinds)


_G71 = {}


def g71_records(pvlib):
    """test 1's run: all three kinds, 64 queries by class, three octaves (an odd count: a padded last block of bands), nine bins (one
    slice in the 16-wide register block; test 3 has the two slices of 32); checked where it is made"""
    if "r" not in _G71:
        g = golden("g71_smallroom")
        pos, classes = g71_queries(pvlib)
        size = (float(g["size"]), float(g["size"]))
        with settings(preset_solver(pvlib, g)) as s:
            recs = run_with(s, pvlib, g["listener"], pos, pvlib.QSPEC_ALL)
            assert (s.gx, s.T, s.fs) == (70, 435, 1443)
            reached = check_against_maps(pvlib, s, size, pos, pvlib.QSPEC_ALL, recs, "g71")
            assert set(range(64)) - set(classes["no onset"] + classes["off the map"]) == set(reached) and len(reached) >= 50
            for k, r in recs.items():
                for i, j in zip(classes["duplicate"], (0, classes["random"][0])):
                    assert same_bits(r[i], r[j]).all(), k
        _G71["r"] = recs
    return _G71["r"]


# 1. the query classes on the preset grid: a full wave of queries with widely different onsets, all three kinds at once
def test_query_classes(pvlib):
    recs = g71_records(pvlib)
    assert [recs[k].shape for k in sorted(recs)] == [(64, 3, 12), (64, 3, 15), (64, 9, 3)]


# 2. every kind alone and every pair; no kind; both selectors together
def test_selections(pvlib):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    with settings(g71_solver(pvlib)) as s:
        for kinds in (1, 2, 4, 3, 5, 6):
            recs = run_with(s, pvlib, g["listener"], pos, kinds)
            assert sorted(recs) == bits(pvlib, kinds)
            for k in want:
                if kinds & k:
                    assert same_bits(recs[k], want[k]).all(), (kinds, k)
                else:
                    with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*not selected"):
                        s.queried_spectral_records(k)
        # no spectral kind: the read-back is refused and the six kinds' records are what they are without this feature
        s.set_query_spectral_records(0)
        s.set_query_records(pvlib.QREC_ALL)
        s.run(g["listener"])
        assert s.query_spectral_kinds() == 0
        for k in want:
            with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*not selected"):
                s.queried_spectral_records(k)
        six = old_records(s, pvlib, pvlib.QREC_ALL)
        assert not np.isnan(six[pvlib.QREC_ROOM_METRICS][0]).any()
        # both selectors: neither changes a bit of the other
        s.set_query_spectral_records(pvlib.QSPEC_ALL)
        s.run(g["listener"])
        for k, r in old_records(s, pvlib, pvlib.QREC_ALL).items():
            assert same_bits(r, six[k]).all(), ("six kinds beside the spectral ones", k)
        for k, r in records(s, pvlib, pvlib.QSPEC_ALL).items():
            assert same_bits(r, want[k]).all(), ("spectral kinds beside the six", k)
        # ... and switching either off leaves the other's records of the last run readable
        s.set_query_records(0)
        for k, r in records(s, pvlib, pvlib.QSPEC_ALL).items():
            assert same_bits(r, want[k]).all(), k


# 3. the extremes of the settings
@pytest.mark.parametrize("name", ["one band, one bin", "eight third-octaves, 32 bins", "custom modulation frequencies"])
def test_extremes_of_the_settings(pvlib, name):
    bands, fraction, nbins, mod = {"one band, one bin": ([125.0], 1, 1, None), "eight third-octaves, 32 bins": (THIRDS8, 3, 32, None),
                                   "custom modulation frequencies": (OCTAVES[:2], 1, 8, MOD_HZ)}[name]
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    size = (float(g["size"]), float(g["size"]))
    with settings(preset_solver(pvlib, g), bands, fraction, BINS[nbins], mod) as s:
        assert [s.query_spectral_floats(k) for k in (1, 2, 4)] == [12 * len(bands), 15 * len(bands), 3 * nbins]
        recs = run_with(s, pvlib, g["listener"], pos, pvlib.QSPEC_ALL)
        assert [recs[k].shape[1] for k in sorted(recs)] == [len(bands), len(bands), nbins]
        assert len(check_against_maps(pvlib, s, size, pos, pvlib.QSPEC_ALL, recs, name)) >= 50
        if mod is not None:  # (not the default series' records)
            assert same_bits(s.modulation_frequencies(), np.float32(MOD_HZ)).all()
            assert not same_bits(recs[pvlib.QSPEC_MODULATION][0], g71_records(pvlib)[pvlib.QSPEC_MODULATION][0, :2]).all()


# 4. record queries of their own: a second wave with one query, a partial last group; the output queries beside them
@pytest.mark.parametrize("n", [65, 150])
def test_record_queries(pvlib, n):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    pos, nan = g71_positions(pvlib, n)
    outs = [cell_of(30, 30), cell_of(70, 10), cell_of(12, 40)]
    with settings(preset_solver(pvlib, g)) as s:
        s.set_output_queries(outs)
        s.set_record_queries(pos)
        s.set_query_spectral_records(pvlib.QSPEC_ALL)
        s.run(g["listener"])
        recs = records(s, pvlib, pvlib.QSPEC_ALL)
        assert [recs[k].shape for k in sorted(recs)] == [(n, 3, 12), (n, 3, 15), (n, 9, 3)]
        reached = check_against_maps(pvlib, s, size, pos, pvlib.QSPEC_ALL, recs, "n = %d" % n)
        assert set(range(n)) - nan == set(reached)
        for k, r in recs.items():
            assert same_bits(r[:64], want[k]).all(), (n, k)  # (the first group is test 1's)
            assert same_bits(r[64], r[0]).all() and not np.isnan(r[0]).any(), k  # (the same cell in two groups)
        q = s.queried_outputs()
        assert q.shape == (3, 8)
        for i, e in enumerate(outs):
            if cells_of(pvlib, size, [e])[0] is not None:
                assert same_bits(q[i], s.get_output(e).as_array()).all(), i


# 5. where the cell lies: a history window smaller than the grid, the walled-in window path, a non-square grid
def test_window_smaller_than_the_grid(pvlib):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400["corner"])
        delay = s.results()[1]
        reached = delay < NO_ONSET
        X, Y = np.meshgrid(np.arange(s.gx), np.arange(s.gy), indexing="ij")
        lx, ly = [int(v) for v in np.unravel_index(np.argmin(delay), delay.shape)]
        far = np.maximum(np.abs(X - lx), np.abs(Y - ly))
        classes = {"inside, no onset": ~reached & (far < 100), "outside the window": ~reached & (far > s.T + 40),
                   "late onset": reached & (s.T - delay <= 8), "first row or column": reached & ((X == 0) | (Y == 0))}
        rng = np.random.default_rng(402)
        cells = []
        for name, m in classes.items():
            assert m.any(), name
            cells += pick(rng, m, 5)
        cells += pick(rng, reached, 61 - len(cells))
        pos = [cell_of(*c) for c in cells] + [cell_of(N400, 7), (-0.5, 0.0, 3.0), cell_of(*cells[-1])]
        assert len(pos) == 64
        settings(s)
        recs = run_with(s, pvlib, L400["corner"], pos, pvlib.QSPEC_ALL)
        assert same_bits(s.results()[1], delay).all()
        got = check_against_maps(pvlib, s, (size, size), pos, pvlib.QSPEC_ALL, recs, "400^2 corner", host=24)
        assert len(got) >= 40


def test_resident_window_path(pvlib):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    with settings(preset_solver(pvlib, g, steps_per_launch=12, tile_rows=36, use_graph=2)) as s:
        for b in BOXES4:
            s.add_geometry(b)
        s.run(L_IN)
        assert s.last_run_resident_window()
        reached = s.results()[1] < NO_ONSET
        assert 4 <= reached.sum() < 200
        rng = np.random.default_rng(5)
        cells = pick(rng, reached, 40) + pick(rng, ~reached, 24)
        pos = [cell_of(*c) for c in cells]
        recs = run_with(s, pvlib, L_IN, pos, pvlib.QSPEC_ALL)
        assert s.last_run_resident_window()
        got = check_against_maps(pvlib, s, size, pos, pvlib.QSPEC_ALL, recs, "window path")
        assert got == list(range(min(40, int(reached.sum()))))  # (inside the enclosure: records; outside: NaN)


def test_non_square_grid(pvlib):
    size = (open_size(95), open_size(70))
    L = cell_of(40, 22)
    with pvlib.Solver(size[0], size[1], 275) as s:
        assert (s.gx, s.gy, s.T) == (95, 70, 435)
        s.load_scene(SMALLROOM)
        s.run(L)
        reached = s.results()[1] < NO_ONSET
        rng = np.random.default_rng(95)
        cells = pick(rng, reached, 56) + pick(rng, ~reached, 4) + [(94, 69), (94, 0), (0, 69)]
        pos = [cell_of(*c) for c in cells] + [cell_of(95, 10)]
        settings(s)
        recs = run_with(s, pvlib, L, pos, pvlib.QSPEC_ALL)
        assert len(check_against_maps(pvlib, s, size, pos, pvlib.QSPEC_ALL, recs, "95 x 70")) >= 56


# 6. every stepping path gives the bits of test 1; runs in flight
@pytest.mark.parametrize("form", list(FORMS))
def test_same_bits_on_every_path(pvlib, form):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    pos, _ = g71_queries(pvlib)
    with settings(preset_solver(pvlib, g, **FORMS[form])) as s:
        s.set_output_queries(pos)
        s.set_query_spectral_records(pvlib.QSPEC_ALL)
        s.run_async(g["listener"])
        s.sync()
        for k, r in records(s, pvlib, pvlib.QSPEC_ALL).items():
            assert same_bits(r, want[k]).all(), (form, k)


def test_runs_in_flight(pvlib):
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    L = [tuple(g["listener"]), L_IN]
    pos, _ = g71_queries(pvlib)
    sets = [pos, pos[40:10:-1]]

    def solver():
        return settings(preset_solver(pvlib, g))

    with solver() as s:  # the second listener's records, checked against both references
        second = run_with(s, pvlib, L[1], sets[1], pvlib.QSPEC_ALL)
        assert len(check_against_maps(pvlib, s, size, sets[1], pvlib.QSPEC_ALL, second, "second listener")) >= 8
    plain = [g71_records(pvlib), second]
    # a batch of two solvers with different listeners and different query sets
    solvers = [solver() for _ in L]
    try:
        for s, q in zip(solvers, sets):
            s.set_output_queries(q)
            s.set_query_spectral_records(pvlib.QSPEC_ALL)
        pvlib.run_batch(solvers, L)
        for s, w in zip(solvers, plain):
            for k, r in records(s, pvlib, pvlib.QSPEC_ALL).items():
                assert same_bits(r, w[k]).all(), ("batch", k)
    finally:
        for s in solvers:
            s.close()
    # two iterations in flight on two solvers
    with solver() as a, solver() as b:
        for s, q in ((a, sets[1]), (b, sets[0])):
            s.set_output_queries(q)
            s.set_query_spectral_records(pvlib.QSPEC_ALL)
        a.run_async(L[1])
        b.run_async_after(a, L[0])
        b.sync()
        a.sync()
        for s, w in ((a, plain[1]), (b, plain[0])):
            for k, r in records(s, pvlib, pvlib.QSPEC_ALL).items():
                assert same_bits(r, w[k]).all(), ("pipelined", k)


# 7. settings and lifetime
def test_settings_and_lifetime(pvlib):
    want = g71_records(pvlib)
    g = golden("g71_smallroom")
    size = (float(g["size"]), float(g["size"]))
    pos, _ = g71_queries(pvlib)
    B, M, S = pvlib.QSPEC_BAND_METRICS, pvlib.QSPEC_MODULATION, pvlib.QSPEC_SPECTRUM
    refused = pytest.raises(pvlib.PlaneverbError, match="^spectral records: ")
    with settings(preset_solver(pvlib, g)) as s:
        recs = run_with(s, pvlib, g["listener"], pos, pvlib.QSPEC_ALL)
        for k in want:
            assert same_bits(recs[k], want[k]).all(), k
        # other centres, the same count: the in-run records (one stamp for the block, as for the six kinds) are refused until the
        # next run
        s.set_bands([80.0, 160.0, 315.0])
        for k in (B, M, S):
            with refused:
                s.queried_spectral_records(k)
        s.run(g["listener"])
        moved = records(s, pvlib, pvlib.QSPEC_ALL)
        assert not same_bits(moved[B], want[B]).all() and same_bits(moved[S], want[S]).all()
        check_against_maps(pvlib, s, size, pos, B | M, moved, "other centres")
        # another count: the sizes follow
        s.set_bands(OCTAVES[:2])
        assert [s.query_spectral_floats(k) for k in (B, M, S)] == [24, 30, 27]
        with refused:
            s.queried_spectral_records(B)
        s.run(g["listener"])
        two = records(s, pvlib, pvlib.QSPEC_ALL)
        assert two[B].shape == (64, 2, 12) and same_bits(two[B], want[B][:, :2]).all() and same_bits(two[M], want[M][:, :2]).all()
        # the bins: other frequencies with the same count, then another count
        s.set_spectrum_bins(BINS[9][::-1])
        for k in (B, S):
            with refused:
                s.queried_spectral_records(k)
        s.run(g["listener"])
        assert same_bits(s.queried_spectral_records(S), want[S][:, ::-1]).all()
        assert same_bits(s.queried_spectral_records(B), two[B]).all()
        s.set_spectrum_bins(BINS[32])
        assert s.query_spectral_floats(S) == 96
        with refused:
            s.queried_spectral_records(S)
        s.run(g["listener"])
        wide = records(s, pvlib, S)
        assert wide[S].shape == (64, 32, 3)
        check_against_maps(pvlib, s, size, pos, S, wide, "32 bins")
        # the modulation frequencies: the modulation records alone are refused until the next run
        s.set_modulation_frequencies(MOD_HZ)
        with refused:
            s.queried_spectral_records(M)
        s.run(g["listener"])
        assert same_bits(s.queried_spectral_records(B), two[B]).all()
        mod = records(s, pvlib, M)
        assert not same_bits(mod[M], two[M]).all()
        check_against_maps(pvlib, s, size, pos, M, mod, "modulation frequencies")
        s.set_modulation_frequencies(None)
        s.run(g["listener"])
        assert same_bits(s.queried_spectral_records(M), two[M]).all()
        # neither the bands nor the bins can go while their kinds are selected
        with refused:
            s.set_bands([])
        with refused:
            s.set_spectrum_bins([])
        assert len(s.bands()[0]) == 2 and len(s.spectrum_bins()) == 32
        assert same_bits(s.queried_spectral_records(B), two[B]).all()
        # a failed read-back leaves `out` untouched
        out = np.full((5, 2, 12), 7.0, np.float32)
        assert pvlib.lib().PvAmdGetQueriedSpectralRecords(s._h, B, out.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float)), 5) == -1
        assert pvlib.last_error().startswith("spectral records: ") and (out == 7.0).all()
        # changing the queries: refused until the next run
        s.set_output_queries(pos[:5])
        with refused:
            s.queried_spectral_records(B)
        s.run(g["listener"])
        assert same_bits(s.queried_spectral_records(B), two[B][:5]).all()
        # no kinds: nothing is recorded, every read is refused, and the settings may go
        s.set_query_spectral_records(0)
        s.run(g["listener"])
        with refused:
            s.queried_spectral_records(B)
        s.set_bands([])
        s.set_spectrum_bins([])


# 8. refusals: a "spectral records: ..." message each
def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*unknown"):
            s.set_query_spectral_records(8)
        for k in (pvlib.QSPEC_BAND_METRICS, pvlib.QSPEC_MODULATION):
            with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*no bands set"):
                s.set_query_spectral_records(k)
            with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*no bands set"):
                s.query_spectral_floats(k)
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*no bins set"):
            s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM)
        assert s.query_spectral_kinds() == 0
        settings(s, OCTAVES[:1], 1, BINS[1])
        s.set_output_queries([E])
        s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM)
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: "):
            s.queried_spectral_records(pvlib.QSPEC_SPECTRUM)  # (no run yet)
        s.run(L)
        assert np.isfinite(s.queried_spectral_records(pvlib.QSPEC_SPECTRUM)).all()
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*not selected"):
            s.queried_spectral_records(pvlib.QSPEC_MODULATION)
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*one kind"):
            s.queried_spectral_records(pvlib.QSPEC_ALL)
        out = np.zeros((2, 1, 3), np.float32)  # a count mismatch
        assert pvlib.lib().PvAmdGetQueriedSpectralRecords(s._h, pvlib.QSPEC_SPECTRUM, out.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float)),
                                                         2) == -1
        assert pvlib.last_error().startswith("spectral records: count differs")
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*history"):
            s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM)
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*onset map"):
            s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM)
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        for call in (lambda: s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM), lambda: s.query_spectral_floats(1),
                     lambda: s.queried_spectral_records(pvlib.QSPEC_SPECTRUM)):
            with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*slab"):
                call()


# 9. the command line: --in-run-records serves the three kinds as well, equal to the API's records
def test_cli(pvlib):
    emitters = [(5.0, 0.0, 6.0), (12.0, 0.0, 9.0), (40.0, 0.0, 3.0)]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4", "--in-run-records", "--bands", "63,125",
           "--modulation", "--spectrum", "50,100"]
    for e in emitters:
        cmd += ["--emitter", ",".join("%g" % v for v in e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout
    rec = json.loads(out)["emitters"]
    assert len(rec) == 3 and all(k in r for r in rec for k in ("bandMetrics", "modulation", "spectrum"))
    with settings(pvlib.Solver(25.0, 25.0, 275), [63.0, 125.0], 1, [50.0, 100.0]) as s:
        s.load_scene(SMALLROOM)
        api = run_with(s, pvlib, (5.0, 0.0, 4.0), emitters, pvlib.QSPEC_ALL)
    for i, r in enumerate(rec):
        band = np.float32([[b[n] for n in pvlib.BAND_METRIC_NAMES] for b in r["bandMetrics"]])
        mod = np.float32([b["m"] + [b["mti"]] for b in r["modulation"]["bands"]])
        spec = np.float32([r["spectrum"]["re"], r["spectrum"]["im"], r["spectrum"]["levelDb"]]).T
        assert same_bits(band, api[pvlib.QSPEC_BAND_METRICS][i]).all(), i
        assert same_bits(mod, api[pvlib.QSPEC_MODULATION][i]).all(), i
        assert same_bits(spec, api[pvlib.QSPEC_SPECTRUM][i]).all(), i
    assert np.isfinite(rec[0]["spectrum"]["levelDb"]).all() and np.isnan(rec[2]["bandMetrics"][0]["edt"])
