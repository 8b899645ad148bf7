"""GPU (-m gpu): source arrays (PvAmdSetArrays / PvAmdComputeArrays; pv_arrays.hip, the mix lane of the query record kernels).

The expected values come from the numpy restatement (tests/_arrays_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t), and from PvAmdHost<Kind> on the
restated response with its restated onset.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _adversarial as adv
import _arrays_ref as ref
import test_gpu_analysis_maps as maps
from conftest import ROOT, SCENES, bits, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_emitter_records import edge_case_cells
from test_gpu_layer import cell_of
from test_gpu_parity import fuse_opts
from test_gpu_spectrum import L400, N400

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
NO_ONSET = 1e30
BANDS = (63.0, 125.0)
BINS = (31.5, 100.0, 250.0)
OFF_MAP = (-3.0, 0.0, 4.0)


def history(s):
    return np.stack([s.history_plane(t) for t in range(s.T)])


def kinds_of(pvlib):
    """(spectral, kind bit, host restatement of one response) of the six kinds"""
    return [(False, pvlib.QREC_ROOM_METRICS, lambda s, y, t0: pvlib.host_room_metrics(y, s.fs, t0)),
            (False, pvlib.QREC_DECAY_TIMES, lambda s, y, t0: pvlib.host_decay_times(y, s.fs, t0)),
            (False, pvlib.QREC_ECHO_CRITERION, lambda s, y, t0: pvlib.host_echo_criterion(y, s.fs, t0)),
            (True, pvlib.QSPEC_BAND_METRICS, lambda s, y, t0: pvlib.host_band_metrics(y, s.fs, t0, s.band_coefs())),
            (True, pvlib.QSPEC_MODULATION, lambda s, y, t0: pvlib.host_modulation(y, s.fs, t0, s.band_coefs(), s.modulation_frequencies())),
            (True, pvlib.QSPEC_SPECTRUM, lambda s, y, t0: pvlib.host_spectrum(y, s.fs, t0, s.spectrum_bins(), s.pulse()))]


def configure(pvlib, s):
    s.set_bands(BANDS, 1)
    s.set_spectrum_bins(BINS)
    s.set_array_records(pvlib.QREC_ROOM_METRICS | pvlib.QREC_DECAY_TIMES | pvlib.QREC_ECHO_CRITERION, pvlib.QSPEC_ALL)
    return s


def members_at(arrays):
    """[[(cell, gain, delay)]] -> what set_arrays takes"""
    return [[(cell_of(*c), g, d) for c, g, d in a] for a in arrays]


def restate(s, hist, arrays, interp):
    """per array: (response, onset) of the numpy restatement on the solver's own planes; the solver's taps are checked on the way"""
    out = []
    for i, a in enumerate(arrays):
        tm, td, tw = ref.expand([(g, d) for _, g, d in a], s.fs, s.T, interp)
        gm, gd, gw = s.array_taps(i)
        assert np.array_equal(gm, tm) and np.array_equal(gd, td) and np.array_equal(bits(gw), bits(tw)), i
        rows = np.stack([hist[:, c[0], c[1]] for c, _, _ in a])
        y = ref.response(rows, tm, td, tw)
        out.append((y, ref.onset(y)))
    return out


def check(pvlib, s, want, ctx, records=True):
    """responses, onsets and the selected records of the last compute_arrays against `want` = [(y, onset)]"""
    onsets = s.array_onsets()
    assert onsets.dtype == np.float32 and len(onsets) == len(want)
    for i, (y, on) in enumerate(want):
        got = s.array_response(i)
        bad = ~same_bits(got, y)
        assert not bad.any(), "%s array %d: %d steps differ, first at %s: %s vs %s" % (ctx, i, bad.sum(), np.argwhere(bad)[0], got[bad][:4], y[bad][:4])
        assert bits(onsets[i]) == bits(on), (ctx, i, onsets[i], on)
    if not records:
        return
    tk, sk = s.array_record_kinds()
    for spectral, kind, host in kinds_of(pvlib):
        if not ((sk if spectral else tk) & kind):
            continue
        got = s.array_records(kind, spectral=spectral)
        assert got.shape[0] == len(want)
        for i, (y, on) in enumerate(want):
            if on == ref.FLT_MAX:
                assert np.isnan(got[i]).all(), (ctx, i, kind)
                continue
            exp = np.asarray(host(s, y, int(on)), np.float32).reshape(-1)
            assert same_bits(got[i], exp).all(), (ctx, "array %d" % i, "spectral" if spectral else "time", kind, got[i][:6], exp[:6])


def preset_arrays(s, delay, beta):
    """the arrays of test 1, as [[(cell, gain, delaySeconds)]]"""
    fs, T = s.fs, s.T
    ec = edge_case_cells({"delay": delay, "beta": beta}, s.info.tileRows, s.info.tileCols) if (beta[:s.gx, :s.gy] == 0).any() else {}
    reached = [tuple(int(v) for v in c) for c in np.argwhere(delay < NO_ONSET)]
    pool = list(ec.values()) + [reached[i] for i in np.linspace(0, len(reached) - 1, 64).astype(int)]
    c0, c1, c2, c3 = (reached[i] for i in np.linspace(0, len(reached) - 1, 4).astype(int))
    dead = ec.get("wall", ec.get("unreached"))
    if dead is None:  # (an open grid: no wall and every cell reached)
        idx = np.argwhere(~(delay < NO_ONSET))
        dead = tuple(int(v) for v in idx[0]) if len(idx) else None
    rng = np.random.default_rng(7)
    dl = lambda k: float(np.float32(k / fs))
    frac = lambda: dl(rng.uniform(1.01, 0.2 * T))
    arrays = [[(c0, 1.0, 0.0)],                                        # the identity array
              [(c0, 0.7, 0.0), (c0, -0.7, 0.0)],                       # the cancelling pair: dead by construction
              [(c1, 0.8, 0.0), (c2, -0.5, dl(7.3))],                   # two members, a polarity flip, a fractional delay
              [(pool[i % len(pool)], float(rng.uniform(-1, 1)), (0.0, dl(5), frac())[i % 3]) for i in range(17)],
              [(pool[i % len(pool)], float(rng.uniform(-1, 1)), (frac(), 0.0, dl(31))[i % 3]) for i in range(64)],
              [(c1, 1.0, 0.0), (c2, 0.5, dl(T - 1.5))],                # the largest tap passes T
              [(c1, 1.0, dl(0.6 * T))],                                # a delay beyond every onset (260 steps at T = 435)
              [(c0, 0.5, dl(3.37)), (c3, 1.0, 0.0)],                   # c0 again: one cell in two arrays
              [(c3, -1.0, dl(2.0))]]
    for k, c in ec.items():                                            # a tile's first row and column, a corner, the wall faces ...
        arrays.append([(c, 0.9, dl(1.5)), (c2, 0.25, 0.0)] if k in ("wall", "unreached") else [(c, 0.9, dl(1.5))])
    if dead is not None:
        arrays.append([(dead, 1.0, 0.0)])                              # a wall cell, or a cell without an onset, alone
    return arrays


# 1. the 70^2 presets (T = 435: not a multiple of 64)
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    g = golden(name)
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        assert (s.gx, s.T, s.fs) == (70, 435, 1443)
        for b in g["boxes"]:
            s.add_geometry(b)
        configure(pvlib, s)
        s.run(g["listener"])
        hist, delay, beta = history(s), s.results()[1], s.material()[0]
        arrays = preset_arrays(s, delay, beta)
        for interp in (pvlib.ARRAY_LAGRANGE3, pvlib.ARRAY_NEAREST):
            s.set_arrays(members_at(arrays), interp)
            count, got_interp = s.arrays()
            assert list(count) == [len(a) for a in arrays] and got_interp == interp
            assert s.compute_arrays() > 0
            want = restate(s, hist, arrays, interp)
            check(pvlib, s, want, "%s interp=%d" % (name, interp))
            live = np.array([on != ref.FLT_MAX for _, on in want])
            assert live.sum() >= 8 and not live.all(), live
            assert not live[1] and (bits(want[1][0]) == 0).all()  # the cancelling pair
            assert same_bits(want[0][0], hist[:, arrays[0][0][0][0], arrays[0][0][0][1]]).all()  # the identity
            assert max(s.array_taps(5)[1]) >= s.T if interp == pvlib.ARRAY_LAGRANGE3 else True
            # NaN records on exactly the arrays without an onset
            rm = s.array_records(pvlib.QREC_ROOM_METRICS)
            assert np.array_equal(np.isnan(rm).all(axis=1), ~live) and np.isfinite(rm[live][:, 4:]).all()


# 2. lane groups: 1, 64, 65 and 256 arrays; an array's bits depend on neither the other arrays nor its index
def test_lane_groups(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        configure(pvlib, s)
        s.run(g["listener"])
        hist, delay = history(s), s.results()[1]
        reached = [tuple(int(v) for v in c) for c in np.argwhere(delay < NO_ONSET)]
        rng = np.random.default_rng(3)
        dl = lambda k: float(np.float32(k / s.fs))
        target = [(reached[len(reached) // 3], 0.8, dl(4.6)), (reached[len(reached) // 2], -0.6, 0.0), (reached[5], 0.3, dl(20.2))]
        others = [[(reached[int(rng.integers(0, len(reached)))], float(rng.uniform(-1, 1)), dl(rng.uniform(1.01, 50.0)))
                   for _ in range(int(rng.integers(1, 4)))] for _ in range(255)]

        def snapshot(i):
            return [s.array_response(i), s.array_onsets()[i:i + 1]] + [s.array_records(k, spectral=sp)[i] for sp, k, _ in kinds_of(pvlib)]

        s.set_arrays(members_at([target]))
        s.compute_arrays()
        check(pvlib, s, restate(s, hist, [target], pvlib.ARRAY_LAGRANGE3), "alone")
        alone = snapshot(0)
        assert alone[1][0] != ref.FLT_MAX
        for n in (64, 65, 256):
            first = [target] + others[:n - 1]
            s.set_arrays(members_at(first))
            s.compute_arrays()
            if n == 65:  # (two groups, the second with one array: everything against the restatement)
                check(pvlib, s, restate(s, hist, first, pvlib.ARRAY_LAGRANGE3), "65 arrays")
            for a, b in zip(snapshot(0), alone):
                assert same_bits(a, b).all(), n
            last = [others[i] for i in rng.permutation(n - 1)] + [target]
            s.set_arrays(members_at(last))
            s.compute_arrays()
            for a, b in zip(snapshot(n - 1), alone):
                assert same_bits(a, b).all(), n


# 3. identity: the one-member array's records are the whole-map records at the member's cell
def test_identity_against_the_whole_map(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        configure(pvlib, s)
        s.run(g["listener"])
        delay = s.results()[1]
        reached = [tuple(int(v) for v in c) for c in np.argwhere(delay < NO_ONSET)]
        cells = [reached[i] for i in np.linspace(0, len(reached) - 1, 70).astype(int)]
        s.set_arrays(members_at([[(c, 1.0, 0.0)] for c in cells]))
        s.compute_arrays()
        assert np.array_equal(s.array_onsets(), np.array([delay[c] for c in cells], np.float32))
        whole = [(False, pvlib.QREC_ROOM_METRICS, s.compute_room_metrics, s.room_metrics_at),
                 (False, pvlib.QREC_DECAY_TIMES, s.compute_decay_times, s.decay_times_at),
                 (False, pvlib.QREC_ECHO_CRITERION, s.compute_echo_criterion, s.echo_criterion_at),
                 (True, pvlib.QSPEC_BAND_METRICS, s.compute_band_metrics, s.band_metrics_at),
                 (True, pvlib.QSPEC_MODULATION, s.compute_modulation, s.modulation_at),
                 (True, pvlib.QSPEC_SPECTRUM, s.compute_spectrum, s.spectrum_at)]
        for spectral, kind, compute, at in whole:
            compute()
            got = s.array_records(kind, spectral=spectral)  # (the map passes do not invalidate the arrays)
            for i, c in enumerate(cells):
                assert same_bits(got[i], np.asarray(at(cell_of(*c)), np.float32).reshape(-1)).all(), (kind, c)


# 4. a history window smaller than the grid, and a non-square grid
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        configure(pvlib, s)
        s.run(L400[where])
        hist, delay = history(s), s.results()[1]
        reached = [tuple(int(v) for v in c) for c in np.argwhere(delay < NO_ONSET)]
        cells = [reached[i] for i in np.linspace(0, len(reached) - 1, 12).astype(int)]
        assert len(set((c[0] // s.info.tileRows, c[1] // s.info.tileCols) for c in cells)) >= 3
        far = (10, 398) if where == "offset" else (398, 398)  # inside the grid, outside the window: zeros
        assert delay[far] >= NO_ONSET and not hist[:, far[0], far[1]].any()
        dl = lambda k: float(np.float32(k / s.fs))
        arrays = [[(c, 1.0, 0.0)] for c in cells[:4]] + [[(c, 0.5, dl(2.5 + i)) for i, c in enumerate(cells)],
                                                          [(far, 1.0, 0.0)], [(cells[6], 1.0, dl(3.3)), (far, 1.0, 0.0)]]
        s.set_arrays(members_at(arrays))
        s.compute_arrays()
        want = restate(s, hist, arrays, pvlib.ARRAY_LAGRANGE3)
        check(pvlib, s, want, where)
        assert want[5][1] == ref.FLT_MAX and want[6][1] != ref.FLT_MAX


def test_non_square_grid(pvlib):
    from test_gpu_non_square import XCD, listeners, solver
    for g in (XCD, XCD[::-1]):
        with solver(pvlib, g) as s:
            configure(pvlib, s)
            s.run(listeners(g)[0])
            hist, delay = history(s), s.results()[1]
            reached = [tuple(int(v) for v in c) for c in np.argwhere(delay < NO_ONSET)]
            cells = [reached[i] for i in np.linspace(0, len(reached) - 1, 9).astype(int)]
            dl = lambda k: float(np.float32(k / s.fs))
            arrays = [[(c, 1.0, 0.0)] for c in cells[:3]] + [[(c, -0.4, dl(1.7 * (i + 1))) for i, c in enumerate(cells)]]
            s.set_arrays(members_at(arrays))
            s.compute_arrays()
            check(pvlib, s, restate(s, hist, arrays, pvlib.ARRAY_LAGRANGE3), "%dx%d" % g)


# 5. injected histories: every family of tests/_adversarial.py, non-finite samples included
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_injected_histories(pvlib):
    with maps.make_solver(pvlib) as s:
        configure(pvlib, s)
        s.run(maps.LISTENER)
        new, fam, delay = adv.inject(s, 20261021)
        hist = history(s)  # (what PvAmdCopyHistoryPlane returns now: the planes set, where the run stored a cell)
        finite = np.isfinite(hist).all(axis=0)
        assert not finite.all()
        arrays, poisoned = [], []
        dl = lambda k: float(np.float32(k / s.fs))
        for f in range(len(adv.FAMILIES)):
            idx = np.argwhere(fam[:s.gx, :s.gy] == f)
            assert len(idx) >= 3, adv.FAMILIES[f]
            c = [tuple(int(v) for v in idx[i]) for i in np.linspace(0, len(idx) - 1, 3).astype(int)]
            arrays += [[(c[0], 1.0, 0.0)], [(c[0], 0.6, dl(3.4)), (c[1], -0.8, 0.0), (c[2], 0.5, dl(11.0))]]
            poisoned += [not finite[c[0]], not all(finite[x] for x in c)]
        assert any(poisoned) and not all(poisoned)
        s.set_arrays(members_at(arrays))
        s.compute_arrays()
        want = restate(s, hist, arrays, pvlib.ARRAY_LAGRANGE3)
        check(pvlib, s, want, "injected", records=False)
        clean = [i for i, p in enumerate(poisoned) if not p]
        kept = [(s.array_response(i), s.array_onsets()[i]) for i in clean]
        # the records of the arrays whose members are finite, against the host restatements
        for spectral, kind, host in kinds_of(pvlib):
            got = s.array_records(kind, spectral=spectral)
            for i in clean:
                y, on = want[i]
                exp = np.full(got.shape[1], np.nan, np.float32) if on == ref.FLT_MAX else np.asarray(host(s, y, int(on)), np.float32).reshape(-1)
                assert same_bits(got[i], exp).all(), (kind, i, adv.FAMILIES[i // 2])
        # without the arrays that hold a NaN member the others keep their bits
        s.set_arrays(members_at([arrays[i] for i in clean]))
        s.compute_arrays()
        for j, (y, on) in enumerate(kept):
            assert same_bits(s.array_response(j), y).all() and bits(s.array_onsets()[j]) == bits(on)


# 6. sparse-emitter mode: the emitters' traces as the sample source, against a second solver that keeps its history
def smallroom(pvlib, **base):
    def make(**opts):
        s = pvlib.Solver(25.0, 25.0, 275, **dict(base, **opts))
        s.load_scene(SMALLROOM)
        return s
    return make


def sparse_case(pvlib, make, L, beside, ctx):
    with make() as full:
        configure(pvlib, full)
        full.run(L)
        delay, beta = full.results()[1], full.material()[0]
        arrays = preset_arrays(full, delay, beta)
        full.set_arrays(members_at(arrays))
        full.compute_arrays()
        want = [(full.array_response(i), full.array_onsets()[i]) for i in range(len(arrays))]
        with make(streaming_analysis=1) as st:
            configure(pvlib, st)
            cells = sorted(set(c for a in arrays for c, _, _ in a))
            st.set_emitters([OFF_MAP] + [cell_of(*c) for c in cells])
            if beside:
                st.set_echogram(0.005, 16)
                st.set_emitter_records(pvlib.QREC_ALL, pvlib.QSPEC_ALL)
                st.set_zones(pvlib.zone_labels_from_rects(st.dx, st.gx, st.gy, [(2.0, 2.0, 9.0, 9.0)]), 1)
                st.set_zone_curves(True)
            st.set_arrays(members_at(arrays))
            st.run(L)
            assert st.compute_arrays() > 0
            for i, (y, on) in enumerate(want):
                assert same_bits(st.array_response(i), y).all(), (ctx, i)
            assert np.array_equal(bits(st.array_onsets()), bits(np.array([on for _, on in want], np.float32)))
            for spectral, kind, _ in kinds_of(pvlib):
                assert same_bits(st.array_records(kind, spectral=spectral), full.array_records(kind, spectral=spectral)).all(), (ctx, kind)
            if beside:  # nothing interferes: the emitter records are there as well
                assert st.emitter_records(pvlib.QREC_ROOM_METRICS).shape[0] == len(cells)
            live = np.array([on != ref.FLT_MAX for _, on in want])
            assert live.sum() >= 8 and not live.all()


@pytest.mark.parametrize("fuse", [0, 1])
def test_sparse_smallroom(pvlib, fuse):
    make = smallroom(pvlib)

    def make_fused(**opts):
        if opts.get("streaming_analysis"):
            opts.update(fuse_opts(fuse))
        return make(**opts)

    with make_fused(streaming_analysis=1) as st:
        assert st.info.streamFuse == fuse
    sparse_case(pvlib, make_fused, (5.0, 0.0, 4.0), fuse == 1, "fuse=%d" % fuse)


def test_sparse_cut_short(pvlib):
    sparse_case(pvlib, smallroom(pvlib, num_steps=100), (5.0, 0.0, 4.0), False, "num_steps=100")


def test_sparse_member_without_an_emitter(pvlib):
    L, E = (5.0, 0.0, 4.0), [(5.0, 0.0, 6.0), (12.0, 0.0, 9.0)]
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_emitters(E)
        s.set_arrays([[(E[0], 1.0, 0.0)], [(E[1], 1.0, 0.0), ((7.0, 0.0, 7.0), 0.5, 0.0)]])
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no completed run"):
            s.compute_arrays()
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="arrays: array 1, member 1: .*registered emitter"):
            s.compute_arrays()
        s.set_arrays([[(E[0], 1.0, 0.0)], [(E[1], 1.0, 0.0), (E[0], 0.5, 0.0)]])
        s.compute_arrays()
        one = s.array_response(0)
        assert same_bits(one, s.emitter_trace(0)).all() and np.abs(one).max() > 0
        s.set_emitters(E + [(7.0, 0.0, 7.0)])  # a change of the emitters: the traces are the old table's
        with pytest.raises(pvlib.PlaneverbError, match="arrays: not computed"):
            s.array_response(0)
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no completed run"):
            s.compute_arrays()
        s.run(L)
        s.compute_arrays()
        assert same_bits(s.array_response(0), one).all()


# 7. lifetime and refusals
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    E = [tuple(e) for e in g["emitters"]][:3]
    A = [[(E[0], 1.0, 0.0)], [(E[1], 0.5, 0.002), (E[2], -0.5, 0.0)]]
    stale = "arrays: not computed"
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        assert s.arrays() is None
        configure(pvlib, s)
        s.set_arrays(A)
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no completed run"):
            s.compute_arrays()
        s.run(g["listener"])
        with pytest.raises(pvlib.PlaneverbError, match=stale):
            s.array_onsets()
        s.compute_arrays()
        first = [s.array_response(i) for i in range(2)], s.array_onsets(), s.array_records(pvlib.QSPEC_MODULATION, spectral=True)
        assert np.isfinite(first[2]).all()

        def fresh(ctx):
            s.compute_arrays()
            assert all(same_bits(s.array_response(i), first[0][i]).all() for i in range(2)), ctx
            assert same_bits(s.array_records(pvlib.QSPEC_MODULATION, spectral=True), first[2]).all(), ctx

        def is_stale():
            for call in (lambda: s.array_response(0), s.array_onsets, lambda: s.array_records(pvlib.QREC_ROOM_METRICS)):
                with pytest.raises(pvlib.PlaneverbError, match=stale):
                    call()

        # read-backs whose count, kind or array do not match
        out = np.zeros(64, np.float32)
        fp = out.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float))
        L = pvlib.lib()
        assert L.PvAmdGetArrayOnsets(s._h, fp, 3) == -1 and "count" in pvlib.last_error()
        assert L.PvAmdGetArrayRecords(s._h, 0, pvlib.QREC_ROOM_METRICS, fp, 1) == -1 and "count" in pvlib.last_error()
        assert L.PvAmdGetArrayRecords(s._h, 0, 3, fp, 2) == -1 and "exactly one kind" in pvlib.last_error()
        assert L.PvAmdGetArrayRecords(s._h, 2, 1, fp, 2) == -1 and "family" in pvlib.last_error()
        assert L.PvAmdCopyArrayResponse(s._h, 2, fp) == -1 and "no such array" in pvlib.last_error()
        assert L.PvAmdGetArrayTaps(s._h, -1, None, None, None, 0) == -1
        assert L.PvAmdArrayRecordFloats(s._h, 0, pvlib.QREC_LATERAL) == -1
        assert L.PvAmdArrayRecordFloats(s._h, 0, pvlib.QREC_DECAY_TIMES) == 8 and L.PvAmdArrayRecordFloats(s._h, 1, pvlib.QSPEC_SPECTRUM) == 9
        # a failed setter keeps the old setting and what was computed
        bad = [dict(arrays=[[]]), dict(arrays=[[(E[0], 1.0, 0.0)] * 65]), dict(arrays=[[(E[0], 1.0, 0.0)]] * 257),
               dict(arrays=[[(OFF_MAP, 1.0, 0.0)]]), dict(arrays=[[(E[0], float("nan"), 0.0)]]), dict(arrays=[[(E[0], 1.0, float("inf"))]]),
               dict(arrays=[[(E[0], 1.0, -0.001)]]), dict(arrays=[[(E[0], 1.0, s.T / s.fs + 0.001)]]), dict(arrays=[[(E[0], 1.0, 0.4 / s.fs)]]),
               dict(arrays=[[(E[0], 1.0, (s.T - 0.25) / s.fs)]], interp=pvlib.ARRAY_NEAREST), dict(arrays=A, interp=2)]
        for b in bad:
            with pytest.raises(pvlib.PlaneverbError, match="arrays:"):
                s.set_arrays(b["arrays"], b.get("interp", pvlib.ARRAY_LAGRANGE3))
        assert L.PvAmdSetArrays(s._h, None, 1, fp, 0) == -1 and L.PvAmdSetArrays(s._h, np.ones(1, np.int32).ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_int)), 1, None, 0) == -1
        assert list(s.arrays()[0]) == [1, 2]
        assert same_bits(s.array_response(1), first[0][1]).all()
        # refused kinds
        for tk, sk in ((pvlib.QREC_LATERAL, 0), (pvlib.QREC_ECHOGRAM, 0), (pvlib.QREC_LOBES, 0), (64, 0), (0, 8)):
            with pytest.raises(pvlib.PlaneverbError, match="arrays: .*(velocity|unknown)"):
                s.set_array_records(tk, sk)
        assert same_bits(s.array_records(pvlib.QSPEC_MODULATION, spectral=True), first[2]).all()
        # invalidation: the setter, the kinds, bands, modulation frequencies, bins, geometry, a run
        s.set_arrays(A)
        is_stale()
        fresh("setter")
        s.set_array_records(pvlib.QREC_ROOM_METRICS, pvlib.QSPEC_MODULATION)
        is_stale()
        s.compute_arrays()
        with pytest.raises(pvlib.PlaneverbError, match="arrays: the kind is not selected"):
            s.array_records(pvlib.QREC_DECAY_TIMES)
        configure(pvlib, s)
        fresh("kinds")
        s.set_bands(BANDS, 1)
        is_stale()
        fresh("bands")
        s.set_modulation_frequencies(None)
        is_stale()
        fresh("modulation frequencies")
        s.set_spectrum_bins(BINS)
        is_stale()
        fresh("bins")
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        is_stale()
        fresh("geometry")  # (the last completed run is still the first one)
        s.remove_geometry(gid)
        s.run((7.0, 0.0, 9.5))
        is_stale()
        s.compute_arrays()
        assert not same_bits(s.array_response(0), first[0][0]).all()
        # a band or spectrum kind without bands or bins
        s.set_array_records(0, 0)
        s.set_bands([], 1)
        s.set_spectrum_bins([])
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no bands set"):
            s.set_array_records(0, pvlib.QSPEC_BAND_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no bins set"):
            s.set_array_records(0, pvlib.QSPEC_SPECTRUM)
        s.compute_arrays()  # (no kind: the mix and the onsets alone)
        assert np.abs(s.array_response(0)).max() > 0
        # cleared
        s.set_arrays([])
        assert s.arrays() is None
        for call in (s.compute_arrays, lambda: s.array_response(0), s.array_onsets):
            with pytest.raises(pvlib.PlaneverbError, match="arrays: no setting"):
                call()


def test_runs_are_unchanged(pvlib):
    """with arrays set, a run's outputs, result map, history and in-run records keep every bit; with none set (never, or cleared)
    a run's launches are those of a solver that never called the setter"""
    g = golden("g71_smallroom")
    E = [tuple(e) for e in g["emitters"]][:3]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s, \
            pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as plain:
        for sv in (s, plain):
            for b in g["boxes"]:
                sv.add_geometry(b)
            sv.set_bands(BANDS, 1)
            sv.set_spectrum_bins(BINS)
            sv.set_output_queries(E)
            sv.set_query_records(pvlib.QREC_ROOM_METRICS | pvlib.QREC_DECAY_TIMES)
            sv.set_query_spectral_records(pvlib.QSPEC_ALL)

        def both(L):
            for sv in (s, plain):
                sv.run(L)
            for a, b in zip(s.results(), plain.results()):
                assert same_bits(a, b).all(), L
            assert same_bits(s.history_plane(200), plain.history_plane(200)).all()
            assert same_bits(s.queried_records(pvlib.QREC_DECAY_TIMES), plain.queried_records(pvlib.QREC_DECAY_TIMES)).all()
            assert same_bits(s.queried_spectral_records(pvlib.QSPEC_MODULATION), plain.queried_spectral_records(pvlib.QSPEC_MODULATION)).all()
            for e in E:
                assert s.get_output(e).rt60 == plain.get_output(e).rt60
            a, b = s.timings(), plain.timings()
            for name, _ in a._fields_:
                v, w = getattr(a, name), getattr(b, name)
                if isinstance(v, int):  # (launch and step counts: the same work was enqueued)
                    assert v == w, name

        s.set_arrays([[(E[0], 1.0, 0.0)], [(E[1], 0.5, 0.002), (E[2], -0.5, 0.0)]])
        s.set_array_records(pvlib.QREC_ROOM_METRICS, pvlib.QSPEC_ALL)
        both(tuple(g["listener"]))
        s.compute_arrays()
        both((7.0, 0.0, 9.5))
        s.compute_arrays()
        s.set_arrays([])
        both((6.0, 0.0, 5.0))


def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    A = [[(E, 1.0, 0.0)]]
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.run(L)
        for call in (lambda: s.set_arrays(A), lambda: s.set_array_records(1, 0), s.compute_arrays):
            with pytest.raises(pvlib.PlaneverbError, match="arrays: .*onset map"):
                call()
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_arrays(A), lambda: s.set_array_records(1, 0), s.compute_arrays, s.arrays, lambda: s.array_taps(0),
                     lambda: s.array_response(0), s.array_record_kinds):
            with pytest.raises(pvlib.PlaneverbError, match="arrays: .*slab"):
                call()
        assert s.get_output(E).occlusion > 0
    s512 = open_size(512)
    rank = pvlib.SlabRank(s512, s512, 275, 0, 0, 2, pvlib.compute_efree(s512, s512, 275))
    try:
        for call in (lambda: rank.solver.set_arrays(A), rank.solver.compute_arrays, rank.solver.arrays, lambda: rank.solver.array_taps(0),
                     rank.solver.array_record_kinds, rank.solver.array_onsets):
            with pytest.raises(pvlib.PlaneverbError, match="^arrays: slab rank"):
                call()
    finally:
        rank.close()
    # (the echo criterion's sampling-rate floor has no test: no grid the library accepts -- resolution 275 and up -- has fs below 112;
    # the refusal is the selectors' own, Solver::recordKindsRefusal, with the prefix replaced)
    # (the refusal of a last run that ended in error has no test: nothing makes a run fail short of a device fault)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_arrays(A)
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="arrays: no completed run"):
            s.compute_arrays()
        s.run(L)
        assert s.compute_arrays() > 0


# 8. the command line
@pytest.mark.parametrize("sparse", [False, True], ids=["history", "sparse-emitters"])
def test_cli(pvlib, sparse):
    L, E = "5,0,4", ["5,0,6", "12,0,9"]
    A = ["5,6,1,0", "5,6,0.5,0.003;12,9,-0.5,0;7,7,0.25,0.0101", "5,6,1,0;5,6,-1,0"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + ["--emitter=" + e for e in E] + ["--array=" + a for a in A]
    cmd += ["--room-metrics", "--decay-times", "--echo-criterion", "--bands", "63,125", "--modulation", "--spectrum", "31.5,100,250"]
    cmd += ["--sparse-emitters"] if sparse else []
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout)
    arrays = [[((float(x), 0.0, float(z)), float(gn), float(d)) for x, z, gn, d in (m.split(",") for m in a.split(";"))] for a in A]
    assert len(out["emitters"]) == 2 and len(out["arrays"]) == 3
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        configure(pvlib, s)
        s.run((5.0, 0.0, 4.0))
        s.set_arrays(arrays)
        s.compute_arrays()
        onsets = s.array_onsets()
        rm, dt, ec = (s.array_records(k) for k in (pvlib.QREC_ROOM_METRICS, pvlib.QREC_DECAY_TIMES, pvlib.QREC_ECHO_CRITERION))
        bm = s.array_records(pvlib.QSPEC_BAND_METRICS, spectral=True).reshape(3, 2, 12)
        mo = s.array_records(pvlib.QSPEC_MODULATION, spectral=True).reshape(3, 2, 15)
        sp = s.array_records(pvlib.QSPEC_SPECTRUM, spectral=True).reshape(3, 3, 3)
        for i, rec in enumerate(out["arrays"]):
            assert list(rec)[:4] == ["members", "interp", "taps", "onset"] and rec["interp"] == "lagrange3"
            assert rec["taps"]["delaySteps"] == [int(v) for v in s.array_taps(i)[1]]
            assert (rec["onset"] is None) == (onsets[i] == ref.FLT_MAX) and (rec["onset"] is None or rec["onset"] == onsets[i])
            f32 = lambda v: np.array(v, np.float32)
            assert same_bits(f32(list(rec["roomMetrics"].values())), rm[i]).all()
            assert same_bits(f32(list(rec["decayTimes"].values())), dt[i]).all()
            assert same_bits(f32(list(rec["echoCriterion"].values())), ec[i]).all()
            for j in range(2):
                assert same_bits(f32(list(rec["bandMetrics"][j].values())[2:]), bm[i, j]).all()
                assert same_bits(f32(rec["modulation"]["bands"][j]["m"] + [rec["modulation"]["bands"][j]["mti"]]), mo[i, j]).all()
            assert same_bits(f32([rec["spectrum"]["re"], rec["spectrum"]["im"], rec["spectrum"]["levelDb"]]).T, sp[i]).all()
        assert onsets[2] == ref.FLT_MAX and np.isfinite(rm[:2, 4:]).all()
