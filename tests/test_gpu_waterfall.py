"""GPU (-m gpu): per-receiver waterfalls (PvAmdComputeWaterfall; pv_waterfall.hip).

The expected values come from the numpy restatement (tests/_waterfall_ref.py, written from the definition in
include/planeverb_amd.h) applied to the SAME solver's recorded planes (history_plane(t) for all t), its own onset map
(results()[1]), its pulse() and the library's tables.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _adversarial as adv
import _waterfall_ref as ref
import test_gpu_analysis_maps as maps
from conftest import ROOT, SCENES, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_emitter_records import configure, edge_case_cells
from test_gpu_layer import cell_of
from test_gpu_parity import fuse_opts
from test_gpu_spectrum import BINS, L400, N400

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
FLT_MAX = np.float32(np.finfo(np.float32).max)
OFF_MAP = (-3.0, 0.0, 4.0)
KEYS = ("onset", "slices", "response", "level")


def bins_of(n, fs):
    return np.linspace(0.0, fs / 2.0, n).astype(np.float32) if n > 1 else np.array([61.7], np.float32)


def history(s):
    return np.stack([s.history_plane(t) for t in range(s.T)])


def expected(pvlib, s, hist, delay, cells):
    """the numpy restatement's records of `cells` ((cx, cy), or None for a position off the map) under the solver's setting"""
    hz, seconds, ns, m = s.waterfall_setting()
    assert ns == ref.slice_steps(seconds, s.fs)
    c, sn = ref.tables(pvlib, s.T, s.fs, hz)
    p = np.zeros((s.T, len(cells)), np.float32)
    d = np.full(len(cells), FLT_MAX, np.float32)
    for i, cell in enumerate(cells):
        if cell is not None:
            p[:, i] = hist[:, cell[0], cell[1]]
            d[i] = delay[cell]
    return ref.parts(ref.waterfall(p, d, c, sn, ns, m, s.pulse()), len(hz), m)


def same(got, want, ctx):
    for k in KEYS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32, (ctx, k, got[k].shape, want[k].shape)
        bad = ~same_bits(got[k], want[k])
        assert not bad.any(), "%s %s: %d values differ, first at %s: %s vs %s" % (
            ctx, k, bad.sum(), np.argwhere(bad)[0], got[k][bad][:4], want[k][bad][:4])


def positions(cells):
    return [OFF_MAP if c is None else cell_of(*c) for c in cells]


def pick_receivers(s, delay, beta):
    """about 12 receivers: reached cells in several tiles (a tile's first row and column among them), one in a wall where the
    scene has one, one without an onset where there is one, one off the map, one duplicated"""
    ec = edge_case_cells({"delay": delay, "beta": beta}, s.info.tileRows, s.info.tileCols) if (beta[:s.gx, :s.gy] == 0).any() else {}
    reached = np.argwhere(delay < ref.NO_ONSET)
    cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 7).astype(int)]
    cells += [c for k, c in ec.items()]
    tiles = set((c[0] // s.info.tileRows, c[1] // s.info.tileCols) for c in cells if delay[c] < ref.NO_ONSET)
    assert len(tiles) >= 2, tiles
    cells = cells[:14] + [None, cells[0]]
    return cells


# 1. the 70^2 presets (T = 435: the resident path)
SHAPES = [(1, 1), (64, 16), (65, 16), (130, 3), (512, 64)]


@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox", "g71_empty"])
def test_preset_grid(pvlib, name):
    g = golden(name)
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        assert (s.gx, s.T, s.fs) == (70, 435, 1443)
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        hist, delay, beta = history(s), s.results()[1], s.material()[0]
        cells = pick_receivers(s, delay, beta)
        live = np.array([c is not None and delay[c] < ref.NO_ONSET for c in cells])
        assert live.sum() >= 8 and not live.all()
        # (the last setting: ns = 72 puts slices 7 .. 15 of every receiver past T)
        for n, m, seconds in [(n, m, 0.02) for n, m in SHAPES] + [(65, 16, 0.05)]:
            s.set_waterfall(bins_of(n, s.fs), seconds, m)
            assert s.compute_waterfall(positions(cells)) > 0
            got = s.waterfall()
            assert got["response"].shape == (len(cells), n, 2) and got["level"].shape == (len(cells), m, n)
            same(got, expected(pvlib, s, hist, delay, cells), "%s n=%d m=%d" % (name, n, m))
            # NaN records on exactly the receivers without an onset
            assert np.array_equal(np.isnan(got["onset"]), ~live)
            assert np.isnan(got["level"][~live]).all() and np.isnan(got["response"][~live]).all()
            assert np.isfinite(got["response"][live]).all()
            assert same_bits(got["level"][-1], got["level"][0]).all()  # (the duplicate)
            if seconds == 0.05:
                assert (got["slices"][live] <= 7).all() and np.isneginf(got["level"][live][:, 7:]).all()
            if n == 65:
                assert (np.abs(got["response"][live][:, 1:-1, 1]) > 0).any()  # (not degenerate)


# 2. a history window smaller than the grid: receivers in tiles with a tile origin other than 0, one outside the window
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < ref.NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 9).astype(int)]
        late = np.argwhere((delay < ref.NO_ONSET) & (delay >= s.T - 4))
        cells.append(tuple(int(v) for v in late[0]))  # (an onset in the run's last steps)
        far = (10, 398) if where == "offset" else (398, 398)  # inside the grid, outside the window
        assert delay[far] >= ref.NO_ONSET
        cells.append(far)
        s.set_waterfall(bins_of(65, s.fs), 0.02, 16)
        s.compute_waterfall(positions(cells))
        got = s.waterfall()
        same(got, expected(pvlib, s, hist, delay, cells), where)
        assert np.isnan(got["level"][-1]).all() and np.isfinite(got["response"][:-1]).all()


# 3. independence: a record's bits do not depend on the other receivers, their order or the receivers a wave takes
def test_independence(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        delay = s.results()[1]
        reached = np.argwhere(delay < ref.NO_ONSET)
        target = tuple(int(v) for v in reached[len(reached) // 3])
        rng = np.random.default_rng(3)
        others = [(int(x), int(y)) for x, y in zip(rng.integers(0, s.gx, 255), rng.integers(0, s.gy, 255))]
        # (130 bins, 256 receivers: two receivers to a wave; 512 bins: four; one receiver alone: one)
        for n, m in ((130, 16), (512, 4)):
            s.set_waterfall(bins_of(n, s.fs), 0.02, m)
            s.compute_waterfall([cell_of(*target)])
            alone = s.waterfall()
            assert np.isfinite(alone["response"]).all() and np.isfinite(alone["level"][0, :int(alone["slices"][0])]).all()
            s.compute_waterfall(positions([target] + others))
            first = s.waterfall()
            shuffled = [others[i] for i in rng.permutation(255)]
            s.compute_waterfall(positions(shuffled + [target]))
            last = s.waterfall()
            for k in KEYS:
                assert same_bits(first[k][0], alone[k][0]).all() and same_bits(last[k][-1], alone[k][0]).all(), (n, k)


# 4. injected histories: every family of tests/_adversarial.py against the host restatement
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_injected_histories(pvlib):
    with maps.make_solver(pvlib) as s:
        s.run(maps.LISTENER)
        new, fam, delay = adv.inject(s, 20261020)
        reached = np.zeros(fam.shape, bool)
        reached[:s.gx, :s.gy] = delay < ref.NO_ONSET
        cells = []
        for f in range(len(adv.FAMILIES)):
            idx = np.argwhere((fam == f) & reached)
            assert len(idx) >= 4, adv.FAMILIES[f]
            cells += [tuple(int(v) for v in idx[i]) for i in np.linspace(0, len(idx) - 1, 4).astype(int)]
        pulse = s.pulse()
        finite = adv.finite_cells(new)
        for c in cells:
            assert finite[c] == (fam[c] != adv.NONFINITE)
        poisoned = [c for c in cells if not finite[c]]
        clean = [c for c in cells if finite[c]]
        assert len(poisoned) == 4 and len(clean) == 40
        # every wave of four receivers holds a receiver with NaN / inf samples beside three finite ones
        mixed = [poisoned[(i // 4) % 4] if i % 4 == 1 else clean[(i - i // 4) % 40] for i in range(256)]
        # (65 bins, 44 receivers: one receiver to a wave; 512 bins, 256 receivers: four)
        for hz, seconds, m, rx in ((bins_of(65, s.fs), 0.0105, 16, cells), (bins_of(512, s.fs), 0.0105, 4, mixed)):
            s.set_waterfall(hz, seconds, m)
            s.compute_waterfall(positions(rx))
            got = s.waterfall()
            want = dict((c, pvlib.host_waterfall(np.ascontiguousarray(new[:, c[0], c[1]]), s.fs, int(delay[c]), hz, seconds, m, pulse))
                        for c in set(rx))
            for i, c in enumerate(rx):
                for k in KEYS:
                    assert same_bits(got[k][i], want[c][k][0]).all(), (len(hz), i, adv.describe(fam, c), k)


# 5. against the spectrum: the same sum in the opposite order
def test_against_the_spectrum(pvlib):
    g = golden("g71_smallroom")
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(g["listener"])
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < ref.NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 24).astype(int)]
        hz = np.array(BINS[32], np.float32)
        s.set_spectrum_bins(hz)
        s.compute_spectrum()
        spec = s.spectrum()
        spow = s.spectrum_source()[:, 2]
        s.set_waterfall(hz, 0.02, 1)
        s.compute_waterfall(positions(cells))
        got = s.waterfall()
        assert same_bits(s.spectrum(), spec).all()  # (the two do not invalidate each other)
        c, sn = pvlib.host_spectrum_tables(s.T, s.fs, hz)
        u = 2.0 ** -24
        for i, cell in enumerate(cells):
            t0 = int(delay[cell])
            N = s.T - t0
            gamma = (N + 1) * u / (1.0 - (N + 1) * u)
            p = hist[t0:, cell[0], cell[1]].astype(np.float64)[:, None]
            for comp, w in ((0, c), (1, sn)):
                bound = 2.0 * gamma * np.abs(p * w[t0:].astype(np.float64)).sum(axis=0)
                err = np.abs(got["response"][i, :, comp].astype(np.float64) - spec[cell][:, comp].astype(np.float64))
                assert (err <= bound).all(), (cell, comp, err.max(), bound.min())
            # spow has the bits of spectrum_source(): the level is that of the record's own sums over it
            R, I = got["response"][i, :, 0], got["response"][i, :, 1]
            with np.errstate(all="ignore"):
                level = np.float32(10.0) * ref.log10f(((R * R) + (I * I)) / spow)
            assert same_bits(got["level"][i, 0], level).all()


# 6. sparse-emitter mode: the emitters' traces as the sample source, against a second solver that keeps its history
def sparse_case(pvlib, make, L, kinds, zones, ctx, late=False):
    with make() as full:
        full.run(L)
        delay, beta = full.results()[1], full.material()[0]
        with make(streaming_analysis=1) as st:
            classes = edge_case_cells({"delay": delay, "beta": beta}, st.info.tileRows, st.info.tileCols)
            cells = list(classes.values())
            assert not delay[classes["wall"]] < ref.NO_ONSET
            if late:  # onsets in the run's last steps: the last accumulate pass
                idx = np.argwhere((delay < ref.NO_ONSET) & (delay >= full.T - 6))
                assert len(idx) >= 3
                cells += [tuple(int(v) for v in c) for c in idx[:6]]
            reached = np.argwhere(delay < ref.NO_ONSET)
            cells += [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 40 - len(cells)).astype(int)]
            if "unreached" not in classes:
                cells[-1] = tuple(int(v) for v in np.argwhere(~(delay < ref.NO_ONSET))[0])
            st.set_emitters([OFF_MAP] + positions(cells))  # (the position off the map is dropped)
            assert [tuple(c) for c in st.emitter_cells()] == cells
            if kinds:
                configure(st)
                st.set_emitter_records(pvlib.QREC_ALL, pvlib.QSPEC_ALL)
            if zones:
                st.set_zones(pvlib.zone_labels_from_rects(st.dx, st.gx, st.gy, [(2.0, 2.0, 9.0, 9.0)]), 1)
                st.set_zone_curves(True)
            hz = bins_of(130, st.fs)
            for sv in (full, st):
                sv.set_waterfall(hz, 0.02, 16)
            st.run(L)
            assert st.compute_waterfall() > 0
            got = st.waterfall()
            full.compute_waterfall(positions(cells))
            want = full.waterfall()
            same(got, want, ctx)
            live = ~np.isnan(want["onset"])
            assert live.sum() >= 24 and not live.all()
            if kinds:  # nothing interferes: the emitter records are there as well
                assert st.emitter_records(pvlib.QREC_ROOM_METRICS).shape[0] == len(cells)
            pulse = st.pulse()
            for i in np.flatnonzero(live)[::5]:
                h = pvlib.host_waterfall(st.emitter_trace(int(i)), st.fs, int(got["onset"][i]), hz, 0.02, 16, pulse)
                assert same_bits(h["response"][0], got["response"][i]).all() and same_bits(h["level"][0], got["level"][i]).all()


def smallroom(pvlib, **base):
    def make(**opts):
        s = pvlib.Solver(25.0, 25.0, 275, **dict(base, **opts))
        s.load_scene(SMALLROOM)
        return s
    return make


@pytest.mark.parametrize("kinds", [False, True], ids=["no-kind", "records+curves"])
def test_sparse_smallroom(pvlib, kinds):
    sparse_case(pvlib, smallroom(pvlib), (5.0, 0.0, 4.0), kinds, kinds, "smallroom kinds=%s" % kinds)


def test_sparse_cut_short(pvlib):
    sparse_case(pvlib, smallroom(pvlib, num_steps=100), (5.0, 0.0, 4.0), False, False, "num_steps=100", late=True)


def test_sparse_fused_254(pvlib):
    size = open_size(254)

    def make(**opts):
        if opts.get("streaming_analysis"):
            opts.update(fuse_opts(1))
        s = pvlib.Solver(size, size, 275, num_steps=300, **opts)
        s.load_scene(SMALLROOM)
        return s

    with make(streaming_analysis=1) as st:
        assert st.info.streamFuse == 1 and st.gx == 254
    sparse_case(pvlib, make, cell_of(120, 100), False, False, "254^2 fused")


# 7. lifetimes and refusals
def test_lifetime(pvlib):
    g = golden("g71_smallroom")
    E = [tuple(e) for e in g["emitters"]][:3]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s, \
            pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as plain:
        for sv in (s, plain):
            for b in g["boxes"]:
                sv.add_geometry(b)
        hz = bins_of(64, s.fs)
        s.set_waterfall(hz, 0.02, 8)
        st = s.waterfall_setting()
        assert same_bits(st[0], hz).all() and st[1:] == (np.float32(0.02), 28, 8)
        assert pvlib.lib().PvAmdWaterfallFloats(s._h) == 2 + 2 * 64 + 8 * 64
        s.run(g["listener"])
        plain.run(g["listener"])
        # the setting changes nothing a run leaves
        for a, b in zip(s.results(), plain.results()):
            assert same_bits(a, b).all()
        s.compute_waterfall(E)
        first = s.waterfall()
        assert np.isfinite(first["level"]).all()
        # the map kinds and the waterfall do not touch each other
        s.compute_room_metrics()
        metrics = s.room_metrics()
        s.compute_waterfall(E)
        assert same_bits(s.room_metrics(), metrics).all()
        same(s.waterfall(), first, "again")
        # a copy with another count
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: .*count"):
            s.waterfall(count=2)
        # another nPos reallocates
        s.compute_waterfall(E + E)
        both = s.waterfall()
        assert both["level"].shape[0] == 6
        for k in KEYS:
            assert same_bits(both[k][:3], first[k]).all() and same_bits(both[k][3:], first[k]).all()
        # refused calls change nothing
        for bad in (dict(positions=[]), dict(positions=[E[0]] * 257)):
            with pytest.raises(pvlib.PlaneverbError, match="waterfall: 1 .. 256 positions"):
                s.compute_waterfall(**bad)
        assert pvlib.lib().PvAmdComputeWaterfall(s._h, None, 2, None) == -1 and "waterfall: no positions" in pvlib.last_error()
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: 1 .. 256 positions"):
            s.compute_waterfall(None)
        for bad in (dict(hz=[float("nan")]), dict(hz=[-1.0]), dict(hz=[s.fs / 2.0 + 1.0]), dict(hz=[1.0] * 513), dict(hz=[1.0], n_slices=65),
                    dict(hz=[1.0], n_slices=0), dict(hz=[1.0], slice_seconds=0.0), dict(hz=[1.0], slice_seconds=float("inf"))):
            with pytest.raises(pvlib.PlaneverbError, match="waterfall:"):
                s.set_waterfall(bad["hz"], bad.get("slice_seconds", 0.02), bad.get("n_slices", 8))
        same(s.waterfall(), both, "after refusals")
        # a changed setting
        s.set_waterfall(hz, 0.02, 4)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall()
        s.compute_waterfall(E)
        four = s.waterfall()
        assert same_bits(four["level"], first["level"][:, :4]).all() and same_bits(four["response"], first["response"]).all()
        # geometry, boundary, layer
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall()
        s.compute_waterfall(E)  # (the last completed run is still the first one)
        same(s.waterfall(), four, "after a geometry change")
        s.set_grid_boundary((1, 0, 0, 0))
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall()
        s.compute_waterfall(E)
        s.set_edge_layer((8, 8, 8, 8))
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall()
        s.set_edge_layer((0, 0, 0, 0))
        s.set_grid_boundary((0, 0, 0, 0))
        s.remove_geometry(gid)
        # a run between compute and copy
        s.compute_waterfall(E)
        s.run((7.0, 0.0, 9.5))
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall()
        s.compute_waterfall(E)
        second = s.waterfall()
        assert not same_bits(second["level"], four["level"]).all()
        # cleared: nothing is left, and a run enqueues what a solver that never called the setter enqueues
        s.set_waterfall([])
        assert s.waterfall_setting() is None and pvlib.lib().PvAmdWaterfallFloats(s._h) == -1
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no setting"):
            s.compute_waterfall(E)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no setting"):
            s.waterfall(count=3)


def test_runs_are_unchanged(pvlib):
    """a run under a setting, a pass between two runs and a run after the setting was cleared leave the result and onset maps and
    the history of a solver that never called the setter"""
    g = golden("g71_smallroom")
    E = [tuple(e) for e in g["emitters"]][:3]
    with pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s, \
            pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as plain:
        for sv in (s, plain):
            for b in g["boxes"]:
                sv.add_geometry(b)

        def both(L):
            for sv in (s, plain):
                sv.run(L)
            for a, b in zip(s.results(), plain.results()):
                assert same_bits(a, b).all(), L
            assert same_bits(s.history_plane(200), plain.history_plane(200)).all()

        s.set_waterfall(bins_of(64, s.fs), 0.02, 8)
        both(tuple(g["listener"]))
        s.compute_waterfall(E)
        both((7.0, 0.0, 9.5))
        s.compute_waterfall(E)
        s.set_waterfall([])
        both((6.0, 0.0, 5.0))


def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    hz = bins_of(64, 1443)
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_waterfall(hz, 0.02, 8)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no emitters registered"):
            s.compute_waterfall()
        s.set_emitters([E])
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no completed run"):
            s.compute_waterfall()
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: a sparse-emitter solver takes no positions"):
            s.compute_waterfall([E])
        s.compute_waterfall()
        one = s.waterfall()
        assert np.isfinite(one["level"]).all()
        s.set_emitters([E, (12.0, 0.0, 9.0)])  # a change of the emitters: the records and the traces are the old table's
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall(count=1)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no completed run"):
            s.compute_waterfall()
        s.run(L)
        s.compute_waterfall()
        two = s.waterfall()
        for k in KEYS:
            assert same_bits(two[k][0], one[k][0]).all()
        s.set_emitters([cell_of(i % 60 + 2, i // 60 + 2) for i in range(257)])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: at most 256 registered emitters"):
            s.compute_waterfall()
        assert s.get_output(E).occlusion > 0
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_waterfall(hz, 0.02, 8)
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: .*onset map"):
            s.compute_waterfall([E])
        assert np.abs(s.history_plane(200)).max() > 0
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_waterfall(hz, 0.02, 8), lambda: s.compute_waterfall([E]), lambda: s.waterfall(count=1),
                     s.waterfall_setting):
            with pytest.raises(pvlib.PlaneverbError, match="waterfall: .*slab"):
                call()
        s.run(L)
        assert s.get_output(E).occlusion > 0
    # a slab rank: one slab of the grid (the refusal of the handle itself, ahead of any solver call)
    s512 = open_size(512)
    rank = pvlib.SlabRank(s512, s512, 275, 0, 0, 2, pvlib.compute_efree(s512, s512, 275))
    try:
        for call in (lambda: rank.solver.set_waterfall(hz, 0.02, 8), lambda: rank.solver.compute_waterfall([E]),
                     lambda: rank.solver.waterfall(count=1), rank.solver.waterfall_setting):
            with pytest.raises(pvlib.PlaneverbError, match="^waterfall: slab rank"):
                call()
        assert pvlib.lib().PvAmdWaterfallFloats(rank.solver._h) == -1 and pvlib.last_error().startswith("waterfall: slab rank")
    finally:
        rank.close()
    # (the refusal of a last run that ended in error has no test: nothing makes a run fail short of a device fault)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no setting"):
            s.compute_waterfall([E])
        s.set_waterfall(hz, 0.02, 8)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no completed run"):
            s.compute_waterfall([E])
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: not computed"):
            s.waterfall(count=1)
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="waterfall: no completed run"):
            s.compute_waterfall([E])
        s.run(L)
        assert s.compute_waterfall([E]) > 0
        assert np.isfinite(s.waterfall()["level"]).all()


# 8. the command line
@pytest.mark.parametrize("sparse", [False, True], ids=["history", "sparse-emitters"])
def test_cli(pvlib, sparse):
    L, E = "5,0,4", ["5,0,6", "12,0,9", "-3,0,4"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", L] + ["--emitter=" + e for e in E]
    cmd += ["--waterfall", "20,275,64", "--waterfall-slices", "0.02,8"] + (["--sparse-emitters"] if sparse else [])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout)
    pos = [(5.0, 0.0, 6.0), (12.0, 0.0, 9.0), (-3.0, 0.0, 4.0)]
    hz = np.linspace(20, 275, 64).astype(np.float32)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.set_waterfall(hz, 0.02, 8)
        s.compute_waterfall(pos)
        want = s.waterfall()
        for i, rec in enumerate(out["emitters"]):
            w = rec["waterfall"]
            assert list(w) == ["hz", "sliceSeconds", "sliceSteps", "onset", "re", "im", "levelDb"]
            assert same_bits(np.array(w["hz"], np.float32), hz).all() and w["sliceSteps"] == 28
            assert same_bits(np.float32(w["sliceSeconds"]), np.float32(0.02))
            got = {"onset": np.float32(w["onset"]), "response": np.array([w["re"], w["im"]], np.float32).T,
                   "level": np.array(w["levelDb"], np.float32)}
            for k in got:
                assert same_bits(got[k], want[k][i]).all(), (i, k)
        assert np.isnan(want["onset"][2]) and np.isfinite(want["level"][:2]).all()
