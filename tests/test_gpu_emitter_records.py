"""GPU (-m gpu): the analysis records of the registered emitters in sparse-emitter mode (PvAmdSetEmitterRecords): computed inside
the run from per-emitter record traces, by the kernels of the in-run query records with a trace lane (pv_record_lane.h).

The reference is always a SECOND solver that keeps its history -- the same scene, listener and settings, compute_<kind>() and the
whole map at the emitter's cell -- never the sparse-emitter solver itself.  Tolerance 0: conftest.same_bits, NaN == NaN, so a NaN
on one side only is a difference."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, same_bits
from test_gpu_layer import cell_of
from test_gpu_non_square import ABSORBING, MIXED, TILE, both, gid, listeners, solver as rect_solver
from test_gpu_parity import fuse_opts
from test_gpu_room_metrics import SMALLROOM

pytestmark = pytest.mark.gpu

NO_ONSET = 1e30
L_ROOM = (5.0, 0.0, 4.0)
ECHOGRAM = (0.005, 16)
LOBES = [0.005, 0.02, 0.08]
BANDS = [63.0, 125.0]
BINS = [61.7, 137.5, 250.0]


def configure(s, echogram=ECHOGRAM):
    s.set_echogram(*echogram)
    s.set_lobe_windows(LOBES)
    s.set_bands(BANDS, 1)
    s.set_spectrum_bins(BINS)
    return s


def whole_maps(pvlib):
    """(spectral, kind bit) -> compute + whole map [gx, gy, floats] of a solver that keeps its history"""
    t = {pvlib.QREC_ROOM_METRICS: lambda s: (s.compute_room_metrics(), s.room_metrics())[1],
         pvlib.QREC_DECAY_TIMES: lambda s: (s.compute_decay_times(), s.decay_times())[1],
         pvlib.QREC_LATERAL: lambda s: (s.compute_lateral_fraction(), s.lateral_fraction())[1],
         pvlib.QREC_ECHOGRAM: lambda s: (s.compute_echogram(), s.echogram())[1],
         pvlib.QREC_ECHO_CRITERION: lambda s: (s.compute_echo_criterion(), s.echo_criterion())[1],
         pvlib.QREC_LOBES: lambda s: (s.compute_lobes(), s.lobes())[1]}
    f = {pvlib.QSPEC_BAND_METRICS: lambda s: (s.compute_band_metrics(), s.band_metrics())[1],
         pvlib.QSPEC_MODULATION: lambda s: (s.compute_modulation(), s.modulation())[1],
         pvlib.QSPEC_SPECTRUM: lambda s: (s.compute_spectrum(), s.spectrum())[1]}
    out = dict(((False, k), v) for k, v in t.items())
    out.update(((True, k), (lambda s, v=v: v(s).reshape(s.gx, s.gy, -1))) for k, v in f.items())
    return out


def selected(pvlib, tk, sk):
    return [(sp, k) for (sp, k) in whole_maps(pvlib) if (sk if sp else tk) & k]


_REF = {}


def reference(pvlib, key, make, L, tk, sk, irs=()):
    """the run of the full-history solver make() returns with its settings, once per key: {"delay", "res", "beta", (spectral, kind): map, "ir": {cell: [T, 3]}}"""
    if key not in _REF:
        with make() as s:
            s.run(L)
            res, delay = s.results()
            w = {"delay": delay, "res": res, "beta": s.material()[0], "T": s.T}
            for sp, k in selected(pvlib, tk, sk):
                w[(sp, k)] = whole_maps(pvlib)[(sp, k)](s)
            w["ir"] = dict((tuple(c), s.impulse_response(*c)) for c in irs)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = w
    return _REF[key]


def check(pvlib, st, ref, tk, sk, ctx, cells=None):
    """record i of every selected kind against the reference's whole map at emitter_cells()[i]; returns the cells"""
    cells = st.emitter_cells() if cells is None else cells
    assert st.emitter_record_kinds() == (tk, sk), ctx
    for sp, k in selected(pvlib, tk, sk):
        got = st.emitter_records(k, spectral=sp)
        m = ref[(sp, k)]
        assert got.shape == (len(cells), m.shape[-1]) and got.dtype == np.float32, (ctx, sp, k, got.shape)
        want = np.stack([m[cx, cy] for cx, cy in cells]) if len(cells) else got
        bad = ~same_bits(got, want)
        print("%s %s kind %d: %d of %d values differ" % (ctx, "spectral" if sp else "time", k, bad.sum(), bad.size))
        assert not bad.any(), "%s %s kind %d: %d values differ from the full-history solver's, first at %s (emitters %s)" % (
            ctx, "spectral" if sp else "time", k, bad.sum(), np.argwhere(bad)[0], sorted({tuple(cells[i]) for i in np.argwhere(bad)[:, 0]}))
        for i, (cx, cy) in enumerate(cells):  # NaN rows exactly where the cell has no onset
            assert np.isnan(got[i]).all() == (ref["delay"][cx, cy] >= NO_ONSET), (ctx, sp, k, i)
    return cells


def smallroom(pvlib, **opts):
    s = pvlib.Solver(25.0, 25.0, 275, **opts)
    s.load_scene(SMALLROOM)
    return s


def room_ref(pvlib, irs=()):
    return reference(pvlib, "smallroom", lambda: configure(smallroom(pvlib)), L_ROOM, pvlib.QREC_ALL, pvlib.QSPEC_ALL, irs or ROOM_IRS)


ROOM_IRS = [(20, 16), (14, 11), (15, 20)]  # (test 7 reads more of them through its own key)


def first(mask, what, prefer=None):
    """the first cell of the mask (of mask & prefer where there is one)"""
    if prefer is not None and (mask & prefer).any():
        mask = mask & prefer
    idx = np.argwhere(mask)
    assert len(idx), what
    return tuple(int(v) for v in idx[len(idx) // 2])


def edge_case_cells(ref, rxi, wi):
    """test 1's emitters by class, from the reference's onset map, its walls and the sparse-emitter solver's tile"""
    on = ref["delay"] < NO_ONSET
    gx, gy = on.shape
    wall = ref["beta"][:gx, :gy] == 0
    X, Y = np.meshgrid(np.arange(gx), np.arange(gy), indexing="ij")
    row0, col0 = (X % rxi == 0) & (X > 0), (Y % wi == 0) & (Y > 0)
    wallX, wallY = np.zeros_like(wall), np.zeros_like(wall)
    wallX[1:] = wall[:-1]
    wallY[:, 1:] = wall[:, :-1]
    cells = {"tile row": first(row0 & ~col0, "a tile's first row", on),
             "tile column": first(col0 & ~row0, "a tile's first column", on),
             "tile corner": first(row0 & col0, "a tile corner", on),
             "interior": first(~row0 & ~col0 & (X % rxi > 1) & (Y % wi > 1) & on, "an interior cell"),
             "wall face x": first(on & wallX, "a reached cell below a wall"),
             "wall face y": first(on & wallY, "a reached cell right of a wall"),
             "grid row 0": first((X == 0) & (Y > 0), "grid row 0", on),
             "grid column 0": first((Y == 0) & (X > 0), "grid column 0", on),
             "wall": first(wall, "a wall cell")}
    if (~on & ~wall).any():
        cells["unreached"] = first(~on & ~wall, "an air cell without an onset")
    return cells


# 1. parity of all nine kinds at the cells where the trace lane differs from the tiled lane
@pytest.mark.parametrize("fuse", [1, 0])
def test_parity_all_kinds(pvlib, fuse):
    ref = room_ref(pvlib)
    with configure(smallroom(pvlib, streaming_analysis=1, **fuse_opts(fuse))) as st:
        assert st.info.streamFuse == fuse
        assert (st.gx, st.T) == (70, 435)
        classes = edge_case_cells(ref, st.info.tileRows, st.info.tileCols)
        print("fuse %d, tile %d x %d: %s" % (fuse, st.info.tileRows, st.info.tileCols, dict(
            (n, (c, bool(ref["delay"][c] < NO_ONSET))) for n, c in classes.items())))
        assert ref["delay"][classes["tile row"]] < NO_ONSET and ref["delay"][classes["tile column"]] < NO_ONSET
        cells = list(classes.values()) + [classes["interior"]]  # (the same cell twice)
        pos = [cell_of(*c) for c in cells]
        pos.insert(3, (-3.0, 0.0, 4.0))  # off the map: dropped
        pos.append((5.0, 0.0, 26.5))     # off the map: dropped
        st.set_emitters(pos)
        st.set_emitter_records(pvlib.QREC_ALL, pvlib.QSPEC_ALL)
        assert [tuple(c) for c in st.emitter_cells()] == cells
        st.run(L_ROOM)
        got = check(pvlib, st, ref, pvlib.QREC_ALL, pvlib.QSPEC_ALL, "fuse %d" % fuse)
        assert len(got) == len(cells)
        # the same cell twice: the same records
        for sp, k in selected(pvlib, pvlib.QREC_ALL, pvlib.QSPEC_ALL):
            r = st.emitter_records(k, spectral=sp)
            assert same_bits(r[cells.index(classes["interior"])], r[-1]).all()


# 2. more than one wave group: 130 emitters, three groups of lanes, the trace planes padded to 192 columns
def test_three_wave_groups(pvlib):
    ref = room_ref(pvlib)
    tk, sk = pvlib.QREC_ROOM_METRICS | pvlib.QREC_LATERAL, pvlib.QSPEC_BAND_METRICS
    cells = [(2 + 5 * i, 1 + 7 * j) for i in range(13) for j in range(10)]
    assert len(cells) == 130
    with configure(smallroom(pvlib, streaming_analysis=1)) as st:
        st.set_emitter_records(tk, sk)
        st.set_emitters([cell_of(*c) for c in cells])
        assert [tuple(c) for c in st.emitter_cells()] == cells
        st.run(L_ROOM)
        check(pvlib, st, ref, tk, sk, "130 emitters")
        assert sum(ref["delay"][c] < NO_ONSET for c in cells) >= 8


# 3. non-square grids in both orientations: 36 x 40 tiles at K = 12, several tiles each way
@pytest.mark.parametrize("fuse", [1, 0])
@pytest.mark.parametrize("R4", [ABSORBING, MIXED], ids=["absorbing", "mixed"])
@pytest.mark.parametrize("g", both(TILE), ids=gid)
def test_non_square(pvlib, g, R4, fuse):
    gx, gy = g
    L = listeners(g)[0]
    tk = pvlib.QREC_LATERAL | pvlib.QREC_ECHOGRAM | pvlib.QREC_LOBES | pvlib.QREC_DECAY_TIMES
    ref = reference(pvlib, ("rect", g, R4), lambda: configure(rect_solver(pvlib, g, R4)), L, tk, 0)
    on = ref["delay"] < NO_ONSET
    with configure(rect_solver(pvlib, g, R4, streaming_analysis=1, **fuse_opts(fuse))) as st:
        assert st.info.streamFuse == fuse
        rxi, wi = st.info.tileRows, st.info.tileCols
        assert (gx + 1) > 2 * rxi and (gy + 1) > 2 * wi  # several tiles each way
        cells = []
        for x, y in ((0, None), (gx - 1, None), (None, 0), (None, gy - 1)):  # one beside each grid edge
            line = on[x, :] if y is None else on[:, y]
            k = int(np.flatnonzero(line)[line.sum() // 2])
            cells.append((x, k) if y is None else (k, y))
        classes = edge_case_cells(ref, rxi, wi)
        for n in ("tile row", "tile column", "tile corner", "interior", "wall face x", "wall face y"):
            assert on[classes[n]], (n, classes[n])
            cells.append(classes[n])
        st.set_emitters([cell_of(*c) for c in cells])
        st.set_emitter_records(tk, 0)
        st.run(L)
        check(pvlib, st, ref, tk, 0, "%dx%d %s fuse %d" % (gx, gy, R4, fuse))


# 4. a longer run: an open grid of 254^2 at 1000 Hz, T about 1580 -- more than a dozen wraps of the ring
def test_longer_run(pvlib):
    L = (10.0, 0.0, 14.0)
    ref = reference(pvlib, "open1000", lambda: configure(pvlib.Solver(25.0, 25.0, 1000)), L, pvlib.QREC_ALL, pvlib.QSPEC_ALL)
    with configure(pvlib.Solver(25.0, 25.0, 1000, streaming_analysis=1)) as st:
        assert st.gx == 254 and 1500 < st.T < 1700 and st.T == ref["T"]
        rxi, wi = st.info.tileRows, st.info.tileCols
        cells = [(0, 100), (100, 0), (2 * rxi, 2 * wi), (2 * rxi + 5, wi + 7)]
        st.set_emitters([((cx + 0.5) * st.dx, 0.0, (cy + 0.5) * st.dx) for cx, cy in cells])
        assert [tuple(c) for c in st.emitter_cells()] == cells
        st.set_emitter_records(pvlib.QREC_ALL, pvlib.QSPEC_ALL)
        st.run(L)
        assert all(ref["delay"][c] < NO_ONSET for c in cells)
        check(pvlib, st, ref, pvlib.QREC_ALL, pvlib.QSPEC_ALL, "254^2")


# 5. state between runs: another listener, a larger emitter table, a changed setting, an asynchronous run
def test_state_between_runs(pvlib):
    tk, sk = pvlib.QREC_ALL, pvlib.QSPEC_BAND_METRICS
    ref = room_ref(pvlib)
    # another listener: an air cell a few cells from the first one (the ninth-earliest onset of the first run)
    L2 = cell_of(*(int(v) for v in np.unravel_index(np.argsort(ref["delay"], axis=None)[8], ref["delay"].shape)))
    ref2 = reference(pvlib, "smallroom L2", lambda: configure(smallroom(pvlib)), L2, tk, sk)
    ref8 = reference(pvlib, "smallroom 8 slots", lambda: configure(smallroom(pvlib), (0.01, 8)), L_ROOM, pvlib.QREC_ECHOGRAM, 0)
    on = (ref["delay"] < NO_ONSET) & (ref2["delay"] < NO_ONSET)
    reached = [tuple(int(v) for v in c) for c in np.argwhere(on)]
    assert len(reached) > 700
    few, more = reached[::len(reached) // 3][:3], reached[::len(reached) // 70][:70]
    with configure(smallroom(pvlib, streaming_analysis=1)) as st:
        st.set_emitters([cell_of(*c) for c in few])
        st.set_emitter_records(tk, sk)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no completed run"):
            st.emitter_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: echogram: the slots cannot be cleared"):
            st.set_echogram(0.0, 0)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: the bands cannot be cleared"):
            st.set_bands([])
        st.run(L_ROOM)
        check(pvlib, st, ref, tk, sk, "first run")
        st.run(L2)  # another listener: every trace is rewritten, nothing of the first run is left
        check(pvlib, st, ref2, tk, sk, "second listener")
        st.set_emitters([cell_of(*c) for c in more])  # more emitters than the tables held: reallocation, and a second wave group
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no completed run"):
            st.emitter_records(pvlib.QREC_ROOM_METRICS)
        st.run(L_ROOM)
        assert [tuple(c) for c in check(pvlib, st, ref, tk, sk, "70 emitters")] == more
        st.set_echogram(0.01, 8)  # the stamp refuses the old slots' records, and only those
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no completed run"):
            st.emitter_records(pvlib.QREC_ECHOGRAM)
        st.run_async(L_ROOM)
        st.sync()
        got = st.emitter_records(pvlib.QREC_ECHOGRAM)
        want = np.stack([ref8[(False, pvlib.QREC_ECHOGRAM)][c] for c in more])
        assert got.shape == want.shape == (70, 25) and same_bits(got, want).all()
        assert same_bits(st.emitter_records(pvlib.QREC_LOBES), np.stack([ref[(False, pvlib.QREC_LOBES)][c] for c in more])).all()
        st.set_emitter_records(0, 0)
        assert st.emitter_record_kinds() == (0, 0)
        st.run(L_ROOM)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: the kind is not selected"):
            st.emitter_records(pvlib.QREC_ROOM_METRICS)


# 6. nothing else moves: the result map, the onset map and get_output with and without the kinds
def test_results_unchanged(pvlib):
    cells = [(20, 16), (14, 11), (24, 30)]
    pos = [cell_of(*c) for c in cells]
    out = []
    for kinds in ((0, 0), (pvlib.QREC_ALL, pvlib.QSPEC_ALL)):
        with configure(smallroom(pvlib, streaming_analysis=1)) as st:
            st.set_emitters(pos)
            st.set_emitter_records(*kinds)
            st.run(L_ROOM)
            out.append(st.results() + tuple(st.get_output(p).as_array() for p in pos))
    for a, b in zip(*out):
        assert same_bits(a, b).all()
    assert np.isfinite(out[0][2]).all() and out[0][2][1] != 0  # (a wet gain at an emitter: the old traces still serve)


# 7. the trace: the emitter's pressure of every step is the full-history solver's impulse response at the cell
def test_trace(pvlib):
    ref = room_ref(pvlib)
    with smallroom(pvlib, streaming_analysis=1) as st:  # (no kind selected)
        st.set_emitters([cell_of(*c) for c in ROOM_IRS])
        with pytest.raises(pvlib.PlaneverbError, match="^emitter trace: no simulation"):
            st.emitter_trace(0)
        st.run(L_ROOM)
        for i, c in enumerate(ROOM_IRS):
            tr = st.emitter_trace(i)
            assert tr.shape == (st.T,) and np.abs(tr).max() > 0
            assert same_bits(tr, ref["ir"][c][:, 0]).all(), c
        with pytest.raises(pvlib.PlaneverbError, match="^emitter trace: no such"):
            st.emitter_trace(3)
    with smallroom(pvlib) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^emitter trace: .*sparse-emitter"):
            s.emitter_trace(0)


# 8. refusals: an "emitter records: ..." message each, and the solver works afterwards
def test_refusals(pvlib):
    ref = room_ref(pvlib)
    E = [cell_of(20, 16)]
    with smallroom(pvlib) as s:  # a solver that keeps its history
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: .*not in sparse-emitter mode.*PvAmdSetQueryRecords"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: .*not in sparse-emitter mode"):
            s.emitter_records(pvlib.QREC_ROOM_METRICS)
        assert s.emitter_record_kinds() == (0, 0)
        s.set_output_queries(E)
        s.set_query_records(pvlib.QREC_ROOM_METRICS)
        s.run(L_ROOM)
        assert same_bits(s.queried_records(pvlib.QREC_ROOM_METRICS)[0], ref[(False, pvlib.QREC_ROOM_METRICS)][20, 16]).all()
    with pvlib.Solver(25.0, 25.0, 275, slabs=[0, 0]) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: .*slab"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS)
    with smallroom(pvlib, streaming_analysis=1, skip_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: .*onset map"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS)
    with smallroom(pvlib, streaming_analysis=1) as s:
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: unknown kind bit \\(PVA_QREC"):
            s.set_emitter_records(64)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: unknown kind bit \\(PVA_QSPEC"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS, 8)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: echogram: no slots set"):
            s.set_emitter_records(pvlib.QREC_ECHOGRAM)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no bands set"):
            s.set_emitter_records(0, pvlib.QSPEC_MODULATION)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no bins set"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS, pvlib.QSPEC_SPECTRUM)
        assert s.emitter_record_kinds() == (0, 0)  # (a refusal of either family leaves both as they were)
        with pytest.raises(pvlib.PlaneverbError, match="^query records: .*history"):
            s.set_query_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="^spectral records: .*history"):
            s.set_query_spectral_records(pvlib.QSPEC_SPECTRUM)
        many = np.tile(np.array(E, np.float32), (1025, 1))
        s.set_emitters(many)  # (allowed while no kind is selected)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: at most 1024 registered emitters"):
            s.set_emitter_records(pvlib.QREC_ROOM_METRICS)
        s.set_emitters(E)
        s.set_emitter_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: at most 1024 registered emitters"):
            s.set_emitters(many)
        assert len(s.emitter_cells()) == 1
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: exactly one kind"):
            s.emitter_records(3)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: the kind is not selected \\(PvAmdSetEmitterRecords\\)"):
            s.emitter_records(pvlib.QREC_LATERAL)
        with pytest.raises(pvlib.PlaneverbError, match="^emitter records: no completed run"):
            s.emitter_records(pvlib.QREC_ROOM_METRICS)
        out = np.zeros(40, np.float32)
        fp = out.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float))
        assert pvlib.lib().PvAmdGetEmitterRecords(s._h, 0, pvlib.QREC_ROOM_METRICS, fp, 2) == -1
        assert pvlib.last_error() == "emitter records: count differs from the registered emitters"
        assert pvlib.lib().PvAmdGetEmitterRecords(s._h, 2, pvlib.QREC_ROOM_METRICS, fp, 1) == -1
        assert pvlib.last_error().startswith("emitter records: family")
        assert pvlib.lib().PvAmdGetEmitterRecords(s._h, 0, pvlib.QREC_ROOM_METRICS, fp, 1025) == -1
        assert pvlib.last_error().startswith("emitter records: PvAmdGetEmitterRecords: 0 .. 1024 emitters")
        # the old readers serve nothing in this mode
        assert pvlib.lib().PvAmdGetQueriedRecords(s._h, pvlib.QREC_ROOM_METRICS, fp, 1) == -1
        assert pvlib.last_error().startswith("query records: the kind is not selected")
        assert s.query_record_kinds() == 0
        # ... and the solver works afterwards
        s.run(L_ROOM)
        assert same_bits(s.emitter_records(pvlib.QREC_ROOM_METRICS)[0], ref[(False, pvlib.QREC_ROOM_METRICS)][20, 16]).all()


# 9. the command line: --sparse-emitters prints what --in-run-records prints
def test_cli(pvlib):
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4", "--emitter", "5,0,6", "--emitter", "40,0,3",
           "--emitter", "12,0,9", "--room-metrics", "--decay-times", "--lateral-fraction", "--echogram", "0.005,16",
           "--echo-criterion", "--lobes", "0.005,0.02,0.08", "--bands", "63,125", "--modulation", "--spectrum", "61.7,137.5,250"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(*more):
        out = subprocess.run(cmd + list(more), capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout
        assert len(re.findall(r'"(?:fdtd_ms|analysis_ms)": [0-9.e+-]+,', out)) == 2
        return re.sub(r'("(?:fdtd_ms|analysis_ms)"): [0-9.e+-]+,', r"\1: 0,", out)

    a, b = run("--in-run-records"), run("--sparse-emitters")
    assert a == b
    rec = json.loads(b)["emitters"]
    assert len(rec) == 3 and all(k in rec[0] for k in ("roomMetrics", "decayTimes", "lateralFraction", "echogram", "echoCriterion",
                                                        "lobes", "bandMetrics", "modulation", "spectrum"))
    assert np.isfinite(rec[0]["roomMetrics"]["c50"]) and np.isnan(rec[1]["roomMetrics"]["c50"])  # (the second one is off the map)
