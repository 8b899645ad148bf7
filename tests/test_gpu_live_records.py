"""GPU (-m gpu): emission records -- the in-run analysis records of the live emitters' cells, by emission id
(PlaneverbSetEmissionRecords ... PlaneverbGetEmissionRecord; pv_context.cpp on top of PvAmdSetRecordQueries).

The module runs the Sandbox's configuration (25 m, 275 Hz: 70 x 70, T = 435) with SmallRoomScene.pv and the golden listener and
emitters, in both worker loops (PLANEVERB_AMD_LIVE_PIPELINE 1 and 2).  The reference is a batch Solver with the same scene,
listener and settings: the whole-map record of the emitter's cell after compute_<kind>() (NaNs off the map).  Tolerance 0
(conftest.same_bits).  The only NaN records are those of positions a test itself placed off the map or in cells without an onset;
their count is asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENES, golden, same_bits
from test_gpu_layer import cell_of
from test_gpu_parity import compare_output
from test_gpu_query_records import ECHOGRAM, NO_ONSET, bits, kinds_of
from test_host_lobes import EDGES5

pytestmark = pytest.mark.gpu

SIZE = (25.0, 25.0)
SCENE = os.path.join(SCENES, "SmallRoomScene.pv")
L2 = (6.5, 0.0, 5.5)                 # the listener after its move
BOX = (9.0, 6.0, 1.0, 3.0, 0.6)      # ... and the box added with it
OFF_MAP = (40.0, 0.0, 5.0)


@pytest.fixture(params=["1", "2"])
def live(request, pvlib, monkeypatch):
    monkeypatch.setenv("PLANEVERB_AMD_LIVE_PIPELINE", request.param)
    pvlib.Init(pvlib.Config(SIZE, 275, 0, ".", 0, pvlib.pv_GPU))
    yield pvlib
    pvlib.Exit()


def settle(pv, n=3):
    target = pv.IterationCount() + n
    assert pv.WaitIterations(target, 60000) >= target


_REF = {}


def reference(pvlib, echogram=ECHOGRAM, edges=EDGES5, moved=False):
    """(whole-map records {kind: [gx, gy, floats]}, onset map) of the batch solver after the module's sequence of runs"""
    key = (tuple(echogram), tuple(edges), moved)
    if key not in _REF:
        g = golden("g71_smallroom")
        with pvlib.Solver(SIZE[0], SIZE[1], 275) as s:
            s.load_scene(SCENE)
            s.set_echogram(*echogram)
            s.set_lobe_windows(edges)
            s.run(g["listener"])
            if moved:
                s.add_geometry(BOX)
                s.run(L2)
            delay = s.results()[1]
            _REF[key] = (dict((k, kinds_of(pvlib)[k][0](s)) for k in bits(pvlib, pvlib.QREC_ALL)), delay)
    return _REF[key]


def cell(pvlib, pos):
    return pvlib.host_cells(SIZE[0], SIZE[1], 275, pos[0], pos[2])[1]


def start(pv, kinds, echogram=ECHOGRAM, edges=EDGES5, emitters=None):
    g = golden("g71_smallroom")
    pv.SetListenerPosition(g["listener"])
    assert pv.LoadScene(SCENE) == 5
    ids = [pv.Emit(e) for e in (g["emitters"] if emitters is None else emitters)]
    pv.SetEmissionEchogram(*echogram)
    pv.SetEmissionLobeWindows(edges)
    pv.SetEmissionRecords(kinds)
    settle(pv)
    return ids


def check(pv, eid, pos, ref, kinds, ctx):
    """every selected kind of one emitter against the reference; returns 1 (records) or 0 (NaNs: off the map or no onset)"""
    maps, delay = ref
    c = cell(pv, pos)
    want_ok = int(c is not None and delay[c] < NO_ONSET)
    for k in bits(pv, kinds):
        ok, rec = pv.GetEmissionRecord(eid, k)
        assert ok == want_ok and rec.shape == (maps[k].shape[-1],), (ctx, k, ok, want_ok, rec.shape)
        if want_ok:
            assert same_bits(rec, maps[k][c]).all(), (ctx, k, c, rec, maps[k][c])
            assert not np.isnan(rec).all(), (ctx, k)
        else:
            assert np.isnan(rec).all(), (ctx, k, rec)
    return want_ok


def test_all_six_kinds(live):
    pv = live
    g = golden("g71_smallroom")
    ref = reference(pv)
    twin = tuple(float(v) + 0.01 for v in g["emitters"][0])  # (another position in emitter 0's cell)
    assert cell(pv, twin) == cell(pv, g["emitters"][0])
    ids = start(pv, pv.QREC_ALL, emitters=list(g["emitters"]) + [twin])
    assert ids == [0, 1, 2, 3]
    assert pv.EmissionRecordKinds() == pv.QREC_ALL
    assert [pv.EmissionRecordFloats(k) for k in bits(pv, pv.QREC_ALL)] == [10, 8, 11, 49, 10, 31]
    assert pv.EmissionRecordCells() == len(set(cell(pv, e) for e in g["emitters"])) == 3
    assert sum(check(pv, i, e, ref, pv.QREC_ALL, "emitter %d" % i) for i, e in zip(ids, list(g["emitters"]) + [twin])) == 4
    for k in bits(pv, pv.QREC_ALL):
        assert same_bits(pv.GetEmissionRecord(ids[0], k)[1], pv.GetEmissionRecord(ids[3], k)[1]).all(), k
    for i, ro in zip(ids, g["emitter_out"]):
        compare_output(pv.GetOutput(i), ro, "emitter %d" % i)


def test_returns_zero_with_nans(live):
    pv = live
    g = golden("g71_smallroom")
    ref = reference(pv)
    no_onset = [tuple(int(v) for v in c) for c in np.argwhere(ref[1] >= NO_ONSET)]
    assert no_onset
    quiet = cell_of(*no_onset[len(no_onset) // 2])
    ids = start(pv, pv.QREC_ALL, emitters=[g["emitters"][0], g["emitters"][1], OFF_MAP, quiet])
    pv.EndEmission(ids[1])
    assert check(pv, ids[0], g["emitters"][0], ref, pv.QREC_ALL, "reached") == 1
    nans = 0
    for eid, why in ((17, "never issued"), (ids[1], "ended"), (ids[2], "off the map"), (ids[3], "no onset")):
        for k, n in zip(bits(pv, pv.QREC_ALL), (10, 8, 11, 49, 10, 31)):
            ok, rec = pv.GetEmissionRecord(eid, k)
            assert ok == 0 and rec.shape == (n,) and np.isnan(rec).all(), (why, k, ok, rec)
            nans += 1
    assert nans == 24
    assert check(pv, ids[2], OFF_MAP, ref, pv.QREC_ALL, "off the map") == 0
    assert check(pv, ids[3], quiet, ref, pv.QREC_ALL, "no onset") == 0


def test_returns_minus_one_for_a_kind_not_selected(live):
    pv = live
    g = golden("g71_smallroom")
    kinds = pv.QREC_ROOM_METRICS | pv.QREC_LOBES
    ids = start(pv, kinds)
    assert pv.EmissionRecordKinds() == kinds and pv.EmissionRecordFloats(pv.QREC_DECAY_TIMES) == -1
    assert check(pv, ids[0], g["emitters"][0], reference(pv), kinds, "selected kinds") == 1
    out = np.full(64, 7.0, np.float32)
    for kind in (pv.QREC_DECAY_TIMES, pv.QREC_ECHOGRAM, 3, 0, 64):
        assert pv.lib().PlaneverbGetEmissionRecord(ids[0], kind, pv._f(out), 64) == -1 and (out == 7.0).all(), kind
    assert pv.lib().PlaneverbGetEmissionRecord(ids[0], pv.QREC_LOBES, pv._f(out), 30) == -1 and (out == 7.0).all()
    assert pv.lib().PlaneverbGetEmissionRecord(ids[0], pv.QREC_LOBES, None, 64) == -1
    assert pv.lib().PlaneverbGetEmissionRecord(ids[0], pv.QREC_LOBES, pv._f(out), 31) == 1 and (out[31:] == 7.0).all()
    # refusals at the call
    for call, what in ((lambda: pv.SetEmissionRecords(64), "unknown"), (lambda: pv.SetEmissionEchogram(0.005, 33), "nSlots"),
                       (lambda: pv.SetEmissionLobeWindows([0.08, 0.01]), "lobes")):
        with pytest.raises(pv.PlaneverbError, match="^emission records: .*" + what):
            call()


def test_moved_emitter(live):
    pv = live
    g = golden("g71_smallroom")
    ref = reference(pv)
    ids = start(pv, pv.QREC_ALL)
    reached = ref[1] < NO_ONSET
    taken = set(cell(pv, e) for e in g["emitters"])
    rng = np.random.default_rng(7)
    cand = [tuple(int(v) for v in c) for c in np.argwhere(reached)]
    new = next(c for c in (cand[i] for i in rng.permutation(len(cand))) if c not in taken)
    pv.UpdateEmission(ids[1], cell_of(*new))
    settle(pv)
    assert check(pv, ids[1], cell_of(*new), ref, pv.QREC_ALL, "moved") == 1
    assert check(pv, ids[0], g["emitters"][0], ref, pv.QREC_ALL, "stayed") == 1
    assert pv.EmissionRecordCells() == 3


def test_settings_change(live):
    pv = live
    g = golden("g71_smallroom")
    ids = start(pv, pv.QREC_ALL)
    assert pv.EmissionRecordFloats(pv.QREC_ECHOGRAM) == 49
    pv.SetEmissionEchogram(0.01, 8)
    settle(pv)
    assert pv.EmissionRecordFloats(pv.QREC_ECHOGRAM) == 25 and pv.EmissionRecordFloats(pv.QREC_LOBES) == 31
    ref = reference(pv, echogram=(0.01, 8))
    assert sum(check(pv, i, e, ref, pv.QREC_ALL, "slots (0.01, 8)") for i, e in zip(ids, g["emitters"])) == 3
    with pytest.raises(pv.PlaneverbError, match="^emission records: .*cannot be cleared"):
        pv.SetEmissionEchogram(0.0, 0)
    pv.SetEmissionLobeWindows(None)  # the default windows
    settle(pv)
    assert pv.EmissionRecordFloats(pv.QREC_LOBES) == 16
    ref = reference(pv, echogram=(0.01, 8), edges=(0.01, 0.08))
    assert sum(check(pv, i, e, ref, pv.QREC_ALL, "default windows") for i, e in zip(ids, g["emitters"])) == 3


def test_switching_off(live):
    pv = live
    g = golden("g71_smallroom")
    ids = start(pv, pv.QREC_ALL)
    assert check(pv, ids[0], g["emitters"][0], reference(pv), pv.QREC_ALL, "on") == 1
    pv.SetEmissionRecords(0)
    settle(pv)
    assert pv.EmissionRecordKinds() == 0 and pv.EmissionRecordCells() == 0
    for k in bits(pv, pv.QREC_ALL):
        assert pv.EmissionRecordFloats(k) == -1
        ok, rec = pv.GetEmissionRecord(ids[0], k, capacity=64)
        assert ok == -1 and (rec == 0).all(), k
    for i, ro in zip(ids, g["emitter_out"]):
        compare_output(pv.GetOutput(i), ro, "emitter %d, records off" % i)
    pv.SetEmissionEchogram(0.0, 0)  # (allowed again)


def test_cap(live):
    pv = live
    ref = reference(pv)
    rng = np.random.default_rng(1100)
    cells = [(int(c) // 70, int(c) % 70) for c in rng.permutation(70 * 70)[:1100]]
    pos = [cell_of(*c) for c in cells]
    ids = start(pv, pv.QREC_ALL, emitters=pos)
    assert ids == list(range(1100))
    assert pv.EmissionRecordCells() == pv.RECORD_QUERIES_MAX == 1024
    spot = sorted(set([0, 1, 63, 64, 65, 511, 512, 1000, 1022, 1023] + [int(i) for i in rng.choice(1024, 8, replace=False)]))
    assert len(spot) >= 16
    served = sum(check(pv, ids[i], pos[i], ref, pv.QREC_ALL, "emitter %d" % i) for i in spot)
    assert served == sum(1 for i in spot if ref[1][cells[i]] < NO_ONSET) >= 8
    for i in range(1024, 1100):  # beyond the cap: not in the table
        for k in (pv.QREC_ROOM_METRICS, pv.QREC_LOBES):
            ok, rec = pv.GetEmissionRecord(ids[i], k)
            assert ok == 0 and np.isnan(rec).all(), (i, k)
    assert sum(1 for i in range(1024, 1100) if ref[1][cells[i]] < NO_ONSET) > 30  # (most of them would have had a record)


def test_listener_and_geometry_change(live):
    pv = live
    g = golden("g71_smallroom")
    ids = start(pv, pv.QREC_ALL)
    assert check(pv, ids[0], g["emitters"][0], reference(pv), pv.QREC_ALL, "before") == 1
    pv.SetListenerPosition(L2)
    pv.AddGeometry(BOX)
    settle(pv)
    ref = reference(pv, moved=True)
    assert not all(same_bits(ref[0][k], reference(pv)[0][k]).all() for k in ref[0])
    n = sum(check(pv, i, e, ref, pv.QREC_ALL, "after") for i, e in zip(ids, g["emitters"]))
    assert n == sum(1 for e in g["emitters"] if ref[1][cell(pv, e)] < NO_ONSET) >= 2


def test_sparse_emitter_mode_refuses(live, pvlib, monkeypatch):
    pvlib.Exit()
    monkeypatch.setenv("PLANEVERB_AMD_LIVE_STREAMING", "1")
    pvlib.Init(pvlib.Config(SIZE, 275, 0, ".", 0, pvlib.pv_GPU))
    assert pvlib.lib().PlaneverbIsStreaming() == 1
    for call in (lambda: pvlib.SetEmissionRecords(pvlib.QREC_LOBES), lambda: pvlib.SetEmissionEchogram(0.005, 16),
                 lambda: pvlib.SetEmissionLobeWindows([0.01, 0.08])):
        with pytest.raises(pvlib.PlaneverbError, match="^emission records: the full pressure history is not kept"):
            call()
    e = pvlib.Emit((5.0, 0.0, 6.0))
    settle(pvlib, 2)
    assert pvlib.EmissionRecordKinds() == 0 and pvlib.GetEmissionRecord(e, pvlib.QREC_LOBES, capacity=64)[0] == -1


def test_cli(live):
    pv = live
    g = golden("g71_smallroom")
    emitters = [tuple(float(v) for v in e) for e in g["emitters"]] + [OFF_MAP]
    ids = start(pv, pv.QREC_ALL, emitters=emitters)
    cmd = [sys.executable, "-m", "planeverb_amd", SCENE, "--listener", ",".join(repr(float(v)) for v in g["listener"]),
           "--echogram", "0.005,16", "--lobes", ",".join(repr(float(v)) for v in EDGES5), "--emission-records"]
    for e in emitters:
        cmd += ["--emitter", ",".join(repr(v) for v in e)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout)["emitters"]
    assert len(out) == 4
    F = lambda v: np.asarray(v, np.float32)
    nans = 0
    for i, e in zip(ids, out):
        flat = {
            pv.QREC_ROOM_METRICS: F(list(e["roomMetrics"].values())),
            pv.QREC_DECAY_TIMES: F(list(e["decayTimes"].values())),
            pv.QREC_LATERAL: F(list(e["lateralFraction"].values())),
            pv.QREC_ECHOGRAM: F([e["echogram"]["n"]] + [v for t in zip(e["echogram"]["e"], e["echogram"]["ix"], e["echogram"]["iy"])
                                                        for v in t]),
            pv.QREC_ECHO_CRITERION: F(list(e["echoCriterion"].values())),
            pv.QREC_LOBES: F([e["lobes"]["n"]] + [v for w in e["lobes"]["windows"] for v in w.values()]),
        }
        assert e["echogram"]["slotSteps"] == 7
        for k, got in flat.items():
            ok, rec = pv.GetEmissionRecord(i, k)
            assert ok == (1 if i != ids[3] else 0) and got.shape == rec.shape and same_bits(got, rec).all(), (i, k, got, rec)
            nans += int(np.isnan(got).all())
    assert nans == 6
