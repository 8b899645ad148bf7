"""CPU: PvAmdHostRoomMetrics -- the room-metric definition of include/planeverb_amd.h (PvAmdRoomMetrics) applied to one impulse
response -- against the numpy restatement of tests/_room_metrics_ref.py, bit for bit (tolerance 0).  No device compute."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden, same_bits
import _room_metrics_ref as ref


def check(pvlib, p, fs, onset):
    got = pvlib.host_room_metrics(p, fs, onset)
    want = ref.room_metrics_ir(p, fs, onset)
    assert got.dtype == np.float32 and got.shape == (10,)
    assert same_bits(got, want).all(), (fs, onset, len(p), got, want)
    return got


@pytest.mark.parametrize("name", ["g71_smallroom", "g96_smallroom_res375"])
def test_reference_impulse_responses(pvlib, name):
    """the reference's own impulse responses, each with its onset from the restated threshold scan"""
    g = golden(name)
    fs = int(pvlib.host_grid_info(float(g["size"]), float(g["size"]), int(g["res"])).fs)
    n = 0
    for ir in g["probe_ir"]:
        p = np.ascontiguousarray(ir[:, 0])
        onset = ref.threshold_onset(p)
        if onset < 0:
            continue
        m = check(pvlib, p, fs, onset)
        assert m[4] > 0  # e50: the onset sample exceeds the threshold
        n += 1
    assert n >= 4, n


def test_random_impulse_responses(pvlib):
    rng = np.random.default_rng(20261017)
    for _ in range(200):
        T = int(rng.integers(1, 601))
        fs = int(rng.choice([1443, 1968, 700, 4000, 12]))
        p = (rng.standard_normal(T) * 10.0 ** rng.uniform(-6, 1)).astype(np.float32)
        check(pvlib, p, fs, int(rng.integers(0, T)))


@pytest.mark.parametrize("fs", [1443, 1968])
def test_window_edges(pvlib, fs):
    """onset = T - 1, onset + n = T, T - 1, T + 1 for both windows, and an all-zero tail"""
    rng = np.random.default_rng(fs)
    T = 400
    p = (rng.standard_normal(T) * 1e-2).astype(np.float32)
    a50, a80 = ref.n50(fs), ref.n80(fs)
    m = check(pvlib, p, fs, T - 1)
    assert np.isposinf(m[0]) and np.isposinf(m[1]) and m[2] == 1 and m[3] == 0
    for n in (a50, a80):
        for d in (-1, 0, 1):
            m = check(pvlib, p, fs, T - n + d)  # onset + n = T + d
            late = m[5] if n == a50 else m[7]
            assert (late == 0) == (d >= 0)
    m = check(pvlib, p, fs, T - a50)
    assert np.isposinf(m[0]) and m[2] == 1
    z = p.copy()
    z[100 + a50 - 3:] = 0  # nothing after the early window: l50 = l80 = 0 by the data
    m = check(pvlib, z, fs, 100)
    assert np.isposinf(m[0]) and np.isposinf(m[1]) and m[5] == 0 and m[7] == 0


def test_window_lengths():
    assert (ref.n50(1443), ref.n80(1443)) == (72, 115)
    assert (ref.n50(1968), ref.n80(1968)) == (98, 157)


def test_window_lengths_in_the_library(pvlib):
    """the library's n50 / n80, seen through the sums: a unit impulse k samples after the onset lands in the early sum iff k < n"""
    for fs, a50, a80 in ((1443, 72, 115), (1968, 98, 157)):
        for k, early50, early80 in ((a50 - 1, True, True), (a50, False, True), (a80 - 1, False, True), (a80, False, False)):
            p = np.zeros(300, np.float32)
            p[10] = 1.0
            p[10 + k] = 2.0
            m = pvlib.host_room_metrics(p, fs, 10)
            assert m[4] == (5.0 if early50 else 1.0) and m[6] == (5.0 if early80 else 1.0), (fs, k, m)
            assert m[8] == 5.0 and m[9] == 4.0 * k


def test_bad_arguments(pvlib):
    L = pvlib.lib()
    p = np.ones(8, np.float32)
    out = pvlib.PvAmdRoomMetrics()
    fp = p.ctypes.data_as(C.POINTER(C.c_float))
    assert L.PvAmdHostRoomMetrics(None, 8, 1443, 0, out) == -1
    assert pvlib.last_error()
    assert L.PvAmdHostRoomMetrics(fp, 8, 1443, 0, None) == -1
    assert L.PvAmdHostRoomMetrics(fp, 0, 1443, 0, out) == -1
    assert L.PvAmdHostRoomMetrics(fp, -3, 1443, 0, out) == -1
    assert L.PvAmdHostRoomMetrics(fp, 8, 1443, -1, out) == -1
    assert L.PvAmdHostRoomMetrics(fp, 8, 1443, 8, out) == -1
    assert L.PvAmdHostRoomMetrics(fp, 8, 1443, 7, out) == 0
    # the solver calls refuse a null handle
    assert L.PvAmdComputeRoomMetrics(None, None) == -1 and pvlib.last_error()
    assert L.PvAmdCopyRoomMetrics(None, fp) == -1
    assert L.PvAmdCopyRoomMetricsBlock(None, 0, 0, 1, 1, fp) == -1
    assert L.PvAmdGetRoomMetrics(None, 0.0, 0.0, 0.0, out) == -1


NEW_EXPORTS = ["PvAmdComputeRoomMetrics", "PvAmdCopyRoomMetrics", "PvAmdCopyRoomMetricsBlock", "PvAmdGetRoomMetrics",
               "PvAmdHostRoomMetrics"]


def test_exports_present_and_guarded(pvlib):
    """the new exports are in the product library, in the header, in the python binding, and each is a function-try-block closed
    by the exception-guard macro of pv_capi.cpp"""
    L = C.CDLL(pvlib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    for n in NEW_EXPORTS:
        assert hasattr(L, n), n
        assert n in pvlib.SYMBOLS
        assert re.search(r"^PVA_EXPORT\s+int\s+%s\s*\(" % n, hdr, re.M), n
        m = re.search(r"^int\s+%s\s*\([^;{}]*?\)\s*try\s*\{.*?^\}\s*PV_API_CATCH\(-1\)" % n, src, re.M | re.S)
        assert m, n
        assert "\n}\n" not in m.group(0), n  # (the match ends at this function's own guard)
    assert pvlib.ROOM_METRIC_NAMES == ref.NAMES
    assert C.sizeof(pvlib.PvAmdRoomMetrics) == 40
    assert b"0.4" in pvlib.lib().PvAmdVersion()
