"""CPU: the emitter records' entry points (PvAmdSetEmitterRecords ...) exist in the header, the library and the Python layer, every
one of them is closed by the exception guard, and the argument checks that need no device answer with their own prefix.  (The
HIP-less build of tests/host/ holds the live module against a fake Solver: these calls are not part of it.)"""
import ctypes as C
import os
import re

from conftest import ROOT

NAMES = ["PvAmdSetEmitterRecords", "PvAmdGetEmitterRecordKinds", "PvAmdEmitterRecordFloats", "PvAmdGetEmitterRecords",
         "PvAmdGetEmitterCells", "PvAmdCopyEmitterTrace"]


def test_exports_exist(pvlib):
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    L = C.CDLL(pvlib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"^PVA_EXPORT int %s\(PvAmdSolver\* s[,)]" % n, hdr, re.M), n
        assert hasattr(L, n), n
        assert n in pvlib.SYMBOLS, n
    for m in ("set_emitter_records", "emitter_record_kinds", "emitter_records", "emitter_cells", "emitter_trace"):
        assert callable(getattr(pvlib.Solver, m)), m


def test_exports_are_guarded():
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    for n in NAMES:
        m = re.search(r"^int %s\([^)]*\) try \{(.*?)^\} PV_API_CATCH\(-1\)$" % n, src, re.M | re.S)
        assert m, n
        assert "\n}" not in m.group(1), n  # (the guard that closes it is its own)


def test_null_handle_is_refused_with_the_calls_prefix(pvlib):
    lib = pvlib.lib()
    t, f = C.c_uint(7), C.c_uint(7)
    out = (C.c_float * 4)()
    cells = (C.c_int * 2)()
    calls = [("emitter records: ", lambda: lib.PvAmdSetEmitterRecords(None, 1, 0)),
             ("emitter records: ", lambda: lib.PvAmdGetEmitterRecordKinds(None, C.byref(t), C.byref(f))),
             ("emitter records: ", lambda: lib.PvAmdEmitterRecordFloats(None, 0, 1)),
             ("emitter records: ", lambda: lib.PvAmdGetEmitterRecords(None, 0, 1, out, 1)),
             ("emitter cells: ", lambda: lib.PvAmdGetEmitterCells(None, cells, 1)),
             ("emitter trace: ", lambda: lib.PvAmdCopyEmitterTrace(None, 0, out))]
    for pre, call in calls:
        assert call() == -1
        assert pvlib.last_error() == pre + "null solver handle", pvlib.last_error()
    assert (t.value, f.value) == (7, 7)
