"""CPU (-m "not gpu"): the live module's emission records (PlaneverbSetEmissionRecords ... PlaneverbGetEmissionRecord) on the host
side -- tests/host_records/: a HIP-less build of pv_core.cpp + pv_context.cpp + pv_capi.cpp against a fake Solver that has the
record calls, hammered by a stand-alone program under ThreadSanitizer and under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("pipeline", ["1", "2"])
@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_emission_records_host_side_under_sanitizers(san, pipeline, tmp_path):
    """tests/host_records/records_hammer.cpp: with the worker held in front of a run, the 1 / 0 / -1 contract of
    PlaneverbGetEmissionRecord (right after a move, an end and a re-emit included; the 0 and 1 outcomes allocate nothing), the
    cap and the ascending-id rule with 1100 emitters; then, free running, readers against threads that emit, move and end emitters
    and flip the kinds and settings: every record is of one iteration, of the emitter's cell and of the kind asked for, and
    GetOutput and a record read under an unchanged PlaneverbIterationCount carry the same iteration.  Both worker loops; the
    sanitizers stay silent.  The program runs directly: nothing is preloaded."""
    out = str(tmp_path / "build")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "host_records"), "OUT=" + out, out + "/records_hammer_" + san],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               PLANEVERB_AMD_LIVE_PIPELINE=pipeline)
    r = subprocess.run([out + "/records_hammer_" + san, "1.0"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    m = re.search(r"records_hammer \(pipeline %s\): (\d+) records, (\d+) NaN reads, (\d+) refusals, (\d+) paired with GetOutput, "
                  r"0 bad" % pipeline, r.stdout)
    assert m and all(int(v) > 10 for v in m.groups()), r.stdout


def test_module_down_values(pvlib):
    """without Init: the readers answer as for a module that is down, the setters refuse with "emission records: ..." """
    pvlib.Exit()
    assert pvlib.EmissionRecordKinds() == 0
    assert pvlib.EmissionRecordCells() == -1
    for kind in (pvlib.QREC_ROOM_METRICS, pvlib.QREC_LOBES, 3, 0, 64):
        assert pvlib.EmissionRecordFloats(kind) == -1
    out = np.full(64, 7.0, np.float32)
    assert pvlib.lib().PlaneverbGetEmissionRecord(0, pvlib.QREC_ROOM_METRICS, pvlib._f(out), 64) == -1
    assert (out == 7.0).all()
    ok, rec = pvlib.GetEmissionRecord(0, pvlib.QREC_LOBES)
    assert ok == -1 and rec.size == 0
    for call in (lambda: pvlib.SetEmissionRecords(pvlib.QREC_LOBES), lambda: pvlib.SetEmissionEchogram(0.005, 16),
                 lambda: pvlib.SetEmissionLobeWindows([0.01, 0.08]), lambda: pvlib.SetEmissionLobeWindows(None)):
        with pytest.raises(pvlib.PlaneverbError, match="^emission records: .*not initialised"):
            call()


def test_header_and_python_agree(pvlib):
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    m = re.search(r"^#define\s+PVA_RECORD_QUERIES_MAX\s+(\d+)", hdr, re.M)
    assert m and int(m.group(1)) == pvlib.RECORD_QUERIES_MAX == 1024
    for name in ("PvAmdSetRecordQueries", "PlaneverbSetEmissionRecords", "PlaneverbSetEmissionEchogram",
                 "PlaneverbSetEmissionLobeWindows", "PlaneverbEmissionRecordKinds", "PlaneverbEmissionRecordFloats",
                 "PlaneverbEmissionRecordCells", "PlaneverbGetEmissionRecord"):
        assert name in pvlib.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr), name


def test_plain_host_build_has_no_record_calls(tmp_path):
    """the HIP-less build WITHOUT PVA_HOST_TEST_RECORDS (tests/host/: a fake Solver with none of the record calls) still compiles,
    its setters refuse with "not in this build" and its readers answer as for a module without records"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include <cstring>\n#include "planeverb_amd.h"\n'
                   'int main() {\n'
                   '    char dir[] = ".";\n'
                   '    PlaneverbInit(25.f, 25.f, 275, 0, dir, 0, 1);\n'
                   '    const int e = PlaneverbEmit(5.f, 0.f, 6.f);\n'
                   '    int bad = 0;\n'
                   '    if (PlaneverbSetEmissionRecords(1u) != -1 || !std::strstr(PvAmdLastError(), "emission records: not in this build")) bad |= 1;\n'
                   '    if (PlaneverbSetEmissionEchogram(0.005f, 4) != -1 || PlaneverbSetEmissionLobeWindows(nullptr, 0) != -1) bad |= 2;\n'
                   '    PlaneverbWaitIterations(3, 20000);\n'
                   '    float out[16];\n'
                   '    if (PlaneverbEmissionRecordKinds() != 0u || PlaneverbEmissionRecordCells() != 0 || PlaneverbEmissionRecordFloats(1u) != -1 ||\n'
                   '        PlaneverbGetEmissionRecord(e, 1u, out, 16) != -1) bad |= 4;\n'
                   '    PlaneverbExit();\n'
                   '    std::printf("probe: %d\\n", bad);\n'
                   '    return bad;\n'
                   '}\n')
    exe = str(tmp_path / "probe")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DPVA_HOST_TEST", "-I", host, "-I", csrc, "-I",
                           os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-Werror",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, str(src),
                           os.path.join(csrc, "pv_core.cpp"), os.path.join(csrc, "pv_context.cpp"), os.path.join(csrc, "pv_capi.cpp"),
                           "-lpthread"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and "probe: 0" in r.stdout, (r.stdout + r.stderr)[-3000:]
