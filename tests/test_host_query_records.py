"""No GPU: the in-run query records' constants, record sizes and C declarations (include/planeverb_amd.h PvAmdSetQueryRecords)."""
import os
import re
import subprocess

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "planeverb_amd.h")
NAMES = {"ROOM_METRICS": 10, "DECAY_TIMES": 8, "LATERAL": 11, "ECHOGRAM": None, "ECHO_CRITERION": 10, "LOBES": None}


def test_constants_equal_the_header(pvlib):
    hdr = open(HEADER).read()
    defs = dict((n, int(v)) for n, v in re.findall(r"^#define PVA_QREC_(\w+)\s+(\d+)u\b", hdr, re.M))
    assert sorted(defs) == sorted(NAMES)
    assert sorted(defs.values()) == [1, 2, 4, 8, 16, 32]
    for n, v in defs.items():
        assert getattr(pvlib, "QREC_" + n) == v, n
    assert pvlib.QREC_ALL == sum(defs.values())


def test_record_floats_follow_the_record_layouts(pvlib):
    """10, 8, 11, 1 + 3 n, 10, 1 + 5 w: the sizes of the whole-map records the in-run ones are copies of"""
    hdr = open(HEADER).read()
    for n, want in NAMES.items():
        m = re.search(r"#define PVA_QREC_%s\s+\d+u\s*/\*(.*?)\*/" % n, hdr)
        assert m, n
        if want is not None:
            assert "%d floats" % want in m.group(1), n
    assert len(pvlib.ROOM_METRIC_NAMES) == 10 and len(pvlib.DECAY_TIME_NAMES) == 8 and len(pvlib.LATERAL_FRACTION_NAMES) == 11
    assert len(pvlib.ECHO_CRITERION_NAMES) == 10 and len(pvlib.LOBE_NAMES) == 5
    for slots in (1, 16, pvlib.ECHOGRAM_MAX_SLOTS):  # the host restatements give records of the sizes the header names
        assert pvlib.host_echogram([1.0] * 8, [0.0] * 8, [0.0] * 8, 1443, 0, 0.005, slots).shape == (1 + 3 * slots,)
    for edges in ((0.01,), (0.01, 0.08), tuple(0.01 * (i + 1) for i in range(pvlib.LOBES_MAX_EDGES))):
        assert pvlib.host_lobes([1.0] * 8, [0.0] * 8, [0.0] * 8, 1443, 0, edges).shape == (1 + 5 * (len(edges) + 1),)


def test_header_with_the_new_calls_is_plain_c(tmp_path):
    src = tmp_path / "qrec.c"
    src.write_text('#include "planeverb_amd.h"\n'
                   'int f(PvAmdSolver* s, float* out) {\n'
                   '    unsigned all = PVA_QREC_ROOM_METRICS | PVA_QREC_DECAY_TIMES | PVA_QREC_LATERAL | PVA_QREC_ECHOGRAM |\n'
                   '                   PVA_QREC_ECHO_CRITERION | PVA_QREC_LOBES;\n'
                   '    if (PvAmdSetQueryRecords(s, all) != 0 || PvAmdGetQueryRecordKinds(s) != all) return -1;\n'
                   '    return PvAmdGetQueriedRecords(s, PVA_QREC_LOBES, out, PvAmdQueryRecordFloats(s, PVA_QREC_LOBES));\n'
                   '}\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])
