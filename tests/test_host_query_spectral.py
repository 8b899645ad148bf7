"""No GPU: the in-run spectral query records' constants, record sizes, C declarations and exports (include/planeverb_amd.h
PvAmdSetQuerySpectralRecords)."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "planeverb_amd.h")
CALLS = ("PvAmdSetQuerySpectralRecords", "PvAmdGetQuerySpectralKinds", "PvAmdQuerySpectralFloats", "PvAmdGetQueriedSpectralRecords")
PER = {"BAND_METRICS": 12, "MODULATION": 15, "SPECTRUM": 3}


def test_constants_equal_the_header(pvlib):
    hdr = open(HEADER).read()
    defs = dict((n, int(v)) for n, v in re.findall(r"^#define PVA_QSPEC_(\w+)\s+(\d+)u\b", hdr, re.M))
    assert defs == {"BAND_METRICS": 1, "MODULATION": 2, "SPECTRUM": 4}
    for n, v in defs.items():
        assert getattr(pvlib, "QSPEC_" + n) == v, n
    assert pvlib.QSPEC_ALL == 7 == sum(defs.values())


def test_the_six_kinds_keep_their_namespace(pvlib):
    """the spectral kinds have a selector of their own: no PVA_QREC_* define was added"""
    hdr = open(HEADER).read()
    qrec = re.findall(r"^#define PVA_QREC_(\w+)\s+(\d+)u\b", hdr, re.M)
    assert len(qrec) == 6 and sorted(int(v) for _, v in qrec) == [1, 2, 4, 8, 16, 32]
    assert pvlib.QREC_ALL == 63


def test_header_with_the_new_calls_is_plain_c(tmp_path):
    src = tmp_path / "qspec.c"
    src.write_text('#include "planeverb_amd.h"\n'
                   'int f(PvAmdSolver* s, float* out, int n) {\n'
                   '    unsigned all = PVA_QSPEC_BAND_METRICS | PVA_QSPEC_MODULATION | PVA_QSPEC_SPECTRUM;\n'
                   '    if (PvAmdSetQuerySpectralRecords(s, all) != 0 || PvAmdGetQuerySpectralKinds(s) != all) return -1;\n'
                   '    if (PvAmdQuerySpectralFloats(s, PVA_QSPEC_SPECTRUM) < 0) return -1;\n'
                   '    return PvAmdGetQueriedSpectralRecords(s, PVA_QSPEC_MODULATION, out, n);\n'
                   '}\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_the_library_exports_the_calls(pvlib):
    import planeverb_amd
    so = ctypes.CDLL(planeverb_amd.LIB_PATH)
    for name in CALLS:
        assert getattr(so, name, None) is not None, name
        assert name in pvlib.SYMBOLS, name
    hdr = open(HEADER).read()
    for name in CALLS:
        assert re.search(r"^PVA_EXPORT (?:int|unsigned) %s\(" % name, hdr, re.M), name


def test_record_floats_follow_the_record_layouts(pvlib):
    """12 n, 15 n, 3 bins: the sizes of the whole-map records the in-run ones are copies of"""
    hdr = open(HEADER).read()
    for n, per in PER.items():
        m = re.search(r"#define PVA_QSPEC_%s\s+\d+u\s*/\*(.*?)\*/" % n, hdr)
        assert m and "%d floats per" % per in m.group(1), n
    assert len(pvlib.BAND_METRIC_NAMES) == 12 and pvlib.MODULATION_FREQS + 1 == 15
    p = np.zeros(64, np.float32)
    p[3] = 1.0
    for n in (1, 3, pvlib.BANDS_MAX):
        coefs = pvlib.host_band_coefs(1443, [63.0 + 20.0 * j for j in range(n)])
        assert pvlib.host_band_metrics(p, 1443, 3, coefs).shape == (n, 12)
        assert pvlib.host_modulation(p, 1443, 3, coefs).shape == (n, 15)
    for bins in (1, 9, pvlib.SPECTRUM_MAX_BINS):
        assert pvlib.host_spectrum(p, 1443, 3, [10.0 * j for j in range(bins)], p).shape == (bins, 3)
    # the pinned block's largest record: 8 bands of 12 and of 15 floats, 32 bins of 3
    assert 12 * pvlib.BANDS_MAX + 15 * pvlib.BANDS_MAX + 3 * pvlib.SPECTRUM_MAX_BINS == 312
