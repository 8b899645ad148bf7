"""GPU (-m gpu): the device compile of csrc/pv_libm.h against the host compile of the same header (api.libm_probe, PvAmdLibmProbe),
bit for bit and NaN by position, in every form the analysis kernels evaluate -- the fused pairs, the staged batch with its
scheduling barriers and the tables in LDS (filled by the kernels' own fillLogTab / fillPowTab) exist on the device only, and the
host check (tools/libm_check.cpp, tests/test_host_cpu.py) cannot see them.  Three input sets:

  sample    every 97th float from +0 through the NaN range (the sample the host test uses);
  mantissa  all 2^24 floats with exponent field 0x7e or 0x7f: where decay ratios live, and the arguments logf sees -- the ones for
            which fusing its five multiply-add pairs was only checked on the host;
  edges     every 7th subnormal, 0, the smallest and largest subnormal and normal, 1 +- 1 ulp, inf and NaN.

The normal-only forms are fed only pvIsNormalPositive inputs.  For the two plain forms the host output is also held to
libm.so.6's own log10f / powf on the first set: the assumption every numpy restatement makes (tests/_room_metrics_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_analysis_maps import identical

pytestmark = pytest.mark.gpu


def floats(bits):
    return np.ascontiguousarray(bits, np.uint32).view(np.float32)


def input_sets():
    one = 0x3f800000
    edges = np.concatenate([np.arange(0, 0x00800000, 7, dtype=np.uint32),
                            np.array([0, 1, 0x007fffff, 0x00800000, 0x7f7fffff, one - 1, one, one + 1, 0x7f800000, 0x7fc00000,
                                      0x7f800001, 0x7fffffff], np.uint32)])
    return {"sample": floats(np.arange(0, 0x80000000, 97, dtype=np.uint32)),
            "mantissa": floats(np.arange(0x3f000000, 0x40000000, dtype=np.uint32)),
            "edges": floats(edges)}


@pytest.fixture(scope="module")
def sets():
    s = input_sets()
    assert len(s["mantissa"]) == 1 << 24 and len(s["sample"]) > 2.2e7 and np.isnan(s["sample"][-1]) and s["sample"][0] == 0
    for v in s.values():
        v.setflags(write=False)
    return s


def normal_positive(x):
    """pvIsNormalPositive (csrc/pv_libm.h)"""
    return (x.view(np.uint32) - np.uint32(0x00800000)) < np.uint32(0x7f000000)


@pytest.mark.parametrize("which", ["sample", "mantissa", "edges"])
@pytest.mark.parametrize("form", range(11), ids=lambda f: "form%d" % f)
def test_device_equals_host(pvlib, sets, form, which):
    name = pvlib.LIBM_FORMS[form]
    x = sets[which]
    if name in pvlib.LIBM_NORMAL_ONLY:
        x = x[normal_positive(x)]
        assert len(x) >= 5  # (of the edges: the smallest and largest normal, 1 and its two neighbours)
    dev, host = pvlib.libm_probe(form, x, True), pvlib.libm_probe(form, x, False)
    if not identical(dev, host):
        bad = np.nonzero(~((dev.view(np.uint32) == host.view(np.uint32)) | (np.isnan(dev) & np.isnan(host))))[0]
        raise AssertionError("%s on %s: %d of %d differ, first x = %r (0x%08x): device 0x%08x, host 0x%08x" % (
            name, which, len(bad), len(x), x[bad[0]], x.view(np.uint32)[bad[0]], dev.view(np.uint32)[bad[0]],
            host.view(np.uint32)[bad[0]]))
    assert np.isfinite(host).any()


def test_forms_agree_on_the_device(pvlib, sets):
    """every logarithm form gives pvLog10f's bits and every power form pvPowf's, on the device, on the edges set"""
    x = sets["edges"]
    xn = x[normal_positive(x)]
    base = pvlib.libm_probe("log10", x, True)
    for f in ("log10_nonneg", "log10_nonneg_tab"):
        assert identical(pvlib.libm_probe(f, x, True), base), f
    for f in pvlib.LIBM_NORMAL_ONLY:
        assert identical(pvlib.libm_probe(f, xn, True), pvlib.libm_probe("log10", xn, True)), f
    for y in ("08", "23"):
        base = pvlib.libm_probe("pow_" + y, x, True)
        for f in ("pow_nonneg_" + y, "pow_nonneg_tab_" + y):
            assert identical(pvlib.libm_probe(f, x, True), base), f


@pytest.fixture(scope="module")
def libm_array(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("libm") / "libm_array.so")
    subprocess.check_call(["gcc", "-O1", "-fno-builtin", "-shared", "-fPIC", os.path.join(ROOT, "tests", "host", "libm_array.c"),
                           "-o", so, "-lm"])
    lib = C.CDLL(so)
    fp = C.POINTER(C.c_float)
    lib.libm_log10f_array.argtypes = [fp, fp, C.c_longlong]
    lib.libm_powf_array.argtypes = [fp, C.c_float, fp, C.c_longlong]
    lib.libm_log10f_array.restype = lib.libm_powf_array.restype = None
    return lib


@pytest.mark.parametrize("form", ["log10", "pow_08", "pow_23"])
def test_host_equals_the_machines_libm(pvlib, sets, libm_array, form):
    x = sets["sample"]
    want = np.empty_like(x)
    px, pw = x.ctypes.data_as(C.POINTER(C.c_float)), want.ctypes.data_as(C.POINTER(C.c_float))
    if form == "log10":
        libm_array.libm_log10f_array(px, pw, len(x))
    else:
        libm_array.libm_powf_array(px, float(np.float32(0.8 if form == "pow_08" else 2.0 / 3.0)), pw, len(x))
    got = pvlib.libm_probe(form, x, False)
    assert identical(got, want), (form, np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:4])


def test_refusals(pvlib):
    x = np.ones(4, np.float32)
    for form in (-1, 11):
        with pytest.raises(pvlib.PlaneverbError, match="^libm probe: unknown form"):
            pvlib.libm_probe(form, x, False)
    assert pvlib.libm_probe("log10", np.empty(0, np.float32), True).shape == (0,)
    assert pvlib.lib().PvAmdLibmProbe(0, None, None, 4, 0) == -1 and pvlib.last_error().startswith("libm probe: null")
