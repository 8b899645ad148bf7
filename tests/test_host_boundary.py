"""CPU (-m "not gpu"): the grid-edge model's test oracle (tests/_boundary_ref.py) and the new C-ABI symbols.

With R = 0 on every side, the ring grid of the pinned oracle is the plain grid of the reference's own absorbing edges
(FDTD.cpp:201-223), bit for bit modulo the sign of zero: fields, history, onsets and all eight members.  That pins the ring
construction the GPU tests compare against.  R = 1 and mixed sides give other results."""
import os
import re

import numpy as np
import pytest

from _boundary_ref import RingOracle, half_cell_box
from conftest import ROOT, same_bits

NAMES8 = ("occlusion", "wetGain", "rt60", "lowpass", "dirX", "dirY", "srcDirX", "srcDirY")


def scene(dx, n):
    """an interior wall (half-cell edges) in an n x n grid"""
    return [half_cell_box(dx, n // 3, n // 3 + 2, 3, n - 12, 0.3), half_cell_box(dx, 5, 12, 2 * n // 3, 2 * n // 3 + 1, 0.9)]


def cell(dx, cx, cy):
    return (float((cx + 0.5) * dx), 0.0, float((cy + 0.5) * dx))


CASES = [(25.0, 275, (10, 50)), (10.0, 375, (30, 8))]


def plain_and_ring(oracle, size, res, lc, R4):
    dx = oracle.grid_params(res)[0]
    probe = oracle.OracleGrid(size, size, res, with_history=False)
    n = probe.gx
    probe.close()
    boxes = np.array(scene(np.float32(dx), n), np.float32)
    L = cell(np.float32(dx), *lc)
    o = oracle.OracleGrid(size, size, res, boxes)
    f = o.fdtd(L, want_fields=True)
    ef = oracle.free_energy(size, size, res)
    r, d, _ = o.analyze(ef, L)
    plain = (f, tuple(h.copy() for h in o.history()), r, d)
    o.close()
    ring = RingOracle(oracle, size, res, boxes, R4)
    rf = ring.fdtd(L)
    rh = tuple(h.copy() for h in ring.history())
    rr, rd = ring.analyze()
    ring.close()
    return plain, (rf, rh, rr, rd)


@pytest.mark.parametrize("size,res,lc", CASES, ids=["70sq", "38sq"])
def test_ring_oracle_absorbing_equals_plain_grid(oracle, size, res, lc):
    (f, h, r, d), (rf, rh, rr, rd) = plain_and_ring(oracle, size, res, lc, (0, 0, 0, 0))
    assert f.shape == rf.shape
    for k, nm in enumerate(("pr", "vx", "vy")):
        assert same_bits(rf[k], f[k]).all(), "final %s" % nm
        assert same_bits(rh[k], h[k]).all(), "history %s: %d samples differ" % (nm, int((~same_bits(rh[k], h[k])).sum()))
    assert same_bits(rd, d).all(), "delay"
    assert (d < 1e30).sum() > 100
    for k, nm in enumerate(NAMES8):
        assert same_bits(rr[..., k], r[..., k]).all(), nm


@pytest.mark.parametrize("R4", [(1, 1, 1, 1), (0, 1, 0.5, 0.25)], ids=["rigid", "mixed"])
def test_ring_oracle_other_edges_differ(oracle, R4):
    size, res, lc = CASES[0]
    (f, h, r, d), (rf, rh, rr, rd) = plain_and_ring(oracle, size, res, lc, R4)
    assert not same_bits(rf[0], f[0]).all()
    assert not same_bits(rr[..., 1], r[..., 1]).all(), "wet gain"
    reached = rd < 1e30
    assert reached.sum() >= (d < 1e30).sum()
    if R4 == (1, 1, 1, 1):  # a closed room keeps its energy: longer decay
        both = reached & (d < 1e30) & np.isfinite(rr[..., 2]) & np.isfinite(r[..., 2])
        assert np.median(rr[..., 2][both]) > np.median(r[..., 2][both])


def test_boundary_symbols_declared_and_exported(pvlib):
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    for name in ("PvAmdSetGridBoundary", "PvAmdGetGridBoundary", "PlaneverbSetGridBoundary"):
        assert re.search(r"PVA_EXPORT\s+\w+\s+%s\s*\(" % name, hdr), name
        assert name in pvlib.SYMBOLS
        assert getattr(pvlib.lib(), name) is not None
    assert pvlib.pv_AbsorbingBoundary == 0 and pvlib.pv_ReflectingBoundary == 1


def test_boundary_refusals_without_a_device(pvlib):
    """argument checks come before any device work: a null handle or a non-finite side is refused"""
    L = pvlib.lib()
    import ctypes as C
    ok = (C.c_float * 4)(0, 0, 0, 0)
    assert L.PvAmdSetGridBoundary(None, ok) == -1
    assert L.PvAmdGetGridBoundary(None, ok) == -1
    for bad in (float("nan"), float("inf"), float("-inf")):
        v = (C.c_float * 4)(0, bad, 0, 0)
        assert L.PvAmdSetGridBoundary(None, v) == -1
        assert "finite" in pvlib.last_error()
    L.PlaneverbSetGridBoundary(1, 1, 1, 1)  # no live module: nothing to do, no crash
