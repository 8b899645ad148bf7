"""CPU: the restatement against the compiled reference itself (oracle/_ref/libpvref.so) on cases beyond the other
fixtures.  The reference's outputs for these cases are pinned in tests/golden/g_vsref.npz (tests/golden/make_golden.py
vsref, which also defines the cases), the FindGain table in g_findgain.npz (make_golden.py findgain)."""
import os
import sys

import numpy as np
import pytest

from conftest import SCENES, golden, same_bits

from oracle import pvref

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_golden import VSREF_EFREE, VSREF_GEOMETRY, VSREF_SCENES, findgain_inputs, vsref_snap_ts  # noqa: E402


@pytest.mark.parametrize("scene,listener,res,size", VSREF_SCENES)
def test_restatement_equals_reference(oracle, scene, listener, res, size):
    g = golden("g_vsref")
    key = "scene%d_" % VSREF_SCENES.index((scene, listener, res, size))
    boxes = pvref.load_pv(os.path.join(SCENES, scene))
    o = oracle.OracleGrid(size, size, res, boxes)
    assert [o.gx, o.gy, o.T, o.fs] == g[key + "dims"].tolist()
    o.fdtd(listener)
    hp, hx, hy = o.history()
    for t, (p, x, y) in zip(vsref_snap_ts(o.T), g[key + "snaps"]):
        assert same_bits(p, hp[t]).all() and same_bits(x, hx[t]).all() and same_bits(y, hy[t]).all()
    ef = oracle.free_energy(size, size, res)
    assert np.float32(ef) == g[key + "efree"]
    res8, delay, valid = o.analyze(ef, listener)
    rres, rdelay = g[key + "results"], g[key + "delay"]
    assert same_bits(delay, rdelay).all()
    for k in range(8):
        m = valid if k not in (4, 5) else np.ones_like(valid)
        assert same_bits(res8[..., k][m], rres[..., k][m]).all(), k
    o.close()


def test_dynamic_geometry_sequence(oracle):
    """Add / Remove / overlapping boxes follow Grid::AddAABB / RemoveAABB incl. quirk Q4 (overlap cleared)"""
    g = golden("g_vsref")
    o = oracle.OracleGrid(25.0, 25.0, 275, None, with_history=False)
    for (op, box), rb, rR in zip(VSREF_GEOMETRY, g["geometry_beta"], g["geometry_R"]):
        getattr(o, op + "_aabb")(np.array(box, np.float32))
        ob, oR = o.material()
        assert np.array_equal(rb, ob) and same_bits(rR, oR).all(), op
    o.close()


@pytest.mark.parametrize("size,res", VSREF_EFREE)
def test_free_energy_incl_truncation_quirk(oracle, size, res):
    """FreeGrid passes its centre cell as metres and GenerateResponse truncates it again (FreeGrid.cpp:84,
    FDTD.cpp:97-98): at 40 m / 275 Hz the source lands one cell off in x AND y and EFree drops to 0.028847
    (SURVEY.md H4).  The restatement must follow the reference through that."""
    efree = golden("g_vsref")["efree"][VSREF_EFREE.index((size, res))]
    assert np.float32(oracle.free_energy(size, size, res)) == efree
    if (size, res) == (40.0, 275):
        assert efree == np.float32(0.028847147)


def test_find_gains_equal_compiled_reference(oracle):
    """the oracle's restatement of FindGainA/B/C against the reference's own compiled
    PvDSPContext.cpp:165-228 (oracle/ref_dsp_harness.cpp), dense sweep incl. the 0.5 / 1.0 / 3.0 s edges: the committed
    table must hold exactly that sweep"""
    g = golden("g_findgain")
    assert np.array_equal(g["inputs"].view(np.uint32), findgain_inputs().view(np.uint32))
    for (rt, w), want in zip(g["inputs"], g["gains"]):
        got = np.array(oracle.find_gains(rt, w), np.float32)
        assert same_bits(got, want).all(), (rt, w, got, want)
