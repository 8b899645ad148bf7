"""CPU: split-field edge layers (PvAmdSetEdgeLayerSplit) -- the tables at a given R0, the numpy restatement and its physics.

* PvAmdHostEdgeLayerTablesR0 equals the documented formula at that R0, computed again in numpy, bit for bit; at R0 = 0.1 it is
  PvAmdHostEdgeLayerTables; it refuses what PvAmdHostEdgeLayerTables refuses and an R0 outside (0, 1).
* With every width 0 the restatement (tests/_split_layer_ref.py) is the pinned oracle, fields and history bit for bit; the GPU
  tests (tests/test_gpu_split_layer.py) then compare the library against the restatement.
* The physics bar, on the harness of tests/test_host_layer.py (an open 160^2 grid at 275 Hz, listener at cell (40, 40), truth =
  the same window of a grid 300 cells larger): the error energy of the pressure of every cell outside the layers, with split
  layers at the default R0 against plain absorbing edges and against the unsplit layer.
* Stability: 20 T steps with walls reaching into the layers; the field energy does not grow past its value at T.
"""
import math
import os

import numpy as np
import pytest

from _boundary_ref import half_cell_box
from _layer_ref import layer_fdtd
from _split_layer_ref import analyze, courant_of, edge_layer_tables, layer_cells, split_fdtd, unit_tables
from test_host_layer import LC, N, PAD, TABLE_CASES, cell, size_of

F = np.float32


@pytest.mark.parametrize("r0", [0.1, 1e-2, 1e-4, 1e-6, 0.5])
@pytest.mark.parametrize("size,res,w4", TABLE_CASES)
def test_tables_r0_match_the_formula(oracle, size, res, w4, r0):
    from planeverb_amd import api
    got = api.edge_layer_tables(size, size, res, w4, r0=r0)
    o = oracle.OracleGrid(size, size, res, with_history=False)
    want = edge_layer_tables(o.gx, o.gy, courant_of(o), w4, R0=r0)
    o.close()
    for k, v in want.items():
        assert got[k].shape == v.shape and np.array_equal(got[k].view(np.uint32), v.view(np.uint32)), (k, r0)
    # layer cells: exactly the cells of depth > 0 along x or along y (the ghost row x = gx has no depth along x, but its
    # cells inside a y layer are layer cells; the ghost column likewise)
    gx, gy = got["apx"].size - 1, got["apy"].size - 1
    lay = layer_cells(got, gx, gy)
    want_lay = np.zeros((gx + 1, gy + 1), bool)
    want_lay[:w4[0]] = want_lay[gx - w4[1]:gx] = True
    want_lay[:, :w4[2]] = want_lay[:, gy - w4[3]:gy] = True
    assert np.array_equal(lay, want_lay)
    assert not lay[gx, w4[2]:gy - w4[3]].any() and not lay[w4[0]:gx - w4[1], gy].any()


@pytest.mark.parametrize("size,res,w4", TABLE_CASES)
def test_tables_r0_default_is_the_unsplit_tables(size, res, w4):
    from planeverb_amd import api
    a = api.edge_layer_tables(size, size, res, w4)
    b = api.edge_layer_tables(size, size, res, w4, r0=0.1)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_tables_r0_refusals():
    from planeverb_amd import api
    for w4 in ((-1, 0, 0, 0), (0, 65, 0, 0), (0, 0, 35, 28), (32, 31, 0, 0)):
        with pytest.raises(api.PlaneverbError):
            api.edge_layer_tables(25.0, 25.0, 275, w4, r0=1e-4)
    for r0 in (0.0, 1.0, -1e-4, 1.5, math.nan, math.inf, -math.inf):
        with pytest.raises(api.PlaneverbError, match="r0"):
            api.edge_layer_tables(25.0, 25.0, 275, (8, 8, 8, 8), r0=r0)
    assert api.EDGE_LAYER_SPLIT_R0 == 1e-4
    api.edge_layer_tables(25.0, 25.0, 275, (31, 31, 31, 31), r0=api.EDGE_LAYER_SPLIT_R0)


def test_zero_width_restatement_is_the_oracle(oracle):
    """all widths 0: the split restatement is the pinned oracle's stencil, fields and history bit for bit"""
    from planeverb_amd import api
    scene = os.path.join(os.path.dirname(__file__), "scenes", "SmallRoomScene.pv")
    boxes = api.load_pv(scene)
    L = (5.0, 0.0, 4.0)
    o = oracle.OracleGrid(25.0, 25.0, 275, boxes)
    want = o.fdtd(L, want_fields=True)
    hp, hx, hy = (h.copy() for h in o.history())
    ef = F(oracle.free_energy(25.0, 25.0, 275))
    r0, d0, _ = o.analyze(ef, L)
    got, hist, _, extra = split_fdtd(o, L, unit_tables(o.gx, o.gy))
    for k in range(3):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "field %d" % k
    for a, b in zip(hist, (hp, hx, hy)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not extra["px"].any()
    r, d = analyze(o, hist, ef, L)
    assert np.array_equal(r.view(np.uint32), r0.view(np.uint32)) and np.array_equal(d.view(np.uint32), d0.view(np.uint32))
    o.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the physics bar (profiles/edge_layer.txt: 43.0 dB at width 24 and 31.7 dB at width 8 with R0 = 1e-4 on this harness; the
# unsplit layer at R0 = 0.1 gives 11.3 dB)
# ------------------------------------------------------------------------------------------------------------------------------
BAR_DB_24 = 35.0
BAR_DB_8 = 25.0
BAR_OVER_UNSPLIT_DB = 20.0


@pytest.fixture(scope="module")
def physics(oracle):
    from planeverb_amd import api
    r0 = api.EDGE_LAYER_SPLIT_R0
    small = oracle.OracleGrid(size_of(N), size_of(N), 275)
    big = oracle.OracleGrid(size_of(N + 2 * PAD), size_of(N + 2 * PAD), 275, with_history=False)
    L, Lb = cell(LC, LC), cell(LC + PAD, LC + PAD)
    _, truth, _ = layer_fdtd(big, Lb, unit_tables(big.gx, big.gy), win=(PAD, PAD, N + 1, N + 1))
    _, plain, _ = layer_fdtd(small, L, unit_tables(N, N))
    out = dict(truth=truth, plain=plain)
    _, out["unsplit24"], _ = layer_fdtd(small, L, api.edge_layer_tables(size_of(N), size_of(N), 275, (24,) * 4))
    for w in (24, 8):
        _, out["split%d" % w], _, _ = split_fdtd(small, L, api.edge_layer_tables(size_of(N), size_of(N), 275, (w,) * 4, r0=r0))
    ef = F(oracle.free_energy(size_of(N), size_of(N), 275))
    for k in ("plain", "unsplit24", "split24"):
        out["r_" + k], _ = analyze(small, out[k], ef, L)
    hp, hx, hy = small.history()
    hp[:], hx[:], hy[:] = truth
    out["r_truth"], _, _ = small.analyze(ef, Lb, offset=(PAD, PAD))
    small.close()
    big.close()
    return out


def error_energy(physics, key, w):
    inner = (slice(None), slice(w, N - w), slice(w, N - w))
    t = physics["truth"][0][inner].astype(np.float64)
    return ((physics[key][0][inner] - t) ** 2).sum()


@pytest.mark.parametrize("w,bar", [(24, BAR_DB_24), (8, BAR_DB_8)])
def test_split_error_energy_below_plain_edges(physics, w, bar):
    db = 10 * np.log10(error_energy(physics, "plain", w) / error_energy(physics, "split%d" % w, w))
    assert db >= bar, "split layer, width %d: error energy only %.2f dB below plain absorbing edges" % (w, db)


def test_split_beats_the_unsplit_layer(physics):
    db = 10 * np.log10(error_energy(physics, "unsplit24", 24) / error_energy(physics, "split24", 24))
    assert db >= BAR_OVER_UNSPLIT_DB, "split layer only %.2f dB below the unsplit layer" % db


def test_split_wet_gain_and_rt60_closer_to_open_field(physics):
    w = 24
    sl = (slice(w, N - w), slice(w, N - w))
    for k, name in ((1, "wetGain"), (2, "rt60")):
        t = physics["r_truth"][sl + (k,)].astype(np.float64)
        eu = np.abs(physics["r_unsplit24"][sl + (k,)] - t)
        es = np.abs(physics["r_split24"][sl + (k,)] - t)
        ok = np.isfinite(t) & np.isfinite(eu) & np.isfinite(es)
        assert ok.sum() > 1000, name
        assert es[ok].mean() < eu[ok].mean(), "%s: mean error %.4g split, %.4g unsplit" % (name, es[ok].mean(), eu[ok].mean())


# ------------------------------------------------------------------------------------------------------------------------------
# stability: walls inside the layers, 20 T steps (the pulse ends at T)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [24, 8])
def test_split_stable_over_20T_with_walls_in_the_layers(oracle, w):
    from planeverb_amd import api
    n = 96
    dx = F(343.21) / F(275) / F(3.5)
    boxes = np.array([half_cell_box(dx, 2, 9, 30, 60, 0.3),           # inside the x = 0 layer
                      half_cell_box(dx, 40, 46, n - 14, n + 1, 0.1),   # across the y = gy layer into the grid edge
                      half_cell_box(dx, n - w - 4, n - 1, 10, 14, 0.8),  # through the x = gx layer's inner boundary
                      half_cell_box(dx, 44, 50, 44, 50, 0.5)], np.float32)
    o = oracle.OracleGrid(size_of(n), size_of(n), 275, boxes, with_history=False)
    assert o.gx == n
    tabs = api.edge_layer_tables(size_of(n), size_of(n), 275, (w,) * 4, r0=api.EDGE_LAYER_SPLIT_R0)
    T = o.T
    _, _, _, extra = split_fdtd(o, cell(60, 40), tabs, steps=20 * T, record=False, energy=True)
    o.close()
    # e[t]: after step t's stencil, before its pulse -- e[T] is the first value with the whole pulse.  pr^2 + vx^2 + vy^2 is
    # not the staggered scheme's conserved form, so it ripples by a few per cent from step to step: the values compared are
    # those at every multiple of T, and every value from 2 T on
    e = extra["energy"]
    assert np.isfinite(e).all() and e[T] > 0
    at = e[np.arange(2, 20) * T]
    assert (at <= e[T]).all(), "width %d: energy at multiples of T %s exceeds %.4g at T" % (w, at, e[T])
    worst = e[2 * T:].max()
    assert worst <= e[T], "width %d: energy %.4g at step %d exceeds %.4g at T" % (w, worst, 2 * T + int(e[2 * T:].argmax()), e[T])
    assert e[-1] < 0.1 * e[T]
