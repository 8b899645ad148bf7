"""GPU (-m gpu): auralisation (PvAmdSetAuralisation / PvAmdComputeAuralResponses / PvAmdAuralise; pv_aural.hip).

The expected values come from the numpy restatement (tests/_aural_ref.py, written from the definition in include/planeverb_amd.h)
applied to the SAME solver's recorded planes (history_plane(t) for all t) and the library's own tables, which are held to the
restatement's tables first.  Tolerance 0: conftest.same_bits, NaN == NaN."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

import _aural_ref as ref
from conftest import ROOT, SCENES, bits, golden, same_bits
from test_gpu_analysis_edges import open_size
from test_gpu_layer import cell_of
from test_gpu_spectrum import L400, N400
from test_gpu_emitter_records import edge_case_cells
from test_gpu_waterfall import history

pytestmark = pytest.mark.gpu

SMALLROOM = os.path.join(SCENES, "SmallRoomScene.pv")
NO_ONSET = 1e30
OFF_MAP = (-3.0, 0.0, 4.0)


def specials(v):
    """a denormal, a -0.0, one inf and one NaN sample, where there is room"""
    for i, s in enumerate((1.0e-41, -0.0, np.inf, np.nan)):
        if 3 * i + 1 < v.size:
            v[3 * i + 1] = s
    return v


def pick_receivers(s, delay, beta):
    """about 14 receivers, after test_gpu_waterfall.pick_receivers: reached cells spread over the tiles, a tile's first row, first
    column and corner, cells beside a wall, one IN a wall, one without an onset where there is one, and the first one once more"""
    ec = edge_case_cells({"delay": delay, "beta": beta}, s.info.tileRows, s.info.tileCols)
    reached = np.argwhere(delay < NO_ONSET)
    cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 4).astype(int)] + list(ec.values())
    return cells + [cells[0]]


def preset(pvlib, name="g71_smallroom", **opts):
    g = golden(name)
    s = pvlib.Solver(float(g["size"]), float(g["size"]), int(g["res"]), **opts)
    for b in g["boxes"]:
        s.add_geometry(b)
    return s, tuple(g["listener"])


def library_tables(pvlib, s, rate, Z, beta=9.0):
    """the solver's tables, held to the host function's and (at the sizes the restatement is quick at) to the restatement's"""
    first, w = s.aural_taps()
    hf, hw = pvlib.host_aural_taps(s.fs, s.T, rate, Z, beta)
    assert np.array_equal(first, hf) and np.array_equal(bits(w), bits(hw))
    rf, rw = ref.taps(s.fs, s.T, rate, Z, beta)
    assert np.array_equal(first, rf) and np.array_equal(bits(w), bits(rw))
    assert s.auralisation_setting() == (rate, Z, np.float32(beta), w.shape[0], w.shape[1])
    return first, w


def responses(s, n):
    return np.stack([s.aural_response(r) for r in range(n)])


def differ(got, want, ctx):
    bad = ~same_bits(got, want)
    assert got.shape == want.shape and not bad.any(), "%s: %d values differ, first at %s: %s vs %s" % (
        ctx, bad.sum(), np.argwhere(bad)[0], got[bad][:4], want[bad][:4])


@pytest.fixture(scope="module")
def room(pvlib):
    """one 70^2 run shared by the tests that only read it: the solver, its planes, its onset map and about 12 receivers"""
    s, L = preset(pvlib)
    with s:
        assert (s.gx, s.T, s.fs) == (70, 435, 1443)
        s.run(L)
        hist, delay, beta = history(s), s.results()[1], s.material()[0]
        cells = pick_receivers(s, delay, beta)
        yield {"s": s, "hist": hist, "delay": delay, "cells": cells, "p": np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)}
        s.set_auralisation(0)


# 1. responses on the 70^2 presets
@pytest.mark.parametrize("name", ["g71_smallroom", "g71_shoebox"])
def test_responses(pvlib, name):
    s, L = preset(pvlib, name)
    with s:
        s.run(L)
        hist, delay, beta = history(s), s.results()[1], s.material()[0]
        cells = pick_receivers(s, delay, beta)
        assert 12 <= len(cells) <= 16 and cells[-1] == cells[0]
        wall = beta[:s.gx, :s.gy] == 0
        assert any(wall[c] for c in cells) and any(not delay[c] < NO_ONSET for c in cells)
        assert len(set((c[0] // s.info.tileRows, c[1] // s.info.tileCols) for c in cells)) >= 2
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        pos = [cell_of(*c) for c in cells]
        for rate in (1443, 1000, 8000):
            for Z in (4, 16):
                s.set_auralisation(rate, Z, 9.0)
                first, w = library_tables(pvlib, s, rate, Z)
                assert s.compute_aural_responses(pos) > 0
                got = responses(s, len(cells))
                differ(got, ref.resample(p, first, w).T, "%s rate=%d Z=%d" % (name, rate, Z))
                assert same_bits(got[-1], got[0]).all() and np.abs(got[0]).max() > 1e-3  # (the duplicate and its twin)
                for i, c in enumerate(cells):
                    if wall[c]:
                        assert not got[i].any()
        # at the grid's own rate the middle tap is 1 and the others vanish at the integers: the response is the history's bits
        # up to the window's roundings
        s.set_auralisation(1443, 16, 9.0)
        s.compute_aural_responses(pos)
        assert np.abs(responses(s, len(cells)) - p.T).max() < 1e-6
        # a position off the map is refused, by its index, and the responses stay
        before = responses(s, len(cells))
        with pytest.raises(pvlib.PlaneverbError, match=r"aural: a position off the map \(position 2\)"):
            s.compute_aural_responses(pos[:2] + [OFF_MAP] + pos[2:4])
        differ(responses(s, len(cells)), before, "after a refusal")


# 2. a history window smaller than the grid: receivers in tiles with a tile origin other than 0, one outside the window
@pytest.mark.parametrize("where", list(L400))
def test_window_smaller_than_the_grid(pvlib, where):
    size = open_size(N400)
    with pvlib.Solver(size, size, 275, num_steps=160) as s:
        assert s.gx == N400 and s.T == 160 and 2 * s.T + 3 < N400
        s.load_scene(SMALLROOM)
        s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
        s.run(L400[where])
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 9).astype(int)]
        far = (10, 398) if where == "offset" else (398, 398)  # inside the grid, outside the window
        assert delay[far] >= NO_ONSET
        cells.append(far)
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        s.set_auralisation(8000, 16, 9.0)
        first, w = s.aural_taps()
        s.compute_aural_responses([cell_of(*c) for c in cells])
        got = responses(s, len(cells))
        differ(got, ref.resample(p, first, w).T, where)
        assert not got[-1].any() and all(np.abs(g).max() > 0 for g in got[:-1])


# 3. the convolution and the mix, both kernels
def render_case(pvlib, s, p, pos, rate, ns, ctx):
    B, C = pvlib.aural_shape()
    s.set_auralisation(rate, 16, 9.0)
    first, w = s.aural_taps()
    s.compute_aural_responses(pos)
    R, L = len(pos), w.shape[0]
    h = responses(s, R)
    differ(h, ref.resample(p, first, w).T, ctx)
    rng = np.random.default_rng(L)
    route = np.array([(0, 1, -1, 2, 1, 0)[r % 6] for r in range(R)], np.int32)   # a -1, repeated signals
    gain = np.array([(1.0, -0.5, 0.25, 0.75, -1.25, 0.5)[r % 6] for r in range(R)], np.float32)
    for N in ns:
        x = rng.standard_normal((3, N)).astype(np.float32)
        specials(x[1])
        want_out, want_mix = ref.render(h, x, route, gain)
        for form in (pvlib.AURAL_TILED, pvlib.AURAL_PLAIN):
            s.set_aural_form(form)
            assert s.auralise(x, route, gain) > 0
            for r in range(R):
                differ(s.aural_output(r), want_out[r], "%s L=%d N=%d form=%d receiver %d" % (ctx, L, N, form, r))
                assert (route[r] >= 0) or not s.aural_output(r).any()
            differ(s.aural_mix(), want_mix, "%s L=%d N=%d form=%d mix" % (ctx, L, N, form))
        s.set_aural_form(pvlib.AURAL_TILED)
    return B, C, L


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("rate", [1000, 8000])
def test_convolution(pvlib, room, rate):
    s, B = room["s"], pvlib.aural_shape()[0]
    L = pvlib.host_aural_shape(s.fs, s.T, rate)[0]
    assert L == {1000: 301, 8000: 2407}[rate]
    k = (L + 100) // B + 1
    ns = [1, 2, 65] + [k * B - L + 1 + d for d in (-1, 0, 1)]  # M = N + L - 1 one below, at and one above a multiple of B
    assert min(ns) >= 1 and max(ns) <= 300
    idx = [0, 1, 2, 3, 5, len(room["cells"]) - 1]
    _, C, _ = render_case(pvlib, s, room["p"][:, idx], [cell_of(*room["cells"][i]) for i in idx], rate, ns, "rate %d" % rate)
    assert L > C


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("steps,want_l", [(100, 69), (185, 128), (186, 129)])
def test_convolution_short_responses(pvlib, steps, want_l):
    """no legal rate puts L at or below the chunk of taps at T = 435 (L = 301 at 1000): shorter runs do"""
    B, C = pvlib.aural_shape()
    assert 65 < C <= 128 and want_l in (69, C, C + 1)
    s, Lpos = preset(pvlib, num_steps=steps)
    with s:
        s.run(Lpos)
        assert s.T == steps
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 4).astype(int)]
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        ns = [1, 2, 65, C, B - want_l, B - want_l + 1, B - want_l + 2, 2 * B + 7]
        _, _, L = render_case(pvlib, s, p, [cell_of(*c) for c in cells], 1000, ns, "T=%d" % steps)
        assert L == want_l


# 4. independence: a receiver's response and output do not depend on the other receivers or their order
def test_independence(pvlib, room):
    s, cells = room["s"], room["cells"]
    s.set_auralisation(8000, 16, 9.0)
    x = np.random.default_rng(5).standard_normal((2, 150)).astype(np.float32)
    target = cells[1]
    s.compute_aural_responses([cell_of(*target)])
    s.auralise(x, [1], [0.5])
    h, o = s.aural_response(0), s.aural_output(0)
    assert np.abs(o).max() > 0
    others = [c for c in cells if c != target][:11]
    for order, at in ((others[:4] + [target] + others[4:], 4), ([target] + others[::-1], 0), (others + [target], 11)):
        s.compute_aural_responses([cell_of(*c) for c in order])
        route = np.zeros(12, np.int32)
        route[at] = 1
        s.auralise(x, route, np.linspace(-1, 1, 12))
        assert same_bits(s.aural_response(at), h).all() and same_bits(s.aural_output(at), o).all(), at


# 5. sparse-emitter mode: the emitters' traces as the sample source, against the solver that keeps its history
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_sparse_emitters(pvlib, room):
    full = room["s"]
    cells = list(dict.fromkeys(room["cells"]))  # (distinct: an emitter per cell)
    pos = [cell_of(*c) for c in cells]
    s, L = preset(pvlib, streaming_analysis=1)
    with s:
        s.set_emitters([OFF_MAP] + pos)  # (the position off the map is dropped)
        assert [tuple(c) for c in s.emitter_cells()] == cells
        x = specials(np.random.default_rng(9).standard_normal((1, 120)).astype(np.float32).reshape(-1)).reshape(1, -1)
        route, gain = np.zeros(len(cells), np.int32), np.linspace(1.0, -1.0, len(cells)).astype(np.float32)
        for sv in (full, s):
            sv.set_auralisation(8000, 16, 9.0)
        with pytest.raises(pvlib.PlaneverbError, match="aural: no completed run"):
            s.compute_aural_responses()
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="aural: a sparse-emitter solver takes no positions"):
            s.compute_aural_responses(pos)
        assert s.compute_aural_responses() > 0
        full.compute_aural_responses(pos)
        for sv in (full, s):
            sv.auralise(x, route, gain)
        for r in range(len(cells)):
            differ(s.aural_response(r), full.aural_response(r), "response %d" % r)
            differ(s.aural_output(r), full.aural_output(r), "output %d" % r)
            assert same_bits(s.aural_response(r), pvlib.host_aural_resample(s.emitter_trace(r), *s.aural_taps())).all()
        differ(s.aural_mix(), full.aural_mix(), "mix")
        # a change of the emitters: the responses and the traces are the old table's
        s.set_emitters(pos[:3])
        for call in (lambda: s.aural_response(0), lambda: s.aural_output(0), s.aural_mix):
            with pytest.raises(pvlib.PlaneverbError, match="aural: no (responses|outputs)"):
                call()
        with pytest.raises(pvlib.PlaneverbError, match="aural: no completed run"):
            s.compute_aural_responses()
        s.run(L)
        s.compute_aural_responses()
        differ(s.aural_response(2), full.aural_response(2), "after new emitters")


# 6. the array source: the responses of the source arrays
def test_array_source(pvlib, room):
    s, cells = room["s"], room["cells"]
    dl = lambda k: float(np.float32(k / s.fs))
    arrays = [[(cell_of(*cells[0]), 1.0, 0.0)],
              [(cell_of(*cells[1]), 0.8, 0.0), (cell_of(*cells[2]), -0.5, dl(7.3)), (cell_of(*cells[3]), 0.25, dl(31))]]
    s.set_auralisation(8000, 16, 9.0)
    first, w = s.aural_taps()
    try:
        s.set_arrays(arrays)
        with pytest.raises(pvlib.PlaneverbError, match="aural: the array responses are not computed"):
            s.compute_aural_responses(source=pvlib.AURAL_ARRAYS)
        s.compute_arrays()
        with pytest.raises(pvlib.PlaneverbError, match="aural: the array source takes no positions"):
            s.compute_aural_responses([cell_of(*cells[0])], source=pvlib.AURAL_ARRAYS)
        assert s.compute_aural_responses(source=pvlib.AURAL_ARRAYS) > 0
        y = np.stack([s.array_response(a) for a in range(2)], axis=1)
        got = responses(s, 2)
        differ(got, ref.resample(y, first, w).T, "arrays")
        differ(got[0], ref.resample(room["p"][:, 0], first, w), "the identity array")
        x = np.random.default_rng(2).standard_normal((1, 90)).astype(np.float32)
        s.auralise(x, [0, 0], [1.0, -1.0])
        want_out, want_mix = ref.render(got, x, [0, 0], [1.0, -1.0])
        differ(np.stack([s.aural_output(0), s.aural_output(1)]), want_out, "array outputs")
        differ(s.aural_mix(), want_mix, "array mix")
        # whatever invalidates the array responses invalidates what was resampled from them: a changed kind selection, a new
        # compute (the responses may be other ones), a new setting
        s.set_array_records(pvlib.QREC_ROOM_METRICS)
        with pytest.raises(pvlib.PlaneverbError, match="aural: no responses"):
            s.aural_response(0)
        s.compute_arrays()
        with pytest.raises(pvlib.PlaneverbError, match="aural: no (responses|outputs)"):
            s.aural_mix()
        s.compute_aural_responses(source=pvlib.AURAL_ARRAYS)
        differ(responses(s, 2), got, "again")
        s.set_arrays(arrays[:1])
        with pytest.raises(pvlib.PlaneverbError, match="aural: no responses"):
            s.aural_response(0)
        # the receivers' responses do not depend on the arrays
        s.compute_aural_responses([cell_of(*cells[0])])
        s.set_arrays([])
        differ(s.aural_response(0), got[0], "receivers after the arrays went")
        with pytest.raises(pvlib.PlaneverbError, match="aural: no arrays set"):
            s.compute_aural_responses(source=pvlib.AURAL_ARRAYS)
    finally:
        s.set_arrays([])
        s.set_array_records(0, 0)


# 7. lifetimes
def test_lifetime(pvlib):
    s, L = preset(pvlib)
    plain, _ = preset(pvlib)
    g = golden("g71_smallroom")
    E = [tuple(e) for e in g["emitters"]][:3]
    x = np.random.default_rng(1).standard_normal((2, 70)).astype(np.float32)
    route, gain = [0, 1, -1], [1.0, 0.5, 2.0]

    def stale(outputs_only=False):
        for call in (lambda: s.aural_output(0), s.aural_mix) + (() if outputs_only else (lambda: s.aural_response(0),)):
            with pytest.raises(pvlib.PlaneverbError, match="aural: no (responses|outputs)"):
                call()

    def render():
        s.compute_aural_responses(E)
        s.auralise(x, route, gain)
        return responses(s, 3), np.stack([s.aural_output(r) for r in range(3)]), s.aural_mix()

    with s, plain:
        # no setting: nothing is there, every call says so, and a run leaves what a solver that never heard of this leaves
        assert s.auralisation_setting() is None
        for call in (s.aural_taps, lambda: s.compute_aural_responses(E), lambda: s.aural_response(0), lambda: s.auralise(x, route, gain),
                     lambda: s.aural_output(0), s.aural_mix):
            with pytest.raises(pvlib.PlaneverbError, match="aural: no setting"):
                call()
        assert pvlib.lib().PvAmdGetAuralTaps(s._h, None, None, 0) == -1 and pvlib.lib().PvAmdCopyAuralMix(s._h, None) == -1
        s.set_auralisation(8000, 16, 9.0)
        with pytest.raises(pvlib.PlaneverbError, match="aural: no completed run"):
            s.compute_aural_responses(E)
        for sv in (s, plain):
            sv.run(L)
        for a, b in zip(s.results(), plain.results()):
            assert same_bits(a, b).all()
        assert same_bits(s.history_plane(200), plain.history_plane(200)).all()
        assert s.timings().fdtdMs > 0
        stale()
        first = render()
        assert np.abs(first[2]).max() > 0 and not first[1][2].any()
        # the map kinds and this section do not touch each other
        s.compute_room_metrics()
        metrics = s.room_metrics()
        again = render()
        for a, b in zip(first, again):
            differ(b, a, "again")
        assert same_bits(s.room_metrics(), metrics).all()
        # refused calls change nothing
        for bad in (dict(rate=999), dict(rate=384001), dict(Z=1), dict(Z=65), dict(beta=-1.0), dict(beta=21.0), dict(beta=float("nan"))):
            a = dict(dict(rate=8000, Z=16, beta=9.0), **bad)
            with pytest.raises(pvlib.PlaneverbError, match="^aural: "):
                s.set_auralisation(a["rate"], a["Z"], a["beta"])
        for bad in (dict(positions=[]), dict(positions=[E[0]] * 257)):
            with pytest.raises(pvlib.PlaneverbError, match="aural: 1 .. 256 positions"):
                s.compute_aural_responses(**bad)
        with pytest.raises(pvlib.PlaneverbError, match="aural: 1 .. 256 positions"):
            s.compute_aural_responses(None)
        with pytest.raises(pvlib.PlaneverbError, match="aural: source is"):
            s.compute_aural_responses(E, source=2)
        lib, fp, ip = pvlib.lib(), lambda a: a.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float)), lambda a: a.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_int))
        rt, gn = np.array(route, np.int32), np.array(gain, np.float32)
        for args, why in (((None, 2, 70, ip(rt), fp(gn), None), "null"), ((fp(x), 2, 70, None, fp(gn), None), "null"),
                          ((fp(x), 2, 70, ip(rt), None, None), "null"), ((fp(x), 0, 70, ip(rt), fp(gn), None), "1 .. 64 signals"),
                          ((fp(x), 65, 70, ip(rt), fp(gn), None), "1 .. 64 signals"), ((fp(x), 2, 0, ip(rt), fp(gn), None), "samples"),
                          ((fp(x), 2, (1 << 20) + 1, ip(rt), fp(gn), None), "samples"),
                          ((fp(x), 1, 70, ip(rt), fp(gn), None), "route"),
                          ((fp(x), 2, 70, ip(np.array([0, -2, 0], np.int32)), fp(gn), None), "route"),
                          ((fp(x), 2, 70, ip(rt), fp(np.array([1.0, np.inf, 1.0], np.float32)), None), "gain")):
            assert lib.PvAmdAuralise(s._h, *args) == -1 and why in pvlib.last_error() and pvlib.last_error().startswith("aural:"), why
        for r in (-1, 3):
            with pytest.raises(pvlib.PlaneverbError, match="aural: no such receiver"):
                s.aural_response(r)
            with pytest.raises(pvlib.PlaneverbError, match="aural: no such receiver"):
                s.aural_output(r)
        differ(s.aural_mix(), first[2], "after refusals")
        # R * M above 2^26: 256 receivers, N = 2^18
        s.compute_aural_responses([E[0]] * 256)
        big = np.zeros((1, 1 << 18), np.float32)
        with pytest.raises(pvlib.PlaneverbError, match="aural: more than 2\\^26 output samples"):
            s.auralise(big, [0] * 256, [1.0] * 256)
        # new responses drop the outputs
        render()
        s.compute_aural_responses(E)
        stale(outputs_only=True)
        differ(s.aural_response(1), first[0][1], "the responses are there")
        # a changed setting
        render()
        s.set_auralisation(8000, 4, 9.0)
        stale()
        s.set_auralisation(8000, 16, 9.0)
        stale()
        # geometry, boundary, layer
        render()
        gid = s.add_geometry((12.0, 12.0, 2.0, 2.0, 0.5))
        stale()
        for a, b in zip(first, render()):  # (the last completed run is still the first one)
            differ(b, a, "after a geometry change")
        s.set_grid_boundary((1, 0, 0, 0))
        stale()
        render()
        s.set_edge_layer((8, 8, 8, 8))
        stale()
        s.set_edge_layer((0, 0, 0, 0))
        s.set_grid_boundary((0, 0, 0, 0))
        s.remove_geometry(gid)
        # a run between compute and copy
        render()
        s.run((7.0, 0.0, 9.5))
        stale()
        second = render()
        assert not same_bits(second[2], first[2]).all()
        # cleared: nothing is left
        s.set_auralisation(0)
        assert s.auralisation_setting() is None
        for call in (lambda: s.compute_aural_responses(E), lambda: s.aural_response(0), s.aural_mix):
            with pytest.raises(pvlib.PlaneverbError, match="aural: no setting"):
                call()


def test_runs_are_unchanged(pvlib):
    """a run under a setting, the passes between two runs and a run after the setting was cleared leave the result and onset maps and
    the history of a solver that never called the setter"""
    s, L = preset(pvlib)
    plain, _ = preset(pvlib)
    E = [tuple(e) for e in golden("g71_smallroom")["emitters"]][:3]
    x = np.random.default_rng(1).standard_normal((1, 70)).astype(np.float32)
    with s, plain:
        def both(at):
            for sv in (s, plain):
                sv.run(at)
            for a, b in zip(s.results(), plain.results()):
                assert same_bits(a, b).all(), at
            assert same_bits(s.history_plane(200), plain.history_plane(200)).all()

        s.set_auralisation(8000, 16, 9.0)
        both(L)
        s.compute_aural_responses(E)
        s.auralise(x, [0, 0, -1])
        both((7.0, 0.0, 9.5))
        s.compute_aural_responses(E)
        s.auralise(x, [0, 0, -1])
        s.set_auralisation(0)
        both((6.0, 0.0, 5.0))


def test_refusals(pvlib):
    L, E = (5.0, 0.0, 4.0), (5.0, 0.0, 6.0)
    # no onset map is needed
    with pvlib.Solver(25.0, 25.0, 275, skip_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_auralisation(8000, 16, 9.0)
        s.run(L)
        s.compute_aural_responses([E])
        h = s.aural_response(0)
        p = np.array([s.history_plane(t)[pvlib.host_cells(25.0, 25.0, 275, E[0], E[2])[1]] for t in range(s.T)], np.float32)
        assert same_bits(h, pvlib.host_aural_resample(p, *s.aural_taps())).all() and np.abs(h).max() > 0
    with pvlib.Solver(25.0, 25.0, 275, streaming_analysis=1) as s:
        s.load_scene(SMALLROOM)
        s.set_auralisation(8000, 16, 9.0)
        with pytest.raises(pvlib.PlaneverbError, match="aural: no emitters registered"):
            s.compute_aural_responses()
        s.set_emitters([cell_of(i % 60 + 2, i // 60 + 2) for i in range(257)])
        s.run(L)
        with pytest.raises(pvlib.PlaneverbError, match="aural: at most 256 registered emitters"):
            s.compute_aural_responses()
    with pvlib.Solver(open_size(512), open_size(512), 275, slabs=[0, 0]) as s:
        s.run(L)
        for call in (lambda: s.set_auralisation(8000, 16, 9.0), lambda: s.compute_aural_responses([E]), lambda: s.aural_response(0),
                     s.auralisation_setting, s.aural_mix):
            with pytest.raises(pvlib.PlaneverbError, match="aural: .*slab"):
                call()
    s512 = open_size(512)
    rank = pvlib.SlabRank(s512, s512, 275, 0, 0, 2, pvlib.compute_efree(s512, s512, 275))
    try:
        for call in (lambda: rank.solver.set_auralisation(8000, 16, 9.0), lambda: rank.solver.compute_aural_responses([E]),
                     rank.solver.auralisation_setting):
            with pytest.raises(pvlib.PlaneverbError, match="^aural: slab rank"):
                call()
    finally:
        rank.close()
    # (the refusal of a last run that ended in error has no test: nothing makes a run fail short of a device fault)
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.set_auralisation(48000, 16, 9.0)
        assert s.auralisation_setting()[3:] == (14437, 33)
        with pytest.raises(pvlib.PlaneverbError, match="aural: a rate of"):
            s.set_auralisation(999, 16, 9.0)
        assert s.auralisation_setting()[0] == 48000  # (a refused setting leaves the one before)
        s.run_steps(8, with_pulse=True, listener=L)  # (raw stepping records no history)
        with pytest.raises(pvlib.PlaneverbError, match="aural: no completed run"):
            s.compute_aural_responses([E])


# 8. the command line, once per mode
@pytest.mark.parametrize("mode", ["history", "sparse-emitters", "array"])
def test_cli(pvlib, mode, tmp_path):
    rate = 8000
    x = (np.random.default_rng(4).standard_normal(200) * 0.2).clip(-0.99, 0.99)
    pcm = np.round(x * 32767.0).astype("<i2")
    sig = str(tmp_path / "dry.wav")
    with wave.open(sig, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(pcm.tobytes())
    dry = pcm.astype(np.float32) / np.float32(32768.0)
    out_path = str(tmp_path / ("mix.wav" if mode == "array" else "mix.npy"))
    E, A = ["5,0,6", "12,0,9", "-3,0,4"], ["5,6,1,0;12,9,-0.5,0.003", "7,7,0.25,0.0101"]
    cmd = [sys.executable, "-m", "planeverb_amd", SMALLROOM, "--listener", "5,0,4"] + ["--emitter=" + e for e in E]
    cmd += ["--auralise", sig, "--aural-rate", str(rate), "--aural-out", out_path]
    cmd += {"history": [], "sparse-emitters": ["--sparse-emitters"], "array": ["--array=" + a for a in A]}[mode]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = json.loads(subprocess.run(cmd, capture_output=True, text=True, check=True, cwd=ROOT, env=env, timeout=300).stdout)
    au = out["auralisation"]
    with pvlib.Solver(25.0, 25.0, 275) as s:
        s.load_scene(SMALLROOM)
        s.run((5.0, 0.0, 4.0))
        s.set_auralisation(rate, 16, 9.0)
        if mode == "array":
            arrays = [[((float(a), 0.0, float(b)), float(c), float(d)) for a, b, c, d in (m.split(",") for m in arr.split(";"))] for arr in A]
            s.set_arrays(arrays)
            s.compute_arrays()
            s.compute_aural_responses(source=pvlib.AURAL_ARRAYS)
            count = 2
        else:
            s.compute_aural_responses([(5.0, 0.0, 6.0), (12.0, 0.0, 9.0)])  # (the emitter off the map renders nothing)
            count = 2
        s.auralise(dry, [0] * count)
        want = s.aural_mix()
        assert (au["rate"], au["receivers"], au["signalSamples"], au["samples"]) == (rate, count, 200, want.size)
        assert (au["responseSamples"], au["tapsPerSample"]) == s.auralisation_setting()[3:]
        assert au["source"] == ("arrays" if mode == "array" else "emitters") and same_bits(np.float32(au["peak"]), np.abs(want).max())
    if mode == "array":
        with wave.open(out_path, "rb") as f:
            assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, rate, want.size)
            got = np.frombuffer(f.readframes(want.size), "<i2")
        assert np.abs(got).max() == 32767
        assert np.array_equal(got, np.round(want.astype(np.float64) / np.abs(want.astype(np.float64)).max() * 32767.0).astype("<i2"))
    else:
        got = np.load(out_path)
        assert got.dtype == np.float32 and same_bits(got, want).all()
