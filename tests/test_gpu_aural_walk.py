"""GPU (-m gpu): the auralisation's convolution on its whole-chunk path, its passes on histories the stencil never produces, and
the resampler and the launch grid at the definition's limits (pv_aural.hip).

tests/test_gpu_aural.py keeps N <= 300 at the long responses, so every chunk of its walks but two takes the general path (the
regression note in tests/test_host_aural.py).  Here every case first asserts, from the restated walk (_aural_ref.chunk_walk, pinned to
brute force without a device), that it reaches the pattern of whole (W) and general (g) chunks it was written for, and then holds
every receiver's output and the mix of BOTH kernels to the numpy restatement of the definition (_aural_ref.render).  Tolerance 0:
conftest.same_bits, NaN == NaN."""
import re

import numpy as np
import pytest

import _adversarial as adv
import _aural_ref as ref
from test_gpu_analysis_edges import open_size
from test_gpu_aural import NO_ONSET, SMALLROOM, differ, library_tables, pick_receivers, preset, responses
from test_gpu_layer import cell_of
from test_gpu_spectrum import L400, N400
from test_gpu_waterfall import history

pytestmark = pytest.mark.gpu

SEED = 20261021
ROUTE6, GAIN6 = (0, 1, -1, 2, 1, 0), (1.0, -0.5, 0.25, 0.75, -1.25, 0.5)  # (test_gpu_aural.render_case's: a -1, repeated signals)


def whole_chunks(walks):
    """(whole chunks, chunks, the longest run of whole chunks in one block)"""
    return (sum(s.count("W") for s in walks), sum(len(s) for s in walks), max([len(m) for s in walks for m in re.findall("W+", s)] + [0]))


def walk_signals(N, seed, count=3, nonfinite=True):
    """`count` signals of N normal samples; signal 0 scaled by 1e-20 and the last by 1e20 (with responses of the adversarial
    families the products go denormal in the one and overflow in the other); every signal carries a denormal and -0.0 and, with
    `nonfinite`, +inf, -inf and NaN, three samples apart from N // 2 + its index on -- inside the span the whole chunks of a walk
    read -- where there is room.  A non-finite sample makes L outputs non-finite whatever the taps are, which at L = 2407 leaves
    whole blocks nothing but NaN == NaN to compare: the signals without them are what holds those blocks to values."""
    x = np.random.default_rng(seed).standard_normal((count, N)).astype(np.float32)
    x[0] *= np.float32(1e-20)
    x[-1] *= np.float32(1e20)
    for i in range(count):
        for j, v in enumerate((1.0e-41, -0.0, np.inf, -np.inf, np.nan)[:5 if nonfinite else 2]):
            at = N // 2 + i + 3 * j
            if at < N:
                x[i, at] = v
    return x


def compare_render(pvlib, s, h, x, route, gain, ctx):
    """both kernels' outputs of every receiver and their mix against ref.render of the responses h: (outputs, mix) as expected"""
    R, (L, N) = h.shape[0], (h.shape[1], x.shape[1])
    want_out, want_mix = ref.render(h, x, route, gain)
    for form in (pvlib.AURAL_TILED, pvlib.AURAL_PLAIN):
        s.set_aural_form(form)
        try:
            assert s.auralise(x, route, gain) > 0
            for r in range(R):
                got = s.aural_output(r)
                differ(got, want_out[r], "%s L=%d N=%d form=%d receiver %d" % (ctx, L, N, form, r))
                assert route[r] >= 0 or not got.any()
            differ(s.aural_mix(), want_mix, "%s L=%d N=%d form=%d mix" % (ctx, L, N, form))
        finally:
            s.set_aural_form(pvlib.AURAL_TILED)
    return want_out, want_mix


def render_walk(pvlib, s, h, N, ctx, must=(), absent=(), least=(0, 0), route=None, gain=None, x=None):
    """the responses h [R, L] the solver holds (already held to ref.resample) rendered with N-sample signals by both kernels,
    against ref.render.  Before anything is compared the walk of (L, N) is asserted: a block with each pattern of `must` as its
    WHOLE walk (or, for a pattern after 'in:', as a part of it), none of `absent` anywhere, at least least[0] whole chunks and
    least[1] of them in a row.  Without `x` there are two renders: first with finite signals, where EVERY block that has a whole
    chunk (the blocks of the `must` patterns among them) must have an expected output row of a routed receiver that is finite
    throughout and not all zero -- the block is held to values --, then with the signals that carry inf and NaN.
    Returns (outputs, mix, route) as expected of the last render."""
    B, C = pvlib.aural_shape()
    R, L = h.shape
    walks = ref.chunk_walk(L, N, B, C)
    n_whole, n_chunks, run = whole_chunks(walks)
    for pat in must:
        assert (any(pat[3:] in w for w in walks) if pat.startswith("in:") else pat in walks), (ctx, L, N, pat, walks)
    for pat in absent:
        assert not any(pat in w for w in walks), (ctx, L, N, pat, walks)
    assert n_whole >= least[0] and run >= least[1], (ctx, L, N, n_whole, n_chunks, run)
    route = np.array([ROUTE6[r % 6] for r in range(R)], np.int32) if route is None else np.asarray(route, np.int32)
    gain = np.array([GAIN6[r % 6] for r in range(R)], np.float32) if gain is None else np.asarray(gain, np.float32)
    if x is None:
        x = walk_signals(N, L * 4099 + N, nonfinite=False)
        assert np.isfinite(x).all() and (x == 0).sum() == 3 and (np.abs(x[x != 0]) < 1.2e-38).sum() == 3
        out, _ = compare_render(pvlib, s, h, x, route, gain, ctx + ", finite signals")
        for b, w in enumerate(walks):
            rows = out[route >= 0, b * B:(b + 1) * B]
            assert "W" not in w or (np.isfinite(rows).all(axis=1) & rows.any(axis=1)).any(), (ctx, L, N, b, w)
        x = walk_signals(N, L * 4099 + N)
    assert x.shape[1] == N and route.max() == x.shape[0] - 1 and route.min() == -1
    return compare_render(pvlib, s, h, x, route, gain, ctx) + (route,)


def respond(pvlib, s, p, pos, rate, Z, ctx, tables=True):
    """set, compute, and hold the responses at `pos` to ref.resample of their samples p [T, R]: (first, w, responses [R, L])"""
    s.set_auralisation(rate, Z, 9.0)
    first, w = library_tables(pvlib, s, rate, Z) if tables else s.aural_taps()
    assert s.compute_aural_responses(pos) > 0
    h = responses(s, len(pos))
    differ(h, ref.resample(p, first, w).T, ctx)
    return first, w, h


@pytest.fixture(scope="module")
def room6(pvlib):
    """one 70^2 run (T = 435): the solver, the planes and the six receivers of test_gpu_aural.test_convolution"""
    s, L = preset(pvlib)
    with s:
        assert (s.gx, s.T, s.fs) == (70, 435, 1443)
        s.run(L)
        hist, delay, beta = history(s), s.results()[1], s.material()[0]
        cells = pick_receivers(s, delay, beta)
        cells = [cells[i] for i in (0, 1, 2, 3, 5, len(cells) - 1)]
        yield {"s": s, "cells": cells, "pos": [cell_of(*c) for c in cells], "p": np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)}
        s.set_auralisation(0)


# 1. the whole-chunk path against the definition
#    N = 383 is the last without a whole chunk and 384 = B + C the first with one; 700 starts a block on two whole chunks and puts one
#    after a general one; 640 and 1000 at the long response put runs of three and five whole chunks AFTER general ones (accumulators
#    that hold sums, kBegin = m0 - N + 1 > 0) and end them on general ones; N = L = 2407 runs up to 16 in a row
WALKS = {(1000, 383): dict(absent=["W"]),
         (1000, 384): dict(must=["gWg"], least=(1, 1)),
         (1000, 700): dict(must=["WWg", "gWg"], least=(3, 2)),
         (8000, 640): dict(must=["ggWWWg", "gWWWgg"], least=(27, 3)),
         (8000, 1000): dict(must=["ggWWWWWggg"], least=(47, 5)),
         (8000, 2407): dict(must=["in:gg" + 16 * "W"], least=(150, 16))}


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("rate", [1000, 8000])
def test_whole_chunks(pvlib, room6, rate):
    s = room6["s"]
    _, _, h = respond(pvlib, s, room6["p"], room6["pos"], rate, 16, "rate %d" % rate, tables=False)
    assert h.shape == (6, {1000: 301, 8000: 2407}[rate])
    cases = [(N, w) for (r, N), w in WALKS.items() if r == rate]
    assert len(cases) == 3
    for N, w in cases:
        out, _, route = render_walk(pvlib, s, h, N, "rate %d" % rate, **w)
        for r in range(6):
            if route[r] < 0:
                assert not out[r].any()
            elif N >= 640:  # (the NaN at N // 2 + i + 12 reaches L outputs whatever the taps are; the outputs below N // 2 meet none)
                assert (~np.isfinite(out[r])).any() and np.isfinite(out[r]).any(), (N, r)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("want_l", [255, 256, 257])
def test_whole_chunk_at_the_end_of_the_response(pvlib, want_l):
    """the chunk k0 = 128 ends at tap 255: the response's last at L = 256 (whole), one past it at L = 255 (general), one short of
    it at L = 257 (whole, and a general chunk of one tap follows)"""
    B, C = pvlib.aural_shape()
    assert (B, C) == (256, 128)
    fs = pvlib.host_grid_info(25.0, 25.0, 275).fs
    steps = min(t for t in range(300, 435) if pvlib.host_aural_shape(fs, t, 1000)[0] == want_l)
    s, Lpos = preset(pvlib, num_steps=steps)
    with s:
        s.run(Lpos)
        assert (s.T, s.fs) == (steps, fs)
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 6).astype(int)]
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        _, _, h = respond(pvlib, s, p, [cell_of(*c) for c in cells], 1000, 16, "T=%d" % steps, tables=False)
        assert h.shape == (6, want_l)
        w = {255: dict(must=["Wg"], absent=["WW", "gW"], least=(2, 1)),
             256: dict(must=["WW", "gW"], least=(5, 2)),
             257: dict(must=["WWg", "gWg"], least=(5, 2))}[want_l]
        render_walk(pvlib, s, h, 1000, "T=%d" % steps, **w)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_no_term_beside_a_whole_chunk(pvlib):
    """A pair one sample past the signal, (m, k) with m - k = N, meets a staged zero: formed by mistake it adds h[k] * 0, which no
    finite response shows.  So the response gets non-finite taps that END at tap C = 128, the first tap of the chunk that is one
    pair short of whole at N = 383 (block m0 = 256: output 511 would meet tap 128 at x[383]): at the grid's own rate row n reads
    the steps n - 16 .. n + 16, and a single +inf at step 112 makes exactly the taps 96 .. 128 non-finite.  Output 511 sums the
    taps 129 .. L - 1 and is finite by the definition.  At N = 384 the same chunk is whole and tap 128 a term of it: every output
    of that block is non-finite then, so that half shows only that the inf reaches output 511 and no further (the whole chunks'
    VALUES are what the finite renders of the other cases hold)."""
    B, C = pvlib.aural_shape()
    assert (B, C) == (256, 128)
    s, Lpos = preset(pvlib, num_steps=300)
    with s:
        s.run(Lpos)
        hist = history(s)
        early = np.argwhere(adv.first_nonzero(hist)[:s.gx, :s.gy] <= C - 16 - 12)
        cell = tuple(int(v) for v in early[len(early) // 2])
        plane = s.history_plane(C - 16)
        plane[cell] = np.inf
        s.set_history_plane(C - 16, plane)
        p = hist[:, cell[0], cell[1]].copy()
        p[C - 16] = np.inf
        first, _, h = respond(pvlib, s, np.stack([p] * 3, axis=1), [cell_of(*cell)] * 3, s.fs, 16, "an inf at step %d" % (C - 16))
        assert h.shape == (3, 300) and np.array_equal(first, np.arange(300) - 16)
        assert np.array_equal(np.flatnonzero(~np.isfinite(h[0])), np.arange(C - 32, C + 1))
        for N, w in ((383, dict(absent=["W"])), (384, dict(must=["gWg"]))):
            x = np.random.default_rng(N).standard_normal((2, N)).astype(np.float32)
            out, _, _ = render_walk(pvlib, s, h, N, "inf taps to %d" % C, route=[0, 1, -1], gain=[1.0, -0.5, 2.0], x=x, **w)
            assert np.isfinite(out[:2, 2 * B - 1]).all() == (N == 383) and np.isfinite(out[:2, 2 * B]).all()
            assert not np.isfinite(out[:2, B]).any()


# 2. responses and convolution on histories the stencil never produces
def scene_preset(pvlib):
    s, L = preset(pvlib)
    return s, L, 435


def scene_offset_window(pvlib):
    """the scene of test_gpu_aural.test_window_smaller_than_the_grid at the offset listener"""
    size = open_size(N400)
    s = pvlib.Solver(size, size, 275, num_steps=160)
    s.load_scene(SMALLROOM)
    s.add_oriented_box(11.0, 9.0, 3.0, 0.6, 0.8, 0.6, 0.4)
    return s, L400["offset"], 160


def injected_cells(fam, reached):
    """one reached cell per family, the poisoned one chosen with a reached, finite (X - 1, Y) neighbour, and that neighbour"""
    cells = []
    for f in range(len(adv.FAMILIES)):
        at = np.argwhere((fam == f) & reached)
        if f == adv.NONFINITE:
            at = np.array([c for c in at if c[0] > 0 and reached[c[0] - 1, c[1]] and 0 <= fam[c[0] - 1, c[1]] < adv.NONFINITE])
        assert len(at), adv.FAMILIES[f]
        cells.append(tuple(int(v) for v in at[len(at) // 2]))
    return cells + [(cells[-1][0] - 1, cells[-1][1])]


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("scene", ["preset_T435", "offset_window"])
def test_injected_histories(pvlib, scene):
    s, listener, T = {"preset_T435": scene_preset, "offset_window": scene_offset_window}[scene](pvlib)
    with s:
        s.run(listener)
        assert s.T == T and s.fs == 1443
        new, fam, delay = adv.inject(s, SEED)
        reached = delay < adv.NO_ONSET
        cells = injected_cells(fam[:s.gx, :s.gy], reached)
        assert len(cells) == 12 and [int(fam[c]) for c in cells[:11]] == list(range(11))
        quiet, loud, poisoned, beside = (adv.FAMILIES.index("quiet"), adv.FAMILIES.index("loud"), adv.NONFINITE, 11)
        pos = [cell_of(*c) for c in cells]
        p = np.stack([new[:, c[0], c[1]] for c in cells], axis=1)
        assert np.isfinite(p[:, beside]).all() and not np.isfinite(p[:, poisoned]).all()
        for rate in (1443, 1000, 8000):
            _, _, h = respond(pvlib, s, p, pos, rate, 16, "%s rate %d" % (scene, rate), tables=False)
            assert np.abs(h[quiet])[h[quiet] != 0].min() < 1e-19 and np.abs(h[quiet]).max() > 0, rate  # (kept, not flushed)
            assert np.abs(h[loud]).max() > 1e19, rate
            assert not np.isfinite(h[poisoned]).all() and np.isfinite(h[beside]).all(), rate
        # (the last setting: rate 8000)
        assert h.shape[1] == pvlib.host_aural_shape(s.fs, T, 8000)[0] >= 384
        route = [ROUTE6[r % 6] for r in range(12)]
        route[loud] = 2
        assert route[quiet] == 0 and -1 in route and 1 in route
        out, _, _ = render_walk(pvlib, s, h, 1000, scene, must=["in:gW", "in:WW", "in:Wg"], least=(8, 2), route=route)
        # the last 200 outputs meet none of the signals' special samples: what is not finite or not normal there is the products'
        assert np.isinf(out[loud][-200:]).any()  # (1e19 x 1e20 overflows)
        tail = np.abs(out[quiet][-200:])
        assert np.isfinite(tail).all() and tail.max() > 0 and tail[tail != 0].min() < 1.2e-38  # (1e-19 x 1e-20: denormal, kept)
        if scene == "preset_T435":
            # nothing of the injection survives into the next run
            s.run(listener)
            s.compute_aural_responses(pos)
            f, _, _ = scene_preset(pvlib)
            with f:
                f.run(listener)
                f.set_auralisation(8000, 16, 9.0)
                f.compute_aural_responses(pos)
                differ(responses(s, len(pos)), responses(f, len(pos)), "the next run")


# 3. the resampler and the launch grid at the definition's limits
def test_resampler_many_zero_crossings(pvlib, room6):
    """rate 1000, Z = 64: K = 185 of T = 435 steps; the first rows start far below step 0, the last reach past T - 1"""
    s = room6["s"]
    assert pvlib.host_aural_shape(s.fs, s.T, 1000, 64) == (301, 185)
    first, w, _ = respond(pvlib, s, room6["p"], room6["pos"], 1000, 64, "Z=64")
    assert w.shape == (301, 185) and first[0] == -92 and first[-1] + 184 > s.T - 1 + 60


def test_resampler_few_taps_long_response(pvlib, room6):
    """rate 48 000, Z = 2: fs / rate = 0.03 steps per sample, K = 5, L = 14 437"""
    s = room6["s"]
    assert pvlib.host_aural_shape(s.fs, s.T, 48000, 2) == (14437, 5)
    first, w, h = respond(pvlib, s, room6["p"], room6["pos"], 48000, 2, "rate 48000 Z=2")
    assert w.shape == (14437, 5) and np.abs(h[0]).max() > 1e-3


def test_resampler_near_the_tap_limit(pvlib):
    """a 6 m x 6 m grid at a resolution that puts fs at 12 757: rate 1000 with Z = 40 takes K = 2 floor(40 fs / 1000) + 1 = 1021
    of the 1024 taps the definition allows, more than twice the run's 400 steps: every row reaches outside 0 .. T - 1 on both sides"""
    res, steps = 2430, 400
    info = pvlib.host_grid_info(6.0, 6.0, res)
    L, K = pvlib.host_aural_shape(info.fs, steps, 1000, 40)
    assert info.fs > 12000 and (L, K) == (int((steps - 1) * 1000 / info.fs) + 1, 2 * int(40 * info.fs / 1000) + 1)
    assert 900 <= K <= pvlib.AURAL_MAX_TAPS and K == 1021
    with pvlib.Solver(6.0, 6.0, res, num_steps=steps) as s:
        s.run((3.0, 0.0, 3.0))
        assert (s.T, s.fs) == (steps, info.fs)
        hist, delay = history(s), s.results()[1]
        reached = np.argwhere(delay < NO_ONSET)
        cells = [tuple(int(v) for v in reached[i]) for i in np.linspace(0, len(reached) - 1, 6).astype(int)]
        dx = float(s.info.dx)
        pos = [((c[0] + 0.5) * dx, 0.0, (c[1] + 0.5) * dx) for c in cells]
        assert [pvlib.host_cells(6.0, 6.0, res, q[0], q[2])[1] for q in pos] == cells
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        first, w, h = respond(pvlib, s, p, pos, 1000, 40, "K=%d" % K)
        assert w.shape == (L, K) and first[0] < 0 and (first + K - 1 > steps - 1).all() and np.abs(h).max() > 0


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_most_receivers_and_signals(pvlib, room6):
    """R = 256 receivers and S = 64 signals, the most PvAmdAuralise accepts, with every signal and a -1 routed"""
    R, S, N = pvlib.AURAL_MAX_RECEIVERS, pvlib.AURAL_MAX_SIGNALS, 400
    assert (R, S) == (256, 64)
    distinct = list(dict.fromkeys(room6["cells"]))
    cells = [distinct[r % len(distinct)] for r in range(R)]
    s, Lpos = preset(pvlib, num_steps=100)
    with s:
        s.run(Lpos)
        hist = history(s)
        p = np.stack([hist[:, c[0], c[1]] for c in cells], axis=1)
        _, _, h = respond(pvlib, s, p, [cell_of(*c) for c in cells], 1000, 16, "R=256", tables=False)
        assert h.shape == (R, 69) and np.abs(h).max() > 0
        rng = np.random.default_rng(SEED)
        route = np.array([r % (S + 1) - 1 for r in range(R)], np.int32)
        assert set(route) == set(range(-1, S))
        gain = rng.uniform(-2.0, 2.0, R).astype(np.float32)
        x = walk_signals(N, SEED, S)
        out, mix, _ = render_walk(pvlib, s, h, N, "R=256 S=64", absent=["W"], route=route, gain=gain, x=x)
        assert out.shape == (R, N + 68) and not out[route < 0].any() and np.isfinite(mix).any()
