"""CPU: what a sparse-emitter run derives from the zones' labels for the in-run zone curves (PvAmdSetZoneCurves): the tiles that must
stay in the ring, the launch box, the union with the emitters' tiles and the chunking of an accumulate pass's steps -- the host
functions of csrc/pv_zone_decay.h through their PvAmdHost* exports, against an independent numpy restatement; the new exports and
their guards; and the edge cases in a stand-alone program under ASan + UBSan (nothing is loaded into Python under a sanitizer)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NAMES = ["PvAmdSetZoneCurves", "PvAmdGetZoneCurves"]
HOST_NAMES = ["PvAmdHostZoneTiles", "PvAmdHostZoneTileUnion", "PvAmdHostZoneCurveChunk"]
# (gx, gy, tile rows, tile columns): the tile forms of the GPU tests -- 12 x 40 and 24 x 48 at 70^2, 12 x 36 and 24 x 48 on the
# non-square grids in both orientations -- and grids below one tile and one block
SHAPES = [(70, 70, 12, 40), (70, 70, 24, 48), (252, 280, 12, 36), (280, 252, 12, 36), (252, 280, 24, 48), (280, 252, 24, 48),
          (254, 254, 24, 48), (5, 3, 12, 40), (64, 64, 8, 24), (65, 129, 8, 24)]
SCRATCH = 32 << 20


def tiles_ref(lab, rxi, wi):
    """the same answer from the label map's own index sets"""
    gx, gy = lab.shape
    ntx, nty = -(-gx // rxi), -(-gy // wi)
    X, Y = np.nonzero(lab)
    flags = np.zeros((ntx, nty), np.uint8)
    flags[X // rxi, Y // wi] = 1
    box = (int(X.min()), int(X.max()), int(Y.min()) // 64, int(Y.max()) // 64) if len(X) else (0, -1, 0, -1)
    return flags, box


def check(pvlib, lab, rxi, wi, ctx):
    flags, box = pvlib.host_zone_tiles(lab, rxi, wi)
    wflags, wbox = tiles_ref(lab, rxi, wi)
    assert flags.shape == wflags.shape and np.array_equal(flags, wflags), ctx
    assert box == wbox, (ctx, box, wbox)
    return flags, box


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dx%d" % s)
def test_tiles_and_box(pvlib, shape):
    gx, gy, rxi, wi = shape
    rng = np.random.default_rng(gx * 1000 + gy + rxi)
    # empty labels
    flags, box = check(pvlib, np.zeros((gx, gy), np.uint8), rxi, wi, "empty")
    assert not flags.any() and box == (0, -1, 0, -1)
    # random labels, dense and sparse
    check(pvlib, rng.integers(0, 6, (gx, gy)).astype(np.uint8), rxi, wi, "dense")
    for k in range(4):
        lab = np.zeros((gx, gy), np.uint8)
        n = int(rng.integers(1, 6))
        lab[rng.integers(0, gx, n), rng.integers(0, gy, n)] = rng.integers(1, 65, n)
        check(pvlib, lab, rxi, wi, "sparse %d" % k)
    # labels confined to one tile: exactly that tile
    ntx, nty = -(-gx // rxi), -(-gy // wi)
    for ti, tj in {(0, 0), (ntx - 1, nty - 1), (ntx // 2, nty // 2)}:
        lab = np.zeros((gx, gy), np.uint8)
        lab[ti * rxi:(ti + 1) * rxi, tj * wi:(tj + 1) * wi] = 3
        flags, box = check(pvlib, lab, rxi, wi, "tile %d %d" % (ti, tj))
        assert flags.sum() == 1 and flags[ti, tj] == 1
        assert box[:2] == (ti * rxi, min((ti + 1) * rxi, gx) - 1)
    # labels on tile edges and on the edges of the 64-blocks: one cell either side of each boundary
    for X in sorted({0, gx - 1} | {x for t in range(1, ntx) for x in (t * rxi - 1, t * rxi)}):
        for Y in sorted({0, gy - 1} | {y for t in range(1, nty) for y in (t * wi - 1, t * wi)} |
                        {y for b in range(64, gy, 64) for y in (b - 1, b)}):
            lab = np.zeros((gx, gy), np.uint8)
            lab[X, Y] = 1
            flags, box = check(pvlib, lab, rxi, wi, (X, Y))
            assert flags.sum() == 1 and flags[X // rxi, Y // wi] == 1 and box == (X, X, Y // 64, Y // 64)
    # a band along a block edge: the box takes both blocks, the alignment at Y = 0 stays
    if gy > 64:
        lab = np.zeros((gx, gy), np.uint8)
        lab[gx // 3:gx // 2 + 1, 63:65] = 2
        assert check(pvlib, lab, rxi, wi, "block edge")[1] == (gx // 3, gx // 2, 0, 1)


def test_union_rule(pvlib):
    rng = np.random.default_rng(5)
    for n in (1, 6, 77):
        em, zn = (rng.integers(0, 2, n).astype(np.uint8) for _ in range(2))
        em[rng.integers(0, n)] = 200  # (any non-zero byte counts)
        assert np.array_equal(pvlib.host_zone_tile_union(em, zn, n), ((em != 0) | (zn != 0)).astype(np.uint8))
        assert np.array_equal(pvlib.host_zone_tile_union(em, None, n), (em != 0).astype(np.uint8))   # the zones cleared
        assert np.array_equal(pvlib.host_zone_tile_union(None, zn, n), (zn != 0).astype(np.uint8))   # the emitters cleared
        assert not pvlib.host_zone_tile_union(None, None, n).any()
    assert pvlib.host_zone_tile_union(None, None, 0).shape == (0,)
    # emitter tiles as Solver.set_emitters derives them united with the zones' tiles of host_zone_tiles: nothing of either is lost
    gx, gy, rxi, wi = 252, 280, 24, 48
    lab = np.zeros((gx, gy), np.uint8)
    lab[60:130, 50:170] = 1
    zn = pvlib.host_zone_tiles(lab, rxi, wi)[0]
    em = np.zeros_like(zn)
    for X, Y in ((0, 0), (251, 279), (100, 100)):
        em[X // rxi, Y // wi] = 1
    u = pvlib.host_zone_tile_union(em, zn, zn.size).reshape(zn.shape)
    assert (u[em == 1] == 1).all() and (u[zn == 1] == 1).all() and u.sum() == ((em | zn) != 0).sum() and u.sum() > zn.sum()


def test_chunks_are_whole_groups_within_the_scratch(pvlib):
    for nz in (1, 2, 5, 64):
        for rows in (1, 23, 70, 252, 820, 4096, 5000):
            c = pvlib.host_zone_curve_chunk(nz, rows, SCRATCH)
            assert c % 16 == 0 and 16 <= c <= 32768, (nz, rows, c)
            assert c * nz * rows * 8 <= SCRATCH or c == 16, (nz, rows, c)
            if c < 32768:
                assert (c + 16) * nz * rows * 8 > SCRATCH, (nz, rows, c)  # (the largest such chunk)
            # an accumulate pass of n steps is dealt in ceil(n / c) chunks: all but the last are whole groups
            for n in (96, 51, 64, 128, 3):
                parts = [min(c, n - t) for t in range(0, n, c)]
                assert sum(parts) == n and all(p % 16 == 0 for p in parts[:-1])
    assert pvlib.host_zone_curve_chunk(64, 4096, SCRATCH) == 16   # exactly the bound
    assert pvlib.host_zone_curve_chunk(64, 8192, SCRATCH) == 16   # one group is more than the bound: one group all the same
    assert pvlib.host_zone_curve_chunk(5, 820, SCRATCH) == SCRATCH // (5 * 820 * 8) // 16 * 16
    for bad in ((0, 1, SCRATCH), (65, 1, SCRATCH), (1, 0, SCRATCH), (1, 1, -1)):
        with pytest.raises(pvlib.PlaneverbError, match="^zone curves: PvAmdHostZoneCurveChunk"):
            pvlib.host_zone_curve_chunk(*bad)


def test_exports_exist_and_are_guarded(pvlib):
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    L = C.CDLL(pvlib.LIB_PATH)
    for n in NAMES + HOST_NAMES:
        assert re.search(r"^PVA_EXPORT int %s\(" % n, hdr, re.M), n
        assert hasattr(L, n) and n in pvlib.SYMBOLS, n
        m = re.search(r"^int %s\([^)]*\) try \{(.*?)^\} PV_API_CATCH\(-1\)$" % n, src, re.M | re.S)
        assert m, n
        assert "\n}" not in m.group(1), n  # (the guard that closes it is its own)
    for n in NAMES:
        assert re.search(r"^PVA_EXPORT int %s\(PvAmdSolver\* s[,)]" % n, hdr, re.M), n
    for m in ("set_zone_curves", "zone_curves"):
        assert callable(getattr(pvlib.Solver, m)), m
    lib = pvlib.lib()
    on = C.c_int(7)
    assert lib.PvAmdSetZoneCurves(None, 1) == -1 and pvlib.last_error() == "zone curves: null solver handle"
    assert lib.PvAmdGetZoneCurves(None, C.byref(on)) == -1 and pvlib.last_error() == "zone curves: null solver handle"
    assert on.value == 7
    box = (C.c_int * 4)()
    assert lib.PvAmdHostZoneTiles(None, 4, 4, 2, 2, None, box) == -1 and pvlib.last_error().startswith("zone curves: PvAmdHostZoneTiles")
    assert lib.PvAmdHostZoneTileUnion(None, None, 3, None) == -1 and pvlib.last_error().startswith("zone curves: PvAmdHostZoneTileUnion")


def test_edge_cases_under_sanitizers(tmp_path):
    """tests/host/stream_zone_tiles_edges.cpp includes csrc/pv_zone_decay.h and runs the edge cases with exactly sized arrays"""
    host, csrc = os.path.join(ROOT, "tests", "host"), os.path.join(ROOT, "planeverb_amd", "csrc")
    exe = str(tmp_path / "stream_zone_tiles_edges")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", csrc, "-Wall",
                           "-Wno-unused-function", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(host, "stream_zone_tiles_edges.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "stream_zone_tiles_edges: 0 failure(s)" in r.stdout, r.stdout
