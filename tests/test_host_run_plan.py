"""pva::planRun (csrc/pv_core.h: which path a run takes) against a restatement of the predicates it replaced.

Every path gives the same bits, so a run on the wrong path fails no parity test; this is the check.  tests/host/enum_plans.cpp
evaluates planRun over the product of its inputs' values (every field takes each value a rule can tell apart, impossible
combinations included: nothing is excluded by hand) and `parent_plan` below restates, in numpy, what commit 78b3afc decided in
csrc/pv_solver.cpp -- written from that commit's code, line ranges quoted, not from planRun.

The product has 2^23 * 3^5 = 2 038 431 744 combinations; all of them are compared (a few minutes).
"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "planeverb_amd", "csrc")
PATHS = ["Streaming", "Window", "Resident", "SmallGrid", "Graph", "Launches"]
STREAMING, WINDOW, RESIDENT, SMALLGRID, GRAPH, LAUNCHES = range(6)
RUN, RAW, SHARED = 0, 1, 2  # PathRun::Kind


@pytest.fixture(scope="module")
def enum_plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_plan") / "enum_plans")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "enum_plans.cpp"), os.path.join(CSRC, "pv_core.cpp"), "-o", exe])
    return exe


def fields(exe):
    out = subprocess.run([exe, "fields"], capture_output=True, text=True, check=True).stdout
    return [(l.split()[0], [int(v) for v in l.split()[1:]]) for l in out.splitlines()]


def parent_plan(v):
    """The decisions of commit 78b3afc (csrc/pv_solver.cpp), for a dict of equally shaped integer arrays named as PathCaps /
    PathRun.  Returns the plan's fields as arrays."""
    b = lambda name: v[name] != 0
    run, raw = v["kind"] == RUN, v["kind"] == RAW
    stacked, merged_ok, layer_active, layer_tiles = b("stacked"), b("mergedOk"), b("layerActive"), b("layerTiles")
    streaming, tk = b("streaming"), v["timeKernels"] != 0
    # init :483 = :500, reachEligible :1518 -- "the plain merged path"
    plain_merged = ~stacked & (v["merged"] == 1) & merged_ok
    # enqueueSteps :1679-1680 -- "the sweep is one launch"
    one_launch = stacked | (((v["merged"] == 1) | layer_tiles) & merged_ok)
    # enqueueRun :2053-2054
    graph = ~tk & ~streaming & ((v["useGraph"] == 1) | ((v["useGraph"] == 0) & (v["ntiles"] <= 4096)))
    # prepareDyn :1273, called with banded = !graph by enqueueRun :2055, true by runSteps :2613, false by runBatch :2387,
    # SlabGroup::run (pv_slabs.cpp :352) and SlabRankOps::begin (:655)
    banded_arg = np.where(run, ~graph, raw)
    banded = banded_arg & (v["bands"] > 1) & ~layer_active
    # prepareDyn :1318-1321
    segments = b("useSeg") & ~banded & ~layer_active & b("segmentsFound")
    # enqueueRun :2071-2074
    small_wanted = (v["smallGrid"] == 1) | ((v["smallGrid"] == 0) & (v["cells"] <= 1536))
    small = (small_wanted & ~b("explicitTile") & ~tk & (v["useGraph"] != 1) & ~streaming & b("smallFits") & b("wholeWindow") &
             ~layer_active)
    # reachEligible :1517-1522 (called at enqueueRun :2076; reachRun_ stays false in runSteps, runBatch and the slab heads)
    reach = (run & (v["reachBound"] != 0) & plain_merged & ~graph & ~small & ~b("useResident") & ~streaming & ~banded & ~segments &
             ~b("usePatch") & ~b("denseHistory") & ~b("edgeTiles") & ~b("slab") & ~tk & b("listenerInside"))
    # enqueueRun :2160, :2163 with windowFor :1545 (x0_ != 0 only on slabs, which reachEligible has refused)
    resident = b("useResident") & ~(small & (v["resident"] != 1)) & ~layer_active
    window = reach & b("windowOk") & ~b("windowOff") & ~layer_active
    # enqueueRun: streaming :2082, window :2176, resident :2180, small :2229, graph :2254, launches :2274
    tiles = np.where(graph, GRAPH, LAUNCHES)
    path = np.where(streaming, STREAMING, np.where(window, WINDOW, np.where(resident, RESIDENT, np.where(small, SMALLGRID, tiles))))
    path = np.where(run, path, LAUNCHES)
    # what a run goes out as when windowFor says no (:2163 -> :2274), the resident budget is used up (:2167-2169 -> :2229 / :2254 /
    # :2274) or the capture is lost (:2261-2268)
    fallback = np.where(path == RESIDENT, np.where(small, SMALLGRID, tiles), np.where((path == WINDOW) | (path == GRAPH), LAUNCHES, path))
    return dict(path=path, fallback=fallback, oneLaunch=one_launch, plainMerged=plain_merged, banded=banded, segments=segments,
                patch=b("usePatch") & ~layer_tiles,  # enqueueSteps :1784
                reach=reach, layer=layer_tiles)  # enqueueSteps :1734 (reachRun_), :1792


def code(p):
    c = np.asarray(p["path"], dtype=np.uint16) | np.asarray(p["fallback"], dtype=np.uint16) << 3
    for k, name in enumerate(["oneLaunch", "plainMerged", "banded", "segments", "patch", "reach", "layer"]):
        c = c | np.asarray(p[name], dtype=np.uint16) << (6 + k)
    return c


def test_every_combination_plans_as_the_parent_commit_did(enum_plans):
    """all 2 038 431 744 combinations, in index order: the program streams its plans, the restatement is evaluated block by block
    (a block = every value of the first INNER fields, whose arrays are made once; the other fields are constant within a block)"""
    fl = fields(enum_plans)
    total = int(np.prod([len(vals) for _, vals in fl], dtype=np.int64))
    assert total == 2 ** 23 * 3 ** 5
    INNER = 20
    block = int(np.prod([len(vals) for _, vals in fl[:INNER]]))
    inner, d = {}, np.arange(block, dtype=np.int64)
    for name, vals in fl[:INNER]:
        inner[name] = np.asarray(vals, dtype=np.int32)[d % len(vals)]
        d //= len(vals)
    proc = subprocess.Popen([enum_plans, "all"], stdout=subprocess.PIPE)
    try:
        for hi in range(total // block):
            v, d = dict(inner), hi
            for name, vals in fl[INNER:]:
                v[name] = np.int32(vals[d % len(vals)])
                d //= len(vals)
            raw = proc.stdout.read(2 * block)
            assert len(raw) == 2 * block, "the program's output ends at block %d" % hi
            got = np.frombuffer(raw, dtype="<u2")
            bad = np.nonzero(code(parent_plan(v)) != got)[0]
            if bad.size:
                i = int(bad[0])
                args = ["%s=%d" % (name, np.broadcast_to(v[name], (block,))[i]) for name, _ in fl]
                mine = subprocess.run([enum_plans, "plan"] + args, capture_output=True, text=True).stdout
                want = {k: int(np.broadcast_to(a, (block,))[i]) for k, a in parent_plan(v).items()}
                raise AssertionError("block %d: %d plans differ; first: %s -> %s, the parent commit: %s" % (hi, bad.size, args, mine, want))
        assert proc.stdout.read(2) == b"" and proc.wait() == 0
    finally:
        proc.kill()


def plan(exe, **kw):
    out = subprocess.run([exe, "plan"] + ["%s=%d" % kv for kv in kw.items()], capture_output=True, text=True, check=True).stdout.split()
    p = dict(path=out[0], fallback=out[1].split("=")[1])
    p.update({k: int(x) for k, x in (f.split("=") for f in out[2:])})
    return p


# what Solver::init resolves for the default options on ...
LARGE = dict(mergedOk=1, ntiles=11742, cells=4097 * 4097, windowOk=1)                      # 4096^2: tile (12, 36), windowed history
PRESET70 = dict(mergedOk=1, ntiles=12, cells=71 * 71, wholeWindow=1, useResident=1, smallFits=1)  # the Sandbox's 70^2: tile (12, 12)
PRESET28 = dict(mergedOk=1, ntiles=3, cells=29 * 29, wholeWindow=1, useResident=1, smallFits=1)
# ... and for steps_per_launch=12, tile_rows=36, use_graph=2 on a 252 x 280 grid (253 x 281 array cells, 8 x 8 tiles): the explicit
# tile keeps the whole-grid resident kernel and the small-grid kernel away, "no graph" leaves the reach-bounded launches, and the
# (12, 36) tile is the window's -- how tests/test_gpu_resident_window_small.py reaches the window path on grids the oracle can run
FORCED_252x280 = dict(mergedOk=1, ntiles=64, cells=253 * 281, wholeWindow=1, explicitTile=1, useGraph=2, windowOk=1)


def test_named_cases(enum_plans):
    # HugeRoom at 4096^2: planned for the resident window; its listener is not walled in (Solver::windowFor), so the run goes out as
    # the fallback -- reach-bounded launches; with the window off it is planned as such
    p = plan(enum_plans, listenerInside=1, **LARGE)
    assert (p["path"], p["fallback"], p["reach"], p["oneLaunch"], p["banded"]) == ("Window", "Launches", 1, 1, 0)
    for off in (dict(windowOff=1), dict(windowOk=0)):
        p = plan(enum_plans, listenerInside=1, **{**LARGE, **off})
        assert (p["path"], p["reach"]) == ("Launches", 1)
    p = plan(enum_plans, listenerInside=1, useGraph=1, **LARGE)
    assert (p["path"], p["fallback"], p["reach"]) == ("Graph", "Launches", 0)
    p = plan(enum_plans, listenerInside=1, **PRESET70)
    assert (p["path"], p["fallback"], p["reach"]) == ("Resident", "Graph", 0)
    p = plan(enum_plans, listenerInside=1, **PRESET28)
    assert (p["path"], p["reach"]) == ("SmallGrid", 0)
    assert plan(enum_plans, listenerInside=1, resident=1, **PRESET28)["path"] == "Resident"
    # the forced (12, 36) tile without a graph on a small grid: the window path; with the automatic graph (64 tiles): the graph
    p = plan(enum_plans, listenerInside=1, **FORCED_252x280)
    assert (p["path"], p["fallback"], p["reach"]) == ("Window", "Launches", 1)
    p = plan(enum_plans, listenerInside=1, **dict(FORCED_252x280, useGraph=0))
    assert (p["path"], p["reach"]) == ("Graph", 0)
    assert plan(enum_plans, listenerInside=0, **FORCED_252x280)["path"] == "Launches"  # (a listener outside the grid)
    # any layer: the tile kernels (replayed from a graph where the grid is small), merged launch + layer launch, no bands
    for base in (LARGE, PRESET70, PRESET28, dict(LARGE, bands=4, useGraph=2), dict(LARGE, useSeg=1, useGraph=2)):
        p = plan(enum_plans, listenerInside=1, layerActive=1, layerTiles=1, **base)
        assert p["path"] == ("Graph" if base["ntiles"] <= 4096 and "useGraph" not in base else "Launches")
        assert (p["oneLaunch"], p["layer"], p["banded"], p["segments"]) == (1, 1, 0, 0)
    # a slab: its group drives plain launches of full sweeps
    p = plan(enum_plans, kind=SHARED, slab=1, useGraph=2, smallGrid=2, listenerInside=1, **LARGE)
    assert (p["path"], p["reach"], p["banded"], p["oneLaunch"]) == ("Launches", 0, 0, 1)
    # segments asked for on a banded solver: the bands win
    p = plan(enum_plans, listenerInside=1, useSeg=1, bands=4, useGraph=2, **LARGE)
    assert (p["path"], p["banded"], p["segments"], p["reach"]) == ("Launches", 1, 0, 0)
    p = plan(enum_plans, listenerInside=1, useSeg=1, useGraph=2, **LARGE)
    assert (p["banded"], p["segments"], p["reach"]) == (0, 1, 0)
