"""GPU: what the in-run zone curves of sparse-emitter mode cost (PvAmdSetZoneCurves): the runs that
profiles/stream_zone_decay.txt quotes.

HugeRoom 25 m in a 4096^2 grid (T = 25 432) in sparse-emitter mode, no emitters.

    python tools/gpu_stream_zone_decay_measure.py --wall off|one|five|whole
        one process: 2 warm-up runs, then 7 timed runs (host clock around run(), which waits for the run); one JSON line with the
        median, the smallest and the largest, the tiles that hold a labelled cell and how many of them would otherwise be fused
        (a host estimate from the material map: the tile's loaded region is all air, away from the grid's edge and from the
        listener).  off: no zones, curves disabled; one: one zone of 5 m x 5 m; five: five zones; whole: the whole grid as one
        zone.  PLANEVERB_AMD_LIB names another build of the library (an older one, which lacks the curves, can run `off`).
    python tools/gpu_stream_zone_decay_measure.py --trace one|five|whole
        one process, meant to run under `rocprofv3 --kernel-trace`: a warm-up run, then one run.
    python tools/gpu_stream_zone_decay_measure.py --parse TRACE.csv
        the kernel trace of --trace: the device time of the curve kernel and of the merge kernel per accumulate pass.
"""
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, RES = 25.0, 16067  # 25 m in 4096^2 cells: T = 25 432
SCENE = os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv")
L = (5.0, 0.0, 4.0)
ZONES = {"off": [],
         "one": [(8.0, 8.0, 13.0, 13.0)],
         "five": [(8.0, 8.0, 13.0, 13.0), (1.0, 1.0, 4.0, 7.0), (15.0, 2.0, 23.0, 6.0), (2.0, 16.0, 9.0, 23.0), (16.0, 15.0, 22.0, 22.0)],
         "whole": [(0.0, 0.0, 26.0, 26.0)]}
KERNELS = ("pv_zone_curve_rows_kernel", "pv_zone_curve_merge_kernel", "pv_stream_accum_kernel")


def load_api():
    from planeverb_amd import api
    have = ctypes.CDLL(api.LIB_PATH)
    for n in [n for n in api.SYMBOLS if not hasattr(have, n)]:  # (an older build: bind what it exports)
        del api.SYMBOLS[n]
    return api


def tiles_of(api, s, labels):
    """(tiles that hold a labelled cell, those of them whose loaded region is all air, off the grid's edge and the listener)"""
    rxi, wi, K = s.info.tileRows, s.info.tileCols, s.info.stepsPerLaunch
    flags = api.host_zone_tiles(labels, rxi, wi)[0]
    wall = s.material()[0] == 0
    lx, ly = int(L[0] / s.dx), int(L[2] / s.dx)
    fused = 0
    for ti, tj in np.argwhere(flags):
        r0, r1, c0, c1 = ti * rxi - K, (ti + 1) * rxi + K, tj * wi - K, (tj + 1) * wi + K
        if r0 < 0 or c0 < 0 or r1 > s.gx or c1 > s.gy or wall[r0:r1, c0:c1].any() or (r0 <= lx < r1 and c0 <= ly < c1):
            continue
        fused += 1
    return int(flags.sum()), fused


def make(api, config):
    s = api.Solver(SIZE, SIZE, RES, streaming_analysis=1)
    s.load_scene(SCENE)
    assert (s.gx, s.T) == (4096, 25432), (s.gx, s.T)
    tiles = (0, 0)
    if ZONES[config]:
        labels = api.zone_labels_from_rects(s.dx, s.gx, s.gy, ZONES[config])
        s.set_zones(labels, len(ZONES[config]))
        s.set_zone_curves(True)
        tiles = tiles_of(api, s, labels)
    return s, tiles


def wall(config, runs=7, warm=2):
    api = load_api()
    s, tiles = make(api, config)
    with s:
        ms = []
        for _ in range(warm + runs):
            t0 = time.perf_counter()
            s.run(L)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[warm:]
        out = dict(config=config, lib="another build" if os.environ.get("PLANEVERB_AMD_LIB") else "this tree's build", grid=[s.gx, s.gy], T=s.T,
                   zones=len(ZONES[config]), zone_tiles=tiles[0], zone_tiles_otherwise_fused=tiles[1],
                   tiles=-(-(s.gx + 1) // s.info.tileRows) * -(-(s.gy + 1) // s.info.tileCols), run_ms_median=round(float(np.median(ms)), 2),
                   run_ms_min=round(min(ms), 2), run_ms_max=round(max(ms), 2), runs=runs)
        if ZONES[config]:
            rec, members_ms = s.zone_decay("absolute", with_ms=True)
            out.update(cells=[int(n) for n in rec["n_cells"]], t30=[round(float(v), 4) for v in rec["t30"]], members_pass_ms=round(members_ms, 3))
        print(json.dumps(out))


def trace(config):
    api = load_api()
    s, _ = make(api, config)
    with s:
        s.run(L)
        s.run(L)
        print(json.dumps(dict(config=config, traced_runs=2, T=s.T)))


def parse(path):
    per = dict((k, []) for k in KERNELS)
    with open(path) as f:
        for r in csv.DictReader(f):
            k = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
            if k:
                per[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k in KERNELS:
        us = per[k][len(per[k]) // 2:]  # (the second run of the two)
        if us:
            print("%-34s %5d launches in the run, median %9.1f us, largest %9.1f us, sum %10.0f us" % (
                k, len(us), float(np.median(us)), max(us), sum(us)))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--wall":
        wall(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "--trace":
        trace(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        sys.exit(__doc__)
