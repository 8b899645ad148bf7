"""GPU: what the in-run zone maps of sparse-emitter mode cost (PvAmdSetZoneMaps): the runs that
profiles/stream_zone_maps.txt quotes.

HugeRoom 25 m in a 4096^2 grid (T = 25 432) in sparse-emitter mode, no emitters.

    python tools/gpu_stream_zone_maps_measure.py --wall off|rm|spec|both|rm_whole
        one process: 2 warm-up runs, then 7 timed runs (host clock around run(), which waits for the run); one JSON line with the
        median, the smallest and the largest, the tiles that hold a labelled cell and how many of them would otherwise be fused
        (the host estimate of tools/gpu_stream_zone_decay_measure.py).  off: no zones, nothing selected; rm: the room metrics over
        one zone of 5 m x 5 m; spec: the spectrum with 3 bins over the same zone; both: both kinds; rm_whole: the room metrics with
        the whole grid as one zone.  PLANEVERB_AMD_LIB names another build of the library (an older one, which lacks the selector,
        can run `off`).
    python tools/gpu_stream_zone_maps_measure.py --trace rm|spec|both|rm_whole
        one process, meant to run under `rocprofv3 --kernel-trace`: a warm-up run, then one run.
    python tools/gpu_stream_zone_maps_measure.py --parse TRACE.csv
        the kernel trace of --trace: the device time of the accumulate kernels per pass and of the finish kernel.
"""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gpu_stream_zone_decay_measure as zd  # noqa: E402  (the scene, the listener, the zones and the tile estimate)

SIZE, RES, SCENE, L = zd.SIZE, zd.RES, zd.SCENE, zd.L
BINS = [50.0, 100.0, 200.0]
CASES = {"off": ("off", 0), "rm": ("one", 1), "spec": ("one", 2), "both": ("one", 3), "rm_whole": ("whole", 1)}  # (zones of zd.ZONES, kinds)
KERNELS = ("pv_zone_maps_room_kernel", "pv_zone_maps_spec_kernel", "pv_zone_maps_finish_kernel", "pv_stream_accum_kernel")


def make(api, config):
    zones, kinds = CASES[config]
    s = api.Solver(SIZE, SIZE, RES, streaming_analysis=1)
    s.load_scene(SCENE)
    assert (s.gx, s.T) == (4096, 25432), (s.gx, s.T)
    tiles, labels = (0, 0), None
    if kinds:
        labels = api.zone_labels_from_rects(s.dx, s.gx, s.gy, zd.ZONES[zones])
        s.set_zones(labels, len(zd.ZONES[zones]))
        if kinds & api.ZMAP_SPECTRUM:
            s.set_spectrum_bins(BINS)
        s.set_zone_maps(kinds)
        tiles = zd.tiles_of(api, s, labels)
    return s, tiles, kinds


def wall(config, runs=7, warm=2):
    api = zd.load_api()
    s, tiles, kinds = make(api, config)
    with s:
        ms = []
        for _ in range(warm + runs):
            t0 = time.perf_counter()
            s.run(L)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[warm:]
        out = dict(config=config, lib="another build" if os.environ.get("PLANEVERB_AMD_LIB") else "this tree's build", grid=[s.gx, s.gy], T=s.T,
                   kinds=kinds, bins=len(BINS) if kinds & 2 else 0, zone_tiles=tiles[0], zone_tiles_otherwise_fused=tiles[1],
                   tiles=-(-(s.gx + 1) // s.info.tileRows) * -(-(s.gy + 1) // s.info.tileCols), run_ms_median=round(float(np.median(ms)), 2),
                   run_ms_min=round(min(ms), 2), run_ms_max=round(max(ms), 2), runs=runs)
        if kinds & 1:
            z, zms = s.zone_stats("room_metrics", with_ms=True)
            out.update(cells_with_onset=int(z["n_finite"][0, 8]), mean_c50=round(float(z["mean"][0, 0]), 3), mean_ts_ms=round(1e3 * float(z["mean"][0, 3]), 2),
                       zone_stats_ms=round(zms, 3))
        if kinds & 2:
            z = s.zone_stats("spectrum")
            out.update(mean_level_db=[round(float(v), 2) for v in z["mean"][0, :, 2]])
        print(json.dumps(out))


def trace(config):
    api = zd.load_api()
    s, _, _ = make(api, config)
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
            print("%-30s %5d launches in the run, median %9.1f us, largest %9.1f us, sum %10.0f us" % (
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
