"""GPU: first measurements of the room-metrics pass (PvAmdComputeRoomMetrics, csrc/pv_metrics.hip) -> profiles/room_metrics.txt.

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups), the same run's analysisMs, the
history bytes the reached cells span (sum over the cells with an onset of (T - onset) x 4 bytes: what the definition reads;
the pass fetches whole 256-byte lines of the 64-cell groups that hold them, so this is a lower bound of its traffic) and those
bytes per second against PvAmdBandwidthProbe's read rate, taken in the same process.

Grids: SmallRoomScene at the 70^2, 127^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench
scene, HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_room_metrics_measure.py [out.txt]        every grid, one child process each under its own time limit;
                                                              stops at the first that fails
    python tools/gpu_room_metrics_measure.py --one NAME       one grid, one JSON line (also what a kernel trace wraps:
        rocprofv3 --kernel-trace --stats -d DIR -- python tools/gpu_room_metrics_measure.py --one shoebox512
        gives pv_room_metrics_kernel beside pv_rt60_tile_kernel / pv_rt60_groups_kernel on the same history)
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
SCENES = os.path.join(ROOT, "tests", "scenes")
L = (5.0, 0.0, 4.0)
# name: (scene, size in metres, resolution, options, time limit of the child in seconds)
GRIDS = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, {}, 120),
    "smallroom127": ("SmallRoomScene.pv", 25.0, 500, {}, 120),
    "smallroom254": ("SmallRoomScene.pv", 25.0, 1000, {}, 120),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, {}, 240),
    "hugeroom4096": ("HugeRoom.pv", float((4096 + 0.5) * DX), 275, {}, 240),
}


def one(name, runs=20, warm=3):
    from planeverb_amd import api
    scene, size, res, opts, _ = GRIDS[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    read_gbs = api.bandwidth_probe(0)["read_dword"]
    with api.Solver(size, size, res, **opts) as s:
        s.load_scene(os.path.join(SCENES, scene))
        s.run(L)  # warm-up: classification, graph capture
        s.run(L)
        t = s.timings()
        ms = [s.compute_room_metrics() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        span = int(((s.T - delay[reached].astype(np.int64)) * 4).sum())
        med = float(np.median(ms))
        rec = dict(grid=name, cells=[s.gx, s.gy], T=s.T, fs=s.fs, reached_cells=int(reached.sum()),
                   metrics_ms_median=round(med, 5), metrics_ms_min=round(float(np.min(ms)), 5),
                   metrics_ms_max=round(float(np.max(ms)), 5), analysis_ms=round(float(t.analysisMs), 5),
                   fdtd_ms=round(float(t.fdtdMs), 5), history_bytes_spanned=span,
                   spanned_gb_per_s=round(span / (med * 1e-3) / 1e9, 2), probe_read_gb_per_s=round(read_gbs, 1),
                   share_of_probe_read=round(span / (med * 1e-3) / 1e9 / read_gbs, 4))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "room_metrics.txt")
    lines = []
    for name, (_, _, _, _, limit) in GRIDS.items():
        # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write("\n%s ended with status %d: stopping here\n" % (name, r.returncode))
            return r.returncode
        lines.append(r.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
        with open(out, "w") as f:
            f.write("# tools/gpu_room_metrics_measure.py: PvAmdComputeRoomMetrics on one MI355X (median of 20 after 3 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
