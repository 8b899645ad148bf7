"""GPU: first measurements of the band-metrics pass (PvAmdComputeBandMetrics, csrc/pv_bands.hip): the runs that
profiles/band_metrics.txt quotes (written to profiles/band_metrics_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 10 after 2 warm-ups) for 1, 2, 3 and 8 octave or third-octave
bands -- one launch per register block of bands, each a re-read of the history -- next to the decay-times pass of the same run in
the same process (the yardstick: the same two walks of the same history without the filters), the history bytes the reached
cells span, and the time per band.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench scene,
HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_band_metrics_measure.py [out.txt]       every grid, one child process each under its own time limit; stops
                                                             at the first that fails
    python tools/gpu_band_metrics_measure.py --one NAME      one grid, one JSON line
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
# name: (scene, size in metres, resolution, time limit of the child in seconds)
GRIDS = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, 120),
    "smallroom254": ("SmallRoomScene.pv", 25.0, 1000, 120),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, 240),
    "hugeroom4096": ("HugeRoom.pv", float((4096 + 0.5) * DX), 275, 240),
}
# (centres, fraction): one band, one full block, a padded block, the most a call takes
SETS = (([63.0], 1), ([63.0, 125.0], 1), ([63.0, 125.0, 250.0], 1), ([31.5, 40.0, 50.0, 63.0, 80.0, 100.0, 125.0, 160.0], 3))


def one(name, runs=10, warm=2):
    from planeverb_amd import api
    scene, size, res, _ = GRIDS[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    with api.Solver(size, size, res) as s:
        s.load_scene(os.path.join(SCENES, scene))
        s.run(L)  # warm-up: classification, graph capture
        s.run(L)
        dm = [s.compute_decay_times() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        span = int(((s.T - delay[reached].astype(np.int64)) * 4).sum())
        dmed = float(np.median(dm))
        rec = dict(grid=name, cells=[s.gx, s.gy], T=s.T, fs=s.fs, reached_cells=int(reached.sum()), history_bytes_spanned=span,
                   decay_ms_median=round(dmed, 5), bands=[])
        for hz, fraction in SETS:
            s.set_bands(hz, fraction)
            bm = [s.compute_band_metrics() for _ in range(warm + runs)][warm:]
            med = float(np.median(bm))
            m = s.band_metrics()
            rec["bands"].append(dict(n=len(hz), fraction=fraction, ms_median=round(med, 5), ms_min=round(float(np.min(bm)), 5),
                                     ms_max=round(float(np.max(bm)), 5), ms_per_band=round(med / len(hz), 5),
                                     over_decay=round(med / dmed, 2),
                                     valid_t20=[int((~np.isnan(m[..., j, 1])).sum()) for j in range(len(hz))]))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "band_metrics_runs.txt")
    lines = []
    for name, (_, _, _, limit) in GRIDS.items():
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
            f.write("# tools/gpu_band_metrics_measure.py: PvAmdComputeBandMetrics on one MI355X (median of 10 after 2 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
