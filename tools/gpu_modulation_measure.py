"""GPU: measurements of the modulation pass (PvAmdComputeModulation, csrc/pv_modulation.hip): the runs that
profiles/modulation.txt quotes (written to profiles/modulation_runs.txt unless another file is named).

Per grid: the pass's own device time (the `ms` out-parameter; median of 20 after 3 warm-ups) for the two octaves 63 and 125 Hz --
one launch and one walk of the history per band -- next to the band-metrics pass (PvAmdComputeBandMetrics: two walks, both bands
in one launch) for the same bands on the same run in the same process: that pass is the yardstick.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history).

    python tools/gpu_modulation_measure.py [out.txt]         every grid, one child process each under its own time limit; stops
                                                             at the first that fails
    python tools/gpu_modulation_measure.py --one NAME        one grid, one JSON line
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = os.path.join(ROOT, "tests", "scenes")
L = (5.0, 0.0, 4.0)
BANDS = [63.0, 125.0]
# name: (scene, size in metres, resolution, time limit of the child in seconds)
GRIDS = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, 120),
    "smallroom254": ("SmallRoomScene.pv", 25.0, 1000, 120),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, 240),
}


def one(name, runs=20, warm=3):
    from planeverb_amd import api
    scene, size, res, _ = GRIDS[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    with api.Solver(size, size, res) as s:
        s.load_scene(os.path.join(SCENES, scene))
        s.run(L)  # warm-up: classification, graph capture
        s.run(L)
        s.set_bands(BANDS)
        bm = [s.compute_band_metrics() for _ in range(warm + runs)][warm:]
        mm = [s.compute_modulation() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        span = int(((s.T - delay[reached].astype(np.int64)) * 4).sum())
        bmed, mmed = float(np.median(bm)), float(np.median(mm))
        m = s.modulation()
        rec = dict(grid=name, cells=[s.gx, s.gy], T=s.T, fs=s.fs, bands=BANDS, reached_cells=int(reached.sum()),
                   history_bytes_spanned=span, band_metrics_ms_median=round(bmed, 5), band_metrics_ms_min=round(float(np.min(bm)), 5),
                   band_metrics_ms_max=round(float(np.max(bm)), 5), modulation_ms_median=round(mmed, 5),
                   modulation_ms_min=round(float(np.min(mm)), 5), modulation_ms_max=round(float(np.max(mm)), 5),
                   modulation_over_band_metrics=round(mmed / bmed, 3),
                   mean_mti=[round(float(np.nanmean(m[..., j, 14])), 4) for j in range(len(BANDS))])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "modulation_runs.txt")
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
            f.write("# tools/gpu_modulation_measure.py: PvAmdComputeModulation beside PvAmdComputeBandMetrics on one MI355X "
                    "(median of 20 after 3 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
