"""GPU: first measurements of the lateral-fraction pass (PvAmdComputeLateralFraction, csrc/pv_lateral.hip): the runs that
profiles/lateral_fraction.txt quotes and explains (written to profiles/lateral_fraction_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups) next to the room-metrics pass of the
same run in the same process (the yardstick: one load per sample, almost no arithmetic, but to T - 1), the history bytes the
pass's own cells span (sum over the cells with an onset of (min(onset + n80, T) - onset) x 4 bytes: the prefix this pass walks)
beside those the room metrics span ((T - onset) x 4 bytes), and the distribution of lf.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench scene,
HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_lateral_measure.py [out.txt]        every grid, one child process each under its own time limit; stops
                                                         at the first that fails
    python tools/gpu_lateral_measure.py --one NAME       one grid, one JSON line
PLANEVERB_AMD_LIB names another build of the library (make BUILD=... OUT=... EXTRA=-DPV_LATERAL_NB=4): its name goes into the line.
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


def one(name, runs=20, warm=3):
    from planeverb_amd import api
    scene, size, res, _ = GRIDS[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    with api.Solver(size, size, res) as s:
        s.load_scene(os.path.join(SCENES, scene))
        s.run(L)  # warm-up: classification, graph capture
        s.run(L)
        mm = [s.compute_room_metrics() for _ in range(warm + runs)][warm:]
        lm = [s.compute_lateral_fraction() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        onset = delay[reached].astype(np.int64)
        n80 = int(np.float32(0.08) * np.float32(s.fs))
        span = int(((np.minimum(onset + n80, s.T) - onset) * 4).sum())
        span_metrics = int(((s.T - onset) * 4).sum())
        lf = s.lateral_fraction()[..., 0][reached]
        ok = np.isfinite(lf)
        med, mmed = float(np.median(lm)), float(np.median(mm))
        rec = dict(grid=name, lib=os.path.basename(os.environ.get("PLANEVERB_AMD_LIB", "libplaneverb_amd.so")), cells=[s.gx, s.gy],
                   T=s.T, fs=s.fs, n80=n80, reached_cells=int(reached.sum()), lf_not_finite=int((~ok).sum()),
                   lf_median_p90_max=[round(float(v), 4) for v in (np.median(lf[ok]), np.percentile(lf[ok], 90), lf[ok].max())],
                   lateral_ms_median=round(med, 5), lateral_ms_min=round(float(np.min(lm)), 5),
                   lateral_ms_max=round(float(np.max(lm)), 5), metrics_ms_median=round(mmed, 5),
                   lateral_over_metrics=round(med / mmed, 2), window_bytes_spanned=span, metrics_bytes_spanned=span_metrics,
                   window_gb_per_s=round(span / (med * 1e-3) / 1e9, 2))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lateral_fraction_runs.txt")
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
            f.write("# tools/gpu_lateral_measure.py: PvAmdComputeLateralFraction on one MI355X (median of 20 after 3 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
