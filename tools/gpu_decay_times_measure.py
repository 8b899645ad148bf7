"""GPU: first measurements of the decay-times pass (PvAmdComputeDecayTimes, csrc/pv_decay.hip): the runs that
profiles/decay_times.txt quotes and explains (written to profiles/decay_times_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups) with both walks of the curve in one
launch and -- in a child process of its own, PLANEVERB_AMD_DECAY_LAUNCHES=2 -- as a launch each, next to the room-metrics pass
of the same run in the same process (the yardstick: the same history, read once, with almost no arithmetic), the history bytes
the reached cells span (sum over the cells with an onset of (T - onset) x 4 bytes; the decay times read them twice) and how many
cells got each time.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench scene,
HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_decay_times_measure.py [out.txt]        every grid and form, one child process each under its own time
                                                             limit; stops at the first that fails
    python tools/gpu_decay_times_measure.py --one NAME       one grid, one JSON line
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
        dm = [s.compute_decay_times() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        span = int(((s.T - delay[reached].astype(np.int64)) * 4).sum())
        d = s.decay_times()
        med, mmed = float(np.median(dm)), float(np.median(mm))
        rec = dict(grid=name, launches=int(os.environ.get("PLANEVERB_AMD_DECAY_LAUNCHES", "1")), cells=[s.gx, s.gy], T=s.T, fs=s.fs,
                   reached_cells=int(reached.sum()), valid_edt_t20_t30=[int((~np.isnan(d[..., k])).sum()) for k in range(3)],
                   decay_ms_median=round(med, 5), decay_ms_min=round(float(np.min(dm)), 5), decay_ms_max=round(float(np.max(dm)), 5),
                   metrics_ms_median=round(mmed, 5), decay_over_metrics=round(med / mmed, 2), history_bytes_spanned=span,
                   spanned_twice_gb_per_s=round(2 * span / (med * 1e-3) / 1e9, 2))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "decay_times_runs.txt")
    lines = []
    for name, (_, _, _, limit) in GRIDS.items():
        for launches in ("1", "2"):
            # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name],
                               capture_output=True, text=True, env=dict(os.environ, PLANEVERB_AMD_DECAY_LAUNCHES=launches))
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.stderr.write("\n%s (%s) ended with status %d: stopping here\n" % (name, launches, r.returncode))
                return r.returncode
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
            with open(out, "w") as f:
                f.write("# tools/gpu_decay_times_measure.py: PvAmdComputeDecayTimes on one MI355X (median of 20 after 3 warm-ups)\n")
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
