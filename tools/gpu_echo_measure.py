"""GPU: first measurements of the echo-criterion pass (PvAmdComputeEchoCriterion, csrc/pv_echo.hip): the runs that
profiles/echo_criterion.txt quotes and explains (written to profiles/echo_criterion_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups) next to the room-metrics and the
decay-times pass of the same run in the same process.  The decay-times pass is the yardstick: one logarithm and one division per
sample, where this pass makes two powf and six divisions.  Also the history bytes the reached cells span (sum over the cells with
an onset of (T - onset) x 4 bytes; this pass reads them three times, two of them nD steps behind the first) and how many cells
exceed the published thresholds.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench scene,
HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_echo_measure.py [out.txt]        every grid, one child process each under its own time limit; stops at the
                                                      first that fails
    python tools/gpu_echo_measure.py --one NAME       one grid, one JSON line
A variant build of the library (make BUILD=build_x OUT=../libplaneverb_amd_x.so EXTRA="-DPV_ECHO_S=8 -DPV_ECHO_NB=2") is measured
by naming it in PLANEVERB_AMD_LIB; the line then carries its file name.
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
        em = [s.compute_echo_criterion() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        span = int(((s.T - delay[reached].astype(np.int64)) * 4).sum())
        e = s.echo_criterion()
        med, mmed, dmed = float(np.median(em)), float(np.median(mm)), float(np.median(dm))
        samples = span // 4
        rec = dict(grid=name, lib=os.path.basename(os.environ.get("PLANEVERB_AMD_LIB", "libplaneverb_amd.so")), cells=[s.gx, s.gy],
                   T=s.T, fs=s.fs, lags=[int(np.float32(v) * np.float32(s.fs)) for v in (0.009, 0.014)],
                   reached_cells=int(reached.sum()),
                   speech_over_crit=int((e[..., 0][reached] > api.ECHO_SPEECH_CRIT).sum()),
                   music_over_crit=int((e[..., 5][reached] > np.float32(api.ECHO_MUSIC_CRIT)).sum()),
                   nan_values_in_reached=int(np.isnan(e[reached]).sum()),
                   echo_ms_median=round(med, 5), echo_ms_min=round(float(np.min(em)), 5), echo_ms_max=round(float(np.max(em)), 5),
                   decay_ms_median=round(dmed, 5), metrics_ms_median=round(mmed, 5), echo_over_decay=round(med / dmed, 2),
                   echo_over_metrics=round(med / mmed, 2), history_bytes_spanned=span,
                   spanned_three_times_gb_per_s=round(3 * span / (med * 1e-3) / 1e9, 2),
                   ns_per_reached_sample=round(med * 1e6 / max(samples, 1), 4))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "echo_criterion_runs.txt")
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
        # (a variant build's lines are added to the product build's)
        with open(out, "a" if (len(lines) > 1 or os.environ.get("PLANEVERB_AMD_LIB")) else "w") as f:
            if len(lines) == 1:
                f.write("# tools/gpu_echo_measure.py: PvAmdComputeEchoCriterion on one MI355X (median of 20 after 3 warm-ups)\n")
            f.write(lines[-1] + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
