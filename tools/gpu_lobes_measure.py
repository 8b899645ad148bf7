"""GPU: measurements of the lobes pass (PvAmdComputeLobes, csrc/pv_lobes.hip): the runs that profiles/lobes.txt quotes
(written to profiles/lobes_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups) at the default windows (10 ms, 80 ms)
and at seven edges, next to two passes of the same run in the same process: the echogram pass at (0.005 s, 16 slots) -- the same
three loads per sample and the same recurrence, over 80 ms only -- and the echo-criterion pass -- three loads per sample over the
whole response, as here.  With them the history bytes the pass spans (sum over the cells with an onset of (T - onset) x 4 bytes,
once; the pass loads three streams of them).

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history).

    python tools/gpu_lobes_measure.py [out.txt]       every grid, one child process each under its own time limit; stops at
                                                      the first that fails
    python tools/gpu_lobes_measure.py --one NAME      one grid, one JSON line
PLANEVERB_AMD_LIB names another build of the library (make BUILD=... OUT=... EXTRA=-DPV_LOBES_NB=4): its name goes into the line.
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
SEVEN = (0.005, 0.01, 0.02, 0.035, 0.05, 0.08, 0.15)
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
        delay = s.results()[1]
        reached = delay < 1e30
        onset = delay[reached].astype(np.int64)
        span = int(((s.T - onset) * 4).sum())
        s.set_echogram(0.005, 16)
        gm = float(np.median([s.compute_echogram() for _ in range(warm + runs)][warm:]))
        cm = float(np.median([s.compute_echo_criterion() for _ in range(warm + runs)][warm:]))
        rec = dict(grid=name, lib=os.path.basename(os.environ.get("PLANEVERB_AMD_LIB", "libplaneverb_amd.so")), cells=[s.gx, s.gy],
                   T=s.T, fs=s.fs, reached_cells=int(reached.sum()), history_bytes_spanned=span,
                   echogram_5ms_x16_ms_median=round(gm, 5), echo_criterion_ms_median=round(cm, 5))
        for key, edges in (("default", None), ("seven_edges", SEVEN)):
            s.set_lobe_windows(edges)
            lm = [s.compute_lobes() for _ in range(warm + runs)][warm:]
            med = float(np.median(lm))
            m = s.lobes_at((5.0, 0.0, 6.0))
            w = m[1:].reshape(-1, 5).astype(np.float64)
            with np.errstate(all="ignore"):
                share = w[:, 1:].max(axis=1) / w[:, 0]
            rec[key] = dict(edge_steps=[int(v) for v in s.lobe_windows()[1]], ms_median=round(med, 5),
                            ms_min=round(float(np.min(lm)), 5), ms_max=round(float(np.max(lm)), 5),
                            over_echogram=round(med / gm, 2), over_echo_criterion=round(med / cm, 2),
                            gb_per_s_three_streams=round(3 * span / (med * 1e-3) / 1e9, 1),
                            ns_per_reached_sample=round(med * 1e6 / max(span // 4, 1), 5),
                            record_bytes_reached=int(reached.sum()) * int(m.size) * 4,
                            largest_lobe_share_at_emitter=[round(float(v), 3) for v in share])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lobes_runs.txt")
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
            f.write("# tools/gpu_lobes_measure.py: PvAmdComputeLobes on one MI355X (median of 20 after 3 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
