"""GPU: measurements of the echogram pass (PvAmdComputeEchogram, csrc/pv_echogram.hip): the runs that profiles/echogram.txt
quotes and explains (written to profiles/echogram_runs.txt unless another file is named).

Per grid: the pass's device time (the `ms` out-parameter; median of 20 after 3 warm-ups) at (0.005 s, 16 slots) -- an 80 ms
window, the one the lateral-fraction pass walks -- and at (0.02 s, 32 slots), next to the lateral-fraction pass of the same run
in the same process (the yardstick: the same three loads per sample and the same recurrence, six running sums instead of three,
no stores inside the window), the history bytes each window spans (sum over the cells with an onset of
(min(onset + ns nSlots, T) - onset) x 4 bytes) and the bytes of records each setting writes.

Grids: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179: a 1.3 GB history) and the bench scene,
HugeRoom in a 4096^2 grid with T = 435.

    python tools/gpu_echogram_measure.py [out.txt]       every grid, one child process each under its own time limit; stops
                                                         at the first that fails
    python tools/gpu_echogram_measure.py --one NAME      one grid, one JSON line
PLANEVERB_AMD_LIB names another build of the library (make BUILD=... OUT=... EXTRA=-DPV_ECHOGRAM_NB=4): its name goes into the line.
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
SETTINGS = ((0.005, 16), (0.02, 32))
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
        lm = [s.compute_lateral_fraction() for _ in range(warm + runs)][warm:]
        delay = s.results()[1]
        reached = delay < 1e30
        onset = delay[reached].astype(np.int64)
        n80 = int(np.float32(0.08) * np.float32(s.fs))
        lmed = float(np.median(lm))
        rec = dict(grid=name, lib=os.path.basename(os.environ.get("PLANEVERB_AMD_LIB", "libplaneverb_amd.so")), cells=[s.gx, s.gy],
                   T=s.T, fs=s.fs, reached_cells=int(reached.sum()), lateral_ms_median=round(lmed, 5),
                   lateral_window_steps=n80, lateral_bytes_spanned=int(((np.minimum(onset + n80, s.T) - onset) * 4).sum()))
        for sec, n in SETTINGS:
            s.set_echogram(sec, n)
            ns = s.echogram_slots()[2]
            em = [s.compute_echogram() for _ in range(warm + runs)][warm:]
            med = float(np.median(em))
            span = int(((np.minimum(onset + ns * n, s.T) - onset) * 4).sum())
            e = s.echogram_at((5.0, 0.0, 6.0))
            key = "%gs_x%d" % (sec, n)
            rec[key] = dict(slot_steps=ns, window_steps=ns * n, ms_median=round(med, 5), ms_min=round(float(np.min(em)), 5),
                            ms_max=round(float(np.max(em)), 5), over_lateral=round(med / lmed, 2), window_bytes_spanned=span,
                            window_gb_per_s=round(span / (med * 1e-3) / 1e9, 2),
                            record_bytes_reached=int(reached.sum()) * (1 + 3 * n) * 4,
                            n_at_emitter=float(e[0]), level_db_at_emitter=[
                                round(float(v), 2) for v in 10.0 * np.log10(np.maximum(e[1::3][:8], 1e-30) / max(float(e[1]), 1e-30))])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "echogram_runs.txt")
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
            f.write("# tools/gpu_echogram_measure.py: PvAmdComputeEchogram on one MI355X (median of 20 after 3 warm-ups)\n")
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
