"""GPU: first measurements of non-absorbing grid edges (profiles/boundary.txt).

Whole-run time (host wall clock around PvAmdRun, which waits for the run) and PvAmdTimings of absorbing edges (R = 0) against
rigid ones (R = 1, pv_ReflectingBoundary) on: 70^2 (25 m SmallRoomScene.pv at 275 Hz, the resident kernel), an open 254^2 grid,
and HugeRoom.pv in a 2048^2 grid (Mode A, 275 Hz).  The two solvers of a workload alternate run by run; medians of N runs.
reachedCells: a closed grid keeps its energy, so more cells reach the audible threshold inside the same history window.
The edge pass alone (pv_edge_coef_kernel) is in a kernel trace of this script: rocprofv3 --kernel-trace --stats -- python ...

    python tools/gpu_boundary_measure.py [runs] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planeverb_amd import api  # noqa: E402

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
SCENES = os.path.join(ROOT, "tests", "scenes")


def workloads():
    s254, s2048 = float((254 + 0.5) * DX), float((2048 + 0.5) * DX)
    return [dict(name="70^2 SmallRoomScene.pv (resident kernel)", size=25.0, scene="SmallRoomScene.pv", L=(5.0, 0.0, 4.0)),
            dict(name="254^2 open", size=s254, scene=None, L=(20.5 * float(DX), 0.0, 20.5 * float(DX))),
            dict(name="2048^2 HugeRoom.pv", size=s2048, scene="HugeRoom.pv", L=(s2048 / 2, 0.0, s2048 / 2))]


def measure(w, runs):
    pair = []
    for R4 in ((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0, 1.0)):
        s = api.Solver(w["size"], w["size"], 275)
        if w["scene"]:
            s.load_scene(os.path.join(SCENES, w["scene"]))
        s.set_grid_boundary(R4)
        s.run(w["L"])  # warm-up: geometry, edge pass, graph capture
        pair.append(s)
    ms = [[], []]
    fdtd = [[], []]
    for _ in range(runs):
        for k, s in enumerate(pair):
            t0 = time.perf_counter()
            s.run(w["L"])
            ms[k].append((time.perf_counter() - t0) * 1e3)
            fdtd[k].append(s.timings().fdtdMs)
    out = dict(workload=w["name"], gx=pair[0].gx, resident=int(pair[0].info.residentKernel))
    for k, tag in enumerate(("absorbing", "rigid")):
        t = pair[k].timings()
        out[tag] = dict(run_ms_median=round(float(np.median(ms[k])), 4), run_ms_min=round(float(np.min(ms[k])), 4),
                        fdtd_ms_median=round(float(np.median(fdtd[k])), 4), reached_cells=int(t.reachedCells),
                        general_launches=int(t.generalLaunches))
    res = [s.results() for s in pair]
    for k, tag in enumerate(("absorbing", "rigid")):
        r, d = res[k]
        on = (d < 1e30) & np.isfinite(r[..., 2])
        out[tag]["median_rt60_s"] = round(float(np.median(r[..., 2][on])), 4) if on.any() else None
        out[tag]["median_wet_gain"] = round(float(np.median(r[..., 1][on])), 4) if on.any() else None
    for s in pair:
        s.close()
    return out


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rows = [measure(w, runs) for w in workloads()]
    for r in rows:
        print(json.dumps(r))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
