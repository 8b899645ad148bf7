"""GPU: first measurements of graded edge layers (profiles/edge_layer.txt).

Whole-run time (host wall clock around PvAmdRun, which waits for the run) and PvAmdTimings.fdtdMs of an open grid without
layers, with unsplit layers and with split-field layers (default R0) of the default width (api.EDGE_LAYER_DEFAULT_WIDTH on every
side) at 127^2, 254^2, 1024^2 and 4096^2 (275 Hz), the listener at the centre.  The three solvers of a size alternate run by
run; medians of N runs.  The layer launch's share of a sweep
is in a kernel trace of this script: rocprofv3 --kernel-trace --stats -- python tools/gpu_layer_measure.py ...

    python tools/gpu_layer_measure.py [runs] [out.json]
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


def measure(n, runs):
    size = float((n + 0.5) * DX)
    L = ((n // 2 + 0.5) * float(DX), 0.0, (n // 2 + 0.5) * float(DX))
    w = api.EDGE_LAYER_DEFAULT_WIDTH
    pair = []
    for w4, split in (((0, 0, 0, 0), False), ((w, w, w, w), False), ((w, w, w, w), True)):
        s = api.Solver(size, size, 275)
        if split:
            s.set_edge_layer_split(w4)
        else:
            s.set_edge_layer(w4)
        s.run(L)  # warm-up: classification, graph capture
        pair.append(s)
    ms, fdtd = [[], [], []], [[], [], []]
    for _ in range(runs):
        for k, s in enumerate(pair):
            t0 = time.perf_counter()
            s.run(L)
            ms[k].append((time.perf_counter() - t0) * 1e3)
            fdtd[k].append(s.timings().fdtdMs)
    out = dict(grid=n, layer_width=w)
    for k, tag in enumerate(("no_layer", "layer", "split_layer")):
        out[tag] = dict(resident=int(pair[k].info.residentKernel), run_ms_median=round(float(np.median(ms[k])), 4),
                        run_ms_min=round(float(np.min(ms[k])), 4), fdtd_ms_median=round(float(np.median(fdtd[k])), 4))
    for s in pair:
        s.close()
    return out


def main():
    runs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    rows = []
    for n in (127, 254, 1024, 4096):
        rows.append(measure(n, runs if n < 4096 else max(3, runs // 4)))
        print(json.dumps(rows[-1]), flush=True)
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
