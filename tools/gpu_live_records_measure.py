"""GPU: the live module's update period with and without emission records (PlaneverbSetEmissionRecords): the runs that
profiles/live_records.txt quotes (written there unless another file is named).

The update period is measured as the caller sees it: published iterations (PlaneverbIterationCount) over 2 s of wall time, as
milliseconds per iteration; every figure the median of 5 such windows, with the smallest and largest next to it.
SmallRoomScene at the 70^2 and 254^2 presets, both worker loops (PLANEVERB_AMD_LIVE_PIPELINE 1 and 2):
  (a) no kinds selected -- with this build, and with the build PLANEVERB_AMD_BASELINE_LIB names (the parent commit's library, which
      has none of the calls).  The launch chain is the same, so the two should agree within the same-GPU repeatability;
  (b) all six kinds (echogram 0.005 s x 16 slots, default lobe windows) with 3, 64 and 1024 emitters in distinct reached cells.
      The cost model to confirm or refute: the slowest selected kind as a lone wave, independent of the number of emitters.

    python tools/gpu_live_records_measure.py [out.txt]      every case, one child process per grid, loop and build, each under its
                                                            own time limit; stops at the first that fails
    python tools/gpu_live_records_measure.py --one GRID PIPELINE [--baseline]    one child: one JSON line per configuration
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE = os.path.join(ROOT, "tests", "scenes", "SmallRoomScene.pv")
L = (5.0, 0.0, 4.0)
GRIDS = {"smallroom70": (25.0, 275), "smallroom254": (25.0, 1000)}  # name: (size in metres, resolution)
WINDOW_S, WINDOWS = 2.0, 5
CHILD_LIMIT_S = 240


def period(api):
    """ms per published iteration: WINDOWS windows of WINDOW_S seconds"""
    out = []
    for _ in range(WINDOWS):
        n0, t0 = api.IterationCount(), time.perf_counter()
        time.sleep(WINDOW_S)
        n1, t1 = api.IterationCount(), time.perf_counter()
        if n1 <= n0:
            raise RuntimeError("the live module published nothing in %.1f s: %s" % (WINDOW_S, api.last_error()))
        out.append((t1 - t0) * 1e3 / (n1 - n0))
    return dict(median=round(float(np.median(out)), 5), min=round(float(np.min(out)), 5), max=round(float(np.max(out)), 5))


def one(grid, pipeline, baseline):
    from planeverb_amd import api
    size, res = GRIDS[grid]
    if baseline:  # a build from before the feature: bind what it has
        import ctypes
        have = ctypes.CDLL(api.LIB_PATH)
        for n in list(api.SYMBOLS):
            if not hasattr(have, n):
                api.SYMBOLS.pop(n)
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    os.environ["PLANEVERB_AMD_LIVE_PIPELINE"] = str(pipeline)
    with api.Solver(size, size, res) as s:  # the reached cells, for the emitters' positions
        s.load_scene(SCENE)
        s.run(L)
        reached = np.argwhere(s.results()[1] < 1e30)
        dx, cells, T = s.dx, [s.gx, s.gy], s.T
    sel = reached[np.random.default_rng(1024).choice(len(reached), 1024, replace=False)]
    pos = [((x + 0.5) * dx, 0.0, (y + 0.5) * dx) for x, y in sel]
    for emitters, kinds in ([(3, 0)] if baseline else [(3, 0), (3, api.QREC_ALL), (64, api.QREC_ALL), (1024, api.QREC_ALL)]):
        api.Init(api.Config((size, size), res, 0, ".", 0, api.pv_GPU))
        try:
            api.SetListenerPosition(L)
            api.LoadScene(SCENE)
            for p in pos[:emitters]:
                api.Emit(p)
            if kinds:
                api.SetEmissionEchogram(0.005, 16)
                api.SetEmissionRecords(kinds)
            target = api.IterationCount() + 10
            if api.WaitIterations(target, 60000) < target:
                raise RuntimeError("the live module does not iterate: " + api.last_error())
            rec = dict(grid=grid, lib=os.path.basename(api.LIB_PATH), cells=cells, T=T, pipeline=pipeline, emitters=emitters,
                       kinds=kinds, ms_per_iteration=period(api))
            if kinds:
                rec["cells_served"] = api.EmissionRecordCells()
                rec["kinds_published"] = api.EmissionRecordKinds()
        finally:
            api.Exit()
        print(json.dumps(rec), flush=True)


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--one":
        one(sys.argv[2], int(sys.argv[3]), "--baseline" in sys.argv[4:])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "live_records.txt")
    base = os.environ.get("PLANEVERB_AMD_BASELINE_LIB")
    lines = []
    for grid in GRIDS:
        for pipeline in (1, 2):
            jobs = [([], dict(os.environ))]
            if base:
                jobs.append((["--baseline"], dict(os.environ, PLANEVERB_AMD_LIB=base)))
            for extra, env in jobs:
                # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
                r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", grid,
                                    str(pipeline)] + extra, capture_output=True, text=True, env=env)
                got = [l for l in r.stdout.splitlines() if l.startswith("{")]
                lines += got
                print("\n".join(got), flush=True)
                with open(out, "w") as f:
                    f.write("# tools/gpu_live_records_measure.py: the live module's update period on one MI355X, ms per published "
                            "iteration\n# (median / min / max of %d windows of %.0f s); kinds = 0: no emission records, 63: all six\n"
                            % (WINDOWS, WINDOW_S))
                    f.write("\n".join(lines) + "\n")
                if r.returncode != 0:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.stderr.write("\n%s pipeline %d ended with status %d: stopping here\n" % (grid, pipeline, r.returncode))
                    return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
