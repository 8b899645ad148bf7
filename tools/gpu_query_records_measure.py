"""GPU: measurements of the in-run query records (PvAmdSetQueryRecords, csrc/pv_query_records.hip): the runs that
profiles/query_records.txt quotes (written there unless another file is named).

Per scene, 64 queries (random reached cells of a first run) and all six kinds, echogram (0.005 s, 16 slots), default lobe
windows; every figure the median of 20 after 3 warm-ups, with the smallest and largest sample next to it:
  * wall time of run_async + sync with NO kind selected -- with this build, and with the build PLANEVERB_AMD_BASELINE_LIB names
    (the parent commit's library, which has no such call at all).  The empty path is meant to cost nothing: the two medians
    should differ by less than the baseline's own spread;
  * the same wall time with the six kinds selected (reading the records back from pinned memory included);
  * the comparison: the same run followed by the six whole-map passes (compute_<kind>(), each with its own synchronisation), as
    wall time, and the sum of the six passes' own device times.

Scenes: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179).

    python tools/gpu_query_records_measure.py [out.txt]     every scene, one child process each under its own time limit;
                                                            stops at the first that fails
    python tools/gpu_query_records_measure.py --one NAME [--baseline]   one scene, one JSON line
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = os.path.join(ROOT, "tests", "scenes")
L = (5.0, 0.0, 4.0)
# name: (scene, size in metres, resolution, time limit of a child in seconds)
GRIDS = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, 120),
    "smallroom254": ("SmallRoomScene.pv", 25.0, 1000, 150),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, 300),
}
NEW_CALLS = ("PvAmdSetQueryRecords", "PvAmdGetQueryRecordKinds", "PvAmdQueryRecordFloats", "PvAmdGetQueriedRecords")


def stats(samples):
    return dict(median=round(float(np.median(samples)), 5), min=round(float(np.min(samples)), 5),
                max=round(float(np.max(samples)), 5))


def timed(f, runs, warm):
    out = []
    for _ in range(warm + runs):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out[warm:]


def one(name, baseline, runs=20, warm=3):
    from planeverb_amd import api
    if baseline:  # a build from before the feature: bind what it has
        have = ctypes.CDLL(api.LIB_PATH)
        for n in NEW_CALLS:
            if not hasattr(have, n):
                api.SYMBOLS.pop(n, None)
    scene, size, res, _ = GRIDS[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    with api.Solver(size, size, res) as s:
        s.load_scene(os.path.join(SCENES, scene))
        s.run(L)  # warm-up: classification, graph capture
        s.run(L)
        delay = s.results()[1]
        idx = np.argwhere(delay < 1e30)
        sel = idx[np.random.default_rng(64).choice(len(idx), 64, replace=False)]
        dx = s.dx
        s.set_output_queries([((x + 0.5) * dx, 0.0, (y + 0.5) * dx) for x, y in sel])

        def run():
            s.run_async(L)
            s.sync()

        rec = dict(scene=name, lib=os.path.basename(api.LIB_PATH), cells=[s.gx, s.gy], T=s.T, queries=64,
                   run_no_kinds_wall_ms=stats(timed(run, runs, warm)))
        if not baseline:
            s.set_echogram(0.005, 16)
            computes = (s.compute_room_metrics, s.compute_decay_times, s.compute_lateral_fraction, s.compute_echogram,
                        s.compute_echo_criterion, s.compute_lobes)
            own = []

            def run_whole():
                run()
                own.append(sum(c() for c in computes))

            rec["run_then_six_whole_map_passes_wall_ms"] = stats(timed(run_whole, runs, warm))
            rec["six_whole_map_passes_own_ms_sum"] = stats(own[warm:])
            rec["each_whole_map_pass_own_ms_median"] = [round(float(np.median([c() for _ in range(5)])), 5) for c in computes]
            s.set_query_records(api.QREC_ALL)

            def run_records():
                run()
                for k in (1, 2, 4, 8, 16, 32):
                    s.queried_records(k)

            rec["run_six_kinds_wall_ms"] = stats(timed(run_records, runs, warm))
            rec["analysis_ms_of_the_last_run"] = round(float(s.timings().analysisMs), 5)
            s.set_query_records(0)
            rec["run_no_kinds_again_wall_ms"] = stats(timed(run, runs, warm))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2], "--baseline" in sys.argv[3:])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "query_records.txt")
    base = os.environ.get("PLANEVERB_AMD_BASELINE_LIB")
    lines = []
    for name, (_, _, _, limit) in GRIDS.items():
        jobs = [([], dict(os.environ))]
        if base:
            jobs.append((["--baseline"], dict(os.environ, PLANEVERB_AMD_LIB=base)))
        for extra, env in jobs:
            # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name] + extra,
                               capture_output=True, text=True, env=env)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.stderr.write("\n%s ended with status %d: stopping here\n" % (name, r.returncode))
                return r.returncode
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
            with open(out, "w") as f:
                f.write("# tools/gpu_query_records_measure.py: PvAmdSetQueryRecords on one MI355X, 64 queries, six kinds "
                        "(wall times in ms: median / min / max of 20 after 3 warm-ups)\n")
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
