"""GPU: measurements of the in-run spectral query records (PvAmdSetQuerySpectralRecords, csrc/pv_query_spectral.hip): the runs that
profiles/query_spectral_records.txt quotes.

Per scene, 64 queries (random reached cells of a first run); every figure the median of 20 after 3 warm-ups, with the smallest
and largest sample next to it:
  (a) wall time of run_async + sync with NO kind selected -- with this build, and with the build PLANEVERB_AMD_BASELINE_LIB names
      (the parent commit's library).  The launch chain is the same, so the two medians should agree within the same-GPU
      repeatability.  A baseline from before the feature has no such call at all and gets (a) alone; one that has the calls
      gets every figure, for a comparison of the host side of two builds;
  (b) the same wall time with each kind alone and with all three (reading the records back from pinned memory included): band
      kinds with two octaves (63, 125 Hz), the spectrum with 8 and with 32 bins.  A launch is expected to cost what its slowest
      work item costs as a lone wave, whatever the number of queries; and all NINE in-run kinds, the six time-domain ones of
      PvAmdSetQueryRecords (4 echogram slots, the default lobe windows) beside the three;
  (c) the comparison: the same run followed by the three whole-map passes (compute_band_metrics, compute_modulation,
      compute_spectrum with 8 bins, each with its own synchronisation), as wall time, and the passes' own device times.

Scenes: SmallRoomScene at the 70^2 and 254^2 presets, Shoebox 25 m at 512^2 (T = 3179).

    python tools/gpu_query_spectral_measure.py [out.txt]    every scene, one child process each under its own time limit;
                                                            stops at the first that fails
    python tools/gpu_query_spectral_measure.py --one NAME [--baseline]   one scene, one JSON line
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
NEW_CALLS = ("PvAmdSetQuerySpectralRecords", "PvAmdGetQuerySpectralKinds", "PvAmdQuerySpectralFloats", "PvAmdGetQueriedSpectralRecords")
BANDS = [63.0, 125.0]


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
    full = True
    if baseline:  # a build from before the feature: bind what it has
        have = ctypes.CDLL(api.LIB_PATH)
        for n in NEW_CALLS:
            if not hasattr(have, n):
                api.SYMBOLS.pop(n, None)
                full = False
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
        if full:
            bins8 = [float(v) for v in np.linspace(20.0, s.fs / 4.0, 8)]
            bins32 = [float(v) for v in np.linspace(20.0, s.fs / 4.0, 32)]
            s.set_bands(BANDS)
            s.set_spectrum_bins(bins8)
            computes = (s.compute_band_metrics, s.compute_modulation, s.compute_spectrum)
            own = []

            def run_whole():
                run()
                own.append([c() for c in computes])

            rec["run_then_three_whole_map_passes_wall_ms"] = stats(timed(run_whole, runs, warm))
            rec["each_whole_map_pass_own_ms_median"] = [round(float(v), 5) for v in np.median(np.array(own[warm:]), axis=0)]

            def case(kinds, six=0):
                s.set_query_spectral_records(kinds)
                s.set_query_records(six)

                def f():
                    run()
                    for k in (1, 2, 4):
                        if kinds & k:
                            s.queried_spectral_records(k)
                    for k in (1, 2, 4, 8, 16, 32):
                        if six & k:
                            s.queried_records(k)

                return stats(timed(f, runs, warm))

            rec["run_band_metrics_wall_ms"] = case(api.QSPEC_BAND_METRICS)
            rec["run_modulation_wall_ms"] = case(api.QSPEC_MODULATION)
            rec["run_spectrum_8_bins_wall_ms"] = case(api.QSPEC_SPECTRUM)
            rec["run_all_three_8_bins_wall_ms"] = case(api.QSPEC_ALL)
            s.set_echogram(0.01, 4)
            rec["run_all_nine_8_bins_wall_ms"] = case(api.QSPEC_ALL, api.QREC_ALL)
            s.set_spectrum_bins(bins32)
            rec["run_spectrum_32_bins_wall_ms"] = case(api.QSPEC_SPECTRUM)
            rec["run_all_three_32_bins_wall_ms"] = case(api.QSPEC_ALL)
            s.set_query_spectral_records(0)
            s.set_query_records(0)
            rec["run_no_kinds_again_wall_ms"] = stats(timed(run, runs, warm))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2], "--baseline" in sys.argv[3:])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "query_spectral_measured.txt")
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
                f.write("# tools/gpu_query_spectral_measure.py: PvAmdSetQuerySpectralRecords on one MI355X, 64 queries "
                        "(wall times in ms: median / min / max of 20 after 3 warm-ups)\n")
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
