"""GPU: what the emitter records of sparse-emitter mode cost (PvAmdSetEmitterRecords): the runs that
profiles/emitter_records.txt quotes.

HugeRoom 25 m in a 4096^2 grid (T = 25 432) in sparse-emitter mode, 64 emitters on a lattice around the listener.

    python tools/gpu_emitter_records_measure.py --wall none|time6|all9
        one process: 2 warm-up runs, then 7 timed runs (host clock around run(), which waits for the run); one JSON line with the
        median, the smallest and the largest.  PLANEVERB_AMD_LIB names another build of the library (an older one, which lacks the
        emitter records, can run `none`).
    python tools/gpu_emitter_records_measure.py --kinds
        one process, meant to run under `rocprofv3 --kernel-trace`: a warm-up, then one run per single kind and one with all nine.
    python tools/gpu_emitter_records_measure.py --parse TRACE.csv
        the kernel trace of --kinds: per run the device time of the two record launches and of the trace kernel (per pass).
"""
import csv
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZE, RES = 25.0, 16067  # 25 m in 4096^2 cells: T = 25 432
SCENE = os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv")
L = (5.0, 0.0, 4.0)
EMITTERS = [(2.0 + 1.0 * i, 0.0, 2.0 + 1.0 * j) for i in range(8) for j in range(8)]
ECHOGRAM, LOBES, BANDS, BINS = (0.005, 16), [0.005, 0.02, 0.08], [63.0, 125.0], [61.7, 137.5, 250.0]
KERNELS = ("pv_query_records_kernel", "pv_query_spectral_kernel", "pv_stream_rectrace_kernel", "pv_stream_trace_kernel")


def load_api():
    from planeverb_amd import api
    have = ctypes.CDLL(api.LIB_PATH)
    for n in [n for n in api.SYMBOLS if not hasattr(have, n)]:  # (an older build: bind what it exports)
        del api.SYMBOLS[n]
    return api


def make(api):
    s = api.Solver(SIZE, SIZE, RES, streaming_analysis=1)
    s.load_scene(SCENE)
    s.set_echogram(*ECHOGRAM)
    s.set_lobe_windows(LOBES)
    s.set_bands(BANDS, 1)
    s.set_spectrum_bins(BINS)
    s.set_emitters(EMITTERS)
    return s


def wall(config, runs=7, warm=2):
    api = load_api()
    kinds = {"none": None, "time6": (api.QREC_ALL, 0), "all9": (api.QREC_ALL, api.QSPEC_ALL)}[config]
    with make(api) as s:
        assert (s.gx, s.T) == (4096, 25432), (s.gx, s.T)
        if kinds:
            s.set_emitter_records(*kinds)
        ms = []
        for _ in range(warm + runs):
            t0 = time.perf_counter()
            s.run(L)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[warm:]
        reached = 0
        if kinds:
            reached = int(np.isfinite(s.emitter_records(api.QREC_ROOM_METRICS)[:, 0]).sum())
        print(json.dumps(dict(config=config, lib=os.path.basename(api.LIB_PATH), grid=[s.gx, s.gy], T=s.T, emitters=len(EMITTERS),
                              emitters_reached=reached, run_ms_median=round(float(np.median(ms)), 2), run_ms_min=round(min(ms), 2),
                              run_ms_max=round(max(ms), 2), runs=runs)))


def kinds_runs():
    api = load_api()
    with make(api) as s:
        s.run(L)
        for t, f in [(1 << k, 0) for k in range(6)] + [(0, 1 << k) for k in range(3)] + [(api.QREC_ALL, api.QSPEC_ALL)]:
            s.set_emitter_records(t, f)
            s.run(L)
        assert (s.gx, s.T) == (4096, 25432), (s.gx, s.T)
        print(json.dumps(dict(kinds_runs=10, T=s.T)))


def parse(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"]
            k = next((k for k in KERNELS if k in name), None)
            if k:
                rows.append((int(r["Start_Timestamp"]), k, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    labels = ["room metrics", "decay times", "lateral", "echogram", "echo criterion", "lobes", "band metrics (2 bands)",
              "modulation (2 bands)", "spectrum (3 bins)", "all nine"]
    # a run = the launches up to and including its last record launch; the warm-up run has none
    run, runs = [], []
    for i, (_, k, us) in enumerate(rows):
        run.append((k, us))
        nxt = rows[i + 1][1] if i + 1 < len(rows) else None
        if k.startswith("pv_query") and (nxt is None or not nxt.startswith("pv_query")):
            runs.append(run)
            run = []
    for label, r in zip(labels, runs):
        rec = [us for k, us in r if k == "pv_query_records_kernel"]
        spec = [us for k, us in r if k == "pv_query_spectral_kernel"]
        tr = [us for k, us in r if k == "pv_stream_rectrace_kernel"]
        old = [us for k, us in r if k == "pv_stream_trace_kernel"][-len(tr):] if tr else []
        print("%-24s records launch %9.1f us  spectral launch %9.1f us  trace kernel %d passes, median %.1f us, sum %.0f us "
              "(the emitter trace kernel beside it: median %.1f us)" % (label, sum(rec), sum(spec), len(tr), float(np.median(tr)), sum(tr),
                                                                          float(np.median(old)) if old else 0.0))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--wall":
        wall(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "--kinds":
        kinds_runs()
    elif len(sys.argv) >= 3 and sys.argv[1] == "--parse":
        parse(sys.argv[2])
    else:
        sys.exit(__doc__)
