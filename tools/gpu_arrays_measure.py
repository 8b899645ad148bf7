"""GPU: measurements of the source-array pass (PvAmdComputeArrays, csrc/pv_arrays.hip): the runs that profiles/source_arrays.txt quotes.

Every figure of the pass is DEVICE time as the call reports it (*ms: a pair of events on the solver's stream around the member-table
launch, the mix, the onsets and the record launches), the median of 20 calls after 3 warm-ups in one process, with the smallest and
largest sample next to it.
  smallroom70     SmallRoomScene at 70^2, T = 435: 8 arrays x 8 members, no kinds and all six
  shoebox512      Shoebox 25 m at 512^2, T = 3179: 64 arrays x 16 members, no kinds and all six.  Beside it the only route to the
                  same mix there was before: reading the 1024 member responses back with PvAmdGetImpulseResponse (a launch and a
                  synchronisation each), WALL time of the 1024 calls, the host mixing not counted; and the wall time of one
                  PvAmdComputeArrays call with no kinds selected (the bar compares wall with wall)
  hugeroom4096    HugeRoom 25 m at 4096^2, T = 25 432, sparse-emitter mode: 16 arrays x 4 members off the emitter traces

    python tools/gpu_arrays_measure.py [out.txt]    every case, one child process each under its own time limit; a case that fails
                                                    is listed as not measured and nothing more is started after it; writes
                                                    profiles/source_arrays.txt (or out.txt)
    python tools/gpu_arrays_measure.py --one NAME   one case, one JSON line
    python tools/gpu_arrays_measure.py --render LINES.jsonl [out.txt]   the same file from JSON lines kept from a run (no GPU)
"""
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
BANDS, BINS = (63.0, 125.0), (31.5, 100.0, 250.0)
# name: (scene, size in metres, resolution, sparse-emitter mode, arrays, members per array, time limit of the child in seconds)
CASES = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, False, 8, 8, 120),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, False, 64, 16, 300),
    "hugeroom4096": ("HugeRoom.pv", 25.0, 16067, True, 16, 4, 420),
}


def stats(samples):
    return dict(median=round(float(np.median(samples)), 5), min=round(float(np.min(samples)), 5), max=round(float(np.max(samples)), 5))


def one(name, runs=20, warm=3):
    from planeverb_amd import api
    scene, size, res, sparse, n_arrays, n_members, _ = CASES[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    rng = np.random.default_rng(64)
    with api.Solver(size, size, res, **(dict(streaming_analysis=1) if sparse else {})) as s:
        s.load_scene(os.path.join(SCENES, scene))
        total = n_arrays * n_members
        if sparse:  # the members on a 1 m lattice: the registered emitters
            pos = [(2.0 + 1.0 * (i % 8), 0.0, 2.0 + 1.0 * (i // 8)) for i in range(total)]
            s.set_emitters(pos)
            cells = None
        s.run(L)
        if not sparse:
            idx = np.argwhere(s.results()[1] < 1e30)
            cells = idx[rng.permutation(len(idx))[:total]]
            pos = [((x + 0.5) * s.dx, 0.0, (y + 0.5) * s.dx) for x, y in cells]
        # gains in [-1, 1], delays up to 30 ms, two in three fractional (four taps)
        members = [(p, float(rng.uniform(-1, 1)), 0.0 if i % 3 == 0 else float(rng.uniform(1.01, 0.03 * s.fs)) / s.fs) for i, p in enumerate(pos)]
        s.set_arrays([members[a * n_members:(a + 1) * n_members] for a in range(n_arrays)])
        taps = sum(len(s.array_taps(a)[0]) for a in range(n_arrays))
        s.set_bands(BANDS, 1)
        s.set_spectrum_bins(BINS)
        rec = dict(case=name, cells=[s.gx, s.gy], T=s.T, sparse_emitters=sparse, arrays=n_arrays, members=n_members, taps=taps, passes=[])
        for label, tk, sk in (("no kinds", 0, 0), ("all six kinds", api.QREC_ROOM_METRICS | api.QREC_DECAY_TIMES | api.QREC_ECHO_CRITERION, api.QSPEC_ALL)):
            s.set_array_records(tk, sk)
            ms, wall = [], []
            for _ in range(warm + runs):
                t0 = time.perf_counter()
                ms.append(s.compute_arrays())
                wall.append((time.perf_counter() - t0) * 1e3)
            on = s.array_onsets()
            rec["passes"].append(dict(kinds=label, with_onset=int((on < 1e30).sum()), device_ms=stats(ms[warm:]), wall_ms=stats(wall[warm:])))
        if name == "shoebox512":  # the route there was before: one read-back per member
            wall = []
            for _ in range(1 + 3):
                t0 = time.perf_counter()
                for x, y in cells:
                    s.impulse_response(int(x), int(y))
                wall.append((time.perf_counter() - t0) * 1e3)
            rec["readback_of_the_members_wall_ms"] = stats(wall[1:])
    print(json.dumps(rec), flush=True)
    return rec


HEAD = """Source-array pass (PvAmdComputeArrays, csrc/pv_arrays.hip, DESIGN.md 4.28).
Written by tools/gpu_arrays_measure.py on one MI355X, one process per case.  device: what the call reports in *ms -- a pair of events
on the solver's stream around the member-table launch, the mix, the onsets and the record launches --; wall: time.perf_counter()
around the whole call, the copies of the onsets and the records to the host included; each the median (min .. max) of 20 calls after
3 warm-ups in that process.  Listener (5, 0, 4); members on a history solver: random reached cells (seed 64), in sparse-emitter mode
the registered emitters of a 1 m lattice; gains in [-1, 1], one delay in three 0, the others fractional up to 30 ms (four taps);
kinds: room metrics, decay times, echo criterion, band metrics and modulation of two bands, spectrum at three bins.
The only bar set in advance: at 512^2 with no kinds selected the call takes less WALL time than reading the 1024 member responses
back with PvAmdGetImpulseResponse (a launch and a synchronisation each; median of 3 rounds after 1 warm-up; the host mixing that
route also needs is not counted).  PvAmdGetImpulseResponse and its kernel are the parent commit's, unchanged by this work.
"""
TAIL = """Not measured: a kernel trace or counters (the mix apart from the member table and the onsets; bytes fetched per tap in history
mode, where a wave's load touches 64 lines); 256 arrays x 64 members; T = 25 432 on a history solver; PvAmdCopyArrayResponse
(a strided copy of T words); the setter's time.
Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / waves per SIMD): pv_array_rows_kernel 14 / 42 / 8,
pv_array_mix_kernel 6 / 30 / 8, pv_array_onsets_kernel 4 / 21 / 8: no scratch, no LDS, no AGPRs; the mix form of
pv_query_records_kernel 112 / 78 / 4 (LDS 1280 B) and of pv_query_spectral_kernel 157 / 106 / 3 (LDS 768 B): no scratch.
"""


def fmt(st):
    return "%9.4f ms  (%.4f .. %.4f)" % (st["median"], st["min"], st["max"])


def write_profile(out, lines):
    """profiles/source_arrays.txt from the children's JSON lines"""
    with open(out, "w") as f:
        f.write(HEAD + "\n")
        for line in lines:
            r = json.loads(line)
            if "not_measured" in r:
                f.write("%s: NOT MEASURED (%s)\n" % (r["case"], r["not_measured"]))
                continue
            f.write("%s: %d x %d cells, T = %d%s: %d arrays x %d members, %d taps\n" % (
                r["case"], r["cells"][0], r["cells"][1], r["T"], ", sparse-emitter mode" if r["sparse_emitters"] else "", r["arrays"],
                r["members"], r["taps"]))
            for p in r["passes"]:
                f.write("  %-14s (%d arrays with an onset)  device %s   wall %s\n" % (p["kinds"], p["with_onset"], fmt(p["device_ms"]), fmt(p["wall_ms"])))
            e = r.get("readback_of_the_members_wall_ms")
            if e:
                first = r["passes"][0]["wall_ms"]["median"]
                f.write("  PvAmdGetImpulseResponse x %d, wall  %s\n" % (r["arrays"] * r["members"], fmt(e)))
                f.write("  the bar (the call with no kinds < the read-backs, wall): %s, a factor of %.0f\n" % ("met" if first < e["median"] else "MISSED", e["median"] / first))
        f.write("\n" + TAIL + "\nThe children's lines:\n" + "\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    default = os.path.join(ROOT, "profiles", "source_arrays.txt")
    if len(sys.argv) > 2 and sys.argv[1] == "--render":
        with open(sys.argv[2]) as f:
            write_profile(sys.argv[3] if len(sys.argv) > 3 else default, [ln.strip() for ln in f if ln.startswith("{")])
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else default
    lines = []
    for name, case in CASES.items():
        # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
        r = subprocess.run(["timeout", "-k", "10", str(case[-1]), sys.executable, os.path.abspath(__file__), "--one", name],
                           capture_output=True, text=True)
        ok = r.returncode == 0
        lines.append(r.stdout.strip().splitlines()[-1] if ok else json.dumps(dict(case=name, not_measured="ended with status %d" % r.returncode)))
        print(lines[-1], flush=True)
        write_profile(out, lines)
        if not ok:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write("\n%s ended with status %d: stopping here\n" % (name, r.returncode))
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
