"""GPU: measurements of the waterfall pass (PvAmdComputeWaterfall, csrc/pv_waterfall.hip): the runs that profiles/waterfall.txt quotes.

Every figure is DEVICE time of the pass as the call reports it (*ms: a pair of events on the solver's stream around the receiver
table's launch and the pass's launch), the median of 20 calls after 3 warm-ups in one process, with the smallest and largest
sample next to it.
  smallroom70     SmallRoomScene at 70^2, T = 435: 8 receivers x 64 bins x 16 slices
  shoebox512      Shoebox 25 m at 512^2, T = 3179: 64 receivers x 256 bins x 16 slices, and 256 x 512 x 64.  Beside it what the
                  library offered for slice 0 of the same 256 bins before this pass: eight rounds of PvAmdSetSpectrumBins (32 bins)
                  + PvAmdComputeSpectrum, the sum of the eight passes' own device times (the tables' upload is not in it)
  hugeroom4096    HugeRoom 25 m at 4096^2, T = 25 432, sparse-emitter mode, 64 emitters: 256 bins x 16 slices off the emitter traces

    python tools/gpu_waterfall_measure.py [out.txt]    every case, one child process each under its own time limit; a case that
                                                       fails is listed as not measured and nothing more is started after it;
                                                       writes profiles/waterfall.txt (or out.txt): the text below, a line per
                                                       figure and the children's JSON lines
    python tools/gpu_waterfall_measure.py --one NAME   one case, one JSON line
    python tools/gpu_waterfall_measure.py --render LINES.jsonl [out.txt]   the same file from JSON lines kept from a run (no GPU)
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
# name: (scene, size in metres, resolution, sparse-emitter mode, [(receivers, bins, slices)], time limit of the child in seconds)
CASES = {
    "smallroom70": ("SmallRoomScene.pv", 25.0, 275, False, [(8, 64, 16)], 120),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, False, [(64, 256, 16), (256, 512, 64)], 300),
    "hugeroom4096": ("HugeRoom.pv", 25.0, 16067, True, [(64, 256, 16)], 420),
}
EMITTERS64 = [(2.0 + 1.0 * i, 0.0, 2.0 + 1.0 * j) for i in range(8) for j in range(8)]


def stats(samples):
    return dict(median=round(float(np.median(samples)), 5), min=round(float(np.min(samples)), 5), max=round(float(np.max(samples)), 5))


def one(name, runs=20, warm=3):
    from planeverb_amd import api
    scene, size, res, sparse, shapes, _ = CASES[name]
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    with api.Solver(size, size, res, **(dict(streaming_analysis=1) if sparse else {})) as s:
        s.load_scene(os.path.join(SCENES, scene))
        if sparse:
            s.set_emitters(EMITTERS64)
        s.run(L)
        rec = dict(case=name, cells=[s.gx, s.gy], T=s.T, sparse_emitters=sparse, passes=[])
        if not sparse:
            delay = s.results()[1]
            idx = np.argwhere(delay < 1e30)
            order = np.random.default_rng(64).permutation(len(idx))
        for nrx, n, m in shapes:
            hz = np.linspace(20.0, s.fs / 8.0, n).astype(np.float32)
            s.set_waterfall(hz, 0.02, m)
            pos = None if sparse else [((x + 0.5) * s.dx, 0.0, (y + 0.5) * s.dx) for x, y in idx[order[:nrx]]]
            ms = [s.compute_waterfall(pos) for _ in range(warm + runs)][warm:]
            w = s.waterfall()
            rec["passes"].append(dict(receivers=int(w["onset"].shape[0]), with_onset=int(np.isfinite(w["onset"]).sum()), bins=n, slices=m,
                                      device_ms=stats(ms)))
            if (nrx, n) == (64, 256) and not sparse:  # slice 0 of the same bins by the whole-map spectrum: eight passes of 32 bins
                tot = []
                for _ in range(warm + 5):
                    t = 0.0
                    for k in range(0, n, 32):
                        s.set_spectrum_bins(hz[k:k + 32])
                        t += s.compute_spectrum()
                    tot.append(t)
                rec["eight_spectrum_passes_of_32_bins_device_ms"] = stats(tot[warm:])
                s.set_spectrum_bins([])
    print(json.dumps(rec), flush=True)
    return rec


HEAD = """Waterfall pass (PvAmdComputeWaterfall, csrc/pv_waterfall.hip, DESIGN.md 4.27): device time of the pass.
Written by tools/gpu_waterfall_measure.py on one MI355X, one process per case.  Every figure is what the call reports in *ms -- a
pair of events on the solver's stream around the receiver-table launch and the pass's launch -- as the median (min .. max) of 20
calls after 3 warm-ups in that process.  Listener (5, 0, 4); receivers on a history solver: random reached cells (seed 64); in
sparse-emitter mode the 64 emitters of the 1 m lattice (2 .. 9 m)^2, samples off their traces; bins np.linspace(20, fs / 8, n);
slices of 0.02 s.  The only bar set in advance: at 512^2 the pass over 64 receivers x 256 bins takes less device time than what the
library offered before for slice 0 of the same bins, eight rounds of PvAmdSetSpectrumBins (32 bins) + PvAmdComputeSpectrum (the sum
of the eight passes' own device times, median of 5 rounds after 3 warm-ups; the table uploads are not in it).
"""
TAIL = """Not measured: a kernel trace or counters of the pass (the receiver-table kernel apart from the pass, twiddle bytes fetched, VALU
busy); other receivers-per-wave choices than the launcher's at these shapes; T = 25 432 with 512 bins (the 104 MB table); the
setter's time (host trigonometry in double and the upload); 8192^2.
Registers (-Rpass-analysis=kernel-resource-usage, gfx950; VGPRs / SGPRs / waves per SIMD): pv_waterfall_kernel<1> 47 / 53 / 8,
<2> 57 / 74 / 8, <4> 78 / 94 / 6; pv_waterfall_receivers_kernel 18 / 41 / 8; no scratch, no LDS, no AGPRs.
"""


def fmt(st):
    return "%9.4f ms  (%.4f .. %.4f)" % (st["median"], st["min"], st["max"])


def write_profile(out, lines):
    """profiles/waterfall.txt from the children's JSON lines"""
    with open(out, "w") as f:
        f.write(HEAD + "\n")
        for line in lines:
            r = json.loads(line)
            if "not_measured" in r:
                f.write("%s: NOT MEASURED (%s)\n" % (r["case"], r["not_measured"]))
                continue
            f.write("%s: %d x %d cells, T = %d%s\n" % (r["case"], r["cells"][0], r["cells"][1], r["T"],
                                                      ", sparse-emitter mode" if r["sparse_emitters"] else ""))
            for p in r["passes"]:
                f.write("  %4d receivers (%d with an onset) x %3d bins x %2d slices  %s\n" % (
                    p["receivers"], p["with_onset"], p["bins"], p["slices"], fmt(p["device_ms"])))
            e = r.get("eight_spectrum_passes_of_32_bins_device_ms")
            if e:
                first = r["passes"][0]["device_ms"]["median"]
                f.write("  eight spectrum passes of 32 bins, every cell of the window  %s\n" % fmt(e))
                f.write("  the bar (pass < eight spectrum passes): %s, a factor of %.0f\n" % ("met" if first < e["median"] else "MISSED", e["median"] / first))
        f.write("\n" + TAIL + "\nThe children's lines:\n" + "\n".join(lines) + "\n")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(sys.argv[2])
        return 0
    default = os.path.join(ROOT, "profiles", "waterfall.txt")
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
