"""Times the two convolution kernels of the auralisation (PvAmdAuralise: PVA_AURAL_TILED against PVA_AURAL_PLAIN, csrc/pv_aural.hip)
in one process on one GPU, at the two shapes DESIGN.md 4.29 names, and prints what profiles/aural.txt holds.

    python tools/gpu_aural_measure.py [--reps 10] > profiles/aural.txt

device: what the call reports in *ms -- a pair of events on the solver's stream around the convolution and the mix --, the median
(min .. max) of --reps calls after 2 warm-ups, the two forms alternating call by call.  The shader clock is PvAmdClockProbe's,
taken before and after the timed calls; the bound is two VALU lane-operations (a multiply and an add) per output-tap on the device's
compute units x 4 SIMDs x 32 lanes per cycle (a wave's VALU instruction issues over two cycles) at that clock."""
import argparse
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from planeverb_amd import api  # noqa: E402


def unique_id():
    try:
        out = subprocess.run(["rocm-smi", "--showuniqueid"], capture_output=True, text=True, timeout=60).stdout
        ids = [ln.split(":")[-1].strip() for ln in out.splitlines() if ln.startswith("GPU[") and "Unique ID" in ln]
        return ids[0] if ids else "unknown"
    except Exception:  # noqa: BLE001
        return "unknown"


def compute_units():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:  # noqa: BLE001
        return 256


def stats(v):
    return "%9.4f ms  (%.4f .. %.4f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    cus = compute_units()
    B, C = api.aural_shape()
    print("Auralisation, the convolution (PvAmdAuralise, csrc/pv_aural.hip, DESIGN.md 4.29): tiled (%d outputs per one-wave block, %d taps "
          "per chunk) against plain (one lane per output, global loads)." % (B, C))
    print("Written by tools/gpu_aural_measure.py on one MI355X, unique_id %s, %d compute units, one process." % (unique_id(), cus))
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g71_smallroom.npz"))
    with api.Solver(float(g["size"]), float(g["size"]), int(g["res"])) as s:
        for b in g["boxes"]:
            s.add_geometry(b)
        s.run(tuple(g["listener"]))
        delay = s.results()[1]
        reached = np.argwhere(delay < 1e30)
        rng = np.random.default_rng(48)
        for R, rate, N in ((64, 48000, 48000), (16, 8000, 8000)):
            cells = reached[rng.choice(len(reached), R, replace=False)]
            pos = [((c[0] + 0.5) * s.dx, 0.0, (c[1] + 0.5) * s.dx) for c in cells]
            s.set_auralisation(rate, 16, 9.0)
            _, _, _, L, K = s.auralisation_setting()
            ms_resp = s.compute_aural_responses(pos)
            x = rng.standard_normal((3, N)).astype(np.float32)
            route = (np.arange(R) % 3).astype(np.int32)
            gain = np.ones(R, np.float32)
            M = N + L - 1
            # the terms the definition forms: per output min(L - 1, m) - max(0, m - N + 1) + 1
            m = np.arange(M, dtype=np.int64)
            taps = int((np.minimum(L - 1, m) - np.maximum(0, m - N + 1) + 1).sum()) * R
            mhz0 = api.clock_probe(0)[0]
            t = {api.AURAL_TILED: [], api.AURAL_PLAIN: []}
            mixes = {}
            for i in range(a.reps + 2):
                for form in t:
                    s.set_aural_form(form)
                    ms = s.auralise(x, route, gain)
                    if i >= 2:
                        t[form].append(ms)
                    mixes[form] = s.aural_mix()
            mhz1 = api.clock_probe(0)[0]
            same = np.array_equal(mixes[api.AURAL_TILED].view(np.uint32), mixes[api.AURAL_PLAIN].view(np.uint32))
            mhz = 0.5 * (mhz0 + mhz1)
            bound = cus * 4 * 32 * mhz * 1e6 / 2.0  # (a SIMD retires 32 lanes per cycle: a wave's VALU instruction takes two)
            print("\nR = %d receivers, rate = %d, N = %d, L = %d, K = %d, M = %d: %.4g output-taps; responses (gather + resample) %.4f ms"
                  % (R, rate, N, L, K, M, taps, ms_resp))
            print("  shader clock %.0f MHz before, %.0f MHz after; bound at two VALU lane-operations per output-tap: %.4g output-taps/s"
                  % (mhz0, mhz1, bound))
            for form, name in ((api.AURAL_TILED, "tiled"), (api.AURAL_PLAIN, "plain")):
                med = float(np.median(t[form]))
                print("  %s  device %s   %.4g output-taps/s   %.1f %% of the bound"
                      % (name, stats(t[form]), taps / (med * 1e-3), 100.0 * taps / (med * 1e-3) / bound))
            print("  tiled / plain: %.3f; the two mixes bit-equal: %s" % (float(np.median(t[api.AURAL_TILED])) / float(np.median(t[api.AURAL_PLAIN])), same))
        s.set_aural_form(api.AURAL_TILED)
        s.set_auralisation(0)


if __name__ == "__main__":
    main()
