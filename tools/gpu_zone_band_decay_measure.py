"""GPU: first measurements of the zone band decay (PvAmdComputeZoneBandDecay, csrc/pv_zone_band_decay.hip) ->
profiles/zone_band_decay.txt.

Per grid (the three scenes of profiles/zone_decay.txt), zone layout (`one`, `full`, `scattered`: tools/gpu_zone_decay_measure.py),
alignment and number of octave bands (1, 2 and 8, from 500 Hz downwards, where the grid's fs allows them):
  bands   the device time of PvAmdComputeZoneBandDecay (the `ms` out-parameter; median of 20 after 3 warm-ups), the wall time of a
          call with both curves, the chunks the pass took, and the history bytes a band group has to load (sum over the labelled
          cells with an onset of (T - t0) x 4 bytes) times the band groups, per second.  Where a call takes more than one chunk
          or more than one band, band 0 of the result is compared bit for bit with a one-band call (another dealing of the work);
  parts   on the PARENT's build, the two existing passes the new one is made of: PvAmdComputeZoneDecay (the loads and the
          butterflies, no filter) per layout and alignment, and PvAmdComputeBandMetrics (the filter, every reached cell, no
          reduction) per number of bands;
  copy    on the PARENT's build, the only route a caller had: reading back all T history planes (PvAmdCopyHistoryPlane) and the
          onset map -- the wall time of the read-back alone is the figure the new pass is held against -- and, on the 70^2 grid,
          the host side behind it for one band and one zone: the filter in numpy over all cells at once and the per-slot sums.
Every form runs in child processes of its own, alternating, each under its own time limit.  --parent-root DIR names the parent
commit's checkout, built there (default: this checkout, for a dry run).

    python tools/gpu_zone_band_decay_measure.py [out.txt] [--parent-root DIR]
    python tools/gpu_zone_band_decay_measure.py --one bands|parts|copy GRID
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (behind PYTHONPATH: a `parts` or `copy` child imports the package of --parent-root)
from gpu_zone_decay_measure import ALIGNS, GRIDS, LAYOUTS, NO_ONSET, setup  # noqa: E402

BAND_LAYOUTS = ("one", "full", "scattered")
OCTAVES8 = [500.0 / 2 ** k for k in range(8)]
BAND_COUNTS = (1, 2, 8)


def band_sets(fs):
    ok = [hz for hz in OCTAVES8 if hz * 2 ** 0.5 < 0.5 * fs]
    return [ok[:n] for n in BAND_COUNTS if n <= len(ok)]


def filter_all(p, delay, coefs):
    """the band filter over every cell of the read-back planes at once (float32, backwards, no step below an onset) and the
    per-slot sums of the squares: what a caller without the pass computes (one zone, ABSOLUTE)"""
    T = len(p)
    t0 = np.where(delay != NO_ONSET, delay, T).astype(np.int64)
    etc = np.zeros((len(coefs), T))
    for b, c in enumerate(coefs):
        z = [np.zeros(delay.shape, np.float32) for _ in range(4)]
        for t in range(T - 1, -1, -1):
            on = t >= t0
            v = p[t]
            for s in (0, 1):
                b0, b1, b2, a1, a2 = c[5 * s:5 * s + 5]
                y = b0 * v + z[2 * s]
                n1 = (b1 * v - a1 * y) + z[2 * s + 1]
                n2 = b2 * v - a2 * y
                z[2 * s], z[2 * s + 1] = np.where(on, n1, z[2 * s]), np.where(on, n2, z[2 * s + 1])
                v = y
            etc[b, t] = (np.where(on, v, 0).astype(np.float64) ** 2).sum()
    return etc


def one(form, name):
    from planeverb_amd import api
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    probe = api.bandwidth_probe(0)
    with setup(api, name) as s:
        delay = s.results()[1]
        reached = delay != NO_ONSET
        base = dict(form=form, grid=name, cells=[s.gx, s.gy], T=s.T, fs=s.fs, reached=int(reached.sum()))
        if form == "bands":
            for layout in BAND_LAYOUTS:
                make, nz = LAYOUTS[layout]
                lab = make(s.gx, s.gy)
                s.set_zones(lab, nz)
                member = (lab != 0) & reached
                hist_bytes = int(((s.T - delay[member].astype(np.int64)) * 4).sum())
                for hz in band_sets(s.fs):
                    for align in ALIGNS:
                        s.set_bands(hz)
                        ms = [s.zone_band_decay(align, with_ms=True)[1] for _ in range(23)][3:]
                        t0 = time.perf_counter()
                        rec, etc, edc = s.zone_band_decay(align, curves=True)
                        wall = (time.perf_counter() - t0) * 1e3
                        chunks, _, per = s.zone_band_decay_chunk()
                        same = None
                        if len(hz) > 1:
                            s.set_bands(hz[:1])
                            same = bool(np.array_equal(s.zone_band_decay(align, curves=True)[1][:, 0].view(np.uint64), etc[:, 0].view(np.uint64)))
                        med = float(np.median(ms))
                        groups = (len(hz) + 1) // 2
                        rate = hist_bytes * groups / (med * 1e-3) / 1e9
                        print(json.dumps(dict(
                            base, layout=layout, zones=nz, bands=len(hz), align=align, chunks=chunks, bands_per_chunk=per,
                            members=int(member.sum()), ms_median=round(med, 5), ms_min=round(float(np.min(ms)), 5),
                            ms_max=round(float(np.max(ms)), 5), ms_per_band=round(med / len(hz), 5), call_wall_ms=round(wall, 4),
                            history_bytes=hist_bytes, band_groups=groups, loaded_gb_per_s=round(rate, 2),
                            probe_read_gb_per_s=round(probe["read_dword"], 1), band0_same_as_one_band_call=same,
                            t30=[round(float(v), 5) for v in rec["t30"][:, 0]])), flush=True)
        elif form == "parts":
            for layout in BAND_LAYOUTS:
                make, nz = LAYOUTS[layout]
                s.set_zones(make(s.gx, s.gy), nz)
                for align in ALIGNS:
                    ms = [s.zone_decay(align, with_ms=True)[1] for _ in range(23)][3:]
                    print(json.dumps(dict(base, part="zone_decay", layout=layout, zones=nz, align=align,
                                          ms_median=round(float(np.median(ms)), 5))), flush=True)
            for hz in band_sets(s.fs):
                s.set_bands(hz)
                ms = [s.compute_band_metrics() for _ in range(23)][3:]
                print(json.dumps(dict(base, part="band_metrics", bands=len(hz), ms_median=round(float(np.median(ms)), 5))), flush=True)
        else:
            t0 = time.perf_counter()
            planes = [s.history_plane(t)[:s.gx, :s.gy] for t in range(s.T)]
            delay = s.results()[1]
            copy_ms = (time.perf_counter() - t0) * 1e3
            row = dict(base, readback_ms=round(copy_ms, 2))
            if s.gx * s.gy * s.T < 1 << 22:  # (the 70^2 grid: the host side behind the read-back, one band)
                s.set_bands(OCTAVES8[:1])
                t1 = time.perf_counter()
                filter_all(np.stack(planes), delay, s.band_coefs())
                row["numpy_filter_one_band_ms"] = round((time.perf_counter() - t1) * 1e3, 2)
            print(json.dumps(row), flush=True)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--one"]:
        one(*args[1:3])
        return 0
    parent = ROOT
    if "--parent-root" in args:
        i = args.index("--parent-root")
        parent = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "zone_band_decay.txt")
    lines = []
    for name, grid in GRIDS.items():
        for form in ("bands", "copy", "parts", "bands", "copy", "parts"):  # two processes each, alternating
            root = ROOT if form == "bands" else parent
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([root, os.path.join(ROOT, "tools")]))
            # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
            r = subprocess.run(["timeout", "-k", "10", str(grid[-1]), sys.executable, os.path.abspath(__file__), "--one", form, name],
                               capture_output=True, text=True, env=env, cwd=root)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.stderr.write("\n%s %s ended with status %d: stopping here\n" % (form, name, r.returncode))
                return r.returncode
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            lines += got
            print("\n".join(got), flush=True)
            with open(out, "w") as f:
                f.write("# tools/gpu_zone_band_decay_measure.py: PvAmdComputeZoneBandDecay on one MI355X; parts and copy: %s\n"
                        % ("the parent commit's build" if parent != ROOT else "this build"))
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
