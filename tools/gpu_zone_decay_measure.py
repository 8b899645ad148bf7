"""GPU: first measurements of the zone decay (PvAmdComputeZoneDecay, csrc/pv_zone_decay.hip) -> profiles/zone_decay.txt.

Per grid, zone layout and alignment (absolute, onset):
  zones   the device time of PvAmdComputeZoneDecay (the `ms` out-parameter; median of 20 after 3 warm-ups), the wall time of a
          call with both curves, and the history bytes the pass has to LOAD: a sample is loaded only for a labelled cell with an
          onset, from its onset on -- sum over those cells of (T - t0) x 4 bytes -- per second, against PvAmdBandwidthProbe's read
          rate taken in the same process.  Layouts: `full` (five strips of columns that cover the grid) and `rects` (five
          rectangles, about 42 % of it), those of tools/gpu_zone_stats_measure.py; and two that hold the bytes of `full` and change
          only the number of labels a 64-cell block holds, i.e. the butterflies per block and slot: `one` (a single zone: one)
          and `scattered` (five labels at random: five).  Time that follows the labels per block at equal bytes is the
          butterflies'; time that follows the bytes is the loads';
  copy    what the same curves cost without the pass: reading back all T history planes (PvAmdCopyHistoryPlane) and the onset map,
          plus a numpy reduction per plane (float64 squares, masked below the onset, one bincount per plane over label -- and over
          label x slot for `onset`), wall time, one pass each (`full` and `rects` only).
Both forms run in child processes of their own, alternating, each under its own time limit.  --copy-root DIR runs the `copy`
children on ANOTHER checkout of the package (the parent commit, built there): its code path is the one a caller had before.

    python tools/gpu_zone_decay_measure.py [out.txt] [--copy-root DIR]
    python tools/gpu_zone_decay_measure.py --one zones|copy GRID
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (behind PYTHONPATH: a `copy` child imports the package of --copy-root)
from gpu_zone_stats_measure import DX, ZONES, full_labels, rect_labels  # noqa: E402

OPEN = float((1024 + 0.5) * DX)
NO_ONSET = np.float32(np.finfo(np.float32).max)
# name: (scene or None, size in metres, resolution, options, listener, time limit of a child in seconds): the 25 m preset (70^2,
# T = 435), an open 1024^2 grid with T = 600, and Shoebox.pv as the real 25 m room at 512^2 (T = 3179: a 1.3 GB history in the room)
GRIDS = {
    "smallroom25m": ("SmallRoomScene.pv", 25.0, 275, {}, (5.0, 0.0, 4.0), 240),
    "open1024": (None, OPEN, 275, dict(num_steps=600), (OPEN / 2, 0.0, OPEN / 2), 420),
    "shoebox512": ("Shoebox.pv", 25.0, 2009, {}, (5.0, 0.0, 4.0), 420),
}
ALIGNS = ("absolute", "onset")


def one_label(gx, gy):
    return np.ones((gx, gy), np.uint8)


def scattered_labels(gx, gy):
    return np.random.default_rng(gx).integers(1, ZONES + 1, (gx, gy)).astype(np.uint8)


LAYOUTS = {"full": (full_labels, ZONES), "rects": (rect_labels, ZONES), "one": (one_label, 1), "scattered": (scattered_labels, ZONES)}
COPY_LAYOUTS = ("full", "rects")


def setup(api, name):
    scene, size, res, opts, listener, _ = GRIDS[name]
    s = api.Solver(size, size, res, **opts)
    if scene:
        s.load_scene(os.path.join(ROOT, "tests", "scenes", scene))
    s.run(listener)
    s.run(listener)
    return s


def numpy_curves(planes, delay, lab, nz, align):
    """etc float64 [nz, T] from the read-back planes: what a caller without the pass computes"""
    T = len(planes)
    member = (lab != 0) & (delay != NO_ONSET)
    z = lab[member].astype(np.int64) - 1
    t0 = delay[member].astype(np.int64)
    etc = np.zeros(nz * T)
    for t, plane in enumerate(planes):
        sq = plane[member].astype(np.float64) ** 2
        live = t0 <= t
        slot = t if align == "absolute" else t - t0[live]
        etc += np.bincount(z[live] * T + slot, weights=sq[live], minlength=nz * T)
    etc = etc.reshape(nz, T)
    return etc, np.cumsum(etc[:, ::-1], axis=1)[:, ::-1]


def one(form, name):
    from planeverb_amd import api
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    probe = api.bandwidth_probe(0)
    with setup(api, name) as s:
        delay = s.results()[1]
        reached = delay != NO_ONSET
        base = dict(form=form, grid=name, cells=[s.gx, s.gy], T=s.T, fs=s.fs, reached=int(reached.sum()))
        if form == "zones":
            for layout, (make, nz) in LAYOUTS.items():
                lab = make(s.gx, s.gy)
                s.set_zones(lab, nz)
                member = (lab != 0) & reached
                hist_bytes = int(((s.T - delay[member].astype(np.int64)) * 4).sum())
                for align in ALIGNS:
                    ms = [s.zone_decay(align, with_ms=True)[1] for _ in range(23)][3:]
                    t0 = time.perf_counter()
                    rec, etc, edc = s.zone_decay(align, curves=True)
                    wall = (time.perf_counter() - t0) * 1e3
                    med = float(np.median(ms))
                    rate = hist_bytes / (med * 1e-3) / 1e9
                    print(json.dumps(dict(
                        base, layout=layout, zones=nz, align=align, chunk_slots=s.zone_decay_chunk_slots(), members=int(member.sum()),
                        zone_ms_median=round(med, 5), zone_ms_min=round(float(np.min(ms)), 5), zone_ms_max=round(float(np.max(ms)), 5),
                        call_wall_ms=round(wall, 4), history_bytes=hist_bytes, history_gb_per_s=round(rate, 2),
                        probe_read_gb_per_s=round(probe["read_dword"], 1), share_of_probe_read=round(rate / probe["read_dword"], 4),
                        t30=[round(float(v), 5) for v in rec["t30"]], n_cells=[int(v) for v in rec["n_cells"]])), flush=True)
        else:
            t0 = time.perf_counter()
            planes = [s.history_plane(t)[:s.gx, :s.gy] for t in range(s.T)]
            delay = s.results()[1]
            copy_ms = (time.perf_counter() - t0) * 1e3
            for layout in COPY_LAYOUTS:
                make, nz = LAYOUTS[layout]
                lab = make(s.gx, s.gy)
                for align in ALIGNS:
                    t1 = time.perf_counter()
                    numpy_curves(planes, delay, lab, nz, align)
                    reduce_ms = (time.perf_counter() - t1) * 1e3
                    print(json.dumps(dict(base, layout=layout, zones=nz, align=align, copy_ms=round(copy_ms, 2), numpy_ms=round(reduce_ms, 2),
                                          total_ms=round(copy_ms + reduce_ms, 2))), flush=True)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--one"]:
        one(*args[1:3])
        return 0
    copy_root = ROOT
    if "--copy-root" in args:
        i = args.index("--copy-root")
        copy_root = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "zone_decay.txt")
    lines = []
    for name, grid in GRIDS.items():
        for form in ("zones", "copy", "zones", "copy"):  # alternating processes
            env = dict(os.environ, PYTHONPATH=os.pathsep.join([copy_root if form == "copy" else ROOT, os.path.join(ROOT, "tools")]))
            # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
            r = subprocess.run(["timeout", "-k", "10", str(grid[-1]), sys.executable, os.path.abspath(__file__), "--one", form, name],
                               capture_output=True, text=True, env=env, cwd=copy_root if form == "copy" else ROOT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.stderr.write("\n%s %s ended with status %d: stopping here\n" % (form, name, r.returncode))
                return r.returncode
            got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            lines += got
            print("\n".join(got), flush=True)
            with open(out, "w") as f:
                f.write("# tools/gpu_zone_decay_measure.py: PvAmdComputeZoneDecay on one MI355X against the read-back of all history planes + "
                        "numpy%s\n" % (" (copy: the parent commit's build)" if copy_root != ROOT else ""))
                f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
