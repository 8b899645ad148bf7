"""GPU: first measurements of the zone statistics (PvAmdComputeZoneStats, csrc/pv_zones.hip) -> profiles/zone_stats.txt.

Per grid and kind (room metrics: 10 planes; band metrics with 8 bands: 96 planes) and per zone layout -- `full`: five strips
that cover the whole grid, `rects`: five rectangles that label about 42 % of it:
  zones   the device time of PvAmdComputeZoneStats (the `ms` out-parameter; median of 20 after 3 warm-ups) and the bytes its two
          walks LOAD: a map value is loaded only where the cell has a label and lies inside the history window, and the grids
          here are chosen so that the window is the whole grid (checked: PvAmdInfo histRows / histPitch) -- so 2 x planes x
          (labelled cells x 4 map bytes + cells x 1 label byte), of which the label bytes of all planes but the first are the
          same one map again; both the map bytes alone and the sum per second, against PvAmdBandwidthProbe's copy and read
          rates taken in the same process;
  copy    what the same numbers cost without it: the kind's whole-map read-back (PvAmdCopy<Kind>: device -> host copy and the
          tile-major gather; a fresh compute before each, so that no host copy is reused) plus a numpy reduction per zone and
          plane (count, mean, std, min, max of the finite members), wall time, median of 5 after 1 warm-up.
Both forms run in child processes of their own, alternating, each under its own time limit.  --copy-root DIR runs the `copy`
children on ANOTHER checkout of the package (the parent commit, built there): its code path is the one a caller had before.

    python tools/gpu_zone_stats_measure.py [out.txt] [--copy-root DIR]
    python tools/gpu_zone_stats_measure.py --one zones|copy GRID KIND
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)  # (behind PYTHONPATH: a `copy` child imports the package of --copy-root)
DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
THIRDS8 = [31.5, 40.0, 63.0, 100.0, 160.0, 250.0, 400.0, 500.0]  # eight third-octave bands below fs / 2 = 721 Hz
OPEN = float((1024 + 0.5) * DX)
# name: (scene or None, size in metres, resolution, options, listener, time limit of a child in seconds): the 25 m preset (70^2
# cells, T = 435) and an open 1024^2 grid, listener at its centre, with T = 600 -- 2 T + 3 cells exceed the grid, so the history
# window is the whole grid at both
GRIDS = {
    "smallroom25m": ("SmallRoomScene.pv", 25.0, 275, {}, (5.0, 0.0, 4.0), 240),
    "open1024": (None, OPEN, 275, dict(num_steps=600), (OPEN / 2, 0.0, OPEN / 2), 300),
}
KINDS = ("room_metrics", "band_metrics")
ZONES = 5


def rect_labels(gx, gy):
    """five rectangles: quadrant-sized, a thin strip, a block across the middle, a small block, the far corner"""
    lab = np.zeros((gx, gy), np.uint8)
    lab[gx // 16:gx // 2, gy // 16:gy // 2] = 1
    lab[gx // 2:gx // 2 + 4, :] = 2
    lab[gx // 3:2 * gx // 3, gy // 2 + 8:gy - 8] = 3
    lab[7:19, 5:30] = 4
    lab[3 * gx // 4:, 3 * gy // 4:] = 5
    return lab


def full_labels(gx, gy):
    """five strips of columns that cover the whole grid: every cell has a label, every strip crosses every row"""
    return np.broadcast_to((1 + np.arange(gy) * ZONES // gy).astype(np.uint8)[None, :], (gx, gy)).copy()


LAYOUTS = {"full": full_labels, "rects": rect_labels}


def setup(api, name):
    scene, size, res, opts, listener, _ = GRIDS[name]
    s = api.Solver(size, size, res, **opts)
    if scene:
        s.load_scene(os.path.join(ROOT, "tests", "scenes", scene))
    s.set_bands(THIRDS8, 3)
    s.run(listener)
    s.run(listener)
    if s.info.histRows < s.gx or s.info.histPitch < s.gy:
        raise RuntimeError("the history window (%d x %d) does not cover the grid: the loaded bytes would not be known" % (
            s.info.histRows, s.info.histPitch))
    return s


def numpy_reduction(m, lab):
    out = []
    flat = m.reshape(m.shape[0], m.shape[1], -1)
    for z in range(1, ZONES + 1):
        x = flat[lab == z].astype(np.float64)
        fin = np.isfinite(x)
        xz = np.where(fin, x, 0.0)
        n = fin.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = xz.sum(axis=0) / n
            std = np.sqrt((np.where(fin, x - mean, 0.0) ** 2).sum(axis=0) / n)
        out.append((n, mean, std, np.where(fin, x, np.inf).min(axis=0), np.where(fin, x, -np.inf).max(axis=0)))
    return out


def one(form, name, kind):
    from planeverb_amd import api
    if api.device_count() < 1:
        raise RuntimeError("needs a HIP device")
    probe = api.bandwidth_probe(0)
    with setup(api, name) as s:
        compute, read = getattr(s, "compute_" + kind), getattr(s, kind)
        compute_ms = compute()
        base = dict(form=form, grid=name, kind=kind, cells=[s.gx, s.gy], T=s.T, window=[s.info.histRows, s.info.histPitch],
                    bands=len(s.bands()[0]), zones=ZONES, compute_ms=round(compute_ms, 4))
        if form == "zones":
            for layout, make in LAYOUTS.items():
                lab = make(s.gx, s.gy)
                s.set_zones(lab, ZONES)
                ms = [s.zone_stats(kind, with_ms=True)[1] for _ in range(23)][3:]
                t0 = time.perf_counter()
                recs = s.zone_stats(kind)
                wall = (time.perf_counter() - t0) * 1e3
                planes = int(np.prod(recs.shape[1:]))
                labelled = int((lab != 0).sum())
                map_bytes, label_bytes = 2 * planes * labelled * 4, 2 * planes * s.gx * s.gy
                med = float(np.median(ms))
                rate = lambda b: b / (med * 1e-3) / 1e9  # noqa: E731
                print(json.dumps(dict(
                    base, layout=layout, planes=planes, labelled_share=round(labelled / (s.gx * s.gy), 4), zone_ms_median=round(med, 5),
                    zone_ms_min=round(float(np.min(ms)), 5), zone_ms_max=round(float(np.max(ms)), 5), call_wall_ms=round(wall, 4),
                    map_bytes_loaded=map_bytes, label_bytes_loaded=label_bytes, map_gb_per_s=round(rate(map_bytes), 2),
                    map_and_label_gb_per_s=round(rate(map_bytes + label_bytes), 2), probe_copy_x4_gb_per_s=round(probe["copy_x4"], 1),
                    probe_read_gb_per_s=round(probe["read_dword"], 1), map_share_of_probe_read=round(rate(map_bytes) / probe["read_dword"], 4),
                    map_and_label_share_of_probe_read=round(rate(map_bytes + label_bytes) / probe["read_dword"], 4),
                    n_finite_plane0=[int(v) for v in recs.reshape(ZONES, -1)["n_finite"][:, 0]])), flush=True)
        else:
            copy_ms, reduce_ms = [], dict((layout, []) for layout in LAYOUTS)
            labs = dict((layout, make(s.gx, s.gy)) for layout, make in LAYOUTS.items())
            for _ in range(6):
                compute()  # (a fresh device map: the read-back below is not served from the host copy)
                t0 = time.perf_counter()
                m = read()
                copy_ms.append((time.perf_counter() - t0) * 1e3)
                for layout, lab in labs.items():
                    t1 = time.perf_counter()
                    numpy_reduction(m, lab)
                    reduce_ms[layout].append((time.perf_counter() - t1) * 1e3)
            for layout in LAYOUTS:
                print(json.dumps(dict(base, layout=layout, planes=int(np.prod(m.shape[2:])), copy_ms_median=round(float(np.median(copy_ms[1:])), 3),
                                      numpy_ms_median=round(float(np.median(reduce_ms[layout][1:])), 3),
                                      total_ms_median=round(float(np.median(np.add(copy_ms, reduce_ms[layout])[1:])), 3))), flush=True)


def main():
    args = sys.argv[1:]
    if args[:1] == ["--one"]:
        one(*args[1:4])
        return 0
    copy_root = ROOT
    if "--copy-root" in args:
        i = args.index("--copy-root")
        copy_root = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "zone_stats.txt")
    lines = []
    for name, grid in GRIDS.items():
        for kind in KINDS:
            for form in ("zones", "copy", "zones", "copy"):  # alternating processes
                env = dict(os.environ, PYTHONPATH=copy_root if form == "copy" else ROOT)
                # every GPU step under a time limit of its own; nothing more is started on the device after one that failed
                r = subprocess.run(["timeout", "-k", "10", str(grid[-1]), sys.executable, os.path.abspath(__file__), "--one", form, name, kind],
                                   capture_output=True, text=True, env=env, cwd=copy_root if form == "copy" else ROOT)
                if r.returncode != 0:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.stderr.write("\n%s %s %s ended with status %d: stopping here\n" % (form, name, kind, r.returncode))
                    return r.returncode
                got = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
                lines += got
                print("\n".join(got), flush=True)
                with open(out, "w") as f:
                    f.write("# tools/gpu_zone_stats_measure.py: PvAmdComputeZoneStats on one MI355X against the whole-map read-back + numpy"
                            "%s\n" % (" (copy: the parent commit's build)" if copy_root != ROOT else ""))
                    f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
