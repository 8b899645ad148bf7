"""GPU: first measurements of the shape layer (profiles/shapes_geometry.txt).

A. PvAmdTimings.geometryMs of an iteration in which N boxes move, as oriented boxes (shapes) and as AABBs, at 1024^2 and 4096^2
   (Mode A, 275 Hz, open grid; runs of 24 steps without analysis, so that the figure is the geometry step's own).
B. Cell-update rate of HugeRoom.pv in a 4096^2 grid (bench.py's workload) with its walls as given (AABBs) and rotated by 30 degrees
   about the room's centre (oriented boxes), with the tiles that hold a wall cell (counted on the host from the material).

    python tools/gpu_shapes_measure.py [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planeverb_amd import api  # noqa: E402

DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)


def size_of(n):
    return float((n + 0.5) * DX)


def geometry_ms(n_cells, nbox, shapes, iters=6):
    size = size_of(n_cells)
    rng = np.random.default_rng(nbox)
    c = rng.uniform(0.05 * size, 0.95 * size, (nbox, 2))
    ang = rng.uniform(0, 2 * np.pi, nbox)
    out = []
    with api.Solver(size, size, 275, num_steps=24, skip_analysis=1) as s:
        ids = []
        for i in range(nbox):
            if shapes:
                ids.append(s.add_oriented_box(c[i, 0], c[i, 1], 3.0, 0.4, np.cos(ang[i]), np.sin(ang[i]), 0.5))
            else:
                ids.append(s.add_geometry((c[i, 0], c[i, 1], 3.0, 0.4, 0.5)))
        s.run((size / 2, 0.0, size / 2))
        for it in range(iters):
            for i in range(nbox):  # every box moves by half a metre and turns by 3 degrees
                c[i] += 0.5
                ang[i] += np.pi / 60
                if shapes:
                    s.update_oriented_box(ids[i], c[i, 0], c[i, 1], 3.0, 0.4, np.cos(ang[i]), np.sin(ang[i]), 0.5)
                else:
                    s.update_geometry(ids[i], (c[i, 0], c[i, 1], 3.0, 0.4, 0.5))
            s.run((size / 2, 0.0, size / 2))
            out.append(s.timings().geometryMs)
    return float(np.median(out)), [round(v, 3) for v in out]


def wall_tiles(beta, rows, cols):
    gx, gy = beta.shape[0] - 1, beta.shape[1] - 1
    wall = beta[:gx, :gy] == 0
    nx, ny = -(-gx // rows), -(-gy // cols)
    pad = np.zeros((nx * rows, ny * cols), bool)
    pad[:gx, :gy] = wall
    return int(pad.reshape(nx, rows, ny, cols).any(axis=(1, 3)).sum()), nx * ny


def rate(rotated, runs=4):
    size = size_of(4096)
    boxes = api.load_pv(os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv"))
    th = np.deg2rad(30.0)
    with api.Solver(size, size, 275) as s:
        if rotated:
            for x, y, w, h, a in boxes:
                dx, dy = x - 12.5, y - 12.5
                s.add_oriented_box(12.5 + dx * np.cos(th) - dy * np.sin(th), 12.5 + dx * np.sin(th) + dy * np.cos(th), w, h,
                                   np.cos(th), np.sin(th), a)
        else:
            for b in boxes:
                s.add_geometry(b)
        L = (12.5, 0.0, 12.5)
        s.run(L)
        ms = []
        for _ in range(runs):
            s.run(L)
            ms.append(s.timings().fdtdMs)
        beta, _ = s.material()
        wt, nt = wall_tiles(beta, s.info.tileRows, s.info.tileCols)
        f = float(np.median(ms))
        return dict(fdtd_ms=round(f, 3), cell_updates_per_s=float(s.gx) * s.gy * s.T / (f * 1e-3),
                    tiles_with_walls=wt, tiles=nt, tile=[s.info.tileRows, s.info.tileCols])


def main():
    out = dict(when=time.strftime("%Y-%m-%d %H:%M:%S"), geometry_ms={}, hugeroom_4096={})
    for n in (1024, 4096):
        for nbox in (1, 16, 256):
            for shapes in (True, False):
                key = "%d^2 %3d %s" % (n, nbox, "oriented boxes" if shapes else "AABBs")
                med, all_ = geometry_ms(n, nbox, shapes)
                out["geometry_ms"][key] = dict(median=round(med, 3), per_iteration=all_)
                print(key, "geometryMs median %.3f" % med, all_, flush=True)
    for rotated in (False, True):
        key = "walls rotated 30 deg (oriented boxes)" if rotated else "axis-aligned (AABBs)"
        out["hugeroom_4096"][key] = rate(rotated)
        print(key, out["hugeroom_4096"][key], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
