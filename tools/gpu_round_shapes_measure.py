"""GPU: the recompose launch's cost with the round and concave kinds (profiles/round_shapes.txt).

One scenario per process, so that a kernel trace of the process (rocprofv3 --kernel-trace --stats -- python
tools/gpu_round_shapes_measure.py SCENARIO N) gives pv_shape_compose_kernel's device time for that scenario alone:

    convex   16 oriented boxes (3.0 x 0.4 m), each moved by one cell per update        (exists before the round kinds: A/B)
    disc     one disc of radius 2 m, moved by one cell per update
    path     one wall path of 16 segments (about 2 m each, radius 0.3 m), moved by one cell per update
    polygon  one simple polygon of 64 vertices (radius 4 to 10 m), moved by one cell per update

N = cells per side (254, 4096); Mode A, 275 Hz, open grid, 40 updates, each followed by a run of 24 steps without analysis.
PLANEVERB_AMD_LIB selects another build of the library (a build without the round kinds can run `convex`).
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from planeverb_amd import api  # noqa: E402

DX = float(np.float32(343.21) / np.float32(275) / np.float32(3.5))
UPDATES = 40


def main():
    scenario, n = sys.argv[1], int(sys.argv[2])
    if os.environ.get("PLANEVERB_AMD_LIB"):  # (an older build: bind what it has)
        L = ctypes.CDLL(api.LIB_PATH)
        api.SYMBOLS = {k: v for k, v in api.SYMBOLS.items() if hasattr(L, k)}
    size = float((n + 0.5) * np.float32(DX))
    rng = np.random.default_rng(1)
    c0 = np.array([0.3 * size, 0.3 * size])
    with api.Solver(size, size, 275, num_steps=24, skip_analysis=1) as s:
        Lst = (size / 2, 0.0, size / 2)
        if scenario == "convex":
            c = c0 + rng.uniform(0, 0.3 * size, (16, 2))
            ang = rng.uniform(0, 2 * np.pi, 16)
            ids = [s.add_oriented_box(c[i, 0], c[i, 1], 3.0, 0.4, np.cos(ang[i]), np.sin(ang[i]), 0.5) for i in range(16)]
            move = lambda k: [s.update_oriented_box(ids[i], c[i, 0] + k * DX, c[i, 1] + k * DX, 3.0, 0.4, np.cos(ang[i]),
                                                    np.sin(ang[i]), 0.5) for i in range(16)]
        elif scenario == "disc":
            sid = s.add_disc(c0[0], c0[1], 2.0, 0.5)
            move = lambda k: s.update_disc(sid, c0[0] + k * DX, c0[1] + k * DX, 2.0, 0.5)
        elif scenario == "path":
            pts = np.cumsum(np.vstack([c0, rng.uniform(-1.0, 1.0, (16, 2)) + [1.5, 0.8]]), 0)
            sid = s.add_wall_path(pts, 0.3, 0.5)
            move = lambda k: s.update_wall_path(sid, pts + k * DX, 0.3, 0.5)
        elif scenario == "polygon":
            a = 2 * np.pi * (np.arange(64) + 0.4 * rng.uniform(0, 1, 64)) / 64
            rad = rng.uniform(4.0, 10.0, 64)
            pts = np.stack([c0[0] + 8 + rad * np.cos(a), c0[1] + 8 + rad * np.sin(a)], 1)
            sid = s.add_polygon(pts, 0.5)
            move = lambda k: s.update_polygon(sid, pts + k * DX, 0.5)
        else:
            raise SystemExit("unknown scenario " + scenario)
        s.run(Lst)
        geo = []
        for k in range(1, UPDATES + 1):
            move(k)
            s.run(Lst)
            geo.append(s.timings().geometryMs)
        print("%s %d^2: %d updates, geometryMs median %.3f (the whole geometry step: upload, recompose, coefficient and tile passes)"
              % (scenario, n, UPDATES, float(np.median(geo))), flush=True)


if __name__ == "__main__":
    main()
