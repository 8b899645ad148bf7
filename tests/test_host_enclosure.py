"""The enclosure search of the resident-window runs (PvAmdHostEnclosure, csrc/pv_core.cpp findEnclosure) against a plain python
flood fill: component size, bounding box, tile window, "not enclosed" answers and the visit cap.  CPU only."""
import os
from collections import deque

import numpy as np

from planeverb_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE = os.path.join(ROOT, "tests", "scenes", "HugeRoom.pv")
DX = np.float32(343.21) / np.float32(275) / np.float32(3.5)
TR, TC = 36, 40  # the large-grid tile


def flood(beta, seed, limit=None):
    """4-connected air component of `seed`: (cells, r0, c0, r1, c1), or None for a wall seed; stops at `limit` cells"""
    nx, ny = beta.shape
    if not (0 <= seed[0] < nx and 0 <= seed[1] < ny) or not beta[seed]:
        return None
    seen = {seed}
    todo = deque([seed])
    while todo:
        x, y = todo.popleft()
        for p in ((x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)):
            if 0 <= p[0] < nx and 0 <= p[1] < ny and beta[p] and p not in seen:
                seen.add(p)
                todo.append(p)
        if limit is not None and len(seen) > limit:
            return None
    a = np.array(sorted(seen))
    return len(seen), int(a[:, 0].min()), int(a[:, 1].min()), int(a[:, 0].max()), int(a[:, 1].max())


def window_of(box, nx, ny):
    r0, c0, r1, c1 = box
    lo, hi = max(r0 - 1, 0), min(r1 + 1, nx - 1)
    lc, hc = max(c0 - 1, 0), min(c1 + 1, ny - 1)
    return lo // TR, lc // TC, hi // TR - lo // TR + 1, hc // TC - lc // TC + 1


def test_random_wall_layouts():
    rng = np.random.default_rng(11)
    for trial in range(12):
        nx, ny = int(rng.integers(60, 260)), int(rng.integers(60, 260))
        beta = np.ones((nx, ny), np.uint8)
        for _ in range(int(rng.integers(2, 9))):  # hollow rectangles: rooms, some of them nested or cut by others
            x0, y0 = int(rng.integers(0, nx - 12)), int(rng.integers(0, ny - 12))
            x1, y1 = min(nx - 1, x0 + int(rng.integers(6, 90))), min(ny - 1, y0 + int(rng.integers(6, 90)))
            beta[x0:x1 + 1, [y0, y1]] = 0
            beta[[x0, x1], y0:y1 + 1] = 0
        beta[rng.random((nx, ny)) < 0.01] = 0  # loose wall cells
        if trial % 3 == 0:  # a gap in some wall
            beta[nx // 2, :] = 1
        for max_tiles in (4, 128):
            for _ in range(12):
                seed = (int(rng.integers(0, nx)), int(rng.integers(0, ny)))
                got = api.host_enclosure(beta, seed, TR, TC, max_tiles)
                want = flood(beta, seed)
                if want is None:
                    assert got["found"] == 0 and got["cells"] == 0, (trial, seed, got)
                    continue
                win = window_of(want[1:], nx, ny)
                fits = win[2] * win[3] <= max_tiles
                assert got["found"] == (1 if fits else 0), (trial, seed, max_tiles, got, want, win)
                assert got["cells"] <= max_tiles * TR * TC
                if fits:
                    assert got["cells"] == want[0] and got["box"] == want[1:] and got["window"] == win, (trial, seed, got, want, win)
                else:
                    assert 0 < got["cells"] <= want[0]


def test_seed_outside_the_grid_and_window_at_the_origin():
    beta = np.zeros((100, 100), np.uint8)
    beta[0:20, 0:30] = 1  # a room in the grid's corner: the ring is clipped to the grid
    beta[60:70, 85:100] = 1
    for seed in ((-1, 5), (5, 100), (100, 0)):
        assert api.host_enclosure(beta, seed, TR, TC, 16) == dict(found=0, cells=0, box=(0, 0, 0, 0), window=(0, 0, 0, 0))
    got = api.host_enclosure(beta, (3, 3), TR, TC, 16)
    assert got == dict(found=1, cells=600, box=(0, 0, 19, 29), window=(0, 0, 1, 1))
    got = api.host_enclosure(beta, (65, 99), TR, TC, 16)
    assert got == dict(found=1, cells=150, box=(60, 85, 69, 99), window=(1, 2, 1, 1))  # rows 59..70 -> tile row 1; cols 84..99 -> tile 2
    assert api.host_enclosure(beta, (30, 30), TR, TC, 16)["found"] == 0  # a wall cell


def test_hugeroom_at_4096():
    n = 4096
    size = float((n + 0.5) * DX)
    beta, _ = api.host_rasterize(size, size, 275, api.load_pv(HUGE))
    assert beta.shape == (n + 1, n + 1)
    listeners = [(5, 4), (8, 8), (12, 6), (15, 15), (20, 5), (5, 20), (20, 20), (12.5, 18)]  # bench.py's
    first = None
    for x, z in listeners:
        seed = api.host_cells(size, size, 275, x, z)[0]
        got = api.host_enclosure(beta, seed, TR, TC, 128)
        assert got["found"] == 1, (seed, got)
        if first is None:  # (the python fill once: the room is one component)
            r0, c0, r1, c1 = got["box"]
            want = flood(beta[:r1 + 40, :c1 + 40], seed)
            assert (got["cells"],) + got["box"] == want
            assert got["window"] == window_of(got["box"], n + 1, n + 1)
            assert got["window"][2] * got["window"][3] <= 6 and 3000 < got["cells"] < 6000  # the 25 m room: ~70^2 cells less its walls
            first = got
        assert got == first, (seed, got, first)
    # outside the room: the open remainder of the grid -- given up within the cap, whatever the grid's size
    for max_tiles in (9, 128):
        got = api.host_enclosure(beta, (2000, 2000), TR, TC, max_tiles)
        assert got["found"] == 0 and 0 < got["cells"] <= max_tiles * TR * TC, got
    # ... and a seed just outside the room's walls
    got = api.host_enclosure(beta, (first["box"][2] + 30, first["box"][3] + 30), TR, TC, 128)
    assert got["found"] == 0 and got["cells"] <= 128 * TR * TC


def test_open_grid_gives_up_within_the_cap():
    beta = np.ones((1500, 1500), np.uint8)
    for max_tiles in (1, 12, 128):
        got = api.host_enclosure(beta, (700, 800), TR, TC, max_tiles)
        assert got["found"] == 0 and 0 < got["cells"] <= max_tiles * TR * TC, (max_tiles, got)
    # a room that fills its window exactly: every cell of 2 x 2 tiles but the ring -> found, cells = (72 - 2) * (80 - 2)
    beta = np.zeros((200, 200), np.uint8)
    beta[37:107, 41:119] = 1
    got = api.host_enclosure(beta, (50, 50), TR, TC, 4)
    assert got == dict(found=1, cells=70 * 78, box=(37, 41, 106, 118), window=(1, 1, 2, 2))
    assert api.host_enclosure(beta, (50, 50), TR, TC, 3)["found"] == 0
