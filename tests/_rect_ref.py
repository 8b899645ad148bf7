"""A non-square grid restated with the pinned oracle, unchanged.

The oracle restates the reference, whose rasteriser, solver and analyser use three different strides on a grid with gx != gy
(SURVEY.md Q1), so OracleGrid(size_x != size_y) is no reference for anything.  The library defines such a grid by one cell array
of stride gy + 1 throughout, and that discrete system exists inside a SQUARE oracle grid: the ring construction of
tests/_boundary_ref.py with G and H taken separately.  A gx x gy grid with edge absorptions R4 is the rectangle of cells enclosed by
a one-cell ring of wall cells (ring_boxes(gx + 2, gy + 2, dx, R4)) inside a square oracle grid of n = max(gx, gy) + 2 cells; the
scene's half-cell boxes and the listener shift by +dx, the analysis runs at cell offset (-1, -1), and the block [1 : gx + 2,
1 : gy + 2] of the square then holds the rectangle's fields, history, onsets and records.  The ring is closed (a face between two
wall cells carries no velocity, a wall cell no pressure), so the cells of the square outside it are never excited; RectRing asserts
that after every run, together with the closed ring, the listener shift and the interior material against the library's host
rasteriser of the non-square grid.

duck() is the rectangle as the object tests/_layer_ref.layer_fdtd and tests/_split_layer_ref.split_fdtd step (both restate the
stencil with stride gy + 1 in numpy); analyze_history() hands such a restated history to the oracle's unchanged analysis.
free_energy() restates the free-field energy of a non-square grid from the cells the library reads (csrc/pv_solver.cpp
Solver::computeEfree)."""
import numpy as np

from _boundary_ref import half_cell_box, ring_boxes

F = np.float32


def walls_rect(dx, gx, gy):
    """half-cell boxes of distinct absorptions on a gx x gy grid: an interior wall, a wall on the x = 0 edge, a wall running into
    the ghost column (y = gy) and one running into the ghost row (x = gx).  Nothing in it is symmetric under x <-> y."""
    a, c = gx // 3, 2 * gx // 3
    return np.array([half_cell_box(dx, a, a + 2, 3, gy - gy // 4, 0.3),
                     half_cell_box(dx, 0, 3, gy // 2, gy // 2 + min(9, gy // 4), 0.6),
                     half_cell_box(dx, c, c + max(2, min(7, gx // 8)), gy - 3, gy + 1, 0.1),
                     half_cell_box(dx, gx - 2, gx + 1, gy // 5, gy // 5 + 4, 0.8)], np.float32)


def listeners_rect(gx, gy):
    """the two listener cells of a chained pair of runs: inside the grid, then a few cells from the far corner"""
    return [(gx // 2, gy // 3 + 3), (gx - 4, gy - 5)]


def size_of(g, dx):
    """metres of a g-cell axis ((int)((1 / dx) * size) = g)"""
    return float((g + 0.5) * F(dx))


class _Duck:
    """the rectangle as a grid object: gx, gy, T, dt, dx, material(), pulse(), listener_cell()"""

    def __init__(self, ring):
        self._r = ring
        self.gx, self.gy, self.T, self.dt, self.dx, self.fs = ring.gx, ring.gy, ring.T, ring.o.dt, ring.o.dx, ring.fs

    def material(self):
        return self._r.material()

    def pulse(self):
        return self._r.o.pulse()[:self.T].copy()

    def listener_cell(self, lx, lz):
        return self._r.o.listener_cell(lx, lz)  # (int)(x / dx): no grid size in it


class RectRing:
    """the gx x gy grid at `res` with half-cell `boxes` and edge absorptions R4, as a ring inside a square grid of the pinned
    oracle.  steps: run and analyse that many steps instead of the grid's own response length (the solver's num_steps; the
    pulse table stays the grid's own)."""

    def __init__(self, oracle, gx, gy, res, boxes, R4, efree, steps=None, check_material=True):
        self.gx, self.gy, self.res = gx, gy, res
        n = max(gx, gy) + 2
        dx = F(oracle.grid_params(res)[0])
        d = float(dx)
        big = F((n + 0.5) * d)
        self.o = oracle.OracleGrid(float(big), float(big), res)
        assert (self.o.gx, self.o.gy) == (n, n) and F(self.o.dx) == dx, ((self.o.gx, self.o.gy), n)
        self.n, self.dx, self.fs = n, self.o.dx, self.o.fs
        if steps is not None:
            assert 0 < steps <= self.o.T
            self.o._g.contents.T = steps  # pvo_fdtd and pvo_analyze_at read it; the planes keep their (larger) allocation
            self.o.T = steps
        self.T = self.o.T
        G, H = gx + 2, gy + 2
        for r in ring_boxes(G, H, dx, [F(v) for v in R4]):
            self.o.add_aabb(r)
        boxes = np.zeros((0, 5), F) if boxes is None else np.asarray(boxes, F).reshape(-1, 5)
        for b in boxes:
            # half-cell boxes only (half_cell_box): both edges at (k + 0.5) dx, so that (int) truncation survives the shift
            for c, w in ((b[0], b[2]), (b[1], b[3])):
                for e in (float(c) - 0.5 * float(w), float(c) + 0.5 * float(w)):
                    assert abs(e / d - np.floor(e / d) - 0.5) < 1e-3, ("not a half-cell box", b)
            self.o.add_aabb(np.array([b[0] + F(d), b[1] + F(d), b[2], b[3], b[4]], F))
        bb, Rb = self.o.material()
        assert (bb[0, :H] == 0).all() and (bb[G - 1, :H] == 0).all() and (bb[:G, 0] == 0).all() and (bb[:G, H - 1] == 0).all(), \
            "ring grid: the ring is not closed"
        if check_material:
            from planeverb_amd import api
            bs, Rs = api.host_rasterize(size_of(gx, dx), size_of(gy, dx), res, boxes)
            assert bs.shape == (gx + 1, gy + 1), (bs.shape, gx, gy)
            assert np.array_equal(bb[1:G, 1:H], bs), "ring grid: interior beta differs from the non-square grid's"
            wall = bs[:gx, :gy] == 0
            assert np.array_equal(Rb[1:gx + 1, 1:gy + 1][wall], Rs[:gx, :gy][wall]), "ring grid: interior absorption differs"
        self.efree = F(efree)
        self.L = None

    def close(self):
        self.o.close()

    def _inside(self):
        m = np.zeros((self.n + 1, self.n + 1), bool)
        m[1:self.gx + 2, 1:self.gy + 2] = True
        return m

    def material(self):
        """(beta, R) [gx + 1, gy + 1] of the rectangle: the ring's far sides are its ghost row and column"""
        b, R = self.o.material()
        return b[1:self.gx + 2, 1:self.gy + 2].copy(), R[1:self.gx + 2, 1:self.gy + 2].copy()

    def load_material(self, b, R):
        """overwrite the rectangle's material [gx + 1, gy + 1] (shapes the oracle cannot rasterise); the ring must stay closed"""
        b = np.asarray(b, np.int16)
        assert b.shape == (self.gx + 1, self.gy + 1) and (b[self.gx, :] == 0).all() and (b[:, self.gy] == 0).all()
        g = self.o._g.contents
        n1 = self.n + 1
        np.ctypeslib.as_array(g.b, (self.o.ncell,)).reshape(n1, n1)[1:self.gx + 2, 1:self.gy + 2] = b
        Rv = np.ctypeslib.as_array(g.R, (self.o.ncell,)).reshape(n1, n1)
        keep = Rv[1:self.gx + 2, 1:self.gy + 2].copy()  # the far ring cells keep the edge absorptions
        new = np.asarray(R, F).copy()
        new[self.gx, :] = keep[self.gx, :]
        new[:, self.gy] = keep[:, self.gy]
        Rv[1:self.gx + 2, 1:self.gy + 2] = new

    def shifted(self, L):
        """the listener in the square grid's metres; its cell moves by exactly (1, 1)"""
        d = F(self.dx)
        Lb = (float(F(L[0]) + d), float(L[1]), float(F(L[2]) + d))
        c0 = self.o.listener_cell(L[0], L[2])
        c1 = self.o.listener_cell(Lb[0], Lb[2])
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1), ("listener cell not shifted by (1, 1)", c0, c1)
        return Lb

    def fdtd(self, L, want_fields=True):
        """run; returns the rectangle's fields [3, gx + 1, gy + 1] (ghost row and column included)"""
        Lb = self.shifted(L)
        self.L = L
        f = self.o.fdtd(Lb, want_fields=True)
        out = ~self._inside()
        assert not f[:, out].any(), "ring grid: the square outside the ring was excited"
        if want_fields:
            return f[:, 1:self.gx + 2, 1:self.gy + 2]

    def history(self):
        """(pr, vx, vy) [T, gx + 1, gy + 1] of the last run"""
        return tuple(h[:self.T, 1:self.gx + 2, 1:self.gy + 2] for h in self.o.history())

    def analyze(self, prev=None):
        """records [gx, gy, 8], delay [gx, gy] of the last run (prev: the rectangle's records of the run before)"""
        p = None
        if prev is not None:
            p = np.zeros((self.n, self.n, 8), F)
            p[1:self.gx + 1, 1:self.gy + 1] = prev
        r, dl, _ = self.o.analyze(self.efree, self.L, offset=(-1, -1), prev=p)
        return r[1:self.gx + 1, 1:self.gy + 1].copy(), dl[1:self.gx + 1, 1:self.gy + 1].copy()

    def duck(self):
        return _Duck(self)

    def analyze_history(self, hist, L, prev=None):
        """the oracle's analysis of a restated history (pr, vx, vy) [T, gx + 1, gy + 1] of the rectangle (what
        _layer_ref.analyze does on square grids): written into the square's history views at the ring offset"""
        self.shifted(L)
        self.L = L
        for view, h in zip(self.o.history(), hist):
            assert h.shape == (self.T, self.gx + 1, self.gy + 1), h.shape
            view[:self.T] = 0
            view[:self.T, 1:self.gx + 2, 1:self.gy + 2] = h
        return self.analyze(prev)


def free_cells(gx, gy, dx):
    """(source cell, read cell, metres between them) of the library's free-field run on a gx x gy grid (csrc/pv_solver.cpp
    Solver::computeEfree: FreeGrid.cpp:78-91): the source at the centre cell, passed in metres and truncated again; the energy
    read (int)(1 / dx) cells to its +x side"""
    dx = F(dx)
    lx0, ly0 = gx // 2, gy // 2
    ex, ey = lx0 + int(F(1) / dx), ly0
    src = (int(F(F(lx0) * dx) / dx), int(F(F(ly0) * dx) / dx))
    return src, (ex, ey), F(F(ex - lx0) * dx)


def free_samples(fs):
    """FreeGrid.cpp:99 (oracle/pv_oracle.c pvo_free_energy): the dry-gain window plus one metre of travel"""
    return int(F(0.01) * F(int(fs))) + int((F(1) / F(343.21)) * F(int(fs)))


def free_energy(oracle, gx, gy, res):
    """pvo_free_energy restated on the empty rectangle with absorbing edges; the sum runs sequentially in float32"""
    n = free_samples(oracle.grid_params(res)[2])
    ring = RectRing(oracle, gx, gy, res, None, (0.0, 0.0, 0.0, 0.0), 0.0, steps=n, check_material=False)
    try:
        dx = F(ring.dx)
        src, (ex, ey), r = free_cells(gx, gy, dx)
        L = ((src[0] + 0.5) * float(dx), 0.0, (src[1] + 0.5) * float(dx))  # (the centre of the re-truncated source cell)
        assert ring.o.listener_cell(L[0], L[2]) == src
        ring.fdtd(L, want_fields=False)
        p = ring.history()[0][:n, ex, ey]
        e = F(0)
        for v in p:
            e = F(e + F(v * v))
        return F(e * r), n
    finally:
        ring.close()
