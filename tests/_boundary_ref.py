"""The grid-edge model (include/planeverb_amd.h PvAmdSetGridBoundary) restated with the pinned oracle, unchanged.

A grid with edge absorptions R0..R3 is the same discrete system as a grid two cells larger in which a one-cell ring of wall cells
has those absorptions, the scene's boxes and the listener are shifted by +dx in both axes, and the analysis runs at cell offset
(-1, -1) with the small grid's free-field energy and listener (OracleGrid.analyze(offset=...)).  Its interior then holds the small
grid's fields, history, onsets and records.  Every ring and scene box edge lies on a half cell: the reference rasterises with
(int) truncation, and an edge on a whole cell can move by one cell after the shift.  The helper asserts that the ring grid's
interior material equals the small grid's and that the listener cell moved by exactly (1, 1)."""
import numpy as np

F = np.float32


def ring_boxes(G, H, dx, R4):
    """the ring of a (G + 1) x (H + 1) cell array: sides x = 0, x = G - 1, y = 0, y = H - 1 (reference AABBs: centre x, centre
    y, width, height, absorption), edges on half cells"""
    d = float(dx)
    xs, ys = (G + 1) * d, (H + 1) * d  # full length along the other axis: -0.5 dx .. (G + 0.5) dx
    return np.array([[0.5 * d, 0.5 * H * d, 2 * d, ys, R4[0]],
                     [G * d, 0.5 * H * d, d, ys, R4[1]],
                     [0.5 * G * d, 0.5 * d, xs, 2 * d, R4[2]],
                     [0.5 * G * d, H * d, xs, d, R4[3]]], np.float32)


def half_cell_box(dx, x0, x1, y0, y1, R):
    """a scene box covering cells [x0, x1) x [y0, y1) whose edges lie on half cells (so that the ring grid's shift keeps it)"""
    d = float(dx)  # edges at (x0 + 0.5) dx and (x1 + 0.5) dx: (int) truncation gives x0 and x1
    return [0.5 * (x0 + x1 + 1) * d, 0.5 * (y0 + y1 + 1) * d, (x1 - x0) * d, (y1 - y0) * d, R]


class RingOracle:
    """the small grid (size, res, boxes) with edge absorptions R4, as a ring grid of the pinned oracle"""

    def __init__(self, oracle, size, res, boxes, R4, efree=None):
        self.small = oracle.OracleGrid(size, size, res, boxes, with_history=False)
        self.dx, self.gx, self.gy, self.T, self.fs = self.small.dx, self.small.gx, self.small.gy, self.small.T, self.small.fs
        gx, gy = self.gx, self.gy
        G, H = gx + 2, gy + 2
        d = float(self.dx)
        big = F((G + 0.5) * d)  # (int)((1 / dx) * big) = G
        self.o = oracle.OracleGrid(float(big), float(big), res)
        assert (self.o.gx, self.o.gy) == (G, H), ((self.o.gx, self.o.gy), (G, H))
        for r in ring_boxes(G, H, self.dx, [F(v) for v in R4]):
            self.o.add_aabb(r)
        for b in (boxes if boxes is not None else []):
            b = np.asarray(b, np.float32)
            self.o.add_aabb(np.array([b[0] + F(d), b[1] + F(d), b[2], b[3], b[4]], np.float32))
        bs, Rs = self.small.material()
        bb, Rb = self.o.material()
        assert np.array_equal(bb[1:G, 1:H], bs), "ring grid: interior beta differs from the small grid's"
        wall = bs[:gx, :gy] == 0
        assert np.array_equal(Rb[1:gx + 1, 1:gy + 1][wall], Rs[:gx, :gy][wall]), "ring grid: interior absorption differs"
        assert (bb[0, :H] == 0).all() and (bb[G - 1, :H] == 0).all() and (bb[:G, 0] == 0).all() and (bb[:G, H - 1] == 0).all()
        self.efree = F(oracle.free_energy(size, size, res)) if efree is None else F(efree)

    def close(self):
        self.o.close()
        self.small.close()

    def fdtd(self, L, want_fields=True):
        """run; returns the small grid's fields [3, gx + 1, gy + 1] (ghost row and column included)"""
        d = F(self.dx)
        Lb = (float(F(L[0]) + d), float(L[1]), float(F(L[2]) + d))
        c0 = self.small.listener_cell(L[0], L[2])
        c1 = self.o.listener_cell(Lb[0], Lb[2])
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 1), ("listener cell not shifted by (1, 1)", c0, c1)
        self.L = L
        f = self.o.fdtd(Lb, want_fields=want_fields)
        if want_fields:
            return f[:, 1:self.gx + 2, 1:self.gy + 2]

    def history(self):
        """(pr, vx, vy) [T, gx + 1, gy + 1] of the last run"""
        return tuple(h[:, 1:self.gx + 2, 1:self.gy + 2] for h in self.o.history())

    def analyze(self, prev=None):
        """records [gx, gy, 8], delay [gx, gy] of the last run (prev: the small grid's records of the run before)"""
        G, H = self.gx + 2, self.gy + 2
        p = None
        if prev is not None:
            p = np.zeros((G, H, 8), np.float32)
            p[1:self.gx + 1, 1:self.gy + 1] = prev
        r, dl, _ = self.o.analyze(self.efree, self.L, offset=(-1, -1), prev=p)
        return r[1:self.gx + 1, 1:self.gy + 1].copy(), dl[1:self.gx + 1, 1:self.gy + 1].copy()
