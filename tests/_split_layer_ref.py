"""The split-field edge-layer model (include/planeverb_amd.h PvAmdSetEdgeLayerSplit) restated in numpy float32.

split_fdtd() is tests/_layer_ref.py layer_fdtd() -- the pinned oracle's stencil on the same flat cell array, with the layer
model's damped velocity air parts and the grid-edge model -- with the pressure of the layer cells split.  A layer cell is a cell
with apx[x] != 1 or apy[y] != 1; it carries px, the x part of its pressure, and the y part is pr - px:
    dvx = vx[x + 1, y] - vx[x, y]        dvy = vy[x, y + 1] - vy[x, y]
    nx  = beta * ((apx[x] * px) - bpx[x] * (C * dvx))
    ny  = beta * ((apy[y] * (pr - px)) - bpy[y] * (C * dvy))
    pr' = nx + ny        px' = nx
Every other cell takes the oracle's beta * (pr - C * div) and px = 0.  numpy never fuses a multiply into an add, so every
operation is the strict-IEEE float32 one.  The pulse goes into pr only.  Analysis: _layer_ref.analyze (the oracle's own)."""
import numpy as np

from _layer_ref import analyze, courant_of, edge_layer_tables, unit_tables  # noqa: F401  (re-exported for the tests)

F = np.float32


def layer_cells(tabs, gx, gy):
    """[gx + 1, gy + 1] bool: the layer cells (apx[x] != 1 or apy[y] != 1)"""
    return (tabs["apx"][:, None] != 1) | (tabs["apy"][None, :] != 1)


def split_fdtd(o, L, tabs, R4=None, steps=None, record=True, cells=None, win=None, energy=False, px0=None, fields0=None,
               with_pulse=True):
    """run the split-layer stencil on OracleGrid o's material with the listener at world L (x, y, z).  Returns (fields
    [3, gx + 1, gy + 1], history (pr, vx, vy) [T, wx, wy] or None, responses {cell: [T, 3]}, extra) where extra = dict(px =
    the final x part [gx + 1, gy + 1], energy = [steps] float64 sum of pr^2 + vx^2 + vy^2 after each step, or None).
    win = (x0, y0, nx, ny): record only that block of cells.  fields0 / px0: start from these fields instead of zeros (the
    raw-stepping form; with_pulse = False: no pulse at all)."""
    gx, gy = o.gx, o.gy
    S, N = gy + 1, (gx + 1) * (gy + 1)
    T = o.T if steps is None else steps
    b, R = o.material()
    beta = b.astype(F).reshape(-1)
    Rf = R.astype(F).reshape(-1)
    Y = (F(1) - Rf) / (F(1) + Rf)
    C = courant_of(o)
    lcx, lcy = o.listener_cell(L[0], L[2])
    lpos = lcx * S + lcy
    pulse = o.pulse() if T <= o.T else np.concatenate([o.pulse(), np.zeros(T - o.T, F)])
    xs = np.arange(N) // S
    ys = np.arange(N) % S
    APX, BPX = tabs["apx"][xs], tabs["bpx"][xs]
    APY, BPY = tabs["apy"][ys], tabs["bpy"][ys]
    LAY = (APX != 1) | (APY != 1)
    AX, BX = tabs["ax"][xs], tabs["bx"][xs]
    AY, BY = tabs["ay"][ys], tabs["by"][ys]
    Ye = [F(1)] * 4 if R4 is None else [(F(1) - F(r)) / (F(1) + F(r)) for r in R4]
    pr = np.zeros(N + S + 2, F)
    vx = np.zeros(N + S + 2, F)
    vy = np.zeros(N + S + 2, F)
    px = np.zeros(N, F)
    if fields0 is not None:
        for f, f0 in zip((pr, vx, vy), fields0):
            f[:N] = np.asarray(f0, F).reshape(-1)
    if px0 is not None:
        px[:] = np.asarray(px0, F).reshape(-1)
    x0, y0, wx, wy = (0, 0, gx + 1, gy + 1) if win is None else win
    hist = tuple(np.empty((T, wx, wy), F) for _ in range(3)) if record else None
    resp = {c: np.empty((T, 3), F) for c in (cells or [])}
    en = np.empty(T, np.float64) if energy else None
    bx_i, bx_n = beta[S:N], beta[0:N - S]
    Yx_i, Yx_n = Y[S:N], Y[0:N - S]
    by_i, by_n = beta[1:N], beta[0:N - 1]
    Yy_i, Yy_n = Y[1:N], Y[0:N - 1]
    Ybx = bx_i * Yx_n + bx_n * Yx_i
    Yby = by_i * Yy_n + by_n * Yy_i
    bbx, dbx = bx_i * bx_n, bx_n - bx_i
    bby, dby = by_i * by_n, by_n - by_i
    e1 = np.arange(gy)
    e2 = gx * S + np.arange(gy)
    f1 = np.arange(gx) * S
    f2 = np.arange(gx) * S + gy
    zero = np.zeros(N, F)
    for t in range(T):
        dvx = vx[S:N + S] - vx[0:N]
        dvy = vy[1:N + 1] - vy[0:N]
        p = pr[:N]
        nx = beta * ((APX * px) - BPX * (C * dvx))
        ny = beta * ((APY * (p - px)) - BPY * (C * dvy))
        plain = beta * (p - C * (dvx + dvy))
        pr[:N] = np.where(LAY, nx + ny, plain)
        px = np.where(LAY, nx, zero)
        p_i, p_n = pr[S:N], pr[0:N - S]
        air = AX[S:N] * vx[S:N] - BX[S:N] * (C * (p_i - p_n))
        wall = Ybx * (p_n * bx_n + p_i * bx_i)
        vx[S:N] = bbx * air + dbx * wall
        p_i, p_n = pr[1:N], pr[0:N - 1]
        air = AY[1:N] * vy[1:N] - BY[1:N] * (C * (p_i - p_n))
        wall = Yby * (p_n * by_n + p_i * by_i)
        vy[1:N] = bby * air + dby * wall
        vx[e1] = -Ye[0] * pr[e1]
        vx[e2] = Ye[1] * pr[e2 - gy - 1]
        vy[f1] = -Ye[2] * pr[f1]
        vy[f2] = Ye[3] * pr[f2 - 1]
        if record:
            for k, f in enumerate((pr, vx, vy)):
                hist[k][t] = f[:N].reshape(gx + 1, gy + 1)[x0:x0 + wx, y0:y0 + wy]
        for (cx, cy), r in resp.items():
            i = cx * S + cy
            r[t] = (pr[i], vx[i], vy[i])
        if energy:
            en[t] = sum(float(np.dot(f[:N].astype(np.float64), f[:N].astype(np.float64))) for f in (pr, vx, vy))
        if with_pulse and t < o.T:
            pr[lpos] += pulse[t]
    fields = np.stack([pr[:N], vx[:N], vy[:N]]).reshape(3, gx + 1, gy + 1)
    return fields, hist, resp, dict(px=px.reshape(gx + 1, gy + 1), energy=en)
