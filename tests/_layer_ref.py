"""The edge-layer model (include/planeverb_amd.h PvAmdSetEdgeLayer) restated in numpy float32.

layer_fdtd() is the pinned oracle's stencil (oracle/pv_oracle.c pvo_fdtd, FDTD.cpp:87-236) on the same flat cell array, with the
two damped expressions of the layer model:
    pressure: pr' = beta * ((apx[x] * apy[y]) * pr - (bpx[x] * bpy[y]) * (C * div))
    vx, vy  : the air part ax[x] * vx - bx[x] * (C * grad) (ay[y], by[y] for vy); the wall part and the beta blend unchanged
numpy never fuses a multiply into an add, so every operation is the strict-IEEE float32 one, and with every factor equal to 1 the
expressions give the oracle's bits (tests/test_host_layer.py pins that).  Grid edges of absorption R4 follow the grid-edge model
(PvAmdSetGridBoundary): vx[0, y] = -Y0 * pr[0, y], vx[gx, y] = Y1 * pr[gx - 1, y], vy likewise with Y2 / Y3.

The analysis stays the oracle's: analyze() writes the restated history into an OracleGrid's history views and calls its analyze(),
so the eight members, onsets and delays come from unchanged oracle code."""
import numpy as np

F = np.float32


def edge_layer_tables(gx, gy, courant, w4, R0=0.1):
    """the eight tables of the documented formula (PvAmdHostEdgeLayerTables) in numpy: dict apx, bpx, ax, bx, apy, bpy, ay, by"""

    def axis(g, wlo, whi):
        C = float(F(courant))
        sc = np.zeros(g + 1)
        sf = np.zeros(g + 1)

        def s_of(depth, w):
            if w <= 0 or depth <= 0:
                return 0.0
            smax = 3.0 * C * np.log(1.0 / R0) / (4.0 * w)
            u = depth / w
            return smax * (u * u)

        for x in range(g + 1):
            if x < g:
                if x < wlo:
                    sc[x] += s_of(wlo - x - 0.5, wlo)
                if x >= g - whi:
                    sc[x] += s_of(x + 0.5 - (g - whi), whi)
            if x <= wlo:
                sf[x] += s_of(float(wlo - x), wlo)
            if x >= g - whi:
                sf[x] += s_of(float(x - (g - whi)), whi)
        return (((1.0 - sc) / (1.0 + sc)).astype(F), (1.0 / (1.0 + sc)).astype(F),
                ((1.0 - sf) / (1.0 + sf)).astype(F), (1.0 / (1.0 + sf)).astype(F))

    t = axis(gx, w4[0], w4[1]) + axis(gy, w4[2], w4[3])
    return dict(zip(["apx", "bpx", "ax", "bx", "apy", "bpy", "ay", "by"], t))


def unit_tables(gx, gy):
    one = lambda n: np.ones(n, F)  # noqa: E731
    return dict(apx=one(gx + 1), bpx=one(gx + 1), ax=one(gx + 1), bx=one(gx + 1), apy=one(gy + 1), bpy=one(gy + 1),
                ay=one(gy + 1), by=one(gy + 1))


def courant_of(o):
    return F(F(F(343.21) * F(o.dt)) / F(o.dx))


def layer_fdtd(o, L, tabs, R4=None, steps=None, record=True, cells=None, win=None):
    """run the restated stencil on OracleGrid o's material with the listener at world L (x, y, z).  Returns (fields [3, gx + 1,
    gy + 1], history (pr, vx, vy) [T, gx + 1, gy + 1] or None, responses {cell: [T, 3]} of `cells`).  win = (x0, y0, nx, ny):
    record only that block of cells."""
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
    AP = (tabs["apx"][xs] * tabs["apy"][ys]).astype(F)
    BP = (tabs["bpx"][xs] * tabs["bpy"][ys]).astype(F)
    AX, BX = tabs["ax"][xs], tabs["bx"][xs]
    AY, BY = tabs["ay"][ys], tabs["by"][ys]
    Ye = [F(1)] * 4 if R4 is None else [(F(1) - F(r)) / (F(1) + F(r)) for r in R4]
    pr = np.zeros(N + S + 2, F)
    vx = np.zeros(N + S + 2, F)
    vy = np.zeros(N + S + 2, F)
    x0, y0, wx, wy = (0, 0, gx + 1, gy + 1) if win is None else win
    hist = tuple(np.empty((T, wx, wy), F) for _ in range(3)) if record else None
    resp = {c: np.empty((T, 3), F) for c in (cells or [])}
    # vx faces i in [S, N) (neighbour i - S), vy faces i in [1, N) (neighbour i - 1): the oracle's loop ranges
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
    for t in range(T):
        div = (vx[S:N + S] - vx[0:N]) + (vy[1:N + 1] - vy[0:N])
        pr[:N] = beta * (AP * pr[:N] - BP * (C * div))
        p_i, p_n = pr[S:N], pr[0:N - S]
        air = AX[S:N] * vx[S:N] - BX[S:N] * (C * (p_i - p_n))
        wall = Ybx * (p_n * bx_n + p_i * bx_i)
        vx[S:N] = bbx * air + dbx * wall
        p_i, p_n = pr[1:N], pr[0:N - 1]
        air = AY[1:N] * vy[1:N] - BY[1:N] * (C * (p_i - p_n))
        wall = Yby * (p_n * by_n + p_i * by_i)
        vy[1:N] = bby * air + dby * wall
        if R4 is None:
            vx[e1] = -pr[e1]
            vx[e2] = pr[e2 - gy - 1]
            vy[f1] = -pr[f1]
            vy[f2] = pr[f2 - 1]
        else:
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
        if t < o.T:
            pr[lpos] += pulse[t]
    fields = np.stack([pr[:N], vx[:N], vy[:N]]).reshape(3, gx + 1, gy + 1)
    return fields, hist, resp


def analyze(o, hist, efree, L, prev=None):
    """the oracle's analysis of the restated history: (records [gx, gy, 8], delay [gx, gy])"""
    hp, hx, hy = o.history()
    hp[:] = hist[0]
    hx[:] = hist[1]
    hy[:] = hist[2]
    r, d, _ = o.analyze(efree, L, prev=prev)
    return r, d
