"""numpy restatement of the directional energy lobes (include/planeverb_amd.h, PvAmdSetLobeWindows .. PvAmdLobeGains), written
from the definition:

    n_i = (int)(edge_i * (float)fs) in float32, onset = (int)delay (FLT_MAX: not reached),
    for t = onset .. T - 1, k = t - onset, w = the window k lies in (k < n_0; n_(j-1) <= k < n_j; k >= n_last):
        e = p p;  a = vx vx;  b = vy vy;  q = a + b;  E[w] += e
        if q > 0:  ex = e (a / q);  ey = e (b / q)
                   (vx > 0) == (p > 0) ? XP[w] += ex : XN[w] += ex;   (vy > 0) == (p > 0) ? YP[w] += ey : YN[w] += ey
    record = n = T - onset, then E, XP, XN, YP, YN per window

p, vx, vy are GIVEN (the velocity is the library's: what PvAmdGetImpulseResponse returns).  Everything is float32, every product,
sum and quotient rounded on its own, every sum strictly sequential in increasing t from +0: per-cell arrays and ONE python loop
over t, each window's sums updated with np.where on that window's members (a cell that is no member, or whose sample does not
feed that lobe, keeps its sum).  No np.sum, no np.cumsum, no np.dot."""
import numpy as np

NO_ONSET = np.float32(3.0e38)  # delay >= this: FLT_MAX, the cell was not reached
MAX_EDGES = 7
DEFAULT_EDGES = (0.01, 0.08)
NAMES = ("e", "xp", "xn", "yp", "yn")


def edge_steps(edges, fs):
    """the step counts of the edges, or None where the setting is refused"""
    edges = DEFAULT_EDGES if edges is None or len(edges) == 0 else edges
    if len(edges) > MAX_EDGES:
        return None
    n = []
    for e in edges:
        with np.errstate(over="ignore"):
            x = np.float32(e) * np.float32(fs)
        if not np.isfinite(x) or not (x >= 1) or int(x) > (1 << 20):
            return None
        n.append(int(x))
    if any(b <= a for a, b in zip(n, n[1:])):
        return None
    return n


def lobes(p, vx, vy, delay, fs, edges=None):
    """p, vx, vy: float32 [T, ...], delay: float32 [...] onset map -> float32 [..., 1 + 5 nW], NaN without an onset"""
    p, vx, vy = (np.asarray(v, np.float32) for v in (p, vx, vy))
    delay = np.asarray(delay, np.float32)
    assert p.shape == vx.shape == vy.shape and p.shape[1:] == delay.shape
    n = edge_steps(edges, fs)
    assert n is not None
    nw = len(n) + 1
    T = p.shape[0]
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int64)
    sums = np.zeros((nw, 5) + delay.shape, np.float32)
    zero = np.float32(0)
    for t in range(T):
        k = t - t0
        mask = reached & (k >= 0)
        if not mask.any():
            continue
        pt, xt, yt = p[t], vx[t], vy[t]
        e, a, b = pt * pt, xt * xt, yt * yt
        q = a + b
        with np.errstate(all="ignore"):
            ex, ey = e * (a / q), e * (b / q)
        has = q > zero
        xpos = (xt > zero) == (pt > zero)
        ypos = (yt > zero) == (pt > zero)
        w = np.zeros(delay.shape, np.int64)
        for ni in n:
            w = w + (k >= ni)
        for j in np.unique(w[mask]):
            m = mask & (w == j)
            s = sums[j]
            with np.errstate(all="ignore"):
                s[0] = np.where(m, s[0] + e, s[0])
                s[1] = np.where(m & has & xpos, s[1] + ex, s[1])
                s[2] = np.where(m & has & ~xpos, s[2] + ex, s[2])
                s[3] = np.where(m & has & ypos, s[3] + ey, s[3])
                s[4] = np.where(m & has & ~ypos, s[4] + ey, s[4])
    assert sums.dtype == np.float32
    out = np.full(delay.shape + (1 + 5 * nw,), np.nan, np.float32)
    out[..., 0][reached] = (T - t0).astype(np.float32)[reached]
    for j in range(nw):
        for c in range(5):
            out[..., 1 + 5 * j + c][reached] = sums[j, c][reached]
    return out


def lobes_ir(p, vx, vy, fs, onset, edges=None):
    """the same for one impulse response p[T], vx[T], vy[T] with its onset step"""
    p, vx, vy = (np.asarray(v, np.float32).reshape(-1, 1) for v in (p, vx, vy))
    return lobes(p, vx, vy, np.array([onset], np.float32), fs, edges)[0]


def pattern(kind, d):
    """c(d): 1 for omni (0); for cardioid (1) (1 + d) / 2, not below 0.01"""
    d = np.float32(d)
    if kind == 0:
        return np.float32(1)
    c = (np.float32(1) + d) / np.float32(2)
    return c if c > np.float32(0.01) else np.float32(0.01)


def lobe_gains(record, forward, kind):
    """PvAmdLobeGains restated: float32 [nW] from a record [1 + 5 nW], the emitter's forward (x, z) and the pattern (0 / 1)"""
    r = np.asarray(record, np.float32).reshape(-1)
    nw = (r.size - 1) // 5
    fx, fy = np.float32(forward[0]), np.float32(forward[1])
    wxp, wxn, wyp, wyn = pattern(kind, -fx), pattern(kind, fx), pattern(kind, -fy), pattern(kind, fy)
    gxp, gxn, gyp, gyn = wxp * wxp, wxn * wxn, wyp * wyp, wyn * wyn
    out = np.empty(nw, np.float32)
    with np.errstate(all="ignore"):
        for w in range(nw):
            xp, xn, yp, yn = (np.float32(v) for v in r[2 + 5 * w:6 + 5 * w])
            num = (((xp * gxp) + (xn * gxn)) + (yp * gyp)) + (yn * gyn)
            den = ((xp + xn) + yp) + yn
            out[w] = num / den
    return out
