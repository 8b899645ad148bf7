"""numpy restatement of the lateral energy fraction and early-sound direction (include/planeverb_amd.h, PvAmdLateralFraction),
written from the definition:

    onset = (int)delay (FLT_MAX: not reached), n5 = (int)(0.005f * (float)fs), n80 = (int)(0.08f * (float)fs),
    tEnd = min(onset + n80, T); for t = onset .. tEnd - 1, k = t - onset:
        e80 += p p;   fx += (k < n5 ? p vx : 0), fy += (k < n5 ? p vy : 0);
        sxx += (k >= n5 ? vx vx : 0), sxy += (k >= n5 ? vx vy : 0), syy += (k >= n5 ? vy vy : 0);
    norm = sqrtf(fx fx + fy fy), dx = fx / norm, dy = fy / norm,
    lat = ((sxx (dy dy)) - (2 (sxy (dx dy)))) + (syy (dx dx)), lf = lat / e80;
    record = lf, dir_x, dir_y, n = tEnd - onset, e80, lateral, fx, fy, sxx, sxy, syy.

p, vx, vy are GIVEN (the velocity is the library's: what PvAmdGetImpulseResponse returns).  Everything is float32, every product,
sum and quotient rounded on its own, every sum strictly sequential in increasing t from +0: per-cell arrays and ONE python loop
over t, a step that is no member of a sum adding +0 as the definition says.  No np.sum, no np.cumsum, no np.dot.  numpy's float32
sqrt and division are correctly rounded."""
import numpy as np

NAMES = ("lf", "dir_x", "dir_y", "n", "e80", "lateral", "fx", "fy", "sxx", "sxy", "syy")
NO_ONSET = np.float32(3.0e38)  # delay >= this: FLT_MAX, the cell was not reached


def n5(fs):
    return int(np.float32(0.005) * np.float32(fs))


def n80(fs):
    return int(np.float32(0.08) * np.float32(fs))


def lateral_fraction(p, vx, vy, delay, fs):
    """p, vx, vy: float32 [T, ...], delay: float32 [...] onset map -> float32 [..., 11], NaN without an onset"""
    p, vx, vy = (np.asarray(v, np.float32) for v in (p, vx, vy))
    delay = np.asarray(delay, np.float32)
    assert p.shape == vx.shape == vy.shape and p.shape[1:] == delay.shape
    T = p.shape[0]
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    a5, a80 = n5(fs), n80(fs)
    t_end = np.minimum(t0 + np.int32(a80), np.int32(T))
    zero = np.float32(0)
    e80, fx, fy, sxx, sxy, syy = (np.zeros(delay.shape, np.float32) for _ in range(6))
    for t in range(T):
        k = np.int32(t) - t0
        mask = reached & (k >= 0) & (np.int32(t) < t_end)
        if not mask.any():
            continue
        pt, xt, yt = p[t], vx[t], vy[t]
        early, late = mask & (k < a5), mask & (k >= a5)
        e80 = e80 + np.where(mask, pt * pt, zero)
        fx = fx + np.where(early, pt * xt, zero)
        fy = fy + np.where(early, pt * yt, zero)
        sxx = sxx + np.where(late, xt * xt, zero)
        sxy = sxy + np.where(late, xt * yt, zero)
        syy = syy + np.where(late, yt * yt, zero)
    out = np.full(delay.shape + (11,), np.nan, np.float32)
    with np.errstate(all="ignore"):
        norm = np.sqrt((fx * fx) + (fy * fy))
        dx, dy = fx / norm, fy / norm
        lat = ((sxx * (dy * dy)) - (np.float32(2.0) * (sxy * (dx * dy)))) + (syy * (dx * dx))
        lf = lat / e80
    for i, v in enumerate((lf, dx, dy, (t_end - t0).astype(np.float32), e80, lat, fx, fy, sxx, sxy, syy)):
        assert v.dtype == np.float32
        out[..., i][reached] = v[reached]
    return out


def lateral_fraction_ir(p, vx, vy, fs, onset):
    """the same for one impulse response p[T], vx[T], vy[T] with its onset step"""
    p, vx, vy = (np.asarray(v, np.float32).reshape(-1, 1) for v in (p, vx, vy))
    return lateral_fraction(p, vx, vy, np.array([onset], np.float32), fs)[0]
