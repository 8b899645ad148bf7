"""numpy restatement of the band metrics (include/planeverb_amd.h, PvAmdBandMetrics), written from the definition:

    filter   per band two biquads (b0, b1, b2, a1, a2), transposed direct form II, float32, state +0 at t = T - 1, BACKWARDS in
             time down to the cell's onset t0 = (int)delay:
                 y = (b0 * x) + z1;  z1 = ((b1 * x) - (a1 * y)) + z2;  z2 = (b2 * x) - (a2 * y)
             section 2 takes section 1's y; x(t) = p(t); nothing below t0 enters
    e(t)     = y(t) * y(t);  E(T) = +0, E(t) = E(t + 1) + e(t) for t = T - 1 down to t0;  E0 = E(t0);  k = t - t0
    first 8  the decay times' record on this e: r = E / E0, L = 10 log10f(r), the three ranges, their double sums in decreasing
             t, completeness by r(tEnd - 1), depth
    last 4   n50 = (int)(0.05f * fs), n80 = (int)(0.08f * fs);  l50 = E(min(t0 + n50, T)), e50 = sum of e over k < n50 (decreasing
             t, from +0), likewise 80;  moment = sum of (float)k * e;  c50 = 10 log10f(e50 / l50), c80,  d50 = e50 / (e50 + l50),
             ts = (moment / E0) / (float)fs

Vectorised over cells, ONE python loop over t per walk, running downwards; every product, sum and quotient is a numpy float32
(or, in the fits, float64) operation of its own.  No np.sum, no np.cumsum, no np.dot, no scipy.  The coefficients are an INPUT:
the bit-level tests take them from the library, so that two libms cannot disagree about a tangent.  From the other restatements
come only what they already state of the decay fit: the range limits, the tail rule, the quiet NaN and the host's log10f."""
import numpy as np

from _decay_ref import QNAN, RANGES, tail_n
from _room_metrics_ref import NO_ONSET, log10f

NAMES = ("edt", "t20", "t30", "n_edt", "n_t20", "n_t30", "e0", "depth", "c50", "c80", "d50", "ts")


def n50_n80(fs):
    return int(np.float32(0.05) * np.float32(fs)), int(np.float32(0.08) * np.float32(fs))


def _onsets(delay):
    delay = np.asarray(delay, np.float32)
    reached = delay < NO_ONSET
    return reached, np.where(reached, delay, 0).astype(np.int32)


def band_filter(hist, delay, c10):
    """hist: float32 [T, ...], delay: float32 [...], c10: the band's ten float32 coefficients -> y float32 [T, ...]: the filter's
    output at every step t >= t0 of every reached cell, +0 elsewhere"""
    hist = np.asarray(hist, np.float32)
    c = np.asarray(c10, np.float32)  # (ten scalars, or ten arrays that broadcast against a plane)
    assert c.shape[0] == 10
    reached, t0 = _onsets(delay)
    T = hist.shape[0]
    y = np.zeros(hist.shape, np.float32)
    z = [np.zeros(t0.shape, np.float32) for _ in range(4)]
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            mask = reached & (np.int32(t) >= t0)
            if not mask.any():
                continue
            x = hist[t]
            for s in range(2):
                b0, b1, b2, a1, a2 = (c[5 * s + i] for i in range(5))
                z1, z2 = z[2 * s], z[2 * s + 1]
                ys = (b0 * x) + z1
                n1 = ((b1 * x) - (a1 * ys)) + z2
                n2 = (b2 * x) - (a2 * ys)
                z[2 * s] = np.where(mask, n1, z1)  # (a cell below its onset: its state no longer matters)
                z[2 * s + 1] = np.where(mask, n2, z2)
                x = ys
            assert x.dtype == np.float32
            y[t] = np.where(mask, x, np.float32(0))
    return y


def records(y, delay, fs):
    """y: float32 [T, ...] one band's filter output, delay: float32 [...] -> float32 [..., 12], NaN without an onset"""
    y = np.asarray(y, np.float32)
    reached, t0 = _onsets(delay)
    shape = t0.shape
    T = y.shape[0]
    t_end = T - tail_n(fs)
    n50, n80 = n50_n80(fs)
    zero, ten = np.float32(0), np.float32(10.0)
    out = np.full(shape + (12,), QNAN, np.float32)

    with np.errstate(all="ignore"):
        # first walk: E0 and the clarity sums
        E = np.zeros(shape, np.float32)
        e50, e80, l50, l80, mom = (np.zeros(shape, np.float32) for _ in range(5))
        for t in range(T - 1, -1, -1):
            k = np.int32(t) - t0
            mask = reached & (k >= 0)
            if not mask.any():
                continue
            e = y[t] * y[t]
            E = np.where(mask, E + e, E)
            l50 = np.where(mask & (k == n50), E, l50)
            l80 = np.where(mask & (k == n80), E, l80)
            e50 = np.where(mask & (k < n50), e50 + e, e50)
            e80 = np.where(mask & (k < n80), e80 + e, e80)
            m = k.astype(np.float32) * e
            mom = np.where(mask, mom + m, mom)
        e0 = E

        # second walk: the same additions, the ratio, the level and the three fits
        E = np.zeros(shape, np.float32)
        r_end = np.zeros(shape, np.float32)
        n = [np.zeros(shape, np.int64) for _ in RANGES]
        kmin = [np.zeros(shape, np.int64) for _ in RANGES]
        kmax = [np.zeros(shape, np.int64) for _ in RANGES]
        sy = [np.zeros(shape, np.float64) for _ in RANGES]
        sky = [np.zeros(shape, np.float64) for _ in RANGES]
        for t in range(T - 1, -1, -1):
            k = np.int32(t) - t0
            mask = reached & (k >= 0)
            if not mask.any():
                continue
            e = y[t] * y[t]
            E = np.where(mask, E + e, E)
            if t >= t_end:
                continue
            r = E / e0
            assert r.dtype == np.float32
            if t == t_end - 1:
                r_end = np.where(mask, r, r_end)
            member = [mask & (r <= hi) & (r >= lo) for hi, lo in RANGES]
            some = member[0] | member[1] | member[2]
            if not some.any():
                continue
            L = np.zeros(shape, np.float32)
            L[some] = ten * log10f(r[some])
            yy = L.astype(np.float64)
            ky = k.astype(np.float64) * yy
            for j, mj in enumerate(member):
                sy[j] = np.where(mj, sy[j] + yy, sy[j])
                sky[j] = np.where(mj, sky[j] + ky, sky[j])
                kmax[j] = np.where(mj & (n[j] == 0), k, kmax[j])
                kmin[j] = np.where(mj, k, kmin[j])
                n[j] = n[j] + mj

        before_tail = reached & (t0 < t_end)
        for j, (hi, lo) in enumerate(RANGES):
            nd = n[j].astype(np.float64)
            kbar = (kmin[j].astype(np.float64) + kmax[j].astype(np.float64)) * 0.5
            slope = (sky[j] - (kbar * sy[j])) / ((nd * ((nd * nd) - 1.0)) / 12.0)
            value = ((-60.0 / slope) / np.float64(fs)).astype(np.float32)
            ok = before_tail & (r_end < lo) & (n[j] >= 2)
            out[..., j][ok] = value[ok]
            out[..., 3 + j][reached] = n[j].astype(np.float32)[reached]
        out[..., 6][reached] = e0[reached]
        out[..., 7][before_tail] = ten * log10f(r_end[before_tail])
        q50, q80 = e50 / l50, e80 / l80
        out[..., 8][reached] = (ten * log10f(q50[reached]))
        out[..., 9][reached] = (ten * log10f(q80[reached]))
        out[..., 10][reached] = (e50 / (e50 + l50))[reached]
        out[..., 11][reached] = ((mom / e0) / np.float32(fs))[reached]
    assert e0.dtype == np.float32 and mom.dtype == np.float32 and all(v.dtype == np.float64 for v in sy + sky)
    return out


def band_metrics(hist, delay, fs, coefs):
    """hist: float32 [T, ...], delay: float32 [...], coefs: float32 [n, 10] -> float32 [..., n, 12].  The bands run side by side as
    one more array axis (each band's arithmetic is its own: nothing is summed across that axis)"""
    coefs = np.asarray(coefs, np.float32).reshape(-1, 10)
    hist = np.asarray(hist, np.float32)
    delay = np.asarray(delay, np.float32)
    n = coefs.shape[0]
    hb = np.broadcast_to(hist[:, None], (hist.shape[0], n) + delay.shape)
    db = np.broadcast_to(delay[None], (n,) + delay.shape)
    cb = coefs.T.reshape((10, n) + (1,) * delay.ndim)
    return np.moveaxis(records(band_filter(hb, db, cb), db, fs), 0, -2)


def band_metrics_ir(p, fs, onset, coefs):
    """the same for one impulse response p[T] with its onset step: float32 [n, 12]"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return band_metrics(p, np.array([onset], np.float32), fs, coefs)[0]
