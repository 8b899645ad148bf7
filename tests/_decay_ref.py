"""numpy restatement of the decay times (include/planeverb_amd.h, PvAmdDecayTimes), written from the definition:

    t0 = (int)delay (FLT_MAX: not reached), tEnd = T - (int)(0.01f * (float)fs), e(t) = p(t) * p(t),
    E(T) = +0, E(t) = E(t + 1) + e(t) for t = T - 1 down to t0, E0 = E(t0), r(t) = E(t) / E0, L(t) = 10 log10f(r(t)), k = t - t0;
    a step t in [t0, tEnd) belongs to the range (hi, lo) iff lo <= r(t) <= hi; per range, in decreasing t:
    n, kmin, kmax, Sy = sum L, Sky = sum k L (double), slope = (Sky - kbar Sy) / (n (n^2 - 1) / 12), kbar = (kmin + kmax) / 2,
    value = (float)((-60 / slope) / fs) if the range is complete (t0 < tEnd and r(tEnd - 1) < lo) and n >= 2, else quiet NaN;
    depth = L(tEnd - 1) if t0 < tEnd else NaN;  record = edt, t20, t30, n_edt, n_t20, n_t30, E0, depth.

e, E, r and L are float32, Sy, Sky and the derive step float64; every product, sum and quotient is rounded on its own and every
sum is strictly sequential in DECREASING t from +0: per-cell arrays and ONE python loop over t per walk, running downwards (the
first walk finds E0, the second repeats the very same additions).  No np.sum, no np.cumsum, no np.dot.  The logarithm is the
host libm's own log10f (tests/_room_metrics_ref.py); the division is numpy's float32 division."""
import numpy as np

from _room_metrics_ref import NO_ONSET, log10f  # noqa: F401

NAMES = ("edt", "t20", "t30", "n_edt", "n_t20", "n_t30", "e0", "depth")
RANGES = ((np.float32(1.0), np.float32(0.1)),
          (np.float32(0.31622776), np.float32(0.0031622776)),
          (np.float32(0.31622776), np.float32(0.00031622776)))
QNAN = np.array([0x7fc00000], np.uint32).view(np.float32)[0]


def tail_n(fs):
    return int(np.float32(0.01) * np.float32(fs))


def decay_times(hist, delay, fs):
    """hist: float32 [T, ...] recorded pressure, delay: float32 [...] onset map -> float32 [..., 8], NaN without an onset"""
    hist = np.asarray(hist, np.float32)
    delay = np.asarray(delay, np.float32)
    T = hist.shape[0]
    t_end = T - tail_n(fs)
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    zero = np.float32(0)
    ten = np.float32(10.0)

    # first walk: E0 = E(t0)
    E = np.zeros(delay.shape, np.float32)
    for t in range(T - 1, -1, -1):
        mask = reached & (np.int32(t) >= t0)
        if not mask.any():
            continue
        p = hist[t]
        E = E + np.where(mask, p * p, zero)
    e0 = E

    # second walk: the same additions, the ratio, the level and the three fits
    E = np.zeros(delay.shape, np.float32)
    r_end = np.zeros(delay.shape, np.float32)
    n = [np.zeros(delay.shape, np.int64) for _ in RANGES]
    kmin = [np.zeros(delay.shape, np.int64) for _ in RANGES]
    kmax = [np.zeros(delay.shape, np.int64) for _ in RANGES]
    sy = [np.zeros(delay.shape, np.float64) for _ in RANGES]
    sky = [np.zeros(delay.shape, np.float64) for _ in RANGES]
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            k = np.int32(t) - t0
            mask = reached & (k >= 0)
            if not mask.any():
                continue
            p = hist[t]
            E = E + np.where(mask, p * p, zero)
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
            L = np.zeros(delay.shape, np.float32)
            L[some] = ten * log10f(r[some])  # (L(t) is needed only where the step belongs to a range)
            y = L.astype(np.float64)
            ky = k.astype(np.float64) * y
            for j, m in enumerate(member):
                sy[j] = np.where(m, sy[j] + y, sy[j])
                sky[j] = np.where(m, sky[j] + ky, sky[j])
                kmax[j] = np.where(m & (n[j] == 0), k, kmax[j])
                kmin[j] = np.where(m, k, kmin[j])
                n[j] = n[j] + m

        out = np.full(delay.shape + (8,), QNAN, np.float32)
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
    assert e0.dtype == np.float32 and E.dtype == np.float32 and all(v.dtype == np.float64 for v in sy + sky)
    return out


def decay_times_ir(p, fs, onset):
    """the same for one impulse response p[T] with its onset step"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return decay_times(p, np.array([onset], np.float32), fs)[0]
