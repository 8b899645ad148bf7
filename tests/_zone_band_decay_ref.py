"""Numpy restatement of the zone band decay of include/planeverb_amd.h (PvAmdZoneBandDecay), written from the definition and
independent of csrc/pv_zone_band_decay.h: the band filter as a loop over numpy float32 scalars (every product and sum a float32
operation of its own, denormals kept; filtered_history is the same loop over all cells at once), the three-level sum and the fits of tests/_zone_decay_ref.py applied to the filtered
history, and the clarity of the curve in Python floats with math.log10 (the C library's)."""
import math
import warnings

import numpy as np

import _zone_decay_ref as zd
from _zone_decay_ref import ABSOLUTE, NO_ONSET, ONSET, same_doubles  # noqa: F401  (re-exported for the tests)

DTYPE = np.dtype([("edt", "<f8"), ("t20", "<f8"), ("t30", "<f8"), ("e0", "<f8"), ("depth", "<f8"), ("c50", "<f8"), ("c80", "<f8"),
                  ("d50", "<f8"), ("ts", "<f8"), ("n_edt", "<i4"), ("n_t20", "<i4"), ("n_t30", "<i4"), ("n_cells", "<i4"),
                  ("t_first", "<i4"), ("t_last", "<i4")])
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0], np.float32)  # b0 = 1, everything else 0, in both sections: y = x


def filter_backwards(x, t0, c10):
    """y[t] for t0 <= t < T of one cell: two sections in transposed direct form II, float32, from t = T - 1 (state +0.0f) DOWN TO
    t0; samples below t0 are neither read nor written (they stay +0.0f)"""
    c = [np.float32(v) for v in c10]
    y = np.zeros(len(x), np.float32)
    z = [np.float32(0.0)] * 4
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (overflow and invalid are values here, not mistakes)
        for t in range(len(x) - 1, t0 - 1, -1):
            v = np.float32(x[t])
            for s in (0, 1):
                b0, b1, b2, a1, a2 = c[5 * s:5 * s + 5]
                out = np.float32(np.float32(b0 * v) + z[2 * s])
                n1 = np.float32(np.float32(np.float32(b1 * v) - np.float32(a1 * out)) + z[2 * s + 1])
                n2 = np.float32(np.float32(b2 * v) - np.float32(a2 * out))
                z[2 * s], z[2 * s + 1] = n1, n2
                v = out
            y[t] = v
    return y


def filtered_history(p, delay, labels, c10):
    """float32 [T, gx, gy]: y of every labelled cell with an onset, +0.0f everywhere else.  The same loop as filter_backwards, over
    all those cells at once: elementwise float32 operations, each rounded on its own; a cell takes no step below its onset"""
    p = np.asarray(p, np.float32)
    T = p.shape[0]
    member = (np.asarray(labels) != 0) & (np.asarray(delay) != NO_ONSET)
    t0 = np.where(member, delay, T).astype(np.int64)
    c = [np.float32(v) for v in c10]
    y = np.zeros_like(p)
    z = [np.zeros(p.shape[1:], np.float32) for _ in range(4)]
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            on = t >= t0
            v = p[t]
            for s in (0, 1):
                b0, b1, b2, a1, a2 = c[5 * s:5 * s + 5]
                out = (b0 * v) + z[2 * s]
                n1 = ((b1 * v) - (a1 * out)) + z[2 * s + 1]
                n2 = (b2 * v) - (a2 * out)
                z[2 * s], z[2 * s + 1] = np.where(on, n1, z[2 * s]), np.where(on, n2, z[2 * s + 1])
                v = out
            y[t] = np.where(on, v, np.float32(0.0))
    return y


def ratio(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def level10(r):
    """10 * log10(r) as the C library has it: NaN for NaN, -inf for 0, +inf for +inf"""
    if r != r:
        return math.nan
    if r == 0.0:
        return -math.inf
    if r == math.inf:
        return math.inf
    return 10.0 * math.log10(r) if r > 0.0 else math.nan


def clarity(etc, fs, j0):
    """(c50, c80, d50, ts) of the curve etc[T] whose beginning is slot j0"""
    T = len(etc)
    e = [float(v) for v in etc]
    edc = [0.0] * (T + 1)
    for j in range(T - 1, -1, -1):
        edc[j] = edc[j + 1] + e[j]
    out = []
    sums = []
    for sec in (np.float32(0.05), np.float32(0.08)):
        n = int(sec * np.float32(fs))
        m = min(j0 + n, T)
        early = 0.0
        for j in range(j0, m):
            early = early + e[j]
        sums.append((early, edc[m]))
        out.append(level10(ratio(early, edc[m])))
    out.append(ratio(sums[0][0], sums[0][0] + sums[0][1]))
    moment = 0.0
    for j in range(j0, T):
        moment = moment + float(j - j0) * e[j]
    out.append(ratio(ratio(moment, edc[j0]), float(fs)))
    return out


def zone_band_decay(p, delay, fs, labels, n_zones, coefs, align):
    """-> (records [n_zones, n_bands], etc [n_zones, n_bands, T], edc likewise)"""
    p = np.asarray(p, np.float32)
    coefs = np.asarray(coefs, np.float32).reshape(-1, 10)
    T, nb = p.shape[0], coefs.shape[0]
    out = np.zeros((n_zones, nb), DTYPE)
    etc, edc = np.zeros((n_zones, nb, T)), np.zeros((n_zones, nb, T))
    for b in range(nb):
        y = filtered_history(p, delay, labels, coefs[b])
        rec, e, d = zd.zone_decay(y, delay, fs, labels, n_zones, align)
        etc[:, b], edc[:, b] = e, d
        for z in range(n_zones):
            for f in zd.DTYPE.names:
                out[z, b][f] = rec[z][f]
            j0 = int(rec[z]["t_first"]) if align == ABSOLUTE and rec[z]["n_cells"] > 0 else 0
            for f, v in zip(("c50", "c80", "d50", "ts"), clarity(e[z], fs, j0)):
                out[z, b][f] = v
    return out, etc, edc


def same_records(a, b):
    """all 96 bytes of every record, NaNs by position"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    for f in a.dtype.names:
        x, y = np.ascontiguousarray(a[f]), np.ascontiguousarray(b[f])
        if x.dtype.kind == "f":
            if not same_doubles(x, y):
                return False
        elif not np.array_equal(x, y):
            return False
    return True


def first_difference(a, b):
    for i in np.ndindex(a.shape):
        for f in a.dtype.names:
            x, y = a[i][f], b[i][f]
            if not (x == y or (x != x and y != y)) or (x == y == 0 and np.signbit(x) != np.signbit(y)):
                return i, f, x, y
    return None
