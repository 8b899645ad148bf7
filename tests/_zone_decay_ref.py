"""Numpy restatement of the zone decay of include/planeverb_amd.h (PvAmdZoneDecay), written from the definition and independent
of csrc/pv_zone_decay.h: plain loops over slots, rows, blocks and the butterfly (tests/_zone_ref.py).  Doubles are Python floats and
numpy float64 (IEEE, every operation rounded on its own); the levels come from math.log10 -- CPython's call into the C library's
log10, the one the product uses -- never from np.log10, which may be another implementation."""
import math

import numpy as np

from _zone_ref import BLOCK, butterfly, first_difference, same_records  # noqa: F401  (re-exported for the tests)

ABSOLUTE, ONSET = 0, 1
NO_ONSET = np.float32(np.finfo(np.float32).max)  # FLT_MAX
DTYPE = np.dtype([("edt", "<f8"), ("t20", "<f8"), ("t30", "<f8"), ("e0", "<f8"), ("depth", "<f8"), ("n_edt", "<i4"),
                  ("n_t20", "<i4"), ("n_t30", "<i4"), ("n_cells", "<i4"), ("t_first", "<i4"), ("t_last", "<i4")])
# the ranges of the per-cell decay times as ratios of E(t0): the float32 literals of the definition, widened to double
HI = [float(np.float32(v)) for v in (1.0, 0.31622776, 0.31622776)]
LO = [float(np.float32(v)) for v in (0.1, 0.0031622776, 0.00031622776)]


def tail_n(fs):
    """the curve's last 10 ms enter no fit: (int)(0.01f * (float)fs)"""
    return int(np.float32(0.01) * np.float32(fs))


def energy_curve(p, t0, member, align):
    """etc[j] of one zone: p float32 [T, gx, gy], t0 int [gx, gy], member bool [gx, gy] -> float64 [T]"""
    T, gx, gy = p.shape
    nb = (gy + BLOCK - 1) // BLOCK
    etc = np.zeros(T, np.float64)
    xs, ys = np.nonzero(member)
    for j in range(T):
        v = np.zeros((gx, nb * BLOCK), np.float64)  # +0.0 for every cell without a sample for slot j and for columns past gy
        has = np.zeros((gx, nb * BLOCK), bool)
        for X, Y in zip(xs, ys):
            t = j if align == ABSOLUTE else int(t0[X, Y]) + j
            if t0[X, Y] <= t < T:
                x = np.float64(p[t, X, Y])
                v[X, Y] = x * x
                has[X, Y] = True
        total = np.float64(0.0)
        for X in range(gx):
            if not has[X].any():
                continue  # a row without such a member is skipped
            row = np.float64(0.0)
            for b in range(nb):
                if has[X, b * BLOCK:(b + 1) * BLOCK].any():  # ... and so is a block
                    row = row + butterfly(v[X, b * BLOCK:(b + 1) * BLOCK])
            total = total + row
        etc[j] = total
    return etc


def schroeder(etc):
    """edc[j] = edc[j + 1] + etc[j] from edc[T] = +0.0"""
    edc = np.zeros(len(etc), np.float64)
    e = 0.0
    for j in range(len(etc) - 1, -1, -1):
        e = e + float(etc[j])
        edc[j] = e
    return edc


def level(r):
    if r != r:
        return math.nan
    return 10.0 * math.log10(r) if r > 0.0 else -math.inf


def ratio(a, b):
    """a / b as IEEE has it (b may be +0.0)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def fits(edc, T, fs, align, t_first, t_last):
    """(edt, t20, t30, e0, depth, n_edt, n_t20, n_t30) of a zone with at least one member"""
    j0 = t_first if align == ABSOLUTE else 0
    j_end = T - tail_n(fs) if align == ABSOLUTE else T - tail_n(fs) - t_last
    e0 = float(edc[j0])
    values, counts = [], []
    for hi, lo in zip(HI, LO):
        n, sy, sky, kmin, kmax = 0, 0.0, 0.0, 0, 0
        for j in range(j_end - 1, j0 - 1, -1):  # decreasing j, as the per-cell definition walks its curve
            r = ratio(edc[j], e0)
            if r <= hi and r >= lo:
                k = j - j0
                y = level(r)
                sy = sy + y
                sky = sky + float(k) * y
                if n == 0:
                    kmax = k
                kmin = k
                n += 1
        complete = j0 < j_end and ratio(edc[j_end - 1], e0) < lo
        value = math.nan
        if complete and n >= 2:
            kbar = (float(kmin) + float(kmax)) * 0.5
            fn = float(n)
            slope = ratio(sky - (kbar * sy), (fn * ((fn * fn) - 1.0)) / 12.0)
            value = ratio(ratio(-60.0, slope), float(fs))
        values.append(value)
        counts.append(n)
    depth = level(ratio(edc[j_end - 1], e0)) if j0 < j_end else math.nan
    return values + [e0, depth] + counts


def zone_decay(p, delay, fs, labels, n_zones, align):
    """p float32 [T, gx, gy], delay float32 [gx, gy] (FLT_MAX: no onset), labels uint8 [gx, gy] -> (records [n_zones], etc, edc)"""
    p = np.asarray(p, np.float32)
    T = p.shape[0]
    delay = np.asarray(delay, np.float32)
    reached = delay != NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int64)
    out = np.zeros(n_zones, DTYPE)
    etc, edc = np.zeros((n_zones, T)), np.zeros((n_zones, T))
    for z in range(1, n_zones + 1):
        member = (np.asarray(labels) == z) & reached
        r = out[z - 1]
        r["n_cells"] = member.sum()
        etc[z - 1] = energy_curve(p, t0, member, align)
        edc[z - 1] = schroeder(etc[z - 1])
        if r["n_cells"] == 0:
            r["t_first"] = r["t_last"] = -1
            r["e0"] = 0.0
            for f in ("edt", "t20", "t30", "depth"):
                r[f] = np.nan
            continue
        r["t_first"], r["t_last"] = t0[member].min(), t0[member].max()
        v = fits(edc[z - 1], T, fs, align, int(r["t_first"]), int(r["t_last"]))
        for f, x in zip(("edt", "t20", "t30", "e0", "depth", "n_edt", "n_t20", "n_t30"), v):
            r[f] = x
    return out, etc, edc


def same_doubles(a, b):
    """bit for bit, NaNs by position"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))
