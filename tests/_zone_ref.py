"""Numpy restatement of the zone statistics of include/planeverb_amd.h (PvAmdZoneStat), written from the definition and
independent of csrc/pv_zones.h: a plain loop over rows, blocks and the butterfly.  Doubles are numpy float64 (IEEE, every
operation rounded on its own); nothing here is vectorised across the order of a sum."""
import numpy as np

BLOCK = 64
DTYPE = np.dtype([("sum", "<f8"), ("mean", "<f8"), ("m2", "<f8"), ("std", "<f8"), ("min", "<f4"), ("max", "<f4"),
                  ("argmin", "<i4"), ("argmax", "<i4"), ("n_finite", "<i4"), ("n_nan", "<i4"), ("n_posinf", "<i4"),
                  ("n_neginf", "<i4")])


def butterfly(v):
    """v: float64 [64] -> v[0] after v[i] = v[i] + v[i + s] for every i that is a multiple of 2 s, s = 1, 2, 4, 8, 16, 32"""
    v = np.array(v, np.float64)
    assert v.shape == (BLOCK,)
    s = 1
    while s < BLOCK:
        for i in range(0, BLOCK, 2 * s):
            v[i] = v[i] + v[i + s]
        s *= 2
    return v[0]


def three_level_sum(v):
    """v: float64 [gx, gy] (+0.0 where a cell does not count) -> block butterflies, rows over increasing b, zone over increasing X"""
    gx, gy = v.shape
    nb = (gy + BLOCK - 1) // BLOCK
    pad = np.zeros((gx, nb * BLOCK), np.float64)  # (columns past gy: +0.0)
    pad[:, :gy] = v
    total = np.float64(0.0)
    for X in range(gx):
        row = np.float64(0.0)
        for b in range(nb):
            row = row + butterfly(pad[X, b * BLOCK:(b + 1) * BLOCK])
        total = total + row
    return total


def zone_stats(map, labels, n_zones):
    """map: float32 [gx, gy, *width]; labels: uint8 [gx, gy]; -> structured [n_zones, *width]"""
    m = np.asarray(map, np.float32)
    gx, gy = m.shape[:2]
    width = m.shape[2:]
    m = m.reshape(gx, gy, -1)
    lab = np.asarray(labels)
    out = np.zeros((n_zones, m.shape[2]), DTYPE)
    cell = np.arange(gx * gy, dtype=np.int64).reshape(gx, gy)
    with np.errstate(invalid="ignore"):
        for z in range(1, n_zones + 1):
            member = lab == z
            for k in range(m.shape[2]):
                x = m[:, :, k]
                finite = member & ((x - x) == 0)
                r = out[z - 1, k]
                r["n_finite"] = finite.sum()
                r["n_nan"] = (member & np.isnan(x)).sum()
                r["n_posinf"] = (member & (x == np.inf)).sum()
                r["n_neginf"] = (member & (x == -np.inf)).sum()
                if r["n_finite"] == 0:
                    r["sum"] = 0.0
                    r["mean"] = r["m2"] = r["std"] = np.nan
                    r["min"] = r["max"] = np.nan
                    r["argmin"] = r["argmax"] = -1
                    continue
                xs, cs = x[finite], cell[finite]  # (row-major: increasing cell index)
                lo = cs[xs == xs.min()].min()     # (== : -0.0 and +0.0 tie; the smallest cell among the ties)
                hi = cs[xs == xs.max()].min()
                r["argmin"], r["argmax"] = lo, hi
                r["min"], r["max"] = x.reshape(-1)[lo], x.reshape(-1)[hi]
                xd = x.astype(np.float64)
                r["sum"] = three_level_sum(np.where(finite, xd, 0.0))
                n = np.float64(r["n_finite"])
                mean = r["sum"] / n
                r["mean"] = mean
                d = xd - mean
                r["m2"] = three_level_sum(np.where(finite, d * d, 0.0))
                r["std"] = np.sqrt(r["m2"] / n)
    return out.reshape((n_zones,) + width)


def same_records(a, b):
    """bit for bit: all struct bytes, NaNs compared by position"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    for name in a.dtype.names:
        fa, fb = a[name], b[name]
        if fa.dtype.kind == "f":
            na, nb = np.isnan(fa), np.isnan(fb)
            if not np.array_equal(na, nb):
                return False
            u = np.uint64 if fa.dtype.itemsize == 8 else np.uint32
            if not np.array_equal(np.ascontiguousarray(fa)[~na].view(u), np.ascontiguousarray(fb)[~nb].view(u)):
                return False
        elif not np.array_equal(fa, fb):
            return False
    return True


def first_difference(a, b):
    """for assertion messages: (index, field, a, b) of the first field that differs, None when same_records"""
    for idx in np.ndindex(a.shape):
        for name in a.dtype.names:
            va, vb = a[idx][name], b[idx][name]
            if not ((va != va and vb != vb) or va.tobytes() == vb.tobytes()):
                return idx, name, va, vb
    return None
