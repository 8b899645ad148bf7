"""numpy restatement of the waterfall records (include/planeverb_amd.h, Waterfall), written from the definition:

    bins hz[j], tables c[t, j] / s[t, j] = (float)cos / sin((2 pi hz[j] t) / fs) over ABSOLUTE run time (handed in: the library's own
    tables, PvAmdHostSpectrumTables, checked against numpy in double by tests/test_host_spectrum.py),
    slices: slice k starts k * ns steps after the receiver's onset t0, ns = (int)(sliceSeconds * (float)fs) in float32,
    re_j = im_j = +0;  for t = T - 1 DOWN TO t0:  re_j = re_j + (p(t) * c[t, j]),  im_j = im_j + (p(t) * s[t, j]),
                       and where t == t0 + k * ns for a k < m:  R[k, j] = re_j, I[k, j] = im_j;
    slices that start at or past T keep R = I = +0,
    record: (float)t0, (float)#{k : t0 + k * ns < T}, R[0, :], I[0, :], level[k, j] = 10 log10f(((R * R) + (I * I)) / spow_j),
    spow_j = (sre * sre) + (sim * sim) of the spectrum's sums over the pulse table with onset 0 (tests/_spectrum_ref.py).

Everything is float32, every product and sum rounded on its own, every sum strictly sequential in DECREASING t from +0: arrays over
receivers and bins and ONE python loop over t (a receiver whose walk has ended adds +0, which leaves a sum that started at +0
unchanged -- and nothing is read off it any more).  No np.sum, no np.dot.  log10f is the host libm's own."""
import numpy as np

from _room_metrics_ref import NO_ONSET, log10f
from _spectrum_ref import source


def tables(api, T, fs, hz):
    """the library's tables [T, n] for any number of bins (PvAmdHostSpectrumTables takes 32 at a time; a column depends on its own
    frequency alone)"""
    hz = np.asarray(hz, np.float32).reshape(-1)
    cs = [api.host_spectrum_tables(T, fs, hz[j:j + 32]) for j in range(0, len(hz), 32)]
    return np.concatenate([c for c, _ in cs], axis=1), np.concatenate([s for _, s in cs], axis=1)


def slice_steps(slice_seconds, fs):
    """ns = (int)(sliceSeconds * (float)fs), the product in float32"""
    return int(np.float32(slice_seconds) * np.float32(fs))


def floats(n, m):
    return 2 + 2 * n + m * n


def sums(p, t0, live, c, s, ns, m):
    """p: float32 [T, N], t0: int [N], live: bool [N], c / s: float32 [T, n] -> R, I: float32 [N, m, n] (+0 where a slice starts
    at or past T, and for the receivers that are not live)"""
    p = np.asarray(p, np.float32)
    c = np.asarray(c, np.float32)
    s = np.asarray(s, np.float32)
    T, n = c.shape
    N = p.shape[1]
    assert p.shape[0] == T and s.shape == c.shape and t0.shape == (N,) and live.shape == (N,)
    zero = np.float32(0)
    re = np.zeros((N, n), np.float32)
    im = np.zeros((N, n), np.float32)
    R = np.zeros((N, m, n), np.float32)
    I = np.zeros((N, m, n), np.float32)
    t0 = t0.astype(np.int64)
    for t in range(T - 1, -1, -1):
        inside = live & (t >= t0)
        if not inside.any():
            continue
        w = inside[:, None]
        q = p[t][:, None]
        re = re + np.where(w, q * c[t][None, :], zero)
        im = im + np.where(w, q * s[t][None, :], zero)
        k = (t - t0) // ns
        hit = inside & ((t - t0) % ns == 0) & (k < m)
        for i in np.nonzero(hit)[0]:
            R[i, k[i]] = re[i]
            I[i, k[i]] = im[i]
    assert re.dtype == np.float32 and im.dtype == np.float32
    return R, I


def waterfall(p, delay, c, s, ns, m, pulse):
    """p: float32 [T, N] the receivers' samples side by side, delay: float32 [N] their onsets (>= NO_ONSET: none; NaN rows), pulse:
    float32 [T] -> the records, float32 [N, 2 + 2 n + m n]"""
    p = np.asarray(p, np.float32)
    delay = np.asarray(delay, np.float32)
    T, n = np.asarray(c).shape
    live = delay < NO_ONSET
    t0 = np.where(live, delay, 0).astype(np.int64)
    assert ((t0 >= 0) & (t0 < T)).all()
    R, I = sums(p, t0, live, c, s, ns, m)
    spow = source(pulse, c, s)[:, 2]
    with np.errstate(all="ignore"):
        ratio = ((R * R) + (I * I)) / spow[None, None, :]
        level = np.float32(10.0) * log10f(ratio.reshape(-1)).reshape(ratio.shape)
    assert ratio.dtype == np.float32 and level.dtype == np.float32
    out = np.full((len(delay), floats(n, m)), np.nan, np.float32)
    count = np.minimum((T - 1 - t0) // ns + 1, m)
    out[:, 0] = t0.astype(np.float32)
    out[:, 1] = count.astype(np.float32)
    out[:, 2:2 + n] = R[:, 0]
    out[:, 2 + n:2 + 2 * n] = I[:, 0]
    out[:, 2 + 2 * n:] = level.reshape(len(delay), m * n)
    out[~live] = np.nan
    return out


def waterfall_ir(p, onset, c, s, ns, m, pulse):
    """the same for one impulse response p[T] with its onset step: float32 [2 + 2 n + m n]"""
    return waterfall(np.asarray(p, np.float32).reshape(-1, 1), np.array([onset], np.float32), c, s, ns, m, pulse)[0]


def parts(rec, n, m):
    """records [N, F] -> onset [N], slices [N], response [N, n, 2], level [N, m, n] (the dict of Solver.waterfall)"""
    rec = np.asarray(rec, np.float32)
    N = rec.shape[0]
    return {"onset": rec[:, 0], "slices": rec[:, 1], "response": np.stack([rec[:, 2:2 + n], rec[:, 2 + n:2 + 2 * n]], axis=-1),
            "level": rec[:, 2 + 2 * n:].reshape(N, m, n)}
