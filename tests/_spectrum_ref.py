"""numpy restatement of the spectrum records (include/planeverb_amd.h, Spectrum), written from the definition:

    bins hz[j], tables c[t, j] / s[t, j] = (float)cos / sin((2 pi hz[j] t) / fs) over ABSOLUTE run time (handed in: the library's
    own tables, PvAmdHostSpectrumTables, checked against numpy in double by tests/test_host_spectrum.py),
    t0 = (int)delay (FLT_MAX: not reached),
    re_j = sum_{t = t0}^{T - 1} (p(t) * c[t, j]),  im_j = sum_{t = t0}^{T - 1} (p(t) * s[t, j]),
    source: the same sums over the pulse table with onset 0, spow_j = (sre * sre) + (sim * sim),
    level_j = 10 log10f(((re * re) + (im * im)) / spow_j).

Everything is float32, every product and sum rounded on its own, every sum strictly sequential in increasing t from +0: per-cell,
per-bin arrays and ONE python loop over t (a term outside a cell's range is replaced by +0, which leaves a sum that started at
+0 unchanged).  No np.sum, no np.dot.  log10f is the host libm's own (tests/_room_metrics_ref.py)."""
import numpy as np

from _room_metrics_ref import NO_ONSET, log10f, threshold_onset  # noqa: F401  (threshold_onset: for the tests)


def tables_f64(T, fs, hz):
    """the tables in double, not yet rounded to float32: [T, n] each"""
    h = np.asarray(hz, np.float32).astype(np.float64)
    t = np.arange(T, dtype=np.float64)[:, None]
    ph = (2.0 * np.pi * h[None, :] * t) / float(fs)
    return np.cos(ph), np.sin(ph)


def sums(hist, t0, reached, c, s):
    """hist: float32 [T, ...], t0: int [...], reached: bool [...], c / s: float32 [T, n] -> re, im: float32 [..., n]"""
    hist = np.asarray(hist, np.float32)
    c = np.asarray(c, np.float32)
    s = np.asarray(s, np.float32)
    T, n = c.shape
    assert hist.shape[0] == T and s.shape == c.shape
    zero = np.float32(0)
    re = np.zeros(t0.shape + (n,), np.float32)
    im = np.zeros(t0.shape + (n,), np.float32)
    for t in range(T):
        mask = reached & (t >= t0)
        if not mask.any():
            continue
        p = hist[t][..., None]
        m = mask[..., None]
        re = re + np.where(m, p * c[t], zero)
        im = im + np.where(m, p * s[t], zero)
    assert re.dtype == np.float32 and im.dtype == np.float32
    return re, im


def source(pulse, c, s):
    """float32 [n, 3]: sre, sim, spow of the pulse table (onset 0)"""
    pulse = np.asarray(pulse, np.float32).reshape(-1, 1)
    re, im = sums(pulse, np.zeros(1, np.int32), np.ones(1, bool), c, s)
    re, im = re[0], im[0]
    return np.stack([re, im, (re * re) + (im * im)], axis=-1).astype(np.float32)


def spectrum(hist, delay, c, s, pulse):
    """hist: float32 [T, ...] recorded pressure, delay: float32 [...] onset map, pulse: float32 [T] -> float32 [..., n, 3], NaN
    without an onset"""
    delay = np.asarray(delay, np.float32)
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    re, im = sums(hist, t0, reached, c, s)
    spow = source(pulse, c, s)[:, 2]
    out = np.full(delay.shape + (c.shape[1], 3), np.nan, np.float32)
    with np.errstate(all="ignore"):
        ratio = (((re * re) + (im * im)) / spow)[reached]
        level = np.float32(10.0) * log10f(ratio)
    assert ratio.dtype == np.float32 and level.dtype == np.float32
    out[..., 0][reached] = re[reached]
    out[..., 1][reached] = im[reached]
    out[..., 2][reached] = level
    return out


def spectrum_ir(p, onset, c, s, pulse):
    """the same for one impulse response p[T] with its onset step: float32 [n, 3]"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return spectrum(p, np.array([onset], np.float32), c, s, pulse)[0]
