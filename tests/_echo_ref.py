"""numpy restatement of the echo criterion (include/planeverb_amd.h, PvAmdEchoCriterion), written from the definition:

    t0 = (int)delay (FLT_MAX: not reached), a(t) = |p(t)|, k = t - t0, t = t0 .. T - 1, N = T - t0,
    speech: w = powf(a, 0.6666667f), nD = (int)(0.009f * (float)fs), nL = (int)(0.05f * (float)fs)
    music:  w = a,                   nD = (int)(0.014f * (float)fs), nL = (int)(0.08f * (float)fs)
    A(k) = A(k-1) + w, B(k) = B(k-1) + ((float)k * w), c(k) = B(k) / A(k),
    x(k) = (c(k) - (k >= nD ? c(k - nD) : +0)) / (float)nD,
    ek / kk: the first maximum of x over every k (strict >, from +0, 0), ekLate / kkLate: the same over k >= nL,
    record: ek, (float)kk / (float)fs, ekLate, (float)kkLate / (float)fs, c(N - 1) / (float)fs;   speech, then music.

Everything is float32, every product, sum and quotient rounded on its own, the sums strictly sequential in increasing k from +0:
per-cell arrays and ONE python loop over t.  c is KEPT per step ([T, ...]), so the lagged term is a look-up of the value computed
nD steps earlier -- the library recomputes it from a second pair of sums instead.  powf is the host libm's own, one call per
distinct value (numpy's float32 power may take a SIMD path with other bits)."""
import ctypes

import numpy as np

NAMES = ("s_ek", "s_tk", "s_ek_late", "s_tk_late", "s_ts", "m_ek", "m_tk", "m_ek_late", "m_tk_late", "m_ts")
NO_ONSET = np.float32(3.0e38)  # delay >= this: FLT_MAX, the cell was not reached
SPEECH_EXPONENT = np.float32(2.0 / 3.0)
SPEECH_CRIT, MUSIC_CRIT = np.float32(1.0), np.float32(1.8)

_libm = ctypes.CDLL("libm.so.6")
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def lags(fs):
    """(speech nD, speech nL, music nD, music nL) in steps"""
    f = np.float32(fs)
    return tuple(int(np.float32(v) * f) for v in (0.009, 0.05, 0.014, 0.08))


def powf(x, y):
    """libm's powf(x, y) on a float32 array: one call per distinct value"""
    x = np.ascontiguousarray(x, np.float32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    f, yy = _libm.powf, float(np.float32(y))
    vals = np.array([f(v, yy) for v in u.view(np.float32).tolist()], np.float32)
    return vals[inv].reshape(x.shape)


def _variant(w, t0, reached, nD, nL, fs):
    """one variant on the weights w [T, ...] -> float32 [..., 5]"""
    T = w.shape[0]
    shape = w.shape[1:]
    zero = np.float32(0)
    A, B, ek, ekl = (np.zeros(shape, np.float32) for _ in range(4))
    kk, kkl = np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    c_all = np.full(w.shape, np.nan, np.float32)
    with np.errstate(all="ignore"):
        for t in range(T):
            k = np.int32(t) - t0
            on = reached & (k >= 0)
            if not on.any():
                continue
            wt = w[t]
            A = np.where(on, A + wt, A)
            B = np.where(on, B + k.astype(np.float32) * wt, B)
            c = B / A
            c_all[t] = c
            lagged = np.where(k >= nD, c_all[t - nD], zero) if t >= nD else zero  # (k >= nD: t - nD >= t0 >= 0)
            x = (c - lagged) / np.float32(nD)
            up = on & (x > ek)
            ek, kk = np.where(up, x, ek), np.where(up, k, kk)
            up = on & (k >= nL) & (x > ekl)
            ekl, kkl = np.where(up, x, ekl), np.where(up, k, kkl)
        f = np.float32(fs)
        out = np.stack([ek, kk.astype(np.float32) / f, ekl, kkl.astype(np.float32) / f, c_all[T - 1] / f], axis=-1)
    assert out.dtype == np.float32 and A.dtype == np.float32 and B.dtype == np.float32
    return out


def echo_criterion(hist, delay, fs):
    """hist: float32 [T, ...] recorded pressure, delay: float32 [...] onset map -> float32 [..., 10], NaN without an onset"""
    hist = np.asarray(hist, np.float32)
    delay = np.asarray(delay, np.float32)
    T = hist.shape[0]
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    nDs, nLs, nDm, nLm = lags(fs)
    assert nDs >= 1
    a = np.abs(hist)
    used = reached & (np.arange(T, dtype=np.int32).reshape((T,) + (1,) * delay.ndim) >= t0)  # [T, ...]
    ws = np.zeros(a.shape, np.float32)
    ws[used] = powf(a[used], SPEECH_EXPONENT)
    out = np.full(delay.shape + (10,), np.nan, np.float32)
    out[..., :5][reached] = _variant(ws, t0, reached, nDs, nLs, fs)[reached]
    out[..., 5:][reached] = _variant(a, t0, reached, nDm, nLm, fs)[reached]
    return out


def echo_criterion_ir(p, fs, onset):
    """the same for one impulse response p[T] with its onset step"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return echo_criterion(p, np.array([onset], np.float32), fs)[0]
