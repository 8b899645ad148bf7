"""numpy restatement of the room metrics (include/planeverb_amd.h, PvAmdRoomMetrics), written from the definition:

    t0 = (int)delay (FLT_MAX: not reached), e(t) = p(t) * p(t), k = t - t0, t = t0 .. T - 1,
    n50 = (int)(0.05f * (float)fs), n80 = (int)(0.08f * (float)fs),
    e50 / l50 = sum e over k < n50 / k >= n50, e80 / l80 the same with n80, total = sum e, moment = sum ((float)k * e),
    c50 = 10 log10f(e50 / l50), c80 = 10 log10f(e80 / l80), d50 = e50 / (e50 + l50), ts = (moment / total) / (float)fs.

Everything is float32, every product and sum rounded on its own, every sum strictly sequential in increasing t from +0: per-cell
arrays and ONE python loop over t (a term outside a sum's range is +0, the identity of these non-negative sums).  The two
logarithms are the host libm's own log10f, one call per distinct argument (numpy's float32 log10 may take a SIMD path with
other bits)."""
import ctypes

import numpy as np

NAMES = ("c50", "c80", "d50", "ts", "e50", "l50", "e80", "l80", "total", "moment")
NO_ONSET = np.float32(3.0e38)  # delay >= this: FLT_MAX, the cell was not reached
AUDIBLE = np.float32(0.00000316)  # the analysis' onset threshold

_libm = ctypes.CDLL("libm.so.6")
_libm.log10f.restype = ctypes.c_float
_libm.log10f.argtypes = [ctypes.c_float]


def n50(fs):
    return int(np.float32(0.05) * np.float32(fs))


def n80(fs):
    return int(np.float32(0.08) * np.float32(fs))


def threshold_onset(p):
    """first step whose |p| exceeds the audible threshold (the analysis' onset scan), or -1"""
    hit = np.abs(np.asarray(p, np.float32)) > AUDIBLE
    return int(np.argmax(hit)) if hit.any() else -1


def log10f(x):
    """libm's log10f on a float32 array: one call per distinct value"""
    x = np.ascontiguousarray(x, np.float32)
    u, inv = np.unique(x.view(np.uint32), return_inverse=True)
    vals = np.array([_libm.log10f(ctypes.c_float(float(v))) for v in u.view(np.float32)], np.float32)
    return vals[inv].reshape(x.shape)


def room_metrics(hist, delay, fs):
    """hist: float32 [T, ...] recorded pressure, delay: float32 [...] onset map -> float32 [..., 10], NaN without an onset"""
    hist = np.asarray(hist, np.float32)
    delay = np.asarray(delay, np.float32)
    T = hist.shape[0]
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    a50, a80 = n50(fs), n80(fs)
    zero = np.float32(0)
    e50, l50, e80, l80, total, moment = (np.zeros(delay.shape, np.float32) for _ in range(6))
    for t in range(T):
        k = np.int32(t) - t0
        mask = reached & (k >= 0)
        if not mask.any():
            continue
        p = hist[t]
        e = p * p
        e50 = e50 + np.where(mask & (k < a50), e, zero)
        l50 = l50 + np.where(mask & (k >= a50), e, zero)
        e80 = e80 + np.where(mask & (k < a80), e, zero)
        l80 = l80 + np.where(mask & (k >= a80), e, zero)
        total = total + np.where(mask, e, zero)
        moment = moment + np.where(mask, k.astype(np.float32) * e, zero)
    out = np.full(delay.shape + (10,), np.nan, np.float32)
    with np.errstate(all="ignore"):
        r50 = (e50 / l50)[reached]
        r80 = (e80 / l80)[reached]
        out[..., 0][reached] = np.float32(10.0) * log10f(r50)
        out[..., 1][reached] = np.float32(10.0) * log10f(r80)
        out[..., 2][reached] = (e50 / (e50 + l50))[reached]
        out[..., 3][reached] = ((moment / total) / np.float32(fs))[reached]
    for i, v in enumerate((e50, l50, e80, l80, total, moment)):
        out[..., 4 + i][reached] = v[reached]
    assert out.dtype == np.float32 and all(v.dtype == np.float32 for v in (e50, l50, e80, l80, total, moment))
    return out


def room_metrics_ir(p, fs, onset):
    """the same for one impulse response p[T] with its onset step"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return room_metrics(p, np.array([onset], np.float32), fs)[0]
