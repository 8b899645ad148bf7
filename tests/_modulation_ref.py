"""numpy restatement of the modulation records (include/planeverb_amd.h, PvAmdModulation), written from the definition:

    y(t)     the band filter's output (tests/_bands_ref.py band_filter, by import): two float32 biquads BACKWARDS in time from
             t = T - 1 (state +0) down to the cell's onset t0; nothing below t0 enters
    e(t)     = y(t) * y(t)
    sums     in DECREASING t from +0:  E += e;  re[i] += e * cos[t][i];  im[i] += e * sin[t][i]   (i = 0 .. 13)
    record   a = re[i] / E,  b = im[i] / E,  m[i] = sqrt((a * a) + (b * b))
             snr[i] = 15 where m[i] >= 1, else v = 10 log10f(m[i] / (1 - m[i])) with v < -15 -> -15, v > 15 -> 15 (a NaN stays)
             ti[i] = (snr[i] + 15) / 30;   mti = (ti[0] + ti[1] + ... + ti[13], sequential from +0) / 14
             15 floats per band: m[0 .. 13], mti.  E == 0: 15 quiet NaNs

Vectorised over cells and over the 14 modulation frequencies (one more array axis: nothing is summed across it except the last
line's sequential sum), ONE python loop over t, running downwards; every product, sum, quotient and root is a numpy float32
operation of its own.  No np.sum, no np.dot, no np.fft.  The table (cos, sin per step and frequency) and the band coefficients
are INPUTS: the bit-level tests take them from the library, so that two libms cannot disagree about a cosine."""
import numpy as np

from _bands_ref import band_filter
from _decay_ref import QNAN
from _room_metrics_ref import NO_ONSET, log10f

M = 14
DEFAULT_HZ = (0.63, 0.8, 1.0, 1.25, 1.6, 2.0, 2.5, 3.15, 4.0, 5.0, 6.3, 8.0, 10.0, 12.5)


def table64(T, fs, hz=None):
    """the table of the definition from python floats (double) and math.cos / math.sin: float32 [T, 14, 2]"""
    import math
    hz = np.asarray(DEFAULT_HZ if hz is None else hz, np.float32)
    out = np.empty((T, M, 2), np.float32)
    for t in range(T):
        for i in range(M):
            ph = (2.0 * math.pi * float(hz[i]) * float(t)) / float(fs)
            out[t, i, 0] = np.float32(math.cos(ph))
            out[t, i, 1] = np.float32(math.sin(ph))
    return out


def transfer_index(m):
    """ti of float32 m (any shape)"""
    m = np.asarray(m, np.float32)
    one, f15, f30, ten = np.float32(1), np.float32(15), np.float32(30), np.float32(10)
    with np.errstate(all="ignore"):
        v = ten * log10f(m / (one - m))
        v = np.where(v < -f15, -f15, np.where(v > f15, f15, v)).astype(np.float32)
        snr = np.where(m >= one, f15, v).astype(np.float32)
        ti = (snr + f15) / f30
    assert ti.dtype == np.float32
    return ti


def records(y, delay, tab):
    """y: float32 [T, ...] one band's filter output (+0 outside a cell's range), delay: float32 [...], tab: float32 [T, 14, 2]
    -> float32 [..., 15], NaN without an onset"""
    y = np.asarray(y, np.float32)
    tab = np.asarray(tab, np.float32)
    delay = np.asarray(delay, np.float32)
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int32)
    shape = t0.shape
    T = y.shape[0]
    assert tab.shape == (T, M, 2)
    E = np.zeros(shape, np.float32)
    re = np.zeros(shape + (M,), np.float32)
    im = np.zeros(shape + (M,), np.float32)
    out = np.full(shape + (M + 1,), QNAN, np.float32)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            mask = reached & (np.int32(t) >= t0)
            if not mask.any():
                continue
            e = y[t] * y[t]
            E = np.where(mask, E + e, E)
            ec = e[..., None] * tab[t, :, 0]
            es = e[..., None] * tab[t, :, 1]
            re = np.where(mask[..., None], re + ec, re)
            im = np.where(mask[..., None], im + es, im)
        assert E.dtype == np.float32 and re.dtype == np.float32 and im.dtype == np.float32
        a = re / E[..., None]
        b = im / E[..., None]
        m = np.sqrt((a * a) + (b * b))
        ti = transfer_index(m)
        s = np.zeros(shape, np.float32)
        for i in range(M):
            s = s + ti[..., i]
        mti = s / np.float32(14.0)
        assert m.dtype == np.float32 and mti.dtype == np.float32
    ok = reached & (E != 0)
    out[..., :M][ok] = m[ok]
    out[..., M][ok] = mti[ok]
    return out


def modulation(hist, delay, coefs, tab):
    """hist: float32 [T, ...], delay: float32 [...], coefs: float32 [n, 10], tab: float32 [T, 14, 2] -> float32 [..., n, 15]"""
    coefs = np.asarray(coefs, np.float32).reshape(-1, 10)
    hist = np.asarray(hist, np.float32)
    delay = np.asarray(delay, np.float32)
    return np.stack([records(band_filter(hist, delay, c), delay, tab) for c in coefs], axis=-2)


def modulation_ir(p, onset, coefs, tab):
    """the same for one impulse response p[T] with its onset step: float32 [n, 15]"""
    p = np.asarray(p, np.float32).reshape(-1, 1)
    return modulation(p, np.array([onset], np.float32), coefs, tab)[0]


def combine_mti(mti, alpha, beta):
    """sum(alpha[k] mti[k]) - sum(beta[k] sqrt(mti[k] mti[k + 1])), float32, sequential, clamped to [0, 1]"""
    mti, alpha, beta = (np.asarray(v, np.float32).reshape(-1) for v in (mti, alpha, beta))
    s = np.float32(0)
    for k in range(len(mti)):
        s = s + alpha[k] * mti[k]
    r = np.float32(0)
    for k in range(len(mti) - 1):
        r = r + beta[k] * np.sqrt(mti[k] * mti[k + 1])
    v = np.float32(s - r)
    return np.float32(0) if v < 0 else (np.float32(1) if v > 1 else v)
