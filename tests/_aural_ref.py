"""The auralisation restated in numpy from the text of include/planeverb_amd.h (section "Auralisation"): the resampling tables in
double, the response, the output and the mix in float32 with every product and every sum rounded on its own.  numpy's float32
and float64 +, *, / and sqrt are IEEE operations; sin is math.sin, the host libm's, as the header says."""
import math

import numpy as np

MAX_TAPS = 1024
F32 = np.float32


class Refused(Exception):
    pass


def i0(x):
    """the header's series, element-wise on a float64 array"""
    x = np.asarray(x, np.float64)
    s, term, h = np.ones_like(x), np.ones_like(x), 0.5 * x
    for k in range(1, 61):
        hk = h / float(k)
        term = term * (hk * hk)
        s = s + term
    return s


def shape(fs, T, rate, Z, beta):
    """(c, half, L, K), or Refused"""
    if not (isinstance(rate, int) and 1000 <= rate <= 384000):
        raise Refused("rate")
    if not (isinstance(Z, int) and 2 <= Z <= 64):
        raise Refused("zero crossings")
    if not (math.isfinite(beta) and 0.0 <= beta <= 20.0):
        raise Refused("beta")
    c = float(rate) / float(fs) if rate < fs else 1.0
    half = float(Z) / c
    K = 2 * int(math.floor(half)) + 1
    L = int(math.floor((float(T - 1) * float(rate)) / float(fs))) + 1
    if K > MAX_TAPS:
        raise Refused("K")
    if L * K > (1 << 24):
        raise Refused("L * K")
    return c, half, L, K


def taps(fs, T, rate, Z, beta):
    """(first int32 [L], w float32 [L, K])"""
    beta = float(F32(beta))
    c, half, L, K = shape(fs, T, rate, Z, beta)
    n = np.arange(L, dtype=np.float64)
    u = (n * float(fs)) / float(rate)
    first = np.ceil(u - half).astype(np.int64)
    t = first[:, None] + np.arange(K, dtype=np.int64)[None, :]
    d = u[:, None] - t.astype(np.float64)
    inside = ~(np.abs(d) > half)
    a = c * d
    pa = math.pi * a
    with np.errstate(all="ignore"):
        sinc = np.array([math.sin(v) for v in pa.ravel()], np.float64).reshape(pa.shape) / pa
    sinc[a == 0.0] = 1.0
    q = d / half
    q = 1.0 - q * q
    q[q < 0.0] = 0.0
    with np.errstate(all="ignore"):
        v = (c * sinc) * (i0(beta * np.sqrt(q)) / i0(np.float64(beta)))
    w = np.where(inside, v, 0.0).astype(F32)
    return first.astype(np.int32), w


def resample(p, first, w):
    """responses float32 [L, R] of samples p [T, R] (or [T]): h = h + (w[n][j] * p(first[n] + j)), j ascending, from +0"""
    p = np.asarray(p, F32)
    one = p.ndim == 1
    p = p.reshape(p.shape[0], -1)
    T, (L, K) = p.shape[0], w.shape
    h = np.zeros((L, p.shape[1]), F32)
    zero = np.zeros(p.shape[1], F32)
    with np.errstate(all="ignore"):
        for j in range(K):
            t = first.astype(np.int64) + j
            ok = (t >= 0) & (t < T)
            v = np.where(ok[:, None], p[np.clip(t, 0, T - 1)], zero[None, :])
            h = h + (w[:, j][:, None] * v)
    return h[:, 0] if one else h


def convolve(h, x):
    """o float32 [N + L - 1]: for k = max(0, m - N + 1) .. min(L - 1, m) ascending o = o + (h[k] * x[m - k]); no other term"""
    h, x = np.asarray(h, F32).reshape(-1), np.asarray(x, F32).reshape(-1)
    L, N = h.size, x.size
    M = N + L - 1
    o = np.zeros(M, F32)
    with np.errstate(all="ignore"):
        for k in range(L):  # (output m takes tap k where 0 <= m - k < N: the slice k .. k + N - 1)
            o[k:k + N] = o[k:k + N] + (h[k] * x)
    return o


def chunk_walk(L, N, B, C):
    """The tiled kernel's walk of k restated from DESIGN.md 4.29, one string per block of B outputs: the block at m0 walks its k
    range, max(0, m0 - N + 1) .. min(L - 1, the block's last output), in chunks of C taps from the range's first tap; a chunk at k0
    is 'W' (whole: every (output, tap) pair of a FULL block and the chunk is a term of the definition) where
    k0 + C - 1 <= min(L - 1, m0) and k0 >= m0 + B - N, else 'g' (general).  Not a reference of any value: the GPU cases assert
    with it that they reach the pattern they were written for."""
    M = N + L - 1
    walks = []
    for m0 in range(0, M, B):
        k_begin, k_end = max(0, m0 - N + 1), min(L - 1, min(m0 + B - 1, M - 1))
        walks.append("".join("W" if k0 + C - 1 <= min(L - 1, m0) and k0 >= m0 + B - N else "g" for k0 in range(k_begin, k_end + 1, C)))
    return walks


def mix(outputs, route, gain):
    """mix float32 [M] over the routed receivers in increasing r: mix = mix + (gain[r] * o_r[m])"""
    y = np.zeros(outputs.shape[1], F32)
    with np.errstate(all="ignore"):
        for r in range(outputs.shape[0]):
            if route[r] >= 0:
                y = y + (F32(gain[r]) * outputs[r])
    return y


def render(responses, signals, route, gain):
    """(outputs float32 [R, M], mix [M]) of responses [R, L]; an unrouted receiver holds zeros"""
    R, L = responses.shape
    N = signals.shape[1]
    out = np.zeros((R, N + L - 1), F32)
    for r in range(R):
        if route[r] >= 0:
            out[r] = convolve(responses[r], signals[route[r]])
    return out, mix(out, route, gain)
