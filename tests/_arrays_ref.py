"""Source arrays (include/planeverb_amd.h, "Source arrays"; csrc/pv_arrays.h) restated in numpy from the header's text: the taps of
a member in float64, the response in np.float32 operation by operation, the onset by the reference's rule.  The host restatement
(tests/test_host_arrays.py) and the kernels (tests/test_gpu_arrays.py) are held to it bit for bit."""
import math

import numpy as np

NEAREST, LAGRANGE3 = 0, 1
FLT_MAX = np.float32(3.4028234663852886e38)
ONSET_THRESHOLD = np.float32(0.00000316)


class Refused(Exception):
    pass


def taps(fs, T, gain, delay_seconds, interp):
    """(delays [n], weights float32 [n]) of one member, or Refused"""
    gain, delay_seconds = np.float32(gain), np.float32(delay_seconds)
    if interp not in (NEAREST, LAGRANGE3):
        raise Refused("interp")
    if not (np.isfinite(gain) and np.isfinite(delay_seconds)) or delay_seconds < 0:
        raise Refused("member")
    d = float(delay_seconds) * float(fs)
    if not d < T:
        raise Refused("d >= T")
    if interp == NEAREST:
        r = math.floor(d + 0.5)
        if not r < T:
            raise Refused("rounds to T")
        return [int(r)], np.array([gain], np.float32)
    n = math.floor(d)
    mu = d - n
    if mu == 0.0:
        return [int(n)], np.array([gain], np.float32)
    if n < 1:
        raise Refused("n < 1")
    D = mu + 1.0
    L = [-(((D - 1.0) * (D - 2.0)) * (D - 3.0)) / 6.0, ((D * (D - 2.0)) * (D - 3.0)) / 2.0,
         -((D * (D - 1.0)) * (D - 3.0)) / 2.0, ((D * (D - 1.0)) * (D - 2.0)) / 6.0]
    return [int(n) - 1 + j for j in range(4)], np.array([np.float32(float(gain) * L[j]) for j in range(4)], np.float32)


def lagrange_double(gain, mu):
    """the four products gain * L_j in float64, before the rounding to float32"""
    D = mu + 1.0
    L = [-(((D - 1.0) * (D - 2.0)) * (D - 3.0)) / 6.0, ((D * (D - 2.0)) * (D - 3.0)) / 2.0,
         -((D * (D - 1.0)) * (D - 3.0)) / 2.0, ((D * (D - 1.0)) * (D - 2.0)) / 6.0]
    return [float(np.float32(gain)) * l for l in L]


def expand(members, fs, T, interp):
    """members = [(gain, delay_seconds)] of one array -> (tap_member, tap_delay, tap_weight) in the response's order"""
    tm, td, tw = [], [], []
    for i, (g, d) in enumerate(members):
        dl, w = taps(fs, T, g, d, interp)
        tm += [i] * len(dl)
        td += dl
        tw += list(w)
    return np.array(tm, np.int32), np.array(td, np.int32), np.array(tw, np.float32)


def shifted(p, delay):
    """q(t) = p(t - delay), +0 outside 0 .. T - 1"""
    T = len(p)
    q = np.zeros(T, np.float32)
    if delay >= 0:
        if delay < T:
            q[delay:] = p[:T - delay]
    else:
        q[:T + delay] = p[-delay:]
    return q


def response(p, tap_member, tap_delay, tap_weight):
    """y float32 [T] from member rows p[M, T]: y = y + (w * p_m(t - delay)), every product and sum a float32 operation of its own"""
    p = np.asarray(p, np.float32)
    p = p.reshape(1, -1) if p.ndim == 1 else p
    y = np.zeros(p.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for m, d, w in zip(tap_member, tap_delay, tap_weight):
            prod = (np.float32(w) * shifted(p[int(m)], int(d))).astype(np.float32)
            y = (y + prod).astype(np.float32)
    return y


def onset(y):
    """the first t with |y(t)| > 0.00000316f as a float32, else FLT_MAX (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(np.abs(np.asarray(y, np.float32)) > ONSET_THRESHOLD)[0]
    return np.float32(hit[0]) if hit.size else FLT_MAX
