"""numpy restatement of the directional echogram (include/planeverb_amd.h, PvAmdSetEchogram .. PvAmdHostEchogram), written from
the definition:

    ns = (int)(slotSeconds * (float)fs) in float32, onset = (int)delay (FLT_MAX: not reached),
    tEnd = min(onset + ns * nSlots, T); for t = onset .. tEnd - 1, k = t - onset, j = k / ns:
        e[j] += p p;   ix[j] += p vx;   iy[j] += p vy;
    record = n = tEnd - onset, then e[0], ix[0], iy[0], e[1], ix[1], iy[1], ...

p, vx, vy are GIVEN (the velocity is the library's: what PvAmdGetImpulseResponse returns).  Everything is float32, every product
and sum rounded on its own, every slot's sums strictly sequential in increasing t from +0: per-cell arrays and ONE python loop
over t, each slot's sums updated with np.where on that slot's members (a cell that is no member keeps its sum).  No np.sum, no
np.cumsum, no np.dot."""
import numpy as np

NO_ONSET = np.float32(3.0e38)  # delay >= this: FLT_MAX, the cell was not reached
MAX_SLOTS = 32


def slot_steps(slot_seconds, fs):
    return int(np.float32(slot_seconds) * np.float32(fs))


def echogram(p, vx, vy, delay, fs, slot_seconds, n_slots):
    """p, vx, vy: float32 [T, ...], delay: float32 [...] onset map -> float32 [..., 1 + 3 n_slots], NaN without an onset"""
    p, vx, vy = (np.asarray(v, np.float32) for v in (p, vx, vy))
    delay = np.asarray(delay, np.float32)
    assert p.shape == vx.shape == vy.shape and p.shape[1:] == delay.shape
    ns = slot_steps(slot_seconds, fs)
    assert ns >= 1 and 1 <= n_slots <= MAX_SLOTS
    T = p.shape[0]
    reached = delay < NO_ONSET
    t0 = np.where(reached, delay, 0).astype(np.int64)
    t_end = np.minimum(t0 + ns * n_slots, T)
    e, ix, iy = (np.zeros((n_slots,) + delay.shape, np.float32) for _ in range(3))
    for t in range(T):
        k = t - t0
        mask = reached & (k >= 0) & (t < t_end)
        if not mask.any():
            continue
        pt, xt, yt = p[t], vx[t], vy[t]
        j = np.where(mask, k // ns, -1)
        for slot in np.unique(j[mask]):
            member = j == slot
            e[slot] = np.where(member, e[slot] + (pt * pt), e[slot])
            ix[slot] = np.where(member, ix[slot] + (pt * xt), ix[slot])
            iy[slot] = np.where(member, iy[slot] + (pt * yt), iy[slot])
    out = np.full(delay.shape + (1 + 3 * n_slots,), np.nan, np.float32)
    out[..., 0][reached] = (t_end - t0).astype(np.float32)[reached]
    for slot in range(n_slots):
        for c, v in enumerate((e, ix, iy)):
            assert v.dtype == np.float32
            out[..., 1 + 3 * slot + c][reached] = v[slot][reached]
    return out


def echogram_ir(p, vx, vy, fs, onset, slot_seconds, n_slots):
    """the same for one impulse response p[T], vx[T], vy[T] with its onset step"""
    p, vx, vy = (np.asarray(v, np.float32).reshape(-1, 1) for v in (p, vx, vy))
    return echogram(p, vx, vy, np.array([onset], np.float32), fs, slot_seconds, n_slots)[0]
