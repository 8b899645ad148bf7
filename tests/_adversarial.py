"""Pressure histories the stencil never produces, for the analysis passes (PvAmdSetHistoryPlane puts them in front of the device
kernels; tests/test_host_adversarial.py holds the host restatements to their numpy restatements on the very same inputs).

generate() takes a recorded history [T, A, B] and returns a replacement of the same shape.  It changes only samples at
t >= t_first(cell), the first step at which the cell's recorded sample is non-zero -- the one structural rule the passes rely on
(include/planeverb_amd.h, PvAmdSetHistoryPlane): nothing sounds ahead of the wave front.  A cell's family is a hash of (X, Y), so
that the 64 cells of a wave, and the 16 or 4 lanes of neighbouring cells, hold different families:

   0 noise      iid normal samples x 10^U(-3, 3) per cell
   1 decay      an exponential decay x noise; the per-cell rate puts -5 / -25 / -35 dB both inside and beyond T
   2 silent     all zeros after the onset: E0 = 0
   3 single     one non-zero sample: at t_first, at T - 1, or at onset + n50
   4 constant
   5 nyquist    alternating +a, -a
   6 quiet      |p| in [1e-23, 1e-19]: squares are subnormal or zero
   7 loud       |p| in [2e19, 1e20]: squares overflow to inf, the ratios are inf / inf
   8 spikes     a 1e-12 floor with sparse unit spikes
   9 control    the run's own samples, untouched
  10 nonfinite  NaN, +inf and -inf samples laid over the cell's family, at positions that include t_first and T - 1; at most
                one such cell in any 64 consecutive cells of the tile-major order the kernels deal to their waves

The families 0 .. 9 are finite.  Everything is float32 and a pure function of (hist, seed, tile, onset, fs)."""
import numpy as np

FAMILIES = ("noise", "decay", "silent", "single", "constant", "nyquist", "quiet", "loud", "spikes", "control", "nonfinite")
N_FINITE = 10
NONFINITE = 10
POISON_PITCH, POISON_AT = 96, 70  # in-tile offsets POISON_AT + k POISON_PITCH: >= 71 cells apart, across tile ends too
NO_ONSET = np.float32(3.0e38)


def first_nonzero(hist):
    """t_first [A, B]: the first step with a non-zero sample, T where there is none"""
    nz = np.asarray(hist) != 0
    return np.where(nz.any(axis=0), nz.argmax(axis=0), hist.shape[0]).astype(np.int64)


def cell_hash(X, Y, seed):
    """a 32-bit mix of (X, Y, seed), the shape of X"""
    h = (np.asarray(X, np.uint64) * np.uint64(0x9E3779B1) + np.asarray(Y, np.uint64) * np.uint64(0x85EBCA6B)
         + np.uint64(seed) * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return h


def families(shape, seed, tile, t_first, T):
    """family [A, B] of every cell: -1 where the cell never sounds, NONFINITE on the sparse poisoned cells"""
    A, B = shape
    X, Y = np.meshgrid(np.arange(A), np.arange(B), indexing="ij")
    h = cell_hash(X, Y, seed)
    fam = (h % np.uint64(N_FINITE)).astype(np.int64)
    rows, cols = tile
    in_tile = (X % rows) * cols + (Y % cols)
    assert rows * cols >= POISON_AT + 1 and POISON_PITCH > 64 and POISON_AT > 64
    fam[in_tile % POISON_PITCH == POISON_AT] = NONFINITE
    fam[t_first >= T] = -1
    return fam, h


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def generate(hist, seed, tile, onset=None, fs=1443):
    """-> (replacement float32 like hist, family int64 [A, B]); onset [A, B] (the run's onset map; default t_first), fs: for the
    'single' family's onset + n50"""
    hist = np.asarray(hist, np.float32)
    T, A, B = hist.shape
    t_first = first_nonzero(hist)
    fam, h = families((A, B), seed, tile, t_first, T)
    on = t_first if onset is None else np.where(np.asarray(onset) < NO_ONSET, np.asarray(onset), 0).astype(np.int64)
    n50 = int(np.float32(0.05) * np.float32(fs))
    rng = np.random.default_rng(seed)
    out = hist.copy()
    t = np.arange(T)[:, None]
    for k in range(NONFINITE + 1):
        xs, ys = np.nonzero(fam == k)
        n = len(xs)
        if n == 0:
            continue
        tf = t_first[xs, ys][None, :]  # [1, n]
        live = t >= tf               # [T, n]
        base = (h[xs, ys] >> np.uint64(8)) % np.uint64(N_FINITE) if k == NONFINITE else np.full(n, k, np.uint64)
        v = np.zeros((T, n))
        for b in range(N_FINITE):
            c = np.nonzero(base == b)[0]
            if len(c):
                v[:, c] = _finite(rng, b, T, len(c), tf[:, c], on[xs, ys][c], n50, hist[:, xs[c], ys[c]])
        with np.errstate(over="ignore"):
            v = v.astype(np.float32)
        if k == NONFINITE:
            v = _poison(rng, v, t_first[xs, ys], h[xs, ys])
        out[:, xs, ys] = np.where(live, v, hist[:, xs, ys])
    return out, fam


def _finite(rng, b, T, n, tf, on, n50, own):
    """family b for n cells: float64 [T, n] (the caller keeps only t >= t_first)"""
    t = np.arange(T)[:, None]
    k = np.maximum(t - tf, 0)
    if b == 0:
        return rng.standard_normal((T, n)) * 10.0 ** rng.uniform(-3, 3, n)
    if b == 1:  # level at the end of the record: -200, -60, -30, -15, -6, -3 dB
        t60 = np.maximum(T - tf, 1) * rng.choice([0.3, 1.0, 2.0, 4.0, 10.0, 20.0], n)
        return rng.standard_normal((T, n)) * 10.0 ** (-3.0 * k / t60) * 10.0 ** rng.uniform(-2, 2, n)
    if b == 2:
        return np.zeros((T, n))
    if b == 3:
        where = rng.integers(0, 3, n)
        at = np.where(where == 0, tf[0], np.where(where == 1, T - 1, on + n50))
        at = np.where((at >= T) | (at < tf[0]), T - 1, at)
        return np.where(t == at[None, :], _signs(rng, n) * 10.0 ** rng.uniform(-3, 3, n), 0.0)
    if b == 4:
        return np.broadcast_to(_signs(rng, n) * 10.0 ** rng.uniform(-2, 2, n), (T, n)).copy()
    if b == 5:
        return np.where(t % 2 == 0, 1.0, -1.0) * 10.0 ** rng.uniform(-2, 2, n)
    if b == 6:
        return _signs(rng, (T, n)) * 10.0 ** rng.uniform(-23, -19, (T, n))
    if b == 7:
        return _signs(rng, (T, n)) * rng.uniform(2e19, 1e20, (T, n))
    if b == 8:
        return np.where(rng.random((T, n)) < 0.04, _signs(rng, (T, n)), 1e-12)
    return own.astype(np.float64)


def _poison(rng, v, t_first, h):
    """NaN, +inf and -inf into float32 v [T, n], at positions that include t_first and T - 1"""
    T, n = v.shape
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    variant = (h >> np.uint64(16)) % np.uint64(5)
    for c in range(n):
        tf, var = int(t_first[c]), int(variant[c])
        mid = int(rng.integers(tf, T))
        if var == 0:
            v[tf, c] = nan
        elif var == 1:
            v[T - 1, c] = inf
        elif var == 2:
            v[tf, c], v[T - 1, c] = -inf, nan
        elif var == 3:
            v[mid, c] = -inf
        else:
            v[tf, c], v[mid, c], v[T - 1, c] = inf, nan, -inf
    return v


def finite_cells(hist):
    """[A, B]: every sample of the cell is finite"""
    return np.isfinite(hist).all(axis=0)


def clean_for_velocity(finite):
    """[A, B]: the cell and its (X - 1, Y) and (X, Y - 1) neighbours are finite (what a cell's vx, vy are made from)"""
    ok = finite.copy()
    ok[1:, :] &= finite[:-1, :]
    ok[:, 1:] &= finite[:, :-1]
    return ok


def describe(fam, cell):
    f = int(fam[tuple(cell)])
    return "cell %s, family %s" % (tuple(int(c) for c in cell), FAMILIES[f] if f >= 0 else "never sounds")


# ------------------------------------------------------------------------------------------------------------------------------
# expected values: the host restatements of the six kinds that read the pressure alone, cell by cell
# ------------------------------------------------------------------------------------------------------------------------------
PRESSURE_KINDS = ("room_metrics", "decay_times", "echo_criterion", "band_metrics", "modulation", "spectrum")


def host_expected(api, p, delay, fs, coefs, mod_hz, bins, pulse, kinds=PRESSURE_KINDS):
    """api.host_<kind> of every reached cell of p [T, gx, gy] with the onset map delay [gx, gy]: {kind: float32 [gx, gy, *width]},
    NaN records without an onset.  coefs = the band coefficient sets [n, 10], mod_hz = the 14 modulation frequencies (None: the
    default), bins = the spectrum's frequencies, pulse = the run's pulse table [T]"""
    gx, gy = delay.shape
    call = {"room_metrics": lambda q, t0: api.host_room_metrics(q, fs, t0),
            "decay_times": lambda q, t0: api.host_decay_times(q, fs, t0),
            "echo_criterion": lambda q, t0: api.host_echo_criterion(q, fs, t0),
            "band_metrics": lambda q, t0: api.host_band_metrics(q, fs, t0, coefs),
            "modulation": lambda q, t0: api.host_modulation(q, fs, t0, coefs, mod_hz),
            "spectrum": lambda q, t0: api.host_spectrum(q, fs, t0, bins, pulse)}
    out = {}
    cells = np.argwhere(delay < NO_ONSET)
    cols = np.ascontiguousarray(p[:, cells[:, 0], cells[:, 1]].T)  # [N, T]: a cell's samples side by side
    for k in kinds:
        first = call[k](cols[0], int(delay[tuple(cells[0])]))
        m = np.full((gx, gy) + first.shape, np.nan, np.float32)
        for q, (x, y) in zip(cols, cells):
            m[x, y] = call[k](q, int(delay[x, y]))
        out[k] = m
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# a solver's history replaced (Solver.set_history_plane)
# ------------------------------------------------------------------------------------------------------------------------------
def history(s):
    """the recorded planes of the last run as history_plane returns them: float32 [T, gx + 1, gy + 1]"""
    return np.stack([s.history_plane(t) for t in range(s.T)])


def inject(s, seed):
    """replace the history of the solver's last run by generate()'s: (the planes set [T, gx + 1, gy + 1], family [gx + 1, gy + 1],
    the run's onset map [gx, gy])"""
    rec = history(s)
    delay = s.results()[1]
    onset = np.full(rec.shape[1:], np.finfo(np.float32).max, np.float32)
    onset[:s.gx, :s.gy] = delay
    new, fam = generate(rec, seed, (s.info.tileRows, s.info.tileCols), onset, s.fs)
    for t in range(s.T):
        s.set_history_plane(t, new[t])
    return new, fam, delay
