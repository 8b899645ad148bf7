"""CPU: every host restatement of the analysis kinds (api.host_*) against its independent numpy restatement (tests/_*_ref.py), bit
for bit and NaN by position, on the adversarial histories of tests/_adversarial.py: a synthetic [160, 24, 24] block with synthetic
onsets, every family.  tests/test_gpu_injected_history.py holds the device kernels to the host restatements on the same families;
its expected values are only as good as this check, which needs no device."""
import numpy as np
import pytest

import _adversarial as adv
import _bands_ref
import _decay_ref
import _echo_ref
import _echogram_ref
import _lateral_ref
import _lobes_ref
import _modulation_ref
import _room_metrics_ref
import _spectrum_ref
import _zone_decay_ref
import _zone_ref
from conftest import same_bits
from test_gpu_analysis_maps import BANDS, BINS, EDGES, SLOTS

T, A, B, FS, SEED = 160, 24, 24, 1443, 20261019
TILE = (12, 12)  # 144 cells a tile: one poisoned cell in each
FLT_MAX = np.float32(np.finfo(np.float32).max)


def block(T=T):
    """(recorded history [T, A, B], onset map [A, B]): a front that leaves cell (5, 7) at one cell a step, decaying noise behind it,
    a 4 x 4 wall that never sounds; onsets 0 .. 3 steps behind the front, T - 1 and T - 3 planted, none in the wall.  In a run too
    short for the front to arrive (tests/test_host_run_lengths.py) a cell has no onset, and every onset lies in [t_first, T - 1]"""
    rng = np.random.default_rng(SEED)
    X, Y = np.meshgrid(np.arange(A), np.arange(B), indexing="ij")
    t_first = np.abs(X - 5) + np.abs(Y - 7)
    t = np.arange(T)[:, None, None]
    hist = (rng.standard_normal((T, A, B)) * 10.0 ** (-0.02 * np.maximum(t - t_first, 0)) * (t >= t_first)).astype(np.float32)
    hist[t_first[None] == t] = np.float32(0.5)  # (the front itself is never zero)
    wall = (X >= 14) & (X < 18) & (Y >= 3) & (Y < 7)
    hist[:, wall] = 0
    delay = (t_first + rng.integers(0, 4, (A, B))).astype(np.float32)
    delay[20, 20], delay[21, 3] = T - 1, T - 3
    delay = np.clip(delay, t_first, T - 1).astype(np.float32)  # (changes nothing where T > 37: the front has passed every cell)
    delay[wall | (t_first >= T)] = FLT_MAX
    return hist, delay


@pytest.fixture(scope="module")
def case(pvlib):
    hist, delay = block()
    p, fam = adv.generate(hist, SEED, TILE, delay, FS)
    vx, _ = adv.generate(hist, SEED + 1, TILE, delay, FS)
    vy, _ = adv.generate(hist, SEED + 2, TILE, delay, FS)
    reached = delay < adv.NO_ONSET
    assert np.array_equal(adv.first_nonzero(hist) < T, reached) and np.array_equal(fam >= 0, reached)
    for f in range(len(adv.FAMILIES)):
        assert ((fam == f) & reached).sum() >= 4, adv.FAMILIES[f]
    # the generator keeps the rule: nothing before the cell's own first recorded sample
    before = np.arange(T)[:, None, None] < adv.first_nonzero(hist)[None]
    for q in (p, vx, vy):
        assert (q[before] == 0).all() and np.array_equal(adv.finite_cells(q), fam != adv.NONFINITE)
        q.setflags(write=False)
    assert np.array_equal(p[:, fam == 9], hist[:, fam == 9]) and not np.array_equal(p[:, fam == 0], hist[:, fam == 0])
    with np.errstate(over="ignore", under="ignore"):
        loud, quiet = p[:, fam == 7], p[:, fam == 6]
        assert (p[:, fam == 2] == 0).all() and np.isinf((loud * loud)[loud != 0]).all()
        sq = (quiet * quiet)[quiet != 0]
    assert (sq < np.finfo(np.float32).tiny).all() and (sq == 0).any() and (sq > 0).any()
    return p, vx, vy, delay, fam


def check(name, got, want, delay, fam):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = ~same_bits(got, want)
    if bad.any():
        cell = np.argwhere(bad)[0][:2]
        c = tuple(cell)
        raise AssertionError("%s: %d values differ, first at %s (onset %s): host %s, numpy %s" % (
            name, bad.sum(), adv.describe(fam, cell), delay[c], got[c][bad[c]][:4], want[c][bad[c]][:4]))


def per_cell(delay, width, fn):
    out = np.full(delay.shape + width, np.nan, np.float32)
    for x, y in np.argwhere(delay < adv.NO_ONSET):
        out[x, y] = fn(x, y, int(delay[x, y]))
    return out


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the numpy restatements overflow and divide as the definitions say)
def test_pressure_kinds(pvlib, case):
    p, _, _, delay, fam = case
    coefs = pvlib.host_band_coefs(FS, BANDS, 1)
    pulse = pvlib.host_pulse(25.0, 25.0, 275)[:T]
    got = adv.host_expected(pvlib, p, delay, FS, coefs, None, BINS, pulse)
    c, s = pvlib.host_spectrum_tables(T, FS, BINS)
    want = {"room_metrics": _room_metrics_ref.room_metrics(p, delay, FS),
            "decay_times": _decay_ref.decay_times(p, delay, FS),
            "echo_criterion": _echo_ref.echo_criterion(p, delay, FS),
            "band_metrics": _bands_ref.band_metrics(p, delay, FS, coefs),
            "modulation": _modulation_ref.modulation(p, delay, coefs, pvlib.host_modulation_table(T, FS, None)),
            "spectrum": _spectrum_ref.spectrum(p, delay, c, s, pulse)}
    for k in adv.PRESSURE_KINDS:
        check(k, got[k], want[k], delay, fam)
    # the families do what they are for: a silent cell has E0 = +0 and no decay time; a loud one an infinite E0
    e0 = got["decay_times"][..., 6]
    assert (e0[fam == 2] == 0).all() and np.isnan(got["decay_times"][..., 0][fam == 2]).all()
    assert np.isinf(e0[(fam == 7) & (delay < T - 1)]).all()


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_velocity_kinds(pvlib, case):
    p, vx, vy, delay, fam = case
    col = lambda q, x, y: np.ascontiguousarray(q[:, x, y])  # noqa: E731
    got = per_cell(delay, (11,), lambda x, y, t0: pvlib.host_lateral_fraction(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0))
    check("lateral_fraction", got, _lateral_ref.lateral_fraction(p, vx, vy, delay, FS), delay, fam)
    got = per_cell(delay, (1 + 3 * SLOTS[1],),
                   lambda x, y, t0: pvlib.host_echogram(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0, *SLOTS))
    check("echogram", got, _echogram_ref.echogram(p, vx, vy, delay, FS, *SLOTS), delay, fam)
    got = per_cell(delay, (1 + 5 * (len(EDGES) + 1),),
                   lambda x, y, t0: pvlib.host_lobes(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0, EDGES))
    check("lobes", got, _lobes_ref.lobes(p, vx, vy, delay, FS, EDGES), delay, fam)


def zones():
    lab = np.random.default_rng(SEED).integers(0, 4, (A, B)).astype(np.uint8)
    lab[2:9, 12:20] = 4  # (a block; zone 5 has no cell)
    lab[5, 10], lab[17, 22] = 1, 2  # (two of the cells with non-finite samples)
    return lab


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("align", ["absolute", "onset"])
def test_zone_decay(pvlib, case, align):
    """the ensemble curves of zones that hold loud, quiet, silent and non-finite cells"""
    p, _, _, delay, _ = case
    lab = zones()
    rec, etc, edc = pvlib.host_zone_decay(p, delay, FS, lab, 5, align)
    wrec, wetc, wedc = _zone_decay_ref.zone_decay(p, delay, FS, lab, 5, ["absolute", "onset"].index(align))
    assert _zone_decay_ref.same_doubles(etc, wetc), np.argwhere(etc != wetc)[:4]
    assert _zone_decay_ref.same_doubles(edc, wedc), np.argwhere(edc != wedc)[:4]
    assert _zone_decay_ref.same_records(rec, wrec), _zone_decay_ref.first_difference(rec, wrec)
    assert not np.isfinite(etc[:2]).all() and np.isfinite(etc[2:]).any() and np.nanmax(etc) > 1e38  # (doubles: a loud square is finite)


@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_zone_stats(pvlib, case):
    """the reductions over maps that hold inf and NaN values"""
    p, _, _, delay, _ = case
    lab = zones()
    for name, m in (("decay_times", _decay_ref.decay_times(p, delay, FS)), ("room_metrics", _room_metrics_ref.room_metrics(p, delay, FS))):
        got, want = pvlib.host_zone_stats(m, lab, 5), _zone_ref.zone_stats(m, lab, 5)
        assert _zone_ref.same_records(got, want), "%s: %s" % (name, _zone_ref.first_difference(got, want))
        assert got["n_posinf"].sum() > 0 and got["n_nan"].sum() > 0 and got["n_finite"].sum() > 0, name
