"""CPU: the host restatements (api.host_*) against their numpy restatements (tests/_*_ref.py) at every run length of
tests/_run_lengths.py -- runs shorter than a chunk, a ring, the tail, the 50 / 80 ms limits, a slot, a window or a slice, runs
that end on a chunk's edge, and runs longer than the grid's own T.  The input is the adversarial block of
tests/test_host_adversarial.py rebuilt for each T; every comparison is bit for bit, NaN by position.
tests/test_gpu_run_lengths.py holds the device kernels to the host restatements at the same lengths: its expected values are
only as good as this check, which needs no device."""
import numpy as np
import pytest

import _adversarial as adv
import _arrays_ref
import _bands_ref
import _decay_ref
import _echo_ref
import _echogram_ref
import _lateral_ref
import _lobes_ref
import _modulation_ref
import _room_metrics_ref
import _run_lengths as rl
import _spectrum_ref
import _zone_band_decay_ref
import _zone_decay_ref
import test_host_adversarial as tha
import test_host_arrays as arrays
import test_host_waterfall as waterfall
from test_gpu_analysis_maps import BANDS, BINS, EDGES, SLOTS

FS, SEED, TILE = tha.FS, tha.SEED, tha.TILE
assert FS == rl.FS
ALIGNS = ["absolute", "onset"]
_CASES = {}


def pulse_of(pvlib, T):
    """the 275 Hz grid's pulse table for a run of T steps: cut short, or zero after the grid's own T (an extended run)"""
    own = pvlib.host_pulse(25.0, 25.0, 275)
    assert len(own) == rl.GRID_T
    return np.concatenate([own, np.zeros(max(T - len(own), 0), np.float32)])[:T]


def case(T):
    """(p, vx, vy, onset map, family) of the block rebuilt for T steps, checked for the structure the comparisons rely on"""
    if T not in _CASES:
        hist, delay = tha.block(T)
        assert hist.shape == (T, tha.A, tha.B)
        p, fam = adv.generate(hist, SEED, TILE, delay, FS)
        vx, _ = adv.generate(hist, SEED + 1, TILE, delay, FS)
        vy, _ = adv.generate(hist, SEED + 2, TILE, delay, FS)
        reached = delay < adv.NO_ONSET
        t_first = adv.first_nonzero(hist)
        assert np.array_equal(t_first < T, reached) and np.array_equal(fam >= 0, reached) and reached[5, 7]
        assert (delay[reached] >= t_first[reached]).all() and (delay[reached] <= T - 1).all()
        if T >= 38:  # (the front has passed every cell outside the wall: the families of the 160-step block)
            assert reached.sum() == tha.A * tha.B - 16
            for f in range(len(adv.FAMILIES)):
                assert ((fam == f) & reached).sum() >= 4, adv.FAMILIES[f]
            assert (delay == T - 1).any() and (delay == T - 3).any()
        before = np.arange(T)[:, None, None] < t_first[None]
        for q in (p, vx, vy):
            assert (q[before] == 0).all()
            q.setflags(write=False)
        _CASES[T] = (p, vx, vy, delay, fam)
    return _CASES[T]


lengths = pytest.mark.parametrize("T", rl.ALL, ids=rl.ident)


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # (the numpy restatements overflow and divide as the definitions say)
def test_pressure_kinds(pvlib, T):
    p, _, _, delay, fam = case(T)
    coefs = pvlib.host_band_coefs(FS, BANDS, 1)
    pulse = pulse_of(pvlib, T)
    got = adv.host_expected(pvlib, p, delay, FS, coefs, None, BINS, pulse)
    c, s = pvlib.host_spectrum_tables(T, FS, BINS)
    want = {"room_metrics": _room_metrics_ref.room_metrics(p, delay, FS),
            "decay_times": _decay_ref.decay_times(p, delay, FS),
            "echo_criterion": _echo_ref.echo_criterion(p, delay, FS),
            "band_metrics": _bands_ref.band_metrics(p, delay, FS, coefs),
            "modulation": _modulation_ref.modulation(p, delay, coefs, pvlib.host_modulation_table(T, FS, None)),
            "spectrum": _spectrum_ref.spectrum(p, delay, c, s, pulse)}
    for k in adv.PRESSURE_KINDS:
        tha.check(k, got[k], want[k], delay, fam)
        assert np.isnan(got[k][delay >= adv.NO_ONSET]).all(), k


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_velocity_kinds(pvlib, T):
    p, vx, vy, delay, fam = case(T)
    col = lambda q, x, y: np.ascontiguousarray(q[:, x, y])  # noqa: E731
    got = tha.per_cell(delay, (11,), lambda x, y, t0: pvlib.host_lateral_fraction(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0))
    tha.check("lateral_fraction", got, _lateral_ref.lateral_fraction(p, vx, vy, delay, FS), delay, fam)
    got = tha.per_cell(delay, (1 + 3 * SLOTS[1],),
                       lambda x, y, t0: pvlib.host_echogram(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0, *SLOTS))
    tha.check("echogram", got, _echogram_ref.echogram(p, vx, vy, delay, FS, *SLOTS), delay, fam)
    got = tha.per_cell(delay, (1 + 5 * (len(EDGES) + 1),),
                       lambda x, y, t0: pvlib.host_lobes(col(p, x, y), col(vx, x, y), col(vy, x, y), FS, t0, EDGES))
    tha.check("lobes", got, _lobes_ref.lobes(p, vx, vy, delay, FS, EDGES), delay, fam)


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("align", ALIGNS)
def test_zone_decay(pvlib, T, align):
    p, _, _, delay, _ = case(T)
    lab = tha.zones()
    rec, etc, edc = pvlib.host_zone_decay(p, delay, FS, lab, 5, align)
    wrec, wetc, wedc = _zone_decay_ref.zone_decay(p, delay, FS, lab, 5, ALIGNS.index(align))
    assert etc.shape == edc.shape == (5, T)
    assert _zone_decay_ref.same_doubles(etc, wetc), np.argwhere(etc != wetc)[:4]
    assert _zone_decay_ref.same_doubles(edc, wedc), np.argwhere(edc != wedc)[:4]
    assert _zone_decay_ref.same_records(rec, wrec), _zone_decay_ref.first_difference(rec, wrec)
    reached = delay < adv.NO_ONSET
    assert [int(n) for n in rec["n_cells"]] == [int(((lab == z) & reached).sum()) for z in range(1, 6)]


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
@pytest.mark.parametrize("align", ALIGNS)
def test_zone_band_decay(pvlib, T, align):
    p, _, _, delay, _ = case(T)
    lab = tha.zones()
    coefs = pvlib.host_band_coefs(FS, BANDS, 1)
    rec, etc, edc = pvlib.host_zone_band_decay(p, delay, FS, lab, coefs, 5, align)
    wrec, wetc, wedc = _zone_band_decay_ref.zone_band_decay(p, delay, FS, lab, 5, coefs, ALIGNS.index(align))
    assert etc.shape == edc.shape == (5, len(BANDS), T)
    assert _zone_band_decay_ref.same_doubles(etc, wetc), np.argwhere(etc != wetc)[:4]
    assert _zone_band_decay_ref.same_doubles(edc, wedc), np.argwhere(edc != wedc)[:4]
    assert _zone_band_decay_ref.same_records(rec, wrec), _zone_band_decay_ref.first_difference(rec, wrec)


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_waterfall(pvlib, T):
    """two cells of every finite family the run reaches, the (n, m) of test_host_waterfall.SHAPES, a 15-step slice (slices past T
    from T = 15 m down), the cell's onset and 0"""
    p, _, _, delay, fam = case(T)
    pulse = (np.random.default_rng(11).standard_normal(T) * 0.1).astype(np.float32)
    done = 0
    for f in range(adv.N_FINITE):
        for i, (x, y) in enumerate(np.argwhere(fam == f)[:2]):
            n, m = waterfall.SHAPES[(f + i) % len(waterfall.SHAPES)]
            q = np.ascontiguousarray(p[:, x, y])
            for onset in (int(delay[x, y]), 0):
                got = waterfall.check_ir(pvlib, q, FS, onset, waterfall.bins_of(n, FS), 0.0105, m, pulse)
                k = int(got["slices"][0])
                assert np.isneginf(got["level"][0, k:]).all()
                done += 1
    assert done >= (40 if T >= 38 else 2), done


@lengths
@pytest.mark.filterwarnings("ignore::RuntimeWarning")
def test_array_responses(pvlib, T):
    """both interpolations; a member delayed by 0.6 T and one by T - 1.5 steps (its largest tap passes T - 1) where the tap rule
    takes them, beside an undelayed one"""
    p, _, _, delay, fam = case(T)
    cells = np.argwhere(fam >= 0)
    rng = np.random.default_rng(17 + T)
    pick = cells[rng.integers(0, len(cells), 4)]
    rows = np.stack([p[:, x, y] for x, y in pick])
    taken = 0
    for interp in (_arrays_ref.NEAREST, _arrays_ref.LAGRANGE3):
        members = [(1.0, 0.0), (-0.7, 0.0)]
        for gain, d in ((0.9, float(np.float32(0.6 * T / FS))), (0.8, float(np.float32((T - 1.5) / FS)))):
            try:
                _arrays_ref.taps(FS, T, gain, d, interp)
                members.append((gain, d))
                taken += 1
            except _arrays_ref.Refused:
                with pytest.raises(pvlib.PlaneverbError):
                    pvlib.host_array_taps(FS, T, gain, d, interp)
        members += [(0.5, 0.0)] * (4 - len(members))
        arrays.check_response(pvlib, rows, members, FS, interp)
        arrays.check_response(pvlib, np.stack([rows[0], rows[0]]), [(0.7, 0.0), (-0.7, 0.0)], FS, interp)
    assert taken == 4 or T < 4, (T, taken)


@lengths
def test_tap_rule(pvlib, T):
    seen = {"kept": 0, "refused": 0}
    for interp in (_arrays_ref.NEAREST, _arrays_ref.LAGRANGE3):
        for gain in (1.0, -2.5e-3):
            for d in arrays.delays_of(FS, T):
                r = arrays.check_taps(pvlib, FS, T, gain, d, interp)
                seen["refused" if r is None else "kept"] += 1
                assert r is None or min(r[0]) >= 0
    assert all(seen.values()), seen
