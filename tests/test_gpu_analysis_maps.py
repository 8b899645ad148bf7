"""GPU (-m gpu): the contract the nine per-cell analysis kinds share (csrc/pv_solver_maps.cpp: one record per kind in the solver,
one set of compute / fetch / block / at routines; the reductions of these maps over zones are csrc/pv_solver_zones.cpp's and have
their own test files).  What the numbers are is each kind's own test file's business; here it is the
plumbing: a kind's device buffer, host copy and validity must not leak into another kind's.  Everything is compared bit for bit,
NaNs by position.  One 25 m x 25 m solver at 275 Hz, 160 steps, one box (its cells have no onset: NaN records)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, RES, STEPS = 25.0, 275, 160
LISTENER = (5.0, 0.0, 4.0)
BOX = (12.0, 12.0, 3.0, 3.0, 0.5)  # cells 30 .. 37 of both axes
BANDS, BINS, SLOTS, EDGES = [125.0, 250.0], [63.0, 125.0, 250.0], (0.01, 4), [0.01, 0.08]
# the block straddles a tile boundary in both directions (this grid's tile is 12 x 40; 36 x 40 tiles split it too) and holds box cells
BLOCK = (30, 34, 12, 12)
ON_MAP = [(5.0, 0.0, 6.0), (12.0, 0.0, 12.0), (20.0, 0.0, 20.0)]  # an emitter, inside the box, in the tile diagonally across
OFF_MAP = [(-0.5, 0.0, 3.0), (3.0, 0.0, 30.0)]

# name = the method stem of api.Solver (compute_<name>, <name>, <name>_block, <name>_at); says = how its refusals start;
# width = a record's trailing dimensions under the settings above; setter = what gives the kind a different setting
KINDS = [
    dict(name="room_metrics", says="room metrics", width=(10,), setter=None),
    dict(name="decay_times", says="decay times", width=(8,), setter=None),
    dict(name="lateral_fraction", says="lateral fraction", width=(11,), setter=None),
    dict(name="echo_criterion", says="echo", width=(10,), setter=None),
    dict(name="echogram", says="echogram", width=(13,), setter=lambda s: s.set_echogram(0.02, 3)),
    dict(name="lobes", says="lobes", width=(16,), setter=lambda s: s.set_lobe_windows([0.02, 0.1, 0.2])),
    dict(name="band_metrics", says="band metrics", width=(2, 12), setter=lambda s: s.set_bands([250.0, 500.0])),
    dict(name="modulation", says="modulation", width=(2, 15), setter=lambda s: s.set_modulation_frequencies([0.5 * (i + 1) for i in range(14)])),
    dict(name="spectrum", says="spectrum", width=(3, 3), setter=lambda s: s.set_spectrum_bins([100.0])),
]
BY_NAME = {k["name"]: k for k in KINDS}
IDS = [k["name"] for k in KINDS]


def identical(a, b):
    """same shape, NaNs at the same places, every other value bit for bit"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    live = ~np.isnan(a)
    return np.array_equal(a[live].view(np.uint32), b[live].view(np.uint32))


def compute(s, k):
    return getattr(s, "compute_" + k["name"])()


def whole(s, k):
    return getattr(s, k["name"])()


def block(s, k, r0, c0, nr, nc):
    return getattr(s, k["name"] + "_block")(r0, c0, nr, nc)


def at(s, k, pos):
    return getattr(s, k["name"] + "_at")(pos)


def reads(s, k):
    return [lambda: whole(s, k), lambda: block(s, k, 0, 0, 2, 2), lambda: at(s, k, ON_MAP[0]), lambda: at(s, k, OFF_MAP[0])]


def refused(pvlib, s, k, why):
    for call in reads(s, k):
        with pytest.raises(pvlib.PlaneverbError, match="^%s: %s" % (k["says"], why)):
            call()


def base_settings(s):
    s.set_bands(BANDS)
    s.set_modulation_frequencies(None)
    s.set_spectrum_bins(BINS)
    s.set_echogram(*SLOTS)
    s.set_lobe_windows(EDGES)


def make_solver(pvlib):
    s = pvlib.Solver(SIZE, SIZE, RES, num_steps=STEPS)
    s.add_geometry(BOX)
    base_settings(s)
    return s


@pytest.fixture(scope="module")
def solver(pvlib):
    with make_solver(pvlib) as s:
        yield s


def fresh_maps(s):
    """the base settings, a new run, all nine kinds computed: name -> whole map"""
    base_settings(s)
    s.run(LISTENER)
    maps = {}
    for k in KINDS:
        assert compute(s, k) > 0
        maps[k["name"]] = whole(s, k)
        assert maps[k["name"]].shape == (s.gx, s.gy) + k["width"]
    return maps


# 1. nothing to compute before a run, nothing to read before a compute
def test_refused_before_a_run_and_before_a_compute(pvlib):
    with make_solver(pvlib) as s:
        assert s.T == STEPS
        for k in KINDS:
            with pytest.raises(pvlib.PlaneverbError, match="^%s: no completed run" % k["says"]):
                compute(s, k)
        s.run(LISTENER)
        for k in KINDS:
            refused(pvlib, s, k, "not computed")


# 2. - 4. block == slice of the map, at == the cell get_output reads, NaNs of the record's width off the map
@pytest.mark.parametrize("name", IDS)
def test_block_at_and_off_map(pvlib, solver, name):
    s, k = solver, BY_NAME[name]
    m = fresh_maps(s)[name]
    assert np.isnan(m).any() and np.isfinite(m).any()  # (the box's cells, the open floor)
    r0, c0, nr, nc = BLOCK
    assert r0 // s.info.tileRows != (r0 + nr - 1) // s.info.tileRows and c0 // s.info.tileCols != (c0 + nc - 1) // s.info.tileCols
    assert r0 + nr <= s.gx and c0 + nc <= s.gy
    b = block(s, k, r0, c0, nr, nc)
    assert b.shape == (nr, nc) + k["width"]
    assert identical(b, m[r0:r0 + nr, c0:c0 + nc])
    assert np.isnan(b).any() and np.isfinite(b).any()
    for pos in ON_MAP:
        _, rc = pvlib.host_cells(SIZE, SIZE, RES, pos[0], pos[2])
        assert rc is not None
        assert identical(at(s, k, pos), m[rc[0], rc[1]]), pos
    assert np.isnan(at(s, k, ON_MAP[1])).all() and np.isfinite(at(s, k, ON_MAP[0])).any()
    for pos in OFF_MAP:
        assert pvlib.host_cells(SIZE, SIZE, RES, pos[0], pos[2])[1] is None
        rec = at(s, k, pos)
        assert rec.shape == k["width"] and rec.dtype == np.float32 and np.isnan(rec).all()


# 5. a kind's records survive every other kind's compute and read-back
@pytest.mark.parametrize("name", IDS)
def test_other_kinds_leave_it_alone(pvlib, solver, name):
    s, k = solver, BY_NAME[name]
    base_settings(s)
    s.run(LISTENER)
    compute(s, k)
    first = whole(s, k)
    assert identical(whole(s, k), first)  # (the second read is served from the host copy)
    for other in KINDS:
        if other is not k:
            refused(pvlib, s, other, "not computed")  # (computing one kind validates no other)
    for other in KINDS:
        if other is not k:
            compute(s, other)
            whole(s, other)
            assert identical(whole(s, k), first), other["name"]
    assert identical(whole(s, k), first)
    assert identical(block(s, k, *BLOCK), first[BLOCK[0]:BLOCK[0] + BLOCK[2], BLOCK[1]:BLOCK[1] + BLOCK[3]])
    compute(s, k)  # (again, now that every other buffer exists)
    assert identical(whole(s, k), first)


# 6. what invalidates every kind
def test_geometry_boundary_and_run_invalidate_all_nine(pvlib, solver):
    s = solver
    first = fresh_maps(s)
    gid = s.add_geometry((20.0, 5.0, 2.0, 2.0, 0.5))
    try:
        for k in KINDS:
            refused(pvlib, s, k, "not computed")
        for k in KINDS:  # (the last completed run is still the first one)
            compute(s, k)
            assert identical(whole(s, k), first[k["name"]])
        s.set_grid_boundary((1, 0, 0, 0))
        for k in KINDS:
            refused(pvlib, s, k, "not computed")
        for k in KINDS:
            compute(s, k)
        s.run(LISTENER)
        for k in KINDS:
            refused(pvlib, s, k, "not computed")
        for k in KINDS:
            compute(s, k)
            assert not identical(whole(s, k), first[k["name"]])  # (another box, a rigid edge)
    finally:
        s.remove_geometry(gid)
        s.set_grid_boundary((0, 0, 0, 0))


# 7. what invalidates one kind: its own setting (the bands: band metrics and modulation)
def test_a_setting_invalidates_its_own_kind_only(pvlib, solver):
    s = solver
    maps = fresh_maps(s)
    hit = {"echogram": ["echogram"], "lobes": ["lobes"], "band_metrics": ["band_metrics", "modulation"], "modulation": ["modulation"],
           "spectrum": ["spectrum"]}
    for k in KINDS:
        if k["setter"] is None:
            continue
        k["setter"](s)
        for other in KINDS:
            if other["name"] in hit[k["name"]]:
                refused(pvlib, s, other, "not computed")
            else:
                assert identical(whole(s, other), maps[other["name"]]), (k["name"], other["name"])
        for nm in hit[k["name"]]:  # under the new setting: another width or other numbers, and valid again
            compute(s, BY_NAME[nm])
            again = whole(s, BY_NAME[nm])
            assert not identical(again, maps[nm]), nm
            maps[nm] = again
    for k in KINDS:
        assert identical(whole(s, k), maps[k["name"]])
