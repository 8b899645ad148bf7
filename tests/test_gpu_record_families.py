"""GPU (-m gpu): the contract the two families of in-run query records share (csrc/pv_solver_records.cpp: one RecordSet per family in
the solver -- the six time-domain kinds of set_query_records, the three frequency-resolved kinds of set_query_spectral_records --
and one select / grow / stamp / read routine).  What the numbers are is test_gpu_query_records.py's, test_gpu_query_spectral.py's
and test_gpu_record_queries.py's business; here it is the plumbing: the refusals word for word and in their order, and a
family's block and stamp that must not leak into the other's.  Everything is compared bit for bit, NaNs by position.  One
25 m x 25 m solver at 275 Hz, 160 steps, one box (its cells have no onset: NaN records)."""
import numpy as np
import pytest

from test_gpu_analysis_maps import BANDS, BINS, BOX, LISTENER, RES, SIZE, SLOTS, STEPS, at, base_settings, compute, identical
from test_gpu_analysis_maps import BY_NAME as MAPS

pytestmark = pytest.mark.gpu

QUERIES = [(5.0, 0.0, 6.0), (12.0, 0.0, 12.0), (-0.5, 0.0, 3.0)]  # an emitter, inside the box, off the map
NO_RUN = "no completed run since the kinds, the queries or the settings changed"


def families(pvlib):
    """per family: the api.Solver method names, the C read-back, the words of its messages, its kinds as (bit, name of the
    whole-map kind in test_gpu_analysis_maps.KINDS), a bit no kind has, and what gives one of its kinds another setting"""
    return {
        "time": dict(select="set_query_records", kinds="query_record_kinds", floats="query_record_floats", read="queried_records",
                     cread="PvAmdGetQueriedRecords", pre="query records: ", bits="PVA_QREC_*", selector="PvAmdSetQueryRecords",
                     all=pvlib.QREC_ALL, unknown=64, other="spectral",
                     bit=[(pvlib.QREC_ROOM_METRICS, "room_metrics"), (pvlib.QREC_DECAY_TIMES, "decay_times"),
                          (pvlib.QREC_LATERAL, "lateral_fraction"), (pvlib.QREC_ECHOGRAM, "echogram"),
                          (pvlib.QREC_ECHO_CRITERION, "echo_criterion"), (pvlib.QREC_LOBES, "lobes")],
                     setting=lambda s: s.set_echogram(0.02, 3)),
        "spectral": dict(select="set_query_spectral_records", kinds="query_spectral_kinds", floats="query_spectral_floats",
                         read="queried_spectral_records", cread="PvAmdGetQueriedSpectralRecords", pre="spectral records: ",
                         bits="PVA_QSPEC_*", selector="PvAmdSetQuerySpectralRecords", all=pvlib.QSPEC_ALL, unknown=8, other="time",
                         bit=[(pvlib.QSPEC_BAND_METRICS, "band_metrics"), (pvlib.QSPEC_MODULATION, "modulation"),
                              (pvlib.QSPEC_SPECTRUM, "spectrum")],
                         setting=lambda s: s.set_bands([250.0, 500.0])),
    }


FAMILIES = ["time", "spectral"]


def select(s, fam, kinds):
    getattr(s, fam["select"])(kinds)
    assert getattr(s, fam["kinds"])() == kinds


def read(s, fam, kind):
    return getattr(s, fam["read"])(kind)


def read_all(s, fam):
    return dict((k, read(s, fam, k)) for k, _ in fam["bit"] if getattr(s, fam["kinds"])() & k)


def c_read(pvlib, s, fam, kind, n):
    """the C read-back with any n: (return value, message, whether the output buffer was left alone)"""
    out = np.full(4096, 7.0, np.float32)
    rc = getattr(pvlib.lib(), fam["cread"])(s._h, kind, out.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float)), n)
    return rc, pvlib.last_error(), bool((out == 7.0).all())


def says(pvlib, text, call):
    """the call is refused with exactly this message"""
    with pytest.raises(pvlib.PlaneverbError) as e:
        call()
    assert str(e.value) == text


def refused_until_a_run(pvlib, s, fam):
    for k in read_all_kinds(s, fam):
        says(pvlib, fam["pre"] + NO_RUN, lambda: read(s, fam, k))


def read_all_kinds(s, fam):
    return [k for k, _ in fam["bit"] if getattr(s, fam["kinds"])() & k]


def same_records(a, b):
    return sorted(a) == sorted(b) and all(identical(a[k], b[k]) for k in a)


def make_solver(pvlib, **opts):
    s = pvlib.Solver(SIZE, SIZE, RES, num_steps=STEPS, **opts)
    s.add_geometry(BOX)
    return s


@pytest.fixture(scope="module")
def solver(pvlib):
    with make_solver(pvlib) as s:
        yield s


def fresh(pvlib, s):
    """the base settings, the three output queries, no record queries, all nine kinds, a new run: family name -> kind -> records"""
    fams = families(pvlib)
    base_settings(s)
    s.set_record_queries([])
    s.set_output_queries(QUERIES)
    for fam in fams.values():
        select(s, fam, fam["all"])
    s.run(LISTENER)
    return dict((name, read_all(s, fam)) for name, fam in fams.items())


# 1. every refusal word for word, and which one wins where several apply
@pytest.mark.parametrize("name", FAMILIES)
def test_exact_messages(pvlib, name):
    fam = families(pvlib)[name]
    pre, one = fam["pre"], fam["pre"] + "exactly one kind (%s)" % fam["bits"]
    first, second = fam["bit"][0][0], fam["bit"][1][0]
    unknown = pre + "unknown kind bit (%s)" % fam["bits"]
    with make_solver(pvlib) as s:
        assert s.T == STEPS
        s.set_output_queries(QUERIES)
        says(pvlib, unknown, lambda: getattr(s, fam["select"])(fam["unknown"]))
        says(pvlib, unknown, lambda: getattr(s, fam["select"])(fam["unknown"] | first))
        # a missing setting, where the kind is selected and where its size is asked for
        if name == "time":
            missing = [(pvlib.QREC_ECHOGRAM, "query records: echogram: no slots set (PvAmdSetEchogram)")]
        else:
            missing = [(pvlib.QSPEC_BAND_METRICS, "spectral records: no bands set (PvAmdSetBands)"),
                       (pvlib.QSPEC_MODULATION, "spectral records: no bands set (PvAmdSetBands)"),
                       (pvlib.QSPEC_SPECTRUM, "spectral records: no bins set (PvAmdSetSpectrumBins)")]
        for k, text in missing:
            says(pvlib, text, lambda: getattr(s, fam["select"])(k))
            says(pvlib, text, lambda: getattr(s, fam["floats"])(k))
        says(pvlib, missing[0][1], lambda: getattr(s, fam["select"])(fam["all"]))  # (the first that is missing)
        if name == "spectral":
            s.set_bands(BANDS)
            says(pvlib, missing[2][1], lambda: getattr(s, fam["select"])(fam["all"]))
        assert getattr(s, fam["kinds"])() == 0
        base_settings(s)
        # exactly one kind: a two-bit and a zero mask, at the size and at the read-back; before "not selected", before "count differs"
        for mask in (first | second, 0):
            says(pvlib, one, lambda: getattr(s, fam["floats"])(mask))
            assert c_read(pvlib, s, fam, mask, 3) == (-1, one, True)
            assert c_read(pvlib, s, fam, mask, 2) == (-1, one, True)
        not_selected = pre + "the kind is not selected (%s)" % fam["selector"]
        says(pvlib, not_selected, lambda: read(s, fam, first))
        select(s, fam, second)
        says(pvlib, not_selected, lambda: read(s, fam, first))
        assert c_read(pvlib, s, fam, first, 2) == (-1, not_selected, True)
        select(s, fam, first)
        assert c_read(pvlib, s, fam, first, 2) == (-1, pre + "count differs from the registered queries", True)
        # the stamp: nothing before the first run; a run in flight is waited for before the stamp is looked at
        says(pvlib, pre + NO_RUN, lambda: read(s, fam, first))
        assert c_read(pvlib, s, fam, first, 3) == (-1, pre + NO_RUN, True)
        s.run_async(LISTENER)
        assert read(s, fam, first).shape[0] == 3
        assert c_read(pvlib, s, fam, first, 2) == (-1, pre + "count differs from the registered queries", True)
        # a setting cannot be cleared while its kind is selected
        select(s, fam, fam["all"])
        if name == "time":
            says(pvlib, "query records: echogram: the slots cannot be cleared while PVA_QREC_ECHOGRAM is selected (PvAmdSetQueryRecords)",
                 lambda: s.set_echogram(0.01, 0))
            assert s.echogram_slots()[0] == SLOTS[1]
        else:
            says(pvlib, "spectral records: the bands cannot be cleared while a band kind is selected (PvAmdSetQuerySpectralRecords)",
                 lambda: s.set_bands([]))
            says(pvlib, "spectral records: the bins cannot be cleared while PVA_QSPEC_SPECTRUM is selected (PvAmdSetQuerySpectralRecords)",
                 lambda: s.set_spectrum_bins([]))
            assert len(s.bands()[0]) == len(BANDS) and len(s.spectrum_bins()) == len(BINS)
        # the C level's own argument checks
        for n in (-1, 1025):
            assert c_read(pvlib, s, fam, first, n) == (-1, pre + fam["cread"] + ": 0 .. 1024 queries and an output buffer", True)
            xyz = np.zeros(3, np.float32)
            assert pvlib.lib().PvAmdSetRecordQueries(s._h, xyz.ctypes.data_as(pvlib.C.POINTER(pvlib.C.c_float)), n) == -1
            assert pvlib.last_error() == "query records: PvAmdSetRecordQueries: 0 .. 1024 positions (NULL only with 0)"
    # the modes without a pressure history or an onset map: behind the unknown bit, in front of the missing setting
    for opt, text in (("streaming_analysis", "the full pressure history is not kept in streaming-analysis mode"),
                      ("skip_analysis", "the run has no onset map (PVA_OPT_SKIP_ANALYSIS)")):
        with make_solver(pvlib, **{opt: 1}) as s:
            says(pvlib, unknown, lambda: getattr(s, fam["select"])(fam["unknown"] | first))
            for k, _ in fam["bit"]:
                says(pvlib, pre + text, lambda: getattr(s, fam["select"])(k))
            getattr(s, fam["select"])(0)
            assert getattr(s, fam["kinds"])() == 0


# 2. a family's selector, setting and stamp leave the other family's records alone
@pytest.mark.parametrize("name", FAMILIES)
def test_isolation(pvlib, solver, name):
    s, fams = solver, families(pvlib)
    a, b = fams[name], fams[fams[name]["other"]]
    first = a["bit"][0][0]
    actions = {"deselect and reselect": lambda: (select(s, a, 0), select(s, a, a["all"])),
               "another setting": lambda: a["setting"](s),
               "a subset": lambda: select(s, a, a["all"] & ~first)}
    for what, act in actions.items():
        before = fresh(pvlib, s)
        assert len(before["time"]) == 6 and len(before["spectral"]) == 3
        for recs in before.values():
            for r in recs.values():
                assert r.shape[0] == 3 and np.isfinite(r[0]).any() and np.isnan(r[1]).all() and np.isnan(r[2]).all()
        act()
        assert same_records(read_all(s, b), before[a["other"]]), what
        refused_until_a_run(pvlib, s, a)
        assert same_records(read_all(s, b), before[a["other"]]), what
        s.run(LISTENER)
        assert same_records(read_all(s, b), before[a["other"]]), what
        got = read_all(s, a)
        if what == "a subset":
            assert sorted(got) == sorted(k for k, _ in a["bit"][1:])
            assert all(identical(got[k], before[name][k]) for k in got)
        elif what == "another setting":
            assert not same_records(got, before[name])


# 3. the record queries: both blocks grow, both stamps follow the table the records follow
def test_query_tables_and_the_stamp(pvlib, solver):
    s, fams = solver, families(pvlib)
    fresh(pvlib, s)  # (the kinds were selected under three output queries: blocks of 64 queries)
    rng = np.random.default_rng(65)
    pos = [(float(x), 0.0, float(z)) for x, z in rng.uniform(0.2, SIZE - 0.2, (61, 2))] + QUERIES + [QUERIES[0]]
    assert len(pos) == 65

    def check_rows(positions):
        for fam in fams.values():
            for k, kind in fam["bit"]:
                got = read(s, fam, k)
                assert got.shape[0] == len(positions)
                compute(s, MAPS[kind])
                for i, p in enumerate(positions):
                    assert identical(got[i], at(s, MAPS[kind], p)), (kind, i)

    for n in (65, 64, 1):  # two waves with one query in the second, one full wave, one query
        s.set_record_queries(pos[:n])
        for fam in fams.values():
            refused_until_a_run(pvlib, s, fam)
        s.run(LISTENER)
        check_rows(pos[:n])
        if n == 65:  # (the same cell in both waves)
            rows = s.queried_records(pvlib.QREC_ROOM_METRICS)
            assert identical(rows[64], rows[61]) and np.isfinite(rows[64]).any()
    # other output queries while there are record queries: neither family's records go
    before = dict((name, read_all(s, fam)) for name, fam in fams.items())
    s.set_output_queries(QUERIES[:2])
    for name, fam in fams.items():
        assert same_records(read_all(s, fam), before[name]), name
    # no record queries: back to the output queries' count, and both stamps go
    s.set_record_queries([])
    for fam in fams.values():
        refused_until_a_run(pvlib, s, fam)
    s.run(LISTENER)
    check_rows(QUERIES[:2])


# 4. the block's lifetime
@pytest.mark.parametrize("name", FAMILIES)
def test_lifetime(pvlib, solver, name):
    s, fam = solver, families(pvlib)[name]
    before = fresh(pvlib, s)[name]
    # freed and allocated again
    select(s, fam, 0)
    s.run(LISTENER)
    for k, _ in fam["bit"]:
        says(pvlib, fam["pre"] + "the kind is not selected (%s)" % fam["selector"], lambda: read(s, fam, k))
    select(s, fam, fam["all"])
    refused_until_a_run(pvlib, s, fam)
    s.run(LISTENER)
    assert same_records(read_all(s, fam), before)
    # the same mask again between a completed run and the read-back: nothing happens
    select(s, fam, fam["all"])
    assert same_records(read_all(s, fam), before)
    s.run_async(LISTENER)
    select(s, fam, fam["all"])  # (waits for the run)
    assert same_records(read_all(s, fam), before)
