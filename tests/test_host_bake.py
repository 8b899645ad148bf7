"""CPU: baked probe tables (include/planeverb_amd.h Part 4) against the numpy restatement of INTEGRATION.md (tests/_bake_ref.py).

Bakes written by the numpy writer are loaded by the library; PvAmdBakeQuery must equal the restatement bit for bit on random
listener / emitter pairs (outside the lattice and the grid too), Save(Load(f)) must reproduce f byte for byte, and damaged files
must be refused.  No GPU: the bakes come from the writer, not from runs."""
import struct

import numpy as np
import pytest

from _bake_ref import ENTRY, HEADER, RefBake, fnv1a64, random_bake, random_pairs
from conftest import same_bits

CASES = [
    dict(),                                        # stride 3, every state, empty blocks, unreached nodes, rt60 finite / NaN / +inf
    dict(stride=1, gx=23, gy=31),
    dict(nx=1, nz=5),
    dict(nx=6, nz=1, stride=2),
    dict(nx=1, nz=1, stride=4, p_state=(0.0, 1.0, 0.0), p_empty=0.0),
    dict(p_state=(0.0, 1.0, 0.0), p_empty=0.0, p_reached=0.95, stride=5, gx=64, gy=48, nx=5, nz=4),
    dict(p_reached=0.3, sx=0.125, sz=0.375),
]


@pytest.fixture(scope="module")
def api(pvlib):
    return pvlib


@pytest.mark.parametrize("case", range(len(CASES)))
def test_query_matches_restatement(api, tmp_path, case):
    rng = np.random.default_rng(1000 + case)
    ref = random_bake(rng, **CASES[case])
    path = str(tmp_path / "b.pvbake")
    ref.write(path)
    b = api.Bake.load(path)
    info = b.info()
    baked, invalid, records = ref.counts()
    assert (info["probesBaked"], info["probesInvalid"], info["records"]) == (baked, invalid, records)
    assert info["materialHash"] == ref.h["materialHash"] and info["stride"] == ref.h["stride"]
    for k, p in enumerate(ref.probes):
        st, rec = b.probe(k)
        assert list(st) == list(p[:5]), k
        assert rec.tobytes() == np.ascontiguousarray(p[5], np.float32).tobytes(), k
    n = 100_000 if case == 0 else 25_000
    L, E = random_pairs(rng, ref.h, n)
    got = b.query(L, E)
    want = ref.query(L, E)
    bad = ~same_bits(got, want).all(axis=1)
    assert not bad.any(), "%d of %d queries differ; first %d: %r vs %r (L %r E %r)" % (
        bad.sum(), n, np.argmax(bad), got[bad][0], want[bad][0], L[bad][0], E[bad][0])
    # the cases are not vacuous: sentinels, single records and blends all occur
    used = want[:, 0] != -1
    assert used.any() and (~used).any()
    b.close()


def test_query_single_contribution_and_blend_rules(api, tmp_path):
    """hand-made bake: 2 x 1 probes, stride 1, one reached node each -> a probe position returns the record unchanged, half way
    between the probes blends (rt60: finite mean over finite ones; +inf only when no finite one)"""
    f32 = np.float32
    hdr = dict(gx=4, gy=4, T=435, fs=1443, res=275, dx=f32(0.5), stride=1, x0=f32(0.25), z0=f32(0.25), sx=f32(1.0), sz=f32(1.0),
               nx=2, nz=1, materialHash=7)
    r0 = np.array([[[0.5, 0.2, 1.0, 0.9, 1.0, 0.0, 0.0, 1.0, 10.0]]], f32)
    r1 = np.array([[[0.3, 0.4, np.inf, 0.7, 0.0, 1.0, 1.0, 0.0, 12.0]]], f32)
    ref = RefBake(hdr, [(1, 1, 1, 1, 1, r0), (1, 1, 1, 1, 1, r1)])
    path = str(tmp_path / "h.pvbake")
    ref.write(path)
    b = api.Bake.load(path)
    E = np.array([[0.75, 0, 0.75]] * 3, f32)
    L = np.array([[0.25, 0, 0.25], [1.25, 0, 0.25], [0.75, 0, 0.25]], f32)
    got = b.query(L, E)
    assert same_bits(got[0], r0[0, 0, :8]).all() and same_bits(got[1], r1[0, 0, :8]).all()
    assert got[2][0] == f32(0.4) and got[2][2] == f32(1.0)  # occlusion mean; rt60 = the finite one
    s = np.float32(np.sqrt(f32(0.5)))
    assert same_bits(got[2][4:6], [f32(0.5) / s, f32(0.5) / s]).all()
    assert same_bits(got, ref.query(L, E)).all()
    # an emitter outside the grid: the sentinel
    out = b.query([[0.25, 0, 0.25]], [[-1.0, 0, 0.75]])
    assert list(out[0]) == [-1, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("case", [0, 2, 5])
def test_save_load_roundtrip_is_byte_identical(api, tmp_path, case):
    ref = random_bake(np.random.default_rng(2000 + case), **CASES[case])
    p1, p2 = str(tmp_path / "a.pvbake"), str(tmp_path / "b.pvbake")
    ref.write(p1)
    api.Bake.load(p1).save(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()


def _refused(api, path, what):
    with pytest.raises(api.PlaneverbError) as e:
        api.Bake.load(path)
    assert what in str(e.value), str(e.value)


def _reseal(body):
    return body + struct.pack("<Q", fnv1a64(body))


def test_damaged_files_are_refused(api, tmp_path):
    ref = random_bake(np.random.default_rng(3), p_state=(0.0, 1.0, 0.0), p_empty=0.0)
    good = ref.to_bytes()
    p = str(tmp_path / "x.pvbake")

    def put(data):
        with open(p, "wb") as f:
            f.write(data)

    put(good)
    api.Bake.load(p).close()
    for cut in (len(good) - 1, len(good) // 2, HEADER.size + 3, 10):  # truncated
        put(good[:cut])
        with pytest.raises(api.PlaneverbError):
            api.Bake.load(p)
    for pos in (HEADER.size + 5, len(good) - 20, 40):  # one flipped byte: the checksum
        bad = bytearray(good)
        bad[pos] ^= 0x10
        put(bytes(bad))
        _refused(api, p, "checksum")
    put(b"PVBAKX\x00\x01" + good[8:])
    _refused(api, p, "magic")
    put(_reseal(good[:8] + struct.pack("<I", 2) + good[12:-8]))
    _refused(api, p, "version")
    # a block that leaves the lattice (checksum made right): probe 0's i0 moved past the last lattice row
    st, i0, j0, ni, nj, off = ENTRY.unpack_from(good, HEADER.size)
    li = -(-ref.h["gx"] // ref.h["stride"])
    body = bytearray(good[:-8])
    ENTRY.pack_into(body, HEADER.size, st, li - ni + 1, j0, ni, nj, off)
    put(_reseal(bytes(body)))
    _refused(api, p, "lattice")
    # a record offset that points elsewhere
    body = bytearray(good[:-8])
    ENTRY.pack_into(body, HEADER.size, st, i0, j0, ni, nj, off + 36)
    put(_reseal(bytes(body)))
    _refused(api, p, "offset")
    # a header record count that disagrees with the table
    body = bytearray(good[:-8])
    struct.pack_into("<q", body, 72, struct.unpack_from("<q", body, 72)[0] - 1)
    put(_reseal(bytes(body)))
    _refused(api, p, "inconsistent sizes")
    with pytest.raises(api.PlaneverbError):
        api.Bake.load(str(tmp_path / "missing"))


def test_merge_of_loaded_bakes(api, tmp_path):
    rng = np.random.default_rng(11)
    full = random_bake(rng, p_state=(0.0, 0.8, 0.2))
    half = [RefBake(full.h, [p if k % 2 == r else (0, 0, 0, 0, 0, np.zeros((0, 0, 9), np.float32))
                             for k, p in enumerate(full.probes)]) for r in range(2)]
    paths = []
    for i, rb in enumerate([full] + half):
        paths.append(str(tmp_path / ("m%d.pvbake" % i)))
        rb.write(paths[-1])
    a, b = api.Bake.load(paths[1]), api.Bake.load(paths[2])
    a.merge(b)
    a.merge(b)  # the same contents twice: accepted
    out = str(tmp_path / "merged.pvbake")
    a.save(out)
    assert open(out, "rb").read() == open(paths[0], "rb").read()
    # a probe held by both with different contents
    k = next(k for k, p in enumerate(full.probes) if p[0] == 1 and p[3] > 0)
    probes = list(full.probes)
    rec = probes[k][5].copy()
    rec[0, 0, 0] += np.float32(0.5)
    probes[k] = probes[k][:5] + (rec,)
    RefBake(full.h, probes).write(paths[1])
    with pytest.raises(api.PlaneverbError, match="different contents"):
        api.Bake.load(paths[0]).merge(api.Bake.load(paths[1]))
    # another lattice
    h2 = dict(full.h, sx=np.float32(2.0))
    RefBake(h2, full.probes).write(paths[1])
    with pytest.raises(api.PlaneverbError, match="lattice"):
        api.Bake.load(paths[0]).merge(api.Bake.load(paths[1]))
