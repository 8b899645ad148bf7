"""CPU: the C-ABI library loads, exports every symbol include/planeverb_amd.h declares, keeps the reference's
sentinels without a module, refuses to run without a HIP device, and its host-side arithmetic (grid parameters,
pulse table, rasteriser, .pv parser, cell lookups) matches the golden vectors from the reference.  No device
compute is called here."""
import os
import re
import subprocess
import ctypes as C

import numpy as np
import pytest

from conftest import ROOT, SCENES, golden, same_bits

SMALL = ["g71_smallroom", "g71_shoebox", "g71_bigroom", "g71_hugeroom", "g71_floorplan", "g71_direction",
         "g71_empty", "g96_smallroom_res375"]


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    return sorted(set(re.findall(r"^PVA_EXPORT\s+[\w\s\*]*?\b(\w+)\s*\(", src, re.MULTILINE)))


def test_library_exports_every_declared_symbol(pvlib):
    names = declared_symbols()
    assert len(names) >= 45
    L = C.CDLL(pvlib.LIB_PATH)
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    # and the python binding covers the same set
    assert sorted(pvlib.SYMBOLS) == names


def test_python_option_keys_match_the_header(pvlib):
    """every PVA_OPT_* of include/planeverb_amd.h has the same value in planeverb_amd/api.py (the ctypes mirror passes the numbers),
    and no two options share one"""
    src = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    header = dict((k, int(v)) for k, v in re.findall(r"\b(PVA_OPT_\w+)\s*=\s*(\d+)", src))
    assert len(header) >= 27 and len(set(header.values())) == len(header)
    for k, v in header.items():
        assert getattr(pvlib, k) == v, k
    mirrored = [k for k in dir(pvlib) if k.startswith("PVA_OPT_")]
    assert sorted(mirrored) == sorted(header), set(mirrored) ^ set(header)


def test_reference_abi_names_present(pvlib):
    """the 11 functions + 2 Unity hooks of PlaneverbUnity.cpp:12-135"""
    for n in ["PlaneverbInit", "PlaneverbExit", "PlaneverbEmit", "PlaneverbUpdateEmission", "PlaneverbEndEmission",
              "PlaneverbGetOutput", "PlaneverbAddGeometry", "PlaneverbUpdateGeometry", "PlaneverbRemoveGeometry",
              "PlaneverbSetListenerPosition", "UnityPluginLoad", "UnityPluginUnload", "PlaneverbCreateGrid"]:
        assert n in pvlib.SYMBOLS
    assert C.sizeof(pvlib.PlaneverbOutput) == 32


def test_sentinels_without_module(pvlib):
    """null-context behaviour: EmissionManager.cpp:13, GeometryManager.cpp:20, FDTD.cpp:22-26"""
    pvlib.Exit()
    assert pvlib.Emit((1, 2, 3)) == -1
    assert pvlib.AddGeometry((1, 1, 1, 1, 0.5)) == -1
    o = pvlib.GetOutput(0)
    assert o.occlusion == -1.0 and o.wetGain == 0 and o.rt60 == 0 and o.lowpass == 0
    pvlib.UpdateEmission(0, (1, 2, 3))
    pvlib.EndEmission(0)
    pvlib.UpdateGeometry(0, (1, 1, 1, 1, 0.5))
    pvlib.RemoveGeometry(0)
    pvlib.SetListenerPosition((1, 2, 3))
    assert pvlib.IterationCount() == 0


def test_invalid_config_is_rejected_not_thrown(pvlib):
    """PvContext.cpp:101-107 throws pv_InvalidConfig; across a C-ABI that becomes 'module stays down'"""
    for cfg in [pvlib.Config((25, 25), 200, 0, ".", 0, 1), pvlib.Config((0, 25), 275, 0, ".", 0, 1),
                pvlib.Config((25, 25), 275, 0, None, 0, 1)]:
        with pytest.raises(pvlib.PlaneverbError):
            pvlib.Init(cfg)
        assert pvlib.lib().PlaneverbIsRunning() == 0
    assert pvlib.lib().PvAmdCreate(25.0, 25.0, 100, 0) is None


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_no_device_fails_loudly(pvlib):
    assert pvlib.device_count() == 0
    with pytest.raises(pvlib.PlaneverbError, match="no HIP device"):
        pvlib.Solver(25.0, 25.0, 275)
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.Init(pvlib.Config((25, 25), 275, 0, ".", 0, 1))


@pytest.mark.parametrize("name", SMALL)
def test_host_arithmetic_matches_reference(pvlib, name):
    g = golden(name)
    size, res = float(g["size"]), int(g["res"])
    i = pvlib.host_grid_info(size, size, res)
    assert [i.gx, i.gy, i.T, i.fs] == [int(v) for v in g["dims"]]
    assert np.float32(i.dx) == g["dx"] and np.float32(i.dt) == g["dt"]
    assert same_bits(pvlib.host_pulse(size, size, res), g["pulse"]).all()
    beta, R = pvlib.host_rasterize(size, size, res, g["boxes"])
    assert np.array_equal(beta, g["beta"]) and same_bits(R, g["R"]).all()


def test_rasteriser_add_remove_sequence(pvlib, oracle):
    a = [10, 10, 6, 1, 0.9]
    b = [12, 10, 1, 6, 0.8]
    edge = [24.9, 12, 1, 30, 0.7]
    seq = [(1, a), (1, b), (-1, a), (1, edge), (-1, edge), (1, a)]
    o = oracle.OracleGrid(25.0, 25.0, 275, None, with_history=False)
    for n in range(1, len(seq) + 1):
        ops = [s[0] for s in seq[:n]]
        boxes = [s[1] for s in seq[:n]]
        (o.add_aabb if ops[-1] > 0 else o.remove_aabb)(np.array(boxes[-1], np.float32))
        beta, R = pvlib.host_rasterize(25.0, 25.0, 275, boxes, ops)
        ob, oR = o.material()
        assert np.array_equal(beta, ob.astype(np.uint8)) and same_bits(R, oR).all()
    o.close()


def test_pv_loader_matches(pvlib):
    from oracle import pvref
    for f in sorted(os.listdir(SCENES)):
        p = os.path.join(SCENES, f)
        assert np.array_equal(pvlib.load_pv(p), pvref.load_pv(p))
    with pytest.raises(pvlib.PlaneverbError):
        pvlib.load_pv(os.path.join(SCENES, "does_not_exist.pv"))


def test_cell_lookups(pvlib, oracle):
    o = oracle.OracleGrid(25.0, 25.0, 275, None, with_history=False)
    rng = np.random.default_rng(5)
    for x, z in rng.uniform(0, 25.2, (200, 2)):
        lc, rc = pvlib.host_cells(25.0, 25.0, 275, x, z)
        assert lc == o.listener_cell(np.float32(x), np.float32(z))
        idx = o.result_index((x, 0, z))
        if rc is None:  # the reference's `>` test admits row/col == gx; the product rejects it
            assert idx < 0 or lc[0] >= o.gx or lc[1] >= o.gy
        else:
            assert idx == rc[0] * o.gx + rc[1]
    o.close()


def test_reverb_bus_gains_match_oracle(pvlib, oracle):
    for rt in [0.2, 0.5, 0.51, 0.79, 1.0, 1.07, 1.76, 2.99, 3.0, 3.5]:
        for w in [0.0, 0.49, 1.73]:
            assert same_bits(np.array(pvlib.reverb_bus_gains(rt, w), np.float32),
                             np.array(oracle.find_gains(rt, w), np.float32)).all()


def test_reverb_bus_gains_match_compiled_reference(pvlib):
    """SURVEY.md 8a row 24 pinned for the PRODUCT: PvAmdReverbBusGains against the table generated from the reference's
    own compiled FindGainA/B/C (PlaneverbDSP/src/PvDSPContext.cpp:165-228; tests/golden/make_golden.py findgain)"""
    g = golden("g_findgain")
    for (rt, w), want in zip(g["inputs"], g["gains"]):
        assert same_bits(np.array(pvlib.reverb_bus_gains(rt, w), np.float32), want).all(), (rt, w)


def test_pv_save_load_round_trip(pvlib, tmp_path):
    """Editor::SaveGeometry / LoadGeometry (Editor.cpp:219-281): what is written is read back unchanged"""
    for f in sorted(os.listdir(SCENES)):
        boxes = pvlib.load_pv(os.path.join(SCENES, f))
        out = str(tmp_path / f)
        pvlib.save_pv(out, boxes, ids=list(range(len(boxes) - 1, -1, -1)))
        assert np.array_equal(pvlib.load_pv(out), boxes)
        first = open(out).read().split()
        assert int(first[0]) == len(boxes) and int(first[1]) == len(boxes) - 1  # count, then the first id


def test_pv_save_keeps_every_float_bit(pvlib, tmp_path):
    """values that are not short decimals survive Save -> Load bit for bit (max_digits10), so the rasterised walls of
    a round-tripped scene cannot move across a cell boundary"""
    rng = np.random.default_rng(5)
    boxes = (rng.random((64, 5)) * np.array([25, 25, 6, 6, 1])).astype(np.float32)
    boxes[0] = [np.float32(1) / np.float32(3), np.nextafter(np.float32(7.1317368), np.float32(8)), 1e-3, 2.0000002, 0.969536]
    out = str(tmp_path / "odd.pv")
    pvlib.save_pv(out, boxes)
    back = pvlib.load_pv(out)
    assert np.array_equal(back.view(np.uint32), boxes.view(np.uint32))
    b0, R0 = pvlib.host_rasterize(25.0, 25.0, 275, boxes)
    b1, R1 = pvlib.host_rasterize(25.0, 25.0, 275, back)
    assert np.array_equal(b0, b1) and np.array_equal(R0.view(np.uint32), R1.view(np.uint32))


def test_cli_save_without_gpu(pvlib, tmp_path):
    import subprocess
    import sys
    out = str(tmp_path / "copy.pv")
    r = subprocess.run([sys.executable, "-m", "planeverb_amd", os.path.join(SCENES, "Shoebox.pv"), "--save", out],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(pvlib.load_pv(out), pvlib.load_pv(os.path.join(SCENES, "Shoebox.pv")))


def test_device_libm_matches_host_libm(tmp_path):
    """pv_libm.h (the log10f / powf the analysis kernels use, compiled here for the host) against this machine's
    libm on a 1-in-97 sample of all floats + special values; tools/libm_check.cpp 1 runs all of them"""
    import json
    import subprocess
    exe = str(tmp_path / "libm_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(ROOT, "planeverb_amd", "csrc"),
                           os.path.join(ROOT, "tools", "libm_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "97"], capture_output=True, text=True)
    out = json.loads(r.stdout)
    assert r.returncode == 0 and out["log10f_mismatches"] == 0 and out["powf_mismatches"] == 0 and out["values"] > 2e7


@pytest.mark.parametrize("src,extra", [("pv_kernels.hip", []), ("pv_kernels.hip", ["-DPV_EXPERIMENTAL"]), ("pv_resident.hip", [])])
def test_inline_asm_dpp_has_no_pipeline_hazard(tmp_path, src, extra):
    """the packed tile kernels subtract a lane-shifted operand with an inline-asm v_subrev_f32_dpp; gfx9-family ISAs need 2
    wait states between a VALU write of a VGPR and a DPP read of it and the compiler cannot see into inline asm -- scan the
    generated gfx950 assembly of every instantiation (tools/check_dpp_hazard.py): the product library's kernels, the
    experimental build's, and the resident kernel"""
    import shutil
    import subprocess
    import sys
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = str(tmp_path / "k.s")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
                           "-std=c++17", "-S", "--cuda-device-only", "-w"] + extra +
                          [os.path.join(ROOT, "planeverb_amd", "csrc", src), "-o", asm])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_dpp_hazard.py"), asm],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


def test_dpp_hazard_lint_follows_branches(tmp_path):
    """the lint walks every path into a DPP read: a writer that reaches it through a branch is found, a fall-through path that has
    its wait states is not flagged, and a kernel with no such instruction fails (nothing was checked)"""
    import subprocess
    import sys
    lint = os.path.join(ROOT, "tools", "check_dpp_hazard.py")
    bad = tmp_path / "bad.s"
    bad.write_text("k:\n\tv_mov_b32_e32 v2, v1\n\ts_cbranch_scc1 .LBB0_2\n\ts_nop 4\n.LBB0_2:\n"
                   "\tv_subrev_f32_dpp v5, v2, v2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_endpgm\n")
    good = tmp_path / "good.s"
    good.write_text("k:\n\tv_mov_b32_e32 v2, v1\n\ts_nop 0\n\ts_cbranch_scc1 .LBB0_2\n\ts_nop 4\n.LBB0_2:\n"
                    "\tv_subrev_f32_dpp v5, v2, v2 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_endpgm\n")
    none = tmp_path / "none.s"
    none.write_text("k:\n\tv_mov_b32_e32 v2, v1\n\ts_endpgm\n")
    assert subprocess.run([sys.executable, lint, str(bad)], capture_output=True).returncode == 1
    assert subprocess.run([sys.executable, lint, str(good)], capture_output=True).returncode == 0
    assert subprocess.run([sys.executable, lint, str(none)], capture_output=True).returncode == 1


def test_cpp_binding_links_against_reference_headers():
    """bindings/PlaneverbAmdBinding.cpp -- the forwarding unit INTEGRATION.md section 2 gives a maintainer: the
    reference's namespace API (Planeverb.h:12-47, all 12 functions) on top of this library's C-ABI.  Where the reference
    is present (the build container) a caller written against the reference's OWN header (tests/host/sandbox_probe.cpp)
    must COMPILE AND LINK with it + -lplaneverb_amd (run on the GPU: tests/test_gpu_live.py); and the text in
    INTEGRATION.md must be that file."""
    src = os.path.join(ROOT, "bindings", "PlaneverbAmdBinding.cpp")
    code = open(src).read()
    assert code in open(os.path.join(ROOT, "INTEGRATION.md")).read(), "INTEGRATION.md section 2 is out of date"
    if not os.path.isdir("/root/reference/ProjectPlaneverb/include"):
        pytest.skip("reference headers not present on this machine")
    import planeverb_amd
    planeverb_amd.build()
    exe = os.path.join(ROOT, "oracle", "_ref", "sandbox_probe")
    if os.path.exists(exe):
        os.remove(exe)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "_ref/sandbox_probe"], stdout=subprocess.DEVNULL)
    undefined = subprocess.run(["nm", "-u", "-C", exe], capture_output=True, text=True, check=True).stdout
    assert "Planeverb::" not in undefined, undefined  # every namespace function the probe calls came from the binding
    defined = subprocess.run(["nm", "-C", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    for fn in ["Init", "Exit", "ChangeSettings", "Emit", "UpdateEmission", "EndEmission", "GetOutput", "AddGeometry",
               "UpdateGeometry", "RemoveGeometry", "SetListenerPosition", "GetImpulseResponse"]:
        assert re.search(r"\bPlaneverb::%s\(" % fn, defined), fn


def test_shard_plan_matches_the_python_layer(pvlib):
    """PvAmdShardPlan (the C++ side's run -> rank -> solver map) on a fake device list: every run exactly
    once over the ranks, rank r holds runs r, r + W, ... (what planeverb_amd.dist.shard_runs says), round-robin over the
    rank's solvers"""
    from planeverb_amd import dist as pvd
    for n_runs in (0, 1, 7, 8, 64, 65):
        for world in (1, 2, 3, 8):
            seen = []
            for rank in range(world):
                for n_local in (1, 2, 4):
                    plan = pvlib.shard_plan(n_runs, world, rank, n_local)
                    assert [k for k, _ in plan] == pvd.shard_runs(n_runs, world, rank)
                    assert [s for _, s in plan] == [j % n_local for j in range(len(plan))]
                seen += [k for k, _ in pvlib.shard_plan(n_runs, world, rank, 1)]
            assert sorted(seen) == list(range(n_runs))
    assert pvlib.shard_plan(5, 2, 2, 1) == [] and pvlib.shard_plan(5, 0, 0, 1) == []


def test_segment_plan_covers_every_air_tile_once(pvlib):
    """PvAmdPlanSegments (the host plan of the row-streaming air segments, PVA_OPT_STREAM_ROWS): on random tile maps every
    air tile row is covered by exactly one segment, no segment touches a non-air tile, widths and heights stay inside what
    the kernel's bookkeeping can hold, the list is sorted, and the target steers the segment count"""
    rng = np.random.default_rng(5)
    for trial in range(60):
        ntx, nty = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        rows, wmax = int(rng.choice([24, 36, 40])), int(rng.choice([2, 5]))
        air = (rng.random((ntx, nty)) < rng.choice([0.3, 0.8, 0.97, 1.0])).astype(np.uint8)
        target = int(rng.choice([1, 7, 64, 1024]))
        seg = pvlib.plan_segments(air, rows, wmax, target)
        cover = np.zeros((ntx * rows, nty), np.int32)
        for r0, n, tj0, w in seg:
            assert 1 <= w <= wmax and 1 <= n <= 7 * rows and r0 >= 0 and r0 + n <= ntx * rows and tj0 + w <= nty
            assert (r0 % rows + n + rows - 1) // rows <= 8  # tile rows a segment touches
            cover[r0:r0 + n, tj0:tj0 + w] += 1
        want = np.repeat(air.astype(np.int32), rows, axis=0)
        assert np.array_equal(cover, want), trial
        keys = [(int(a), int(c)) for a, _, c, _ in seg]
        assert keys == sorted(keys)
    # an open 114 x 103 tile grid (4096^2 at 36 x 40 tiles) with its border tiles general, 1024 segments wanted
    air = np.ones((114, 103), np.uint8)
    air[0, :] = air[-1, :] = 0
    air[:, 0] = air[:, -1] = 0
    seg = pvlib.plan_segments(air, 36, 5, 1024)
    assert 900 <= len(seg) <= 1300 and seg[:, 3].max() == 5 and (seg[:, 1] <= 7 * 36).all()
    assert len(pvlib.plan_segments(air, 36, 5, 64)) < len(seg) < len(pvlib.plan_segments(air, 36, 5, 4096))
    assert len(pvlib.plan_segments(np.zeros((3, 3), np.uint8), 36, 5, 10)) == 0


def test_batch_policy_helpers():
    """pure host logic: which grids are run in batches, and with which tile"""
    from planeverb_amd import api, dist
    assert dist.default_batch(512, 512) == 8 and dist.default_batch(1024, 1024) == 8
    assert dist.default_batch(2048, 2048) == 1 and dist.default_batch(4096, 4096) == 1
    assert dist.default_inflight(4096, 4096) == 2 and dist.default_inflight(512, 512) == 4
    for n, (k, rows) in ((256, (8, 40)), (512, (8, 40)), (1024, (10, 36)), (2048, (12, 36))):
        o = api.batch_solver_options(n)
        assert (o["steps_per_launch"], o["tile_rows"], o["edge_tiles"]) == (k, rows, 1)


@pytest.mark.parametrize("pipeline", ["1", "2"])
@pytest.mark.parametrize("san", ["tsan", "asan"])
def test_live_module_host_side_under_sanitizers(san, pipeline, tmp_path):
    """SURVEY.md section 5 ("run host code under TSan/ASan"): a HIP-less build of pv_core.cpp + pv_context.cpp +
    pv_capi.cpp (Part 1) against tests/host/fake_solver.h, hammered through the C-ABI by 4 threads (GetOutput /
    Emit / UpdateEmission / EndEmission / Add-Update-RemoveGeometry / SetListenerPosition / GetImpulseResponse) while
    the main thread cycles Exit / Init, then a worker failure.  ThreadSanitizer resp. AddressSanitizer + UBSan must stay
    silent and every record read must come from one iteration and belong to the cell asked for.
    pipeline = 2: the worker loop that keeps two iterations in flight on two solvers (three result slots)."""
    out = str(tmp_path / "build")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "host"), "OUT=" + out, out + "/hammer_" + san],
                          stdout=subprocess.DEVNULL)
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", ASAN_OPTIONS="detect_leaks=1 exitcode=67",
               PLANEVERB_AMD_LIVE_PIPELINE=pipeline)
    r = subprocess.run([out + "/hammer_" + san, "1.5"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert " 0 bad, phase3 flags 0" in r.stdout, r.stdout


@pytest.mark.parametrize("pipeline", ["1", "2"])
def test_no_exception_crosses_the_c_abi(pipeline, tmp_path):
    """SURVEY.md 5 / 8b ("a C-ABI must not leak C++ exceptions -- catch at the boundary"; the reference throws from Init,
    PvContext.cpp:106,123, Grid.cpp:69).  (i) EVERY extern "C" definition of pv_capi.cpp is a function-try-block closed by one
    of the PV_API_CATCH macros; (ii) tests/host/alloc_fault.cpp replaces operator new in the HIP-less build of the live module
    and fails every allocation of every Part 1 call, one at a time (and one on the worker thread, and an exception thrown by
    the solver inside an iteration): each call returns its sentinel, PvAmdLastError names the function, the id tables are
    unchanged, the per-frame calls allocate nothing, the worker stops instead of terminating the host.  Under ASan + UBSan."""
    import re
    src = open(os.path.join(ROOT, "planeverb_amd", "csrc", "pv_capi.cpp")).read()
    body = src[src.index('extern "C" {'):src.index('}  // extern "C"')]
    defs = re.findall(r"^(?!static|struct|//|#|\}|typedef)[A-Za-z][^;{}()]*?\b(\w+)\s*\([^;{}]*?\)\s*(try)?\s*\{", body, re.M)
    names = [n for n, _ in defs]
    assert len(names) >= 92, len(names)
    assert {"PvAmdSetHistoryPlane", "PvAmdLibmProbe"} <= set(names)  # (the two test seams are exports like any other)
    unguarded = [n for n, t in defs if not t]
    assert not unguarded, unguarded
    assert body.count("PV_API_CATCH") == len(names), (body.count("PV_API_CATCH"), len(names))
    # every symbol the header declares is one of them
    hdr = open(os.path.join(ROOT, "include", "planeverb_amd.h")).read()
    declared = set(re.findall(r"\b((?:Planeverb|PvAmd|UnityPlugin)\w+)\s*\(", hdr))
    assert declared <= set(names), sorted(declared - set(names))
    out = str(tmp_path / "build")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "host"), "OUT=" + out, out + "/alloc_fault_asan"],
                          stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1 exitcode=67", PLANEVERB_AMD_LIVE_PIPELINE=pipeline,
               PV_TEST_SCENE=os.path.join(ROOT, "tests", "scenes", "SmallRoomScene.pv"))
    r = subprocess.run([out + "/alloc_fault_asan"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "Sanitizer" not in r.stderr, r.stderr[-4000:]
    assert "alloc_fault: 0 failure(s)" in r.stdout, r.stdout
    assert "injected exception" not in r.stdout  # (only ever in PlaneverbWorkerError, checked inside)


def test_header_is_plain_c(tmp_path):
    """include/planeverb_amd.h is a C header (the drop-in boundary: extern "C", plain pointers and sizes): it must compile
    as C99 on its own, and PlaneverbOutput / PlaneverbCell must have the reference's sizes (8 floats; 16 bytes)"""
    src = tmp_path / "abi.c"
    src.write_text('#include "planeverb_amd.h"\n'
                   'typedef char out_is_32_bytes[sizeof(PlaneverbOutput) == 32 ? 1 : -1];\n'
                   'typedef char cell_is_16_bytes[sizeof(PlaneverbCell) == 16 ? 1 : -1];\n'
                   'int main(void) { PvAmdSlabInfo i; PvAmdInfo j; (void)i; (void)j; return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I",
                           os.path.join(ROOT, "include"), str(src)])


def test_host_libm_reproduces_the_reference_pulse(pvlib):
    """the Gaussian pulse is made with the HOST's expf (Grid.cpp:12-27): the library checks five samples of the reference's
    275 Hz table once per process and warns; here the check itself must hold (glibc 2.35 in this image and on the GPU box)"""
    assert pvlib.lib().PvAmdHostPulseSelfCheck() == 1


def test_worker_error_accessor_without_module(pvlib):
    assert pvlib.lib().PlaneverbWorkerError() == b""
    assert pvlib.lib().PlaneverbIsStreaming() == 0


def test_dominant_kernel_compiled_form():
    """The merged step kernel's register allocation decides the headline: tools/check_kernel_isa.py compiles pv_kernels.hip for
    gfx950 (no GPU needed) and checks the large-grid instantiations for the two compiled forms that were measured 3-4 % and
    18-23 % slower on MI355X (parked scalar offsets reloaded inside the steps; tile loads issued in groups with full waits)."""
    import shutil
    import subprocess
    import sys
    import warnings
    if not os.path.exists(shutil.which("hipcc") or "/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_kernel_isa.py")], capture_output=True, text=True,
                       timeout=900)
    # A PERFORMANCE guard, not a correctness test: by default a changed compiled form is REPORTED (a compiler bump may move
    # it without anything being wrong with the sources); PV_ISA_GUARD_STRICT=1 turns it into a failure (what a developer
    # who edits pv_kernels.hip wants before measuring on the GPU).
    if r.returncode != 0:
        if os.environ.get("PV_ISA_GUARD_STRICT") == "1":
            pytest.fail(r.stdout + r.stderr)
        warnings.warn("dominant kernel's compiled form changed (tools/check_kernel_isa.py):\n" + r.stdout[-1500:])
