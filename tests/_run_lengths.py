"""The run lengths (num_steps, T) at which the kernels that walk a run's history change what they do, for
tests/test_host_run_lengths.py and tests/test_gpu_run_lengths.py.  Every length is derived from the constant whose boundary it
sits on: the chunk (S) and ring (NB) sizes are read from the kernels' own sources, the sample counts are the float32 products the
library forms, and K (stepsPerLaunch) is stated here and asserted against Solver.info by the GPU tests."""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "planeverb_amd", "csrc")


def _constant(path, pattern):
    m = re.search(pattern, open(os.path.join(CSRC, path)).read(), re.M)
    assert m, (path, pattern)
    return int(m.group(1))


def _define(path, name):
    return _constant(path, r"^#define\s+%s\s+(\d+)\b" % name)


def steps_of(seconds, fs):
    """int(seconds * fs) as the library forms it: a float32 product, truncated"""
    return int(np.float32(seconds) * np.float32(fs))


FS = 1443      # the sampling rate of every 275 Hz grid (the GPU tests assert Solver.fs)
GRID_T = 435   # such a grid's own run length: num_steps above it is an extended run
K = 12         # stepsPerLaunch of the 24 x 50 grid (the GPU tests assert Solver.info.stepsPerLaunch)

# decay, bands, modulation, metrics, spectrum: one chunk, one ring
WALKS = {n: (_define("pv_%s_dev.h" % n, "PV_%s_S" % n.upper()), _define("pv_%s_dev.h" % n, "PV_%s_NB" % n.upper()))
         for n in ("decay", "bands", "modulation", "metrics", "spectrum", "echo", "lateral", "echogram", "lobes")}
S, NB = WALKS["decay"]
assert all(WALKS[n] == (S, NB) for n in ("bands", "modulation", "metrics", "spectrum")), WALKS
S_ECHO, NB_ECHO = WALKS["echo"]
S_VEL, NB_VEL = WALKS["lateral"]  # lateral, echogram, lobes: three loads per plane, a shorter ring
assert WALKS["echogram"] == WALKS["lobes"] == (S_VEL, NB_VEL) and S_VEL == S, WALKS
S_CORE = _define("pv_analysis_dev.h", "PV_RT60_TILE_S")  # the core analysis walks down from T - 1 in chunks of 2 S_CORE and S_CORE
assert S_CORE == S
WATERFALL_CHUNK = _constant("pv_waterfall.hip", r"^constexpr int kChunk = (\d+);")
MIX_BLOCK = _constant("pv_arrays.hip", r"^constexpr int kMixBlock = (\d+);")
TAIL = steps_of(0.01, FS)  # tailN = nCut = nDry
N50, N80 = steps_of(0.05, FS), steps_of(0.08, FS)
HALF_RING = 8 * K          # pv_solver.cpp: halfRing_ = min(roundUp(T, K), 8 K)
assert (S, NB, S_ECHO, NB_ECHO, NB_VEL, WATERFALL_CHUNK, MIX_BLOCK, TAIL, N50, N80, HALF_RING) == (8, 4, 4, 4, 2, 64, 256, 14, 72, 115, 96)

LENGTHS = {}  # T -> the boundaries it stands for


def _add(T, what):
    LENGTHS[T] = LENGTHS[T] + "; " + what if T in LENGTHS else what


# very short: the first chunk begins below step 0, every window and slot lies past T
_add(1, "one step: the onset is the last step")
_add(2, "two steps")
_add(3, "three steps")
# around S, 2 S and NB S (and the echo criterion's S)
_add(S_ECHO, "S of the echo criterion: its first chunk begins at step 0")
_add(S_ECHO + 1, "S of the echo criterion + 1: a second chunk of one step")
_add(S - 1, "S - 1: the first chunk begins at step -1")
_add(S, "S: exactly one full chunk (two of the echo criterion's)")
_add(S + 1, "S + 1: a second chunk of one step")
_add(2 * S - 1, "2 S - 1 (NB S - 1 of the echo criterion and of the two-chunk rings)")
_add(2 * S, "2 S: the ring of the velocity kinds exactly full; the 16-sample chunk of the core analysis; NB S of the echo criterion")
_add(2 * S + 1, "2 S + 1: the first refill of the velocity kinds' ring")
_add(NB * S - 1, "NB S - 1: the prologue's last chunk is short")
_add(NB * S, "NB S: the prologue's loads are the whole run")
_add(NB * S + 1, "NB S + 1: the first refill of the ring")
# around tailN = nCut = nDry
_add(TAIL - 1, "tailN - 1: tEnd = T - tailN and endPoint = T - nCut are negative")
_add(TAIL, "tailN: tEnd = endPoint = 0")
_add(TAIL + 1, "tailN + 1: tEnd = endPoint = 1")
_add(2 * TAIL - 1, "2 tailN - 1: nDry + nCut exceed the run by one")
_add(2 * TAIL + 1, "2 tailN + 1: one step between the dry window and the cut")
# around K = stepsPerLaunch
_add(K - 1, "K - 1: a single short launch")
_add(K, "K: exactly one launch")
_add(K + 1, "K + 1: a second launch of one step")
# around the 50 ms and 80 ms limits
_add(N50, "n50: the 50 ms limit is the first step past the run for an onset at 0")
_add(N50 + 1, "n50 + 1")
_add(N80, "n80: the 80 ms limit likewise")
_add(N80 + 1, "n80 + 1")
# around the waterfall's chunk
_add(WATERFALL_CHUNK - 1, "waterfall chunk - 1")
_add(WATERFALL_CHUNK, "waterfall chunk: exactly one sample load; two rings of NB S")
_add(WATERFALL_CHUNK + 1, "waterfall chunk + 1")
_add(2 * WATERFALL_CHUNK, "two waterfall chunks; four rings of NB S")
# around one and two halfRings of the sparse-emitter accumulate passes
_add(HALF_RING - 1, "halfRing - 1: roundUp(T, K) = 8 K, one short pass")
_add(HALF_RING, "halfRing: exactly one accumulate pass; three rings of NB S")
_add(HALF_RING + 1, "halfRing + 1: a second pass of one step")
_add(2 * HALF_RING, "two halfRings: both halves of the ring exactly full; six rings of NB S")
_add(2 * HALF_RING + 1, "two halfRings + 1: the first half is used again")
# around the array mix block (and the 256-thread row groups of the zone kernels)
_add(MIX_BLOCK - 1, "mix block - 1")
_add(MIX_BLOCK, "mix block: exactly one block of the array mix, one row group of the zone kernels; eight rings of NB S")
_add(MIX_BLOCK + 1, "mix block + 1")
# extended runs: num_steps above the grid's own T, no pulse after it
_add(GRID_T + 1, "the grid's T + 1: the shortest extended run")
_add(2 * HALF_RING + MIX_BLOCK, "an extended run that is a multiple of NB S and of the waterfall chunk")
_add(500, "an extended run well past the pulse table")
assert sorted(LENGTHS) == [1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 27, 29, 31, 32, 33, 63, 64, 65, 72, 73, 95, 96, 97, 115, 116,
                           128, 192, 193, 255, 256, 257, 436, 448, 500]

ALL = sorted(LENGTHS)
WITHIN = [T for T in ALL if T <= GRID_T]  # the oracle's ring refuses more steps than the grid's own T
EXTENDED = [T for T in ALL if T > GRID_T]
# the zone reductions: around S, tailN, the waterfall chunk (four row groups of 16 slots) and the 256-thread row group
ZONES = [S - 1, S, S + 1, TAIL - 1, TAIL, TAIL + 1, WATERFALL_CHUNK - 1, WATERFALL_CHUNK, WATERFALL_CHUNK + 1,
         MIX_BLOCK - 1, MIX_BLOCK, MIX_BLOCK + 1]
# waterfalls and source arrays: one step, the 15-step slice, the chunk, the mix block, an extended run
RECEIVERS = [1, 2 * S - 1, 2 * S, WATERFALL_CHUNK - 1, WATERFALL_CHUNK, WATERFALL_CHUNK + 1, MIX_BLOCK - 1, MIX_BLOCK, MIX_BLOCK + 1,
             2 * HALF_RING + MIX_BLOCK]
# in-run records and sparse-emitter mode: one step, K, one and two halfRings, an extended run
IN_RUN = [1, K - 1, K, K + 1, HALF_RING - 1, HALF_RING, HALF_RING + 1, 2 * HALF_RING, 2 * HALF_RING + 1, GRID_T + 1]
assert set(ZONES + RECEIVERS + IN_RUN) <= set(ALL)


def ident(T):
    return "T%d" % T
