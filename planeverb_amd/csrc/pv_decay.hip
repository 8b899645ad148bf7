// pv_decay.hip -- per-cell decay times (EDT, T20, T30: pv_decay.h) of the LAST COMPLETED run, read off the backward-integrated
// (Schroeder) curve of the recorded pressure history.  The one analysis pass that walks the history BACKWARDS in time.
//
// Kept from pv_room_metrics_kernel (pv_metrics.hip), because it is what makes every line of the history be fetched once per
// walk: one lane per cell, the cell being the lane's OFFSET g inside a history plane (pv_analysis.h planeCell), so the 64
// lanes of a wave read 256 contiguous bytes of one plane per load instruction; a ring of NB chunks of S planes of loads in
// flight per wave; a lane outside its own range loading through an out-of-extent buffer offset (the load returns 0 without
// touching memory -- a tile's history is stored only from the launch in which it first became non-zero, so nothing below a
// cell's onset may be read); every 64-cell group of the history window is visited, a wave without a live lane leaves at once,
// and every offset of the plane gets a record: eight quiet NaNs where the cell has no onset in this run.
//
// New here:
//  * Time runs DOWN, wave-uniform, from T - 1 to the smallest onset among the wave's live lanes; chunk c holds the steps
//    [T - (c + 1) S, T - c S) and its samples are consumed from the last to the first.
//  * The steps below a lane's own onset therefore come LAST.  There the load returned 0, e = 0 * 0 = +0.0f, and E + (+0.0f)
//    leaves E's bits alone: E is a sum of squares from +0.0f, never -0.0f, and x + (+0) = x for every other x.  So a lane
//    that has passed its onset holds E(t0) until the wave is done.  Its ratio r then stays 1, which lies inside the EDT
//    range: membership in a range is masked by k = t - t0 >= 0 (and t < tEnd), and a step that is no member changes none of
//    the range's sums (selects, not additions of zero).
//  * E0 = E(t0) is needed before the first ratio, so the curve is walked TWICE with the same loads in the same order and the
//    same additions: E(t0) of the second walk is E0 bit for bit.  The first walk is one multiply and one add per sample.  The
//    second adds the correctly rounded division, the logarithm, six compares and three pairs of double add / multiply.
//  * Skips that cannot change a bit, all wave-uniform: chunks at or after tEnd only advance E; while no lane of the wave has
//    r >= 0.00031622776f at the chunk's earliest step (r never decreases as t does, so none had it earlier in the walk) no step
//    can belong to a range and the division, the logarithm and the fits are skipped -- that is the late part of the record,
//    walked first; r(tEnd - 1), which completeness and depth need, is E(tEnd - 1) / E0 from the kept E.
//  * The logarithm inside the loop is pvLog10fNormalT (bit-identical to pvLog10f on positive normal floats, pv_libm.h) with
//    its table in LDS: a member step has r in [0.00031622776f, 1], and a step that is no member is given 1.0f instead.
//    depth takes the general pvLog10f once per cell (r(tEnd - 1) may be +0).
//
// Both walks live in ONE launch by default; PV_DECAY phase 1 / 2 are the two-launch form (E0 through the record's plane 6),
// kept for the comparison of profiles/decay_times.txt.
// One launch was the faster form on every grid measured (3 .. 8 %).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, S = 8, NB = 4; the ring holds 32 values, the three fits six
// doubles and nine ints): 94 VGPRs, no AGPRs, scratch size 0 bytes per lane, 768 bytes of LDS, 5 waves per SIMD.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_metrics.hip and
// pv_spectrum.hip and is covered by that parallel only: no test can afford such a plane.
//
// The text of the pass is decayTimesBody (pv_decay_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_decay.h"
#include "pv_decay_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kDecayBlock = 256;

template <int S, int NB, bool CHUNK, int PHASE>
__global__ __launch_bounds__(kDecayBlock) void pv_decay_times_kernel(const AnalyzeArgs a, float* __restrict__ out, int tailN) {
    __shared__ double tab[96];
    if (PHASE != 1) {
        fillLogTab(tab, threadIdx.x, kDecayBlock);
        __syncthreads();  // (before any wave leaves)
    }
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kDecayBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    decayTimesBody<S, NB, CHUNK, PHASE>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, LogTabLds{tab}, tailN);
}

template <int PHASE>
void launchDecayPhase(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int tailN = decayTailN((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kDecayBlock - 1) / kDecayBlock));
    if (a.histPlane * 4 * PV_DECAY_S < (1ll << 31))
        hipLaunchKernelGGL((pv_decay_times_kernel<PV_DECAY_S, PV_DECAY_NB, true, PHASE>), grid, dim3(kDecayBlock), 0, stream, a, out, tailN);
    else
        hipLaunchKernelGGL((pv_decay_times_kernel<PV_DECAY_S, PV_DECAY_NB, false, PHASE>), grid, dim3(kDecayBlock), 0, stream, a, out, tailN);
}

}  // namespace

// out: kDecayFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchDecayTimes(const AnalyzeArgs& a, float* out, bool twoLaunches, hipStream_t stream) {
    if (!twoLaunches) return launchDecayPhase<0>(a, out, stream);
    launchDecayPhase<1>(a, out, stream);
    launchDecayPhase<2>(a, out, stream);
}

}  // namespace pva
