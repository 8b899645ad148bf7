// pv_lateral.hip -- per-cell early lateral energy fraction and early-sound direction (pv_lateral.h) of the LAST COMPLETED run:
// the pass that carries the velocity recurrence of the stencil through the whole 80 ms window of every reached cell at once.
//
// Kept from pv_room_metrics_kernel (pv_metrics.hip): one lane per cell, the cell being the lane's OFFSET g inside a history plane
// (pv_analysis.h planeCell), so the 64 lanes of a wave read 256 contiguous bytes of one plane per load instruction; a ring of NB
// chunks of S planes of buffer loads in flight per wave; a lane outside its own range loading through an out-of-extent buffer
// offset (the load returns 0 without touching memory -- a tile's history is stored only from the launch in which it first became
// non-zero); every 64-cell group of the history window is visited, a wave without a live lane leaves at once, and every offset of
// the plane gets a record: eleven quiet NaNs where the cell has no onset in this run.
//
// New here:
//  * THREE loads per sample: the cell itself and its upstream neighbours (X - 1, Y) and (X, Y - 1), whose offsets are computed as
//    encodeWave (pv_analysis_dev.h) computes them: one row / one cell back inside a tile, into the tile above / to the left
//    across a tile's first row / column.  A neighbour outside the window, or a sample before the neighbour tile's own first
//    recorded step, is exactly zero by causality and is loaded as zero (out-of-extent offset).  The neighbours' lines are the
//    lines other lanes of this or a nearby wave load as their own: the bytes fetched from memory stay those of one read.
//  * vx, vy by the stencil's own recurrence (v_t = v_{t-1} - C (p_t[i] - p_t[n]) on air|air faces, k (p_i + p_n) otherwise,
//    face coefficients read once per lane), from tBegin = max(tileFirst, m - 1), the first sample that can be non-zero (encodeWave):
//    before it the cell's and its neighbours' pressure are zero and an air face's velocity stays +0, so the values from tBegin on
//    are bit for bit those of pv_ir_kernel, which starts at the tile's first recorded sample.
//  * Time is wave-uniform from the smallest tBegin of the wave's live lanes to its largest min(onset + n80, T) -- NOT to T - 1:
//    the first of these passes that reads only a prefix of the history, so its cost does not grow with T.
//  * Membership of the recurrence (t in [tBegin, tEnd)) and of each sum (t in [onset, tEnd), k < n5 or k >= n5) is by select
//    (lateralStep), not by adding products of zero; pv_lateral.h says why that gives the bits of the definition, which adds +0.0f.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see profiles/lateral_fraction.txt; no scratch, no LDS.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_metrics.hip and is
// covered by that parallel only: no test can afford such a plane.
//
// The text of the pass is lateralBody (pv_lateral_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_lateral.h"
#include "pv_lateral_dev.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kLateralBlock = 256;

template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kLateralBlock) void pv_lateral_kernel(const AnalyzeArgs a, float* __restrict__ out, int n5, int n80) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kLateralBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    lateralBody<S, NB, CHUNK>(a, dyn, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, n5, n80);
}

}  // namespace

// out: kLateralFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchLateralFraction(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int n5 = lateralN5((int)a.fs), n80 = lateralN80((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kLateralBlock - 1) / kLateralBlock));
    if (a.histPlane * 4 * PV_LATERAL_S < (1ll << 31))
        hipLaunchKernelGGL((pv_lateral_kernel<PV_LATERAL_S, PV_LATERAL_NB, true>), grid, dim3(kLateralBlock), 0, stream, a, out, n5, n80);
    else
        hipLaunchKernelGGL((pv_lateral_kernel<PV_LATERAL_S, PV_LATERAL_NB, false>), grid, dim3(kLateralBlock), 0, stream, a, out, n5, n80);
}

}  // namespace pva
