// pv_lobes.hip -- per-cell directional energy lobes (pv_lobes.h) of the LAST COMPLETED run: the energy p^2 of every reached cell
// per time window after its onset, and that energy split over the four axial travel directions +x, -x, +y, -y by the squared
// direction cosines of the particle velocity, opposite directions kept apart.
//
// The frame is pv_echogram_kernel's (pv_echogram.hip), which see: one lane per cell, the cell being the lane's OFFSET g inside a
// history plane; THREE buffer loads per sample (the cell and its upstream neighbours (X - 1, Y) and (X, Y - 1), across tile
// edges as encodeWave computes them); an out-of-extent offset for everything that is zero by causality (the load returns 0
// without touching memory); a ring of NB chunks of S planes of loads in flight per wave with a sched_barrier behind each chunk's
// loads; face coefficients read once per lane; vx, vy by the stencil's own recurrence from tBegin = max(tileFirst, m - 1); time
// wave-uniform from the wave's smallest tBegin on; the CHUNK / !CHUNK descriptor forms; a wave without a live lane leaves after
// writing its NaNs; every float of the storage written by the one launch, no memset pass; 64-bit addressing of the record planes.
//
// Different here:
//  * The walk goes to T - 1: the last window is open-ended, so the cost is three loads per sample over the whole response, not
//    over a short window.
//  * Windows of unequal lengths.  Per lane: tNext, the step at which the lane's current window ends (onset + the smallest edge
//    above the current step count, or T), and w, the address of the current window's E plane.  At t + 1 == tNext the lane stores
//    its five sums, resets them to +0.0f and finds the next end by a chain of selects over the (at most 7) edges, which are
//    kernel arguments: no division per sample, no window index that could index a register array.
//  * Two correctly rounded divisions per sample (a / q, b / q).
//  * A live lane also writes n = (float)(T - onset) and five +0.0f into each window past its last one, a dead lane 1 + 5 nW quiet
//    NaNs.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see profiles/lobes.txt; no scratch, no LDS.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_lateral.hip and is
// covered by that parallel only: no test can afford such a plane.
//
// The text of the pass is lobesBody (pv_lobes_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_lobes.h"
#include "pv_lobes_dev.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kLobesBlock = 256;

template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kLobesBlock) void pv_lobes_kernel(const AnalyzeArgs a, float* __restrict__ out, const LobeEdges ed, int nW) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kLobesBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    lobesBody<S, NB, CHUNK>(a, dyn, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, ed, nW);
}

}  // namespace

// out: 1 + 5 nW planes of a.histPlane floats, float k of the cell at history offset g at out[k * histPlane + g]
void launchLobes(const AnalyzeArgs& a, float* out, const LobeEdges& ed, int nW, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kLobesBlock - 1) / kLobesBlock));
    if (a.histPlane * 4 * PV_LOBES_S < (1ll << 31))
        hipLaunchKernelGGL((pv_lobes_kernel<PV_LOBES_S, PV_LOBES_NB, true>), grid, dim3(kLobesBlock), 0, stream, a, out, ed, nW);
    else
        hipLaunchKernelGGL((pv_lobes_kernel<PV_LOBES_S, PV_LOBES_NB, false>), grid, dim3(kLobesBlock), 0, stream, a, out, ed, nW);
}

}  // namespace pva
