// pv_echogram.hip -- per-cell directional echogram (pv_echogram.h) of the LAST COMPLETED run: the energy p^2 and the flux p vx,
// p vy of every reached cell per time slot of ns steps, over the nSlots slots that follow the cell's onset.
//
// Kept from pv_lateral_kernel (pv_lateral.hip), of which this pass is the continuation: one lane per cell, the cell being the
// lane's OFFSET g inside a history plane; THREE buffer loads per sample (the cell and its upstream neighbours (X - 1, Y) and
// (X, Y - 1), across tile edges as encodeWave computes them); an out-of-extent offset for everything that is zero by causality
// (the load returns 0 without touching memory); a ring of NB chunks of S planes of loads in flight per wave with a sched_barrier
// behind each chunk's loads; face coefficients read once per lane; vx, vy by the stencil's own recurrence from
// tBegin = max(tileFirst, m - 1); time wave-uniform from the wave's smallest tBegin to its largest tEnd, so the cost follows the
// window ns * nSlots and not T; the CHUNK / !CHUNK descriptor forms; a wave without a live lane leaves after writing its NaNs.
//
// New here:
//  * Slot bookkeeping per lane, because onsets differ per lane: tNext, the step at which the lane's current slot ends
//    (min(onset + (j + 1) ns, tEnd)), and w, the address of the current slot's e plane.  A counter that moves by ns at each
//    flush: no division per sample, and no slot index that could index a register array.
//  * Flush as you go.  At t + 1 == tNext the lane stores its three sums (three predicated 4-byte stores per lane per ns steps,
//    next to 3 ns loads), resets them to +0.0f and moves on to the next slot.  ns and nSlots are kernel arguments.
//  * A live lane also writes n = (float)(tEnd - onset) and +0.0f into the slots past its last one, a dead lane 1 + 3 nSlots quiet
//    NaNs: every float of the storage is defined by one launch, there is no memset pass.
//  * The records' planes (out[k * histPlane + g], k = 0 .. 3 nSlots) are addressed through 64-bit pointers: at 4096^2 cells and
//    32 slots they span 6.5 GB.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see profiles/echogram.txt; no scratch, no LDS.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_lateral.hip and is
// covered by that parallel only: no test can afford such a plane.
//
// The text of the pass is echogramBody (pv_echogram_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_echogram.h"
#include "pv_echogram_dev.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kEchogramBlock = 256;

template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kEchogramBlock) void pv_echogram_kernel(const AnalyzeArgs a, float* __restrict__ out, int ns, int nSlots) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kEchogramBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    echogramBody<S, NB, CHUNK>(a, dyn, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, ns, nSlots);
}

}  // namespace

// out: 1 + 3 nSlots planes of a.histPlane floats, float k of the cell at history offset g at out[k * histPlane + g]
void launchEchogram(const AnalyzeArgs& a, float* out, int ns, int nSlots, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kEchogramBlock - 1) / kEchogramBlock));
    if (a.histPlane * 4 * PV_ECHOGRAM_S < (1ll << 31))
        hipLaunchKernelGGL((pv_echogram_kernel<PV_ECHOGRAM_S, PV_ECHOGRAM_NB, true>), grid, dim3(kEchogramBlock), 0, stream, a, out, ns, nSlots);
    else
        hipLaunchKernelGGL((pv_echogram_kernel<PV_ECHOGRAM_S, PV_ECHOGRAM_NB, false>), grid, dim3(kEchogramBlock), 0, stream, a, out, ns, nSlots);
}

}  // namespace pva
