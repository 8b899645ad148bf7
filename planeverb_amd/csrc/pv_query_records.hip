// pv_query_records.hip -- the per-cell analysis records of a run for the cells of its registered output queries, computed INSIDE
// the run (PvAmdSetQueryRecords): one launch behind the run's analysis, in front of its last kernel, straight into pinned host
// memory.  No pass over the history window, no per-cell device storage, no host synchronisation of its own.
//
// One wave per block; blockIdx.x is the selected-kind ordinal (a wave-uniform switch), blockIdx.y the group of 64 queries: lane l
// of group g serves query i = 64 g + l (up to kMaxRecordQueries; one group, the launch of before, up to 64).  A lane's cell comes
// from the query table (recordLaneOfCell, pv_record_lane.h: the history offset g of the cell, where the cell lies inside the
// run's history window), its record goes to the query's AoS slot.  Between the two runs the body of the kind's whole-map pass
// (pv_metrics_dev.h ... pv_lobes_dev.h), the SAME text the whole-map kernel is made of: the same loads with the same
// out-of-extent rules, the same ring, the same step functions in the same order from +0.0f.  What a lane adds at a step is
// decided by selects on its own ranges, so a record's bits do not depend on the other lanes of the wave: record i is bit for bit
// what PvAmdGet<Kind> returns at the query's position after PvAmdCompute<Kind> on the same run.
//
// In sparse-emitter mode (PvAmdSetEmitterRecords) the same kernel serves the registered emitters: the history planes are the
// emitters' record traces and a lane's offsets are its columns there (recordLaneOfTrace); the bodies do not know the difference.
//
// For the source arrays (PvAmdComputeArrays, pv_arrays.hip) the same kernel serves the arrays after a completed run: the history
// planes are the mix planes and a lane's offset is its column there (recordLaneOfMix); the record block is device memory.
//
// Lanes at or above nq have no slot and no cell; a query off the map, outside the window or without an onset gets quiet NaNs.
// The stores are plain vector stores to host-coherent memory; they are visible to the host when the stream has drained, as
// pv_gather_queries_kernel's are.
//
// Cost: a lone wave per kind walks its dependent chain once -- the launch takes what its slowest selected kind takes for one
// wave, whatever the grid, the window or the number of queries (the groups are independent waves on other compute units).  The
// wave's 64 loads of a step hit up to 64 different lines.
#include <hip/hip_runtime.h>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_decay_dev.h"
#include "pv_device.h"
#include "pv_echo_dev.h"
#include "pv_echogram_dev.h"
#include "pv_lateral_dev.h"
#include "pv_launch.h"
#include "pv_lobes_dev.h"
#include "pv_metrics_dev.h"
#include "pv_query_records.h"
#include "pv_record_lane.h"

namespace pva {

namespace {

static_assert(PV_METRICS_S <= 8 && PV_DECAY_S <= 8 && PV_LATERAL_S <= 8 && PV_ECHOGRAM_S <= 8 && PV_ECHO_S <= 8 && PV_LOBES_S <= 8,
              "launchQueryRecords chooses the one-descriptor-per-chunk form for chunks of at most 8 planes");

// FORM (pv_record_lane.h RecordLaneForm): kLaneCell, the registered queries' cells; kLaneTrace, the lanes are the registered emitters
// of sparse-emitter mode and the history is their record traces (recordLaneOfTrace); kLaneMix, the lanes are the source arrays and
// the history is their mix planes (recordLaneOfMix) -- a mix has no cell, so the three velocity kinds are not in that form
template <bool CHUNK, int FORM>
__global__ __launch_bounds__(64) void pv_query_records_kernel(const AnalyzeArgs a, const QueryRecordArgs q) {
    __shared__ double logTab[96];
    __shared__ double powLt[32];
    __shared__ uint64_t powEt[32];
    // the blockIdx.x-th selected kind (wave-uniform)
    int kind = -1;
    for (int k = 0, left = (int)blockIdx.x; k < kQueryRecordKinds; ++k)
        if ((q.kinds >> k) & 1u) {
            if (left == 0) {
                kind = k;
                break;
            }
            --left;
        }
    if (kind < 0) return;
    const int lane = (int)threadIdx.x;
    if (kind == kQrecDecay) fillLogTab(logTab, lane, 64);
    if (kind == kQrecEchoCriterion) fillPowTab(powLt, powEt, lane);
    __syncthreads();

    const DynParams dyn = *a.dyn;
    const int i = 64 * (int)blockIdx.y + lane;  // the query (the group is wave-uniform)
    const bool slot = i < q.nq;
    const RecordLane ln = recordLaneOfForm<FORM>(a, dyn, q.cells, i, slot);
    // (a lane without a slot never stores: it is not live, and the NaN fill asks for the slot)
    const SlotStore out{q.out + q.offset[kind] + (long long)(slot ? i : 0) * q.floats[kind]};
    switch (kind) {
        case kQrecRoomMetrics:
            roomMetricsBody<PV_METRICS_S, PV_METRICS_NB, CHUNK>(a, ln, out, q.n50, q.n80);
            break;
        case kQrecDecay:
            decayTimesBody<PV_DECAY_S, PV_DECAY_NB, CHUNK, 0>(a, ln, out, LogTabLds{logTab}, q.tailN);
            break;
        case kQrecLateral:
            if constexpr (FORM != kLaneMix) lateralBody<PV_LATERAL_S, PV_LATERAL_NB, CHUNK>(a, dyn, ln, out, q.n5, q.latN80);
            break;
        case kQrecEchogram:
            if constexpr (FORM != kLaneMix) echogramBody<PV_ECHOGRAM_S, PV_ECHOGRAM_NB, CHUNK>(a, dyn, ln, out, q.ns, q.nSlots);
            break;
        case kQrecEchoCriterion:
            echoBody<PV_ECHO_S, PV_ECHO_NB, CHUNK>(a, ln, out, PowTabLds{powLt, powEt}, q.nDs, q.nDm, q.nLs, q.nLm);
            break;
        case kQrecLobes:
            if constexpr (FORM != kLaneMix) lobesBody<PV_LOBES_S, PV_LOBES_NB, CHUNK>(a, dyn, ln, out, q.ed, q.nW);
            break;
        default: break;
    }
}

}  // namespace

// q.kinds != 0, 0 < q.nq <= kMaxRecordQueries; q.cells, q.out: device-visible pinned host memory (q.out holds, per selected kind, nq x floats[kind] floats from
// offset[kind] on); the settings of every selected kind filled in by the caller
void launchQueryRecords(const AnalyzeArgs& a, const QueryRecordArgs& q, hipStream_t stream) {
    const dim3 grid((unsigned)__builtin_popcount(q.kinds), (unsigned)((q.nq + 63) / 64));
    // (the largest chunk of the six passes is 8 planes: one descriptor per chunk below 2^31 bytes, as in their own launchers)
    // (record traces -- a.hist = a.recTrace, planes of at most 3 x 1024 floats -- always take the chunk form)
    // (mix planes -- q.mix, a.hist = the planes of at most kArraysMax floats -- too)
    if (q.mix)
        hipLaunchKernelGGL((pv_query_records_kernel<true, kLaneMix>), grid, dim3(64), 0, stream, a, q);
    else if (a.recTrace)
        hipLaunchKernelGGL((pv_query_records_kernel<true, kLaneTrace>), grid, dim3(64), 0, stream, a, q);
    else if (a.histPlane * 4 * 8 < (1ll << 31))
        hipLaunchKernelGGL((pv_query_records_kernel<true, kLaneCell>), grid, dim3(64), 0, stream, a, q);
    else
        hipLaunchKernelGGL((pv_query_records_kernel<false, kLaneCell>), grid, dim3(64), 0, stream, a, q);
}

}  // namespace pva
