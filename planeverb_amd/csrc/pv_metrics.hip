// pv_metrics.hip -- per-cell room-acoustic metrics (C50, C80, D50, Ts: pv_metrics.h) of the LAST COMPLETED run, one forward
// pass over the recorded pressure history.
//
// One lane per cell, the cell being the lane's OFFSET g inside a history plane (pv_analysis.h planeCell, as in
// pv_rt60_tile_kernel): the 64 lanes of a wave read 256 contiguous bytes of one plane per load instruction, and every line of
// the history is fetched once.  Time is wave-uniform, from the smallest onset among the wave's live lanes to T - 1; a lane
// outside its own range loads through an out-of-range buffer offset (the load returns 0 without touching memory -- a tile's
// history is stored only from the launch in which it first became non-zero, so nothing below a cell's onset may be read) and
// adds 0 * 0 = +0.0f, the identity of these non-negative sums, bit for bit.  The k < n50 / k < n80 selection between the early
// and the late sums is the same trick.  Once every live lane of the wave is past its 80 ms window (t >= largest onset + n80)
// the early sums would only receive +0.0f: those chunks advance the three late sums and the moment alone.
// The loop body is one multiply, one convert-multiply and at most six adds per sample, so the pass is meant to be bound by the
// history bytes: a ring of NB chunks of S planes of loads is in flight per wave, as in pv_rt60_tile_kernel.
//
// Which groups: the run's list of live 64-cell groups (AnalyzeArgs::unitList) is NOT valid after a run -- the run's last kernel
// (pv_run_finish_kernel / pv_run_status_kernel) resets its count for the next run -- so the pass walks every 64-cell group of
// the history window and a wave without a live lane leaves at once (one gathered read of the delay map, one ballot).  Every
// offset of the plane gets a record: NaN where the cell has no onset in this run (or lies outside the result map).
//
// The text of the pass is roomMetricsBody (pv_metrics_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_metrics.h"
#include "pv_metrics_dev.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kMetricsBlock = 256;

template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kMetricsBlock) void pv_room_metrics_kernel(const AnalyzeArgs a, float* __restrict__ out, int n50, int n80) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kMetricsBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    roomMetricsBody<S, NB, CHUNK>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, n50, n80);
}

}  // namespace

// out: kRoomMetricFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchRoomMetrics(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int n50 = roomMetricsN50((int)a.fs), n80 = roomMetricsN80((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kMetricsBlock - 1) / kMetricsBlock));
    if (a.histPlane * 4 * PV_METRICS_S < (1ll << 31))
        hipLaunchKernelGGL((pv_room_metrics_kernel<PV_METRICS_S, PV_METRICS_NB, true>), grid, dim3(kMetricsBlock), 0, stream, a, out, n50, n80);
    else
        hipLaunchKernelGGL((pv_room_metrics_kernel<PV_METRICS_S, PV_METRICS_NB, false>), grid, dim3(kMetricsBlock), 0, stream, a, out, n50, n80);
}

}  // namespace pva
