// pv_echo.hip -- per-cell echo criterion (Dietsch and Kraak; speech and music variant: pv_echo.h) of the LAST COMPLETED run, one
// forward pass over the recorded pressure history.
//
// The frame is pv_room_metrics_kernel's (pv_metrics.hip): one lane per OFFSET g of a history plane, wave-uniform time from the
// smallest onset among the wave's live lanes to T - 1, a lane outside its own range loading 0 through an out-of-extent buffer
// offset, a ring of NB chunks of S planes of loads in flight, both descriptor forms, a NaN record for every offset without an
// onset, and a wave without a live lane leaving at once.
//
// New here are the lagged centres.  x(k) needs c(k - nD), the value this very lane computed nD steps earlier, and nD has no bound
// that fits registers (12 and 20 steps at 70^2, hundreds on fine grids).  The pass keeps no c: per variant a second pair of sums,
// A' and B', is fed from p(t - nD) -- three load streams, p(t), p(t - nDs) and p(t - nDm) -- and makes exactly the additions the
// leading pair made nD steps earlier, masked by select while k - nD < 0.  B' / A' therefore has the bits of c(k - nD) (the
// argument is spelled out in DESIGN.md 4.15).  Nothing is added outside a lane's own range [onset, T): every update of pv_echo.h
// echoStep is a select on `on`, so the steps that wave-uniform time visits below a lane's onset or past T - 1 leave the lane's
// state untouched, whatever the loads returned.  A lagged plane t - nD is read only where t - nD >= onset (the tile's history
// exists from its first recorded launch, which is not later than the onset of any of its cells); everywhere else the lane's
// offset is out of extent.
//
// The speech weight is |p|^(2/3), glibc's powf (pv_libm.h pvPowfNonNegT): two evaluations per sample and lane, the leading and
// the lagged one, with the function's two tables (32 + 32 doubles) in LDS, filled by the block's first wave.  The 2 S
// evaluations of a chunk are written in front of the chunk's sequential part, so the scheduler has S independent chains of
// each.  Per sample the pass also makes six correctly rounded divisions (c and c' of both variants, x of both); it is bound by
// these and the double-precision work of powf, not by the history bytes (three times the room-metrics pass's, two thirds of
// them re-reads of lines the same wave fetched nD steps earlier).
//
// The text of the pass is echoBody (pv_echo_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that gives
// the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_records.hip runs the
// same body for the cells of a run's output queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_echo.h"
#include "pv_echo_dev.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kEchoBlock = 256;

template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kEchoBlock) void pv_echo_kernel(const AnalyzeArgs a, float* __restrict__ out, int nDs, int nDm, int nLs, int nLm) {
    __shared__ double powLt[32];
    __shared__ uint64_t powEt[32];
    fillPowTab(powLt, powEt, (int)threadIdx.x);
    __syncthreads();
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kEchoBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    echoBody<S, NB, CHUNK>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, PowTabLds{powLt, powEt}, nDs, nDm, nLs, nLm);
}

}  // namespace

// out: kEchoFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchEchoCriterion(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int fs = (int)a.fs;
    const int nDs = echoSpeechLag(fs), nDm = echoMusicLag(fs), nLs = echoSpeechLimit(fs), nLm = echoMusicLimit(fs);
    const dim3 grid((unsigned)((a.histPlane + kEchoBlock - 1) / kEchoBlock));
    if (a.histPlane * 4 * PV_ECHO_S < (1ll << 31))
        hipLaunchKernelGGL((pv_echo_kernel<PV_ECHO_S, PV_ECHO_NB, true>), grid, dim3(kEchoBlock), 0, stream, a, out, nDs, nDm, nLs, nLm);
    else
        hipLaunchKernelGGL((pv_echo_kernel<PV_ECHO_S, PV_ECHO_NB, false>), grid, dim3(kEchoBlock), 0, stream, a, out, nDs, nDm, nLs, nLm);
}

}  // namespace pva
