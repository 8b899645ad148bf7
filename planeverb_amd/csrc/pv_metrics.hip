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
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_metrics.h"
#include "pv_prims.h"

#ifndef PV_METRICS_S
#define PV_METRICS_S 8  // planes per chunk
#endif
#ifndef PV_METRICS_NB
#define PV_METRICS_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

namespace {

constexpr int kMetricsBlock = 256;

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kMetricsBlock) void pv_room_metrics_kernel(const AnalyzeArgs a, float* __restrict__ out, int n50, int n80) {
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kMetricsBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (g < plane && !live) {
        const float qnan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < kRoomMetricFloats; ++k) out[k * plane + g] = qnan;
    }
    if (__ballot(live) == 0ull) return;

    const int t0 = live ? (int)delay : 0;
    const int t0l = live ? t0 : INT_MAX;  // (a dead lane never loads)
    int t0min = live ? t0 : INT_MAX, t0max = live ? t0 : INT_MIN;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        t0min = min(t0min, __shfl_xor(t0min, off));
        t0max = max(t0max, __shfl_xor(t0max, off));
    }
    // (wave-uniform by value; said so to the compiler: scalar loop counters and descriptors)
    t0min = max(__builtin_amdgcn_readfirstlane(t0min), 0);
    t0max = __builtin_amdgcn_readfirstlane(t0max);
    const int hiAll = t0max + n80;  // from here on every live lane is in both late windows (n80 >= n50)
    const int voff = (int)g * 4;
    const int lvoff = live ? voff : kOut;

    float ring[NB][S];
    // the S loads of the chunk that begins at step tc (issued whatever tc is: the counts are the same on every path)
    auto loadChunk = [&](float (&dst)[S], int tc) {
        const int tb = min(tc, T - 1);  // (a chunk past the end: every lane out of range, the base stays inside the history)
        const rsrc_t rs = makeRsrc(a.hist + (long long)tb * plane, CHUNK ? (long long)S * planeBytes : (long long)planeBytes);
        if (tc >= t0max && tc + S <= T) {  // every live lane is inside its range
#pragma unroll
            for (int k = 0; k < S; ++k)
                dst[k] = CHUNK ? bufLoadF(rs, lvoff, (int)((unsigned)k * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)(tc + k) * plane, planeBytes), lvoff, 0);
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k;
                const int vo = (t < T && t >= t0l) ? voff : kOut;
                dst[k] = CHUNK ? bufLoadF(rs, vo, (int)((unsigned)k * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)min(t, T - 1) * plane, planeBytes), vo, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    RoomSums s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int n = (T - t0min + S - 1) / S;  // chunks from the wave's smallest onset to T - 1
#pragma unroll
    for (int b = 0; b < NB; ++b) loadChunk(ring[b], t0min + b * S);
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int tc = t0min + (c0 + b) * S;
            float p[S];
#pragma unroll
            for (int k = 0; k < S; ++k) p[k] = ring[b][k];
            loadChunk(ring[b], tc + NB * S);  // the slot's next occupant
            if (tc >= T) continue;  // (past the last chunk: those loads returned 0)
            if (tc >= hiAll) {
                float kf = (float)(tc - t0);  // (float)k, counted up: exact (integers below 2^24)
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const float e = p[k] * p[k];  // (+0 past T - 1)
                    s.l50 = s.l50 + e;
                    s.l80 = s.l80 + e;
                    s.total = s.total + e;
                    const float m = kf * e;
                    s.moment = s.moment + m;
                    kf = kf + 1.f;
                }
            } else {
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const int kk = tc + k - t0;   // (below the lane's onset: negative, and e = +0)
                    const float e = p[k] * p[k];
                    s.e50 = s.e50 + (kk < n50 ? e : 0.f);
                    s.l50 = s.l50 + (kk < n50 ? 0.f : e);
                    s.e80 = s.e80 + (kk < n80 ? e : 0.f);
                    s.l80 = s.l80 + (kk < n80 ? 0.f : e);
                    s.total = s.total + e;
                    const float m = (float)kk * e;
                    s.moment = s.moment + m;
                }
            }
        }
    }
    if (!live) return;
    float c50, c80, d50, ts;
    roomMetricsDerive(s, (int)a.fs, &c50, &c80, &d50, &ts);
    out[0 * plane + g] = c50;
    out[1 * plane + g] = c80;
    out[2 * plane + g] = d50;
    out[3 * plane + g] = ts;
    out[4 * plane + g] = s.e50;
    out[5 * plane + g] = s.l50;
    out[6 * plane + g] = s.e80;
    out[7 * plane + g] = s.l80;
    out[8 * plane + g] = s.total;
    out[9 * plane + g] = s.moment;
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
