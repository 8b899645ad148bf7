// pv_metrics_dev.h -- the body of the room-metrics pass (pv_metrics.hip, which describes it), shared by the whole-map kernel and
// the in-run query kernel (pv_query_records.hip): which cell the lane owns and where its record goes come from the caller
// (pv_record_lane.h), everything else -- loads, ring, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_metrics.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_METRICS_S
#define PV_METRICS_S 8  // planes per chunk
#endif
#ifndef PV_METRICS_NB
#define PV_METRICS_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void roomMetricsBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, int n50, int n80) {
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ln.g;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (ln.slot && !live) {
        const float qnan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < kRoomMetricFloats; ++k) out(k, qnan);
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
    out(0, c50);
    out(1, c80);
    out(2, d50);
    out(3, ts);
    out(4, s.e50);
    out(5, s.l50);
    out(6, s.e80);
    out(7, s.l80);
    out(8, s.total);
    out(9, s.moment);
}

}  // namespace pva
