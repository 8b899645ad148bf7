// pv_decay_dev.h -- the body of the decay-times pass (pv_decay.hip, which describes it), shared by the whole-map kernel and the in-run query
// kernel (pv_query_records.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_decay.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_DECAY_S
#define PV_DECAY_S 8  // planes per chunk
#endif
#ifndef PV_DECAY_NB
#define PV_DECAY_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

// PHASE 0: both walks;  1: the first walk alone, E0 to out plane 6;  2: the second walk alone, E0 from out plane 6.
// CHUNK: a chunk's S planes through ONE descriptor and S scalar offsets (S planes must stay below 2^31 bytes); otherwise one
// descriptor per plane
// ltab: the logarithm's table in LDS (fillLogTab and a barrier, by the caller; PHASE 1 does not read it)
template <int S, int NB, bool CHUNK, int PHASE, class Store>
__device__ __forceinline__ void decayTimesBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, const LogTabLds& ltab, int tailN) {
    const int T = a.T;
    const int tEnd = T - tailN;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ln.g;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (PHASE != 2 && ln.slot && !live) {
        const float qnan = decayQuietNan();
#pragma unroll
        for (int k = 0; k < kDecayFloats; ++k) out(k, qnan);
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
    t0min = min(max(__builtin_amdgcn_readfirstlane(t0min), 0), T);
    t0max = __builtin_amdgcn_readfirstlane(t0max);
    const int voff = (int)g * 4;
    const int lvoff = live ? voff : kOut;

    float ring[NB][S];
    // the S loads of the chunk that begins at step tc <= T - S (issued whatever tc is: the counts are the same on every path)
    auto loadChunk = [&](float (&dst)[S], int tc) {
        const int tb = max(tc, 0);  // (a chunk that reaches below step 0: those steps are out of every lane's range)
        const rsrc_t rs = makeRsrc(a.hist + (long long)tb * plane, CHUNK ? (long long)S * planeBytes : (long long)planeBytes);
        if (tc >= t0max) {  // every live lane is inside its range (t0max >= 0)
#pragma unroll
            for (int k = 0; k < S; ++k)
                dst[k] = CHUNK ? bufLoadF(rs, lvoff, (int)((unsigned)k * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)(tc + k) * plane, planeBytes), lvoff, 0);
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k;
                const int vo = t >= t0l ? voff : kOut;  // (t0l >= 0)
                const int rel = max(t - tb, 0);         // (k, unless the chunk reaches below step 0)
                dst[k] = CHUNK ? bufLoadF(rs, vo, (int)((unsigned)rel * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)max(t, 0) * plane, planeBytes), vo, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    const int n = (T - t0min + S - 1) / S;  // chunks from T - 1 down to the wave's smallest onset
    float E0 = 0.f;
    if (PHASE != 2) {
        // ---- first walk: E(t0)
        float E = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) loadChunk(ring[b], T - (b + 1) * S);
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const int tc = T - (c0 + b + 1) * S;
                float p[S];
#pragma unroll
                for (int k = 0; k < S; ++k) p[k] = ring[b][k];
                loadChunk(ring[b], tc - NB * S);  // the slot's next occupant
                if (c0 + b >= n) continue;        // (below the last chunk: those loads returned 0)
#pragma unroll
                for (int k = S - 1; k >= 0; --k) {
                    const float e = p[k] * p[k];  // (+0 below the lane's onset)
                    E = E + e;
                }
            }
        }
        E0 = E;
        if (PHASE == 1) {
            if (live) out(6, E0);
            return;
        }
    } else {
        E0 = live ? out.load(6) : 0.f;
    }

    // ---- second walk: the same sums again, and the fits
    DecayFit f[kDecayRanges] = {{0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}};
    float E = 0.f, eEnd = 0.f;
    bool deep = false;  // wave-uniform: some lane has reached r >= kDecayLoAll
#pragma unroll
    for (int b = 0; b < NB; ++b) loadChunk(ring[b], T - (b + 1) * S);
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int tc = T - (c0 + b + 1) * S;
            float p[S];
#pragma unroll
            for (int k = 0; k < S; ++k) p[k] = ring[b][k];
            loadChunk(ring[b], tc - NB * S);  // the slot's next occupant
            if (c0 + b >= n) continue;        // (below the last chunk: those loads returned 0)
            float Es[S];
#pragma unroll
            for (int k = S - 1; k >= 0; --k) {
                const float e = p[k] * p[k];  // (+0 below the lane's onset)
                E = E + e;
                Es[k] = E;
            }
            if (tc >= tEnd) continue;  // the tail: E alone
            if (tc + S >= tEnd) {      // (the chunk that holds step tEnd - 1)
#pragma unroll
                for (int k = 0; k < S; ++k) eEnd = (tc + k == tEnd - 1) ? Es[k] : eEnd;
            }
            if (!deep) {
                deep = __ballot((Es[0] / E0) >= kDecayLoAll) != 0ull;  // (a dead lane: E0 = 0, the ratio is NaN)
                if (!deep) continue;
            }
#pragma unroll
            for (int k = S - 1; k >= 0; --k) {
                const int t = tc + k, kk = t - t0;
                const float r = Es[k] / E0;
                const bool own = kk >= 0 && t < tEnd && r >= kDecayLoAll;  // (r <= 1 always)
                const float L = 10.0f * pvLog10fNormalT(own ? r : 1.0f, ltab);
#pragma unroll
                for (int j = 0; j < kDecayRanges; ++j) decayFitStep(f[j], own && decayInRange(j, r), kk, L);
            }
        }
    }
    if (!live) return;
    float rec[kDecayFloats];
    decayDerive(f, E0, eEnd / E0, t0 < tEnd, (int)a.fs, rec);
#pragma unroll
    for (int k = 0; k < kDecayFloats; ++k) out(k, rec[k]);
}

}  // namespace pva
