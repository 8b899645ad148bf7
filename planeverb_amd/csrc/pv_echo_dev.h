// pv_echo_dev.h -- the body of the echo-criterion pass (pv_echo.hip, which describes it), shared by the whole-map kernel and the in-run query
// kernel (pv_query_records.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_echo.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_ECHO_S
#define PV_ECHO_S 4  // planes per chunk and stream
#endif
#ifndef PV_ECHO_NB
#define PV_ECHO_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

struct PowTabLds {
    const double* lt;    // 16 x {invc, logc}
    const uint64_t* et;  // 32 exp2 entries
    __device__ __forceinline__ void log2(int i, double* invc, double* logc) const {
        *invc = lt[2 * i];
        *logc = lt[2 * i + 1];
    }
    __device__ __forceinline__ uint64_t exp2(int j) const { return et[j]; }
};

// CHUNK: a chunk's S planes through ONE descriptor and S scalar offsets (S planes must stay below 2^31 bytes); otherwise one
// descriptor per plane
// powf's two tables into LDS (32 doubles, 32 words), by the block's first wave; the caller synchronises behind it
__device__ __forceinline__ void fillPowTab(double* powLt, uint64_t* powEt, const int tid) {
    if (tid < 32) {
        double invc, logc;
        PvPowTabConst{}.log2(tid >> 1, &invc, &logc);
        powLt[tid] = (tid & 1) ? logc : invc;
    } else if (tid < 64) {
        powEt[tid - 32] = PvPowTabConst{}.exp2(tid - 32);
    }
}

template <int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void echoBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, const PowTabLds& ptab, int nDs, int nDm,
                                         int nLs, int nLm) {
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
        for (int k = 0; k < kEchoFloats; ++k) out(k, qnan);
    }
    if (__ballot(live) == 0ull) return;

    const int t0 = live ? (int)delay : 0;
    const int t0l = live ? t0 : INT_MAX;  // (a dead lane never loads and is never `on`)
    int t0min = live ? t0 : INT_MAX, t0max = live ? t0 : INT_MIN;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        t0min = min(t0min, __shfl_xor(t0min, off));
        t0max = max(t0max, __shfl_xor(t0max, off));
    }
    // (wave-uniform by value; said so to the compiler: scalar loop counters and descriptors)
    t0min = max(__builtin_amdgcn_readfirstlane(t0min), 0);
    t0max = __builtin_amdgcn_readfirstlane(t0max);
    const int voff = (int)g * 4;
    const int lvoff = live ? voff : kOut;

    // the S loads of one stream's chunk: steps tc .. tc + S - 1, planes tc - lag .. (issued whatever tc is: the counts are the
    // same on every path).  A lane gets p(t - lag) where t < T and t - lag >= its onset, 0 elsewhere
    auto loadStream = [&](float (&dst)[S], int tc, int lag) {
        const int tl = tc - lag;                  // the chunk's first plane (negative: the stream has not begun)
        const int tb = min(max(tl, 0), T - 1);    // (the base stays inside the history)
        const rsrc_t rs = makeRsrc(a.hist + (long long)tb * plane, CHUNK ? (long long)S * planeBytes : (long long)planeBytes);
        if (tl >= t0max && tc + S <= T) {  // every live lane is inside its range (t0max >= 0: tb = tl)
#pragma unroll
            for (int k = 0; k < S; ++k)
                dst[k] = CHUNK ? bufLoadF(rs, lvoff, (int)((unsigned)k * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)(tl + k) * plane, planeBytes), lvoff, 0);
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k, tp = t - lag;
                const int vo = (t < T && tp >= t0l) ? voff : kOut;
                // (a lane in range has 0 <= tp - tb <= k: tb = tl, or tb = 0 > tl; the clamp serves the others)
                const int dk = min(max(tp - tb, 0), S - 1);
                dst[k] = CHUNK ? bufLoadF(rs, vo, (int)((unsigned)dk * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)min(max(tp, 0), T - 1) * plane, planeBytes), vo, 0);
            }
        }
    };
    float ring[NB][3][S];
    auto loadChunk = [&](float (&dst)[3][S], int tc) {
        loadStream(dst[0], tc, 0);
        loadStream(dst[1], tc, nDs);
        loadStream(dst[2], tc, nDm);
        __builtin_amdgcn_sched_barrier(0);
    };

    EchoVar sp = echoVarInit(), mu = echoVarInit();
    const float nDsf = (float)nDs, nDmf = (float)nDm;
    const int n = (T - t0min + S - 1) / S;  // chunks from the wave's smallest onset to T - 1
#pragma unroll
    for (int b = 0; b < NB; ++b) loadChunk(ring[b], t0min + b * S);
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int tc = t0min + (c0 + b) * S;
            float a0[S], as[S], am[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                a0[k] = echoAbs(ring[b][0][k]);
                as[k] = echoAbs(ring[b][1][k]);
                am[k] = echoAbs(ring[b][2][k]);
            }
            loadChunk(ring[b], tc + NB * S);  // the slot's next occupant
            if (tc >= T) continue;            // (past the last chunk)
            float ws[S], wls[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                ws[k] = pvPowfNonNegT(a0[k], kEchoSpeechExponent, ptab);
                wls[k] = pvPowfNonNegT(as[k], kEchoSpeechExponent, ptab);
            }
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k;
                const bool on = t >= t0l && t < T;
                const int kk = t - t0;  // (below the lane's onset: negative, and `on` is false)
                echoStep(sp, on, kk, ws[k], wls[k], nDs, nDsf, nLs);
                echoStep(mu, on, kk, a0[k], am[k], nDm, nDmf, nLm);
            }
        }
    }
    if (!live) return;
    float rec[kEchoFloats];
    echoRecord(sp, (int)a.fs, rec);
    echoRecord(mu, (int)a.fs, rec + 5);
#pragma unroll
    for (int k = 0; k < kEchoFloats; ++k) out(k, rec[k]);
}

}  // namespace pva
