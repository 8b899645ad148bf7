// pv_modulation_dev.h -- the body of the modulation pass (pv_modulation.hip, which describes it), shared by the whole-map kernel and the
// in-run query kernel (pv_query_spectral.hip): which cell the lane owns and where its record goes come from the caller
// (pv_record_lane.h), everything else -- loads, ring, filter, table rows, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_modulation.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_MODULATION_S
#define PV_MODULATION_S 8  // planes per chunk
#endif
#ifndef PV_MODULATION_NB
#define PV_MODULATION_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

static_assert(PV_MODULATION_S * PV_MODULATION_NB <= kModTablePad, "the last chunk may begin at step -(S - 1): table rows down to there");

struct ModBandCoefs {
    float c[kBandCoefs];
};

// cf: the band's coefficients, wave-uniform (kernel arguments: SGPRs).  tab: row 0 of the device table, indexed by ABSOLUTE step
// (wave-uniform whatever cells the lanes own).  Float k of the band's record goes to out(k, v), after the loop.
template <int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void modulationBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, const ModBandCoefs& cf,
                                               const float* __restrict__ tab) {
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ln.g;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (__ballot(live) == 0ull) {
        if (ln.slot) {
            const float qnan = decayQuietNan();
#pragma unroll
            for (int k = 0; k < kModFloats; ++k) out(k, qnan);
        }
        return;
    }

    const int t0 = live ? (int)delay : 0;
    const int t0l = live ? t0 : INT_MAX;  // (a dead lane never loads)
    int t0min = live ? t0 : INT_MAX, t0max = live ? t0 : INT_MIN;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        t0min = min(t0min, __shfl_xor(t0min, off));
        t0max = max(t0max, __shfl_xor(t0max, off));
    }
    // (wave-uniform by value; said so to the compiler: scalar loop counters, descriptors and table addresses)
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

    float z[4] = {0.f, 0.f, 0.f, 0.f};
    float E = 0.f;
    v2f acc[kModFreqs];  // (re, im) per modulation frequency
#pragma unroll
    for (int i = 0; i < kModFreqs; ++i) acc[i] = v2f{0.f, 0.f};
    const int n = (T - t0min + S - 1) / S;  // chunks from T - 1 down to the wave's smallest onset
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
            // wave-uniform: rows tc .. tc + S - 1, tc > t0min - S >= -S: inside the table and the padding in front of it
            const float* row = tab + (long long)tc * kModRowStride;
#pragma unroll
            for (int k = S - 1; k >= 0; --k) {
                // The step's row offset passes through an empty asm statement together with the lane's sums.  The compiler can then
                // neither issue this step's 28 scalar loads before the step above has finished (left to itself it issues a chunk's
                // 224 at the chunk's top and spills 200 SGPRs to VGPR lanes: measured 2 to 9 % slower, profiles/modulation.txt) nor
                // sink a step's sums below later loads.
                int ro = k * kModRowStride;
                asm volatile(""
                             : "+s"(ro), "+v"(E), "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                               "+v"(acc[6]), "+v"(acc[7]), "+v"(acc[8]), "+v"(acc[9]), "+v"(acc[10]), "+v"(acc[11]), "+v"(acc[12]),
                               "+v"(acc[13]));
                const float* rk = row + ro;
                const bool in = tc + k - t0 >= 0;
                float zn[4] = {z[0], z[1], z[2], z[3]};
                const float y = bandFilterStep(cf.c, p[k], zn);
#pragma unroll
                for (int i = 0; i < 4; ++i) z[i] = in ? zn[i] : z[i];
                const float e = in ? y * y : 0.f;
                E = E + e;
                const v2f ee{e, e};
#pragma unroll
                for (int i = 0; i < kModFreqs; ++i) {
                    const v2f w{rk[2 * i], rk[2 * i + 1]};
                    const v2f m = ee * w;
                    acc[i] = acc[i] + m;
                }
            }
        }
    }
    if (!ln.slot) return;
    float rec[kModFloats];
    if (live) {
        float re[kModFreqs], im[kModFreqs];
#pragma unroll
        for (int i = 0; i < kModFreqs; ++i) {
            re[i] = acc[i].x;
            im[i] = acc[i].y;
        }
        modulationDerive(E, re, im, rec);
    } else {
#pragma unroll
        for (int k = 0; k < kModFloats; ++k) rec[k] = decayQuietNan();
    }
#pragma unroll
    for (int k = 0; k < kModFloats; ++k) out(k, rec[k]);
}

}  // namespace pva
