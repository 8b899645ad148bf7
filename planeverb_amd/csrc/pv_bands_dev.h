// pv_bands_dev.h -- the body of the band-metrics pass (pv_bands.hip, which describes it), shared by the whole-map kernel and the in-run
// query kernel (pv_query_spectral.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, filters, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_bands.h"
#include "pv_device.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_BANDS_S
#define PV_BANDS_S 8  // planes per chunk
#endif
#ifndef PV_BANDS_NB
#define PV_BANDS_NB 4  // chunks of loads in flight per wave
#endif
#ifndef PV_BANDS_B
#define PV_BANDS_B 2  // bands per launch
#endif

namespace pva {

template <int B>
struct BandBlockCoefs {
    float c[B][kBandCoefs];
};

// cf: the block's coefficient sets, wave-uniform (kernel arguments: SGPRs).  nb <= B: the bands of this block that are real; float
// k of band j of the block goes to out(j * kBandFloats + k, v).
// ltab: the logarithm's table in LDS (fillLogTab and a barrier, by the caller)
template <int S, int NB, bool CHUNK, int B, class Store>
__device__ __forceinline__ void bandMetricsBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, const BandBlockCoefs<B>& cf,
                                                int nb, const LogTabLds& ltab, int tailN, int n50, int n80) {
    const int T = a.T;
    const int tEnd = T - tailN;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ln.g;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (ln.slot && !live) {
        const float qnan = decayQuietNan();
        for (int j = 0; j < nb; ++j)
#pragma unroll
            for (int k = 0; k < kBandFloats; ++k) out(j * kBandFloats + k, qnan);
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

    // one filter step of band j on a lane that is `in` its range; every other lane keeps its state.  Returns e = y * y
    auto filt = [&](int j, float x, bool in, float (&z)[4]) {
        float zn[4] = {z[0], z[1], z[2], z[3]};
        const float y = bandFilterStep(cf.c[j], x, zn);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = in ? zn[i] : z[i];
        return y * y;
    };

    const int n = (T - t0min + S - 1) / S;  // chunks from T - 1 down to the wave's smallest onset
    float E0[B];
    {
        // ---- first walk: E(t0) and the clarity sums
        float z[B][4], E[B], e50[B], e80[B], l50[B], l80[B], mom[B];
#pragma unroll
        for (int j = 0; j < B; ++j) {
            z[j][0] = z[j][1] = z[j][2] = z[j][3] = 0.f;
            E[j] = e50[j] = e80[j] = l50[j] = l80[j] = mom[j] = 0.f;
        }
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
                    const int kk = tc + k - t0;
                    const bool in = kk >= 0;
                    const float fk = (float)kk;
#pragma unroll
                    for (int j = 0; j < B; ++j) {
                        const float e = filt(j, p[k], in, z[j]);
                        const float En = E[j] + e, e50n = e50[j] + e, e80n = e80[j] + e;
                        const float m = fk * e;
                        const float momn = mom[j] + m;
                        E[j] = in ? En : E[j];
                        l50[j] = kk == n50 ? En : l50[j];
                        l80[j] = kk == n80 ? En : l80[j];
                        e50[j] = (in && kk < n50) ? e50n : e50[j];
                        e80[j] = (in && kk < n80) ? e80n : e80[j];
                        mom[j] = in ? momn : mom[j];
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < B; ++j) {
            E0[j] = E[j];
            if (live && j < nb) {
                float c4[4];
                bandClarityDerive(e50[j], l50[j], e80[j], l80[j], mom[j], E0[j], (int)a.fs, c4);
#pragma unroll
                for (int k = 0; k < 4; ++k) out(j * kBandFloats + kDecayFloats + k, c4[k]);
            }
        }
    }

    // ---- second walk: the same filter and the same sums again, and the fits
    DecayFit f[B][kDecayRanges];
    float z[B][4], E[B], eEnd[B];
    bool deep[B];  // wave-uniform: some lane has reached r >= kDecayLoAll in band j
#pragma unroll
    for (int j = 0; j < B; ++j) {
#pragma unroll
        for (int q = 0; q < kDecayRanges; ++q) f[j][q] = DecayFit{0., 0., 0, 0, 0};
        z[j][0] = z[j][1] = z[j][2] = z[j][3] = 0.f;
        E[j] = eEnd[j] = 0.f;
        deep[j] = false;
    }
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
            float Es[B][S];
#pragma unroll
            for (int k = S - 1; k >= 0; --k) {
                const bool in = tc + k - t0 >= 0;
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const float e = filt(j, p[k], in, z[j]);
                    const float En = E[j] + e;
                    E[j] = in ? En : E[j];
                    Es[j][k] = E[j];
                }
            }
            if (tc >= tEnd) continue;  // the tail: filter and E alone
            if (tc + S >= tEnd) {      // (the chunk that holds step tEnd - 1)
#pragma unroll
                for (int j = 0; j < B; ++j)
#pragma unroll
                    for (int k = 0; k < S; ++k) eEnd[j] = (tc + k == tEnd - 1) ? Es[j][k] : eEnd[j];
            }
#pragma unroll
            for (int j = 0; j < B; ++j) {
                if (!deep[j]) {
                    deep[j] = __ballot((Es[j][0] / E0[j]) >= kDecayLoAll) != 0ull;  // (E0 = 0: the ratio is NaN)
                    if (!deep[j]) continue;
                }
#pragma unroll
                for (int k = S - 1; k >= 0; --k) {
                    const int t = tc + k, kk = t - t0;
                    const float r = Es[j][k] / E0[j];
                    const bool own = kk >= 0 && t < tEnd && r >= kDecayLoAll && r <= 1.0f;
                    const float L = 10.0f * pvLog10fNormalT(own ? r : 1.0f, ltab);
#pragma unroll
                    for (int q = 0; q < kDecayRanges; ++q) decayFitStep(f[j][q], own && decayInRange(q, r), kk, L);
                }
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (j >= nb) continue;
        float rec[kDecayFloats];
        decayDerive(f[j], E0[j], eEnd[j] / E0[j], t0 < tEnd, (int)a.fs, rec);
#pragma unroll
        for (int k = 0; k < kDecayFloats; ++k) out(j * kBandFloats + k, rec[k]);
    }
}

}  // namespace pva
