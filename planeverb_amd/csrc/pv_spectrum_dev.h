// pv_spectrum_dev.h -- the body of the spectrum pass (pv_spectrum.hip, which describes it), shared by the whole-map kernel and the in-run
// query kernel (pv_query_spectral.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, table rows, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"
#include "pv_record_lane.h"
#include "pv_spectrum.h"

#ifndef PV_SPECTRUM_S
#define PV_SPECTRUM_S 8  // planes per chunk
#endif
#ifndef PV_SPECTRUM_NB
#define PV_SPECTRUM_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

static_assert(PV_SPECTRUM_S <= kSpectrumTablePad, "the last chunk's tail reads table rows up to T - 2 + S");

// One slice of `bins` <= B bins: tab and spow are the slice's table and source powers (wave-uniform; rows by ABSOLUTE step).  Float
// 3 j + {0, 1, 2} = re, im, level of the slice's bin j goes to out(k, v), after the loop.
// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int B, int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void spectrumBody(const AnalyzeArgs& a, const RecordLane& ln, const Store& out, int bins,
                                             const float* __restrict__ tab, const float* __restrict__ spow) {
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ln.g;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (__ballot(live) == 0ull) {
        if (ln.slot) {
            const float qnan = __builtin_nanf("");
            for (int k = 0; k < kSpectrumFloats * bins; ++k) out(k, qnan);
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
    t0min = max(__builtin_amdgcn_readfirstlane(t0min), 0);
    t0max = __builtin_amdgcn_readfirstlane(t0max);
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

    v2f acc[B];  // (re, im) of the pass's bins
#pragma unroll
    for (int j = 0; j < B; ++j) acc[j] = v2f{0.f, 0.f};
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
            const float* row = tab + (long long)tc * (2 * B);  // wave-uniform: rows tc .. tc + S - 1 <= T - 2 + S, inside the padding
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const v2f pp{p[k], p[k]};  // (+0 outside the lane's range)
#pragma unroll
                for (int j = 0; j < B; ++j) {
                    const v2f w{row[k * 2 * B + 2 * j], row[k * 2 * B + 2 * j + 1]};
                    const v2f m = pp * w;
                    acc[j] = acc[j] + m;
                }
            }
        }
    }
    if (!ln.slot) return;
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (j >= bins) continue;  // (the block's padding)
        const float re = acc[j].x, im = acc[j].y;
        out(3 * j + 0, live ? re : qnan);
        out(3 * j + 1, live ? im : qnan);
        out(3 * j + 2, live ? spectrumLevel(re, im, spow[j]) : qnan);
    }
}

}  // namespace pva
