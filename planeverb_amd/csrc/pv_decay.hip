// pv_decay.hip -- per-cell decay times (EDT, T20, T30: pv_decay.h) of the LAST COMPLETED run, read off the backward-integrated
// (Schroeder) curve of the recorded pressure history.  The one analysis pass that walks the history BACKWARDS in time.
//
// Kept from pv_room_metrics_kernel (pv_metrics.hip), because it is what makes every line of the history be fetched once per
// walk: one lane per cell, the cell being the lane's OFFSET g inside a history plane (pv_analysis.h planeCell), so the 64
// lanes of a wave read 256 contiguous bytes of one plane per load instruction; a ring of NB chunks of S planes of loads in
// flight per wave; a lane outside its own range loading through an out-of-extent buffer offset (the load returns 0 without
// touching memory -- a tile's history is stored only from the launch in which it first became non-zero, so nothing below a
// cell's onset may be read); every 64-cell group of the history window is visited, a wave without a live lane leaves at once,
// and every offset of the plane gets a record: eight quiet NaNs where the cell has no onset in this run.
//
// New here:
//  * Time runs DOWN, wave-uniform, from T - 1 to the smallest onset among the wave's live lanes; chunk c holds the steps
//    [T - (c + 1) S, T - c S) and its samples are consumed from the last to the first.
//  * The steps below a lane's own onset therefore come LAST.  There the load returned 0, e = 0 * 0 = +0.0f, and E + (+0.0f)
//    leaves E's bits alone: E is a sum of squares from +0.0f, never -0.0f, and x + (+0) = x for every other x.  So a lane
//    that has passed its onset holds E(t0) until the wave is done.  Its ratio r then stays 1, which lies inside the EDT
//    range: membership in a range is masked by k = t - t0 >= 0 (and t < tEnd), and a step that is no member changes none of
//    the range's sums (selects, not additions of zero).
//  * E0 = E(t0) is needed before the first ratio, so the curve is walked TWICE with the same loads in the same order and the
//    same additions: E(t0) of the second walk is E0 bit for bit.  The first walk is one multiply and one add per sample.  The
//    second adds the correctly rounded division, the logarithm, six compares and three pairs of double add / multiply.
//  * Skips that cannot change a bit, all wave-uniform: chunks at or after tEnd only advance E; while no lane of the wave has
//    r >= 0.00031622776f at the chunk's earliest step (r never decreases as t does, so none had it earlier in the walk) no step
//    can belong to a range and the division, the logarithm and the fits are skipped -- that is the late part of the record,
//    walked first; r(tEnd - 1), which completeness and depth need, is E(tEnd - 1) / E0 from the kept E.
//  * The logarithm inside the loop is pvLog10fNormalT (bit-identical to pvLog10f on positive normal floats, pv_libm.h) with
//    its table in LDS: a member step has r in [0.00031622776f, 1], and a step that is no member is given 1.0f instead.
//    depth takes the general pvLog10f once per cell (r(tEnd - 1) may be +0).
//
// Both walks live in ONE launch by default; PV_DECAY phase 1 / 2 are the two-launch form (E0 through the record's plane 6),
// kept for the comparison of profiles/decay_times.txt.
// One launch was the faster form on every grid measured (3 .. 8 %).
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, S = 8, NB = 4; the ring holds 32 values, the three fits six
// doubles and nine ints): 94 VGPRs, no AGPRs, scratch size 0 bytes per lane, 768 bytes of LDS, 5 waves per SIMD.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_metrics.hip and
// pv_spectrum.hip and is covered by that parallel only: no test can afford such a plane.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_decay.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"

#ifndef PV_DECAY_S
#define PV_DECAY_S 8  // planes per chunk
#endif
#ifndef PV_DECAY_NB
#define PV_DECAY_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

namespace {

constexpr int kDecayBlock = 256;

// PHASE 0: both walks;  1: the first walk alone, E0 to out plane 6;  2: the second walk alone, E0 from out plane 6.
// CHUNK: a chunk's S planes through ONE descriptor and S scalar offsets (S planes must stay below 2^31 bytes); otherwise one
// descriptor per plane
template <int S, int NB, bool CHUNK, int PHASE>
__global__ __launch_bounds__(kDecayBlock) void pv_decay_times_kernel(const AnalyzeArgs a, float* __restrict__ out, int tailN) {
    __shared__ double tab[96];
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    const int tEnd = T - tailN;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    if (PHASE != 1) {
        fillLogTab(tab, threadIdx.x, kDecayBlock);
        __syncthreads();  // (before any wave leaves)
    }
    const LogTabLds ltab{tab};

    const long long g = ((long long)blockIdx.x * (kDecayBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (PHASE != 2 && g < plane && !live) {
        const float qnan = decayQuietNan();
#pragma unroll
        for (int k = 0; k < kDecayFloats; ++k) out[k * plane + g] = qnan;
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
            if (live) out[6 * plane + g] = E0;
            return;
        }
    } else {
        E0 = live ? out[6 * plane + g] : 0.f;
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
    for (int k = 0; k < kDecayFloats; ++k) out[k * plane + g] = rec[k];
}

template <int PHASE>
void launchDecayPhase(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int tailN = decayTailN((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kDecayBlock - 1) / kDecayBlock));
    if (a.histPlane * 4 * PV_DECAY_S < (1ll << 31))
        hipLaunchKernelGGL((pv_decay_times_kernel<PV_DECAY_S, PV_DECAY_NB, true, PHASE>), grid, dim3(kDecayBlock), 0, stream, a, out, tailN);
    else
        hipLaunchKernelGGL((pv_decay_times_kernel<PV_DECAY_S, PV_DECAY_NB, false, PHASE>), grid, dim3(kDecayBlock), 0, stream, a, out, tailN);
}

}  // namespace

// out: kDecayFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchDecayTimes(const AnalyzeArgs& a, float* out, bool twoLaunches, hipStream_t stream) {
    if (!twoLaunches) return launchDecayPhase<0>(a, out, stream);
    launchDecayPhase<1>(a, out, stream);
    launchDecayPhase<2>(a, out, stream);
}

}  // namespace pva
