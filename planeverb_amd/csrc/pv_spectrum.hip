// pv_spectrum.hip -- per-cell transfer functions at chosen frequencies (pv_spectrum.h) of the LAST COMPLETED run: the forward pass
// of pv_metrics.hip over the recorded pressure history with another loop body.
//
// Kept from pv_room_metrics_kernel, because it is what makes every line of the history be fetched exactly once: one lane per
// OFFSET g inside a history plane (pv_analysis.h planeCell), wave-uniform time from the smallest onset among the wave's live lanes
// to T - 1, a ring of NB chunks of S planes of buffer loads in flight per wave, a lane outside its own range loading through an
// out-of-extent buffer offset (the load returns 0 without touching memory: nothing below a cell's onset may be read), NaN records
// for the offsets without an onset, and a wave without a live lane leaving at once.
//
// The identity argument for this body.  The definition sums p(t) * w over t = t0 .. T - 1 from +0.0f; the lane sums over the
// WAVE's range and feeds p = +0.0f outside its own.  A twiddle w is finite (a rounded cosine or sine, or the table's zero padding),
// so the extra product is +0 * w = +0 or, for a negative twiddle, -0.  Adding either to a running sum leaves its bits unchanged:
// x + (+-0) = x for every x that is not a zero, (+0) + (+0) = +0, and (+0) + (-0) = +0 in round-to-nearest.  The remaining case,
// (-0) + (+-0), never arises: a sum is -0 only if both of its operands are, so one that started at +0 can never become -0 --
// neither here nor in the definition, which starts at +0 as well.  The steps below a lane's onset come first, while its sums are
// still +0; the steps past T - 1 (the last chunk's tail: the table rows there are zero) come last and add +0.
//
// New here:
//   twiddles   the 2 B twiddles of a step are the same for all 64 lanes: row t of the pass's table, {cos, sin} pairs, is read
//              through a wave-uniform address (kernel-argument pointer, scalar step counter), i.e. by scalar loads into SGPRs,
//              and every multiply takes its twiddle from there.  No lane reads the table, and the device evaluates no
//              trigonometric function.
//   bins       B bins per pass are register-blocked: 2 B accumulators per lane, as B (re, im) pairs.  A pair is advanced by one
//              packed multiply and one packed add (v_pk_mul_f32 / v_pk_add_f32 round each half on its own); nothing is fused
//              (-ffp-contract=off).  2 B multiply-adds per history sample against one load: the pass's time goes with the bins,
//              not with the history bytes -- docs/experiments/spectrum.md has the measured times.
//   n > B      the host (Solver::computeSpectrum) runs one pass per slice of the bins, each with its own table slice.
// The records are stored after the loop (the only stores of the kernel), which keeps the table loads provably unclobbered.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"
#include "pv_spectrum.h"

#ifndef PV_SPECTRUM_S
#define PV_SPECTRUM_S 8  // planes per chunk
#endif
#ifndef PV_SPECTRUM_NB
#define PV_SPECTRUM_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

namespace {

constexpr int kSpectrumThreads = 256;
static_assert(PV_SPECTRUM_S <= kSpectrumTablePad, "the last chunk's tail reads table rows up to T - 2 + S");

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int B, int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kSpectrumThreads) void pv_spectrum_kernel(const AnalyzeArgs a, int bins, const float* __restrict__ tab,
                                                                      const float* __restrict__ spow, float* __restrict__ out) {
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kSpectrumThreads / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (__ballot(live) == 0ull) {
        if (g < plane) {
            const float qnan = __builtin_nanf("");
            for (int k = 0; k < kSpectrumFloats * bins; ++k) out[k * plane + g] = qnan;
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
    if (g >= plane) return;
    const float qnan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < B; ++j) {
        if (j >= bins) continue;  // (the block's padding)
        const float re = acc[j].x, im = acc[j].y;
        out[(3 * j + 0) * plane + g] = live ? re : qnan;
        out[(3 * j + 1) * plane + g] = live ? im : qnan;
        out[(3 * j + 2) * plane + g] = live ? spectrumLevel(re, im, spow[j]) : qnan;
    }
}

template <int B>
void launchSpectrumB(const AnalyzeArgs& a, int bins, const float* tab, const float* spow, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kSpectrumThreads - 1) / kSpectrumThreads));
    if (a.histPlane * 4 * PV_SPECTRUM_S < (1ll << 31))
        hipLaunchKernelGGL((pv_spectrum_kernel<B, PV_SPECTRUM_S, PV_SPECTRUM_NB, true>), grid, dim3(kSpectrumThreads), 0, stream, a, bins, tab, spow, out);
    else
        hipLaunchKernelGGL((pv_spectrum_kernel<B, PV_SPECTRUM_S, PV_SPECTRUM_NB, false>), grid, dim3(kSpectrumThreads), 0, stream, a, bins, tab, spow, out);
}

}  // namespace

// B = 32 was built and timed as well (136 VGPRs) and never won: docs/experiments/spectrum.md
bool spectrumBlockOk(int block) { return block == 8 || block == 16; }

void launchSpectrum(const AnalyzeArgs& a, int block, int bins, const float* tab, const float* spow, float* out, hipStream_t stream) {
    if (block == 8)
        launchSpectrumB<8>(a, bins, tab, spow, out, stream);
    else
        launchSpectrumB<16>(a, bins, tab, spow, out, stream);
}

}  // namespace pva
