// pv_modulation.hip -- per-cell, per-band modulation transfer function and modulation transfer index (pv_modulation.h) of the LAST
// COMPLETED run: each reached cell's recorded pressure is band-pass filtered BACKWARDS in time (pv_bands.h bandFilterStep), and
// the squared output is summed against 14 (cos, sin) pairs per step (the accumulators of pv_spectrum.hip) on the same walk.
//
// The frame is pv_band_metrics_kernel's (pv_bands.hip), kept line for line where it can be: one lane per history-plane offset g,
// time DOWN and wave-uniform from T - 1 to the smallest onset among the wave's live lanes, a ring of NB chunks of S buffer loads
// in flight per wave, out-of-extent offsets that load 0 below a lane's onset, a record of quiet NaNs for every offset without an
// onset, waves without a live lane leaving at once, the per-plane-descriptor form for very large planes, records by plane offset.
//
// New here:
//  * ONE band per launch and ONE walk: the record needs E(t0) only as the divisor of the sums, after the loop.  Per lane: the band's
//    four filter states, E and 14 (re, im) pairs.  The band's ten coefficients arrive as kernel arguments (SGPRs).
//  * The 28 twiddles of a step are the same for all 64 lanes: row t of the table (ABSOLUTE step, so the row address is
//    wave-uniform whatever the lanes' onsets are) is read through a kernel-argument pointer and a scalar step counter, i.e. by
//    scalar loads into SGPRs.  A pair is advanced by one packed multiply and one packed add (v_pk_mul_f32 / v_pk_add_f32 round
//    each half on its own; nothing is fused: -ffp-contract=off).  No lane reads the table, and the device evaluates no
//    trigonometric function.  tab points at row 0; kModTablePad zero rows lie in front of it, for the last chunk of a wave whose
//    smallest onset is below S - 1.
//  * FREEZING.  The steps below a lane's own onset come last (time runs down) and the wave goes on to its smallest onset.  A filter
//    fed zeros rings on, so the four filter states are SELECTED on k = t - t0 >= 0, as in the band kernel, and the e of such a
//    step is replaced by +0.0f.  That is enough for the 29 sums -- the identity argument: E + (+0) = E for every E (E is a sum of
//    squares from +0, never -0).  A twiddle w is finite, so (+0) * w is +0 or -0, and x + (+-0) = x for every x that is not a
//    zero, (+0) + (+-0) = +0 in round-to-nearest; an accumulator is never -0, because a sum is -0 only if both operands are and it
//    started at +0.  So a frozen lane's sums keep their bits without a select per accumulator, and a lane above its onset
//    computes exactly the host restatement's operations in its order.
//  * The records are stored after the loop (the only stores of a live wave), which keeps the table loads provably unclobbered.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, S = 8, NB = 4): profiles/modulation.txt.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_modulation.h"
#include "pv_prims.h"

#ifndef PV_MODULATION_S
#define PV_MODULATION_S 8  // planes per chunk
#endif
#ifndef PV_MODULATION_NB
#define PV_MODULATION_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

namespace {

constexpr int kModBlock = 256;
static_assert(PV_MODULATION_S * PV_MODULATION_NB <= kModTablePad, "the last chunk may begin at step -(S - 1): table rows down to there");

struct ModBandCoefs {
    float c[kBandCoefs];
};

// out: the band's kModFloats planes (float k of the cell at history offset g at out[k * plane + g])
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kModBlock) void pv_modulation_kernel(const AnalyzeArgs a, const ModBandCoefs cf, const float* __restrict__ tab,
                                                                  float* __restrict__ out) {
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kModBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (__ballot(live) == 0ull) {
        if (g < plane) {
            const float qnan = decayQuietNan();
#pragma unroll
            for (int k = 0; k < kModFloats; ++k) out[k * plane + g] = qnan;
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
    if (g >= plane) return;
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
    for (int k = 0; k < kModFloats; ++k) out[k * plane + g] = rec[k];
}

}  // namespace

// coefs: n x kBandCoefs floats on the HOST.  tab: row 0 of the device table (kModTablePad zero rows in front of it, T rows of
// kModRowStride floats).
// out: n x kModFloats planes of a.histPlane floats, float k of band j of the cell at history offset g at
// out[(j * kModFloats + k) * histPlane + g]
void launchModulation(const AnalyzeArgs& a, const float* coefs, int n, const float* tab, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kModBlock - 1) / kModBlock));
    for (int j = 0; j < n; ++j) {
        ModBandCoefs cf;
        for (int k = 0; k < kBandCoefs; ++k) cf.c[k] = coefs[(size_t)j * kBandCoefs + k];
        float* o = out + (size_t)j * kModFloats * (size_t)a.histPlane;
        if (a.histPlane * 4 * PV_MODULATION_S < (1ll << 31))
            hipLaunchKernelGGL((pv_modulation_kernel<PV_MODULATION_S, PV_MODULATION_NB, true>), grid, dim3(kModBlock), 0, stream, a, cf, tab, o);
        else
            hipLaunchKernelGGL((pv_modulation_kernel<PV_MODULATION_S, PV_MODULATION_NB, false>), grid, dim3(kModBlock), 0, stream, a, cf, tab, o);
    }
}

}  // namespace pva
