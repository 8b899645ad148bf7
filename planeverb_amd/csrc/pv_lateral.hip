// pv_lateral.hip -- per-cell early lateral energy fraction and early-sound direction (pv_lateral.h) of the LAST COMPLETED run:
// the pass that carries the velocity recurrence of the stencil through the whole 80 ms window of every reached cell at once.
//
// Kept from pv_room_metrics_kernel (pv_metrics.hip): one lane per cell, the cell being the lane's OFFSET g inside a history plane
// (pv_analysis.h planeCell), so the 64 lanes of a wave read 256 contiguous bytes of one plane per load instruction; a ring of NB
// chunks of S planes of buffer loads in flight per wave; a lane outside its own range loading through an out-of-extent buffer
// offset (the load returns 0 without touching memory -- a tile's history is stored only from the launch in which it first became
// non-zero); every 64-cell group of the history window is visited, a wave without a live lane leaves at once, and every offset of
// the plane gets a record: eleven quiet NaNs where the cell has no onset in this run.
//
// New here:
//  * THREE loads per sample: the cell itself and its upstream neighbours (X - 1, Y) and (X, Y - 1), whose offsets are computed as
//    encodeWave (pv_analysis_dev.h) computes them: one row / one cell back inside a tile, into the tile above / to the left
//    across a tile's first row / column.  A neighbour outside the window, or a sample before the neighbour tile's own first
//    recorded step, is exactly zero by causality and is loaded as zero (out-of-extent offset).  The neighbours' lines are the
//    lines other lanes of this or a nearby wave load as their own: the bytes fetched from memory stay those of one read.
//  * vx, vy by the stencil's own recurrence (v_t = v_{t-1} - C (p_t[i] - p_t[n]) on air|air faces, k (p_i + p_n) otherwise,
//    face coefficients read once per lane), from tBegin = max(tileFirst, m - 1), the first sample that can be non-zero (encodeWave):
//    before it the cell's and its neighbours' pressure are zero and an air face's velocity stays +0, so the values from tBegin on
//    are bit for bit those of pv_ir_kernel, which starts at the tile's first recorded sample.
//  * Time is wave-uniform from the smallest tBegin of the wave's live lanes to its largest min(onset + n80, T) -- NOT to T - 1:
//    the first of these passes that reads only a prefix of the history, so its cost does not grow with T.
//  * Membership of the recurrence (t in [tBegin, tEnd)) and of each sum (t in [onset, tEnd), k < n5 or k >= n5) is by select
//    (lateralStep), not by adding products of zero; pv_lateral.h says why that gives the bits of the definition, which adds +0.0f.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see profiles/lateral_fraction.txt; no scratch, no LDS.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_metrics.hip and is
// covered by that parallel only: no test can afford such a plane.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_lateral.h"
#include "pv_launch.h"
#include "pv_prims.h"

#ifndef PV_LATERAL_S
#define PV_LATERAL_S 8  // planes per chunk
#endif
#ifndef PV_LATERAL_NB
#define PV_LATERAL_NB 2  // chunks of loads in flight per wave (three loads per plane)
#endif

namespace pva {

namespace {

constexpr int kLateralBlock = 256;

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kLateralBlock) void pv_lateral_kernel(const AnalyzeArgs a, float* __restrict__ out, int n5, int n80) {
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kLateralBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (g < plane && !live) {
        const float qnan = lateralQuietNan();
#pragma unroll
        for (int k = 0; k < kLateralFloats; ++k) out[k * plane + g] = qnan;
    }
    if (__ballot(live) == 0ull) return;

    // the neighbours (X - 1, Y) and (X, Y - 1) as plane offsets, and the first recorded step of their tiles: encodeWave
    const int tileCells = a.rxi * a.wi;
    const bool hasX = pc.hti > 0 || pc.row > 0, hasY = pc.htj > 0 || pc.col > 0;
    const int gX = pc.row > 0 ? pc.g - a.wi : pc.g - dyn.histTilesY * tileCells + (a.rxi - 1) * a.wi;
    const int gY = pc.col > 0 ? pc.g - 1 : pc.g - tileCells + (a.wi - 1);
    const int tileX = pc.row > 0 ? pc.tile : pc.tile - a.nty, tileY = pc.col > 0 ? pc.tile : pc.tile - 1;
    int tFirst = T, tFx = INT_MAX, tFy = INT_MAX;
    FaceCoef fc{0.f, 0.f, 0.f};
    if (live) {
        tFirst = a.tileFirst[pc.tile];
        if (hasX) tFx = a.tileFirst[tileX];
        if (hasY) tFy = a.tileFirst[tileY];
        fc = a.coef[(size_t)(pc.X + a.G) * a.pitch + (pc.Y + a.G)];
    }
    const float kx = fc.kx, ky = fc.ky;
    const bool airX = kx != kx, airY = ky != ky;
    const float C = a.courant;

    const int onset = live ? (int)delay : 0;
    const int m = abs(pc.X - (dyn.lrow - a.G)) + abs(pc.Y - (dyn.lcol - a.G));
    // a lane's ranges: the recurrence and the own loads over [tBegin, tEnd), a neighbour's loads from its tile's first step on,
    // the sums over [onset, tEnd); a dead lane's are empty
    const int tEnd = live ? min(onset + n80, T) : 0;
    const int tBegin = live ? max(max(tFirst, m - 1), 0) : INT_MAX;
    const int tLoX = (live && hasX) ? max(tBegin, tFx) : INT_MAX, tLoY = (live && hasY) ? max(tBegin, tFy) : INT_MAX;
    // (wave-uniform by value; said so to the compiler by waveMin / waveMax: scalar loop counters and descriptors)
    const int tLo = min(waveMin(tBegin), T), tHi = min(waveMax(tEnd), T);
    const int vo = pc.g * 4, voX = gX * 4, voY = gY * 4;

    float ring[NB][3][S];
    // the 3 S loads of the chunk that begins at step tc >= 0 (issued whatever tc is: the counts are the same on every path)
    auto loadChunk = [&](float (&dst)[3][S], int tc) {
        const int tb = min(tc, T - 1);  // (a chunk past the end: every lane out of range, the base stays inside the history)
        const rsrc_t rs = makeRsrc(a.hist + (long long)tb * plane, CHUNK ? (long long)S * planeBytes : (long long)planeBytes);
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int t = tc + k;
            const bool in = t < tEnd;  // (tEnd <= T)
            const int o = (in && t >= tBegin) ? vo : kOut, oX = (in && t >= tLoX) ? voX : kOut, oY = (in && t >= tLoY) ? voY : kOut;
            const rsrc_t r = CHUNK ? rs : makeRsrc(a.hist + (long long)min(t, T - 1) * plane, planeBytes);
            const int so = CHUNK ? (int)((unsigned)k * (unsigned)planeBytes) : 0;
            dst[0][k] = bufLoadF(r, o, so);
            dst[1][k] = bufLoadF(r, oX, so);
            dst[2][k] = bufLoadF(r, oY, so);
        }
        __builtin_amdgcn_sched_barrier(0);
    };

    LateralSums s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float vx = 0.f, vy = 0.f;
    const int n = (tHi - tLo + S - 1) / S;  // chunks from the wave's smallest tBegin to its largest tEnd
#pragma unroll
    for (int b = 0; b < NB; ++b) loadChunk(ring[b], tLo + b * S);
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int tc = tLo + (c0 + b) * S;
            float p[S], px[S], py[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                p[k] = ring[b][0][k];
                px[k] = ring[b][1][k];
                py[k] = ring[b][2][k];
            }
            loadChunk(ring[b], tc + NB * S);  // the slot's next occupant
            if (tc >= tHi) continue;          // (past the last chunk: those loads returned 0)
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k;
                const bool mineV = t >= tBegin && t < tEnd, mine = t >= onset && t < tEnd;
                const float ax = vx - C * (p[k] - px[k]), wx = kx * (p[k] + px[k]);
                const float ay = vy - C * (p[k] - py[k]), wy = ky * (p[k] + py[k]);
                vx = mineV ? (airX ? ax : wx) : vx;
                vy = mineV ? (airY ? ay : wy) : vy;
                lateralStep(s, mine, t - onset < n5, p[k], vx, vy);
            }
        }
    }
    if (!live) return;
    float rec[kLateralFloats];
    lateralDerive(s, tEnd - onset, rec);
#pragma unroll
    for (int k = 0; k < kLateralFloats; ++k) out[k * plane + g] = rec[k];
}

}  // namespace

// out: kLateralFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchLateralFraction(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int n5 = lateralN5((int)a.fs), n80 = lateralN80((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kLateralBlock - 1) / kLateralBlock));
    if (a.histPlane * 4 * PV_LATERAL_S < (1ll << 31))
        hipLaunchKernelGGL((pv_lateral_kernel<PV_LATERAL_S, PV_LATERAL_NB, true>), grid, dim3(kLateralBlock), 0, stream, a, out, n5, n80);
    else
        hipLaunchKernelGGL((pv_lateral_kernel<PV_LATERAL_S, PV_LATERAL_NB, false>), grid, dim3(kLateralBlock), 0, stream, a, out, n5, n80);
}

}  // namespace pva
