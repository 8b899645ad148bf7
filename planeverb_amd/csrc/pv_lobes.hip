// pv_lobes.hip -- per-cell directional energy lobes (pv_lobes.h) of the LAST COMPLETED run: the energy p^2 of every reached cell
// per time window after its onset, and that energy split over the four axial travel directions +x, -x, +y, -y by the squared
// direction cosines of the particle velocity, opposite directions kept apart.
//
// The frame is pv_echogram_kernel's (pv_echogram.hip), which see: one lane per cell, the cell being the lane's OFFSET g inside a
// history plane; THREE buffer loads per sample (the cell and its upstream neighbours (X - 1, Y) and (X, Y - 1), across tile
// edges as encodeWave computes them); an out-of-extent offset for everything that is zero by causality (the load returns 0
// without touching memory); a ring of NB chunks of S planes of loads in flight per wave with a sched_barrier behind each chunk's
// loads; face coefficients read once per lane; vx, vy by the stencil's own recurrence from tBegin = max(tileFirst, m - 1); time
// wave-uniform from the wave's smallest tBegin on; the CHUNK / !CHUNK descriptor forms; a wave without a live lane leaves after
// writing its NaNs; every float of the storage written by the one launch, no memset pass; 64-bit addressing of the record planes.
//
// Different here:
//  * The walk goes to T - 1: the last window is open-ended, so the cost is three loads per sample over the whole response, not
//    over a short window.
//  * Windows of unequal lengths.  Per lane: tNext, the step at which the lane's current window ends (onset + the smallest edge
//    above the current step count, or T), and w, the address of the current window's E plane.  At t + 1 == tNext the lane stores
//    its five sums, resets them to +0.0f and finds the next end by a chain of selects over the (at most 7) edges, which are
//    kernel arguments: no division per sample, no window index that could index a register array.
//  * Two correctly rounded divisions per sample (a / q, b / q).
//  * A live lane also writes n = (float)(T - onset) and five +0.0f into each window past its last one, a dead lane 1 + 5 nW quiet
//    NaNs.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see profiles/lobes.txt; no scratch, no LDS.
// The per-plane-descriptor form (!CHUNK: a plane of 2^31 / S bytes and more) is line for line the one of pv_lateral.hip and is
// covered by that parallel only: no test can afford such a plane.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_lobes.h"
#include "pv_prims.h"

#ifndef PV_LOBES_S
#define PV_LOBES_S 8  // planes per chunk
#endif
#ifndef PV_LOBES_NB
#define PV_LOBES_NB 2  // chunks of loads in flight per wave (three loads per plane)
#endif

namespace pva {

namespace {

constexpr int kLobesBlock = 256;

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kLobesBlock) void pv_lobes_kernel(const AnalyzeArgs a, float* __restrict__ out, const LobeEdges ed, int nW) {
    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kLobesBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (g < plane && !live) {
        const float qnan = lobesQuietNan();
        float* q = out + g;
        for (int k = 0; k < 1 + 5 * nW; ++k, q += plane) *q = qnan;
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

    // (a reached cell's onset is a step of the run; the clamp keeps a live lane's stores inside its planes whatever the map holds)
    const int onset = live ? min(max((int)delay, 0), T - 1) : 0;
    const int N = T - onset;  // the steps of the lane's response
    const int m = abs(pc.X - (dyn.lrow - a.G)) + abs(pc.Y - (dyn.lcol - a.G));
    // a lane's ranges: the recurrence and the own loads over [tBegin, tEnd), a neighbour's loads from its tile's first step on,
    // the sums over [onset, tEnd); a dead lane's are empty
    const int tEnd = live ? T : 0;
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

    // the current window of the lane: its sums, the step at which it ends, where it goes.  Live lanes: g < plane, and the lane
    // flushes at most nW times -- the ends it meets are distinct edges below N, at most nW - 1 of them, and T -- so w stays inside
    // plane 5 nW
    LobeSums s{0.f, 0.f, 0.f, 0.f, 0.f};
    int tNext = live ? onset + lobesWindowEnd(ed, 0, N) : INT_MAX;
    float* w = out + plane + (live ? g : 0);
    float* const wEnd = out + (1 + 5 * (long long)nW) * plane + (live ? g : 0);
    float vx = 0.f, vy = 0.f;
    const int n = (tHi - tLo + S - 1) / S;  // chunks from the wave's smallest tBegin to T
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
                lobesStep(s, mine, p[k], vx, vy);
                if (mine && t + 1 == tNext && w < wEnd) {  // the window ends here, at an edge or at T (w < wEnd: by the count above)
                    w[0] = s.e;
                    w[plane] = s.xp;
                    w[2 * plane] = s.xn;
                    w[3 * plane] = s.yp;
                    w[4 * plane] = s.yn;
                    w += 5 * plane;
                    s = LobeSums{0.f, 0.f, 0.f, 0.f, 0.f};
                    tNext = onset + lobesWindowEnd(ed, t + 1 - onset, N);
                }
            }
        }
    }
    if (!live) return;
    // (onset >= tBegin >= tLo and T <= tHi: the lane's last window has been written)
    out[g] = (float)N;
    for (; w < wEnd; w += plane) *w = 0.f;  // the windows the response does not reach
}

}  // namespace

// out: 1 + 5 nW planes of a.histPlane floats, float k of the cell at history offset g at out[k * histPlane + g]
void launchLobes(const AnalyzeArgs& a, float* out, const LobeEdges& ed, int nW, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kLobesBlock - 1) / kLobesBlock));
    if (a.histPlane * 4 * PV_LOBES_S < (1ll << 31))
        hipLaunchKernelGGL((pv_lobes_kernel<PV_LOBES_S, PV_LOBES_NB, true>), grid, dim3(kLobesBlock), 0, stream, a, out, ed, nW);
    else
        hipLaunchKernelGGL((pv_lobes_kernel<PV_LOBES_S, PV_LOBES_NB, false>), grid, dim3(kLobesBlock), 0, stream, a, out, ed, nW);
}

}  // namespace pva
