// pv_lobes_dev.h -- the body of the lobes pass (pv_lobes.hip, which describes it), shared by the whole-map kernel and the in-run query
// kernel (pv_query_records.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_lobes.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_LOBES_S
#define PV_LOBES_S 8  // planes per chunk
#endif
#ifndef PV_LOBES_NB
#define PV_LOBES_NB 2  // chunks of loads in flight per wave (three loads per plane)
#endif

namespace pva {

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void lobesBody(const AnalyzeArgs& a, const DynParams& dyn, const RecordLane& ln, const Store& out, const LobeEdges& ed, int nW) {
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const PlaneCell& pc = ln.pc;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (ln.slot && !live) {
        const float qnan = lobesQuietNan();
        for (int k = 0; k < 1 + 5 * nW; ++k) out(k, qnan);
    }
    if (__ballot(live) == 0ull) return;

    // the neighbours (X - 1, Y) and (X, Y - 1) as plane offsets, and the first recorded step of their tiles: the lane's (pv_record_lane.h)
    const bool hasX = ln.hasX, hasY = ln.hasY;
    const int gX = ln.gX, gY = ln.gY;
    const int tFirst = ln.tFirst, tFx = ln.tFx, tFy = ln.tFy;
    FaceCoef fc{0.f, 0.f, 0.f};
    if (live) {
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

    // the current window of the lane: its sums, the step at which it ends, where it goes: w, the record float of the window's E.
    // The lane flushes at most nW times -- the ends it meets are distinct edges below N, at most nW - 1 of them, and T -- so w
    // stays below wEnd = 1 + 5 nW
    LobeSums s{0.f, 0.f, 0.f, 0.f, 0.f};
    int tNext = live ? onset + lobesWindowEnd(ed, 0, N) : INT_MAX;
    int w = 1;
    const int wEnd = 1 + 5 * nW;
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
                    out(w, s.e);
                    out(w + 1, s.xp);
                    out(w + 2, s.xn);
                    out(w + 3, s.yp);
                    out(w + 4, s.yn);
                    w += 5;
                    s = LobeSums{0.f, 0.f, 0.f, 0.f, 0.f};
                    tNext = onset + lobesWindowEnd(ed, t + 1 - onset, N);
                }
            }
        }
    }
    if (!live) return;
    // (onset >= tBegin >= tLo and T <= tHi: the lane's last window has been written)
    out(0, (float)N);
    for (; w < wEnd; ++w) out(w, 0.f);  // the windows the response does not reach
}

}  // namespace pva
