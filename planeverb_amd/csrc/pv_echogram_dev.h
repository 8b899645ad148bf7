// pv_echogram_dev.h -- the body of the echogram pass (pv_echogram.hip, which describes it), shared by the whole-map kernel and the in-run query
// kernel (pv_query_records.hip): which cell the lane owns and where its record goes come from the caller (pv_record_lane.h),
// everything else -- loads, ring, sums, order -- is this one text.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_echogram.h"
#include "pv_prims.h"
#include "pv_record_lane.h"

#ifndef PV_ECHOGRAM_S
#define PV_ECHOGRAM_S 8  // planes per chunk
#endif
#ifndef PV_ECHOGRAM_NB
#define PV_ECHOGRAM_NB 2  // chunks of loads in flight per wave (three loads per plane)
#endif

namespace pva {

// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int S, int NB, bool CHUNK, class Store>
__device__ __forceinline__ void echogramBody(const AnalyzeArgs& a, const DynParams& dyn, const RecordLane& ln, const Store& out, int ns, int nSlots) {
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const PlaneCell& pc = ln.pc;
    const float delay = ln.delay;
    const bool live = ln.live;
    if (ln.slot && !live) {
        const float qnan = echogramQuietNan();
        for (int k = 0; k < 1 + 3 * nSlots; ++k) out(k, qnan);
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

    const int onset = live ? (int)delay : 0;
    const int m = abs(pc.X - (dyn.lrow - a.G)) + abs(pc.Y - (dyn.lcol - a.G));
    // a lane's ranges: the recurrence and the own loads over [tBegin, tEnd), a neighbour's loads from its tile's first step on,
    // the sums over [onset, tEnd); a dead lane's are empty.  (ns * nSlots <= 2^25, onset < T: no overflow)
    const int tEnd = live ? min(onset + ns * nSlots, T) : 0;
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

    // the current slot of the lane: its sums, the step at which it ends, where it goes: w, the record float of the slot's e (the
    // lane flushes at most nSlots times -- once per ns steps of [onset, tEnd), tEnd - onset <= ns nSlots -- so w stays below 1 + 3 nSlots)
    EchogramSums s{0.f, 0.f, 0.f};
    int tNext = live ? min(onset + ns, tEnd) : INT_MAX;
    int w = 1;
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
                echogramStep(s, mine, p[k], vx, vy);
                if (mine && t + 1 == tNext) {  // the slot ends here, by its length or by tEnd
                    out(w, s.e);
                    out(w + 1, s.ix);
                    out(w + 2, s.iy);
                    w += 3;
                    s = EchogramSums{0.f, 0.f, 0.f};
                    tNext = min(tNext + ns, tEnd);
                }
            }
        }
    }
    if (!live) return;
    // (onset >= tBegin >= tLo and tEnd <= tHi: the lane's last slot has been written)
    out(0, (float)(tEnd - onset));
    for (; w < 1 + 3 * nSlots; ++w) out(w, 0.f);  // the slots the record does not reach
}

}  // namespace pva
