// pv_lobes.h -- directional energy lobes (energy of each time window split over the four axial directions +x, -x, +y, -y with
// cos^2 weights) of one impulse response with its particle velocity: the definition of include/planeverb_amd.h
// (PvAmdSetLobeWindows .. PvAmdLobeGains), shared by the device pass (pv_lobes.hip) and the host restatement (PvAmdHostLobes).
// All arithmetic is float32, every product, sum and quotient rounded on its own (-ffp-contract=off), division correctly rounded,
// every window's five sums sequential in increasing t from +0.0f.
//
// Selects.  As pv_echogram.h: the device pass walks wave-uniform time, keeps ONE quintuple of running sums per lane, the current
// window's, and leaves it unchanged by select at a step outside the lane's [onset, T) (lobesStep).  A sum that the definition
// does not touch at a step -- the lobe of the other sign, every lobe when q == 0 -- is left unchanged by select as well, never
// "added +0.0f to": each sum receives exactly the terms the definition gives it, in its order, from +0.0f.
#pragma once

#include <climits>

#include "pv_libm.h"

namespace pva {

constexpr int kLobesMaxEdges = 7;  // PVA_LOBES_MAX_EDGES
constexpr int kLobesMaxWindows = kLobesMaxEdges + 1;
constexpr int kLobesMaxEdgeSteps = 1 << 20;
constexpr float kLobesDefaultEdges[2] = {0.01f, 0.08f};  // direct, early, late

PV_HD inline int lobesFloats(int nWindows) { return 1 + 5 * nWindows; }  // n, then E, XP, XN, YP, YN per window

PV_HD inline float lobesQuietNan() { return pvFloatBits(0x7fc00000u); }

// the window edges in steps, n[i] = (int)(edge_i * (float)fs) (the expression of lateralN5); unused entries are INT_MAX, which
// no step count reaches.  They travel to the kernel by value
struct LobeEdges {
    int n[kLobesMaxEdges];
};

// edges (nEdges of them, 1 .. kLobesMaxEdges) to steps.  False, and *out unspecified, unless every edge is finite (checked on the
// float product, so the conversion to int is defined), n[0] >= 1, every n[i] <= 2^20 and the n[i] are strictly increasing
inline bool lobesEdgeSteps(const float* edges, int nEdges, int fs, LobeEdges* out) {
    if (!edges || nEdges < 1 || nEdges > kLobesMaxEdges) return false;
    for (int i = 0; i < kLobesMaxEdges; ++i) out->n[i] = INT_MAX;
    for (int i = 0; i < nEdges; ++i) {
        const float x = edges[i] * (float)fs;
        if (!(x >= 1.0f && x < (float)(kLobesMaxEdgeSteps + 1))) return false;  // (false for NaN; an infinite edge gives inf or NaN)
        out->n[i] = (int)x;
        if (i > 0 && out->n[i] <= out->n[i - 1]) return false;
    }
    return true;
}

// what a refusal by lobesEdgeSteps says, wherever it is made
constexpr const char* kLobesEdgesError =
    "lobes: 0 .. PVA_LOBES_MAX_EDGES (7) finite edges whose step counts (int)(edge * (float)fs) are 1 .. 2^20 and strictly increasing";

struct LobeSums {
    float e, xp, xn, yp, yn;
};

// one step of the current window by selects: `in` = the step lies in [onset, T)
PV_HD inline void lobesStep(LobeSums& s, bool in, float p, float vx, float vy) {
    const float e = p * p, a = vx * vx, b = vy * vy;
    const float q = a + b;
    const float ex = e * (a / q), ey = e * (b / q);
    const bool dir = in && q > 0.0f;  // (false for a NaN q: such a sample adds to E only)
    const bool px = (vx > 0.0f) == (p > 0.0f), py = (vy > 0.0f) == (p > 0.0f);
    const float e1 = s.e + e, xp1 = s.xp + ex, xn1 = s.xn + ex, yp1 = s.yp + ey, yn1 = s.yn + ey;
    s.e = in ? e1 : s.e;
    s.xp = (dir && px) ? xp1 : s.xp;
    s.xn = (dir && !px) ? xn1 : s.xn;
    s.yp = (dir && py) ? yp1 : s.yp;
    s.yn = (dir && !py) ? yn1 : s.yn;
}

// the step count k' > k at which the window that holds step k of a response of N steps ends: the smallest edge above k, or N
// where there is none below N.  (Edges increase: walking them downwards, the last one taken is the smallest)
PV_HD inline int lobesWindowEnd(const LobeEdges& ed, int k, int N) {
    int r = N;
#pragma unroll
    for (int i = kLobesMaxEdges - 1; i >= 0; --i) r = (ed.n[i] > k && ed.n[i] < N) ? ed.n[i] : r;
    return r;
}

// the definition applied to one impulse response p[T], vx[T], vy[T] with its onset (0 <= onset < T) and nEdges valid edges
// (lobesEdgeSteps), as it is written down; out: lobesFloats(nEdges + 1) floats
inline void lobesOfIr(const float* p, const float* vx, const float* vy, int T, int onset, const LobeEdges& ed, int nEdges, float* out) {
    LobeSums s[kLobesMaxWindows];
    for (int j = 0; j <= nEdges; ++j) s[j] = LobeSums{0.f, 0.f, 0.f, 0.f, 0.f};
    int w = 0;
    for (int t = onset; t < T; ++t) {
        const int k = t - onset;
        while (w < nEdges && k >= ed.n[w]) ++w;
        lobesStep(s[w], true, p[t], vx[t], vy[t]);
    }
    out[0] = (float)(T - onset);
    for (int j = 0; j <= nEdges; ++j) {
        float* o = out + 1 + 5 * j;
        o[0] = s[j].e;
        o[1] = s[j].xp;
        o[2] = s[j].xn;
        o[3] = s[j].yp;
        o[4] = s[j].yn;
    }
}

// PvAmdLobeGains: an emitter's directivity pattern (0 omni, 1 cardioid with a floor of 0.01) applied to one record's windows.
// The sound that travels towards +x at the cell left the emitter towards -x (reciprocity), so the +x lobe is weighted by the
// pattern at -forward.x
PV_HD inline float lobesPattern(int pattern, float d) {
    if (pattern == 0) return 1.0f;
    const float c = (1.0f + d) / 2.0f;
    return c > 0.01f ? c : 0.01f;
}

inline void lobeGainsOfRecord(const float* record, int nWindows, float fwdX, float fwdY, int pattern, float* gains) {
    const float wXP = lobesPattern(pattern, -fwdX), wXN = lobesPattern(pattern, fwdX);
    const float wYP = lobesPattern(pattern, -fwdY), wYN = lobesPattern(pattern, fwdY);
    const float gXP = wXP * wXP, gXN = wXN * wXN, gYP = wYP * wYP, gYN = wYN * wYN;
    for (int w = 0; w < nWindows; ++w) {
        const float* r = record + 1 + 5 * w;
        const float XP = r[1], XN = r[2], YP = r[3], YN = r[4];
        const float num = (((XP * gXP) + (XN * gXN)) + (YP * gYP)) + (YN * gYN);
        const float den = ((XP + XN) + YP) + YN;
        gains[w] = num / den;
    }
}

}  // namespace pva
