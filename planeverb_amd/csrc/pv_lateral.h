// pv_lateral.h -- early lateral energy fraction (LF, ISO 3382-1 A.2) and early-sound direction of one impulse response with its
// particle velocity: the definition of include/planeverb_amd.h (PvAmdLateralFraction), shared by the device pass (pv_lateral.hip)
// and the host restatement (PvAmdHostLateralFraction).  All arithmetic is float32, every product, sum and quotient rounded on its
// own (-ffp-contract=off), every sum sequential in increasing t from +0.0f.
//
// The three second moments sxx, sxy, syy make the lateral energy a quadratic form in the direction, so the direction (known only
// after the first 5 ms) does not have to be known while the window is walked.
//
// Selects and additions of zero.  The definition adds +0.0f where a step is no member of a sum; the device pass selects instead
// (lateralStep), also for the steps outside [onset, tEnd) that its wave-uniform time visits.  Both give the same bits although
// the flux and sxy are signed sums: a sum that starts at +0.0f is never -0.0f (x + y is -0.0f only if both are, and an exact
// cancellation gives +0.0f in round-to-nearest), and s + (+0.0f) == s bit for bit for every s other than -0.0f -- finite, infinite
// or NaN.  The non-negative-sum argument of the room metrics is the special case in which no term is negative.
#pragma once

#include <cmath>

#include "pv_libm.h"

namespace pva {

constexpr int kLateralFloats = 11;  // lf, dir_x, dir_y, n, e80, lateral, fx, fy, sxx, sxy, syy

PV_HD inline int lateralN5(int fs) { return (int)(0.005f * (float)fs); }
PV_HD inline int lateralN80(int fs) { return (int)(0.08f * (float)fs); }

PV_HD inline float lateralQuietNan() { return pvFloatBits(0x7fc00000u); }

struct LateralSums {
    float e80, fx, fy, sxx, sxy, syy;
};

// one step of the window by selects: `in` = the step lies in [onset, tEnd), early = k < n5
PV_HD inline void lateralStep(LateralSums& s, bool in, bool early, float p, float vx, float vy) {
    const float e = p * p, px = p * vx, py = p * vy;
    const float xx = vx * vx, xy = vx * vy, yy = vy * vy;
    const float e80 = s.e80 + e, fx = s.fx + px, fy = s.fy + py;
    const float sxx = s.sxx + xx, sxy = s.sxy + xy, syy = s.syy + yy;
    const bool fl = in && early, mo = in && !early;
    s.e80 = in ? e80 : s.e80;
    s.fx = fl ? fx : s.fx;
    s.fy = fl ? fy : s.fy;
    s.sxx = mo ? sxx : s.sxx;
    s.sxy = mo ? sxy : s.sxy;
    s.syy = mo ? syy : s.syy;
}

// the record from the six sums and n = tEnd - onset; nothing is special-cased (a zero flux gives NaN for dx, dy, lf)
PV_HD inline void lateralDerive(const LateralSums& s, int n, float out[kLateralFloats]) {
    const float norm = sqrtf((s.fx * s.fx) + (s.fy * s.fy));
    const float dx = s.fx / norm, dy = s.fy / norm;
    const float lat = ((s.sxx * (dy * dy)) - (2.0f * (s.sxy * (dx * dy)))) + (s.syy * (dx * dx));
    out[0] = lat / s.e80;
    out[1] = dx;
    out[2] = dy;
    out[3] = (float)n;
    out[4] = s.e80;
    out[5] = lat;
    out[6] = s.fx;
    out[7] = s.fy;
    out[8] = s.sxx;
    out[9] = s.sxy;
    out[10] = s.syy;
}

// the definition applied to one impulse response p[T], vx[T], vy[T] with its onset (0 <= onset < T), as it is written down:
// a step that is no member of a sum adds +0.0f
inline void lateralFractionOfIr(const float* p, const float* vx, const float* vy, int T, int fs, int onset, float out[kLateralFloats]) {
    const int n5 = lateralN5(fs), n80 = lateralN80(fs);
    const int tEnd = onset + n80 < T ? onset + n80 : T;
    LateralSums s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = onset; t < tEnd; ++t) {
        const int k = t - onset;
        s.e80 = s.e80 + (p[t] * p[t]);
        s.fx = s.fx + (k < n5 ? p[t] * vx[t] : 0.f);
        s.fy = s.fy + (k < n5 ? p[t] * vy[t] : 0.f);
        s.sxx = s.sxx + (k >= n5 ? vx[t] * vx[t] : 0.f);
        s.sxy = s.sxy + (k >= n5 ? vx[t] * vy[t] : 0.f);
        s.syy = s.syy + (k >= n5 ? vy[t] * vy[t] : 0.f);
    }
    lateralDerive(s, tEnd - onset, out);
}

}  // namespace pva
