// pv_arrays.h -- source arrays: the combined response of weighted, delayed emitters at the listener (by reciprocity: of one
// source at a delay-and-sum microphone array).  The definition of include/planeverb_amd.h (Source arrays), shared by the device
// pass (pv_arrays.hip), the solver (pv_solver_arrays.cpp) and the host restatements (PvAmdHostArrayTaps, PvAmdHostArrayResponse).
//
//   setting   nArrays in 1 .. kArraysMax; array a has count[a] members, 1 .. kArrayMembersMax; a member is five floats
//             {x, y, z, gain, delaySeconds} (a negative gain is polarity); interp = kArrayNearest or kArrayLagrange3
//   member    its position maps to a result cell as the output queries' positions do; p_m(t) is what PvAmdCopyHistoryPlane(t)
//             returns at that cell (+0 where nothing was stored, +0 for t < 0), samples below the member's own onset included
//   taps      arrayTaps below: host, double precision
//   response  y_a(t), t = 0 .. T - 1, from +0.0f; over the members in the given order and each member's taps in increasing delay
//                 y = y + (w * p_m(t - delay))                                      (arrayMixStep)
//             float32, every product and every sum rounded on its own, nothing fused, denormals kept
//   onset     the first t with fabsf(y_a(t)) > kArrayOnsetThreshold (NaN compares false), else FLT_MAX  (Analyzer.cpp:146-165)
//   records   PvAmdHost<Kind>(y_a, T, fs, onset_a, ...) of the selected kinds; an array without an onset: quiet NaNs
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>

#include "pv_libm.h"

namespace pva {

constexpr int kArraysMax = 256;        // PVA_ARRAYS_MAX
constexpr int kArrayMembersMax = 64;   // PVA_ARRAY_MEMBERS_MAX
constexpr int kArrayNearest = 0;       // PVA_ARRAY_NEAREST
constexpr int kArrayLagrange3 = 1;     // PVA_ARRAY_LAGRANGE3
constexpr int kArrayMemberFloats = 5;  // x, y, z, gain, delaySeconds
constexpr int kArrayMaxTaps = 4;       // of one member
constexpr float kArrayOnsetThreshold = 0.00000316f;

// one term of a response: `row` = whose samples (on the device: the member's row of the member table), delay in steps, weight
struct ArrayTap {
    int row, delay;
    float w;
    int pad;
};

// The taps of one member: their count (1 or 4) with delays (increasing) and weights written, or -1 with *why set.
//   d = (double)delaySeconds * (double)fs; gain and delaySeconds finite, delaySeconds >= 0, d < T; n = floor(d), mu = d - n
//   NEAREST                one tap {(int)floor(d + 0.5), gain}; a delay that rounds to T is refused
//   LAGRANGE3, mu == 0     one tap {n, gain}
//   LAGRANGE3, mu != 0     n >= 1; four taps at n - 1 .. n + 2 with D = mu + 1.0, each product evaluated left to right in double,
//                          w_j = (float)((double)gain * L_j); taps whose delay is >= T are kept and contribute nothing
inline int arrayTaps(int fs, int T, float gain, float delaySeconds, int interp, int* delay4, float* w4, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    if (interp != kArrayNearest && interp != kArrayLagrange3) return *why = "arrays: interp is PVA_ARRAY_NEAREST or PVA_ARRAY_LAGRANGE3", -1;
    if (fs <= 0 || T <= 0) return *why = "arrays: fs > 0 and T > 0", -1;
    if (!(gain - gain == 0.f)) return *why = "arrays: a gain that is not finite", -1;
    if (!(delaySeconds - delaySeconds == 0.f)) return *why = "arrays: a delay that is not finite", -1;
    if (delaySeconds < 0.f) return *why = "arrays: a negative delay", -1;
    const double d = (double)delaySeconds * (double)fs;
    if (!(d < (double)T)) return *why = "arrays: a delay of T steps or more", -1;
    if (interp == kArrayNearest) {
        const double r = std::floor(d + 0.5);
        if (!(r < (double)T)) return *why = "arrays: a delay that rounds to T steps", -1;
        delay4[0] = (int)r;
        w4[0] = gain;
        return 1;
    }
    const double nf = std::floor(d), mu = d - nf;
    const int n = (int)nf;
    if (mu == 0.0) {
        delay4[0] = n;
        w4[0] = gain;
        return 1;
    }
    if (n < 1) return *why = "arrays: a fractional delay below one step (PVA_ARRAY_LAGRANGE3 reaches one step back)", -1;
    const double D = mu + 1.0;
    const double L[4] = {-(((D - 1.0) * (D - 2.0)) * (D - 3.0)) / 6.0, ((D * (D - 2.0)) * (D - 3.0)) / 2.0,
                         -((D * (D - 1.0)) * (D - 3.0)) / 2.0, ((D * (D - 1.0)) * (D - 2.0)) / 6.0};
    for (int j = 0; j < 4; ++j) {
        delay4[j] = n - 1 + j;
        w4[j] = (float)((double)gain * L[j]);
    }
    return 4;
}

// one term: the product rounded, then the sum rounded (the build keeps contraction off)
PV_HD inline float arrayMixStep(float y, float w, float p) {
    const float m = w * p;
    return y + m;
}

PV_HD inline bool arrayOnsetAt(float y) { return fabsf(y) > kArrayOnsetThreshold; }

// the response of one array from member rows pMT[M][T]: taps in their order (tap.row = the member's row, 0 .. M - 1; the caller
// has checked it), a sample at t - delay outside 0 .. T - 1 is +0.  Returns the onset (FLT_MAX: none)
inline float arrayResponse(const float* pMT, int T, const ArrayTap* taps, int nTaps, float* outT) {
    float onset = FLT_MAX;
    for (int t = 0; t < T; ++t) {
        float y = 0.f;
        for (int k = 0; k < nTaps; ++k) {
            const long long ts = (long long)t - taps[k].delay;
            const float p = ts >= 0 && ts < T ? pMT[(size_t)taps[k].row * T + (size_t)ts] : 0.f;
            y = arrayMixStep(y, taps[k].w, p);
        }
        outT[t] = y;
        if (onset == FLT_MAX && arrayOnsetAt(y)) onset = (float)t;
    }
    return onset;
}

// the counts of a setting; nullptr: fine
inline const char* arraysCountError(const int* count, int nArrays, const float* members5) {
    if (nArrays < 1 || nArrays > kArraysMax) return "arrays: 1 .. 256 arrays (PVA_ARRAYS_MAX)";
    if (!count) return "arrays: null count table";
    if (!members5) return "arrays: null member table";
    for (int a = 0; a < nArrays; ++a)
        if (count[a] < 1 || count[a] > kArrayMembersMax) return "arrays: 1 .. 64 members per array (PVA_ARRAY_MEMBERS_MAX)";
    return nullptr;
}

}  // namespace pva
