// pv_decay.h -- decay times of one impulse response (EDT, T20, T30 read off the backward-integrated Schroeder curve): the
// definition of include/planeverb_amd.h (PvAmdDecayTimes), shared by the device pass (pv_decay.hip) and the host restatement
// (PvAmdHostDecayTimes).  The curve E, the ratio r and the level L are float32, the two regression sums of a range and its
// derive step are double; every product, sum and quotient is rounded on its own (-ffp-contract=off), every sum is sequential in
// DECREASING t from +0.0; log10f is glibc's (pv_libm.h, general form: the argument may be +0 or NaN).
#pragma once

#include "pv_libm.h"

namespace pva {

constexpr int kDecayFloats = 8;  // edt, t20, t30, n_edt, n_t20, n_t30, e0, depth
constexpr int kDecayRanges = 3;  // EDT 0 .. -10 dB, T20 -5 .. -25 dB, T30 -5 .. -35 dB, as ratios of E(t0)
constexpr float kDecayHi[kDecayRanges] = {1.0f, 0.31622776f, 0.31622776f};
constexpr float kDecayLo[kDecayRanges] = {0.1f, 0.0031622776f, 0.00031622776f};
constexpr float kDecayLoAll = 0.00031622776f;  // the smallest lower limit: below it a step belongs to no range

// the curve's last 10 ms enter no fit (the reference's PV_SCHROEDER_OFFSET_S rule)
PV_HD inline int decayTailN(int fs) { return (int)(0.01f * (float)fs); }

PV_HD inline float decayQuietNan() { return pvFloatBits(0x7fc00000u); }

// one range's regression state; its steps arrive in DECREASING t, so the first one has the largest k
struct DecayFit {
    double sy, sky;
    int n, kmin, kmax;
};

PV_HD inline bool decayInRange(int j, float r) { return r <= kDecayHi[j] && r >= kDecayLo[j]; }

// step k = t - t0 with level L = 10.0f * log10f(r) joins the range iff `in`
PV_HD inline void decayFitStep(DecayFit& f, bool in, int k, float L) {
    const double y = (double)L;
    const double ky = (double)k * y;  // (exact: 24 x 24 bits)
    const double sy = f.sy + y, sky = f.sky + ky;
    f.sy = in ? sy : f.sy;
    f.sky = in ? sky : f.sky;
    f.kmax = (in && f.n == 0) ? k : f.kmax;
    f.kmin = in ? k : f.kmin;
    f.n = in ? f.n + 1 : f.n;
}

// seconds for 60 dB from a range's sums; nothing is special-cased beyond completeness and n >= 2 (slope >= 0 gives -inf or a
// negative value)
PV_HD inline float decayFitValue(const DecayFit& f, bool complete, int fs) {
    if (!complete || f.n < 2) return decayQuietNan();
    const double n = (double)f.n;
    const double kbar = ((double)f.kmin + (double)f.kmax) * 0.5;
    const double slope = (f.sky - (kbar * f.sy)) / ((n * ((n * n) - 1.0)) / 12.0);
    return (float)((-60.0 / slope) / (double)fs);
}

// the record from the three fits, E0 = E(t0) and rEnd = r(tEnd - 1) (ignored where the onset lies in the tail: t0 >= tEnd)
PV_HD inline void decayDerive(const DecayFit (&f)[kDecayRanges], float e0, float rEnd, bool beforeTail, int fs, float out[kDecayFloats]) {
    for (int j = 0; j < kDecayRanges; ++j) {
        out[j] = decayFitValue(f[j], beforeTail && rEnd < kDecayLo[j], fs);
        out[3 + j] = (float)f[j].n;
    }
    out[6] = e0;
    out[7] = beforeTail ? 10.0f * pvLog10f(rEnd) : decayQuietNan();
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T)
inline void decayTimesOfIr(const float* p, int T, int fs, int onset, float out[kDecayFloats]) {
    const int tEnd = T - decayTailN(fs);
    float E = 0.f;
    for (int t = T - 1; t >= onset; --t) {
        const float e = p[t] * p[t];
        E = E + e;
    }
    const float e0 = E;
    DecayFit f[kDecayRanges] = {{0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}};
    float rEnd = 0.f;
    E = 0.f;
    for (int t = T - 1; t >= onset; --t) {
        const float e = p[t] * p[t];
        E = E + e;
        if (t >= tEnd) continue;
        const float r = E / e0;
        if (t == tEnd - 1) rEnd = r;
        const float L = 10.0f * pvLog10f(r);
        for (int j = 0; j < kDecayRanges; ++j) decayFitStep(f[j], decayInRange(j, r), t - onset, L);
    }
    decayDerive(f, e0, rEnd, onset < tEnd, fs, out);
}

}  // namespace pva
