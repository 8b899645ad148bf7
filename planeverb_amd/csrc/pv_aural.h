// pv_aural.h -- auralisation: a recorded response resampled from the grid's rate fs to an audio rate and convolved with dry
// signals.  The definition of include/planeverb_amd.h (Auralisation), shared by the device passes (pv_aural.hip), the solver
// (pv_solver_aural.cpp) and the host restatements (PvAmdHostAuralTaps, PvAmdHostAuralResample, PvAmdHostAuralConvolve).
//
//   setting   rate in 1000 .. 384000, zeroCrossings Z in 2 .. 64, beta finite in 0 .. 20 (the Kaiser window's parameter)
//   tables    auralTaps below: host, double precision, a Kaiser-windowed sinc whose cutoff is the lower of the two Nyquist rates;
//             output sample n reads the K source steps first[n] .. first[n] + K - 1 with the weights w[n][0 .. K)
//   response  h_r[n], n = 0 .. L - 1, from +0.0f; for j = 0 .. K - 1 ascending
//                 h = h + (w[n][j] * p_r(first[n] + j))                              (auralStep), p_r = +0.0f outside 0 .. T - 1
//   output    o_r[m], m = 0 .. N + L - 2, from +0.0f; for k = max(0, m - N + 1) .. min(L - 1, m) ascending
//                 o = o + (h_r[k] * x[m - k])                                        (auralStep); no other term is formed
//   mix       mix[m] from +0.0f; over the routed receivers in increasing r:  mix = mix + (gain[r] * o_r[m])   (auralStep)
// float32, every product and every sum rounded on its own, nothing fused, denormals kept; NaN and inf propagate as IEEE says.
#pragma once

#include <cmath>
#include <cstddef>

#include "pv_libm.h"

namespace pva {

constexpr int kAuralMinRate = 1000;
constexpr int kAuralMaxRate = 384000;
constexpr int kAuralMinCrossings = 2;
constexpr int kAuralMaxCrossings = 64;
constexpr int kAuralMaxTaps = 1024;                 // PVA_AURAL_MAX_TAPS
constexpr int kAuralMaxReceivers = 256;             // PVA_AURAL_MAX_RECEIVERS
constexpr int kAuralMaxSignals = 64;                // PVA_AURAL_MAX_SIGNALS
constexpr int kAuralMaxSignalSamples = 1 << 20;     // PVA_AURAL_MAX_SAMPLES
constexpr long long kAuralMaxTableFloats = 1 << 24; // L * K
constexpr long long kAuralMaxOutputFloats = 1 << 26; // R * M
constexpr int kAuralReceivers = 0;                  // PVA_AURAL_RECEIVERS
constexpr int kAuralArrays = 1;                     // PVA_AURAL_ARRAYS
constexpr int kAuralTiled = 0;                      // PVA_AURAL_TILED
constexpr int kAuralPlain = 1;                      // PVA_AURAL_PLAIN
constexpr double kAuralPi = 3.14159265358979323846; // M_PI

// the modified Bessel function of order zero as the tables take it: 60 terms of the power series, in double
inline double auralI0(double x) {
    double s = 1.0, term = 1.0;
    const double h = 0.5 * x;
    for (int k = 1; k <= 60; ++k) {
        term = term * ((h / k) * (h / k));
        s = s + term;
    }
    return s;
}

// the rule PvAmdSetAuralisation and PvAmdHostAuralTaps share: nullptr with *L and *K written, else what is wrong
inline const char* auralShape(unsigned fs, int T, int rate, int Z, float beta, int* L, int* K) {
    if (fs < 1u || T < 1) return "aural: fs > 0 and T > 0";
    if (rate < kAuralMinRate || rate > kAuralMaxRate) return "aural: a rate of 1000 .. 384000 samples per second";
    if (Z < kAuralMinCrossings || Z > kAuralMaxCrossings) return "aural: 2 .. 64 zero crossings";
    if (!(beta - beta == 0.f) || beta < 0.f || beta > 20.f) return "aural: a finite beta of 0 .. 20";
    const double c = (double)rate < (double)fs ? (double)rate / (double)fs : 1.0;
    const double half = (double)Z / c;
    const double fk = 2.0 * std::floor(half) + 1.0;
    if (fk > (double)kAuralMaxTaps) return "aural: more than 1024 taps per sample (PVA_AURAL_MAX_TAPS): 2 floor(Z fs / rate) + 1";
    const double fl = std::floor(((double)(T - 1) * (double)rate) / (double)fs) + 1.0;
    if (fl * fk > (double)kAuralMaxTableFloats) return "aural: a table of more than 2^24 weights (L * K)";
    *K = (int)fk;
    *L = (int)fl;
    return nullptr;
}

// the tables of a checked setting: first[L], w[L * K] row-major
inline void auralTaps(unsigned fs, int rate, int Z, float beta, int L, int K, int* first, float* w) {
    const double c = (double)rate < (double)fs ? (double)rate / (double)fs : 1.0;
    const double half = (double)Z / c;
    const double i0b = auralI0((double)beta);
    for (int n = 0; n < L; ++n) {
        const double u = ((double)n * (double)fs) / (double)rate;
        const int f = (int)std::ceil(u - half);
        first[n] = f;
        for (int j = 0; j < K; ++j) {
            const int t = f + j;
            const double d = u - (double)t;
            float v = 0.0f;
            if (!(std::fabs(d) > half)) {
                const double a = c * d;
                const double sinc = (a == 0.0) ? 1.0 : std::sin(kAuralPi * a) / (kAuralPi * a);
                double q = d / half;
                q = 1.0 - q * q;
                if (q < 0.0) q = 0.0;
                v = (float)((c * sinc) * (auralI0((double)beta * std::sqrt(q)) / i0b));
            }
            w[(size_t)n * K + j] = v;
        }
    }
}

// one term of a response, an output or the mix: the product rounded, then the sum rounded (the build keeps contraction off)
PV_HD inline float auralStep(float acc, float a, float b) {
    const float m = a * b;
    return acc + m;
}

// the first and last tap of output m: k = auralTapLo .. auralTapHi (L >= 1, N >= 1, 0 <= m <= N + L - 2: never empty)
PV_HD inline int auralTapLo(int m, int N) { return m - N + 1 > 0 ? m - N + 1 : 0; }
PV_HD inline int auralTapHi(int m, int L) { return m < L - 1 ? m : L - 1; }

inline void auralResample(const float* p, int T, const int* first, const float* w, int L, int K, float* outL) {
    for (int n = 0; n < L; ++n) {
        float h = 0.f;
        for (int j = 0; j < K; ++j) {
            const long long t = (long long)first[n] + j;
            h = auralStep(h, w[(size_t)n * K + j], t >= 0 && t < T ? p[t] : 0.f);
        }
        outL[n] = h;
    }
}

inline void auralConvolve(const float* h, int L, const float* x, int N, float* outM) {
    const int M = N + L - 1;
    for (int m = 0; m < M; ++m) {
        float o = 0.f;
        for (int k = auralTapLo(m, N), k1 = auralTapHi(m, L); k <= k1; ++k) o = auralStep(o, h[k], x[m - k]);
        outM[m] = o;
    }
}

}  // namespace pva
