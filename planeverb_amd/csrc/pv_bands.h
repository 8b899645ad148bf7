// pv_bands.h -- octave / third-octave band filters and the per-band record of one impulse response (decay times and clarity of
// the band-filtered response): the definition of include/planeverb_amd.h (PvAmdBandMetrics), shared by the device pass
// (pv_bands.hip) and the host restatements (PvAmdHostBandCoefs, PvAmdHostBandMetrics).
//
//   design    on the host, in double: the order-2 Butterworth low-pass prototype (poles exp(+-i 3 pi / 4)), the LP -> BP transform
//             s -> (s^2 + W1 W2) / ((W2 - W1) s) with the pre-warped edges W = tan(pi f / fs), the bilinear transform
//             z = (1 + s) / (1 - s).  Two biquads, the one whose pole angle is smaller first, each with zeros at z = +1 and
//             z = -1 (b = g (1, 0, -1)) and g chosen for unit gain at the pre-warped geometric centre w0 = 2 atan(sqrt(W1 W2)).
//             Every coefficient rounded to float32 once: b0, b1, b2, a1, a2 per section, 10 floats per band.
//   filter    float32, transposed direct form II, BACKWARDS in time from t = T - 1 (state +0.0f) down to the onset t0; every
//             product and sum rounded on its own (-ffp-contract=off), denormals kept; section 2 takes section 1's y.
//   record    12 floats: the eight of pv_decay.h with e(t) = y(t) * y(t), then c50, c80, d50, ts from sums taken in DECREASING t.
#pragma once

#include <cmath>
#include <complex>

#include "pv_decay.h"
#include "pv_metrics.h"

namespace pva {

constexpr int kBandsMax = 8;        // PVA_BANDS_MAX
constexpr int kBandCoefs = 10;      // b0, b1, b2, a1, a2 of section 1, then of section 2
constexpr int kBandFloats = 12;     // edt, t20, t30, n_edt, n_t20, n_t30, e0, depth, c50, c80, d50, ts

// one biquad step (c: b0, b1, b2, a1, a2); returns y
PV_HD inline float bandSectionStep(const float* c, float x, float& z1, float& z2) {
    const float y = (c[0] * x) + z1;
    const float n1 = ((c[1] * x) - (c[3] * y)) + z2;
    const float n2 = (c[2] * x) - (c[4] * y);
    z1 = n1;
    z2 = n2;
    return y;
}

// the band's two sections in series; z: z1, z2 of section 1, then of section 2
PV_HD inline float bandFilterStep(const float* c10, float x, float (&z)[4]) {
    const float y1 = bandSectionStep(c10, x, z[0], z[1]);
    return bandSectionStep(c10 + 5, y1, z[2], z[3]);
}

// the last four floats from the sums of the first walk
PV_HD inline void bandClarityDerive(float e50, float l50, float e80, float l80, float moment, float e0, int fs, float out4[4]) {
    out4[0] = 10.0f * pvLog10f(e50 / l50);
    out4[1] = 10.0f * pvLog10f(e80 / l80);
    out4[2] = e50 / (e50 + l50);
    out4[3] = (moment / e0) / (float)fs;
}

// the rule PvAmdSetBands and PvAmdHostBandCoefs share (n >= 1); nullptr: fine, else what is wrong
inline const char* bandsError(const float* centreHz, int n, int fraction, int fs) {
    if (n < 1 || n > kBandsMax) return "band metrics: 0 .. 8 bands (PVA_BANDS_MAX)";
    if (fraction != 1 && fraction != 3) return "band metrics: fraction is 1 (octave) or 3 (third octave)";
    if (!centreHz) return "band metrics: null centre list";
    if (fs <= 0) return "band metrics: fs > 0";
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(centreHz[j])) return "band metrics: a centre that is not finite";
        const double half = 1.0 / (2.0 * (double)fraction);
        const double f1 = (double)centreHz[j] * std::exp2(-half), f2 = (double)centreHz[j] * std::exp2(half);
        if (!(f1 > 0.0)) return "band metrics: a band whose lower edge is not above 0";
        if (!(f2 < 0.5 * (double)fs)) return "band metrics: a band whose upper edge is not below fs / 2";
    }
    return nullptr;
}

// the ten float32 coefficients of one band (bandsError has passed)
inline void bandDesign(double fs, double fc, int fraction, float out10[kBandCoefs]) {
    typedef std::complex<double> cd;
    const double half = 1.0 / (2.0 * (double)fraction);
    const double f1 = fc * std::exp2(-half), f2 = fc * std::exp2(half);
    const double W1 = std::tan(M_PI * f1 / fs), W2 = std::tan(M_PI * f2 / fs);
    const double bw = W2 - W1, w0sq = W1 * W2;
    const cd p(-std::sqrt(0.5), std::sqrt(0.5));  // the prototype's pole of positive imaginary part; the other is its conjugate
    const cd pb = p * bw;
    const cd root = std::sqrt((pb * pb) - (4.0 * w0sq));
    const cd s[2] = {(pb + root) * 0.5, (pb - root) * 0.5};  // one analog pole of each conjugate pair
    cd zp[2];
    for (int k = 0; k < 2; ++k) zp[k] = (1.0 + s[k]) / (1.0 - s[k]);
    if (std::fabs(std::arg(zp[1])) < std::fabs(std::arg(zp[0]))) std::swap(zp[0], zp[1]);
    const double w0 = 2.0 * std::atan(std::sqrt(w0sq));
    const cd zi = std::polar(1.0, -w0);  // z^-1 at the centre
    for (int k = 0; k < 2; ++k) {
        const double a1 = -2.0 * zp[k].real(), a2 = std::norm(zp[k]);
        const double g = std::abs((1.0 + (a1 * zi) + (a2 * zi * zi)) / (1.0 - (zi * zi)));
        out10[5 * k + 0] = (float)g;
        out10[5 * k + 1] = 0.0f;
        out10[5 * k + 2] = (float)(-g);
        out10[5 * k + 3] = (float)a1;
        out10[5 * k + 4] = (float)a2;
    }
}

inline void bandCoefs(int fs, const float* centreHz, int n, int fraction, float* out10n) {
    for (int j = 0; j < n; ++j) bandDesign((double)fs, (double)centreHz[j], fraction, out10n + (size_t)kBandCoefs * j);
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T) and one band's coefficients
inline void bandMetricsOfIr(const float* p, int T, int fs, int onset, const float* c10, float out[kBandFloats]) {
    const int tEnd = T - decayTailN(fs);
    const int n50 = roomMetricsN50(fs), n80 = roomMetricsN80(fs);
    // first walk: E0 and the clarity sums
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    float E = 0.f, e50 = 0.f, e80 = 0.f, l50 = 0.f, l80 = 0.f, moment = 0.f;
    for (int t = T - 1; t >= onset; --t) {
        const int k = t - onset;
        const float y = bandFilterStep(c10, p[t], z);
        const float e = y * y;
        E = E + e;
        if (k == n50) l50 = E;  // E(t0 + n50); +0.0f where t0 + n50 >= T
        if (k == n80) l80 = E;
        if (k < n50) e50 = e50 + e;
        if (k < n80) e80 = e80 + e;
        const float m = (float)k * e;
        moment = moment + m;
    }
    const float e0 = E;
    // second walk: the same filter and the same sums again, and the fits of pv_decay.h
    DecayFit f[kDecayRanges] = {{0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}};
    float rEnd = 0.f;
    E = 0.f;
    for (int k = 0; k < 4; ++k) z[k] = 0.f;
    for (int t = T - 1; t >= onset; --t) {
        const float y = bandFilterStep(c10, p[t], z);
        const float e = y * y;
        E = E + e;
        if (t >= tEnd) continue;
        const float r = E / e0;
        if (t == tEnd - 1) rEnd = r;
        const float L = 10.0f * pvLog10f(r);
        for (int j = 0; j < kDecayRanges; ++j) decayFitStep(f[j], decayInRange(j, r), t - onset, L);
    }
    decayDerive(f, e0, rEnd, onset < tEnd, fs, out);
    bandClarityDerive(e50, l50, e80, l80, moment, e0, fs, out + kDecayFloats);
}

}  // namespace pva
