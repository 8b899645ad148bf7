// pv_modulation.h -- per-cell, per-band modulation transfer function (MTF) and modulation transfer index (MTI) of one impulse
// response, after Schroeder 1981 and the indirect method of IEC 60268-16: the definition of include/planeverb_amd.h
// (PvAmdModulation), shared by the device pass (pv_modulation.hip) and the host restatements (PvAmdHostModulation,
// PvAmdHostModulationTable, PvAmdCombineMti).
//
//   bands     the bands of pv_bands.h: the same ten float32 coefficients, the same two sections, the same backward walk from
//             t = T - 1 (state +0.0f) down to the onset t0; y(t) is bandFilterStep's output and e(t) = y(t) * y(t)
//   table     M = 14 modulation frequencies F[i]; row t (ABSOLUTE step, t = 0 .. T - 1) holds the 14 pairs
//             {(float)cos(ph), (float)sin(ph)}, ph = (2.0 * M_PI * (double)F[i] * (double)t) / (double)fs, in double with the host
//             libm: 28 floats per row.  The device evaluates no trigonometric function
//   sums      in DECREASING t from +0.0f, every product and sum rounded on its own (-ffp-contract=off), denormals kept:
//                 E += e;   re[i] += e * cos[t][i];   im[i] += e * sin[t][i]
//   record    a = re[i] / E,  b = im[i] / E,  m[i] = sqrtf((a * a) + (b * b))           (the ratios first: re^2 + im^2 of a faint
//                                                                                        cell would underflow)
//             snr[i] = m[i] >= 1.0f ? 15.0f : clamp(10.0f * pvLog10f(m[i] / (1.0f - m[i])))
//                      clamp(v) = v < -15.0f ? -15.0f : (v > 15.0f ? 15.0f : v)          (a NaN stays a NaN)
//             ti[i]  = (snr[i] + 15.0f) / 30.0f
//             mti    = (((ti[0] + ti[1]) + ...) + ti[13], sequential from +0.0f) / 14.0f
//             15 floats: m[0 .. 13], mti.  E == 0: 15 quiet NaNs.  Nothing else is special-cased
#pragma once

#include <cmath>
#include <cstddef>

#include "pv_bands.h"
#include "pv_decay.h"
#include "pv_libm.h"

namespace pva {

constexpr int kModFreqs = 14;                   // PVA_MODULATION_FREQS
constexpr int kModFloats = kModFreqs + 1;       // m[0 .. 13], mti
constexpr int kModRowFloats = 2 * kModFreqs;    // {cos, sin} pairs of one step
constexpr int kModRowStride = 32;               // floats from row to row of the DEVICE table (128-byte rows; the last four are zero)
// zero rows in front of row 0 of the DEVICE table: the walk's last chunk may begin below step 0 (by less than a chunk; the pad
// covers a whole ring of chunks)
constexpr int kModTablePad = 64;

// the IEC 60268-16 third-octave series of modulation frequencies
constexpr float kModDefaultHz[kModFreqs] = {0.63f, 0.8f, 1.0f, 1.25f, 1.6f, 2.0f, 2.5f, 3.15f, 4.0f, 5.0f, 6.3f, 8.0f, 10.0f, 12.5f};

// the rule PvAmdSetModulationFrequencies and the host calls share (hz: 14 values); nullptr: fine, else what is wrong
inline const char* modulationFreqsError(const float* hz14, int fs) {
    if (fs <= 0) return "modulation: fs > 0";
    for (int i = 0; i < kModFreqs; ++i) {
        if (!std::isfinite(hz14[i])) return "modulation: a modulation frequency that is not finite";
        if (hz14[i] < 0.f) return "modulation: a negative modulation frequency";
        if ((double)hz14[i] > 0.5 * (double)fs) return "modulation: a modulation frequency above fs / 2";
    }
    return nullptr;
}

// rows 0 .. T - 1, kModRowFloats floats each
inline void modulationTable(int T, int fs, const float* hz14, float* out28T) {
    for (int t = 0; t < T; ++t)
        for (int i = 0; i < kModFreqs; ++i) {
            const double ph = (2.0 * M_PI * (double)hz14[i] * (double)t) / (double)fs;
            out28T[(size_t)t * kModRowFloats + 2 * i] = (float)std::cos(ph);
            out28T[(size_t)t * kModRowFloats + 2 * i + 1] = (float)std::sin(ph);
        }
}

PV_HD inline float modulationTi(float m) {
    float snr = 15.0f;
    if (!(m >= 1.0f)) {
        const float v = 10.0f * pvLog10f(m / (1.0f - m));
        snr = v < -15.0f ? -15.0f : (v > 15.0f ? 15.0f : v);
    }
    return (snr + 15.0f) / 30.0f;
}

// the record from the sums of the walk; re / im: element i of each
PV_HD inline void modulationDerive(float E, const float* re, const float* im, float out[kModFloats]) {
    if (E == 0.f) {
        for (int i = 0; i < kModFloats; ++i) out[i] = decayQuietNan();
        return;
    }
    float sum = 0.f;
    for (int i = 0; i < kModFreqs; ++i) {
        const float a = re[i] / E;
        const float b = im[i] / E;
        const float m = sqrtf((a * a) + (b * b));
        out[i] = m;
        sum = sum + modulationTi(m);
    }
    out[kModFreqs] = sum / 14.0f;
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T), one band's coefficients and the table
inline void modulationOfIr(const float* p, int T, int onset, const float* c10, const float* tab28T, float out[kModFloats]) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    float E = 0.f, re[kModFreqs], im[kModFreqs];
    for (int i = 0; i < kModFreqs; ++i) re[i] = im[i] = 0.f;
    for (int t = T - 1; t >= onset; --t) {
        const float y = bandFilterStep(c10, p[t], z);
        const float e = y * y;
        const float* row = tab28T + (size_t)t * kModRowFloats;
        E = E + e;
        for (int i = 0; i < kModFreqs; ++i) {
            const float ec = e * row[2 * i];
            const float es = e * row[2 * i + 1];
            re[i] = re[i] + ec;
            im[i] = im[i] + es;
        }
    }
    modulationDerive(E, re, im, out);
}

// sum of alpha[k] mti[k] minus sum of beta[k] sqrtf(mti[k] mti[k + 1]), float32, sequential, clamped to [0, 1] (a NaN stays)
inline float combineMti(const float* mti, const float* alpha, const float* beta, int n) {
    float s = 0.f;
    for (int k = 0; k < n; ++k) {
        const float w = alpha[k] * mti[k];
        s = s + w;
    }
    float r = 0.f;
    for (int k = 0; k + 1 < n; ++k) {
        const float q = beta[k] * sqrtf(mti[k] * mti[k + 1]);
        r = r + q;
    }
    const float v = s - r;
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

}  // namespace pva
