// pv_spectrum.h -- per-cell transfer functions at chosen frequencies: the definition of include/planeverb_amd.h (Spectrum),
// shared by the device pass (pv_spectrum.hip) and the host restatement (PvAmdHostSpectrum / PvAmdHostSpectrumTables).
//
//   bins      n frequencies hz[j], 1 <= n <= kSpectrumMaxBins, each finite and 0 <= hz[j] <= fs / 2; neither sorted nor distinct
//   tables    c[t * n + j] = (float)cos(ph), s[t * n + j] = (float)sin(ph), ph = (2.0 * M_PI * (double)hz[j] * (double)t) / (double)fs,
//             t = 0 .. T - 1: ABSOLUTE run time (phase zero is the start of the run, not the cell's onset), computed on the host
//             in double with the host libm.  The device never evaluates a trigonometric function.
//   sums      re_j = sum_{t = t0}^{T - 1} (p(t) * c[t * n + j]),  im_j = sum_{t = t0}^{T - 1} (p(t) * s[t * n + j]),
//             X(f_j) = re_j - i im_j; samples before the onset t0 do not enter
//   record    re, im, level = 10.0f * log10f(((re * re) + (im * im)) / spow_j)  (dB), spow_j = (sre * sre) + (sim * sim) of the
//             same sums over the run's pulse table with onset 0
// All arithmetic is float32, every product and sum rounded on its own (-ffp-contract=off), every sum sequential in increasing t
// from +0.0f, denormals kept; log10f is glibc's (pv_libm.h, general form).  Nothing is special-cased: spow_j = 0 gives +-inf or
// NaN as IEEE says.
// A level means something only inside the pulse's band (up to about the grid resolution in Hz): above it spow_j is the square of
// rounding noise.  Cells inside an edge layer get records like any other cell, as unphysical there as their other outputs.
#pragma once

#include <cmath>

#include "pv_libm.h"

namespace pva {

constexpr int kSpectrumMaxBins = 32;  // PVA_SPECTRUM_MAX_BINS
constexpr int kSpectrumFloats = 3;    // re, im, level per bin

// the rule of a list of bins with the cap as a parameter (the waterfall, pv_waterfall.h, shares it with a larger one): what is wrong
enum BinsFault { kBinsOk, kBinsCount, kBinsNull, kBinsNotFinite, kBinsNegative, kBinsAboveNyquist };
inline BinsFault spectrumBinsFault(const float* hz, int n, int fs, int cap) {
    if (n < 1 || n > cap) return kBinsCount;
    if (!hz) return kBinsNull;
    for (int j = 0; j < n; ++j) {
        if (!std::isfinite(hz[j])) return kBinsNotFinite;
        if (hz[j] < 0.f) return kBinsNegative;
        if ((double)hz[j] > 0.5 * (double)fs) return kBinsAboveNyquist;
    }
    return kBinsOk;
}

// the rule PvAmdSetSpectrumBins and the host calls share; nullptr: fine, else what is wrong
inline const char* spectrumBinsError(const float* hz, int n, int fs) {
    switch (spectrumBinsFault(hz, n, fs, kSpectrumMaxBins)) {
        case kBinsCount: return "spectrum: 1 .. 32 bins (PVA_SPECTRUM_MAX_BINS)";
        case kBinsNull: return "spectrum: null frequency list";
        case kBinsNotFinite: return "spectrum: a frequency that is not finite";
        case kBinsNegative: return "spectrum: a negative frequency";
        case kBinsAboveNyquist: return "spectrum: a frequency above fs / 2";
        default: return nullptr;
    }
}

inline void spectrumTables(int T, int fs, const float* hz, int n, float* c, float* s) {
    for (int t = 0; t < T; ++t)
        for (int j = 0; j < n; ++j) {
            const double ph = (2.0 * M_PI * (double)hz[j] * (double)t) / (double)fs;
            c[(size_t)t * n + j] = (float)std::cos(ph);
            s[(size_t)t * n + j] = (float)std::sin(ph);
        }
}

// one sample of the definition: what p = p(t) adds to a bin's two sums, c and s the bin's table values at the same step t.  The
// walk below and the in-run accumulate pass of sparse-emitter mode (pv_zone_maps.hip) are both this text
PV_HD inline void spectrumStep(float p, float c, float s, float& re, float& im) {
    const float pc = p * c;
    const float ps = p * s;
    re = re + pc;
    im = im + ps;
}

// the two sums of bin j over p[onset .. T - 1]
inline void spectrumSums(const float* p, int T, int onset, const float* c, const float* s, int n, int j, float* re, float* im) {
    float r = 0.f, i = 0.f;
    for (int t = onset; t < T; ++t) spectrumStep(p[t], c[(size_t)t * n + j], s[(size_t)t * n + j], r, i);
    *re = r;
    *im = i;
}

// The sums of all n bins carried over the steps [max(tA, onset), min(tB, T)) of one accumulate pass [tA, tB) -- reim2n = re, im of
// bin j at 2 j, 2 j + 1: a cell whose onset lies in the pass (onset >= tA) starts from +0.0f and never reads them
inline void spectrumAdvance(const float* p, int T, int onset, int tA, int tB, const float* c, const float* s, int n, float* reim2n) {
    const int tEnd = tB < T ? tB : T;
    if (onset < 0 || onset >= tEnd) return;
    for (int j = 0; j < n; ++j) {
        float r = onset >= tA ? 0.f : reim2n[2 * j], i = onset >= tA ? 0.f : reim2n[2 * j + 1];
        for (int t = onset > tA ? onset : tA; t < tEnd; ++t) spectrumStep(p[t], c[(size_t)t * n + j], s[(size_t)t * n + j], r, i);
        reim2n[2 * j] = r;
        reim2n[2 * j + 1] = i;
    }
}

PV_HD inline float spectrumPower(float re, float im) { return (re * re) + (im * im); }
PV_HD inline float spectrumLevel(float re, float im, float spow) { return 10.0f * pvLog10f(spectrumPower(re, im) / spow); }

// sre, sim, spow of every bin from the pulse table (onset 0)
inline void spectrumSource(const float* pulse, int T, const float* c, const float* s, int n, float* out3n) {
    for (int j = 0; j < n; ++j) {
        float re, im;
        spectrumSums(pulse, T, 0, c, s, n, j, &re, &im);
        out3n[3 * j] = re;
        out3n[3 * j + 1] = im;
        out3n[3 * j + 2] = spectrumPower(re, im);
    }
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T)
inline void spectrumOfIr(const float* p, int T, int onset, const float* c, const float* s, int n, const float* source3n, float* out3n) {
    for (int j = 0; j < n; ++j) {
        float re, im;
        spectrumSums(p, T, onset, c, s, n, j, &re, &im);
        out3n[3 * j] = re;
        out3n[3 * j + 1] = im;
        out3n[3 * j + 2] = spectrumLevel(re, im, source3n[3 * j + 2]);
    }
}

}  // namespace pva
