// pv_waterfall.h -- per-receiver waterfalls (cumulative spectral decay): the definition of include/planeverb_amd.h (Waterfall),
// shared by the device pass (pv_waterfall.hip) and the host restatement (PvAmdHostWaterfall).
//
//   bins      n frequencies hz[j], 1 <= n <= kWaterfallMaxBins, each finite and 0 <= hz[j] <= fs / 2; neither sorted nor distinct
//             (the rule of the spectrum's bins, pv_spectrum.h spectrumBinsFault, with the larger cap)
//   slices    m of them, 1 <= m <= kWaterfallMaxSlices; slice k starts k * ns steps after the receiver's onset,
//             ns = (int)(sliceSeconds * (float)fs) in float32 (the echogram's expression), sliceSeconds finite, 1 <= ns <= 2^20
//   tables    the spectrum's (spectrumTables): absolute run time, host libm in double
//   source    spow_j by spectrumSource
//   record    F = 2 + 2 n + m n floats of one receiver with onset t0 and samples p(t):
//                 re_j = im_j = +0.0f
//                 for t = T - 1 down to t0:          (DECREASING t: one backward walk gives every slice)
//                     spectrumStep(p(t), c[t * n + j], s[t * n + j], re_j, im_j)
//                     if t == t0 + k * ns for a k in 0 .. m - 1:  R[k][j] = re_j, I[k][j] = im_j
//                 slices that start at or past T keep R = I = +0.0f
//             [0] (float)t0, [1] (float) the count of slices with t0 + k * ns < T, R[0][0 .. n), I[0][0 .. n),
//             level[k][j] = spectrumLevel(R[k][j], I[k][j], spow_j), slice-major
// X_k(f_j) = R[k][j] - i I[k][j] is the transform of the response with its first k * ns steps after the onset removed.  Float32
// throughout, nothing fused, denormals kept, nothing special-cased (an empty slice: 10 log10f(0 / spow) = -inf).  Slice 0 is the
// spectrum's sum in the opposite order: equal in exact arithmetic, not bit for bit.
#pragma once

#include <cmath>
#include <cstddef>

#include "pv_libm.h"
#include "pv_spectrum.h"

namespace pva {

constexpr int kWaterfallMaxBins = 512;       // PVA_WATERFALL_MAX_BINS
constexpr int kWaterfallMaxSlices = 64;      // PVA_WATERFALL_MAX_SLICES
constexpr int kWaterfallMaxReceivers = 256;  // PVA_WATERFALL_MAX_RECEIVERS
constexpr int kWaterfallMaxSliceSteps = 1 << 20;

// record layout: where the parts of a record of n bins and m slices start
constexpr int kWaterfallHead = 2;  // onset, slice count
PV_HD inline int waterfallFloats(int n, int m) { return kWaterfallHead + 2 * n + m * n; }
PV_HD inline int waterfallReOff(int) { return kWaterfallHead; }
PV_HD inline int waterfallImOff(int n) { return kWaterfallHead + n; }
PV_HD inline int waterfallLevelOff(int n, int k) { return kWaterfallHead + 2 * n + k * n; }

// steps per slice: the echogram's expression.  Call only with waterfallSliceOk(sliceSeconds, fs)
PV_HD inline int waterfallSliceSteps(float sliceSeconds, int fs) { return (int)(sliceSeconds * (float)fs); }
// sliceSeconds finite and 1 <= ns <= 2^20 (checked on the float product: the conversion to int is then defined)
PV_HD inline bool waterfallSliceOk(float sliceSeconds, int fs) {
    const float x = sliceSeconds * (float)fs;
    return x >= 1.0f && x < (float)(kWaterfallMaxSliceSteps + 1);  // (false for NaN; an infinite sliceSeconds gives inf or NaN)
}

// the slices that start inside the run: those with onset + k * ns < T, k < m (0 <= onset < T: at least one)
PV_HD inline int waterfallSliceCount(int T, int onset, int ns, int m) {
    const int k = (T - 1 - onset) / ns + 1;
    return k < m ? k : m;
}

// the rule PvAmdSetWaterfall and PvAmdHostWaterfall share; nullptr: fine, else what is wrong
inline const char* waterfallSettingError(const float* hz, int n, int fs, float sliceSeconds, int nSlices) {
    switch (spectrumBinsFault(hz, n, fs, kWaterfallMaxBins)) {
        case kBinsCount: return "waterfall: 1 .. 512 bins (PVA_WATERFALL_MAX_BINS)";
        case kBinsNull: return "waterfall: null frequency list";
        case kBinsNotFinite: return "waterfall: a frequency that is not finite";
        case kBinsNegative: return "waterfall: a negative frequency";
        case kBinsAboveNyquist: return "waterfall: a frequency above fs / 2";
        default: break;
    }
    if (nSlices < 1 || nSlices > kWaterfallMaxSlices) return "waterfall: 1 .. 64 slices (PVA_WATERFALL_MAX_SLICES)";
    if (!waterfallSliceOk(sliceSeconds, fs)) return "waterfall: a slice of 1 .. 2^20 steps ((int)(sliceSeconds * (float)fs))";
    return nullptr;
}

inline float waterfallQuietNan() { return pvFloatBits(0x7fc00000u); }

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T): c, s the tables [T * n], source3n the
// triples of spectrumSource, out the record of waterfallFloats(n, m) floats
inline void waterfallOfIr(const float* p, int T, int onset, const float* c, const float* s, int n, int ns, int m, const float* source3n,
                          float* out) {
    out[0] = (float)onset;
    out[1] = (float)waterfallSliceCount(T, onset, ns, m);
    for (int j = 0; j < n; ++j) {
        const float spow = source3n[3 * j + 2];
        // (the slices that start at or past T: R = I = +0.0f; the walk below overwrites the others)
        for (int k = 0; k < m; ++k) out[waterfallLevelOff(n, k) + j] = spectrumLevel(0.f, 0.f, spow);
        float re = 0.f, im = 0.f;
        int k = waterfallSliceCount(T, onset, ns, m) - 1;  // the next boundary down the walk: t = onset + k * ns
        for (int t = T - 1; t >= onset; --t) {
            spectrumStep(p[t], c[(size_t)t * n + j], s[(size_t)t * n + j], re, im);
            if (k >= 0 && t == onset + k * ns) {
                out[waterfallLevelOff(n, k) + j] = spectrumLevel(re, im, spow);
                if (k == 0) {
                    out[waterfallReOff(n) + j] = re;
                    out[waterfallImOff(n) + j] = im;
                }
                --k;
            }
        }
    }
}

}  // namespace pva
