// pv_bands.hip -- per-cell, per-band decay times and clarity (pv_bands.h) of the LAST COMPLETED run: each reached cell's recorded
// pressure is band-pass filtered BACKWARDS in time (two float32 biquads per band) and the filtered energy goes through the
// decay-times definition of pv_decay.h and the clarity formulas of pv_metrics.h.
//
// The frame is pv_decay_times_kernel's (pv_decay.hip), kept line for line where it can be: one lane per history-plane offset g,
// time DOWN and wave-uniform from T - 1 to the smallest onset among the wave's live lanes, a ring of NB chunks of S buffer loads
// in flight per wave, out-of-extent offsets that load 0 below a lane's onset, a record of quiet NaNs for every offset without an
// onset, waves without a live lane leaving at once, the per-plane-descriptor form for very large planes, records by plane offset.
//
// New here:
//  * Bands are register-blocked, B to a launch (PV_BANDS_B); a launch re-reads the history for its block, as the spectrum pass
//    does for its bins.  The last block is padded with all-zero coefficient sets: their y is +-0, their E +0, and their records
//    are not stored.
//  * The coefficients are wave-uniform: they arrive as kernel arguments (BandBlockCoefs by value), so they sit in SGPRs and the
//    multiplies take them as scalar operands.
//  * Two walks in ONE launch.  The first filters, sums E per band and takes the clarity sums (e50, e80, the two values of the curve
//    l50 / l80, the moment) on the way; c50, c80, d50 and ts are derived and stored at its end, so none of that state lives through
//    the second walk.  The second walk repeats the same loads in the same order and the same filter arithmetic from the same +0
//    state, so its E(t0) is E0 bit for bit, and adds the ratio, the logarithm and the three fits.
//  * FREEZING.  The steps below a lane's own onset come last (time runs down) and the wave goes on to its smallest onset.  The
//    decay pass may let such a lane run on: its input is 0, and E + (+0) = E.  A filter is another matter: with input 0 its state
//    goes on ringing (z1 <- (-a1 y) + z2, ...), so y != 0 and E would grow.  Every piece of a lane's state -- the four filter
//    states of a band, E, the clarity sums, the fits -- is therefore SELECTED on k = t - t0 >= 0: a step below the onset computes
//    values and throws them away.  A lane above its onset computes exactly the host restatement's operations in its order.
//  * The decay pass's wave-uniform skips carry over per band: chunks at or after tEnd only filter and advance E; while no lane has
//    r >= 0.00031622776f at the chunk's earliest step there is neither division nor logarithm nor fit.  The filter is never
//    skipped: its state is needed at every step.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, S = 8, NB = 4): profiles/band_metrics.txt.
//
// The text of the pass is bandMetricsBody (pv_bands_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that
// fills the logarithm's table and gives the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher;
// pv_query_spectral.hip runs the same body for the cells of a run's queries.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_bands.h"
#include "pv_bands_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kBandsBlock = 256;

// nb <= B: the bands of this block that are real (their records are stored to out, band j at out + j * kBandFloats * plane)
template <int S, int NB, bool CHUNK, int B>
__global__ __launch_bounds__(kBandsBlock) void pv_band_metrics_kernel(const AnalyzeArgs a, const BandBlockCoefs<B> cf, int nb,
                                                                      float* __restrict__ out, int tailN, int n50, int n80) {
    __shared__ double tab[96];
    fillLogTab(tab, threadIdx.x, kBandsBlock);
    __syncthreads();  // (before any wave leaves)
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kBandsBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    bandMetricsBody<S, NB, CHUNK, B>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, cf, nb, LogTabLds{tab}, tailN, n50, n80);
}

}  // namespace

int bandMetricsBlock() { return PV_BANDS_B; }

// coefs: n x kBandCoefs floats on the HOST.  out: n x kBandFloats planes of a.histPlane floats, plane k of band j of the cell at
// history offset g at out[(j * kBandFloats + k) * histPlane + g]
void launchBandMetrics(const AnalyzeArgs& a, const float* coefs, int n, float* out, hipStream_t stream) {
    constexpr int B = PV_BANDS_B;
    const int tailN = decayTailN((int)a.fs), n50 = roomMetricsN50((int)a.fs), n80 = roomMetricsN80((int)a.fs);
    const dim3 grid((unsigned)((a.histPlane + kBandsBlock - 1) / kBandsBlock));
    for (int b0 = 0; b0 < n; b0 += B) {
        const int nb = n - b0 < B ? n - b0 : B;
        BandBlockCoefs<B> cf;
        for (int j = 0; j < B; ++j)
            for (int k = 0; k < kBandCoefs; ++k) cf.c[j][k] = j < nb ? coefs[(size_t)(b0 + j) * kBandCoefs + k] : 0.f;
        float* o = out + (size_t)b0 * kBandFloats * (size_t)a.histPlane;
        if (a.histPlane * 4 * PV_BANDS_S < (1ll << 31))
            hipLaunchKernelGGL((pv_band_metrics_kernel<PV_BANDS_S, PV_BANDS_NB, true, B>), grid, dim3(kBandsBlock), 0, stream, a, cf, nb, o,
                               tailN, n50, n80);
        else
            hipLaunchKernelGGL((pv_band_metrics_kernel<PV_BANDS_S, PV_BANDS_NB, false, B>), grid, dim3(kBandsBlock), 0, stream, a, cf, nb, o,
                               tailN, n50, n80);
    }
}

}  // namespace pva
