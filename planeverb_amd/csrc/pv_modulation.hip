// pv_modulation.hip -- per-cell, per-band modulation transfer function and modulation transfer index (pv_modulation.h) of the LAST
// COMPLETED run: each reached cell's recorded pressure is band-pass filtered BACKWARDS in time (pv_bands.h bandFilterStep), and
// the squared output is summed against 14 (cos, sin) pairs per step (the accumulators of pv_spectrum.hip) on the same walk.
//
// The frame is pv_band_metrics_kernel's (pv_bands.hip), kept line for line where it can be: one lane per history-plane offset g,
// time DOWN and wave-uniform from T - 1 to the smallest onset among the wave's live lanes, a ring of NB chunks of S buffer loads
// in flight per wave, out-of-extent offsets that load 0 below a lane's onset, a record of quiet NaNs for every offset without an
// onset, waves without a live lane leaving at once, the per-plane-descriptor form for very large planes, records by plane offset.
//
// New here:
//  * ONE band per launch and ONE walk: the record needs E(t0) only as the divisor of the sums, after the loop.  Per lane: the band's
//    four filter states, E and 14 (re, im) pairs.  The band's ten coefficients arrive as kernel arguments (SGPRs).
//  * The 28 twiddles of a step are the same for all 64 lanes: row t of the table (ABSOLUTE step, so the row address is
//    wave-uniform whatever the lanes' onsets are) is read through a kernel-argument pointer and a scalar step counter, i.e. by
//    scalar loads into SGPRs.  A pair is advanced by one packed multiply and one packed add (v_pk_mul_f32 / v_pk_add_f32 round
//    each half on its own; nothing is fused: -ffp-contract=off).  No lane reads the table, and the device evaluates no
//    trigonometric function.  tab points at row 0; kModTablePad zero rows lie in front of it, for the last chunk of a wave whose
//    smallest onset is below S - 1.
//  * FREEZING.  The steps below a lane's own onset come last (time runs down) and the wave goes on to its smallest onset.  A filter
//    fed zeros rings on, so the four filter states are SELECTED on k = t - t0 >= 0, as in the band kernel, and the e of such a
//    step is replaced by +0.0f.  That is enough for the 29 sums -- the identity argument: E + (+0) = E for every E (E is a sum of
//    squares from +0, never -0).  A twiddle w is finite, so (+0) * w is +0 or -0, and x + (+-0) = x for every x that is not a
//    zero, (+0) + (+-0) = +0 in round-to-nearest; an accumulator is never -0, because a sum is -0 only if both operands are and it
//    started at +0.  So a frozen lane's sums keep their bits without a select per accumulator, and a lane above its onset
//    computes exactly the host restatement's operations in its order.
//  * The records are stored after the loop (the only stores of a live wave), which keeps the table loads provably unclobbered.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, S = 8, NB = 4): profiles/modulation.txt.
//
// The text of the pass is modulationBody (pv_modulation_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that
// gives the body the lane's consecutive offset and the out[k * plane + g] store -- and its launcher; pv_query_spectral.hip runs the
// same body for the cells of a run's queries (the table rows are indexed by absolute step: wave-uniform there as well).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_modulation.h"
#include "pv_modulation_dev.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kModBlock = 256;
// out: the band's kModFloats planes (float k of the cell at history offset g at out[k * plane + g])
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kModBlock) void pv_modulation_kernel(const AnalyzeArgs a, const ModBandCoefs cf, const float* __restrict__ tab,
                                                                  float* __restrict__ out) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kModBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    modulationBody<S, NB, CHUNK>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, cf, tab);
}

}  // namespace

// coefs: n x kBandCoefs floats on the HOST.  tab: row 0 of the device table (kModTablePad zero rows in front of it, T rows of
// kModRowStride floats).
// out: n x kModFloats planes of a.histPlane floats, float k of band j of the cell at history offset g at
// out[(j * kModFloats + k) * histPlane + g]
void launchModulation(const AnalyzeArgs& a, const float* coefs, int n, const float* tab, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kModBlock - 1) / kModBlock));
    for (int j = 0; j < n; ++j) {
        ModBandCoefs cf;
        for (int k = 0; k < kBandCoefs; ++k) cf.c[k] = coefs[(size_t)j * kBandCoefs + k];
        float* o = out + (size_t)j * kModFloats * (size_t)a.histPlane;
        if (a.histPlane * 4 * PV_MODULATION_S < (1ll << 31))
            hipLaunchKernelGGL((pv_modulation_kernel<PV_MODULATION_S, PV_MODULATION_NB, true>), grid, dim3(kModBlock), 0, stream, a, cf, tab, o);
        else
            hipLaunchKernelGGL((pv_modulation_kernel<PV_MODULATION_S, PV_MODULATION_NB, false>), grid, dim3(kModBlock), 0, stream, a, cf, tab, o);
    }
}

}  // namespace pva
