// pv_spectrum.hip -- per-cell transfer functions at chosen frequencies (pv_spectrum.h) of the LAST COMPLETED run: the forward pass
// of pv_metrics.hip over the recorded pressure history with another loop body.
//
// Kept from pv_room_metrics_kernel, because it is what makes every line of the history be fetched exactly once: one lane per
// OFFSET g inside a history plane (pv_analysis.h planeCell), wave-uniform time from the smallest onset among the wave's live lanes
// to T - 1, a ring of NB chunks of S planes of buffer loads in flight per wave, a lane outside its own range loading through an
// out-of-extent buffer offset (the load returns 0 without touching memory: nothing below a cell's onset may be read), NaN records
// for the offsets without an onset, and a wave without a live lane leaving at once.
//
// The identity argument for this body.  The definition sums p(t) * w over t = t0 .. T - 1 from +0.0f; the lane sums over the
// WAVE's range and feeds p = +0.0f outside its own.  A twiddle w is finite (a rounded cosine or sine, or the table's zero padding),
// so the extra product is +0 * w = +0 or, for a negative twiddle, -0.  Adding either to a running sum leaves its bits unchanged:
// x + (+-0) = x for every x that is not a zero, (+0) + (+0) = +0, and (+0) + (-0) = +0 in round-to-nearest.  The remaining case,
// (-0) + (+-0), never arises: a sum is -0 only if both of its operands are, so one that started at +0 can never become -0 --
// neither here nor in the definition, which starts at +0 as well.  The steps below a lane's onset come first, while its sums are
// still +0; the steps past T - 1 (the last chunk's tail: the table rows there are zero) come last and add +0.
//
// New here:
//   twiddles   the 2 B twiddles of a step are the same for all 64 lanes: row t of the pass's table, {cos, sin} pairs, is read
//              through a wave-uniform address (kernel-argument pointer, scalar step counter), i.e. by scalar loads into SGPRs,
//              and every multiply takes its twiddle from there.  No lane reads the table, and the device evaluates no
//              trigonometric function.
//   bins       B bins per pass are register-blocked: 2 B accumulators per lane, as B (re, im) pairs.  A pair is advanced by one
//              packed multiply and one packed add (v_pk_mul_f32 / v_pk_add_f32 round each half on its own); nothing is fused
//              (-ffp-contract=off).  2 B multiply-adds per history sample against one load: the pass's time goes with the bins,
//              not with the history bytes -- docs/experiments/spectrum.md has the measured times.
//   n > B      the host (Solver::computeSpectrum) runs one pass per slice of the bins, each with its own table slice.
// The records are stored after the loop (the only stores of the kernel), which keeps the table loads provably unclobbered.
//
// The text of the pass is spectrumBody (pv_spectrum_dev.h): this file keeps the description, the whole-map kernel -- a wrapper that
// gives the body the lane's consecutive offset and the out[k * plane + g] store -- and its launchers; pv_query_spectral.hip runs the
// same body for the cells of a run's queries (the table rows are indexed by absolute step: wave-uniform there as well).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"
#include "pv_spectrum.h"
#include "pv_spectrum_dev.h"

namespace pva {

namespace {

constexpr int kSpectrumThreads = 256;
// CHUNK: a chunk's S planes through ONE descriptor and S constant scalar offsets (S planes must stay below 2^31 bytes);
// otherwise one descriptor per plane
template <int B, int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kSpectrumThreads) void pv_spectrum_kernel(const AnalyzeArgs a, int bins, const float* __restrict__ tab,
                                                                      const float* __restrict__ spow, float* __restrict__ out) {
    const DynParams dyn = *a.dyn;
    const long long g = ((long long)blockIdx.x * (kSpectrumThreads / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    spectrumBody<B, S, NB, CHUNK>(a, recordLaneAt(a, dyn, g), PlaneStore{out, a.histPlane, g}, bins, tab, spow);
}

template <int B>
void launchSpectrumB(const AnalyzeArgs& a, int bins, const float* tab, const float* spow, float* out, hipStream_t stream) {
    const dim3 grid((unsigned)((a.histPlane + kSpectrumThreads - 1) / kSpectrumThreads));
    if (a.histPlane * 4 * PV_SPECTRUM_S < (1ll << 31))
        hipLaunchKernelGGL((pv_spectrum_kernel<B, PV_SPECTRUM_S, PV_SPECTRUM_NB, true>), grid, dim3(kSpectrumThreads), 0, stream, a, bins, tab, spow, out);
    else
        hipLaunchKernelGGL((pv_spectrum_kernel<B, PV_SPECTRUM_S, PV_SPECTRUM_NB, false>), grid, dim3(kSpectrumThreads), 0, stream, a, bins, tab, spow, out);
}

}  // namespace

// B = 32 was built and timed as well (136 VGPRs) and never won: docs/experiments/spectrum.md
bool spectrumBlockOk(int block) { return block == 8 || block == 16; }

void launchSpectrum(const AnalyzeArgs& a, int block, int bins, const float* tab, const float* spow, float* out, hipStream_t stream) {
    if (block == 8)
        launchSpectrumB<8>(a, bins, tab, spow, out, stream);
    else
        launchSpectrumB<16>(a, bins, tab, spow, out, stream);
}

}  // namespace pva
