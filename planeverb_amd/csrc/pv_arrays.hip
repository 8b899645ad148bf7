// pv_arrays.hip -- source arrays (pv_arrays.h): the responses y_a(t) of up to kArraysMax arrays of weighted, delayed members from
// what the LAST COMPLETED run left on the device -- the pressure history, or in sparse-emitter mode the emitters' traces --, and
// the onset of every response.  A reduction [members][T] -> [arrays][T]; the records are then computed by the query record
// kernels off the mix planes (recordLaneOfMix, pv_record_lane.h).
//
// Three kernels, no atomics, no LDS, no inline assembly, plain vector stores:
//   rows    pv_array_rows_kernel, one thread per member: where its samples are -- (offset, stride) into ONE sample base, as
//           pv_waterfall_receivers_kernel does it: (histOffset(..), histPlane) into the history, (i * T, 1) into the emitter
//           traces -- and its first loadable step (its tile's first recorded step; 0 for a trace, whose row is cleared when a run
//           begins).  A cell outside the run's history window gets "no samples" (INT_MAX).  Unlike a waterfall receiver a member is
//           NOT cut at its own onset: the definition takes what PvAmdCopyHistoryPlane returns.
//   mix     pv_array_mix_kernel: time runs along the lanes (a wave = 64 consecutive steps, a block = 256), blockIdx.y is the
//           COLUMN of the mix planes.  The column's tap list {row, delay, weight} is walked wave-uniformly (the index depends on
//           blockIdx.y and the loop counter alone: scalar loads, SGPRs), and so is the member row it names.  A tap is then ONE
//           vector load per lane with its own bounds select: lane t loads sample t - delay where tLoad <= t - delay (delay >= 0, so
//           t - delay <= T - 1 where t is), else holds +0.0f and loads nothing.  y = y + (w * p), product and sum each rounded
//           (-ffp-contract=off), from +0.0f, in tap order.  Trace mode: a wave's load is 64 consecutive words.  History mode: lane
//           t reads plane t - delay, 64 different lines per instruction, one word used of each -- the history is time-major and
//           the mix wants one cell's time series; taps x T words per array either way.  The addresses are 64-bit global ones: a
//           wave's 64 steps span 64 planes, and the history spans more than the 2^32 bytes one buffer descriptor reaches, so the
//           bounds are the selects (every address formed lies inside the sample base: 0 <= tLoad <= t - delay < T, offset <
//           histPlane or row i of the traces).  The result goes to planes [T][P], P = the arrays rounded up to 64 -- the layout
//           the record bodies read, a response being column a; columns a >= nArrays are zero.  A wave's store is 64 words P apart.
//   onset   pv_array_onsets_kernel: one wave per column scans chunks of 64 steps in increasing t; the first chunk with a lane
//           above the threshold gives the onset as the first set bit of the ballot.  Columns a >= nArrays get FLT_MAX.
//
// A response's bits depend on its own tap list and its members' samples alone: not on the other arrays, its column or the launch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_arrays.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"

namespace pva {

namespace {

constexpr int kMixBlock = 256;  // steps per block: four waves

// src[m]: the member's result cell X * gy + Y (history), or the index of the registered emitter whose cell it is (trace)
__global__ void pv_array_rows_kernel(const AnalyzeArgs a, const long long* __restrict__ src, int nRows, int trace, ArrayRow* __restrict__ rows) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= nRows) return;
    ArrayRow r{0, 0, INT_MAX, 0};  // (no samples)
    const long long s = src[m];
    if (trace) {
        if (s >= 0) {
            r.offset = s * a.T;
            r.stride = 1;
            r.tLoad = 0;
        }
    } else if (s >= 0 && s < (long long)a.gx * a.gy) {
        const DynParams dyn = *a.dyn;
        const int X = (int)(s / a.gy), Y = (int)(s - (long long)X * a.gy);
        const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
        if (hr >= 0 && hc >= 0 && hr < dyn.histTilesX * a.rxi && hc < dyn.histTilesY * a.wi) {
            const long long g = histOffset(hr, hc, a.rxi, a.wi, dyn.histTilesY);
            if (g < a.histPlane) {
                r.offset = g;
                r.stride = a.histPlane;
                r.tLoad = max(a.tileFirst[(X / a.rxi) * a.nty + Y / a.wi], 0);
            }
        }
    }
    rows[m] = r;
}

__global__ __launch_bounds__(kMixBlock) void pv_array_mix_kernel(const ArrayMixArgs a) {
    const int col = (int)blockIdx.y;  // (wave-uniform)
    const int t = (int)blockIdx.x * kMixBlock + (int)threadIdx.x;
    if (t >= a.T) return;
    float y = 0.f;
    if (col < a.nArrays) {
        const int k0 = a.tapOff[col], k1 = a.tapOff[col + 1];
        const float* __restrict__ smp = a.samples;
#pragma unroll 1
        for (int k = k0; k < k1; ++k) {
            const ArrayTap tp = a.taps[k];
            const ArrayRow r = a.rows[tp.row];
            const int ts = t - tp.delay;
            const float p = ts >= r.tLoad ? smp[r.offset + (long long)ts * r.stride] : 0.f;
            y = arrayMixStep(y, tp.w, p);
        }
    }
    a.mix[(long long)t * a.P + col] = y;
}

__global__ __launch_bounds__(64) void pv_array_onsets_kernel(const float* __restrict__ mix, int T, int P, int nArrays, float* __restrict__ onsets) {
    const int col = (int)blockIdx.x, lane = (int)threadIdx.x;
    float onset = FLT_MAX;
    if (col < nArrays) {
#pragma unroll 1
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            const float y = t < T ? mix[(long long)t * P + col] : 0.f;
            const unsigned long long hit = __ballot(arrayOnsetAt(y));
            if (hit) {  // (wave-uniform)
                onset = (float)(t0 + (int)__builtin_ctzll(hit));
                break;
            }
        }
    }
    if (lane == 0) onsets[col] = onset;
}

}  // namespace

void launchArrayRows(const AnalyzeArgs& a, const long long* src, int nRows, bool trace, ArrayRow* rows, hipStream_t stream) {
    hipLaunchKernelGGL(pv_array_rows_kernel, dim3((unsigned)((nRows + 63) / 64)), dim3(64), 0, stream, a, src, nRows, trace ? 1 : 0, rows);
}

void launchArrayMix(const ArrayMixArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.T + kMixBlock - 1) / kMixBlock), (unsigned)a.P);
    hipLaunchKernelGGL(pv_array_mix_kernel, grid, dim3(kMixBlock), 0, stream, a);
}

void launchArrayOnsets(const float* mix, int T, int P, int nArrays, float* onsets, hipStream_t stream) {
    hipLaunchKernelGGL(pv_array_onsets_kernel, dim3((unsigned)P), dim3(64), 0, stream, mix, T, P, nArrays, onsets);
}

}  // namespace pva
