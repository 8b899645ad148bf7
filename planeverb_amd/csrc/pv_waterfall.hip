// pv_waterfall.hip -- per-receiver waterfalls (pv_waterfall.h) of the LAST COMPLETED run: few cells, many bins, which is the
// transpose of pv_spectrum_kernel (many cells, few bins, twiddles in SGPRs).
//
// Shape.  A lane owns a BIN, a wave owns 64 consecutive bins of a register block of RB receivers (one workgroup = one wave; grid =
// bin blocks x receiver groups).  Time is wave-uniform and runs BACKWARDS from T - 1: one walk passes every slice boundary
// onset + k * ns of a receiver, and at a boundary the lane stores the level of its bin -- for slice 0 also its two sums -- with
// plain vector stores.  Nothing is reduced across lanes, nothing is atomic, the device evaluates no trigonometric function.
//   twiddles   row t of the table, laid out as the kernel reads it: [bin block][kWaterfallTablePad zero rows, then T rows][64 lanes]
//              {cos, sin} pairs, so a wave's read of a step is ONE 8-byte load per lane, 512 contiguous bytes; the bins past n of
//              the last block are zero and are never stored.  Rows of a sub-chunk of kSub steps are fetched one sub-chunk ahead.
//   samples    one (offset, stride) pair per receiver into one base: (g, histPlane) into the history with g the cell's offset in a
//              history plane (histOffset, as recordLaneOfCell computes it), or (i * T, 1) into the emitter traces of sparse-emitter
//              mode -- one kernel text for both.  A chunk of 64 steps of a receiver is ONE vector load, lane l fetching step
//              tc - l (64 words in flight per receiver and instruction, the next chunk fetched while this one is summed); the step's
//              sample then reaches every lane through v_readlane.  A lane whose step lies below the receiver's first loadable step
//              -- the larger of its onset and its tile's first recorded step, before which the history holds no data -- loads
//              nothing and holds +0.0f, which is what PvAmdCopyHistoryPlane returns there.
//   blocking   RB receivers share a wave's twiddle loads (the table is re-read per receiver group, not per receiver).  RB is
//              chosen by the launcher from the number of waves the call gives (DESIGN.md 4.27 has the resource table).
//
// The identity argument of pv_spectrum.hip, for this walk.  The definition sums p(t) * w over t = T - 1 down to the onset, from
// +0.0f; the wave walks from T - 1 down to the SMALLEST onset of its receivers, in whole chunks, and a receiver outside its own
// range contributes p = +0.0f.  A twiddle w is finite (a rounded cosine or sine, or the table's zero padding), so such a product
// is +0 or -0, and adding either to a running sum leaves its bits unchanged: x + (+-0) = x for x != 0, (+0) + (+-0) = +0 in
// round-to-nearest, and a sum that started at +0 is never -0 (a sum is -0 only if both operands are).  Backwards the argument is
// needed even less than forwards: the extra steps of a receiver all lie BELOW its onset, i.e. behind its last boundary (slice 0,
// at the onset itself), so nothing that is added there is ever stored.  What a record holds therefore depends on its own cell's
// samples and on the tables alone -- not on the other receivers of the wave, their order, or RB.
//
// A receiver without a record (off the map, outside the run's history window, no onset: a wall, a cell the pulse never reached)
// gets F quiet NaNs and never loads.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"
#include "pv_waterfall.h"

namespace pva {

namespace {

constexpr int kChunk = 64;  // steps per sample load: one per lane
constexpr int kSub = 8;     // steps per twiddle fetch
static_assert(kChunk + kSub - 1 <= kWaterfallTablePad, "the fetch behind the last chunk reads table rows down to -(kChunk + kSub - 1)");
static_assert(kChunk % (2 * kSub) == 0, "whole pairs of sub-chunks");

// The receiver table: one thread per receiver.  cells[i] = result cell X * gy + Y, -1 off the map; trace: the samples are the
// emitter traces (row i of [nPos][T]) instead of the history
__global__ void pv_waterfall_receivers_kernel(const AnalyzeArgs a, const long long* __restrict__ cells, int nPos, int trace,
                                              WaterfallRx* __restrict__ rx) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nPos) return;
    const DynParams dyn = *a.dyn;
    WaterfallRx r{0, 0, -1, INT_MAX};
    const long long cell = cells[i];
    if (cell >= 0 && cell < (long long)a.gx * a.gy) {
        const int X = (int)(cell / a.gy), Y = (int)(cell - (long long)X * a.gy);
        const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
        if (hr >= 0 && hc >= 0 && hr < dyn.histTilesX * a.rxi && hc < dyn.histTilesY * a.wi) {
            const long long g = histOffset(hr, hc, a.rxi, a.wi, dyn.histTilesY);
            const float delay = a.delay[cell];
            const int onset = delay != FLT_MAX ? (int)delay : -1;
            if ((trace || g < a.histPlane) && onset >= 0 && onset < a.T) {
                r.onset = onset;
                if (trace) {
                    r.offset = (long long)i * a.T;
                    r.stride = 1;
                    r.tLoad = onset;
                } else {
                    r.offset = g;
                    r.stride = a.histPlane;
                    r.tLoad = max(onset, a.tileFirst[(X / a.rxi) * a.nty + Y / a.wi]);
                }
            }
        }
    }
    rx[i] = r;
}

template <int RB>
__global__ __launch_bounds__(64) void pv_waterfall_kernel(const WaterfallArgs a) {
    const int lane = threadIdx.x;
    const int blk = blockIdx.x;
    const int bin = blk * 64 + lane;
    const int n = a.n, m = a.m, ns = a.ns, T = a.T;
    const bool mine = bin < n;
    const float spow = mine ? a.spow[bin] : 1.0f;
    const float qnan = __builtin_nanf("");
    const int F = waterfallFloats(n, m);

    // the wave's receivers (everything here is wave-uniform: block index and kernel arguments)
    long long off[RB], stride[RB];
    int tLoad[RB], tNext[RB], kNext[RB];
    float* rec[RB];
    int tmin = INT_MAX;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int idx = blockIdx.y * RB + r;
        off[r] = stride[r] = 0;
        tLoad[r] = INT_MAX;  // (never loads)
        tNext[r] = INT_MIN;  // (no boundary)
        kNext[r] = -1;
        rec[r] = nullptr;
        if (idx >= a.nPos) continue;
        const WaterfallRx rx = a.rx[idx];
        float* const rc = a.rec + (size_t)idx * (size_t)F;
        rec[r] = rc;
        if (rx.onset < 0) {  // no record: F quiet NaNs
            if (blk == 0 && lane < kWaterfallHead) rc[lane] = qnan;
            if (mine) {
                rc[waterfallReOff(n) + bin] = qnan;
                rc[waterfallImOff(n) + bin] = qnan;
                for (int k = 0; k < m; ++k) rc[waterfallLevelOff(n, k) + bin] = qnan;
            }
            continue;
        }
        const int count = waterfallSliceCount(T, rx.onset, ns, m);
        if (blk == 0 && lane == 0) {
            rc[0] = (float)rx.onset;
            rc[1] = (float)count;
        }
        if (mine) {  // the slices that start at or past T: R = I = +0.0f
            const float empty = spectrumLevel(0.f, 0.f, spow);
            for (int k = count; k < m; ++k) rc[waterfallLevelOff(n, k) + bin] = empty;
        }
        off[r] = rx.offset;
        stride[r] = rx.stride;
        tLoad[r] = rx.tLoad;
        kNext[r] = count - 1;
        tNext[r] = rx.onset + (count - 1) * ns;
        tmin = min(tmin, rx.onset);
    }
    if (tmin == INT_MAX) return;  // (no receiver of the group has a record)

    const float* __restrict__ smp = a.samples;
    // the 64 steps tc, tc - 1, .. of every receiver: lane l holds step tc - l, +0.0f below the receiver's first loadable step
    auto loadSamples = [&](float (&dst)[RB], int tc) {
        const int t = tc - lane;
#pragma unroll
        for (int r = 0; r < RB; ++r) dst[r] = t >= tLoad[r] ? smp[off[r] + (long long)t * stride[r]] : 0.f;
    };
    // rows t = tc .. tc - 63 of the block's table: row t, this lane, at row0[-(tc - t) * 64]
    const v2f* __restrict__ tab = reinterpret_cast<const v2f*>(a.tab) + ((size_t)blk * (size_t)(T + kWaterfallTablePad) + kWaterfallTablePad) * 64 + lane;
    auto loadRows = [&](v2f (&w)[kSub], int t) {
        const v2f* row = tab + (long long)t * 64;
#pragma unroll
        for (int u = 0; u < kSub; ++u) w[u] = row[-u * 64];
    };

    float re[RB], im[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) re[r] = im[r] = 0.f;
    float cur[RB], nxt[RB];
    // The kSub steps t0, t0 - 1, .. whose samples sit in lanes l0, l0 + 1, .. of cur and whose rows are w.  No boundary of any
    // receiver among them (the common case): the sums alone.  Else step by step with the boundary test -- the row comes again
    // from memory there (w[u] at a run-time u would leave the registers), so the store's text exists RB times, not kSub x RB times
    auto steps = [&](const v2f (&w)[kSub], int t0, int l0) {
        int tb = INT_MIN;  // the wave's next boundary
#pragma unroll
        for (int r = 0; r < RB; ++r) tb = max(tb, tNext[r]);
        if (tb <= t0 - kSub) {
#pragma unroll
            for (int u = 0; u < kSub; ++u)
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const float p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur[r]), l0 + u));
                    spectrumStep(p, w[u].x, w[u].y, re[r], im[r]);
                }
            return;
        }
#pragma unroll 1
        for (int u = 0; u < kSub; ++u) {
            const int t = t0 - u;
            const v2f wu = tab[(long long)t * 64];
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const float p = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cur[r]), l0 + u));
                spectrumStep(p, wu.x, wu.y, re[r], im[r]);
                if (t == tNext[r]) {  // wave-uniform: the boundary of slice kNext[r]
                    const int k = kNext[r];
                    if (mine) {
                        float* const rc = rec[r];
                        rc[waterfallLevelOff(n, k) + bin] = spectrumLevel(re[r], im[r], spow);
                        if (k == 0) {
                            rc[waterfallReOff(n) + bin] = re[r];
                            rc[waterfallImOff(n) + bin] = im[r];
                        }
                    }
                    kNext[r] = k - 1;
                    tNext[r] = k > 0 ? t - ns : INT_MIN;
                }
            }
        }
    };

    loadSamples(cur, T - 1);
    v2f wA[kSub], wB[kSub];
    loadRows(wA, T - 1);
#pragma unroll 1
    for (int tc = T - 1; tc >= tmin; tc -= kChunk) {
        loadSamples(nxt, tc - kChunk);  // (past the last chunk: every lane below every first step, nothing is loaded)
#pragma unroll 1
        for (int l0 = 0; l0 < kChunk; l0 += 2 * kSub) {
            // the rows of a sub-chunk are fetched while the one before it is summed; the lowest row read is that of the fetch
            // behind the last chunk: tc - kChunk - (kSub - 1) >= -(kChunk + kSub - 1), inside the table's front padding
            const int t0 = tc - l0;
            loadRows(wB, t0 - kSub);
            steps(wA, t0, l0);
            loadRows(wA, t0 - 2 * kSub);
            steps(wB, t0 - kSub, l0 + kSub);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) cur[r] = nxt[r];
    }
}

template <int RB>
void launchWaterfallRB(const WaterfallArgs& a, hipStream_t stream) {
    const dim3 grid((unsigned)((a.n + 63) / 64), (unsigned)((a.nPos + RB - 1) / RB));
    hipLaunchKernelGGL((pv_waterfall_kernel<RB>), grid, dim3(64), 0, stream, a);
}

}  // namespace

void launchWaterfallReceivers(const AnalyzeArgs& a, const long long* cells, int nPos, bool trace, WaterfallRx* rx, hipStream_t stream) {
    hipLaunchKernelGGL(pv_waterfall_receivers_kernel, dim3((unsigned)((nPos + 63) / 64)), dim3(64), 0, stream, a, cells, nPos, trace ? 1 : 0, rx);
}

bool waterfallBlockOk(int block) { return block == 1 || block == 2 || block == 4; }

// The receivers a wave takes: the largest block that still gives every one of the device's `cus` compute units a wave (a wave
// walks all T steps on its own, so below that the pass's time is one wave's time and sharing twiddle loads only lengthens it)
int waterfallBlockFor(int n, int nPos, int cus) {
    const int blocks = (n + 63) / 64;
    for (int rb = 4; rb > 1; rb >>= 1)
        if (blocks * ((nPos + rb - 1) / rb) >= cus) return rb;
    return 1;
}

void launchWaterfall(const WaterfallArgs& a, int block, hipStream_t stream) {
    if (block == 4)
        launchWaterfallRB<4>(a, stream);
    else if (block == 2)
        launchWaterfallRB<2>(a, stream);
    else
        launchWaterfallRB<1>(a, stream);
}

}  // namespace pva
