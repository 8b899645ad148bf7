// pv_aural.hip -- auralisation (pv_aural.h): the responses of up to kAuralMaxReceivers receivers resampled from the grid's rate to
// an audio rate, their convolution with dry signals, and the mix.  Plain HIP: no atomics, no inline assembly, plain vector stores.
//
//   gather    pv_aural_gather_kernel: a receiver's samples are strided by plane in the history (or column a of the array mix
//             planes, or row i of the emitter traces); one thread per (t, receiver) copies them into a contiguous row [R][T],
//             +0.0f below the row's first loadable step, as pv_array_mix_kernel reads a member.
//   resample  pv_aural_resample_kernel: one lane per output sample n, a wave = 64 consecutive n of one receiver (blockIdx.y).  The
//             weights are stored transposed [K][L], so slot j of 64 consecutive n is one coalesced load; first[n] grows with n by
//             fs / rate per sample, so the 64 sample loads of a slot fall into a few lines of the gathered row.  A sample outside
//             0 .. T - 1 is a select to +0.0f: no address outside the row is formed.
//   convolve  the hot path, two forms with the same bits:
//             tiled  pv_aural_convolve_tiled_kernel: a block is ONE wave that owns kAuralOutputsPerBlock = 64 x kP consecutive
//                    outputs of one receiver, kP consecutive ones per lane, their accumulators in registers for the whole k walk:
//                    k is never split, so every output sums in the definition's order.  The block walks ITS k range -- from
//                    max(0, m0 - N + 1) to min(L - 1, m0 + B - 1), what its outputs can reach -- in chunks of kAuralTapsPerChunk
//                    taps.  A chunk stages its taps and the B + C - 1 samples they meet in LDS (zero where the index is outside
//                    the response or the signal).  A tap is read from LDS at a wave-uniform address (a broadcast, four taps per
//                    ds_read_b128); the samples are a register window per lane that slides down one sample per tap: four taps
//                    cost one ds_read_b128 of four new samples (lane stride 16 bytes: a 16-lane group reads one 256-byte bank
//                    row, conflict-free) and 2 x kP x 4 VALU operations.  A chunk all of whose (output, tap) pairs are terms of the
//                    definition takes that path; a chunk at an edge of the response or the signal takes the general path, the
//                    same walk with the sum SELECTED per output (a term outside the definition is not formed: 0 * inf would
//                    be a NaN the definition does not have).
//             plain  pv_aural_convolve_plain_kernel: one lane per output, taps and samples from global memory.
//             An unrouted receiver's outputs are written as +0.0f by either form.
//   mix       pv_aural_mix_kernel: one lane per m, sequential over r.
#include <hip/hip_runtime.h>

#include "pv_aural.h"
#include "pv_launch.h"

namespace pva {

namespace {

constexpr int kP = 4;                        // outputs per lane
constexpr int kB = kAuralOutputsPerBlock;    // outputs per block: one wave
constexpr int kC = kAuralTapsPerChunk;       // taps per staged chunk
constexpr int kSpan = kB + kC;               // staged samples: B + C - 1, rounded up
static_assert(kB == 64 * kP && kP == 4 && kC % 4 == 0, "a float4 of taps and of new samples per four taps");

__global__ __launch_bounds__(256) void pv_aural_gather_kernel(const float* __restrict__ samples, const ArrayRow* __restrict__ src, int T,
                                                              float* __restrict__ rows) {
    const int r = (int)blockIdx.y;  // (wave-uniform)
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= T) return;
    const ArrayRow s = src[r];
    rows[(size_t)r * T + t] = t >= s.tLoad ? samples[s.offset + (long long)t * s.stride] : 0.f;
}

__global__ __launch_bounds__(256) void pv_aural_resample_kernel(const float* __restrict__ rows, int T, const int* __restrict__ first,
                                                                const float* __restrict__ wT, int L, int K, float* __restrict__ resp) {
    const int r = (int)blockIdx.y;
    const int n = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (n >= L) return;
    const float* __restrict__ p = rows + (size_t)r * T;
    const int f = first[n];
    float h = 0.f;
#pragma unroll 1
    for (int j = 0; j < K; ++j) {
        const int t = f + j;
        const float v = (t >= 0 && t < T) ? p[t] : 0.f;
        h = auralStep(h, wT[(size_t)j * L + n], v);
    }
    resp[(size_t)r * L + n] = h;
}

__global__ __launch_bounds__(64) void pv_aural_convolve_tiled_kernel(const AuralConvolveArgs a) {
    __shared__ __attribute__((aligned(16))) float hs[kC];
    __shared__ __attribute__((aligned(16))) float xs[kSpan];
    const int r = (int)blockIdx.y, lane = (int)threadIdx.x;
    const int L = a.L, N = a.N, M = N + L - 1;
    const int m0 = (int)blockIdx.x * kB;  // (m0 < M: the launcher's grid)
    const int mb = m0 + lane * kP;
    float* __restrict__ out = a.out + (size_t)r * M;
    const int sig = a.route[r];  // (wave-uniform)
    float acc[kP];
#pragma unroll
    for (int i = 0; i < kP; ++i) acc[i] = 0.f;
    if (sig >= 0) {
        const float* __restrict__ h = a.resp + (size_t)r * L;
        const float* __restrict__ x = a.signals + (size_t)sig * N;
        const int mLast = min(m0 + kB - 1, M - 1);      // the block's last output
        const int kBegin = auralTapLo(m0, N);           // the lowest tap any of its outputs has
        const int kEnd = auralTapHi(mLast, L);          // the highest
#pragma unroll 1
        for (int k0 = kBegin; k0 <= kEnd; k0 += kC) {
            // stage: hs[j] = h[k0 + j]; xs[i] = x[xb + i], xb = m0 - (k0 + kC - 1): output m meets tap k0 + j at xs[m - m0 - j + kC - 1]
            const int xb = m0 - (k0 + kC - 1);
            __syncthreads();  // (the chunk before has been read)
            for (int j = lane; j < kC; j += 64) hs[j] = k0 + j < L ? h[k0 + j] : 0.f;
            for (int i = lane; i < kSpan; i += 64) {
                const int g = xb + i;
                xs[i] = (g >= 0 && g < N) ? x[g] : 0.f;
            }
            __syncthreads();
            // every (output, tap) pair of the chunk a term: the last tap within the response and at or below the first output,
            // the first tap not below what the last output of a FULL block starts at
            const bool whole = k0 + kC - 1 <= min(L - 1, m0) && k0 >= m0 + kB - N;
            const int base = lane * kP + kC - 1;  // xs index of (output mb, tap k0)
            float w[2 * kP - 1];                  // w[d + kP - 1] = xs[base - jc + d], d = -(kP - 1) .. kP - 1
#pragma unroll
            for (int d = 1; d < kP; ++d) w[d + kP - 1] = xs[base + d];
            if (whole) {
#pragma unroll 2
                for (int jc = 0; jc < kC; jc += kP) {
                    const float4 lo = *reinterpret_cast<const float4*>(&xs[base - jc - (kP - 1)]);
                    const float4 t4 = *reinterpret_cast<const float4*>(&hs[jc]);
                    w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w;
                    const float tap[kP] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                    for (int jj = 0; jj < kP; ++jj)
#pragma unroll
                        for (int i = 0; i < kP; ++i) acc[i] = auralStep(acc[i], tap[jj], w[i - jj + kP - 1]);
#pragma unroll
                    for (int q = 0; q < kP - 1; ++q) w[kP + q] = w[q];
                }
            } else {
                const int jEnd = min(kC, kEnd - k0 + 1);  // (the taps past the block's range meet nothing)
#pragma unroll 1
                for (int jc = 0; jc < jEnd; jc += kP) {
                    const float4 lo = *reinterpret_cast<const float4*>(&xs[base - jc - (kP - 1)]);
                    const float4 t4 = *reinterpret_cast<const float4*>(&hs[jc]);
                    w[0] = lo.x, w[1] = lo.y, w[2] = lo.z, w[3] = lo.w;
                    const float tap[kP] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                    for (int jj = 0; jj < kP; ++jj) {
                        const int k = k0 + jc + jj;
#pragma unroll
                        for (int i = 0; i < kP; ++i) {
                            const int xi = mb + i - k;  // the sample's index: a term where 0 <= xi < N and k < L
                            const float next = auralStep(acc[i], tap[jj], w[i - jj + kP - 1]);
                            acc[i] = ((unsigned)xi < (unsigned)N && k < L) ? next : acc[i];
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kP - 1; ++q) w[kP + q] = w[q];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < kP; ++i)
        if (mb + i < M) out[mb + i] = acc[i];
}

__global__ __launch_bounds__(256) void pv_aural_convolve_plain_kernel(const AuralConvolveArgs a) {
    const int r = (int)blockIdx.y;
    const int L = a.L, N = a.N, M = N + L - 1;
    const int m = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (m >= M) return;
    const int sig = a.route[r];
    float o = 0.f;
    if (sig >= 0) {
        const float* __restrict__ h = a.resp + (size_t)r * L;
        const float* __restrict__ x = a.signals + (size_t)sig * N;
        const int k1 = auralTapHi(m, L);
#pragma unroll 1
        for (int k = auralTapLo(m, N); k <= k1; ++k) o = auralStep(o, h[k], x[m - k]);
    }
    a.out[(size_t)r * M + m] = o;
}

__global__ __launch_bounds__(256) void pv_aural_mix_kernel(const float* __restrict__ out, const int* __restrict__ route,
                                                           const float* __restrict__ gain, int R, int M, float* __restrict__ mix) {
    const int m = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (m >= M) return;
    float y = 0.f;
#pragma unroll 1
    for (int r = 0; r < R; ++r)
        if (route[r] >= 0) y = auralStep(y, gain[r], out[(size_t)r * M + m]);  // (wave-uniform)
    mix[m] = y;
}

}  // namespace

void launchAuralGather(const float* samples, const ArrayRow* src, int R, int T, float* rows, hipStream_t stream) {
    hipLaunchKernelGGL(pv_aural_gather_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)R), dim3(256), 0, stream, samples, src, T, rows);
}

void launchAuralResample(const float* rows, int R, int T, const int* first, const float* wT, int L, int K, float* resp, hipStream_t stream) {
    hipLaunchKernelGGL(pv_aural_resample_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)R), dim3(256), 0, stream, rows, T, first, wT, L, K,
                       resp);
}

void launchAuralConvolve(const AuralConvolveArgs& a, int form, hipStream_t stream) {
    const int M = a.N + a.L - 1;
    if (form == kAuralPlain)
        hipLaunchKernelGGL(pv_aural_convolve_plain_kernel, dim3((unsigned)((M + 255) / 256), (unsigned)a.R), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(pv_aural_convolve_tiled_kernel, dim3((unsigned)((M + kB - 1) / kB), (unsigned)a.R), dim3(64), 0, stream, a);
}

void launchAuralMix(const float* out, const int* route, const float* gain, int R, int M, float* mix, hipStream_t stream) {
    hipLaunchKernelGGL(pv_aural_mix_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, out, route, gain, R, M, mix);
}

}  // namespace pva
