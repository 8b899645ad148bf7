// pv_echo.hip -- per-cell echo criterion (Dietsch and Kraak; speech and music variant: pv_echo.h) of the LAST COMPLETED run, one
// forward pass over the recorded pressure history.
//
// The frame is pv_room_metrics_kernel's (pv_metrics.hip): one lane per OFFSET g of a history plane, wave-uniform time from the
// smallest onset among the wave's live lanes to T - 1, a lane outside its own range loading 0 through an out-of-extent buffer
// offset, a ring of NB chunks of S planes of loads in flight, both descriptor forms, a NaN record for every offset without an
// onset, and a wave without a live lane leaving at once.
//
// New here are the lagged centres.  x(k) needs c(k - nD), the value this very lane computed nD steps earlier, and nD has no bound
// that fits registers (12 and 20 steps at 70^2, hundreds on fine grids).  The pass keeps no c: per variant a second pair of sums,
// A' and B', is fed from p(t - nD) -- three load streams, p(t), p(t - nDs) and p(t - nDm) -- and makes exactly the additions the
// leading pair made nD steps earlier, masked by select while k - nD < 0.  B' / A' therefore has the bits of c(k - nD) (the
// argument is spelled out in DESIGN.md 4.15).  Nothing is added outside a lane's own range [onset, T): every update of pv_echo.h
// echoStep is a select on `on`, so the steps that wave-uniform time visits below a lane's onset or past T - 1 leave the lane's
// state untouched, whatever the loads returned.  A lagged plane t - nD is read only where t - nD >= onset (the tile's history
// exists from its first recorded launch, which is not later than the onset of any of its cells); everywhere else the lane's
// offset is out of extent.
//
// The speech weight is |p|^(2/3), glibc's powf (pv_libm.h pvPowfNonNegT): two evaluations per sample and lane, the leading and
// the lagged one, with the function's two tables (32 + 32 doubles) in LDS, filled by the block's first wave.  The 2 S
// evaluations of a chunk are written in front of the chunk's sequential part, so the scheduler has S independent chains of
// each.  Per sample the pass also makes six correctly rounded divisions (c and c' of both variants, x of both); it is bound by
// these and the double-precision work of powf, not by the history bytes (three times the room-metrics pass's, two thirds of
// them re-reads of lines the same wave fetched nD steps earlier).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_echo.h"
#include "pv_launch.h"
#include "pv_prims.h"

#ifndef PV_ECHO_S
#define PV_ECHO_S 4  // planes per chunk and stream
#endif
#ifndef PV_ECHO_NB
#define PV_ECHO_NB 4  // chunks of loads in flight per wave
#endif

namespace pva {

namespace {

constexpr int kEchoBlock = 256;

struct PowTabLds {
    const double* lt;    // 16 x {invc, logc}
    const uint64_t* et;  // 32 exp2 entries
    __device__ __forceinline__ void log2(int i, double* invc, double* logc) const {
        *invc = lt[2 * i];
        *logc = lt[2 * i + 1];
    }
    __device__ __forceinline__ uint64_t exp2(int j) const { return et[j]; }
};

// CHUNK: a chunk's S planes through ONE descriptor and S scalar offsets (S planes must stay below 2^31 bytes); otherwise one
// descriptor per plane
template <int S, int NB, bool CHUNK>
__global__ __launch_bounds__(kEchoBlock) void pv_echo_kernel(const AnalyzeArgs a, float* __restrict__ out, int nDs, int nDm, int nLs, int nLm) {
    __shared__ double powLt[32];
    __shared__ uint64_t powEt[32];
    if (threadIdx.x < 32) {
        double invc, logc;
        PvPowTabConst{}.log2((int)threadIdx.x >> 1, &invc, &logc);
        powLt[threadIdx.x] = (threadIdx.x & 1) ? logc : invc;
    } else if (threadIdx.x < 64) {
        powEt[threadIdx.x - 32] = PvPowTabConst{}.exp2((int)threadIdx.x - 32);
    }
    __syncthreads();
    const PowTabLds ptab{powLt, powEt};

    const DynParams dyn = *a.dyn;
    const int T = a.T;
    constexpr int kOut = 0x7fffffff;  // >= every descriptor's extent: the load returns 0
    const long long plane = a.histPlane;
    const int planeBytes = (int)(plane * 4);

    const long long g = ((long long)blockIdx.x * (kEchoBlock / 64) + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
    const PlaneCell pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    const float delay = pc.inGrid ? a.delay[(long long)pc.X * a.gy + pc.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (g < plane && !live) {
        const float qnan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < kEchoFloats; ++k) out[k * plane + g] = qnan;
    }
    if (__ballot(live) == 0ull) return;

    const int t0 = live ? (int)delay : 0;
    const int t0l = live ? t0 : INT_MAX;  // (a dead lane never loads and is never `on`)
    int t0min = live ? t0 : INT_MAX, t0max = live ? t0 : INT_MIN;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        t0min = min(t0min, __shfl_xor(t0min, off));
        t0max = max(t0max, __shfl_xor(t0max, off));
    }
    // (wave-uniform by value; said so to the compiler: scalar loop counters and descriptors)
    t0min = max(__builtin_amdgcn_readfirstlane(t0min), 0);
    t0max = __builtin_amdgcn_readfirstlane(t0max);
    const int voff = (int)g * 4;
    const int lvoff = live ? voff : kOut;

    // the S loads of one stream's chunk: steps tc .. tc + S - 1, planes tc - lag .. (issued whatever tc is: the counts are the
    // same on every path).  A lane gets p(t - lag) where t < T and t - lag >= its onset, 0 elsewhere
    auto loadStream = [&](float (&dst)[S], int tc, int lag) {
        const int tl = tc - lag;                  // the chunk's first plane (negative: the stream has not begun)
        const int tb = min(max(tl, 0), T - 1);    // (the base stays inside the history)
        const rsrc_t rs = makeRsrc(a.hist + (long long)tb * plane, CHUNK ? (long long)S * planeBytes : (long long)planeBytes);
        if (tl >= t0max && tc + S <= T) {  // every live lane is inside its range (t0max >= 0: tb = tl)
#pragma unroll
            for (int k = 0; k < S; ++k)
                dst[k] = CHUNK ? bufLoadF(rs, lvoff, (int)((unsigned)k * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)(tl + k) * plane, planeBytes), lvoff, 0);
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k, tp = t - lag;
                const int vo = (t < T && tp >= t0l) ? voff : kOut;
                // (a lane in range has 0 <= tp - tb <= k: tb = tl, or tb = 0 > tl; the clamp serves the others)
                const int dk = min(max(tp - tb, 0), S - 1);
                dst[k] = CHUNK ? bufLoadF(rs, vo, (int)((unsigned)dk * (unsigned)planeBytes))
                               : bufLoadF(makeRsrc(a.hist + (long long)min(max(tp, 0), T - 1) * plane, planeBytes), vo, 0);
            }
        }
    };
    float ring[NB][3][S];
    auto loadChunk = [&](float (&dst)[3][S], int tc) {
        loadStream(dst[0], tc, 0);
        loadStream(dst[1], tc, nDs);
        loadStream(dst[2], tc, nDm);
        __builtin_amdgcn_sched_barrier(0);
    };

    EchoVar sp = echoVarInit(), mu = echoVarInit();
    const float nDsf = (float)nDs, nDmf = (float)nDm;
    const int n = (T - t0min + S - 1) / S;  // chunks from the wave's smallest onset to T - 1
#pragma unroll
    for (int b = 0; b < NB; ++b) loadChunk(ring[b], t0min + b * S);
#pragma unroll 1
    for (int c0 = 0; c0 < n; c0 += NB) {
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int tc = t0min + (c0 + b) * S;
            float a0[S], as[S], am[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                a0[k] = echoAbs(ring[b][0][k]);
                as[k] = echoAbs(ring[b][1][k]);
                am[k] = echoAbs(ring[b][2][k]);
            }
            loadChunk(ring[b], tc + NB * S);  // the slot's next occupant
            if (tc >= T) continue;            // (past the last chunk)
            float ws[S], wls[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                ws[k] = pvPowfNonNegT(a0[k], kEchoSpeechExponent, ptab);
                wls[k] = pvPowfNonNegT(as[k], kEchoSpeechExponent, ptab);
            }
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int t = tc + k;
                const bool on = t >= t0l && t < T;
                const int kk = t - t0;  // (below the lane's onset: negative, and `on` is false)
                echoStep(sp, on, kk, ws[k], wls[k], nDs, nDsf, nLs);
                echoStep(mu, on, kk, a0[k], am[k], nDm, nDmf, nLm);
            }
        }
    }
    if (!live) return;
    float rec[kEchoFloats];
    echoRecord(sp, (int)a.fs, rec);
    echoRecord(mu, (int)a.fs, rec + 5);
#pragma unroll
    for (int k = 0; k < kEchoFloats; ++k) out[k * plane + g] = rec[k];
}

}  // namespace

// out: kEchoFloats planes of a.histPlane floats, plane k of the cell at history offset g at out[k * histPlane + g]
void launchEchoCriterion(const AnalyzeArgs& a, float* out, hipStream_t stream) {
    const int fs = (int)a.fs;
    const int nDs = echoSpeechLag(fs), nDm = echoMusicLag(fs), nLs = echoSpeechLimit(fs), nLm = echoMusicLimit(fs);
    const dim3 grid((unsigned)((a.histPlane + kEchoBlock - 1) / kEchoBlock));
    if (a.histPlane * 4 * PV_ECHO_S < (1ll << 31))
        hipLaunchKernelGGL((pv_echo_kernel<PV_ECHO_S, PV_ECHO_NB, true>), grid, dim3(kEchoBlock), 0, stream, a, out, nDs, nDm, nLs, nLm);
    else
        hipLaunchKernelGGL((pv_echo_kernel<PV_ECHO_S, PV_ECHO_NB, false>), grid, dim3(kEchoBlock), 0, stream, a, out, nDs, nDm, nLs, nLm);
}

}  // namespace pva
