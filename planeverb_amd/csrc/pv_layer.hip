// pv_layer.hip -- graded absorbing layers at the grid edges (pv_layer.h).  No reference counterpart.
//
// The layer tiles are advanced by a launch of their own beside each merged launch (Solver::enqueueSteps).  Its tile body is the
// two-kernel form's scalar general tile (pv_kernels.hip stepTile<..., GENERAL = true>, leapfrogStepCoef) restated with the
// damping behind a compile-time flag (and the split-field pressure behind a second one); pv_kernels.hip itself is untouched, so
// the merged kernel compiles to what it did.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "pv_layer.h"
#include "pv_prims.h"

namespace pva {

// ---------------------------------------------------------------------------------------------------------------
// layer tile body
// ---------------------------------------------------------------------------------------------------------------

// leapfrogStepCoef with the damping (DAMP) or without it (the general tile's expressions, unchanged).  Per-row factors are
// wave-uniform (rf: apx, bpx, ax, bx of the row), per-column ones (apy, bpy, ay, by) one value per lane.
// SPLIT (the split-field model, DAMP too): a layer cell (apx != 1 or apy != 1) carries px, the x part of its pressure (the y
// part is pr - px), and damps each part by its own axis only; every other cell takes the general tile's expression, px = 0:
//   nx = beta * ((apx * px) - bpx * (C * dvx))    ny = beta * ((apy * (pr - px)) - bpy * (C * dvy))    pr' = nx + ny, px' = nx
template <int ROWS, bool DAMP, bool SPLIT>
__device__ __forceinline__ void leapfrogStepLayer(float (&pr)[ROWS], float (&px)[ROWS], float (&vx)[ROWS], float (&vy)[ROWS],
                                                  const float (&kx)[ROWS], const float (&ky)[ROWS], const float (&bt)[ROWS],
                                                  const float* __restrict__ rf, const int rpitch, const float apy,
                                                  const float bpy, const float ay, const float by, const float C) {
    static_assert(DAMP || !SPLIT, "the split form is a damped form");
    const bool colLayer = apy != 1.f;  // (per lane)
#pragma unroll
    for (int r = 0; r < ROWS - 1; ++r) {
        const float vyR = laneNext(vy[r]);
        const float dvx = vx[r + 1] - vx[r], dvy = vyR - vy[r];
        if constexpr (SPLIT) {
            const float apx = rf[r];  // (wave-uniform: the row flag)
            const bool layer = apx != 1.f || colLayer;
            const float nx = bt[r] * ((apx * px[r]) - rf[rpitch + r] * (C * dvx));
            const float ny = bt[r] * ((apy * (pr[r] - px[r])) - bpy * (C * dvy));
            const float plain = bt[r] * (pr[r] - C * (dvx + dvy));
            pr[r] = layer ? nx + ny : plain;
            px[r] = layer ? nx : 0.f;
        } else if constexpr (DAMP) {
            pr[r] = bt[r] * ((rf[r] * apy) * pr[r] - (rf[rpitch + r] * bpy) * (C * (dvx + dvy)));
        } else {
            pr[r] = bt[r] * (pr[r] - C * (dvx + dvy));
        }
    }
#pragma unroll
    for (int r = ROWS - 1; r >= 1; --r) {
        const float pi = pr[r], pn = pr[r - 1];
        float air;
        if constexpr (DAMP)
            air = rf[2 * rpitch + r] * vx[r] - rf[3 * rpitch + r] * (C * (pi - pn));
        else
            air = vx[r] - C * (pi - pn);
        const float wall = kx[r] * (pi + pn);
        vx[r] = (kx[r] != kx[r]) ? air : wall;
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const float pi = pr[r];
        const float pn = lanePrev(pi);
        float air;
        if constexpr (DAMP)
            air = ay * vy[r] - by * (C * (pi - pn));
        else
            air = vy[r] - C * (pi - pn);
        const float wall = ky[r] * (pi + pn);
        vy[r] = (ky[r] != ky[r]) ? air : wall;
    }
}

// a general tile's `part`-th slice of SUB interior rows (+ K halo rows either side): walls, the listener's pulse, history
// recording, tileFirst and nzOut exactly as stepTile<K, RXI, SUB, true> does them; SPLIT: px from l.pxIn, to l.pxOut
template <int K, int RXI, int SUB, bool DAMP, bool SPLIT>
__device__ __forceinline__ void stepLayerTile(const LayerArgs& l, const int tile, const int part, const int lane) {
    const StepArgs& a = l.a;
    constexpr int ROWS = SUB + 2 * K;
    constexpr int WI = 64 - 2 * K;
    const int ti = tile / a.nty;
    const int tj = tile - ti * a.nty;
    const int row0 = a.G - K + ti * RXI + part * SUB;
    const int col0 = a.G - K + tj * WI;
    const int voff = lane * 4;
    const int pitchB = a.pitch * 4;
    const int soff0 = (row0 * a.pitch + col0) * 4;

    const rsrc_t rPrIn = makeRsrc(a.prIn, a.inBytes), rVxIn = makeRsrc(a.vxIn, a.inBytes),
                 rVyIn = makeRsrc(a.vyIn, a.inBytes);
    const rsrc_t rCoef = makeRsrc(a.coef, a.planeBytes * 3);
    typedef unsigned int u3v __attribute__((ext_vector_type(3)));

    float pr[ROWS], px[ROWS], vx[ROWS], vy[ROWS], kx[ROWS], ky[ROWS], bt[ROWS];
    const rsrc_t rPxIn = makeRsrc(l.pxIn, SPLIT ? a.inBytes : 0);  // (a run's first launch: zero extent, as the fields)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int so = soff0 + r * pitchB;
        pr[r] = bufLoadF(rPrIn, voff, so);
        px[r] = SPLIT ? bufLoadF(rPxIn, voff, so) : 0.f;
        vx[r] = bufLoadF(rVxIn, voff, so);
        vy[r] = bufLoadF(rVyIn, voff, so);
        const u3v c = __builtin_amdgcn_raw_buffer_load_b96(rCoef, lane * 12, 3 * so, 0);
        kx[r] = __uint_as_float(c.x);
        ky[r] = __uint_as_float(c.y);
        bt[r] = __uint_as_float(c.z);
    }
    // (the tables: rows [row0, row0 + ROWS) and columns [col0, col0 + 64) lie inside the padded planes, as the field loads do)
    const float* rf = l.rowTab + row0;
    const int col = col0 + lane;
    const float apy = l.colTab[col], bpy = l.colTab[l.cols + col], ay = l.colTab[2 * l.cols + col],
                by = l.colTab[3 * l.cols + col];

    uint32_t nz = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
        nz |= (__float_as_uint(pr[r]) | __float_as_uint(vx[r]) | __float_as_uint(vy[r])) & 0x7fffffffu;
    bool active = __ballot(nz != 0u) != 0ull;

    const DynParams dyn = *a.dyn;
    const int lr = dyn.lrow - row0;
    const int lc = dyn.lcol - col0;
    const bool hasL = a.withPulse && lr >= 0 && lr < ROWS && lc >= 0 && lc < 64;
    active = active || hasL;
    if (lane == 0) a.nzOut[tile] = 1;  // (general tiles always count as non-zero)

    const int hti = ti - dyn.histTileX0, htj = tj - dyn.histTileY0;
    const bool inWin = hti >= 0 && hti < dyn.histTilesX && htj >= 0 && htj < dyn.histTilesY;
    const bool rec = a.record && inWin;
    if (a.record && active && lane == 0) atomicMin(&a.tileFirst[tile], a.t0);
    if (a.record && active && !inWin && lane == 0) atomicExch(a.errFlag, 1);

    const float C = a.courant;
    const bool inCols = lane >= K && lane < 64 - K;
    const float* hplane = a.hist + (long long)a.histSlot * a.histPlane;
    const int hpitchB = WI * 4;
    const int hsoff0 = ((hti * dyn.histTilesY + htj) * RXI + part * SUB - K) * hpitchB;
    const int hvoff = (lane - K) * 4;

#pragma unroll 1
    for (int s = 0; s < a.nsteps; ++s) {
        leapfrogStepLayer<ROWS, DAMP, SPLIT>(pr, px, vx, vy, kx, ky, bt, rf, l.rows, apy, bpy, ay, by, C);
        if (rec) {  // the pressure of this step before the pulse (FDTD.cpp:226-234)
            const rsrc_t rH = makeRsrc(hplane, a.histPlane * 4);
            if (inCols) {
#pragma unroll
                for (int r = K; r < ROWS - K; ++r) bufStoreF(pr[r], rH, hvoff, hsoff0 + r * hpitchB);
            }
        }
        hplane += a.histPlane;
        if (hasL) {  // soft source: p[listener] += pulse[t], FDTD.cpp:234
            const float pv = (lane == lc) ? a.pulse[a.t0 + s] : 0.f;
            int lrS = lr;
            asm volatile("" : "+s"(lrS));
#pragma unroll
            for (int r = 0; r < ROWS; ++r) pr[r] += (r == lrS) ? pv : 0.f;
        }
    }

    const rsrc_t rPrOut = makeRsrc(a.prOut, a.planeBytes), rVxOut = makeRsrc(a.vxOut, a.planeBytes),
                 rVyOut = makeRsrc(a.vyOut, a.planeBytes);
    if (inCols) {
#pragma unroll
        for (int r = K; r < ROWS - K; ++r) {
            const int so = soff0 + r * pitchB;
            bufStoreF(pr[r], rPrOut, voff, so);
            bufStoreF(vx[r], rVxOut, voff, so);
            bufStoreF(vy[r], rVyOut, voff, so);
        }
        if constexpr (SPLIT) {
            const rsrc_t rPxOut = makeRsrc(l.pxOut, a.planeBytes);
#pragma unroll
            for (int r = K; r < ROWS - K; ++r) bufStoreF(px[r], rPxOut, voff, soff0 + r * pitchB);
        }
    }
}

// one wave per SUB-row slice of a layer tile, RXI / SUB slices per tile, four waves per block
template <int K, int RXI, int SUB, bool SPLIT>
__global__ __launch_bounds__(256) void pv_step_layer_kernel(const LayerArgs l) {
    constexpr int S = RXI / SUB;
    static_assert(S * SUB == RXI, "layer-tile split must divide the tile");
    const StepArgs& a = l.a;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int idx = blockIdx.x * 4 + wave;
    if (idx >= l.count * S) return;
    const int tile = __builtin_amdgcn_readfirstlane(l.list[idx / S]);
    const int ti = tile / a.nty, tj = tile - ti * a.nty;
    if (a.tileDead && a.tileDead[tile]) {  // (the general arm's rule: dead unless the listener is in the loaded region)
        const int lr = a.dyn->lrow - (a.G - K + ti * RXI), lc = a.dyn->lcol - (a.G - K + tj * (64 - 2 * K));
        if (!a.withPulse || !(lr >= 0 && lr < RXI + 2 * K + 8 && lc >= 0 && lc < 64)) return;
    }
    // reach-bounded launch: a tile the fields cannot have reached stays zero, as in the merged launch's arms
    if (a.winTis > 0 && !tileInReach(ti, tj, RXI, 64 - 2 * K, a.G, a.reachGrow, a.reachRow, a.reachCol, a.reach)) return;
    stepLayerTile<K, RXI, SUB, true, SPLIT>(l, tile, idx % S, lane);
}

// (K steps per launch, interior rows per tile, rows per slice): the product library's tiles (pv_kernels.hip
// PV_PRODUCT_STEP_CONFIGS), with the slices of its two-kernel form
#define PV_LAYER_CONFIGS(X) X(8, 24, 12) X(10, 36, 9) X(12, 36, 9) X(8, 40, 10) X(12, 12, 6) X(10, 20, 10)

bool layerConfigOk(int K, int rxi) {
#define X(k, r, sub) \
    if (K == k && rxi == r) return true;
    PV_LAYER_CONFIGS(X)
#undef X
    return false;
}

template <int K, int RXI, int SUB, bool SPLIT>
static void launchStepLayerT(const LayerArgs& l, hipStream_t stream) {
    const int blocks = (l.count * (RXI / SUB) + 3) / 4;
    hipLaunchKernelGGL((pv_step_layer_kernel<K, RXI, SUB, SPLIT>), dim3(blocks), dim3(256), 0, stream, l);
}

void launchStepLayer(int K, int rxi, const LayerArgs& l, hipStream_t stream) {
    if (l.count <= 0) return;
    if (l.pxOut) {  // (the split form fits the same slices: no scratch, profiles/edge_layer.txt)
#define X(k, r, sub) \
    if (K == k && rxi == r) return launchStepLayerT<k, r, sub, true>(l, stream);
        PV_LAYER_CONFIGS(X)
#undef X
        return;
    }
#define X(k, r, sub) \
    if (K == k && rxi == r) return launchStepLayerT<k, r, sub, false>(l, stream);
    PV_LAYER_CONFIGS(X)
#undef X
}

}  // namespace pva
