// pv_analysis.hip -- the per-cell impulse-response analysis, one pass per launch: onset, encode (dry gain, source direction,
// low-pass), the far cells, the listener direction (walk and pointer jumping), and the streaming form of the sparse-emitter
// mode.  The per-cell bodies are device functions of pv_analysis_dev.h; wet gain and decay time are pv_rt60.hip.
//
// Reference semantics implemented here (paths relative to the reference's ProjectPlaneverb directory):
//   pv_onset_kernel, pv_encode_kernel   src/DSP/Analyzer.cpp:139-328  onset, dry gain, source direction, lowpass, wet, RT60
//   pv_direction_kernel                 src/DSP/Analyzer.cpp:340-431  listener direction by delay-map descent
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cstdint>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_libm.h"
#include "pv_prims.h"
#include "pv_record_lane.h"
#include "pv_zone_maps.h"

namespace pva {

// ---------------------------------------------------------------------------------------------------------------
// impulse-response analysis
// ---------------------------------------------------------------------------------------------------------------

// pvLog10f / pvPowf: glibc-2.35-exact log10f and powf, see pv_libm.h

// CH samples (i0, i0-1, ..., i0-CH+1; those below startingPoint are skipped) of the backward Schroeder integration
// + regression sums, Analyzer.cpp:300-318.  Three passes over the chunk: the running energy (sequential, the
// reference's order), 10*log10f of each partial sum (independent of each other: branch-free, so the compiler
// interleaves the CH evaluations -- with one thread per cell and few waves this loop is bound by the latency of one
// evaluation, ~1800 cycles per sample when they ran one after the other), the two regression sums (sequential).
template <int CH>
__device__ __forceinline__ void rt60Chunk(const float (&pc)[CH], const int i0, const int startingPoint, float& edc,
                                          float& xysum, float& ysum) {
    float e[CH], y[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        edc = (i0 - k >= startingPoint) ? edc + pc[k] * pc[k] : edc;
        e[k] = edc;
    }
#pragma unroll
    for (int k = 0; k < CH; ++k) y[k] = 10.f * pvLog10fNonNeg(e[k]);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const bool v = i0 - k >= startingPoint;
        xysum = v ? xysum + y[k] * (float)(i0 - k - startingPoint) : xysum;
        ysum = v ? ysum + y[k] : ysum;
    }
}

// One thread per result cell (X, Y); lanes along Y so every history read is a coalesced row segment of one
// recorded plane.  All sums are sequential float32 accumulations in the reference's order.
// vx / vy are not stored: they are re-derived from the pressure history with the stencil's own recurrence
// (v_t = v_{t-1} - C*(p_t[i] - p_t[n]) on air|air faces, k*(p_i + p_n) otherwise), bit-identical to the values
// the step kernel held.
// The analysis kernels run over the HISTORY WINDOW only (winRows x winCols cells from the window's origin, which
// lives in dyn so that the launch grid does not depend on the listener): a cell outside it cannot have been reached
// by the pulse.  What the reference computes for such a cell -- delay = FLT_MAX, direction = the unit vector from
// the listener to the cell itself -- is written for the whole map by pv_far_cells_kernel first.  (The first version
// launched one thread per grid cell: 67 M threads at 8192^2 to find the 0.6 M reached cells.)
__device__ __forceinline__ bool analysisWindowCell(const AnalyzeArgs& a, const DynParams& dyn, int* X, int* Y) {
    const int wc = blockIdx.x * blockDim.x + threadIdx.x, wr = blockIdx.y;
    if (wc >= a.winCols) return false;
    *X = dyn.histRow0 - a.G + wr;
    *Y = dyn.histCol0 - a.G + wc;
    return *X < a.gx && *Y < a.gy;
}

// Onset of every window cell (Analyzer.cpp:146-165: first sample whose |pressure| exceeds the audible threshold), round 5.
// Rounds 1-4 found it inside pv_encode_kernel, one thread per cell walking forward through time: the kernel lasted as long as
// its slowest thread, and the slowest threads were the SILENT cells -- air cells of a reached tile that never become audible
// (the air outside a closed room, in the tiles its walls cross): all T samples, 16 per memory round trip, 280 us of a 370 us
// kernel at 512^2 / T = 3179 -- and the decay-time pass could only start behind it.  Here the search is parallel IN TIME: a
// block is 64 consecutive cells of the tile-major plane (planeCell: one coalesced 256-byte read per plane) x 16 waves, wave w
// scans the samples t = tBeg + (16 j + w) 16 + k; the earliest hit per cell is kept with an LDS minimum, and a wave stops once
// no cell of the block can improve.  A silent cell costs T / 256 round trips instead of T / 16.  pv_encode_kernel and the
// decay-time kernels read the onset from the delay map, side by side on two streams.
#ifndef PV_ONSET_WAVES
#define PV_ONSET_WAVES 4
#endif
#ifndef PV_ONSET_SC
#define PV_ONSET_SC 32
#endif
constexpr int kOnsetWaves = PV_ONSET_WAVES, kOnsetSC = PV_ONSET_SC;
__global__ __launch_bounds__(64 * kOnsetWaves) void pv_onset_kernel(const AnalyzeArgs a) {
    __shared__ int found[64];
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long g = (long long)blockIdx.x * 64 + lane;
    const PlaneCell c = planeCell(a, dyn, g);
    const int T = a.T;
    int tF = INT_MAX;
    bool live = c.inGrid;
    if (live) {
        tF = a.tileFirst[c.tile];
        // never reached by the pulse, or a wall (beta = 0: pr is identically zero, FDTD.cpp:139): no onset
        live = tF < T && a.coef[(size_t)(c.X + a.G) * a.pitch + (c.Y + a.G)].beta != 0.f;
    }
    const bool air = live;  // (an air cell of a reached tile: without an onset it counts as silent)
    if (a.labels) {
        // ... nor has a cell that no chain of air cells joins to the listener's (AnalyzeArgs::labels): not scanned
        const int lX = dyn.lrow - a.G, lY = dyn.lcol - a.G;
        const int mine = live ? a.labels[(size_t)c.X * a.labelNY + c.Y] : -1;
        const int theirs = (lX >= 0 && lX <= a.gx && lY >= 0 && lY < a.labelNY) ? a.labels[(size_t)lX * a.labelNY + lY] : -2;
        live = live && mine == theirs;
    }
    if (wave == 0) found[lane] = INT_MAX;
    if (a.stamp && blockIdx.x == 0 && threadIdx.x == 0) a.stamp[1] = wall_clock64();
    __syncthreads();
    // near box (AnalyzeArgs::box): the cells the PREVIOUS run reached get "no onset" back unless this run reaches them again --
    // every other cell of the map holds it already.  A cell of this window is its own lane's business (below, and where the
    // search ends); the previous box's cells OUTSIDE this window (the listener moved far) are dealt over the workgroups here.
    bool inPrev = false;
    if (a.box) {
        const int p0 = a.prevBox[0], p1 = a.prevBox[1], p2 = min(a.prevBox[2], a.gx - 1), p3 = min(a.prevBox[3], a.gy - 1);
        inPrev = c.inGrid && c.X >= p0 && c.X <= p2 && c.Y >= p1 && c.Y <= p3;
        if (p2 >= p0 && p3 >= p1) {  // (empty: INT_MAX / -1 -- no arithmetic on those)
            const int wr0 = dyn.histRow0 - a.G, wc0 = dyn.histCol0 - a.G;
            const int wr1 = wr0 + min(a.winRows, a.gx - wr0) - 1, wc1 = wc0 + min(a.winCols, a.gy - wc0) - 1;
            if (p0 < wr0 || p2 > wr1 || p1 < wc0 || p3 > wc1)  // (block-uniform)
                for (int r = p0 + (int)blockIdx.x; r <= p2; r += (int)gridDim.x)
                    for (int cc = p1 + (int)threadIdx.x; cc <= p3; cc += (int)blockDim.x)
                        if (r < wr0 || r > wr1 || cc < wc0 || cc > wc1) a.delay[r * a.gy + cc] = FLT_MAX;
        }
    }
    if (a.wholeWindow || a.box) {
        // no far-frame launch in front of this one: "no onset" for the cells that will not get one, and the count of active cells
        // (what pv_far_frame_kernel's first block does; the run's last kernel has left the other counters at zero)
        if (wave == 0 && c.inGrid && !live && (a.wholeWindow || inPrev)) a.delay[c.X * a.gy + c.Y] = FLT_MAX;
        if (blockIdx.x == 0 && wave == 1) {
            int n = 0;
            for (int i = lane; i < dyn.histTilesX * dyn.histTilesY; i += 64) {
                const int ti = dyn.histTileX0 + i / dyn.histTilesY, tj = dyn.histTileY0 + i % dyn.histTilesY;
                if (a.tileFirst[ti * a.nty + tj] < T) n += a.rxi * a.wi;
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) n += __shfl_xor(n, off);
            if (lane == 0) a.activeCount[0] = n;
        }
    }
    if (__ballot(live) == 0ull) {  // (the same lanes in every wave of the block: block-uniform)
        const unsigned long long ms = __ballot(air);
        if (wave == 0 && lane == 0 && ms) atomicAdd(a.activeCount + 3, __popcll(ms));
        return;
    }
    // A run starts from zero fields and the stencil moves a value by one cell per step along one axis (FDTD.cpp:124-199): the
    // recorded pressure of a cell at Manhattan distance m from the listener is exactly zero up to and including step m,
    // whatever the geometry.  The search starts there (cells far from the listener: half the samples between the tile's first
    // recorded step and the onset).  No listener in the grid: no pulse, no onset.
    const int m = abs(c.X - (dyn.lrow - a.G)) + abs(c.Y - (dyn.lcol - a.G));
    const int tS = live ? min(max(tF, m), T) : INT_MAX;
    int tBeg = tS;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) tBeg = min(tBeg, __shfl_xor(tBeg, off));
    tBeg = __builtin_amdgcn_readfirstlane(tBeg);  // (wave-uniform by value: scalar loop counter, scalar descriptors)
    const int voff = (int)g * 4;
    const int planeBytes = (int)(a.histPlane * 4);
    constexpr int SC = kOnsetSC;
#pragma unroll 1
    for (int t = tBeg + wave * SC; t < T; t += kOnsetWaves * SC) {
        const int best = found[lane];
        if (__ballot(live && best > t) == 0ull) break;  // nothing at or after t can be the first
        float pc[SC];
#pragma unroll
        for (int k = 0; k < SC; ++k) {
            const int tt = t + k;
            const bool want = live && tt >= tS && tt < T && tt < best;  // (a tile's history starts at its first recorded step)
            pc[k] = bufLoadF(makeRsrc(a.hist + (long long)min(tt, T - 1) * a.histPlane, planeBytes), want ? voff : 0x7fffffff, 0);
        }
        int hit = INT_MAX;
#pragma unroll
        for (int k = SC - 1; k >= 0; --k) hit = fabsf(pc[k]) > kAudibleThresholdDev ? t + k : hit;
        if (hit != INT_MAX) atomicMin(&found[lane], hit);
    }
    __syncthreads();
    if (wave != 0) return;
    const int onset = found[lane];
    if (live) {
        if (onset != INT_MAX) a.delay[c.X * a.gy + c.Y] = (float)onset;
        else if (a.wholeWindow || inPrev) a.delay[c.X * a.gy + c.Y] = FLT_MAX;
    }
    // reached cells of this run (bench / PvAmdTimings.reachedCells) and silent ones: one atomic each per block
    const bool reached = live && onset != INT_MAX;
    const unsigned long long mr = __ballot(reached), ms = __ballot(air && !reached);
    if (a.box && mr) {  // the reached cells' bounding box (AnalyzeArgs::box): four atomics per group with work
        int r0 = reached ? c.X : INT_MAX, c0 = reached ? c.Y : INT_MAX, r1 = reached ? c.X : -1, c1 = reached ? c.Y : -1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            r0 = min(r0, __shfl_xor(r0, off));
            c0 = min(c0, __shfl_xor(c0, off));
            r1 = max(r1, __shfl_xor(r1, off));
            c1 = max(c1, __shfl_xor(c1, off));
        }
        // (an atomic only where the group can still move a bound: in an open field 4 300 groups have work, and four atomics each on
        // the same four words took 330 us of the kernel -- same-address atomics are served one after the other; the plain reads
        // may be stale, which only means an atomic that changes nothing)
        if (lane == 0) {
            const int b0 = __hip_atomic_load(a.box + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int b1 = __hip_atomic_load(a.box + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int b2 = __hip_atomic_load(a.box + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int b3 = __hip_atomic_load(a.box + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (r0 < b0) atomicMin(a.box + 0, r0);
            if (c0 < b1) atomicMin(a.box + 1, c0);
            if (r1 > b2) atomicMax(a.box + 2, r1);
            if (c1 > b3) atomicMax(a.box + 3, c1);
        }
    }
    if (lane == 0) {
        if (mr) {
            atomicAdd(a.activeCount + 1, __popcll(mr));
            a.unitList[atomicAdd(a.activeCount + 4, 1)] = (int)blockIdx.x;  // this group of 64 cells has work for the passes behind
        }
        if (ms) atomicAdd(a.activeCount + 3, __popcll(ms));
    }
}

// dry gain, source directivity, low-pass cutoff (+ wet gain beside the lane-per-cell decay-time form) of the cells that have an
// onset, behind pv_onset_kernel: one wave per entry of the list of 64-cell groups with work (encodeWave, pv_analysis_dev.h)
__global__ __launch_bounds__(256) void pv_encode_kernel(const AnalyzeArgs a) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    const int unit = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (unit >= a.activeCount[4]) return;
    const PlaneCell pc0 = planeCell(a, dyn, (long long)a.unitList[unit] * 64 + (threadIdx.x & 63));
    const float delay = pc0.inGrid ? a.delay[pc0.X * a.gy + pc0.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;  // no onset (Analyzer.cpp:160-165): the result record stays as it is
    if (__ballot(live) == 0ull) return;
    encodeWave<false>(a, dyn, pc0, live, live ? (int)delay : 0, rt60LanesPerCell(a, a.activeCount[1]) == 1);
}

// the same pass with L lanes per cell (encodeGroups, pv_analysis_dev.h): the small windows, where the longest walk is the kernel.
// A 64-cell group of the list is L waves: L / 4 workgroups
template <int L>
__global__ __launch_bounds__(256) void pv_encode_groups_kernel(const AnalyzeArgs a) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    constexpr int BPU = L / 4;  // workgroups per group of 64 cells
    const int unit = blockIdx.x / BPU;
    if (unit >= a.activeCount[4]) return;
    const int ww = (blockIdx.x % BPU) * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const PlaneCell pc0 = planeCell(a, dyn, (long long)a.unitList[unit] * 64 + ww * (64 / L) + lane / L);
    const float delay = pc0.inGrid ? a.delay[pc0.X * a.gy + pc0.Y] : FLT_MAX;
    const bool live = delay != FLT_MAX;
    if (__ballot(live) == 0ull) return;
    encodeGroups<L, false>(a, dyn, pc0, lane % L, live, live ? (int)delay : 0);
}

// every cell of the map: no onset (Analyzer.cpp:64-68), listener direction = towards the cell itself (a walk that
// finds no neighbour with a smaller delay stays where it is, Analyzer.cpp:365-391).  The window's cells are
// overwritten by the kernels that follow.
// Upper bound of the cells the pulse reached: the cells of the window's tiles that were ever non-zero.  Computed by
// block 0 of pv_far_cells_kernel (the first launch of the analysis); its result chooses, on the device, between the
// cell form (inside pv_encode_kernel) and the wave form of the wet gain / decay time.
__device__ __forceinline__ void countActiveCells(const AnalyzeArgs& a) {
    __shared__ int part[256];
    const DynParams dyn = *a.dyn;
    int n = 0;
    for (int i = threadIdx.x; i < dyn.histTilesX * dyn.histTilesY; i += 256) {
        const int ti = dyn.histTileX0 + i / dyn.histTilesY, tj = dyn.histTileY0 + i % dyn.histTilesY;
        if (a.tileFirst[ti * a.nty + tj] < a.T) n += a.rxi * a.wi;
    }
    part[threadIdx.x] = n;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.activeCount[0] = part[0];
        a.activeCount[1] = 0;
        a.activeCount[3] = 0;
        a.activeCount[4] = 0;
    }
}

__global__ __launch_bounds__(256) void pv_far_cells_kernel(const AnalyzeArgs a) {
    if (analysisAborted(a)) return;  // (grid-uniform)
    if (blockIdx.x == 0 && a.tileFirst) countActiveCells(a);  // (before any thread leaves: the reduction has barriers)
    const int index = blockIdx.x * blockDim.x + threadIdx.x;
    if (index >= a.gx * a.gy) return;
    a.delay[index] = FLT_MAX;
    storeDirection(a, index, index);
}

// The far-cell pass restricted to where something can have changed: blockIdx.z = 0 the previous run's window block,
// 1 this run's.  Every cell of both gets "no onset" and the default direction; the kernels that follow overwrite this
// run's reached cells.  All other cells of the map keep delay = FLT_MAX from the solver's creation / their own last reset,
// and their direction is made on demand (pv_far_dir_kernel, farDirectionOf).
__global__ __launch_bounds__(256) void pv_far_frame_kernel(const AnalyzeArgs a) {
    if (analysisAborted(a)) return;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && a.tileFirst) countActiveCells(a);
    const DynParams dyn = *a.dyn;
    int r0, c0, nr, nc;
    if (blockIdx.z == 0) {
        r0 = a.prevR0, c0 = a.prevC0, nr = a.prevNR, nc = a.prevNC;
    } else {
        r0 = dyn.histRow0 - a.G, c0 = dyn.histCol0 - a.G;
        nr = min(a.winRows, a.gx - r0), nc = min(a.winCols, a.gy - c0);
    }
    const int wc = blockIdx.x * blockDim.x + threadIdx.x, wr = blockIdx.y;
    if (wc >= nc || wr >= nr) return;
    const int index = (r0 + wr) * a.gy + (c0 + wc);
    a.delay[index] = FLT_MAX;
    storeDirection(a, index, index);
}

// the cells a listener-direction pass covers: one thread per cell of the window block -- with a near box only the cells inside
// it (the workgroups of the other rows and column blocks leave at once: a closed room's box is ~90 of the window's 3 500
// workgroups.  A bounded grid whose workgroups stride over the box was measured first: fine for that room, but an open field's
// box IS the window, and three cells per thread one after the other tripled these latency-bound passes -- 8192^2 open field
// analysis 0.41 -> 0.75 ms)
template <class F>
__device__ __forceinline__ void forDirectionCells(const AnalyzeArgs& a, const DynParams& dyn, F&& f) {
    int X, Y;
    if (!analysisWindowCell(a, dyn, &X, &Y)) return;
    if (a.box && !nearBoxOf(a, dyn).holds(X, Y)) return;
    f(X * a.gy + Y);
}

// (farDirectionOf / isFarCell: pv_analysis.h)

// materialise the direction planes of the far cells (whole-map read-backs)
__global__ __launch_bounds__(256) void pv_far_dir_kernel(float* __restrict__ dirX, float* __restrict__ dirY, long long n,
                                                         const FarInfo f) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !isFarCell(f, i)) return;
    float ox, oy;
    farDirectionOf(f, i, &ox, &oy);
    dirX[i] = ox;
    dirY[i] = oy;
}

void launchFarDirections(float* res, long long n, const FarInfo& f, hipStream_t stream) {
    hipLaunchKernelGGL(pv_far_dir_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, res + 4 * n, res + 5 * n, n, f);
}

void launchFillDelay(float* delay, long long n, hipStream_t stream);

__device__ __forceinline__ void directionWalkCell(const AnalyzeArgs& a, const int index) {
    float loudness = a.out[index];
    int cur = index;
    float delay = FLT_MAX;
    const float samplingRate = (float)a.fs;
    const float wavelength = kCDev / (float)a.res;
    const float thresholdDist = 0.3f * wavelength;

    while (delay > kDelayCloseDev && loudness < kDistanceGainDev) {
        const int r = cur / a.gy, c = cur - r * a.gy;
        float bestLoud = 0.f, bestDelay = FLT_MAX;
        for (int i = 0; i < 8; ++i) {
            const int nr = r + neighbourDr(i), nc = c + neighbourDc(i);
            if (nr < 0 || nc < 0 || nr >= a.gx || nc >= a.gy) continue;
            const int ni = nr * a.gy + nc;
            const float occ = a.out[ni];
            const float d = a.delay[ni];
            if (occ == 0.f) continue;               // Analyzer.cpp:372 (the (unsigned)delay test never fires)
            if (d < bestDelay && occ > 0.f) {       // strict <: first neighbour wins ties
                bestLoud = occ;
                cur = ni;                           // kept even if the step is rejected below (Analyzer.cpp:377)
                bestDelay = d;
            }
        }
        if (bestDelay == FLT_MAX || bestDelay >= delay) break;
        delay = bestDelay;
        loudness = bestLoud;
        // line-of-sight test, Analyzer.cpp:393-411
        const float geodesic = kCDev * bestDelay / samplingRate;
        const int r2 = cur / a.gy, c2 = cur - r2 * a.gy;
        const float tx = (float)r2 * a.dx - a.lx, ty = (float)c2 * a.dx - a.lz;
        const float euclid = sqrtf((tx * tx) + (ty * ty));
        if (fabsf(geodesic - euclid) < thresholdDist) break;
    }
    storeDirection(a, index, cur);
}
__global__ __launch_bounds__(256) void pv_direction_kernel(const AnalyzeArgs a) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    forDirectionCells(a, dyn, [&](const int index) { directionWalkCell(a, index); });
}

// listener direction by pointer jumping: the per-cell steps are dirInitCell / dirJumpCell / dirFinalCell (pv_analysis_dev.h)
__global__ __launch_bounds__(256) void pv_dir_init_kernel(const AnalyzeArgs a, int* J) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    forDirectionCells(a, dyn, [&](const int p) { dirInitCell<false>(a, dyn, J, p); });
}

__global__ __launch_bounds__(256) void pv_dir_jump_kernel(const AnalyzeArgs a, int* J) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    forDirectionCells(a, dyn, [&](const int p) { dirJumpCell<false>(a, dyn, J, p); });
}

__global__ __launch_bounds__(256) void pv_dir_final_kernel(const AnalyzeArgs a, const int* J) {
    if (analysisAborted(a)) return;
    const DynParams dyn = *a.dyn;
    forDirectionCells(a, dyn, [&](const int p) { dirFinalCell<false>(a, dyn, J, p); });
}

static dim3 analysisWindowGrid(const AnalyzeArgs& a) { return dim3((a.winCols + 255) / 256, a.winRows); }

static void launchDirectionJump(const AnalyzeArgs& a, int* J, hipStream_t stream) {
    const dim3 grid = analysisWindowGrid(a), block(256);
    hipLaunchKernelGGL(pv_dir_init_kernel, grid, block, 0, stream, a, J);
    for (int i = 0; i < dirJumpPasses(a.T); ++i) hipLaunchKernelGGL(pv_dir_jump_kernel, grid, block, 0, stream, a, J);
    hipLaunchKernelGGL(pv_dir_final_kernel, grid, block, 0, stream, a, J);
}

__global__ void pv_fill_delay_kernel(float* delay, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) delay[i] = FLT_MAX;  // Analyzer.cpp:64-68
}

// far cells of the whole map (delay = FLT_MAX, default listener direction): the first analysis launch
void launchFarCells(const AnalyzeArgs& a, hipStream_t stream) {
    const int n = a.gx * a.gy;
    hipLaunchKernelGGL(pv_far_cells_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
}

// onset, dry gain, source directivity, lowpass, wet gain, decay time of the window's cells (everything but the listener
// direction, which needs the delay / occlusion maps of the WHOLE window: launchAnalysisDirection)
void launchOnset(const AnalyzeArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pv_onset_kernel, dim3((unsigned)((a.histPlane + 63) / 64)), dim3(64 * kOnsetWaves), 0, stream, a);
}
void launchEncode(const AnalyzeArgs& a, hipStream_t stream) {
    // lanes per cell by the window's size (an upper bound of the cells with work): sixteen where a cell's walk IS the kernel's
    // duration, four up to the sizes the four-lane decay-time form serves, one (which then also takes the wet gain beside the
    // lane-per-cell decay-time form) above
    const unsigned units = (unsigned)((a.histPlane + 63) / 64);
    if (a.rt60Lanes != 1 && a.histPlane <= 16384)
        hipLaunchKernelGGL(pv_encode_groups_kernel<16>, dim3(units * 4), dim3(256), 0, stream, a);
    else if (a.rt60Lanes != 1 && a.histPlane <= kRt60TileMinCells)
        hipLaunchKernelGGL(pv_encode_groups_kernel<4>, dim3(units), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(pv_encode_kernel, dim3((unsigned)((a.histPlane + 255) / 256)), dim3(256), 0, stream, a);
}
// wet gain + decay time (pv_rt60.hip): the form is decided on the device from the number of cells with an onset
void launchRt60(const AnalyzeArgs& a, hipStream_t stream) { launchRt60Forms(a, stream); }

void launchAnalysisCells(const AnalyzeArgs& a, hipStream_t stream) {
    launchOnset(a, stream);
    launchEncode(a, stream);
    launchRt60(a, stream);
}

void launchAnalysisDirection(const AnalyzeArgs& a, hipStream_t stream) {
    const dim3 grid = analysisWindowGrid(a);
    // (the whole pass in ONE workgroup with the table in LDS -- no kernel boundaries between init, jumps and final -- was built and
    // measured for the windows of up to 16 384 cells: 25-80 us slower, one CU's memory pipeline does the 17 loads per cell of
    // init and final for everybody: docs/experiments/fused_analysis.md)
    if (a.dirJump)
        launchDirectionJump(a, a.dirScratch, stream);
    else
        hipLaunchKernelGGL(pv_direction_kernel, grid, dim3(256), 0, stream, a);
}

void launchFillDelay(float* delay, long long n, hipStream_t stream) {
    hipLaunchKernelGGL(pv_fill_delay_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, delay, (int)n);
}

void launchAnalysisFar(const AnalyzeArgs& a, hipStream_t stream) {
    if (a.wholeWindow || a.box) return;  // (no far-cell pass: pv_onset_kernel does what is left of it)
    const int n = a.gx * a.gy;
    if (a.lazyFar) {
        const int nr = max(a.prevNR, min(a.winRows, a.gx)), nc = max(a.prevNC, min(a.winCols, a.gy));
        hipLaunchKernelGGL(pv_far_frame_kernel, dim3((unsigned)((max(nc, 1) + 255) / 256), (unsigned)max(nr, 1), 2), dim3(256), 0,
                           stream, a);
    } else {
        hipLaunchKernelGGL(pv_far_cells_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
    }
}

void launchAnalysis(const AnalyzeArgs& a, hipStream_t stream) {
    launchAnalysisFar(a, stream);
    launchAnalysisCells(a, stream);
    // listener direction: the plain walk where walks are short (small windows: rooms, the sandbox's grids), pointer
    // jumping where a window is wide enough for hundreds of steps (a dozen tiny launches, path-length independent)
    launchAnalysisDirection(a, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// streaming analysis (sparse-emitter mode)
// ---------------------------------------------------------------------------------------------------------------
// With T in the tens of thousands (a 25 m scene at a 4096^2 grid: T = 25432) the full pressure history cannot be
// kept.  What needs ALL of a cell's samples is only the wet gain and the RT60 regression; onset, dry energy and
// flux are forward sums that close N_dry samples after the onset.  So the history becomes a ring of `ring` planes;
// after every `ring` steps pv_stream_accum_kernel advances the forward sums of every open cell in the reference's
// sample order (state carried in per-cell planes), and the pressure of the REGISTERED emitter cells is copied to
// per-emitter traces, from which wet gain and RT60 are computed at the end exactly as pv_encode_kernel does.

__global__ __launch_bounds__(256) void pv_stream_accum_kernel(const AnalyzeArgs a) {
    int X, Y;
    if (a.ringList) {
        // forward sums of the air tiles inside the stencil (pv_stream.h): this pass serves only the listed tiles (walls, grid
        // edges, listener, registered emitters) -- blockIdx.x = list entry * chunks + 256-cell chunk of the tile (a grid's y
        // extent stops at 65 535: a 16k^2 scene with many wall tiles has more list entries than that)
        const int chunks = (a.rxi * a.wi + 255) / 256;
        const int entry = blockIdx.x / chunks;
        const int t = a.ringList[entry];
        const int idx = (blockIdx.x - entry * chunks) * blockDim.x + threadIdx.x;
        if (idx >= a.rxi * a.wi) return;
        const int ti = t / a.nty, r = idx / a.wi;
        X = ti * a.rxi + r;
        Y = (t - ti * a.nty) * a.wi + (idx - r * a.wi);
    } else {
        Y = blockIdx.x * blockDim.x + threadIdx.x;
        X = blockIdx.y;
    }
    if (Y >= a.gy || X >= a.gx) return;
    const int s = X * a.gy + Y;
    const DynParams dyn = *a.dyn;
    const int tile = (X / a.rxi) * a.nty + (Y / a.wi);
    // tiles whose sums advance inside the stencil (pv_stream.h) are not this pass's business
    if (a.fuseClass && !a.ringList &&
        fusedTile(a.fuseClass, a.fuseEmit, dyn, X / a.rxi, Y / a.wi, a.nty, a.G, a.fuseK, a.rxi, a.wi, a.rxi + 2 * a.fuseK, 1))
        return;
    const int tFirst = a.tileFirst[tile];
    if (tFirst == INT_MAX || tFirst >= a.tB) return;
    int onset = a.sOnset[s];
    int sourceDirEnd = onset >= 0 ? onset + a.nDir : INT_MAX;
    int directEnd = onset >= 0 ? onset + a.nDry : INT_MAX;
    if (a.tA >= directEnd) return;  // this cell's dry window is closed
    // a wall cell's pressure is identically zero: it never has an onset and must not keep its tile recording
    if (a.coef[(size_t)(X + a.G) * a.pitch + (Y + a.G)].beta == 0.f) return;

    const int prow = X + a.G, pcol = Y + a.G;
    const int hr = prow - dyn.histRow0, hcol = pcol - dyn.histCol0;
    const long long hoff = histOffset(hr, hcol, a.rxi, a.wi, dyn.histTilesY);
    int tFx = INT_MAX, tFy = INT_MAX;
    if (X > 0 && prow - 1 >= dyn.histRow0) tFx = a.tileFirst[((X - 1) / a.rxi) * a.nty + (Y / a.wi)];
    if (Y > 0 && pcol - 1 >= dyn.histCol0) tFy = a.tileFirst[(X / a.rxi) * a.nty + ((Y - 1) / a.wi)];
    const float* hc = a.hist + hoff;
    const float* hx = a.hist + (tFx != INT_MAX ? histOffset(hr - 1, hcol, a.rxi, a.wi, dyn.histTilesY) : hoff);
    const float* hy = a.hist + (tFy != INT_MAX ? histOffset(hr, hcol - 1, a.rxi, a.wi, dyn.histTilesY) : hoff);
    const FaceCoef fc = a.coef[(size_t)prow * a.pitch + pcol];
    const float kx = fc.kx, ky = fc.ky;
    const bool airX = kx != kx, airY = ky != ky;
    const float C = a.courant;

    float Edry = a.sEdry[s], fluxX = a.sFx[s], fluxY = a.sFy[s], vx = a.sVx[s], vy = a.sVy[s];
    constexpr int CH = 8;
    bool done = false;
    const int tEnd = min(a.tB, a.T);
    for (int t0 = max(a.tA, tFirst); t0 < tEnd && !done; t0 += CH) {
        float pc[CH], pxc[CH], pyc[CH];
        const bool needVChunk = t0 < sourceDirEnd;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int tt = min(t0 + k, tEnd - 1);
            const long long o = (long long)(tt % a.ring) * a.histPlane;
            pc[k] = hc[o];
            pxc[k] = (needVChunk && tt >= tFx) ? hx[o] : 0.f;
            pyc[k] = (needVChunk && tt >= tFy) ? hy[o] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            if (done || t >= tEnd || t >= directEnd) {
                done = done || t >= directEnd;
                continue;
            }
            const float p = pc[k];
            if (t < sourceDirEnd) {
                const float pxn = pxc[k], pyn = pyc[k];
                const float ax = vx - C * (p - pxn), wx = kx * (p + pxn);
                const float ay = vy - C * (p - pyn), wy = ky * (p + pyn);
                vx = airX ? ax : wx;
                vy = airY ? ay : wy;
            }
            if (onset < 0 && fabsf(p) > kAudibleThresholdDev) {
                onset = t;
                sourceDirEnd = t + a.nDir;
                directEnd = t + a.nDry;
                if (t >= directEnd) {
                    done = true;
                    continue;
                }
            }
            Edry += p * p;
            if (t < sourceDirEnd) {
                fluxX += p * vx;
                fluxY += p * vy;
            }
        }
    }
    // still open after this pass?  (no onset yet, or the dry window reaches past tB) -> keep the tile recording
    if (onset < 0 || a.tB < directEnd) a.tileOpenOut[tile] = 1;
    a.sOnset[s] = onset;
    a.sEdry[s] = Edry;
    a.sFx[s] = fluxX;
    a.sFy[s] = fluxY;
    a.sVx[s] = vx;
    a.sVy[s] = vy;
}

// pressure of the registered emitter cells for steps [tA, tB): ring -> per-emitter trace
__global__ void pv_stream_trace_kernel(const AnalyzeArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = a.tB - a.tA;
    if (i >= a.numEmitters * n) return;
    const int e = i / n, t = a.tA + (i - e * n);
    if (t >= a.T) return;
    const DynParams dyn = *a.dyn;
    const int cell = a.emCells[e];
    const int X = cell / a.gy, Y = cell - X * a.gy;
    const int tFirst = a.tileFirst[(X / a.rxi) * a.nty + (Y / a.wi)];
    float v = 0.f;
    if (t >= tFirst)
        v = a.hist[(long long)(t % a.ring) * a.histPlane +
                   histOffset(X + a.G - dyn.histRow0, Y + a.G - dyn.histCol0, a.rxi, a.wi, dyn.histTilesY)];
    a.emTrace[(size_t)e * a.T + t] = v;
}

// The same pass for the record traces (AnalyzeArgs::recTrace): plane t of recCols x (1 or 3) columns, lanes along the columns so
// that a step's stores are consecutive.  Column part 0 = the emitters' own cells, parts 1 / 2 = their neighbours (X - 1, Y) /
// (X, Y - 1), each zero before its own tile's first step; a neighbour outside the window (traceNeighbours) and a column without
// an emitter stay zero
__global__ __launch_bounds__(256) void pv_stream_rectrace_kernel(const AnalyzeArgs a) {
    const int plane = a.recCols * (a.recVel ? 3 : 1);
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = a.tA + (int)blockIdx.y;
    if (c >= plane || t >= a.tB || t >= a.T) return;
    const int part = c / a.recCols, e = c - part * a.recCols;
    float v = 0.f;
    if (e < a.numEmitters) {
        const DynParams dyn = *a.dyn;
        const int cell = a.emCells[e];
        int X = cell / a.gy, Y = cell - X * a.gy;
        bool hasX, hasY;
        traceNeighbours(a, dyn, X, Y, &hasX, &hasY);
        const bool has = part == 0 || (part == 1 ? hasX : hasY);
        if (part == 1) --X;
        if (part == 2) --Y;
        if (has && t >= a.tileFirst[(X / a.rxi) * a.nty + (Y / a.wi)])
            v = a.hist[(long long)(t % a.ring) * a.histPlane +
                       histOffset(X + a.G - dyn.histRow0, Y + a.G - dyn.histCol0, a.rxi, a.wi, dyn.histTilesY)];
    }
    a.recTrace[(long long)t * plane + c] = v;
}

// end of run: onset map + the outputs that come from the forward sums (Analyzer.cpp:197-230), every cell
__global__ __launch_bounds__(256) void pv_stream_finalize_kernel(const AnalyzeArgs a) {
    const int Y = blockIdx.x * blockDim.x + threadIdx.x;
    const int X = blockIdx.y;
    if (Y >= a.gy || X >= a.gx) return;
    const int s = X * a.gy + Y;
    const int onset = a.sOnset[s];
    if (onset < 0) {
        a.delay[s] = FLT_MAX;
        return;
    }
    a.delay[s] = (float)onset;
    const float Edry = a.sEdry[s], fluxX = a.sFx[s], fluxY = a.sFy[s];
    const float EfreePr = efreePerR(a.efree, a.dx, a.lcx, a.lcy, X, Y);
    const float occ = sqrtf(Edry / EfreePr);
    float norm = sqrtf(fluxX * fluxX + fluxY * fluxY);
    norm = -1.0f / (norm > 0.0f ? norm : 1.0f);
    const float rr = 1.0f / ((0.001f < occ) ? occ : 0.001f);
    a.out[s] = occ;
    a.out[3 * a.resN + s] = -147.f + (18390.f) / (1.f + pvPowf(rr / 12.f, 0.8f));
    a.out[6 * a.resN + s] = norm * fluxX;
    a.out[7 * a.resN + s] = norm * fluxY;
}

// wet gain + RT60 of the registered emitter cells from their traces (Analyzer.cpp:235-327); one thread each
__global__ void pv_stream_emitter_kernel(const AnalyzeArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.numEmitters) return;
    const int s = a.emCells[e];
    const int onset = a.sOnset[s];
    if (onset < 0) return;
    const float* tr = a.emTrace + (size_t)e * a.T;
    const int T = a.T;
    const int directEnd = onset + a.nDry;
    float wetEnergy = 0.f;
    {
        int end = directEnd + 1 + a.nWet;
        if (T < end) end = T;
        for (int j = directEnd + 1; j < end; ++j) wetEnergy += tr[j] * tr[j];
    }
    const int startingPoint = directEnd + 1;
    const int endPoint = T - a.nCut;
    const float rn = (float)(endPoint - startingPoint);
    const float xmean = (rn - 1.0f) * 0.5f;
    const float xsum = rn * xmean;
    const float denominator = (1.0f / 12.0f) * rn * (rn * rn - 1.0f);
    float edc = 0.f, xysum = 0.f, ysum = 0.f;
    for (int i = T - 1; i >= endPoint && i >= 0; --i) edc += tr[i] * tr[i];
    constexpr int CH = 8;
    for (int i0 = endPoint - 1; i0 >= startingPoint; i0 -= CH) {
        float pc[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) pc[k] = tr[max(i0 - k, 0)];
        rt60Chunk<CH>(pc, i0, startingPoint, edc, xysum, ysum);
    }
    const float ymean = ysum / rn;
    const float numerator = xysum - ymean * xsum - xmean * ysum + rn * xmean * ymean;
    const float slopePerSec = (numerator / denominator) * (float)a.fs;
    a.out[a.resN + s] = sqrtf(wetEnergy / a.efree);
    a.out[2 * a.resN + s] = -60.f / slopePerSec;
}

// tileOpen[tile] for the next launches: some cell marked it open in this pass, or the wave has not reached it yet,
// or it holds a registered emitter (its whole trace is needed) or a cell of a zone whose curve is accumulated (every step of it is)
__global__ void pv_stream_tilegate_kernel(const uint8_t* marks, const uint8_t* hasEmitter, const int* tileFirst, int tB,
                                          uint8_t* tileOpen, int ntiles) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < ntiles) tileOpen[t] = (marks[t] || hasEmitter[t] || tileFirst[t] >= tB) ? 1 : 0;
}

void launchStreamAccum(const AnalyzeArgs& a, const uint8_t* hasEmitter, uint8_t* tileOpen, int ntiles,
                       hipStream_t stream, const ZoneRingCurveArgs* zc, int zcChunk, const ZoneMapArgs* zm,
                       const ZoneMapSpecSlice* zmSlices, int zmSliceCount) {
    dim3 grid((a.gy + 255) / 256, a.gx);
    if (a.ringList) grid = dim3((unsigned)((a.rxi * a.wi + 255) / 256) * (unsigned)(a.numRing > 0 ? a.numRing : 1), 1);
    hipMemsetAsync(a.tileOpenOut, 0, (size_t)ntiles, stream);
    if (!a.ringList || a.numRing > 0) hipLaunchKernelGGL(pv_stream_accum_kernel, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(pv_stream_tilegate_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, stream, a.tileOpenOut,
                       hasEmitter, a.tileFirst, a.tB, tileOpen, ntiles);
    const int n = a.numEmitters * (a.tB - a.tA);
    if (n > 0) hipLaunchKernelGGL(pv_stream_trace_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a);
    if (n > 0 && a.recTrace)
        hipLaunchKernelGGL(pv_stream_rectrace_kernel, dim3((unsigned)((a.recCols * (a.recVel ? 3 : 1) + 255) / 256), (unsigned)(a.tB - a.tA)),
                           dim3(256), 0, stream, a);
    // the zones' curves of this pass's steps: behind the accumulate kernel, whose onsets decide the members, and -- as everything
    // in here -- in front of the event that hands the half ring back to the step kernels
    if (zc) launchStreamZoneCurves(*zc, a.tA, a.tB, zcChunk, stream);
    // the labelled cells' map sums of this pass's steps: the same two conditions
    if (zm) {
        ZoneMapArgs m = *zm;
        m.tA = a.tA;
        m.tB = a.tB;
        launchStreamZoneMaps(m, zmSlices, zmSliceCount, stream);
    }
}

void launchStreamFinalize(const AnalyzeArgs& a, hipStream_t stream) {
    dim3 grid((a.gy + 255) / 256, a.gx);
    const int n = a.gx * a.gy;
    hipLaunchKernelGGL(pv_fill_delay_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a.delay, n);
    hipLaunchKernelGGL(pv_stream_finalize_kernel, grid, dim3(256), 0, stream, a);
    if (a.numEmitters > 0)
        hipLaunchKernelGGL(pv_stream_emitter_kernel, dim3((a.numEmitters + 63) / 64), dim3(64), 0, stream, a);
    // T is large in this mode: resolve the delay-map descent by pointer jumping (the window is the whole grid here)
    launchDirectionJump(a, a.dirScratch, stream);
}

}  // namespace pva
