// pv_copy.hip -- read-back and copy kernels: result records (pack, gather), history rows / planes / one cell's impulse response,
// block copies and halo pushes between slabs, the free-field energy sum, dense <-> padded planes.
//
// Reference semantics implemented here (paths relative to the reference's ProjectPlaneverb directory):
//   pv_efree_kernel     src/FDTD/FreeGrid.cpp:96-110  free-field energy sum
//   pv_ir_kernel        src/FDTD/FDTD.cpp:60-79       impulse response (pr, vx, vy) of one cell
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_prims.h"
namespace pva {

// SoA result planes -> the reference's array of PlaneverbOutput structs (AnalyzerResult, Analyzer.h:11-22)
__global__ void pv_pack_results_kernel(const float* __restrict__ res, long long n, float* __restrict__ res8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 lo = make_float4(res[i], res[n + i], res[2 * n + i], res[3 * n + i]);
    float4 hi = make_float4(res[4 * n + i], res[5 * n + i], res[6 * n + i], res[7 * n + i]);
    reinterpret_cast<float4*>(res8)[2 * i] = lo;
    reinterpret_cast<float4*>(res8)[2 * i + 1] = hi;
}

// the nr x nc block of the result map whose first cell is (r0, c0) as AoS records (the live module publishes only
// the history window's block of every iteration: everything outside it is stale values + a closed-form direction)
__global__ void pv_pack_window_kernel(const float* __restrict__ res, long long n, int gy, int r0, int c0, int nr, int nc,
                                      float* __restrict__ out8, const FarInfo f) {
    const int wc = blockIdx.x * blockDim.x + threadIdx.x, wr = blockIdx.y;
    if (wc >= nc || wr >= nr) return;
    const long long i = (long long)(r0 + wr) * gy + (c0 + wc);
    const long long o = (long long)wr * nc + wc;
    float4 lo = make_float4(res[i], res[n + i], res[2 * n + i], res[3 * n + i]);
    float4 hi = make_float4(res[4 * n + i], res[5 * n + i], res[6 * n + i], res[7 * n + i]);
    if (isFarCell(f, i)) farDirectionOf(f, i, &hi.x, &hi.y);  // (a far cell: its direction is not in the planes)
    reinterpret_cast<float4*>(out8)[2 * o] = lo;
    reinterpret_cast<float4*>(out8)[2 * o + 1] = hi;
}

void launchPackWindow(const float* res, long long n, int gy, int r0, int c0, int nr, int nc, float* out8, const FarInfo& far,
                      hipStream_t stream) {
    if (nr <= 0 || nc <= 0) return;
    hipLaunchKernelGGL(pv_pack_window_kernel, dim3((unsigned)((nc + 255) / 256), (unsigned)nr), dim3(256), 0, stream, res,
                       n, gy, r0, c0, nr, nc, out8, far);
}

// one cell of the result map -> 8 floats in pinned host memory (Analyzer::GetResponseResult, Analyzer.cpp:106-116)
__global__ void pv_gather_output_kernel(const float* __restrict__ res, long long n, long long cell, float* out8,
                                        const FarInfo f) {
    if (threadIdx.x < 8) {
        float v = res[threadIdx.x * n + cell];
        if ((threadIdx.x == 4 || threadIdx.x == 5) && isFarCell(f, cell)) {  // a far cell: its direction is not in the planes
            float ox, oy;
            farDirectionOf(f, cell, &ox, &oy);
            v = threadIdx.x == 4 ? ox : oy;
        }
        out8[threadIdx.x] = v;
    }
}

void launchGatherOutput(const float* res, long long n, long long cell, float* out8Host, const FarInfo& f, hipStream_t stream) {
    hipLaunchKernelGGL(pv_gather_output_kernel, dim3(1), dim3(64), 0, stream, res, n, cell, out8Host, f);
}

// the registered output queries of a run (PvAmdSetOutputQueries): nq result cells -> nq x 8 floats in pinned host
// memory, enqueued behind the analysis so that the caller's one stream sync also delivers the outputs.
// cells[] lives in pinned host memory too (cell < 0: position outside the result map, left to the host's sentinel)
__global__ void pv_gather_queries_kernel(const float* __restrict__ res, long long n, const long long* cells, int nq,
                                         float* out, const FarInfo f) {
    const int q = threadIdx.x >> 3, k = threadIdx.x & 7;
    if (q < nq) {
        const long long c = cells[q];
        float v = c >= 0 ? res[k * n + c] : 0.f;
        if (c >= 0 && (k == 4 || k == 5) && isFarCell(f, c)) {
            float ox, oy;
            farDirectionOf(f, c, &ox, &oy);
            v = k == 4 ? ox : oy;
        }
        out[q * 8 + k] = v;
    }
}

void launchGatherQueries(const float* res, long long n, const long long* cellsHost, int nq, float* outHost, const FarInfo& f,
                         hipStream_t stream) {
    hipLaunchKernelGGL(pv_gather_queries_kernel, dim3(1), dim3(512), 0, stream, res, n, cellsHost, nq, outHost, f);
}

void launchPackResults(const float* res, long long n, float* res8, hipStream_t stream) {
    hipLaunchKernelGGL(pv_pack_results_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, res, n, res8);
}

// One row of the history window over all T steps as a dense [T][histPitch] array (zeros where the tile had not been
// reached yet): what the slab BELOW this one needs for the vx recurrence of its first row (AnalyzeArgs::histAbove).
__global__ void pv_hist_row_kernel(const AnalyzeArgs a, int X, float* __restrict__ out) {
    const int wc = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (wc >= a.histPitch || t >= a.T) return;
    const DynParams dyn = *a.dyn;
    const int pcol = dyn.histCol0 + wc, prow = X + a.G;
    float v = 0.f;
    const int ti = X / a.rxi, tj = (pcol - a.G) / a.wi;
    const int wti = ti - dyn.histTileX0, wtj = tj - dyn.histTileY0;
    if (wc < a.winCols && pcol >= a.G && wti >= 0 && wti < dyn.histTilesX && wtj >= 0 && wtj < dyn.histTilesY &&
        t >= a.tileFirst[ti * a.nty + tj])
        v = a.hist[(long long)t * a.histPlane + histOffset(prow - dyn.histRow0, wc, a.rxi, a.wi, dyn.histTilesY)];
    out[(long long)t * a.histPitch + wc] = v;
}

void launchHistRow(const AnalyzeArgs& a, int X, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(pv_hist_row_kernel, dim3((a.histPitch + 255) / 256, a.T), dim3(256), 0, stream, a, X, out);
}

// nplanes planes: the nr x nc block at (sr0, sc0) of src planes (row pitch spitch, plane stride sstride) into the block at
// (dr0, dc0) of dst planes -- a slab's part of the history window into the whole grid's result / delay maps
__global__ void pv_copy_block_kernel(const float* __restrict__ src, long long sstride, int spitch, int sr0, int sc0,
                                     float* __restrict__ dst, long long dstride, int dpitch, int dr0, int dc0, int nr,
                                     int nc, const int* srcPlanes, const int* dstPlanes, const unsigned* abortWord) {
    if (abortWord && *abortWord != 0u) return;  // (AnalyzeArgs::abortWord)
    const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    const int ks = srcPlanes ? srcPlanes[blockIdx.z] : blockIdx.z, kd = dstPlanes ? dstPlanes[blockIdx.z] : blockIdx.z;
    if (c >= nc || r >= nr) return;
    dst[kd * dstride + (long long)(dr0 + r) * dpitch + dc0 + c] = src[ks * sstride + (long long)(sr0 + r) * spitch + sc0 + c];
}

void launchCopyBlock(const float* src, long long sstride, int spitch, int sr0, int sc0, float* dst, long long dstride,
                     int dpitch, int dr0, int dc0, int nr, int nc, int nplanes, const int* srcPlanesDev,
                     const int* dstPlanesDev, hipStream_t stream, const unsigned* abortWord) {
    if (nr <= 0 || nc <= 0) return;
    hipLaunchKernelGGL(pv_copy_block_kernel, dim3((unsigned)((nc + 255) / 256), (unsigned)nr, (unsigned)nplanes), dim3(256),
                       0, stream, src, sstride, spitch, sr0, sc0, dst, dstride, dpitch, dr0, dc0, nr, nc, srcPlanesDev,
                       dstPlanesDev, abortWord);
}

// Slab decomposition (pv_slabs.cpp): after a K-step launch a slab PUSHES the K rows next to each of its boundaries into the
// neighbour's guard band -- one launch for all six blocks (3 planes x 2 directions) instead of six hipMemcpyAsync on the
// receiver's stream (each a 5 us copy kernel of its own: 20-85 us per sweep in round 2).  Every block is K whole padded
// rows = a contiguous run of floats (a multiple of 64); the destination may live on another device (peer access is
// enabled by the group: plain stores over xGMI).
struct HaloPushArgs {
    const float* src[6];
    float* dst[6];
    long long n;  // floats per block
    HaloHandoff h;
};
// Device-side hand-off between slabs on ONE device (HaloHandoff, pv_device.h).  A cross-queue event wait per slab and sweep
// costs ~50 us on this runtime (the waiting queue is parked until the command processor looks at it again: a 2048^2 run with two
// slabs took 95 us per sweep for 37 us of stencil, profiles/r04_slabs.txt); a word in memory costs 2-3 us.  So the push kernel
// of sweep li (a) copies its rows, (b) fence + count: the block that completes the count raises the words its neighbours
// look at to li + 1, (c) that same block then waits until the slab's own words -- raised by the neighbours' pushes of the
// same sweep -- have reached li + 1.  The slab's next step launch follows in stream order: behind the neighbours' halos,
// without an event.  (Write-after-read: a neighbour's push of sweep li comes behind its step li, which came behind its wait
// for THIS slab's push li - 1, which came behind this slab's step li - 1 -- the last reader of the guard rows it overwrites.)
// One wave spins, bounded; the others leave: the neighbours' kernels never lack a place to run.
__global__ __launch_bounds__(256) void pv_halo_push_kernel(const HaloPushArgs h) {
    typedef unsigned int v4u __attribute__((__vector_size__(16)));
    const int b = blockIdx.y;
    const bool hand = h.h.count != nullptr;
    if (h.dst[b]) {
        // (with the hand-off the rows are written THROUGH to memory -- sc1 -- so that nothing has to be flushed before the word
        // is raised: a release fence here writes back and invalidates the whole L2 under the other slab's running step kernel,
        // measured 65 us per sweep)
        const rsrc_t rs = makeRsrc(h.src[b], h.n * 4), rd = makeRsrc(h.dst[b], h.n * 4);
        const int n4 = (int)(h.n >> 2);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
            const v4u v = __builtin_amdgcn_raw_buffer_load_b128(rs, i * 16, 0, 0);
            if (hand)
                __builtin_amdgcn_raw_buffer_store_b128(v, rd, i * 16, 0, 16 /* sc1 */);
            else
                __builtin_amdgcn_raw_buffer_store_b128(v, rd, i * 16, 0, 0);
        }
    }
    if (!hand) return;
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this thread's rows are in memory
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned nblocks = gridDim.x * gridDim.y;
    if (__hip_atomic_fetch_add(h.h.count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u != h.h.seq * nblocks) return;
    for (int i = 0; i < 2; ++i)
        if (h.h.raise[i]) __hip_atomic_store(h.h.raise[i], h.h.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int i = 0; i < 2; ++i) {
        if (!h.h.await[i]) continue;
        int spins = 0;
        while (__hip_atomic_load(h.h.await[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < h.h.seq) {
            __builtin_amdgcn_s_sleep(2);
            if (++spins > (1 << 19)) {  // (~0.5 s: a neighbour whose launches do not run beside this one must not hang the device;
                                        // SlabGroup::run then repeats the run with events -- the abort word keeps this run's
                                        // analysis away from the result maps)
                atomicExch(h.h.err, 5);
                if (h.h.abortWord) __hip_atomic_store(h.h.abortWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
        }
    }
}

void launchHaloPush(const float* const src[6], float* const dst[6], long long n, const HaloHandoff& hand, hipStream_t stream) {
    HaloPushArgs h;
    for (int i = 0; i < 6; ++i) {
        h.src[i] = src[i];
        h.dst[i] = dst[i];
    }
    h.n = n;
    h.h = hand;
    const unsigned bx = (unsigned)std::min<long long>(64, (n / 4 + 255) / 256);
    hipLaunchKernelGGL(pv_halo_push_kernel, dim3(bx, 6), dim3(256), 0, stream, h);
}

// FreeGrid::CalculateEFree + SimulateFreeFieldEnergy tail, FreeGrid.cpp:86-110: sequential float sum of p^2 over
// the first n samples at one cell, times the discrete distance r.
__global__ void pv_efree_kernel(const float* hist, long long plane, long long cellOff, int n, float r,
                                float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float e = 0.f;
    for (int i = 0; i < n; ++i) {
        const float p = hist[(long long)i * plane + cellOff];
        e += p * p;
    }
    out[0] = e * r;
}

void launchEfree(const float* hist, long long plane, long long cellOff, int n, float r, float* out,
                 hipStream_t stream) {
    hipLaunchKernelGGL(pv_efree_kernel, dim3(1), dim3(64), 0, stream, hist, plane, cellOff, n, r, out);
}

// Grid::GetResponse, FDTD.cpp:74-79: the (pr, vx, vy) impulse response of one array cell, rebuilt from the
// pressure history (see pv_encode_kernel).  out = T x 3 floats.
__global__ void pv_ir_kernel(const AnalyzeArgs a, int X, int Y, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const DynParams dyn = *a.dyn;
    const int prow = X + a.G, pcol = Y + a.G;
    const int tj = (Y / a.wi), ti = (X / a.rxi);
    const int wti = ti - dyn.histTileX0, wtj = tj - dyn.histTileY0;
    const bool inWin = wti >= 0 && wti < dyn.histTilesX && wtj >= 0 && wtj < dyn.histTilesY;
    const int tFirst = inWin ? a.tileFirst[ti * a.nty + tj] : INT_MAX;
    const long long hoff = inWin ? histOffset(prow - dyn.histRow0, pcol - dyn.histCol0, a.rxi, a.wi, dyn.histTilesY) : 0;
    int tFx = INT_MAX, tFy = INT_MAX;
    if (X > 0 && prow - 1 >= dyn.histRow0) tFx = a.tileFirst[((X - 1) / a.rxi) * a.nty + tj];
    if (Y > 0 && pcol - 1 >= dyn.histCol0) tFy = a.tileFirst[ti * a.nty + ((Y - 1) / a.wi)];
    const long long hoffX = tFx != INT_MAX ? histOffset(prow - 1 - dyn.histRow0, pcol - dyn.histCol0, a.rxi, a.wi, dyn.histTilesY) : 0;
    const long long hoffY = tFy != INT_MAX ? histOffset(prow - dyn.histRow0, pcol - 1 - dyn.histCol0, a.rxi, a.wi, dyn.histTilesY) : 0;
    const FaceCoef fc = a.coef[(size_t)prow * a.pitch + pcol];
    const float kx = fc.kx, ky = fc.ky;
    const bool airX = kx != kx, airY = ky != ky;
    const bool above = X == 0 && a.histAbove;  // first row of a slab: the row above lives in the neighbouring slab
    float vx = 0.f, vy = 0.f;
    for (int t = 0; t < a.T; ++t) {
        float p = 0.f;
        if (t >= tFirst) {
            p = a.hist[(long long)t * a.histPlane + hoff];
            const float pxn = above ? a.histAbove[(long long)t * a.histPitch + (pcol - dyn.histCol0)]
                                    : (t >= tFx) ? a.hist[(long long)t * a.histPlane + hoffX] : 0.f;
            const float pyn = (t >= tFy) ? a.hist[(long long)t * a.histPlane + hoffY] : 0.f;
            const float ax = vx - a.courant * (p - pxn), wx = kx * (p + pxn);
            const float ay = vy - a.courant * (p - pyn), wy = ky * (p + pyn);
            vx = airX ? ax : wx;
            vy = airY ? ay : wy;
        }
        out[3 * t + 0] = p;
        out[3 * t + 1] = vx;
        out[3 * t + 2] = vy;
    }
}

void launchIr(const AnalyzeArgs& a, int X, int Y, float* out, hipStream_t stream) {
    hipLaunchKernelGGL(pv_ir_kernel, dim3(1), dim3(64), 0, stream, a, X, Y, out);
}

// gather / scatter between the reference's dense (gx+1)x(gy+1) order and the padded device planes
__global__ void pv_unpad_kernel(const float* padded, float* dense, Geometry g) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    const int x = blockIdx.y;
    if (y < g.NY && x < g.NX) dense[(size_t)x * g.NY + y] = padded[(size_t)(x + g.G) * g.pitch + (y + g.G)];
}
__global__ void pv_pad_kernel(const float* dense, float* padded, Geometry g) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    const int x = blockIdx.y;
    if (y < g.NY && x < g.NX) padded[(size_t)(x + g.G) * g.pitch + (y + g.G)] = dense[(size_t)x * g.NY + y];
}
// recorded pressure plane t -> dense order, zero where nothing was stored
__global__ void pv_histplane_kernel(const AnalyzeArgs a, int t, float* dense, int NX, int NY, int histRows) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    const int x = blockIdx.y;
    if (y >= NY || x >= NX) return;
    const DynParams dyn = *a.dyn;
    const int hr = x + a.G - dyn.histRow0, hcn = y + a.G - dyn.histCol0;
    float v = 0.f;
    if (hr >= 0 && hr < histRows && hcn >= 0 && hcn < dyn.histTilesY * a.wi) {
        const int tF = a.tileFirst[(x / a.rxi) * a.nty + (y / a.wi)];
        if (t >= tF) v = a.hist[(long long)t * a.histPlane + histOffset(hr, hcn, a.rxi, a.wi, dyn.histTilesY)];
    }
    dense[(size_t)x * NY + y] = v;
}
// the inverse (PvAmdSetHistoryPlane, a test seam): dense order -> recorded pressure plane t, through the same window, tile and
// tileFirst tests; a cell that is not stored at step t is left out, so that the read-back gives 0 there as before
__global__ void pv_set_histplane_kernel(const AnalyzeArgs a, int t, const float* dense, int NX, int NY, int histRows,
                                        float* hist) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    const int x = blockIdx.y;
    if (y >= NY || x >= NX) return;
    const DynParams dyn = *a.dyn;
    const int hr = x + a.G - dyn.histRow0, hcn = y + a.G - dyn.histCol0;
    if (hr >= 0 && hr < histRows && hcn >= 0 && hcn < dyn.histTilesY * a.wi) {
        const int tF = a.tileFirst[(x / a.rxi) * a.nty + (y / a.wi)];
        if (t >= tF) hist[(long long)t * a.histPlane + histOffset(hr, hcn, a.rxi, a.wi, dyn.histTilesY)] = dense[(size_t)x * NY + y];
    }
}

void launchUnpad(const float* padded, float* dense, const Geometry& g, hipStream_t stream) {
    dim3 grid((g.NY + 255) / 256, g.NX);
    hipLaunchKernelGGL(pv_unpad_kernel, grid, dim3(256), 0, stream, padded, dense, g);
}
void launchPad(const float* dense, float* padded, const Geometry& g, hipStream_t stream) {
    dim3 grid((g.NY + 255) / 256, g.NX);
    hipLaunchKernelGGL(pv_pad_kernel, grid, dim3(256), 0, stream, dense, padded, g);
}
void launchHistPlane(const AnalyzeArgs& a, int t, float* dense, int NX, int NY, int histRows,
                     hipStream_t stream) {
    dim3 grid((NY + 255) / 256, NX);
    hipLaunchKernelGGL(pv_histplane_kernel, grid, dim3(256), 0, stream, a, t, dense, NX, NY, histRows);
}
void launchSetHistPlane(const AnalyzeArgs& a, int t, const float* dense, int NX, int NY, int histRows, float* hist,
                        hipStream_t stream) {
    dim3 grid((NY + 255) / 256, NX);
    hipLaunchKernelGGL(pv_set_histplane_kernel, grid, dim3(256), 0, stream, a, t, dense, NX, NY, histRows, hist);
}

}  // namespace pva
