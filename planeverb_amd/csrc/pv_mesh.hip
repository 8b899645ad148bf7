// pv_mesh.hip -- the mesh layer's kernels (pv_mesh.h).  No reference counterpart: the reference takes a collider's bounding box
// while the listener's height lies inside it.  The arithmetic is that of pv_core.cpp meshSection / meshCoverage, operation for
// operation in float32 (compiled with -ffp-contract=off), and every accumulation is order-independent, so the planes are
// the same bits as the CPU restatement's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "pv_mesh.h"

namespace pva {

// ---- slice: one lane per triangle, slot i <- triangle i's segment or "none" (no compaction: the section is deterministic) ----
__global__ __launch_bounds__(256) void pv_mesh_slice_kernel(MeshSliceArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nt) return;
    float p[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* __restrict__ v = a.verts + (size_t)3 * a.tris[3 * i + k];
        const float x = v[0], y = v[1], z = v[2];
        if (a.hasM) {
#pragma unroll
            for (int r = 0; r < 3; ++r) p[k][r] = ((a.m[4 * r] * x + a.m[4 * r + 1] * y) + a.m[4 * r + 2] * z) + a.m[4 * r + 3];
        } else {
            p[k][0] = x;
            p[k][1] = y;
            p[k][2] = z;
        }
    }
    const bool up0 = p[0][1] > a.h, up1 = p[1][1] > a.h, up2 = p[2][1] > a.h;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    uint8_t valid = 0;
    if (!(up0 == up1 && up1 == up2)) {
        const bool up[3] = {up0, up1, up2};
        int n = 0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int e2 = e == 2 ? 0 : e + 1;
            if (up[e] == up[e2]) continue;
            // p = the end that is not above, q = the end above, whichever way the triangle lists them
            const float lx = up[e] ? p[e2][0] : p[e][0], ly = up[e] ? p[e2][1] : p[e][1], lz = up[e] ? p[e2][2] : p[e][2];
            const float hx = up[e] ? p[e][0] : p[e2][0], hy = up[e] ? p[e][1] : p[e2][1], hz = up[e] ? p[e][2] : p[e2][2];
            const float t = (a.h - ly) / (hy - ly);
            const float X = lx + (t * (hx - lx)), Z = lz + (t * (hz - lz));
            if (n == 0) {
                o[0] = X;
                o[1] = Z;
            } else {
                o[2] = X;
                o[3] = Z;
            }
            ++n;
        }
        valid = 1;
    }
    a.seg[i] = make_float4(o[0], o[1], o[2], o[3]);
    a.valid[i] = valid;
}

// ---- scatter ----
struct LaneBounds {
    int x0, x1, y0, y1;
};

// cells x of 0 .. gx - 1 with ((float)x + 0.5f) * dx < xi form a prefix [0, k): the estimate, corrected by the predicate itself
__device__ __forceinline__ int crossingPrefix(float xi, float dx, int gx) {
    const float kf = ceilf(xi / dx - 0.5f);
    if (!(kf >= 0.f)) return 0;
    int k = kf >= (float)gx ? gx : (int)kf;
    while (k > 0 && !(((float)(k - 1) + 0.5f) * dx < xi)) --k;
    while (k < gx && ((float)k + 0.5f) * dx < xi) ++k;
    return k;
}

// clamp a float cell coordinate to [0, n] (NaN -> 0)
__device__ __forceinline__ int clampCell(float c, int n) { return !(c > 0.f) ? 0 : (c >= (float)n ? n : (int)c); }

// one row of one solid segment: at most one mark
__device__ __forceinline__ void solidRow(const float4 s, int y, const MeshScatterArgs& a, LaneBounds& lb) {
    const float py = ((float)y + 0.5f) * a.dx;
    if ((s.y > py) == (s.w > py)) return;
    const float xi = (((s.z - s.x) * (py - s.y)) / (s.w - s.y)) + s.x;
    const int k = crossingPrefix(xi, a.dx, a.gx);
    if (k > 0) {
        atomicXor(&a.bits[(size_t)((k - 1) >> 5) * a.NY + y], 1u << ((k - 1) & 31));
        lb.x1 = max(lb.x1, k);
        lb.y0 = min(lb.y0, y);
        lb.y1 = max(lb.y1, y + 1);
    }
}

// one row of one shell segment: the covered cells of columns [x0, x1), a word at a time
__device__ __forceinline__ void shellRow(const float4 s, int y, int x0, int x1, const MeshScatterArgs& a, LaneBounds& lb) {
    const float ex = s.z - s.x, ey = s.w - s.y, ee = (ex * ex) + (ey * ey), rr = a.r * a.r;
    const float wy = ((float)y + 0.5f) * a.dx - s.y, wyey = wy * ey;
    for (int w = x0 >> 5; w <= (x1 - 1) >> 5; ++w) {
        unsigned m = 0;
        const int xa = max(x0, w << 5), xb = min(x1, (w << 5) + 32);
        for (int x = xa; x < xb; ++x) {
            const float wx = ((float)x + 0.5f) * a.dx - s.x;
            float t = 0.f;
            if (ee != 0.f) {
                t = ((wx * ex) + wyey) / ee;
                t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
            }
            const float qx = wx - (t * ex), qy = wy - (t * ey);
            if ((qx * qx) + (qy * qy) <= rr) m |= 1u << (x & 31);
        }
        if (m) {
            atomicOr(&a.bits[(size_t)w * a.NY + y], m);
            lb.x0 = min(lb.x0, (w << 5) + (__ffs(m) - 1));
            lb.x1 = max(lb.x1, (w << 5) + 32 - __clz(m));
            lb.y0 = min(lb.y0, y);
            lb.y1 = max(lb.y1, y + 1);
        }
    }
}

constexpr int kMeshLaneRows = 4;  // a segment of up to this many rows is its lane's own; a longer one is spread over the wave

// One lane per triangle slot.  Lanes run along y: a segment that crosses more than kMeshLaneRows rows is taken by the whole wave,
// lane l the rows y0 + l, y0 + l + 64, ... (so the atomics of one wave-instruction fall on consecutive words of one word column),
// one such segment after the other; the short ones -- all of them in a finely tessellated mesh -- are each lane's own few rows.
// The bounds go through LDS: one global atomic per block and bound.
__global__ __launch_bounds__(256) void pv_mesh_scatter_kernel(MeshScatterArgs a) {
    __shared__ int sb[4];
    if (threadIdx.x < 4) sb[threadIdx.x] = (threadIdx.x & 1) ? 0 : INT_MAX;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    LaneBounds lb = {INT_MAX, 0, INT_MAX, 0};
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    int x0 = 0, x1 = 0, y0 = 0, y1 = 0;  // the cells this segment can touch (conservative; the predicates decide)
    if (i < a.nt && a.valid[i]) {
        s = a.seg[i];
        if (a.shell) {
            float m = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fmaxf(fabsf(s.z), fabsf(s.w)));
            m = fmaxf(m, a.extent) + a.r;
            const float pad = 2.f + ceilf(m * 4e-6f / a.dx);  // (as shapeCellBounds for a round shape; non-finite: every cell)
            x0 = clampCell(floorf((fminf(s.x, s.z) - a.r) / a.dx - 0.5f - pad), a.gx);
            x1 = clampCell(ceilf((fmaxf(s.x, s.z) + a.r) / a.dx - 0.5f + pad) + 1.f, a.gx);
            y0 = clampCell(floorf((fminf(s.y, s.w) - a.r) / a.dx - 0.5f - pad), a.gy);
            y1 = clampCell(ceilf((fmaxf(s.y, s.w) + a.r) / a.dx - 0.5f + pad) + 1.f, a.gy);
            if (!(m - m == 0.f)) {
                x0 = y0 = 0;
                x1 = a.gx;
                y1 = a.gy;
            }
            if (x0 >= x1) y1 = y0;
        } else {
            x1 = a.gx;
            y0 = clampCell(floorf(fminf(s.y, s.w) / a.dx - 0.5f) - 1.f, a.gy);
            y1 = clampCell(ceilf(fmaxf(s.y, s.w) / a.dx - 0.5f) + 2.f, a.gy);
            if (!((s.y - s.y) + (s.w - s.w) == 0.f)) {
                y0 = 0;
                y1 = a.gy;
            }
        }
    }
    const int rows = y1 - y0;
    if (rows > 0 && rows <= kMeshLaneRows) {
        for (int y = y0; y < y1; ++y) {
            if (a.shell)
                shellRow(s, y, x0, x1, a, lb);
            else
                solidRow(s, y, a, lb);
        }
    }
    unsigned long long longOnes = __ballot(rows > kMeshLaneRows);
    while (longOnes) {
        const int src = __ffsll((long long)longOnes) - 1;
        longOnes &= longOnes - 1;
        const float4 t = make_float4(__shfl(s.x, src), __shfl(s.y, src), __shfl(s.z, src), __shfl(s.w, src));
        const int tx0 = __shfl(x0, src), tx1 = __shfl(x1, src), ty0 = __shfl(y0, src), ty1 = __shfl(y1, src);
        for (int y = ty0 + lane; y < ty1; y += 64) {
            if (a.shell)
                shellRow(t, y, tx0, tx1, a, lb);
            else
                solidRow(t, y, a, lb);
        }
    }
    if (lb.x1 > 0) {
        atomicMin(&sb[0], lb.x0);
        atomicMax(&sb[1], lb.x1);
        atomicMin(&sb[2], lb.y0);
        atomicMax(&sb[3], lb.y1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && sb[1] > 0) {
        atomicMin(&a.bounds->x0, sb[0]);
        atomicMax(&a.bounds->x1, sb[1]);
        atomicMin(&a.bounds->y0, sb[2]);
        atomicMax(&a.bounds->y1, sb[3]);
    }
}

// ---- scan (solid): coverage(x) = XOR of the marks at x' >= x.  One lane per column y, from the highest marked word down to word
// 0: inside a word a suffix XOR by shifts, across words a carried parity bit (the coverage of the word's bit 0).  No mark lies at
// x >= gx, so the partial last word's upper bits stay 0.  bounds->x0 becomes the lowest covered cell's word start. ----
__global__ __launch_bounds__(64) void pv_mesh_scan_kernel(unsigned* __restrict__ bits, MeshBounds* bounds, int NY) {
    const int y0 = bounds->y0, y1 = bounds->y1, x1 = bounds->x1;
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (x1 <= 0) return;  // (uniform: every lane stays for the shuffles below)
    unsigned carry = 0;
    int lowest = INT_MAX;
    for (int w = (y >= y0 && y < y1) ? (x1 - 1) >> 5 : -1; w >= 0; --w) {
        unsigned v = bits[(size_t)w * NY + y];
        v ^= v >> 1;
        v ^= v >> 2;
        v ^= v >> 4;
        v ^= v >> 8;
        v ^= v >> 16;
        if (carry) v = ~v;
        carry = v & 1u;
        bits[(size_t)w * NY + y] = v;
        if (v) lowest = (w << 5) + (__ffs(v) - 1);
    }
    // (per wave: the lowest of its lanes, then one atomic)
    for (int d = 32; d > 0; d >>= 1) lowest = min(lowest, __shfl_xor(lowest, d));
    if ((threadIdx.x & 63) == 0 && lowest != INT_MAX) atomicMin(&bounds->x0, lowest);
}

// ---- restore / apply: lanes along y, one cell row x per step ----
__global__ __launch_bounds__(256) void pv_mesh_restore_kernel(const float* __restrict__ base, float* __restrict__ mat,
                                                              uint8_t* __restrict__ owner, int x0, int x1, int y0, int y1, int NY) {
    const int y = y0 + blockIdx.x * 64 + (threadIdx.x & 63);
    if (y >= y1) return;
    for (int x = x0 + blockIdx.y * 4 + (threadIdx.x >> 6); x < x1; x += 4 * gridDim.y) {
        const size_t i = (size_t)x * NY + y;
        mat[i] = base[i];
        owner[i] = 0;
    }
}

// a thread takes one coverage word of its column: up to 32 cells along x
__global__ __launch_bounds__(256) void pv_mesh_apply_kernel(MeshApplyArgs a) {
    const int y = a.y0 + blockIdx.x * 64 + (threadIdx.x & 63);
    const int w = (a.x0 >> 5) + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= a.y1 || w > (a.x1 - 1) >> 5) return;
    unsigned v = a.bits[(size_t)w * a.NY + y];
    while (v) {
        const int b = __ffs(v) - 1;
        v &= v - 1;
        const int x = (w << 5) + b;
        if (x < a.x0 || x >= a.x1) continue;
        a.mat[(size_t)x * a.NY + y] = a.Y;
        a.owner[(size_t)x * a.NY + y] = (uint8_t)(a.id + 1);
    }
}

void launchMeshSlice(const MeshSliceArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pv_mesh_slice_kernel, dim3((a.nt + 255) / 256), dim3(256), 0, stream, a);
}

void launchMeshScatter(const MeshScatterArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(pv_mesh_scatter_kernel, dim3((a.nt + 255) / 256), dim3(256), 0, stream, a);
}

void launchMeshScan(unsigned* bits, MeshBounds* bounds, int gx, int NY, hipStream_t stream) {
    (void)gx;
    hipLaunchKernelGGL(pv_mesh_scan_kernel, dim3((NY + 63) / 64), dim3(64), 0, stream, bits, bounds, NY);
}

void launchMeshRestore(const float* base, float* mat, uint8_t* owner, int x0, int x1, int y0, int y1, int NY, hipStream_t stream) {
    if (x0 >= x1 || y0 >= y1) return;
    const int by = std::min(256, (x1 - x0 + 3) / 4);
    hipLaunchKernelGGL(pv_mesh_restore_kernel, dim3((y1 - y0 + 63) / 64, by), dim3(256), 0, stream, base, mat, owner, x0, x1, y0, y1,
                       NY);
}

void launchMeshApply(const MeshApplyArgs& a, hipStream_t stream) {
    if (a.x0 >= a.x1 || a.y0 >= a.y1) return;
    const int words = ((a.x1 - 1) >> 5) - (a.x0 >> 5) + 1;
    hipLaunchKernelGGL(pv_mesh_apply_kernel, dim3((a.y1 - a.y0 + 63) / 64, (words + 3) / 4), dim3(256), 0, stream, a);
}

}  // namespace pva
