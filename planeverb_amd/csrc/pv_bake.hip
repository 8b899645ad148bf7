// pv_bake.hip -- kernels of the baked probe tables (pv_bake.h): the after-run gather of a probe's emitter-lattice block and the
// device form of the query rule.  A file of their own, so that the step kernels' compiled form does not change.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "pv_bake.h"

namespace pva {

// pass 1: bounding box of the reached lattice nodes of the window (lattice indices, atomics on the device words)
__global__ void pv_bake_box_kernel(const BakeGatherArgs a) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)a.nni * a.nnj) return;
    const int ii = (int)(t / a.nnj), jj = (int)(t - (long long)ii * a.nnj);
    const int i = a.ni0 + ii, j = a.nj0 + jj;
    const long long s = (long long)i * a.stride * a.gy + (long long)j * a.stride;
    if (!(a.delay[s] < FLT_MAX)) return;
    atomicMax(a.box + 0, -i);
    atomicMax(a.box + 1, -j);
    atomicMax(a.box + 2, i);
    atomicMax(a.box + 3, j);
}

// pass 2: the box's records (8 members + onset; an unreached node: zeros + FLT_MAX) and the box into the pinned staging
__global__ void pv_bake_write_kernel(const BakeGatherArgs a) {
    const int bi1 = a.box[2], bj1 = a.box[3];
    const bool empty = bi1 < 0;
    const int bi0 = -a.box[0], bj0 = -a.box[1];
    const int bni = empty ? 0 : bi1 - bi0 + 1, bnj = empty ? 0 : bj1 - bj0 + 1;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        a.stage[0] = empty ? 0 : bi0;
        a.stage[1] = empty ? 0 : bj0;
        a.stage[2] = bni;
        a.stage[3] = bnj;
    }
    if (t >= (long long)bni * bnj) return;
    const int ii = (int)(t / bnj), jj = (int)(t - (long long)ii * bnj);
    const long long s = (long long)(bi0 + ii) * a.stride * a.gy + (long long)(bj0 + jj) * a.stride;
    float* o = reinterpret_cast<float*>(a.stage + 4) + t * kBakeRecFloats;
    const float d = a.delay[s];
    const bool reached = d < FLT_MAX;
    for (int k = 0; k < 8; ++k) o[k] = reached ? a.res[k * a.resN + s] : 0.f;
    o[8] = reached ? d : FLT_MAX;
}

void launchBakeGather(const BakeGatherArgs& a, hipStream_t stream) {
    hipMemsetAsync(a.box, 0x80, 4 * sizeof(int), stream);  // 0x80808080: below every -i and every i
    const long long nodes = (long long)a.nni * a.nnj;
    const unsigned blocks = (unsigned)((nodes + 255) / 256);
    if (blocks > 0) hipLaunchKernelGGL(pv_bake_box_kernel, dim3(blocks), dim3(256), 0, stream, a);
    // (the block lies inside the window's nodes: `blocks` covers it; one block at least writes the header)
    hipLaunchKernelGGL(pv_bake_write_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, a);
}

__global__ void pv_bake_query_kernel(const BakeView v, const float* __restrict__ lxyz, const float* __restrict__ exyz, int n,
                                     float* __restrict__ out8) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    float o[8];
    bakeQuery(v, lxyz[3 * (long long)q], lxyz[3 * (long long)q + 2], exyz[3 * (long long)q], exyz[3 * (long long)q + 2], o);
    for (int k = 0; k < 8; ++k) out8[8 * (long long)q + k] = o[k];
}

void launchBakeQuery(const BakeView& v, const float* lxyz, const float* exyz, int n, float* out8, hipStream_t stream) {
    if (n > 0) hipLaunchKernelGGL(pv_bake_query_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v, lxyz, exyz, n, out8);
}

}  // namespace pva
