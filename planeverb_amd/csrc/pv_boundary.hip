// pv_boundary.hip -- the grid-edge pass (pv_boundary.h).  No reference counterpart: the reference stores gridBoundaryType and
// steps absorbing edges whatever it says (FDTD.cpp:201-223).  An edge face of admittance Y is a wall face like any other
// (pv_device.h FaceCoef), so the stencil kernels step it unchanged; only its coefficient differs.
#include <hip/hip_runtime.h>

#include "pv_boundary.h"

namespace pva {

// One thread per edge face of the padded plane.  Threads [0, 2 rows): the y = 0 / y = gy face of every padded row whose
// whole-grid row lies in the cell array (guard rows included).  Threads [2 rows, 2 rows + 2 NY): the x = 0 / x = gxg face
// of every column, where that row lies inside this plane.  kx and ky are separate 4-byte stores: the corner cells' two
// faces are written by two threads without a race.  "Cell air" is the beta pv_coef_kernel wrote (air and not ghost).
__global__ __launch_bounds__(256) void pv_edge_coef_kernel(FaceCoef* __restrict__ coef, Geometry g, EdgeY e) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 2 * g.rows) {
        const int row = i >> 1, side = i & 1;
        const int x = row - g.G + g.x0;
        if (x < 0 || x >= g.NXg) return;
        const int y = side ? g.gy : 0;
        FaceCoef* c = coef + (size_t)row * g.pitch + (g.G + y);
        if (side)
            c->ky = x < g.gxg ? e.y[3] : 0.f;
        else
            c->ky = (c->beta != 0.f && x < g.gxg) ? -e.y[2] : 0.f;
        return;
    }
    const int j = i - 2 * g.rows;
    if (j >= 2 * g.NY) return;
    const int y = j >> 1, side = j & 1;
    const int x = side ? g.gxg : 0;
    const int row = x - g.x0 + g.G;
    if (row < 0 || row >= g.rows) return;
    FaceCoef* c = coef + (size_t)row * g.pitch + (g.G + y);
    if (side)
        c->kx = y < g.gy ? e.y[1] : 0.f;
    else
        c->kx = (c->beta != 0.f && y < g.gy) ? -e.y[0] : 0.f;
}

void launchEdgeCoefs(FaceCoef* coef, const Geometry& g, const EdgeY& y, hipStream_t stream) {
    const int n = 2 * g.rows + 2 * g.NY;
    hipLaunchKernelGGL(pv_edge_coef_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, coef, g, y);
}

}  // namespace pva
