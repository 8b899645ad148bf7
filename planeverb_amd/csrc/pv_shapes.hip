// pv_shapes.hip -- rasterise-and-compose of the shape layer (pv_shapes.h).  No reference counterpart: the reference has
// axis-aligned boxes only.  Coverage is the cell-centre rule of pv_core.cpp shapeCovers, in the same float32 operations
// (compiled with -ffp-contract=off, so e.x * (P.y - a.y) - e.y * (P.x - a.x) stays two multiplies and a subtract).
#include <hip/hip_runtime.h>

#include "pv_shapes.h"

namespace pva {

__device__ __forceinline__ bool covers(const DevShape& s, float px, float py) {
    bool in = true;
    for (int i = 0; i < s.n; ++i) {
        const int j = i + 1 == s.n ? 0 : i + 1;
        const float ax = s.xy[2 * i], ay = s.xy[2 * i + 1];
        const float ex = s.xy[2 * j] - ax, ey = s.xy[2 * j + 1] - ay;
        in = in && ((ex * (py - ay)) - (ey * (px - ax)) >= 0.f);
    }
    return in;
}

// One workgroup of 256 threads per dirty bin: 64 lanes along y (contiguous), 4 rows at a time.  A cell starts from the AABB
// layer and takes the Y of the first covering shape of its bin's list (highest sequence number first).  The ghost row and
// column are never covered: DevShape::x1 / y1 stop at gx / gy.
__global__ __launch_bounds__(256) void pv_shape_compose_kernel(ShapeArgs a) {
    const int bin = a.dirtyBins[blockIdx.x];
    const int bx = bin / a.nby, by = bin - bx * a.nby;
    const int y = by * kShapeBin + (threadIdx.x & 63);
    const int first = a.binStart[bin], last = a.binStart[bin + 1];
    if (y >= a.NY) return;
    const float py = ((float)y + 0.5f) * a.dx;
    for (int r = threadIdx.x >> 6; r < kShapeBin; r += 4) {
        const int x = bx * kShapeBin + r;
        if (x >= a.NX) break;
        const size_t i = (size_t)x * a.NY + y;
        float v = a.base[i];
        const float px = ((float)x + 0.5f) * a.dx;
        for (int k = first; k < last; ++k) {
            const DevShape& s = a.shapes[a.binList[k]];
            if (x < s.x0 || x >= s.x1 || y < s.y0 || y >= s.y1) continue;
            if (covers(s, px, py)) {
                v = s.Y;
                break;
            }
        }
        a.mat[i] = v;
    }
}

void launchShapeCompose(const ShapeArgs& a, hipStream_t stream) {
    if (a.numDirty <= 0) return;
    hipLaunchKernelGGL(pv_shape_compose_kernel, dim3(a.numDirty), dim3(256), 0, stream, a);
}

}  // namespace pva
