// pv_shapes.hip -- rasterise-and-compose of the shape layer (pv_shapes.h).  No reference counterpart: the reference has
// axis-aligned boxes only.  Coverage is the cell-centre rule of pv_core.cpp shapeCovers, in the same float32 operations
// (compiled with -ffp-contract=off, so e.x * (P.y - a.y) - e.y * (P.x - a.x) stays two multiplies and a subtract).
#include <hip/hip_runtime.h>

#include "pv_shapes.h"

namespace pva {

constexpr int kRowsPerLane = kShapeBin / 4;  // a lane owns the cells (xb + 4 j, y), j = 0 .. 15, of its bin

// One workgroup of 256 threads per dirty bin: 64 lanes along y (contiguous), wave w the rows w, w + 4, ...  A cell starts from
// the AABB layer and takes the Y of the first covering shape of its bin's list (highest sequence number first).  The ghost row
// and column are never covered: DevShape::x1 / y1 stop at gx / gy.
//
// The loop over the bin's shapes is the outer one and its counter is the same for every lane of a wave, so a shape's record, its
// kind and its points are scalar loads, made once per wave and shape, and the kind dispatch is a uniform branch.  Control flow
// is not uniform throughout: the tests against a shape's cell bounds (y here, x in `cand`) and the exit once a lane has no
// uncovered row left are per lane, as the coverage predicate is; `open` holds the lane's still uncovered rows, one bit each.
// What depends on y alone (an edge's e.x * (P.y - a.y), a segment's w.y * e.y, a polygon edge's intersection abscissa with its
// one division) is computed once per lane and edge, not once per cell.  The AABB layer's 16 values are loaded before the loop,
// so that their latency passes behind the shapes' scalar loads.
__global__ __launch_bounds__(256) void pv_shape_compose_kernel(ShapeArgs a) {
    const float* __restrict__ base = a.base;
    float* __restrict__ mat = a.mat;
    const DevShape* __restrict__ shapes = a.shapes;
    const float* __restrict__ pool = a.pool;
    const int* __restrict__ binList = a.binList;
    const int bin = a.dirtyBins[blockIdx.x];
    const int bx = bin / a.nby, by = bin - bx * a.nby;
    const int y = by * kShapeBin + (threadIdx.x & 63);
    const int first = a.binStart[bin], last = a.binStart[bin + 1];
    if (y >= a.NY) return;
    const int xb = bx * kShapeBin + (threadIdx.x >> 6);
    const float py = ((float)y + 0.5f) * a.dx;
    float px[kRowsPerLane], v[kRowsPerLane];
    unsigned open = 0;
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        px[j] = ((float)(xb + 4 * j) + 0.5f) * a.dx;
        v[j] = 0.f;
        if (xb + 4 * j < a.NX) {
            open |= 1u << j;
            v[j] = base[(size_t)(xb + 4 * j) * a.NY + y];
        }
    }
    for (int k = first; k < last && open; ++k) {
        const DevShape& s = shapes[binList[k]];
        if (y < s.y0 || y >= s.y1) continue;
        unsigned cand = 0;  // the open rows inside the shape's cell bounds
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j)
            if (xb + 4 * j >= s.x0 && xb + 4 * j < s.x1) cand |= 1u << j;
        cand &= open;
        if (!cand) continue;
        const int n = s.n;
        const float* __restrict__ pts = n > kShapeMaxVerts ? pool + s.off : s.xy;
        unsigned cov;
        if (s.kind == kShapeConvex) {
            cov = cand;
            for (int i = 0; i < n; ++i) {
                const int i2 = i + 1 == n ? 0 : i + 1;
                const float ax = s.xy[2 * i], ay = s.xy[2 * i + 1];
                const float ex = s.xy[2 * i2] - ax, ey = s.xy[2 * i2 + 1] - ay;
                const float t1 = ex * (py - ay);
#pragma unroll
                for (int j = 0; j < kRowsPerLane; ++j)
                    if (!(t1 - (ey * (px[j] - ax)) >= 0.f)) cov &= ~(1u << j);
            }
        } else if (s.kind == kShapeRound) {
            cov = 0;
            const float rr = s.r * s.r;
            const int segs = n > 1 ? n - 1 : 1;
            for (int i = 0; i < segs; ++i) {
                const int i2 = i + 1 < n ? i + 1 : i;
                const float ax = pts[2 * i], ay = pts[2 * i + 1];
                const float ex = pts[2 * i2] - ax, ey = pts[2 * i2 + 1] - ay;
                const float ee = (ex * ex) + (ey * ey);
                const float wy = py - ay, wyey = wy * ey;
                if (ee != 0.f) {
#pragma unroll
                    for (int j = 0; j < kRowsPerLane; ++j) {
                        const float wx = px[j] - ax;
                        float t = ((wx * ex) + wyey) / ee;
                        t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                        const float qx = wx - (t * ex), qy = wy - (t * ey);
                        if ((qx * qx) + (qy * qy) <= rr) cov |= 1u << j;
                    }
                } else {  // a disc: t = 0, q = w - 0 = w
                    const float wy2 = wy * wy;
#pragma unroll
                    for (int j = 0; j < kRowsPerLane; ++j) {
                        const float wx = px[j] - ax;
                        if ((wx * wx) + wy2 <= rr) cov |= 1u << j;
                    }
                }
            }
            cov &= cand;
        } else {  // kShapePolygon: even-odd crossings
            cov = 0;
            for (int i = 0; i < n; ++i) {
                const int i2 = i + 1 == n ? 0 : i + 1;
                const float ax = pts[2 * i], ay = pts[2 * i + 1], bx2 = pts[2 * i2], by2 = pts[2 * i2 + 1];
                if ((ay > py) != (by2 > py)) {
                    const float xi = (((bx2 - ax) * (py - ay)) / (by2 - ay)) + ax;
#pragma unroll
                    for (int j = 0; j < kRowsPerLane; ++j)
                        if (px[j] < xi) cov ^= 1u << j;
                }
            }
            cov &= cand;
        }
        const float Y = s.Y;
#pragma unroll
        for (int j = 0; j < kRowsPerLane; ++j)
            if (cov >> j & 1) v[j] = Y;
        open &= ~cov;
    }
#pragma unroll
    for (int j = 0; j < kRowsPerLane; ++j) {
        const int x = xb + 4 * j;
        if (x < a.NX) mat[(size_t)x * a.NY + y] = v[j];
    }
}

void launchShapeCompose(const ShapeArgs& a, hipStream_t stream) {
    if (a.numDirty <= 0) return;
    hipLaunchKernelGGL(pv_shape_compose_kernel, dim3(a.numDirty), dim3(256), 0, stream, a);
}

}  // namespace pva
