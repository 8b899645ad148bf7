// pv_shapes.h -- the shape layer's device table and its rasterise-and-compose launch (pv_shapes.hip).
//
// A solver that has had a shape keeps the AABB layer's material in a plane of its own (base) and writes the composed
// material -- base, overwritten by the covering shape with the highest sequence number -- into the plane pv_coef_kernel
// reads.  Only dirty bins are recomposed: kShapeBin x kShapeBin cells each, a pure function of the current shape set.
#pragma once

#include <hip/hip_runtime.h>

#include "pv_core.h"

namespace pva {

constexpr int kShapeBin = 64;  // cells per bin side

struct DevShape {
    float xy[2 * kShapeMaxVerts];  // convex: counter-clockwise vertices, grid metres; round / polygon: the points when n <= 8
    int n;
    int kind;                      // ShapeKind (pv_core.h)
    float r;                       // radius of a round shape
    int off;                       // n > kShapeMaxVerts: the points are pool[off .. off + 2 n)
    float Y;                       // admittance (1 - R) / (1 + R), float32 as applyGeometry computes it for AABBs
    int x0, x1, y0, y1;            // cells [x0, x1) x [y0, y1) that can be covered (shapeCellBounds)
};

struct ShapeArgs {
    const float* base;        // AABB-layer material, NX x NY (NaN = air, else Y)
    float* mat;               // composed material, NX x NY
    const DevShape* shapes;
    const float* pool;        // point lists longer than kShapeMaxVerts (nullptr when no shape has one)
    const int* binStart;      // nbx * nby + 1 offsets into binList
    const int* binList;       // per bin: shape indices, highest sequence number first
    const int* dirtyBins;     // bins to recompose
    int numDirty;
    int NX, NY, nby;
    float dx;
};

// one workgroup per dirty bin; stream-ordered behind the table uploads
void launchShapeCompose(const ShapeArgs& a, hipStream_t stream);

}  // namespace pva
