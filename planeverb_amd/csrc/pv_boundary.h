// pv_boundary.h -- the grid-edge pass (pv_boundary.hip): edge faces with an admittance other than the absorbing Y = 1.
//
// Sides, in this order everywhere: 0 = faces at x = 0 (world x = 0), 1 = faces at x = gx, 2 = faces at y = 0 (world z = 0),
// 3 = faces at y = gy.  Each side has an absorption R, as PlaneverbAddGeometry takes it, and the admittance
// Y = (1 - R) / (1 + R) in float32 (Solver::applyGeometry's expression for wall cells).  R = 0 everywhere is the reference's
// absorbing grid (FDTD.cpp:201-223), and the pass is then not launched at all.
#pragma once

#include <hip/hip_runtime.h>

#include "pv_device.h"

namespace pva {

struct EdgeY {
    float y[4];
};

// Rewrites the edge faces of the padded coefficient plane that pv_coef_kernel has just written, with Y in place of 1:
//   x = 0  : kx = (cell air && y < gy) ? -Y0 : 0        x = gx : kx = (y < gy) ? +Y1 : 0
//   y = 0  : ky = (cell air && x < gx) ? -Y2 : 0        y = gy : ky = (x < gx) ? +Y3 : 0
// in whole-grid coordinates (Geometry::x0, gxg), so a slab's guard rows get the owner's coefficients.  Stream-ordered
// behind launchCoefs and in front of the tile classification.
void launchEdgeCoefs(FaceCoef* coef, const Geometry& g, const EdgeY& y, hipStream_t stream);

}  // namespace pva
