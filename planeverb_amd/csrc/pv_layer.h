// pv_layer.h -- graded absorbing layers at the grid edges (pv_layer.hip).  No reference counterpart.
//
// Sides, in the order of the grid-edge pass (pv_boundary.h): 0 = x = 0, 1 = x = gx, 2 = y = 0, 3 = y = gy.  A layer of width
// w (0..kEdgeLayerMaxWidth cells, 0 = none) is the outermost w cells of its side.  Its damping is eight float32 tables (below);
// the stencil of a layer tile is the general tile's with two expressions changed, multiplications only, without contraction:
//   pressure: pr' = beta * ((apx[x] * apy[y]) * pr - (bpx[x] * bpy[y]) * (C * div))
//   vx, air : ax[x] * vx - bx[x] * (C * (pr[x, y] - pr[x - 1, y]))      vy, air : ay[y] * vy - by[y] * (C * (pr[x, y] - pr[x, y - 1]))
// Every factor is exactly 1 outside the layers, where the expressions give the reference's bits.
// The split-field model (Solver::setEdgeLayer(..., split = true, r0)) changes the pressure of the layer cells only (apx[x] != 1
// or apy[y] != 1): such a cell carries px, the x part of its pressure (the y part is pr - px), in a plane of its own, and
//   nx = beta * ((apx * px) - bpx * (C * dvx))    ny = beta * ((apy * (pr - px)) - bpy * (C * dvy))    pr' = nx + ny, px' = nx
// every other cell: beta * (pr - C * div), px = 0.  The velocities are the unsplit model's.
#pragma once

#include <hip/hip_runtime.h>

#include "pv_core.h"
#include "pv_device.h"

namespace pva {

// the layer launch of one K-step sweep: the stencil arguments of the sweep's merged launch plus the layer tiles and the tables
// as padded planes (row table t at rowTab[t * rows + padded row], column table t at colTab[t * pitch + padded column];
// 1 in the padding)
struct LayerArgs {
    StepArgs a;
    const int* list;     // layer tiles (disjoint from the general list and tile class 1 for the air arm)
    int count;
    int rows, cols;      // pitches of the two tables (Geometry::rows, Geometry::pitch)
    const float* rowTab;  // apx, bpx, ax, bx
    const float* colTab;  // apy, bpy, ay, by
    // the split-field model (Solver::setEdgeLayerSplit): the x part of the pressure of the layer cells, a padded plane per
    // buffer set (read set n, write set n + 1; 0 in every other cell).  pxOut == NULL: the unsplit model
    const float* pxIn;
    float* pxOut;
};

// is there a layer kernel for this (K, rows) configuration (the product library's tiles)?
bool layerConfigOk(int K, int rxi);
// the layer tiles of the sweep, beside the merged launch (they read buffer set n and write disjoint tiles of set n + 1)
void launchStepLayer(int K, int rxi, const LayerArgs& l, hipStream_t stream);

}  // namespace pva
