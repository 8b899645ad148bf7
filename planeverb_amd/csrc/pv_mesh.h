// pv_mesh.h -- the mesh layer's device side (pv_mesh.hip): slice a resident triangle mesh at the solver's height, scatter the
// section into a bit plane, scan marks into coverage (solid meshes) and apply the mesh's admittance to the plane the shape
// compose reads as its base.  The model is stated in include/planeverb_amd.h ("Triangle meshes"); pv_core.cpp meshSection /
// meshCoverage restate it on the CPU.
//
// The bit plane holds one bit per cell: 32-bit words of 32 consecutive x, word w of column y at bits[w * NY + y] (y contiguous,
// as every other plane).  Both accumulation rules are order-independent -- parity by atomicXor, union by atomicOr -- so the plane
// is the same bits whatever order the waves run in.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace pva {

// cell bounds accumulated on the device: {x0, x1, y0, y1}, cells [x0, x1) x [y0, y1); empty = {INT_MAX, 0, INT_MAX, 0}
struct MeshBounds {
    int x0, x1, y0, y1;
};

struct MeshSliceArgs {
    const float* verts;  // nv x (x, y, z)
    const int* tris;     // nt x 3
    int nt;
    int hasM;            // 0: no transform (the vertices as they are)
    float m[12];         // row-major 3 x 4
    float h;
    float4* seg;         // slot i: (a.x, a.z, b.x, b.z) of triangle i
    uint8_t* valid;      // slot i: 1 = a segment, 0 = none
};

struct MeshScatterArgs {
    const float4* seg;
    const uint8_t* valid;
    int nt;
    unsigned* bits;      // zeroed before the launch
    MeshBounds* bounds;  // shell: the covered cells' bounds; solid: rows and highest mark (the scan completes x0)
    int gx, gy, NY;
    float dx;
    int shell;           // 0: solid (marks by atomicXor), 1: shell (coverage by atomicOr)
    float r;
    float extent;        // max(gsx, gsy) * dx, for the shell's pad
};

struct MeshApplyArgs {
    const unsigned* bits;
    float* mat;          // AABB layer overwritten by the meshes, NX x NY
    uint8_t* owner;      // 0 = the AABB layer, else 1 + the covering mesh's id
    int x0, x1, y0, y1;  // cells to visit
    int NY;
    float Y;
    int id;
};

void launchMeshSlice(const MeshSliceArgs& a, hipStream_t stream);
void launchMeshScatter(const MeshScatterArgs& a, hipStream_t stream);
// solid only: marks -> coverage over the rows the scatter found, bounds->x0 from the lowest covered word
void launchMeshScan(unsigned* bits, MeshBounds* bounds, int gx, int NY, hipStream_t stream);
// mat / owner <- base / 0 over cells [x0, x1) x [y0, y1)
void launchMeshRestore(const float* base, float* mat, uint8_t* owner, int x0, int x1, int y0, int y1, int NY, hipStream_t stream);
void launchMeshApply(const MeshApplyArgs& a, hipStream_t stream);

}  // namespace pva
