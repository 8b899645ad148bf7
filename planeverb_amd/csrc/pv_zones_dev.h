// pv_zones_dev.h -- the cross-lane pieces the zone passes share (pv_zones.hip, pv_zone_decay.hip, pv_zone_band_decay.hip): DPP
// moves, the wave form of the block butterfly of pv_zones.h, its sixteen-slot form, a cell's offset inside a plane of the history
// window and the member rule of the two zone-decay passes.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "pv_prims.h"
#include "pv_zone_decay.h"

namespace pva {

// Cross-lane moves without the LDS crossbar where the pattern allows: DPP controls (gfx9: quad_perm, row_shl:n = 0x100 + n --
// dst[i] = src[i + n] inside a row of 16 lanes --, row_half_mirror, row_mirror), a lane's value by v_readlane where the lane is
// wave-uniform.  Every caller has all 64 lanes active
template <int CTRL>
__device__ __forceinline__ int zoneDpp(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
template <int CTRL>
__device__ __forceinline__ float zoneDpp(float v) {
    return __builtin_bit_cast(float, zoneDpp<CTRL>(__builtin_bit_cast(int, v)));
}
template <int CTRL>
__device__ __forceinline__ double zoneDpp(double v) {
    return __hiloint2double(zoneDpp<CTRL>(__double2hiint(v)), zoneDpp<CTRL>(__double2loint(v)));
}
__device__ __forceinline__ double zoneReadLane(double v, int lane) {  // lane: wave-uniform
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// the butterfly of pv_zones.h zoneBlockSum across the wave: lane i = v[i]; every lane returns v[0].  v[i + s] of a lane i that
// is a multiple of 2 s lies in i's own row of 16 for s <= 8 (row_shl); lanes that are no multiple of 2 s hold values nobody reads
__device__ __forceinline__ double zoneWaveBlockSum(double v) {
    v = v + zoneDpp<0x101>(v);
    v = v + zoneDpp<0x102>(v);
    v = v + zoneDpp<0x104>(v);
    v = v + zoneDpp<0x108>(v);
    v = v + __shfl_down(v, 16);
    v = v + __shfl_down(v, 32);
    return zoneReadLane(v, 0);
}

// The one place a zone kernel finds result cell (X, Y) in a tile-major plane of the window: is it inside, and at which offset
// (floats; the caller still holds it against the plane's size).  Two functions and not one with an "outside" value: a kernel
// tests the window in one condition with its own refusals of the cell, and these kernels sit at the scalar-register limit, where
// another shape of that condition compiles to other code (profiles/zone_passes_refactor.txt)
__device__ __forceinline__ bool zoneWindowHas(const ZoneWindow& w, int X, int Y) {
    const int hr = X - w.r0, hc = Y - w.c0;
    return hr >= 0 && hc >= 0 && hr < w.nr && hc < w.nc;
}
__device__ __forceinline__ long long zoneWindowOffset(const ZoneWindow& w, int X, int Y) {
    return histOffset(X - w.r0, Y - w.c0, w.rxi, w.wi, w.tilesY);
}

// ---- the pieces the two zone-decay passes share (pv_zone_decay.hip, pv_zone_band_decay.hip)

// a lane's cell of a block: label 0 where the cell is no member (no label, past gy, no onset, outside the window)
struct ZoneCurveCell {
    int label;
    int t0;
    long long g;  // offset inside a history plane
};
// the kept history's: the onset map of the run (float, FLT_MAX = none) and the window of the args
__device__ __forceinline__ ZoneCurveCell zoneCurveCellAt(const ZoneCurveArgs& a, int X, int Y) {
    ZoneCurveCell c{0, 0, 0};
    if (Y >= a.gy) return c;
    const long long s = (long long)X * a.gy + Y;
    const int label = (int)a.labels[s];
    if (label == 0) return c;
    const float d = a.delay[s];
    if (d == FLT_MAX || !(d >= 0.0f && d < (float)a.T) || !zoneWindowHas(a.w, X, Y)) return c;
    const long long g = zoneWindowOffset(a.w, X, Y);
    if (g >= a.histPlane) return c;
    c.label = label;
    c.t0 = (int)d;
    c.g = g;
    return c;
}

// The butterflies of zoneWaveBlockSum for SIXTEEN slots at once: v[k] = the lane's value of slot k; lane k (< 16) returns the block
// value of slot k.  After the step s of one butterfly only the lanes that are multiples of 2 s hold values anybody reads, so the
// other lanes carry another slot's: at step s = 1, 2, 4, 8 the lanes whose bit s is clear keep the even slot of a pair and the
// others the odd one, and each hands the partner lane (lane ^ s) the value IT needs -- 8 + 4 + 2 + 1 adds instead of 16 x 4.  Every
// add has the operands of the definition's v[i] = v[i] + v[i + s], for the odd slot with the two sides exchanged (IEEE addition is
// commutative).  Lane i then holds, for slot i & 15, the value of its row of 16 lanes; s = 16 and 32 add the rows as before.
// Exchanges: quad_perm [1, 0, 3, 2] and [2, 3, 0, 1], row_shl:4 / row_shr:4 by the side of the lane, row_ror:8
__device__ __forceinline__ double zoneWaveBlockSums16(const double (&v)[kZoneCurveSlots], int lane) {
    static_assert(kZoneCurveSlots == 16, "four halvings");
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
    double y[8], z[4], w[2];
#pragma unroll
    for (int m = 0; m < 8; ++m) y[m] = (b0 ? v[2 * m + 1] : v[2 * m]) + zoneDpp<0xB1>(b0 ? v[2 * m] : v[2 * m + 1]);
#pragma unroll
    for (int m = 0; m < 4; ++m) z[m] = (b1 ? y[2 * m + 1] : y[2 * m]) + zoneDpp<0x4E>(b1 ? y[2 * m] : y[2 * m + 1]);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const double send = b2 ? z[2 * m] : z[2 * m + 1];
        const double up = zoneDpp<0x104>(send), down = zoneDpp<0x114>(send);  // lane + 4, lane - 4 (0 outside the row: not selected)
        w[m] = (b2 ? z[2 * m + 1] : z[2 * m]) + (b2 ? down : up);
    }
    double u = (b3 ? w[1] : w[0]) + zoneDpp<0x128>(b3 ? w[0] : w[1]);
    u = u + __shfl_down(u, 16);
    u = u + __shfl_down(u, 32);
    return u;
}

__device__ __forceinline__ int zoneWaveMin(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s));
    return v;
}
__device__ __forceinline__ int zoneWaveMax(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s));
    return v;
}

}  // namespace pva
