// pv_zones_dev.h -- the cross-lane pieces the zone passes share (pv_zones.hip, pv_zone_decay.hip): DPP moves and the wave form of
// the block butterfly of pv_zones.h.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

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

}  // namespace pva
