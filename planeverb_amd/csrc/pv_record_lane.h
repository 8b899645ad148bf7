// pv_record_lane.h -- which cell a lane of a per-cell record pass owns, and where its record goes.  The bodies of the record
// passes (pv_metrics_dev.h, pv_decay_dev.h, pv_lateral_dev.h, pv_echogram_dev.h, pv_echo_dev.h, pv_lobes_dev.h) take both from
// their caller, so the one body serves two kernels:
//  * the whole-map pass (pv_metrics.hip ...): lane = a consecutive OFFSET g of a history plane, record float k at out[k * plane + g];
//  * the in-run query pass (pv_query_records.hip): lane i = registered output query i, g = the history offset of its cell, record
//    float k at rec[k] of the query's slot in pinned host memory.
// Everything a body computes depends on the lane's own cell alone (time is wave-uniform, but what a lane adds at a step is decided
// by selects on its own ranges), so the bits of a record do not depend on which other cells share the wave.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>

#include "pv_analysis.h"
#include "pv_device.h"
#include "pv_prims.h"

namespace pva {

struct RecordLane {
    long long g;   // offset inside a history plane (>= histPlane: none)
    PlaneCell pc;  // planeCell(a, dyn, g)
    float delay;   // the cell's onset from the delay map, FLT_MAX = none
    bool live;     // the cell has an onset in this run: the lane computes a record
    bool slot;     // the lane has a record to write (NaN where !live)
};

// whole-map pass: the lane's consecutive offset
__device__ __forceinline__ RecordLane recordLaneAt(const AnalyzeArgs& a, const DynParams& dyn, long long g) {
    RecordLane l;
    l.g = g;
    l.pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    l.delay = l.pc.inGrid ? a.delay[(long long)l.pc.X * a.gy + l.pc.Y] : FLT_MAX;
    l.live = l.delay != FLT_MAX;
    l.slot = g < a.histPlane;
    return l;
}

// query pass: result cell X * gy + Y (-1: a position off the map) of a lane that has a slot.  The inverse of planeCell is
// histOffset (rt60Cell uses it the same way); a cell outside the run's history window has no sample recorded and no onset
__device__ __forceinline__ RecordLane recordLaneOfCell(const AnalyzeArgs& a, const DynParams& dyn, long long cell, bool slot) {
    RecordLane l;
    l.g = a.histPlane;
    l.slot = slot;
    if (slot && cell >= 0 && cell < (long long)a.gx * a.gy) {
        const int X = (int)(cell / a.gy), Y = (int)(cell - (long long)X * a.gy);
        const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
        if (hr >= 0 && hc >= 0 && hr < dyn.histTilesX * a.rxi && hc < dyn.histTilesY * a.wi) {
            const long long g = histOffset(hr, hc, a.rxi, a.wi, dyn.histTilesY);
            if (g < a.histPlane) l.g = g;
        }
    }
    l.pc = planeCell(a, dyn, l.g);
    l.delay = l.pc.inGrid ? a.delay[(long long)l.pc.X * a.gy + l.pc.Y] : FLT_MAX;
    l.live = l.delay != FLT_MAX;
    return l;
}

// where a record goes: float k of the lane's record
struct PlaneStore {  // plane k of the whole-map storage, at the lane's offset (64-bit addressing: the planes span gigabytes)
    float* out;
    long long plane, g;
    __device__ __forceinline__ void operator()(int k, float v) const { out[k * plane + g] = v; }
    __device__ __forceinline__ float load(int k) const { return out[k * plane + g]; }
};
struct SlotStore {  // the query's AoS slot
    float* rec;
    __device__ __forceinline__ void operator()(int k, float v) const { rec[k] = v; }
    __device__ __forceinline__ float load(int k) const { return rec[k]; }
};

}  // namespace pva
