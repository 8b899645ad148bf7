// pv_record_lane.h -- which cell a lane of a per-cell record pass owns, and where its record goes.  The bodies of the record
// passes (pv_metrics_dev.h, pv_decay_dev.h, pv_lateral_dev.h, pv_echogram_dev.h, pv_echo_dev.h, pv_lobes_dev.h) take both from
// their caller, so the one body serves several lane forms:
//  * the whole-map pass (pv_metrics.hip ...): lane = a consecutive OFFSET g of a history plane, record float k at out[k * plane + g];
//  * the in-run query pass (pv_query_records.hip): lane i = registered output query i, g = the history offset of its cell, record
//    float k at rec[k] of the query's slot in pinned host memory.
//  * the emitter pass of sparse-emitter mode (the same two kernels): lane i = registered emitter i, g = its COLUMN of the record
//    traces, which stand in for the history planes (recordLaneOfTrace).
//  * the array pass (pv_arrays.hip, the same two kernels): lane i = source array i, g = its COLUMN of the mix planes, which stand in
//    for the history planes, its onset from the table of the responses' own onsets (recordLaneOfMix).
// Everything a body computes depends on the lane's own cell alone (time is wave-uniform, but what a lane adds at a step is decided
// by selects on its own ranges), so the bits of a record do not depend on which other cells share the wave.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

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
    // what the velocity kinds (lateral, echogram, lobes) need beside the cell itself: the neighbours (X - 1, Y) and (X, Y - 1) as
    // plane offsets, whether they exist, and the first recorded steps of the cell's tile and of theirs (T / INT_MAX where !live)
    bool hasX, hasY;
    int gX, gY;
    int tFirst, tFx, tFy;
};

// the first recorded steps of a live lane's tile and of its neighbours' tiles (the real tiles of the real cell: pc.tile, pc.row, pc.col)
__device__ __forceinline__ void recordLaneFirstSteps(const AnalyzeArgs& a, RecordLane& l) {
    const PlaneCell& pc = l.pc;
    const int tileX = pc.row > 0 ? pc.tile : pc.tile - a.nty, tileY = pc.col > 0 ? pc.tile : pc.tile - 1;
    l.tFirst = a.T;
    l.tFx = INT_MAX;
    l.tFy = INT_MAX;
    if (l.live) {
        l.tFirst = a.tileFirst[pc.tile];
        if (l.hasX) l.tFx = a.tileFirst[tileX];
        if (l.hasY) l.tFy = a.tileFirst[tileY];
    }
}

// a lane of the tiled history window: the neighbours' offsets from the tile geometry (encodeWave)
__device__ __forceinline__ void recordLaneNeighbours(const AnalyzeArgs& a, const DynParams& dyn, RecordLane& l) {
    const PlaneCell& pc = l.pc;
    const int tileCells = a.rxi * a.wi;
    l.hasX = pc.hti > 0 || pc.row > 0;
    l.hasY = pc.htj > 0 || pc.col > 0;
    l.gX = pc.row > 0 ? pc.g - a.wi : pc.g - dyn.histTilesY * tileCells + (a.rxi - 1) * a.wi;
    l.gY = pc.col > 0 ? pc.g - 1 : pc.g - tileCells + (a.wi - 1);
    recordLaneFirstSteps(a, l);
}

// whole-map pass: the lane's consecutive offset
__device__ __forceinline__ RecordLane recordLaneAt(const AnalyzeArgs& a, const DynParams& dyn, long long g) {
    RecordLane l;
    l.g = g;
    l.pc = planeCell(a, dyn, g);  // (g >= histPlane: not in the grid)
    l.delay = l.pc.inGrid ? a.delay[(long long)l.pc.X * a.gy + l.pc.Y] : FLT_MAX;
    l.live = l.delay != FLT_MAX;
    l.slot = g < a.histPlane;
    recordLaneNeighbours(a, dyn, l);
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
    recordLaneNeighbours(a, dyn, l);
    return l;
}

// The record traces of sparse-emitter mode (AnalyzeArgs::recTrace, written by pv_stream_rectrace_kernel) are planes of recCols x
// (1 or 3) floats, one per step: emitter i's own pressure in column i and, where a velocity kind is selected (recVel), the
// pressure of (X - 1, Y) in column recCols + i and of (X, Y - 1) in column 2 recCols + i.
// Which of a window cell's two neighbours exist, by the rule of recordLaneNeighbours -- the trace writer gives a column to the
// neighbours this says, so that a trace lane loads what a tiled lane loads
__device__ __forceinline__ void traceNeighbours(const AnalyzeArgs& a, const DynParams& dyn, int X, int Y, bool* hasX, bool* hasY) {
    const int ti = X / a.rxi, tj = Y / a.wi;
    *hasX = ti - dyn.histTileX0 > 0 || X - ti * a.rxi > 0;
    *hasY = tj - dyn.histTileY0 > 0 || Y - tj * a.wi > 0;
}

// emitter pass of sparse-emitter mode: lane i = registered emitter i, result cell X * gy + Y, of a lane that has a slot.  `a.hist`
// / `a.histPlane` are the record traces', so the lane's offsets are its COLUMNS; the cell (face coefficients, distance to the
// listener), its onset and the first steps are those of the real cell and of the real tiles.  A cell outside the run's history
// window has no column and no onset, as in recordLaneOfCell
__device__ __forceinline__ RecordLane recordLaneOfTrace(const AnalyzeArgs& a, const DynParams& dyn, long long cell, int i, bool slot) {
    RecordLane l;
    l.g = a.histPlane;
    l.slot = slot;
    l.pc = PlaneCell{false, 0, 0, 0, 0, 0, 0, 0, 0};
    l.hasX = l.hasY = false;
    l.gX = l.gY = 0;
    if (slot && cell >= 0 && cell < (long long)a.gx * a.gy && i < a.recCols) {
        const int X = (int)(cell / a.gy), Y = (int)(cell - (long long)X * a.gy);
        const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
        if (hr >= 0 && hc >= 0 && hr < dyn.histTilesX * a.rxi && hc < dyn.histTilesY * a.wi) {
            const int ti = X / a.rxi, tj = Y / a.wi;
            l.g = i;
            l.pc = PlaneCell{true, X, Y, ti * a.nty + tj, X - ti * a.rxi, Y - tj * a.wi, i, ti - dyn.histTileX0, tj - dyn.histTileY0};
            if (a.recVel) {
                traceNeighbours(a, dyn, X, Y, &l.hasX, &l.hasY);
                l.gX = a.recCols + i;
                l.gY = 2 * a.recCols + i;
            }
        }
    }
    l.delay = l.pc.inGrid ? a.delay[(long long)l.pc.X * a.gy + l.pc.Y] : FLT_MAX;
    l.live = l.delay != FLT_MAX;
    recordLaneFirstSteps(a, l);
    return l;
}

// array pass (pv_arrays.hip, pv_solver_arrays.cpp): lane i = array i of the setting.  `a.hist` / `a.histPlane` are the mix planes'
// ([T][P], a response being a column) and `a.delay` is the table of the responses' own onsets (P floats, FLT_MAX: none), so the
// lane's offset is its COLUMN and its onset comes from that table.  A mix has no cell: no face coefficients, no neighbours, and
// every step of a column was written, so the first steps are 0.  The velocity kinds are never launched with this lane
__device__ __forceinline__ RecordLane recordLaneOfMix(const AnalyzeArgs& a, int i, bool slot) {
    RecordLane l;
    l.slot = slot;
    l.g = slot && i < a.histPlane ? i : a.histPlane;
    l.pc = PlaneCell{false, 0, 0, 0, 0, 0, 0, 0, 0};
    l.hasX = l.hasY = false;
    l.gX = l.gY = 0;
    l.delay = l.g < a.histPlane ? a.delay[l.g] : FLT_MAX;
    l.live = l.delay != FLT_MAX;
    l.tFirst = l.live ? 0 : a.T;
    l.tFx = l.tFy = INT_MAX;
    return l;
}

// which of the three a record launch's lanes are
enum RecordLaneForm { kLaneCell = 0, kLaneTrace = 1, kLaneMix = 2 };
template <int FORM>
__device__ __forceinline__ RecordLane recordLaneOfForm(const AnalyzeArgs& a, const DynParams& dyn, const long long* cells, int i, bool slot) {
    if constexpr (FORM == kLaneMix) {
        return recordLaneOfMix(a, i, slot);
    } else {
        const long long cell = slot ? cells[i] : -1;
        if constexpr (FORM == kLaneTrace)
            return recordLaneOfTrace(a, dyn, cell, i, slot);
        else
            return recordLaneOfCell(a, dyn, cell, slot);
    }
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
