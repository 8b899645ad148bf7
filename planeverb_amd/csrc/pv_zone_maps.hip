// pv_zone_maps.hip -- sparse-emitter mode: the room-metrics and spectrum records of every labelled cell, accumulated inside the
// run off the ring (PvAmdSetZoneMaps; pv_zone_maps.h).
//
//   pv_zone_maps_room_kernel        once per accumulate pass [tA, tB), behind pv_stream_accum_kernel of the same pass (whose onsets
//   pv_zone_maps_spec_kernel<B>     it reads) and in front of the event that hands the half ring back to the step kernels.  The work
//                                   items are the labelled cells with 0 <= onset < min(tB, T); each walks t = max(tA, onset) ..
//                                   min(tB, T) - 1 in increasing order and applies the kind's own per-sample update (pv_metrics.h
//                                   roomSumsStep, pv_spectrum.h spectrumStep).  The sums live in the record's own planes (room
//                                   metrics: 4 .. 9, spectrum: 3 j and 3 j + 1): a cell whose onset lies in the pass starts from +0.0f
//                                   and never reads them, one with an earlier onset reads what the pass before stored.  Nothing
//                                   before a cell's onset is loaded (before tileFirst the ring holds another step's data).
//   pv_zone_maps_finish_kernel      behind the finalize pass, i.e. behind every accumulate pass: planes 0 .. 3 from roomMetricsDerive,
//                                   the level plane of every bin from spectrumLevel; a labelled cell without an onset in this run
//                                   gets quiet NaN in all of its planes.
//
// Launch shape: the list of labelled tiles, 256 consecutive cells of a tile per block.  Ring planes and map planes are tile-major
// (pv_prims.h histOffset), so a wave's 64 lanes read and write 256 contiguous bytes of every plane.  Time is wave-uniform (the
// ring plane index is a scalar); what a lane adds at a step is decided by its own onset alone, so the bits of a record do not depend
// on the launch shape.  CH loads are in flight per lane, as in pv_stream_accum_kernel.  Unlabelled cells are never written here.
#include <hip/hip_runtime.h>

#include <climits>

#include "pv_device.h"
#include "pv_launch.h"
#include "pv_metrics.h"
#include "pv_prims.h"
#include "pv_spectrum.h"
#include "pv_zone_maps.h"

namespace pva {

namespace {

constexpr int kZoneMapChunk = 8;  // samples in flight per lane

struct ZoneMapLane {
    long long off;  // the cell's offset inside a plane (ring and maps alike)
    int s;          // result index X * gy + Y
    bool labelled;  // a result cell with a label whose offset lies inside the plane
};

// blockIdx.x = list entry * chunks + 256-cell chunk of the tile (pv_stream_accum_kernel's shape)
__device__ __forceinline__ ZoneMapLane zoneMapLane(const ZoneMapArgs& a) {
    ZoneMapLane l{0, 0, false};
    const int tileCells = a.rxi * a.wi;
    const int chunks = (tileCells + 255) / 256;
    const int entry = blockIdx.x / chunks;
    const int idx = (blockIdx.x - entry * chunks) * 256 + threadIdx.x;
    if (entry >= a.nTiles || idx >= tileCells) return l;
    const int t = a.tiles[entry];
    const int ti = t / a.nty, r = idx / a.wi;
    const int X = ti * a.rxi + r, Y = (t - ti * a.nty) * a.wi + (idx - r * a.wi);
    if (X >= a.gx || Y >= a.gy) return l;
    const DynParams dyn = *a.dyn;
    const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
    if (hr < 0 || hc < 0 || hr >= dyn.histTilesX * a.rxi || hc >= dyn.histTilesY * a.wi) return l;
    l.off = histOffset(hr, hc, a.rxi, a.wi, dyn.histTilesY);
    l.s = X * a.gy + Y;
    l.labelled = l.off < a.histPlane && a.labels[l.s] != 0;
    return l;
}

// the pass's range of a lane: live = the cell takes part in [tA, tB); start = its first step (INT_MAX where !live); *first = the
// wave's smallest start as a scalar.  false: no live lane in the wave
__device__ __forceinline__ bool zoneMapRange(const ZoneMapArgs& a, const ZoneMapLane& l, int tEnd, int* onset, bool* live, int* start, int* first) {
    const int on = l.labelled ? a.onset[l.s] : -1;
    *onset = on;
    *live = on >= 0 && on < tEnd;
    *start = *live ? max(a.tA, on) : INT_MAX;
    if (__ballot(*live) == 0ull) return false;
    int lo = *start;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) lo = min(lo, __shfl_xor(lo, o));
    *first = __builtin_amdgcn_readfirstlane(lo);
    return true;
}

}  // namespace

__global__ __launch_bounds__(256) void pv_zone_maps_room_kernel(const ZoneMapArgs a) {
    const ZoneMapLane l = zoneMapLane(a);
    const int tEnd = min(a.tB, a.T);
    int onset, start, first;
    bool live;
    if (!zoneMapRange(a, l, tEnd, &onset, &live, &start, &first)) return;
    const int n50 = roomMetricsN50(a.fs), n80 = roomMetricsN80(a.fs);
    float* rec = a.room + l.off;
    RoomSums s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (live && onset < a.tA) {
        s.e50 = rec[4 * a.histPlane];
        s.l50 = rec[5 * a.histPlane];
        s.e80 = rec[6 * a.histPlane];
        s.l80 = rec[7 * a.histPlane];
        s.total = rec[8 * a.histPlane];
        s.moment = rec[9 * a.histPlane];
    }
    const float* hc = a.hist + l.off;
    constexpr int CH = kZoneMapChunk;
    for (int t0 = first; t0 < tEnd; t0 += CH) {
        float pc[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            const long long o = (long long)(min(t, tEnd - 1) % a.ring) * a.histPlane;
            pc[k] = (t >= start && t < tEnd) ? hc[o] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            if (t >= start && t < tEnd) roomSumsStep(s, pc[k], t - onset, n50, n80);
        }
    }
    if (!live) return;
    rec[4 * a.histPlane] = s.e50;
    rec[5 * a.histPlane] = s.l50;
    rec[6 * a.histPlane] = s.e80;
    rec[7 * a.histPlane] = s.l80;
    rec[8 * a.histPlane] = s.total;
    rec[9 * a.histPlane] = s.moment;
}

// one slice of `bins` <= B bins, B {re, im} pairs to a lane; tab: rows of B {cos, sin} pairs by absolute step (wave-uniform loads)
template <int B>
__global__ __launch_bounds__(256) void pv_zone_maps_spec_kernel(const ZoneMapArgs a, const float* __restrict__ tab, int bin0, int bins) {
    const ZoneMapLane l = zoneMapLane(a);
    const int tEnd = min(a.tB, a.T);
    int onset, start, first;
    bool live;
    if (!zoneMapRange(a, l, tEnd, &onset, &live, &start, &first)) return;
    float* rec = a.spec + (long long)3 * bin0 * a.histPlane + l.off;
    float re[B], im[B];
    const bool carried = live && onset < a.tA;
#pragma unroll
    for (int j = 0; j < B; ++j) {
        re[j] = 0.f;
        im[j] = 0.f;
        if (j < bins && carried) {
            re[j] = rec[(long long)(3 * j) * a.histPlane];
            im[j] = rec[(long long)(3 * j + 1) * a.histPlane];
        }
    }
    const float* hc = a.hist + l.off;
    constexpr int CH = kZoneMapChunk;
    for (int t0 = first; t0 < tEnd; t0 += CH) {
        float pc[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            const long long o = (long long)(min(t, tEnd - 1) % a.ring) * a.histPlane;
            pc[k] = (t >= start && t < tEnd) ? hc[o] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int t = t0 + k;
            if (t >= tEnd) continue;  // (wave-uniform: no table row is read past the pass)
            const float* row = tab + (size_t)t * (2 * B);
            if (t >= start) {
#pragma unroll
                for (int j = 0; j < B; ++j)
                    if (j < bins) spectrumStep(pc[k], row[2 * j], row[2 * j + 1], re[j], im[j]);
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int j = 0; j < B; ++j)
        if (j < bins) {
            rec[(long long)(3 * j) * a.histPlane] = re[j];
            rec[(long long)(3 * j + 1) * a.histPlane] = im[j];
        }
}

__global__ __launch_bounds__(256) void pv_zone_maps_finish_kernel(const ZoneMapArgs a) {
    const ZoneMapLane l = zoneMapLane(a);
    if (!l.labelled) return;
    const int onset = a.onset[l.s];
    const bool has = onset >= 0 && onset < a.T;
    const float qnan = __builtin_nanf("");
    if (a.room) {
        float* rec = a.room + l.off;
        if (has) {
            RoomSums s;
            s.e50 = rec[4 * a.histPlane];
            s.l50 = rec[5 * a.histPlane];
            s.e80 = rec[6 * a.histPlane];
            s.l80 = rec[7 * a.histPlane];
            s.total = rec[8 * a.histPlane];
            s.moment = rec[9 * a.histPlane];
            float c50, c80, d50, ts;
            roomMetricsDerive(s, a.fs, &c50, &c80, &d50, &ts);
            rec[0] = c50;
            rec[a.histPlane] = c80;
            rec[2 * a.histPlane] = d50;
            rec[3 * a.histPlane] = ts;
        } else {
            for (int k = 0; k < kRoomMetricFloats; ++k) rec[k * a.histPlane] = qnan;
        }
    }
    if (a.spec) {
        float* rec = a.spec + l.off;
        for (int j = 0; j < a.nBins; ++j) {
            float* r = rec + (long long)(3 * j) * a.histPlane;
            if (has) {
                r[2 * a.histPlane] = spectrumLevel(r[0], r[a.histPlane], a.specPow[j]);
            } else {
                r[0] = qnan;
                r[a.histPlane] = qnan;
                r[2 * a.histPlane] = qnan;
            }
        }
    }
}

static unsigned zoneMapBlocks(const ZoneMapArgs& a) { return (unsigned)((a.rxi * a.wi + 255) / 256) * (unsigned)a.nTiles; }

void launchStreamZoneMaps(const ZoneMapArgs& a, const ZoneMapSpecSlice* slices, int nSlices, hipStream_t stream) {
    if (a.nTiles < 1) return;
    const dim3 grid(zoneMapBlocks(a));
    if (a.room) hipLaunchKernelGGL(pv_zone_maps_room_kernel, grid, dim3(256), 0, stream, a);
    if (!a.spec) return;
    for (int i = 0; i < nSlices; ++i) {
        const ZoneMapSpecSlice& sl = slices[i];
        if (sl.block == 8)
            hipLaunchKernelGGL(pv_zone_maps_spec_kernel<8>, grid, dim3(256), 0, stream, a, sl.tab, sl.bin0, sl.bins);
        else
            hipLaunchKernelGGL(pv_zone_maps_spec_kernel<16>, grid, dim3(256), 0, stream, a, sl.tab, sl.bin0, sl.bins);
    }
}

void launchStreamZoneMapsFinish(const ZoneMapArgs& a, hipStream_t stream) {
    if (a.nTiles < 1 || (!a.room && !a.spec)) return;
    hipLaunchKernelGGL(pv_zone_maps_finish_kernel, dim3(zoneMapBlocks(a)), dim3(256), 0, stream, a);
}

}  // namespace pva
