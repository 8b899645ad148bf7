// pv_zone_decay.hip -- per-zone ensemble decay curves (pv_zone_decay.h has the definition): the reduction of the recorded pressure
// history itself, [T][cells] -> [zones][T], by the summation order of pv_zones.h applied per time slot.
//
// The history is T planes in the tile-major layout; labels and onsets are row-major over the result map.  Per chunk of slots:
//   pv_zone_curve_rows_kernel<ONSET>  a wave owns one result row X and a group of kZoneCurveSlots consecutive slots, and walks the
//                                     row in blocks of 64 consecutive Y, one per lane.  Label, onset and the cell's offset inside
//                                     a plane are found ONCE per block and serve all slots of the group -- the zone-statistics
//                                     pass pays them per plane.  The group's loads of a block are issued together: plane j of
//                                     every lane in ABSOLUTE mode (a block touches at most three tile rows' pieces of a plane,
//                                     each contiguous), plane t0 + j of the lane's own onset t0 in ONSET mode (lanes with one
//                                     onset share their lines).  A lane loads only where t0 <= t < T and the cell lies in the
//                                     history window: a tile's history is stored only from the launch in which it first became
//                                     non-zero, so nothing below an onset may be read; every other lane contributes +0.0.
//                                     Per label present the wave runs the butterflies of zoneWaveBlockSum over (double)p *
//                                     (double)p for the group's sixteen slots TOGETHER (zoneWaveBlockSums16: the lanes a
//                                     butterfly step leaves idle carry another slot); lane z - 1 keeps zone z's row
//                                     accumulators of the group in registers and writes them to rows[slot][zone][X].
//                                     Skipped wave-uniformly, because they could only add +0.0 to sums that start at +0.0:
//                                     lanes that have no sample in any slot of the group (ABSOLUTE: onset after the group;
//                                     ONSET: t0 + first slot >= T), and with them whole blocks and whole groups;
//   pv_zone_curve_merge_kernel        a wave per (zone, slot) adds the row sums in increasing X, as pv_zone_merge_kernel does.
// Once per call, before the chunks:
//   pv_zone_members_rows_kernel, pv_zone_members_merge_kernel: members, smallest and largest onset of every zone (integers:
//                                     the order does not matter).
// Sparse-emitter mode keeps a ring of planes instead of the history; there the ABSOLUTE curve is reduced inside the run, per
// accumulate pass (launchStreamZoneCurves, from launchStreamAccum):
//   pv_stream_zone_curve_rows_kernel  the ABSOLUTE rows kernel over the ring: plane t % ring, the onsets of the accumulate pass
//                                     (int, -1 = none yet), loads only where onset <= t < T, and a launch over the rows and
//                                     64-blocks of the labels' bounding box alone; merged by pv_zone_curve_merge_kernel over the
//                                     box's rows.
// A block is reduced while the samples of the next block and the label and onset of the one after are in flight.  edc, the fits and the empty-zone values are
// the host's (zoneDecayFinish).  Plane offsets are 64-bit throughout.  Only vector stores; nothing is atomic.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "pv_launch.h"
#include "pv_prims.h"
#include "pv_zone_decay.h"
#include "pv_zones_dev.h"

namespace pva {

namespace {

constexpr int kZoneCurveBlock = 256;  // four waves: four consecutive rows of one slot group (they share the lines of a tile's rows)

template <bool ONSET>
__global__ __launch_bounds__(kZoneCurveBlock) void pv_zone_curve_rows_kernel(const ZoneCurveArgs a) {
    constexpr int TC = kZoneCurveSlots;
    const int lane = threadIdx.x & 63;
    const int X = blockIdx.x * (kZoneCurveBlock / 64) + (threadIdx.x >> 6);
    if (X >= a.gx) return;  // (wave-uniform)
    const int jl0 = blockIdx.y * TC;                           // the group's first slot inside the chunk
    const int j0 = a.slot0 + jl0;                              // ... and in the curve
    const int nj = a.slots - jl0 < TC ? a.slots - jl0 : TC;   // its slots (the chunk's last group may be short)
    double acc[TC];
#pragma unroll
    for (int k = 0; k < TC; ++k) acc[k] = 0.0;
    const int nb = (a.gy + kZoneBlock - 1) / kZoneBlock;
    // a member with a sample in some slot of the group
    const auto liveIn = [&](const ZoneCurveCell& c) { return c.label != 0 && (ONSET ? c.t0 + j0 < a.T : c.t0 <= j0 + nj - 1); };
    // the group's samples of a block's cell (+0.0f where the cell has none)
    const auto loadGroup = [&](const ZoneCurveCell& c, bool live, float (&p)[TC]) {
        const float* __restrict__ h = a.hist + c.g;
#pragma unroll
        for (int k = 0; k < TC; ++k) {
            const int t = ONSET ? c.t0 + j0 + k : j0 + k;
            const bool has = live && k < nj && t >= c.t0 && t < a.T;
            p[k] = has ? h[(long long)t * a.histPlane] : 0.0f;
        }
    };
    // two blocks ahead: block b is reduced while the samples of block b + 1 and the label and onset of block b + 2 are in flight
    ZoneCurveCell c = zoneCurveCellAt(a, X, lane);
    bool live = liveIn(c);
    float p[TC];
    loadGroup(c, live, p);
    ZoneCurveCell c1 = nb > 1 ? zoneCurveCellAt(a, X, kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
    for (int b = 0; b < nb; ++b) {
        const bool live1 = liveIn(c1);  // (label 0 past the last block)
        float p1[TC];
        loadGroup(c1, live1, p1);
        const ZoneCurveCell c2 = b + 2 < nb ? zoneCurveCellAt(a, X, (b + 2) * kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
        unsigned long long left = __ballot(live);
        while (left) {  // (wave-uniform)
            const int z = __builtin_amdgcn_readlane(c.label, __ffsll((long long)left) - 1);
            const bool mine = live && c.label == z;
            left &= ~__ballot(mine);
            double v[TC];
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                const double x = mine ? (double)p[k] : 0.0;
                v[k] = x * x;
            }
            const double sums = zoneWaveBlockSums16(v, lane);  // lane k: slot k's block value
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                const double bv = zoneReadLane(sums, k);
                if (lane == z - 1) acc[k] = acc[k] + bv;
            }
        }
        c = c1;
        live = live1;
#pragma unroll
        for (int k = 0; k < TC; ++k) p[k] = p1[k];
        c1 = c2;
    }
    if (lane >= a.nZones) return;
#pragma unroll
    for (int k = 0; k < TC; ++k)
        if (k < nj) a.rows[((long long)(jl0 + k) * a.nZones + lane) * a.gx + X] = acc[k];
}

// slot slot0 + blockIdx.y of zone blockIdx.x: the row sums in increasing X
__global__ __launch_bounds__(64) void pv_zone_curve_merge_kernel(const ZoneCurveArgs a) {
    const int lane = threadIdx.x;
    const int z = blockIdx.x, sl = blockIdx.y;
    const double* __restrict__ rows = a.rows + ((long long)sl * a.nZones + z) * a.gx;
    double total = 0.0;
    for (int X0 = 0; X0 < a.gx; X0 += 64) {
        const int X = X0 + lane;
        const double r = X < a.gx ? rows[X] : 0.0;
        // increasing X, wave-uniform (pv_zone_merge_kernel); the rows past gx add +0.0, which changes no bit
#pragma unroll
        for (int i = 0; i < 64; ++i) total = total + zoneReadLane(r, i);
    }
    if (lane == 0) a.etc[(long long)z * a.T + a.slot0 + sl] = total;
}

// a lane's cell of a block in sparse-emitter mode: the onset is the accumulate pass's (int, -1 = none yet), the plane offset the
// run's window's (the whole tile grid in this mode; checked all the same)
__device__ __forceinline__ ZoneCurveCell streamZoneCurveCellAt(const StreamZoneCurveArgs& a, const DynParams& dyn, int X, int Y) {
    ZoneCurveCell c{0, 0, 0};
    if (Y >= a.gy) return c;
    const long long s = (long long)X * a.gy + Y;
    const int label = (int)a.labels[s];
    if (label == 0) return c;
    const int on = a.onset[s];
    const int hr = X + a.G - dyn.histRow0, hc = Y + a.G - dyn.histCol0;
    if (on < 0 || on >= a.T || hr < 0 || hc < 0 || hr >= dyn.histTilesX * a.rxi || hc >= dyn.histTilesY * a.wi) return c;
    const long long g = histOffset(hr, hc, a.rxi, a.wi, dyn.histTilesY);
    if (g >= a.histPlane) return c;
    c.label = label;
    c.t0 = on;
    c.g = g;
    return c;
}

// pv_zone_curve_rows_kernel<false> over the ring of a sparse-emitter run, for the steps of one accumulate pass: a wave owns result
// row a.row0 + x of the labels' bounding box and a group of sixteen steps, and walks the box's blocks of 64 Y.  Step t lies in
// plane t % ring; a lane loads only where onset <= t < T with an onset this pass or an earlier one has found -- before a tile's
// first step the ring holds another step's data, and no member's sample lies there.  Everything else is the kernel above
__global__ __launch_bounds__(kZoneCurveBlock) void pv_stream_zone_curve_rows_kernel(const StreamZoneCurveArgs a) {
    constexpr int TC = kZoneCurveSlots;
    const int lane = threadIdx.x & 63;
    const int xr = blockIdx.x * (kZoneCurveBlock / 64) + (threadIdx.x >> 6);
    if (xr >= a.rows) return;  // (wave-uniform)
    const int X = a.row0 + xr;
    const int jl0 = blockIdx.y * TC;                           // the group's first step inside the chunk
    const int j0 = a.slot0 + jl0;                              // ... and in the run
    const int nj = a.slots - jl0 < TC ? a.slots - jl0 : TC;   // its steps (the chunk's last group may be short)
    const int r0 = j0 % a.ring;                                // the plane of its first step
    const DynParams dyn = *a.dyn;
    double acc[TC];
#pragma unroll
    for (int k = 0; k < TC; ++k) acc[k] = 0.0;
    // a member with a sample in some step of the group
    const auto liveIn = [&](const ZoneCurveCell& c) { return c.label != 0 && c.t0 <= j0 + nj - 1; };
    // the group's samples of a block's cell (+0.0f where the cell has none)
    const auto loadGroup = [&](const ZoneCurveCell& c, bool live, float (&p)[TC]) {
        const float* __restrict__ h = a.hist + c.g;
#pragma unroll
        for (int k = 0; k < TC; ++k) {
            const int t = j0 + k;
            const int r = (r0 + k) % a.ring;  // (wave-uniform)
            const bool has = live && k < nj && t >= c.t0 && t < a.T;
            p[k] = has ? h[(long long)r * a.histPlane] : 0.0f;
        }
    };
    const int bEnd = a.blk0 + a.blks;
    ZoneCurveCell c = streamZoneCurveCellAt(a, dyn, X, a.blk0 * kZoneBlock + lane);
    bool live = liveIn(c);
    float p[TC];
    loadGroup(c, live, p);
    ZoneCurveCell c1 = a.blks > 1 ? streamZoneCurveCellAt(a, dyn, X, (a.blk0 + 1) * kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
    for (int b = a.blk0; b < bEnd; ++b) {
        const bool live1 = liveIn(c1);  // (label 0 past the last block)
        float p1[TC];
        loadGroup(c1, live1, p1);
        const ZoneCurveCell c2 = b + 2 < bEnd ? streamZoneCurveCellAt(a, dyn, X, (b + 2) * kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
        unsigned long long left = __ballot(live);
        while (left) {  // (wave-uniform)
            const int z = __builtin_amdgcn_readlane(c.label, __ffsll((long long)left) - 1);
            const bool mine = live && c.label == z;
            left &= ~__ballot(mine);
            double v[TC];
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                const double x = mine ? (double)p[k] : 0.0;
                v[k] = x * x;
            }
            const double sums = zoneWaveBlockSums16(v, lane);  // lane k: step k's block value
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                const double bv = zoneReadLane(sums, k);
                if (lane == z - 1) acc[k] = acc[k] + bv;
            }
        }
        c = c1;
        live = live1;
#pragma unroll
        for (int k = 0; k < TC; ++k) p[k] = p1[k];
        c1 = c2;
    }
    if (lane >= a.nZones) return;
#pragma unroll
    for (int k = 0; k < TC; ++k)
        if (k < nj) a.rowSums[((long long)(jl0 + k) * a.nZones + lane) * a.rows + xr] = acc[k];
}

// members, smallest and largest onset of every zone in one result row
__global__ __launch_bounds__(kZoneCurveBlock) void pv_zone_members_rows_kernel(const ZoneCurveArgs a) {
    const int lane = threadIdx.x & 63;
    const int X = blockIdx.x * (kZoneCurveBlock / 64) + (threadIdx.x >> 6);
    if (X >= a.gx) return;  // (wave-uniform)
    ZoneMembers m{0, INT_MAX, -1};
    const int nb = (a.gy + kZoneBlock - 1) / kZoneBlock;
    for (int b = 0; b < nb; ++b) {
        const ZoneCurveCell c = zoneCurveCellAt(a, X, b * kZoneBlock + lane);
        unsigned long long left = __ballot(c.label != 0);
        while (left) {
            const int z = __builtin_amdgcn_readlane(c.label, __ffsll((long long)left) - 1);
            const bool mine = c.label == z;
            const unsigned long long who = __ballot(mine);
            left &= ~who;
            const int lo = zoneWaveMin(mine ? c.t0 : INT_MAX), hi = zoneWaveMax(mine ? c.t0 : -1);
            if (lane == z - 1) {
                m.n_cells += __popcll(who);
                m.t_first = min(m.t_first, lo);
                m.t_last = max(m.t_last, hi);
            }
        }
    }
    if (lane < a.nZones) a.memberRows[(long long)lane * a.gx + X] = m;
}

__global__ __launch_bounds__(64) void pv_zone_members_merge_kernel(const ZoneCurveArgs a) {
    const int lane = threadIdx.x, z = blockIdx.x;
    int n = 0, lo = INT_MAX, hi = -1;
    for (int X = lane; X < a.gx; X += 64) {
        const ZoneMembers m = a.memberRows[(long long)z * a.gx + X];
        n += m.n_cells;
        lo = min(lo, m.t_first);
        hi = max(hi, m.t_last);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) n += __shfl_xor(n, s);
    lo = zoneWaveMin(lo);
    hi = zoneWaveMax(hi);
    if (lane == 0) a.members[z] = ZoneMembers{n, lo, hi};
}

}  // namespace

void launchZoneMembers(const ZoneCurveArgs& a, hipStream_t stream) {
    const dim3 rowsGrid((unsigned)((a.gx + kZoneCurveBlock / 64 - 1) / (kZoneCurveBlock / 64)));
    hipLaunchKernelGGL(pv_zone_members_rows_kernel, rowsGrid, dim3(kZoneCurveBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_members_merge_kernel, dim3((unsigned)a.nZones), dim3(64), 0, stream, a);
}

// slots a.slot0 .. a.slot0 + a.slots - 1 of every zone's etc
void launchZoneCurves(const ZoneCurveArgs& a, bool onset, hipStream_t stream) {
    const dim3 rowsGrid((unsigned)((a.gx + kZoneCurveBlock / 64 - 1) / (kZoneCurveBlock / 64)),
                        (unsigned)((a.slots + kZoneCurveSlots - 1) / kZoneCurveSlots));
    if (onset)
        hipLaunchKernelGGL(pv_zone_curve_rows_kernel<true>, rowsGrid, dim3(kZoneCurveBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(pv_zone_curve_rows_kernel<false>, rowsGrid, dim3(kZoneCurveBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_curve_merge_kernel, dim3((unsigned)a.nZones, (unsigned)a.slots), dim3(64), 0, stream, a);
}

// steps [tA, min(tB, T)) of every zone's etc, off the ring: per chunk the rows kernel over the box and the merge kernel above, whose
// "gx" is the box's rows (the rows outside the box could only add +0.0)
void launchStreamZoneCurves(const StreamZoneCurveArgs& a, double* etc, int tA, int tB, int chunk, hipStream_t stream) {
    const int tEnd = tB < a.T ? tB : a.T;
    StreamZoneCurveArgs s = a;
    ZoneCurveArgs m{};
    m.rows = a.rowSums;
    m.nZones = a.nZones;
    m.gx = a.rows;
    m.T = a.T;
    m.etc = etc;
    for (int t0 = tA; t0 < tEnd; t0 += chunk) {
        s.slot0 = m.slot0 = t0;
        s.slots = m.slots = tEnd - t0 < chunk ? tEnd - t0 : chunk;
        const dim3 rowsGrid((unsigned)((a.rows + kZoneCurveBlock / 64 - 1) / (kZoneCurveBlock / 64)),
                            (unsigned)((s.slots + kZoneCurveSlots - 1) / kZoneCurveSlots));
        hipLaunchKernelGGL(pv_stream_zone_curve_rows_kernel, rowsGrid, dim3(kZoneCurveBlock), 0, stream, s);
        hipLaunchKernelGGL(pv_zone_curve_merge_kernel, dim3((unsigned)a.nZones, (unsigned)s.slots), dim3(64), 0, stream, m);
    }
}

}  // namespace pva
