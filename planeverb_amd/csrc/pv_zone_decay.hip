// pv_zone_decay.hip -- per-zone ensemble decay curves (pv_zone_decay.h has the definition): the reduction of the recorded pressure
// history itself, [T][cells] -> [zones][T], by the summation order of pv_zones.h applied per time slot.
//
// The planes are in the tile-major layout; labels and onsets are row-major over the result map.  Per chunk of slots:
//   pv_zone_curve_rows_kernel<ONSET, Source>
//                                     ONE body for both places the samples can lie in (the sources below).  A wave owns one result
//                                     row X and a group of kZoneCurveSlots consecutive slots, and walks the row in blocks of 64
//                                     consecutive Y, one per lane.  Label, onset and the cell's offset inside a plane are found
//                                     ONCE per block and serve all slots of the group -- the zone-statistics pass pays them per
//                                     plane.  The group's loads of a block are issued together: the plane of slot j of every lane
//                                     in ABSOLUTE mode (a block touches at most three tile rows' pieces of a plane, each
//                                     contiguous), plane t0 + j of the lane's own onset t0 in ONSET mode (lanes with one onset
//                                     share their lines).  A lane loads only where t0 <= t < T and the cell lies in the window: a
//                                     tile's history is stored only from the launch in which it first became non-zero, so nothing
//                                     below an onset may be read; every other lane contributes +0.0.
//                                     Per label present the wave runs the butterflies of zoneWaveBlockSum over (double)p *
//                                     (double)p for the group's sixteen slots TOGETHER (zoneWaveBlockSums16: the lanes a
//                                     butterfly step leaves idle carry another slot); lane z - 1 keeps zone z's row
//                                     accumulators of the group in registers and writes them to rows[slot][zone][row].
//                                     Skipped wave-uniformly, because they could only add +0.0 to sums that start at +0.0:
//                                     lanes that have no sample in any slot of the group (ABSOLUTE: onset after the group;
//                                     ONSET: t0 + first slot >= T), and with them whole blocks and whole groups;
//   pv_zone_curve_merge_kernel        a wave per (zone, slot) adds the row sums of the rows walked in increasing X, as
//                                     pv_zone_merge_kernel does (a row outside them could only add +0.0).
// A source is a compile-time policy; it says where a lane's cell comes from, which plane holds a step and what the launch walks:
//   ZoneHistorySource                 the kept history after a run (launchZoneCurves): the run's onset map (float, FLT_MAX = none),
//                                     the window of the arguments, step t in plane t, every row and block of the map.  Neither a
//                                     modulo nor a load of the run's DynParams is in these instantiations;
//   ZoneRingSource                    the ring of a sparse-emitter run, inside the run, per accumulate pass (launchStreamZoneCurves,
//                                     from launchStreamAccum): the onsets of the accumulate pass (int, -1 = none yet), the window
//                                     of the run's device DynParams, step t in plane t % ring, the rows and 64-blocks of the
//                                     labels' bounding box alone.  Before a tile's first step the ring holds another step's data,
//                                     and no member's sample lies there: the rule "only where onset <= t" covers it.  ABSOLUTE
//                                     only: an ONSET curve needs planes the ring no longer has.
// Once per call, before the chunks:
//   pv_zone_members_rows_kernel, pv_zone_members_merge_kernel: members, smallest and largest onset of every zone (integers:
//                                     the order does not matter).
// A block is reduced while the samples of the next block and the label and onset of the one after are in flight.  edc, the fits
// and the empty-zone values are the host's (zoneDecayFinish).  Plane offsets are 64-bit throughout.  Only vector stores; nothing
// is atomic.
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

// the kept history: every row and block of the map, step t in plane t
struct ZoneHistorySource {
    using Args = ZoneCurveArgs;
    static constexpr bool kRing = false;
    const ZoneCurveArgs& c;
    __device__ __forceinline__ ZoneHistorySource(const Args& a, int) : c(a) {}
    __host__ __device__ __forceinline__ static const ZoneCurveArgs& common(const Args& a) { return a; }
    __device__ __forceinline__ ZoneCurveCell cellAt(int X, int Y) const { return zoneCurveCellAt(c, X, Y); }
    __device__ __forceinline__ int plane(int t, int) const { return t; }
    __device__ __forceinline__ static int row0(const Args&) { return 0; }
    __device__ __forceinline__ static int rows(const Args& a) { return a.gx; }
    __device__ __forceinline__ static int blk0(const Args&) { return 0; }
    __device__ __forceinline__ static int blks(const Args& a) { return (a.gy + kZoneBlock - 1) / kZoneBlock; }
};

// the ring of a sparse-emitter run, for a group of steps that begins at j0: the labels' bounding box, step j0 + k in plane
// (j0 + k) % ring, kept as a running index from r0 = j0 % ring
struct ZoneRingSource {
    using Args = ZoneRingCurveArgs;
    static constexpr bool kRing = true;
    const ZoneRingCurveArgs& a;
    ZoneWindow w;                  // the run's, from *dyn (the whole tile grid in this mode; checked all the same)
    int planeOf[kZoneCurveSlots];  // the plane of step j0 + k, found once for both load groups of the block loop
    __device__ __forceinline__ ZoneRingSource(const Args& args, int j0) : a(args) {
        const int r0 = j0 % a.ring;
#pragma unroll
        for (int k = 0; k < kZoneCurveSlots; ++k) planeOf[k] = (r0 + k) % a.ring;  // (wave-uniform)
        const DynParams dyn = *a.dyn;
        const int rxi = a.c.w.rxi, wi = a.c.w.wi;
        w = ZoneWindow{dyn.histRow0 - a.G, dyn.histCol0 - a.G, dyn.histTilesX * rxi, dyn.histTilesY * wi, rxi, wi, dyn.histTilesY};
    }
    __host__ __device__ __forceinline__ static const ZoneCurveArgs& common(const Args& a) { return a.c; }
    __device__ __forceinline__ ZoneCurveCell cellAt(int X, int Y) const {
        const ZoneCurveCell none{0, 0, 0};
        if (Y >= a.c.gy) return none;
        const long long s = (long long)X * a.c.gy + Y;
        const int label = (int)a.c.labels[s];
        if (label == 0) return none;
        const int on = a.onset[s];
        if (on < 0 || on >= a.c.T || !zoneWindowHas(w, X, Y)) return none;
        const long long g = zoneWindowOffset(w, X, Y);
        if (g >= a.c.histPlane) return none;
        return ZoneCurveCell{label, on, g};
    }
    __device__ __forceinline__ int plane(int, int k) const { return planeOf[k]; }
    __device__ __forceinline__ static int row0(const Args& a) { return a.row0; }
    __device__ __forceinline__ static int rows(const Args& a) { return a.nRows; }
    __device__ __forceinline__ static int blk0(const Args& a) { return a.blk0; }
    __device__ __forceinline__ static int blks(const Args& a) { return a.nBlks; }
};

template <bool ONSET, class Source>
__global__ __launch_bounds__(kZoneCurveBlock) void pv_zone_curve_rows_kernel(const typename Source::Args args) {
    static_assert(!(ONSET && Source::kRing), "an ONSET curve needs the whole history");
    constexpr int TC = kZoneCurveSlots;
    const ZoneCurveArgs& a = Source::common(args);
    const int lane = threadIdx.x & 63;
    const int xr = blockIdx.x * (kZoneCurveBlock / 64) + (threadIdx.x >> 6);
    if (xr >= Source::rows(args)) return;  // (wave-uniform)
    const int X = Source::row0(args) + xr;
    const int jl0 = blockIdx.y * TC;                           // the group's first slot inside the chunk
    const int j0 = a.slot0 + jl0;                              // ... and in the curve
    const int nj = a.slots - jl0 < TC ? a.slots - jl0 : TC;   // its slots (the chunk's last group may be short)
    const Source src(args, j0);
    double acc[TC];
#pragma unroll
    for (int k = 0; k < TC; ++k) acc[k] = 0.0;
    // a member with a sample in some slot of the group
    const auto liveIn = [&](const ZoneCurveCell& c) { return c.label != 0 && (ONSET ? c.t0 + j0 < a.T : c.t0 <= j0 + nj - 1); };
    // the group's samples of a block's cell (+0.0f where the cell has none)
    const auto loadGroup = [&](const ZoneCurveCell& c, bool live, float (&p)[TC]) {
        const float* __restrict__ h = a.hist + c.g;
#pragma unroll
        for (int k = 0; k < TC; ++k) {
            const int t = ONSET ? c.t0 + j0 + k : j0 + k;
            const bool has = live && k < nj && t >= c.t0 && t < a.T;
            p[k] = has ? h[(long long)src.plane(t, k) * a.histPlane] : 0.0f;
        }
    };
    // two blocks ahead: block b is reduced while the samples of block b + 1 and the label and onset of block b + 2 are in flight
    const int bEnd = Source::blk0(args) + Source::blks(args);
    ZoneCurveCell c = src.cellAt(X, Source::blk0(args) * kZoneBlock + lane);
    bool live = liveIn(c);
    float p[TC];
    loadGroup(c, live, p);
    ZoneCurveCell c1 = Source::blks(args) > 1 ? src.cellAt(X, (Source::blk0(args) + 1) * kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
    for (int b = Source::blk0(args); b < bEnd; ++b) {
        const bool live1 = liveIn(c1);  // (label 0 past the last block)
        float p1[TC];
        loadGroup(c1, live1, p1);
        const ZoneCurveCell c2 = b + 2 < bEnd ? src.cellAt(X, (b + 2) * kZoneBlock + lane) : ZoneCurveCell{0, 0, 0};
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
        if (k < nj) a.rows[((long long)(jl0 + k) * a.nZones + lane) * Source::rows(args) + xr] = acc[k];
}

// slot slot0 + blockIdx.y of zone blockIdx.x: the sums of the nRows rows the rows kernel walked, in increasing X
__global__ __launch_bounds__(64) void pv_zone_curve_merge_kernel(const ZoneCurveArgs a, const int nRows) {
    const int lane = threadIdx.x;
    const int z = blockIdx.x, sl = blockIdx.y;
    const double* __restrict__ rows = a.rows + ((long long)sl * a.nZones + z) * nRows;
    double total = 0.0;
    for (int X0 = 0; X0 < nRows; X0 += 64) {
        const int X = X0 + lane;
        const double r = X < nRows ? rows[X] : 0.0;
        // increasing X, wave-uniform (pv_zone_merge_kernel); the rows past the last add +0.0, which changes no bit
#pragma unroll
        for (int i = 0; i < 64; ++i) total = total + zoneReadLane(r, i);
    }
    if (lane == 0) a.etc[(long long)z * a.T + a.slot0 + sl] = total;
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

// the rows kernel of a source over nRows rows and the merge kernel, for the chunk slot0 .. slot0 + slots - 1 of the common arguments
template <bool ONSET, class Source>
void launchZoneCurveChunk(const typename Source::Args& a, int nRows, hipStream_t stream) {
    const ZoneCurveArgs& c = Source::common(a);
    const dim3 rowsGrid((unsigned)((nRows + kZoneCurveBlock / 64 - 1) / (kZoneCurveBlock / 64)),
                        (unsigned)((c.slots + kZoneCurveSlots - 1) / kZoneCurveSlots));
    hipLaunchKernelGGL((pv_zone_curve_rows_kernel<ONSET, Source>), rowsGrid, dim3(kZoneCurveBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_curve_merge_kernel, dim3((unsigned)c.nZones, (unsigned)c.slots), dim3(64), 0, stream, c, nRows);
}

}  // namespace

void launchZoneMembers(const ZoneCurveArgs& a, hipStream_t stream) {
    const dim3 rowsGrid((unsigned)((a.gx + kZoneCurveBlock / 64 - 1) / (kZoneCurveBlock / 64)));
    hipLaunchKernelGGL(pv_zone_members_rows_kernel, rowsGrid, dim3(kZoneCurveBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_members_merge_kernel, dim3((unsigned)a.nZones), dim3(64), 0, stream, a);
}

// slots a.slot0 .. a.slot0 + a.slots - 1 of every zone's etc, off the kept history
void launchZoneCurves(const ZoneCurveArgs& a, bool onset, hipStream_t stream) {
    if (onset)
        launchZoneCurveChunk<true, ZoneHistorySource>(a, a.gx, stream);
    else
        launchZoneCurveChunk<false, ZoneHistorySource>(a, a.gx, stream);
}

// steps [tA, min(tB, T)) of every zone's etc, off the ring, in chunks of `chunk` steps
void launchStreamZoneCurves(const ZoneRingCurveArgs& a, int tA, int tB, int chunk, hipStream_t stream) {
    const int tEnd = tB < a.c.T ? tB : a.c.T;
    ZoneRingCurveArgs s = a;
    for (int t0 = tA; t0 < tEnd; t0 += chunk) {
        s.c.slot0 = t0;
        s.c.slots = tEnd - t0 < chunk ? tEnd - t0 : chunk;
        launchZoneCurveChunk<false, ZoneRingSource>(s, s.nRows, stream);
    }
}

}  // namespace pva
