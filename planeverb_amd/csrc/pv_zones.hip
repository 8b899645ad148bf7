// pv_zones.hip -- per-zone statistics of a per-cell analysis map (pv_zones.h has the definition and its order of summation).
//
// The map is `planes` SoA planes in the tile-major history layout; the labels are row-major over the result map.  Four launches
// per chunk of planes:
//   pv_zone_rows_kernel<false>   a wave owns one result row X of one plane and walks it in blocks of 64 consecutive Y, one per lane
//                                (a block touches at most three tile rows' pieces of the plane, each contiguous).  The labels
//                                present in a block are found by a ballot loop; per label the wave counts the four classes (ballot
//                                + popcount), reduces the finite members' (double)x by the butterfly of the definition
//                                (DPP row shifts for the steps inside a row of 16 lanes, __shfl_down across rows: lane 0 ends
//                                with v[0]) and finds their extremes: the value by a DPP / shuffle all-reduce, its cell as the
//                                first lane that holds it.
//                                Lane z - 1 keeps zone z's row accumulators in registers (nZones <= 64), so no LDS is needed, and
//                                writes the row's record to scratch;
//   pv_zone_merge_kernel<false>  a wave per (zone, plane) adds the row sums in increasing X -- 64 rows per load, the adds
//                                wave-uniform -- merges counts and extremes (order-independent: the comparison breaks ties by
//                                cell), and leaves sum, mean, counts and extremes in the record;
//   pv_zone_rows_kernel<true>, pv_zone_merge_kernel<true>: the same walk over d * d, d = (double)x - mean, for m2.
// The next block's label and value are loaded before the current block is reduced.  std and the empty-zone values are the host's
// (zoneStatFinish).  Only vector stores; nothing is atomic.
#include <hip/hip_runtime.h>

#include <climits>

#include "pv_launch.h"
#include "pv_zones.h"
#include "pv_zones_dev.h"

namespace pva {

namespace {

constexpr int kZoneRowsBlock = 256;  // four waves: four consecutive rows of one plane (they share the lines of a tile's rows)

// (value, cell) of an extreme; cell == INT_MAX: none
struct Extreme {
    float v;
    int cell;
};

// does b replace a?  LESS: the minimum, else the maximum; -0.0f == +0.0f, a tie goes to the smaller cell
template <bool LESS>
__device__ __forceinline__ bool zoneBetter(const Extreme& a, const Extreme& b) {
    if (b.cell == INT_MAX) return false;
    if (a.cell == INT_MAX) return true;
    return (LESS ? b.v < a.v : b.v > a.v) || (b.v == a.v && b.cell < a.cell);
}

template <bool LESS>
__device__ __forceinline__ Extreme zoneWaveExtreme(Extreme e) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        Extreme o;
        o.v = __shfl_xor(e.v, s);
        o.cell = __shfl_xor(e.cell, s);
        if (zoneBetter<LESS>(e, o)) e = o;
    }
    return e;
}

// the smallest (LESS) or largest value of the wave in every lane: quads, halves of a row and rows by DPP, then across the rows
template <bool LESS>
__device__ __forceinline__ float zoneWaveBest(float m) {
    const auto pick = [](float a, float b) { return (LESS ? b < a : b > a) ? b : a; };
    m = pick(m, zoneDpp<0xB1>(m));   // quad_perm [1, 0, 3, 2]
    m = pick(m, zoneDpp<0x4E>(m));   // quad_perm [2, 3, 0, 1]
    m = pick(m, zoneDpp<0x141>(m));  // row_half_mirror: the other quad of the half
    m = pick(m, zoneDpp<0x140>(m));  // row_mirror: the other half of the row
    m = pick(m, __shfl_xor(m, 16));
    m = pick(m, __shfl_xor(m, 32));
    return m;
}

// The extreme of a block's members (at least one) with its cell: the value by zoneWaveBest, then the FIRST lane that holds it --
// the smallest Y, so the smallest cell; -0.0f == +0.0f -- and that lane's own bits.  cell0 = the cell of lane 0
template <bool LESS>
__device__ __forceinline__ Extreme zoneBlockExtreme(float x, bool member, int cell0) {
    const float best = zoneWaveBest<LESS>(member ? x : (LESS ? __builtin_inff() : -__builtin_inff()));
    const int src = __ffsll((long long)__ballot(member && x == best)) - 1;
    return Extreme{__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), src)), cell0 + src};
}

// label and value of result cell (X, Y): label 0 past gy; NaN outside the map's history window
struct ZoneCell {
    int label;
    float x;
};
__device__ __forceinline__ ZoneCell zoneCellAt(const ZoneArgs& a, const float* __restrict__ plane, int X, int Y) {
    ZoneCell c;
    c.label = Y < a.gy ? (int)a.labels[(long long)X * a.gy + Y] : 0;
    c.x = __builtin_nanf("");
    if (c.label != 0 && zoneWindowHas(a.w, X, Y)) {
        const long long g = zoneWindowOffset(a.w, X, Y);
        if (g < a.histPlane) c.x = plane[g];
    }
    return c;
}

template <bool M2>
__global__ __launch_bounds__(kZoneRowsBlock) void pv_zone_rows_kernel(const ZoneArgs a) {
    const int lane = threadIdx.x & 63;
    const int X = blockIdx.x * (kZoneRowsBlock / 64) + (threadIdx.x >> 6);
    const int p = blockIdx.y;
    if (X >= a.gx) return;  // (wave-uniform)
    const float* __restrict__ plane = a.map + (long long)p * a.histPlane;
    const bool owner = lane < a.nZones;  // lane z - 1 keeps zone z
    double acc = 0.0, mean = 0.0;
    if (M2 && owner) mean = a.out[(long long)lane * a.totalPlanes + a.plane0 + p].mean;
    int nf = 0, nn = 0, np = 0, nm = 0;
    Extreme lo{0.f, INT_MAX}, hi{0.f, INT_MAX};
    const int nb = (a.gy + kZoneBlock - 1) / kZoneBlock;
    ZoneCell next = zoneCellAt(a, plane, X, lane);
    for (int b = 0; b < nb; ++b) {
        const ZoneCell c = next;
        const int Y = b * kZoneBlock + lane;
        if (b + 1 < nb) next = zoneCellAt(a, plane, X, Y + kZoneBlock);
        const bool fin = zoneFinite(c.x);
        unsigned long long left = __ballot(c.label != 0);
        while (left) {
            const int z = __builtin_amdgcn_readlane(c.label, __ffsll((long long)left) - 1);
            const bool mine = c.label == z;
            left &= ~__ballot(mine);
            const bool member = mine && fin;
            const double zmean = M2 ? zoneReadLane(mean, z - 1) : 0.0;  // (read here, where every lane is active)
            double v = 0.0;
            if (member) {
                if (M2) {
                    const double d = (double)c.x - zmean;
                    v = d * d;
                } else {
                    v = (double)c.x;
                }
            }
            const double bv = zoneWaveBlockSum(v);
            if (lane == z - 1) acc = acc + bv;
            if (!M2) {
                const int cf = __popcll(__ballot(member)), cn = __popcll(__ballot(mine && c.x != c.x));
                const int cp = __popcll(__ballot(mine && c.x == __builtin_inff())), cm = __popcll(__ballot(mine && c.x == -__builtin_inff()));
                if (lane == z - 1) {
                    nf += cf;
                    nn += cn;
                    np += cp;
                    nm += cm;
                }
                if (cf) {  // (wave-uniform: no finite member, no extremes)
                    const int cell0 = X * a.gy + b * kZoneBlock;
                    const Extreme bl = zoneBlockExtreme<true>(c.x, member, cell0), bh = zoneBlockExtreme<false>(c.x, member, cell0);
                    if (lane == z - 1) {
                        if (zoneBetter<true>(lo, bl)) lo = bl;
                        if (zoneBetter<false>(hi, bh)) hi = bh;
                    }
                }
            }
        }
    }
    if (!owner) return;
    const long long at = ((long long)p * a.nZones + lane) * a.gx + X;
    if (M2) {
        a.rowM2[at] = acc;
    } else {
        ZoneRow r;
        r.sum = acc;
        r.min = lo.v;
        r.max = hi.v;
        r.argmin = lo.cell;
        r.argmax = hi.cell;
        r.n_finite = nf;
        r.n_nan = nn;
        r.n_posinf = np;
        r.n_neginf = nm;
        a.rows[at] = r;
    }
}

template <bool M2>
__global__ __launch_bounds__(64) void pv_zone_merge_kernel(const ZoneArgs a) {
    const int lane = threadIdx.x;
    const int z = blockIdx.x, p = blockIdx.y;
    const long long base = ((long long)p * a.nZones + z) * a.gx;
    double total = 0.0;
    int nf = 0, nn = 0, np = 0, nm = 0;
    Extreme lo{0.f, INT_MAX}, hi{0.f, INT_MAX};
    for (int X0 = 0; X0 < a.gx; X0 += 64) {
        const int X = X0 + lane;
        double r = 0.0;
        if (X < a.gx) {
            if (M2) {
                r = a.rowM2[base + X];
            } else {
                const ZoneRow row = a.rows[base + X];
                r = row.sum;
                nf += row.n_finite;
                nn += row.n_nan;
                np += row.n_posinf;
                nm += row.n_neginf;
                const Extreme rl{row.min, row.argmin}, rh{row.max, row.argmax};
                if (zoneBetter<true>(lo, rl)) lo = rl;
                if (zoneBetter<false>(hi, rh)) hi = rh;
            }
        }
        // increasing X, wave-uniform: lane i's row sum by two v_readlane (the unrolled i is a constant) into one dependent add each.
        // The rows past gx add +0.0, which changes no bit of a sum that started at +0.0
#pragma unroll
        for (int i = 0; i < 64; ++i)
            total = total + __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(r), i), __builtin_amdgcn_readlane(__double2loint(r), i));
    }
    ZoneStat* out = a.out + (long long)z * a.totalPlanes + a.plane0 + p;
    if (M2) {
        if (lane == 0) out->m2 = total;
        return;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        nf += __shfl_xor(nf, s);
        nn += __shfl_xor(nn, s);
        np += __shfl_xor(np, s);
        nm += __shfl_xor(nm, s);
    }
    lo = zoneWaveExtreme<true>(lo);
    hi = zoneWaveExtreme<false>(hi);
    if (lane != 0) return;
    ZoneStat r;
    r.sum = total;
    r.mean = zoneMean(total, nf);  // (no finite member: 0 / 0, never read by the m2 walk; the host writes the record's NaNs)
    r.m2 = r.std = 0.0;
    r.min = lo.v;
    r.max = hi.v;
    r.argmin = lo.cell == INT_MAX ? -1 : lo.cell;
    r.argmax = hi.cell == INT_MAX ? -1 : hi.cell;
    r.n_finite = nf;
    r.n_nan = nn;
    r.n_posinf = np;
    r.n_neginf = nm;
    *out = r;
}

}  // namespace

// a.planes planes from a.map on: the records of planes a.plane0 .. a.plane0 + a.planes - 1 into a.out
void launchZoneStats(const ZoneArgs& a, hipStream_t stream) {
    const dim3 rowsGrid((unsigned)((a.gx + kZoneRowsBlock / 64 - 1) / (kZoneRowsBlock / 64)), (unsigned)a.planes);
    const dim3 mergeGrid((unsigned)a.nZones, (unsigned)a.planes);
    hipLaunchKernelGGL(pv_zone_rows_kernel<false>, rowsGrid, dim3(kZoneRowsBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_merge_kernel<false>, mergeGrid, dim3(64), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_rows_kernel<true>, rowsGrid, dim3(kZoneRowsBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_merge_kernel<true>, mergeGrid, dim3(64), 0, stream, a);
}

}  // namespace pva
