// pv_zone_band_decay.hip -- per-zone ensemble decay curves per band (pv_zone_band_decay.h has the definition): the reduction of the
// band-FILTERED pressure history, [T][cells] -> [zones][bands][T].  The filter makes the pass sequential in time per cell; the
// summation order of pv_zones.h makes it a reduction across cells per time slot in a fixed order.  Time is NOT cut: a launch walks
// whole histories, and the work is dealt in chunks of (zone, band) pairs whose rows of T doubles fit the scratch bound
// (zoneBandDecayChunks) -- a band is filtered once per chunk it appears in, a cell is read only by the chunks its zone is in.
//
//   pv_zone_band_rows_kernel<ONSET>   a wave owns one result row X and a group of kZoneBandWave bands of the chunk, and walks the row
//                                     in blocks of 64 consecutive Y, one cell per lane (zoneCurveCellAt's rule: label, onset and the
//                                     offset inside a plane once per block).  A block is walked from the last slot down in groups of
//                                     sixteen -- the groups of the broadband pass, slots 16 g .. 16 g + 15 --: the lane takes the
//                                     group's samples (plane j in ABSOLUTE mode, plane t0 + j of its own onset in ONSET mode; only
//                                     where t0 <= t < T, so nothing below an onset or outside the history window is loaded), runs
//                                     bandFilterStep over them in decreasing time with its state in registers, and keeps the sixteen
//                                     y.  A lane without a sample for a slot takes no filter step there: before its first sample
//                                     (ONSET: j > T - 1 - t0) it holds the zero state, below its onset (ABSOLUTE: j < t0) it holds
//                                     what it has, and it contributes +0.0.  The next group's samples are in flight meanwhile.
//                                     Per band and per label present the wave runs zoneWaveBlockSums16 over (double)y * (double)y
//                                     and lanes 0 .. 15 add the sixteen block values into the pair's row in scratch,
//                                     rows[pair][X][j] -- the SAME wave for every block of the row, in increasing block order, so
//                                     the adds into a row are the definition's.  The scratch starts as +0.0 (the solver clears it per chunk).
//                                     Skipped wave-uniformly, because they could only add +0.0 to sums that are never -0.0: blocks
//                                     without a member of the chunk's zones, groups in which no lane has a sample (ABSOLUTE: every
//                                     group below the block's smallest onset ends the walk; ONSET: groups above T - 1 - the
//                                     smallest onset), labels without a sample in the group;
//   pv_zone_band_merge_kernel         a lane per (pair, slot) adds the row sums in increasing X from +0.0.
// The members come from launchZoneMembers (pv_zone_decay.hip); edc, the fits, the clarity and the empty-zone values are the host's
// (zoneBandDecayFinish).  Plane offsets are 64-bit throughout.  Only vector stores; nothing is atomic.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "pv_launch.h"
#include "pv_zone_band_decay.h"
#include "pv_zones_dev.h"

namespace pva {

namespace {

constexpr int kZoneBandBlock = 256;  // four waves: four consecutive rows of one band group (they share the lines of a tile's rows)

template <bool ONSET>
__global__ __launch_bounds__(kZoneBandBlock) void pv_zone_band_rows_kernel(const ZoneBandCurveArgs a) {
    constexpr int TC = kZoneCurveSlots, B = kZoneBandWave;
    const ZoneCurveArgs& c = a.c;
    const int lane = threadIdx.x & 63;
    const int X = blockIdx.x * (kZoneBandBlock / 64) + (threadIdx.x >> 6);
    if (X >= c.gx) return;  // (wave-uniform)
    const int bl0 = blockIdx.y * B;                                // the wave's first band inside the chunk
    const int nbw = a.bands - bl0 < B ? a.bands - bl0 : B;       // its bands (the chunk's last group may be short)
    const float* __restrict__ coef = a.coefs + (a.band0 + bl0) * kBandCoefs;
    const int T = c.T;
    const int groups = (T + TC - 1) / TC;
    const int nb = (c.gy + kZoneBlock - 1) / kZoneBlock;
    for (int b = 0; b < nb; ++b) {
        ZoneCurveCell cell = zoneCurveCellAt(c, X, b * kZoneBlock + lane);
        const int zl = cell.label - 1 - a.zone0;  // the zone inside the chunk
        if (zl < 0 || zl >= a.zones) cell.label = 0;
        const bool member = cell.label != 0;
        if (!__ballot(member)) continue;  // (wave-uniform)
        const int tmin = zoneWaveMin(member ? cell.t0 : T);
        // the groups in which some lane has a sample: ABSOLUTE j >= tmin, ONSET j <= T - 1 - tmin
        const int gLast = ONSET ? (T - 1 - tmin) / TC : groups - 1, gFirst = ONSET ? 0 : tmin / TC;
        const float* __restrict__ h = c.hist + cell.g;
        // the group's samples of the lane's cell (+0.0f where it has none)
        const auto loadGroup = [&](int g, float (&p)[TC]) {
#pragma unroll
            for (int k = 0; k < TC; ++k) {
                const int j = g * TC + k, t = ONSET ? cell.t0 + j : j;
                const bool has = member && t >= cell.t0 && t < T;
                p[k] = has ? h[(long long)t * c.histPlane] : 0.0f;
            }
        };
        float st[B][4];
#pragma unroll
        for (int q = 0; q < B; ++q)
#pragma unroll
            for (int i = 0; i < 4; ++i) st[q][i] = 0.0f;
        float p[TC];
        loadGroup(gLast, p);
        for (int g = gLast; g >= gFirst; --g) {
            float p1[TC];
            loadGroup(g - 1, p1);  // (no lane has a sample in a group below gFirst: nothing is loaded)
            const int j0 = g * TC;
            float y[B][TC];
            bool live = false;  // a sample in some slot of the group
#pragma unroll
            for (int k = TC - 1; k >= 0; --k) {
                const int j = j0 + k, t = ONSET ? cell.t0 + j : j;
                const bool has = member && t >= cell.t0 && t < T;
                live = live || has;
#pragma unroll
                for (int q = 0; q < B; ++q) {
                    y[q][k] = 0.0f;
                    if (q >= nbw) continue;  // (wave-uniform)
                    float z[4] = {st[q][0], st[q][1], st[q][2], st[q][3]};
                    const float yy = bandFilterStep(coef + q * kBandCoefs, p[k], z);
                    y[q][k] = has ? yy : 0.0f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) st[q][i] = has ? z[i] : st[q][i];
                }
            }
            unsigned long long left = __ballot(live);
            while (left) {  // (wave-uniform)
                const int z = __builtin_amdgcn_readlane(cell.label, __ffsll((long long)left) - 1);
                const bool mine = live && cell.label == z;
                left &= ~__ballot(mine);
#pragma unroll
                for (int q = 0; q < B; ++q) {
                    if (q >= nbw) break;  // (wave-uniform)
                    double v[TC];
#pragma unroll
                    for (int k = 0; k < TC; ++k) {
                        const double x = mine ? (double)y[q][k] : 0.0;
                        v[k] = x * x;
                    }
                    const double sums = zoneWaveBlockSums16(v, lane);  // lane k: slot k's block value
                    if (lane < TC && j0 + lane < T) {
                        double* r =
                            c.rows + (((long long)(z - 1 - a.zone0) * a.bands + (bl0 + q)) * c.gx + X) * (long long)T + j0 + lane;
                        *r = *r + sums;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < TC; ++k) p[k] = p1[k];
        }
    }
}

// slot blockIdx.x * 64 + lane of pair blockIdx.y of the chunk: the row sums in increasing X, from +0.0
__global__ __launch_bounds__(64) void pv_zone_band_merge_kernel(const ZoneBandCurveArgs a) {
    const ZoneCurveArgs& c = a.c;
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= c.T) return;
    const int pair = blockIdx.y, zl = pair / a.bands, bl = pair - zl * a.bands;
    const double* __restrict__ rows = c.rows + (long long)pair * c.gx * (long long)c.T + j;
    double total = 0.0;
    for (int X = 0; X < c.gx; ++X) total = total + rows[(long long)X * c.T];
    c.etc[((long long)(a.zone0 + zl) * a.nBands + (a.band0 + bl)) * c.T + j] = total;
}

}  // namespace

// etc of the chunk's (zone, band) pairs into a.c.etc; a.c.rows (zones x bands x gx x T doubles) is scratch the caller has cleared
void launchZoneBandCurves(const ZoneBandCurveArgs& a, bool onset, hipStream_t stream) {
    const ZoneCurveArgs& c = a.c;
    const dim3 rowsGrid((unsigned)((c.gx + kZoneBandBlock / 64 - 1) / (kZoneBandBlock / 64)),
                        (unsigned)((a.bands + kZoneBandWave - 1) / kZoneBandWave));
    if (onset)
        hipLaunchKernelGGL(pv_zone_band_rows_kernel<true>, rowsGrid, dim3(kZoneBandBlock), 0, stream, a);
    else
        hipLaunchKernelGGL(pv_zone_band_rows_kernel<false>, rowsGrid, dim3(kZoneBandBlock), 0, stream, a);
    hipLaunchKernelGGL(pv_zone_band_merge_kernel, dim3((unsigned)((c.T + 63) / 64), (unsigned)(a.zones * a.bands)), dim3(64), 0, stream, a);
}

}  // namespace pva
