// pv_zones.h -- per-zone statistics of a per-cell analysis map: the definition of include/planeverb_amd.h (PvAmdZoneStat), shared
// by the device pass (pv_zones.hip) and the host restatement (PvAmdHostZoneStats).  A zone is a label per result cell; a record
// holds, for one zone and one plane of a map, the four class counts, the extremes of the finite members with their cells, and
// sum / mean / m2 / std in double.
//
// The sums follow ONE order, fixed by result coordinates alone (zoneBlockSum -> row -> zone):
//   block  the 64 values v(X, 64 b .. 64 b + 63) by a butterfly: for s = 1, 2, 4, 8, 16, 32: v[i] = v[i] + v[i + s] for every i
//          that is a multiple of 2 s; the block value is v[0];
//   row    the block values of row X added sequentially in increasing b, from +0.0;
//   zone   the row sums added sequentially in increasing X, from +0.0.
// v is (double)x -- or d * d, d = (double)x - mean -- for a finite member of the zone and +0.0 for every other cell and for the
// columns past gy.  Every add, the subtract and the product are rounded on their own (-ffp-contract=off).  A running sum that starts
// at +0.0 is never -0.0, so adding the +0.0 of a block or row WITHOUT a member changes no bit: both implementations skip those.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "pv_libm.h"

namespace pva {

constexpr int kZonesMax = 64;     // labels 1 .. nZones <= 64 (a wave's lane z - 1 keeps zone z's row accumulators)
constexpr int kZoneBlock = 64;    // cells of a butterfly block

// the record (PvAmdZoneStat, include/planeverb_amd.h)
struct ZoneStat {
    double sum, mean, m2, std;
    float min, max;
    int argmin, argmax;
    int n_finite, n_nan, n_posinf, n_neginf;
};
static_assert(sizeof(ZoneStat) == 64, "PvAmdZoneStat");

// Device scratch: what one row of one plane contributes to one zone (pv_zones.hip), [plane][zone][X]
struct ZoneRow {
    double sum;
    float min, max;
    int argmin, argmax;  // INT_MAX: no finite member in the row
    int n_finite, n_nan, n_posinf, n_neginf;
};
static_assert(sizeof(ZoneRow) == 40, "the scratch bound counts on it");

// The history window of a run in RESULT coordinates, rows [r0, r0 + nr) x columns [c0, c0 + nc), and what places a cell of it
// inside a tile-major plane (pv_zones_dev.h zoneWindowOffset).  Every zone pass carries one.  The plane's size stays a field of
// the pass's own arguments, beside the pointer it goes with: seven ints keep every kernel's argument block as it was, and the
// kernels of these passes sit at the scalar-register limit, where a moved argument is a measurable change
struct ZoneWindow {
    int r0, c0, nr, nc;
    int rxi, wi, tilesY;  // tile interior and tile columns of the window (pv_prims.h histOffset)
};

// One chunk of planes of a map for launchZoneStats (pv_launch.h).  A cell outside the map's window w is NaN, as the read-backs
// give it
struct ZoneArgs {
    const float* map;             // plane 0 of the chunk: `planes` planes of histPlane floats
    long long histPlane;
    const unsigned char* labels;  // gx * gy
    int gx, gy, nZones;
    ZoneWindow w;
    int planes;                   // of the chunk
    int plane0, totalPlanes;      // the chunk's first plane in the map, the map's planes
    ZoneRow* rows;                // planes x nZones x gx
    double* rowM2;                // planes x nZones x gx
    ZoneStat* out;                // nZones x totalPlanes, zone-major
};

// finite as the definition has it: x - x == 0 (false for NaN and both infinities)
PV_HD inline bool zoneFinite(float x) { return x - x == 0.0f; }

// an empty record: what the counts and extremes start from
PV_HD inline void zoneStatClear(ZoneStat* r) {
    r->sum = r->mean = r->m2 = r->std = 0.0;
    r->min = r->max = 0.0f;
    r->argmin = r->argmax = -1;
    r->n_finite = r->n_nan = r->n_posinf = r->n_neginf = 0;
}

// mean from sum (both passes need it between them)
PV_HD inline double zoneMean(double sum, int nFinite) { return sum / (double)nFinite; }

// what follows from sum, m2 and the counts; a zone without a finite member: sum = +0.0, the other values quiet NaN, no cells
inline void zoneStatFinish(ZoneStat* r) {
    if (r->n_finite > 0) {
        r->mean = zoneMean(r->sum, r->n_finite);
        r->std = std::sqrt(r->m2 / (double)r->n_finite);
        return;
    }
    r->sum = 0.0;
    r->mean = r->m2 = r->std = std::numeric_limits<double>::quiet_NaN();
    r->min = r->max = std::numeric_limits<float>::quiet_NaN();
    r->argmin = r->argmax = -1;
}

// the butterfly of one block (v is overwritten)
inline double zoneBlockSum(double v[kZoneBlock]) {
    for (int s = 1; s < kZoneBlock; s *= 2)
        for (int i = 0; i < kZoneBlock; i += 2 * s) v[i] = v[i] + v[i + s];
    return v[0];
}

// the refusals PvAmdSetZones and PvAmdHostZoneStats share (nullptr: fine)
inline const char* zoneLabelsError(const unsigned char* labels, long long cells, int nZones) {
    if (nZones < 1 || nZones > kZonesMax) return "zone statistics: nZones is 1 .. 64";
    if (!labels) return "zone statistics: null labels";
    for (long long i = 0; i < cells; ++i)
        if (labels[i] > nZones) return "zone statistics: a label above nZones";
    return nullptr;
}

// The definition on the CPU: map = gx * gy records of `planes` floats (what PvAmdCopy<Kind> returns), labels = gx * gy bytes,
// out = nZones x planes records, zone-major.  Two walks per plane: counts, extremes and sum; then m2 about the mean
inline void zoneStatsOfMap(const float* map, int gx, int gy, int planes, const unsigned char* labels, int nZones, ZoneStat* out) {
    const int nb = (gy + kZoneBlock - 1) / kZoneBlock;
    std::vector<double> row((size_t)nZones), total((size_t)nZones), mean((size_t)nZones);
    double v[kZoneBlock];
    for (int k = 0; k < planes; ++k) {
        for (int z = 0; z < nZones; ++z) zoneStatClear(&out[(size_t)z * planes + k]);
        for (int pass = 0; pass < 2; ++pass) {
            for (int z = 0; z < nZones; ++z) total[(size_t)z] = 0.0;
            for (int X = 0; X < gx; ++X) {
                for (int z = 0; z < nZones; ++z) row[(size_t)z] = 0.0;
                for (int b = 0; b < nb; ++b) {
                    const int y0 = b * kZoneBlock, n = gy - y0 < kZoneBlock ? gy - y0 : kZoneBlock;
                    const unsigned char* L = labels + (size_t)X * gy + y0;
                    const float* m = map + ((size_t)X * gy + y0) * planes + k;
                    uint64_t present = 0;
                    for (int i = 0; i < n; ++i)
                        if (L[i]) present |= 1ull << (L[i] - 1);
                    for (int z = 0; z < nZones; ++z) {
                        if (!(present >> z & 1)) continue;
                        ZoneStat& r = out[(size_t)z * planes + k];
                        for (int i = 0; i < kZoneBlock; ++i) {
                            v[i] = 0.0;
                            if (i >= n || L[i] != z + 1) continue;
                            const float x = m[(size_t)i * planes];
                            if (pass) {
                                if (zoneFinite(x)) {
                                    const double d = (double)x - mean[(size_t)z];
                                    v[i] = d * d;
                                }
                                continue;
                            }
                            const int cell = X * gy + y0 + i;
                            if (zoneFinite(x)) {
                                v[i] = (double)x;
                                if (r.n_finite == 0 || x < r.min) r.min = x, r.argmin = cell;  // (a tie keeps the smaller cell)
                                if (r.n_finite == 0 || x > r.max) r.max = x, r.argmax = cell;
                                ++r.n_finite;
                            } else if (x != x) {
                                ++r.n_nan;
                            } else if (x > 0.0f) {
                                ++r.n_posinf;
                            } else {
                                ++r.n_neginf;
                            }
                        }
                        row[(size_t)z] = row[(size_t)z] + zoneBlockSum(v);
                    }
                }
                for (int z = 0; z < nZones; ++z) total[(size_t)z] = total[(size_t)z] + row[(size_t)z];
            }
            for (int z = 0; z < nZones; ++z) {
                ZoneStat& r = out[(size_t)z * planes + k];
                if (pass) {
                    r.m2 = total[(size_t)z];
                    zoneStatFinish(&r);
                } else {
                    r.sum = total[(size_t)z];
                    mean[(size_t)z] = zoneMean(r.sum, r.n_finite);  // (no finite member: never read)
                }
            }
        }
    }
}

// labels from rectangles (PvAmdHostZoneRects): cell (X, Y) gets j + 1 where xmin_j <= (X + 0.5f) * dx < xmax_j and the same in z
// with Y, float32; later rectangles overwrite earlier ones; 0 elsewhere
inline void zoneLabelsFromRects(float dx, int gx, int gy, const float* rect4, int n, unsigned char* labels) {
    std::memset(labels, 0, (size_t)gx * gy);
    for (int j = 0; j < n; ++j) {
        const float* r = rect4 + 4 * j;
        for (int X = 0; X < gx; ++X) {
            const float cx = ((float)X + 0.5f) * dx;
            if (!(r[0] <= cx && cx < r[2])) continue;
            for (int Y = 0; Y < gy; ++Y) {
                const float cz = ((float)Y + 0.5f) * dx;
                if (r[1] <= cz && cz < r[3]) labels[(size_t)X * gy + Y] = (unsigned char)(j + 1);
            }
        }
    }
}

}  // namespace pva
