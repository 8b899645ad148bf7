// pv_zone_decay.h -- per-zone ensemble decay curves and the decay times read off them: the definition of include/planeverb_amd.h
// (PvAmdZoneDecay), shared by the device pass (pv_zone_decay.hip) and the host restatement (PvAmdHostZoneDecay).  The squared
// pressure histories of a zone's cells are summed into ONE energy-time curve etc[j] per zone -- by the three-level order of
// pv_zones.h, applied per time slot j to v = (double)p * (double)p, an exact product -- the Schroeder curve edc is its backward
// running sum, and EDT, T20 and T30 are the per-cell fits of pv_decay.h carried out in double on that one curve.
//
// The device computes etc and the three integers of a zone (members, smallest and largest onset); zoneDecayFinish -- called by both
// paths, as zoneStatFinish is -- makes edc and the record from them.  Every add, product and quotient is rounded on its own
// (-ffp-contract=off); log10 is the host libm's.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "pv_decay.h"
#include "pv_zones.h"

namespace pva {

constexpr int kZoneDecayAbsolute = 0;  // slot j = t: time since emission
constexpr int kZoneDecayOnset = 1;     // slot j = t - t0(s): every cell's beginning at slot 0
constexpr int kZoneCurveSlots = 16;    // consecutive slots a wave of the device pass keeps in registers (pv_zone_decay.hip)
constexpr int kZoneCurveMaxChunk = 32768;  // slots of one launch at the most (a multiple of kZoneCurveSlots; the merge grid's y)

// the record (PvAmdZoneDecay, include/planeverb_amd.h)
struct ZoneDecay {
    double edt, t20, t30, e0, depth;
    int n_edt, n_t20, n_t30, n_cells, t_first, t_last;
};
static_assert(sizeof(ZoneDecay) == 64, "PvAmdZoneDecay");

// what the device reduces besides etc: a zone's members (per result row in the scratch, then per zone)
struct ZoneMembers {
    int n_cells, t_first, t_last;  // INT_MAX / -1 while there is no member
};
static_assert(sizeof(ZoneMembers) == 12, "the scratch bound counts on it");

// One chunk of time slots for launchZoneCurves and what launchZoneMembers reads (pv_launch.h): the kept history of a run, step t
// in plane t, the run's onset map, the window as the run recorded it.  A cell outside the window has no sample recorded and is no
// member.  The band pass embeds this struct (pv_zone_band_decay.h), and so does the ring's below
struct ZoneCurveArgs {
    const float* hist;            // plane 0: planes of histPlane floats
    long long histPlane;
    const float* delay;           // gx * gy: the onset map, FLT_MAX = none
    const unsigned char* labels;  // gx * gy
    int gx, gy, nZones, T;
    ZoneWindow w;
    int slot0, slots;             // the chunk: slots slot0 .. slot0 + slots - 1
    double* rows;                 // slots x nZones x (rows walked): the row sums of the chunk
    double* etc;                  // nZones x T, zone-major
    ZoneMembers* memberRows;      // nZones x gx
    ZoneMembers* members;         // nZones
};

// ---- sparse-emitter mode: the ABSOLUTE curve inside the run (launchStreamZoneCurves).  c.hist is a ring of planes there, step t
// in plane t % ring, so the reduction runs per accumulate pass over the pass's steps, with the onsets that pass has just settled
// (slot t needs plane t and the onsets <= t only); origin and extent of the window are read from *dyn on the device (c.w gives rxi
// and wi; c.delay is not used).  The launch covers the labels' bounding box: a row or a 64-block without a labelled cell is
// skipped by the definition itself
struct DynParams;  // (pv_device.h)
struct ZoneRingCurveArgs {
    ZoneCurveArgs c;
    const int* onset;             // gx * gy: the accumulate pass's onsets, -1 = none yet
    const DynParams* dyn;         // the run's history window (device)
    int ring, G;
    int row0, nRows;              // the result rows of the launch: row0 .. row0 + nRows - 1
    int blk0, nBlks;              // ... and its blocks of 64 Y, aligned at Y = 0: blk0 .. blk0 + nBlks - 1
};

// The scratch of a curve pass: the row sums of one chunk | the curves | the zones' member rows, rounded up to 8 bytes | the
// zones' members.  Offsets in bytes, every one a multiple of 8 (a pass without row sums or curves gives 0 bytes for them)
struct ZoneCurveScratch {
    size_t rows, etc, memberRows, members, total;
};
inline ZoneCurveScratch zoneCurveScratch(size_t rowsBytes, size_t etcBytes, int nZones, int gx) {
    const size_t memberRowsBytes = ((size_t)nZones * (size_t)gx * sizeof(ZoneMembers) + 7) / 8 * 8;
    ZoneCurveScratch s;
    s.rows = 0;
    s.etc = rowsBytes;
    s.memberRows = s.etc + etcBytes;
    s.members = s.memberRows + memberRowsBytes;
    s.total = s.members + (size_t)nZones * sizeof(ZoneMembers);
    return s;
}

// What a zone's labels mean for the tiles and for the launch above (Solver::setZones): flags[ti * nty + tj] = 1 for every tile of
// rxi x wi result cells that holds a labelled cell -- ntx = ceil(gx / rxi) rows of nty = ceil(gy / wi) tiles --, the first and
// last labelled result row and the first and last labelled block of 64 Y.  Nothing labelled: no flag, rows 0 .. -1, blocks 0 .. -1
struct ZoneTileBox {
    int row0, row1, blk0, blk1;
};
inline ZoneTileBox zoneTileFlags(const unsigned char* labels, int gx, int gy, int rxi, int wi, unsigned char* flags) {
    const int ntx = (gx + rxi - 1) / rxi, nty = (gy + wi - 1) / wi;
    for (int t = 0; t < ntx * nty; ++t) flags[t] = 0;
    ZoneTileBox b{0, -1, 0, -1};
    bool any = false;
    for (int X = 0; X < gx; ++X)
        for (int Y = 0; Y < gy; ++Y) {
            if (!labels[(size_t)X * gy + Y]) continue;
            flags[(X / rxi) * nty + Y / wi] = 1;
            const int blk = Y / kZoneBlock;
            if (!any) b = ZoneTileBox{X, X, blk, blk};
            any = true;
            b.row1 = X;  // (X only grows)
            if (blk < b.blk0) b.blk0 = blk;
            if (blk > b.blk1) b.blk1 = blk;
        }
    return b;
}

// the tile plane of a sparse-emitter run: a tile stays in the ring and records for the whole run where it holds a registered
// emitter or -- while the curves are enabled -- a labelled cell.  Either side may be nullptr (none)
inline void zoneTileUnion(const unsigned char* emitterFlags, const unsigned char* zoneFlags, int ntiles, unsigned char* out) {
    for (int t = 0; t < ntiles; ++t) out[t] = ((emitterFlags && emitterFlags[t]) || (zoneFlags && zoneFlags[t])) ? 1 : 0;
}

// the slots that one pair of launches takes: whole groups of kZoneCurveSlots whose row sums (a double per slot, zone and row
// walked -- the map's rows, or the box's in an accumulate pass) stay within scratchBytes -- one group where even that is more
inline int streamZoneCurveChunk(int nZones, int rows, size_t scratchBytes) {
    const size_t perSlot = (size_t)(nZones > 1 ? nZones : 1) * (size_t)(rows > 1 ? rows : 1) * sizeof(double);
    const size_t fit = scratchBytes / perSlot / kZoneCurveSlots * kZoneCurveSlots;
    if (fit < (size_t)kZoneCurveSlots) return kZoneCurveSlots;
    return (int)(fit < (size_t)kZoneCurveMaxChunk ? fit : (size_t)kZoneCurveMaxChunk);
}

// the refusals of PvAmdHostZoneDecay beyond the labels' (nullptr: fine): every labelled cell with an onset has it inside the run
inline const char* zoneDecayOnsetsError(const float* delay, const unsigned char* labels, long long cells, int T) {
    for (long long s = 0; s < cells; ++s)
        if (labels[s] && delay[s] != FLT_MAX && !(delay[s] >= 0.0f && delay[s] < (float)T)) return "zone decay: an onset outside 0 .. T - 1";
    return nullptr;
}

// One range's regression in double (pv_decay.h DecayFit: the steps arrive in DECREASING j, so the first one has the largest k)
inline void zoneDecayFitStep(DecayFit& f, bool in, int k, double y) {
    if (!in) return;
    const double ky = (double)k * y;
    f.sy = f.sy + y;
    f.sky = f.sky + ky;
    if (f.n == 0) f.kmax = k;
    f.kmin = k;
    ++f.n;
}

inline double zoneDecayFitValue(const DecayFit& f, bool complete, int fs) {
    if (!complete || f.n < 2) return std::numeric_limits<double>::quiet_NaN();
    const double n = (double)f.n;
    const double kbar = ((double)f.kmin + (double)f.kmax) * 0.5;
    const double slope = (f.sky - (kbar * f.sy)) / ((n * ((n * n) - 1.0)) / 12.0);
    return (-60.0 / slope) / (double)fs;
}

// edc[0 .. T - 1] and the record of one zone from its etc[0 .. T - 1] and its members (r->n_cells, t_first, t_last as reduced:
// a zone without a member may carry any t_first / t_last)
inline void zoneDecayFinish(const double* etc, double* edc, int T, int fs, int align, ZoneDecay* r) {
    double E = 0.0;
    for (int j = T - 1; j >= 0; --j) {
        E = E + etc[j];
        edc[j] = E;
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    r->n_edt = r->n_t20 = r->n_t30 = 0;
    if (r->n_cells <= 0) {
        r->n_cells = 0;
        r->t_first = r->t_last = -1;
        r->e0 = 0.0;
        r->edt = r->t20 = r->t30 = r->depth = qnan;
        return;
    }
    const int tailN = decayTailN(fs);
    const int j0 = align == kZoneDecayAbsolute ? r->t_first : 0;
    const int jEnd = align == kZoneDecayAbsolute ? T - tailN : T - tailN - r->t_last;
    const double e0 = edc[j0];
    r->e0 = e0;
    DecayFit f[kDecayRanges] = {{0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}, {0., 0., 0, 0, 0}};
    const bool beforeTail = j0 < jEnd;
    double rEnd = 0.0;
    if (beforeTail) {
        rEnd = edc[jEnd - 1] / e0;
        for (int j = jEnd - 1; j >= j0; --j) {
            const double q = edc[j] / e0;
            if (!(q >= (double)kDecayLoAll)) continue;  // (below every range, or NaN: the level is needed by no sum)
            const double L = 10.0 * std::log10(q);
            for (int i = 0; i < kDecayRanges; ++i) zoneDecayFitStep(f[i], q <= (double)kDecayHi[i] && q >= (double)kDecayLo[i], j - j0, L);
        }
    }
    double v[kDecayRanges];
    for (int i = 0; i < kDecayRanges; ++i) v[i] = zoneDecayFitValue(f[i], beforeTail && rEnd < (double)kDecayLo[i], fs);
    r->edt = v[0];
    r->t20 = v[1];
    r->t30 = v[2];
    r->n_edt = f[0].n;
    r->n_t20 = f[1].n;
    r->n_t30 = f[2].n;
    r->depth = beforeTail ? 10.0 * std::log10(rEnd) : qnan;
}

// The definition on the CPU: p = T planes of gx * gy floats (p[t * gx * gy + X * gy + Y], what PvAmdCopyHistoryPlane gives at
// array cell (X, Y)), delay and labels = gx * gy; out = nZones records, etc / edc (either may be nullptr) = nZones x T, zone-major.
// The caller has checked labels and onsets (zoneLabelsError, zoneDecayOnsetsError)
inline void zoneDecayOfHistory(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels, int nZones,
                               int align, ZoneDecay* out, double* etcOut, double* edcOut) {
    const size_t cells = (size_t)gx * gy;
    const int nb = (gy + kZoneBlock - 1) / kZoneBlock;
    std::vector<double> total((size_t)nZones * T, 0.0), row((size_t)nZones * T);
    std::vector<unsigned char> rowUsed((size_t)nZones);
    for (int z = 0; z < nZones; ++z) out[z].n_cells = 0, out[z].t_first = INT32_MAX, out[z].t_last = -1;
    double v[kZoneBlock];
    int t0[kZoneBlock];
    for (int X = 0; X < gx; ++X) {
        for (int z = 0; z < nZones; ++z) rowUsed[(size_t)z] = 0;
        for (int b = 0; b < nb; ++b) {
            const int y0 = b * kZoneBlock, n = gy - y0 < kZoneBlock ? gy - y0 : kZoneBlock;
            const size_t s0 = (size_t)X * gy + y0;
            uint64_t present = 0;
            for (int i = 0; i < n; ++i) {
                t0[i] = -1;  // no member
                if (!labels[s0 + i] || delay[s0 + i] == FLT_MAX) continue;
                t0[i] = (int)delay[s0 + i];
                present |= 1ull << (labels[s0 + i] - 1);
                ZoneDecay& r = out[labels[s0 + i] - 1];
                ++r.n_cells;
                if (t0[i] < r.t_first) r.t_first = t0[i];
                if (t0[i] > r.t_last) r.t_last = t0[i];
            }
            for (int z = 0; z < nZones; ++z) {
                if (!(present >> z & 1)) continue;
                double* acc = row.data() + (size_t)z * T;
                if (!rowUsed[(size_t)z]) {
                    rowUsed[(size_t)z] = 1;
                    for (int j = 0; j < T; ++j) acc[j] = 0.0;
                }
                int tmin = T;
                for (int i = 0; i < n; ++i)
                    if (t0[i] >= 0 && labels[s0 + i] == z + 1 && t0[i] < tmin) tmin = t0[i];
                // the slots for which a member of the block has a sample: ABSOLUTE j >= tmin, ONSET j < T - tmin
                const int ja = align == kZoneDecayAbsolute ? tmin : 0, jb = align == kZoneDecayAbsolute ? T : T - tmin;
                for (int j = ja; j < jb; ++j) {
                    for (int i = 0; i < kZoneBlock; ++i) {
                        v[i] = 0.0;
                        if (i >= n || t0[i] < 0 || labels[s0 + i] != z + 1) continue;
                        const int t = align == kZoneDecayAbsolute ? j : t0[i] + j;
                        if (t < t0[i] || t >= T) continue;
                        const double x = (double)p[(size_t)t * cells + s0 + i];
                        v[i] = x * x;
                    }
                    acc[j] = acc[j] + zoneBlockSum(v);
                }
            }
        }
        for (int z = 0; z < nZones; ++z) {
            if (!rowUsed[(size_t)z]) continue;
            const double* acc = row.data() + (size_t)z * T;
            double* tot = total.data() + (size_t)z * T;
            for (int j = 0; j < T; ++j) tot[j] = tot[j] + acc[j];
        }
    }
    std::vector<double> edc((size_t)T);
    for (int z = 0; z < nZones; ++z) {
        const double* e = total.data() + (size_t)z * T;
        zoneDecayFinish(e, edc.data(), T, fs, align, &out[z]);
        for (int j = 0; j < T; ++j) {
            if (etcOut) etcOut[(size_t)z * T + j] = e[j];
            if (edcOut) edcOut[(size_t)z * T + j] = edc[(size_t)j];
        }
    }
}

}  // namespace pva
