// pv_zone_band_decay.h -- per-zone ensemble decay curves PER BAND, and the clarity of an energy-time curve: the definition of
// include/planeverb_amd.h (PvAmdZoneBandDecay), shared by the device pass (pv_zone_band_decay.hip) and the host restatements
// (PvAmdHostZoneBandDecay, PvAmdHostZoneCurveClarity).  It composes three rules that exist and adds one:
//   filter   pv_bands.h bandFilterStep: the band's two float32 sections, backwards from t = T - 1 (state +0.0f) down to the cell's
//            onset t0 and no further; y_{s,b}(t) for t0 <= t < T;
//   etc      pv_zone_decay.h, word for word, with y in the place of p: the three-level sum of pv_zones.h per time slot over
//            v = (double)y * (double)y;
//   finish   pv_zone_decay.h zoneDecayFinish on etc[z][b]: edc, e0, the fits, depth -- the one copy;
//   clarity  zoneCurveClarity below (new): C50, C80, D50 and Ts of ONE curve, in double.
// Every add, product and quotient is rounded on its own (-ffp-contract=off); log10 is the host libm's.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "pv_bands.h"
#include "pv_metrics.h"
#include "pv_zone_decay.h"

namespace pva {

constexpr int kZoneBandWave = 2;  // bands whose filter state a lane of the device pass carries (pv_zone_band_decay.hip; PV_BANDS_B)

// the record (PvAmdZoneBandDecay, include/planeverb_amd.h): ZoneDecay with the four clarity doubles behind depth
struct ZoneBandDecay {
    double edt, t20, t30, e0, depth, c50, c80, d50, ts;
    int n_edt, n_t20, n_t30, n_cells, t_first, t_last;
};
static_assert(sizeof(ZoneBandDecay) == 96, "PvAmdZoneBandDecay");

// One chunk of (zone, band) pairs for launchZoneBandCurves (pv_launch.h): the zones zone0 + 1 .. zone0 + zones and the bands
// band0 .. band0 + bands - 1, every pair with a row of T doubles per result row in c.rows.  c carries the history, the onset map,
// the labels, the window and the scratch as for the broadband pass (c.slot0 / c.slots are not used; c.etc = nZones x nBands x T)
struct ZoneBandCurveArgs {
    ZoneCurveArgs c;
    int nBands;  // of the whole call: the stride of c.etc
    int zone0, zones, band0, bands;
    float coefs[kBandsMax * kBandCoefs];  // of ALL bands
};

// The chunk rule.  A (zone, band) pair takes gx rows of T doubles of scratch; pairs are dealt so that a chunk's rows stay within
// `bound` bytes: all bands of as many whole zones as fit, or, where not even one zone's bands fit, one zone and as many bands as
// fit -- one pair where a single pair's rows exceed the bound: that is what it takes.  Returns the number of chunks
inline int zoneBandDecayChunks(int gx, int T, int nZones, int nBands, size_t bound, int* zonesPer, int* bandsPer) {
    const size_t perPair = (size_t)gx * (size_t)T * sizeof(double);
    const size_t fit = bound / perPair;
    int zp, bp;
    if (fit >= (size_t)nBands) {
        bp = nBands;
        zp = (int)(fit / (size_t)nBands < (size_t)nZones ? fit / (size_t)nBands : (size_t)nZones);
    } else {
        zp = 1;
        bp = fit < 1 ? 1 : (int)fit;
    }
    if (zonesPer) *zonesPer = zp;
    if (bandsPer) *bandsPer = bp;
    return ((nZones + zp - 1) / zp) * ((nBands + bp - 1) / bp);
}

// Clarity of an energy-time curve etc[0 .. T - 1] whose beginning is slot j0 (0 <= j0 < T): out4 = c50, c80, d50, ts.
//   edc[T] = +0.0, edc[j] = edc[j + 1] + etc[j] (zoneDecayFinish's); e0 = edc[j0];
//   n50 = (int)(0.05f * (float)fs), m50 = min(j0 + n50, T), l50 = edc[m50], e50 = etc[j0] + .. + etc[m50 - 1] in increasing j
//   from +0.0; n80 = (int)(0.08f * (float)fs) likewise; moment = the sum of (double)(j - j0) * etc[j], j = j0 .. T - 1, increasing;
//   c50 = 10 log10(e50 / l50), c80 likewise, d50 = e50 / (e50 + l50), ts = (moment / e0) / (double)fs.
// Nothing is special-cased: l50 = +0.0 gives c50 = +inf and d50 = 1, an all-zero curve gives NaNs
inline void zoneCurveClarity(const double* etc, int T, int fs, int j0, double out4[4]) {
    const int n50 = roomMetricsN50(fs), n80 = roomMetricsN80(fs);
    const int m50 = (long long)j0 + n50 < T ? j0 + n50 : T, m80 = (long long)j0 + n80 < T ? j0 + n80 : T;
    double E = 0.0, l50 = 0.0, l80 = 0.0, e0 = 0.0;
    for (int j = T - 1; j >= j0; --j) {
        E = E + etc[j];
        if (j == m50) l50 = E;
        if (j == m80) l80 = E;
        if (j == j0) e0 = E;
    }
    double e50 = 0.0, e80 = 0.0, moment = 0.0;
    for (int j = j0; j < T; ++j) {
        if (j < m50) e50 = e50 + etc[j];
        if (j < m80) e80 = e80 + etc[j];
        const double m = (double)(j - j0) * etc[j];
        moment = moment + m;
    }
    out4[0] = 10.0 * std::log10(e50 / l50);
    out4[1] = 10.0 * std::log10(e80 / l80);
    out4[2] = e50 / (e50 + l50);
    out4[3] = (moment / e0) / (double)fs;
}

// The record of zone z, band b from its etc[0 .. T - 1] and the zone's members (n_cells, t_first, t_last as reduced): the shared
// finish, then the clarity from the fits' j0 (ABSOLUTE: t_first; ONSET: 0; a zone without a member: 0, its curve is all +0.0)
inline void zoneBandDecayFinish(const double* etc, double* edc, int T, int fs, int align, int nCells, int tFirst, int tLast,
                                ZoneBandDecay* r) {
    ZoneDecay d{};
    d.n_cells = nCells;
    d.t_first = tFirst;
    d.t_last = tLast;
    zoneDecayFinish(etc, edc, T, fs, align, &d);
    r->edt = d.edt, r->t20 = d.t20, r->t30 = d.t30, r->e0 = d.e0, r->depth = d.depth;
    r->n_edt = d.n_edt, r->n_t20 = d.n_t20, r->n_t30 = d.n_t30;
    r->n_cells = d.n_cells, r->t_first = d.t_first, r->t_last = d.t_last;
    const int j0 = d.n_cells > 0 && align == kZoneDecayAbsolute ? d.t_first : 0;
    double c[4];
    zoneCurveClarity(etc, T, fs, j0, c);
    r->c50 = c[0], r->c80 = c[1], r->d50 = c[2], r->ts = c[3];
}

// The definition on the CPU: p, delay, labels as for zoneDecayOfHistory; coefs = nBands sets of ten floats; out = nZones x nBands
// records, etc / edc (either may be nullptr) = nZones x nBands x T, zone-major then band.  Per band the members' histories are
// filtered into a history of their own -- samples below an onset are neither read nor written -- and that history goes through
// zoneDecayOfHistory: the sum and the finish are that function's.  The caller has checked labels and onsets
inline void zoneBandDecayOfHistory(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels,
                                   int nZones, const float* coefs, int nBands, int align, ZoneBandDecay* out, double* etcOut,
                                   double* edcOut) {
    const size_t cells = (size_t)gx * gy;
    std::vector<float> y(cells * (size_t)T, 0.0f);
    std::vector<ZoneDecay> rec((size_t)nZones);
    std::vector<double> etc((size_t)nZones * T), edc((size_t)nZones * T);
    for (int b = 0; b < nBands; ++b) {
        const float* c10 = coefs + (size_t)kBandCoefs * b;
        for (size_t s = 0; s < cells; ++s) {
            if (!labels[s] || delay[s] == FLT_MAX) continue;
            const int t0 = (int)delay[s];
            float z[4] = {0.f, 0.f, 0.f, 0.f};
            for (int t = T - 1; t >= t0; --t) y[(size_t)t * cells + s] = bandFilterStep(c10, p[(size_t)t * cells + s], z);
        }
        zoneDecayOfHistory(y.data(), delay, gx, gy, T, fs, labels, nZones, align, rec.data(), etc.data(), edc.data());
        for (int z = 0; z < nZones; ++z) {
            const size_t at = ((size_t)z * nBands + b) * T;
            const ZoneDecay& d = rec[(size_t)z];
            // (the finish again on the same curve: the same bits, and the clarity behind it)
            zoneBandDecayFinish(etc.data() + (size_t)z * T, edc.data() + (size_t)z * T, T, fs, align, d.n_cells, d.t_first, d.t_last,
                                &out[(size_t)z * nBands + b]);
            for (int j = 0; j < T; ++j) {
                if (etcOut) etcOut[at + j] = etc[(size_t)z * T + j];
                if (edcOut) edcOut[at + j] = edc[(size_t)z * T + j];
            }
        }
    }
}

}  // namespace pva
