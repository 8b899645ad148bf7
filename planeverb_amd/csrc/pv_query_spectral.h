// pv_query_spectral.h -- the in-run per-query FREQUENCY-RESOLVED records (PvAmdSetQuerySpectralRecords, pv_query_spectral.hip): band
// metrics, modulation and spectrum for the cells the six kinds of pv_query_records.h follow.  A selector, a pinned block and a
// kernel of their own: the PVA_QREC_* namespace and pv_query_records_kernel are untouched.
#pragma once

#include "pv_bands.h"
#include "pv_modulation.h"
#include "pv_query_records.h"
#include "pv_spectrum.h"

namespace pva {

// bit k of the kinds mask = PVA_QSPEC_* (include/planeverb_amd.h)
constexpr int kQspecBandMetrics = 0, kQspecModulation = 1, kQspecSpectrum = 2;
constexpr int kQuerySpectralKinds = 3;
constexpr unsigned kQuerySpectralMask = (1u << kQuerySpectralKinds) - 1u;
constexpr unsigned kQspecBandKinds = (1u << kQspecBandMetrics) | (1u << kQspecModulation);  // the kinds that follow setBands
// coefficient sets that travel with a launch: kBandsMax, and room for the zero sets that pad the last block of the band metrics
// (any register block up to 8 bands)
constexpr int kQspecCoefSets = 2 * kBandsMax;
// slices of the spectrum's bins: kSpectrumMaxBins in register blocks of 8 at the least
constexpr int kQspecMaxSlices = kSpectrumMaxBins / 8;

struct QuerySpectralSlice {
    int bin0, bins, block;  // the slice's first bin, its bins (<= block) and its register block (8 or 16)
    long long tabOff;       // of the slice's table inside specTab, in floats
};

struct QuerySpectralArgs {
    const long long* cells;  // nq result-cell indices (-1: off the map), pinned host memory
    float* out;              // pinned host memory
    int nq;                  // <= kMaxRecordQueries
    int items[kQuerySpectralKinds];   // work items (blockIdx.x) of a kind, 0 where it is not selected: blocks of bands, bands, slices
    int offset[kQuerySpectralKinds];  // of a kind's nq x floats block inside out, in floats
    int floats[kQuerySpectralKinds];  // per query
    int nBands;
    float coefs[kQspecCoefSets][kBandCoefs];  // the bands' coefficient sets, zero sets behind them
    int tailN, n50, n80;                      // band metrics
    const float* modTab;                      // modulation: row 0 of the device table
    const float* specTab;                     // spectrum: the device tables of all slices, and the bins' source powers
    const float* specPow;
    QuerySpectralSlice slice[kQspecMaxSlices];
    int mix;                 // the lanes are source arrays, a.hist their mix planes, a.delay their onsets (cells is not read)
};

}  // namespace pva
