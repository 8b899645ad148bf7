// pv_zone_maps.h -- sparse-emitter mode: the room-metrics and spectrum records of every labelled cell, accumulated inside the run
// (PvAmdSetZoneMaps; the kernels: pv_zone_maps.hip).  Both kinds are forward sums from the cell's onset (pv_metrics.h roomSumsStep,
// pv_spectrum.h spectrumStep), so a cell's sums are carried from one accumulate pass to the next in the record's own planes and end
// with the bits a walk over a kept history gives.
#pragma once

namespace pva {

struct DynParams;  // (pv_device.h)

constexpr unsigned kZoneMapRoomMetrics = 1u, kZoneMapSpectrum = 2u;  // PVA_ZMAP_*

// What the accumulate pass and the finish pass are told.  The ring and the maps share one layout (a cell's offset inside a history
// plane, pv_prims.h histOffset): step t of the ring lies in plane t % ring, float k of a record in plane k of its map.
struct ZoneMapArgs {
    const float* hist;            // the ring: planes of histPlane floats
    long long histPlane;
    const int* onset;             // gx * gy: the accumulate pass's onsets, -1 = none yet
    const unsigned char* labels;  // gx * gy, 0 = no zone
    const DynParams* dyn;         // the run's history window (device): the whole grid in this mode
    const int* tiles;             // the tiles that hold a labelled cell, ti * nty + tj each
    int nTiles;
    int gx, gy, G, rxi, wi, nty, ring, T, fs;
    int tA, tB;                   // the accumulate pass [tA, tB)
    float* room;                  // kRoomMetricFloats planes, nullptr: the kind is not selected
    float* spec;                  // 3 nBins planes, nullptr: the kind is not selected
    int nBins;
    const float* specPow;         // nBins: spow of every bin
};

// a slice of the bins as the spectrum's own passes deal them (Solver::specPasses_): `block` registers, rows of `block` {cos, sin}
// pairs indexed by absolute step
struct ZoneMapSpecSlice {
    int bin0, bins, block;
    const float* tab;
};

}  // namespace pva
