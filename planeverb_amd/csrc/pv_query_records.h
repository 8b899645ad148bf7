// pv_query_records.h -- the in-run per-query analysis records (PvAmdSetQueryRecords, pv_query_records.hip): the kinds, their record
// sizes, and what travels to the kernel
#pragma once

#include "pv_decay.h"
#include "pv_echo.h"
#include "pv_echogram.h"
#include "pv_lateral.h"
#include "pv_lobes.h"
#include "pv_metrics.h"

namespace pva {

// bit k of the kinds mask = PVA_QREC_* (include/planeverb_amd.h)
constexpr int kQrecRoomMetrics = 0, kQrecDecay = 1, kQrecLateral = 2, kQrecEchogram = 3, kQrecEchoCriterion = 4, kQrecLobes = 5;
constexpr int kQueryRecordKinds = 6;
constexpr unsigned kQueryRecordMask = (1u << kQueryRecordKinds) - 1u;
// queries of one launch: groups of 64 on blockIdx.y (PVA_RECORD_QUERIES_MAX)
constexpr int kMaxRecordQueries = 1024;

// the bit of a mask that names ONE of a family's `kinds` kinds, or -1
inline int oneKindBit(unsigned kind, int kinds) {
    for (int k = 0; k < kinds; ++k)
        if (kind == (1u << k)) return k;
    return -1;
}

struct QueryRecordArgs {
    const long long* cells;  // nq result-cell indices (-1: off the map), pinned host memory
    float* out;              // pinned host memory
    int nq;                  // <= kMaxRecordQueries
    unsigned kinds;
    int offset[kQueryRecordKinds];  // of a kind's nq x floats block inside out, in floats
    int floats[kQueryRecordKinds];  // per query
    int n50, n80;            // room metrics
    int n5, latN80;          // lateral fraction
    int tailN;               // decay times
    int ns, nSlots;          // echogram
    int nDs, nDm, nLs, nLm;  // echo criterion
    LobeEdges ed;            // lobes
    int nW;
    int mix;                 // the lanes are source arrays, a.hist their mix planes, a.delay their onsets (cells is not read)
};

}  // namespace pva
