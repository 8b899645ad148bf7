// pv_query_spectral.hip -- the frequency-resolved records of a run (band metrics, modulation, spectrum) for the cells of its
// registered queries, computed INSIDE the run (PvAmdSetQuerySpectralRecords): one launch directly behind the launch of
// pv_query_records.hip, in front of the run's last kernel, straight into pinned host memory.  No pass over the history window, no
// per-cell device storage, no host synchronisation of its own.
//
// One wave per block; blockIdx.y is the group of 64 queries (lane l of group g serves query i = 64 g + l), blockIdx.x a WORK ITEM,
// decoded wave-uniformly from the three counts of the argument struct:
//   band metrics   one item per block of PV_BANDS_B bands, the last block padded with zero coefficient sets as launchBandMetrics
//                  pads it (their records are not stored);
//   modulation     one item per band;
//   spectrum       one item per slice of the bins -- the slices, register blocks (8 or 16) and device table offsets that
//                  Solver::setSpectrumBins builds for the whole-map pass.
// An item is what ONE launch of the whole-map pass is: the same coefficient sets by value (kernel arguments, so they are read by
// scalar loads and sit in SGPRs), the same table slice.  A lane's cell comes from the query table (recordLaneOfCell), its record
// goes to the query's AoS slot at the item's offset: band b0 + j at b0 * 12 + j * 12, band j at 15 j, bin bin0 + j at 3 (bin0 + j).
// Between the two runs the body of the kind's whole-map pass (pv_bands_dev.h, pv_modulation_dev.h, pv_spectrum_dev.h), the SAME
// text the whole-map kernel is made of.
//
// Why a record has the whole-map record's bits although its wave mates are other cells:
//   band metrics   every piece of a lane's state is SELECTED on k = t - t0 >= 0 with the lane's own onset; the wave-uniform skips
//                  (the tail, `deep`) only decide whether steps are looked at whose membership is then decided per lane, by selects.
//   modulation     a lane below its onset feeds e = +0 into its 29 sums, and x + (+-0) keeps x's bits (pv_modulation.hip); the
//                  filter states are selected.  A wave of scattered cells only has MORE such steps (its smallest onset is lower).
//   spectrum       a lane outside its range feeds p = +0 (pv_spectrum.hip); the wave's chunks begin at ITS smallest onset, so the
//                  chunk boundaries differ from the whole-map wave's, but a lane's sums take the steps in ascending order either way.
// The tables are indexed by ABSOLUTE step, so a row address is wave-uniform whatever cells the lanes own: scalar loads, as before.
//
// In sparse-emitter mode (PvAmdSetEmitterRecords) the same kernel serves the registered emitters from their record traces
// (recordLaneOfTrace), as pv_query_records.hip does.
//
// For the source arrays (PvAmdComputeArrays) the lanes are the arrays and the history is their mix planes (recordLaneOfMix), as in
// pv_query_records.hip.
//
// Lanes at or above nq have no slot and no cell; a query off the map, outside the window or without an onset gets quiet NaNs.
// The stores are plain vector stores to host-coherent memory, all behind the loops; they are visible to the host when the stream
// has drained.  The device tables are uploaded where the kinds are selected and where the settings change (both wait for a run in
// flight), never from the enqueue path.
//
// Cost: the launch takes what its slowest work item takes as a lone wave, whatever the grid, the window or the number of queries.
// Registers: profiles/query_spectral_records.txt.
#include <hip/hip_runtime.h>

#include "pv_analysis.h"
#include "pv_analysis_dev.h"
#include "pv_bands_dev.h"
#include "pv_device.h"
#include "pv_launch.h"
#include "pv_modulation_dev.h"
#include "pv_query_spectral.h"
#include "pv_record_lane.h"
#include "pv_spectrum_dev.h"

namespace pva {

namespace {

static_assert(PV_BANDS_S <= 8 && PV_MODULATION_S <= 8 && PV_SPECTRUM_S <= 8,
              "launchQuerySpectral chooses the one-descriptor-per-chunk form for chunks of at most 8 planes");
static_assert(PV_BANDS_B <= kBandsMax && kBandsMax + PV_BANDS_B - 1 <= kQspecCoefSets, "the padded last block of bands reads zero sets");

// FORM (pv_record_lane.h RecordLaneForm): the registered queries' cells, the registered emitters of sparse-emitter mode with their
// record traces as the history (recordLaneOfTrace), or the source arrays with their mix planes (recordLaneOfMix)
template <bool CHUNK, int FORM>
__global__ __launch_bounds__(64) void pv_query_spectral_kernel(const AnalyzeArgs a, const QuerySpectralArgs q) {
    __shared__ double logTab[96];
    // the work item (wave-uniform): kind and ordinal inside the kind
    int item = (int)blockIdx.x, kind = 0;
    while (kind < kQuerySpectralKinds && item >= q.items[kind]) item -= q.items[kind++];
    if (kind >= kQuerySpectralKinds) return;
    const int lane = (int)threadIdx.x;
    if (kind == kQspecBandMetrics) fillLogTab(logTab, lane, 64);
    __syncthreads();

    const DynParams dyn = *a.dyn;
    const int i = 64 * (int)blockIdx.y + lane;  // the query (the group is wave-uniform)
    const bool slot = i < q.nq;
    const RecordLane ln = recordLaneOfForm<FORM>(a, dyn, q.cells, i, slot);
    // (a lane without a slot never stores: it is not live, and the NaN fill asks for the slot)
    float* rec = q.out + q.offset[kind] + (long long)(slot ? i : 0) * q.floats[kind];
    switch (kind) {
        case kQspecBandMetrics: {
            constexpr int B = PV_BANDS_B;
            const int b0 = item * B;
            BandBlockCoefs<B> cf;
#pragma unroll
            for (int j = 0; j < B; ++j)
#pragma unroll
                for (int k = 0; k < kBandCoefs; ++k) cf.c[j][k] = q.coefs[b0 + j][k];  // (zero sets behind the last band)
            const int nb = max(min(q.nBands - b0, B), 1);  // (an item has a real band: said so to the compiler)
            bandMetricsBody<PV_BANDS_S, PV_BANDS_NB, CHUNK, B>(a, ln, SlotStore{rec + b0 * kBandFloats}, cf, nb, LogTabLds{logTab}, q.tailN,
                                                               q.n50, q.n80);
            break;
        }
        case kQspecModulation: {
            ModBandCoefs cf;
#pragma unroll
            for (int k = 0; k < kBandCoefs; ++k) cf.c[k] = q.coefs[item][k];
            modulationBody<PV_MODULATION_S, PV_MODULATION_NB, CHUNK>(a, ln, SlotStore{rec + item * kModFloats}, cf, q.modTab);
            break;
        }
        case kQspecSpectrum: {
            const QuerySpectralSlice sl = q.slice[item];
            const SlotStore out{rec + kSpectrumFloats * sl.bin0};
            if (sl.block == 8)
                spectrumBody<8, PV_SPECTRUM_S, PV_SPECTRUM_NB, CHUNK>(a, ln, out, sl.bins, q.specTab + sl.tabOff, q.specPow + sl.bin0);
            else
                spectrumBody<16, PV_SPECTRUM_S, PV_SPECTRUM_NB, CHUNK>(a, ln, out, sl.bins, q.specTab + sl.tabOff, q.specPow + sl.bin0);
            break;
        }
        default: break;
    }
}

}  // namespace

// some q.items[k] != 0, 0 < q.nq <= kMaxRecordQueries; q.cells, q.out: device-visible pinned host memory (q.out holds, per selected
// kind, nq x floats[kind] floats from offset[kind] on); the tables on the device, the settings filled in by the caller
void launchQuerySpectral(const AnalyzeArgs& a, const QuerySpectralArgs& q, hipStream_t stream) {
    const dim3 grid((unsigned)(q.items[0] + q.items[1] + q.items[2]), (unsigned)((q.nq + 63) / 64));
    // (the largest chunk of the three passes is 8 planes: one descriptor per chunk below 2^31 bytes, as in their own launchers)
    // (record traces -- a.hist = a.recTrace, planes of at most 3 x 1024 floats -- always take the chunk form)
    // (mix planes -- q.mix, a.hist = the planes of at most kArraysMax floats -- too)
    if (q.mix)
        hipLaunchKernelGGL((pv_query_spectral_kernel<true, kLaneMix>), grid, dim3(64), 0, stream, a, q);
    else if (a.recTrace)
        hipLaunchKernelGGL((pv_query_spectral_kernel<true, kLaneTrace>), grid, dim3(64), 0, stream, a, q);
    else if (a.histPlane * 4 * 8 < (1ll << 31))
        hipLaunchKernelGGL((pv_query_spectral_kernel<true, kLaneCell>), grid, dim3(64), 0, stream, a, q);
    else
        hipLaunchKernelGGL((pv_query_spectral_kernel<false, kLaneCell>), grid, dim3(64), 0, stream, a, q);
}

}  // namespace pva
