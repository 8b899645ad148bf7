// pv_solver_arrays.cpp -- the source arrays of a Solver (pv_solver.h; the definition: pv_arrays.h; the passes: pv_arrays.hip): the
// setting with its expanded tap table and device tables, the mix of the last completed run -- off the history, or in sparse-emitter
// mode off the registered emitters' traces --, the onsets, the records of the selected kinds through the query record kernels
// with the mix planes as their history (recordLaneOfMix), the stamp and the refusals.  After the pattern of
// pv_solver_waterfall.cpp: setting -> compute after a completed run -> copy, invalidated with the analysis maps.
#include "pv_solver.h"

#include <algorithm>
#include <cstring>
#include <unordered_map>

#include "pv_arrays.h"
#include "pv_launch.h"

namespace pva {

namespace {
constexpr unsigned kArrayTimeKinds = (1u << kQrecRoomMetrics) | (1u << kQrecDecay) | (1u << kQrecEchoCriterion);
constexpr unsigned kArrayVelocityKinds = (1u << kQrecLateral) | (1u << kQrecEchogram) | (1u << kQrecLobes);
}  // namespace

void Solver::freeArrays() {
    for (void** p : {&arTaps_, (void**)&arTapOff_, (void**)&arSrc_, &arRows_, (void**)&arMix_, (void**)&arOnsets_, (void**)&arRec_})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    arRecCap_ = 0;
    arCount_.clear();
    arMembers_.clear();
    arCells_.clear();
    arTapOffHost_.clear();
    arTapRow_.clear();
    arTapDelay_.clear();
    arTapW_.clear();
    arP_ = 0;
    arValid_ = false;
    arOnsetsHost_.clear();
    arRecHost_.clear();
}

bool Solver::setArrays(const int* count, int nArrays, const float* members5, int interp) {
    // every refusal first: a refused call leaves the setting, the tables and what was computed
    if (isSlab()) return fail("arrays: not available on a slab");
    if (opt_.skipAnalysis) return fail("arrays: the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    std::vector<long long> cells;
    std::vector<ArrayTap> taps;
    std::vector<int> tapOff;
    if (nArrays != 0) {
        if (const char* e = arraysCountError(count, nArrays, members5)) return fail(e);
        if (interp != kArrayNearest && interp != kArrayLagrange3) return fail("arrays: interp is PVA_ARRAY_NEAREST or PVA_ARRAY_LAGRANGE3");
        tapOff.push_back(0);
        for (int a = 0, m = 0; a < nArrays; ++a) {
            for (int j = 0; j < count[a]; ++j, ++m) {
                const float* mb = members5 + (size_t)kArrayMemberFloats * m;
                const std::string who = "array " + std::to_string(a) + ", member " + std::to_string(j);
                int cx, cy;  // (as setOutputQueries maps its positions)
                if (!(mb[0] - mb[0] == 0.f) || !(mb[2] - mb[2] == 0.f) || !resultCell(g_, mb[0], mb[2], &cx, &cy))
                    return fail("arrays: a member off the map (" + who + ")");
                int d4[kArrayMaxTaps];
                float w4[kArrayMaxTaps];
                const char* why = nullptr;
                const int n = arrayTaps((int)g_.fs, T_, mb[3], mb[4], interp, d4, w4, &why);
                if (n < 0) return fail(std::string(why) + " (" + who + ")");
                cells.push_back((long long)cx * g_.gy + cy);
                for (int k = 0; k < n; ++k) taps.push_back(ArrayTap{m, d4[k], w4[k], 0});
            }
            tapOff.push_back((int)taps.size());
        }
    }
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (nArrays == 0) {
        freeArrays();
        return true;
    }
    // the new tables beside the old ones, which go only once everything has worked
    const int P = (nArrays + 63) / 64 * 64;
    ArrayTap* nTaps = nullptr;
    int* nOff = nullptr;
    long long* nSrc = nullptr;
    ArrayRow* nRows = nullptr;
    float *nMix = nullptr, *nOn = nullptr;
    const bool ok = dalloc(&nTaps, taps.size(), false) && dalloc(&nOff, tapOff.size(), false) && dalloc(&nSrc, cells.size(), false) &&
                    dalloc(&nRows, cells.size(), false) && dalloc(&nMix, (size_t)T_ * P, false) && dalloc(&nOn, (size_t)P, false) &&
                    hipOk(hipMemcpyAsync(nTaps, taps.data(), taps.size() * sizeof(ArrayTap), hipMemcpyHostToDevice, stream_), "arrays table upload") &&
                    hipOk(hipMemcpyAsync(nOff, tapOff.data(), tapOff.size() * sizeof(int), hipMemcpyHostToDevice, stream_), "arrays table upload") &&
                    hipOk(hipStreamSynchronize(stream_), "arrays table sync");
    if (!ok) {  // (the setting of before stays)
        for (void* p : {(void*)nTaps, (void*)nOff, (void*)nSrc, (void*)nRows, (void*)nMix, (void*)nOn})
            if (p) hipFree(p);
        return false;
    }
    const unsigned kinds[kRecordFamilies] = {arKinds_[kRecTime], arKinds_[kRecSpectral]};
    freeArrays();
    arTaps_ = nTaps;
    arTapOff_ = nOff;
    arSrc_ = nSrc;
    arRows_ = nRows;
    arMix_ = nMix;
    arOnsets_ = nOn;
    arP_ = P;
    arInterp_ = interp;
    arCount_.assign(count, count + nArrays);
    arMembers_.assign(members5, members5 + (size_t)kArrayMemberFloats * cells.size());
    arCells_ = cells;
    arTapOffHost_ = tapOff;
    for (const ArrayTap& t : taps) {
        arTapRow_.push_back(t.row);
        arTapDelay_.push_back(t.delay);
        arTapW_.push_back(t.w);
    }
    arKinds_[kRecTime] = kinds[kRecTime];  // (the selection is no part of the setting)
    arKinds_[kRecSpectral] = kinds[kRecSpectral];
    return true;
}

int Solver::arrays(int* count, int cap, int* interp) const {
    const int n = (int)arCount_.size();
    for (int a = 0; a < n && a < cap && count; ++a) count[a] = arCount_[(size_t)a];
    if (interp && n) *interp = arInterp_;
    return n;
}

int Solver::arrayTapsOf(int array, int* memberIndex, int* delaySteps, float* weight, int cap) {
    if (array < 0 || array >= (int)arCount_.size()) {
        fail("arrays: no such array");
        return -1;
    }
    int row0 = 0;
    for (int a = 0; a < array; ++a) row0 += arCount_[(size_t)a];
    const int k0 = arTapOffHost_[(size_t)array], n = arTapOffHost_[(size_t)array + 1] - k0;
    for (int k = 0; k < n && k < cap; ++k) {
        if (memberIndex) memberIndex[k] = arTapRow_[(size_t)(k0 + k)] - row0;
        if (delaySteps) delaySteps[k] = arTapDelay_[(size_t)(k0 + k)];
        if (weight) weight[k] = arTapW_[(size_t)(k0 + k)];
    }
    return n;
}

// what the settings hold against computing `kinds` for a mix, in the order it is said; empty: nothing
std::string Solver::arrayKindsRefusal(unsigned timeKinds, unsigned spectralKinds) const {
    const std::string pre = "arrays: ";
    if (timeKinds & kArrayVelocityKinds)
        return pre + "the velocity kinds (lateral, echogram, lobes) are not available: a mix has no cell and no face coefficients";
    if (timeKinds & ~kArrayTimeKinds) return pre + "unknown kind bit (PVA_QREC_*)";
    if (spectralKinds & ~kQuerySpectralMask) return pre + "unknown kind bit (PVA_QSPEC_*)";
    const unsigned kinds[kRecordFamilies] = {timeKinds, spectralKinds};
    for (int f = 0; f < kRecordFamilies; ++f)
        if (const char* why = recordKindsRefusal((RecordFamily)f, kinds[f]))  // (said with the family's own prefix)
            return pre + (why + std::char_traits<char>::length(recs_[f].prefix));
    return std::string();
}

bool Solver::setArrayRecords(unsigned timeKinds, unsigned spectralKinds) {
    if (isSlab()) return fail("arrays: not available on a slab");
    if (opt_.skipAnalysis) return fail("arrays: the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    const std::string why = arrayKindsRefusal(timeKinds, spectralKinds);
    if (!why.empty()) return fail(why);
    const auto inUse = queue_.lockUse();
    if (timeKinds != arKinds_[kRecTime] || spectralKinds != arKinds_[kRecSpectral]) arValid_ = false;
    arKinds_[kRecTime] = timeKinds;
    arKinds_[kRecSpectral] = spectralKinds;
    return true;
}

void Solver::arrayRecordKinds(unsigned* timeKinds, unsigned* spectralKinds) const {
    if (timeKinds) *timeKinds = arKinds_[kRecTime];
    if (spectralKinds) *spectralKinds = arKinds_[kRecSpectral];
}

int Solver::arrayRecordFloats(int family, unsigned kind) {
    if (family != kRecTime && family != kRecSpectral) {
        fail("arrays: family 0 (PVA_QREC_*) or 1 (PVA_QSPEC_*)");
        return -1;
    }
    const int k = oneKindBit(kind, recs_[family].nKinds);
    if (k < 0 || (family == kRecTime && !(kind & kArrayTimeKinds))) {
        fail(std::string("arrays: exactly one kind of the family (") + recs_[family].bits + "; no velocity kind)");
        return -1;
    }
    const int n = recordFloatsOf((RecordFamily)family, k);
    if (n < 0) fail(k == kQspecSpectrum ? "arrays: no bins set (PvAmdSetSpectrumBins)" : "arrays: no bands set (PvAmdSetBands)");
    return n;
}

bool Solver::computeArrays(float* ms) {
    // every refusal first: a refused call changes nothing, what an earlier call left included
    if (isSlab()) return fail("arrays: not available on a slab");
    if (opt_.skipAnalysis) return fail("arrays: the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    if (arCount_.empty()) return fail("arrays: no setting (PvAmdSetArrays)");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight; one that ends in error leaves its message)
    if (lastRun_ == LastRun::None || !dynValid_ || (opt_.streaming && !streamedOnce_)) return fail("arrays: no completed run");
    if (lastRun_ != LastRun::Ok) return fail("arrays: the last run ended in error");
    const std::string why = arrayKindsRefusal(arKinds_[kRecTime], arKinds_[kRecSpectral]);  // (the bands or bins may have gone since)
    if (!why.empty()) return fail(why);
    const int nArrays = (int)arCount_.size(), nRows = (int)arCells_.size();
    std::vector<long long> src(arCells_);
    if (opt_.streaming) {  // a member reads the trace of the kept registered emitter of its cell
        std::unordered_map<long long, int> emitterOf;
        for (int i = numEmitters_ - 1; i >= 0; --i) emitterOf[emRecCells_[i]] = i;
        for (int a = 0, m = 0; a < nArrays; ++a)
            for (int j = 0; j < arCount_[(size_t)a]; ++j, ++m) {
                const auto it = emitterOf.find(arCells_[(size_t)m]);
                if (it == emitterOf.end())
                    return fail("arrays: array " + std::to_string(a) + ", member " + std::to_string(j) +
                                ": its cell is not the cell of a registered emitter (PvAmdSetEmitters)");
                src[(size_t)m] = it->second;
            }
    }
    const unsigned tk = arKinds_[kRecTime], sk = arKinds_[kRecSpectral];
    if ((sk & (1u << kQspecSpectrum)) && (!specTab_ || !specPow_ || (int)specPasses_.size() > kQspecMaxSlices))
        return fail("arrays: the spectrum's tables are not on the device (PvAmdSetSpectrumBins)");
    // the layout of the record block: the time family's kinds, then the spectral family's, each nArrays x floats
    int floats[kRecordFamilies][kQueryRecordKinds] = {};
    size_t offset[kRecordFamilies][kQueryRecordKinds] = {};
    size_t need = 0;
    for (int f = 0; f < kRecordFamilies; ++f)
        for (int k = 0; k < recs_[f].nKinds; ++k) {
            offset[f][k] = need;
            floats[f][k] = (arKinds_[f] >> k) & 1u ? recordFloatsOf((RecordFamily)f, k) : 0;
            need += (size_t)floats[f][k] * nArrays;
        }
    const size_t timeFloats = offset[kRecSpectral][0];

    arValid_ = false;
    if (need > arRecCap_) {
        if (arRec_) hipFree(arRec_);
        arRec_ = nullptr;
        arRecCap_ = 0;
        if (!dalloc(&arRec_, need, false)) return false;
        arRecCap_ = need;
    }
    if ((sk & (1u << kQspecModulation)) && !ensureModTable()) return false;
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    if (!hipOk(hipMemcpyAsync(arSrc_, src.data(), src.size() * sizeof(long long), hipMemcpyHostToDevice, stream_), "arrays members upload") ||
        !hipOk(hipStreamSynchronize(stream_), "arrays members sync"))  // (`src` is pageable: the copy is done before the timed interval)
        return false;

    const AnalyzeArgs a = analyzeArgs(lastLx_, lastLz_);
    ArrayMixArgs mx{};
    mx.samples = opt_.streaming ? emTrace_ : hist_;
    mx.rows = static_cast<const ArrayRow*>(arRows_);
    mx.taps = static_cast<const ArrayTap*>(arTaps_);
    mx.tapOff = arTapOff_;
    mx.mix = arMix_;
    mx.nArrays = nArrays;
    mx.P = arP_;
    mx.T = T_;
    // the record launches' arguments: the mix planes as the history, the responses' onsets as the onset map
    AnalyzeArgs ra = a;
    ra.hist = arMix_;
    ra.histPlane = arP_;
    ra.delay = arOnsets_;
    ra.recTrace = nullptr;
    ra.ring = 0;
    const int fs = (int)g_.fs;

    hipEventRecord(mapEv_[0], stream_);
    launchArrayRows(a, arSrc_, nRows, opt_.streaming, static_cast<ArrayRow*>(arRows_), stream_);
    launchArrayMix(mx, stream_);
    launchArrayOnsets(arMix_, T_, arP_, nArrays, arOnsets_, stream_);
    if (tk) {
        QueryRecordArgs q{};
        q.out = arRec_;
        q.nq = nArrays;
        q.kinds = tk;
        q.mix = 1;
        for (int k = 0; k < kQueryRecordKinds; ++k) {
            q.offset[k] = (int)offset[kRecTime][k];
            q.floats[k] = floats[kRecTime][k];
        }
        q.n50 = roomMetricsN50(fs);
        q.n80 = roomMetricsN80(fs);
        q.tailN = decayTailN(fs);
        q.nDs = echoSpeechLag(fs);
        q.nDm = echoMusicLag(fs);
        q.nLs = echoSpeechLimit(fs);
        q.nLm = echoMusicLimit(fs);
        launchQueryRecords(ra, q, stream_);
    }
    if (sk) {
        QuerySpectralArgs q{};
        q.out = arRec_ + timeFloats;
        q.nq = nArrays;
        q.mix = 1;
        const int n = (int)bandHz_.size(), B = bandMetricsBlock();
        q.nBands = n;
        for (int j = 0; j < n; ++j)
            for (int k = 0; k < kBandCoefs; ++k) q.coefs[j][k] = bandCoefs_[(size_t)j * kBandCoefs + k];
        q.items[kQspecBandMetrics] = (sk & (1u << kQspecBandMetrics)) ? (n + B - 1) / B : 0;
        q.items[kQspecModulation] = (sk & (1u << kQspecModulation)) ? n : 0;
        q.items[kQspecSpectrum] = (sk & (1u << kQspecSpectrum)) ? (int)specPasses_.size() : 0;
        for (int k = 0; k < kQuerySpectralKinds; ++k) {
            q.offset[k] = (int)(offset[kRecSpectral][k] - timeFloats);
            q.floats[k] = floats[kRecSpectral][k];
        }
        q.tailN = decayTailN(fs);
        q.n50 = roomMetricsN50(fs);
        q.n80 = roomMetricsN80(fs);
        q.modTab = modTab_ ? modTab_ + (size_t)kModTablePad * kModRowStride : nullptr;
        q.specTab = specTab_;
        q.specPow = specPow_;
        for (int i = 0; i < q.items[kQspecSpectrum]; ++i) {
            const SpecPass& ps = specPasses_[(size_t)i];
            q.slice[i] = QuerySpectralSlice{ps.bin0, ps.bins, ps.block, (long long)ps.tabOff};
        }
        launchQuerySpectral(ra, q, stream_);
    }
    hipEventRecord(mapEv_[1], stream_);
    if (!hipOk(hipGetLastError(), "arrays launch") || !hipOk(hipStreamSynchronize(stream_), "arrays sync")) return false;
    if (ms && !hipOk(hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]), "arrays timing")) return false;
    // the onsets and the records to the host: what the read-backs hand out
    arOnsetsHost_.resize((size_t)nArrays);
    arRecHost_.resize(need);
    if (!hipOk(hipMemcpyAsync(arOnsetsHost_.data(), arOnsets_, (size_t)nArrays * 4, hipMemcpyDeviceToHost, stream_), "arrays onsets copy") ||
        (need && !hipOk(hipMemcpyAsync(arRecHost_.data(), arRec_, need * 4, hipMemcpyDeviceToHost, stream_), "arrays records copy")) ||
        !hipOk(hipStreamSynchronize(stream_), "arrays copy sync"))
        return false;
    for (int f = 0; f < kRecordFamilies; ++f) {
        arRunKinds_[f] = arKinds_[f];
        for (int k = 0; k < kQueryRecordKinds; ++k) {
            arRunFloats_[f][k] = floats[f][k];
            arRunOffset_[f][k] = offset[f][k];
        }
    }
    arValid_ = true;
    ++arStamp_;
    return true;
}

namespace {
const char kArraysStale[] =
    "arrays: not computed for the last run, the current geometry, the current setting, kinds and emitters (PvAmdComputeArrays)";
}

bool Solver::copyArrayResponse(int array, float* outT) {
    if (arCount_.empty()) return fail("arrays: no setting (PvAmdSetArrays)");
    if (array < 0 || array >= (int)arCount_.size()) return fail("arrays: no such array");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;  // (a run in flight: its responses are not the ones asked for)
    if (!arValid_) return fail(kArraysStale);
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    // column `array` of the planes [T][arP_]
    return hipOk(hipMemcpy2DAsync(outT, 4, arMix_ + array, (size_t)arP_ * 4, 4, (size_t)T_, hipMemcpyDeviceToHost, stream_), "arrays response copy") &&
           hipOk(hipStreamSynchronize(stream_), "arrays sync");
}

bool Solver::arrayOnsets(float* out, int nArrays) {
    if (arCount_.empty()) return fail("arrays: no setting (PvAmdSetArrays)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;
    if (!arValid_) return fail(kArraysStale);
    if (nArrays != (int)arCount_.size()) return fail("arrays: the count differs from the arrays set");
    std::memcpy(out, arOnsetsHost_.data(), (size_t)nArrays * 4);
    return true;
}

bool Solver::arrayRecords(int family, unsigned kind, float* out, int nArrays) {
    if (arCount_.empty()) return fail("arrays: no setting (PvAmdSetArrays)");
    if (family != kRecTime && family != kRecSpectral) return fail("arrays: family 0 (PVA_QREC_*) or 1 (PVA_QSPEC_*)");
    const int k = oneKindBit(kind, recs_[family].nKinds);
    if (k < 0) return fail(std::string("arrays: exactly one kind (") + recs_[family].bits + ")");
    if (!(arKinds_[family] & kind)) return fail("arrays: the kind is not selected (PvAmdSetArrayRecords)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;
    if (nArrays != (int)arCount_.size()) return fail("arrays: the count differs from the arrays set");
    if (!arValid_ || arRunKinds_[kRecTime] != arKinds_[kRecTime] || arRunKinds_[kRecSpectral] != arKinds_[kRecSpectral] ||
        arRunFloats_[family][k] != recordFloatsOf((RecordFamily)family, k))
        return fail(kArraysStale);
    std::memcpy(out, arRecHost_.data() + arRunOffset_[family][k], (size_t)nArrays * arRunFloats_[family][k] * 4);
    return true;
}

}  // namespace pva
