// pv_solver_aural.cpp -- the auralisation of a Solver (pv_solver.h; the definition: pv_aural.h; the passes: pv_aural.hip): the
// setting with its resampling tables, the receivers of a call -- positions mapped as the output queries are, the registered emitters
// of sparse-emitter mode with their traces, or the array responses computeArrays left --, the responses, the convolution with the
// caller's signals and the mix, the stamps and the refusals.  After the pattern of pv_solver_waterfall.cpp: setting -> compute after
// a completed run -> copy, invalidated with the analysis maps.  It needs no onset map.
#include "pv_solver.h"

#include <algorithm>
#include <cstring>

#include "pv_aural.h"
#include "pv_launch.h"

namespace pva {

void Solver::freeAuralisation() {
    for (void** p : {(void**)&auFirstDev_, (void**)&auWT_, (void**)&auCells_, &auRows_, (void**)&auGather_, (void**)&auResp_, (void**)&auSig_,
                     (void**)&auRoute_, (void**)&auGain_, (void**)&auOut_, (void**)&auMix_})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    auGatherCap_ = auRespCap_ = auSigCap_ = auOutCap_ = auMixCap_ = 0;
    auRate_ = auZ_ = auL_ = auK_ = 0;
    auBeta_ = 0.f;
    auFirst_.clear();
    auFirst_.shrink_to_fit();
    auW_.clear();
    auW_.shrink_to_fit();
    auCount_ = auM_ = 0;
    auRespValid_ = auOutValid_ = false;
}

bool Solver::setAuralisation(int rate, int zeroCrossings, float beta) {
    if (isSlab()) return fail("aural: not available on a slab");
    int L = 0, K = 0;
    if (rate != 0)
        if (const char* e = auralShape(g_.fs, T_, rate, zeroCrossings, beta, &L, &K)) return fail(e);
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (rate == 0) {
        freeAuralisation();
        return true;
    }
    // the new tables beside the old ones, which go only once everything has worked
    std::vector<int> first((size_t)L);
    std::vector<float> w((size_t)L * K), wT((size_t)L * K);
    auralTaps(g_.fs, rate, zeroCrossings, beta, L, K, first.data(), w.data());
    for (int n = 0; n < L; ++n)
        for (int j = 0; j < K; ++j) wT[(size_t)j * L + n] = w[(size_t)n * K + j];
    int* nFirst = nullptr;
    float* nW = nullptr;
    long long* cells = auCells_;
    ArrayRow* rows = static_cast<ArrayRow*>(auRows_);
    const bool ok = dalloc(&nFirst, (size_t)L, false) && dalloc(&nW, (size_t)L * K, false) &&
                    (cells || dalloc(&cells, (size_t)kAuralMaxReceivers, false)) && (rows || dalloc(&rows, (size_t)kAuralMaxReceivers, false)) &&
                    hipOk(hipMemcpyAsync(nFirst, first.data(), (size_t)L * sizeof(int), hipMemcpyHostToDevice, stream_), "aural table upload") &&
                    hipOk(hipMemcpyAsync(nW, wT.data(), (size_t)L * K * 4, hipMemcpyHostToDevice, stream_), "aural table upload") &&
                    hipOk(hipStreamSynchronize(stream_), "aural table sync");
    auCells_ = cells;
    auRows_ = rows;
    if (!ok) {  // (the setting of before stays)
        if (nFirst) hipFree(nFirst);
        if (nW) hipFree(nW);
        return false;
    }
    // (the responses and outputs are the old setting's: their storage goes with it)
    for (void** p : {(void**)&auFirstDev_, (void**)&auWT_, (void**)&auResp_, (void**)&auOut_, (void**)&auMix_})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    auRespCap_ = auOutCap_ = auMixCap_ = 0;
    auFirstDev_ = nFirst;
    auWT_ = nW;
    auFirst_.swap(first);
    auW_.swap(w);
    auRate_ = rate;
    auZ_ = zeroCrossings;
    auBeta_ = beta;
    auL_ = L;
    auK_ = K;
    auCount_ = auM_ = 0;
    auRespValid_ = auOutValid_ = false;
    return true;
}

bool Solver::auralisation(int* rate, int* zeroCrossings, float* beta, int* L, int* K) const {
    if (!auRate_) return false;
    if (rate) *rate = auRate_;
    if (zeroCrossings) *zeroCrossings = auZ_;
    if (beta) *beta = auBeta_;
    if (L) *L = auL_;
    if (K) *K = auK_;
    return true;
}

int Solver::auralTapsOf(int* first, float* w, int capN) {
    if (!auRate_) {
        fail("aural: no setting (PvAmdSetAuralisation)");
        return -1;
    }
    const int n = std::max(0, std::min(capN, auL_));
    if (first) std::memcpy(first, auFirst_.data(), (size_t)n * sizeof(int));
    if (w) std::memcpy(w, auW_.data(), (size_t)n * auK_ * 4);
    return auL_;
}

bool Solver::computeAuralResponses(int source, const float* xyz, int nPos, float* ms) {
    // every refusal first: a refused call changes nothing, the responses of an earlier call included
    if (isSlab()) return fail("aural: not available on a slab");
    if (!auRate_) return fail("aural: no setting (PvAmdSetAuralisation)");
    if (source != kAuralReceivers && source != kAuralArrays) return fail("aural: source is PVA_AURAL_RECEIVERS or PVA_AURAL_ARRAYS");
    const bool positions = source == kAuralReceivers && !opt_.streaming;
    if (!positions) {
        if (xyz || nPos != 0)
            return fail(source == kAuralArrays
                            ? "aural: the array source takes no positions (NULL, 0): the receivers are the arrays (PvAmdSetArrays)"
                            : "aural: a sparse-emitter solver takes no positions (NULL, 0): the receivers are the registered emitters (PvAmdSetEmitters)");
    } else {
        if (nPos > 0 && !xyz) return fail("aural: no positions");
        if (nPos < 1 || nPos > kAuralMaxReceivers) return fail("aural: 1 .. 256 positions (PVA_AURAL_MAX_RECEIVERS)");
    }
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight; one that ends in error leaves its message)
    int count = nPos;
    if (source == kAuralArrays) {
        count = (int)arCount_.size();
        if (count < 1) return fail("aural: no arrays set (PvAmdSetArrays)");
        if (!arValid_) return fail("aural: the array responses are not computed for the last run and the current settings (PvAmdComputeArrays)");
    } else if (opt_.streaming) {
        count = numEmitters_;
        if (count < 1) return fail("aural: no emitters registered (PvAmdSetEmitters)");
        if (count > kAuralMaxReceivers) return fail("aural: at most 256 registered emitters (PVA_AURAL_MAX_RECEIVERS)");
    }
    if (lastRun_ == LastRun::None || !dynValid_ || (opt_.streaming && !streamedOnce_)) return fail("aural: no completed run");
    if (lastRun_ != LastRun::Ok) return fail("aural: the last run ended in error");
    std::vector<long long> cells((size_t)count);
    std::vector<ArrayRow> rows;
    if (source == kAuralArrays) {  // response a is column a of the mix planes [T][arP_]
        for (int a = 0; a < count; ++a) rows.push_back(ArrayRow{a, arP_, 0, 0});
    } else {
        for (int i = 0; i < count; ++i) {
            if (opt_.streaming) {
                cells[(size_t)i] = i;  // (launchArrayRows with trace: the emitter whose trace is read)
                continue;
            }
            int cx, cy;  // (as setOutputQueries maps its positions)
            const float x = xyz[3 * i], z = xyz[3 * i + 2];
            if (!(x - x == 0.f) || !(z - z == 0.f) || !resultCell(g_, x, z, &cx, &cy))
                return fail("aural: a position off the map (position " + std::to_string(i) + ")");
            cells[(size_t)i] = (long long)cx * g_.gy + cy;
        }
    }

    const size_t needGather = (size_t)count * T_, needResp = (size_t)count * auL_;
    auRespValid_ = auOutValid_ = false;
    if (needGather > auGatherCap_) {
        if (auGather_) hipFree(auGather_);
        auGather_ = nullptr;
        auGatherCap_ = 0;
        if (!dalloc(&auGather_, needGather, false)) return false;
        auGatherCap_ = needGather;
    }
    if (needResp > auRespCap_) {
        if (auResp_) hipFree(auResp_);
        auResp_ = nullptr;
        auRespCap_ = 0;
        if (!dalloc(&auResp_, needResp, false)) return false;
        auRespCap_ = needResp;
    }
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    // (`cells` and `rows` are pageable: the copies are done before the timed interval)
    if (source == kAuralArrays) {
        if (!hipOk(hipMemcpyAsync(auRows_, rows.data(), rows.size() * sizeof(ArrayRow), hipMemcpyHostToDevice, stream_), "aural rows upload")) return false;
    } else if (!hipOk(hipMemcpyAsync(auCells_, cells.data(), cells.size() * sizeof(long long), hipMemcpyHostToDevice, stream_), "aural cells upload")) {
        return false;
    }
    if (!hipOk(hipStreamSynchronize(stream_), "aural cells sync")) return false;
    const AnalyzeArgs a = analyzeArgs(lastLx_, lastLz_);
    const float* samples = source == kAuralArrays ? arMix_ : opt_.streaming ? emTrace_ : hist_;
    hipEventRecord(mapEv_[0], stream_);
    if (source != kAuralArrays) launchArrayRows(a, auCells_, count, opt_.streaming, static_cast<ArrayRow*>(auRows_), stream_);
    launchAuralGather(samples, static_cast<const ArrayRow*>(auRows_), count, T_, auGather_, stream_);
    launchAuralResample(auGather_, count, T_, auFirstDev_, auWT_, auL_, auK_, auResp_, stream_);
    hipEventRecord(mapEv_[1], stream_);
    if (!hipOk(hipGetLastError(), "aural launch") || !hipOk(hipStreamSynchronize(stream_), "aural sync")) return false;
    if (ms && !hipOk(hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]), "aural timing")) return false;
    auCount_ = count;
    auSource_ = source;
    auArStamp_ = arStamp_;
    auRespValid_ = true;
    return true;
}

namespace {
const char kAuralStale[] =
    "aural: no responses for the last run, the current geometry, the current setting, emitters and array responses (PvAmdComputeAuralResponses)";
}

bool Solver::copyAuralResponse(int r, float* outL) {
    if (!auRate_) return fail("aural: no setting (PvAmdSetAuralisation)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;  // (a run in flight: its responses are not the ones asked for)
    if (!auralResponsesValid()) return fail(kAuralStale);
    if (r < 0 || r >= auCount_) return fail("aural: no such receiver");
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    return hipOk(hipMemcpyAsync(outL, auResp_ + (size_t)r * auL_, (size_t)auL_ * 4, hipMemcpyDeviceToHost, stream_), "aural response copy") &&
           hipOk(hipStreamSynchronize(stream_), "aural sync");
}

bool Solver::setAuralForm(int form) {
    if (form != kAuralTiled && form != kAuralPlain) return fail("aural: form is PVA_AURAL_TILED or PVA_AURAL_PLAIN");
    const auto inUse = queue_.lockUse();
    auForm_ = form;
    return true;
}

bool Solver::auralise(const float* signals, int nSignals, int N, const int* route, const float* gain, float* ms) {
    if (isSlab()) return fail("aural: not available on a slab");
    if (!auRate_) return fail("aural: no setting (PvAmdSetAuralisation)");
    if (!signals || !route || !gain) return fail("aural: null signal, route or gain table");
    if (nSignals < 1 || nSignals > kAuralMaxSignals) return fail("aural: 1 .. 64 signals (PVA_AURAL_MAX_SIGNALS)");
    if (N < 1 || N > kAuralMaxSignalSamples) return fail("aural: signals of 1 .. 2^20 samples (PVA_AURAL_MAX_SAMPLES)");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;
    if (!auralResponsesValid()) return fail(kAuralStale);
    const int R = auCount_, M = N + auL_ - 1;
    if ((long long)R * M > kAuralMaxOutputFloats) return fail("aural: more than 2^26 output samples (receivers x (N + L - 1))");
    for (int r = 0; r < R; ++r) {
        if (route[r] < -1 || route[r] >= nSignals) return fail("aural: a route outside -1 .. nSignals - 1 (receiver " + std::to_string(r) + ")");
        if (!(gain[r] - gain[r] == 0.f)) return fail("aural: a gain that is not finite (receiver " + std::to_string(r) + ")");
    }
    auOutValid_ = false;
    const size_t needSig = (size_t)nSignals * N, needOut = (size_t)R * M;
    if (needSig > auSigCap_) {
        if (auSig_) hipFree(auSig_);
        auSig_ = nullptr;
        auSigCap_ = 0;
        if (!dalloc(&auSig_, needSig, false)) return false;
        auSigCap_ = needSig;
    }
    if (needOut > auOutCap_) {
        if (auOut_) hipFree(auOut_);
        auOut_ = nullptr;
        auOutCap_ = 0;
        if (!dalloc(&auOut_, needOut, false)) return false;
        auOutCap_ = needOut;
    }
    if ((size_t)M > auMixCap_) {
        if (auMix_) hipFree(auMix_);
        auMix_ = nullptr;
        auMixCap_ = 0;
        if (!dalloc(&auMix_, (size_t)M, false)) return false;
        auMixCap_ = (size_t)M;
    }
    if (!auRoute_ && !dalloc(&auRoute_, (size_t)kAuralMaxReceivers, false)) return false;
    if (!auGain_ && !dalloc(&auGain_, (size_t)kAuralMaxReceivers, false)) return false;
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    // (the caller's tables are pageable: the copies are done before the timed interval)
    if (!hipOk(hipMemcpyAsync(auSig_, signals, needSig * 4, hipMemcpyHostToDevice, stream_), "aural signals upload") ||
        !hipOk(hipMemcpyAsync(auRoute_, route, (size_t)R * sizeof(int), hipMemcpyHostToDevice, stream_), "aural route upload") ||
        !hipOk(hipMemcpyAsync(auGain_, gain, (size_t)R * 4, hipMemcpyHostToDevice, stream_), "aural gain upload") ||
        !hipOk(hipStreamSynchronize(stream_), "aural upload sync"))
        return false;
    AuralConvolveArgs c{};
    c.resp = auResp_;
    c.signals = auSig_;
    c.route = auRoute_;
    c.out = auOut_;
    c.R = R;
    c.L = auL_;
    c.N = N;
    hipEventRecord(mapEv_[0], stream_);
    launchAuralConvolve(c, auForm_, stream_);
    launchAuralMix(auOut_, auRoute_, auGain_, R, M, auMix_, stream_);
    hipEventRecord(mapEv_[1], stream_);
    if (!hipOk(hipGetLastError(), "aural launch") || !hipOk(hipStreamSynchronize(stream_), "aural sync")) return false;
    if (ms && !hipOk(hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]), "aural timing")) return false;
    auM_ = M;
    auOutValid_ = true;
    return true;
}

namespace {
const char kAuralNoOutput[] = "aural: no outputs for the current responses (PvAmdAuralise)";
}

bool Solver::copyAuralOutput(int r, float* outM) {
    if (!auRate_) return fail("aural: no setting (PvAmdSetAuralisation)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;
    if (!auralResponsesValid() || !auOutValid_) return fail(kAuralNoOutput);
    if (r < 0 || r >= auCount_) return fail("aural: no such receiver");
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    return hipOk(hipMemcpyAsync(outM, auOut_ + (size_t)r * auM_, (size_t)auM_ * 4, hipMemcpyDeviceToHost, stream_), "aural output copy") &&
           hipOk(hipStreamSynchronize(stream_), "aural sync");
}

bool Solver::copyAuralMix(float* outM) {
    if (!auRate_) return fail("aural: no setting (PvAmdSetAuralisation)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;
    if (!auralResponsesValid() || !auOutValid_) return fail(kAuralNoOutput);
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    return hipOk(hipMemcpyAsync(outM, auMix_, (size_t)auM_ * 4, hipMemcpyDeviceToHost, stream_), "aural mix copy") &&
           hipOk(hipStreamSynchronize(stream_), "aural sync");
}

}  // namespace pva
