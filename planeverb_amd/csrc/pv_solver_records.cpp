// pv_solver_records.cpp -- what a run leaves in pinned host memory for the registered queries of a Solver (pv_solver.h): the eight
// outputs of the output queries, and the in-run analysis records in their two families (pv_query_records.hip, six time-domain
// kinds; pv_query_spectral.hip, three frequency-resolved ones).  A family's selector, pinned block and stamp are written once, for
// a RecordSet; what is a family's own: its record sizes, the preconditions of its kinds, and its launch with the arguments.  In
// sparse-emitter mode the same path serves the registered emitters (PvAmdSetEmitterRecords): the cell table is theirs, the history
// planes are their record traces.
#include "pv_solver.h"

#include <algorithm>

#include "pv_launch.h"
#include "pv_bands.h"
#include "pv_modulation.h"
#include "pv_decay.h"
#include "pv_echo.h"
#include "pv_echogram.h"
#include "pv_lateral.h"
#include "pv_lobes.h"
#include "pv_metrics.h"
#include "pv_spectrum.h"

namespace pva {

// ----------------------------------------------------------------------------------------------------------------
// output queries, record queries, and the tail of a run
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setOutputQueries(const float* xyz, int n) {
    if (n < 0 || n > kMaxQueries) return fail("at most 64 output queries");
    if (pendingTimings_ && !sync()) return false;  // the gather of a run in flight still reads the cell table
    for (int i = 0; i < n; ++i) {
        int cx, cy;
        qCellsHost_[i] = resultCell(g_, xyz[3 * i], xyz[3 * i + 2], &cx, &cy) ? (long long)cx * g_.gy + cy : -1;
    }
    numQueries_ = n;
    if (numRecQueries_ == 0)  // (the records in the pinned blocks belong to the queries of before)
        for (int f = 0; f < kRecordFamilies; ++f) invalidateRecords((RecordFamily)f);
    return true;
}

bool Solver::setRecordQueries(const float* xyz, int n) {
    if (n < 0 || n > kMaxRecordQueries) return fail("query records: at most 1024 record queries");
    if (n > 0 && !xyz) return fail("query records: no positions");
    if (n > 0 && isSlab()) return fail("query records: not available on a slab");
    if (n > 0 && opt_.streaming) return fail("query records: the full pressure history is not kept in streaming-analysis mode");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // the launch of a run in flight still reads the cell table
    if (n > rqCap_) {
        long long* t = nullptr;
        if (!hipOk(hipHostMalloc((void**)&t, (size_t)n * sizeof(long long)), "hipHostMalloc")) return false;
        if (rqCellsHost_) hipHostFree(rqCellsHost_);
        rqCellsHost_ = t;
        rqCap_ = n;
    }
    for (int f = 0; f < kRecordFamilies; ++f)
        if (!growRecordBlock((RecordFamily)f, n)) return false;
    for (int i = 0; i < n; ++i) {
        int cx, cy;
        rqCellsHost_[i] = resultCell(g_, xyz[3 * i], xyz[3 * i + 2], &cx, &cy) ? (long long)cx * g_.gy + cy : -1;
    }
    numRecQueries_ = n;
    for (int f = 0; f < kRecordFamilies; ++f) invalidateRecords((RecordFamily)f);  // (the records belong to the table of before)
    return true;
}

// last kernel of a run: its status words into pinned memory (sync() then needs no copy and no second synchronisation)
void Solver::enqueueRunStatus() {
    launchRunStatus(errFlag_, activeCount_, plan_.oneXcd ? resFlags_ + runTiles_ + 1 : nullptr, statusHost_, stream_);
    statusQueued_ = true;
}

void Solver::enqueueQueries() {
    enqueueQueryRecords();
    enqueueQuerySpectralRecords();
    if (numQueries_ > 0 && !opt_.skipAnalysis)
        launchGatherQueries(res_, (long long)g_.gx * g_.gy, qCellsHost_, numQueries_, qOutHost_, farInfo(), stream_);
    enqueueTap();
}

void Solver::enqueueTap() {
    if (tap_ && !opt_.skipAnalysis) {
        const Block b = curWindow();
        tap_->afterRun(res_, delay_, (long long)g_.gx * g_.gy, g_.gy, b.r0, b.c0, b.nr, b.nc, stream_);
    }
}

// after sync(): the registered queries' outputs of the last run, straight from pinned memory
bool Solver::queriedOutputs(float* out8n, unsigned char* valid, int n) {
    if (n != numQueries_) return fail("queriedOutputs: count differs from the registered queries");
    if (pendingTimings_ && !sync()) return false;
    for (int i = 0; i < n; ++i) {
        valid[i] = qCellsHost_[i] >= 0;
        for (int k = 0; k < 8; ++k) out8n[8 * i + k] = qOutHost_[8 * i + k];
    }
    return true;
}

// ----------------------------------------------------------------------------------------------------------------
// in-run records: a family's own
// ----------------------------------------------------------------------------------------------------------------

// Floats per query of kind bit k, -1 where the kind's setting is missing: under the current settings, or under the largest ones,
// which is what the pinned block is sized for, so that a later change of slots, windows, bands or bins needs no allocation
int Solver::recordFloatsOf(RecordFamily f, int k, bool largest) const {
    if (f == kRecTime) {
        const int slots = largest ? kEchogramMaxSlots : echoSlots_;
        switch (k) {
            case kQrecRoomMetrics: return kRoomMetricFloats;
            case kQrecDecay: return kDecayFloats;
            case kQrecLateral: return kLateralFloats;
            case kQrecEchogram: return slots > 0 ? echogramFloats(slots) : -1;
            case kQrecEchoCriterion: return kEchoFloats;
            case kQrecLobes: return lobesFloats(largest ? kLobesMaxWindows : lobeEdgeCount_ + 1);
        }
        return -1;
    }
    const int n = largest ? kBandsMax : (int)bandHz_.size(), bins = largest ? kSpectrumMaxBins : (int)specHz_.size();
    switch (k) {
        case kQspecBandMetrics: return n > 0 ? kBandFloats * n : -1;
        case kQspecModulation: return n > 0 ? kModFloats * n : -1;
        case kQspecSpectrum: return bins > 0 ? kSpectrumFloats * bins : -1;
    }
    return -1;
}

namespace {
// the refusal where kind bit k's setting is missing
const char* noRecordSetting(int family, int k) {
    if (family == Solver::kRecTime) return "query records: echogram: no slots set (PvAmdSetEchogram)";
    return k == kQspecSpectrum ? "spectral records: no bins set (PvAmdSetSpectrumBins)" : "spectral records: no bands set (PvAmdSetBands)";
}
}  // namespace

// what the settings hold against selecting `kinds`, in the order it is said: the refusal, or nullptr
const char* Solver::recordKindsRefusal(RecordFamily f, unsigned kinds) const {
    if (f == kRecTime) {
        LobeEdges ed;
        if ((kinds & (1u << kQrecEchogram)) && !echoSlots_) return noRecordSetting(f, kQrecEchogram);
        if ((kinds & (1u << kQrecEchoCriterion)) && !echoFsOk((int)g_.fs))
            return "query records: echo: the sampling rate gives a speech lag below one step ((int)(0.009f * (float)fs) < 1)";
        if ((kinds & (1u << kQrecLobes)) && !lobesEdgeSteps(lobeEdges_, lobeEdgeCount_, (int)g_.fs, &ed))
            return "query records: lobes: the default windows (10 ms, 80 ms) need a sampling rate of 100 Hz or more (PvAmdSetLobeWindows)";
        return nullptr;
    }
    if ((kinds & kQspecBandKinds) && bandHz_.empty()) return noRecordSetting(f, kQspecBandMetrics);
    if ((kinds & (1u << kQspecSpectrum)) && specHz_.empty()) return noRecordSetting(f, kQspecSpectrum);
    return nullptr;
}

// The settings are those of this moment: PvAmdSetEchogram / PvAmdSetLobeWindows wait for a run in flight, and the stamp keeps the
// layout the run was enqueued with
void Solver::enqueueQueryRecords() {
    const RecordSet& r = recs_[kRecTime];
    if (!r.kinds || opt_.skipAnalysis) return;
    QueryRecordArgs q{};
    q.cells = recordCells();
    q.out = r.host;
    q.nq = recordQueryCount();
    q.kinds = r.kinds;
    bool on[kQueryRecordKinds];
    for (int k = 0; k < kQueryRecordKinds; ++k) on[k] = (r.kinds >> k) & 1u;
    stampRecords(kRecTime, q.nq, on, q.offset, q.floats);
    const int fs = (int)g_.fs;
    q.n50 = roomMetricsN50(fs);
    q.n80 = roomMetricsN80(fs);
    q.n5 = lateralN5(fs);
    q.latN80 = lateralN80(fs);
    q.tailN = decayTailN(fs);
    q.ns = echoSteps_;
    q.nSlots = echoSlots_;
    q.nDs = echoSpeechLag(fs);
    q.nDm = echoMusicLag(fs);
    q.nLs = echoSpeechLimit(fs);
    q.nLm = echoMusicLimit(fs);
    lobesEdgeSteps(lobeEdges_, lobeEdgeCount_, fs, &q.ed);  // (valid: checked where the kind was selected and where the windows are set)
    q.nW = lobeEdgeCount_ + 1;
    if (q.nq > 0) launchQueryRecords(recordArgs(), q, stream_);
}

// The settings are those of this moment: PvAmdSetBands, PvAmdSetModulationFrequencies and PvAmdSetSpectrumBins wait for a run in
// flight and leave the device tables valid, and the stamp keeps the layout the run was enqueued with.  A kind whose tables are
// missing (an upload that failed in a setter) is left out: its stamp then differs from the settings and its read-back is refused
void Solver::enqueueQuerySpectralRecords() {
    const RecordSet& r = recs_[kRecSpectral];
    if (!r.kinds || opt_.skipAnalysis) return;
    QuerySpectralArgs q{};
    q.cells = recordCells();
    q.out = r.host;
    q.nq = recordQueryCount();
    const int n = (int)bandHz_.size(), B = bandMetricsBlock();
    q.nBands = n;
    for (int j = 0; j < n; ++j)
        for (int k = 0; k < kBandCoefs; ++k) q.coefs[j][k] = bandCoefs_[(size_t)j * kBandCoefs + k];
    const bool on[kQuerySpectralKinds] = {(r.kinds & (1u << kQspecBandMetrics)) && n > 0,
                                          (r.kinds & (1u << kQspecModulation)) && n > 0 && modTab_ && modTabValid_,
                                          (r.kinds & (1u << kQspecSpectrum)) && !specPasses_.empty() && specTab_ && specPow_ &&
                                              (int)specPasses_.size() <= kQspecMaxSlices};
    q.items[kQspecBandMetrics] = on[kQspecBandMetrics] ? (n + B - 1) / B : 0;
    q.items[kQspecModulation] = on[kQspecModulation] ? n : 0;
    q.items[kQspecSpectrum] = on[kQspecSpectrum] ? (int)specPasses_.size() : 0;
    stampRecords(kRecSpectral, q.nq, on, q.offset, q.floats);
    const int fs = (int)g_.fs;
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
    if (q.nq > 0 && q.items[kQspecBandMetrics] + q.items[kQspecModulation] + q.items[kQspecSpectrum] > 0)
        launchQuerySpectral(recordArgs(), q, stream_);
}

// The record launches' arguments.  A sparse-emitter run's history is a ring: its record launches get the record traces as their
// history planes (a.recTrace set: the launchers take the trace lane, recordLaneOfTrace)
AnalyzeArgs Solver::recordArgs() const {
    AnalyzeArgs a = analyzeArgs(lastLx_, lastLz_);
    if (opt_.streaming) {
        a.hist = a.recTrace;
        a.histPlane = (long long)a.recCols * (a.recVel ? 3 : 1);
        a.ring = 0;
    }
    return a;
}

// ----------------------------------------------------------------------------------------------------------------
// emitter records: the two families with the registered emitters of sparse-emitter mode as the cell source
// ----------------------------------------------------------------------------------------------------------------

namespace {
const char kEmitterPre[] = "emitter records: ";
const char kEmitterMode[] = "the solver is not in sparse-emitter mode (PvAmdSetQueryRecords serves the output queries of a solver that keeps its history)";
const char kEmitterMax[] = "at most 1024 registered emitters while a kind is selected";
constexpr unsigned kVelocityKinds = (1u << kQrecLateral) | (1u << kQrecEchogram) | (1u << kQrecLobes);
}  // namespace

// The record traces for `emitters` emitters under the two families' kinds: none while no kind is selected, else [T][P] floats, P
// = the emitters rounded up to whole waves, times three where a velocity kind asks for the neighbours' columns
bool Solver::fitRecTrace(int emitters, unsigned timeKinds, unsigned spectralKinds) {
    if (!(timeKinds | spectralKinds)) {
        if (recTrace_) hipFree(recTrace_);
        recTrace_ = nullptr;
        recTraceCap_ = 0;
        recCols_ = 0;
        recVel_ = false;
        return true;
    }
    const int cols = (std::max(emitters, 1) + 63) / 64 * 64;
    const bool vel = (timeKinds & kVelocityKinds) != 0;
    const size_t need = (size_t)T_ * cols * (vel ? 3 : 1);
    if (need > recTraceCap_) {
        float* t = nullptr;
        if (!hipOk(hipMalloc((void**)&t, need * sizeof(float)), "hipMalloc (record traces)")) return false;
        if (recTrace_) hipFree(recTrace_);
        recTrace_ = t;
        recTraceCap_ = need;
    }
    recCols_ = cols;
    recVel_ = vel;
    return true;
}

bool Solver::setEmitterRecords(unsigned timeKinds, unsigned spectralKinds) {
    const unsigned kinds[kRecordFamilies] = {timeKinds, spectralKinds};
    for (int f = 0; f < kRecordFamilies; ++f) {  // (both families' refusals in front of either family's change)
        const std::string why = selectRefusal((RecordFamily)f, kinds[f], true);
        if (!why.empty()) return fail(why);
    }
    for (int f = 0; f < kRecordFamilies; ++f)
        if (!selectRecords((RecordFamily)f, kinds[f], true)) return false;
    // (no run in flight: selectRecords waited.  Every pass of a run writes every column of its steps: nothing to clear)
    if (!fitRecTrace(numEmitters_, timeKinds, spectralKinds)) return false;
    for (int f = 0; f < kRecordFamilies; ++f) invalidateRecords((RecordFamily)f);  // (the traces' layout may have changed)
    return true;
}

int Solver::emitterRecordFloats(RecordFamily f, unsigned kind) {
    if (!opt_.streaming) {
        fail(std::string(kEmitterPre) + kEmitterMode);
        return -1;
    }
    const int n = recordFloats(f, kind);
    if (n < 0 && err_.compare(0, std::char_traits<char>::length(recs_[f].prefix), recs_[f].prefix) == 0)
        err_ = kEmitterPre + err_.substr(std::char_traits<char>::length(recs_[f].prefix));
    return n;
}

int Solver::emitterCells(int* cxcy, int cap) const {
    for (int i = 0; i < numEmitters_ && i < cap; ++i) {
        cxcy[2 * i] = (int)(emRecCells_[i] / g_.gy);
        cxcy[2 * i + 1] = (int)(emRecCells_[i] % g_.gy);
    }
    return numEmitters_;
}

bool Solver::copyEmitterTrace(int emitter, float* outT) {
    if (!opt_.streaming) return fail("emitter trace: the solver is not in sparse-emitter mode (PvAmdGetImpulseResponse serves a solver that keeps its history)");
    if (emitter < 0 || emitter >= numEmitters_) return fail("emitter trace: no such registered emitter");
    if (pendingTimings_ && !sync()) return false;
    if (!streamedOnce_) return fail("emitter trace: no simulation has run yet");
    if (lastRun_ == LastRun::Failed) return fail("emitter trace: the last run ended in error");
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (!hipOk(hipMemcpyAsync(outT, emTrace_ + (size_t)emitter * T_, (size_t)T_ * 4, hipMemcpyDeviceToHost, stream_), "trace copy")) return false;
    return hipOk(hipStreamSynchronize(stream_), "trace sync");
}

// ----------------------------------------------------------------------------------------------------------------
// in-run records: the selector, the pinned block and the stamp, for either family
// ----------------------------------------------------------------------------------------------------------------

std::string Solver::selectRefusal(RecordFamily f, unsigned kinds, bool emitters) const {
    const RecordSet& r = recs_[f];
    const std::string pre = emitters ? kEmitterPre : r.prefix;
    if (emitters && !opt_.streaming) return pre + kEmitterMode;
    if (kinds & ~((1u << r.nKinds) - 1u)) return pre + "unknown kind bit (" + r.bits + ")";
    if (kinds) {
        if (isSlab()) return pre + "not available on a slab";
        if (opt_.streaming && !emitters) return pre + "the full pressure history is not kept in streaming-analysis mode";
        if (opt_.skipAnalysis) return pre + "the run has no onset map (PVA_OPT_SKIP_ANALYSIS)";
    }
    if (const char* why = recordKindsRefusal(f, kinds))  // (said with the family's own prefix)
        return emitters ? pre + (why + std::char_traits<char>::length(r.prefix)) : std::string(why);
    if (emitters && kinds && numEmitters_ > kMaxRecordQueries) return pre + kEmitterMax;
    return std::string();
}

bool Solver::selectRecords(RecordFamily f, unsigned kinds, bool emitters) {
    RecordSet& r = recs_[f];
    const std::string why = selectRefusal(f, kinds, emitters);
    if (!why.empty()) return fail(why);
    if (opt_.streaming && !emitters) return true;  // (kinds = 0: nothing of the output queries' is selected in this mode)
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // the launch of a run in flight still writes the pinned block
    if (kinds == r.kinds) return true;
    // (the spectrum's tables are on the device from PvAmdSetSpectrumBins on; the modulation's are made valid here)
    if (f == kRecSpectral && (kinds & (1u << kQspecModulation)) && !ensureModTable()) return false;
    const int table = opt_.streaming ? numEmitters_ : numRecQueries_;
    if (!swapRecordBlock(f, kinds, table > kMaxQueries ? table : kMaxQueries)) return false;
    r.kinds = kinds;
    return true;
}

int Solver::recordFloats(RecordFamily f, unsigned kind) {
    const RecordSet& r = recs_[f];
    const int k = oneKindBit(kind, r.nKinds);
    if (k < 0) {
        fail(std::string(r.prefix) + "exactly one kind (" + r.bits + ")");
        return -1;
    }
    const int n = recordFloatsOf(f, k);
    if (n < 0) fail(noRecordSetting(f, k));
    return n;
}

// a new pinned block in the old one's place, no run in flight: `queries` queries of `kinds` at their largest settings (no block for
// no kinds); its records are nobody's yet
bool Solver::swapRecordBlock(RecordFamily f, unsigned kinds, int queries) {
    RecordSet& r = recs_[f];
    size_t cap = 0;
    for (int k = 0; k < r.nKinds; ++k)
        if ((kinds >> k) & 1u) cap += (size_t)recordFloatsOf(f, k, true);
    float* block = nullptr;
    if (cap && !hipOk(hipHostMalloc((void**)&block, cap * queries * sizeof(float)), "hipHostMalloc")) return false;
    if (r.host) hipHostFree(r.host);
    r.host = block;
    r.blockQueries = block ? queries : 0;
    r.run = RecordSet::Run::None;
    return true;
}

// the pinned block of the selected kinds with room for `queries` queries (no run in flight); nothing while no kind is selected
bool Solver::growRecordBlock(RecordFamily f, int queries) {
    const RecordSet& r = recs_[f];
    return !r.kinds || queries <= r.blockQueries || swapRecordBlock(f, r.kinds, queries);
}

// at enqueue: the layout of the launch's nq queries -- kind k's block of nq x floats[k] at offset[k], 0 floats where it is not `on`
// -- into the launch's arguments and into the stamp, pending until sync() has seen the run through
void Solver::stampRecords(RecordFamily f, int nq, const bool* on, int* offset, int* floats) {
    RecordSet& r = recs_[f];
    int off = 0;
    for (int k = 0; k < r.nKinds; ++k) {
        r.runFloats[k] = floats[k] = on[k] ? recordFloatsOf(f, k) : 0;
        r.runOffset[k] = offset[k] = off;
        off += floats[k] * nq;
    }
    r.runKinds = r.kinds;
    r.runQueries = nq;
    r.run = RecordSet::Run::Pending;
}

// after the run has been waited for: the records of one kind, straight from pinned memory
bool Solver::readRecords(RecordFamily f, unsigned kind, float* out, int n, bool emitters) {
    const RecordSet& r = recs_[f];
    const std::string pre = emitters ? kEmitterPre : r.prefix, selector = emitters ? "PvAmdSetEmitterRecords" : r.selector;
    if (emitters && !opt_.streaming) return fail(pre + kEmitterMode);
    const int k = oneKindBit(kind, r.nKinds);
    if (k < 0) return fail(pre + "exactly one kind (" + r.bits + ")");
    if (!(r.kinds & kind) || emitters != opt_.streaming) return fail(pre + "the kind is not selected (" + selector + ")");
    if (n != recordQueryCount()) return fail(pre + (emitters ? "count differs from the registered emitters" : "count differs from the registered queries"));
    if (pendingTimings_ && !sync()) return false;
    if (lastRun_ == LastRun::Failed) return fail(pre + "the last run ended in error");
    if (r.run != RecordSet::Run::Ok || r.runKinds != r.kinds || r.runQueries != recordQueryCount() || r.runFloats[k] != recordFloatsOf(f, k))
        return fail(pre + (emitters ? "no completed run since the kinds, the emitters or the settings changed"
                                    : "no completed run since the kinds, the queries or the settings changed"));
    const float* src = r.host + r.runOffset[k];
    for (int i = 0; i < n * r.runFloats[k]; ++i) out[i] = src[i];
    return true;
}

}  // namespace pva
