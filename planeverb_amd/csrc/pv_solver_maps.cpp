// pv_solver_maps.cpp -- the per-cell analysis maps of a Solver (pv_solver.h): nine kinds computed after a run over its pressure
// history.  The kernels differ (one .hip file and one launch* per kind); everything around them is written once here: the
// refusals, the storage, the timing, the host copy, the tile-major gather and the read-backs.  A kind is a row of kAnalysisInfo,
// its computeX with the launch line, and its setting where it has one.
#include "pv_solver.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <limits>

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

namespace {
// The words of a kind's messages: every refusal starts "<prefix>: ", a failed HIP call is named "<label> launch / sync / copy";
// the two sentences are whole because their wording differs from kind to kind (noSetting: nullptr where the kind has no setting
// that can be missing).
struct AnalysisInfo {
    const char* prefix;
    const char* label;
    const char* notComputed;
    const char* noSetting;
};
const AnalysisInfo kAnalysisInfo[kAnalysisKinds] = {
    {"room metrics", "room metrics", "room metrics: not computed for the last run and the current geometry (PvAmdComputeRoomMetrics)", nullptr},
    {"decay times", "decay times", "decay times: not computed for the last run and the current geometry (PvAmdComputeDecayTimes)", nullptr},
    {"lateral fraction", "lateral fraction",
     "lateral fraction: not computed for the last run and the current geometry (PvAmdComputeLateralFraction)", nullptr},
    {"echo", "echo criterion", "echo: not computed for the last run and the current geometry (PvAmdComputeEchoCriterion)", nullptr},
    {"echogram", "echogram", "echogram: not computed for the last run, the current geometry and the current slots (PvAmdComputeEchogram)",
     "echogram: no slots set (PvAmdSetEchogram)"},
    {"lobes", "lobes", "lobes: not computed for the last run, the current geometry and the current windows (PvAmdComputeLobes)", nullptr},
    {"band metrics", "band metrics",
     "band metrics: not computed for the last run, the current geometry and the current bands (PvAmdComputeBandMetrics)",
     "band metrics: no bands set (PvAmdSetBands)"},
    {"modulation", "modulation",
     "modulation: not computed for the last run, the current geometry, the current bands and the current modulation "
     "frequencies (PvAmdComputeModulation)",
     "modulation: no bands set (PvAmdSetBands)"},
    {"spectrum", "spectrum", "spectrum: not computed for the last run, the current geometry and the current bins (PvAmdComputeSpectrum)",
     "spectrum: no bins set (PvAmdSetSpectrumBins)"},
};

// PLANEVERB_AMD_DECAY_LAUNCHES = 2: the two walks of the curve as a launch each (measurement: profiles/decay_times.txt)
bool decayTwoLaunches() {
    static const bool two = [] {
        const char* e = std::getenv("PLANEVERB_AMD_DECAY_LAUNCHES");
        return e && std::atoi(e) == 2;
    }();
    return two;
}

// "<prefix>: <what>" of kind k (appended in place: no operator+ instantiation for the library to export)
std::string refusalOf(AnalysisKind k, const char* what) {
    std::string s(kAnalysisInfo[k].prefix);
    s += ": ";
    s += what;
    return s;
}

// The register block that takes the next of `left` bins: time goes with the bins a pass holds, padding included, and B = 16 was
// the fastest form for 32 bins, B = 8 for 8 (docs/experiments/spectrum.md).  PLANEVERB_AMD_SPECTRUM_BLOCK = 8 / 16 forces one
// form (measurement).
int spectrumBlockFor(int left) {
    static const int forced = [] {
        const char* e = std::getenv("PLANEVERB_AMD_SPECTRUM_BLOCK");
        const int b = e ? std::atoi(e) : 0;
        return spectrumBlockOk(b) ? b : 0;
    }();
    if (forced) return forced;
    return left <= 8 ? 8 : 16;
}
}  // namespace

// ----------------------------------------------------------------------------------------------------------------
// what every kind shares
// ----------------------------------------------------------------------------------------------------------------

bool Solver::analysisSettingPresent(AnalysisKind k) const {
    switch (k) {
        case kMapEchogram: return echoSlots_ != 0;
        case kMapBandMetrics:
        case kMapModulation: return !bandHz_.empty();
        case kMapSpectrum: return !specHz_.empty();
        default: return true;  // (no setting, or one that is never unset: the lobes' windows)
    }
}

// the planes of a kind under the current settings, -1 where a setting is missing (the zone statistics' width: pv_solver_zones.cpp)
int Solver::zoneStatPlanes(AnalysisKind k) const {
    if (!analysisSettingPresent(k)) return -1;
    switch (k) {
        case kMapRoomMetrics: return kRoomMetricFloats;
        case kMapDecayTimes: return kDecayFloats;
        case kMapLateralFraction: return kLateralFloats;
        case kMapEchoCriterion: return kEchoFloats;
        case kMapEchogram: return echogramFloats(echoSlots_);
        case kMapLobes: return lobesFloats(lobeEdgeCount_ + 1);
        case kMapBandMetrics: return kBandFloats * (int)bandHz_.size();
        case kMapModulation: return kModFloats * (int)bandHz_.size();
        case kMapSpectrum: return kSpectrumFloats * (int)specHz_.size();
        default: return -1;
    }
}

bool Solver::analysisReadable(AnalysisKind k) {
    if (!analysisSettingPresent(k)) return fail(kAnalysisInfo[k].noSetting);
    // (a sparse-emitter solver with the kind selected by setZoneMaps: the map is the last run's own, pv_solver_zones.cpp)
    if (opt_.streaming && (zoneMapKinds_ & (k == kMapRoomMetrics ? kZoneMapRoomMetrics : k == kMapSpectrum ? kZoneMapSpectrum : 0u)))
        return zoneMapReadable(k);
    if (!maps_[k].valid) return fail(kAnalysisInfo[k].notComputed);
    return true;
}

bool Solver::analysisHipOk(AnalysisKind k, hipError_t e, const char* step) {
    if (e == hipSuccess) return true;
    std::string what(kAnalysisInfo[k].label);
    what += step;
    return hipOk(e, what.c_str());
}

void Solver::dropAnalysisMap(AnalysisKind k, bool freeDev) {
    AnalysisMap& m = maps_[k];
    m.valid = m.hostValid = false;
    if (!freeDev) return;
    if (m.dev) hipFree(m.dev);
    m.dev = nullptr;
    m.planes = 0;
}

bool Solver::beginAnalysisPass(AnalysisKind k, int planes, const char* refusal, AnalysisPass* p, bool (Solver::*prepare)()) {
    if (isSlab()) return fail(refusalOf(k, "not available on a slab"));
    if (opt_.streaming) return fail(refusalOf(k, "the full pressure history is not kept in streaming-analysis mode"));
    if (opt_.skipAnalysis) return fail(refusalOf(k, "the run has no onset map (PVA_OPT_SKIP_ANALYSIS)"));
    if (refusal) return fail(refusal);
    if (!analysisSettingPresent(k)) return fail(kAnalysisInfo[k].noSetting);
    p->kind = k;
    p->inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight; one that ends in error leaves its message)
    if (lastRun_ == LastRun::None || !dynValid_) return fail(refusalOf(k, "no completed run"));
    if (lastRun_ != LastRun::Ok) return fail(refusalOf(k, "the last run ended in error"));
    AnalysisMap& m = maps_[k];
    if (m.dev && m.planes != planes) {
        hipFree(m.dev);
        m.dev = nullptr;
    }
    if (!m.dev) {
        if (!dalloc(&m.dev, (size_t)planes * (size_t)histPlane_, false)) return false;
        m.planes = planes;
    }
    if (prepare && !(this->*prepare)()) return false;
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    m.valid = m.hostValid = false;
    p->a = analyzeArgs(lastLx_, lastLz_);
    p->dev = m.dev;
    hipEventRecord(mapEv_[0], stream_);
    return true;
}

bool Solver::endAnalysisPass(AnalysisPass& p, float* ms) {
    hipEventRecord(mapEv_[1], stream_);
    if (!analysisHipOk(p.kind, hipGetLastError(), " launch") || !analysisHipOk(p.kind, hipStreamSynchronize(stream_), " sync")) return false;
    if (ms) hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]);
    maps_[p.kind].dyn = dynCur_;
    maps_[p.kind].valid = true;
    return true;
}

bool Solver::fetchAnalysisMap(AnalysisKind k) {
    if (!analysisReadable(k)) return false;
    AnalysisMap& m = maps_[k];
    if (m.hostValid) return true;
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    m.host.resize((size_t)m.planes * (size_t)histPlane_);
    if (!analysisHipOk(k, hipMemcpyAsync(m.host.data(), m.dev, m.host.size() * 4, hipMemcpyDeviceToHost, stream_), " copy") ||
        !analysisHipOk(k, hipStreamSynchronize(stream_), " sync"))
        return false;
    m.hostValid = true;
    return true;
}

bool Solver::copyAnalysisBlock(AnalysisKind k, int r0, int c0, int nr, int nc, float* out) {
    if (r0 < 0 || c0 < 0 || nr < 1 || nc < 1 || r0 + nr > g_.gx || c0 + nc > g_.gy)
        return fail(refusalOf(k, "block outside the map"));
    if (!fetchAnalysisMap(k)) return false;
    // a cell outside the run's history window is unreached by construction; inside, its record sits at its offset in a history
    // plane (tile-major, as the device's histOffset of pv_prims.h)
    const AnalysisMap& m = maps_[k];
    const int wr0 = m.dyn.histRow0 - geo_.G, wc0 = m.dyn.histCol0 - geo_.G;
    const int wnr = histTilesX_ * rxi_, wnc = histTilesY_ * wi_;
    const int nf = m.planes;
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    for (int r = 0; r < nr; ++r)
        for (int c = 0; c < nc; ++c) {
            float* o = out + ((size_t)r * nc + c) * (size_t)nf;
            const int hr = r0 + r - wr0, hc = c0 + c - wc0;
            if (hr < 0 || hc < 0 || hr >= wnr || hc >= wnc) {
                for (int j = 0; j < nf; ++j) o[j] = qnan;
                continue;
            }
            const int ti = hr / rxi_, tj = hc / wi_;
            const size_t g = ((size_t)(ti * m.dyn.histTilesY + tj) * rxi_ + (hr - ti * rxi_)) * wi_ + (hc - tj * wi_);
            for (int j = 0; j < nf; ++j) o[j] = m.host[(size_t)j * histPlane_ + g];
        }
    return true;
}

bool Solver::analysisAt(AnalysisKind k, float ex, float ez, float* out) {
    int cx, cy;
    if (!resultCell(g_, ex, ez, &cx, &cy)) {  // (a position off the map, as getOutput finds it: nothing to fetch)
        if (!analysisReadable(k)) return false;
        for (int j = 0; j < maps_[k].planes; ++j) out[j] = std::numeric_limits<float>::quiet_NaN();
        return true;
    }
    return copyAnalysisBlock(k, cx, cy, 1, 1, out);
}

// ----------------------------------------------------------------------------------------------------------------
// the kinds without a setting: room metrics (pv_metrics.hip), decay times (pv_decay.hip), lateral energy fraction and early-sound
// direction (pv_lateral.hip), echo criterion (pv_echo.hip: refused where the speech lag is below a step)
// ----------------------------------------------------------------------------------------------------------------

bool Solver::computeRoomMetrics(float* ms) {
    AnalysisPass p;
    if (!beginAnalysisPass(kMapRoomMetrics, kRoomMetricFloats, nullptr, &p)) return false;
    launchRoomMetrics(p.a, p.dev, stream_);
    return endAnalysisPass(p, ms);
}

bool Solver::computeDecayTimes(float* ms) {
    AnalysisPass p;
    if (!beginAnalysisPass(kMapDecayTimes, kDecayFloats, nullptr, &p)) return false;
    launchDecayTimes(p.a, p.dev, decayTwoLaunches(), stream_);
    return endAnalysisPass(p, ms);
}

bool Solver::computeLateralFraction(float* ms) {
    AnalysisPass p;
    if (!beginAnalysisPass(kMapLateralFraction, kLateralFloats, nullptr, &p)) return false;
    launchLateralFraction(p.a, p.dev, stream_);
    return endAnalysisPass(p, ms);
}

bool Solver::computeEchoCriterion(float* ms) {
    const char* refusal = echoFsOk((int)g_.fs) ? nullptr : "echo: the sampling rate gives a speech lag below one step ((int)(0.009f * (float)fs) < 1)";
    AnalysisPass p;
    if (!beginAnalysisPass(kMapEchoCriterion, kEchoFloats, refusal, &p)) return false;
    launchEchoCriterion(p.a, p.dev, stream_);
    return endAnalysisPass(p, ms);
}

// ----------------------------------------------------------------------------------------------------------------
// directional echogram (pv_echogram.hip): 1 + 3 nSlots planes
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setEchogram(float slotSeconds, int nSlots) {
    if (isSlab()) return fail("echogram: not available on a slab");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (nSlots == 0 && (recs_[kRecTime].kinds & (1u << kQrecEchogram)))
        return fail(opt_.streaming ? "emitter records: echogram: the slots cannot be cleared while PVA_QREC_ECHOGRAM is selected (PvAmdSetEmitterRecords)"
                                   : "query records: echogram: the slots cannot be cleared while PVA_QREC_ECHOGRAM is selected (PvAmdSetQueryRecords)");
    invalidateRecords(kRecTime, 1u << kQrecEchogram);  // (the records in the pinned block are the old slots')
    dropAnalysisMap(kMapEchogram, nSlots == 0);
    if (nSlots == 0) {
        echoSeconds_ = 0.f;
        echoSteps_ = echoSlots_ = 0;
        return true;
    }
    echoSeconds_ = slotSeconds;
    echoSteps_ = echogramSlotSteps(slotSeconds, (int)g_.fs);
    echoSlots_ = nSlots;
    return true;
}

int Solver::echogramSlots(float* slotSeconds, int* slotSteps) const {
    if (slotSeconds && echoSlots_) *slotSeconds = echoSeconds_;
    if (slotSteps && echoSlots_) *slotSteps = echoSteps_;
    return echoSlots_;
}

bool Solver::computeEchogram(float* ms) {
    AnalysisPass p;
    if (!beginAnalysisPass(kMapEchogram, echogramFloats(echoSlots_), nullptr, &p)) return false;
    launchEchogram(p.a, p.dev, echoSteps_, echoSlots_, stream_);
    return endAnalysisPass(p, ms);
}

// ----------------------------------------------------------------------------------------------------------------
// directional energy lobes (pv_lobes.hip): 1 + 5 nW planes; the windows are never unset, a solver that was given none uses the
// default edges
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setLobeWindows(const float* edgesSeconds, int nEdges) {
    if (isSlab()) return fail("lobes: not available on a slab");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    invalidateRecords(kRecTime, 1u << kQrecLobes);  // (the records in the pinned block are the old windows')
    dropAnalysisMap(kMapLobes, false);
    if (nEdges == 0) {
        edgesSeconds = kLobesDefaultEdges;
        nEdges = 2;
    }
    for (int i = 0; i < kLobesMaxEdges; ++i) lobeEdges_[i] = i < nEdges ? edgesSeconds[i] : 0.f;
    lobeEdgeCount_ = nEdges;
    return true;
}

int Solver::lobeWindows(float* edgesSeconds, int* edgeSteps) const {
    LobeEdges ed;
    const bool ok = lobesEdgeSteps(lobeEdges_, lobeEdgeCount_, (int)g_.fs, &ed);  // (false: the default at an fs below 100)
    for (int i = 0; i < lobeEdgeCount_; ++i) {
        if (edgesSeconds) edgesSeconds[i] = lobeEdges_[i];
        if (edgeSteps) edgeSteps[i] = ok ? ed.n[i] : 0;
    }
    return lobeEdgeCount_;
}

bool Solver::computeLobes(float* ms) {
    LobeEdges ed;
    const char* refusal = lobesEdgeSteps(lobeEdges_, lobeEdgeCount_, (int)g_.fs, &ed)
                              ? nullptr
                              : "lobes: the default windows (10 ms, 80 ms) need a sampling rate of 100 Hz or more (PvAmdSetLobeWindows)";
    const int nW = lobeEdgeCount_ + 1;
    AnalysisPass p;
    if (!beginAnalysisPass(kMapLobes, lobesFloats(nW), refusal, &p)) return false;
    launchLobes(p.a, p.dev, ed, nW, stream_);
    return endAnalysisPass(p, ms);
}

// ----------------------------------------------------------------------------------------------------------------
// band metrics (pv_bands.hip): 12 planes per band
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setBands(const float* centreHz, int n, int fraction) {
    if (isSlab()) return fail("band metrics: not available on a slab");
    if (n == 0 && (recs_[kRecSpectral].kinds & kQspecBandKinds))
        return fail(opt_.streaming ? "emitter records: the bands cannot be cleared while a band kind is selected (PvAmdSetEmitterRecords)"
                                   : "spectral records: the bands cannot be cleared while a band kind is selected (PvAmdSetQuerySpectralRecords)");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    dropAnalysisMap(kMapBandMetrics, n == 0);
    dropAnalysisMap(kMapModulation, n == 0);  // (the modulation records are per band)
    invalidateRecords(kRecSpectral, kQspecBandKinds);  // (the records in the pinned block are the old bands')
    invalidateArrays(kQspecBandKinds);
    bandHz_.clear();
    bandCoefs_.clear();
    if (n == 0) return true;
    bandHz_.assign(centreHz, centreHz + n);
    bandFraction_ = fraction;
    bandCoefs_.resize((size_t)kBandCoefs * n);
    pva::bandCoefs((int)g_.fs, centreHz, n, fraction, bandCoefs_.data());
    return true;
}

int Solver::bands(float* centreHz, int cap, int* fraction) const {
    const int n = (int)bandHz_.size();
    for (int j = 0; j < n && j < cap && centreHz; ++j) centreHz[j] = bandHz_[(size_t)j];
    if (fraction && n) *fraction = bandFraction_;
    return n;
}

bool Solver::bandCoefs(float* out10n) {
    if (bandHz_.empty()) return fail("band metrics: no bands set (PvAmdSetBands)");
    std::memcpy(out10n, bandCoefs_.data(), bandCoefs_.size() * 4);
    return true;
}

bool Solver::computeBandMetrics(float* ms) {
    const int n = (int)bandHz_.size();
    AnalysisPass p;
    if (!beginAnalysisPass(kMapBandMetrics, kBandFloats * n, nullptr, &p)) return false;
    launchBandMetrics(p.a, bandCoefs_.data(), n, p.dev, stream_);
    return endAnalysisPass(p, ms);
}

// ----------------------------------------------------------------------------------------------------------------
// modulation (pv_modulation.hip): 15 planes per band of setBands; the modulation frequencies are never unset, a solver that was
// given none uses the default series
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setModulationFrequencies(const float* hz14) {
    if (isSlab()) return fail("modulation: not available on a slab");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    dropAnalysisMap(kMapModulation, false);
    modTabValid_ = false;
    for (int i = 0; i < kModFreqs; ++i) modHz_[i] = hz14 ? hz14[i] : kModDefaultHz[i];
    invalidateRecords(kRecSpectral, 1u << kQspecModulation);  // (the records in the pinned block are the old frequencies')
    invalidateArrays(1u << kQspecModulation);
    // (the next run's launch reads the table: never uploaded from the enqueue path)
    return !(recs_[kRecSpectral].kinds & (1u << kQspecModulation)) || ensureModTable();
}

// the twiddle table of the current modulation frequencies on the device (no run in flight: the upload waits for the stream)
bool Solver::ensureModTable() {
    const int T = T_;  // the run's steps (PVA_OPT_NUM_STEPS): the planes of the history
    const size_t rows = (size_t)T + kModTablePad;
    if (!modTab_ && !dalloc(&modTab_, rows * kModRowStride, false)) return false;
    if (!modTabValid_) {  // rows -kModTablePad .. -1: zero; rows 0 .. T - 1: the table, 28 floats and four zeros each
        std::vector<float> def((size_t)T * kModRowFloats), tab(rows * kModRowStride, 0.f);
        modulationTable(T, (int)g_.fs, modHz_, def.data());
        for (int t = 0; t < T; ++t)
            std::memcpy(&tab[((size_t)t + kModTablePad) * kModRowStride], &def[(size_t)t * kModRowFloats], kModRowFloats * sizeof(float));
        if (!hipOk(hipMemcpyAsync(modTab_, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, stream_), "modulation table upload") ||
            !hipOk(hipStreamSynchronize(stream_), "modulation table sync"))
            return false;
        modTabValid_ = true;
    }
    return true;
}

void Solver::modulationFrequencies(float* hz14) const {
    for (int i = 0; i < kModFreqs; ++i) hz14[i] = modHz_[i];
}

bool Solver::computeModulation(float* ms) {
    const int n = (int)bandHz_.size();
    AnalysisPass p;
    if (!beginAnalysisPass(kMapModulation, kModFloats * n, nullptr, &p, &Solver::ensureModTable)) return false;
    launchModulation(p.a, bandCoefs_.data(), n, modTab_ + (size_t)kModTablePad * kModRowStride, p.dev, stream_);
    return endAnalysisPass(p, ms);
}

// ----------------------------------------------------------------------------------------------------------------
// spectrum (pv_spectrum.hip): 3 planes per bin, one launch per pass the bins are dealt to
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setSpectrumBins(const float* hz, int n) {
    if (isSlab()) return fail("spectrum: not available on a slab");
    if (n == 0 && (recs_[kRecSpectral].kinds & (1u << kQspecSpectrum)))
        return fail(opt_.streaming ? "emitter records: the bins cannot be cleared while PVA_QSPEC_SPECTRUM is selected (PvAmdSetEmitterRecords)"
                                   : "spectral records: the bins cannot be cleared while PVA_QSPEC_SPECTRUM is selected (PvAmdSetQuerySpectralRecords)");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (n == 0 && (zoneMapKinds_ & kZoneMapSpectrum))
        return fail("spectrum: the bins cannot be cleared while PVA_ZMAP_SPECTRUM is selected (PvAmdSetZoneMaps)");
    dropAnalysisMap(kMapSpectrum, n == 0);
    invalidateRecords(kRecSpectral, 1u << kQspecSpectrum);  // (the records in the pinned block are the old bins')
    invalidateArrays(1u << kQspecSpectrum);
    for (float** p : {&specTab_, &specPow_})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    specHz_.clear();
    specPasses_.clear();
    if (n == 0) {
        specCos_.clear();
        specSin_.clear();
        specSource_.clear();
        return true;
    }
    const int T = T_;  // the run's steps (PVA_OPT_NUM_STEPS): the planes of the history; pulse_ holds at least as many
    specHz_.assign(hz, hz + n);
    specCos_.resize((size_t)T * n);
    specSin_.resize((size_t)T * n);
    spectrumTables(T, (int)g_.fs, hz, n, specCos_.data(), specSin_.data());
    specSource_.resize((size_t)3 * n);
    pva::spectrumSource(pulse_.data(), T, specCos_.data(), specSin_.data(), n, specSource_.data());
    // the device tables: per pass, rows of {cos, sin} pairs of the pass's block (bins past the slice and rows past T - 1: zero)
    const size_t rows = (size_t)T + kSpectrumTablePad;
    size_t total = 0;
    for (int b0 = 0; b0 < n;) {
        const int block = spectrumBlockFor(n - b0), bins = std::min(block, n - b0);
        specPasses_.push_back(SpecPass{b0, bins, block, total});
        total += rows * 2 * (size_t)block;
        b0 += bins;
    }
    std::vector<float> tab(total, 0.f), pw((size_t)n);
    for (const SpecPass& ps : specPasses_)
        for (int t = 0; t < T; ++t)
            for (int j = 0; j < ps.bins; ++j) {
                float* w = &tab[ps.tabOff + ((size_t)t * ps.block + j) * 2];
                w[0] = specCos_[(size_t)t * n + ps.bin0 + j];
                w[1] = specSin_[(size_t)t * n + ps.bin0 + j];
            }
    for (int j = 0; j < n; ++j) pw[(size_t)j] = specSource_[(size_t)3 * j + 2];
    const bool ok = dalloc(&specTab_, total, false) && dalloc(&specPow_, (size_t)n, false) &&
                    hipOk(hipMemcpyAsync(specTab_, tab.data(), total * 4, hipMemcpyHostToDevice, stream_), "spectrum table upload") &&
                    hipOk(hipMemcpyAsync(specPow_, pw.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream_), "spectrum table upload") &&
                    hipOk(hipStreamSynchronize(stream_), "spectrum table sync");
    if (!ok) {  // (nothing half-set: no bins)
        specHz_.clear();
        specPasses_.clear();
        if (zoneMapKinds_ & kZoneMapSpectrum) dropZoneMaps(kZoneMapSpectrum), rebuildZoneTiles();
        return false;
    }
    // (sparse-emitter mode, the spectrum selected by setZoneMaps: the storage follows the bins, every record goes back to NaN, and the
    // map of the last run is the old bins' and is refused until the next one)
    if ((zoneMapKinds_ & kZoneMapSpectrum) && !deriveZoneMaps(kZoneMapSpectrum)) {
        const std::string why = err_;
        dropZoneMaps(kZoneMapSpectrum);
        rebuildZoneTiles();
        return fail(why);
    }
    return ok;
}

int Solver::spectrumBins(float* hz, int cap) const {
    const int n = (int)specHz_.size();
    for (int j = 0; j < n && j < cap && hz; ++j) hz[j] = specHz_[(size_t)j];
    return n;
}

bool Solver::spectrumSource(float* out3n) {
    if (specHz_.empty()) return fail("spectrum: no bins set (PvAmdSetSpectrumBins)");
    std::memcpy(out3n, specSource_.data(), specSource_.size() * 4);
    return true;
}

bool Solver::computeSpectrum(float* ms) {
    AnalysisPass p;
    if (!beginAnalysisPass(kMapSpectrum, kSpectrumFloats * (int)specHz_.size(), nullptr, &p)) return false;
    for (const SpecPass& ps : specPasses_)
        launchSpectrum(p.a, ps.block, ps.bins, specTab_ + ps.tabOff, specPow_ + ps.bin0, p.dev + (size_t)3 * ps.bin0 * (size_t)histPlane_, stream_);
    return endAnalysisPass(p, ms);
}

}  // namespace pva
