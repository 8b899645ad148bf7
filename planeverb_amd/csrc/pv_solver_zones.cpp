// pv_solver_zones.cpp -- the reductions over zones of a Solver (pv_solver.h): zone statistics of a computed map (pv_zones.hip), the
// zones' ensemble decay curves (pv_zone_decay.hip: off the kept history after a run, or accumulated inside a sparse-emitter run)
// and the same per band (pv_zone_band_decay.hip).  The kernels differ; everything around them is written once here: the refusals
// in each call's own order, the lock, the window, the arguments and the scratch of the curve passes, the members pass, the
// timing and the copy.  A reduction is its own refusals, its chunk loop of launches and its finish loop.
#include "pv_solver.h"

#include <algorithm>
#include <cstring>

#include "pv_launch.h"
#include "pv_bands.h"
#include "pv_zone_band_decay.h"
#include "pv_zone_decay.h"
#include "pv_zones.h"

namespace pva {

// ----------------------------------------------------------------------------------------------------------------
// the zones and the switch of the curves inside a sparse-emitter run
// ----------------------------------------------------------------------------------------------------------------

bool Solver::setZones(const unsigned char* labels, int nZones) {
    if (isSlab()) return fail("zone statistics: not available on a slab");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (nZones == 0) {
        if (zoneCurvesOn_) return fail("zone statistics: the zones cannot be cleared while the zone curves are enabled (PvAmdSetZoneCurves)");
        if (zoneMapKinds_) return fail("zone statistics: the zones cannot be cleared while a zone map kind is selected (PvAmdSetZoneMaps)");
        zoneCount_ = 0;
        zoneHost_.clear();
        return true;
    }
    const size_t cells = (size_t)g_.gx * (size_t)g_.gy;
    if (!zoneLabels_ && !dalloc(&zoneLabels_, cells, false)) return false;
    if (!hipOk(hipMemcpyAsync(zoneLabels_, labels, cells, hipMemcpyHostToDevice, stream_), "zone labels upload") ||
        !hipOk(hipStreamSynchronize(stream_), "zone labels sync")) {
        zoneCount_ = 0;  // (the device labels are neither the old nor the new ones)
        zoneHost_.clear();
        if (zoneMapKinds_) dropZoneMaps(zoneMapKinds_);
        if (zoneCurvesOn_) disableZoneCurves();
        else rebuildZoneTiles();
        return false;
    }
    zoneHost_.assign(labels, labels + cells);
    zoneCount_ = nZones;
    // (sparse-emitter mode with the curves enabled: the tiles, the box and the buffers follow the labels; the curves of the last run
    // are the old labels' and are refused until the next one)
    if (zoneCurvesOn_ && !deriveZoneCurves()) {
        const std::string why = err_;
        if (zoneMapKinds_) dropZoneMaps(zoneMapKinds_);  // (nothing half-derived stays selected)
        disableZoneCurves();
        return fail(why);
    }
    // (a selected map kind: the tiles and the tile list follow the labels too, every record goes back to NaN, and the maps of the last
    // run are the old labels' and are refused until the next one)
    if (zoneMapKinds_ && !(rebuildZoneTiles() && deriveZoneMaps(zoneMapKinds_))) {
        const std::string why = err_;
        dropZoneMaps(zoneMapKinds_);
        rebuildZoneTiles();
        return fail(why);
    }
    return true;
}

void Solver::freeZoneCurves() {
    if (zoneCurveEtc_) hipFree(zoneCurveEtc_), deviceBytes_ -= (long long)zoneCurveEtcBytes_;
    if (zoneCurveRows_) hipFree(zoneCurveRows_), deviceBytes_ -= (long long)zoneCurveRowsBytes_;
    zoneCurveEtc_ = zoneCurveRows_ = nullptr;
    zoneCurveEtcBytes_ = zoneCurveRowsBytes_ = 0;
}

// (no run in flight) back to the emitters' tile plane; the buffers go
bool Solver::disableZoneCurves() {
    zoneCurvesOn_ = false;
    ++zoneCurveSetting_;
    freeZoneCurves();
    return rebuildZoneTiles();
}

// (no run in flight) the tiles that hold a labelled cell, for the curves or a map kind -- whoever is enabled -- and the tile plane
bool Solver::rebuildZoneTiles() {
    zoneTilesHost_.clear();
    zoneBox_[0] = 0, zoneBox_[1] = -1, zoneBox_[2] = 0, zoneBox_[3] = -1;
    std::vector<int> list;
    if ((zoneCurvesOn_ || zoneMapKinds_) && zoneCount_) {
        const int ntx = (g_.gx + rxi_ - 1) / rxi_, nty = (g_.gy + wi_ - 1) / wi_;
        if (ntx > geo_.ntx || nty > geo_.nty) return fail("the result map reaches past the tile grid");
        std::vector<unsigned char> flags((size_t)ntx * nty);
        const ZoneTileBox b = zoneTileFlags(zoneHost_.data(), g_.gx, g_.gy, rxi_, wi_, flags.data());
        zoneTilesHost_.assign((size_t)geo_.ntx * geo_.nty, 0);
        for (int ti = 0; ti < ntx; ++ti)
            for (int tj = 0; tj < nty; ++tj)
                if ((zoneTilesHost_[(size_t)ti * geo_.nty + tj] = flags[(size_t)ti * nty + tj]) != 0) list.push_back(ti * geo_.nty + tj);
        zoneBox_[0] = b.row0, zoneBox_[1] = b.row1, zoneBox_[2] = b.blk0, zoneBox_[3] = b.blk1;
    }
    // the map kinds walk the list of those tiles on the device
    zoneMapTileCount_ = 0;
    if (zoneMapKinds_ && !list.empty()) {
        if ((int)list.size() > zoneMapTileCap_) {
            if (zoneMapTiles_) hipFree(zoneMapTiles_), deviceBytes_ -= (long long)zoneMapTileCap_ * (long long)sizeof(int);
            zoneMapTiles_ = nullptr;
            zoneMapTileCap_ = 0;
            if (!dalloc(&zoneMapTiles_, list.size(), false)) return false;
            zoneMapTileCap_ = (int)list.size();
        }
        if (!hipOk(hipMemcpyAsync(zoneMapTiles_, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, stream_), "zone tile list")) return false;
        zoneMapTileCount_ = (int)list.size();
    } else if (!zoneMapKinds_ && zoneMapTiles_) {
        hipFree(zoneMapTiles_), deviceBytes_ -= (long long)zoneMapTileCap_ * (long long)sizeof(int);
        zoneMapTiles_ = nullptr;
        zoneMapTileCap_ = 0;
    }
    return uploadTileEmit() && hipOk(hipStreamSynchronize(stream_), "tile plane upload");  // (the list above is a local: copied by now)
}

bool Solver::deriveZoneCurves() {
    ++zoneCurveSetting_;
    if (!rebuildZoneTiles()) return false;
    const int rows = std::max(zoneBox_[1] - zoneBox_[0] + 1, 1);
    // the steps of a pass per pair of launches; a pass has halfRing_ of them at the most
    zoneCurveChunk_ = std::min(streamZoneCurveChunk(zoneCount_, rows, kZoneScratchBytes),
                               (halfRing_ + kZoneCurveSlots - 1) / kZoneCurveSlots * kZoneCurveSlots);
    const size_t etcBytes = (size_t)zoneCount_ * (size_t)T_ * sizeof(double);
    const size_t rowsBytes = (size_t)zoneCurveChunk_ * (size_t)zoneCount_ * (size_t)rows * sizeof(double);
    if (etcBytes != zoneCurveEtcBytes_ || rowsBytes > zoneCurveRowsBytes_) {
        freeZoneCurves();
        if (!dalloc(&zoneCurveEtc_, etcBytes / sizeof(double), false)) return false;
        zoneCurveEtcBytes_ = etcBytes;
        if (!dalloc(&zoneCurveRows_, rowsBytes / sizeof(double), false)) return false;
        zoneCurveRowsBytes_ = rowsBytes;
    }
    return true;
}

bool Solver::setZoneCurves(bool on) {
    if (isSlab()) return fail("zone curves: not available on a slab");
    if (!opt_.streaming) return fail("zone curves: sparse-emitter solvers only (PVA_OPT_STREAMING_ANALYSIS): a solver that keeps its history computes the curves after the run");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight reads the tile plane and writes the curves)
    if (!on) return zoneCurvesOn_ ? disableZoneCurves() : true;
    if (!zoneCount_) return fail("zone curves: no zones set (PvAmdSetZones)");
    if (zoneCurvesOn_) return true;
    zoneCurvesOn_ = true;
    if (!deriveZoneCurves()) {
        const std::string why = err_;
        disableZoneCurves();
        return fail("zone curves: " + why);
    }
    return true;
}

bool Solver::zoneCurves() const {
    const auto inUse = queue_.lockUse();
    return zoneCurvesOn_;
}

// ----------------------------------------------------------------------------------------------------------------
// the zones' per-cell maps inside a sparse-emitter run (pv_zone_maps.hip)
// ----------------------------------------------------------------------------------------------------------------

namespace {
constexpr AnalysisKind kZoneMapKindOf[2] = {kMapRoomMetrics, kMapSpectrum};
}

// (no run in flight) the storage of `kinds` at the current plane counts and quiet NaN in every plane of it: a run writes the labelled
// cells only, and writes every one of them.  The maps of the last run are no longer the current setting's
bool Solver::deriveZoneMaps(unsigned kinds) {
    for (int i = 0; i < 2; ++i) {
        if (!(kinds & (1u << i))) continue;
        const AnalysisKind k = kZoneMapKindOf[i];
        const int planes = zoneStatPlanes(k);
        if (planes < 1) return fail(std::string("zone maps: ") + (i ? "no bins set (PvAmdSetSpectrumBins)" : "no planes"));
        ++zoneMapSetting_[i];
        AnalysisMap& m = maps_[k];
        m.valid = m.hostValid = false;
        if (m.dev && m.planes != planes) {
            hipFree(m.dev);
            deviceBytes_ -= (long long)m.planes * histPlane_ * 4;
            m.dev = nullptr;
            m.planes = 0;
        }
        if (!m.dev) {
            if (!dalloc(&m.dev, (size_t)planes * (size_t)histPlane_, false)) return false;
            m.planes = planes;
        }
        if (!hipOk(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.dev), 0x7fc00000, (size_t)planes * (size_t)histPlane_, stream_), "zone map fill"))
            return false;
    }
    return hipOk(hipStreamSynchronize(stream_), "zone map fill");
}

void Solver::dropZoneMaps(unsigned kinds) {
    for (int i = 0; i < 2; ++i) {
        if (!(kinds & zoneMapKinds_ & (1u << i))) continue;
        AnalysisMap& m = maps_[kZoneMapKindOf[i]];
        if (m.dev) hipFree(m.dev), deviceBytes_ -= (long long)m.planes * histPlane_ * 4;
        m.dev = nullptr;
        m.planes = 0;
        m.valid = m.hostValid = false;
        std::vector<float>().swap(m.host);
        ++zoneMapSetting_[i];
    }
    zoneMapKinds_ &= ~kinds;
}

bool Solver::setZoneMaps(unsigned kinds) {
    if (kinds & ~(kZoneMapRoomMetrics | kZoneMapSpectrum)) return fail("zone maps: kinds is a combination of PVA_ZMAP_ROOM_METRICS and PVA_ZMAP_SPECTRUM");
    if (!opt_.streaming)
        return fail("zone maps: sparse-emitter solvers only (PVA_OPT_STREAMING_ANALYSIS): a solver that keeps its history computes the maps after the run "
                    "(PvAmdComputeRoomMetrics, PvAmdComputeSpectrum)");
    if (isSlab()) return fail("zone maps: not available on a slab");
    if (opt_.skipAnalysis) return fail("zone maps: the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight reads the tile plane and writes the maps)
    if (kinds && !zoneCount_) return fail("zone maps: no zones set (PvAmdSetZones)");
    if ((kinds & kZoneMapSpectrum) && specHz_.empty()) return fail("zone maps: PVA_ZMAP_SPECTRUM: no bins set (PvAmdSetSpectrumBins)");
    if (kinds == zoneMapKinds_) return true;
    const unsigned fresh = kinds & ~zoneMapKinds_;
    dropZoneMaps(zoneMapKinds_ & ~kinds);
    zoneMapKinds_ = kinds;
    if (!(rebuildZoneTiles() && deriveZoneMaps(fresh))) {
        const std::string why = err_;
        dropZoneMaps(fresh);
        rebuildZoneTiles();
        return fail(why.rfind("zone maps: ", 0) == 0 ? why : "zone maps: " + why);
    }
    return true;
}

unsigned Solver::zoneMaps() const {
    const auto inUse = queue_.lockUse();
    return zoneMapKinds_;
}

// a read of kind k's map on a sparse-emitter solver that has the kind selected: the run in flight waited for, then the refusals
bool Solver::zoneMapReadable(AnalysisKind k) {
    const int i = k == kMapSpectrum ? 1 : 0;
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight; one that ends in error leaves its message)
    std::string pre(k == kMapSpectrum ? "spectrum: " : "room metrics: ");
    if (const char* why = zoneRunRefusal()) return fail(pre + why);
    if (zoneMapRun_[i] != zoneMapSetting_[i])
        return fail(pre + "the last run was enqueued before the kind was selected (PvAmdSetZoneMaps) or before the current zones or bins were set");
    if (!maps_[k].valid) return fail(pre + "not accumulated for the last run and the current geometry");
    return true;
}

ZoneMapArgs Solver::zoneMapArgs(const AnalyzeArgs& a) const {
    ZoneMapArgs z{};
    z.hist = a.hist;
    z.histPlane = a.histPlane;
    z.onset = sOnset_;
    z.labels = zoneLabels_;
    z.dyn = a.dyn;
    z.tiles = zoneMapTiles_;
    z.nTiles = zoneMapTileCount_;
    z.gx = g_.gx;
    z.gy = g_.gy;
    z.G = geo_.G;
    z.rxi = rxi_;
    z.wi = wi_;
    z.nty = geo_.nty;
    z.ring = ring_;
    z.T = T_;
    z.fs = (int)g_.fs;
    z.room = (zoneMapKinds_ & kZoneMapRoomMetrics) ? maps_[kMapRoomMetrics].dev : nullptr;
    z.spec = (zoneMapKinds_ & kZoneMapSpectrum) ? maps_[kMapSpectrum].dev : nullptr;
    z.nBins = (int)specHz_.size();
    z.specPow = specPow_;
    return z;
}

int Solver::zones(unsigned char* labels) const {
    const auto inUse = queue_.lockUse();  // (setZones changes both under it)
    if (labels && zoneCount_) std::memcpy(labels, zoneHost_.data(), zoneHost_.size());
    return zoneCount_;
}

int Solver::zoneDecayChunkSlots() const { return streamZoneCurveChunk(zoneCount_, g_.gx, kZoneScratchBytes); }

int Solver::zoneBandDecayChunks(int* slots, int* bands) const {
    const auto inUse = queue_.lockUse();  // (setZones and setBands change what is read here under it)
    const int nb = (int)bandHz_.size();
    if (slots) *slots = T_;
    if (bands) *bands = 0;
    if (!zoneCount_ || !nb) return 0;
    return pva::zoneBandDecayChunks(g_.gx, T_, zoneCount_, nb, kZoneScratchBytes, nullptr, bands);
}

// ----------------------------------------------------------------------------------------------------------------
// what every reduction shares
// ----------------------------------------------------------------------------------------------------------------

bool Solver::growZoneScratch(size_t need) {
    if (zoneScratchBytes_ >= need) return true;
    if (zoneScratch_) {
        hipFree(zoneScratch_);
        deviceBytes_ -= (long long)zoneScratchBytes_;
        zoneScratch_ = nullptr;
        zoneScratchBytes_ = 0;
    }
    if (!dalloc(&zoneScratch_, need, false)) return false;
    zoneScratchBytes_ = need;
    return true;
}

// the window of the run `dyn` describes, tilesX x tilesY tiles of it, in result coordinates (as copyAnalysisBlock reads it)
ZoneWindow Solver::zoneWindow(const DynParams& dyn, int tilesX, int tilesY) const {
    ZoneWindow w{};
    w.r0 = dyn.histRow0 - geo_.G;
    w.c0 = dyn.histCol0 - geo_.G;
    w.nr = tilesX * rxi_;
    w.nc = tilesY * wi_;
    w.rxi = rxi_;
    w.wi = wi_;
    w.tilesY = dyn.histTilesY;
    return w;
}

// what every curve pass is told: the planes, the window as the last run recorded it, the onset map and the labels.  The chunk and
// the scratch are the caller's; a sparse-emitter run embeds these in its own arguments (enqueueStreamingRun)
ZoneCurveArgs Solver::zoneCurveArgs() const {
    ZoneCurveArgs a{};
    a.hist = hist_;
    a.histPlane = histPlane_;
    a.w = zoneWindow(dynCur_, std::min(dynCur_.histTilesX, histTilesX_), std::min(dynCur_.histTilesY, histTilesY_));
    a.delay = delay_;
    a.labels = zoneLabels_;
    a.gx = g_.gx;
    a.gy = g_.gy;
    a.nZones = zoneCount_;
    a.T = T_;
    return a;
}

bool Solver::zoneHipOk(const ZonePass& p, hipError_t e, const char* step) {
    if (e == hipSuccess) return true;
    return hipOk(e, (std::string(p.name) + step).c_str());
}

// What every call refuses ahead of the lock -- a slab; a sparse-emitter solver where the call needs the kept history
// (kZoneNeedsHistory); a solver without onset map where it needs one (kZoneNeedsOnsets), in that order --, then the lock, the device
// and the wait for a run in flight.  The refusals under the lock are the caller's, listed there in ITS order: the four calls do
// not test alike, and a caller sees the first refusal that holds
bool Solver::beginZonePass(ZonePass* p, const char* name, unsigned flags) {
    p->name = name;
    if (isSlab()) return zoneRefuse(*p, "not available on a slab");
    if ((flags & kZoneNeedsHistory) && opt_.streaming) return zoneRefuse(*p, "the full pressure history is not kept in streaming-analysis mode");
    if ((flags & kZoneNeedsOnsets) && opt_.skipAnalysis) return zoneRefuse(*p, "the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    p->inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    return !pendingTimings_ || sync();  // (a run in flight; one that ends in error leaves its message)
}

bool Solver::zoneRefuse(const ZonePass& p, const std::string& what) { return fail(std::string(p.name) + ": " + what); }

// the refusals of a call that reads the last run directly (nullptr: there is one, and it ended well)
const char* Solver::zoneRunRefusal() const {
    if (lastRun_ == LastRun::None || !dynValid_) return "no completed run";
    return lastRun_ != LastRun::Ok ? "the last run ended in error" : nullptr;
}

// the event pair of the analysis passes, and the first event
bool Solver::startZoneTimer() {
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    hipEventRecord(mapEv_[0], stream_);
    return true;
}

// A curve pass behind the refusals: the scratch (pv_zone_decay.h zoneCurveScratch: rowsBytes of row sums, etcBytes of curves,
// member rows, members), the arguments, the first event and the members pass.  runCurves: where the curves are when they are
// not this call's to compute -- a sparse-emitter solver's, accumulated by the last run (etcBytes = 0 then).  The caller enqueues
// its curve launches with p->c on stream_
bool Solver::beginZoneCurves(ZonePass* p, size_t rowsBytes, size_t etcBytes, double* runCurves) {
    const ZoneCurveScratch s = zoneCurveScratch(rowsBytes, etcBytes, zoneCount_, g_.gx);
    if (!growZoneScratch(s.total)) return false;
    ZoneCurveArgs& c = p->c = zoneCurveArgs();
    c.rows = reinterpret_cast<double*>(zoneScratch_ + s.rows);
    c.etc = runCurves ? runCurves : reinterpret_cast<double*>(zoneScratch_ + s.etc);
    c.memberRows = reinterpret_cast<ZoneMembers*>(zoneScratch_ + s.memberRows);
    c.members = reinterpret_cast<ZoneMembers*>(zoneScratch_ + s.members);
    if (!startZoneTimer()) return false;
    launchZoneMembers(c, stream_);
    return true;
}

// the second event, the launch check, `curves` curves of T doubles into *etc (nullptr: into the pass's own vector, and *etc is
// set to it) and the zones' members into p.members, the wait, *ms
bool Solver::endZoneCurves(ZonePass& p, size_t curves, double** etc, float* ms) {
    hipEventRecord(mapEv_[1], stream_);
    if (!*etc) p.etcHost.resize(curves * (size_t)T_), *etc = p.etcHost.data();
    p.members.resize((size_t)zoneCount_);
    if (!zoneHipOk(p, hipGetLastError(), " launch") ||
        !zoneHipOk(p, hipMemcpyAsync(*etc, p.c.etc, curves * (size_t)T_ * sizeof(double), hipMemcpyDeviceToHost, stream_), " copy") ||
        !zoneHipOk(p, hipMemcpyAsync(p.members.data(), p.c.members, p.members.size() * sizeof(ZoneMembers), hipMemcpyDeviceToHost, stream_), " copy") ||
        !zoneHipOk(p, hipStreamSynchronize(stream_), " sync"))
        return false;
    if (ms) hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]);
    return true;
}

// ----------------------------------------------------------------------------------------------------------------
// zone statistics (pv_zones.hip): one reduction for every kind, straight off the kind's device planes
// ----------------------------------------------------------------------------------------------------------------

bool Solver::computeZoneStats(AnalysisKind k, void* out, int cap, float* ms, int* count) {
    ZonePass p;
    // (a sparse-emitter solver has a map of the two kinds of setZoneMaps while they are selected, and no other)
    const auto pre = queue_.lockUse();
    const unsigned bit = k == kMapRoomMetrics ? kZoneMapRoomMetrics : k == kMapSpectrum ? kZoneMapSpectrum : 0u;
    if (!beginZonePass(&p, "zone statistics", (opt_.streaming && (zoneMapKinds_ & bit)) ? 0u : kZoneNeedsHistory)) return false;
    const AnalysisMap& m = maps_[k];
    // (neither the run nor the onset map is tested here: analysisReadable refuses where the kind has no valid map)
    if (!zoneCount_) return zoneRefuse(p, "no zones set (PvAmdSetZones)");
    if (!analysisReadable(k)) return zoneRefuse(p, std::string(err_));
    if (cap < zoneCount_ * m.planes) return zoneRefuse(p, "PvAmdComputeZoneStats: the output holds fewer than nZones x planes records");
    const int records = zoneCount_ * m.planes;
    // scratch: the rows' records and m2 sums of one chunk of planes, then the zones' records
    const size_t perPlane = (size_t)zoneCount_ * (size_t)g_.gx * (sizeof(ZoneRow) + sizeof(double));
    const int chunk = (int)std::min<size_t>((size_t)m.planes, std::max<size_t>(1, kZoneScratchBytes / perPlane));
    const size_t rowsBytes = (size_t)chunk * (size_t)zoneCount_ * (size_t)g_.gx * sizeof(ZoneRow), m2Bytes = perPlane * chunk - rowsBytes;
    const size_t need = rowsBytes + m2Bytes + (size_t)records * sizeof(ZoneStat);
    if (!growZoneScratch(need)) return false;
    ZoneArgs a{};
    a.histPlane = histPlane_;
    a.w = zoneWindow(m.dyn, histTilesX_, histTilesY_);
    a.labels = zoneLabels_;
    a.gx = g_.gx;
    a.gy = g_.gy;
    a.nZones = zoneCount_;
    a.totalPlanes = m.planes;
    a.rows = reinterpret_cast<ZoneRow*>(zoneScratch_);
    a.rowM2 = reinterpret_cast<double*>(zoneScratch_ + rowsBytes);
    a.out = reinterpret_cast<ZoneStat*>(zoneScratch_ + rowsBytes + m2Bytes);
    if (!startZoneTimer()) return false;
    for (int p0 = 0; p0 < m.planes; p0 += chunk) {
        a.map = m.dev + (size_t)p0 * (size_t)histPlane_;
        a.plane0 = p0;
        a.planes = std::min(chunk, m.planes - p0);
        launchZoneStats(a, stream_);
    }
    hipEventRecord(mapEv_[1], stream_);
    ZoneStat* recs = static_cast<ZoneStat*>(out);
    if (!zoneHipOk(p, hipGetLastError(), " launch") ||
        !zoneHipOk(p, hipMemcpyAsync(recs, a.out, (size_t)records * sizeof(ZoneStat), hipMemcpyDeviceToHost, stream_), " copy") ||
        !zoneHipOk(p, hipStreamSynchronize(stream_), " sync"))
        return false;
    if (ms) hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]);
    for (int i = 0; i < records; ++i) zoneStatFinish(&recs[i]);
    *count = records;
    return true;
}

// ----------------------------------------------------------------------------------------------------------------
// zone decay (pv_zone_decay.hip): the ensemble decay curve of every zone, straight off the history planes and the onset map -- or,
// on a sparse-emitter solver, the last run's own (enqueueStreamingRun): there no curve kernel is launched here, what is left is the
// members pass over the finalize pass's delay map, one copy and the host finish, and *ms is the members pass
// ----------------------------------------------------------------------------------------------------------------

bool Solver::computeZoneDecay(int align, void* out, int cap, double* etc, double* edc, float* ms, int* count) {
    const bool ring = opt_.streaming;
    ZonePass p;
    if (!beginZonePass(&p, "zone decay", kZoneNeedsOnsets)) return false;
    if (ring && !zoneCurvesOn_)
        return zoneRefuse(p, "the full pressure history is not kept in streaming-analysis mode: the ABSOLUTE curves are accumulated "
                             "inside the runs that follow PvAmdSetZoneCurves");
    if (ring && align != kZoneDecayAbsolute)
        return zoneRefuse(p, "onset-synchronised curves need the full pressure history, which streaming-analysis mode does not keep "
                             "(PVA_ZONE_DECAY_ABSOLUTE only)");
    if (!zoneCount_) return zoneRefuse(p, "no zones set (PvAmdSetZones)");
    if (cap < zoneCount_) return zoneRefuse(p, "PvAmdComputeZoneDecay: the output holds fewer than nZones records");
    if (const char* why = zoneRunRefusal()) return zoneRefuse(p, why);
    if (ring && zoneCurveRun_ != zoneCurveSetting_)
        return zoneRefuse(p, "the last run was enqueued before the zone curves were enabled or before the current zones were set");
    const int T = T_, nz = zoneCount_;
    // scratch: the row sums of one chunk of slots and the curves (neither on a sparse-emitter solver), the member rows and records
    const int chunk = std::min(zoneDecayChunkSlots(), T);
    const size_t rowsBytes = ring ? 0 : (size_t)chunk * (size_t)nz * (size_t)g_.gx * sizeof(double);
    if (!beginZoneCurves(&p, rowsBytes, ring ? 0 : (size_t)nz * (size_t)T * sizeof(double), ring ? zoneCurveEtc_ : nullptr)) return false;
    if (!ring)  // (a sparse-emitter solver: p.c.etc is the last run's own, and nothing but the members pass is launched)
        for (int j0 = 0; j0 < T; j0 += chunk) {
            p.c.slot0 = j0;
            p.c.slots = std::min(chunk, T - j0);
            launchZoneCurves(p.c, align == kZoneDecayOnset, stream_);
        }
    if (!endZoneCurves(p, (size_t)nz, &etc, ms)) return false;
    std::vector<double> edcHost(edc ? 0 : (size_t)T);
    ZoneDecay* recs = static_cast<ZoneDecay*>(out);
    for (int z = 0; z < nz; ++z) {
        recs[z].n_cells = p.members[(size_t)z].n_cells;
        recs[z].t_first = p.members[(size_t)z].t_first;
        recs[z].t_last = p.members[(size_t)z].t_last;
        zoneDecayFinish(etc + (size_t)z * T, edc ? edc + (size_t)z * T : edcHost.data(), T, (int)g_.fs, align, &recs[z]);
    }
    *count = nz;
    return true;
}

// ----------------------------------------------------------------------------------------------------------------
// zone band decay (pv_zone_band_decay.hip): the same curve per band of setBands, off the band-filtered history
// ----------------------------------------------------------------------------------------------------------------

bool Solver::computeZoneBandDecay(int align, void* out, int cap, double* etc, double* edc, float* ms, int* count) {
    ZonePass p;
    if (!beginZonePass(&p, "zone band decay", kZoneNeedsHistory | kZoneNeedsOnsets)) return false;
    if (!zoneCount_) return zoneRefuse(p, "no zones set (PvAmdSetZones)");
    if (bandHz_.empty()) return zoneRefuse(p, "no bands set (PvAmdSetBands)");
    if (cap < zoneCount_ * (int)bandHz_.size())
        return zoneRefuse(p, "PvAmdComputeZoneBandDecay: the output holds fewer than nZones x nBands records");
    if (const char* why = zoneRunRefusal()) return zoneRefuse(p, why);
    const int T = T_, nz = zoneCount_, nBands = (int)bandHz_.size(), records = nz * nBands;
    // scratch: the rows of one chunk of pairs, the curves, the zones' member rows and records
    int zonesPer = 0, bandsPer = 0;
    pva::zoneBandDecayChunks(g_.gx, T, nz, nBands, kZoneScratchBytes, &zonesPer, &bandsPer);
    const size_t pairBytes = (size_t)g_.gx * (size_t)T * sizeof(double);
    if (!beginZoneCurves(&p, (size_t)zonesPer * (size_t)bandsPer * pairBytes, (size_t)records * (size_t)T * sizeof(double))) return false;
    ZoneBandCurveArgs a{};
    a.c = p.c;
    a.nBands = nBands;
    std::copy(bandCoefs_.begin(), bandCoefs_.begin() + (size_t)nBands * kBandCoefs, a.coefs);
    for (int z0 = 0; z0 < nz; z0 += zonesPer)
        for (int b0 = 0; b0 < nBands; b0 += bandsPer) {
            a.zone0 = z0;
            a.zones = std::min(zonesPer, nz - z0);
            a.band0 = b0;
            a.bands = std::min(bandsPer, nBands - b0);
            if (!zoneHipOk(p, hipMemsetAsync(a.c.rows, 0, (size_t)a.zones * (size_t)a.bands * pairBytes, stream_), " clear")) return false;
            launchZoneBandCurves(a, align == kZoneDecayOnset, stream_);
        }
    if (!endZoneCurves(p, (size_t)records, &etc, ms)) return false;
    std::vector<double> edcHost(edc ? 0 : (size_t)T);
    ZoneBandDecay* recs = static_cast<ZoneBandDecay*>(out);
    for (int z = 0; z < nz; ++z)
        for (int b = 0; b < nBands; ++b) {
            const size_t r = (size_t)z * nBands + b;
            const ZoneMembers& m = p.members[(size_t)z];
            zoneBandDecayFinish(etc + r * T, edc ? edc + r * T : edcHost.data(), T, (int)g_.fs, align, m.n_cells, m.t_first, m.t_last, &recs[r]);
        }
    *count = records;
    return true;
}

}  // namespace pva
