// pv_solver_waterfall.cpp -- the waterfall of a Solver (pv_solver.h; the definition: pv_waterfall.h; the pass: pv_waterfall.hip): the
// setting and its device tables, the receivers of a call -- positions mapped as the output queries are, or the registered emitters
// of sparse-emitter mode with their traces as the sample source --, the record storage, the stamp and the refusals.  It is no tenth
// map kind: its records are per receiver, not per cell, and it touches none of maps_.
#include "pv_solver.h"

#include <algorithm>
#include <cstring>

#include "pv_launch.h"
#include "pv_waterfall.h"

namespace pva {

void Solver::freeWaterfall() {
    for (float** p : {&wfTab_, &wfPow_, &wfRec_})
        if (*p) {
            hipFree(*p);
            *p = nullptr;
        }
    if (wfCells_) hipFree(wfCells_);
    if (wfRx_) hipFree(wfRx_);
    wfCells_ = nullptr;
    wfRx_ = nullptr;
    wfRecFloats_ = 0;
    wfCount_ = 0;
    wfValid_ = false;
    wfHz_.clear();
    wfSeconds_ = 0.f;
    wfSteps_ = wfSlices_ = 0;
}

bool Solver::setWaterfall(const float* hz, int n, float sliceSeconds, int nSlices) {
    if (isSlab()) return fail("waterfall: not available on a slab");
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight)
    if (n == 0) {
        freeWaterfall();
        return true;
    }
    // The new tables are built and uploaded beside the old ones, which go only once that has worked: a failed allocation or upload
    // leaves the setting, the tables and the records of before.  Host memory: the device table's image (8 (T + 128) bytes per bin
    // rounded up to 64: 105 MB at T = 25 432 and 512 bins) and the tables of one block of 64 bins at a time (13 MB there)
    const int T = T_, fs = (int)g_.fs;  // the run's steps (PVA_OPT_NUM_STEPS): the planes of the history; pulse_ holds at least as many
    const int blocks = (n + 63) / 64;
    const size_t rows = (size_t)T + kWaterfallTablePad, total = (size_t)blocks * rows * 128;
    // the device table: per block of 64 bins kWaterfallTablePad zero rows, then row t = the block's 64 {cos, sin} pairs (bins past n: zero)
    std::vector<float> tab(total, 0.f), pw((size_t)n), c, s, src;
    for (int b = 0; b < blocks; ++b) {  // (a bin's table column and source power depend on its own frequency alone)
        const int j0 = b * 64, w = std::min(64, n - j0);
        c.resize((size_t)T * w);
        s.resize((size_t)T * w);
        src.resize((size_t)3 * w);
        spectrumTables(T, fs, hz + j0, w, c.data(), s.data());
        pva::spectrumSource(pulse_.data(), T, c.data(), s.data(), w, src.data());
        for (int l = 0; l < w; ++l) pw[(size_t)(j0 + l)] = src[(size_t)3 * l + 2];
        for (int t = 0; t < T; ++t) {
            float* row = &tab[((size_t)b * rows + kWaterfallTablePad + (size_t)t) * 128];
            for (int l = 0; l < w; ++l) {
                row[2 * l] = c[(size_t)t * w + l];
                row[2 * l + 1] = s[(size_t)t * w + l];
            }
        }
    }
    float *newTab = nullptr, *newPow = nullptr;
    WaterfallRx* rx = static_cast<WaterfallRx*>(wfRx_);
    int cus = 0;
    const bool ok = dalloc(&newTab, total, false) && dalloc(&newPow, (size_t)n, false) &&
                    (wfCells_ || dalloc(&wfCells_, (size_t)kWaterfallMaxReceivers, false)) &&
                    (rx || dalloc(&rx, (size_t)kWaterfallMaxReceivers, false)) &&
                    hipOk(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_), "hipDeviceGetAttribute") &&
                    hipOk(hipMemcpyAsync(newTab, tab.data(), total * 4, hipMemcpyHostToDevice, stream_), "waterfall table upload") &&
                    hipOk(hipMemcpyAsync(newPow, pw.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream_), "waterfall table upload") &&
                    hipOk(hipStreamSynchronize(stream_), "waterfall table sync");
    wfRx_ = rx;
    if (!ok) {  // (the setting of before stays)
        if (newTab) hipFree(newTab);
        if (newPow) hipFree(newPow);
        return false;
    }
    for (float** p : {&wfTab_, &wfPow_, &wfRec_})  // (the records are the old setting's)
        if (*p) hipFree(*p);
    wfTab_ = newTab;
    wfPow_ = newPow;
    wfRec_ = nullptr;
    wfRecFloats_ = 0;
    wfCount_ = 0;
    wfValid_ = false;
    wfCus_ = cus;
    wfHz_.assign(hz, hz + n);
    wfSeconds_ = sliceSeconds;
    wfSteps_ = waterfallSliceSteps(sliceSeconds, fs);
    wfSlices_ = nSlices;
    return true;
}

int Solver::waterfall(float* hz, int cap, float* sliceSeconds, int* sliceSteps, int* nSlices) const {
    const int n = (int)wfHz_.size();
    for (int j = 0; j < n && j < cap && hz; ++j) hz[j] = wfHz_[(size_t)j];
    if (sliceSeconds && n) *sliceSeconds = wfSeconds_;
    if (sliceSteps && n) *sliceSteps = wfSteps_;
    if (nSlices && n) *nSlices = wfSlices_;
    return n;
}

int Solver::waterfallRecordFloats() const { return wfHz_.empty() ? -1 : waterfallFloats((int)wfHz_.size(), wfSlices_); }

bool Solver::computeWaterfall(const float* xyz, int nPos, float* ms) {
    // every refusal first: a refused call changes nothing, the records of an earlier call included
    if (isSlab()) return fail("waterfall: not available on a slab");
    if (opt_.skipAnalysis) return fail("waterfall: the run has no onset map (PVA_OPT_SKIP_ANALYSIS)");
    if (wfHz_.empty()) return fail("waterfall: no setting (PvAmdSetWaterfall)");
    if (opt_.streaming) {
        if (xyz || nPos != 0)
            return fail("waterfall: a sparse-emitter solver takes no positions (NULL, 0): the receivers are the registered emitters (PvAmdSetEmitters)");
    } else {
        if (nPos > 0 && !xyz) return fail("waterfall: no positions");
        if (nPos < 1 || nPos > kWaterfallMaxReceivers) return fail("waterfall: 1 .. 256 positions (PVA_WATERFALL_MAX_RECEIVERS)");
    }
    const auto inUse = queue_.lockUse();
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    if (pendingTimings_ && !sync()) return false;  // (a run in flight; one that ends in error leaves its message)
    const int count = opt_.streaming ? numEmitters_ : nPos;
    if (opt_.streaming && count < 1) return fail("waterfall: no emitters registered (PvAmdSetEmitters)");
    if (opt_.streaming && count > kWaterfallMaxReceivers) return fail("waterfall: at most 256 registered emitters (PVA_WATERFALL_MAX_RECEIVERS)");
    if (lastRun_ == LastRun::None || !dynValid_ || (opt_.streaming && !streamedOnce_)) return fail("waterfall: no completed run");
    if (lastRun_ != LastRun::Ok) return fail("waterfall: the last run ended in error");

    const int n = (int)wfHz_.size(), F = waterfallFloats(n, wfSlices_);
    std::vector<long long> cells((size_t)count);
    for (int i = 0; i < count; ++i) {
        if (opt_.streaming) {
            cells[(size_t)i] = emRecCells_[i];
            continue;
        }
        int cx, cy;  // (as setOutputQueries maps its positions)
        cells[(size_t)i] = resultCell(g_, xyz[3 * i], xyz[3 * i + 2], &cx, &cy) ? (long long)cx * g_.gy + cy : -1;
    }
    const size_t need = (size_t)count * (size_t)F;
    wfValid_ = false;
    if (wfRec_ && wfRecFloats_ != need) {
        hipFree(wfRec_);
        wfRec_ = nullptr;
        wfRecFloats_ = 0;
    }
    if (!wfRec_) {
        if (!dalloc(&wfRec_, need, false)) return false;
        wfRecFloats_ = need;
    }
    for (auto& e : mapEv_)
        if (!e && !hipOk(hipEventCreate(&e), "hipEventCreate")) return false;
    if (!hipOk(hipMemcpyAsync(wfCells_, cells.data(), cells.size() * sizeof(long long), hipMemcpyHostToDevice, stream_), "waterfall cells upload") ||
        !hipOk(hipStreamSynchronize(stream_), "waterfall cells sync"))  // (`cells` is pageable: the copy is done before the timed interval)
        return false;
    const AnalyzeArgs a = analyzeArgs(lastLx_, lastLz_);
    WaterfallArgs w{};
    w.samples = opt_.streaming ? emTrace_ : hist_;
    w.rx = static_cast<const WaterfallRx*>(wfRx_);
    w.tab = wfTab_;
    w.spow = wfPow_;
    w.rec = wfRec_;
    w.nPos = count;
    w.n = n;
    w.m = wfSlices_;
    w.ns = wfSteps_;
    w.T = T_;
    hipEventRecord(mapEv_[0], stream_);
    launchWaterfallReceivers(a, wfCells_, count, opt_.streaming, static_cast<WaterfallRx*>(wfRx_), stream_);
    launchWaterfall(w, waterfallBlockFor(n, count, wfCus_), stream_);
    hipEventRecord(mapEv_[1], stream_);
    if (!hipOk(hipGetLastError(), "waterfall launch") || !hipOk(hipStreamSynchronize(stream_), "waterfall sync")) return false;
    if (ms && !hipOk(hipEventElapsedTime(ms, mapEv_[0], mapEv_[1]), "waterfall timing")) return false;
    wfCount_ = count;
    wfValid_ = true;
    return true;
}

bool Solver::copyWaterfall(float* out, int nPos) {
    if (wfHz_.empty()) return fail("waterfall: no setting (PvAmdSetWaterfall)");
    const auto inUse = queue_.lockUse();
    if (pendingTimings_ && !sync()) return false;  // (a run in flight: its records are not the ones asked for, and sync() says why)
    if (!wfValid_)
        return fail("waterfall: not computed for the last run, the current geometry, the current setting and the current emitters (PvAmdComputeWaterfall)");
    if (nPos != wfCount_) return fail("waterfall: the count differs from the computed receivers");
    if (!hipOk(hipSetDevice(device_), "hipSetDevice")) return false;
    return hipOk(hipMemcpyAsync(out, wfRec_, wfRecFloats_ * 4, hipMemcpyDeviceToHost, stream_), "waterfall copy") &&
           hipOk(hipStreamSynchronize(stream_), "waterfall sync");
}

}  // namespace pva
