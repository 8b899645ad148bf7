// tests/host_records/fake_solver.h -- TEST INFRASTRUCTURE: the HIP-less stand-in for pva::Solver of tests/host/fake_solver.h,
// with the record calls the live module's emission records use (setQueryRecords, setRecordQueries, queriedRecords and the two
// settings calls).  It is found in front of tests/host/'s by the include path of tests/host_records/Makefile, which also defines
// PVA_HOST_TEST_RECORDS.  It computes nothing acoustic: every float of a record encodes (iteration, cell, kind), so that
// records_hammer.cpp can tell a torn or mis-attributed read from a good one, and run() can be paced from the test.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "pv_core.h"

namespace pva {

struct SolverOptions {
    bool streaming = false, autoStreaming = false;
};

class Solver {
public:
    struct WindowBlock {
        int r0 = 0, c0 = 0, nr = 0, nc = 0;
        float lx = 0, lz = 0;
    };
    static constexpr int kWin = 24;  // the fake's "history window": kWin x kWin cells around the listener cell

    // ---- test hooks
    static std::atomic<long long>& liveInstances() {
        static std::atomic<long long> v{0};
        return v;
    }
    // pacing: a run() starts only while fewer than allowedRuns() runs have started in this process (-1: no limit)
    static std::atomic<long long>& allowedRuns() {
        static std::atomic<long long> v{-1};
        return v;
    }
    static std::atomic<long long>& startedRuns() {
        static std::atomic<long long> v{0};
        return v;
    }
    static std::atomic<long long>& blockedRuns() {  // run() calls waiting for the gate right now
        static std::atomic<long long> v{0};
        return v;
    }
    // what the live module handed over: the largest table, and tables that were not sorted, distinct and inside the map
    static std::atomic<int>& largestTable() {
        static std::atomic<int> v{0};
        return v;
    }
    static std::atomic<long long>& badTables() {
        static std::atomic<long long> v{0};
        return v;
    }
    static std::atomic<long long>& recordRuns() {  // runs that computed records
        static std::atomic<long long> v{0};
        return v;
    }

    // a cell "without an onset": its records are quiet NaNs
    static bool noOnset(long long cell) { return cell % 7 == 3; }
    // float of the record of `cell`, kind bit b, computed by run number `it`: exact in a float (6 + 13 + 3 bits)
    static float recordFloat(long long it, long long cell, int b) { return (float)(((it % 64) * 8192 + cell) * 8 + b); }

    static Solver* create(const GridSpec& spec, int, const SolverOptions& o, std::string* err) {
        if (spec.gx < 1 || spec.gy < 1 || (long long)spec.gx * spec.gy > 8192) {
            if (err) *err = "fake solver: 1 .. 8192 cells";
            return nullptr;
        }
        std::unique_ptr<Solver> s(new Solver());
        s->opt_ = o;
        s->g_ = spec;
        s->mat_.init(spec);
        return s.release();
    }
    ~Solver() { liveInstances().fetch_sub(1); }

    const GridSpec& spec() const { return g_; }
    int T() const { return g_.T; }
    const std::string& lastError() const { return err_; }
    SolverOptions& options() { return opt_; }
    bool setEmitters(const float*, int) { return true; }
    void rasterAdd(const Box& b) { mat_.add(b); }
    void rasterRemove(const Box& b) { mat_.remove(b); }

    // ---- the record calls (pv_solver.h)
    unsigned queryRecordKinds() const { return kinds_; }
    bool setQueryRecords(unsigned kinds) {
        if (kinds & ~63u) return fail("query records: unknown kind bit (PVA_QREC_*)");
        if ((kinds & 8u) && !echoSlots_) return fail("query records: echogram: no slots set (PvAmdSetEchogram)");
        kinds_ = kinds;
        stamped_ = false;
        return true;
    }
    int queryRecordFloats(unsigned kind) const {
        switch (kind) {
            case 1u: return 10;
            case 2u: return 8;
            case 4u: return 11;
            case 8u: return echoSlots_ ? 1 + 3 * echoSlots_ : -1;
            case 16u: return 10;
            case 32u: return 1 + 5 * (lobeEdges_ + 1);
        }
        return -1;
    }
    bool setEchogram(float, int nSlots) {
        if (nSlots == 0 && (kinds_ & 8u)) return fail("query records: echogram: the slots cannot be cleared");
        echoSlots_ = nSlots;
        stamped_ = false;
        return true;
    }
    bool setLobeWindows(const float*, int nEdges) {
        lobeEdges_ = nEdges ? nEdges : 2;
        stamped_ = false;
        return true;
    }
    bool setRecordQueries(const float* xyz, int n) {
        if (n < 0 || n > 1024) return fail("query records: at most 1024 record queries");
        cells_.resize((size_t)n);
        bool bad = false;
        for (int i = 0; i < n; ++i) {
            int cx, cy;
            cells_[(size_t)i] = resultCell(g_, xyz[3 * i], xyz[3 * i + 2], &cx, &cy) ? (long long)cx * g_.gy + cy : -1;
            bad = bad || cells_[(size_t)i] < 0 || (i > 0 && cells_[(size_t)i] <= cells_[(size_t)i - 1]);
        }
        if (bad) badTables().fetch_add(1);
        int seen = largestTable().load();
        while (n > seen && !largestTable().compare_exchange_weak(seen, n)) {
        }
        stamped_ = false;
        return true;
    }
    bool queriedRecords(unsigned kind, float* out, int n) {
        int b = -1;
        for (int k = 0; k < 6; ++k)
            if (kind == (1u << k)) b = k;
        if (b < 0 || !(kinds_ & kind)) return fail("query records: the kind is not selected (PvAmdSetQueryRecords)");
        if (!stamped_ || runKinds_ != kinds_ || n != (int)runCells_.size() || runFloats_[b] != queryRecordFloats(kind))
            return fail("query records: no completed run since the kinds, the queries or the settings changed");
        const int f = runFloats_[b];
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < f; ++j)
                out[(size_t)i * f + j] = noOnset(runCells_[(size_t)i]) ? std::numeric_limits<float>::quiet_NaN()
                                                                       : recordFloat(runIt_, runCells_[(size_t)i], b);
        return true;
    }

    bool residentKernel() const { return false; }
    bool run(float lx, float, float lz, bool, Solver* carryFrom = nullptr) {
        (void)carryFrom;
        blockedRuns().fetch_add(1);
        for (;;) {  // the gate
            const long long allowed = allowedRuns().load();
            long long started = startedRuns().load();
            if (allowed >= 0 && started >= allowed) {
                std::this_thread::sleep_for(std::chrono::microseconds(50));
                continue;
            }
            if (startedRuns().compare_exchange_weak(started, started + 1)) break;
        }
        blockedRuns().fetch_sub(1);
        ++runs_;
        lx_ = lx;
        lz_ = lz;
        int cx, cy;
        listenerCell(g_, lx, lz, &cx, &cy);
        cx = std::min(std::max(cx, 0), g_.gx - 1);
        cy = std::min(std::max(cy, 0), g_.gy - 1);
        r0_ = std::min(std::max(cx - kWin / 2, 0), std::max(0, g_.gx - kWin));
        c0_ = std::min(std::max(cy - kWin / 2, 0), std::max(0, g_.gy - kWin));
        mat_.clearDirty();
        stamped_ = false;
        if (kinds_) {  // "the records launch": the layout of this moment
            runKinds_ = kinds_;
            runCells_ = cells_;
            runIt_ = runs_;
            for (int b = 0; b < 6; ++b) runFloats_[b] = (kinds_ >> b) & 1u ? queryRecordFloats(1u << b) : 0;
            stamped_ = true;
            recordRuns().fetch_add(1);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));  // "the GPU is busy"
        return true;
    }
    bool sync() { return true; }
    size_t windowCapacity() const { return (size_t)std::min(kWin, g_.gx) * (size_t)std::min(kWin, g_.gy); }

    // record of cell (cx, cy) published by run number `it` (tests/host/fake_solver.h)
    static void record(long long it, int cx, int cy, float out[8]) {
        out[0] = (float)(it % 1000000);
        out[1] = (float)cx;
        out[2] = (float)cy;
        out[3] = (float)((it * 7 + cx) % 1000);
        out[4] = 0.25f;
        out[5] = -0.5f;
        out[6] = (float)(it % 1000000);
        out[7] = (float)(cx + cy);
    }

    bool waitPublish() { return true; }
    bool publishWindowAsync(float* dst, WindowBlock* info, bool = false) {
        WindowBlock w;
        w.r0 = r0_;
        w.c0 = c0_;
        w.nr = std::min(kWin, g_.gx - r0_);
        w.nc = std::min(kWin, g_.gy - c0_);
        w.lx = lx_;
        w.lz = lz_;
        for (int r = 0; r < w.nr; ++r)
            for (int c = 0; c < w.nc; ++c) {
                float v[8];
                record(runs_, w.r0 + r, w.c0 + c, v);
                for (int k = 0; k < 8; ++k) {
                    uint32_t u;
                    std::memcpy(&u, &v[k], 4);
                    __atomic_store_n(reinterpret_cast<uint32_t*>(dst) + ((size_t)r * w.nc + c) * 8 + k, u, __ATOMIC_RELAXED);
                }
            }
        *info = w;
        return true;
    }

    bool impulseResponseCells(int, int, void*) { return fail("fake solver: no impulse responses"); }

    static void* hostAlloc(size_t bytes) { return std::malloc(bytes); }
    static void hostFree(void* p) { std::free(p); }

private:
    Solver() { liveInstances().fetch_add(1); }
    bool fail(const char* what) {
        err_ = what;
        return false;
    }
    GridSpec g_;
    SolverOptions opt_;
    MaterialPlane mat_;
    std::string err_;
    long long runs_ = 0;
    float lx_ = 0, lz_ = 0;
    int r0_ = 0, c0_ = 0;
    unsigned kinds_ = 0, runKinds_ = 0;
    int echoSlots_ = 0, lobeEdges_ = 2;
    std::vector<long long> cells_, runCells_;
    long long runIt_ = 0;
    int runFloats_[6] = {0, 0, 0, 0, 0, 0};
    bool stamped_ = false;
};

}  // namespace pva
