// tests/host_records/records_hammer.cpp -- TEST INFRASTRUCTURE: the live module's emission records (PlaneverbSetEmissionRecords ...
// PlaneverbGetEmissionRecord, include/planeverb_amd.h) hammered from several threads in a HIP-less build (pv_core.cpp +
// pv_context.cpp + pv_capi.cpp against tests/host_records/fake_solver.h, -DPVA_HOST_TEST -DPVA_HOST_TEST_RECORDS) under
// -fsanitize=thread and -fsanitize=address,undefined.  A stand-alone program: nothing is preloaded.
//
//   records_hammer [seconds]     exit code 0 = every invariant held (a sanitizer report fails the process on its own)
//
// Phase 1, paced (the fake's gate holds the worker in front of a run, so nothing is published meanwhile): the 1 / 0 / -1 contract
//   of PlaneverbGetEmissionRecord, right after a move, an end and a re-emit included; no allocation on the 0 and 1 outcomes.
// Phase 2, paced: the cap and the ascending-id rule with 1100 emitters, ended ids and shared cells.
// Phase 3, free running: readers (GetEmissionRecord, GetOutput, EmissionRecordKinds) against threads that emit, move and end
//   emitters, move the listener and flip the kinds and the settings: every record read is of ONE iteration, of the emitter's
//   cell at the time of the read and of the kind asked for; GetOutput and a record read under an unchanged
//   PlaneverbIterationCount carry the same iteration.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <random>
#include <thread>
#include <vector>

#include "planeverb_amd.h"
#include "fake_solver.h"

// ---- operator new, counted per thread
static thread_local long long t_news = 0;
void* operator new(std::size_t n) {
    ++t_news;
    if (void* p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void* operator new[](std::size_t n) { return operator new(n); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

using pva::Solver;

static const float kSize = 25.0f;
static const int kRes = 275;
static const int kCap = 128;  // floats of the readers' buffers (the largest record: 1 + 3 x 32)
static const float kFill = -12345.f;
static float g_dx = 0.f;
static int g_gx = 0, g_gy = 0;
static std::atomic<long long> g_bad{0};
static std::atomic<bool> g_stop{false};
static std::atomic<long long> g_ones{0}, g_zeros{0}, g_minus{0}, g_paired{0};

static void bad(const char* what, long long a = 0, long long b = 0, long long c = 0) {
    if (g_bad.fetch_add(1) < 12) std::fprintf(stderr, "BAD %s (%lld, %lld, %lld)\n", what, a, b, c);
}
static void posOf(long long cell, float* x, float* z) {
    *x = (float)(((double)(cell / g_gy) + 0.5) * (double)g_dx);
    *z = (float)(((double)(cell % g_gy) + 0.5) * (double)g_dx);
}
static int bitOf(unsigned kind) {
    for (int b = 0; b < 6; ++b)
        if (kind == (1u << b)) return b;
    return -1;
}
static bool sizeOk(unsigned kind, int n) {  // a record size the churn thread's settings can give
    switch (kind) {
        case 1u: return n == 10;
        case 2u: return n == 8;
        case 4u: return n == 11;
        case 8u: return n == 1 + 3 * 4 || n == 1 + 3 * 8;
        case 16u: return n == 10;
        case 32u: return n == 16 || n == 21;
    }
    return false;
}

// One read with a pre-filled buffer: the outcome, the floats written, and -- for outcome 1 -- the iteration tag (it % 64) all its
// floats agree on.  Checks everything that holds whatever the other threads do.
struct Read {
    int r = -2, written = 0;
    long long tag = -1;
};
static Read readRecord(int id, unsigned kind, long long cell, bool cellKnown) {
    float buf[kCap];
    for (float& v : buf) v = kFill;
    const long long news = t_news;
    Read o;
    o.r = PlaneverbGetEmissionRecord(id, kind, buf, kCap);
    const long long allocated = t_news - news;
    while (o.written < kCap && !(buf[o.written] == kFill)) ++o.written;
    for (int i = o.written; i < kCap; ++i)
        if (!(buf[i] == kFill)) bad("a float behind the record was written", i);
    if (o.r == -1) {
        g_minus.fetch_add(1, std::memory_order_relaxed);
        if (o.written) bad("-1 wrote floats", o.written);
    } else if (o.r == 0 || o.r == 1) {
        if (allocated) bad("the read allocated", allocated, o.r);
        if (!sizeOk(kind, o.written)) bad("record size", kind, o.written, o.r);
        if (o.r == 0) {
            g_zeros.fetch_add(1, std::memory_order_relaxed);
            for (int i = 0; i < o.written; ++i)
                if (buf[i] == buf[i]) bad("0 with a float that is not NaN", i);
        } else {
            g_ones.fetch_add(1, std::memory_order_relaxed);
            const long long v0 = (long long)buf[0];
            for (int i = 0; i < o.written; ++i)
                if (buf[i] != buf[0]) bad("torn record", i, (long long)buf[i], v0);
            const long long gotCell = (v0 / 8) % 8192;
            o.tag = v0 / 8 / 8192;
            if ((int)(v0 % 8) != bitOf(kind)) bad("record of another kind", v0 % 8, kind);
            if (cellKnown && gotCell != cell) bad("record of another cell", gotCell, cell);
            if (Solver::noOnset(gotCell)) bad("1 for a cell without an onset", gotCell);
        }
    } else {
        bad("outcome", o.r);
    }
    return o;
}

static bool waitFor(const std::atomic<long long>& v, long long want) {
    for (int i = 0; i < 200000 && v.load() < want; ++i) std::this_thread::sleep_for(std::chrono::microseconds(50));
    return v.load() >= want;
}
// the worker stands in front of a run: nothing is published until the gate opens
static bool holdWorker() {
    for (int tries = 0; tries < 100; ++tries) {
        const long long started = Solver::startedRuns().load();
        Solver::allowedRuns().store(started);
        if (!waitFor(Solver::blockedRuns(), 1)) return false;
        // (a run that was passing the gate while it closed counts as blocked for a moment: it has started, try again)
        if (Solver::startedRuns().load() == started) return true;
    }
    return false;
}
static void releaseWorker() { Solver::allowedRuns().store(-1); }
static bool iterate(int n) {
    releaseWorker();
    const long long want = PlaneverbIterationCount() + n;
    return PlaneverbWaitIterations(want, 20000) >= want;
}

// ---- phase 1
static void contractPhase() {
    char dir[] = ".";
    const long long A = 70 * 20 + 30, B = 70 * 40 + 32, NOON = 70 * 10 + 3;  // (NOON % 7 == 3)
    if (A % 7 == 3 || B % 7 == 3 || NOON % 7 != 3) bad("cells of the contract phase");
    float buf[kCap];
    // module down
    if (PlaneverbGetEmissionRecord(0, 1u, buf, kCap) != -1 || PlaneverbEmissionRecordKinds() != 0u ||
        PlaneverbEmissionRecordFloats(1u) != -1 || PlaneverbEmissionRecordCells() != -1 || PlaneverbSetEmissionRecords(1u) != -1 ||
        std::strncmp(PvAmdLastError(), "emission records: ", 18) != 0)
        bad("module-down values");
    PlaneverbInit(kSize, kSize, kRes, 0, dir, 0, 1);
    float x, z;
    posOf(A, &x, &z);
    const int e = PlaneverbEmit(x, 0.f, z);
    posOf(NOON, &x, &z);
    const int eNo = PlaneverbEmit(x, 0.f, z);
    const int eOff = PlaneverbEmit(40.f, 0.f, 5.f);
    // refusals at the call
    if (PlaneverbSetEmissionRecords(64u) != -1 || std::strncmp(PvAmdLastError(), "emission records: ", 18) != 0) bad("unknown bit");
    if (PlaneverbSetEmissionRecords(8u) != -1 || !std::strstr(PvAmdLastError(), "no slots")) bad("echogram without slots");
    if (PlaneverbSetEmissionEchogram(0.005f, 33) != -1 || PlaneverbSetEmissionEchogram(NAN, 4) != -1) bad("echogram settings");
    const float down[2] = {0.08f, 0.01f};
    if (PlaneverbSetEmissionLobeWindows(down, 2) != -1 || PlaneverbSetEmissionLobeWindows(nullptr, 3) != -1) bad("lobe windows");
    if (PlaneverbSetEmissionEchogram(0.005f, 4) != 0 || PlaneverbSetEmissionRecords(1u | 8u | 32u) != 0) bad("accepted setters");
    if (PlaneverbSetEmissionEchogram(0.f, 0) != -1) bad("slots cleared while the echogram is selected");
    if (!iterate(6)) bad("no iterations");
    if (!holdWorker()) bad("the worker did not reach the gate");
    if (PlaneverbEmissionRecordKinds() != (1u | 8u | 32u) || PlaneverbEmissionRecordFloats(1u) != 10 ||
        PlaneverbEmissionRecordFloats(8u) != 13 || PlaneverbEmissionRecordFloats(32u) != 16 || PlaneverbEmissionRecordFloats(2u) != -1 ||
        PlaneverbEmissionRecordFloats(3u) != -1 || PlaneverbEmissionRecordCells() != 2)
        bad("published kinds, floats or cells", PlaneverbEmissionRecordKinds(), PlaneverbEmissionRecordCells());
    for (unsigned kind : {1u, 8u, 32u}) {
        if (readRecord(e, kind, A, true).r != 1) bad("1 expected", kind);
        if (readRecord(eNo, kind, NOON, true).r != 0) bad("0 expected: no onset", kind);
        if (readRecord(eOff, kind, 0, false).r != 0) bad("0 expected: off the map", kind);
        if (readRecord(77, kind, 0, false).r != 0 || readRecord(-1, kind, 0, false).r != 0) bad("0 expected: never issued", kind);
    }
    if (readRecord(e, 2u, A, true).r != -1 || readRecord(e, 3u, A, true).r != -1 || readRecord(e, 0u, A, true).r != -1 ||
        readRecord(e, 64u, A, true).r != -1)
        bad("-1 expected: kind not carried or not one bit");
    for (float& v : buf) v = kFill;
    if (PlaneverbGetEmissionRecord(e, 1u, buf, 9) != -1 || buf[0] != kFill || PlaneverbGetEmissionRecord(e, 1u, nullptr, kCap) != -1)
        bad("-1 expected: capacity or NULL");
    if (PlaneverbGetEmissionRecord(e, 1u, buf, 10) != 1 || buf[9] == kFill || buf[10] != kFill) bad("exact capacity");
    // immediacy: the read follows the emitter's position of NOW
    posOf(B, &x, &z);
    PlaneverbUpdateEmission(e, x, 0.f, z);
    if (readRecord(e, 1u, B, true).r != 0) bad("0 expected right after a move to a cell outside the table");
    posOf(NOON, &x, &z);
    PlaneverbUpdateEmission(e, x, 0.f, z);
    if (readRecord(e, 1u, NOON, true).r != 0) bad("0 expected right after a move to the cell without an onset");
    posOf(A, &x, &z);
    PlaneverbUpdateEmission(e, x, 0.f, z);
    if (readRecord(e, 1u, A, true).r != 1) bad("1 expected right after the move back");
    PlaneverbUpdateEmission(eOff, x, 0.f, z);
    if (readRecord(eOff, 1u, A, true).r != 1) bad("1 expected: another emitter moved into a cell of the table");
    PlaneverbEndEmission(e);
    if (readRecord(e, 1u, A, true).r != 0) bad("0 expected right after EndEmission");
    if (PlaneverbEmit(x, 0.f, z) != e) bad("the id is recycled");
    if (readRecord(e, 1u, A, true).r != 1) bad("1 expected: the recycled id in a cell of the table");
    posOf(B, &x, &z);
    PlaneverbUpdateEmission(e, x, 0.f, z);
    // ... and one iteration after the one in front of the gate (its table was latched before the move) the new cell is served
    if (!iterate(6) || !holdWorker()) bad("no iterations after the move");
    if (readRecord(e, 1u, B, true).r != 1 || readRecord(e, 32u, B, true).r != 1) bad("1 expected at the new cell");
    // a settings change and switching off show in the published iteration
    const float edges3[3] = {0.005f, 0.02f, 0.08f};
    if (PlaneverbSetEmissionEchogram(0.01f, 8) != 0 || PlaneverbSetEmissionLobeWindows(edges3, 3) != 0) bad("settings refused");
    if (!iterate(6) || !holdWorker()) bad("no iterations after the settings");
    if (PlaneverbEmissionRecordFloats(8u) != 25 || PlaneverbEmissionRecordFloats(32u) != 21 || readRecord(e, 8u, B, true).written != 25)
        bad("the settings did not arrive", PlaneverbEmissionRecordFloats(8u), PlaneverbEmissionRecordFloats(32u));
    if (PlaneverbSetEmissionRecords(0u) != 0 || !iterate(6) || !holdWorker()) bad("switching off");
    const long long runs = Solver::recordRuns().load();
    if (PlaneverbEmissionRecordKinds() != 0u || PlaneverbEmissionRecordCells() != 0 || readRecord(e, 1u, B, true).r != -1)
        bad("still carried after switching off");
    if (!iterate(6) || Solver::recordRuns().load() != runs) bad("records computed while switched off");
    releaseWorker();
    PlaneverbExit();
}

// ---- phase 2
static void capPhase() {
    char dir[] = ".";
    PlaneverbInit(kSize, kSize, kRes, 0, dir, 0, 1);
    // 1100 emitters in 1100 distinct cells (cell 4 i + 1), then 20 more that share cells of the first ones
    std::vector<int> ids;
    float x, z;
    for (int i = 0; i < 1100; ++i) {
        posOf(4 * i + 1, &x, &z);
        ids.push_back(PlaneverbEmit(x, 0.f, z));
    }
    for (int i = 0; i < 20; ++i) {
        posOf(4 * i + 1, &x, &z);
        ids.push_back(PlaneverbEmit(x, 0.f, z));
    }
    for (int i = 0; i < 1120; ++i)
        if (ids[(size_t)i] != i) bad("ids in order", i, ids[(size_t)i]);
    if (PlaneverbSetEmissionRecords(4u) != 0 || !iterate(6) || !holdWorker()) bad("cap phase: no iterations");
    if (PlaneverbEmissionRecordCells() != 1024) bad("cells served", PlaneverbEmissionRecordCells());
    auto expect = [&](int i, long long cell, bool inTable) {
        const int want = inTable && !Solver::noOnset(cell) ? 1 : 0;
        const Read r = readRecord(ids[(size_t)i], 4u, cell, true);
        if (r.r != want) bad("cap: outcome", i, r.r, want);
    };
    for (int i = 0; i < 1100; ++i) expect(i, 4 * i + 1, i < 1024);
    for (int i = 0; i < 20; ++i) expect(1100 + i, 4 * i + 1, true);  // (their cells are in the table through the first ones)
    // ended ids are skipped: ten of the first 1024 go, the next ten distinct cells come in
    for (int i = 100; i < 110; ++i) PlaneverbEndEmission(ids[(size_t)i]);
    if (!iterate(6) || !holdWorker()) bad("cap phase: no iterations after the ends");
    if (PlaneverbEmissionRecordCells() != 1024) bad("cells served after the ends", PlaneverbEmissionRecordCells());
    for (int i = 0; i < 1100; ++i) {
        const bool ended = i >= 100 && i < 110;
        if (ended) {
            if (readRecord(ids[(size_t)i], 4u, 0, false).r != 0) bad("cap: an ended id", i);
        } else {
            expect(i, 4 * i + 1, i < 1034);
        }
    }
    if (Solver::largestTable().load() != 1024 || Solver::badTables().load() != 0)
        bad("tables handed to the solver", Solver::largestTable().load(), Solver::badTables().load());
    releaseWorker();
    PlaneverbExit();
}

// ---- phase 3
static const int kLattice = 300;  // static emitters on cells 16 i + 5: the cells the readers hop between
static long long latticeCell(unsigned i) { return 16 * (long long)(i % kLattice) + 5; }

static void readerThread(unsigned seed) {
    std::mt19937 rng(seed);
    float x, z;
    long long cell = latticeCell(rng());
    posOf(cell, &x, &z);
    int id = PlaneverbEmit(x, 0.f, z);
    while (!g_stop.load(std::memory_order_relaxed)) {
        const unsigned dice = rng() % 16;
        if (dice == 0) {  // somewhere else: mostly a cell nobody else occupies
            cell = (long long)(rng() % (unsigned)(g_gx * g_gy));
            posOf(cell, &x, &z);
            PlaneverbUpdateEmission(id, x, 0.f, z);
        } else if (dice < 4) {
            cell = latticeCell(rng());
            posOf(cell, &x, &z);
            PlaneverbUpdateEmission(id, x, 0.f, z);
        } else if (dice == 4) {
            PlaneverbEndEmission(id);
            cell = latticeCell(rng());
            posOf(cell, &x, &z);
            id = PlaneverbEmit(x, 0.f, z);
        }
        const unsigned kind = 1u << (rng() % 6);
        const long long it1 = PlaneverbIterationCount();
        const PlaneverbOutput o = PlaneverbGetOutput(id);
        const Read r = readRecord(id, kind, cell, true);
        const unsigned kinds = PlaneverbEmissionRecordKinds();
        const long long it2 = PlaneverbIterationCount();
        if (kinds & ~63u) bad("kinds", kinds);
        if (it1 == it2) {
            if (r.r == -1 && (kinds & kind)) bad("-1 for a kind the same iteration carries", kind, kinds);
            if (r.r >= 0 && !(kinds & kind)) bad("a record of a kind the same iteration does not carry", kind, kinds);
            // the output of the same publish: an in-window record carries the run's number
            if (r.r == 1 && o.directionX == 0.25f && o.directionY == -0.5f && o.occlusion == o.sourceDirectionX) {
                g_paired.fetch_add(1, std::memory_order_relaxed);
                if (((long long)o.occlusion) % 64 != r.tag) bad("GetOutput and the record are of two iterations", (long long)o.occlusion, r.tag);
            }
        }
    }
}

static void churnThread(unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> pos(-1.f, kSize + 1.f);
    std::vector<int> em;
    const float e2[2] = {0.01f, 0.08f}, e3[3] = {0.005f, 0.02f, 0.08f};
    const unsigned sets[5] = {63u, 1u | 32u, 8u | 4u, 0u, 2u | 16u | 8u};
    while (!g_stop.load(std::memory_order_relaxed)) {
        switch (rng() % 8) {
            case 0: em.push_back(PlaneverbEmit(pos(rng), 0.f, pos(rng))); break;
            case 1:
                if (em.size() > 40) {
                    PlaneverbEndEmission(em.back());
                    em.pop_back();
                }
                break;
            case 2:
                if (!em.empty()) PlaneverbUpdateEmission(em[rng() % em.size()], pos(rng), 0.f, pos(rng));
                break;
            case 3: PlaneverbSetListenerPosition(pos(rng), 0.f, pos(rng)); break;
            case 4:
                if (rng() % 8 == 0) PlaneverbSetEmissionRecords(sets[rng() % 5]);
                break;
            case 5:
                if (rng() % 8 == 0) PlaneverbSetEmissionEchogram(rng() % 2 ? 0.005f : 0.01f, rng() % 2 ? 4 : 8);
                break;
            case 6:
                if (rng() % 8 == 0) (rng() % 2) ? PlaneverbSetEmissionLobeWindows(e2, 2) : PlaneverbSetEmissionLobeWindows(e3, 3);
                break;
            default: PlaneverbAddGeometry(pos(rng), pos(rng), 2.f, 0.5f, 0.9f); break;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

static void freePhase(double seconds) {
    char dir[] = ".";
    PlaneverbInit(kSize, kSize, kRes, 0, dir, 0, 1);
    PlaneverbSetListenerPosition(12.f, 0.f, 12.f);
    float x, z;
    for (int i = 0; i < kLattice; ++i) {
        posOf(latticeCell((unsigned)i), &x, &z);
        PlaneverbEmit(x, 0.f, z);
    }
    if (PlaneverbSetEmissionEchogram(0.005f, 4) != 0 || PlaneverbSetEmissionRecords(63u) != 0 || !iterate(6)) bad("free phase: start");
    std::vector<std::thread> th;
    th.emplace_back(readerThread, 11u);
    th.emplace_back(readerThread, 12u);
    th.emplace_back(readerThread, 13u);
    th.emplace_back(churnThread, 14u);
    std::this_thread::sleep_for(std::chrono::duration<double>(seconds));
    g_stop.store(true);
    for (auto& t : th) t.join();
    PlaneverbExit();
    if (Solver::badTables().load() != 0) bad("free phase: tables handed to the solver", Solver::badTables().load());
}

int main(int argc, char** argv) {
    const double seconds = argc > 1 ? std::atof(argv[1]) : 1.5;
    PvAmdInfo info;
    if (PvAmdHostGridInfo(kSize, kSize, kRes, &info) != 0) return 2;
    g_dx = info.dx;
    g_gx = info.gx;
    g_gy = info.gy;
    if (g_gx != 70 || g_gy != 70) return 2;
    if (PVA_RECORD_QUERIES_MAX != 1024) return 2;
    contractPhase();
    capPhase();
    freePhase(seconds);
    if (Solver::liveInstances().load() != 0) bad("solvers left behind");
    const char* pl = std::getenv("PLANEVERB_AMD_LIVE_PIPELINE");
    std::printf("records_hammer (pipeline %s): %lld records, %lld NaN reads, %lld refusals, %lld paired with GetOutput, %lld bad\n",
                pl ? pl : "default", g_ones.load(), g_zeros.load(), g_minus.load(), g_paired.load(), g_bad.load());
    return (g_bad.load() == 0 && g_ones.load() > 1000 && g_zeros.load() > 100 && g_minus.load() > 10 && g_paired.load() > 10) ? 0 : 1;
}
