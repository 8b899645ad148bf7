// tests/host/alloc_fault_round.cpp -- TEST INFRASTRUCTURE: the round and concave live-module calls under allocation failure.
//
// The method of alloc_fault.cpp, for PlaneverbAdd/Update/Remove{Disc, WallPath, ConcavePolygon}Geometry: the global operator
// new of a HIP-less build of the live module (pv_core.cpp + pv_context.cpp + pv_capi.cpp against fake_solver.h) fails the
// 0th, 1st, 2nd ... allocation a call makes, one at a time, until the call gets through.  After every injected failure the
// call has returned (an exception across extern "C" would have ended the process) with its sentinel, PvAmdLastError names the
// function, and the shape id table is what it was: the next un-faulted Add hands out the id the failed one would have.
//
//   alloc_fault_round     exit code 0 = every sweep held
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include "planeverb_amd.h"
#include "fake_solver.h"

static thread_local long t_failAt = -1;  // >= 0: fail the allocation that finds this at 0 (this thread), once
static thread_local bool t_fired = false;

static void* hookedAlloc(std::size_t n) {
    if (t_failAt >= 0 && t_failAt-- == 0) {
        t_fired = true;
        throw std::bad_alloc();
    }
    void* p = std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void* operator new(std::size_t n) { return hookedAlloc(n); }
void* operator new[](std::size_t n) { return hookedAlloc(n); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }
void operator delete[](void* p, std::size_t) noexcept { std::free(p); }

static int g_failures = 0;
#define EXPECT(cond, ...)                                             \
    do {                                                              \
        if (!(cond)) {                                                \
            ++g_failures;                                             \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                        \
            std::fprintf(stderr, "\n");                               \
        }                                                             \
    } while (0)

static bool lastErrorNames(const char* fn) {
    const char* e = PvAmdLastError();
    return e && std::strstr(e, "exception in ") && std::strstr(e, fn) && std::strstr(e, "bad_alloc");
}

static long g_faults = 0;
template <class Call, class After>
static void sweep(const char* what, Call call, After after, int limit = 4000) {
    int k = 0;
    for (; k < limit; ++k) {
        t_fired = false;
        t_failAt = k;
        call();
        t_failAt = -1;
        const bool faulted = t_fired;
        after(faulted);
        if (!faulted) break;
    }
    EXPECT(k < limit, "%s: still faulting after %d allocations", what, limit);
    g_faults += k;
}

int main() {
    static char tmp[] = "";
    PlaneverbInit(25.f, 25.f, 275, 0, tmp, 0, 0);
    PlaneverbWaitIterations(1, 5000);
    EXPECT(PlaneverbIsRunning() == 1, "module did not come up: %s", PvAmdLastError());

    float path[2 * 64], poly[2 * 64];
    for (int i = 0; i < 64; ++i) {
        path[2 * i] = 1.f + 0.3f * i;
        path[2 * i + 1] = 3.f + (i % 2);
        // a comb: 64 vertices, concave
        poly[2 * i] = i < 32 ? 2.f + 0.5f * i : 2.f + 0.5f * (63 - i);
        poly[2 * i + 1] = i < 32 ? 8.f + (i % 2) : 12.f;
    }
    int nextId = 0;
    for (int round = 0; round < 60; ++round) {  // (the change queue and the id tables grow several times)
        int got = -2;
        const char* fn = round % 3 == 0 ? "PlaneverbAddDiscGeometry" : round % 3 == 1 ? "PlaneverbAddWallPathGeometry" : "PlaneverbAddConcavePolygonGeometry";
        sweep(fn,
              [&] {
                  if (round % 3 == 0) got = PlaneverbAddDiscGeometry(5.f + 0.1f * round, 5.f, 1.f, 0.5f);
                  if (round % 3 == 1) got = PlaneverbAddWallPathGeometry(path, 2 + round, 0.25f, 0.5f);
                  if (round % 3 == 2) got = PlaneverbAddConcavePolygonGeometry(poly, 64, 0.5f);
              },
              [&](bool faulted) {
                  if (faulted) {
                      EXPECT(got == -1, "%s faulted and returned %d", fn, got);
                      EXPECT(lastErrorNames(fn), "%s: last error '%s'", fn, PvAmdLastError());
                  } else {
                      EXPECT(got == nextId, "%s returned id %d, expected %d (a faulted call changed the table)", fn, got, nextId);
                  }
              });
        ++nextId;
    }
    for (int id = 0; id < 30; ++id) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));  // (the worker swaps the change queue out: room is needed again)
        const char* fn = id % 3 == 0 ? "PlaneverbUpdateDiscGeometry" : id % 3 == 1 ? "PlaneverbUpdateWallPathGeometry" : "PlaneverbUpdateConcavePolygonGeometry";
        sweep(fn,
              [&] {
                  if (id % 3 == 0) PlaneverbUpdateDiscGeometry(id, 6.f, 6.f, 2.f, 0.25f);
                  if (id % 3 == 1) PlaneverbUpdateWallPathGeometry(id, path, 17, 0.4f, 0.25f);
                  if (id % 3 == 2) PlaneverbUpdateConcavePolygonGeometry(id, poly, 64, 0.25f);
              },
              [&](bool faulted) {
                  if (faulted) EXPECT(lastErrorNames(fn), "%s: last error '%s'", fn, PvAmdLastError());
              });
    }
    // Remove: a removed id is re-used exactly once, whichever kind's Remove took it
    const int victims[3] = {7, 11, 21};
    for (int k = 0; k < 3; ++k) {
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
        const char* fn = k == 0 ? "PlaneverbRemoveDiscGeometry" : k == 1 ? "PlaneverbRemoveWallPathGeometry" : "PlaneverbRemoveConcavePolygonGeometry";
        bool removed = false;
        sweep(fn,
              [&] {
                  if (k == 0) PlaneverbRemoveDiscGeometry(victims[k]);
                  if (k == 1) PlaneverbRemoveWallPathGeometry(victims[k]);
                  if (k == 2) PlaneverbRemoveConcavePolygonGeometry(victims[k]);
              },
              [&](bool faulted) {
                  if (faulted)
                      EXPECT(lastErrorNames(fn), "%s: last error '%s'", fn, PvAmdLastError());
                  else
                      removed = true;
              });
        EXPECT(removed, "%s never got through", fn);
        const int a = PlaneverbAddDiscGeometry(1.f, 1.f, 1.f, 0.5f), b = PlaneverbAddDiscGeometry(2.f, 2.f, 1.f, 0.5f);
        EXPECT(a == victims[k] && b == nextId, "after %s(%d): ids %d, %d (expected %d, %d)", fn, victims[k], a, b, victims[k], nextId);
        ++nextId;
    }
    // refused shapes allocate nothing and change nothing
    EXPECT(PlaneverbAddDiscGeometry(1.f, 1.f, 0.f, 0.5f) == -1, "a disc of radius 0 must be refused");
    EXPECT(PlaneverbAddWallPathGeometry(path, 1, 0.5f, 0.5f) == -1, "a path of one point must be refused");
    const float bow[8] = {0, 0, 2, 2, 2, 0, 0, 2};
    EXPECT(PlaneverbAddConcavePolygonGeometry(bow, 4, 0.5f) == -1, "a bow tie must be refused");
    const float nan = std::nanf(""), inf = HUGE_VALF;
    for (float bad : {nan, inf, -inf}) {
        EXPECT(PlaneverbAddDiscGeometry(3.f, 3.f, 1.f, bad) == -1, "a disc with absorption %f must be refused", bad);
        EXPECT(std::strstr(PvAmdLastError(), "non-finite absorption") != nullptr, "disc: last error '%s'", PvAmdLastError());
        EXPECT(PlaneverbAddWallPathGeometry(path, 5, 0.5f, bad) == -1, "a wall path with absorption %f must be refused", bad);
        EXPECT(std::strstr(PvAmdLastError(), "non-finite absorption") != nullptr, "path: last error '%s'", PvAmdLastError());
        EXPECT(PlaneverbAddConcavePolygonGeometry(poly, 64, bad) == -1, "a polygon with absorption %f must be refused", bad);
        EXPECT(std::strstr(PvAmdLastError(), "non-finite absorption") != nullptr, "polygon: last error '%s'", PvAmdLastError());
        PlaneverbUpdateDiscGeometry(0, 3.f, 3.f, 1.f, bad);  // (void: nothing is queued)
        PlaneverbUpdateWallPathGeometry(0, path, 5, 0.5f, bad);
        PlaneverbUpdateConcavePolygonGeometry(0, poly, 64, bad);
    }
    EXPECT(PlaneverbAddDiscGeometry(3.f, 3.f, nan, 0.5f) == -1 && PlaneverbAddDiscGeometry(nan, 3.f, 1.f, 0.5f) == -1,
           "a disc with a NaN radius or centre must be refused");
    EXPECT(PlaneverbAddDiscGeometry(3.f, 3.f, 1.f, 0.5f) == nextId, "a refused shape changed the id table");
    PlaneverbWaitIterations(PlaneverbIterationCount() + 2, 5000);
    EXPECT(PlaneverbIsRunning() == 1, "module stopped during the sweeps: %s", PlaneverbWorkerError());
    EXPECT(g_faults > 0, "no allocation was failed: the hook is not in the path");
    PlaneverbExit();
    EXPECT(pva::Solver::liveInstances().load() == 0, "Exit left %lld solver(s)", pva::Solver::liveInstances().load());
    std::printf("  %ld allocation(s) failed one at a time\n", g_faults);
    std::printf("alloc_fault_round: %d failure(s)\n", g_failures);
    return g_failures ? 1 : 0;
}
