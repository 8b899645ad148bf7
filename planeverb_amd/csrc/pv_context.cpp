// pv_context.cpp -- see pv_context.h
#include "pv_context.h"
#ifndef PVA_HOST_TEST
#include "pv_layer.h"
#endif

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>

namespace pva {

// ----------------------------------------------------------------------------------------------------------------
// lifetime: one published pointer, pinned by every API call for its duration
// ----------------------------------------------------------------------------------------------------------------

static std::atomic<Context*> g_context{nullptr};
static std::atomic<int> g_pinned{0};  // callers between Ref() and ~Ref() that hold a non-null context
static std::mutex g_lifeMutex;        // serialises Init / Exit

Context::Ref::Ref() {
    // Load, pin, re-check: once Exit has unpublished the pointer no new caller touches the counter, so the counter
    // only drains and Exit's wait ends.  A caller that loses the race between its two loads backs off without
    // having dereferenced anything.
    Context* c = g_context.load(std::memory_order_seq_cst);
    if (c) {
        g_pinned.fetch_add(1, std::memory_order_seq_cst);
        if (g_context.load(std::memory_order_seq_cst) != c) {
            g_pinned.fetch_sub(1, std::memory_order_seq_cst);
            c = nullptr;
        }
    }
    c_ = c;
}

Context::Ref::~Ref() {
    if (c_) g_pinned.fetch_sub(1, std::memory_order_seq_cst);
}

void retireContext(Context* c) {
    if (!c) return;
    // wake the callers that block INSIDE the context (WaitIterations) and let the worker finish its iteration, so that
    // the pins drain at once instead of after the callers' own timeouts.  The wake-up is repeated while pins remain: a
    // waiter that tested its predicate just before retiring_ was set and blocks just after the first notify is caught by
    // the next one (no mutex is taken here, so nothing of the context is held when it is deleted).
    c->beginRetire();
    while (g_pinned.load(std::memory_order_seq_cst) != 0) {  // callers still inside
        c->iterCv_.notify_all();
        std::this_thread::yield();
    }
    delete c;
}

void Context::beginRetire() {
    running_.store(false);
    retiring_.store(true, std::memory_order_seq_cst);
    iterCv_.notify_all();
}

uint64_t Context::packXZ(float x, float z) {
    uint32_t a, b;
    std::memcpy(&a, &x, 4);
    std::memcpy(&b, &z, 4);
    return ((uint64_t)a << 32) | b;
}
void Context::unpackXZ(uint64_t v, float* x, float* z) {
    const uint32_t a = (uint32_t)(v >> 32), b = (uint32_t)v;
    std::memcpy(x, &a, 4);
    std::memcpy(z, &b, 4);
}

bool Context::init(const LiveConfig& cfg, std::string* err) {
    std::lock_guard<std::mutex> lock(g_lifeMutex);
    // Init while running = Exit + Init, PvContext.cpp:27-31
    retireContext(g_context.exchange(nullptr, std::memory_order_seq_cst));
    // PvContext.cpp:101-107
    if (cfg.res < kLowResolution || cfg.sizeX == 0.f || cfg.sizeY == 0.f || cfg.tempDir == nullptr ||
        cfg.maxThreads < 0) {
        if (err) *err = "invalid config (pv_InvalidConfig)";
        return false;
    }
    int device = 0;
    if (const char* e = std::getenv("PLANEVERB_AMD_DEVICE")) device = std::atoi(e);
    GridSpec spec = makeGridSpec(cfg.sizeX, cfg.sizeY, cfg.res);
    if (spec.gx != spec.gy)
        std::fprintf(stderr, "[planeverb_amd] warning: %d x %d grid -- the reference indexes non-square grids "
                             "inconsistently (SURVEY.md Q1); results there are defined by this library (cell array "
                             "stride gy+1 throughout), not by the reference\n", spec.gx, spec.gy);
    // Planeverb::Init takes any resolution >= 275 (PvContext.cpp:101-107).  Where the T-step pressure history does not fit
    // the device (25 m at 16 kHz: T = 25 432 on a 4096^2 grid) the solver falls back to the sparse-emitter mode by itself;
    // PLANEVERB_AMD_LIVE_STREAMING=1 forces that mode (tests, memory-tight hosts).
    SolverOptions opt;
    opt.autoStreaming = true;
    if (const char* e = std::getenv("PLANEVERB_AMD_LIVE_STREAMING")) opt.streaming = std::atoi(e) != 0;
    // (owned until it is published: an exception from underneath -- a table or the worker thread that cannot be created --
    // unwinds through ~Context, which stops the worker and releases the solvers, and ends at the C-ABI's barrier, pv_capi.cpp)
    struct Owner {
        Context* c;
        ~Owner() { delete c; }
    } own{new Context()};
    Context* const c = own.c;
    static std::atomic<unsigned long long> generations{0};
    c->generation_ = generations.fetch_add(1) + 1;
    c->solver_ = Solver::create(spec, device, opt, err);
    if (!c->solver_) return false;
    c->streaming_ = c->solver_->options().streaming;
    c->lastSolver_ = c->solver_;
    // Two iterations in flight where an iteration leaves most of the chip idle: the grids the resident kernel serves (the
    // reference's presets).  PLANEVERB_AMD_LIVE_PIPELINE=1 / 2 forces one / two.
    int pipeline = (!c->streaming_ && c->solver_->residentKernel()) ? 2 : 1;
    if (const char* e = std::getenv("PLANEVERB_AMD_LIVE_PIPELINE")) pipeline = std::atoi(e) >= 2 && !c->streaming_ ? 2 : 1;
    if (pipeline == 2) {
        c->solver2_ = Solver::create(spec, device, opt, err);
        if (!c->solver2_) return false;
    }
#ifndef PVA_HOST_TEST  // (the HIP-less fake has no grid edges)
    // gridBoundaryType (PvTypes.h:32-36): 1 = pv_ReflectingBoundary, R = 1 on every side of both solvers.  The reference stores
    // the value and ignores it; any value but 0 and 1 keeps absorbing edges, as before, and says so.
    if (cfg.boundaryType == 1) {
        const float rigid[4] = {1.f, 1.f, 1.f, 1.f};
        if (!c->solver_->setGridBoundary(rigid) || (c->solver2_ && !c->solver2_->setGridBoundary(rigid))) {
            if (err) *err = "grid boundary: " + c->solver_->lastError();
            return false;
        }
    } else if (cfg.boundaryType != 0) {
        std::fprintf(stderr, "[planeverb_amd] warning: gridBoundaryType %d is neither pv_AbsorbingBoundary (0) nor "
                             "pv_ReflectingBoundary (1): absorbing grid edges\n", cfg.boundaryType);
    }
#endif
    if (c->streaming_)
        std::fprintf(stderr, "[planeverb_amd] %d x %d grid, T = %d: sparse-emitter mode (wet gain / RT60 for the cells of the "
                             "emitters registered at the start of an iteration)\n", spec.gx, spec.gy, c->solver_->T());
    const size_t bytes = c->solver_->windowCapacity() * 32;
    for (Slot& s : c->slots_) {
        s.data = static_cast<float*>(Solver::hostAlloc(bytes));
        if (!s.data) {
            if (err) *err = "pinned host allocation failed for the published result block";
            return false;
        }
    }
    c->running_.store(true);
    c->worker_ = std::thread(&Context::workerMain, c);  // PvContext.cpp:160
    own.c = nullptr;
    g_context.store(c, std::memory_order_seq_cst);
    return true;
}

void Context::exit() {
    std::lock_guard<std::mutex> lock(g_lifeMutex);
    retireContext(g_context.exchange(nullptr, std::memory_order_seq_cst));
}

Context::~Context() {
    running_.store(false);  // PvContext.cpp:166-167
    if (worker_.joinable()) worker_.join();
    delete solver2_;
    delete solver_;
    for (Slot& s : slots_) Solver::hostFree(s.data);
    std::free(base_.load());
    for (RecSlot& r : rec_) {
        std::free(r.cells.load());
        std::free(r.data.load());
    }
    for (auto& c : chunks_) {
        Emitter* p = c.load();
        delete[] p;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// worker: PvContext.cpp:63-94
// ----------------------------------------------------------------------------------------------------------------

// sparse-emitter mode: the emitters alive now are the cells whose wet gain / RT60 this iteration computes
// (EmissionManager.cpp:37-54 keeps the same table; ended ids are skipped)
bool Context::registerEmitters() {
    std::vector<float> xyz;
    {
        std::lock_guard<std::mutex> lock(emitMutex_);
        const int n = emitterCount_.load(std::memory_order_acquire);
        std::vector<uint8_t> ended((size_t)n, 0);
        for (int id : emitterFree_)
            if (id >= 0 && id < n) ended[(size_t)id] = 1;
        for (int id = 0; id < n; ++id) {
            if (ended[(size_t)id]) continue;
            Emitter* e = emitterAt(id);
            if (!e) continue;
            xyz.push_back(e->x.load());
            xyz.push_back(e->y.load());
            xyz.push_back(e->z.load());
        }
    }
    return solver_->setEmitters(xyz.data(), (int)(xyz.size() / 3));
}

// The thread's entry: no exception leaves the worker (std::terminate would take the host process -- the game -- with it).
// One that reaches this point stops the worker like a solver error does: IsRunning reports 0, PvAmdLastError /
// PlaneverbWorkerError carry the reason, GetOutput keeps serving the last published iteration.
void Context::workerMain() {
    try {
        if (solver2_)
            workerLoopPipelined();
        else
            workerLoop();
        return;
    } catch (const std::exception& e) {
        try {
            std::lock_guard<std::mutex> lock(errMutex_);
            workerErr_ = std::string("exception in the simulation worker: ") + e.what();
        } catch (...) {
        }
    } catch (...) {
        try {
            std::lock_guard<std::mutex> lock(errMutex_);
            workerErr_ = "unknown exception in the simulation worker";
        } catch (...) {
        }
    }
    std::fprintf(stderr, "[planeverb_amd] simulation worker stopped on an exception\n");
    failed_.store(true, std::memory_order_release);
    running_.store(false);
    iterCv_.notify_all();
}

void Context::workerLoop() {
    float lx, lz, ly = ly_.load();
    unpackXZ(lxz_.load(), &lx, &lz);
    std::unique_lock<std::mutex> solverLock(solverMutex_);
    auto stop = [&]() {
        finishPublish();  // (the last COMPLETED iteration's block may still be on its way: it is valid, make it visible)
        // The worker stops; the host can see it: IsRunning reports 0, PvAmdLastError carries the reason, GetOutput keeps
        // serving the last published iteration.
        std::string e = solver_->lastError();
        std::fprintf(stderr, "[planeverb_amd] simulation worker stopped: %s\n", e.c_str());
        {
            std::lock_guard<std::mutex> lock(errMutex_);
            workerErr_ = std::move(e);
        }
        failed_.store(true, std::memory_order_release);
        running_.store(false);
    };
    while (running_.load(std::memory_order_acquire)) {
        // Iteration i: enqueue FDTD + analysis; make iteration i - 1 visible (its result block has been travelling to the
        // host on the copy stream since it was packed); queue this iteration's block behind its analysis; wait for the
        // DEVICE work of iteration i -- not for its copy, which overlaps the next iteration's first launches.
        // (sparse-emitter mode: enqueueing a run BLOCKS for the front phase of the run -- the host paces the fused forward sums
        // -- so the previous iteration is made visible first instead of ~100 ms late)
        // (emission records: the table is latched in front of the run -- the solver's previous run has been waited for -- and the
        // records leave the solver's pinned block behind sync(), before the next run overwrites it)
        if (!((!streaming_ || (finishPublish() && registerEmitters())) && latchRecords(0) && solver_->run(lx, ly, lz, /*wait=*/false) &&
              finishPublish() && beginPublish() && solver_->sync() && collectRecords(0, pendBack_))) {
            stop();
            break;
        }
        pushGeometryChanges();            // PvContext.cpp:86: after the iteration's analysis
        unpackXZ(lxz_.load(), &lx, &lz);  // PvContext.cpp:89
        ly = ly_.load();
        if (solverWaiters_.load(std::memory_order_acquire) > 0) {  // a GetImpulseResponse call wants the solver
            // (it reads the iteration just completed: publish it first, so that "the last completed iteration" and the
            // published outputs agree)
            if (!finishPublish()) {
                stop();
                break;
            }
            solverLock.unlock();
            while (solverWaiters_.load(std::memory_order_acquire) > 0) std::this_thread::yield();
            solverLock.lock();
        }
    }
    if (!failed_.load()) finishPublish();  // the last iteration's block
    solverLock.unlock();
    iterCv_.notify_all();
}

void Context::workerLoopPipelined() {
    float lx, lz, ly = ly_.load();
    unpackXZ(lxz_.load(), &lx, &lz);
    std::unique_lock<std::mutex> solverLock(solverMutex_);
    Solver* const sv[2] = {solver_, solver2_};
    struct Flight {
        int k, slot;
        Solver::WindowBlock win;
    };
    std::deque<Flight> flights;
    auto fail = [&](Solver* s) {
        std::string e = s->lastError();
        std::fprintf(stderr, "[planeverb_amd] simulation worker stopped: %s\n", e.c_str());
        {
            std::lock_guard<std::mutex> lock(errMutex_);
            workerErr_ = std::move(e);
        }
        failed_.store(true, std::memory_order_release);
        running_.store(false);
    };
    // the oldest iteration in flight: wait for its device work and its block's copy, make it visible
    auto complete = [&]() -> bool {
        const Flight f = flights.front();
        flights.pop_front();
        if (!(sv[f.k]->sync() && sv[f.k]->waitPublish() && collectRecords(f.k, f.slot))) {
            fail(sv[f.k]);
            return false;
        }
        publishSlot(f.slot, f.win);
        lastSolver_ = sv[f.k];
        pushGeometryChanges();            // PvContext.cpp:86: after an iteration's analysis
        unpackXZ(lxz_.load(), &lx, &lz);  // PvContext.cpp:89
        ly = ly_.load();
        return true;
    };
    long long started = 0;
    int prevK = -1;
    bool ok = true;
    while (ok && running_.load(std::memory_order_acquire)) {
        const int k = (int)(started & 1);
        while (ok && !flights.empty() && (flights.size() >= 2 || flights.front().k == k)) ok = complete();
        if (!ok) break;
        applyPending(k);
        // a slot that is neither readable nor the target of an iteration in flight
        int slot = 0;
        for (; slot < 3; ++slot) {
            bool used = slot == front_.load(std::memory_order_relaxed);
            for (const Flight& f : flights) used = used || f.slot == slot;
            if (!used) break;
        }
        Flight f{k, slot, {}};
        rec_[slot].pendKinds = 0;  // (until collectRecords has seen the iteration through)
        if (!(latchRecords(k) && sv[k]->run(lx, ly, lz, /*wait=*/false, prevK >= 0 ? sv[prevK] : nullptr) &&
              sv[k]->publishWindowAsync(slots_[slot].data, &f.win, false))) {
            // (the iteration still in flight on the other solver is valid: make it visible first, as the one-solver loop does)
            while (!flights.empty() && complete()) {
            }
            if (!failed_.load()) fail(sv[k]);
            break;
        }
        flights.push_back(f);
        prevK = k;
        // (the first iteration runs alone: the reference pushes the geometry its caller added after Init behind it,
        // PvContext.cpp:80-86)
        if (started++ == 0) ok = complete();
        if (ok && solverWaiters_.load(std::memory_order_acquire) > 0) {  // a GetImpulseResponse call wants the solvers
            while (ok && !flights.empty()) ok = complete();
            if (!ok) break;
            solverLock.unlock();
            while (solverWaiters_.load(std::memory_order_acquire) > 0) std::this_thread::yield();
            solverLock.lock();
        }
    }
    while (!failed_.load() && !flights.empty() && complete()) {
    }
    solverLock.unlock();
    iterCv_.notify_all();
}

std::string Context::workerError() {
    std::lock_guard<std::mutex> lock(errMutex_);
    return workerErr_;
}

long long Context::waitIterations(long long count, int timeoutMs) {
    std::unique_lock<std::mutex> lock(iterMutex_);
    // (system_clock: pthread_cond_timedwait, which ThreadSanitizer models; wait_for's pthread_cond_clockwait it does not)
    iterCv_.wait_until(lock, std::chrono::system_clock::now() + std::chrono::milliseconds(timeoutMs),
                     [&] { return iterations_.load() >= count || !running_.load() || retiring_.load(); });
    return iterations_.load();
}

void Context::setListener(float x, float y, float z) {
    lxz_.store(packXZ(x, z));
    ly_.store(y);
}

// ----------------------------------------------------------------------------------------------------------------
// publish / read
// ----------------------------------------------------------------------------------------------------------------

namespace {
// 32-bit relaxed atomic accesses: readers may overlap a writer (they then discard what they read, see pubSeq_)
inline void storeRelaxed(float* dst, const float* src, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t v;
        std::memcpy(&v, src + i, 4);
        __atomic_store_n(reinterpret_cast<uint32_t*>(dst) + i, v, __ATOMIC_RELAXED);
    }
}
inline void loadRelaxed(float* dst, const float* src, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const uint32_t v = __atomic_load_n(reinterpret_cast<const uint32_t*>(src) + i, __ATOMIC_RELAXED);
        std::memcpy(dst + i, &v, 4);
    }
}
}  // namespace

// Copy the block the finished iteration can have changed into the back slot, keep what leaves the window, flip.
// Two halves, so that the device -> host copy of iteration i overlaps iteration i + 1's first launches: beginPublish is
// enqueued right behind iteration i's analysis (pack on the solver's stream, copy on a second stream into the BACK slot);
// finishPublish -- called once iteration i + 1 has been enqueued -- waits for that copy alone, does the host bookkeeping and
// flips the slots.  Readers only ever see the front slot, which no copy is writing.
bool Context::beginPublish() {
    const int f = front_.load(std::memory_order_relaxed);
    pendBack_ = f < 0 ? 0 : f ^ 1;
    // (small blocks -- the Sandbox's 157 kB -- ride on the solver's own stream: the cross-stream hand-over costs more than
    // their copy, measured 0.77 against 0.71 ms per iteration at 71^2)
    const bool overlap = solver_->windowCapacity() * 32 > (size_t)(1u << 20);
    if (!solver_->publishWindowAsync(slots_[pendBack_].data, &pendWin_, overlap)) return false;
    rec_[pendBack_].pendKinds = 0;  // (until collectRecords has seen the iteration through)
    pendPublish_ = true;
    return true;
}

bool Context::finishPublish() {
    if (!pendPublish_) return true;
    pendPublish_ = false;
    if (!solver_->waitPublish()) return false;
    publishSlot(pendBack_, pendWin_);
    return true;
}

// host part of a publish: the block has landed in slots_[back]
void Context::publishSlot(const int back, const Solver::WindowBlock& w) {
    const int f = front_.load(std::memory_order_relaxed);
    if (f >= 0) {
        // Cells of the old block outside the new one keep the old block's values from now on (the reference leaves
        // m_results untouched where an iteration finds no onset, Analyzer.cpp:160-165).  Nobody can be reading these
        // cells from base_ now: a reader that started after the last publish takes them from the front slot, and one
        // that started before it repeats.
        const Slot& o = slots_[f];
        const int or0 = o.r0.load(std::memory_order_relaxed), oc0 = o.c0.load(std::memory_order_relaxed);
        const int onr = o.nr.load(std::memory_order_relaxed), onc = o.nc.load(std::memory_order_relaxed);
        const bool same = or0 == w.r0 && oc0 == w.c0 && onr == w.nr && onc == w.nc;
        if (!same && onr > 0 && onc > 0) {
            const int gy = solver_->spec().gy;
            float* b = base_.load(std::memory_order_relaxed);
            if (!b) {
                b = static_cast<float*>(std::calloc((size_t)solver_->spec().gx * gy, 32));
                if (!b) std::abort();  // (a map of 32 bytes per cell on the host)
                base_.store(b, std::memory_order_release);
            }
            for (int r = or0; r < or0 + onr; ++r) {
                const bool rowInside = r >= w.r0 && r < w.r0 + w.nr;
                for (int c = oc0; c < oc0 + onc;) {
                    if (rowInside && c >= w.c0 && c < w.c0 + w.nc) {
                        c = w.c0 + w.nc;  // the part of the row the new block covers
                        continue;
                    }
                    const int end = (rowInside && c < w.c0) ? std::min(oc0 + onc, w.c0) : oc0 + onc;
                    storeRelaxed(b + ((size_t)r * gy + c) * 8, o.data + ((size_t)(r - or0) * onc + (c - oc0)) * 8,
                                 (size_t)(end - c) * 8);
                    c = end;
                }
            }
        }
    }
    pubSeq_.fetch_add(1, std::memory_order_seq_cst);  // odd: publish in progress
    Slot& s = slots_[back];
    s.r0.store(w.r0, std::memory_order_relaxed);
    s.c0.store(w.c0, std::memory_order_relaxed);
    s.nr.store(w.nr, std::memory_order_relaxed);
    s.nc.store(w.nc, std::memory_order_relaxed);
    s.lx.store(w.lx, std::memory_order_relaxed);
    s.lz.store(w.lz, std::memory_order_relaxed);
    // the iteration's emission records (collectRecords left them in the slot): readable from the same flip on
    RecSlot& r = rec_[back];
    r.kinds.store(r.pendKinds, std::memory_order_relaxed);
    r.n.store(r.pendKinds ? r.pendN : 0, std::memory_order_relaxed);
    for (int k = 0; k < kQueryRecordKinds; ++k) {
        r.floats[k].store(r.pendFloats[k], std::memory_order_relaxed);
        r.offset[k].store(r.pendOffset[k], std::memory_order_relaxed);
    }
    front_.store(back, std::memory_order_relaxed);
    pubSeq_.fetch_add(1, std::memory_order_seq_cst);  // even
    {
        std::lock_guard<std::mutex> lock(iterMutex_);
        iterations_.fetch_add(1, std::memory_order_acq_rel);
    }
    iterCv_.notify_all();
}

Out8 Context::outputAt(int cx, int cy) {
    const GridSpec& g = solver_->spec();
    for (;;) {
        const uint64_t s1 = pubSeq_.load(std::memory_order_acquire);
        if (s1 & 1) continue;  // the worker is between its two stores
        Out8 o;
        std::memset(&o, 0, sizeof(o));  // nothing published yet: the zeroed pool of a fresh context, PvContext.cpp:132
        const int f = front_.load(std::memory_order_relaxed);
        if (f >= 0) {
            const Slot& s = slots_[f];
            const int r0 = s.r0.load(std::memory_order_relaxed), c0 = s.c0.load(std::memory_order_relaxed);
            const int nr = s.nr.load(std::memory_order_relaxed), nc = s.nc.load(std::memory_order_relaxed);
            if (cx >= r0 && cx < r0 + nr && cy >= c0 && cy < c0 + nc) {
                loadRelaxed(o.v, s.data + ((size_t)(cx - r0) * nc + (cy - c0)) * 8, 8);
            } else {
                if (const float* b = base_.load(std::memory_order_acquire))
                    loadRelaxed(o.v, b + ((size_t)cx * g.gy + cy) * 8, 8);
                // no neighbour of a cell out here has an onset, so the listener-direction walk stays put
                // (Analyzer.cpp:365-391) and the direction is the normalised (cellPos - listener), :415-428
                float ox = (float)cx * g.dx - s.lx.load(std::memory_order_relaxed);
                float oy = (float)cy * g.dx - s.lz.load(std::memory_order_relaxed);
                float len = (ox * ox) + (oy * oy);
                if (len != 0.f) {
                    len = std::sqrt(len);
                    ox /= len;
                    oy /= len;
                }
                o.v[4] = ox;
                o.v[5] = oy;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (pubSeq_.load(std::memory_order_relaxed) == s1) return o;
    }
}

// ----------------------------------------------------------------------------------------------------------------
// emissions
// ----------------------------------------------------------------------------------------------------------------

Context::Emitter* Context::emitterAt(int id) {
    if (id < 0 || id >= emitterCount_.load(std::memory_order_acquire)) return nullptr;
    Emitter* c = chunks_[id / kChunk].load(std::memory_order_acquire);
    return c ? &c[id % kChunk] : nullptr;
}

int Context::emit(float x, float y, float z) {
    std::lock_guard<std::mutex> lock(emitMutex_);
    int id;
    if (!emitterFree_.empty()) {  // EmissionManager.cpp:40-46
        id = emitterFree_.back();
        emitterFree_.pop_back();
    } else {  // EmissionManager.cpp:48-53
        id = emitterCount_.load();
        if (id >= kChunk * kMaxChunks) return -1;
        if (!chunks_[id / kChunk].load()) chunks_[id / kChunk].store(new Emitter[kChunk], std::memory_order_release);
    }
    Emitter* e = &chunks_[id / kChunk].load()[id % kChunk];
    e->x.store(x);
    e->y.store(y);
    e->z.store(z);
    e->live.store(1, std::memory_order_release);
    if (id == emitterCount_.load()) emitterCount_.store(id + 1, std::memory_order_release);
    return id;
}

void Context::updateEmission(int id, float x, float y, float z) {
    if (Emitter* e = emitterAt(id)) {  // EmissionManager.cpp:56-61
        e->x.store(x);
        e->y.store(y);
        e->z.store(z);
    }
}

void Context::endEmission(int id) {
    // EmissionManager.cpp:63-67 pushes any id unchecked (an out-of-range id later corrupts memory there);
    // ids that were never handed out are ignored here, a double end is kept (the id is then handed out twice).
    if (id < 0 || id >= emitterCount_.load()) return;
    std::lock_guard<std::mutex> lock(emitMutex_);
    emitterFree_.push_back(id);
    if (Emitter* e = emitterAt(id)) e->live.store(0, std::memory_order_release);
}

Out8 Context::getOutput(int id) {
    Out8 o;
    std::memset(&o, 0, sizeof(o));
    Emitter* e = emitterAt(id);
    if (!e) {  // FDTD.cpp:34-38
        o.v[0] = kInvalidDryGain;
        return o;
    }
    int cx, cy;
    if (!resultCell(solver_->spec(), e->x.load(), e->z.load(), &cx, &cy)) {  // FDTD.cpp:43-47
        o.v[0] = kInvalidDryGain;
        return o;
    }
    return outputAt(cx, cy);
}

// FDTD.cpp:60-79: cell = ((int)(x / dx), (int)(z / dx)) of the (gx+1) x (gy+1) array
int Context::impulseResponse(float x, float y, float z, void* cells16, int cap) {
    (void)y;
    const GridSpec& g = solver_->spec();
    const int cx = (int)(x / g.dx), cy = (int)(z / g.dx);
    if (cx < 0 || cx > g.gx || cy < 0 || cy > g.gy) return 0;  // (the reference indexes past its array here)
    solverWaiters_.fetch_add(1, std::memory_order_acq_rel);
    std::unique_lock<std::mutex> lock(solverMutex_);
    solverWaiters_.fetch_sub(1, std::memory_order_acq_rel);
    const int T = solver_->T();
    std::vector<char> buf((size_t)T * 16);
    if (!lastSolver_->impulseResponseCells(cx, cy, buf.data())) return -1;
    lock.unlock();
    if (cells16 && cap > 0) std::memcpy(cells16, buf.data(), (size_t)std::min(cap, T) * 16);
    return T;
}

// ----------------------------------------------------------------------------------------------------------------
// geometry
// ----------------------------------------------------------------------------------------------------------------

namespace {
// Room for k more elements BEFORE a table operation commits anything: the only step that can throw (std::bad_alloc) then
// happens while the tables are still what they were, and the push_backs behind it cannot fail (geometric growth kept).
template <class V>
void ensureRoom(V& v, size_t k) {
    if (v.capacity() - v.size() < k) v.reserve(std::max(v.capacity() * 2, v.size() + k));
}
}  // namespace

// ----------------------------------------------------------------------------------------------------------------
// emission records (pv_context.h): settings, the worker's latch and collect steps, the lock-free read
// ----------------------------------------------------------------------------------------------------------------

#if !defined(PVA_HOST_TEST) || defined(PVA_HOST_TEST_RECORDS)
#define PVA_LIVE_RECORDS 1
#endif

namespace {
const char kRecPrefix[] = "emission records: ";
inline long long loadCell(const long long* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
}  // namespace

bool Context::setEmissionRecords(unsigned kinds, std::string* err) {
#ifdef PVA_LIVE_RECORDS
    const int fs = (int)spec().fs;
    std::lock_guard<std::mutex> lock(geomMutex_);
    const char* why = nullptr;
    LobeEdges ed;
    if (kinds & ~kQueryRecordMask)
        why = "unknown kind bit (PVA_QREC_*)";
    else if (kinds && streaming_)
        why = "the full pressure history is not kept in sparse-emitter mode";
    else if ((kinds & (1u << kQrecEchogram)) && !wantSlots_)
        why = "echogram: no slots set (PlaneverbSetEmissionEchogram)";
    else if ((kinds & (1u << kQrecEchoCriterion)) && !echoFsOk(fs))
        why = "echo: the sampling rate gives a speech lag below one step ((int)(0.009f * (float)fs) < 1)";
    else if ((kinds & (1u << kQrecLobes)) &&
             !lobesEdgeSteps(wantEdges_ ? wantEdge_ : kLobesDefaultEdges, wantEdges_ ? wantEdges_ : 2, fs, &ed))
        why = "lobes: the default windows (10 ms, 80 ms) need a sampling rate of 100 Hz or more (PlaneverbSetEmissionLobeWindows)";
    if (why) {
        *err = std::string(kRecPrefix) + why;
        return false;
    }
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.rec = 1;
    c.recKinds = kinds;
    changes_.push_back(c);
    wantKinds_ = kinds;
    return true;
#else
    (void)kinds;
    *err = std::string(kRecPrefix) + "not in this build";
    return false;
#endif
}

bool Context::setEmissionEchogram(float slotSeconds, int nSlots, std::string* err) {
#ifdef PVA_LIVE_RECORDS
    std::lock_guard<std::mutex> lock(geomMutex_);
    const char* why = nullptr;
    if (streaming_)
        why = "the full pressure history is not kept in sparse-emitter mode";
    else if (nSlots < 0 || nSlots > kEchogramMaxSlots)
        why = "echogram: nSlots is 0 .. PVA_ECHOGRAM_MAX_SLOTS (32)";
    else if (nSlots > 0 && !echogramSlotOk(slotSeconds, (int)spec().fs))
        why = "echogram: slotSeconds must be finite and give 1 .. 2^20 steps per slot ((int)(slotSeconds * (float)fs))";
    else if (nSlots == 0 && (wantKinds_ & (1u << kQrecEchogram)))
        why = "echogram: the slots cannot be cleared while PVA_QREC_ECHOGRAM is selected (PlaneverbSetEmissionRecords)";
    if (why) {
        *err = std::string(kRecPrefix) + why;
        return false;
    }
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.rec = 2;
    c.recSeconds = slotSeconds;
    c.recN = nSlots;
    changes_.push_back(c);
    wantSlots_ = nSlots;
    return true;
#else
    (void)slotSeconds;
    (void)nSlots;
    *err = std::string(kRecPrefix) + "not in this build";
    return false;
#endif
}

bool Context::setEmissionLobeWindows(const float* edgesSeconds, int nEdges, std::string* err) {
#ifdef PVA_LIVE_RECORDS
    const int fs = (int)spec().fs;
    std::lock_guard<std::mutex> lock(geomMutex_);
    std::string why;
    LobeEdges ed;
    if (streaming_)
        why = "the full pressure history is not kept in sparse-emitter mode";
    else if (nEdges != 0 && !lobesEdgeSteps(edgesSeconds, nEdges, fs, &ed))
        why = kLobesEdgesError;
    else if (nEdges == 0 && (wantKinds_ & (1u << kQrecLobes)) && !lobesEdgeSteps(kLobesDefaultEdges, 2, fs, &ed))
        why = "lobes: the default windows (10 ms, 80 ms) need a sampling rate of 100 Hz or more";
    if (!why.empty()) {
        *err = kRecPrefix + why;
        return false;
    }
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.rec = 3;
    c.recN = nEdges;
    for (int i = 0; i < nEdges; ++i) c.recEdges[i] = wantEdge_[i] = edgesSeconds[i];
    changes_.push_back(c);
    wantEdges_ = nEdges;
    return true;
#else
    (void)edgesSeconds;
    (void)nEdges;
    *err = std::string(kRecPrefix) + "not in this build";
    return false;
#endif
}

// Start of an iteration on solver k: the cells of the live emitters, in ascending id as registerEmitters walks them, the first
// kMaxRecordQueries distinct in-map ones, sorted, as that solver's record queries.  Nothing when no kind is selected.
bool Context::latchRecords(const int k) {
    Latch& L = latch_[k];
    L.kinds = 0;
    L.cells.clear();
#ifdef PVA_LIVE_RECORDS
    Solver* const s = k == 0 ? solver_ : solver2_;
    L.kinds = s->queryRecordKinds();
    if (!L.kinds) return true;
    const GridSpec& g = s->spec();
    auto& seen = latchScratch_;  // (cell, order of first appearance)
    seen.clear();
    {
        std::lock_guard<std::mutex> lock(emitMutex_);
        const int n = emitterCount_.load(std::memory_order_acquire);
        for (int id = 0; id < n; ++id) {
            Emitter* e = emitterAt(id);
            if (!e || !e->live.load(std::memory_order_acquire)) continue;  // (ended)
            int cx, cy;
            if (resultCell(g, e->x.load(), e->z.load(), &cx, &cy)) seen.emplace_back((long long)cx * g.gy + cy, (int)seen.size());
        }
    }
    // distinct cells, each with its first appearance; then the first kMaxRecordQueries of them by appearance; then by cell
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end(), [](const auto& a, const auto& b) { return a.first == b.first; }), seen.end());
    if (seen.size() > (size_t)kMaxRecordQueries) {
        std::nth_element(seen.begin(), seen.begin() + kMaxRecordQueries, seen.end(),
                         [](const auto& a, const auto& b) { return a.second < b.second; });
        seen.resize((size_t)kMaxRecordQueries);
        std::sort(seen.begin(), seen.end());
    }
    // the solver takes positions: the cell centres ((c + 0.5) dx divided by dx lands within 2^-22 c of c + 0.5: the same cell)
    latchXyz_.clear();
    for (const auto& c : seen) {
        L.cells.push_back(c.first);
        latchXyz_.push_back((float)(((double)(c.first / g.gy) + 0.5) * (double)g.dx));
        latchXyz_.push_back(0.f);
        latchXyz_.push_back((float)(((double)(c.first % g.gy) + 0.5) * (double)g.dx));
    }
    return s->setRecordQueries(latchXyz_.data(), (int)L.cells.size());
#else
    return true;
#endif
}

// Solver k's run has been waited for: its records leave the pinned block for record slot `slot` (not the readable one; relaxed
// stores, because a late reader may still be looking at it -- it then discards what it read), to be made visible by publishSlot
bool Context::collectRecords(const int k, const int slot) {
    RecSlot& r = rec_[slot];
    r.pendKinds = 0;
    r.pendN = 0;
#ifdef PVA_LIVE_RECORDS
    const Latch& L = latch_[k];
    if (!L.kinds) return true;
    Solver* const s = k == 0 ? solver_ : solver2_;
    long long* cells = r.cells.load(std::memory_order_relaxed);
    float* data = r.data.load(std::memory_order_relaxed);
    if (!cells) {
        cells = static_cast<long long*>(std::calloc((size_t)kMaxRecordQueries, sizeof(long long)));
        data = static_cast<float*>(std::calloc(kRecSlotFloats, sizeof(float)));
        if (!cells || !data) {
            std::free(cells);
            std::free(data);
            throw std::bad_alloc();  // (ends at the worker's barrier)
        }
        r.cells.store(cells, std::memory_order_release);
        r.data.store(data, std::memory_order_release);
    }
    const int n = (int)L.cells.size();
    int off = 0;
    for (int b = 0; b < kQueryRecordKinds; ++b) {
        r.pendFloats[b] = 0;
        r.pendOffset[b] = off;
        if (!((L.kinds >> b) & 1u)) continue;
        const int f = s->queryRecordFloats(1u << b);
        if (f < 0) return false;
        r.pendFloats[b] = f;
        if (n > 0) {
            recStage_.resize((size_t)n * f);
            if (!s->queriedRecords(1u << b, recStage_.data(), n)) return false;
            storeRelaxed(data + off, recStage_.data(), (size_t)n * f);
        }
        off += n * f;
    }
    for (int i = 0; i < n; ++i) __atomic_store_n(cells + i, L.cells[(size_t)i], __ATOMIC_RELAXED);
    r.pendKinds = L.kinds;
    r.pendN = n;
#else
    (void)k;
#endif
    return true;
}

unsigned Context::emissionRecordKinds() {
    for (;;) {
        const uint64_t s1 = pubSeq_.load(std::memory_order_acquire);
        if (s1 & 1) continue;
        const int f = front_.load(std::memory_order_relaxed);
        const unsigned kinds = f >= 0 ? rec_[f].kinds.load(std::memory_order_relaxed) : 0u;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (pubSeq_.load(std::memory_order_relaxed) == s1) return kinds;
    }
}

int Context::emissionRecordFloats(unsigned kind) {
    const int b = oneKindBit(kind, kQueryRecordKinds);
    if (b < 0) return -1;
    for (;;) {
        const uint64_t s1 = pubSeq_.load(std::memory_order_acquire);
        if (s1 & 1) continue;
        const int f = front_.load(std::memory_order_relaxed);
        int n = -1;
        if (f >= 0 && (rec_[f].kinds.load(std::memory_order_relaxed) & kind)) n = rec_[f].floats[b].load(std::memory_order_relaxed);
        std::atomic_thread_fence(std::memory_order_acquire);
        if (pubSeq_.load(std::memory_order_relaxed) == s1) return n;
    }
}

int Context::emissionRecordCells() {
    for (;;) {
        const uint64_t s1 = pubSeq_.load(std::memory_order_acquire);
        if (s1 & 1) continue;
        const int f = front_.load(std::memory_order_relaxed);
        const int n = f >= 0 ? rec_[f].n.load(std::memory_order_relaxed) : 0;
        std::atomic_thread_fence(std::memory_order_acquire);
        if (pubSeq_.load(std::memory_order_relaxed) == s1) return n;
    }
}

int Context::emissionRecord(int id, unsigned kind, float* out, int cap) {
    const int b = oneKindBit(kind, kQueryRecordKinds);
    if (b < 0 || !out) return -1;
    const GridSpec& g = solver_->spec();
    float rec[kRecMaxFloats];
    for (;;) {
        const uint64_t s1 = pubSeq_.load(std::memory_order_acquire);
        if (s1 & 1) continue;  // the worker is between its two stores
        int res = -1, nf = 0;
        const int f = front_.load(std::memory_order_relaxed);
        if (f >= 0 && (rec_[f].kinds.load(std::memory_order_relaxed) & kind)) {
            const RecSlot& r = rec_[f];
            nf = r.floats[b].load(std::memory_order_relaxed);
            if (nf < 1 || nf > kRecMaxFloats) {
                nf = 0;  // (a torn read: the check below repeats it)
            } else if (cap >= nf) {
                res = 0;
                // the emitter's position NOW: a cell it moved to since the latch is not in the table (one iteration later it is)
                Emitter* e = emitterAt(id);
                int cx, cy;
                if (e && e->live.load(std::memory_order_acquire) && resultCell(g, e->x.load(), e->z.load(), &cx, &cy)) {
                    const long long cell = (long long)cx * g.gy + cy;
                    const long long* cells = r.cells.load(std::memory_order_acquire);
                    const float* data = r.data.load(std::memory_order_acquire);
                    int lo = 0, hi = std::min(std::max(r.n.load(std::memory_order_relaxed), 0), kMaxRecordQueries);
                    const int n = hi;
                    while (cells && lo < hi) {
                        const int mid = (lo + hi) / 2;
                        if (loadCell(cells + mid) < cell)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    const int off = r.offset[b].load(std::memory_order_relaxed);
                    if (cells && data && lo < n && loadCell(cells + lo) == cell && off >= 0 &&
                        (size_t)off + (size_t)n * nf <= kRecSlotFloats) {
                        loadRelaxed(rec, data + off + (size_t)lo * nf, (size_t)nf);
                        for (int i = 0; i < nf; ++i) res |= rec[i] == rec[i] ? 1 : 0;  // (all NaN: no onset in that run)
                    }
                }
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        if (pubSeq_.load(std::memory_order_relaxed) != s1) continue;
        if (res == 1) {
            std::memcpy(out, rec, (size_t)nf * sizeof(float));
        } else if (res == 0) {
            const float qnan = std::numeric_limits<float>::quiet_NaN();
            for (int i = 0; i < nf; ++i) out[i] = qnan;
        }
        return res;
    }
}

// ---- the geometry table

int Context::addGeometry(const Box& b) {
    // (a non-finite absorption is refused: NaN marks air in the material and coefficient planes, pv_solver.cpp addBox)
    if (!std::isfinite(b.R)) return -1;
    std::lock_guard<std::mutex> lock(geomMutex_);
    int id;
    ensureRoom(changes_, 1);
    if (geometryFree_.empty()) {  // GeometryManager.cpp:70-79
        id = (int)geometry_.size();
        geometry_.push_back(b);
    } else {  // :81-92
        id = geometryFree_.back();
        geometryFree_.pop_back();
        geometry_[(size_t)id] = b;
    }
    changes_.push_back({true, b, -1, Shape{}});
    return id;
}

void Context::removeGeometry(int id) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)geometry_.size()) return;
    ensureRoom(changes_, 1);
    ensureRoom(geometryFree_, 1);
    changes_.push_back({false, geometry_[(size_t)id], -1, Shape{}});  // GeometryManager.cpp:101-110
    geometry_[(size_t)id] = Box{0, 0, 0, 0, 0};
    geometryFree_.push_back(id);
}

void Context::updateGeometry(int id, const Box& b) {
    if (!std::isfinite(b.R)) return;
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)geometry_.size()) return;
    ensureRoom(changes_, 2);
    changes_.push_back({false, geometry_[(size_t)id], -1, Shape{}});  // GeometryManager.cpp:112-121
    geometry_[(size_t)id] = b;
    changes_.push_back({true, b, -1, Shape{}});
}

int Context::addShape(const Shape& sh) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    ensureRoom(changes_, 1);
    ensureRoom(shapeUsed_, 1);
    int id;
    if (shapeFree_.empty()) {
        id = (int)shapeUsed_.size();
        shapeUsed_.push_back(1);
    } else {
        id = shapeFree_.back();
        shapeFree_.pop_back();
        shapeUsed_[(size_t)id] = 1;
    }
    changes_.push_back({true, Box{0, 0, 0, 0, 0}, id, sh});
    return id;
}

void Context::updateShape(int id, const Shape& sh) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)shapeUsed_.size() || !shapeUsed_[(size_t)id]) return;
    ensureRoom(changes_, 1);
    changes_.push_back({true, Box{0, 0, 0, 0, 0}, id, sh});
}

void Context::removeShape(int id) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)shapeUsed_.size() || !shapeUsed_[(size_t)id]) return;
    ensureRoom(changes_, 1);
    ensureRoom(shapeFree_, 1);
    changes_.push_back({false, Box{0, 0, 0, 0, 0}, id, Shape{}});
    shapeUsed_[(size_t)id] = 0;
    shapeFree_.push_back(id);
}

int Context::addMesh(const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius, std::string* err) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    int live = 0;
    long long total = nt;
    for (int n : meshTris_) {
        live += n > 0;
        total += n;
    }
    if (live >= kMeshMax) {
        *err = "PlaneverbAddMeshGeometry: 64 meshes are live already";
        return -1;
    }
    if (total > kMeshMaxTrisTotal) {
        *err = "PlaneverbAddMeshGeometry: more than 1 << 22 triangles over all meshes";
        return -1;
    }
    // everything that can fail first (the copies among it): the tables are still what they were
    ensureRoom(changes_, 1);
    ensureRoom(meshStore_, 1);
    ensureRoom(meshTris_, 1);
    std::unique_ptr<MeshEntry> e(new MeshEntry);
    e->verts.assign(verts, verts + (size_t)3 * nv);
    e->tris.assign(tris, tris + (size_t)3 * nt);
    e->serial = meshSerialNext_++;
    e->uploadsLeft = solver2_ ? 2 : 1;
    e->nv = nv;
    e->nt = nt;
    e->mode = mode;
    e->R = R;
    e->r = radius;
    int id;
    if (meshFree_.empty()) {
        id = (int)meshTris_.size();
        meshTris_.push_back(nt);
    } else {
        id = meshFree_.back();
        meshFree_.pop_back();
        meshTris_[(size_t)id] = nt;
    }
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.mesh = 1;
    c.meshId = id;
    c.meshSerial = e->serial;
    meshStore_.push_back(std::move(e));
    changes_.push_back(c);
    return id;
}

void Context::setMeshTransform(int id, const float* m12) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)meshTris_.size() || !meshTris_[(size_t)id]) return;
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.mesh = 2;
    c.meshId = id;
    for (int k = 0; k < 12; ++k) c.m12[k] = m12[k];
    changes_.push_back(c);
}

void Context::removeMesh(int id) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (id < 0 || id >= (int)meshTris_.size() || !meshTris_[(size_t)id]) return;
    ensureRoom(changes_, 1);
    ensureRoom(meshFree_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.mesh = 3;
    c.meshId = id;
    changes_.push_back(c);
    meshTris_[(size_t)id] = 0;
    meshFree_.push_back(id);
}

void Context::setSliceHeight(float h) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.mesh = 4;
    c.h = h;
    changes_.push_back(c);
}

// (the worker's thread.  A failure of a solver call here -- a device allocation -- surfaces as the solver's error at its next run.)
void Context::applyMeshChange(Solver* s, const Change& c) {
#ifndef PVA_HOST_TEST  // (the HIP-less fake has no mesh layer)
    if (c.mesh == 2) {
        s->setMeshTransform(c.meshId, c.m12);
    } else if (c.mesh == 3) {
        s->meshClear(c.meshId);
    } else if (c.mesh == 4) {
        s->setSliceHeight(c.h);
    }
#endif
    if (c.mesh != 1) return;
    MeshEntry* e = nullptr;
    {
        std::lock_guard<std::mutex> lock(geomMutex_);
        for (auto& p : meshStore_)
            if (p->serial == c.meshSerial) e = p.get();
    }
    if (!e) return;
#ifndef PVA_HOST_TEST
    // (only this thread erases entries, so e stays valid without the lock; meshSet returns with the data on the device)
    s->meshSet(c.meshId, e->verts.data(), e->nv, e->tris.data(), e->nt, e->R, e->mode, e->r);
#else
    (void)s;
#endif
    std::lock_guard<std::mutex> lock(geomMutex_);
    if (--e->uploadsLeft <= 0)
        for (size_t i = 0; i < meshStore_.size(); ++i)
            if (meshStore_[i].get() == e) {
                meshStore_.erase(meshStore_.begin() + (long)i);
                break;
            }
}

void Context::setGridBoundary(const float R4[4]) {
    std::lock_guard<std::mutex> lock(geomMutex_);
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.boundary = true;
    for (int k = 0; k < 4; ++k) c.R4[k] = R4[k];
    changes_.push_back(c);
}

bool Context::setEdgeLayer(const int w4[4], std::string* err, bool split, double r0) {
#ifndef PVA_HOST_TEST
    const std::string nm = split ? "PlaneverbSetEdgeLayerSplit: " : "PlaneverbSetEdgeLayer: ";
    if (streaming_) {
        *err = nm + "edge layers are not available in sparse-emitter mode";
        return false;
    }
    const GridSpec& g = spec();
    const char* why = edgeLayerRefusal(g.gx, g.gy, w4);
    if (*why) {
        *err = nm + why;
        return false;
    }
    if ((w4[0] || w4[1] || w4[2] || w4[3]) && !layerConfigOk(solver_->K(), solver_->rxi())) {
        *err = nm + "no layer kernel for this grid's tile configuration";
        return false;
    }
#endif
    std::lock_guard<std::mutex> lock(geomMutex_);
    ensureRoom(changes_, 1);
    Change c{false, Box{0, 0, 0, 0, 0}, -1, Shape{}};
    c.layer = true;
    for (int k = 0; k < 4; ++k) c.W4[k] = w4[k];
    c.split = split;
    c.r0 = split ? r0 : kEdgeLayerR0;
    changes_.push_back(c);
    return true;
}

void Context::applyChange(Solver* s, const Change& c) {
    if (c.rec) {
#ifdef PVA_LIVE_RECORDS
        // (validated by the setters against the state these changes lead to, in queue order; a failure here -- the pinned block's
        // allocation -- leaves the solver's kinds as they were, and the latch follows the solver's kinds)
        if (c.rec == 1) {
            s->setQueryRecords(c.recKinds);
            if (!c.recKinds) s->setRecordQueries(nullptr, 0);
        } else if (c.rec == 2) {
            s->setEchogram(c.recSeconds, c.recN);
        } else {
            s->setLobeWindows(c.recN ? c.recEdges : nullptr, c.recN);
        }
#endif
        return;
    }
    if (c.layer) {
#ifndef PVA_HOST_TEST
        s->setEdgeLayer(c.W4, c.split, c.r0);  // (validated by setEdgeLayer: the widths fit the grid and the configuration)
#endif
        return;
    }
    if (c.boundary) {
#ifndef PVA_HOST_TEST
        s->setGridBoundary(c.R4);  // (validated by the caller: finite values cannot be refused)
#endif
        return;
    }
    if (c.shapeId >= 0) {
#ifndef PVA_HOST_TEST  // (the HIP-less fake has no shape layer)
        // (a failure here -- the device allocation of the first shape -- surfaces as the solver's error at its next run)
        if (c.add)
            s->shapeSet(c.shapeId, c.shape);
        else
            s->shapeClear(c.shapeId);
#endif
        return;
    }
    if (c.add)  // GeometryManager.cpp:123-152
        s->rasterAdd(c.box);
    else
        s->rasterRemove(c.box);
}

void Context::pushGeometryChanges() {
    std::vector<Change> q;
    {
        std::lock_guard<std::mutex> lock(geomMutex_);
        q.swap(changes_);
    }
    if (solver2_) {  // pipelined: every solver rasterises every change, in queue order, before ITS next iteration
        for (auto& pend : pending_) pend.insert(pend.end(), q.begin(), q.end());
        return;
    }
    for (const Change& c : q) {  // GeometryManager.cpp:123-152, applied in queue order
        if (c.mesh)
            applyMeshChange(solver_, c);
        else
            applyChange(solver_, c);
    }
}

void Context::applyPending(const int k) {
    Solver* s = k == 0 ? solver_ : solver2_;
    for (const Change& c : pending_[k]) {
        if (c.mesh)
            applyMeshChange(s, c);
        else
            applyChange(s, c);
    }
    pending_[k].clear();
}

}  // namespace pva
