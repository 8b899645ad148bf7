// pv_context.h -- the live acoustics module behind the reference's C-ABI (PlaneverbInit ... PlaneverbExit).
//
// Mirrors ProjectPlaneverb/src/Context/PvContext.{h,cpp}: a singleton that owns the grid, the geometry and
// emission tables, and one library-owned worker that loops
//     GenerateResponse(listener) -> AnalyzeResponses(listener) -> PushGeometryChanges() -> latch listener
// (PvContext.cpp:63-94).  Here the worker owns a Solver (one HIP stream on one MI355X) instead of running the
// sweeps itself, and publishes what each iteration can have changed -- the history-window block of the result map
// -- into a pinned host double buffer, so that GetOutput stays O(1), never touches the device and never takes a
// lock (the reference reads the result grid unsynchronised while it is rewritten).
//
// Threading contract (checked under ThreadSanitizer / AddressSanitizer by tests/host/, a HIP-less build of this
// file and pv_core.cpp against a fake Solver):
//   * any API function may be called from any thread at any time, including concurrently with Exit / re-Init:
//     entry points pin the context with Context::Ref (one fetch_add + one load, wait-free); Exit unpublishes the
//     pointer, marks the context as retiring (which wakes the callers that block inside it: WaitIterations) and waits
//     for the pinned callers to leave before it deletes anything;
//   * GetOutput never takes a lock and never touches the device.  It reads one consistent iteration through a
//     sequence lock around the publish step (a few stores): a reader repeats only if a publish happened while it
//     copied its 32 bytes -- LOCK-FREE, not wait-free (a reader can in principle lose against every publish; publishes
//     are one per iteration, milliseconds apart).
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pv_core.h"
#include "pv_query_records.h"
#ifdef PVA_HOST_TEST
#include "fake_solver.h"  // tests/host/: same interface, no HIP
#else
#include "pv_solver.h"
#endif

namespace pva {

struct LiveConfig {
    float sizeX = 0, sizeY = 0;
    int res = 0;
    int boundaryType = 0;
    const char* tempDir = nullptr;
    int maxThreads = 0;
    int executionType = 0;
};

struct Out8 {
    float v[8];
};

class Context {
public:
    // Planeverb::Init / Exit (PvContext.cpp:25-44).  init() returns false (and leaves no context) where the
    // reference throws pv_InvalidConfig / pv_NotEnoughMemory.
    static bool init(const LiveConfig& cfg, std::string* err);
    static void exit();

    // Pins the current context for the duration of one API call (see the threading contract above).
    class Ref {
    public:
        Ref();
        ~Ref();
        Ref(const Ref&) = delete;
        Ref& operator=(const Ref&) = delete;
        explicit operator bool() const { return c_ != nullptr; }
        Context* operator->() const { return c_; }
        Context* get() const { return c_; }

    private:
        Context* c_;
    };

    // EmissionManager (Emissions/EmissionManager.cpp:37-75)
    int emit(float x, float y, float z);
    void updateEmission(int id, float x, float y, float z);
    void endEmission(int id);
    // Planeverb::GetOutput (FDTD.cpp:16-58)
    Out8 getOutput(int id);
    // the published result record of result cell (cx, cy) (what GetOutput reads after its position -> cell step)
    Out8 outputAt(int cx, int cy);

    // GeometryManager (Geometry/GeometryManager.cpp:67-152)
    int addGeometry(const Box& b);
    void updateGeometry(int id, const Box& b);
    void removeGeometry(int id);
    // shapes (pv_core.h Shape, already validated): ids of their own, recycled LIFO; queued with the AABB changes
    int addShape(const Shape& sh);
    void updateShape(int id, const Shape& sh);
    void removeShape(int id);
    // Triangle meshes (Solver::meshSet, already validated by pv_core.h validateMesh): ids of their own, recycled LIFO.  The
    // vertex data is copied into a store the context owns AT THE CALL -- the one step that can fail: -1 + *err, nothing changed --
    // and the queued change carries only the id, the operation, twelve floats and h, so it stays a fixed-size record.  An entry
    // of the store lives until every solver has taken it to the device.
    int addMesh(const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius, std::string* err);
    void setMeshTransform(int id, const float* m12);
    void removeMesh(int id);
    void setSliceHeight(float h);
    // grid edges (Solver::setGridBoundary, finite values already checked): queued with the geometry changes, applied to every
    // solver at the same iteration boundary
    void setGridBoundary(const float R4[4]);
    // edge layers (Solver::setEdgeLayer): refused in sparse-emitter mode and for widths the grid cannot hold (false + *err);
    // else queued with the geometry changes and applied to every solver at the same iteration boundary
    // (split, r0: the model, Solver::setEdgeLayer)
    bool setEdgeLayer(const int w4[4], std::string* err, bool split = false, double r0 = kEdgeLayerR0);

    // Emission records: the in-run analysis records (Solver::setQueryRecords, pv_query_records.hip) of the live emitters' cells,
    // published with every iteration.  The three setters validate at the call with the rules of the Solver calls (false + *err,
    // "emission records: ..."; refused in sparse-emitter mode), then queue with the geometry changes and take effect on every
    // solver at the same iteration boundary.  At the start of an iteration with kinds selected the worker latches the live
    // emitters' cells (ascending id, ended ids skipped, the first kMaxRecordQueries DISTINCT in-map cells, sorted) into that
    // iteration's solver; the iteration's records then become readable in the same publish step as its outputs.
    bool setEmissionRecords(unsigned kinds, std::string* err);
    bool setEmissionEchogram(float slotSeconds, int nSlots, std::string* err);
    bool setEmissionLobeWindows(const float* edgesSeconds, int nEdges, std::string* err);
    // of the PUBLISHED iteration: its kinds, the floats of one kind (-1: not carried), its distinct cells
    unsigned emissionRecordKinds();
    int emissionRecordFloats(unsigned kind);
    int emissionRecordCells();
    // The record of the emitter's CURRENT cell in the published iteration: 1 = written; 0 = quiet NaNs written (an id never issued
    // or ended, a position off the map, a cell that is not in the iteration's table or has no onset in it); -1 = nothing written
    // (not one kind, the iteration does not carry it, no buffer, cap too small).  Lock-free like getOutput: no device access, no
    // lock, no allocation.
    int emissionRecord(int id, unsigned kind, float* out, int cap);

    void setListener(float x, float y, float z);  // PvContext.cpp:50-56
    // Planeverb::GetImpulseResponse (FDTD.cpp:60-70): the IR of the last COMPLETED iteration at a world position as
    // reference Cells (16 B each).  Waits for the iteration in flight.  Returns the response length T (cells16 gets
    // min(cap, T) cells), 0 for a position outside the cell array, -1 on error.
    int impulseResponse(float x, float y, float z, void* cells16, int cap);

    // Published iterations, read off the publish step's sequence lock (two counts per publish): the count changes with the flip
    // itself, so two reads -- GetOutput, an emission record -- between two equal counts are of ONE iteration
    long long iterations() const { return (long long)(pubSeq_.load(std::memory_order_acquire) >> 1); }
    // a number no other context of this process has had (a new context can land on a retired one's address)
    unsigned long long generation() const { return generation_; }
    long long waitIterations(long long count, int timeoutMs);
    const GridSpec& spec() const { return solver_->spec(); }
    // the worker stops for good on a solver error: then this is true, workerError() says why and IsRunning reports 0
    bool failed() const { return failed_.load(std::memory_order_acquire); }
    std::string workerError();
    // true when the solver runs in the sparse-emitter mode (the T-step history did not fit, or PLANEVERB_AMD_LIVE_STREAMING=1):
    // the worker registers the emitters alive at the start of every iteration, wet gain / RT60 exist for their cells
    bool streaming() const { return streaming_; }

private:
    Context() = default;
    ~Context();
    void workerMain();
    void workerLoop();
    // Pipelined iterations (small grids): TWO solvers, two iterations in flight.  Iteration i + 1 starts -- with the listener
    // latched and the geometry pushed at that moment, as in the reference's loop (PvContext.cpp:86-89) -- while iteration i is
    // still running on the other solver: every result still answers the listener its run started with one run time later,
    // but results arrive twice as often.  What an iteration leaves untouched (cells without an onset keep the previous
    // iteration's values, Analyzer.cpp:160-165) is carried from the other solver's maps on the device (Solver::run's
    // carryFrom), so the published records are those of the one-solver loop.
    void workerLoopPipelined();
    void pushGeometryChanges();
    void applyPending(int k);
    bool beginPublish();
    bool finishPublish();
    void publishSlot(int back, const Solver::WindowBlock& w);
    bool pendPublish_ = false;
    int pendBack_ = 0;
    Solver::WindowBlock pendWin_;
    void beginRetire();
    bool registerEmitters();
    bool latchRecords(int k);
    bool collectRecords(int k, int slot);
    friend void retireContext(Context*);

    unsigned long long generation_ = 0;
    Solver* solver_ = nullptr;
    Solver* solver2_ = nullptr;           // pipelined mode only
    Solver* lastSolver_ = nullptr;        // the solver that ran the last PUBLISHED iteration (GetImpulseResponse reads it)
    std::thread worker_;
    std::atomic<bool> running_{false};
    std::atomic<bool> retiring_{false};
    std::atomic<bool> failed_{false};
    bool streaming_ = false;
    std::atomic<long long> iterations_{0};
    std::mutex iterMutex_;
    std::condition_variable iterCv_;
    std::mutex errMutex_;
    std::string workerErr_;
    // the worker holds this while it uses the solver (an iteration + the geometry push); GetImpulseResponse takes it
    std::mutex solverMutex_;
    std::atomic<int> solverWaiters_{0};

    // listener (a plain vec3 in the reference, PvContext.h:40, where a reader can see x of one SetListenerPosition and
    // z of the next).  The simulation uses x and z only (world y is ignored, FDTD.cpp:97-98): both live in ONE 64-bit
    // atomic, so the worker always latches a position some caller actually set.
    std::atomic<uint64_t> lxz_{0};
    std::atomic<float> ly_{0.f};
    static uint64_t packXZ(float x, float z);
    static void unpackXZ(uint64_t v, float* x, float* z);

    // emitters: fixed-capacity chunks so readers never race a reallocation
    struct Emitter {
        std::atomic<float> x{0.f}, y{0.f}, z{0.f};
        std::atomic<int> live{0};  // 1 between Emit and EndEmission (what emissionRecord asks; GetOutput never did)
    };
    static constexpr int kChunk = 1024, kMaxChunks = 1024;
    std::atomic<Emitter*> chunks_[kMaxChunks] = {};
    std::atomic<int> emitterCount_{0};
    std::vector<int> emitterFree_;
    std::mutex emitMutex_;
    Emitter* emitterAt(int id);

    // geometry table + change queue (GeometryManager.h:28-46)
    struct Change {
        bool add;
        Box box;
        int shapeId;  // >= 0: slot shapeId of the shape table takes `shape` (add) or is emptied; box unused
        Shape shape;
        bool boundary = false;  // a grid-edge change: R4 replaces the four edge absorptions; the rest is unused
        float R4[4] = {0.f, 0.f, 0.f, 0.f};
        bool layer = false;  // an edge-layer change: W4 replaces the four widths
        int W4[4] = {0, 0, 0, 0};
        bool split = false;  // ... and the model
        double r0 = kEdgeLayerR0;
        // an emission-records change: 1 = the kinds, 2 = the echogram slots, 3 = the lobe windows (recN edges; 0 = the default)
        int rec = 0;
        unsigned recKinds = 0;
        float recSeconds = 0.f;
        int recN = 0;
        float recEdges[kLobesMaxEdges] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // a mesh change: 1 = slot meshId takes the store's entry meshSerial, 2 = its transform, 3 = it is emptied, 4 = the slice height
        int mesh = 0;
        int meshId = -1;
        int meshSerial = 0;
        float m12[12] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float h = 0.f;
    };
    static void applyChange(Solver* s, const Change& c);
    void applyMeshChange(Solver* s, const Change& c);
    struct MeshEntry {
        int serial = 0, uploadsLeft = 0;  // (one upload per solver)
        int nv = 0, nt = 0, mode = 0;
        float R = 0.f, r = 0.f;
        std::vector<float> verts;
        std::vector<int> tris;
    };
    std::vector<std::unique_ptr<MeshEntry>> meshStore_;
    std::vector<int> meshTris_;  // per id: the live mesh's triangle count, 0 = empty slot
    std::vector<int> meshFree_;
    int meshSerialNext_ = 1;
    std::vector<Box> geometry_;
    std::vector<int> geometryFree_;
    std::vector<uint8_t> shapeUsed_;
    std::vector<int> shapeFree_;
    std::vector<Change> changes_;
    std::vector<Change> pending_[2];  // pipelined mode: drained from the queue, not yet rasterised into solver k
    std::mutex geomMutex_;

    // Published results.  Only the block of the map an iteration can have changed (the history window) crosses PCIe:
    // two pinned slots of windowCapacity() records, `front_` selects the readable one, `pubSeq_` is the sequence lock
    // of the publish step (odd while the worker flips front_ and the slot's block description).  Cells outside the
    // front block keep the values they had when they were last inside one -- `base_`, a full-size map allocated the
    // first time the window moves (all zeros before: a fresh context's pool, PvContext.cpp:132) -- except the listener
    // direction, which the reference recomputes for every cell on every iteration and which is the unit vector
    // listener -> cell there (Analyzer.cpp:365-391,415-428).
    struct Slot {
        float* data = nullptr;
        std::atomic<int> r0{0}, c0{0}, nr{0}, nc{0};
        std::atomic<float> lx{0.f}, lz{0.f};
    };
    Slot slots_[3];  // one readable + one per iteration in flight
    std::atomic<int> front_{-1};
    std::atomic<uint64_t> pubSeq_{0};
    std::atomic<float*> base_{nullptr};

    // Emission records.  What the callers have asked for so far (the state the queued changes lead to: the setters validate against
    // it), under geomMutex_:
    unsigned wantKinds_ = 0;
    int wantSlots_ = 0, wantEdges_ = 0;
    float wantEdge_[kLobesMaxEdges] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // the worker's: the table latched into solver k at the start of its iteration (sorted distinct cells), and its scratch
    struct Latch {
        unsigned kinds = 0;
        std::vector<long long> cells;
    };
    Latch latch_[2];
    std::vector<std::pair<long long, int>> latchScratch_;
    std::vector<float> latchXyz_, recStage_;
    // One record slot per result slot, selected by front_ and read under pubSeq_ like the result block: the iteration's sorted cell
    // table, its kinds with their floats and offsets, and the floats (per kind n x floats[kind] from offset[kind] on).  The tables
    // are allocated by the worker the first time an iteration carries records (kMaxRecordQueries cells, every kind at its largest
    // setting) and live as long as the context: a reader may still be looking at them.  The pend* members are the worker's own: what
    // collectRecords left in the slot, made visible by publishSlot.
    static constexpr int kRecMaxFloats = 1 + 3 * kEchogramMaxSlots;  // the largest record of one kind
    static constexpr size_t kRecSlotFloats =
        (size_t)kMaxRecordQueries * (kRoomMetricFloats + kDecayFloats + kLateralFloats + (1 + 3 * kEchogramMaxSlots) + kEchoFloats +
                                     (1 + 5 * kLobesMaxWindows));
    struct RecSlot {
        std::atomic<long long*> cells{nullptr};
        std::atomic<float*> data{nullptr};
        std::atomic<int> n{0};
        std::atomic<unsigned> kinds{0};
        std::atomic<int> floats[kQueryRecordKinds] = {}, offset[kQueryRecordKinds] = {};
        unsigned pendKinds = 0;
        int pendN = 0, pendFloats[kQueryRecordKinds] = {}, pendOffset[kQueryRecordKinds] = {};
    };
    RecSlot rec_[3];
};

}  // namespace pva
