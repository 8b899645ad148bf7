// pv_solver.h -- host side of the MI355X solver: owns the HBM planes, the HIP stream and the launch schedule.
//
// One Solver = the reference's Grid + FreeGrid + Analyzer for one config on one GPU
// (ProjectPlaneverb/src/FDTD/Grid.h:25-74, FreeGrid.h:7-24, DSP/Analyzer.h:24-50), without any thread: run()
// enqueues  [geometry deltas] -> reset -> T/K fused step launches -> analysis  on the solver's stream, which is
// what one iteration of Context's background loop does (Context/PvContext.cpp:74-93).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "pv_core.h"
#include "pv_device.h"
#include "pv_query_spectral.h"
#include "pv_zone_decay.h"
#include "pv_zone_maps.h"

namespace pva {

struct SolverOptions {
    int K = 0;            // steps per launch (0 = default)
    int rxi = 0;          // interior rows per tile (0 = default)
    bool denseHistory = false;
    int numSteps = 0;     // override T (0 = reference value)
    bool skipAnalysis = false;
    int useGraph = 0;     // 0 = auto (small grids), 1 = always, 2 = never: replay the run from a captured hipGraph
    bool withFreeGrid = true;
    int tileOrder = -1;   // air-kernel block->tile map: 0 = linear, 1 = XCD band of tile rows, row-major (1-5 % faster than 0),
                          // 2 / >= 4 = compact variants of it (fewer bytes, slower), 3 = XCD strip of tile COLUMNS, row-major:
                          // a tile's vertical halo neighbours are nty/8 tiles away instead of nty, so they are still in the
                          // 4 MiB L2 (HBM reads 316 -> 268 MB per launch at 4096^2, 1400 -> 948 MB at 8192^2; +2.5 % / +4 %
                          // cell-updates/s; -3 % at 2048^2 and below).  -1 = by grid size: 3 for the large-grid tile, else 1
    int merged = 1;       // 1 = general + air tiles in one launch per K steps (where it compiles spill-free), 0 = two kernels on two streams
    int segments = 0;     // N > 0: row-streaming air segments (pv_seg.h) instead of one wave per air tile, about N per
                          // sweep; only the (K, rows) = (8, 40) and (12, 36) configurations have the kernel.  0 = off
    bool streaming = false;  // sparse-emitter mode: ring history + incremental forward analysis
    bool autoStreaming = false;  // switch to the sparse-emitter mode when the T-step pressure history does not fit the
                                 // device (the live module: Planeverb::Init accepts any resolution, PvContext.cpp:101-107)
    bool packed = true;   // packed-f32 arithmetic in the air-tile kernel (VALU-issue bound otherwise)
    bool edgeTiles = false;  // grid-edge tiles of empty regions on the air path + overrides (tile class 2): only the
                             // batched kernel has that arm, so every run of such a solver goes through it
    int smallGrid = 0;    // 0 = auto: grids that fit one CU's LDS run in the whole-grid-resident kernel; 2 = never
    int timeKernels = 0;  // N > 0: HIP events around every Nth step-kernel launch (bench / roofline)
    // Row slab of a larger grid (single-grid domain decomposition, pv_slabs.h): this solver owns the tile rows
    // [ntx * slabIndex / slabCount, ntx * (slabIndex + 1) / slabCount) of the grid, allocates planes for those rows only
    // and keeps the K rows its neighbours own next to them current in its guard band (SlabGroup exchanges them after
    // every launch).  slabCount = 1: a whole grid.
    int slabIndex = 0, slabCount = 1;
    int auxStreams = 0;   // streams created and never used (PVA_OPT_AUX_STREAMS: hardware-queue placement of the solvers' main streams)
    int streamFuse = -1;  // sparse-emitter mode: forward sums of air tiles inside the stencil (pv_stream.h): -1 = by grid size (on from 6000 tiles: it costs two more launches per sweep and pays where the ring traffic binds), 0 = ring + accumulate pass for every tile (round 2's form), 1 = on
    bool lazyFar = true;  // far cells of the result map lazily (see Solver::lazyFar_)
    int patch = -1;       // air tiles by the persistent patch kernel (pv_patch.h): -1 = default of the configuration, 0 off, 1 on
    int patchStrip = 3;   // patch columns per strip of its walk
    int streamPriority = 0;  // PVA_OPT_STREAM_PRIORITY: 1 = main stream on the highest priority (a hardware queue apart from the default-priority streams)
    bool debugLoseFirstCapture = false;  // PVA_OPT_DEBUG_LOSE_FIRST_CAPTURE: the solver's first graph capture counts as lost
    int fusedAnalysis = -1; // 1 = grids whose history window is the whole grid (up to 98 304 cells) run their analysis as ONE launch (pv_fused.hip: EXPERIMENTAL build only, refused by the product build); -1 / 0 (default) = the separate kernels
    int analysisFork = 1; // 0: wet gain / decay time behind the encode pass instead of beside it (measurements)
    int rt60Lanes = 0;    // decay-time pass: lanes per cell (pv_rt60.hip): 0 = by the number of reachable cells, 16 / 4 / 1 = forced
    int resident = 0;     // resident kernel (pv_resident.hip: one launch per run, every tile a workgroup that stays on its CU for
                          // all T steps): 0 = auto (default tile of the launch-bound grids, whole-grid history window, all
                          // blocks co-resident), 1 = also with an explicitly chosen tile, 2 = never
    int xcdRegions = -1;       // tile order 3: 1 = every XCD owns one of 2 x 4 regions of the grid instead of one of 8 strips of tile
                               // columns (half as many boundary lines fetched by two XCDs); -1 = default (on), 0 = strips
    int alternateSweeps = -1;  // tile order 3: odd launches of a run walk the XCD strips backwards (StepArgs::sweepReverse):
                               // -1 = default, 0 = off, 1 = on
    int rowBands = 0;     // B > 1: each sweep = B launches (bands of tile rows, one stream each) with 3-point
                          // dependencies between consecutive sweeps; 0 = auto, 1 = off
    int reachBound = -1;  // PVA_OPT_REACH_BOUND: runs of the plain merged-launch path advance only the tiles the pulse can have
                          // reached by each launch (Solver::setReachArgs); -1 = default (on), 0 = full sweeps, 1 = on
    int residentWindow = -1;  // PVA_OPT_RESIDENT_WINDOW: a reach-bounded run whose listener is walled in steps only the tile window
                              // around its air component, in one launch of the resident kernel (Solver::enqueueWindowRun);
                              // -1 = default (on), 0 = off, 1 = on
};

struct SolverTimings {
    float fdtdMs = 0, analysisMs = 0, geometryMs = 0;
    float stepLoopMs = 0;  // the back-to-back step launches alone (fdtdMs minus the field reset); 0 when replayed from a graph
    float airKernelMs = 0, generalKernelMs = 0;  // mean duration per launch (timeKernels only)
    int airLaunches = 0, generalLaunches = 0;
    int stepLaunches = 0;
    int reachedCells = 0;  // cells with an onset in the last analysed run (whole grids, full-history analysis)
    int activeCells = 0;   // cells of the window's ever-non-zero tiles
    int silentCells = 0;   // air cells among them whose whole history stayed below the audible threshold
};

// the per-cell analysis maps a solver keeps (Solver::maps_; their messages: kAnalysisInfo, pv_solver_maps.cpp)
enum AnalysisKind {
    kMapRoomMetrics,
    kMapDecayTimes,
    kMapLateralFraction,
    kMapEchoCriterion,
    kMapEchogram,
    kMapLobes,
    kMapBandMetrics,
    kMapModulation,
    kMapSpectrum,
    kAnalysisKinds
};

class SlabGroup;
class SlabRoot;
struct SlabRankOps;

// A stream with a hardware queue apart from every other claimed stream of its device.  The runtime multiplexes a process's streams
// on a small pool of hardware queues (four per priority by default), dealt by the number of streams that already use each; packets
// of two streams on one queue run one after the other, and a waiting packet parks what sits behind it.  claim() probes the stream
// against every claimed, idle stream of the device (streamsShareQueue, pv_probe.hip) and replaces it while it shares -- the
// replaced ones stay alive ("parked") until release(), so that the pool deals the next one elsewhere.
struct QueueClaim {
    std::vector<hipStream_t> parked;
    hipStream_t claimed = nullptr;
    int redeals = 0;
    // The probe of a NEW solver launches on the claimed streams of the live ones, from the creating thread.  `use` serialises it
    // with the stream's owner: the owner holds it while it enqueues on (or captures) its stream, the prober only tries it and
    // leaves a stream whose owner is at work alone (round 5's hipStreamQuery alone left a window in which the owner could begin
    // a graph capture under the sleepers: ADVICE r05).
    std::shared_ptr<std::recursive_mutex> use;
    std::unique_lock<std::recursive_mutex> lockUse() const { return use ? std::unique_lock<std::recursive_mutex>(*use) : std::unique_lock<std::recursive_mutex>(); }  // (recursive: a run that falls back to the replayed graph re-enters enqueueRun from sync)
    enum { kNormal = 0, kHigh = 1, kLow = 2 };  // the runtime keeps a pool of hardware queues per priority
    bool claim(int device, hipStream_t* stream, int priority, const void* owner);
    // another stream of the same priority in place of the claimed one (which stays parked, so that the pool deals elsewhere): a
    // slab group whose hand-off's dry run did not come through on the streams it was dealt (SlabGroup::init)
    bool replace(hipStream_t* stream);
    int priorityClass = kNormal;
    void release();  // before the stream itself is destroyed
};

// Work enqueued on a solver's stream behind every run's analysis and output queries (a baked probe table's gather, pv_bake.cpp),
// also behind a run that sync() repeats: res = the 8 SoA result planes, delay = the onset map, [r0, r0 + nr) x [c0, c0 + nc) =
// the run's history-window block of the result map
struct RunTap {
    virtual ~RunTap() = default;
    virtual void afterRun(const float* res, const float* delay, long long resN, int gy, int r0, int c0, int nr, int nc,
                          hipStream_t stream) = 0;
};

class Solver {
    friend class SlabGroup;
    friend class SlabRoot;
    friend struct SlabRankOps;

public:
    static Solver* create(const GridSpec& spec, int device, const SolverOptions& opt, std::string* err);
    ~Solver();

    const GridSpec& spec() const { return g_; }
    const Geometry& geometry() const { return geo_; }
    int device() const { return device_; }
    int K() const { return K_; }
    int rxi() const { return rxi_; }
    float efree() const { return efree_; }
    void setEfree(float e) { efree_ = e; }  // slab ranks: computed once for the whole grid
    int T() const { return T_; }
    long long deviceBytes() const { return deviceBytes_; }
    int histRows() const { return histRows_; }
    int histPitch() const { return histPitch_; }
    const std::string& lastError() const { return err_; }
    bool streamFuse() const { return streamFuse_; }
    bool lastRunResidentWindow() const { return plan_.path == StepPath::Window; }
    bool lastRunOneXcd() const { return plan_.oneXcd; }  // the last run's hand-off went through one XCD's L2 (pv_resident.hip)
    bool residentKernel() const { return caps_.useResident && !layerActive(); }  // runs of this solver go through pv_resident_kernel (when the
                                                          // device's resident-block budget allows: else the replayed graph)
    SolverOptions& options() { return opt_; }

    // geometry table with the reference's id recycling (Geometry/GeometryManager.cpp:67-121)
    int addBox(const Box& b);
    bool updateBox(int id, const Box& b);
    bool removeBox(int id);
    int numBoxes() const;
    std::vector<std::pair<int, Box>> boxes() const;
    // raw rasteriser access (Grid::AddAABB / RemoveAABB), used by the live context's change queue
    void rasterAdd(const Box& b) {
        mat_.add(b);
        invalidateAnalysisMaps();
    }
    void rasterRemove(const Box& b) {
        mat_.remove(b);
        invalidateAnalysisMaps();
    }

    // Shape layer (pv_shapes.h): convex polygons, round shapes and simple polygons (pv_core.h Shape::kind) over the AABB layer,
    // ids of their own with the same LIFO recycling.  The
    // first shape gives the solver a device plane for the AABB layer; a solver that never has one keeps the AABB-only path.
    int addShape(const Shape& sh);
    bool updateShape(int id, const Shape& sh);
    bool removeShape(int id);
    int numShapes() const;
    // raw access for the live context, which keeps the id table itself: slot `id` takes `sh` (added or updated: it becomes the
    // most recent shape) / is emptied
    bool shapeSet(int id, const Shape& sh);
    bool shapeClear(int id);

    // Mesh layer (pv_mesh.h; the model: include/planeverb_amd.h, "Triangle meshes"): triangle meshes kept on the device, sliced at
    // sliceHeight() and rasterised between the AABB layer and the shape layer by applyGeometry.  The data is validated by the
    // caller (pv_core.h validateMesh); the limits on live meshes and on triangles over all of them are checked here.  Ids are a
    // table of their own with LIFO recycling.  A solver that never has a mesh allocates and launches nothing of this.
    int addMesh(const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius);
    bool updateMesh(int id, const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius);
    bool setMeshTransform(int id, const float* m12);
    bool removeMesh(int id);
    int numMeshes() const;
    int meshTriangles(int id) const;  // -1: no such mesh
    bool setSliceHeight(float h);
    float sliceHeight() const { return sliceH_; }
    // the segments as the device sliced them, out4[4 nt] and valid[nt] (applyGeometry first: changes may be pending)
    bool copyMeshSection(int id, float* out4, uint8_t* valid);
    // raw access for the live context, which keeps the id table itself (as shapeSet / shapeClear)
    bool meshSet(int id, const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius);
    bool meshClear(int id);

    // Grid edges (pv_boundary.h): absorption R of sides x = 0, x = gx, y = 0, y = gy, as PlaneverbAddGeometry takes it; all 0
    // (the default) is the reference's absorbing grid.  A change takes effect at the next run of any form.  Finite values only.
    bool setGridBoundary(const float R4[4]);
    void gridBoundary(float R4[4]) const;
    bool boundaryAbsorbing() const;  // every side has Y = 1 (the edge pass is not launched)

    // Graded absorbing layers (pv_layer.h): widths in cells of sides x = 0, x = gx, y = 0, y = gy, 0..64, 0 = none.  A change
    // takes effect at the next run of any form (tiles reclassified, a captured graph dropped).  Refused on sparse-emitter solvers,
    // slabs, edge-tile solvers and tile configurations without a layer kernel.  A solver with a layer runs the tile path: merged
    // launches + the layer launch; the resident, small-grid, segment, patch, row-band and two-kernel forms resolve off.
    // split = the split-field model (pv_layer.h) with design reflection r0 (0 < r0 < 1, else refused); split = false: the
    // unsplit model, R0 = kEdgeLayerR0.  A width, model or R0 change reclassifies and drops a captured graph alike.
    bool setEdgeLayer(const int w4[4], bool split = false, double r0 = kEdgeLayerR0);
    void edgeLayer(int w4[4]) const;
    void edgeLayerModel(bool* split, double* r0) const {
        *split = layerSplit_;
        *r0 = layerR0_;
    }
    bool layerActive() const { return layerW_[0] > 0 || layerW_[1] > 0 || layerW_[2] > 0 || layerW_[3] > 0; }

    // carryFrom (live module, two iterations in flight on two solvers): the solver that ran the PREVIOUS iteration.  The cells
    // in which this run finds no onset take their occlusion / wet gain / decay time / lowpass / source direction from that
    // solver's maps, on the device, behind that solver's analysis and in front of this run's listener-direction pass -- what one
    // solver's persistent result map does by itself (Analyzer.cpp:160-165 leaves m_results untouched there, and the direction
    // walk reads those values, :340-431)
    bool run(float lx, float ly, float lz, bool wait, Solver* carryFrom = nullptr);
    bool runCells(int lcx, int lcy, float lx, float lz, bool wait);
    bool sync();
    // n <= 8 identically configured solvers of one device: n independent runs (listeners lxyz[3n]) advanced by one
    // launch per K steps (pv_step_batch_kernel); each solver then holds its run's results as after run()
    static bool runBatch(Solver* const* s, int n, const float* lxyz, bool wait, std::string* err);
    bool runSteps(int nsteps, bool withPulse, float lx, float lz);
    const SolverTimings& timings() const { return tim_; }

    bool getOutput(float ex, float ey, float ez, float out8[8], bool* valid);
    // output queries: up to kMaxQueries emitter positions whose 8 outputs every following run leaves in pinned host
    // memory (one gather kernel behind the analysis): after sync() they are read without any further GPU work
    static constexpr int kMaxQueries = 64;
    bool setOutputQueries(const float* xyz, int n);
    bool queriedOutputs(float* out8n, unsigned char* valid, int n);
    // In-run analysis records of the registered queries' cells, in two families with a selector, a pinned block, a launch and a
    // stamp each (pv_solver_records.cpp): the six time-domain kinds (bits kQrec*, pv_query_records.h / .hip; PvAmdSetQueryRecords)
    // and, directly behind them, the three frequency-resolved ones (bits kQspec*, pv_query_spectral.h / .hip;
    // PvAmdSetQuerySpectralRecords).  Every following run computes a family's selected kinds for the queries' cells in ONE launch
    // behind its analysis and in front of its last kernel, straight into pinned host memory; the records are bit for bit the
    // whole-map passes' at the same cells, under the settings in force when the run was enqueued.  kinds = 0 (the default): nothing
    // is launched and the block is freed.  Every setter waits for a run in flight.  queried...Records: n x ...Floats(kind) floats of
    // ONE kind, after the run has been waited for; refused until a run enqueued under the current kinds, queries and settings has
    // completed without error.  The spectral kinds' device tables are made valid in the setters, never on the enqueue path
    enum RecordFamily { kRecTime = 0, kRecSpectral = 1, kRecordFamilies = 2 };
    bool setQueryRecords(unsigned kinds) { return selectRecords(kRecTime, kinds); }
    unsigned queryRecordKinds() const { return opt_.streaming ? 0u : recs_[kRecTime].kinds; }
    int queryRecordFloats(unsigned kind) { return recordFloats(kRecTime, kind); }  // -1: not one kind, or its setting is missing
    bool queriedRecords(unsigned kind, float* out, int n) { return readRecords(kRecTime, kind, out, n); }
    bool setQuerySpectralRecords(unsigned kinds) { return selectRecords(kRecSpectral, kinds); }
    unsigned querySpectralKinds() const { return opt_.streaming ? 0u : recs_[kRecSpectral].kinds; }
    int querySpectralFloats(unsigned kind) { return recordFloats(kRecSpectral, kind); }
    bool queriedSpectralRecords(unsigned kind, float* out, int n) { return readRecords(kRecSpectral, kind, out, n); }
    // Record queries: up to kMaxRecordQueries (pv_query_records.h) positions of their own, mapped in the given order as
    // setOutputQueries maps them.  While n > 0 the in-run records are computed for THESE cells instead of the output queries'
    // (64 queries per wave, one more block row per 64), and queried...Records take this n; the eight-output gather keeps serving
    // the output queries.  n = 0, the default, returns to the output queries.  The pinned cell table and the record blocks grow to
    // the registered count.  Waits for a run in flight; a change invalidates the records until the next run
    bool setRecordQueries(const float* xyz, int n);
    int recordQueries() const { return numRecQueries_; }
    // Emitter records (sparse-emitter mode only, PvAmdSetEmitterRecords): the same two families, selectors, pinned blocks, launches
    // and stamps with the registered emitters (setEmitters) as the cell source -- record i belongs to the i-th emitter setEmitters
    // kept.  The mode keeps a ring of pressure planes, not the history, so while a kind is selected every accumulate pass also
    // copies the emitters' cells -- and, for the velocity kinds, their neighbours (X - 1, Y) and (X, Y - 1) -- from the ring into
    // record traces laid out as history planes ([T][P] floats, AnalyzeArgs::recTrace: 104 MB at T = 25 432 and 1024 emitters, 312 MB
    // with the neighbour columns), and the two record launches behind the run's finalize pass walk those.  The records are bit for
    // bit what a full-history solver's whole-map passes give at the emitters' cells.  At most kMaxRecordQueries emitters while a kind
    // is selected.  The selectors of the output queries' records keep refusing in this mode
    bool setEmitterRecords(unsigned timeKinds, unsigned spectralKinds);
    unsigned emitterRecordKinds(RecordFamily f) const { return opt_.streaming ? recs_[f].kinds : 0u; }
    int emitterRecordFloats(RecordFamily f, unsigned kind);
    bool emitterRecords(RecordFamily f, unsigned kind, float* out, int n) { return readRecords(f, kind, out, n, true); }
    int emitters() const { return numEmitters_; }
    int emitterCells(int* cxcy, int cap) const;  // the kept emitters' count; the first min(count, cap) result cells (cx, cy) into cxcy
    bool copyEmitterTrace(int emitter, float* outT);  // the emitter's pressure at every step of the last run
    bool copyResults(float* res8, float* delay);
    // the block [r0, r0 + nr) x [c0, c0 + nc) of the result map (AoS records) and of the onset map, row-major nr x nc
    bool copyResultsBlock(int r0, int c0, int nr, int nc, float* res8, float* delay);
    // device -> caller-provided (pinned) host buffers, asynchronously on the solver's stream
    bool copyResultsAsync(float* res8Host);
    // The block of the result map the LAST run could have changed: the history window, clipped to the map (everything
    // outside it keeps its earlier values, except the listener direction, which is the unit vector from the listener
    // to the cell: Analyzer.cpp:64-68,365-391,415-428).  publishWindowAsync packs that block as nr*nc AoS records
    // and copies it to hostDst (pinned, >= windowCapacity() records) on the solver's stream.
    struct WindowBlock {
        int r0 = 0, c0 = 0, nr = 0, nc = 0;  // result-map cells [r0, r0+nr) x [c0, c0+nc)
        float lx = 0, lz = 0;                // the run's listener position, metres
    };
    size_t windowCapacity() const;  // records: upper bound of nr*nc for any listener position
    void windowExtent(int* rows, int* cols) const;  // upper bounds of nr and nc for any listener position
    void setRunTap(RunTap* t) { tap_ = t; }  // (nullptr: none; the caller syncs the solver before it lets the tap go)
    // overlap = true: only the pack runs on the solver's stream; the device -> host copy goes to a second stream, so that the
    // NEXT run's launches need not wait for it (the live module's loop); waitPublish() then waits for that copy alone.
    bool publishWindowAsync(float* hostDst, WindowBlock* info, bool overlap = false);
    bool waitPublish();
    // pinned host memory for the buffers above
    static void* hostAlloc(size_t bytes);
    static void hostFree(void* p);
    bool impulseResponse(int cx, int cy, float* out3T);
    // the same as T reference Cells {f32 pr, vx, vy; i16 b, by} (PvTypes.h:106-121; recorded at FDTD.cpp:226-230 with
    // the b / by the cell had during the run)
    bool impulseResponseCells(int cx, int cy, void* out16T);
    bool copyFields(float* pr, float* vx, float* vy);
    bool setFields(const float* pr, const float* vx, const float* vy);
    bool copyHistoryPlane(int t, float* pr);
    // the inverse (a test seam): NX x NY floats into the stored cells of plane t; waits for a run in flight, leaves every
    // analysis map "not computed" and the run's results, onsets, tileFirst and query records alone
    bool setHistoryPlane(int t, const float* pr);
    // Per-cell analysis maps of the last completed run (pv_solver_maps.cpp; include/planeverb_amd.h names the records): nine
    // kinds (AnalysisKind), each one pass over the run's history on stream_, synchronised before computeX returns; *ms
    // (optional) = its device time.  A kind's records stay valid until the next run, geometry, boundary or layer change, or a
    // change of the kind's own setting.  Refused on slabs, on sparse-emitter solvers, without an onset map and before a run has
    // completed.  copyAnalysisBlock: nr x nc records of the kind's width, NaN where the cell has no onset in that run;
    // analysisAt: the record of the cell getOutput reads, NaNs for a position off the map
    bool copyAnalysisBlock(AnalysisKind k, int r0, int c0, int nr, int nc, float* out);
    bool analysisAt(AnalysisKind k, float ex, float ez, float* out);
    // Room metrics (pv_metrics.hip): records of ten floats
    bool computeRoomMetrics(float* ms);
    // Decay times (pv_decay.hip): EDT, T20, T30 off the backward-integrated curve of the history; records of eight floats
    bool computeDecayTimes(float* ms);
    // Lateral energy fraction and early-sound direction (pv_lateral.hip): vx, vy of every reached cell re-derived from its
    // history through the 80 ms window; records of eleven floats
    bool computeLateralFraction(float* ms);
    // Directional echogram (pv_echogram.hip): energy and flux per time slot after each cell's onset, for the slots set here;
    // records of 1 + 3 nSlots floats.  setEchogram: the caller has validated the setting (pv_echogram.h echogramSlotOk,
    // 0 <= nSlots <= kEchogramMaxSlots); nSlots = 0 clears and frees; waits for a run in flight
    bool setEchogram(float slotSeconds, int nSlots);
    int echogramSlots(float* slotSeconds, int* slotSteps) const;
    bool computeEchogram(float* ms);
    // Directional energy lobes (pv_lobes.hip): the energy per time window after each cell's onset, split over the travel
    // directions +x, -x, +y, -y; records of 1 + 5 nW floats.  setLobeWindows: the caller has validated the edges (pv_lobes.h
    // lobesEdgeSteps); nEdges = 0 restores the default; waits for a run in flight
    bool setLobeWindows(const float* edgesSeconds, int nEdges);
    int lobeWindows(float* edgesSeconds, int* edgeSteps) const;
    bool computeLobes(float* ms);
    // Echo criterion (pv_echo.hip): speech and music variant from one forward pass over the history; records of ten floats;
    // refused where the sampling rate gives a speech lag below one step
    bool computeEchoCriterion(float* ms);
    // Band metrics (pv_bands.hip): decay times and clarity per octave or third-octave band set here; n records of twelve floats
    // per cell.  setBands: the caller has validated the centres (pv_bands.h bandsError); n = 0 clears and frees; waits for a run
    // in flight
    bool setBands(const float* centreHz, int n, int fraction);
    int bands(float* centreHz, int cap, int* fraction) const;
    bool bandCoefs(float* out10n);
    bool computeBandMetrics(float* ms);
    // Modulation (pv_modulation.hip): the modulation transfer function at 14 modulation frequencies and the modulation transfer
    // index per band of setBands; n records of fifteen floats per cell; a change of bands or of the modulation frequencies
    // invalidates them.  setModulationFrequencies: the caller has validated hz14 (pv_modulation.h modulationFreqsError); nullptr
    // restores the default; waits for a run in flight
    bool setModulationFrequencies(const float* hz14);
    void modulationFrequencies(float* hz14) const;
    bool computeModulation(float* ms);
    // Spectrum (pv_spectrum.hip): transfer functions at the bins set here; n records of three floats per cell.
    // setSpectrumBins: the caller has validated hz (pv_spectrum.h spectrumBinsError); n = 0 clears and frees; waits for a run
    // in flight
    bool setSpectrumBins(const float* hz, int n);
    int spectrumBins(float* hz, int cap) const;
    bool spectrumSource(float* out3n);
    bool computeSpectrum(float* ms);
    // Waterfall (pv_solver_waterfall.cpp, pv_waterfall.hip; include/planeverb_amd.h names the record): the cumulative spectral decay
    // of up to kWaterfallMaxReceivers receivers of the last completed run at the bins and slices set here.  setWaterfall: the
    // caller has validated the setting (pv_waterfall.h waterfallSettingError); n = 0 clears and frees; waits for a run in flight;
    // uploads the tables.  computeWaterfall: positions mapped as setOutputQueries maps them -- on a sparse-emitter solver xyz =
    // nullptr, nPos = 0 and the receivers are the registered emitters, their samples the emitter traces; synchronised before it
    // returns, *ms (optional) = its device time.  The records stay valid until the next run, geometry, boundary or layer change,
    // change of the setting or, in sparse-emitter mode, of the emitters; they and the nine map kinds do not touch each other
    bool setWaterfall(const float* hz, int n, float sliceSeconds, int nSlices);
    int waterfall(float* hz, int cap, float* sliceSeconds, int* sliceSteps, int* nSlices) const;
    int waterfallRecordFloats() const;  // -1 without a setting
    bool computeWaterfall(const float* xyz, int nPos, float* ms);
    bool copyWaterfall(float* out, int nPos);
    // Source arrays (pv_solver_arrays.cpp, pv_arrays.hip; the definition: pv_arrays.h): the combined response of weighted, delayed
    // members at the listener, up to kArraysMax arrays of up to kArrayMembersMax members, mixed on the device from the history (in
    // sparse-emitter mode: the emitter traces) of the last completed run; the onset of every response; and the selected record
    // kinds of every response through the query record kernels (recordLaneOfMix).  setArrays: nArrays = 0 clears and frees; a
    // refused or failed call leaves the setting of before; waits for a run in flight.  computeArrays is synchronised before it
    // returns, *ms (optional) = its device time.  What it leaves stays valid until the next run, geometry, boundary or layer
    // change, a successful setter, a change of bands / modulation frequencies / bins while a dependent kind is selected or, in
    // sparse-emitter mode, a change of the emitters
    bool setArrays(const int* count, int nArrays, const float* members5, int interp);
    int arrays(int* count, int cap, int* interp) const;
    int arrayTapsOf(int array, int* memberIndex, int* delaySteps, float* weight, int cap);  // the tap count, -1: no such array
    bool setArrayRecords(unsigned timeKinds, unsigned spectralKinds);
    void arrayRecordKinds(unsigned* timeKinds, unsigned* spectralKinds) const;
    int arrayRecordFloats(int family, unsigned kind);  // -1: not one kind of the family, or its setting is missing
    bool computeArrays(float* ms);
    bool copyArrayResponse(int array, float* outT);
    bool arrayOnsets(float* out, int nArrays);
    bool arrayRecords(int family, unsigned kind, float* out, int nArrays);
    // Auralisation (pv_solver_aural.cpp, pv_aural.hip; the definition: pv_aural.h): the responses of up to kAuralMaxReceivers
    // receivers of the last completed run -- positions mapped as setOutputQueries maps them, on a sparse-emitter solver the
    // registered emitters' traces, or the array responses computeArrays left -- resampled to the rate set here, and their
    // convolution with dry signals and mix.  setAuralisation: rate = 0 clears and frees; a refused or failed call leaves the
    // setting of before; waits for a run in flight.  The computes are synchronised before they return, *ms (optional) = their
    // device time.  Responses and outputs stay valid until the next run, geometry, boundary or layer change, change of the setting,
    // in sparse-emitter mode of the emitters, and for the array source until the array responses go; new responses drop the outputs
    bool setAuralisation(int rate, int zeroCrossings, float beta);
    bool auralisation(int* rate, int* zeroCrossings, float* beta, int* L, int* K) const;  // false: no setting
    int auralTapsOf(int* first, float* w, int capN);                                       // L, -1 without a setting
    bool computeAuralResponses(int source, const float* xyz, int nPos, float* ms);
    bool copyAuralResponse(int r, float* outL);
    bool setAuralForm(int form);
    bool auralise(const float* signals, int nSignals, int N, const int* route, const float* gain, float* ms);
    bool copyAuralOutput(int r, float* outM);
    bool copyAuralMix(float* outM);
    // The reductions over zones: pv_solver_zones.cpp.
    // Zone statistics (pv_zones.hip; include/planeverb_amd.h PvAmdZoneStat): a label per result cell, 0 = no zone, 1 .. nZones;
    // computeZoneStats reduces the valid map of one kind to nZones x planes records on the device -- no host copy of the map,
    // nothing cached, no kind touched.  setZones: the caller has validated the labels (pv_zones.h zoneLabelsError); nullptr / 0
    // clears; waits for a run in flight; the labels survive runs and geometry changes.  zoneStatPlanes: the planes of a kind under
    // the current settings, -1 where its setting is missing
    bool setZones(const unsigned char* labels, int nZones);
    int zones(unsigned char* labels) const;
    int zoneStatPlanes(AnalysisKind k) const;
    bool computeZoneStats(AnalysisKind k, void* out, int cap, float* ms, int* count);
    // Zone decay (pv_zone_decay.hip; include/planeverb_amd.h PvAmdZoneDecay): the ensemble decay curve of every zone of setZones
    // from the last completed run's history and onset map, and the decay times read off it -- out = nZones records, etc / edc
    // (either may be nullptr) = nZones x T doubles.  Nothing cached, no map, plan or run chain touched; waits for a run in flight.
    // zoneDecayChunkSlots: the time slots one pair of launches covers under the current zones (T and more: all of them at once)
    bool computeZoneDecay(int align, void* out, int cap, double* etc, double* edc, float* ms, int* count);
    int zoneDecayChunkSlots() const;
    // Sparse-emitter solvers keep a ring, not the history: there the ABSOLUTE curves are accumulated INSIDE every run enqueued
    // while setZoneCurves(true) holds (pv_zone_decay.hip, the rows kernel over the ring source, per accumulate pass), and
    // computeZoneDecay(ABSOLUTE) reads them -- members pass, one copy, the host finish.  Needs zones; waits for a run in flight;
    // allocates on enable (nZones x T doubles and the row sums of one chunk of steps), frees on disable; while enabled the tiles
    // that hold a labelled cell stay in the ring and record for the whole run, as the emitters' tiles do, and the zones cannot be
    // cleared.  The curves carry the stamp of the run they were enqueued with: a call after setZones / setZoneCurves and before
    // the next run is refused
    bool setZoneCurves(bool on);
    bool zoneCurves() const;
    // Sparse-emitter solvers, the per-cell maps of the zones (pv_zone_maps.hip): while a kind of setZoneMaps (kZoneMapRoomMetrics |
    // kZoneMapSpectrum) is selected, every run accumulates that kind's record of every LABELLED cell inside the run, off the ring, in
    // the kind's own map (maps_: planes x histPlane_ floats, 10 resp. 3 n planes; unlabelled cells quiet NaN) -- bit for bit what
    // computeRoomMetrics / computeSpectrum give on a solver that keeps its history.  The read-backs of the two kinds and
    // computeZoneStats of them then work on that map.  Needs zones (and bins for the spectrum); waits for a run in flight; allocates
    // on select, frees on deselect; while a kind is selected the tiles that hold a labelled cell stay in the ring, as with the curves,
    // and the zones (the bins) cannot be cleared.  A map carries the stamp of the run it was enqueued with: a read after
    // setZoneMaps / setZones / setSpectrumBins and before the next run is refused
    bool setZoneMaps(unsigned kinds);
    unsigned zoneMaps() const;
    // Zone band decay (pv_zone_band_decay.hip; include/planeverb_amd.h PvAmdZoneBandDecay): the same curve per band of setBands,
    // off the band-filtered history -- out = nZones x nBands records, etc / edc (either may be nullptr) = nZones x nBands x T
    // doubles.  Nothing cached, no map, plan or run chain touched; the bands are read at the call; waits for a run in flight.
    // zoneBandDecayChunks: the chunks of (zone, band) pairs the pass takes under the current zones and bands (0: none set), the
    // slots (T: time is never cut) and the bands of one chunk
    bool computeZoneBandDecay(int align, void* out, int cap, double* etc, double* edc, float* ms, int* count);
    int zoneBandDecayChunks(int* slots, int* bands) const;
    bool copyPulse(float* out);
    bool copyMaterial(uint8_t* beta, float* R);
    bool freeFieldEnergyAt(int cellX, int cellY, int n, float r, float* out);
    // streaming mode: the cells whose wet gain / RT60 are wanted (world positions -> result cells)
    bool setEmitters(const float* xyz, int n);

private:
    Solver() = default;
    bool init(const GridSpec& spec, int device, const SolverOptions& opt);
    bool applyGeometry();
    bool computeEfree();
    // Which path a run takes (pv_core.h planRun): caps_ is resolved by init, plan_ describes the run in flight / the last run.
    // beginRun is the head of every run, whoever drives its launches: the pending run synced, the geometry applied, the run
    // planned and its parameters staged (prepareDyn), the per-run counters reset, the planes as the plan's form needs them.
    PathCaps caps_;
    RunPlan plan_;
    bool beginRun(PathRun::Kind kind, int lcx, int lcy, bool withPulse, float lx, float lz);
    bool enqueueRun(int lcx, int lcy, float lx, float lz);
    bool enqueueStreamingRun(float lx, float lz);
    void enqueueResidentRun();
    void launchResidentRun(int tileRows, const int* win);
    bool enqueueSmallGridRun();
    bool enqueueGraphRun();
    bool enqueueSteps(int firstStep, int nsteps, bool withPulse, bool record, bool fromZero = false);
    StepArgs baseStepArgs(bool withPulse, bool record) const;
    void setLaunchArgs(StepArgs& a, int t0, int k, bool firstOfRun, int li) const;
    bool prepareDyn(int lcx, int lcy, bool withPulse);
    void enqueueBeginRun(bool resetTiles);
    bool zeroPlanesIfNeeded();
    AnalyzeArgs analyzeArgs(float lx, float lz) const;
    // Far cells lazily: a run resets only the previous and the current window block; the far cells'
    // listener direction is materialised for whole-map read-backs and computed in closed form by the output gathers
    bool lazyFar_ = false;
    struct Block {
        int r0 = 0, c0 = 0, nr = 0, nc = 0;
    };
    Block curWindow() const;        // the history-window block of the result map of the run prepared last
    Block farWin_;                  // window block of the last ANALYSED run (the far cells lie outside it)
    bool farDirValid_ = true;       // the direction planes hold the far cells' directions of that run
    // Near box (AnalyzeArgs::box): two sets of four device words, the reached cells' bounding box of the run analysed last
    // (nearBox_ + 4 nearPar_) and of the one before it; PLANEVERB_AMD_NEAR_BOX=0 keeps the window-wide passes
    int* nearBox_ = nullptr;
    int nearPar_ = 0;
    bool useNearBox_ = false;
    bool nearBoxValid_ = false;     // the last analysed run went through the near-box passes
    // Timings of a resident-kernel run without event packets between its kernels (an event record on the stream is a barrier
    // packet: ~7 us of bubble in front of the next kernel, three of them per 0.3 ms run): the run's first kernel, the analysis'
    // first kernel and the run's last kernel write the 100 MHz counter into three pinned words, sync() takes the differences
    unsigned long long* stampsHost_ = nullptr;
    bool stampTimed() const { return (plan_.path == StepPath::Resident || plan_.path == StepPath::Window) && stampsHost_; }  // the run in flight is timed that way
    bool labelsValid_ = false;      // labelDev_ holds the air components of the current material plane
    int lastReached_ = -1;          // cells with an onset in the last run read back (-1: none yet): AnalyzeArgs::rt60Tile
    FarInfo farInfo() const;
    bool ensureFarDirections();
    void enqueueAnalysis(float lx, float lz);
    Solver* carryFrom_ = nullptr;  // for the run being enqueued
    RunTap* tap_ = nullptr;
    void enqueueTap();  // behind the run's last kernel
    bool fail(const std::string& what);
    bool hipOk(hipError_t e, const char* what);
    template <typename Tp>
    bool dalloc(Tp** p, size_t count, bool zero);

    GridSpec g_;         // always the WHOLE grid
    // what this solver owns of it (a whole grid: x0_ = 0, lNX_ = g_.NX, lgx_ = g_.gx)
    int x0_ = 0;         // first cell-array row
    int tileRow0_ = 0;   // = x0_ / rxi_
    int lNX_ = 0;        // cell-array rows owned (the last slab also owns the ghost row)
    int lgx_ = 0;        // result-map rows owned
    int ntxG_ = 0, histTilesXG_ = 0;  // the whole grid's tile rows / history-window tile rows
    bool isSlab() const { return opt_.slabCount > 1; }
    int globalWindowTileRow0(int lcx) const;
    float* histAbove_ = nullptr;  // [T][histPitch]: pressure history of the row above this slab (from the neighbour)
    float* histEdge_ = nullptr;   // [T][histPitch]: this slab's last row, for the neighbour below
    Geometry geo_{};
    SolverOptions opt_;
    int device_ = 0;
    int K_ = 4, rxi_ = 32, wi_ = 56;
    int T_ = 0;
    hipStream_t stream_ = nullptr;
    hipStream_t stream2_ = nullptr;        // general-tile kernels run here, concurrently with the air kernel
    bool lastRunBatched_ = false;          // the last run was a member of a batch of several
    std::vector<hipStream_t> auxStreams_;  // PVA_OPT_AUX_STREAMS
    std::vector<hipEvent_t> airDone_, genDone_;  // per-launch cross-stream dependencies (no timing)
    int stepWhich_ = 4;                    // launchStep's `which` of the merged launch (applyGeometry: | kStepGeneralPacked)
    QueueClaim queue_;                     // stream_'s hardware queue, apart from the other solvers' (Solver::init)
    bool redealMainStream() { return queue_.replace(&stream_); }  // (before any run: nothing of the old stream is in flight)
    hipEvent_t forkEv_ = nullptr;
    hipEvent_t anaEv_[2] = {nullptr, nullptr};  // enqueueAnalysis: onsets known -> stream2_, decay times done -> stream_
    // captured launch schedule of one run (reset + all step launches on both streams), replayed per run
    hipGraph_t graph_ = nullptr;
    hipGraphExec_t graphExec_ = nullptr;
    int graphCap_ = -1;  // general-list capacity the graph was captured with
    bool captureLossInjected_ = false;  // (test hook, buildGraph)
    bool buildGraph(int cap);
    void dropGraph();
    bool enqueueResetAndSteps();
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t pubEv_[2] = {nullptr, nullptr};  // window block packed / copied to the host (publishWindowAsync, overlap form)
    bool pubCopyPending_ = false;
    long long deviceBytes_ = 0;
    std::string err_;

    // HBM
    float* pr_[2] = {nullptr, nullptr};
    float* vx_[2] = {nullptr, nullptr};
    float* vy_[2] = {nullptr, nullptr};
    int cur_ = 0;  // which set holds the current fields
    FaceCoef* coef_ = nullptr;      // face coefficients + beta of every padded cell (pv_device.h)
    float* matDev_ = nullptr;       // material plane: NaN = air cell, else the wall cell's admittance Y
    float* pulseDev_ = nullptr;
    float* hist_ = nullptr;
    long long histPlane_ = 0;
    int histRows_ = 0, histPitch_ = 0, histTilesX_ = 0, histTilesY_ = 0;
    uint8_t* nz_[2] = {nullptr, nullptr};  // per-tile non-zero flags, ping-pong per launch
    int* tileFirst_ = nullptr;
    uint8_t* tileClass_ = nullptr;
    uint8_t* tileDead_ = nullptr;   // per tile: all-wall interior (skipped by runs that start from zero fields)
    int* deadCount_ = nullptr;
    int numDead_ = 0;
    bool planesDirty_ = false;      // the field planes may hold non-zero values inside dead tiles
    // Reach-bounded runs (PVA_OPT_REACH_BOUND) write only the tiles of their launches' windows, so both buffer sets must hold
    // zeros everywhere else when one starts (clearReachPlanes).  sweptDirty_: a run of another path has left fields anywhere
    // since the last full clear; reachRect_: tile rows [0], +[1] x tile columns [2], +[3] = the last reach-bounded run's final
    // window (the windows of a run only grow), the only place that run left non-zero values.
    bool sweptDirty_ = true;
    int reachRect_[4] = {0, 0, 0, 0};
    bool clearReachPlanes(const int* win);  // win: the window of a window run, nullptr: reach-bounded launches
    void setReachArgs(StepArgs& a, int t0);
    int* generalList_ = nullptr;
    int* generalCount_ = nullptr;
    DynParams* dynDev_ = nullptr;
    int* errFlag_ = nullptr;
    int residentBudget_ = 0;        // blocks of the resident kernel this device holds at once x 3/4 (init)
    int* labelDev_ = nullptr;       // AnalyzeArgs::labels (grids of up to kLabelMaxCells array cells), re-made by applyGeometry
    std::vector<int> labelHost_;
    bool makeLabels();
    unsigned* fusedCtl_ = nullptr;  // FusedArgs::ctl
    bool useFused_ = false;
    int* unitList_ = nullptr;     // AnalyzeArgs::unitList: histPlane / 64 + 1 ints
    int* activeCount_ = nullptr;  // cells with an onset in the last analysis (chooses the RT60 kernel on the device)
    float* res_ = nullptr;   // 8 SoA result planes (see AnalyzeArgs::res)
    float* res8_ = nullptr;  // AoS copy for whole-map read-backs, allocated and packed on demand
    float* win8_ = nullptr;  // AoS staging of the window block (publishWindowAsync), allocated on demand
    bool packResults();
    float* delay_ = nullptr;
    // streaming analysis state
    int ring_ = 0;             // history planes allocated (T_ when not streaming)
    int halfRing_ = 0;         // streaming: steps per accumulate pass (the ring holds two such halves)
    hipEvent_t streamEv_[4] = {nullptr, nullptr, nullptr, nullptr};  // stepDone[2], accDone[2]
    hipStream_t openStream_ = nullptr;  // sparse-emitter mode: the open half tiles of a sweep, beside the merged launch
    hipEvent_t openEv_[4] = {nullptr, nullptr, nullptr, nullptr};  // classified[2], openDone[2] (alternating sweeps)
    bool openPending_ = false;
    void joinOpen(int li);
    int* sOnset_ = nullptr;
    float* sState_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // Edry, fluxX, fluxY, vx, vy
    uint8_t* tileOpen_ = nullptr;   // per tile: history still wanted (streaming mode)
    uint8_t* tileMarks_ = nullptr;  // scratch of one accumulate pass
    uint8_t* tileEmit_ = nullptr;   // per tile: holds a registered emitter or, while the zone curves are enabled, a labelled cell
    // forward sums inside the stencil (pv_stream.h)
    bool streamFuse_ = false;
    uint8_t* classStream_ = nullptr;   // per-launch tile classes (open air tiles masked out of the merged launch)
    uint8_t* ringOpen_ = nullptr;      // per-launch `tileOpen` of the step kernels: open RING tiles only
    uint8_t* cellsOpen2_ = nullptr;    // per tile half: a dry window is still open
    int* openList_ = nullptr;
    int* idleHost_ = nullptr;          // pinned, 2 ints (one per ring half): every fused tile has closed for good
    bool fuseIdle_ = false;            // ... as the host has seen it: the rest of the run is plain merged launches
    ClassifyArgs classifyArgs(const StepArgs& a, int li, bool withPulse) const;
    int* ringList_ = nullptr;          // the tiles the accumulate pass still serves (general list + emitter tiles), per run
    int* ringHost_ = nullptr;          // pinned staging of it
    int numRing_ = 0;
    std::vector<uint8_t> emTilesHost_; // host copy of tileEmit_
    std::vector<uint8_t> emitterTilesHost_;  // the registered emitters' part of it (setEmitters; uploadTileEmit adds the zones')
    int* openCount_ = nullptr;         // two counters, alternating from launch to launch
    int* emCells_ = nullptr;
    float* emTrace_ = nullptr;
    int numEmitters_ = 0, emCap_ = 0;
    // emitter records: the emitters' result cells as the record launches read them (pinned, emCap_ entries), the record traces
    // (allocated while a kind is selected; recTraceCap_ floats) and their layout under the current emitters and kinds
    long long* emRecCells_ = nullptr;
    float* recTrace_ = nullptr;
    size_t recTraceCap_ = 0;
    int recCols_ = 0;
    bool recVel_ = false;
    bool streamedOnce_ = false;  // a sparse-emitter run has been enqueued: emTrace_ holds a run's traces
    bool fitRecTrace(int emitters, unsigned timeKinds, unsigned spectralKinds);  // (no run in flight)
    // resident kernel (pv_resident.hip)
    unsigned* resFlags_ = nullptr;     // ntiles epoch counters + 1 abort word
    int residentHeld_ = 0;             // blocks of the device's resident budget held by the run in flight
    // one-XCD mode of the resident kernel (grids of up to kResidentXcdMaxTiles tiles): hand-off through one XCD's L2
    bool xcdOk_ = true;                // false once a launch found fewer blocks on its XCD than tiles (errFlag 4)
    int xcdTarget_ = 0;                // this solver's XCD (solvers take turns, so that pipelined solvers do not share one)
    int xcdHeld_ = 0;                  // blocks of that XCD's budget held by the run in flight
    int runTiles_ = 0;                 // tiles of the resident launch in flight (the grid's or the window's): its claim counter is flag word runTiles_ + 1
    bool xcdWindowOk_ = false;         // window runs may take the mode: init's throw-away window launch passed its claim check
    bool probeWindow_ = false;         // ... which is the run being enqueued (windowFor answers with tile (0, 0))
    bool repeating_ = false;           // sync() is repeating a run that was given up (it clears as a reach-bounded run would)
    int lastLcx_ = 0, lastLcy_ = 0;    // (a run given up by the claim check is repeated in the placement-independent mode)
    void releaseResident();
    // Resident window: on the large-grid tile a run whose listener's air component is walled in and small goes out
    // as ONE launch of the resident kernel over the tile window around that component instead of T / K reach-bounded launches
    bool windowOff_ = false;           // a window run was given up (errFlag 3): reach-bounded runs until the geometry changes
    int resFlagWords_ = 0;             // words of resFlags_
    struct EnclosureRec {
        Enclosure e;
        std::vector<int> cells;        // ascending cell indices of the component (or of the part walked before the give-up)
    };
    std::vector<EnclosureRec> enclosures_;  // answers of findEnclosure for this geometry (dropped when a cell changes between air and wall)
    const Enclosure* enclosureOf(int lcx, int lcy);
    bool windowFor(int lcx, int lcy, int win[4]);
    ResidentArgs residentArgs(const int* win) const;  // win = nullptr: the grid's own tiles
    void enqueueWindowRun(const int win[4]);
    float* scratch_ = nullptr;  // max(3T, NX*NY) floats
    enum class LastRun { None, Failed, Ok };  // Failed: in flight, or ended in error (a run is Ok once sync() has seen it through)
    LastRun lastRun_ = LastRun::None;
    // The analysis maps (pv_solver_maps.cpp): one record per kind.  dev = `planes` planes of histPlane_ floats, a cell's record
    // at its offset inside a history plane, (re)allocated by the kind's compute when the wanted plane count differs; dyn = the
    // window of the run the records belong to; host = a copy fetched by the first read-back.  valid is cleared for every kind by
    // invalidateAnalysisMaps (a new run, a geometry, boundary or layer change) and for one kind by a change of its setting; no
    // computation touches another kind's record.  All passes are timed with the one event pair: each synchronises the stream and
    // reads the time before it returns, under queue_.lockUse()
    struct AnalysisMap {
        float* dev = nullptr;
        int planes = 0;
        bool valid = false, hostValid = false;
        DynParams dyn{};
        std::vector<float> host;
    };
    AnalysisMap maps_[kAnalysisKinds];
    hipEvent_t mapEv_[2] = {nullptr, nullptr};
    void invalidateAnalysisMaps() {
        for (AnalysisMap& m : maps_) m.valid = false;
        wfValid_ = false;  // (the waterfall's records have the maps' lifetime)
        arValid_ = false;  // (and so has what computeArrays left)
        auRespValid_ = auOutValid_ = false;  // (and the auralisation's responses and outputs)
    }
    void dropAnalysisMap(AnalysisKind k, bool freeDev);  // a changed setting: records invalid, the device storage freed on request
    bool analysisSettingPresent(AnalysisKind k) const;
    bool analysisReadable(AnalysisKind k);  // the missing-setting refusal, then the not-computed refusal
    bool analysisHipOk(AnalysisKind k, hipError_t e, const char* step);
    // A compute pass: begin = every refusal (`refusal`: the kind's own, nullptr where its precondition holds), the run in flight
    // waited for, the storage at `planes` planes, `prepare` (stream work in front of the timed interval), the start event;
    // the caller enqueues its launches on stream_; end = the stop event, the error check, the wait, *ms, the record valid
    struct AnalysisPass {
        AnalysisKind kind;
        std::unique_lock<std::recursive_mutex> inUse;
        AnalyzeArgs a;
        float* dev;
    };
    bool beginAnalysisPass(AnalysisKind k, int planes, const char* refusal, AnalysisPass* p, bool (Solver::*prepare)() = nullptr);
    bool endAnalysisPass(AnalysisPass& p, float* ms);
    bool fetchAnalysisMap(AnalysisKind k);
    // echogram (pv_echogram.h): the slot length as given and in steps, the slots; planes: n, then e, ix, iy of slot j at 1 + 3 j ..
    float echoSeconds_ = 0.f;
    int echoSteps_ = 0, echoSlots_ = 0;
    // lobes (pv_lobes.h): the window edges as given (the default until some are set); planes: n, then E, XP, XN, YP, YN of
    // window j at 1 + 5 j ..
    float lobeEdges_[7] = {0.01f, 0.08f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int lobeEdgeCount_ = 2;
    // band metrics (pv_bands.h): the centres, their fraction and the 10 float32 coefficients per band on the host (the kernel takes
    // them as arguments); planes: band j at 12 j .. 12 j + 11
    std::vector<float> bandHz_, bandCoefs_;
    int bandFraction_ = 1;
    // modulation (pv_modulation.h): the 14 modulation frequencies (the default until some are set) and their twiddle table on the
    // device (kModTablePad zero rows, then T rows of 28 floats padded to 32), uploaded by ensureModTable after a change; planes:
    // band j at 15 j .. 15 j + 14
    float modHz_[14] = {0.63f, 0.8f, 1.0f, 1.25f, 1.6f, 2.0f, 2.5f, 3.15f, 4.0f, 5.0f, 6.3f, 8.0f, 10.0f, 12.5f};
    float* modTab_ = nullptr;
    bool modTabValid_ = false;
    // spectrum (pv_spectrum.h): the bins, their tables c / s [T * n] and source values (sre, sim, spow per bin) on the host; the
    // passes the bins are dealt to (specPasses_: a slice of the bins, the register block that takes it, where its table slice
    // starts in specTab_); planes: re, im, level of bin j at 3 j .. 3 j + 2
    struct SpecPass {
        int bin0, bins, block;
        size_t tabOff;
    };
    std::vector<float> specHz_, specCos_, specSin_, specSource_;
    std::vector<SpecPass> specPasses_;
    float* specTab_ = nullptr;
    float* specPow_ = nullptr;
    // waterfall (pv_waterfall.h): the setting; on the device from the setter on the tables as pv_waterfall.hip reads them (per
    // block of 64 bins: kWaterfallTablePad zero rows and T rows of 64 {cos, sin} pairs -- 2 x 4 x T x n bytes for n a multiple of
    // 64: 104 MB at T = 25 432 and 512 bins) and the source powers, the cell and receiver tables (kWaterfallMaxReceivers entries);
    // from the first compute on the records, wfCount_ x F floats (at most 34.6 MB), reallocated when the count or F changes
    std::vector<float> wfHz_;
    float wfSeconds_ = 0.f;
    int wfSteps_ = 0, wfSlices_ = 0;
    float* wfTab_ = nullptr;
    float* wfPow_ = nullptr;
    long long* wfCells_ = nullptr;
    void* wfRx_ = nullptr;  // WaterfallRx (pv_launch.h)
    float* wfRec_ = nullptr;
    size_t wfRecFloats_ = 0;
    int wfCount_ = 0;
    int wfCus_ = 0;  // the device's compute units: how many receivers a wave takes (pv_launch.h waterfallBlockFor)
    bool wfValid_ = false;
    void freeWaterfall();
    // source arrays (pv_arrays.h): the setting as given and its expanded tap table (tap.row = the member's index in the setting's
    // order); on the device from the setter on the taps, their offsets per array, the members' sources and rows, the mix planes
    // [T][arP_] (arP_ = the arrays rounded up to 64: 26 MB at T = 25 432 and 256 arrays) and the onsets; from the first compute
    // with a kind selected on the record block.  Nothing of it exists while no arrays are set
    std::vector<int> arCount_;
    std::vector<float> arMembers_;     // five floats per member
    std::vector<long long> arCells_;   // per member: its result cell
    std::vector<int> arTapOffHost_;    // nArrays + 1
    std::vector<int> arTapRow_, arTapDelay_;
    std::vector<float> arTapW_;
    int arInterp_ = 0, arP_ = 0;
    void* arTaps_ = nullptr;  // ArrayTap (pv_arrays.h)
    int* arTapOff_ = nullptr;
    long long* arSrc_ = nullptr;
    void* arRows_ = nullptr;  // ArrayRow (pv_launch.h)
    float* arMix_ = nullptr;
    float* arOnsets_ = nullptr;
    float* arRec_ = nullptr;
    size_t arRecCap_ = 0;
    unsigned arKinds_[kRecordFamilies] = {0u, 0u};
    // what the last computeArrays left: the stamp, the onsets and the records on the host, a kind's block of nArrays x floats at its offset
    bool arValid_ = false;
    unsigned arRunKinds_[kRecordFamilies] = {0u, 0u};
    int arRunFloats_[kRecordFamilies][kQueryRecordKinds] = {};
    size_t arRunOffset_[kRecordFamilies][kQueryRecordKinds] = {};
    std::vector<float> arOnsetsHost_, arRecHost_;
    void freeArrays();
    std::string arrayKindsRefusal(unsigned timeKinds, unsigned spectralKinds) const;
    void invalidateArrays(unsigned spectralKinds) {  // a changed band, modulation or bin setting
        if (arKinds_[kRecSpectral] & spectralKinds) arValid_ = false;
    }
    unsigned long long arStamp_ = 0;  // counts the computeArrays that went through: what auralised array responses are held to
    // auralisation (pv_aural.h): the setting and its tables on the host as given out (auW_ row-major [L][K]); on the device from
    // the setter on first[L] and the weights transposed [K][L] -- L * K * 4 + L * 4 bytes --, the receivers' cells and rows
    // (kAuralMaxReceivers entries); from computeAuralResponses on the gathered samples [R][T] and the responses [R][L]; from
    // auralise on the signals, route and gains and the outputs [R][M] and the mix [M].  Nothing of it exists while no setting does
    int auRate_ = 0, auZ_ = 0, auL_ = 0, auK_ = 0;
    float auBeta_ = 0.f;
    std::vector<int> auFirst_;
    std::vector<float> auW_;
    int* auFirstDev_ = nullptr;
    float* auWT_ = nullptr;
    long long* auCells_ = nullptr;
    void* auRows_ = nullptr;  // ArrayRow (pv_launch.h)
    float* auGather_ = nullptr;
    float* auResp_ = nullptr;
    float* auSig_ = nullptr;
    int* auRoute_ = nullptr;
    float* auGain_ = nullptr;
    float* auOut_ = nullptr;
    float* auMix_ = nullptr;
    size_t auGatherCap_ = 0, auRespCap_ = 0, auSigCap_ = 0, auOutCap_ = 0, auMixCap_ = 0;
    int auCount_ = 0, auSource_ = 0, auM_ = 0, auForm_ = 0;
    unsigned long long auArStamp_ = 0;
    bool auRespValid_ = false, auOutValid_ = false;
    void freeAuralisation();
    bool auralResponsesValid() const { return auRespValid_ && (auSource_ == 0 || (arValid_ && arStamp_ == auArStamp_)); }
    // zone statistics (pv_zones.h): the labels on the device and as given, and the pass's scratch -- per plane in flight, zone and
    // result row one ZoneRow and one double (48 bytes), the planes dealt in chunks that keep it within kZoneScratchBytes (one
    // plane's where that is more), then the nZones x planes records; grown on demand, kept.  The zone-decay pass uses the same
    // scratch: per time slot in flight, zone and result row one double, the slots dealt in chunks within the same bound, then
    // nZones x T doubles of curves and the zones' member rows and records.  The zone-band-decay pass too: per (zone, band) pair in
    // flight and result row T doubles, the pairs dealt in chunks within the same bound (one pair's where that is more), then nZones x
    // nBands x T doubles of curves and the member rows and records
    bool growZoneScratch(size_t need);
    // A zone pass (pv_solver_zones.cpp), after the pattern of AnalysisPass.  beginZonePass = the refusals every call makes ahead of
    // the lock (a slab; by flag: a sparse-emitter solver, a solver without onset map), the lock, the run in flight waited for.  The
    // call then lists its remaining refusals in its own order (zoneRefuse; zoneRunRefusal: the two about the last run).  A curve pass
    // goes on with beginZoneCurves = the scratch carved, the arguments (zoneCurveArgs: window and common fields from the last run),
    // the first event, the members pass; the caller enqueues its launches with p.c; endZoneCurves = the second event, the error
    // check, curves and members copied, the wait, *ms.  Zone statistics keep their own scratch and tail
    enum : unsigned { kZoneNeedsHistory = 1, kZoneNeedsOnsets = 2 };
    struct ZonePass {
        const char* name;  // the prefix of the refusals, the label of a failed HIP call
        std::unique_lock<std::recursive_mutex> inUse;
        ZoneCurveArgs c;
        std::vector<double> etcHost;  // the curves where the caller takes none
        std::vector<ZoneMembers> members;
    };
    bool beginZonePass(ZonePass* p, const char* name, unsigned flags);
    bool zoneRefuse(const ZonePass& p, const std::string& what);
    const char* zoneRunRefusal() const;
    bool beginZoneCurves(ZonePass* p, size_t rowsBytes, size_t etcBytes, double* runCurves = nullptr);
    bool endZoneCurves(ZonePass& p, size_t curves, double** etc, float* ms);
    bool startZoneTimer();
    bool zoneHipOk(const ZonePass& p, hipError_t e, const char* step);
    ZoneWindow zoneWindow(const DynParams& dyn, int tilesX, int tilesY) const;
    ZoneCurveArgs zoneCurveArgs() const;
    static constexpr size_t kZoneScratchBytes = 32u << 20;
    unsigned char* zoneLabels_ = nullptr;
    std::vector<unsigned char> zoneHost_;
    int zoneCount_ = 0;
    unsigned char* zoneScratch_ = nullptr;
    size_t zoneScratchBytes_ = 0;
    // sparse-emitter mode, curves enabled (setZoneCurves): the curves of the last run enqueued with them (nZones x T), the row sums
    // of one chunk of an accumulate pass's steps -- a scratch of their own: the pass runs on stream2_, the calls above on stream_
    // --, the tiles that hold a labelled cell, the labels' bounding box, and two stamps: zoneCurveSetting_ counts the changes of
    // labels or switch, zoneCurveRun_ is its value when the last run was enqueued (0: that run accumulated no curves)
    bool deriveZoneCurves();  // (everything below from zoneHost_ / zoneCount_; uploads the tile plane)
    bool disableZoneCurves();
    void freeZoneCurves();
    bool uploadTileEmit();    // tileEmit_ = the emitters' tiles, united with the zones' while the curves or a map kind are enabled
    // the zones' tiles and box for whoever is enabled -- the curves or a map kind; cleared where neither is -- and the tile plane
    // uploaded: setZones, setZoneCurves and setZoneMaps all come through here, so none drops another's tiles
    bool rebuildZoneTiles();
    // the map kinds (setZoneMaps): the storage is maps_[kMapRoomMetrics / kMapSpectrum].dev; the list of labelled tiles on the
    // device; per kind (0: room metrics, 1: spectrum) a stamp as the curves': zoneMapSetting_ counts the changes of selection, labels
    // or bins, zoneMapRun_ is its value when the last run was enqueued (0: that run accumulated no such map)
    bool deriveZoneMaps(unsigned kinds);  // storage at the current plane counts, NaN everywhere, the tile list; bumps the stamps
    void dropZoneMaps(unsigned kinds);    // the kinds' storage freed and their selection cleared
    bool zoneMapReadable(AnalysisKind k);
    ZoneMapArgs zoneMapArgs(const AnalyzeArgs& a) const;
    unsigned zoneMapKinds_ = 0;
    int* zoneMapTiles_ = nullptr;
    int zoneMapTileCount_ = 0, zoneMapTileCap_ = 0;
    unsigned long long zoneMapSetting_[2] = {0, 0}, zoneMapRun_[2] = {0, 0};
    bool zoneCurvesOn_ = false;
    double* zoneCurveEtc_ = nullptr;
    double* zoneCurveRows_ = nullptr;
    size_t zoneCurveEtcBytes_ = 0, zoneCurveRowsBytes_ = 0;
    std::vector<uint8_t> zoneTilesHost_;  // per tile of the grid (geo_.ntx x geo_.nty); empty while disabled
    int zoneBox_[4] = {0, -1, 0, -1};     // first / last labelled row, first / last labelled 64-block
    int zoneCurveChunk_ = 0;
    unsigned long long zoneCurveSetting_ = 0, zoneCurveRun_ = 0;
    size_t scratchCount_ = 0;

    // pinned host staging
    DynParams* dynHost_ = nullptr;
    float* outHost_ = nullptr;  // 8 floats the output-gather kernel writes straight into host memory
    int* statusHost_ = nullptr; // the words the last kernel of a run leaves here: error flag, two cell counts, resident claims, silent cells
    bool statusQueued_ = false; // ... for the run in flight (else sync() copies them back)
    void enqueueRunStatus();
    long long* qCellsHost_ = nullptr;  // kMaxQueries result-cell indices (-1 = outside the map), device-visible
    float* qOutHost_ = nullptr;        // kMaxQueries x 8 floats
    int numQueries_ = 0;
    void enqueueQueries();
    // In-run query records, one RecordSet per family: what differs between the families as data (how its refusals start, how they
    // name the kind bits and the selector, the number of kinds), the selected kinds, the pinned block -- blockQueries queries at the
    // selected kinds' largest settings -- and the stamp of the run whose records it holds: the layout that run was enqueued with,
    // pending until sync() has seen the run through
    static constexpr int kRecordKindsMax = kQueryRecordKinds > kQuerySpectralKinds ? kQueryRecordKinds : kQuerySpectralKinds;
    struct RecordSet {
        const char *prefix, *bits, *selector;
        int nKinds;
        unsigned kinds = 0;
        float* host = nullptr;
        int blockQueries = 0;
        enum class Run { None, Pending, Ok } run = Run::None;
        unsigned runKinds = 0;
        int runQueries = 0;
        int runOffset[kRecordKindsMax] = {}, runFloats[kRecordKindsMax] = {};
    };
    RecordSet recs_[kRecordFamilies] = {{"query records: ", "PVA_QREC_*", "PvAmdSetQueryRecords", kQueryRecordKinds},
                                        {"spectral records: ", "PVA_QSPEC_*", "PvAmdSetQuerySpectralRecords", kQuerySpectralKinds}};
    // the record queries' own pinned cell table (setRecordQueries)
    long long* rqCellsHost_ = nullptr;
    int rqCap_ = 0, numRecQueries_ = 0;
    int recordQueryCount() const {  // of the table the records follow
        return opt_.streaming ? numEmitters_ : numRecQueries_ > 0 ? numRecQueries_ : numQueries_;
    }
    const long long* recordCells() const { return opt_.streaming ? emRecCells_ : numRecQueries_ > 0 ? rqCellsHost_ : qCellsHost_; }
    AnalyzeArgs recordArgs() const;  // of the record launches: the history, or the record traces in its place
    int recordFloatsOf(RecordFamily f, int k, bool largest = false) const;  // per query of kind bit k; -1: its setting is missing
    const char* recordKindsRefusal(RecordFamily f, unsigned kinds) const;  // of the kinds' settings, nullptr where none
    // (emitters: the call came through the emitter records' entry points, which serve sparse-emitter solvers and those alone)
    std::string selectRefusal(RecordFamily f, unsigned kinds, bool emitters) const;  // what needs no device; empty: none
    bool selectRecords(RecordFamily f, unsigned kinds, bool emitters = false);
    bool swapRecordBlock(RecordFamily f, unsigned kinds, int queries);
    bool growRecordBlock(RecordFamily f, int queries);
    int recordFloats(RecordFamily f, unsigned kind);
    void stampRecords(RecordFamily f, int nq, const bool* on, int* offset, int* floats);
    bool readRecords(RecordFamily f, unsigned kind, float* out, int n, bool emitters = false);
    void invalidateRecords(RecordFamily f, unsigned kinds = ~0u) {  // the block's records are those of other queries or settings
        if (recs_[f].kinds & kinds) recs_[f].run = RecordSet::Run::None;
    }
    bool ensureModTable();               // the modulation twiddle table on the device (no run in flight)
    void enqueueQueryRecords();          // behind a run's analysis, in front of its last kernel (nothing when no kind is selected)
    void enqueueQuerySpectralRecords();  // directly behind enqueueQueryRecords (nothing when no kind is selected)
    int* listHost_ = nullptr;
    int listCap_ = 0;
    // row-streaming air segments (pv_seg.h): rebuilt for every run (they avoid the tiles around the listener)
    int patchBlocks_ = 0;      // its grid: one workgroup per CU, a multiple of 8
    long long* patchTrace_ = nullptr;  // development aid (PV_PATCH_TRACE)
    int segWMax_ = 0;          // tile columns a segment can span
    SegDesc* segHost_ = nullptr;  // pinned
    SegDesc* segList_ = nullptr;  // device
    int segCap_ = 0, numSeg_ = 0;
    void buildSegments(int listed);

    // host state
    MaterialPlane mat_;
    std::vector<float> matHost_;     // host copy of matDev_
    std::vector<uint8_t> betaHost_;  // Cell::b as of the last applyGeometry() (= during the last run)
    std::vector<uint8_t> byHost_;  // Cell::by as of the last applyGeometry() (= during the last run)
    std::vector<float> pulse_;
    std::vector<int> wallTiles_;
    std::vector<uint8_t> tileClassHost_;
    int numGeneral_ = 0;
    int launchCap_ = 0;  // general-list entries the general kernel's grid is sized for
    bool geometryDirty_ = true;
    float edgeR_[4] = {0.f, 0.f, 0.f, 0.f};  // setGridBoundary
    bool boundaryDirty_ = false;             // edgeR_ changed since the last applyGeometry (no flood fill: air is unchanged)
    int layerW_[4] = {0, 0, 0, 0};  // setEdgeLayer
    bool layerSplit_ = false;       // the split-field model (else unsplit)
    double layerR0_ = kEdgeLayerR0;  // the tables' design reflection
    bool layerDirty_ = false;       // layerW_, layerSplit_ or layerR0_ changed since the last applyGeometry
    float* px_[2] = {nullptr, nullptr};  // the split model's x part of the pressure, one padded plane per buffer set (one
                                         // allocation, made by the first applyGeometry with the split model; 0 outside layers)
    float* layerTab_ = nullptr;     // LayerArgs::rowTab (4 x rows) then colTab (4 x pitch)
    int* layerList_ = nullptr;      // the layer tiles (capacity: every tile)
    int numLayer_ = 0;
    std::vector<float> layerTabHost_;
    std::vector<int> layerListHost_;
    bool classifyLayer();           // applyGeometry: layer tiles off the air / general lists, onto layerList_; tables uploaded
    float efree_ = 0.f;
    DynParams dynCur_{};
    bool dynValid_ = false;
    float lastLx_ = 0, lastLz_ = 0;

    // geometry table (GeometryManager.cpp)
    std::vector<Box> boxTable_;
    std::vector<uint8_t> boxUsed_;
    std::vector<int> boxFree_;

    // shape layer (pv_shapes.h); shapesActive_ from the first shape on
    bool shapesActive_ = false;
    std::vector<Shape> shapeTable_;
    std::vector<int> shapeSeq_;                 // sequence number of the slot's last add / update, -1 = empty slot
    std::vector<int> shapeFree_;
    int shapeSeqNext_ = 0;
    std::vector<int> shapeDirty_;               // cell rectangles (x0, x1, y0, y1) to recompose at the next applyGeometry
    void markShapeDirty(int id);
    bool composeShapes(int aabbLo, int aabbHi, bool* airChanged);
    float* matBaseDev_ = nullptr;               // AABB-layer material (matDev_ holds the composed one)
    void* shapeDev_ = nullptr;                  // DevShape table + bin lists + dirty bins, one allocation
    size_t shapeDevBytes_ = 0;
    std::vector<unsigned char> shapeStage_;     // host image of that allocation
    std::vector<uint8_t> compBeta_;             // composed beta / R (copyMaterial)
    std::vector<float> compR_;
    // what composeShapes leaves for composeMirrors, which fills the host mirrors behind the geometry sync
    struct ShapeMirrorJob {
        std::vector<uint8_t> dirty;             // per bin
        std::vector<int> order, binStart, binList;
        std::vector<int> x0, x1, y0, y1;        // the table entries' cell bounds
        int nby = 0;
    } mirror_;
    void composeMirrors(bool* airChanged);

    // mesh layer (pv_mesh.h); meshActive_ from the first mesh on (which also turns the shape layer's planes on: the shape
    // compose then reads matMeshDev_ as its base)
    struct MeshSlot {
        int seq = -1;                           // sequence number of the last add / update / transform, -1 = empty slot
        int nv = 0, nt = 0, mode = 0;
        float R = 0.f, r = 0.f;
        bool hasM = false;
        float m[12] = {};
        unsigned char* dev = nullptr;           // vertices, triangles, segments, valid marks, bit plane: one allocation
        size_t devBytes = 0, oTris = 0, oSeg = 0, oValid = 0, oBits = 0;
        bool reslice = false;                   // slice and rasterise again at the next applyGeometry
        int bounds[4] = {0, 0, 0, 0};           // cells covered as of the last applyGeometry
    };
    bool meshActive_ = false, meshPending_ = false, meshAllDirty_ = false;
    float sliceH_ = 0.f;
    std::vector<MeshSlot> meshTable_;
    std::vector<int> meshFree_;
    int meshSeqNext_ = 0;
    std::vector<int> meshDirty_;                // cell rectangles to re-derive from the AABB layer (removed meshes' bounds)
    float* matMeshDev_ = nullptr;               // AABB layer overwritten by the meshes: the shape compose's base
    uint8_t* meshOwnerDev_ = nullptr;           // per cell: 0 = AABB layer, else 1 + the id of the covering mesh
    void* meshBoundsDev_ = nullptr;             // kMeshMax MeshBounds
    std::vector<int> meshBoundsHost_;
    std::vector<uint8_t> meshOwnerHost_;        // read-back of meshOwnerDev_ (the mirrors' base under the shapes)
    long long meshTrisTotal() const;
    void meshFreeSlot(MeshSlot& m);
    bool composeMeshes(int aabbLo, int aabbHi);

    // row bands: band b covers tile rows [bandRow_[b], bandRow_[b+1])
    int nb_ = 1;
    std::vector<int> bandRow_;
    std::vector<hipStream_t> bandStream_;  // [0] = stream_
    std::vector<hipEvent_t> bandEv_;       // 2 per band: sweep parity
    std::vector<int> bandListOff_, bandListCount_;
    DynParams* dynBandsDev_ = nullptr;
    DynParams* dynBandsHost_ = nullptr;
    StepArgs bandStepArgs(const StepArgs& a, int b) const;

    std::vector<hipEvent_t> kev_;  // 3 events per step launch when opt_.timeKernels
    int kevUsed_ = 0;
    SolverTimings tim_;
    bool pendingTimings_ = false;
    bool loopTimed() const { return plan_.path == StepPath::Launches && plan_.kind == PathRun::Run; }  // ev_[3] was recorded between the reset and the first step launch of this run
};

template <typename Tp>
bool Solver::dalloc(Tp** p, size_t count, bool zero) {  // (here: pv_solver.cpp, pv_solver_maps.cpp and pv_solver_zones.cpp all allocate)
    const size_t bytes = count * sizeof(Tp);
    if (!hipOk(hipMalloc((void**)p, bytes), "hipMalloc")) return false;
    deviceBytes_ += (long long)bytes;
    if (zero && !hipOk(hipMemsetAsync(*p, 0, bytes, stream_), "hipMemsetAsync")) return false;
    return true;
}

}  // namespace pva
