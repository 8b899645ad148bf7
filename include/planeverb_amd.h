/* planeverb_amd.h -- C-ABI of libplaneverb_amd.so (MI355X / gfx950 build of Planeverb's FDTD + IR-analysis path)
 *
 * Part 1 is the reference's own flat C-ABI, symbol for symbol -- the functions Unity P/Invokes from
 * ProjectPlaneverbUnityPlugin (reference: ProjectPlaneverb/PlaneverbUnityPluginAPI/PlaneverbUnity.cpp:12-135,
 * C# mirror PlaneverbContext.cs:25-60).  A build of the Acoustics module that loads this library instead of
 * ProjectPlaneverbUnityPlugin.dll needs no source change.  threadExecutionType 0 (pv_CPU) and 1 (pv_GPU, the value
 * the C# enum already defines, PlaneverbConfig.cs:23-29) are accepted alike and BOTH run on the HIP device: this
 * library has no CPU path and fails loudly without a HIP device.
 *
 * Part 2 (PvAmd*) is an extension: a handle-based, synchronous batch interface to the same solver, used by the
 * benchmarks, the parity tests and the multi-GPU sharding layer.  It replaces nothing in the reference; it exposes
 * what the reference's classes Grid / FreeGrid / Analyzer expose to its own Context (PvContext.cpp:63-94).
 *
 * Plain C types only.  No C++ exception crosses this boundary: errors are reported by return code
 * (0 = ok) and PvAmdLastError().
 */
#ifndef PLANEVERB_AMD_H
#define PLANEVERB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define PVA_EXPORT __attribute__((visibility("default")))
#else
#define PVA_EXPORT
#endif

/* ------------------------------------------------------------------------------------------------------------
 * Part 1 -- reference C-ABI
 * ---------------------------------------------------------------------------------------------------------- */

/* PlaneverbUnity.cpp:66-76 (returned BY VALUE, 8 floats) */
typedef struct PlaneverbOutput {
    float occlusion;        /* dry/obstruction gain; -1 (PV_INVALID_DRY_GAIN) = invalid, PvTypes.h:80 */
    float wetGain;
    float rt60;
    float lowpass;
    float directionX;
    float directionY;
    float sourceDirectionX;
    float sourceDirectionY;
} PlaneverbOutput;

/* PlaneverbUnity.cpp:12-20 (no-ops) */
PVA_EXPORT void UnityPluginLoad(void* unityInterfaces);
PVA_EXPORT void UnityPluginUnload(void);

/* PlaneverbUnity.cpp:25-40 -> Planeverb::Init (PvContext.cpp:25-32).  Invalid config (res < 275, size 0,
 * tempFileDir NULL: PvContext.cpp:101-107) leaves the module un-initialised instead of throwing.
 * gridBoundaryType (PvTypes.h:32-36): 0 = pv_AbsorbingBoundary, the reference's grid edges; 1 = pv_ReflectingBoundary, absorption
 * R = 1 (a rigid edge) on all four sides of the grid (PvAmdSetGridBoundary).  The reference stores the value and ignores it.
 * Any other value runs absorbing edges, as before, with one warning on stderr. */
PVA_EXPORT void PlaneverbInit(float gridSizeX, float gridSizeY, int gridResolution, int gridBoundaryType,
                              char* tempFileDir, int maxThreadUsage, int threadExecutionType);
/* PlaneverbUnity.cpp:42-46 */
PVA_EXPORT void PlaneverbExit(void);
/* PlaneverbUnity.cpp:48-52 ; -1 when the module is not initialised (EmissionManager.cpp:13) */
PVA_EXPORT int PlaneverbEmit(float x, float y, float z);
/* PlaneverbUnity.cpp:54-58 */
PVA_EXPORT void PlaneverbUpdateEmission(int id, float x, float y, float z);
/* PlaneverbUnity.cpp:60-64 */
PVA_EXPORT void PlaneverbEndEmission(int id);
/* PlaneverbUnity.cpp:78-92 -> Planeverb::GetOutput (FDTD.cpp:16-58); O(1), no lock, no device access (lock-free: a
 * reader repeats its 32-byte copy only if the once-per-iteration publish step ran meanwhile).
 * Sparse-emitter mode (configurations whose T-step pressure history does not fit the device, e.g. 25 m at 16 kHz; chosen
 * by PlaneverbInit by itself, forced by the environment variable PLANEVERB_AMD_LIVE_STREAMING=1): occlusion, lowpass and
 * both directions are valid for every cell as usual; wetGain and rt60 are computed for the cells of the emitters that
 * existed when the iteration started (an emitter added or moved to another cell gets them one iteration later). */
PVA_EXPORT PlaneverbOutput PlaneverbGetOutput(int emissionID);
/* PlaneverbUnity.cpp:94-107 ; -1 when not initialised (GeometryManager.cpp:20) */
PVA_EXPORT int PlaneverbAddGeometry(float posX, float posY, float width, float height, float absorption);
/* PlaneverbUnity.cpp:109-123 */
PVA_EXPORT void PlaneverbUpdateGeometry(int id, float posX, float posY, float width, float height,
                                        float absorption);
/* PlaneverbUnity.cpp:125-129 */
PVA_EXPORT void PlaneverbRemoveGeometry(int id);
/* PlaneverbUnity.cpp:131-135 */
PVA_EXPORT void PlaneverbSetListenerPosition(float x, float y, float z);

/* Extensions next to the geometry calls (no reference counterpart): oriented boxes and convex polygons, the shape model of
 * PvAmdAddShape below.  Their ids are a table of their own (not the AABB ids).  Queued like the AABB calls and applied at the
 * same iteration boundary, in call order.  Add returns -1 for a refused shape (PvAmdLastError says why); Update and Remove of
 * an unknown id, or Update with a refused shape, do nothing. */
PVA_EXPORT int PlaneverbAddOrientedGeometry(float posX, float posY, float width, float height, float axisX, float axisY,
                                            float absorption);
PVA_EXPORT void PlaneverbUpdateOrientedGeometry(int id, float posX, float posY, float width, float height, float axisX,
                                                float axisY, float absorption);
PVA_EXPORT void PlaneverbRemoveOrientedGeometry(int id);
PVA_EXPORT int PlaneverbAddPolygonGeometry(const float* xy, int n, float absorption);
PVA_EXPORT void PlaneverbUpdatePolygonGeometry(int id, const float* xy, int n, float absorption);
PVA_EXPORT void PlaneverbRemovePolygonGeometry(int id);
/* Round and concave objects, the models of PvAmdAddDisc / PvAmdAddWallPath / PvAmdAddPolygon below, in the same id table and
 * the same queue as the two calls above (any Remove...Geometry of this group removes a shape of any kind). */
PVA_EXPORT int PlaneverbAddDiscGeometry(float posX, float posY, float radius, float absorption);
PVA_EXPORT void PlaneverbUpdateDiscGeometry(int id, float posX, float posY, float radius, float absorption);
PVA_EXPORT void PlaneverbRemoveDiscGeometry(int id);
PVA_EXPORT int PlaneverbAddWallPathGeometry(const float* xy, int n, float radius, float absorption);
PVA_EXPORT void PlaneverbUpdateWallPathGeometry(int id, const float* xy, int n, float radius, float absorption);
PVA_EXPORT void PlaneverbRemoveWallPathGeometry(int id);
PVA_EXPORT int PlaneverbAddConcavePolygonGeometry(const float* xy, int n, float absorption);
PVA_EXPORT void PlaneverbUpdateConcavePolygonGeometry(int id, const float* xy, int n, float absorption);
PVA_EXPORT void PlaneverbRemoveConcavePolygonGeometry(int id);
/* Triangle meshes, the model of PvAmdAddMesh below (slice, coverage, composition, refusals), in an id table of their own.  The
 * vertex data is copied into a store the module owns at the Add call, which may fail cleanly with -1 (PvAmdLastError); the
 * changes are queued with the others and applied at the iteration boundary in call order, to both live solvers.
 * PlaneverbSetSliceHeight sets the world height of the slice (0 at Init): a Unity caller passes the listener's y; the module does
 * not follow the listener by itself.  A non-finite height or transform entry is ignored (PvAmdLastError says so). */
PVA_EXPORT int PlaneverbAddMeshGeometry(const float* verts, int nv, const int* tris, int nt, float absorption, int mode,
                                        float radius);
PVA_EXPORT void PlaneverbSetMeshGeometryTransform(int id, const float m12[12]);
PVA_EXPORT void PlaneverbRemoveMeshGeometry(int id);
PVA_EXPORT void PlaneverbSetSliceHeight(float h);
/* Extension: the absorption of the four grid edges (PvAmdSetGridBoundary: xMin = side 0, xMax = 1, zMin = 2, zMax = 3), queued
 * like the geometry calls and applied to both live solvers at the same iteration boundary.  A non-finite value is refused
 * (nothing changes; PvAmdLastError says why). */
PVA_EXPORT void PlaneverbSetGridBoundary(float xMin, float xMax, float zMin, float zMax);
/* Extension: graded absorbing layers of widths xMin (side x = 0), xMax (x = gx), zMin (y = 0), zMax (y = gy) in cells
 * (PvAmdSetEdgeLayer), queued like PlaneverbSetGridBoundary and applied to both live solvers at the same iteration boundary.
 * Refused (nothing changes; PvAmdLastError says why) in sparse-emitter mode and for widths PvAmdSetEdgeLayer refuses. */
PVA_EXPORT void PlaneverbSetEdgeLayer(int xMin, int xMax, int zMin, int zMax);
/* Extension: the same widths with the split-field model (PvAmdSetEdgeLayerSplit) at r0 = PVA_EDGE_LAYER_SPLIT_R0, queued and
 * refused like PlaneverbSetEdgeLayer; PlaneverbSetEdgeLayer afterwards selects the unsplit model again. */
PVA_EXPORT void PlaneverbSetEdgeLayerSplit(int xMin, int xMax, int zMin, int zMax);

/* Extensions to the live module (not in the reference's flat ABI) */
/* One sample of an impulse response as the reference stores it (Cell, PvTypes.h:106-121: 16 bytes) */
typedef struct PlaneverbCell {
    float pr, vx, vy;
    short b;  /* beta of the cell during the run (0 = wall / ghost row or column) */
    short by; /* never read by the solver; carried for layout compatibility (Grid.cpp:93-108,241-242,281-290) */
} PlaneverbCell;
/* Planeverb::GetImpulseResponse (Planeverb.h:47, FDTD.cpp:60-79) for the live module: the impulse response of the
 * last COMPLETED iteration at the cell holding world position (x, z) -- (int)(x/dx), (int)(z/dx) -- as reference
 * Cells.  Writes min(capacity, T) cells to `out` and returns T (the response length; call with capacity 0 to size the
 * buffer), 0 for a position outside the cell array, -1 when the module is not initialised / on error.  Waits for the
 * iteration in flight (the reference reads the cube while the worker rewrites it); a debugging call, like upstream. */
PVA_EXPORT int PlaneverbGetImpulseResponse(float x, float y, float z, PlaneverbCell* out, int capacity);

/* Emission records: the per-cell analysis records of Part 2 (room metrics, decay times, lateral fraction, echogram, echo
 * criterion, lobes -- PVA_QREC_*, PvAmdSetQueryRecords) for the cells of the LIVE EMITTERS, by emission id.  `kinds` is a mask of
 * PVA_QREC_*.  While any kind is selected, the worker latches, at the start of every iteration, the cells of the emitters alive at
 * that moment -- in ascending id, ended ids skipped, the first PVA_RECORD_QUERIES_MAX (1024) DISTINCT cells inside the result map,
 * sorted -- and that iteration computes the selected kinds for them with ONE launch inside its run (64 cells per wave), straight
 * into pinned host memory.  The records become readable in the same publish step as the iteration's outputs: a caller that reads
 * PlaneverbGetOutput and a record between two publishes (an unchanged PlaneverbIterationCount) sees one iteration.
 *   The three setters validate at the call -- PlaneverbSetEmissionEchogram by PvAmdSetEchogram's rules, PlaneverbSetEmissionLobeWindows
 * by PvAmdSetLobeWindows' rules (nEdges = 0: the default windows), PlaneverbSetEmissionRecords by PvAmdSetQueryRecords' (an
 * unknown bit; PVA_QREC_ECHOGRAM with no slots set; the sampling-rate floors of the echo criterion and the default lobe windows)
 * -- and return 0, or -1 with nothing changed and PvAmdLastError "emission records: ...".  They are refused while the module is
 * down and in sparse-emitter mode (PlaneverbIsStreaming: "the full pressure history is not kept").  An accepted change is queued
 * with the geometry changes and takes effect at an iteration boundary, on both solvers of the pipelined loop at the same one; the
 * readers below describe the PUBLISHED iteration, so a change shows there one to three iterations later.  kinds = 0, the default,
 * switches the records off and frees the solvers' pinned blocks: nothing is launched, latched or copied, and an iteration's
 * launches are exactly those of a module that never called this.
 *   PlaneverbEmissionRecordKinds: the kinds the published iteration carries (0 when the module is down or nothing is published).
 * PlaneverbEmissionRecordFloats: floats of ONE kind in the published iteration (10, 8, 11, 1 + 3 nSlots, 10, 1 + 5 nWindows), -1 if
 * it does not carry the kind.  PlaneverbEmissionRecordCells: the distinct cells it served, -1 when the module is down.
 *   PlaneverbGetEmissionRecord reads the emitter's CURRENT position, maps it to a result cell as PlaneverbGetOutput does and looks
 * the cell up in the published iteration's table.  It is lock-free like PlaneverbGetOutput: no device access, no lock, and no
 * allocation.  It returns
 *    1: the record was written -- bit for bit what PvAmdGet<Kind> gives at that position after PvAmdCompute<Kind> on the same run;
 *    0: PlaneverbEmissionRecordFloats(kind) quiet NaNs were written: an id that was never issued or has ended; a position off the
 *       map; a cell that is not in the table (the emitter was added or moved to another cell since the latch -- it gets its record
 *       one iteration later, the rule sparse-emitter mode has for wet gain and RT60 -- or the cell lies beyond the cap); a cell
 *       without an onset in that run;
 *   -1: nothing was written: the module is down; `kind` is not exactly one known bit; the published iteration does not carry the
 *       kind (not selected, or not in effect yet); `out` is NULL; `capacity` is below PlaneverbEmissionRecordFloats(kind). */
PVA_EXPORT int PlaneverbSetEmissionRecords(unsigned kinds);
PVA_EXPORT int PlaneverbSetEmissionEchogram(float slotSeconds, int nSlots);
PVA_EXPORT int PlaneverbSetEmissionLobeWindows(const float* edgesSeconds, int nEdges);
PVA_EXPORT unsigned PlaneverbEmissionRecordKinds(void);
PVA_EXPORT int PlaneverbEmissionRecordFloats(unsigned kind);
PVA_EXPORT int PlaneverbEmissionRecordCells(void);
PVA_EXPORT int PlaneverbGetEmissionRecord(int emissionID, unsigned kind, float* out, int capacity);
/* Load a .pv scene (PlaneverbSandbox/src/Editor/Editor.cpp:245-281) into the live module; returns #boxes or <0 */
PVA_EXPORT int PlaneverbLoadScene(const char* pvPath);
/* Number of completed (published) simulation iterations since Init (an iteration = FDTD + analysis, PvContext.cpp:74-93).  The
 * count changes in the publish step itself: PlaneverbGetOutput and PlaneverbGetEmissionRecord calls made between two reads of the
 * same count all answer from that one iteration. */
PVA_EXPORT long long PlaneverbIterationCount(void);
/* Block until at least `count` iterations have completed, or timeoutMs elapsed; returns the iteration count */
PVA_EXPORT long long PlaneverbWaitIterations(long long count, int timeoutMs);
/* 1 if the module is initialised and its simulation worker is alive (0 after a worker error: PvAmdLastError) */
PVA_EXPORT int PlaneverbIsRunning(void);
/* why the simulation worker stopped ("" while it runs / when the module is down); valid until this thread's next call */
PVA_EXPORT const char* PlaneverbWorkerError(void);
/* 1 if the live module runs in the sparse-emitter mode (see PlaneverbGetOutput), else 0 */
PVA_EXPORT int PlaneverbIsStreaming(void);

/* ------------------------------------------------------------------------------------------------------------
 * Part 2 -- batch solver handle (extension)
 * ---------------------------------------------------------------------------------------------------------- */

typedef struct PvAmdSolver PvAmdSolver;

typedef struct PvAmdInfo {
    int gx, gy;             /* (int)m_gridSize: result map is gx*gy, cell array (gx+1)*(gy+1)  (Grid.cpp:48-53) */
    int T;                  /* response length in samples (Grid.cpp:55) */
    int fs;                 /* sampling rate (Grid.cpp:390-396) */
    int res;
    float dx, dt;
    float efree;            /* FreeGrid energy at 1 m (FreeGrid.cpp:71-94) */
    int device;
    int stepsPerLaunch;     /* K: time steps fused per kernel launch */
    int tileRows, tileCols; /* interior cells per wave tile */
    int pitch, rows;        /* padded device array geometry (floats per row, rows) */
    int histRows, histPitch;/* history window geometry */
    int numGeometry;
    long long deviceBytes;  /* bytes of HBM held by this solver */
    int streamFuse;         /* streaming analysis: 1 = the forward sums of air tiles advance inside the step kernel (PVA_OPT_STREAM_FUSE as resolved for this grid and tile) */
    int residentKernel;     /* 1 = runs go out as ONE launch of the resident kernel (PVA_OPT_RESIDENT_KERNEL as resolved for this grid and tile) */
} PvAmdInfo;

typedef struct PvAmdTimings {
    float fdtdMs;           /* HIP-event time of the T-step loop (incl. IR record) of the last run */
    float analysisMs;       /* HIP-event time of both analysis kernels of the last run */
    float geometryMs;       /* material upload + face-code build, last time it ran */
    float stepKernelMs;     /* fdtdMs / number of step launches */
    int stepLaunches;
    float airKernelMs;      /* mean duration of one air-tile step-kernel launch (PVA_OPT_TIME_KERNELS) */
    float generalKernelMs;  /* mean duration of one general-tile step-kernel launch */
    int airLaunches, generalLaunches;
    float stepLoopMs;       /* HIP-event time of the back-to-back step launches alone (fdtdMs minus the field reset);
                               0 when the run was replayed from a hipGraph */
    int reachedCells;       /* cells with an onset in the last run's analysis (Analyzer.cpp:146-165): the impulse responses that
                               were actually analysed -- the others leave at once */
    int activeCells;        /* cells of the history window's tiles that ever held a non-zero value: what the analysis kernels
                               look at (an upper bound of reachedCells) */
    int silentCells;        /* air cells among them whose whole history stayed below the audible threshold (no onset: Analyzer.cpp:160-165);
                               many of them make the next run's analysis look for an audible sample before anything else */
} PvAmdTimings;

/* option keys for PvAmdSetOption (must be set before the first run)
 *
 * Run length (PVA_OPT_NUM_STEPS, numSteps).  Any numSteps > 0 is a run, and every record below means at that T what its
 * definition says with T = numSteps: no length is refused, clamped or special-cased, and nothing is extrapolated past the
 * record.  A RUN SHORTER than a definition's window ends the window at T:
 *   - the eight outputs: the dry window [onset, min(onset + nDry, T)) and the wet window behind it are cut by T; a cell with
 *     fewer than nDry + 2 + nCut steps between its onset and T is a late-onset cell (every reached cell of a run that short):
 *     samples past T read as zero, the decay-time regression ends at T - nCut, which may lie below its start or below step 0, and
 *     rt60 is what the reference's formula gives for the sums over that range -- +inf over an empty one, NaN over a single
 *     step (0 / 0) --, nothing special-cased.  A run of one step reaches no cell: every onset is FLT_MAX;
 *   - decay times, band metrics, zone decay: tEnd = T - tailN may be <= t0, or <= 0 when T <= tailN; then no step enters a fit,
 *     every range is incomplete (NaN), depth is NaN, and E0 is still the sum over [t0, T);
 *   - the 50 / 80 ms limits: where t0 + n50 >= T the late energy l50 is +0.0f, so c50 is what IEEE gives for e50 / 0 and d50 is 1
 *     (l80 likewise); the lateral fraction sums over [onset, min(onset + n80, T)); the echo criterion's late windows are empty;
 *   - echogram slots, lobe windows and waterfall slices that begin at or past T hold their +0.0f sums (a waterfall level of
 *     -inf, and `slices` counts the others); one cut by T holds its partial sums;
 *   - an array member's taps past T - 1 read +0.0f; a delay of T steps or more is refused by PvAmdSetArrays, at every T;
 *   - sparse-emitter mode accumulates in passes of min(roundUp(T, K), 8 K) steps and returns the same bits as a solver that
 *     keeps its history, whether T is less than one pass, exactly one or two, or one step more.
 * An EXTENDED RUN (numSteps above the grid's own T) injects nothing after the grid's T -- the pulse table is zero from there --
 * and goes on stepping and recording: planes 0 .. T_grid - 1, the onset map, and every output whose windows end below T_grid
 * are those of the default run; every sum defined "to T" (E0, rt60's range, tEnd, the spectrum, the modulation) runs to
 * numSteps.  tests/test_host_run_lengths.py and tests/test_gpu_run_lengths.py hold the host restatements and the kernels to
 * this at 39 lengths from 1 to 500 steps. */
enum {
    PVA_OPT_DENSE_HISTORY = 1, /* 1 = record every tile every step (no zero-tile skipping) */
    PVA_OPT_NUM_STEPS = 2,     /* override T (extension); 0 = reference value */
    PVA_OPT_SKIP_ANALYSIS = 3, /* 1 = PvAmdRun does the FDTD loop only */
    PVA_OPT_USE_GRAPH = 4,     /* replay a run from a captured hipGraph: 0 = auto (launch-bound small grids), 1 = always, 2 = never */
    PVA_OPT_STEPS_PER_LAUNCH = 5, /* K: time steps fused per kernel launch (tuning) */
    PVA_OPT_TILE_ROWS = 6,     /* interior rows of a wave tile (tuning; must pair with a compiled K) */
    PVA_OPT_NO_FREE_GRID = 7,  /* 1 = skip the free-field run (efree = 0; stencil-only use) */
    PVA_OPT_TIME_KERNELS = 8,  /* N > 0: HIP events around every Nth step-kernel launch (per-kernel durations) */
    PVA_OPT_TILE_ORDER = 9,    /* air-kernel workgroup->tile map: 0 linear, 1 XCD band of tile rows walked row-major, 2 the band column-major, 3 XCD strip of tile columns walked row-major (vertical halo neighbours stay in the XCD's L2), >= 4 sub-bands of that many tile rows; default: 3 for grids of >= 4500 tiles (3072^2 and up), else 1 */
    PVA_OPT_SMALL_GRID_KERNEL = 10, /* the kernel that keeps the whole grid in one CU's LDS for all T steps: 0 = auto (grids of up to 1536 array cells, where it beats the replayed tile-kernel graph: 28^2 ... 38^2), 1 = whenever the grid fits one CU (up to ~110^2), 2 = never */
    PVA_OPT_PACKED_MATH = 11,  /* air-tile kernel arithmetic: 1 = packed f32 (default), 0 = scalar f32 */
    PVA_OPT_STREAMING_ANALYSIS = 12, /* 1 = sparse-emitter mode: ring history + incremental analysis (see PvAmdSetEmitters) */
    PVA_OPT_STREAM_ROWS = 13,  /* N > 0: the air part of the grid is advanced by about N row-streaming segments per sweep (a wave streams down a 256-column strip, K time levels in flight) instead of one wave per air tile; tile configurations (8, 40) and (12, 36) only, ignored elsewhere and with slabs / row bands / graphs / streaming analysis.  Bit-identical; experimental: slower than the tile kernels at 4096^2.  Default 0 = off */
    PVA_OPT_MERGED_LAUNCH = 14, /* 1 (default) = general + air tiles in one launch per K steps; 0 = two kernels, two streams */
    PVA_OPT_ROW_BANDS = 16,    /* B > 1: every K-step sweep is launched as B bands of tile rows on B HIP streams; band b of sweep n+1 waits only for bands b-1, b, b+1 of sweep n, so consecutive sweeps of ONE run overlap (no chip-wide drain between launches).  Bit-identical; on the current runtime the cross-queue event waits cost more than the overlap gains (4096^2, one run in flight: 1.52e12 with one launch per sweep, 1.34e12 with two bands, 1.13e12 with three -- round 5), so 0 = auto means 1 = one launch per sweep.  Large grids with the merged kernel only; ignored elsewhere (streaming analysis, graphs, batched runs) */
    PVA_OPT_PATCH_KERNEL = 17, /* air tiles by the persistent per-CU kernel with LDS-DMA run-ahead (csrc/pv_patch.h: one 512-thread workgroup per CU, the next 4-tile patch lands in LDS while the current one computes) instead of one wave per tile; general tiles in a launch of their own.  Only the large-grid tile (steps per launch 12, tile rows 36) has the kernel; ignored elsewhere and with streaming analysis, slabs, edge tiles, kernel timing.  -1 = default for the configuration, 0 = off, 1 = on */
    PVA_OPT_LAZY_FAR_CELLS = 19, /* 1 (default): a run resets "no onset" / the default listener direction only in the previous and the current history-window block of the result map; the listener direction of the other far cells (unit vector listener -> cell, Analyzer.cpp:365-391,415-428) is materialised when a whole-map read-back asks for it and computed in closed form by PvAmdGetOutput / the output queries.  0: rewrite every far cell on every run (201 MB at 4096^2), the form of rounds 1-2 (validation) */
    PVA_OPT_STREAM_FUSE = 20,  /* streaming analysis only: the forward sums of the analysis (onset, dry energy, source-direction flux) of AIR tiles advance inside the step kernel (csrc/pv_stream.h: open half tiles with the sums in registers); the ring of pressure planes and the accumulate pass then serve only tiles with walls, grid edges, the listener or a registered emitter.  -1 (default): by grid size (on from 6000 tiles, where the ring traffic binds); 0: ring + accumulate pass for every tile (round 2's form); 1: on */
    PVA_OPT_AUX_STREAMS = 21,  /* HIP streams the solver creates beside its own two and never launches on (default 0).  The streams of a process share a handful of hardware queues, handed out by creation order, and two step loops that land on one queue run their launches strictly one after the other.  Measured on MI355X / ROCm 7.0 at 512^2: with 1, the two batch groups' step loops overlap (batched launches 33 instead of 63 us: 3.5e11 instead of 2.1e11 cell-updates/s); with 0, four pipelined single runs keep 2.8e11 instead of 2.5e11.  api.batch_solver_options sets 1 */
    PVA_OPT_RESIDENT_KERNEL = 22, /* the resident kernel (csrc/pv_resident.hip): ONE launch per run, every tile a workgroup that stays on its CU for all T steps and hands its interior to its neighbours every K steps through write-through stores + one flag word per tile (no kernel boundary, no grid barrier) -- for the grids the reference ships (its 275 ... 750 Hz presets on a 25 m scene: 70^2 ... 191^2) and everything else whose history window is the whole grid and whose tiles fit the chip at once.  0 (default) = auto: where the solver runs its default tile for launch-bound grids; 1 = also with an explicitly chosen (steps per launch, tile rows) = (12, 12); 2 = never (the replayed graph of tile-kernel launches) */
    PVA_OPT_RT60_LANES = 23,   /* wet gain + decay time (Analyzer.cpp:235-247,282-327): lanes that share a cell -- 16 (DPP row: few cells, parallel logarithms), 1 (lane per cell over the tile-major history, csrc/pv_rt60.hip: fewest instructions and bytes per sample) or 4 (round 4's blocked form, kept for validation); same bits in every form.  0 (default) = 16 or 1, chosen on the device from the number of reachable cells */
    PVA_OPT_FUSED_ANALYSIS = 29, /* grids whose pressure history covers the whole grid, up to 98 304 cells (the reference's presets): 1 = the whole analysis of a run is ONE launch (csrc/pv_fused.hip: onsets, dry / wet gain, decay time, listener direction as phases of workers that draw items from a ticket counter) -- an arm of the EXPERIMENTAL build of the library (bit-identical, measured slower); the product build refuses it.  -1 / 0 (default) = the separate kernels.  Results do not depend on it */
    PVA_OPT_ANALYSIS_FORK = 28, /* 1 (default) = on windows of 4 096 cells and more (PV_ANALYSIS_FORK_CELLS, csrc/pv_solver.cpp) the wet gain / decay-time pass runs on the solver's second stream beside the dry-gain pass (both only read the onsets); 0 = behind it; 2 = beside it on every window.  Results do not depend on it */
    PVA_OPT_STREAM_PRIORITY = 25, /* 1 = the solver's main stream is created with the device's highest priority.  Streams of different priorities never share a hardware queue (the runtime multiplexes the streams of a process on a handful of them, and launches of streams that share one run one after the other): give every other solver of a group that is meant to run side by side -- two runs in flight on one GPU -- this option.  Results do not depend on it.  Default 0 */
    PVA_OPT_ALTERNATE_SWEEPS = 26, /* tile order 3 only: 1 = odd launches of a run walk every XCD's strip of tiles from its last tile row to its first, so that a launch reads first what the previous launch wrote last (still in the 256 MiB Infinity Cache) instead of streaming through the cache in the order that evicts everything before it is read again.  Results do not depend on it.  -1 = default, 0 = off */
    PVA_OPT_XCD_REGIONS = 27, /* tile order 3 only: 1 = every XCD owns one of 2 x 4 regions of the grid (walked row-major) instead of one of 8 strips of tile columns: a region is twice as wide, so half as many cache lines on its sides are fetched by two XCDs, and a tile's vertical neighbours are still close enough for the XCD's L2.  Results do not depend on it.  -1 = default (on), 0 = strips */
    PVA_OPT_REACH_BOUND = 30, /* runs that go out as plain merged launches (grids of more than 4096 tiles, or with PVA_OPT_USE_GRAPH set to 2; not with row bands, slabs, streaming analysis, dense history, edge tiles, kernel timing or a listener outside the grid): 1 = every K-step launch advances only the tiles that the pulse can have reached by then (a run starts from zero fields and a value moves one cell per step), the rest of both buffer sets is kept at zero.  Bit-identical to full sweeps.  -1 = default (on), 0 = every launch sweeps the whole grid */
    PVA_OPT_RESIDENT_WINDOW = 31, /* runs that would go out reach-bounded (PVA_OPT_REACH_BOUND) on the large-grid tile (steps per launch 12, tile rows 36: grids from 3072^2): 1 = when the listener's 4-connected air component is walled in and the tile window around it (bounding box + one cell, rounded out to tiles) lies inside the run's history window and fits the device's resident-block budget at that moment, the run's T steps are ONE launch of the resident kernel over that window (three 12-row resident tiles per 36-row tile) instead of T / 12 dependent launches: pressure never crosses a wall cell, so nothing outside the window can become non-zero.  Every other run -- open field, listener inside a wall, window too large, budget taken by runs in flight -- is reach-bounded as before.  Bit-identical.  PvAmdLastRunResidentWindow tells which path the last run took.  -1 = default (on), 0 = off */
    PVA_OPT_DEBUG_LOSE_FIRST_CAPTURE = 24, /* validation: 1 = the solver's first run-graph capture counts as lost (what a legacy-stream operation of another host thread does to it): that run goes out as plain launches, the next one captures again (tests/test_gpu_parity.py) */
    PVA_OPT_PATCH_STRIP = 18,  /* patch columns per strip of the patch kernel's walk over the grid (development; default 3) */
    PVA_OPT_EDGE_TILES = 15    /* 1 = tiles whose only non-air faces are the grid's absorbing edges run the air-tile code + edge overrides (tile class 2) instead of the general path.  Only the batched kernels of the mirror-pair tiles (K, rows = (8,40), (10,36), (12,36)) have that arm -- inside the merged kernel it slows the air tiles by 25-40 %, DESIGN.md 8.4 -- so every run of such a solver goes through PvAmdRunBatch's kernel (PvAmdRun = a batch of one) and PvAmdRunSteps is refused; ignored for other configurations.  Default 0 */
};

PVA_EXPORT int PvAmdDeviceCount(void);
PVA_EXPORT const char* PvAmdLastError(void);
PVA_EXPORT const char* PvAmdVersion(void);

/* Create the grid for a config (Grid::Grid, Grid.cpp:30-117, + FreeGrid, FreeGrid.cpp:6-34) on HIP device
 * `device`.  PlaneverbCreateGrid is the same function under the name BASELINE.json uses. */
PVA_EXPORT PvAmdSolver* PvAmdCreate(float gridSizeX, float gridSizeY, int gridResolution, int device);
PVA_EXPORT PvAmdSolver* PlaneverbCreateGrid(float gridSizeX, float gridSizeY, int gridResolution, int device);
/* SURVEY.md 8f N4 -- ONE grid decomposed into `nslabs` row slabs (whole tile rows), slab i on HIP device devices[i] (all
 * equal: several slabs on one GPU).  Each slab holds planes, pressure history and result maps for its own rows only;
 * per K-step launch the K boundary rows of pr, vx, vy travel into the neighbours' guard bands, per run the boundary rows'
 * pressure histories and the window block of the per-slab result maps.  The reference has no
 * counterpart (its loop advances the whole grid, PvContext.cpp:63-94); results are bit-identical to PvAmdCreate's.
 * The handle supports: SetOption (tile / step options), GetInfo, Add / Update / RemoveGeometry, LoadScene, Run,
 * GetOutput, CopyResults, CopyFields, CopyHistoryPlane, GetImpulseResponse, CopyPulse, CopyMaterial, GetTimings,
 * GetSlabInfo, Destroy; the other PvAmd* calls return -1 for it. */
PVA_EXPORT PvAmdSolver* PvAmdCreateSlabs(float gridSizeX, float gridSizeY, int gridResolution, const int* devices,
                                         int nslabs);
typedef struct PvAmdSlabInfo {
    int nslabs;
    int row0[16], rows[16], device[16];  /* cell-array rows [row0, row0 + rows) of slab i */
    long long haloBytesPerLaunch;        /* pr, vx, vy boundary rows moved between slabs per K-step launch */
    long long exchangeBytesPerRun;       /* boundary histories + result blocks of the last run */
    long long deviceBytes[16];           /* HBM held by slab i (whole-grid result maps: see PvAmdGetInfo) */
    int handoffWords;                    /* 1: slabs of one device hand over through words in device memory, 0: stream events */
    int streamRedeals;                   /* times every slab was given another stream at creation: the hand-off's dry run timed out or was slow */
    float dryRunUsPerSweep;              /* how long a sweep of that dry run took (launches and sync included; ~4 us per slab when the streams run beside each other) */
} PvAmdSlabInfo;
PVA_EXPORT int PvAmdGetSlabInfo(PvAmdSolver* s, PvAmdSlabInfo* out);
/* The same decomposition with the slabs in DIFFERENT PROCESSES (one rank per GPU): a rank creates ITS slab, the host
 * language moves the halos between ranks (planeverb_amd/dist_slabs.py: torch.distributed send / recv, RCCL on GPU ranks),
 * rank 0 additionally holds the whole-grid maps (PvAmdSlabRoot*).  Per run and rank:
 *   SlabBegin; for li < SlabNumLaunches: { SlabLaunch(li); SlabExportHalo(side) -> neighbour -> SlabImportHalo(side) };
 *   SlabExportEdgeHistory -> rank below -> SlabImportAboveHistory; SlabAnalyze; SlabWindowBlock -> rank 0 ->
 *   SlabRootImportBlock; rank 0: SlabRootBegin before the blocks, SlabRootFinish after them, then SlabRootGetOutput.
 * side 0 = towards the slab above (smaller rows), 1 = towards the slab below.  Buffers are host memory. */
PVA_EXPORT PvAmdSolver* PvAmdCreateSlabRank(float gridSizeX, float gridSizeY, int gridResolution, int device,
                                            int slabIndex, int slabCount);
/* FreeGrid energy (FreeGrid.cpp:71-110) of a config: computed once (rank 0) and given to every slab rank */
PVA_EXPORT int PvAmdComputeEfree(float gridSizeX, float gridSizeY, int gridResolution, int device, float* efree);
PVA_EXPORT int PvAmdSlabSetEfree(PvAmdSolver* slab, float efree);
PVA_EXPORT int PvAmdSlabBegin(PvAmdSolver* slab, float lx, float ly, float lz);
PVA_EXPORT int PvAmdSlabNumLaunches(PvAmdSolver* slab);
PVA_EXPORT int PvAmdSlabLaunch(PvAmdSolver* slab, int li);
PVA_EXPORT int PvAmdSlabHaloFloats(PvAmdSolver* slab);    /* 3 x K x pitch */
/* (the buffers of the next four calls may be HOST or DEVICE memory of the slab's device -- e.g. the device tensors an RCCL
 * transport sends and receives: nothing is staged through the host then) */
PVA_EXPORT int PvAmdSlabExportHalo(PvAmdSolver* slab, int side, float* host);
PVA_EXPORT int PvAmdSlabImportHalo(PvAmdSolver* slab, int side, const float* host);
PVA_EXPORT int PvAmdSlabHistoryFloats(PvAmdSolver* slab); /* T x histPitch */
PVA_EXPORT int PvAmdSlabExportEdgeHistory(PvAmdSolver* slab, float* host);
PVA_EXPORT int PvAmdSlabImportAboveHistory(PvAmdSolver* slab, const float* host);
PVA_EXPORT int PvAmdSlabAnalyze(PvAmdSolver* slab);
/* info4 = {first whole-grid row, first column, rows, columns} of the block; returns the floats needed (7 planes), and
 * fills `host` when capacity suffices; < 0 on error */
PVA_EXPORT long long PvAmdSlabWindowBlock(PvAmdSolver* slab, int* info4, float* host, long long capacityFloats);
typedef struct PvAmdSlabRoot PvAmdSlabRoot;
PVA_EXPORT PvAmdSlabRoot* PvAmdSlabRootCreate(PvAmdSolver* anySlab, int device);
PVA_EXPORT void PvAmdSlabRootDestroy(PvAmdSlabRoot* r);
PVA_EXPORT int PvAmdSlabRootBegin(PvAmdSlabRoot* r, float lx, float ly, float lz);
PVA_EXPORT int PvAmdSlabRootImportBlock(PvAmdSlabRoot* r, const int* info4, const float* host);
PVA_EXPORT int PvAmdSlabRootFinish(PvAmdSlabRoot* r);
PVA_EXPORT int PvAmdSlabRootGetOutput(PvAmdSlabRoot* r, float ex, float ey, float ez, PlaneverbOutput* out);
PVA_EXPORT int PvAmdSlabRootCopyResults(PvAmdSlabRoot* r, float* res8, float* delay);
PVA_EXPORT void PvAmdDestroy(PvAmdSolver* s);
PVA_EXPORT int PvAmdSetOption(PvAmdSolver* s, int key, long long value);
PVA_EXPORT int PvAmdGetInfo(PvAmdSolver* s, PvAmdInfo* out);

/* Geometry (Grid::AddAABB / RemoveAABB / UpdateAABB, Grid.cpp:136-303); applied before the next run */
PVA_EXPORT int PvAmdAddGeometry(PvAmdSolver* s, float posX, float posY, float width, float height,
                                float absorption);
PVA_EXPORT int PvAmdUpdateGeometry(PvAmdSolver* s, int id, float posX, float posY, float width, float height,
                                   float absorption);
PVA_EXPORT int PvAmdRemoveGeometry(PvAmdSolver* s, int id);
PVA_EXPORT int PvAmdLoadScene(PvAmdSolver* s, const char* pvPath);
/* Write the current boxes as a .pv file (Editor.cpp:219-243).  The .pv format is the reference's and holds axis-aligned
 * boxes only: shapes of any kind (convex, disc, capsule, wall path, polygon) are not written. */
PVA_EXPORT int PvAmdSaveScene(PvAmdSolver* s, const char* pvPath);

/* Shapes (no reference counterpart).
 *
 * A shape is a convex polygon of 3 to 8 vertices xy[2n] = {x0, y0, x1, y1, ...} in grid metres (x = grid x = world x,
 * y = grid y = world z, as for the AABBs) with an absorption value.  Refused (-1, PvAmdLastError): a non-finite coordinate or
 * absorption, fewer than 3 or more than 8 vertices, zero area, a non-convex (or self-intersecting) list.  A clockwise list is
 * reversed to counter-clockwise.  Absorption is accepted by the rule of PvAmdAddGeometry (any finite value).
 *
 * Coverage: cell (x, y), 0 <= x < gx, 0 <= y < gy, is covered when its centre P = (((float)x + 0.5f) * dx,
 * ((float)y + 0.5f) * dx) satisfies (e.x * (P.y - a.y)) - (e.y * (P.x - a.x)) >= 0 for every edge a -> b, e = b - a, all in
 * float32 without contraction.  The ghost row and column are never covered.  This is a cell-CENTRE rule, not the reference's
 * truncation rule for AABBs: an axis-aligned oriented box need not cover the cells of the AABB with the same numbers.
 *
 * Composition: shapes are a layer on top of the AABB layer, which stays exactly what it is (quirks included).  A covered cell
 * is a wall (b = by = 0) with the absorption of the covering shape added or updated most recently; an uncovered cell has
 * the AABB layer's material.  Removing or moving a shape brings back the AABB layer beneath it: the layer is a pure function
 * of the current set of shapes.  Shape ids are their own table, recycled last-in first-out like the AABB ids.
 * PvAmdCopyMaterial and the b / by of PvAmdGetImpulseResponseCells report the composed material.  A solver that never has a
 * shape runs exactly as before.  Slab groups (PvAmdCreateSlabs) take shapes; slab ranks (PvAmdCreateSlabRank) refuse them. */
PVA_EXPORT int PvAmdAddShape(PvAmdSolver* s, const float* xy, int n, float absorption);
PVA_EXPORT int PvAmdUpdateShape(PvAmdSolver* s, int id, const float* xy, int n, float absorption);
PVA_EXPORT int PvAmdRemoveShape(PvAmdSolver* s, int id);
/* An oriented box: centre (px, py), full width w along the axis (ax, ay) and full height h along its left normal.  A Unity
 * caller passes transform.right.x / .z as the axis.  u = (ax, ay) * inv with inv = 1.0f / sqrtf(ax*ax + ay*ay), v = (-u.y, u.x),
 * vertices (c - w/2 u - h/2 v, c + w/2 u - h/2 v, c + w/2 u + h/2 v, c - w/2 u + h/2 v), as PvAmdHostOrientedBoxVertices
 * returns them.  A zero axis is refused. */
PVA_EXPORT int PvAmdAddOrientedBox(PvAmdSolver* s, float px, float py, float w, float h, float ax, float ay, float absorption);
PVA_EXPORT int PvAmdUpdateOrientedBox(PvAmdSolver* s, int id, float px, float py, float w, float h, float ax, float ay,
                                      float absorption);
/* Round and concave shapes (no reference counterpart): three more kinds in the SAME layer.  They share the id table, the
 * sequence rule (the shape added or updated most recently wins), the composition over the AABB layer and PvAmdRemoveShape
 * with the convex shapes above; an Update call may change a shape's kind.  Coordinates are grid metres, P is the cell centre
 * of the convex rule, every operation below is float32 without contraction, in the order the brackets give, and the ghost row
 * and column are never covered.
 *
 * Disc: centre c, radius r.  d = P - c; covered when (d.x*d.x) + (d.y*d.y) <= r*r.
 * Capsule (a thick wall segment): end points a, b, radius r (half the wall's thickness).  e = b - a, w = P - a,
 *   ee = (e.x*e.x) + (e.y*e.y); t = 0 when ee == 0, else t = ((w.x*e.x) + (w.y*e.y)) / ee, then t = 0 if t < 0, 1 if t > 1;
 *   q = (w.x - (t*e.x), w.y - (t*e.y)); covered when (q.x*q.x) + (q.y*q.y) <= r*r.  (The t = 0 case is decided by the float32
 *   value ee, not by e, so that an e whose squares underflow is a disc too.)  a == b gives the disc's bits.
 * Wall path: a polyline xy[2n] of 2 to PVA_POLY_MAX_VERTS points with one radius: ONE shape (one id, one sequence number)
 *   that covers a cell when any of its n - 1 capsules (xy[i], xy[i+1]) does.  Consecutive capsules share an end point, so
 *   corners are round and have neither notch nor overlap.
 * Simple polygon: 3 to PVA_POLY_MAX_VERTS vertices, concave allowed, either winding (the list is kept as given).  Even-odd
 *   crossing count over the edges a -> b (the last vertex back to the first): an edge toggles the cell when
 *   (a.y > P.y) != (b.y > P.y) and P.x < (((b.x - a.x) * (P.y - a.y)) / (b.y - a.y)) + a.x; covered after an odd number of
 *   toggles.  This rule and the convex half-plane rule of PvAmdAddShape may differ on cells whose centre lies exactly on an
 *   edge (there the convex rule covers on every edge, this one on some of them only), which is why this is an entry
 *   point of its own and not a relaxation of PvAmdAddShape.  Holes are not supported.
 *
 * Refused (-1, PvAmdLastError, the table unchanged): a non-finite coordinate, radius or absorption; a radius <= 0 (or whose
 * float32 square is 0 or infinite); a segment whose ee is infinite; a wall path of fewer than 2 or more than
 * PVA_POLY_MAX_VERTS points; a polygon of fewer than 3 or more than PVA_POLY_MAX_VERTS vertices, of zero area (shoelace sum
 * in double), or self-intersecting.  Self-intersection is checked on the host in O(n^2), in double, with
 * o(p, q, r) = (q.x - p.x)*(r.y - p.y) - (q.y - p.y)*(r.x - p.x): refused are a zero-length edge; two neighbouring edges p -> v,
 * v -> q that fold back (o(p, v, q) == 0 and (p - v).(q - v) > 0); and two other edges p1p2, p3p4 that cross (o(p3,p4,p1) and
 * o(p3,p4,p2) of opposite strict signs, and o(p1,p2,p3) and o(p1,p2,p4) too) or touch (one of those four is 0 and its point
 * lies in the other edge's bounding box).  Collinear runs of vertices are accepted.  A radius below half a cell may cover
 * no cell at all: that is a valid shape.  Slab groups take these kinds, slab ranks refuse them, as for PvAmdAddShape.  The .pv
 * scene format holds axis-aligned boxes only: none of these is written by PvAmdSaveScene. */
#define PVA_POLY_MAX_VERTS 64
PVA_EXPORT int PvAmdAddDisc(PvAmdSolver* s, float cx, float cy, float radius, float absorption);
PVA_EXPORT int PvAmdUpdateDisc(PvAmdSolver* s, int id, float cx, float cy, float radius, float absorption);
PVA_EXPORT int PvAmdAddCapsule(PvAmdSolver* s, float ax, float ay, float bx, float by, float radius, float absorption);
PVA_EXPORT int PvAmdUpdateCapsule(PvAmdSolver* s, int id, float ax, float ay, float bx, float by, float radius, float absorption);
PVA_EXPORT int PvAmdAddWallPath(PvAmdSolver* s, const float* xy, int n, float radius, float absorption);
PVA_EXPORT int PvAmdUpdateWallPath(PvAmdSolver* s, int id, const float* xy, int n, float radius, float absorption);
PVA_EXPORT int PvAmdAddPolygon(PvAmdSolver* s, const float* xy, int n, float absorption);
PVA_EXPORT int PvAmdUpdatePolygon(PvAmdSolver* s, int id, const float* xy, int n, float absorption);
/* Triangle meshes (no reference counterpart: the reference adds a collider's bounding box while the listener's height lies
 * inside it).  The grid is a horizontal slice of a 3-D world; a mesh stays on the device and is sliced at the solver's slice
 * height h, and the section is rasterised there, in a layer of its own BETWEEN the AABB layer and the shape layer.  Everything
 * below is float32 without contraction, in the order the brackets give.
 *
 * Mesh: nv vertices (x, y, z) in world units, y = height, grid x = world x and grid y = world z as for the AABBs; nt triangles
 *   of three int32 indices; an absorption value, taken as PvAmdAddGeometry takes it; a mode, PVA_MESH_SOLID or PVA_MESH_SHELL;
 *   in shell mode a radius r, half the wall's thickness (ignored in solid mode).  An optional affine transform m[12],
 *   row-major 3 x 4: world = ((m0*x + m1*y) + m2*z) + m3 per row.  A mesh without a transform call has none: its vertices are
 *   used as they are, bit for bit.  At most PVA_MESH_MAX live meshes, PVA_MESH_MAX_TRIS triangles per mesh and
 *   PVA_MESH_MAX_TRIS_TOTAL over all meshes of a solver.
 * Slice: one height h per solver, 0 by default (PvAmdSetSliceHeight).  A vertex is ABOVE when v.y > h, strictly: a vertex on
 *   the plane is not above.  A triangle whose three vertices agree gives no segment.  Otherwise exactly two of its edges, in
 *   the order (v0,v1), (v1,v2), (v2,v0), have ends that disagree; for each, p = the end that is not above and q = the end
 *   above, whichever way the triangle lists them (so two triangles that share an edge compute the same bits):
 *   t = (h - p.y) / (q.y - p.y), X = p.x + (t * (q.x - p.x)), Z = p.z + (t * (q.z - p.z)).  The triangle's segment is a -> b,
 *   a from the first such edge and b from the second, in grid coordinates (X, Z).  A face lying exactly in the plane yields no
 *   segment in either mode: its neighbours' sections outline it.
 * Coverage (P = the cell centre of the rules above; the ghost row and column are never covered):
 *   Solid: even-odd crossings over the mesh's segments by the edge rule of PvAmdAddPolygon, word for word: a segment toggles
 *   the cell when (a.y > P.y) != (b.y > P.y) and P.x < (((b.x - a.x) * (P.y - a.y)) / (b.y - a.y)) + a.x; covered after an odd
 *   number of toggles.  A section with a hole is an annulus: the one kind here that expresses holes.
 *   Shell: covered when the capsule rule of PvAmdAddCapsule with radius r covers the cell for any segment (ee == 0, a disc,
 *   included: a segment with a == b can arise).
 * Composition: the AABB layer, overwritten by the mesh layer -- among meshes the one added or updated most recently wins, and
 *   PvAmdSetMeshTransform counts as an update -- overwritten by the shape layer.  Each layer is a pure function of its current
 *   set and h.  Mesh ids are a table of their own, recycled last-in first-out.  A solver that never has a mesh runs exactly
 *   as before.
 * Refused (-1, PvAmdLastError, the tables unchanged): a non-finite vertex, transform entry, h, absorption or (shell) radius; in
 *   shell mode r <= 0 or an r whose float32 square is 0 or infinite; an index outside [0, nv); nt < 1 or a count over the
 *   limits; a triangle with two equal indices; in solid mode a mesh in which some undirected edge is not shared by exactly two
 *   triangles (checked on the host when the mesh is added: it is what makes the parity fill well defined; the same open mesh
 *   is accepted in shell mode).  Slab groups and slab ranks refuse meshes.  The .pv scene format holds boxes only.
 * PvAmdCopyMeshSection: the segments as the device sliced them at the current h and transform, out4nt[4 i ..] = (a.x, a.z,
 *   b.x, b.z) and valid_nt[i] = 1, or zeros and 0 for a triangle without one; slot i belongs to triangle i (no compaction), so
 *   the result is deterministic.  Either array may be NULL. */
#define PVA_MESH_SOLID 0
#define PVA_MESH_SHELL 1
#define PVA_MESH_MAX 64
#define PVA_MESH_MAX_TRIS (1 << 20)
#define PVA_MESH_MAX_TRIS_TOTAL (1 << 22)
PVA_EXPORT int PvAmdAddMesh(PvAmdSolver* s, const float* verts, int nv, const int* tris, int nt, float absorption, int mode,
                            float radius);
PVA_EXPORT int PvAmdUpdateMesh(PvAmdSolver* s, int id, const float* verts, int nv, const int* tris, int nt, float absorption,
                               int mode, float radius);
PVA_EXPORT int PvAmdSetMeshTransform(PvAmdSolver* s, int id, const float m12[12]);
PVA_EXPORT int PvAmdRemoveMesh(PvAmdSolver* s, int id);
PVA_EXPORT int PvAmdSetSliceHeight(PvAmdSolver* s, float h);
PVA_EXPORT float PvAmdGetSliceHeight(PvAmdSolver* s);
PVA_EXPORT int PvAmdMeshTriangles(PvAmdSolver* s, int id); /* nt of a live mesh, -1 otherwise */
PVA_EXPORT int PvAmdCopyMeshSection(PvAmdSolver* s, int id, float* out4nt, uint8_t* valid_nt);
/* The same rules on the CPU, without a device.  PvAmdHostMeshSection: the section of triangles that need not form a valid
 * mesh (indices inside [0, nv) and finite inputs are still required); m12_or_null = NULL: no transform.
 * PvAmdHostMeshCoverage: cover[NX * NY], index x * NY + y, 0 / 1, of one mesh (validated as PvAmdAddMesh validates it). */
PVA_EXPORT int PvAmdHostMeshSection(const float* verts, int nv, const int* tris, int nt, const float* m12_or_null, float h,
                                    float* out4nt, uint8_t* valid_nt);
PVA_EXPORT int PvAmdHostMeshCoverage(float gridSizeX, float gridSizeY, int gridResolution, const float* verts, int nv,
                                     const int* tris, int nt, const float* m12_or_null, float h, int mode, float radius,
                                     uint8_t* cover);
/* Grid edges.  absorption4 = R of the sides 0: faces at x = 0 (world x = 0), 1: faces at x = gx, 2: faces at y = 0 (world
 * z = 0), 3: faces at y = gy, taken as PvAmdAddGeometry takes absorption (any finite value); the admittance of side k is
 * Y = (1 - R) / (1 + R) in float32.  The edge faces are the reference's absorbing edges (FDTD.cpp:201-223) with Y in place of
 * 1: x = 0: kx = (cell air && y < gy) ? -Y0 : 0;  x = gx: kx = (y < gy) ? +Y1 : 0;  y = 0 / y = gy likewise with Y2 / Y3.
 * R = 0 on every side (the default) is the reference's grid, bit for bit; R = 1 is a rigid edge (pv_ReflectingBoundary).
 * The free-field energy stays that of the open grid, so occlusion stays normalised by the free field.  A change takes effect
 * at the next run of any form.  NULL or a non-finite value returns -1 and changes nothing.  Slab groups forward the call to
 * every slab; slab ranks (PvAmdCreateSlabRank) refuse any non-zero side.  The .pv scene format does not hold the boundary. */
PVA_EXPORT int PvAmdSetGridBoundary(PvAmdSolver* s, const float absorption4[4]);
PVA_EXPORT int PvAmdGetGridBoundary(PvAmdSolver* s, float out4[4]);
/* Graded absorbing layers (PML-style damping bands) along the grid edges, for open scenes: the absorbing edge above reflects a
 * wave that meets it at an angle (about (cos t - 1) / (cos t + 1) of it).  width4 = widths in cells of the sides in the order of
 * PvAmdSetGridBoundary (x = 0, x = gx, y = 0, y = gy), 0..64, 0 = no layer (the default: every path and result as without this
 * call).  A layer is the outermost w cells of its side, inside the grid: coordinates, gx / gy and the result map do not change,
 * and the cells of a layer get results like any other cell, but those results are NOT physical (the field is being damped
 * there).  The damping is eight float32 tables (PvAmdHostEdgeLayerTables); in the stencil only two expressions change,
 * multiplications only, without contraction (C = the Courant number, div / grad as in FDTD.cpp:124-199):
 *   pressure: pr' = beta * ((apx[x] * apy[y]) * pr - (bpx[x] * bpy[y]) * (C * div))
 *   vx, air : ax[x] * vx - bx[x] * (C * grad_x)          vy, air : ay[y] * vy - by[y] * (C * grad_y)
 * The wall-face terms, the beta blend, the grid-edge rule (with PvAmdSetGridBoundary's R: a layer may sit in front of a rigid
 * edge) and the record-then-pulse order are unchanged; every factor is exactly 1 outside the layers.  The library records the
 * pressure only and re-derives velocities without the damping, so the source direction (srcDir) and the impulse-response
 * velocities of cells inside a layer are not the damped stencil's either.
 * Refused (-1, nothing changes): NULL, a width below 0 or above 64, widths that leave fewer than 8 cells between two opposite
 * layers (or a layer and the far edge), sparse-emitter (PVA_OPT_STREAMING_ANALYSIS) solvers, slab groups and slab ranks, edge
 * tiles (PVA_OPT_EDGE_TILES) and tile configurations without a layer kernel (the product library's tiles have one).
 * A solver with a layer runs the tile path: merged launches plus one layer launch per K-step sweep, as a captured graph or plain
 * launches, reach-bounded where PVA_OPT_REACH_BOUND applies.  The resident kernel, the small-grid kernel, the stacked, segment
 * and patch forms, row bands and the two-kernel form need a layer-free grid and resolve off (PvAmdInfo.residentKernel = 0);
 * batched runs (PvAmdRunBatch) refuse a solver with a layer.  A change takes effect at the next run of any form.  Bakes fold the
 * widths into the material hash when some width is non-zero.  The .pv scene format does not hold the layer. */
PVA_EXPORT int PvAmdSetEdgeLayer(PvAmdSolver* s, const int width4[4]);
PVA_EXPORT int PvAmdGetEdgeLayer(PvAmdSolver* s, int out4[4]);
/* Split-field (Berenger) edge layers: the same widths, tables and refusals as PvAmdSetEdgeLayer, with the design reflection r0
 * of the tables given (PvAmdHostEdgeLayerTablesR0) and the pressure of a layer cell -- a cell with apx[x] != 1 or apy[y] != 1 --
 * carried in two parts, each damped by its own axis only.  The unsplit layer damps the whole pressure (apx * apy), the part of
 * its divergence that comes from the velocity along the layer included; a wave that meets it at an angle sees that mismatch
 * and it reflects, the more the stronger the grading.  The split layer does not: on an open 160^2 grid at 275 Hz (width 24 on
 * every side) it cuts the error energy outside the layers 43 dB below plain absorbing edges, against 11 dB for the unsplit
 * layer (profiles/edge_layer.txt).  Layer cells are the cells of depth > 0 along either axis (so the ghost row's cells inside a
 * y layer too, and the ghost column's inside an x layer).  A layer cell carries px, the x part of its pressure; the y part is
 * pr - px.  Per
 * step, strict IEEE float32 without contraction, dvx / dvy = the stencil's own velocity differences along x / y:
 *   nx = beta * ((apx[x] * px) - bpx[x] * (C * dvx))      ny = beta * ((apy[y] * (pr - px)) - bpy[y] * (C * dvy))
 *   pr' = nx + ny        px' = nx
 * Every other cell: the reference's beta * (pr - C * div), px = 0.  The velocities, wall terms, beta blend, grid-edge rule,
 * record-then-pulse order and the recording of pr only are the unsplit layer's; the pulse goes into pr only (a listener inside
 * a layer puts it into the y part).  px is part of the fields: zero at the start of every run, after PvAmdSetFields and after
 * every geometry, layer or model change, carried between PvAmdRunSteps calls, never exposed.  Refused (-1, nothing changes):
 * whatever PvAmdSetEdgeLayer refuses, and r0 that is NaN or outside (0, 1).  PvAmdSetEdgeLayer afterwards selects the unsplit
 * model again.  A width, model or r0 change takes effect at the next run.  Bakes of a solver with the split model and some
 * non-zero width fold a model tag and r0 into the material hash after the widths.  Recommended r0: PVA_EDGE_LAYER_SPLIT_R0
 * (a sweep over widths 8-24 on the grid above). */
#define PVA_EDGE_LAYER_SPLIT_R0 1e-4
PVA_EXPORT int PvAmdSetEdgeLayerSplit(PvAmdSolver* s, const int width4[4], double r0);
/* the model of the solver's layers: *split = 1 for the split-field model (with its *r0), 0 for the unsplit one (*r0 = 0.1) */
PVA_EXPORT int PvAmdGetEdgeLayerModel(PvAmdSolver* s, int* split, double* r0);
/* CPU only: the layer tables of the grid (sizeX, sizeY, res) with widths width4, into out[4 (gx + 1) + 4 (gy + 1)] in this order:
 * apx[gx + 1], bpx[gx + 1], ax[gx + 1], bx[gx + 1], apy[gy + 1], bpy[gy + 1], ay[gy + 1], by[gy + 1] (index = cell row x for apx
 * / bpx, velocity face x -- between cells x - 1 and x -- for ax / bx; y likewise).  For a damping value s:
 * a = (1 - s) / (1 + s), b = 1 / (1 + s), computed in double and rounded to float.  Cells sit at half depths, faces at whole
 * depths: with a layer of width w on side 0, face x has depth w - x (x <= w) and cell x depth w - x - 1/2 (x < w); on side 1,
 * face x has depth x - (gx - w) (x >= gx - w) and cell x depth x + 1/2 - (gx - w) (gx - w <= x < gx); the ghost cell x = gx
 * lies outside every layer.  s = s_max * (depth / w)^2 for depth > 0, else 0; s_max = 3 C ln(1 / R0) / (4 w) (the grading rule
 * with m = 2) with R0 = 0.1 and C the grid's float32 Courant number taken to double.  Returns the number of floats written,
 * or -1 (a refused width, res < 275, NULL). */
PVA_EXPORT int PvAmdHostEdgeLayerTables(float gridSizeX, float gridSizeY, int gridResolution, const int width4[4], float* out);
/* CPU only: PvAmdHostEdgeLayerTables with the design reflection R0 = r0 (0 < r0 < 1, else -1) in s_max, computed in double;
 * r0 = 0.1 gives PvAmdHostEdgeLayerTables' bits.  The tables of PvAmdSetEdgeLayerSplit. */
PVA_EXPORT int PvAmdHostEdgeLayerTablesR0(float gridSizeX, float gridSizeY, int gridResolution, const int width4[4], double r0,
                                          float* out);
/* CPU only: the enclosure search of the resident-window runs (PVA_OPT_RESIDENT_WINDOW).  beta[nx * ny] (index x * ny + y, non-zero =
 * air): the 4-connected air component of cell (seedX, seedY), walked until the tile window around it -- its bounding box grown by
 * one cell, clipped to the grid, rounded out to tileRows x tileCols-cell tiles -- holds more than maxTiles tiles; at most
 * maxTiles * tileRows * tileCols cells are visited whatever the grid's size.  out10 = {found, cells visited, box r0, c0, r1, c1
 * (inclusive), window first tile row, first tile column, tile rows, tile columns}; found = 1: the component was walked completely
 * (cells = its size) and the window fits; a seed in a wall or outside the grid: found = 0, no cell visited.  Returns the cells
 * visited, or -1 for bad arguments. */
PVA_EXPORT int PvAmdHostEnclosure(const uint8_t* beta, int nx, int ny, int seedX, int seedY, int tileRows, int tileCols, int maxTiles,
                                  int* out10);
/* CPU only: what a reach-bounded (windowRun = 0) or resident-window (1) run clears in front of its first launch.  win4 = the run's
 * tile window, prevRect4 = the rectangle the previous such run wrote, both {first tile row, tile rows, first tile column, tile
 * columns}; planesDirty / sweptDirty: the planes were written by something else since; splitPlanes: an edge layer's split planes
 * are in use.  Returns 0: nothing (a window run over the very window of the previous run), 1: prevRect4 in every plane, 2: every
 * plane, whole; -1 for bad arguments. */
PVA_EXPORT int PvAmdHostWindowClear(int windowRun, const int* win4, const int* prevRect4, int planesDirty, int sweptDirty,
                                    int splitPlanes);
/* CPU only: the four vertices out8 the library uses for that oriented box (0, or -1 for a refused input) */
PVA_EXPORT int PvAmdHostOrientedBoxVertices(float px, float py, float w, float h, float ax, float ay, float* out8);
/* CPU only: the shape the library makes of a vertex list (counter-clockwise, out16 gets 2n floats); returns n, or -1 for a
 * refused list (PvAmdLastError) */
PVA_EXPORT int PvAmdHostShape(const float* xy, int n, float absorption, float* out16);
/* CPU only: the coverage rule on a grid of that configuration: cover[(gx+1)*(gy+1)] = 1 for the cells the shape covers */
PVA_EXPORT int PvAmdHostShapeCoverage(float gridSizeX, float gridSizeY, int gridResolution, const float* xy, int n,
                                      uint8_t* cover);
/* CPU only: the coverage rules of the round and concave kinds on a grid of that configuration, with the refusals of the Add
 * calls.  kind: PVA_SHAPE_DISC (xy[2], n = 1), PVA_SHAPE_CAPSULE (xy[4], n = 2), PVA_SHAPE_WALL_PATH (xy[2n]) or
 * PVA_SHAPE_POLYGON (xy[2n], radius ignored).  cover[(gx+1)*(gy+1)] = 1 for the covered cells. */
#define PVA_SHAPE_DISC 1
#define PVA_SHAPE_CAPSULE 2
#define PVA_SHAPE_WALL_PATH 3
#define PVA_SHAPE_POLYGON 4
PVA_EXPORT int PvAmdHostRoundShapeCoverage(float gridSizeX, float gridSizeY, int gridResolution, int kind, const float* xy,
                                           int n, float radius, uint8_t* cover);

/* One iteration of the reference's background loop (PvContext.cpp:80-83): GenerateResponse + AnalyzeResponses
 * for a listener position; synchronous. */
PVA_EXPORT int PvAmdRun(PvAmdSolver* s, float lx, float ly, float lz);
/* Enqueue the same work on the solver's stream without waiting; PvAmdSync waits. */
PVA_EXPORT int PvAmdRunAsync(PvAmdSolver* s, float lx, float ly, float lz);
/* Two solvers taking turns on ONE sequence of iterations (what the live module does for small grids: two iterations in
 * flight): a run of `s` that continues `prev`'s result map -- the cells in which this run finds no onset keep the values the
 * run enqueued LAST on `prev` left there (the reference never touches them, Analyzer.cpp:160-165, and its listener-direction
 * walk reads them), carried over on the device behind prev's analysis.  Same grid, same device; asynchronous like
 * PvAmdRunAsync (PvAmdSync(s) waits for it; prev's run need not have finished when this is called). */
PVA_EXPORT int PvAmdRunAsyncAfter(PvAmdSolver* s, PvAmdSolver* prev, float lx, float ly, float lz);
PVA_EXPORT int PvAmdSync(PvAmdSolver* s);
/* n (1..8) independent runs -- one per solver, listener i at listenersXYZ[3i..3i+2] -- advanced together by ONE
 * kernel launch per K steps instead of n launches on n streams (the reference would make these n iterations of its
 * background loop one after the other, PvContext.cpp:74-93).  The solvers must sit on one device and share grid
 * size, resolution and tile configuration (scenes may differ); streaming analysis and kernel timing are excluded.
 * Afterwards every solver holds its own run's results exactly as after PvAmdRun (same bits).  wait = 0 returns after
 * enqueueing; PvAmdSync each solver before reading results. */
PVA_EXPORT int PvAmdRunBatch(PvAmdSolver* const* solvers, int n, const float* listenersXYZ, int wait);
/* The shader clock (MHz) the device sustains at this moment: one wave sleeps a known number of shader-clock cycles and times
 * them against the constant 100 MHz counter, on a stream of its own (so it can run beside solvers at work).  *byMemtimeMHz
 * (optional) = the same span by s_memtime.  0 on failure.  bench.py's device record. */
PVA_EXPORT float PvAmdClockProbe(int device, float* byMemtimeMHz);
/* The device's own streaming bandwidth, GB/s ("confirm on the box with a device-to-device copy micro-benchmark
 * and report against both"): gbPerS4[0] = device-to-device copy, 16 B per lane (bytes read + written per second), [1] = the
 * same with 4 B per lane, [2] = read only and [3] = write only, 4 B per lane in 256-byte rows per wave (the stencil kernels'
 * pattern).  1 GiB per buffer (2 GiB of device memory while it runs), best of five launches each, ~60 ms, on a stream of its
 * own; call it on an idle device.  0, or -1 on failure.  bench.py's roofline record. */
PVA_EXPORT int PvAmdBandwidthProbe(int device, float* gbPerS4);
/* The library's own log10f / powf (the restatement of glibc's that every analysis pass evaluates), one form per call:
 * out[i] = form(in[i]), i < n, computed on the current device (onDevice != 0: the device compile, with the logarithm's and the
 * power's tables in LDS exactly as the analysis kernels fill them) or by the same source on the host (onDevice = 0).  A test
 * seam: the two must agree bit for bit for every float.  PVA_LIBM_LOG10_NORMAL_TAB and _NORMAL_BATCH are defined for positive
 * normal finite inputs only; the batch form evaluates eight inputs that lie ceil(n / 8) apart together.  0, or -1 on failure. */
#define PVA_LIBM_LOG10               0  /* log10f, the branching form                              */
#define PVA_LIBM_LOG10_NONNEG        1  /* branch-free, x >= +0, constant table                    */
#define PVA_LIBM_LOG10_NONNEG_TAB    2  /* the same with the table in LDS                          */
#define PVA_LIBM_LOG10_NORMAL_TAB    3  /* normal-only form, table in LDS                          */
#define PVA_LIBM_LOG10_NORMAL_BATCH  4  /* eight of them stage by stage (the decay-time kernel's)  */
#define PVA_LIBM_POW_08              5  /* powf(x, 0.8f), the branching form                       */
#define PVA_LIBM_POW_23              6  /* powf(x, (float)(2.0 / 3.0))                             */
#define PVA_LIBM_POW_NONNEG_08       7  /* branch-free, constant tables                            */
#define PVA_LIBM_POW_NONNEG_23       8
#define PVA_LIBM_POW_NONNEG_TAB_08   9  /* the same with the tables in LDS                         */
#define PVA_LIBM_POW_NONNEG_TAB_23  10
PVA_EXPORT int PvAmdLibmProbe(int form, const float* in, float* out, long long n, int onDevice);
PVA_EXPORT int PvAmdGetTimings(PvAmdSolver* s, PvAmdTimings* out);
/* 1: the last run (PvAmdRun / PvAmdRunAsync + PvAmdSync) went out as one resident-kernel launch over the tile window around the
 * listener's walled-in air component (PVA_OPT_RESIDENT_WINDOW), 0: by any other path, -1: error.  Results do not depend on it. */
PVA_EXPORT int PvAmdLastRunResidentWindow(PvAmdSolver* s);
/* 1: the last run was one resident-kernel launch -- over the whole grid or over a window -- whose workgroups handed their tiles over
 * through ONE XCD's L2 (launches of up to 32 workgroups, PLANEVERB_AMD_RESIDENT_XCD), 0: the placement-independent hand-off or
 * another path, -1: error.  Results do not depend on it. */
PVA_EXPORT int PvAmdLastRunOneXcd(PvAmdSolver* s);

/* Streaming-analysis (sparse-emitter) mode only -- SURVEY.md 8f N3.  Registers the emitter positions (n x {x,y,z})
 * whose wet gain and RT60 the next runs compute; onset, occlusion, lowpass, source directivity and listener direction
 * are still produced for EVERY cell, wet gain / RT60 only at these cells (0 elsewhere).  This removes the
 * T x cells pressure history, which is what makes T ~ 25 000 (a 25 m scene at 4096^2) possible at all. */
PVA_EXPORT int PvAmdSetEmitters(PvAmdSolver* s, const float* xyz, int n);
/* Analyzer::GetResponseResult + Planeverb::GetOutput (Analyzer.cpp:106-116, FDTD.cpp:16-58) */
PVA_EXPORT int PvAmdGetOutput(PvAmdSolver* s, float ex, float ey, float ez, PlaneverbOutput* out);
/* Output queries: the emitter positions (n <= 64, n x {x,y,z}) whose PlaneverbOutput every FOLLOWING run gathers into
 * pinned host memory with one kernel behind its analysis -- the batch-API counterpart of the reference's registered
 * emitters (Emit / GetOutput(id), EmissionManager.cpp:11-38, FDTD.cpp:16-58).  After PvAmdSync,
 * PvAmdGetQueriedOutputs returns them without any further GPU work or stream synchronisation (PvAmdGetOutput costs a
 * launch and a sync per emitter).  n must equal the registered count; positions outside the grid give the
 * reference's sentinel (occlusion = -1, the rest 0).  Setting queries waits for a run in flight. */
PVA_EXPORT int PvAmdSetOutputQueries(PvAmdSolver* s, const float* xyz, int n);
PVA_EXPORT int PvAmdGetQueriedOutputs(PvAmdSolver* s, PlaneverbOutput* out, int n);
/* Query records: the per-cell analysis records further down (room metrics, decay times, lateral fraction, echogram, echo
 * criterion, lobes) for the cells of the registered output queries, computed INSIDE the run.  `kinds` is a mask of PVA_QREC_*.
 * Every FOLLOWING run of any form (PvAmdRun, PvAmdRunAsync, PvAmdRunAsyncAfter, a member of PvAmdRunBatch, a run that PvAmdSync
 * repeats) computes the selected kinds for the queries' cells with ONE launch on the solver's stream, behind the run's analysis
 * and in front of its last kernel, straight into pinned host memory: no pass over the history window, no per-cell device
 * storage (the pinned block holds at most 64 x the sum of the kinds' floats x 4 bytes), no host synchronisation.
 * PvAmdGetQueriedRecords waits for the run as PvAmdGetQueriedOutputs does and then copies ONE kind's records from pinned memory
 * without GPU work: nQueries x PvAmdQueryRecordFloats(kind) floats, one record after the other in query order.
 *   A record is bit for bit what PvAmdGet<Kind>(s, position) returns after PvAmdCompute<Kind> on the same run: the same
 * definition, the same cell mapping.  A query off the map gives NaNs, and so does a query whose cell has no onset in that run;
 * the call returns 0 for them, as PvAmdGet<Kind> does.  The echogram slots and lobe windows are those in force when the run was
 * enqueued (PvAmdSetEchogram and PvAmdSetLobeWindows wait for a run in flight) and the record sizes follow them; selecting
 * PVA_QREC_ECHOGRAM with no slots set is refused, and so is PvAmdSetEchogram(.., 0) while it is selected.  In-run records and
 * the whole-map records (PvAmdCompute<Kind>) do not invalidate each other.
 *   kinds = 0, the default, clears the selection and frees the pinned block: nothing is launched, recorded or allocated, and a
 * run's launches are exactly those of a solver that never called this.  PvAmdSetQueryRecords and PvAmdSetOutputQueries wait
 * for a run in flight (the launch reads the cell table).
 *   Refused with -1 and nothing changed, PvAmdLastError "query records: ...": an unknown bit; sparse-emitter
 * (PVA_OPT_STREAMING_ANALYSIS) solvers; PVA_OPT_SKIP_ANALYSIS; slab groups and slab ranks; PVA_QREC_ECHO_CRITERION at a
 * sampling rate below 112 Hz; PVA_QREC_LOBES with the default windows at a sampling rate below 100 Hz.
 * PvAmdGetQueriedRecords is refused when the kind is not selected (or is not exactly one bit), nQueries differs from the
 * registered count, no run has completed since the kinds, the queries or the kind's settings changed, or the last run ended in
 * error.  PvAmdQueryRecordFloats: floats per query of ONE kind under the current settings, -1 where it has none. */
#define PVA_QREC_ROOM_METRICS   1u    /* PvAmdRoomMetrics      10 floats */
#define PVA_QREC_DECAY_TIMES    2u    /* PvAmdDecayTimes        8 floats */
#define PVA_QREC_LATERAL        4u    /* PvAmdLateralFraction  11 floats */
#define PVA_QREC_ECHOGRAM       8u    /* 1 + 3 nSlots floats   (PvAmdSetEchogram) */
#define PVA_QREC_ECHO_CRITERION 16u   /* PvAmdEchoCriterion    10 floats */
#define PVA_QREC_LOBES          32u   /* 1 + 5 nWindows floats (PvAmdSetLobeWindows; default windows when never set) */
PVA_EXPORT int PvAmdSetQueryRecords(PvAmdSolver* s, unsigned kinds);
PVA_EXPORT unsigned PvAmdGetQueryRecordKinds(PvAmdSolver* s);
PVA_EXPORT int PvAmdQueryRecordFloats(PvAmdSolver* s, unsigned kind);
PVA_EXPORT int PvAmdGetQueriedRecords(PvAmdSolver* s, unsigned kind, float* out, int nQueries);
/* Record queries: up to PVA_RECORD_QUERIES_MAX positions (n x {x,y,z}) of their own for the in-run records, mapped to result cells
 * in the given order exactly as PvAmdSetOutputQueries maps its positions.  While n > 0 every following run computes the selected
 * kinds for THESE cells instead of the output queries' cells -- still one launch, 64 queries per wave and one more block row per
 * 64 -- and PvAmdGetQueriedRecords takes this n; PvAmdGetQueriedOutputs keeps serving the (<= 64) output queries.  n = 0, the
 * default, returns to the output queries.  The pinned cell table and record block grow to the registered count (at most
 * 1024 x 177 floats with every kind selected).  The call waits for a run in flight, and a change of the table invalidates the
 * records until the next run has completed.  A record's bits do not depend on the other queries of the table.
 *   Refused with -1 and nothing changed, PvAmdLastError "query records: ...": n outside 0 .. PVA_RECORD_QUERIES_MAX; NULL with
 * n > 0; slab groups and slab ranks; sparse-emitter (PVA_OPT_STREAMING_ANALYSIS) solvers. */
#define PVA_RECORD_QUERIES_MAX 1024
PVA_EXPORT int PvAmdSetRecordQueries(PvAmdSolver* s, const float* xyz, int n);
/* Spectral query records: the three frequency-resolved record kinds further down -- band metrics, modulation, spectrum -- for
 * the same cells, computed INSIDE the run.  `kinds` is a mask of PVA_QSPEC_*, a selector of its own beside PVA_QREC_*: the two
 * selections, their pinned blocks and their launches are independent, and neither invalidates the other.  Every FOLLOWING run of
 * any form (PvAmdRun, PvAmdRunAsync, PvAmdRunAsyncAfter, a member of PvAmdRunBatch, a run that PvAmdSync repeats) computes the
 * selected kinds with ONE more launch on the solver's stream, directly behind the launch of the PVA_QREC_* kinds and in front of
 * the run's last kernel, straight into pinned host memory: one wave per 64 queries and per block of bands (band metrics), per
 * band (modulation) and per slice of 8 or 16 bins (spectrum); no pass over the history window, no per-cell device storage, no
 * host synchronisation.  The cells are those of the record queries (PvAmdSetRecordQueries) when there are any, else those of the
 * output queries.  PvAmdGetQueriedSpectralRecords waits for the run and then copies ONE kind's records from pinned memory without
 * GPU work: nQueries x PvAmdQuerySpectralFloats(kind) floats, one record after the other in query order, each record in the
 * layout of the whole-map read-back at one position -- band after band of 12 floats (PvAmdBandMetrics), band after band of 15
 * floats (PvAmdModulation), bin after bin of {re, im, level}.
 *   A record is bit for bit what PvAmdGetBandMetrics / PvAmdGetModulation / PvAmdGetSpectrum return at the query's position
 * after the whole-map pass on the same run.  A query off the map gives NaNs, and so does a query whose cell has no onset in that
 * run; the call returns 0 for them.  The bands, modulation frequencies and bins are those in force when the run was enqueued and
 * the record sizes follow them.  PvAmdSetBands, PvAmdSetModulationFrequencies and PvAmdSetSpectrumBins wait for a run in flight
 * as before; while a kind that depends on them is selected they also invalidate the in-run records until the next run has
 * completed, and clearing the bands or the bins (n = 0) is refused.  The device tables are uploaded by the selector and by these
 * setters, never by a run.
 *   kinds = 0, the default, clears the selection and frees the pinned block (at most 312 floats per query, for at least 64
 * queries, growing with the record queries): nothing is launched, and a run's launches are exactly those of a solver that never
 * called this.
 *   Refused with -1 and nothing changed, PvAmdLastError "spectral records: ...": an unknown bit; sparse-emitter
 * (PVA_OPT_STREAMING_ANALYSIS) solvers; PVA_OPT_SKIP_ANALYSIS; slab groups and slab ranks; a band kind with no bands set; the
 * spectrum kind with no bins set.  PvAmdGetQueriedSpectralRecords is refused when the kind is not selected (or is not exactly one
 * bit), nQueries differs from the registered count, no run has completed since the kinds, the queries or the kind's settings
 * changed, or the last run ended in error.  PvAmdQuerySpectralFloats: floats per query of ONE kind under the current settings, -1
 * where it has none. */
#define PVA_QSPEC_BAND_METRICS 1u   /* 12 floats per band of PvAmdSetBands      (PvAmdBandMetrics) */
#define PVA_QSPEC_MODULATION   2u   /* 15 floats per band of PvAmdSetBands      (PvAmdModulation)  */
#define PVA_QSPEC_SPECTRUM     4u   /* 3 floats per bin of PvAmdSetSpectrumBins (re, im, level)    */
PVA_EXPORT int PvAmdSetQuerySpectralRecords(PvAmdSolver* s, unsigned kinds);
PVA_EXPORT unsigned PvAmdGetQuerySpectralKinds(PvAmdSolver* s);
PVA_EXPORT int PvAmdQuerySpectralFloats(PvAmdSolver* s, unsigned kind);
PVA_EXPORT int PvAmdGetQueriedSpectralRecords(PvAmdSolver* s, unsigned kind, float* out, int nQueries);
/* Emitter records: the same nine record kinds for the registered emitters (PvAmdSetEmitters) of a sparse-emitter
 * (PVA_OPT_STREAMING_ANALYSIS) solver, the mode the selectors above refuse because it keeps a ring of pressure planes instead of
 * the history.  `timeKinds` is a mask of PVA_QREC_*, `spectralKinds` one of PVA_QSPEC_*; both are set by the one call, and both 0
 * (the default) clears the selection.  While a kind is selected every accumulate pass of a run also copies the emitters' cells
 * -- and, for PVA_QREC_LATERAL, PVA_QREC_ECHOGRAM and PVA_QREC_LOBES, their neighbours (X - 1, Y) and (X, Y - 1) -- from the ring
 * into record traces on the device, laid out as history planes: T x P floats, P = the emitters rounded up to a multiple of 64,
 * times 3 with the neighbour columns (104 MB at T = 25 432 and 1024 emitters, 312 MB with the neighbours; allocated only while
 * a kind is selected, growing with the emitter table).  Behind the run's finalize pass the launches of PvAmdSetQueryRecords and
 * PvAmdSetQuerySpectralRecords -- the same kernels, one wave per kind (or work item) and 64 emitters -- walk the traces and write
 * the records straight into pinned host memory.
 *   Record i belongs to the i-th emitter that PvAmdSetEmitters KEPT (it drops positions off the map: PvAmdGetEmitterCells says
 * which cell became which index), and is bit for bit what PvAmdGet<Kind> returns at that cell after PvAmdCompute<Kind> on a
 * solver that keeps its history, for the same scene and listener.  An emitter in a wall or without an onset gives NaNs.  The
 * settings (echogram slots, lobe windows, bands, modulation frequencies, bins) are those in force when the run was enqueued.
 * PvAmdGetEmitterRecords waits for the run and copies ONE kind of ONE family (0: PVA_QREC_*, 1: PVA_QSPEC_*) from pinned memory:
 * nEmitters x PvAmdEmitterRecordFloats(family, kind) floats.  With no kind selected a run enqueues exactly what it enqueued
 * before these calls existed; with kinds selected the result map, the onset map and PvAmdGetOutput keep every bit.
 *   Refused with -1 and nothing changed, PvAmdLastError "emitter records: ...": a solver that is not in sparse-emitter mode (use
 * PvAmdSetQueryRecords there); slab groups and slab ranks; PVA_OPT_SKIP_ANALYSIS; an unknown bit; a kind whose setting is
 * missing (echogram slots, bands, bins) or whose sampling rate is too low, as for the selectors above; more than
 * PVA_RECORD_QUERIES_MAX registered emitters -- and PvAmdSetEmitters with more than that many while a kind is selected.
 * PvAmdGetEmitterRecords is refused when the kind is not selected (or is not exactly one bit), nEmitters differs from the kept
 * count, no run has completed since the kinds, the emitters or the kind's settings changed, or the last run ended in error.
 *   PvAmdGetEmitterCells: returns the kept emitters' count and writes the first min(count, cap) result cells as {cx, cy} pairs.
 *   PvAmdCopyEmitterTrace: the pressure of kept emitter `emitter` at every step of the last run (T floats, PvAmdGetInfo), the
 * impulse response PvAmdGetImpulseResponse cannot give in this mode; it needs no kind selected. */
PVA_EXPORT int PvAmdSetEmitterRecords(PvAmdSolver* s, unsigned timeKinds, unsigned spectralKinds);
PVA_EXPORT int PvAmdGetEmitterRecordKinds(PvAmdSolver* s, unsigned* timeKinds, unsigned* spectralKinds);
PVA_EXPORT int PvAmdEmitterRecordFloats(PvAmdSolver* s, int family, unsigned kind);
PVA_EXPORT int PvAmdGetEmitterRecords(PvAmdSolver* s, int family, unsigned kind, float* out, int nEmitters);
PVA_EXPORT int PvAmdGetEmitterCells(PvAmdSolver* s, int* cxcy, int cap);
PVA_EXPORT int PvAmdCopyEmitterTrace(PvAmdSolver* s, int emitter, float* outT);
/* Whole result map: res8 = gx*gy*8 floats in AnalyzerResult order (Analyzer.h:13-21), delay = gx*gy */
PVA_EXPORT int PvAmdCopyResults(PvAmdSolver* s, float* res8, float* delay);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records / onsets, row-major (either may be NULL) */
PVA_EXPORT int PvAmdCopyResultsBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* res8, float* delay);
/* Planeverb::GetImpulseResponse (FDTD.cpp:60-70): T x {pr, vx, vy} at array cell (cx, cy) */
PVA_EXPORT int PvAmdGetImpulseResponse(PvAmdSolver* s, int cx, int cy, float* out3T);
/* the same as T reference Cells (pr, vx, vy + the cell's b / by), the layout Planeverb::GetImpulseResponse hands out */
PVA_EXPORT int PvAmdGetImpulseResponseCells(PvAmdSolver* s, int cx, int cy, PlaneverbCell* outT);
/* Final fields of the last run, (gx+1)*(gy+1) each, reference order (x*(gy+1)+y) */
PVA_EXPORT int PvAmdCopyFields(PvAmdSolver* s, float* pr, float* vx, float* vy);
/* Recorded pressure plane of step t (zeros where the history was provably zero and not stored) */
PVA_EXPORT int PvAmdCopyHistoryPlane(PvAmdSolver* s, int t, float* pr);
/* The inverse, a test seam like PvAmdSetFields / PvAmdRunSteps: pr = one float per cell in exactly the order and extent
 * PvAmdCopyHistoryPlane(t) returns them (the array cells, x * (gy + 1) + y), written into the recorded plane of step t of the
 * LAST COMPLETED run, so that the analysis passes below can be fed histories the stencil never produces.  A cell that is not
 * stored at step t -- outside the run's history window, or in a tile the pulse had not reached by step t -- is ignored and
 * still reads back as 0.  Waits for a run in flight; marks all nine analysis maps "not computed", as a geometry change does;
 * leaves the run's result map, onset map, first-step table and in-run query records as they are; the next run overwrites the
 * history as always.
 *   One structural rule the passes rely on, and the caller keeps: A CELL'S SAMPLES BEFORE ITS OWN FIRST NON-ZERO RECORDED SAMPLE
 * STAY ZERO.  The velocity passes (lateral fraction, echogram, lobes) start a cell's recurrence at the step the light cone allows,
 * PvAmdGetImpulseResponse at the tile's first stored step; the two agree only where nothing sounds ahead of the wave front.
 *   Records of cells whose own samples (for the velocity kinds: or those of the (X - 1, Y) / (X, Y - 1) neighbours) are not all
 * finite are whatever the definitions below give in IEEE arithmetic; no other cell's record depends on them.
 *   Refused with -1, PvAmdLastError "set history plane: ...": a null handle or plane, t outside [0, T), no completed run, sparse-
 * emitter (PVA_OPT_STREAMING_ANALYSIS) solvers, slab groups and slab ranks. */
PVA_EXPORT int PvAmdSetHistoryPlane(PvAmdSolver* s, int t, const float* pr);
/* ---- Room metrics: clarity C50 / C80, definition D50 and centre time Ts (ISO 3382) of every reached cell ----
 * The recorded pressure of a reached cell is the impulse response from the listener to that cell; PvAmdComputeRoomMetrics
 * reduces the history of the LAST COMPLETED run to one record per cell in one pass on the device (pv_metrics.hip).
 * Definition, for result cell s = X * gy + Y:
 *   onset   t0 = (int)delay[s], delay = the run's own onset map (FLT_MAX: not reached);
 *   p(t)    = the recorded pressure, exactly what PvAmdCopyHistoryPlane(t) returns at array cell (X, Y); 0 for t >= T;
 *   e(t)    = p(t) * p(t);   n50 = (int)(0.05f * (float)fs),  n80 = (int)(0.08f * (float)fs);   k = t - t0, t = t0 .. T - 1;
 *   e50 = sum e(t) over k < n50      l50 = sum e(t) over k >= n50
 *   e80 = sum e(t) over k < n80      l80 = sum e(t) over k >= n80
 *   total = sum e(t)                 moment = sum ((float)k * e(t))
 *   c50 = 10.0f * log10f(e50 / l50)  c80 = 10.0f * log10f(e80 / l80)   (dB)
 *   d50 = e50 / (e50 + l50)          ts  = (moment / total) / (float)fs  (seconds)
 * All arithmetic is float32; every product and every sum is rounded on its own; every sum is sequential in increasing t from
 * +0.0f; division is correctly rounded; log10f is glibc's.  Nothing is special-cased: a late-onset cell whose late window is
 * empty (t0 + n50 >= T) has l50 = 0, c50 = +inf and d50 = 1.
 * A cell WITHOUT an onset in that run holds ten quiet NaNs.  Unlike the result map (PvAmdCopyResults), nothing is carried over
 * from earlier runs.  Cells inside an edge layer get values like any other cell, as unphysical there as the eight outputs.
 * Device storage: 10 x 4 bytes per cell of the history window (tile-rounded), allocated by the first call, freed with the
 * solver; cells outside the window are unreached by construction.  The records stay valid until the next run, geometry,
 * boundary or layer change on that solver: PvAmdCopyRoomMetrics* / PvAmdGetRoomMetrics then return -1 until computed again.
 * Refused (-1, nothing changed, PvAmdLastError says why): NULL, no completed run, a last run that ended in error, sparse-emitter
 * solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks.
 * On a sparse-emitter solver PvAmdComputeRoomMetrics stays refused (there is no history), but the records of the LABELLED cells
 * can be accumulated inside the run: PvAmdSetZoneMaps(PVA_ZMAP_ROOM_METRICS) below; the three read-backs then serve that map. */
typedef struct PvAmdRoomMetrics {
    float c50, c80, d50, ts, e50, l50, e80, l80, total, moment;
} PvAmdRoomMetrics;
/* Compute the room metrics of the LAST COMPLETED run of s (waits for a run in flight; works after PvAmdRun, PvAmdRunAsync +
 * PvAmdSync, PvAmdRunAsyncAfter and a PvAmdRunBatch member, whatever path the run took).  The pass runs on the solver's own
 * stream and is synchronised before the call returns.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeRoomMetrics(PvAmdSolver* s, float* ms);
/* gx*gy*10 floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyRoomMetrics(PvAmdSolver* s, float* out10);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyRoomMetricsBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out10);
/* the record at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives ten NaNs
 * and 0 */
PVA_EXPORT int PvAmdGetRoomMetrics(PvAmdSolver* s, float ex, float ey, float ez, PvAmdRoomMetrics* out);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T; the restatement the tests hold the
 * kernel to */
PVA_EXPORT int PvAmdHostRoomMetrics(const float* p, int T, int fs, int onset, PvAmdRoomMetrics* out);
/* ---- Decay times: EDT, T20 and T30 (ISO 3382) of every reached cell, read off the backward-integrated (Schroeder) curve ----
 * PvAmdComputeDecayTimes reduces the history of the LAST COMPLETED run to one record per cell on the device (pv_decay.hip):
 * the one pass that walks the history backwards in time, and it walks it twice (E0 is needed before the first ratio).
 * Definition, for result cell s = X * gy + Y, with p(t) exactly what PvAmdCopyHistoryPlane(t) returns at array cell (X, Y)
 * and delay the run's own onset map:
 *   t0    = (int)delay[s]                      (FLT_MAX: not reached)
 *   tailN = (int)(0.01f * (float)fs)           (the reference's PV_SCHROEDER_OFFSET_S rule: the curve's last 10 ms dip
 *   tEnd  = T - tailN                           towards 0 because the record ends, and enter no fit)
 *   e(t)  = p(t) * p(t)                                                        float32
 *   E(T)  = +0.0f;  E(t) = E(t + 1) + e(t),  t = T-1 down to t0                float32, sequential in DECREASING t
 *   E0    = E(t0)
 *   r(t)  = E(t) / E0                          correctly rounded float32 division;  r(t0) == 1.0f
 *   L(t)  = 10.0f * log10f(r(t))               glibc's log10f
 *   k     = t - t0
 *   ranges (hi, lo), as float literals:
 *      EDT  (1.0f,        0.1f)                 0 .. -10 dB
 *      T20  (0.31622776f, 0.0031622776f)       -5 .. -25 dB
 *      T30  (0.31622776f, 0.00031622776f)      -5 .. -35 dB
 *   a step t in [t0, tEnd) belongs to a range iff  r(t) <= hi && r(t) >= lo
 *   per range, over its steps in DECREASING t:
 *      n    = their number;  kmax / kmin = largest / smallest k among them
 *      Sy   = sum (double)L(t)                  double, from +0.0, every sum rounded on its own
 *      Sky  = sum ((double)k * (double)L(t))    double (the product is exact)
 *      kbar  = ((double)kmin + (double)kmax) * 0.5
 *      slope = (Sky - (kbar * Sy)) / ((((double)n * (((double)n * (double)n) - 1.0))) / 12.0)        dB per step
 *      value = (float)((-60.0 / slope) / (double)fs)                                                  seconds for 60 dB
 *   a range is COMPLETE iff  t0 < tEnd  &&  r(tEnd - 1) < lo     (the curve fell below the lower limit before the tail)
 *   value = quiet NaN (0x7fc00000) unless the range is complete and n >= 2; otherwise nothing is special-cased
 *           (slope >= 0 gives -inf or a negative value, as IEEE says)
 *   depth = t0 < tEnd ? L(tEnd - 1) : quiet NaN                   (how deep the usable curve goes, dB)
 *   record (8 floats): edt, t20, t30, (float)n_edt, (float)n_t20, (float)n_t30, E0, depth
 * Because e(t) >= 0, E and therefore r never increase with t: each range's steps form one contiguous interval, kbar is its
 * exact midpoint and n (n^2 - 1) / 12 its exact centred sum of squares -- the reference's own centred regression
 * (Analyzer.cpp:290-294) without a pass that finds the interval first.  The two regression sums are double because
 * Sky - kbar Sy cancels.  Nothing is fused: no FMA, in float or in double.
 * The records describe the recorded T steps only: a decay that has not fallen below a range's lower limit before the tail
 * leaves that range incomplete (NaN) rather than extrapolated.  depth and the three n are there so that a caller can apply a
 * headroom rule of their own, for example require depth <= lower limit - 10 dB.  The reference's rt60 (PvAmdCopyResults) is
 * another quantity -- one float32 regression over the whole curve -- and stays as it is.
 * A cell WITHOUT an onset in that run holds eight quiet NaNs; nothing is carried over from earlier runs.  Cells inside an edge
 * layer get records like any other cell, as unphysical there as their other outputs.
 * Device storage: 8 x 4 bytes per cell of the history window (tile-rounded), allocated by the first call, freed with the
 * solver; cells outside the window are unreached by construction.  The records stay valid until the next run, geometry,
 * boundary or layer change on that solver: PvAmdCopyDecayTimes* / PvAmdGetDecayTimes then return -1 until computed again.
 * Room metrics, spectrum and decay times do not invalidate each other.
 * Refused (-1, nothing changed, PvAmdLastError says why, "decay times: ..."): NULL, no completed run, a last run that ended in
 * error, sparse-emitter solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks. */
typedef struct PvAmdDecayTimes {
    float edt, t20, t30, n_edt, n_t20, n_t30, e0, depth;
} PvAmdDecayTimes;
/* Compute the decay times of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeRoomMetrics).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeDecayTimes(PvAmdSolver* s, float* ms);
/* gx*gy*8 floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyDecayTimes(PvAmdSolver* s, float* out8);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyDecayTimesBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out8);
/* the record at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives eight NaNs
 * and 0 */
PVA_EXPORT int PvAmdGetDecayTimes(PvAmdSolver* s, float ex, float ey, float ez, PvAmdDecayTimes* out);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T (refused otherwise); the restatement
 * the tests hold the kernel to */
PVA_EXPORT int PvAmdHostDecayTimes(const float* p, int T, int fs, int onset, PvAmdDecayTimes* out);
/* ---- Lateral energy fraction and early-sound direction: the spatial measure of ISO 3382-1 (LF, A.2) of every reached cell ----
 * The share of the first 80 ms of energy that arrives from the side, as seen by a figure-of-eight microphone whose null points
 * at the source -- here: along the direction the early sound travels in.  A pressure-only tool cannot compute it; an FDTD
 * solver can, because the particle velocity is part of its state.  PvAmdComputeLateralFraction reduces the history of the LAST
 * COMPLETED run to one record per cell on the device (pv_lateral.hip), re-deriving vx, vy of every reached cell from the
 * recorded pressure with the stencil's own recurrence through the whole window.
 * Definition, for result cell s = X * gy + Y, with delay the run's own onset map and p(t), vx(t), vy(t) exactly what
 * PvAmdGetImpulseResponse returns for array cell (X, Y).  vx, vy are the library's velocity of a cell:
 *   on an air|air face     v(t) = v(t - 1) - C * (p(t)[cell] - p(t)[neighbour])      neighbours (X - 1, Y) for vx, (X, Y - 1) for vy
 *   otherwise              v(t) = k * (p(t)[cell] + p(t)[neighbour])                 k the face's wall coefficient
 *   the recurrence starts from 0 at the cell's first recorded sample, not at its onset.
 * Inside an edge layer this is the UNDAMPED recurrence (the layer's damping of the velocity is not applied), as it already is
 * for the source directivity of the eight outputs.
 *   onset = (int)delay[s]                      (FLT_MAX: not reached)
 *   n5    = (int)(0.005f * (float)fs)          the direct sound: the first 5 ms give the direction
 *   n80   = (int)(0.08f * (float)fs)
 *   tEnd  = min(onset + n80, T)
 *   for t = onset .. tEnd - 1, k = t - onset, every sum float32, sequential in increasing t from +0.0f:
 *      e80 = e80 + p*p
 *      fx  = fx  + (k <  n5 ? p*vx  : 0.f)      fy  = fy  + (k <  n5 ? p*vy  : 0.f)
 *      sxx = sxx + (k >= n5 ? vx*vx : 0.f)      sxy = sxy + (k >= n5 ? vx*vy : 0.f)      syy = syy + (k >= n5 ? vy*vy : 0.f)
 *   norm = sqrtf(fx*fx + fy*fy);  dx = fx / norm;  dy = fy / norm
 *   lat  = ((sxx * (dy*dy)) - (2.0f * (sxy * (dx*dy)))) + (syy * (dx*dx))
 *   lf   = lat / e80
 *   record (11 floats): lf, dir_x, dir_y, n = (float)(tEnd - onset), e80, lateral, fx, fy, sxx, sxy, syy
 * Every product, sum and quotient is rounded on its own (no FMA).  lat is the energy of the velocity component perpendicular
 * to (dx, dy) over the steps after the direct sound: the three second moments make it a quadratic form in the direction, which
 * therefore need not be known while the window is walked.  Pressure and velocity are in the solver's own units, so lf is the
 * library's measure, comparable between cells and scenes of one resolution; an open field reads near 0, a closed room 0.1 .. 0.5,
 * and values above 1 occur beside walls and at pressure nodes and are kept.
 * (dx, dy) is the direction in which the early sound TRAVELS at the cell (away from the listener); it is not negated as the
 * source directivity of the eight outputs is.
 * Nothing is special-cased: a zero flux gives NaN for dx, dy and lf (the sums stay numbers), and a window cut off by T is
 * reported through n < n80.
 * A cell WITHOUT an onset in that run holds eleven quiet NaNs; nothing is carried over from earlier runs.  Cells inside an edge
 * layer get records like any other cell.
 * Device storage: 11 x 4 bytes per cell of the history window (tile-rounded), allocated by the first call, freed with the
 * solver.  The records stay valid until the next run, geometry, boundary or layer change on that solver:
 * PvAmdCopyLateralFraction* / PvAmdGetLateralFraction then return -1 until computed again.  Room metrics, spectrum, decay times
 * and lateral fraction do not invalidate each other.
 * Refused (-1, nothing changed, PvAmdLastError says why, "lateral fraction: ..."): NULL, no completed run, a last run that ended
 * in error, sparse-emitter solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks. */
typedef struct PvAmdLateralFraction {
    float lf, dir_x, dir_y, n, e80, lateral, fx, fy, sxx, sxy, syy;
} PvAmdLateralFraction;
/* Compute the lateral-fraction records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run,
 * as PvAmdComputeRoomMetrics).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeLateralFraction(PvAmdSolver* s, float* ms);
/* gx*gy*11 floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyLateralFraction(PvAmdSolver* s, float* out11);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyLateralFractionBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out11);
/* the record at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives eleven NaNs
 * and 0 */
PVA_EXPORT int PvAmdGetLateralFraction(PvAmdSolver* s, float ex, float ey, float ez, PvAmdLateralFraction* out);
/* CPU only: the definition above applied to one impulse response p[T], vx[T], vy[T] with 0 <= onset < T (refused otherwise);
 * the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostLateralFraction(const float* p, const float* vx, const float* vy, int T, int fs, int onset,
                                        PvAmdLateralFraction* out);
/* ---- Directional echogram: the energy and the flux of every reached cell per time slot after its onset ----
 * Every record above folds the impulse response into a few scalars; none says WHEN the energy arrives after the direct sound
 * and FROM WHERE.  The echogram (energy-time curve) does, one tap per time slot with a gain and a direction -- what a room-
 * acoustics user looks at first and what an early-reflection renderer is driven by.  The energy per slot a pressure-only tool
 * can give; the direction each slot's sound travels in needs the particle velocity.  PvAmdComputeEchogram reduces the history of
 * the LAST COMPLETED run to 1 + 3 nSlots floats per cell on the device (pv_echogram.hip), with the velocity recurrence of the
 * lateral-fraction pass carried through the window the caller chooses.  It touches no run and no result map.
 * Slots: nSlots of them, 0 .. PVA_ECHOGRAM_MAX_SLOTS, each of
 *   ns = (int)(slotSeconds * (float)fs)        in float32 -- the expression of n5 above, so slotSeconds = 0.005f gives ns == n5
 * steps.  nSlots = 0 clears the setting and frees the device storage.  Refused with -1 and nothing changed unless slotSeconds is
 * finite and 1 <= ns <= (1 << 20).
 * Definition, for result cell s = X * gy + Y, with delay the run's own onset map and p(t), vx(t), vy(t) exactly what
 * PvAmdGetImpulseResponse returns for array cell (X, Y) -- the library's velocity, the UNDAMPED recurrence of the lateral-fraction
 * section above, started from 0 at the cell's first recorded sample:
 *   onset = (int)delay[s]                      (FLT_MAX: not reached)
 *   tEnd  = min(onset + ns * nSlots, T)
 *   for t = onset .. tEnd - 1,  k = t - onset,  j = k / ns        (integer division; 0 <= j < nSlots)
 *      e[j]  = e[j]  + (p * p)
 *      ix[j] = ix[j] + (p * vx)
 *      iy[j] = iy[j] + (p * vy)
 *   record (1 + 3 nSlots floats): n = (float)(tEnd - onset), then e[0], ix[0], iy[0], e[1], ix[1], iy[1], ...
 * Everything is float32, every product and sum rounded on its own (no FMA); every slot's three sums start at +0.0f and are
 * sequential in increasing t.  Nothing is special-cased: a slot the record does not reach (onset + j * ns >= T) holds three
 * +0.0f, a slot cut by T holds its partial sums, and n < ns * nSlots reports either case.
 * (ix[j], iy[j]) is the net direction in which slot j's sound TRAVELS (away from its source); it is neither negated nor
 * normalised: a caller normalises it, and negates it for a direction of arrival.  Levels, 10 log10(e[j] / e[0]), are left to
 * the caller, and so is any picking of discrete reflections: the pulse is band-limited, and local maxima of the slot energies
 * are mostly its ringing.
 * A cell WITHOUT an onset in that run holds 1 + 3 nSlots quiet NaNs (0x7fc00000); nothing is carried over from earlier runs.
 * Cells inside an edge layer get records like any other cell.
 * Device storage: (1 + 3 nSlots) x 4 bytes per cell of the history window, allocated by the first PvAmdComputeEchogram (again
 * when nSlots changes), freed by PvAmdSetEchogram(..., 0) and with the solver.  The records stay valid until the next run, a
 * geometry, boundary or layer change, or a PvAmdSetEchogram call on that solver: PvAmdCopyEchogram* / PvAmdGetEchogram then
 * return -1 until computed again.  The echogram and the five record kinds above and below (room metrics, spectrum, decay times,
 * lateral fraction, band metrics) do not invalidate each other.
 * Refused (-1, nothing changed, PvAmdLastError says why, "echogram: ..."): NULL, no slots set ("echogram: no slots set"), no
 * completed run, a last run that ended in error, sparse-emitter solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab
 * groups and slab ranks. */
#define PVA_ECHOGRAM_MAX_SLOTS 32
/* Set (nSlots > 0) or clear (nSlots = 0: the device storage is freed) the slots; waits for a run in flight */
PVA_EXPORT int PvAmdSetEchogram(PvAmdSolver* s, float slotSeconds, int nSlots);
/* returns nSlots; slotSeconds as set and ns to *slotSeconds and *slotSteps (both optional; untouched when no slots are set) */
PVA_EXPORT int PvAmdGetEchogramSlots(PvAmdSolver* s, float* slotSeconds, int* slotSteps);
/* Compute the echogram records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeLateralFraction).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeEchogram(PvAmdSolver* s, float* ms);
/* gx*gy*(1+3n) floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyEchogram(PvAmdSolver* s, float* out);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyEchogramBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out);
/* the record (1+3n floats) at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives
 * NaNs and 0 */
PVA_EXPORT int PvAmdGetEchogram(PvAmdSolver* s, float ex, float ey, float ez, float* out);
/* CPU only: the definition above applied to one impulse response p[T], vx[T], vy[T] with 0 <= onset < T and 1 <= nSlots <=
 * PVA_ECHOGRAM_MAX_SLOTS (refused otherwise, as a slotSeconds PvAmdSetEchogram would refuse at that fs); out: 1 + 3 nSlots
 * floats; the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostEchogram(const float* p, const float* vx, const float* vy, int T, int fs, int onset,
                                 float slotSeconds, int nSlots, float* out);
/* ---- Echo criterion (Dietsch and Kraak, Acustica 60, 1986; the "EK" of room-acoustics programs), speech and music ----
 * Will this position hear a distinct echo, and at what delay?  The echogram above leaves picking to the caller because local
 * maxima of its slot energies are mostly the band-limited pulse's ringing.  The echo criterion tracks the running centre time of
 * the |p|^n-weighted response and takes its difference quotient over a short window, which smooths the ringing away by
 * construction, and it comes with published thresholds.  PvAmdComputeEchoCriterion reduces the history of the LAST COMPLETED run
 * to one record of ten floats per cell in one forward pass on the device (pv_echo.hip).  It touches no run and no result map.
 * Definition, for result cell s = X * gy + Y:
 *   onset   t0 = (int)delay[s], delay = the run's own onset map (FLT_MAX: not reached);
 *   p(t)    = the recorded pressure, exactly what PvAmdCopyHistoryPlane(t) returns at array cell (X, Y);
 *   k = t - t0 for t = t0 .. T - 1,   N = T - t0,   a(t) = fabsf(p(t));
 *   variant   weight w(t)                              lag nD                       echo limit nL
 *   speech    powf(a, PVA_ECHO_SPEECH_EXPONENT)        (int)(0.009f * (float)fs)    n50 = (int)(0.05f * (float)fs)
 *   music     a                                        (int)(0.014f * (float)fs)    n80 = (int)(0.08f * (float)fs)
 * and per variant, sequential in increasing k from +0.0f:
 *   A(k) = A(k-1) + w                     B(k) = B(k-1) + ((float)k * w)
 *   c(k) = B(k) / A(k)                                            (centre of the build-up, in steps)
 *   x(k) = (c(k) - (k >= nD ? c(k - nD) : +0.0f)) / (float)nD
 *   ek, kk         start at +0.0f, 0;   if (x(k) > ek) { ek = x(k); kk = k; }                          for every k
 *   ekLate, kkLate start at +0.0f, 0;   if (k >= nL && x(k) > ekLate) { ekLate = x(k); kkLate = k; }
 *   ts = c(N - 1) / (float)fs
 *   record (5 floats): ek, (float)kk / (float)fs, ekLate, (float)kkLate / (float)fs, ts
 * The whole record is the speech variant's five floats, then the music variant's (PvAmdEchoCriterion).
 * All arithmetic is float32; every product, sum and quotient is rounded on its own (no FMA); division is correctly rounded; powf
 * is glibc's.  The comparison is strict: the first maximum wins and a NaN x never does.  Nothing is special-cased: A = 0 gives
 * 0 / 0 as IEEE says (an all-zero response has ek = +0 and ts = NaN), and a response shorter than nL leaves ekLate = +0,
 * kkLate = 0.
 * Reading the values: a position is said to hear an echo where ek exceeds PVA_ECHO_SPEECH_CRIT (speech) or PVA_ECHO_MUSIC_CRIT
 * (music), for half of the listeners; tk says at which delay after the direct sound.  CAVEAT: the published thresholds were
 * derived for test signals of 700 - 1400 Hz (speech) and 700 - 2800 Hz (music).  Here the response is the grid's band-limited
 * one, and at the low presets the direct pulse alone is a good part of nD wide: in an empty, open scene it reaches ek of about
 * 0.75 - 0.96 by itself.  ekLate / tkLate, the maximum over k >= nL only, is the part that lies past the fusion limit
 * (50 ms / 80 ms), where the direct pulse's own build-up no longer counts.
 * A cell WITHOUT an onset in that run holds ten quiet NaNs; nothing is carried over from earlier runs.  Cells inside an edge
 * layer get records like any other cell.
 * Device storage: 10 x 4 bytes per cell of the history window, allocated by the first call, freed with the solver.  The records
 * stay valid until the next run, geometry, boundary or layer change on that solver: PvAmdCopyEchoCriterion* /
 * PvAmdGetEchoCriterion then return -1 until computed again.  The echo criterion and the seven other record kinds (room metrics,
 * spectrum, decay times, lateral fraction, echogram, lobes, band metrics) do not invalidate each other.
 * Refused (-1, nothing changed, PvAmdLastError says why, "echo: ..."): what the room metrics refuse (NULL, no completed run, a
 * last run that ended in error, sparse-emitter solvers, PVA_OPT_SKIP_ANALYSIS, slab groups and slab ranks), and a sampling rate
 * whose speech lag is below one step, (int)(0.009f * (float)fs) < 1, i.e. fs < 112. */
#define PVA_ECHO_SPEECH_EXPONENT 0.6666667f /* (float)(2.0 / 3.0) */
#define PVA_ECHO_SPEECH_CRIT 1.0f
#define PVA_ECHO_MUSIC_CRIT 1.8f
typedef struct PvAmdEchoCriterion {
    float sEk, sTk, sEkLate, sTkLate, sTs, mEk, mTk, mEkLate, mTkLate, mTs;
} PvAmdEchoCriterion;
/* Compute the echo-criterion records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run,
 * as PvAmdComputeRoomMetrics).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeEchoCriterion(PvAmdSolver* s, float* ms);
/* gx*gy*10 floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyEchoCriterion(PvAmdSolver* s, float* out10);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyEchoCriterionBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out10);
/* the record at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives ten NaNs
 * and 0 */
PVA_EXPORT int PvAmdGetEchoCriterion(PvAmdSolver* s, float ex, float ey, float ez, PvAmdEchoCriterion* out);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T and a sampling rate the criterion
 * accepts (fs >= 112); the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostEchoCriterion(const float* p, int T, int fs, int onset, PvAmdEchoCriterion* out);
/* ---- Directional energy lobes: the energy of every reached cell per time window, split over four axial travel directions ----
 * In which directions does the energy of a response travel, and when?  sourceDirectivity is one vector from the first
 * milliseconds, the lateral fraction one scalar for the first 80 ms, and the echogram's flux is a NET vector per slot: two
 * reflections that cross a cell from opposite sides within one slot cancel in it, and a diffuse tail has a net flux near 0
 * whatever its directional balance.  The lobes keep opposite directions apart: each sample's energy p^2 is split over the x and
 * the y axis by the squared direction cosines of the particle velocity (cos^2 weights, which add up to 1), and goes to the lobe
 * of the sign in which the sound travels along that axis.  Four lobes, +x, -x, +y, -y, per time window; a few windows of unequal
 * lengths after each cell's onset (direct, early, late by default).  PvAmdComputeLobes reduces the history of the LAST COMPLETED
 * run to 1 + 5 nW floats per cell on the device (pv_lobes.hip), with the velocity recurrence of the lateral-fraction pass carried
 * through the whole response.  It touches no run and no result map.
 * Windows: nEdges edges in seconds, 0 <= nEdges <= PVA_LOBES_MAX_EDGES, with step counts
 *   n_i = (int)(edge_i * (float)fs)            in float32 -- the expression of n5 / n80 above.
 * Refused with -1 and nothing changed unless every edge is finite, n_0 >= 1, every n_i <= (1 << 20) and the n_i are strictly
 * increasing.  nW = nEdges + 1 windows; with k = t - onset, window 0 is k < n_0, window j is n_(j-1) <= k < n_j, and the last
 * window is k >= n_last, up to T - 1.  A solver on which no windows were ever set uses the default edges {0.01f, 0.08f}
 * (direct, early, late); nEdges = 0 (edgesSeconds is then not read and may be NULL) restores that default, also in
 * PvAmdHostLobes.
 * Definition, for result cell s = X * gy + Y, with delay the run's own onset map and p(t), vx(t), vy(t) exactly what
 * PvAmdGetImpulseResponse returns for array cell (X, Y) -- the library's velocity, the UNDAMPED recurrence of the lateral-fraction
 * section above, started from 0 at the cell's first recorded sample:
 *   onset = (int)delay[s]                      (FLT_MAX: not reached)
 *   for t = onset .. T - 1,  k = t - onset,  w = the window k lies in:
 *      e = p * p;   a = vx * vx;   b = vy * vy;   q = a + b
 *      E[w] = E[w] + e
 *      if (q > 0.0f) {
 *         ex = e * (a / q);   ey = e * (b / q)
 *         if ((vx > 0.0f) == (p > 0.0f)) XP[w] = XP[w] + ex;  else XN[w] = XN[w] + ex;
 *         if ((vy > 0.0f) == (p > 0.0f)) YP[w] = YP[w] + ey;  else YN[w] = YN[w] + ey;
 *      }
 *   record (1 + 5 nW floats): n = (float)(T - onset), then E, XP, XN, YP, YN of window 0, of window 1, ...
 * Everything is float32; every product, sum and quotient is rounded on its own (no FMA); division is correctly rounded; every
 * sum starts at +0.0f and is sequential in increasing t.  Nothing else is special-cased: a sample with q == 0 adds to E only
 * (the caller sees it as E - (XP + XN + YP + YN)), a window the response does not reach holds five +0.0f, and a NaN or Inf
 * input propagates as IEEE says.  The sign test uses the signs of p and v, not the product p * v, so an underflowing product
 * cannot move energy to the wrong lobe.
 * Meaning: XP is the energy of window w carried by sound that TRAVELS towards +x at the cell (array rows; away from the
 * listener's side of the path); like dir of the lateral fraction and the echogram's flux it is not negated.  By reciprocity --
 * the run's source is the listener, so the response recorded at a cell is the response at the listener to an emitter at that
 * cell -- it is the energy an emitter at the cell sends to the listener by radiating towards -x.  PvAmdLobeGains below uses
 * that reading to apply an emitter's directivity pattern to the reverberant path, per window.
 * Per window of N steps the four lobes add up to E within  |(XP + XN + YP + YN) - E| <= (N + 8) * 2^-23 * E  wherever no sample
 * has q == 0: all terms are non-negative, each sample's ex + ey differs from e by a few ulp, and a sequential float32 sum of N
 * non-negative terms has a relative error of at most N * 2^-24.
 * A cell WITHOUT an onset in that run holds 1 + 5 nW quiet NaNs (0x7fc00000); nothing is carried over from earlier runs.
 * Cells inside an edge layer get records like any other cell.
 * Device storage: (1 + 5 nW) x 4 bytes per cell of the history window, allocated by the first compute call (again when nW
 * changes), freed with the solver.  The records stay valid until the next run, a geometry, boundary or layer change, or a
 * window-setting call on that solver: the copy and point calls then return -1 until computed again.  The lobes and the seven
 * other record kinds (room metrics, spectrum, decay times, lateral fraction, echogram, echo criterion, band metrics) do not
 * invalidate each other.
 * Refused (-1, nothing changed, PvAmdLastError says why, "lobes: ..."): NULL, no completed run, a last run that ended in error,
 * sparse-emitter solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks, a block outside the
 * map, and the default windows at a sampling rate below 100 Hz. */
#define PVA_LOBES_MAX_EDGES 7
/* Set the window edges (nEdges > 0) or restore the default (nEdges = 0); waits for a run in flight */
PVA_EXPORT int PvAmdSetLobeWindows(PvAmdSolver* s, const float* edgesSeconds, int nEdges);
/* returns nEdges; the edges as set (or the default) and their step counts to edgesSeconds[nEdges] and edgeSteps[nEdges] (both
 * optional; room for PVA_LOBES_MAX_EDGES is always enough) */
PVA_EXPORT int PvAmdGetLobeWindows(PvAmdSolver* s, float* edgesSeconds, int* edgeSteps);
/* Compute the lobe records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeEchogram).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeLobes(PvAmdSolver* s, float* ms);
/* gx*gy*(1+5nW) floats, AoS records, cell s = X*gy + Y */
PVA_EXPORT int PvAmdCopyLobes(PvAmdSolver* s, float* out);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc records, row-major */
PVA_EXPORT int PvAmdCopyLobesBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out);
/* the record (1+5nW floats) at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map
 * gives NaNs and 0 */
PVA_EXPORT int PvAmdGetLobes(PvAmdSolver* s, float ex, float ey, float ez, float* out);
/* CPU only: the definition above applied to one impulse response p[T], vx[T], vy[T] with 0 <= onset < T, fs > 0 and edges that
 * the window-setting call would accept at that fs (refused otherwise); out: 1 + 5 (nEdges + 1) floats (16 for nEdges = 0, the
 * default edges); the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostLobes(const float* p, const float* vx, const float* vy, int T, int fs, int onset,
                              const float* edgesSeconds, int nEdges, float* out);
/* CPU only: an emitter's directivity pattern applied to the reverberant path, per window of one lobe record (1 + 5 nWindows
 * floats).  pattern 0 = omni, 1 = cardioid; (fwdX, fwdY) is the emitter's forward in the (x, z) plane, used as given (the caller
 * normalises it).  In float32, each operation rounded on its own:
 *   c(d)  = pattern == 0 ? 1.0f : max((1.0f + d) / 2.0f, 0.01f)
 *   wXP = c(-fwdX),  wXN = c(fwdX),  wYP = c(-fwdY),  wYN = c(fwdY)         (emission direction = minus travel direction)
 *   gains[w] = ((((XP * (wXP*wXP)) + (XN * (wXN*wXN))) + (YP * (wYP*wYP))) + (YN * (wYN*wYN))) / (((XP + XN) + YP) + YN)
 * gains[w] is an ENERGY ratio; the amplitude factor is its square root and is left to the caller.  0 / 0 gives NaN as IEEE says
 * (a window without directional energy).  Refused (-1) for NULL, nWindows outside 1 .. 8, or a pattern other than 0 / 1. */
PVA_EXPORT int PvAmdLobeGains(const float* record, int nWindows, float fwdX, float fwdY, int pattern, float* gains);
/* ---- Band metrics: decay times and clarity of every reached cell per octave or third-octave band ----
 * The records above are broadband: the decay of a cell is that of whichever part of the pulse's band decays slowest there.
 * PvAmdComputeBandMetrics filters each reached cell's recorded pressure into the bands set by PvAmdSetBands and reduces every
 * band's output to one record of twelve floats on the device (pv_bands.hip).  It touches no run and no result map.
 * Bands: n centres fc (Hz), 0 <= n <= PVA_BANDS_MAX, and fraction 1 (octave) or 3 (third octave); in double
 *   f1 = fc * 2^(-1 / (2 fraction)),  f2 = fc * 2^(+1 / (2 fraction));  refused unless fc is finite, f1 > 0 and f2 < fs / 2
 * Filter: a 4th-order Butterworth band-pass, designed on the host in double (host libm):
 *   the order-2 low-pass prototype (poles exp(+-i 3 pi / 4));  W1 = tan(pi f1 / fs), W2 = tan(pi f2 / fs)  (pre-warped edges)
 *   LP -> BP:  s -> (s^2 + W1 W2) / ((W2 - W1) s)   -- two conjugate pole pairs;  bilinear:  z = (1 + s) / (1 - s)
 *   two biquads, one per pole pair, the one whose pole angle |arg z| is smaller FIRST;  per section
 *      a1 = -2 Re z,  a2 = |z|^2,  zeros at z = +1 and z = -1:  b0 = g, b1 = 0, b2 = -g
 *      g  = unit gain at the pre-warped geometric centre  w0 = 2 atan(sqrt(W1 W2))  (|H(exp(i w0))| = 1 for the section)
 *   each coefficient rounded to float32 ONCE: b0, b1, b2, a1, a2 of section 1, then of section 2 -- 10 floats per band.
 *   The whole band-pass has 0 dB at w0 and -3.01 dB at f1 and f2.  PvAmdGetBandCoefs returns exactly what the device uses.
 * Filtering runs BACKWARDS in time (the time-reversed filtering of Jacobsen & Rindel: the filter's own ringing, which would
 * otherwise mask decays shorter than its impulse response, falls before the onset), the direction the Schroeder integral walks.
 * For result cell s = X * gy + Y, with x(t) = p(t) exactly what PvAmdCopyHistoryPlane(t) returns there, t0 = (int)delay[s]:
 *   per section, transposed direct form II, float32, state z1 = z2 = +0.0f at t = T - 1, t = T-1 down to t0:
 *      y  = (b0 * x) + z1
 *      z1 = ((b1 * x) - (a1 * y)) + z2
 *      z2 = (b2 * x) - (a2 * y)
 *   section 2 takes section 1's y as its x;  y(t) = section 2's y.  Every product and sum is rounded on its own (no FMA),
 *   denormals are kept.  The walk STOPS at t0: what the reversed filter would ring out below the onset is not in the record.
 * Record per band (12 floats): edt, t20, t30, n_edt, n_t20, n_t30, e0, depth, c50, c80, d50, ts
 *   the first eight: PvAmdDecayTimes above, word for word, with  e(t) = y(t) * y(t)  in place of p(t) * p(t)
 *   the last four, with E the same backward curve, k = t - t0, n50 = (int)(0.05f * (float)fs), n80 = (int)(0.08f * (float)fs):
 *      l50    = E(min(t0 + n50, T))   (a value of the curve itself; +0.0f where t0 + n50 >= T)      l80 likewise
 *      e50    = sum of e(t) over k < n50,  from +0.0f, sequential in DECREASING t                    e80 likewise
 *      moment = sum of ((float)k * e(t)) over all k, likewise
 *      c50 = 10.0f * log10f(e50 / l50),  c80 likewise,  d50 = e50 / (e50 + l50),  ts = (moment / e0) / (float)fs
 *   Nothing is special-cased: a band without energy gives e0 = 0 and what IEEE then gives (NaN ratios).
 * A cell WITHOUT an onset in that run holds 12 n quiet NaNs; nothing is carried over from earlier runs.
 * Device storage: 12 n x 4 bytes per cell of the history window, allocated by the first PvAmdComputeBandMetrics (again when n
 * changes), freed by PvAmdSetBands(n = 0) and with the solver.  Lifetime and refusals are the decay times' ("band metrics: ...");
 * besides, computing or reading with no bands set is refused ("no bands set"), and PvAmdSetBands invalidates the records.  Room
 * metrics, spectrum, decay times, lateral fraction and band metrics do not invalidate each other. */
#define PVA_BANDS_MAX 8
typedef struct PvAmdBandMetrics {
    float edt, t20, t30, n_edt, n_t20, n_t30, e0, depth, c50, c80, d50, ts;
} PvAmdBandMetrics;
/* Set (n > 0) or clear (n = 0: the device storage is freed) the bands; waits for a run in flight.  -1 and nothing changed:
 * centreHz = NULL with n > 0, n outside 0 .. PVA_BANDS_MAX, fraction other than 1 or 3, a centre that is not finite, f1 <= 0 or
 * f2 >= fs / 2 */
PVA_EXPORT int PvAmdSetBands(PvAmdSolver* s, const float* centreHz, int n, int fraction);
/* the number of bands set; the first min(n, cap) centres to centreHz and the fraction to *fraction (both optional) */
PVA_EXPORT int PvAmdGetBands(PvAmdSolver* s, float* centreHz, int cap, int* fraction);
/* the 10 n float32 coefficients the device uses */
PVA_EXPORT int PvAmdGetBandCoefs(PvAmdSolver* s, float* out10n);
/* Compute the band records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeDecayTimes).  Synchronous on the solver's own stream.  *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeBandMetrics(PvAmdSolver* s, float* ms);
/* gx*gy*n*12 floats: cell s = X*gy + Y, then band, then the 12 floats */
PVA_EXPORT int PvAmdCopyBandMetrics(PvAmdSolver* s, float* out12n);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc x n records, row-major */
PVA_EXPORT int PvAmdCopyBandMetricsBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out12n);
/* the n records at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives NaNs and 0 */
PVA_EXPORT int PvAmdGetBandMetrics(PvAmdSolver* s, float ex, float ey, float ez, PvAmdBandMetrics* out12n);
/* CPU only: the coefficients of the design above for a sampling rate fs, without a solver (the same refusals) */
PVA_EXPORT int PvAmdHostBandCoefs(int fs, const float* centreHz, int n, int fraction, float* out10n);
/* CPU only: filter and record above applied to one impulse response p[T] with 0 <= onset < T and n (1 .. PVA_BANDS_MAX)
 * coefficient sets of 10 floats; the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostBandMetrics(const float* p, int T, int fs, int onset, const float* coefs10n, int n, PvAmdBandMetrics* out12n);
/* ---- Modulation: the modulation transfer function and modulation transfer index of every reached cell, per band ----
 * How intelligible speech is at a cell: a room smears the slow intensity modulations (0.63 .. 12.5 Hz) that carry speech, and the
 * modulation transfer function m(F) says by how much (Schroeder 1981; IEC 60268-16, indirect method: m(F) is the normalised
 * Fourier transform of the squared, band-filtered impulse response).  PvAmdComputeModulation reduces the history of the LAST
 * COMPLETED run to 15 floats per band and cell in one walk per band on the device (pv_modulation.hip).  It touches no run and no
 * result map.
 * Settings: the bands of PvAmdSetBands (n bands, their ten float32 coefficients, either fraction) and M = 14 modulation
 * frequencies F[i] (Hz).  The default is the IEC third-octave series 0.63, 0.8, 1, 1.25, 1.6, 2, 2.5, 3.15, 4, 5, 6.3, 8, 10, 12.5.
 * Table (T = the run's steps): built on the host in double with the host libm, row t = 0 .. T - 1, 28 floats per row:
 *   ph = (2.0 * M_PI * (double)F[i] * (double)t) / (double)fs;   row[2 i] = (float)cos(ph),  row[2 i + 1] = (float)sin(ph)
 *   t is the ABSOLUTE step, not t - t0: the magnitude does not depend on the time origin.  The device evaluates no trigonometric
 *   function.
 * For result cell s = X * gy + Y with onset t0 = (int)delay[s], per band:
 *   y(t)   the band metrics' filtered sample: the same two sections, the same backward walk from T - 1 (state +0.0f) down to t0;
 *          the walk STOPS at t0
 *   e(t) = y(t) * y(t)
 *   in DECREASING t from +0.0f, every product and sum rounded on its own (no FMA), denormals kept:
 *      E += e;     re[i] += e * row_t[2 i];     im[i] += e * row_t[2 i + 1]
 *   then per modulation frequency (division and sqrtf correctly rounded; log10f is glibc's):
 *      a = re[i] / E;   b = im[i] / E;   m[i] = sqrtf((a * a) + (b * b))
 *        (the ratios are taken first, so that re^2 + im^2 cannot underflow in a faint cell)
 *      snr[i] = +15.0f where m[i] >= 1.0f, else v = 10.0f * log10f(m[i] / (1.0f - m[i])) clamped:
 *               v < -15.0f ? -15.0f : (v > 15.0f ? 15.0f : v)                       (a NaN stays a NaN)
 *      ti[i]  = (snr[i] + 15.0f) / 30.0f
 *   mti = (the sequential sum of ti[0 .. 13] from +0.0f) / 14.0f
 *   A band with E == 0 gives 15 quiet NaNs.  Nothing else is special-cased.
 * Record per band (15 floats): m[0 .. 13], mti.  A cell WITHOUT an onset in that run holds 15 n quiet NaNs; nothing is carried
 * over from earlier runs.
 * What this is NOT: a full speech transmission index (STI) needs the seven octave bands from 125 Hz to 8 kHz.  A grid carries only
 * the bands below its gridResolution, and PvAmdSetBands refuses a band at or above fs / 2 -- so what most solvers yield is the
 * per-band MTI and, through PvAmdCombineMti, a PARTIAL index over the two or three bands they have.  No noise, masking or
 * level-dependent correction of IEC 60268-16 is applied, and the library holds no table of band weights.
 * Device storage: the table (28 x 4 bytes per step) and 15 n x 4 bytes per cell of the history window, allocated by the first
 * PvAmdComputeModulation (again when n changes), freed by PvAmdSetBands(n = 0) and with the solver.  Lifetime and refusals are the
 * band metrics', word for word, with the prefix "modulation: "; computing or reading with no bands set is refused ("no bands
 * set"); PvAmdSetBands and PvAmdSetModulationFrequencies invalidate the records.  The other analysis kinds and this one do not
 * invalidate each other. */
#define PVA_MODULATION_FREQS 14
typedef struct PvAmdModulation {
    float m[PVA_MODULATION_FREQS], mti;
} PvAmdModulation;
/* Set the 14 modulation frequencies (copied); hz14 = NULL restores the default series.  Waits for a run in flight; invalidates the
 * records.  -1 and nothing changed: a frequency that is not finite, negative or above fs / 2 */
PVA_EXPORT int PvAmdSetModulationFrequencies(PvAmdSolver* s, const float* hz14);
/* the 14 modulation frequencies in use */
PVA_EXPORT int PvAmdGetModulationFrequencies(PvAmdSolver* s, float* hz14);
/* Compute the modulation records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeBandMetrics).  Synchronous on the solver's own stream.  *ms (optional): device time of the passes. */
PVA_EXPORT int PvAmdComputeModulation(PvAmdSolver* s, float* ms);
/* gx*gy*n*15 floats: cell s = X*gy + Y, then band, then the 15 floats */
PVA_EXPORT int PvAmdCopyModulation(PvAmdSolver* s, float* out15n);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc x n records, row-major */
PVA_EXPORT int PvAmdCopyModulationBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out15n);
/* the n records at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives NaNs and 0 */
PVA_EXPORT int PvAmdGetModulation(PvAmdSolver* s, float ex, float ey, float ez, PvAmdModulation* out15n);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T, n (1 .. PVA_BANDS_MAX) coefficient
 * sets of 10 floats and the 14 modulation frequencies (NULL: the default); the restatement the tests hold the kernel to */
PVA_EXPORT int PvAmdHostModulation(const float* p, int T, int fs, int onset, const float* coefs10n, int n, const float* hz14,
                                   PvAmdModulation* out15n);
/* CPU only: the table above, T rows of 28 floats (hz14 = NULL: the default) */
PVA_EXPORT int PvAmdHostModulationTable(int T, int fs, const float* hz14, float* out28T);
/* CPU only: combine the MTI of n (1 .. PVA_BANDS_MAX) adjacent bands into one index, in float32, sequentially from +0.0f:
 *   *out = clamp((sum over k < n of (alpha[k] * mti[k])) - (sum over k < n - 1 of (beta[k] * sqrtf(mti[k] * mti[k + 1]))))
 *   clamp(v) = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)                              (a NaN stays a NaN)
 * alpha: n weights, beta: n - 1 redundancy weights (may be NULL for n = 1) -- the caller supplies the IEC 60268-16 values for the
 * bands it has.  Over fewer than the seven octaves 125 Hz .. 8 kHz the result is a partial index, not an STI. */
PVA_EXPORT int PvAmdCombineMti(const float* mti, const float* alpha, const float* beta, int n, float* out);
/* ---- Spectrum: the transfer function from the listener to every reached cell, at chosen frequencies ----
 * How loud the room is at ONE frequency at one position (room modes and their nodal lines, comb filtering behind an obstacle,
 * per-band gains): PvAmdComputeSpectrum reduces the history of the LAST COMPLETED run to three floats per bin and cell in one
 * pass on the device per block of bins (pv_spectrum.hip).  Definition (T = the run's steps, PvAmdInfo::T):
 *   bins     n frequencies hz[j], 1 <= n <= PVA_SPECTRUM_MAX_BINS, each finite and 0 <= hz[j] <= fs / 2; neither sorted nor
 *            distinct;
 *   tables   c[t * n + j] = (float)cos(ph), s[t * n + j] = (float)sin(ph), t = 0 .. T - 1, with
 *            ph = (2.0 * M_PI * (double)hz[j] * (double)t) / (double)fs in double and the host libm's cos / sin: ABSOLUTE run
 *            time, phase zero is the start of the run, not the cell's onset.  The device evaluates no trigonometric function;
 *   sums     for result cell s = X * gy + Y with onset t0 = (int)delay[s] (the run's own onset map) and p(t) exactly what
 *            PvAmdCopyHistoryPlane(t) returns at array cell (X, Y):
 *              re_j = sum_{t = t0}^{T - 1} (p(t) * c[t * n + j])      im_j = sum_{t = t0}^{T - 1} (p(t) * s[t * n + j])
 *            so X(f_j) = re_j - i im_j; samples before the onset do not enter;
 *   source   the same sums over the run's pulse table (PvAmdCopyPulse, its first T floats) with onset 0: sre_j, sim_j and
 *            spow_j = (sre * sre) + (sim * sim), computed on the host when the bins are set;
 *   record   re, im, level = 10.0f * log10f(((re * re) + (im * im)) / spow_j)  (dB re the source).
 * All arithmetic is float32; every product and every sum is rounded on its own; every sum is sequential in increasing t from
 * +0.0f; denormals are kept; division is correctly rounded; log10f is glibc's.  Nothing is special-cased: spow_j = 0 gives
 * +-inf or NaN as IEEE says.
 * A level is meaningful only inside the pulse's band (up to about the grid resolution in Hz): above it spow_j is the square of
 * rounding noise.  Cells inside an edge layer get records like any other cell, as unphysical there as their other outputs.
 * A cell WITHOUT an onset in that run holds 3 n quiet NaNs; nothing is carried over from earlier runs.
 * Device storage: the tables (2 x 4 bytes per step and bin, padded to the register block) from PvAmdSetSpectrumBins on, and
 * 3 n x 4 bytes per cell of the history window from the first PvAmdComputeSpectrum on (allocated again when n changes).
 * Lifetime: the records stay valid until the next run, geometry, boundary or layer change on that solver -- exactly as the room
 * metrics' -- or a change of the bins; the read-backs then return -1 until computed again.  Room metrics and spectrum do not
 * invalidate each other.  Options (PVA_OPT_NUM_STEPS among them) are fixed before the first call, so T cannot change under
 * the tables.
 * Refused (-1, nothing changed, PvAmdLastError says why, "spectrum: ..."): no bins set, no completed run, a last run that ended
 * in error, sparse-emitter solvers (no history), PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks.
 * On a sparse-emitter solver PvAmdComputeSpectrum stays refused (there is no history), but the records of the LABELLED cells can
 * be accumulated inside the run: PvAmdSetZoneMaps(PVA_ZMAP_SPECTRUM) below; the three read-backs then serve that map, and the
 * bins cannot be cleared while it is selected (changing them is allowed: the map of the run before is then refused). */
#define PVA_SPECTRUM_MAX_BINS 32
/* Set the bins (copied).  n = 0 clears them and frees the device storage; waits for a run in flight.  Refused with -1 and nothing
 * changed: hz = NULL with n > 0, n outside 0 .. PVA_SPECTRUM_MAX_BINS, a frequency that is not finite, negative or above fs / 2 */
PVA_EXPORT int PvAmdSetSpectrumBins(PvAmdSolver* s, const float* hz, int n);
/* the bins as set: up to cap of them into hz (may be NULL); returns n */
PVA_EXPORT int PvAmdGetSpectrumBins(PvAmdSolver* s, float* hz, int cap);
/* sre, sim, spow of every bin: 3 n floats */
PVA_EXPORT int PvAmdGetSpectrumSource(PvAmdSolver* s, float* out3n);
/* Compute the records of the LAST COMPLETED run of s (waits for a run in flight; works after every form of run, as
 * PvAmdComputeRoomMetrics).  Synchronous on the solver's own stream.  *ms (optional): device time of the passes. */
PVA_EXPORT int PvAmdComputeSpectrum(PvAmdSolver* s, float* ms);
/* gx*gy*n*3 floats: cell-major (s = X*gy + Y), then bin, then {re, im, level} */
PVA_EXPORT int PvAmdCopySpectrum(PvAmdSolver* s, float* out);
/* the same for the block of result cells [r0, r0 + nr) x [c0, c0 + nc): nr x nc x n x 3 floats, row-major */
PVA_EXPORT int PvAmdCopySpectrumBlock(PvAmdSolver* s, int r0, int c0, int nr, int nc, float* out);
/* the n records at an emitter position, mapped to a cell exactly as PvAmdGetOutput does; a position off the map gives 3 n NaNs
 * and 0 */
PVA_EXPORT int PvAmdGetSpectrum(PvAmdSolver* s, float ex, float ey, float ez, float* out3n);
/* CPU only: the tables of the definition above, T * n floats each */
PVA_EXPORT int PvAmdHostSpectrumTables(int T, int fs, const float* hz, int n, float* cosTn, float* sinTn);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T and the pulse table pulseT[T]; the
 * restatement the tests hold the kernel to.  The bins are checked by the rule of PvAmdSetSpectrumBins */
PVA_EXPORT int PvAmdHostSpectrum(const float* p, int T, int fs, int onset, const float* hz, int n, const float* pulseT,
                                 float* out3n);

/* ---- Waterfall: the cumulative spectral decay of chosen receivers, on a dense frequency grid ----
 * Below about 1 kHz a room is its modes: which frequencies ring, and for how long.  The waterfall is the picture of that: a
 * receiver's frequency response at up to 512 bins, and how that response decays slice by slice after the direct sound.  It is
 * the transpose of the Spectrum above -- few cells, many bins -- in one pass on the device (pv_waterfall.hip) over what the LAST
 * COMPLETED run left there: the pressure history, or in sparse-emitter mode the emitters' traces.  Definition (T = the run's
 * steps, PvAmdInfo::T):
 *   bins     n frequencies hz[j], 1 <= n <= PVA_WATERFALL_MAX_BINS, each finite and 0 <= hz[j] <= fs / 2; neither sorted nor
 *            distinct (the Spectrum's rule with the larger cap);
 *   slices   m of them, 1 <= m <= PVA_WATERFALL_MAX_SLICES; slice k starts k * ns steps after the receiver's onset, with
 *            ns = (int)(sliceSeconds * (float)fs) in float32 (the echogram's expression); refused unless sliceSeconds is finite
 *            and 1 <= ns <= (1 << 20);
 *   tables   exactly those of the Spectrum: c[t * n + j] = (float)cos(ph), s[t * n + j] = (float)sin(ph), t = 0 .. T - 1, with
 *            ph = (2.0 * M_PI * (double)hz[j] * (double)t) / (double)fs in double and the host libm's cos / sin: ABSOLUTE run
 *            time.  The device evaluates no trigonometric function;
 *   source   spow_j as the Spectrum defines it: the bits of PvAmdGetSpectrumSource for the same frequency;
 *   record   of ONE receiver = result cell s = X * gy + Y with onset t0 = (int)delay[s] (the run's own onset map) and p(t) exactly
 *            what PvAmdCopyHistoryPlane(t) returns at array cell (X, Y) -- in sparse-emitter mode what PvAmdCopyEmitterTrace
 *            returns --, F = 2 + 2 n + m n floats:
 *              re_j = +0.0f, im_j = +0.0f
 *              for t = T - 1 down to t0:                      (DECREASING t: one backward walk gives every slice)
 *                  re_j = re_j + (p(t) * c[t * n + j])
 *                  im_j = im_j + (p(t) * s[t * n + j])
 *                  if t == t0 + k * ns for a k in 0 .. m - 1:  R[k][j] = re_j,  I[k][j] = im_j
 *              slices that start at or past T keep R = I = +0.0f
 *            so X_k(f_j) = R[k][j] - i I[k][j] is the transform of the response with its first k * ns steps after the onset
 *            removed: the cumulative spectral decay with a rectangular window.  The floats, in order:
 *              [0]  (float)t0
 *              [1]  (float) the count of slices with t0 + k * ns < T
 *              R[0][0 .. n), then I[0][0 .. n): slice 0 is the receiver's complex frequency response (callers need the phase)
 *              level[k][j] = 10.0f * log10f(((R * R) + (I * I)) / spow_j) of R[k][j], I[k][j], k = 0 .. m - 1, slice-major
 *              (dB re the source).
 * All arithmetic is float32; every product and every sum is rounded on its own; nothing is fused; denormals are kept; log10f is
 * glibc's.  Nothing is special-cased: an empty slice gives 10 log10f(0 / spow) = -inf, spow_j = 0 gives what IEEE gives.
 * Slice 0 is NOT bit-equal to PvAmdComputeSpectrum's re, im at the same cell and bin: the mathematical sum is the same, the
 * order of summation is the opposite (each lies within the sequential-summation bound of the exact sum).
 * A receiver off the map, in a wall, outside the run's history window or without an onset in that run holds F quiet NaNs
 * (0x7fc00000).  A record's bits depend on its own cell alone: not on the other receivers of the call, their order, or the
 * launch shape.  Reading ridge decay times off the levels is left to the caller, as the echogram leaves its levels; a window
 * taper at T and rise-time windows are not provided.
 * Receivers.  On a solver that keeps its history: 1 <= nPos <= PVA_WATERFALL_MAX_RECEIVERS positions, mapped to cells exactly as
 * PvAmdSetOutputQueries maps its positions; duplicates are allowed.  On a sparse-emitter solver xyz must be NULL and nPos = 0:
 * the receivers are the emitters PvAmdSetEmitters kept, in that order (at most 256; more is refused), the samples come from the
 * emitter traces, and no emitter-record kind needs to be selected.
 * Device storage: the tables, 2 x 4 x T x n bytes (n rounded up to a multiple of 64) from PvAmdSetWaterfall on -- 104 MB at
 * T = 25 432 and 512 bins --, and the records, nPos x F x 4 bytes from the first PvAmdComputeWaterfall on (at most 34.6 MB;
 * allocated again when nPos or F changes).
 * Lifetime: that of the Spectrum's records -- a run, a geometry, boundary or layer change, a change of the setting and, in
 * sparse-emitter mode, a change of the emitters invalidate the records; PvAmdCopyWaterfall then returns -1.  The waterfall and
 * the nine map kinds do not invalidate each other.  With no setting nothing is allocated or launched.
 * Refused (-1, nothing changed, PvAmdLastError says why, "waterfall: ..."): no setting, no completed run, a last run that ended
 * in error, PVA_OPT_SKIP_ANALYSIS (no onset map), slab groups and slab ranks, xyz = NULL with nPos > 0, nPos out of range,
 * positions given on a sparse-emitter solver or no emitter registered there, nPos of the copy differing from the computed count. */
#define PVA_WATERFALL_MAX_BINS      512
#define PVA_WATERFALL_MAX_SLICES    64
#define PVA_WATERFALL_MAX_RECEIVERS 256
/* Set bins (copied) and slices, and upload the tables.  nBins = 0 clears the setting and frees tables and records; waits for a
 * run in flight.  Refused with -1 and nothing changed: the bin rule, the slice rule and the caps above.  The new tables are built
 * (host libm in double; host memory: the device table's image, 105 MB at T = 25 432 and 512 bins, and 13 MB beside it) and
 * uploaded BESIDE the old ones, which are freed only once that has worked: a failed allocation or upload also returns -1 with
 * the setting, the tables and the records of before in place.  A successful call frees the records of the setting before */
PVA_EXPORT int PvAmdSetWaterfall(PvAmdSolver* s, const float* hz, int nBins, float sliceSeconds, int nSlices);
/* the setting: up to cap bins into hz (may be NULL), the slice length as given and in steps, the slices (each may be NULL;
 * written only while a setting exists); returns nBins */
PVA_EXPORT int PvAmdGetWaterfall(PvAmdSolver* s, float* hz, int cap, float* sliceSeconds, int* sliceSteps, int* nSlices);
/* F under the current setting, -1 without one */
PVA_EXPORT int PvAmdWaterfallFloats(PvAmdSolver* s);
/* Compute the records of the LAST COMPLETED run of s (waits for a run in flight).  Synchronous on the solver's own stream.
 * *ms (optional): device time of the pass. */
PVA_EXPORT int PvAmdComputeWaterfall(PvAmdSolver* s, const float* xyz, int nPos, float* ms);
/* nPos x F floats, receiver-major; nPos = the computed count (the kept emitters' in sparse-emitter mode) */
PVA_EXPORT int PvAmdCopyWaterfall(PvAmdSolver* s, float* out, int nPos);
/* CPU only: the definition above applied to one impulse response p[T] with 0 <= onset < T and the pulse table pulseT[T]; the
 * restatement the tests hold the kernel to.  The setting is checked by the rule of PvAmdSetWaterfall */
PVA_EXPORT int PvAmdHostWaterfall(const float* p, int T, int fs, int onset, const float* hz, int n, float sliceSeconds, int nSlices,
                                  const float* pulseT, float* outF);

/* ---- Source arrays: the combined response of weighted, delayed emitters ----
 * Every other record here is for one source and one receiver.  A delayed fill system, a line of ceiling speakers or a steered
 * sub array heard at a seat -- or, by reciprocity, a delay-and-sum microphone array listening to one source -- is a SUM: the
 * stencil is linear and the recorded pressure at cell c is the response between the listener and c, so the response of an array
 * at the listener is  sum_k g_k h_k(t - tau_k)  over its members' recorded responses.  PvAmdComputeArrays forms that sum on the
 * device (pv_arrays.hip) from what the LAST COMPLETED run left there -- the pressure history, or in sparse-emitter mode the
 * emitters' traces -- and computes the selected records of every sum.  Definition (T = the run's steps, PvAmdInfo::T):
 *   setting   nArrays in 1 .. PVA_ARRAYS_MAX; array a has count[a] members, 1 .. PVA_ARRAY_MEMBERS_MAX; a member is five floats
 *             {x, y, z, gain, delaySeconds}, the members of array 0 first; a negative gain is polarity; interp is
 *             PVA_ARRAY_NEAREST or PVA_ARRAY_LAGRANGE3;
 *   cell      a member's position maps to a result cell exactly as PvAmdSetOutputQueries maps its positions; a member off the map
 *             is refused at set time; a member in a wall, or in a cell the run's history window does not hold, is legal and
 *             contributes zeros.  p_m(t) is what PvAmdCopyHistoryPlane(t) returns at the member's cell: +0 where nothing was
 *             stored, and +0 for t < 0.  Samples below the member's own onset are included;
 *   taps      on the host, in double: d = (double)delaySeconds * (double)fs; refused unless gain and delaySeconds are finite,
 *             delaySeconds >= 0 and d < T; n = floor(d), mu = d - n.
 *               NEAREST               one tap {delay = (int)floor(d + 0.5), w = gain}; a delay that rounds to T is refused
 *               LAGRANGE3, mu == 0    one tap {n, gain}
 *               LAGRANGE3, mu != 0    n >= 1 is required; four taps at delays n - 1, n, n + 1, n + 2, with D = mu + 1.0 and
 *                                       L0 = -((D - 1) (D - 2) (D - 3)) / 6     L1 = (D (D - 2) (D - 3)) / 2
 *                                       L2 = -(D (D - 1) (D - 3)) / 2           L3 = (D (D - 1) (D - 2)) / 6
 *                                     each product evaluated left to right in double, w_j = (float)((double)gain * L_j); taps
 *                                     whose delay is >= T are kept and contribute nothing;
 *   response  y_a(t), t = 0 .. T - 1, starts from +0.0f; over the array's members in the given order and each member's taps in
 *             increasing delay:  y = y + (w * p_m(t - delay)).  All arithmetic is float32, every product and every sum rounded on
 *             its own, nothing fused, denormals kept;
 *   onset     the reference's rule (Analyzer.cpp:146-165) applied to y_a: the first t with fabsf(y_a(t)) > 0.00000316f as a
 *             float, else FLT_MAX; NaN compares false;
 *   records   for the selected kinds among PVA_QREC_ROOM_METRICS, PVA_QREC_DECAY_TIMES, PVA_QREC_ECHO_CRITERION,
 *             PVA_QSPEC_BAND_METRICS, PVA_QSPEC_MODULATION and PVA_QSPEC_SPECTRUM the record of array a is by definition
 *             PvAmdHost<Kind>(y_a, T, fs, onset_a, ...) under the solver's current bands, modulation frequencies, bins and pulse;
 *             an array without an onset gives quiet NaNs.  The three velocity kinds are refused: a mix has no cell and no face
 *             coefficients.
 * A response's bits depend on its own members and taps alone: not on the other arrays, their order or its index.
 * Sparse-emitter mode: every member's cell must be the cell of a kept registered emitter (PvAmdSetEmitters); this is checked by
 * PvAmdComputeArrays, which names the array and the member; the samples are the emitter traces, and no emitter-record kind needs
 * to be selected.
 * Device storage, only while arrays are set: the tables and the mix planes, T x P x 4 bytes with P = nArrays rounded up to 64
 * (26 MB at T = 25 432 and 256 arrays); the record block from the first compute with a kind selected.
 * Lifetime: a run, a geometry, boundary or layer change, a successful PvAmdSetArrays or a changed PvAmdSetArrayRecords, a
 * PvAmdSetBands / PvAmdSetModulationFrequencies / PvAmdSetSpectrumBins while a dependent kind is selected and, in sparse-emitter
 * mode, a change of the emitters invalidate what PvAmdComputeArrays left; the read-backs then return -1.  With no arrays set
 * nothing is allocated or launched, and a run enqueues exactly what it does without this section.
 * Refused (-1, nothing changed, PvAmdLastError says why, "arrays: ..."): slab groups and slab ranks, PVA_OPT_SKIP_ANALYSIS, no
 * completed run or a last run in error, counts out of range, NULL tables, a bad member or interp, an unknown or velocity kind, a
 * band or spectrum kind without bands or bins, the sampling-rate floor of the echo criterion, a read-back whose count, kind or
 * stamp does not match. */
#define PVA_ARRAYS_MAX        256
#define PVA_ARRAY_MEMBERS_MAX 64
#define PVA_ARRAY_NEAREST     0
#define PVA_ARRAY_LAGRANGE3   1
/* Set the arrays (copied): count[nArrays], members5 = five floats per member, array 0's members first.  nArrays = 0 clears the
 * setting and frees everything.  Waits for a run in flight.  A refused or failed call leaves the setting of before */
PVA_EXPORT int PvAmdSetArrays(PvAmdSolver* s, const int* count, int nArrays, const float* members5, int interp);
/* the setting: up to cap counts (may be NULL) and interp (may be NULL; written only while a setting exists); returns nArrays */
PVA_EXPORT int PvAmdGetArrays(PvAmdSolver* s, int* count, int cap, int* interp);
/* the expanded taps of one array in the order the response takes them: up to cap of {member index inside the array, delay in
 * steps, weight} (each may be NULL); returns the tap count, -1: no such array */
PVA_EXPORT int PvAmdGetArrayTaps(PvAmdSolver* s, int array, int* memberIndex, int* delaySteps, float* weight, int cap);
/* the record kinds PvAmdComputeArrays computes for every array: PVA_QREC_* bits (room metrics, decay times, echo criterion) and
 * PVA_QSPEC_* bits; 0, 0 selects none.  Independent of the output queries' and the emitters' selections */
PVA_EXPORT int PvAmdSetArrayRecords(PvAmdSolver* s, unsigned timeKinds, unsigned spectralKinds);
PVA_EXPORT int PvAmdGetArrayRecordKinds(PvAmdSolver* s, unsigned* timeKinds, unsigned* spectralKinds);
/* floats per array of ONE kind under the current settings; family 0: PVA_QREC_*, family 1: PVA_QSPEC_* */
PVA_EXPORT int PvAmdArrayRecordFloats(PvAmdSolver* s, int family, unsigned kind);
/* Mix, onsets and the selected records of the LAST COMPLETED run of s (waits for a run in flight).  Synchronous on the solver's
 * own stream.  *ms (optional): device time of the call's kernels */
PVA_EXPORT int PvAmdComputeArrays(PvAmdSolver* s, float* ms);
/* y_a(t), T floats */
PVA_EXPORT int PvAmdCopyArrayResponse(PvAmdSolver* s, int array, float* outT);
/* the onsets of all arrays (FLT_MAX: none); nArrays = the arrays set */
PVA_EXPORT int PvAmdGetArrayOnsets(PvAmdSolver* s, float* out, int nArrays);
/* nArrays x floats of one selected kind, array-major: the layout of PvAmdGetEmitterRecords */
PVA_EXPORT int PvAmdGetArrayRecords(PvAmdSolver* s, int family, unsigned kind, float* out, int nArrays);
/* CPU only: the taps of one member by the rule above; returns the tap count (1 or 4) with delay4 / w4 written, or -1 */
PVA_EXPORT int PvAmdHostArrayTaps(int fs, int T, float gain, float delaySeconds, int interp, int* delay4, float* w4);
/* CPU only: the response of one array from its members' responses pMT[M][T] and its taps in order (tapMember in 0 .. M - 1; a
 * sample at t - delay outside 0 .. T - 1 is +0): outT[T], *onset (optional) by the rule above */
PVA_EXPORT int PvAmdHostArrayResponse(const float* pMT, int M, int T, const int* tapMember, const int* tapDelay,
                                      const float* tapWeight, int nTaps, float* outT, float* onset);

/* ---- Auralisation: audio-rate responses and their convolution with dry signals ----
 * Every record above is a number ABOUT a response.  The response itself leaves the library only raw, at the grid's own rate
 * fs = PvAmdInfo::fs (1443 Hz at the 70 x 70 preset, 84 351 Hz at 4096 x 4096): no audio tool takes that rate.  This section
 * resamples recorded responses to an audio rate with a Kaiser-windowed sinc and convolves them with dry signals, both on the device
 * (pv_aural.hip), so a run can be listened to.  It is the PHYSICAL path the recorded history makes possible, not the reference's
 * parametric PlaneverbDSP renderer.  Definition (T = the run's steps, PvAmdInfo::T; all device arithmetic float32, every product and
 * every sum rounded on its own, nothing fused, denormals kept; the device evaluates no transcendental function):
 *   setting   rate, an int in 1000 .. 384000; zeroCrossings Z, an int in 2 .. 64; beta, the Kaiser window's parameter, finite in
 *             0 .. 20;
 *   tables    built at set time on the host, in double:
 *               c = rate < fs ? (double)rate / (double)fs : 1.0        half = (double)Z / c        K = 2 * (int)floor(half) + 1
 *               L = (int)floor(((double)(T - 1) * (double)rate) / (double)fs) + 1   -- the response length in output samples: the
 *                   last n whose source time is <= T - 1
 *               for n = 0 .. L - 1:  u = ((double)n * (double)fs) / (double)rate,  first[n] = (int)ceil(u - half)
 *               for slot j = 0 .. K - 1:  t = first[n] + j,  d = u - (double)t;
 *                   fabs(d) > half:  w[n][j] = +0.0f
 *                   else  a = c * d,  sinc = (a == 0.0) ? 1.0 : sin(M_PI * a) / (M_PI * a),  q = d / half,  q = 1.0 - q * q,
 *                         if (q < 0.0) q = 0.0,  w[n][j] = (float)((c * sinc) * (I0(beta * sqrt(q)) / I0(beta)))
 *               I0(x):  s = 1.0, term = 1.0, h = 0.5 * x;  for k = 1 .. 60:  term = term * ((h / k) * (h / k)),  s = s + term
 *               sin and sqrt are the host libm's;
 *   receivers PVA_AURAL_RECEIVERS on a history-keeping solver: 1 .. PVA_AURAL_MAX_RECEIVERS positions, mapped to cells exactly as
 *             PvAmdSetOutputQueries maps them; duplicates are allowed; a position off the map is refused, and the error names its
 *             index.  p_r(t) is what PvAmdCopyHistoryPlane(t) returns at the cell: +0 in a wall or outside the history window (the
 *             rule of an array member).  On a sparse-emitter solver: xyz = NULL, nPos = 0; the receivers are the kept registered
 *             emitters in their order, at most 256, and the samples their traces; no emitter-record kind needs to be selected.
 *             PVA_AURAL_ARRAYS: xyz = NULL, nPos = 0; the receivers are the arrays, p_r(t) = y_a(t) of the last
 *             PvAmdComputeArrays; refused while that result is invalid;
 *   response  h_r[n], n = 0 .. L - 1, starts from +0.0f; for j = 0 .. K - 1 ascending:
 *                 h = h + (w[n][j] * p_r(first[n] + j)),   p_r = +0.0f outside 0 .. T - 1.
 *             Time is absolute: n = 0 is the emission, so the propagation delays between receivers are kept.  No onset and no NaN
 *             rule applies: a receiver nothing reached gives the samples it has.  A response's bits depend on its own receiver
 *             alone;
 *   signals   signals[nSignals][N], mono float32 at `rate`, 1 <= nSignals <= PVA_AURAL_MAX_SIGNALS, 1 <= N <=
 *             PVA_AURAL_MAX_SAMPLES; route[R] is a signal index per receiver, or -1 for a receiver that is not rendered; gain[R]
 *             finite, a negative gain is polarity; M = N + L - 1;
 *   output    of a routed receiver: o_r[m], m = 0 .. M - 1, starts from +0.0f; for k = max(0, m - N + 1) .. min(L - 1, m)
 *             ascending:  o = o + (h_r[k] * x[m - k]).  Terms outside that range are not formed.  Unrouted receivers hold +0.0f;
 *   mix       mix[m] starts from +0.0f; over the routed receivers in increasing r:  mix = mix + (gain[r] * o_r[m]).
 * NaN, inf and denormal samples propagate as IEEE says.
 * Device storage, only while a setting exists: the tables, L * K * 4 + L * 4 bytes, from PvAmdSetAuralisation on; the gathered
 * samples, R * T * 4 bytes, and the responses, R * L * 4 bytes, from the first PvAmdComputeAuralResponses on; the signals and the
 * outputs, R * M * 4 + M * 4 bytes, from the first PvAmdAuralise on.
 * Lifetime: a run, a geometry, boundary or layer change, a changed setting, in sparse-emitter mode a change of the emitters and,
 * for the array source, whatever invalidates the array responses invalidate the responses and the outputs; a new
 * PvAmdComputeAuralResponses invalidates the outputs; the read-backs then return -1.  With no setting nothing is allocated or
 * launched, and a run enqueues exactly what it does without this section.
 * Refused (-1, nothing changed, PvAmdLastError says why, "aural: ..."): the ranges above, K > PVA_AURAL_MAX_TAPS,
 * L * K > 2^24, R * M > 2^26, slab groups and slab ranks, no completed run or a last run in error, bad indices, NULL tables, no
 * valid responses.  PVA_OPT_SKIP_ANALYSIS is no reason to refuse: no onset map is needed. */
#define PVA_AURAL_MAX_TAPS      1024
#define PVA_AURAL_MAX_RECEIVERS 256
#define PVA_AURAL_MAX_SIGNALS   64
#define PVA_AURAL_MAX_SAMPLES   (1 << 20)
#define PVA_AURAL_RECEIVERS     0
#define PVA_AURAL_ARRAYS        1
#define PVA_AURAL_TILED         0
#define PVA_AURAL_PLAIN         1
/* Set the resampler (the tables are built and uploaded beside the old ones: a refused or failed call leaves the setting of
 * before).  rate = 0 clears the setting and frees everything.  Waits for a run in flight */
PVA_EXPORT int PvAmdSetAuralisation(PvAmdSolver* s, int rate, int zeroCrossings, float beta);
/* the setting with the response length L and the taps per sample K (each may be NULL); -1 without a setting */
PVA_EXPORT int PvAmdGetAuralisation(PvAmdSolver* s, int* rate, int* zeroCrossings, float* beta, int* L, int* K);
/* the tables: first[n] and w[n][0 .. K) of the first min(capN, L) samples (each may be NULL); returns L, -1 without a setting */
PVA_EXPORT int PvAmdGetAuralTaps(PvAmdSolver* s, int* first, float* w, int capN);
/* The responses of the LAST COMPLETED run of s (waits for a run in flight).  Synchronous on the solver's own stream.  *ms
 * (optional): device time of the call's kernels */
PVA_EXPORT int PvAmdComputeAuralResponses(PvAmdSolver* s, int source, const float* xyz, int nPos, float* ms);
/* h_r, L floats */
PVA_EXPORT int PvAmdCopyAuralResponse(PvAmdSolver* s, int r, float* outL);
/* Convolve and mix: route[R] and gain[R] with R the receivers of the responses.  Synchronous; *ms (optional): device time of the
 * convolution and the mix */
PVA_EXPORT int PvAmdAuralise(PvAmdSolver* s, const float* signals, int nSignals, int N, const int* route, const float* gain, float* ms);
/* o_r, M floats (zeros for an unrouted receiver) */
PVA_EXPORT int PvAmdCopyAuralOutput(PvAmdSolver* s, int r, float* outM);
/* mix, M floats */
PVA_EXPORT int PvAmdCopyAuralMix(PvAmdSolver* s, float* outM);
/* the tiling of the convolution kernel: a block owns outputsPerBlock consecutive outputs and stages tapsPerChunk taps at a time */
PVA_EXPORT void PvAmdAuralShape(int* outputsPerBlock, int* tapsPerChunk);
/* which convolution kernel PvAmdAuralise launches: PVA_AURAL_TILED (the default, the one above) or PVA_AURAL_PLAIN (one lane per
 * output, taps and samples from global memory: what the tiled form is measured against).  The same bits either way */
PVA_EXPORT int PvAmdSetAuralForm(PvAmdSolver* s, int form);
/* CPU only: the shape and the tables of a setting by the rule above: *L, *K (optional), and first[L], w[L * K] where both are given
 * (capN >= L; both NULL: the shape alone); -1 where PvAmdSetAuralisation would refuse */
PVA_EXPORT int PvAmdHostAuralTaps(int fs, int T, int rate, int zeroCrossings, float beta, int* first, float* w, int capN, int* L, int* K);
/* CPU only: one response from samples p[T] and tables first[L], w[L * K]: outL[L] */
PVA_EXPORT int PvAmdHostAuralResample(const float* p, int T, const int* first, const float* w, int L, int K, float* outL);
/* CPU only: one output from a response h[L] and a signal x[N]: outM[N + L - 1] */
PVA_EXPORT int PvAmdHostAuralConvolve(const float* h, int L, const float* x, int N, float* outM);

/* ---- Zone statistics: spatial statistics of a computed map over receiver areas ----
 * ISO 3382-1 reports its quantities as averages over receiver areas, with their spread.  A ZONE is a label per result cell;
 * PvAmdComputeZoneStats reduces one computed map of the nine kinds above to one record per zone and plane ON THE DEVICE
 * (pv_zones.hip) and only the records cross to the host -- no copy of the map is made.  Definition, for zone z and plane k:
 *   members  the result cells s = X * gy + Y with labels[s] == z (label 0: no zone; labels 1 .. nZones, nZones <= PVA_ZONES_MAX;
 *            zones do not overlap);
 *   x(s)     exactly what PvAmdCopy<Kind> gives at cell s, float k of its record: cells without an onset, and cells outside
 *            the run's history window, are NaN there and count as NaN here;
 *   counts   every member is in exactly one class: finite (x - x == 0), NaN, +inf, -inf; the four counts add up to the zone's
 *            size;
 *   min, max over the FINITE members only; -0.0 and +0.0 compare equal; a tie goes to the smallest cell index s, and that
 *            cell's bits are reported; argmin / argmax are cell indices s;
 *   sum      double, in ONE order that depends on result coordinates alone (never on tiles, the history window or the launch
 *            shape).  v(X, Y) = (double)x for a finite member, +0.0 for every other cell and for columns Y >= gy;
 *              block  row X, block b: v(X, 64 b .. 64 b + 63) by a butterfly -- for st = 1, 2, 4, 8, 16, 32: v[i] = v[i] +
 *                     v[i + st] for every i that is a multiple of 2 st; the block value is v[0];
 *              row    the block values added sequentially in increasing b, from +0.0;
 *              zone   the row sums added sequentially in increasing X over all rows 0 .. gx - 1, from +0.0;
 *   mean     sum / (double)n_finite;
 *   m2       the same three-level rule over d * d, d = (double)x - mean; the subtract, the product and every add are rounded
 *            on their own (no fused multiply-add);
 *   std      sqrt(m2 / (double)n_finite): the population form; divide and sqrt correctly rounded (std is computed on the host
 *            from the device's m2);
 *   empty    n_finite == 0: sum = +0.0; mean, m2, std, min, max quiet NaN; argmin = argmax = -1.
 * PvAmdHostZoneStats applies the same rule on the CPU, bit for bit.
 * Device storage: the labels (one byte per result cell) from PvAmdSetZones on; scratch of 48 bytes per zone, result row and
 * plane in flight from the first PvAmdComputeZoneStats on -- the planes of a map are dealt in chunks that keep it within
 * 32 MiB (one plane's nZones x gx x 48 bytes where that is more) -- plus the records.
 * Out of scope: the eight-output result map (its far cells are kept lazily and carry values over between runs), histograms
 * and percentiles, overlapping zones, in-run or live-module zone records, slab groups and slab ranks.  Sparse-emitter solvers
 * take the labels (PvAmdSetZones, for the in-run zone curves and zone maps below) but keep no history: PvAmdComputeZoneStats is
 * refused there, except for PVA_MAP_ROOM_METRICS and PVA_MAP_SPECTRUM while PvAmdSetZoneMaps has the kind selected -- the map is
 * then the last run's own, and the records are those of a solver that keeps its history, byte for byte. */
#define PVA_MAP_ROOM_METRICS     0
#define PVA_MAP_DECAY_TIMES      1
#define PVA_MAP_LATERAL_FRACTION 2
#define PVA_MAP_ECHO_CRITERION   3
#define PVA_MAP_ECHOGRAM         4
#define PVA_MAP_LOBES            5
#define PVA_MAP_BAND_METRICS     6
#define PVA_MAP_MODULATION       7
#define PVA_MAP_SPECTRUM         8
#define PVA_ZONES_MAX 64
typedef struct PvAmdZoneStat {
    double sum, mean, m2, std;
    float min, max;
    int argmin, argmax;
    int n_finite, n_nan, n_posinf, n_neginf;
} PvAmdZoneStat; /* 64 bytes */
/* Set the zones: labels = gx*gy bytes, cell X*gy + Y, each 0 or 1 .. nZones (copied to the device; they survive runs and
 * geometry changes).  labels = NULL with nZones = 0 clears them.  Waits for a run in flight.  Refused with -1 and nothing
 * changed ("zone statistics: ..."): a label above nZones, nZones outside 1 .. PVA_ZONES_MAX, labels = NULL with nZones > 0,
 * slab groups and slab ranks; on a sparse-emitter solver also clearing the zones while PvAmdSetZoneCurves is enabled or a kind of
 * PvAmdSetZoneMaps is selected.  Labels alone change nothing about a sparse-emitter run; with the curves enabled (a map kind
 * selected), new labels re-derive the tiles, the launch box and the buffers (the tile list and the NaN fill), and the curves
 * (the maps) of the run before are refused */
PVA_EXPORT int PvAmdSetZones(PvAmdSolver* s, const unsigned char* labels, int nZones);
/* the labels as set (gx*gy bytes; labels may be NULL; untouched when no zones are set) and their count (0: none); returns 0 */
PVA_EXPORT int PvAmdGetZones(PvAmdSolver* s, unsigned char* labels, int* nZones);
/* the planes of a kind (PVA_MAP_*) under the current settings: 10, 8, 11, 10, 1 + 3 slots, 1 + 5 windows, 12 bands, 15 bands,
 * 3 bins; -1 where the kind's setting is missing */
PVA_EXPORT int PvAmdZoneStatPlanes(PvAmdSolver* s, int kind);
/* The records of the computed map of `kind` for the current zones: nZones x planes records, zone-major -- zone z, plane k at
 * out[(z - 1) * planes + k]; returns their number, or -1 with PvAmdLastError.  Refused: no zones set, cap below
 * nZones x planes, a kind whose map is not valid (the kind's own "not computed ..." or missing-setting message behind
 * "zone statistics: ").  Synchronous on the solver's own stream (waits for a run in flight); *ms (optional): device time of the
 * passes.  Nothing is cached: the call neither changes the map nor invalidates any kind. */
PVA_EXPORT int PvAmdComputeZoneStats(PvAmdSolver* s, int kind, PvAmdZoneStat* out, int cap, float* ms);
/* CPU only: the definition above applied to a map as PvAmdCopy<Kind> returns it (gx*gy records of `planes` floats, cell-major);
 * out = nZones x planes records, zone-major.  The restatement the tests hold the kernel to.  The labels are checked by the rule
 * of PvAmdSetZones */
PVA_EXPORT int PvAmdHostZoneStats(const float* map, int gx, int gy, int planes, const unsigned char* labels, int nZones,
                                  PvAmdZoneStat* out);
/* CPU only: labels from n <= PVA_ZONES_MAX rectangles rect4[4 j ..] = {xmin, zmin, xmax, zmax} in metres: cell (X, Y) gets j + 1
 * where xmin <= (X + 0.5f) * dx < xmax and zmin <= (Y + 0.5f) * dx < zmax in float32; later rectangles overwrite earlier ones;
 * cells in no rectangle get 0 */
PVA_EXPORT int PvAmdHostZoneRects(float dx, int gx, int gy, const float* rect4, int n, unsigned char* labels);

/* ---- Zone decay: the ensemble decay curve of a receiver area and the decay times read off it ----
 * ISO 3382-2 states the reverberation time of a room or an area either as the average of the positions' decay times (the zone
 * statistics of PVA_MAP_DECAY_TIMES above) or from ONE ensemble decay curve: the squared impulse responses of all positions summed,
 * integrated backwards, and EDT, T20 and T30 read off that curve.  PvAmdComputeZoneDecay reduces the recorded history itself,
 * [T][cells] -> [zones][T], ON THE DEVICE (pv_zone_decay.hip); only nZones x T doubles and the records cross to the host.
 * Inputs: the last completed run, the labels of PvAmdSetZones, and align.  Definition, for zone z:
 *   members  the result cells s = X * gy + Y with labels[s] == z that have an onset in that run (delay[s] != FLT_MAX; cells
 *            outside the run's history window have none); t0(s) = (int)delay[s]; n_cells = their number, t_first / t_last the
 *            smallest / largest t0, both -1 for a zone without a member;
 *   p_s(t)   exactly what PvAmdCopyHistoryPlane(t) gives at array cell (X, Y); only the samples t0(s) <= t < T are used;
 *   slot     of a sample: PVA_ZONE_DECAY_ABSOLUTE j = t (time since emission); PVA_ZONE_DECAY_ONSET j = t - t0(s) (the
 *            beginnings synchronised);
 *   etc[j]   the energy-time curve, j = 0 .. T - 1: the three-level sum of the zone statistics above, unchanged -- butterfly over
 *            blocks of 64 consecutive Y, the blocks of a row sequentially, the rows sequentially in X, each from +0.0 -- applied
 *            to v(X, Y) = (double)p * (double)p (exact in double) for a member whose sample for slot j exists (ABSOLUTE:
 *            j >= t0; ONSET: t0 + j < T) and +0.0 for every other cell; blocks and rows without such a member are skipped;
 *   edc[j]   the Schroeder curve: edc[T] = +0.0, edc[j] = edc[j + 1] + etc[j] for j = T - 1 .. 0, in double; slots before the
 *            first member sample add +0.0, so edc[0] holds E0 bit for bit;
 *   fits     tailN as for PvAmdDecayTimes; j0 = ABSOLUTE ? t_first : 0; jEnd = ABSOLUTE ? T - tailN : T - tailN - t_last (in
 *            ONSET mode the slots past jEnd no longer hold every cell); e0 = edc[j0]; r(j) = edc[j] / e0; L(j) = 10.0 *
 *            log10(r(j)) in double with the host libm's log10; the three ranges of PvAmdDecayTimes with the same float limits
 *            widened to double; membership r <= hi && r >= lo for j in [j0, jEnd), k = j - j0; n, kmin, kmax, Sy, Sky, kbar and
 *            slope as there, all in double, the steps taken in decreasing j, nothing fused; value = (-60.0 / slope) /
 *            (double)fs.  A range is complete iff j0 < jEnd && r(jEnd - 1) < lo; value is quiet NaN unless the range is complete
 *            and n >= 2; depth = j0 < jEnd ? L(jEnd - 1) : NaN;
 *   empty    a zone without a member: e0 = +0.0, the five doubles quiet NaN, the three n zero.
 * The device computes etc and the three integers (order-independent); edc and the fits are finished on the host by the function
 * PvAmdHostZoneDecay ends with.  PvAmdHostZoneDecay applies the whole rule on the CPU, bit for bit.
 * Device storage: the zone scratch of the zone statistics, grown on demand -- 8 bytes per zone, result row and time slot in
 * flight, the slots dealt in chunks that keep it within 32 MiB, plus nZones x T doubles and 12 bytes per zone and result row.
 * Per-band curves and the clarity and centre time of a zone's curve: the zone band decay below.
 * Sparse-emitter (PVA_OPT_STREAMING_ANALYSIS) solvers keep a ring of planes instead of the history.  There the ABSOLUTE curve
 * is a streaming reduction -- etc[j] needs plane j and the onsets <= j only -- and is accumulated INSIDE every run that follows
 * PvAmdSetZoneCurves(s, 1), per accumulate pass off the ring, by the definition above word for word (the launch covers the
 * labels' bounding box: the rows and blocks it leaves out hold no member).  PvAmdComputeZoneDecay(ABSOLUTE) then runs the members
 * pass over the run's onset map, copies nZones x T doubles and finishes on the host: the same records and curves, bit for bit,
 * as a solver that keeps its history gives for the same scene, listener and labels.  While enabled, a tile that holds a
 * labelled cell stays in the ring and records for the whole run, as a registered emitter's tile does; device storage:
 * nZones x T doubles plus the row sums of one chunk of steps (8 bytes per zone, row of the box and step, within 32 MiB).
 * PvAmdHostZoneCurveClarity gives such a curve its clarity and centre time.
 * Out of scope: normalising each cell by its own E0, live-module records, overlapping zones, slab groups and slab ranks; in
 * sparse-emitter mode also PVA_ZONE_DECAY_ONSET (every member's sample of a slot is needed at once, and they arrive at different
 * steps) and the band curves (the filter walks backwards in time).  The zone statistics of the room metrics and the spectrum are
 * available there through PvAmdSetZoneMaps; those of the seven other kinds are not (decay times, band metrics and modulation walk
 * backwards in time, the echo criterion needs c(k - nD), the three velocity kinds need the neighbours from the light cone on). */
#define PVA_ZONE_DECAY_ABSOLUTE 0
#define PVA_ZONE_DECAY_ONSET    1
typedef struct PvAmdZoneDecay {
    double edt, t20, t30, e0, depth;
    int n_edt, n_t20, n_t30, n_cells, t_first, t_last;
} PvAmdZoneDecay; /* 64 bytes */
/* The records of the current zones for the last completed run: out[z - 1] for zone z; returns nZones, or -1 with PvAmdLastError.
 * etc / edc (optional): nZones x T doubles each, zone-major.  *ms (optional): device time of the passes.  Synchronous on the
 * solver's own stream (waits for a run in flight).  Nothing is cached and nothing invalidated: no map, plan or run chain is
 * touched.  Refused ("zone decay: ..."): NULL solver or out, a bad align, no zones set, cap < nZones, no completed run or a last
 * run that ended in error, PVA_OPT_SKIP_ANALYSIS, slab groups and slab ranks; on a sparse-emitter (streaming) solver: curves not
 * enabled ("... history is not kept ..."), align = ONSET, and a last run that was enqueued before the curves were enabled or
 * before the current labels were set.  There the call launches the members pass only (*ms is its time) */
PVA_EXPORT int PvAmdComputeZoneDecay(PvAmdSolver* s, int align, PvAmdZoneDecay* out, int cap, double* etc, double* edc, float* ms);
/* Sparse-emitter solvers only: accumulate the ABSOLUTE zone curves inside every following run (enable != 0), or stop (0).  Needs
 * zones (PvAmdSetZones); waits for a run in flight; allocates on enable and frees on disable; enabling twice changes nothing.
 * Returns 0, or -1 with PvAmdLastError "zone curves: ...": NULL, a solver that keeps its history (it needs none of this), slab
 * groups and slab ranks, no zones set.  With the curves disabled a run is launch for launch what it was before */
PVA_EXPORT int PvAmdSetZoneCurves(PvAmdSolver* s, int enable);
/* *enabled = 1 while PvAmdSetZoneCurves holds, else 0 (a solver that keeps its history: 0); returns 0 */
PVA_EXPORT int PvAmdGetZoneCurves(PvAmdSolver* s, int* enabled);
/* ---- Zone maps: room-metrics and spectrum records of every labelled cell, accumulated inside a sparse-emitter run ----
 * Sparse-emitter solvers only.  Both kinds are forward sums from the cell's onset -- six float32 sums for the room metrics, re
 * and im per bin for the spectrum, each sequential in increasing t from +0.0f -- so they are advanced per accumulate pass off the
 * ring, in the pass that follows the one that settles the onset, and end with the same bits a walk over a kept history gives.
 * Definition: the record of a LABELLED cell (PvAmdSetZones, label != 0) is the kind's own definition above (PvAmdRoomMetrics,
 * spectrum) word for word -- ten quiet NaNs / 3 n quiet NaNs where the cell has no onset in that run (wall cells among them;
 * nothing is carried over from earlier runs); every UNLABELLED cell holds quiet NaN in every float.  Every record matches, bit for
 * bit, what PvAmdComputeRoomMetrics / PvAmdComputeSpectrum give at that cell on a second solver that keeps its history (same
 * scene, listener, labels and bins), and PvAmdComputeZoneStats of the two kinds matches byte for byte.
 * PvAmdSetZoneMaps(kinds) selects PVA_ZMAP_ROOM_METRICS and / or PVA_ZMAP_SPECTRUM for every following run; kinds = 0 deselects.
 * It waits for a run in flight, allocates on select and frees on deselect.  Device storage: the kind's own map over the whole
 * grid (tile-rounded) -- 10 x 4 bytes per cell for the room metrics (about 0.67 GB at 4096^2), 3 n x 4 bytes per cell for the
 * spectrum -- plus 4 bytes per labelled tile; storage over the labelled tiles only is out of scope.  While a kind is selected a
 * tile that holds a labelled cell stays in the ring and records for the whole run, as with PvAmdSetZoneCurves (neither selector
 * drops the other's tiles), PvAmdSetZones(NULL, 0) is refused, and PvAmdSetSpectrumBins(.., 0) is refused while PVA_ZMAP_SPECTRUM
 * is selected.  Changing labels or bins is allowed and re-derives the storage.
 * After a run that accumulated a kind, PvAmdCopyRoomMetrics / ..Block / PvAmdGetRoomMetrics, PvAmdCopySpectrum / ..Block /
 * PvAmdGetSpectrum and PvAmdComputeZoneStats(PVA_MAP_ROOM_METRICS / PVA_MAP_SPECTRUM) work on that map (they wait for a run in
 * flight).  Refused there ("room metrics: ..." / "spectrum: ..."): no completed run, a last run that ended in error, and a last run
 * that was enqueued before the kind was selected, before the current labels were set or before the current bins were set.  With no
 * kind selected every call refuses as it did.  With nothing selected a run is launch for launch what it was before.
 * Returns 0, or -1 with PvAmdLastError "zone maps: ..." and nothing changed: NULL, unknown bits, a solver that keeps its history
 * (it has PvAmdCompute*), slab groups and slab ranks, PVA_OPT_SKIP_ANALYSIS, no zones set, PVA_ZMAP_SPECTRUM with no bins set.
 * Out of scope: the seven other map kinds, ONSET and band curves, the live module, slab groups and slab ranks. */
#define PVA_ZMAP_ROOM_METRICS 1u
#define PVA_ZMAP_SPECTRUM     2u
PVA_EXPORT int PvAmdSetZoneMaps(PvAmdSolver* s, unsigned kinds);
/* *kinds = the kinds PvAmdSetZoneMaps holds (a solver that keeps its history: 0); returns 0 */
PVA_EXPORT int PvAmdGetZoneMaps(PvAmdSolver* s, unsigned* kinds);
/* CPU only: one accumulate pass [tA, tB) of the room metrics restated -- the six sums (e50, l50, e80, l80, total, moment) advanced
 * over t = max(tA, onset) .. min(tB, T) - 1 by the per-sample update of the definition; a cell whose onset lies in the pass
 * (onset >= tA) starts from +0.0f and never reads sums6; onset >= min(tB, T) changes nothing */
PVA_EXPORT int PvAmdHostRoomSumsAdvance(const float* p, int T, int fs, int onset, int tA, int tB, float sums6[6]);
/* CPU only: the record of six such sums: c50, c80, d50, ts derived as the definition says, then the sums themselves */
PVA_EXPORT int PvAmdHostRoomMetricsFromSums(const float sums6[6], int fs, PvAmdRoomMetrics* out);
/* CPU only: the same pass for the spectrum -- re, im of bin j at reim2n[2 j], [2 j + 1], the tables of PvAmdHostSpectrumTables
 * (T x n floats each, indexed by absolute step) */
PVA_EXPORT int PvAmdHostSpectrumAdvance(const float* p, int T, int onset, int tA, int tB, const float* cosTn, const float* sinTn,
                                        int n, float* reim2n);
/* CPU only: what labels mean for a sparse-emitter run with the curves enabled -- flags = ceil(gx / tileRows) x ceil(gy / tileCols)
 * bytes, 1 for every tile that holds a labelled cell (it stays in the ring), box4 = the first and last labelled row and the
 * first and last labelled block of 64 Y (0, -1, 0, -1 for no labelled cell): the extent of the curve launches */
PVA_EXPORT int PvAmdHostZoneTiles(const unsigned char* labels, int gx, int gy, int tileRows, int tileCols, unsigned char* flags,
                                  int box4[4]);
/* CPU only: out[t] = 1 where emitterFlags[t] or zoneFlags[t] is set (either may be NULL: none): the tile plane of a run */
PVA_EXPORT int PvAmdHostZoneTileUnion(const unsigned char* emitterFlags, const unsigned char* zoneFlags, int ntiles,
                                      unsigned char* out);
/* CPU only: the steps of an accumulate pass one pair of curve launches takes for nZones zones and a box of `rows` rows under a
 * scratch bound: a multiple of 16 whose row sums fit the bound, 16 where even that is more */
PVA_EXPORT int PvAmdHostZoneCurveChunk(int nZones, int rows, long long scratchBytes);
/* the time slots PvAmdComputeZoneDecay deals per pair of launches under the current zones (the scratch bound above); T and more:
 * all at once */
PVA_EXPORT int PvAmdZoneDecayChunkSlots(PvAmdSolver* s);
/* CPU only: the definition above applied to a history p[t * gx * gy + X * gy + Y] of T planes and an onset map delay[X * gy + Y]
 * (FLT_MAX: none); out = nZones records, etc / edc (optional) = nZones x T doubles.  The restatement the tests hold the kernel to.
 * The labels are checked by the rule of PvAmdSetZones; an onset of a labelled cell outside 0 .. T - 1 is refused */
PVA_EXPORT int PvAmdHostZoneDecay(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels,
                                  int nZones, int align, PvAmdZoneDecay* out, double* etc, double* edc);
/* ---- Zone band decay: the ensemble decay curve of a receiver area PER OCTAVE OR THIRD-OCTAVE BAND, and the clarity of a curve ----
 * ISO 3382-2 reports an area's reverberation time per band.  The average of the positions' band decay times is the zone
 * statistics of PVA_MAP_BAND_METRICS; this is the other method, one ensemble curve per zone AND band: the band-filtered histories
 * squared, summed, integrated backwards.  PvAmdComputeZoneBandDecay reduces the FILTERED history, [T][cells] -> [zones][bands][T],
 * ON THE DEVICE (pv_zone_band_decay.hip); only nZones x nBands x T doubles and the records cross to the host.
 * Inputs: the last completed run, the labels of PvAmdSetZones, the bands of PvAmdSetBands (nBands >= 1) and align.  Definition,
 * for zone z and band b:
 *   members, t0(s), n_cells, t_first, t_last   PvAmdZoneDecay's, word for word; they do not depend on the band;
 *   y_{s,b}(t)  the band-metrics filter, word for word: the ten float32 coefficients PvAmdGetBandCoefs returns for band b, two
 *            sections in transposed direct form II, float32, every product and sum rounded on its own (no FMA), denormals kept;
 *            state +0.0f at t = T - 1, walking t = T - 1 DOWN TO t0(s) and stopping there; x(t) is exactly what
 *            PvAmdCopyHistoryPlane(t) gives at array cell (X, Y); nothing below t0(s) is read;
 *   slot     of a sample: PVA_ZONE_DECAY_ABSOLUTE j = t; PVA_ZONE_DECAY_ONSET j = t - t0(s);
 *   etc[z][b][j]  j = 0 .. T - 1: the three-level sum of the zone statistics, unchanged -- butterfly over blocks of 64 consecutive
 *            Y, the blocks of a row sequentially, the rows sequentially in X, each from +0.0 -- applied to v(X, Y) = (double)y *
 *            (double)y (exact in double) for a member whose sample for slot j exists and +0.0 for every other cell.  Blocks and
 *            rows without such a member are skipped, which changes no bit: no sum here is ever -0.0 (every term is a square or
 *            +0.0), so adding +0.0 to it returns it;
 *   edc, edt, t20, t30, e0, depth, n_*   the finish of PvAmdZoneDecay applied to etc[z][b], unchanged and shared (one function);
 *   clarity  of the curve (double throughout, the host libm's log10, nothing fused): j0 and tailN as in the fits (an empty zone:
 *            j0 = 0); n50 = (int)(0.05f * (float)fs), n80 = (int)(0.08f * (float)fs); m50 = min(j0 + n50, T); l50 = edc[m50] with
 *            edc[T] = +0.0; e50 = the sum of etc[j] for j = j0 .. m50 - 1 in increasing j from +0.0; e80, l80 likewise; moment =
 *            the sum of (double)(j - j0) * etc[j] for j = j0 .. T - 1 in increasing j; c50 = 10 * log10(e50 / l50), c80 likewise;
 *            d50 = e50 / (e50 + l50); ts = (moment / e0) / (double)fs.  Nothing is special-cased: an empty zone has quiet NaNs.
 *            These are the ISO 3382-1 quantities in ONSET alignment.  In ABSOLUTE alignment they are measured from the zone's FIRST
 *            onset and mix the cells' travel times.
 * The device computes etc and the three integers; the rest is finished on the host by the function PvAmdHostZoneBandDecay ends
 * with.  Time is not cut into chunks (the filter state crosses them): the pass deals its work in chunks of (zone, band) pairs.
 * Device storage: the zone scratch, grown on demand -- per (zone, band) pair in flight gx rows of T doubles; all bands of as many
 * whole zones as stay within 32 MiB, or one zone and as many bands as stay within it; where ONE pair's rows exceed 32 MiB, one
 * pair's rows are what it takes -- plus nZones x nBands x T doubles and 12 bytes per zone and result row.
 * Out of scope: in-run or live-module zone records, overlapping zones, normalising each cell by its own E0, slab groups, slab
 * ranks and sparse-emitter solvers (refused). */
typedef struct PvAmdZoneBandDecay {
    double edt, t20, t30, e0, depth, c50, c80, d50, ts;
    int n_edt, n_t20, n_t30, n_cells, t_first, t_last;
} PvAmdZoneBandDecay; /* 96 bytes */
/* The records of the current zones and bands for the last completed run: out[(z - 1) * nBands + b]; returns nZones x nBands, or
 * -1 with PvAmdLastError.  etc / edc (optional): nZones x nBands x T doubles each, zone-major then band.  *ms (optional): device
 * time of the passes.  Synchronous on the solver's own stream (waits for a run in flight).  Nothing is cached and nothing
 * invalidated: no map, plan or run chain is touched, and every call reads the bands as set at that moment.  Refused ("zone band
 * decay: ..."): what PvAmdComputeZoneDecay refuses, no bands set, cap < nZones x nBands */
PVA_EXPORT int PvAmdComputeZoneBandDecay(PvAmdSolver* s, int align, PvAmdZoneBandDecay* out, int cap, double* etc, double* edc,
                                         float* ms);
/* how PvAmdComputeZoneBandDecay deals its work under the current zones and bands: returns the number of chunks of (zone, band)
 * pairs (0: no zones or no bands set); *slots (optional) = the time slots of a chunk (T: time is never cut), *bands (optional) =
 * the bands of a chunk */
PVA_EXPORT int PvAmdZoneBandDecayChunk(PvAmdSolver* s, int* slots, int* bands);
/* CPU only: the whole rule applied to a history p[t * gx * gy + X * gy + Y] of T planes, an onset map delay[X * gy + Y]
 * (FLT_MAX: none) and nBands (1 .. PVA_BANDS_MAX) coefficient sets of ten floats (PvAmdHostBandCoefs / PvAmdGetBandCoefs); out =
 * nZones x nBands records, etc / edc (optional) = nZones x nBands x T doubles.  The restatement the kernels are held to.  Labels
 * and onsets are checked as by PvAmdHostZoneDecay */
PVA_EXPORT int PvAmdHostZoneBandDecay(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels,
                                      int nZones, const float* coefs10n, int nBands, int align, PvAmdZoneBandDecay* out, double* etc,
                                      double* edc);
/* CPU only: the clarity rule above applied to ANY energy-time curve etc[T] whose beginning is slot j0 (0 <= j0 < T): out4 = c50,
 * c80, d50, ts.  With the etc of PvAmdComputeZoneDecay it gives the broadband curve its clarity and centre time */
PVA_EXPORT int PvAmdHostZoneCurveClarity(const double* etc, int T, int fs, int j0, double out4[4]);
/* Gaussian pulse table (Grid.cpp:12-27), T floats */
PVA_EXPORT int PvAmdCopyPulse(PvAmdSolver* s, float* out);
/* Material planes after rasterisation: beta (uint8) and R (float), (gx+1)*(gy+1) each (with shapes: the composed material) */
PVA_EXPORT int PvAmdCopyMaterial(PvAmdSolver* s, uint8_t* beta, float* R);
/* Overwrite the fields the NEXT PvAmdRunSteps starts from (test / benchmark hook; reference order) */
PVA_EXPORT int PvAmdSetFields(PvAmdSolver* s, const float* pr, const float* vx, const float* vy);
/* Advance `nsteps` time steps from the current fields without resetting them, without pulse when
 * withPulse == 0 and without recording history: the raw stencil (used for roofline measurements and for
 * linearity / equivalence property tests). */
PVA_EXPORT int PvAmdRunSteps(PvAmdSolver* s, int nsteps, int withPulse, float lx, float lz);

/* ------------------------------------------------------------------------------------------------------------
 * Part 3 -- independent runs sharded over the GPUs of one node, C++ host side
 * A "run" = one listener position on one scene (one iteration of the reference's loop, PvContext.cpp:74-93).  Runs share
 * nothing: run k belongs to rank k mod world (a rank = one process, normally one GPU); inside a rank the runs go round-
 * robin over the rank's solvers, kept busy through their own HIP streams.  The only exchange is ONE all-gather of the
 * per-emitter records, RCCL (ncclAllGather over xGMI) when the ranks span processes.  RCCL is bound at run time
 * (dlopen): a single-GPU user of this library needs no RCCL.
 * ---------------------------------------------------------------------------------------------------------- */
/* the plan itself (no device needed): fills runIdx[i] / solverIdx[i] for this rank's i-th run, returns their number
 * (<= cap entries written) */
PVA_EXPORT int PvAmdShardPlan(int nRuns, int world, int rank, int nLocalSolvers, int* runIdx, int* solverIdx, int cap);
/* the segment plan of PVA_OPT_STREAM_ROWS (no device needed; test hook): air[ti * nty + tj] != 0 marks the air tiles;
 * fills seg4[4 i .. 4 i + 3] = {first array row, rows, first tile column, tile columns} for up to cap segments, returns
 * their number.  Every air tile is covered by exactly one segment. */
PVA_EXPORT int PvAmdPlanSegments(const unsigned char* air, int ntx, int nty, int tileRows, int maxTileColumns, int target,
                                 int* seg4, int cap);
typedef struct PvAmdComm PvAmdComm;
/* rank 0 creates the 128-byte id (ncclGetUniqueId) and hands it to every rank by whatever bootstrap the host has
 * (a file, MPI, torch.distributed's store); every rank then joins (ncclCommInitRank) with its HIP device */
PVA_EXPORT int PvAmdCommUniqueId(char id128[128]);
PVA_EXPORT PvAmdComm* PvAmdCommCreate(const char id128[128], int rank, int world, int device);
PVA_EXPORT void PvAmdCommDestroy(PvAmdComm* c);
/* every rank contributes countPerRank floats; all = world * countPerRank floats, rank-major, on every rank */
PVA_EXPORT int PvAmdCommAllGather(PvAmdComm* c, const float* mine, int countPerRank, float* all);
/* Simulate nRuns listener positions (listenersXYZ[3k..]) with emittersPerRun emitter positions each
 * (emittersXYZ[(k*emittersPerRun + e)*3 ..]) on this rank's `solvers` (identically configured, scenes loaded by the
 * caller; two per GPU keep two runs in flight) and gather all records: out[k*emittersPerRun + e] on every
 * rank.  world == 1: comm may be NULL.  Returns 0, or -1 with PvAmdLastError. */
PVA_EXPORT int PvAmdRunSharded(PvAmdSolver* const* solvers, int nSolvers, const float* listenersXYZ, int nRuns,
                               const float* emittersXYZ, int emittersPerRun, int rank, int world, PvAmdComm* comm,
                               PlaneverbOutput* out);

/* Host-side pieces of the path that need no device (grid arithmetic, pulse table, rasteriser, .pv parser); the
 * solver uses exactly these internally.  Exposed so that they can be checked without a GPU. */
/* Grid.cpp:390-396,46-55: fills gx, gy, T, fs, res, dx, dt (other fields 0) */
PVA_EXPORT int PvAmdHostGridInfo(float gridSizeX, float gridSizeY, int gridResolution, PvAmdInfo* out);
/* Grid.cpp:12-27: T floats */
PVA_EXPORT int PvAmdHostPulse(float gridSizeX, float gridSizeY, int gridResolution, float* out);
/* 1 if this host's expf reproduces five samples of the reference's 275 Hz pulse table bit for bit (the pulse is made
 * with the host libm, as in the reference: Grid.cpp:12-27), else 0.  The solver checks this once per process by itself
 * and warns on stderr. */
PVA_EXPORT int PvAmdHostPulseSelfCheck(void);
/* Grid::AddAABB / RemoveAABB on a fresh grid: ops[i] = +1 add / -1 remove of boxes5[5*i..]; beta, R are
 * (gx+1)*(gy+1) */
PVA_EXPORT int PvAmdHostRasterize(float gridSizeX, float gridSizeY, int gridResolution, const float* boxes5,
                                  const int* ops, int n, uint8_t* beta, float* R);
/* Editor.cpp:245-281: returns the number of boxes (<= maxBoxes written as 5 floats each) or -1 */
PVA_EXPORT int PvAmdHostLoadPv(const char* pvPath, float* boxes5, int maxBoxes);
/* Editor.cpp:219-243: writes `n` boxes (ids[i] or i when ids == NULL) in the .pv text format; 0 = ok */
PVA_EXPORT int PvAmdHostSavePv(const char* pvPath, const float* boxes5, const int* ids, int n);
/* FDTD.cpp:97-98 listener cell and Analyzer.cpp:106-116 result cell (valid = 0 where GetOutput returns -1) */
PVA_EXPORT int PvAmdHostCells(float gridSizeX, float gridSizeY, int gridResolution, float x, float z, int* listenerCx,
                              int* listenerCy, int* resultCx, int* resultCy, int* resultValid);

/* PlaneverbDSP reverb-bus split of wetGain by rt60 (PlaneverbDSP/src/PvDSPContext.cpp:165-228) */
PVA_EXPORT void PvAmdReverbBusGains(float rt60, float wetGain, float* a, float* b, float* c);

/* ------------------------------------------------------------------------------------------------------------
 * Part 4 -- baked probe tables (extension; INTEGRATION.md "Baked probe tables" documents the query rule and the file format)
 * A bake simulates a lattice of listener positions ("probes") (x0 + i sx, 0, z0 + j sz), i < nx, j < nz, probe k = j nx + i, and
 * keeps, per probe, the block of emitter-lattice nodes -- result cells (r, c) with r % stride == 0 and c % stride == 0 -- that
 * its run reached: the bounding box of the reached nodes inside the run's history window, 9 float32 per node (the 8 members in
 * PvAmdCopyResults order, then the onset delay; an unreached node inside the box: zeros and FLT_MAX).  Probe state: 0 = not
 * baked, 1 = baked, 2 = baked but invalid (the listener cell (int)((x + 0) / dx), (int)((z + 0) / dx) of FDTD.cpp:97-98 lies
 * outside the result map or is not air in the composed material: not run).  PvAmdBakeQuery interpolates a record for any
 * listener / emitter pair from the 4 probes and 4 emitter nodes around them, with no solver.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct PvAmdBake PvAmdBake;
typedef struct PvAmdBakeInfo {
    int gx, gy, T, fs, res;
    float dx;
    int stride;                 /* emitter-lattice stride d >= 1 (result cells) */
    float x0, z0, sx, sz;       /* probe lattice origin and spacing, metres */
    int nx, nz;
    int probesBaked;            /* probes in state 1 or 2 */
    int probesInvalid;          /* probes in state 2 */
    long long records;          /* stored nodes (9 floats each) */
    unsigned long long materialHash; /* FNV-1a 64 of the composed material: beta ((gx+1)(gy+1) bytes), then R ((gx+1)(gy+1) float32) */
} PvAmdBakeInfo;
/* a bake of nothing yet, for the grid (gx, gy, T -- PVA_OPT_NUM_STEPS included --, fs, res, dx) and the material of `like`;
 * NULL with PvAmdLastError for stride < 1, nx or nz < 1, a non-finite origin or a spacing that is not finite and > 0 */
PVA_EXPORT PvAmdBake* PvAmdBakeCreate(PvAmdSolver* like, int stride, float x0, float z0, float sx, float sz, int nx, int nz);
/* bake the probes k with k % world == rank, dealt round-robin over the n solvers (one run in flight each: two solvers on a GPU
 * keep two runs in flight), through PvAmdRunAsync.  Refused (-1): a solver with another grid or material hash, a slab group or
 * slab rank, a solver in sparse-emitter mode (PVA_OPT_STREAMING_ANALYSIS) or one that skips the analysis.  The solvers' result
 * maps change as after their runs; what they carried from earlier runs never enters the bake (only this run's onsets decide
 * what is reached, unreached nodes are stored as zeros + FLT_MAX). */
PVA_EXPORT int PvAmdBakeRun(PvAmdBake* b, PvAmdSolver* const* solvers, int n, int rank, int world);
/* copy src's baked probes (state != 0) into dst; refused for another lattice, grid or material hash, or a probe that both hold
 * with different contents */
PVA_EXPORT int PvAmdBakeMerge(PvAmdBake* dst, const PvAmdBake* src);
PVA_EXPORT int PvAmdBakeSave(const PvAmdBake* b, const char* path);
/* NULL + PvAmdLastError for a wrong magic or version, inconsistent sizes, offsets or blocks outside the file or the lattice, a
 * checksum mismatch.  PvAmdBakeSave(PvAmdBakeLoad(f)) reproduces f byte for byte. */
PVA_EXPORT PvAmdBake* PvAmdBakeLoad(const char* path);
PVA_EXPORT void PvAmdBakeDestroy(PvAmdBake* b);
PVA_EXPORT int PvAmdBakeGetInfo(const PvAmdBake* b, PvAmdBakeInfo* out);
/* probe k: state5 = {state, i0, j0, ni, nj} (the block: lattice nodes [i0, i0 + ni) x [j0, j0 + nj), node (i, j) = result
 * cell (i stride, j stride)), rec9 (may be NULL) = ni nj x 9 floats, row-major; returns ni nj, or -1 */
PVA_EXPORT int PvAmdBakeProbe(const PvAmdBake* b, int k, int* state5 /* state, i0, j0, ni, nj */, float* rec9 /* may be NULL */);
/* n listener / emitter pairs (x, y, z each; y is ignored) -> n records by the query rule; CPU only */
PVA_EXPORT int PvAmdBakeQuery(const PvAmdBake* b, const float* listenersXYZ, const float* emittersXYZ, int n, PlaneverbOutput* out);
/* the same on HIP device `device`, one thread per query, bit-identical to PvAmdBakeQuery; the bake is uploaded once per device
 * and kept there until PvAmdBakeRun or PvAmdBakeMerge changes it */
PVA_EXPORT int PvAmdBakeQueryDevice(const PvAmdBake* b, int device, const float* listenersXYZ, const float* emittersXYZ, int n,
                                    PlaneverbOutput* out);

#ifdef __cplusplus
}
#endif
#endif /* PLANEVERB_AMD_H */
