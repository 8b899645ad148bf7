// pv_capi.cpp -- extern "C" boundary of libplaneverb_amd.so (declared in include/planeverb_amd.h).
// No C++ exception leaves this file; the reference's sentinels are kept (-1 ids, occlusion = -1).
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "../../include/planeverb_amd.h"
#include "pv_context.h"
#include "pv_core.h"
#include "pv_bands.h"
#include "pv_modulation.h"
#include "pv_decay.h"
#include "pv_echo.h"
#include "pv_echogram.h"
#include "pv_lateral.h"
#include "pv_lobes.h"
#include "pv_metrics.h"
#include "pv_query_records.h"
#include "pv_query_spectral.h"
#include "pv_spectrum.h"
#include "pv_waterfall.h"
#include "pv_arrays.h"
#include "pv_aural.h"
#include "pv_zone_band_decay.h"
#include "pv_zone_decay.h"
#include "pv_zones.h"
#ifndef PVA_HOST_TEST  // (tests/host/: HIP-less sanitizer build of the live module against a fake Solver)
#include "pv_bake.h"
#include "pv_shard.h"
#include "pv_slabs.h"
#include "pv_launch.h"
#include "pv_layer.h"
#include "pv_solver.h"
#endif

using namespace pva;

static thread_local std::string g_lastError;

// ---------------------------------------------------------------------------------------------------------------
// The exception barrier (the reference throws from Init, PvContext.cpp:106,123, Grid.cpp:69; a C-ABI must
// not).  EVERY extern "C" body below is a function-try-block closed by one of these macros: whatever is thrown underneath
// (std::bad_alloc from a table growing, std::system_error from a thread or a mutex, anything from the HIP runtime's C++
// side) ends here, the call returns its failure sentinel and PvAmdLastError() names the function and the exception.
// tests/host/alloc_fault.cpp drives every allocation of the Part 1 calls into failure, one at a time.
// ---------------------------------------------------------------------------------------------------------------
static void noteException(const char* fn) noexcept {
    try {
        std::string what = "unknown exception";
        try {
            throw;
        } catch (const std::bad_alloc&) {
            what = "out of memory (std::bad_alloc)";
        } catch (const std::exception& e) {
            what = e.what();
        } catch (...) {
        }
        g_lastError = std::string("exception in ") + fn + ": " + what;
    } catch (...) {  // (not even the message could be built)
        g_lastError.clear();
    }
}
static PlaneverbOutput invalidOutput() noexcept {
    PlaneverbOutput o;
    std::memset(&o, 0, sizeof(o));
    o.occlusion = kInvalidDryGain;  // FDTD.cpp:22-26
    return o;
}
#define PV_API_CATCH(sentinel) catch (...) { noteException(__func__); return sentinel; }
#define PV_API_CATCH_VOID      catch (...) { noteException(__func__); }
#define PV_API_CATCH_OUTPUT    catch (...) { noteException(__func__); return invalidOutput(); }

#ifndef PVA_HOST_TEST
struct PvAmdSolver {
    Solver* s = nullptr;
    SlabGroup* g = nullptr;     // a slab group instead of one solver (PvAmdCreateSlabs)
    std::vector<int> slabDevices;
    SolverOptions opt;
    GridSpec spec;
    int device = 0;
    ~PvAmdSolver() {
        delete s;
        delete g;
    }
};

// creates the solver / slab group on first use (options come first); `slabsOk` = the call is implemented for groups
static bool ensure(PvAmdSolver* h, bool slabsOk = false) {
    if (!h) {
        g_lastError = "null solver handle";
        return false;
    }
    if (!h->slabDevices.empty()) {
        if (!slabsOk) {
            g_lastError = "not available for a slab group (PvAmdCreateSlabs)";
            return false;
        }
        if (!h->g) h->g = SlabGroup::create(h->spec, h->slabDevices, h->opt, &g_lastError);
        return h->g != nullptr;
    }
    if (h->s) return true;
    h->s = Solver::create(h->spec, h->device, h->opt, &g_lastError);
    return h->s != nullptr;
}

// A handle from PvAmdCreateSlabRank holds ONE slab of the grid (no FreeGrid, no halo exchange of its own): the whole-grid
// entry points (run / outputs / result maps) would silently work on a partial grid, so they refuse it.
static bool wholeGrid(PvAmdSolver* h) {
    if (h && h->opt.slabCount > 1) {
        g_lastError = "slab rank handle: use the PvAmdSlab* / PvAmdSlabRoot* primitives (PvAmdCreateSlabRank)";
        return false;
    }
    return true;
}

struct PvAmdBake {
    std::unique_ptr<Bake> b;
};
static bool bakeOk(const PvAmdBake* b) {
    if (b && b->b) return true;
    g_lastError = "null bake handle";
    return false;
}

static int ret(PvAmdSolver* h, bool ok) {
    if (ok) return 0;
    if (h && h->s && !h->s->lastError().empty()) g_lastError = h->s->lastError();
    if (h && h->g && !h->g->lastError().empty()) g_lastError = h->g->lastError();
    return -1;
}
#endif  // !PVA_HOST_TEST

extern "C" {

// ---------------------------------------------------------------------------------------------------------------
// Part 1: reference C-ABI
// ---------------------------------------------------------------------------------------------------------------

void UnityPluginLoad(void*) try {} PV_API_CATCH_VOID
void UnityPluginUnload(void) try {} PV_API_CATCH_VOID

void PlaneverbInit(float gridSizeX, float gridSizeY, int gridResolution, int gridBoundaryType, char* tempFileDir,
                   int maxThreadUsage, int threadExecutionType) try {
    LiveConfig c;
    c.sizeX = gridSizeX;
    c.sizeY = gridSizeY;
    c.res = gridResolution;
    c.boundaryType = gridBoundaryType;
    c.tempDir = tempFileDir;
    c.maxThreads = maxThreadUsage;
    c.executionType = threadExecutionType;  // 0 (pv_CPU) and 1 (pv_GPU) both run on the HIP device here
    std::string err;
    if (!Context::init(c, &err)) {
        g_lastError = err;
        std::fprintf(stderr, "[planeverb_amd] PlaneverbInit failed: %s\n", err.c_str());
    }
} PV_API_CATCH_VOID

void PlaneverbSetGridBoundary(float xMin, float xMax, float zMin, float zMax) try {
    const float R4[4] = {xMin, xMax, zMin, zMax};
    for (int k = 0; k < 4; ++k)
        if (!(R4[k] - R4[k] == 0.f)) {
            g_lastError = "PlaneverbSetGridBoundary: absorption of side " + std::to_string(k) + " is not finite";
            return;
        }
    Context::Ref c;
    if (c) c->setGridBoundary(R4);
} PV_API_CATCH_VOID

void PlaneverbSetEdgeLayer(int xMin, int xMax, int zMin, int zMax) try {
    const int w4[4] = {xMin, xMax, zMin, zMax};
    Context::Ref c;
    if (!c) {
        g_lastError = "PlaneverbSetEdgeLayer: the module is not initialised";
        return;
    }
    std::string err;
    if (!c->setEdgeLayer(w4, &err)) g_lastError = err;
} PV_API_CATCH_VOID

void PlaneverbSetEdgeLayerSplit(int xMin, int xMax, int zMin, int zMax) try {
    const int w4[4] = {xMin, xMax, zMin, zMax};
    Context::Ref c;
    if (!c) {
        g_lastError = "PlaneverbSetEdgeLayerSplit: the module is not initialised";
        return;
    }
    std::string err;
    if (!c->setEdgeLayer(w4, &err, true, kEdgeLayerSplitR0)) g_lastError = err;
} PV_API_CATCH_VOID

void PlaneverbExit(void) try {
    Context::exit();
} PV_API_CATCH_VOID

int PlaneverbEmit(float x, float y, float z) try {
    Context::Ref c;
    return c ? c->emit(x, y, z) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateEmission(int id, float x, float y, float z) try {
    Context::Ref c;
    if (c) c->updateEmission(id, x, y, z);
} PV_API_CATCH_VOID

void PlaneverbEndEmission(int id) try {
    Context::Ref c;
    if (c) c->endEmission(id);
} PV_API_CATCH_VOID

PlaneverbOutput PlaneverbGetOutput(int emissionID) try {
    PlaneverbOutput o;
    std::memset(&o, 0, sizeof(o));
    Context::Ref c;
    if (!c) {  // FDTD.cpp:22-26
        o.occlusion = kInvalidDryGain;
        return o;
    }
    const Out8 r = c->getOutput(emissionID);
    std::memcpy(&o, r.v, sizeof(o));
    return o;
} PV_API_CATCH_OUTPUT

int PlaneverbAddGeometry(float posX, float posY, float width, float height, float absorption) try {
    Context::Ref c;
    return c ? c->addGeometry(Box{posX, posY, width, height, absorption}) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateGeometry(int id, float posX, float posY, float width, float height, float absorption) try {
    Context::Ref c;
    if (c) c->updateGeometry(id, Box{posX, posY, width, height, absorption});
} PV_API_CATCH_VOID

void PlaneverbRemoveGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeGeometry(id);
} PV_API_CATCH_VOID

// shapes in the live module (pv_core.h makeShape / orientedBoxVertices), queued like the AABB changes (pv_context.cpp)
static bool orientedShape(float px, float py, float w, float h, float ax, float ay, float absorption, Shape* out) {
    float v[8];
    return orientedBoxVertices(px, py, w, h, ax, ay, v, &g_lastError) && makeShape(v, 4, absorption, out, &g_lastError);
}

int PlaneverbAddOrientedGeometry(float posX, float posY, float width, float height, float axisX, float axisY, float absorption) try {
    Context::Ref c;
    Shape sh;
    return (c && orientedShape(posX, posY, width, height, axisX, axisY, absorption, &sh)) ? c->addShape(sh) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateOrientedGeometry(int id, float posX, float posY, float width, float height, float axisX, float axisY,
                                     float absorption) try {
    Context::Ref c;
    Shape sh;
    if (c && orientedShape(posX, posY, width, height, axisX, axisY, absorption, &sh)) c->updateShape(id, sh);
} PV_API_CATCH_VOID

void PlaneverbRemoveOrientedGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeShape(id);
} PV_API_CATCH_VOID

int PlaneverbAddPolygonGeometry(const float* xy, int n, float absorption) try {
    Context::Ref c;
    Shape sh;
    return (c && makeShape(xy, n, absorption, &sh, &g_lastError)) ? c->addShape(sh) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdatePolygonGeometry(int id, const float* xy, int n, float absorption) try {
    Context::Ref c;
    Shape sh;
    if (c && makeShape(xy, n, absorption, &sh, &g_lastError)) c->updateShape(id, sh);
} PV_API_CATCH_VOID

void PlaneverbRemovePolygonGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeShape(id);
} PV_API_CATCH_VOID

// round and concave shapes (pv_core.h makeRound / makePolygon): the same queue and the same ids
static_assert(PVA_POLY_MAX_VERTS == kPolyMaxVerts, "planeverb_amd.h vs pv_core.h");
static bool discShape(float cx, float cy, float radius, float absorption, Shape* out) {
    const float c[2] = {cx, cy};
    return makeRound(c, 1, radius, absorption, out, &g_lastError);
}
static bool capsuleShape(float ax, float ay, float bx, float by, float radius, float absorption, Shape* out) {
    const float p[4] = {ax, ay, bx, by};
    return makeRound(p, 2, radius, absorption, out, &g_lastError);
}
static bool wallPathShape(const float* xy, int n, float radius, float absorption, Shape* out) {
    if (n < 2) {
        g_lastError = "wall path: 2 to 64 points";
        return false;
    }
    return makeRound(xy, n, radius, absorption, out, &g_lastError);
}

int PlaneverbAddDiscGeometry(float posX, float posY, float radius, float absorption) try {
    Context::Ref c;
    Shape sh;
    return (c && discShape(posX, posY, radius, absorption, &sh)) ? c->addShape(sh) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateDiscGeometry(int id, float posX, float posY, float radius, float absorption) try {
    Context::Ref c;
    Shape sh;
    if (c && discShape(posX, posY, radius, absorption, &sh)) c->updateShape(id, sh);
} PV_API_CATCH_VOID

void PlaneverbRemoveDiscGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeShape(id);
} PV_API_CATCH_VOID

int PlaneverbAddWallPathGeometry(const float* xy, int n, float radius, float absorption) try {
    Context::Ref c;
    Shape sh;
    return (c && wallPathShape(xy, n, radius, absorption, &sh)) ? c->addShape(sh) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateWallPathGeometry(int id, const float* xy, int n, float radius, float absorption) try {
    Context::Ref c;
    Shape sh;
    if (c && wallPathShape(xy, n, radius, absorption, &sh)) c->updateShape(id, sh);
} PV_API_CATCH_VOID

void PlaneverbRemoveWallPathGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeShape(id);
} PV_API_CATCH_VOID

int PlaneverbAddConcavePolygonGeometry(const float* xy, int n, float absorption) try {
    Context::Ref c;
    Shape sh;
    return (c && makePolygon(xy, n, absorption, &sh, &g_lastError)) ? c->addShape(sh) : -1;
} PV_API_CATCH(-1)

void PlaneverbUpdateConcavePolygonGeometry(int id, const float* xy, int n, float absorption) try {
    Context::Ref c;
    Shape sh;
    if (c && makePolygon(xy, n, absorption, &sh, &g_lastError)) c->updateShape(id, sh);
} PV_API_CATCH_VOID

void PlaneverbRemoveConcavePolygonGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeShape(id);
} PV_API_CATCH_VOID

// triangle meshes (pv_context.h): validated here, the vertex data copied into the context's store at the Add call
int PlaneverbAddMeshGeometry(const float* verts, int nv, const int* tris, int nt, float absorption, int mode, float radius) try {
    Context::Ref c;
    if (!c || !validateMesh(verts, nv, tris, nt, absorption, mode, radius, &g_lastError)) return -1;
    return c->addMesh(verts, nv, tris, nt, absorption, mode, radius, &g_lastError);
} PV_API_CATCH(-1)

void PlaneverbSetMeshGeometryTransform(int id, const float* m12) try {
    Context::Ref c;
    if (c && validateMeshTransform(m12, &g_lastError)) c->setMeshTransform(id, m12);
} PV_API_CATCH_VOID

void PlaneverbRemoveMeshGeometry(int id) try {
    Context::Ref c;
    if (c) c->removeMesh(id);
} PV_API_CATCH_VOID

void PlaneverbSetSliceHeight(float h) try {
    Context::Ref c;
    if (!(h - h == 0.f)) {
        g_lastError = "PlaneverbSetSliceHeight: the height is not finite";
        return;
    }
    if (c) c->setSliceHeight(h);
} PV_API_CATCH_VOID

void PlaneverbSetListenerPosition(float x, float y, float z) try {
    Context::Ref c;
    if (c) c->setListener(x, y, z);
} PV_API_CATCH_VOID

int PlaneverbLoadScene(const char* pvPath) try {
    Context::Ref c;
    if (!c || !pvPath) return -1;
    std::vector<Box> boxes;
    if (!loadPv(pvPath, &boxes, &g_lastError)) return -1;
    for (const Box& b : boxes) c->addGeometry(b);
    return (int)boxes.size();
} PV_API_CATCH(-1)

long long PlaneverbIterationCount(void) try {
    Context::Ref c;
    return c ? c->iterations() : 0;
} PV_API_CATCH(0)

long long PlaneverbWaitIterations(long long count, int timeoutMs) try {
    Context::Ref c;
    return c ? c->waitIterations(count, timeoutMs) : 0;
} PV_API_CATCH(0)

// 0 also when the simulation worker has stopped on an error (PvAmdLastError then says why)
int PlaneverbIsRunning(void) try {
    Context::Ref c;
    return (c && !c->failed()) ? 1 : 0;
} PV_API_CATCH(0)

int PlaneverbIsStreaming(void) try {
    Context::Ref c;
    return (c && c->streaming()) ? 1 : 0;
} PV_API_CATCH(0)

int PlaneverbGetImpulseResponse(float x, float y, float z, PlaneverbCell* out, int capacity) try {
    Context::Ref c;
    if (!c || capacity < 0) return -1;
    const int n = c->impulseResponse(x, y, z, out, capacity);
    if (n < 0) g_lastError = "impulse response not available (no completed iteration yet, or solver error)";
    return n;
} PV_API_CATCH(-1)

// emission records (pv_context.cpp): the setters answer 0, or -1 with PvAmdLastError "emission records: ..."
static_assert(PVA_RECORD_QUERIES_MAX == kMaxRecordQueries, "planeverb_amd.h vs pv_query_records.h");
static int emissionSetterDown() {
    g_lastError = "emission records: the module is not initialised";
    return -1;
}

int PlaneverbSetEmissionRecords(unsigned kinds) try {
    Context::Ref c;
    if (!c) return emissionSetterDown();
    return c->setEmissionRecords(kinds, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PlaneverbSetEmissionEchogram(float slotSeconds, int nSlots) try {
    Context::Ref c;
    if (!c) return emissionSetterDown();
    return c->setEmissionEchogram(slotSeconds, nSlots, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PlaneverbSetEmissionLobeWindows(const float* edgesSeconds, int nEdges) try {
    Context::Ref c;
    if (!c) return emissionSetterDown();
    return c->setEmissionLobeWindows(edgesSeconds, nEdges, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

unsigned PlaneverbEmissionRecordKinds(void) try {
    Context::Ref c;
    return c ? c->emissionRecordKinds() : 0u;
} PV_API_CATCH(0u)

int PlaneverbEmissionRecordFloats(unsigned kind) try {
    Context::Ref c;
    return c ? c->emissionRecordFloats(kind) : -1;
} PV_API_CATCH(-1)

int PlaneverbEmissionRecordCells(void) try {
    Context::Ref c;
    return c ? c->emissionRecordCells() : -1;
} PV_API_CATCH(-1)

int PlaneverbGetEmissionRecord(int emissionID, unsigned kind, float* out, int capacity) try {
    Context::Ref c;
    return c ? c->emissionRecord(emissionID, kind, out, capacity) : -1;
} PV_API_CATCH(-1)

// ---------------------------------------------------------------------------------------------------------------
// Part 2: batch solver handle
// ---------------------------------------------------------------------------------------------------------------

const char* PvAmdLastError(void) try {
    // A live module whose worker died reports that -- ONCE per failed context and thread, so that the errors of later,
    // unrelated calls on this thread (batch solver, slabs, communicator) stay readable.  PlaneverbWorkerError() always
    // has the worker's reason.
    {
        static thread_local unsigned long long reported = 0;  // (a generation number: addresses are re-used)
        Context::Ref c;
        if (c && c->failed() && reported != c->generation()) {
            reported = c->generation();
            g_lastError = "simulation worker stopped: " + c->workerError();
        }
    }
    return g_lastError.c_str();
} PV_API_CATCH("")
const char* PlaneverbWorkerError(void) try {
    static thread_local std::string w;
    Context::Ref c;
    w = (c && c->failed()) ? c->workerError() : std::string();
    return w.c_str();
} PV_API_CATCH("")
const char* PvAmdVersion(void) try { return "planeverb_amd 0.4.1 (gfx950)"; } PV_API_CATCH("")

// (PvAmdComputeZoneDecay and PvAmdHostZoneDecay)
static bool zoneDecayAlign(int align, const char* pre = "zone decay: ") {
    if (align == kZoneDecayAbsolute || align == kZoneDecayOnset) return true;
    g_lastError = std::string(pre) + "align is PVA_ZONE_DECAY_ABSOLUTE or PVA_ZONE_DECAY_ONSET";
    return false;
}

#ifndef PVA_HOST_TEST
int PvAmdDeviceCount(void) try {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
} PV_API_CATCH(0)

PvAmdSolver* PvAmdCreate(float gridSizeX, float gridSizeY, int gridResolution, int device) try {
    if (gridResolution < kLowResolution || gridSizeX == 0.f || gridSizeY == 0.f) {
        g_lastError = "invalid config (pv_InvalidConfig)";  // PvContext.cpp:101-107
        return nullptr;
    }
    int n = PvAmdDeviceCount();
    if (n <= 0) {
        g_lastError = "no HIP device: libplaneverb_amd has no CPU path";
        return nullptr;
    }
    if (device < 0 || device >= n) {
        g_lastError = "HIP device index out of range";
        return nullptr;
    }
    std::unique_ptr<PvAmdSolver> h(new PvAmdSolver());
    h->spec = makeGridSpec(gridSizeX, gridSizeY, gridResolution);
    h->device = device;
    if (h->spec.gx != h->spec.gy) {
        static bool warned = false;
        if (!warned)
            std::fprintf(stderr, "[planeverb_amd] warning: %d x %d grid -- the reference indexes non-square grids "
                                 "inconsistently (SURVEY.md Q1); results there are defined by this library (cell array stride "
                                 "gy+1 throughout), not by the reference\n", h->spec.gx, h->spec.gy);
        warned = true;
    }
    return h.release();
} PV_API_CATCH(nullptr)

PvAmdSolver* PlaneverbCreateGrid(float gridSizeX, float gridSizeY, int gridResolution, int device) try {
    return PvAmdCreate(gridSizeX, gridSizeY, gridResolution, device);
} PV_API_CATCH(nullptr)

PvAmdSolver* PvAmdCreateSlabs(float gridSizeX, float gridSizeY, int gridResolution, const int* devices, int nslabs) try {
    if (!devices || nslabs < 2 || nslabs > 16) {
        g_lastError = "PvAmdCreateSlabs: 2..16 slabs and their devices";
        return nullptr;
    }
    std::unique_ptr<PvAmdSolver> h(PvAmdCreate(gridSizeX, gridSizeY, gridResolution, devices[0]));
    if (!h) return nullptr;
    const int n = PvAmdDeviceCount();
    for (int i = 0; i < nslabs; ++i) {
        if (devices[i] < 0 || devices[i] >= n) {
            g_lastError = "HIP device index out of range";
            return nullptr;
        }
        h->slabDevices.push_back(devices[i]);
    }
    return h.release();
} PV_API_CATCH(nullptr)

int PvAmdGetSlabInfo(PvAmdSolver* h, PvAmdSlabInfo* out) try {
    if (!out || !ensure(h, true) || !h->g) return -1;
    std::memset(out, 0, sizeof(*out));
    out->nslabs = h->g->numSlabs();
    for (int i = 0; i < out->nslabs; ++i) {
        out->row0[i] = h->g->slabRow0(i);
        out->rows[i] = h->g->slabRows(i);
        out->device[i] = h->g->slab(i)->device();
        out->deviceBytes[i] = h->g->slab(i)->deviceBytes();
    }
    out->haloBytesPerLaunch = h->g->haloBytesPerLaunch();
    out->exchangeBytesPerRun = h->g->exchangeBytesPerRun();
    out->handoffWords = h->g->handoffWords() ? 1 : 0;
    out->streamRedeals = h->g->streamRedeals();
    out->dryRunUsPerSweep = h->g->dryRunUsPerSweep();
    return 0;
} PV_API_CATCH(-1)

PvAmdSolver* PvAmdCreateSlabRank(float gridSizeX, float gridSizeY, int gridResolution, int device, int slabIndex,
                                 int slabCount) try {
    if (slabCount < 2 || slabIndex < 0 || slabIndex >= slabCount) {
        g_lastError = "PvAmdCreateSlabRank: 0 <= slabIndex < slabCount, slabCount >= 2";
        return nullptr;
    }
    PvAmdSolver* h = PvAmdCreate(gridSizeX, gridSizeY, gridResolution, device);
    if (!h) return nullptr;
    h->opt.slabIndex = slabIndex;
    h->opt.slabCount = slabCount;
    return h;
} PV_API_CATCH(nullptr)

int PvAmdComputeEfree(float gridSizeX, float gridSizeY, int gridResolution, int device, float* efree) try {
    if (!efree) return -1;
    std::unique_ptr<PvAmdSolver> h(PvAmdCreate(gridSizeX, gridSizeY, gridResolution, device));
    if (!h) return -1;
    // a throw-away solver of a tiny grid would have another centre cell: the free-field run depends on the grid size
    // (FreeGrid.cpp:78-84), so the real config is used; its planes are what the windowed FreeGrid run needs anyway
    const bool ok = ensure(h.get());
    if (ok) *efree = h->s->efree();
    return ok ? 0 : -1;
} PV_API_CATCH(-1)

static Solver* slabOf(PvAmdSolver* h) {
    if (!ensure(h)) return nullptr;
    if (h->opt.slabCount < 2) {
        g_lastError = "not a slab rank handle (PvAmdCreateSlabRank)";
        return nullptr;
    }
    return h->s;
}

int PvAmdSlabSetEfree(PvAmdSolver* h, float efree) try {
    Solver* s = slabOf(h);
    if (!s) return -1;
    s->setEfree(efree);
    return 0;
} PV_API_CATCH(-1)
int PvAmdSlabBegin(PvAmdSolver* h, float lx, float ly, float lz) try {
    Solver* s = slabOf(h);
    return s ? ret(h, SlabRankOps::begin(*s, lx, ly, lz)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabNumLaunches(PvAmdSolver* h) try {
    Solver* s = slabOf(h);
    return s ? SlabRankOps::numLaunches(*s) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabLaunch(PvAmdSolver* h, int li) try {
    Solver* s = slabOf(h);
    return s ? ret(h, SlabRankOps::launch(*s, li)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabHaloFloats(PvAmdSolver* h) try {
    Solver* s = slabOf(h);
    return s ? SlabRankOps::haloFloats(*s) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabExportHalo(PvAmdSolver* h, int side, float* host) try {
    Solver* s = slabOf(h);
    return (s && host) ? ret(h, SlabRankOps::exportHalo(*s, side, host)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabImportHalo(PvAmdSolver* h, int side, const float* host) try {
    Solver* s = slabOf(h);
    return (s && host) ? ret(h, SlabRankOps::importHalo(*s, side, host)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabHistoryFloats(PvAmdSolver* h) try {
    Solver* s = slabOf(h);
    return s ? SlabRankOps::historyFloats(*s) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabExportEdgeHistory(PvAmdSolver* h, float* host) try {
    Solver* s = slabOf(h);
    return (s && host) ? ret(h, SlabRankOps::exportEdgeHistory(*s, host)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabImportAboveHistory(PvAmdSolver* h, const float* host) try {
    Solver* s = slabOf(h);
    return (s && host) ? ret(h, SlabRankOps::importAboveHistory(*s, host)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabAnalyze(PvAmdSolver* h) try {
    Solver* s = slabOf(h);
    return s ? ret(h, SlabRankOps::analyze(*s)) : -1;
} PV_API_CATCH(-1)
long long PvAmdSlabWindowBlock(PvAmdSolver* h, int* info4, float* host, long long cap) try {
    Solver* s = slabOf(h);
    if (!s || !info4) return -1;
    const long long n = SlabRankOps::windowBlock(*s, &info4[0], &info4[1], &info4[2], &info4[3], host, cap);
    if (n < 0) ret(h, false);
    return n;
} PV_API_CATCH(-1)

struct PvAmdSlabRoot {
    SlabRoot* r = nullptr;
    ~PvAmdSlabRoot() { delete r; }
};
PvAmdSlabRoot* PvAmdSlabRootCreate(PvAmdSolver* anySlab, int device) try {
    Solver* s = slabOf(anySlab);
    if (!s) return nullptr;
    std::unique_ptr<PvAmdSlabRoot> h(new PvAmdSlabRoot());
    h->r = SlabRoot::create(*s, device, &g_lastError);
    return h->r ? h.release() : nullptr;
} PV_API_CATCH(nullptr)
void PvAmdSlabRootDestroy(PvAmdSlabRoot* h) try {
    delete h;
} PV_API_CATCH_VOID
static int rootRet(PvAmdSlabRoot* h, bool ok) {
    if (!ok && h && h->r) g_lastError = h->r->lastError();
    return ok ? 0 : -1;
}
int PvAmdSlabRootBegin(PvAmdSlabRoot* h, float lx, float ly, float lz) try {
    return (h && h->r) ? rootRet(h, h->r->begin(lx, ly, lz)) : -1;
} PV_API_CATCH(-1)
int PvAmdSlabRootImportBlock(PvAmdSlabRoot* h, const int* info4, const float* host) try {
    return (h && h->r && info4 && (host || info4[2] * info4[3] == 0))
               ? rootRet(h, h->r->importBlock(info4[0], info4[1], info4[2], info4[3], host))
               : -1;
} PV_API_CATCH(-1)
int PvAmdSlabRootFinish(PvAmdSlabRoot* h) try { return (h && h->r) ? rootRet(h, h->r->finish()) : -1; } PV_API_CATCH(-1)
int PvAmdSlabRootGetOutput(PvAmdSlabRoot* h, float ex, float ey, float ez, PlaneverbOutput* out) try {
    if (!h || !h->r || !out) return -1;
    float v[8];
    bool valid = false;
    if (!h->r->getOutput(ex, ey, ez, v, &valid)) return rootRet(h, false);
    std::memset(out, 0, sizeof(*out));
    if (valid)
        std::memcpy(out, v, sizeof(*out));
    else
        out->occlusion = kInvalidDryGain;
    return 0;
} PV_API_CATCH(-1)
int PvAmdSlabRootCopyResults(PvAmdSlabRoot* h, float* res8, float* delay) try {
    return (h && h->r) ? rootRet(h, h->r->copyResults(res8, delay)) : -1;
} PV_API_CATCH(-1)

void PvAmdDestroy(PvAmdSolver* h) try {
    delete h;
} PV_API_CATCH_VOID

int PvAmdSetOption(PvAmdSolver* h, int key, long long value) try {
    if (!h) return -1;
    if (h->s || h->g) {
        g_lastError = "options must be set before the solver is first used";
        return -1;
    }
    switch (key) {
        case PVA_OPT_DENSE_HISTORY: h->opt.denseHistory = value != 0; break;
        case PVA_OPT_NUM_STEPS: h->opt.numSteps = (int)value; break;
        case PVA_OPT_SKIP_ANALYSIS: h->opt.skipAnalysis = value != 0; break;
        case PVA_OPT_USE_GRAPH: h->opt.useGraph = (int)value; break;
        case PVA_OPT_STEPS_PER_LAUNCH: h->opt.K = (int)value; break;
        case PVA_OPT_TILE_ROWS: h->opt.rxi = (int)value; break;
        case PVA_OPT_NO_FREE_GRID: h->opt.withFreeGrid = value == 0; break;
        case PVA_OPT_TIME_KERNELS: h->opt.timeKernels = (int)value; break;
        case PVA_OPT_TILE_ORDER: h->opt.tileOrder = (int)value; break;
        case PVA_OPT_SMALL_GRID_KERNEL: h->opt.smallGrid = (int)value; break;
        case PVA_OPT_PACKED_MATH: h->opt.packed = value != 0; break;
        case PVA_OPT_STREAMING_ANALYSIS: h->opt.streaming = value != 0; break;
        case PVA_OPT_STREAM_ROWS: h->opt.segments = (int)value; break;
        case PVA_OPT_MERGED_LAUNCH: h->opt.merged = (int)value; break;
        case PVA_OPT_EDGE_TILES: h->opt.edgeTiles = value != 0; break;
        case PVA_OPT_ROW_BANDS: h->opt.rowBands = (int)value; break;
        case PVA_OPT_PATCH_KERNEL: h->opt.patch = (int)value; break;
        case PVA_OPT_LAZY_FAR_CELLS: h->opt.lazyFar = value != 0; break;
        case PVA_OPT_STREAM_FUSE: h->opt.streamFuse = (int)value; break;
        case PVA_OPT_AUX_STREAMS: h->opt.auxStreams = (int)std::max<long long>(0, std::min<long long>(value, 8)); break;
        case PVA_OPT_PATCH_STRIP: h->opt.patchStrip = (int)value; break;
        case PVA_OPT_RESIDENT_KERNEL: h->opt.resident = (int)value; break;
        case PVA_OPT_RT60_LANES: h->opt.rt60Lanes = (int)value; break;
        case PVA_OPT_ANALYSIS_FORK: h->opt.analysisFork = (int)value; break;
        case PVA_OPT_FUSED_ANALYSIS: h->opt.fusedAnalysis = (int)value; break;
        case PVA_OPT_DEBUG_LOSE_FIRST_CAPTURE: h->opt.debugLoseFirstCapture = value != 0; break;
        case PVA_OPT_STREAM_PRIORITY: h->opt.streamPriority = (int)value; break;
        case PVA_OPT_ALTERNATE_SWEEPS: h->opt.alternateSweeps = (int)value; break;
        case PVA_OPT_XCD_REGIONS: h->opt.xcdRegions = (int)value; break;
        case PVA_OPT_REACH_BOUND: h->opt.reachBound = (int)value; break;
        case PVA_OPT_RESIDENT_WINDOW: h->opt.residentWindow = (int)value; break;
        default: g_lastError = "unknown option"; return -1;
    }
    return 0;
} PV_API_CATCH(-1)

int PvAmdGetInfo(PvAmdSolver* h, PvAmdInfo* out) try {
    if (!out || !ensure(h, true)) return -1;
    if (h->g) {
        const GridSpec& g = h->g->spec();
        const Solver* s0 = h->g->slab(0);
        std::memset(out, 0, sizeof(*out));
        out->gx = g.gx;
        out->gy = g.gy;
        out->T = h->g->T();
        out->fs = (int)g.fs;
        out->res = g.res;
        out->dx = g.dx;
        out->dt = g.dt;
        out->efree = h->g->efree();
        out->device = s0->device();
        out->stepsPerLaunch = s0->K();
        out->tileRows = s0->geometry().rxi;
        out->tileCols = s0->geometry().wi;
        out->pitch = s0->geometry().pitch;
        out->rows = s0->geometry().rows;
        out->histRows = s0->histRows();
        out->histPitch = s0->histPitch();
        out->numGeometry = h->g->numBoxes();
        out->deviceBytes = h->g->deviceBytes();
        return 0;
    }
    const GridSpec& g = h->s->spec();
    const Geometry& geo = h->s->geometry();
    std::memset(out, 0, sizeof(*out));
    out->gx = g.gx;
    out->gy = g.gy;
    out->T = h->s->T();
    out->fs = (int)g.fs;
    out->res = g.res;
    out->dx = g.dx;
    out->dt = g.dt;
    out->efree = h->s->efree();
    out->device = h->s->device();
    out->stepsPerLaunch = h->s->K();
    out->tileRows = geo.rxi;
    out->tileCols = geo.wi;
    out->pitch = geo.pitch;
    out->rows = geo.rows;
    out->histRows = h->s->histRows();
    out->histPitch = h->s->histPitch();
    out->numGeometry = h->s->numBoxes();
    out->deviceBytes = h->s->deviceBytes();
    out->streamFuse = h->s->streamFuse() ? 1 : 0;
    out->residentKernel = h->s->residentKernel() ? 1 : 0;
    return 0;
} PV_API_CATCH(-1)

int PvAmdAddGeometry(PvAmdSolver* h, float posX, float posY, float width, float height, float absorption) try {
    if (!ensure(h, true)) return -1;
    if (h->g) return h->g->addBox(Box{posX, posY, width, height, absorption});
    return h->s->addBox(Box{posX, posY, width, height, absorption});
} PV_API_CATCH(-1)

int PvAmdUpdateGeometry(PvAmdSolver* h, int id, float posX, float posY, float width, float height,
                        float absorption) try {
    if (!ensure(h, true)) return -1;
    if (h->g) return ret(h, h->g->updateBox(id, Box{posX, posY, width, height, absorption}));
    return ret(h, h->s->updateBox(id, Box{posX, posY, width, height, absorption}));
} PV_API_CATCH(-1)

int PvAmdRemoveGeometry(PvAmdSolver* h, int id) try {
    if (!ensure(h, true)) return -1;
    if (h->g) return ret(h, h->g->removeBox(id));
    return ret(h, h->s->removeBox(id));
} PV_API_CATCH(-1)

int PvAmdLoadScene(PvAmdSolver* h, const char* pvPath) try {
    if (!ensure(h, true) || !pvPath) return -1;
    std::vector<Box> boxes;
    if (!loadPv(pvPath, &boxes, &g_lastError)) return -1;
    for (const Box& b : boxes) {
        if (h->g)
            h->g->addBox(b);
        else
            h->s->addBox(b);
    }
    return (int)boxes.size();
} PV_API_CATCH(-1)

int PvAmdSaveScene(PvAmdSolver* h, const char* pvPath) try {
    if (!ensure(h) || !pvPath) return -1;
    return savePv(pvPath, h->s->boxes(), &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

// shapes (pv_core.h makeShape; Solver::addShape, SlabGroup::addShape).  A slab rank handle refuses them.
static bool shapesOk(PvAmdSolver* h) {
    if (h && h->opt.slabCount > 1) {
        g_lastError = "shapes are not available on a slab rank handle (PvAmdCreateSlabRank): use PvAmdCreateSlabs";
        return false;
    }
    return ensure(h, true);
}

static int addShape(PvAmdSolver* h, const Shape& sh) {
    const int id = h->g ? h->g->addShape(sh) : h->s->addShape(sh);
    if (id < 0) ret(h, false);
    return id;
}

int PvAmdAddShape(PvAmdSolver* h, const float* xy, int n, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !makeShape(xy, n, absorption, &sh, &g_lastError)) return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdateShape(PvAmdSolver* h, int id, const float* xy, int n, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !makeShape(xy, n, absorption, &sh, &g_lastError)) return -1;
    return ret(h, h->g ? h->g->updateShape(id, sh) : h->s->updateShape(id, sh));
} PV_API_CATCH(-1)

int PvAmdRemoveShape(PvAmdSolver* h, int id) try {
    if (!shapesOk(h)) return -1;
    return ret(h, h->g ? h->g->removeShape(id) : h->s->removeShape(id));
} PV_API_CATCH(-1)

int PvAmdAddOrientedBox(PvAmdSolver* h, float px, float py, float w, float hgt, float ax, float ay, float absorption) try {
    float v[8];
    Shape sh;
    if (!shapesOk(h) || !orientedBoxVertices(px, py, w, hgt, ax, ay, v, &g_lastError) || !makeShape(v, 4, absorption, &sh, &g_lastError))
        return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdateOrientedBox(PvAmdSolver* h, int id, float px, float py, float w, float hgt, float ax, float ay, float absorption) try {
    float v[8];
    Shape sh;
    if (!shapesOk(h) || !orientedBoxVertices(px, py, w, hgt, ax, ay, v, &g_lastError) || !makeShape(v, 4, absorption, &sh, &g_lastError))
        return -1;
    return ret(h, h->g ? h->g->updateShape(id, sh) : h->s->updateShape(id, sh));
} PV_API_CATCH(-1)

static int updateShape(PvAmdSolver* h, int id, const Shape& sh) {
    return ret(h, h->g ? h->g->updateShape(id, sh) : h->s->updateShape(id, sh));
}

int PvAmdAddDisc(PvAmdSolver* h, float cx, float cy, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !discShape(cx, cy, radius, absorption, &sh)) return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdateDisc(PvAmdSolver* h, int id, float cx, float cy, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !discShape(cx, cy, radius, absorption, &sh)) return -1;
    return updateShape(h, id, sh);
} PV_API_CATCH(-1)

int PvAmdAddCapsule(PvAmdSolver* h, float ax, float ay, float bx, float by, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !capsuleShape(ax, ay, bx, by, radius, absorption, &sh)) return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdateCapsule(PvAmdSolver* h, int id, float ax, float ay, float bx, float by, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !capsuleShape(ax, ay, bx, by, radius, absorption, &sh)) return -1;
    return updateShape(h, id, sh);
} PV_API_CATCH(-1)

int PvAmdAddWallPath(PvAmdSolver* h, const float* xy, int n, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !wallPathShape(xy, n, radius, absorption, &sh)) return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdateWallPath(PvAmdSolver* h, int id, const float* xy, int n, float radius, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !wallPathShape(xy, n, radius, absorption, &sh)) return -1;
    return updateShape(h, id, sh);
} PV_API_CATCH(-1)

int PvAmdAddPolygon(PvAmdSolver* h, const float* xy, int n, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !makePolygon(xy, n, absorption, &sh, &g_lastError)) return -1;
    return addShape(h, sh);
} PV_API_CATCH(-1)

int PvAmdUpdatePolygon(PvAmdSolver* h, int id, const float* xy, int n, float absorption) try {
    Shape sh;
    if (!shapesOk(h) || !makePolygon(xy, n, absorption, &sh, &g_lastError)) return -1;
    return updateShape(h, id, sh);
} PV_API_CATCH(-1)

// triangle meshes (pv_core.h validateMesh; Solver::addMesh).  One solver only: slab groups and slab ranks refuse them.
static bool meshesOk(PvAmdSolver* h) {
    if (h && (h->opt.slabCount > 1 || !h->slabDevices.empty())) {
        g_lastError = "meshes are not available on slabs (PvAmdCreateSlabs, PvAmdCreateSlabRank)";
        return false;
    }
    return ensure(h);
}

int PvAmdAddMesh(PvAmdSolver* h, const float* verts, int nv, const int* tris, int nt, float absorption, int mode, float radius) try {
    if (!meshesOk(h) || !validateMesh(verts, nv, tris, nt, absorption, mode, radius, &g_lastError)) return -1;
    const int id = h->s->addMesh(verts, nv, tris, nt, absorption, mode, radius);
    if (id < 0) ret(h, false);
    return id;
} PV_API_CATCH(-1)

int PvAmdUpdateMesh(PvAmdSolver* h, int id, const float* verts, int nv, const int* tris, int nt, float absorption, int mode,
                    float radius) try {
    if (!meshesOk(h) || !validateMesh(verts, nv, tris, nt, absorption, mode, radius, &g_lastError)) return -1;
    return ret(h, h->s->updateMesh(id, verts, nv, tris, nt, absorption, mode, radius));
} PV_API_CATCH(-1)

int PvAmdSetMeshTransform(PvAmdSolver* h, int id, const float* m12) try {
    if (!meshesOk(h) || !validateMeshTransform(m12, &g_lastError)) return -1;
    return ret(h, h->s->setMeshTransform(id, m12));
} PV_API_CATCH(-1)

int PvAmdRemoveMesh(PvAmdSolver* h, int id) try {
    if (!meshesOk(h)) return -1;
    return ret(h, h->s->removeMesh(id));
} PV_API_CATCH(-1)

int PvAmdSetSliceHeight(PvAmdSolver* h, float height) try {
    if (!(height - height == 0.f)) {
        g_lastError = "PvAmdSetSliceHeight: the height is not finite";
        return -1;
    }
    if (!meshesOk(h)) return -1;
    return ret(h, h->s->setSliceHeight(height));
} PV_API_CATCH(-1)

float PvAmdGetSliceHeight(PvAmdSolver* h) try { return meshesOk(h) ? h->s->sliceHeight() : 0.f; } PV_API_CATCH(0.f)

int PvAmdMeshTriangles(PvAmdSolver* h, int id) try { return meshesOk(h) ? h->s->meshTriangles(id) : -1; } PV_API_CATCH(-1)

int PvAmdCopyMeshSection(PvAmdSolver* h, int id, float* out4nt, uint8_t* valid_nt) try {
    if (!meshesOk(h)) return -1;
    return ret(h, h->s->copyMeshSection(id, out4nt, valid_nt));
} PV_API_CATCH(-1)

int PvAmdSetGridBoundary(PvAmdSolver* h, const float* absorption4) try {
    if (!absorption4) {
        g_lastError = "PvAmdSetGridBoundary: null absorption array";
        return -1;
    }
    for (int k = 0; k < 4; ++k)
        if (!(absorption4[k] - absorption4[k] == 0.f)) {
            g_lastError = "PvAmdSetGridBoundary: absorption of side " + std::to_string(k) + " is not finite";
            return -1;
        }
    if (h && h->opt.slabCount > 1) {  // a rank would need its neighbours' edges in the halo exchange: out of scope
        for (int k = 0; k < 4; ++k)
            if (absorption4[k] != 0.f) {
                g_lastError = "a slab rank handle (PvAmdCreateSlabRank) has absorbing grid edges only: use PvAmdCreateSlabs";
                return -1;
            }
    }
    if (!ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->setGridBoundary(absorption4) : h->s->setGridBoundary(absorption4));
} PV_API_CATCH(-1)

// PvAmdSetEdgeLayer (split = false) and PvAmdSetEdgeLayerSplit: the same refusals, plus r0 for the split model
static int setEdgeLayerModel(PvAmdSolver* h, const int* width4, bool split, double r0, const char* name) {
    if (!width4) {
        g_lastError = std::string(name) + ": null width array";
        return -1;
    }
    if (split && !edgeLayerR0Ok(r0)) {
        g_lastError = std::string(name) + ": r0 must lie strictly between 0 and 1";
        return -1;
    }
    const bool any = width4[0] != 0 || width4[1] != 0 || width4[2] != 0 || width4[3] != 0;
    if (h && any && (h->opt.slabCount > 1 || !h->slabDevices.empty())) {
        g_lastError = std::string(name) + ": edge layers are not available on slab groups or slab ranks";
        return -1;
    }
    if (h && !h->slabDevices.empty()) return 0;  // (all widths 0 on a slab group: nothing to change)
    if (!ensure(h)) return -1;
    return ret(h, h->s->setEdgeLayer(width4, split, split ? r0 : kEdgeLayerR0));
}

int PvAmdSetEdgeLayer(PvAmdSolver* h, const int* width4) try {
    return setEdgeLayerModel(h, width4, false, kEdgeLayerR0, "PvAmdSetEdgeLayer");
} PV_API_CATCH(-1)

int PvAmdSetEdgeLayerSplit(PvAmdSolver* h, const int* width4, double r0) try {
    return setEdgeLayerModel(h, width4, true, r0, "PvAmdSetEdgeLayerSplit");
} PV_API_CATCH(-1)

int PvAmdGetEdgeLayerModel(PvAmdSolver* h, int* split, double* r0) try {
    if (!split || !r0) {
        g_lastError = "PvAmdGetEdgeLayerModel: null output";
        return -1;
    }
    if (h && !h->slabDevices.empty()) {  // (slab groups hold no layer)
        *split = 0;
        *r0 = kEdgeLayerR0;
        return 0;
    }
    if (!ensure(h)) return -1;
    bool sp;
    h->s->edgeLayerModel(&sp, r0);
    *split = sp ? 1 : 0;
    return 0;
} PV_API_CATCH(-1)

int PvAmdGetEdgeLayer(PvAmdSolver* h, int* out4) try {
    if (!out4) {
        g_lastError = "PvAmdGetEdgeLayer: null output array";
        return -1;
    }
    if (h && !h->slabDevices.empty()) {
        for (int k = 0; k < 4; ++k) out4[k] = 0;
        return 0;
    }
    if (!ensure(h)) return -1;
    h->s->edgeLayer(out4);
    return 0;
} PV_API_CATCH(-1)

int PvAmdGetGridBoundary(PvAmdSolver* h, float* out4) try {
    if (!out4) {
        g_lastError = "PvAmdGetGridBoundary: null output array";
        return -1;
    }
    if (!ensure(h, true)) return -1;
    if (h->g)
        h->g->gridBoundary(out4);
    else
        h->s->gridBoundary(out4);
    return 0;
} PV_API_CATCH(-1)

int PvAmdRun(PvAmdSolver* h, float lx, float ly, float lz) try {
    if (!wholeGrid(h) || !ensure(h, true)) return -1;
    if (h->g) return ret(h, h->g->run(lx, ly, lz));
    return ret(h, h->s->run(lx, ly, lz, true));
} PV_API_CATCH(-1)

int PvAmdRunAsync(PvAmdSolver* h, float lx, float ly, float lz) try {
    if (!wholeGrid(h) || !ensure(h)) return -1;
    return ret(h, h->s->run(lx, ly, lz, false));
} PV_API_CATCH(-1)

int PvAmdRunAsyncAfter(PvAmdSolver* h, PvAmdSolver* prev, float lx, float ly, float lz) try {
    if (!wholeGrid(h) || !ensure(h) || !prev || !wholeGrid(prev) || !ensure(prev)) return -1;
    if (prev->s->spec().gx != h->s->spec().gx || prev->s->spec().gy != h->s->spec().gy || prev->s->device() != h->s->device()) {
        g_lastError = "PvAmdRunAsyncAfter: the two solvers must have the same grid and device";
        return -1;
    }
    return ret(h, h->s->run(lx, ly, lz, false, prev->s));
} PV_API_CATCH(-1)

int PvAmdRunBatch(PvAmdSolver* const* hs, int n, const float* listenersXYZ, int wait) try {
    if (!hs || !listenersXYZ || n < 1 || n > kBatchMax) {
        g_lastError = "PvAmdRunBatch: 1..8 solvers and their listener positions";
        return -1;
    }
    Solver* s[kBatchMax];
    for (int i = 0; i < n; ++i) {
        if (!wholeGrid(hs[i]) || !ensure(hs[i])) return -1;
        s[i] = hs[i]->s;
    }
    std::string err;
    if (Solver::runBatch(s, n, listenersXYZ, wait != 0, &err)) return 0;
    g_lastError = err.empty() ? "batched run failed" : err;
    return -1;
} PV_API_CATCH(-1)

int PvAmdSync(PvAmdSolver* h) try {
    if (!wholeGrid(h) || !ensure(h)) return -1;
    return ret(h, h->s->sync());
} PV_API_CATCH(-1)

float PvAmdClockProbe(int device, float* byMemtimeMHz) try {
    return clockProbeMHz(device, byMemtimeMHz);
} PV_API_CATCH(0.f)

int PvAmdBandwidthProbe(int device, float* gbPerS4) try {
    if (!gbPerS4) return -1;
    if (bandwidthProbeGBs(device, gbPerS4)) return 0;
    g_lastError = "PvAmdBandwidthProbe: allocation or launch failed (2 GiB of device memory are needed)";
    return -1;
} PV_API_CATCH(-1)

int PvAmdLibmProbe(int form, const float* in, float* out, long long n, int onDevice) try {
    return libmProbe(form, in, out, n, onDevice != 0, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdGetTimings(PvAmdSolver* h, PvAmdTimings* out) try {
    if (!out || !ensure(h, true)) return -1;
    const SolverTimings& t = h->g ? h->g->timings() : h->s->timings();
    out->fdtdMs = t.fdtdMs;
    out->analysisMs = t.analysisMs;
    out->geometryMs = t.geometryMs;
    out->stepLaunches = t.stepLaunches;
    out->stepKernelMs = t.stepLaunches ? t.fdtdMs / (float)t.stepLaunches : 0.f;
    out->airKernelMs = t.airKernelMs;
    out->generalKernelMs = t.generalKernelMs;
    out->airLaunches = t.airLaunches;
    out->generalLaunches = t.generalLaunches;
    out->stepLoopMs = t.stepLoopMs;
    out->reachedCells = t.reachedCells;
    out->activeCells = t.activeCells;
    out->silentCells = t.silentCells;
    return 0;
} PV_API_CATCH(-1)

int PvAmdLastRunResidentWindow(PvAmdSolver* h) try {
    if (!wholeGrid(h) || !ensure(h, true)) return -1;
    return h->s->lastRunResidentWindow() ? 1 : 0;
} PV_API_CATCH(-1)

int PvAmdLastRunOneXcd(PvAmdSolver* h) try {
    if (!wholeGrid(h) || !ensure(h, true)) return -1;
    return h->s->lastRunOneXcd() ? 1 : 0;
} PV_API_CATCH(-1)

int PvAmdSetEmitters(PvAmdSolver* h, const float* xyz, int n) try {
    if (!wholeGrid(h) || !ensure(h) || (n > 0 && !xyz)) return -1;
    return ret(h, h->s->setEmitters(xyz, n));
} PV_API_CATCH(-1)

int PvAmdGetOutput(PvAmdSolver* h, float ex, float ey, float ez, PlaneverbOutput* out) try {
    if (!wholeGrid(h) || !out || !ensure(h, true)) return -1;
    float v[8];
    bool valid = false;
    if (!(h->g ? h->g->getOutput(ex, ey, ez, v, &valid) : h->s->getOutput(ex, ey, ez, v, &valid))) return ret(h, false);
    if (!valid) {
        std::memset(out, 0, sizeof(*out));
        out->occlusion = kInvalidDryGain;
        return 0;
    }
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdSetOutputQueries(PvAmdSolver* h, const float* xyz, int n) try {
    if (!wholeGrid(h) || (n > 0 && !xyz) || !ensure(h)) return -1;
    return ret(h, h->s->setOutputQueries(xyz, n));
} PV_API_CATCH(-1)

int PvAmdGetQueriedOutputs(PvAmdSolver* h, PlaneverbOutput* out, int n) try {
    if (n < 0 || n > Solver::kMaxQueries || (n > 0 && !out) || !wholeGrid(h) || !ensure(h)) return -1;
    float v[Solver::kMaxQueries * 8];
    unsigned char valid[Solver::kMaxQueries];
    if (!h->s->queriedOutputs(v, valid, n)) return ret(h, false);
    for (int i = 0; i < n; ++i) {
        if (valid[i]) {
            std::memcpy(&out[i], v + 8 * i, sizeof(PlaneverbOutput));
        } else {  // the reference's sentinel for a position outside the grid (FDTD.cpp:19-47)
            std::memset(&out[i], 0, sizeof(PlaneverbOutput));
            out[i].occlusion = kInvalidDryGain;
        }
    }
    return 0;
} PV_API_CATCH(-1)

// In-run records of the registered queries, two families (pv_solver_records.cpp): single whole-grid solvers only.  `pre` is what
// every refusal of a family's calls starts with, the member what serves the call for that family
static bool analysisHandle(PvAmdSolver* h, const char* pre);
static bool analysisCall(PvAmdSolver* h, const char* pre, const char* fn, const void* out);
static const char kQrecPre[] = "query records: ", kQspecPre[] = "spectral records: ";
static_assert(PVA_QSPEC_BAND_METRICS == 1u << kQspecBandMetrics && PVA_QSPEC_MODULATION == 1u << kQspecModulation &&
                  PVA_QSPEC_SPECTRUM == 1u << kQspecSpectrum,
              "planeverb_amd.h vs pv_query_spectral.h");

static int recordsSelect(PvAmdSolver* h, const char* pre, bool (Solver::*select)(unsigned), unsigned kinds) {
    if (!analysisHandle(h, pre)) return -1;
    return ret(h, (h->s->*select)(kinds));
}

static unsigned recordsKinds(PvAmdSolver* h, const char* pre, unsigned (Solver::*kinds)() const) {
    if (!analysisHandle(h, pre)) return 0u;
    return (h->s->*kinds)();
}

static int recordsFloats(PvAmdSolver* h, const char* pre, int (Solver::*floats)(unsigned), unsigned kind) {
    if (!analysisHandle(h, pre)) return -1;
    const int n = (h->s->*floats)(kind);
    if (n < 0) ret(h, false);
    return n;
}

static int recordsRead(PvAmdSolver* h, const char* pre, const char* fn, bool (Solver::*read)(unsigned, float*, int), unsigned kind,
                       float* out, int nQueries) {
    if (!analysisHandle(h, pre)) return -1;
    if (nQueries < 0 || nQueries > kMaxRecordQueries || (nQueries > 0 && !out)) {
        g_lastError = std::string(pre) + fn + ": 0 .. 1024 queries and an output buffer";
        return -1;
    }
    return ret(h, (h->s->*read)(kind, out, nQueries));
}

int PvAmdSetQueryRecords(PvAmdSolver* h, unsigned kinds) try {
    return recordsSelect(h, kQrecPre, &Solver::setQueryRecords, kinds);
} PV_API_CATCH(-1)

unsigned PvAmdGetQueryRecordKinds(PvAmdSolver* h) try {
    return recordsKinds(h, kQrecPre, &Solver::queryRecordKinds);
} PV_API_CATCH(0u)

int PvAmdQueryRecordFloats(PvAmdSolver* h, unsigned kind) try {
    return recordsFloats(h, kQrecPre, &Solver::queryRecordFloats, kind);
} PV_API_CATCH(-1)

int PvAmdGetQueriedRecords(PvAmdSolver* h, unsigned kind, float* out, int nQueries) try {
    return recordsRead(h, kQrecPre, __func__, &Solver::queriedRecords, kind, out, nQueries);
} PV_API_CATCH(-1)

int PvAmdSetRecordQueries(PvAmdSolver* h, const float* xyz, int n) try {
    if (!analysisHandle(h, kQrecPre)) return -1;
    if (n < 0 || n > kMaxRecordQueries || (n > 0 && !xyz)) {
        g_lastError = "query records: PvAmdSetRecordQueries: 0 .. 1024 positions (NULL only with 0)";
        return -1;
    }
    return ret(h, h->s->setRecordQueries(xyz, n));
} PV_API_CATCH(-1)

int PvAmdSetQuerySpectralRecords(PvAmdSolver* h, unsigned kinds) try {
    return recordsSelect(h, kQspecPre, &Solver::setQuerySpectralRecords, kinds);
} PV_API_CATCH(-1)

unsigned PvAmdGetQuerySpectralKinds(PvAmdSolver* h) try {
    return recordsKinds(h, kQspecPre, &Solver::querySpectralKinds);
} PV_API_CATCH(0u)

int PvAmdQuerySpectralFloats(PvAmdSolver* h, unsigned kind) try {
    return recordsFloats(h, kQspecPre, &Solver::querySpectralFloats, kind);
} PV_API_CATCH(-1)

int PvAmdGetQueriedSpectralRecords(PvAmdSolver* h, unsigned kind, float* out, int nQueries) try {
    return recordsRead(h, kQspecPre, __func__, &Solver::queriedSpectralRecords, kind, out, nQueries);
} PV_API_CATCH(-1)

// Emitter records of sparse-emitter mode: the same two families with the registered emitters as the cell source
static const char kEmitterPre[] = "emitter records: ";
static bool emitterFamily(int family, Solver::RecordFamily* f) {
    if (family == 0 || family == 1) {
        *f = family ? Solver::kRecSpectral : Solver::kRecTime;
        return true;
    }
    g_lastError = std::string(kEmitterPre) + "family: 0 (PVA_QREC_*) or 1 (PVA_QSPEC_*)";
    return false;
}

int PvAmdSetEmitterRecords(PvAmdSolver* h, unsigned timeKinds, unsigned spectralKinds) try {
    if (!analysisHandle(h, kEmitterPre)) return -1;
    return ret(h, h->s->setEmitterRecords(timeKinds, spectralKinds));
} PV_API_CATCH(-1)

int PvAmdGetEmitterRecordKinds(PvAmdSolver* h, unsigned* timeKinds, unsigned* spectralKinds) try {
    if (!analysisHandle(h, kEmitterPre)) return -1;
    if (timeKinds) *timeKinds = h->s->emitterRecordKinds(Solver::kRecTime);
    if (spectralKinds) *spectralKinds = h->s->emitterRecordKinds(Solver::kRecSpectral);
    return 0;
} PV_API_CATCH(-1)

int PvAmdEmitterRecordFloats(PvAmdSolver* h, int family, unsigned kind) try {
    Solver::RecordFamily f;
    if (!analysisHandle(h, kEmitterPre) || !emitterFamily(family, &f)) return -1;
    const int n = h->s->emitterRecordFloats(f, kind);
    if (n < 0) ret(h, false);
    return n;
} PV_API_CATCH(-1)

int PvAmdGetEmitterRecords(PvAmdSolver* h, int family, unsigned kind, float* out, int nEmitters) try {
    Solver::RecordFamily f;
    if (!analysisHandle(h, kEmitterPre) || !emitterFamily(family, &f)) return -1;
    if (nEmitters < 0 || nEmitters > kMaxRecordQueries || (nEmitters > 0 && !out)) {
        g_lastError = std::string(kEmitterPre) + __func__ + ": 0 .. 1024 emitters and an output buffer";
        return -1;
    }
    return ret(h, h->s->emitterRecords(f, kind, out, nEmitters));
} PV_API_CATCH(-1)

int PvAmdGetEmitterCells(PvAmdSolver* h, int* cxcy, int cap) try {
    if (!analysisHandle(h, "emitter cells: ")) return -1;
    if (cap < 0 || (cap > 0 && !cxcy)) {
        g_lastError = std::string("emitter cells: ") + __func__ + ": a capacity of 0 or more, and a buffer with it";
        return -1;
    }
    return h->s->emitterCells(cxcy, cap);
} PV_API_CATCH(-1)

int PvAmdCopyEmitterTrace(PvAmdSolver* h, int emitter, float* outT) try {
    if (!analysisCall(h, "emitter trace: ", __func__, outT)) return -1;
    return ret(h, h->s->copyEmitterTrace(emitter, outT));
} PV_API_CATCH(-1)

int PvAmdCopyResults(PvAmdSolver* h, float* res8, float* delay) try {
    if (!wholeGrid(h) || !ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->copyResults(res8, delay) : h->s->copyResults(res8, delay));
} PV_API_CATCH(-1)

int PvAmdCopyResultsBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* res8, float* delay) try {
    if (!wholeGrid(h) || !ensure(h)) return -1;
    return ret(h, h->s->copyResultsBlock(r0, c0, nr, nc, res8, delay));
} PV_API_CATCH(-1)

int PvAmdGetImpulseResponse(PvAmdSolver* h, int cx, int cy, float* out3T) try {
    if (!out3T || !ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->impulseResponse(cx, cy, out3T) : h->s->impulseResponse(cx, cy, out3T));
} PV_API_CATCH(-1)

int PvAmdGetImpulseResponseCells(PvAmdSolver* h, int cx, int cy, PlaneverbCell* outT) try {
    if (!outT || !ensure(h)) return -1;
    static_assert(sizeof(PlaneverbCell) == 16, "PvTypes.h:106-121");
    return ret(h, h->s->impulseResponseCells(cx, cy, outT));
} PV_API_CATCH(-1)

int PvAmdCopyFields(PvAmdSolver* h, float* pr, float* vx, float* vy) try {
    if (!ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->copyFields(pr, vx, vy) : h->s->copyFields(pr, vx, vy));
} PV_API_CATCH(-1)

int PvAmdCopyHistoryPlane(PvAmdSolver* h, int t, float* pr) try {
    if (!pr || !ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->copyHistoryPlane(t, pr) : h->s->copyHistoryPlane(t, pr));
} PV_API_CATCH(-1)

// The nine per-cell analysis kinds (pv_solver_maps.cpp): single whole-grid solvers only -- slab groups (ensure) and slab ranks
// (wholeGrid) are refused.  `pre` is what every refusal of a kind's calls starts with ("decay times: "; none for the room
// metrics and the spectrum); `fn` names the call in a null-output refusal.  Settings are checked against the handle's own grid
// before anything else happens (the rules the PvAmdHost* calls apply too).  World y is ignored, as everywhere.
static bool analysisHandle(PvAmdSolver* h, const char* pre) {
    if (wholeGrid(h) && ensure(h)) return true;
    g_lastError = pre + g_lastError;
    return false;
}

static bool analysisCall(PvAmdSolver* h, const char* pre, const char* fn, const void* out) {
    if (!analysisHandle(h, pre)) return false;
    if (!out) g_lastError = std::string(pre) + fn + ": null output";
    return out != nullptr;
}

// the inverse of PvAmdCopyHistoryPlane, with the analysis passes' refusals (what it feeds)
int PvAmdSetHistoryPlane(PvAmdSolver* h, int t, const float* pr) try {
    if (!analysisCall(h, "set history plane: ", __func__, pr)) return -1;
    return ret(h, h->s->setHistoryPlane(t, pr));
} PV_API_CATCH(-1)

static int analysisCopy(PvAmdSolver* h, AnalysisKind k, const char* pre, const char* fn, float* out) {
    if (!analysisCall(h, pre, fn, out)) return -1;
    return ret(h, h->s->copyAnalysisBlock(k, 0, 0, h->s->spec().gx, h->s->spec().gy, out));
}

static int analysisCopyBlock(PvAmdSolver* h, AnalysisKind k, const char* pre, const char* fn, int r0, int c0, int nr, int nc, float* out) {
    if (!analysisCall(h, pre, fn, out)) return -1;
    return ret(h, h->s->copyAnalysisBlock(k, r0, c0, nr, nc, out));
}

static int analysisGet(PvAmdSolver* h, AnalysisKind k, const char* pre, const char* fn, float ex, float ez, void* out) {
    if (!analysisCall(h, pre, fn, out)) return -1;
    return ret(h, h->s->analysisAt(k, ex, ez, static_cast<float*>(out)));  // (*out is written only where the call succeeds)
}

static_assert(sizeof(PvAmdRoomMetrics) == kRoomMetricFloats * sizeof(float), "ten floats");
static_assert(sizeof(PvAmdDecayTimes) == kDecayFloats * sizeof(float), "eight floats");
static_assert(sizeof(PvAmdLateralFraction) == kLateralFloats * sizeof(float), "eleven floats");
static_assert(sizeof(PvAmdEchoCriterion) == kEchoFloats * sizeof(float), "ten floats");
static_assert(sizeof(PvAmdBandMetrics) == kBandFloats * sizeof(float), "twelve floats");
static_assert(sizeof(PvAmdModulation) == kModFloats * sizeof(float), "fifteen floats");

// room metrics (pv_metrics.hip)
int PvAmdComputeRoomMetrics(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "")) return -1;
    return ret(h, h->s->computeRoomMetrics(ms));
} PV_API_CATCH(-1)

int PvAmdCopyRoomMetrics(PvAmdSolver* h, float* out10) try {
    return analysisCopy(h, kMapRoomMetrics, "", __func__, out10);
} PV_API_CATCH(-1)

int PvAmdCopyRoomMetricsBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out10) try {
    return analysisCopyBlock(h, kMapRoomMetrics, "", __func__, r0, c0, nr, nc, out10);
} PV_API_CATCH(-1)

int PvAmdGetRoomMetrics(PvAmdSolver* h, float ex, float ey, float ez, PvAmdRoomMetrics* out) try {
    return analysisGet(h, kMapRoomMetrics, "", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// decay times (pv_decay.hip)
int PvAmdComputeDecayTimes(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "decay times: ")) return -1;
    return ret(h, h->s->computeDecayTimes(ms));
} PV_API_CATCH(-1)

int PvAmdCopyDecayTimes(PvAmdSolver* h, float* out8) try {
    return analysisCopy(h, kMapDecayTimes, "decay times: ", __func__, out8);
} PV_API_CATCH(-1)

int PvAmdCopyDecayTimesBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out8) try {
    return analysisCopyBlock(h, kMapDecayTimes, "decay times: ", __func__, r0, c0, nr, nc, out8);
} PV_API_CATCH(-1)

int PvAmdGetDecayTimes(PvAmdSolver* h, float ex, float ey, float ez, PvAmdDecayTimes* out) try {
    return analysisGet(h, kMapDecayTimes, "decay times: ", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// lateral fraction (pv_lateral.hip)
int PvAmdComputeLateralFraction(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "lateral fraction: ")) return -1;
    return ret(h, h->s->computeLateralFraction(ms));
} PV_API_CATCH(-1)

int PvAmdCopyLateralFraction(PvAmdSolver* h, float* out11) try {
    return analysisCopy(h, kMapLateralFraction, "lateral fraction: ", __func__, out11);
} PV_API_CATCH(-1)

int PvAmdCopyLateralFractionBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out11) try {
    return analysisCopyBlock(h, kMapLateralFraction, "lateral fraction: ", __func__, r0, c0, nr, nc, out11);
} PV_API_CATCH(-1)

int PvAmdGetLateralFraction(PvAmdSolver* h, float ex, float ey, float ez, PvAmdLateralFraction* out) try {
    return analysisGet(h, kMapLateralFraction, "lateral fraction: ", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// echo criterion (pv_echo.hip)
int PvAmdComputeEchoCriterion(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "echo: ")) return -1;
    return ret(h, h->s->computeEchoCriterion(ms));
} PV_API_CATCH(-1)

int PvAmdCopyEchoCriterion(PvAmdSolver* h, float* out10) try {
    return analysisCopy(h, kMapEchoCriterion, "echo: ", __func__, out10);
} PV_API_CATCH(-1)

int PvAmdCopyEchoCriterionBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out10) try {
    return analysisCopyBlock(h, kMapEchoCriterion, "echo: ", __func__, r0, c0, nr, nc, out10);
} PV_API_CATCH(-1)

int PvAmdGetEchoCriterion(PvAmdSolver* h, float ex, float ey, float ez, PvAmdEchoCriterion* out) try {
    return analysisGet(h, kMapEchoCriterion, "echo: ", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// echogram (pv_echogram.hip; the setting: pv_echogram.h echogramSlotOk)
static const char* echogramSettingError(float slotSeconds, int nSlots, int fs) {
    if (nSlots < 0 || nSlots > kEchogramMaxSlots) return "echogram: nSlots is 0 .. PVA_ECHOGRAM_MAX_SLOTS (32)";
    if (nSlots > 0 && !echogramSlotOk(slotSeconds, fs))
        return "echogram: slotSeconds must be finite and give 1 .. 2^20 steps per slot ((int)(slotSeconds * (float)fs))";
    return nullptr;
}

int PvAmdSetEchogram(PvAmdSolver* h, float slotSeconds, int nSlots) try {
    if (!h) {
        g_lastError = "echogram: null solver handle";
        return -1;
    }
    if (const char* e = echogramSettingError(slotSeconds, nSlots, (int)h->spec.fs)) {
        g_lastError = e;
        return -1;
    }
    if (!analysisHandle(h, "echogram: ")) return -1;
    return ret(h, h->s->setEchogram(slotSeconds, nSlots));
} PV_API_CATCH(-1)

int PvAmdGetEchogramSlots(PvAmdSolver* h, float* slotSeconds, int* slotSteps) try {
    if (!analysisHandle(h, "echogram: ")) return -1;
    return h->s->echogramSlots(slotSeconds, slotSteps);
} PV_API_CATCH(-1)

int PvAmdComputeEchogram(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "echogram: ")) return -1;
    return ret(h, h->s->computeEchogram(ms));
} PV_API_CATCH(-1)

int PvAmdCopyEchogram(PvAmdSolver* h, float* out) try {
    return analysisCopy(h, kMapEchogram, "echogram: ", __func__, out);
} PV_API_CATCH(-1)

int PvAmdCopyEchogramBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out) try {
    return analysisCopyBlock(h, kMapEchogram, "echogram: ", __func__, r0, c0, nr, nc, out);
} PV_API_CATCH(-1)

int PvAmdGetEchogram(PvAmdSolver* h, float ex, float ey, float ez, float* out) try {
    return analysisGet(h, kMapEchogram, "echogram: ", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// lobes (pv_lobes.hip; the setting: pv_lobes.h lobesEdgeSteps)
int PvAmdSetLobeWindows(PvAmdSolver* h, const float* edgesSeconds, int nEdges) try {
    if (!h) {
        g_lastError = "lobes: null solver handle";
        return -1;
    }
    LobeEdges ed;
    if (nEdges != 0 && !lobesEdgeSteps(edgesSeconds, nEdges, (int)h->spec.fs, &ed)) {
        g_lastError = kLobesEdgesError;
        return -1;
    }
    if (!analysisHandle(h, "lobes: ")) return -1;
    return ret(h, h->s->setLobeWindows(edgesSeconds, nEdges));
} PV_API_CATCH(-1)

int PvAmdGetLobeWindows(PvAmdSolver* h, float* edgesSeconds, int* edgeSteps) try {
    if (!analysisHandle(h, "lobes: ")) return -1;
    return h->s->lobeWindows(edgesSeconds, edgeSteps);
} PV_API_CATCH(-1)

int PvAmdComputeLobes(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "lobes: ")) return -1;
    return ret(h, h->s->computeLobes(ms));
} PV_API_CATCH(-1)

int PvAmdCopyLobes(PvAmdSolver* h, float* out) try {
    return analysisCopy(h, kMapLobes, "lobes: ", __func__, out);
} PV_API_CATCH(-1)

int PvAmdCopyLobesBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out) try {
    return analysisCopyBlock(h, kMapLobes, "lobes: ", __func__, r0, c0, nr, nc, out);
} PV_API_CATCH(-1)

int PvAmdGetLobes(PvAmdSolver* h, float ex, float ey, float ez, float* out) try {
    return analysisGet(h, kMapLobes, "lobes: ", __func__, ex, ez, out);
} PV_API_CATCH(-1)

// band metrics (pv_bands.hip; the setting: pv_bands.h bandsError)
int PvAmdSetBands(PvAmdSolver* h, const float* centreHz, int n, int fraction) try {
    if (!h) {
        g_lastError = "band metrics: null solver handle";
        return -1;
    }
    if (n != 0) {
        if (const char* e = bandsError(centreHz, n, fraction, (int)h->spec.fs)) {
            g_lastError = e;
            return -1;
        }
    } else if (fraction != 1 && fraction != 3) {
        g_lastError = "band metrics: fraction is 1 (octave) or 3 (third octave)";
        return -1;
    }
    if (!analysisHandle(h, "band metrics: ")) return -1;
    return ret(h, h->s->setBands(centreHz, n, fraction));
} PV_API_CATCH(-1)

int PvAmdGetBands(PvAmdSolver* h, float* centreHz, int cap, int* fraction) try {
    if (!analysisHandle(h, "band metrics: ")) return -1;
    return h->s->bands(centreHz, cap, fraction);
} PV_API_CATCH(-1)

int PvAmdGetBandCoefs(PvAmdSolver* h, float* out10n) try {
    if (!analysisCall(h, "band metrics: ", __func__, out10n)) return -1;
    return ret(h, h->s->bandCoefs(out10n));
} PV_API_CATCH(-1)

int PvAmdComputeBandMetrics(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "band metrics: ")) return -1;
    return ret(h, h->s->computeBandMetrics(ms));
} PV_API_CATCH(-1)

int PvAmdCopyBandMetrics(PvAmdSolver* h, float* out12n) try {
    return analysisCopy(h, kMapBandMetrics, "band metrics: ", __func__, out12n);
} PV_API_CATCH(-1)

int PvAmdCopyBandMetricsBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out12n) try {
    return analysisCopyBlock(h, kMapBandMetrics, "band metrics: ", __func__, r0, c0, nr, nc, out12n);
} PV_API_CATCH(-1)

int PvAmdGetBandMetrics(PvAmdSolver* h, float ex, float ey, float ez, PvAmdBandMetrics* out12n) try {
    return analysisGet(h, kMapBandMetrics, "band metrics: ", __func__, ex, ez, out12n);
} PV_API_CATCH(-1)

// modulation (pv_modulation.hip; the setting: pv_modulation.h modulationFreqsError)
int PvAmdSetModulationFrequencies(PvAmdSolver* h, const float* hz14) try {
    if (!h) {
        g_lastError = "modulation: null solver handle";
        return -1;
    }
    if (hz14) {
        if (const char* e = modulationFreqsError(hz14, (int)h->spec.fs)) {
            g_lastError = e;
            return -1;
        }
    }
    if (!analysisHandle(h, "modulation: ")) return -1;
    return ret(h, h->s->setModulationFrequencies(hz14));
} PV_API_CATCH(-1)

int PvAmdGetModulationFrequencies(PvAmdSolver* h, float* hz14) try {
    if (!analysisCall(h, "modulation: ", __func__, hz14)) return -1;
    h->s->modulationFrequencies(hz14);
    return 0;
} PV_API_CATCH(-1)

int PvAmdComputeModulation(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "modulation: ")) return -1;
    return ret(h, h->s->computeModulation(ms));
} PV_API_CATCH(-1)

int PvAmdCopyModulation(PvAmdSolver* h, float* out15n) try {
    return analysisCopy(h, kMapModulation, "modulation: ", __func__, out15n);
} PV_API_CATCH(-1)

int PvAmdCopyModulationBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out15n) try {
    return analysisCopyBlock(h, kMapModulation, "modulation: ", __func__, r0, c0, nr, nc, out15n);
} PV_API_CATCH(-1)

int PvAmdGetModulation(PvAmdSolver* h, float ex, float ey, float ez, PvAmdModulation* out15n) try {
    return analysisGet(h, kMapModulation, "modulation: ", __func__, ex, ez, out15n);
} PV_API_CATCH(-1)

// spectrum (pv_spectrum.hip; the setting: pv_spectrum.h spectrumBinsError)
int PvAmdSetSpectrumBins(PvAmdSolver* h, const float* hz, int n) try {
    if (!h) {
        g_lastError = "null solver handle";
        return -1;
    }
    if (n != 0) {
        if (const char* e = spectrumBinsError(hz, n, (int)h->spec.fs)) {
            g_lastError = e;
            return -1;
        }
    }
    if (!analysisHandle(h, "")) return -1;
    return ret(h, h->s->setSpectrumBins(hz, n));
} PV_API_CATCH(-1)

int PvAmdGetSpectrumBins(PvAmdSolver* h, float* hz, int cap) try {
    if (!analysisHandle(h, "")) return -1;
    return h->s->spectrumBins(hz, cap);
} PV_API_CATCH(-1)

int PvAmdGetSpectrumSource(PvAmdSolver* h, float* out3n) try {
    if (!analysisCall(h, "", __func__, out3n)) return -1;
    return ret(h, h->s->spectrumSource(out3n));
} PV_API_CATCH(-1)

int PvAmdComputeSpectrum(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "")) return -1;
    return ret(h, h->s->computeSpectrum(ms));
} PV_API_CATCH(-1)

int PvAmdCopySpectrum(PvAmdSolver* h, float* out) try {
    return analysisCopy(h, kMapSpectrum, "", __func__, out);
} PV_API_CATCH(-1)

int PvAmdCopySpectrumBlock(PvAmdSolver* h, int r0, int c0, int nr, int nc, float* out) try {
    return analysisCopyBlock(h, kMapSpectrum, "", __func__, r0, c0, nr, nc, out);
} PV_API_CATCH(-1)

int PvAmdGetSpectrum(PvAmdSolver* h, float ex, float ey, float ez, float* out3n) try {
    return analysisGet(h, kMapSpectrum, "", __func__, ex, ez, out3n);
} PV_API_CATCH(-1)

// waterfall (pv_waterfall.hip, pv_solver_waterfall.cpp; the setting: pv_waterfall.h waterfallSettingError)
static_assert(PVA_WATERFALL_MAX_BINS == kWaterfallMaxBins && PVA_WATERFALL_MAX_SLICES == kWaterfallMaxSlices &&
                  PVA_WATERFALL_MAX_RECEIVERS == kWaterfallMaxReceivers,
              "planeverb_amd.h vs pv_waterfall.h");

int PvAmdSetWaterfall(PvAmdSolver* h, const float* hz, int nBins, float sliceSeconds, int nSlices) try {
    if (!h) {
        g_lastError = "null solver handle";
        return -1;
    }
    if (nBins != 0) {
        if (const char* e = waterfallSettingError(hz, nBins, (int)h->spec.fs, sliceSeconds, nSlices)) {
            g_lastError = e;
            return -1;
        }
    }
    if (!analysisHandle(h, "waterfall: ")) return -1;
    return ret(h, h->s->setWaterfall(hz, nBins, sliceSeconds, nSlices));
} PV_API_CATCH(-1)

int PvAmdGetWaterfall(PvAmdSolver* h, float* hz, int cap, float* sliceSeconds, int* sliceSteps, int* nSlices) try {
    if (!analysisHandle(h, "waterfall: ")) return -1;
    return h->s->waterfall(hz, cap, sliceSeconds, sliceSteps, nSlices);
} PV_API_CATCH(-1)

int PvAmdWaterfallFloats(PvAmdSolver* h) try {
    if (!analysisHandle(h, "waterfall: ")) return -1;
    const int f = h->s->waterfallRecordFloats();
    if (f < 0) g_lastError = "waterfall: no setting (PvAmdSetWaterfall)";
    return f;
} PV_API_CATCH(-1)

int PvAmdComputeWaterfall(PvAmdSolver* h, const float* xyz, int nPos, float* ms) try {
    if (!analysisHandle(h, "waterfall: ")) return -1;
    return ret(h, h->s->computeWaterfall(xyz, nPos, ms));
} PV_API_CATCH(-1)

int PvAmdCopyWaterfall(PvAmdSolver* h, float* out, int nPos) try {
    if (!analysisCall(h, "waterfall: ", __func__, out)) return -1;
    return ret(h, h->s->copyWaterfall(out, nPos));
} PV_API_CATCH(-1)

// source arrays (pv_arrays.hip, pv_solver_arrays.cpp; the definition: pv_arrays.h)
static_assert(PVA_ARRAYS_MAX == kArraysMax && PVA_ARRAY_MEMBERS_MAX == kArrayMembersMax && PVA_ARRAY_NEAREST == kArrayNearest &&
                  PVA_ARRAY_LAGRANGE3 == kArrayLagrange3,
              "planeverb_amd.h vs pv_arrays.h");

int PvAmdSetArrays(PvAmdSolver* h, const int* count, int nArrays, const float* members5, int interp) try {
    if (!h) {
        g_lastError = "null solver handle";
        return -1;
    }
    if (nArrays != 0) {  // (what needs no grid, in front of creating a solver)
        if (const char* e = arraysCountError(count, nArrays, members5)) {
            g_lastError = e;
            return -1;
        }
    }
    if (!analysisHandle(h, "arrays: ")) return -1;
    return ret(h, h->s->setArrays(count, nArrays, members5, interp));
} PV_API_CATCH(-1)

int PvAmdGetArrays(PvAmdSolver* h, int* count, int cap, int* interp) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    return h->s->arrays(count, cap, interp);
} PV_API_CATCH(-1)

int PvAmdGetArrayTaps(PvAmdSolver* h, int array, int* memberIndex, int* delaySteps, float* weight, int cap) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    const int n = h->s->arrayTapsOf(array, memberIndex, delaySteps, weight, cap);
    if (n < 0) ret(h, false);
    return n;
} PV_API_CATCH(-1)

int PvAmdSetArrayRecords(PvAmdSolver* h, unsigned timeKinds, unsigned spectralKinds) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    return ret(h, h->s->setArrayRecords(timeKinds, spectralKinds));
} PV_API_CATCH(-1)

int PvAmdGetArrayRecordKinds(PvAmdSolver* h, unsigned* timeKinds, unsigned* spectralKinds) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    h->s->arrayRecordKinds(timeKinds, spectralKinds);
    return 0;
} PV_API_CATCH(-1)

int PvAmdArrayRecordFloats(PvAmdSolver* h, int family, unsigned kind) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    const int n = h->s->arrayRecordFloats(family, kind);
    if (n < 0) ret(h, false);
    return n;
} PV_API_CATCH(-1)

int PvAmdComputeArrays(PvAmdSolver* h, float* ms) try {
    if (!analysisHandle(h, "arrays: ")) return -1;
    return ret(h, h->s->computeArrays(ms));
} PV_API_CATCH(-1)

int PvAmdCopyArrayResponse(PvAmdSolver* h, int array, float* outT) try {
    if (!analysisCall(h, "arrays: ", __func__, outT)) return -1;
    return ret(h, h->s->copyArrayResponse(array, outT));
} PV_API_CATCH(-1)

int PvAmdGetArrayOnsets(PvAmdSolver* h, float* out, int nArrays) try {
    if (!analysisCall(h, "arrays: ", __func__, out)) return -1;
    return ret(h, h->s->arrayOnsets(out, nArrays));
} PV_API_CATCH(-1)

int PvAmdGetArrayRecords(PvAmdSolver* h, int family, unsigned kind, float* out, int nArrays) try {
    if (!analysisCall(h, "arrays: ", __func__, out)) return -1;
    return ret(h, h->s->arrayRecords(family, kind, out, nArrays));
} PV_API_CATCH(-1)

// auralisation (pv_aural.hip, pv_solver_aural.cpp; the definition: pv_aural.h)
static_assert(PVA_AURAL_MAX_TAPS == kAuralMaxTaps && PVA_AURAL_MAX_RECEIVERS == kAuralMaxReceivers && PVA_AURAL_MAX_SIGNALS == kAuralMaxSignals &&
                  PVA_AURAL_MAX_SAMPLES == kAuralMaxSignalSamples && PVA_AURAL_RECEIVERS == kAuralReceivers && PVA_AURAL_ARRAYS == kAuralArrays &&
                  PVA_AURAL_TILED == kAuralTiled && PVA_AURAL_PLAIN == kAuralPlain,
              "planeverb_amd.h vs pv_aural.h");

int PvAmdSetAuralisation(PvAmdSolver* h, int rate, int zeroCrossings, float beta) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    return ret(h, h->s->setAuralisation(rate, zeroCrossings, beta));
} PV_API_CATCH(-1)

int PvAmdGetAuralisation(PvAmdSolver* h, int* rate, int* zeroCrossings, float* beta, int* L, int* K) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    if (h->s->auralisation(rate, zeroCrossings, beta, L, K)) return 0;
    g_lastError = "aural: no setting (PvAmdSetAuralisation)";
    return -1;
} PV_API_CATCH(-1)

int PvAmdGetAuralTaps(PvAmdSolver* h, int* first, float* w, int capN) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    const int n = h->s->auralTapsOf(first, w, capN);
    if (n < 0) ret(h, false);
    return n;
} PV_API_CATCH(-1)

int PvAmdComputeAuralResponses(PvAmdSolver* h, int source, const float* xyz, int nPos, float* ms) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    return ret(h, h->s->computeAuralResponses(source, xyz, nPos, ms));
} PV_API_CATCH(-1)

int PvAmdCopyAuralResponse(PvAmdSolver* h, int r, float* outL) try {
    if (!analysisCall(h, "aural: ", __func__, outL)) return -1;
    return ret(h, h->s->copyAuralResponse(r, outL));
} PV_API_CATCH(-1)

int PvAmdSetAuralForm(PvAmdSolver* h, int form) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    return ret(h, h->s->setAuralForm(form));
} PV_API_CATCH(-1)

int PvAmdAuralise(PvAmdSolver* h, const float* signals, int nSignals, int N, const int* route, const float* gain, float* ms) try {
    if (!analysisHandle(h, "aural: ")) return -1;
    return ret(h, h->s->auralise(signals, nSignals, N, route, gain, ms));
} PV_API_CATCH(-1)

int PvAmdCopyAuralOutput(PvAmdSolver* h, int r, float* outM) try {
    if (!analysisCall(h, "aural: ", __func__, outM)) return -1;
    return ret(h, h->s->copyAuralOutput(r, outM));
} PV_API_CATCH(-1)

int PvAmdCopyAuralMix(PvAmdSolver* h, float* outM) try {
    if (!analysisCall(h, "aural: ", __func__, outM)) return -1;
    return ret(h, h->s->copyAuralMix(outM));
} PV_API_CATCH(-1)

void PvAmdAuralShape(int* outputsPerBlock, int* tapsPerChunk) try {
    if (outputsPerBlock) *outputsPerBlock = kAuralOutputsPerBlock;
    if (tapsPerChunk) *tapsPerChunk = kAuralTapsPerChunk;
} PV_API_CATCH_VOID

// zone statistics (pv_zones.hip; the labels: pv_zones.h zoneLabelsError)
static_assert(sizeof(PvAmdZoneStat) == sizeof(ZoneStat), "64 bytes");
static_assert(PVA_MAP_ROOM_METRICS == kMapRoomMetrics && PVA_MAP_SPECTRUM == kMapSpectrum && PVA_MAP_SPECTRUM + 1 == kAnalysisKinds,
              "the order of AnalysisKind");
static_assert(PVA_ZONES_MAX == kZonesMax, "a lane per zone");

static bool zoneKind(int kind) {
    if (kind >= 0 && kind < kAnalysisKinds) return true;
    g_lastError = "zone statistics: kind is one of PVA_MAP_*";
    return false;
}

int PvAmdSetZones(PvAmdSolver* h, const unsigned char* labels, int nZones) try {
    if (!h) {
        g_lastError = "zone statistics: null solver handle";
        return -1;
    }
    if (labels || nZones != 0) {
        if (const char* e = zoneLabelsError(labels, (long long)h->spec.gx * h->spec.gy, nZones)) {
            g_lastError = e;
            return -1;
        }
    }
    if (!analysisHandle(h, "zone statistics: ")) return -1;
    return ret(h, h->s->setZones(labels, nZones));
} PV_API_CATCH(-1)

int PvAmdGetZones(PvAmdSolver* h, unsigned char* labels, int* nZones) try {
    if (!analysisHandle(h, "zone statistics: ")) return -1;
    const int n = h->s->zones(labels);
    if (nZones) *nZones = n;
    return 0;
} PV_API_CATCH(-1)

int PvAmdZoneStatPlanes(PvAmdSolver* h, int kind) try {
    if (!zoneKind(kind) || !analysisHandle(h, "zone statistics: ")) return -1;
    const int n = h->s->zoneStatPlanes((AnalysisKind)kind);
    if (n < 0) g_lastError = "zone statistics: the kind's setting is missing (slots, bands or bins)";
    return n;
} PV_API_CATCH(-1)

int PvAmdComputeZoneStats(PvAmdSolver* h, int kind, PvAmdZoneStat* out, int cap, float* ms) try {
    if (!zoneKind(kind) || !analysisCall(h, "zone statistics: ", __func__, out)) return -1;
    int count = 0;
    if (!h->s->computeZoneStats((AnalysisKind)kind, out, cap, ms, &count)) return ret(h, false);
    return count;
} PV_API_CATCH(-1)

// zone decay (pv_zone_decay.hip)
static_assert(sizeof(PvAmdZoneDecay) == sizeof(ZoneDecay), "64 bytes");
static_assert(PVA_ZONE_DECAY_ABSOLUTE == kZoneDecayAbsolute && PVA_ZONE_DECAY_ONSET == kZoneDecayOnset, "the alignments");

int PvAmdComputeZoneDecay(PvAmdSolver* h, int align, PvAmdZoneDecay* out, int cap, double* etc, double* edc, float* ms) try {
    if (!analysisCall(h, "zone decay: ", __func__, out) || !zoneDecayAlign(align)) return -1;
    int count = 0;
    if (!h->s->computeZoneDecay(align, out, cap, etc, edc, ms, &count)) return ret(h, false);
    return count;
} PV_API_CATCH(-1)

int PvAmdZoneDecayChunkSlots(PvAmdSolver* h) try {
    if (!analysisHandle(h, "zone decay: ")) return -1;
    return h->s->zoneDecayChunkSlots();
} PV_API_CATCH(-1)

// the ABSOLUTE curves inside a sparse-emitter run (pv_zone_decay.hip: the rows kernel over the ring source)
int PvAmdSetZoneCurves(PvAmdSolver* h, int enable) try {
    if (!analysisHandle(h, "zone curves: ")) return -1;
    return ret(h, h->s->setZoneCurves(enable != 0));
} PV_API_CATCH(-1)

int PvAmdGetZoneCurves(PvAmdSolver* h, int* enabled) try {
    if (!analysisHandle(h, "zone curves: ")) return -1;
    if (enabled) *enabled = h->s->zoneCurves() ? 1 : 0;
    return 0;
} PV_API_CATCH(-1)

// the room-metrics and spectrum maps of the labelled cells inside a sparse-emitter run (pv_zone_maps.hip)
static_assert(PVA_ZMAP_ROOM_METRICS == kZoneMapRoomMetrics && PVA_ZMAP_SPECTRUM == kZoneMapSpectrum, "the map kinds");

int PvAmdSetZoneMaps(PvAmdSolver* h, unsigned kinds) try {
    if (!analysisHandle(h, "zone maps: ")) return -1;
    return ret(h, h->s->setZoneMaps(kinds));
} PV_API_CATCH(-1)

int PvAmdGetZoneMaps(PvAmdSolver* h, unsigned* kinds) try {
    if (!analysisHandle(h, "zone maps: ")) return -1;
    if (kinds) *kinds = h->s->zoneMaps();
    return 0;
} PV_API_CATCH(-1)

// zone band decay (pv_zone_band_decay.hip)
static_assert(sizeof(PvAmdZoneBandDecay) == sizeof(ZoneBandDecay), "96 bytes");

int PvAmdComputeZoneBandDecay(PvAmdSolver* h, int align, PvAmdZoneBandDecay* out, int cap, double* etc, double* edc, float* ms) try {
    if (!analysisCall(h, "zone band decay: ", __func__, out) || !zoneDecayAlign(align, "zone band decay: ")) return -1;
    int count = 0;
    if (!h->s->computeZoneBandDecay(align, out, cap, etc, edc, ms, &count)) return ret(h, false);
    return count;
} PV_API_CATCH(-1)

int PvAmdZoneBandDecayChunk(PvAmdSolver* h, int* slots, int* bands) try {
    if (!analysisHandle(h, "zone band decay: ")) return -1;
    return h->s->zoneBandDecayChunks(slots, bands);
} PV_API_CATCH(-1)

int PvAmdCopyPulse(PvAmdSolver* h, float* out) try {
    if (!out || !ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->copyPulse(out) : h->s->copyPulse(out));
} PV_API_CATCH(-1)

int PvAmdCopyMaterial(PvAmdSolver* h, uint8_t* beta, float* R) try {
    if (!ensure(h, true)) return -1;
    return ret(h, h->g ? h->g->copyMaterial(beta, R) : h->s->copyMaterial(beta, R));
} PV_API_CATCH(-1)

int PvAmdSetFields(PvAmdSolver* h, const float* pr, const float* vx, const float* vy) try {
    if (!ensure(h)) return -1;
    return ret(h, h->s->setFields(pr, vx, vy));
} PV_API_CATCH(-1)

int PvAmdRunSteps(PvAmdSolver* h, int nsteps, int withPulse, float lx, float lz) try {
    if (!wholeGrid(h) || !ensure(h)) return -1;
    return ret(h, h->s->runSteps(nsteps, withPulse != 0, lx, lz));
} PV_API_CATCH(-1)

// ---------------------------------------------------------------------------------------------------------------
// Part 3: sharded runs + RCCL gather
// ---------------------------------------------------------------------------------------------------------------

struct PvAmdComm {
    Comm* c = nullptr;
    ~PvAmdComm() { delete c; }
};

int PvAmdShardPlan(int nRuns, int world, int rank, int nLocalSolvers, int* runIdx, int* solverIdx, int cap) try {
    const std::vector<ShardItem> plan = shardPlan(nRuns, world, rank, nLocalSolvers);
    for (int i = 0; i < (int)plan.size() && i < cap; ++i) {
        if (runIdx) runIdx[i] = plan[(size_t)i].run;
        if (solverIdx) solverIdx[i] = plan[(size_t)i].solver;
    }
    return (int)plan.size();
} PV_API_CATCH(-1)

int PvAmdPlanSegments(const unsigned char* air, int ntx, int nty, int tileRows, int maxTileColumns, int target, int* seg4,
                      int cap) try {
    if (!air || ntx < 1 || nty < 1) return 0;
    const std::vector<SegRect> segs = planSegments(air, ntx, nty, tileRows, maxTileColumns, target);
    for (int i = 0; i < (int)segs.size() && i < cap && seg4; ++i) {
        seg4[4 * i] = segs[(size_t)i].row0;
        seg4[4 * i + 1] = segs[(size_t)i].nrows;
        seg4[4 * i + 2] = segs[(size_t)i].tj0;
        seg4[4 * i + 3] = segs[(size_t)i].w;
    }
    return (int)segs.size();
} PV_API_CATCH(0)

int PvAmdCommUniqueId(char id128[128]) try {
    if (!id128) return -1;
    return Comm::uniqueId(id128, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

PvAmdComm* PvAmdCommCreate(const char id128[128], int rank, int world, int device) try {
    if (!id128) return nullptr;
    std::unique_ptr<PvAmdComm> h(new PvAmdComm());
    h->c = Comm::create(id128, rank, world, device, &g_lastError);
    return h->c ? h.release() : nullptr;
} PV_API_CATCH(nullptr)

void PvAmdCommDestroy(PvAmdComm* h) try {
    delete h;
} PV_API_CATCH_VOID

int PvAmdCommAllGather(PvAmdComm* h, const float* mine, int countPerRank, float* all) try {
    if (!h || !h->c || !mine || !all) return -1;
    return h->c->allGather(mine, countPerRank, all, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdRunSharded(PvAmdSolver* const* hs, int nSolvers, const float* listenersXYZ, int nRuns, const float* emittersXYZ,
                    int E, int rank, int world, PvAmdComm* comm, PlaneverbOutput* out) try {
    if (!hs || nSolvers < 1 || !listenersXYZ || nRuns < 0 || (E > 0 && !emittersXYZ) || E < 0 || E > Solver::kMaxQueries ||
        !out || world < 1 || rank < 0 || rank >= world) {
        g_lastError = "PvAmdRunSharded: invalid arguments";
        return -1;
    }
    if (world > 1 && (!comm || !comm->c || comm->c->world() != world || comm->c->rank() != rank)) {
        g_lastError = "PvAmdRunSharded: ranks span processes, a matching PvAmdComm is required";
        return -1;
    }
    std::vector<Solver*> sv;
    for (int i = 0; i < nSolvers; ++i) {
        if (!wholeGrid(hs[i]) || !ensure(hs[i])) return -1;
        sv.push_back(hs[i]->s);
    }
    const std::vector<ShardItem> plan = shardPlan(nRuns, world, rank, nSolvers);
    const int perRank = (nRuns + world - 1) / world;
    const size_t rec = (size_t)E * 8;
    std::vector<float> mine((size_t)perRank * rec, 0.f);
    std::vector<int> pending((size_t)nSolvers, -1);
    auto collect = [&](int s) -> bool {  // wait for solver s's run, take its records (gathered behind the analysis)
        const int j = pending[(size_t)s];
        pending[(size_t)s] = -1;
        float v[Solver::kMaxQueries * 8];
        unsigned char valid[Solver::kMaxQueries];
        if (!sv[(size_t)s]->sync() || !sv[(size_t)s]->queriedOutputs(v, valid, E)) return false;
        for (int e = 0; e < E; ++e) {
            float* dst = mine.data() + (size_t)j * rec + (size_t)e * 8;
            if (valid[e]) {
                std::memcpy(dst, v + 8 * e, 32);
            } else {  // the reference's sentinel for a position outside the grid (FDTD.cpp:19-47)
                std::memset(dst, 0, 32);
                dst[0] = kInvalidDryGain;
            }
        }
        return true;
    };
    for (size_t j = 0; j < plan.size(); ++j) {
        const int s = plan[j].solver, k = plan[j].run;
        if (pending[(size_t)s] >= 0 && !collect(s)) return ret(hs[s], false);  // the other solvers keep the GPU busy
        if (!sv[(size_t)s]->setOutputQueries(emittersXYZ + (size_t)k * E * 3, E) ||
            !sv[(size_t)s]->run(listenersXYZ[3 * k], listenersXYZ[3 * k + 1], listenersXYZ[3 * k + 2], /*wait=*/false))
            return ret(hs[s], false);
        pending[(size_t)s] = (int)j;
    }
    for (int s = 0; s < nSolvers; ++s)
        if (pending[(size_t)s] >= 0 && !collect(s)) return ret(hs[s], false);
    float* o = reinterpret_cast<float*>(out);
    if (world == 1) {
        for (int k = 0; k < nRuns; ++k) std::memcpy(o + (size_t)k * rec, mine.data() + (size_t)k * rec, rec * 4);
        return 0;
    }
    std::vector<float> all((size_t)world * perRank * rec);
    if (rec > 0 && !comm->c->allGather(mine.data(), (int)((size_t)perRank * rec), all.data(), &g_lastError)) return -1;
    for (int k = 0; k < nRuns; ++k)  // run k = the (k / world)-th run of rank k mod world
        std::memcpy(o + (size_t)k * rec, all.data() + ((size_t)(k % world) * perRank + (size_t)(k / world)) * rec, rec * 4);
    return 0;
} PV_API_CATCH(-1)

#endif  // !PVA_HOST_TEST

int PvAmdHostGridInfo(float sx, float sy, int res, PvAmdInfo* out) try {
    if (!out || res < kLowResolution) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    std::memset(out, 0, sizeof(*out));
    out->gx = g.gx;
    out->gy = g.gy;
    out->T = g.T;
    out->fs = (int)g.fs;
    out->res = g.res;
    out->dx = g.dx;
    out->dt = g.dt;
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostPulseSelfCheck(void) try { return pulseMatchesReferenceLibm() ? 1 : 0; } PV_API_CATCH(0)

int PvAmdHostPulse(float sx, float sy, int res, float* out) try {
    if (!out || res < kLowResolution) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    const std::vector<float> p = gaussianPulse(g);
    std::memcpy(out, p.data(), p.size() * sizeof(float));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostRasterize(float sx, float sy, int res, const float* b5, const int* ops, int n, uint8_t* beta,
                       float* R) try {
    if (res < kLowResolution) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    MaterialPlane m;
    m.init(g);
    for (int i = 0; i < n; ++i) {
        const Box b{b5[5 * i], b5[5 * i + 1], b5[5 * i + 2], b5[5 * i + 3], b5[5 * i + 4]};
        if (ops && ops[i] < 0)
            m.remove(b);
        else
            m.add(b);
    }
    const size_t cells = (size_t)g.NX * g.NY;
    if (beta) std::memcpy(beta, m.beta().data(), cells);
    if (R) std::memcpy(R, m.R().data(), cells * sizeof(float));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostOrientedBoxVertices(float px, float py, float w, float h, float ax, float ay, float* out8) try {
    return (out8 && orientedBoxVertices(px, py, w, h, ax, ay, out8, &g_lastError)) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdHostShape(const float* xy, int n, float absorption, float* out16) try {
    Shape sh;
    if (!out16 || !makeShape(xy, n, absorption, &sh, &g_lastError)) return -1;
    std::memcpy(out16, sh.xy, (size_t)2 * sh.n * sizeof(float));
    return sh.n;
} PV_API_CATCH(-1)

int PvAmdHostShapeCoverage(float sx, float sy, int res, const float* xy, int n, uint8_t* cover) try {
    Shape sh;
    if (res < kLowResolution || !cover || !makeShape(xy, n, 0.f, &sh, &g_lastError)) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    std::memset(cover, 0, (size_t)g.NX * g.NY);
    int x0, x1, y0, y1;
    shapeCellBounds(sh, g, &x0, &x1, &y0, &y1);
    for (int x = x0; x < x1; ++x)
        for (int y = y0; y < y1; ++y) cover[(size_t)x * g.NY + y] = shapeCovers(sh, g.dx, x, y) ? 1 : 0;
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostRoundShapeCoverage(float sx, float sy, int res, int kind, const float* xy, int n, float radius, uint8_t* cover) try {
    Shape sh;
    if (res < kLowResolution || !cover) {
        g_lastError = "PvAmdHostRoundShapeCoverage: resolution below 275 or a null array";
        return -1;
    }
    bool ok = false;
    if (kind == PVA_SHAPE_POLYGON) {
        ok = makePolygon(xy, n, 0.f, &sh, &g_lastError);
    } else if (kind == PVA_SHAPE_WALL_PATH) {
        ok = wallPathShape(xy, n, radius, 0.f, &sh);
    } else if (kind == PVA_SHAPE_DISC || kind == PVA_SHAPE_CAPSULE) {
        if (n != kind)  // (1 point, 2 points)
            g_lastError = kind == PVA_SHAPE_DISC ? "disc: one point" : "capsule: two points";
        else
            ok = makeRound(xy, n, radius, 0.f, &sh, &g_lastError);
    } else {
        g_lastError = "PvAmdHostRoundShapeCoverage: unknown kind";
    }
    if (!ok) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    std::memset(cover, 0, (size_t)g.NX * g.NY);
    int x0, x1, y0, y1;
    shapeCellBounds(sh, g, &x0, &x1, &y0, &y1);
    for (int x = x0; x < x1; ++x)
        for (int y = y0; y < y1; ++y) cover[(size_t)x * g.NY + y] = shapeCovers(sh, g.dx, x, y) ? 1 : 0;
    return 0;
} PV_API_CATCH(-1)

// indices and finite inputs only: what the section needs (a mesh's other rules are validateMesh's)
static bool sectionInputsOk(const float* verts, int nv, const int* tris, int nt, const float* m12, float h, const char* name) {
    bool ok = verts && tris && nv >= 1 && nt >= 1 && nt <= kMeshMaxTris && h - h == 0.f;
    for (size_t i = 0; ok && i < (size_t)3 * nv; ++i) ok = std::isfinite(verts[i]);
    for (size_t i = 0; ok && i < (size_t)3 * nt; ++i) ok = tris[i] >= 0 && tris[i] < nv;
    if (!ok) {
        g_lastError = std::string(name) + ": a null array, a count out of range, a non-finite input or an index outside [0, nv)";
        return false;
    }
    return !m12 || validateMeshTransform(m12, &g_lastError);
}

int PvAmdHostMeshSection(const float* verts, int nv, const int* tris, int nt, const float* m12, float h, float* out4nt,
                         uint8_t* valid_nt) try {
    if (!out4nt || !valid_nt) {
        g_lastError = "PvAmdHostMeshSection: a null array";
        return -1;
    }
    if (!sectionInputsOk(verts, nv, tris, nt, m12, h, "PvAmdHostMeshSection")) return -1;
    meshSection(verts, tris, nt, m12, h, out4nt, valid_nt);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostMeshCoverage(float sx, float sy, int res, const float* verts, int nv, const int* tris, int nt, const float* m12, float h,
                          int mode, float radius, uint8_t* cover) try {
    if (res < kLowResolution || !cover) {
        g_lastError = "PvAmdHostMeshCoverage: resolution below 275 or a null array";
        return -1;
    }
    if (!(h - h == 0.f)) {
        g_lastError = "PvAmdHostMeshCoverage: the height is not finite";
        return -1;
    }
    if (!validateMesh(verts, nv, tris, nt, 0.f, mode, radius, &g_lastError) || (m12 && !validateMeshTransform(m12, &g_lastError)))
        return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    std::vector<float> seg((size_t)4 * nt);
    std::vector<uint8_t> valid((size_t)nt);
    meshSection(verts, tris, nt, m12, h, seg.data(), valid.data());
    meshCoverage(g, seg.data(), valid.data(), nt, mode, radius, cover);
    return 0;
} PV_API_CATCH(-1)

static int hostEdgeLayerTables(float sx, float sy, int res, const int* width4, double r0, float* out, const char* name) {
    if (res < kLowResolution || !width4 || !out) {
        g_lastError = std::string(name) + ": resolution below 275 or a null array";
        return -1;
    }
    if (!edgeLayerR0Ok(r0)) {
        g_lastError = std::string(name) + ": r0 must lie strictly between 0 and 1";
        return -1;
    }
    const GridSpec g = makeGridSpec(sx, sy, res);
    if (g.gx < 1 || g.gy < 1) {
        g_lastError = std::string(name) + ": grid has no cells";
        return -1;
    }
    const char* why = edgeLayerRefusal(g.gx, g.gy, width4);
    if (*why) {
        g_lastError = std::string(name) + ": " + why;
        return -1;
    }
    edgeLayerTables(g.gx, g.gy, g.courant, width4, out, r0);
    return 4 * (g.NX + g.NY);
}

int PvAmdHostEdgeLayerTables(float sx, float sy, int res, const int* width4, float* out) try {
    return hostEdgeLayerTables(sx, sy, res, width4, kEdgeLayerR0, out, "PvAmdHostEdgeLayerTables");
} PV_API_CATCH(-1)

int PvAmdHostEdgeLayerTablesR0(float sx, float sy, int res, const int* width4, double r0, float* out) try {
    return hostEdgeLayerTables(sx, sy, res, width4, r0, out, "PvAmdHostEdgeLayerTablesR0");
} PV_API_CATCH(-1)

int PvAmdHostEnclosure(const uint8_t* beta, int nx, int ny, int seedX, int seedY, int tileRows, int tileCols, int maxTiles,
                       int* out10) try {
    if (!beta || !out10 || nx < 1 || ny < 1 || tileRows < 1 || tileCols < 1 || (long long)nx * ny > INT_MAX) {
        g_lastError = "PvAmdHostEnclosure: bad arguments";
        return -1;
    }
    const Enclosure e = findEnclosure(beta, nx, ny, seedX, seedY, tileRows, tileCols, maxTiles, nullptr);
    const int v[10] = {e.found, e.cells, e.r0, e.c0, e.r1, e.c1, e.ti0, e.tj0, e.tis, e.tjs};
    std::copy(v, v + 10, out10);
    return e.cells;
} PV_API_CATCH(-1)

int PvAmdHostWindowClear(int windowRun, const int* win4, const int* prevRect4, int planesDirty, int sweptDirty, int splitPlanes) try {
    if (!win4 || !prevRect4) {
        g_lastError = "PvAmdHostWindowClear: bad arguments";
        return -1;
    }
    return (int)planClear(windowRun != 0, win4, prevRect4, planesDirty != 0, sweptDirty != 0, splitPlanes != 0);
} PV_API_CATCH(-1)

int PvAmdHostLoadPv(const char* path, float* b5, int maxBoxes) try {
    if (!path) return -1;
    std::vector<Box> boxes;
    if (!loadPv(path, &boxes, &g_lastError)) return -1;
    for (int i = 0; i < (int)boxes.size() && i < maxBoxes; ++i) {
        b5[5 * i] = boxes[(size_t)i].x;
        b5[5 * i + 1] = boxes[(size_t)i].y;
        b5[5 * i + 2] = boxes[(size_t)i].w;
        b5[5 * i + 3] = boxes[(size_t)i].h;
        b5[5 * i + 4] = boxes[(size_t)i].R;
    }
    return (int)boxes.size();
} PV_API_CATCH(-1)

int PvAmdHostSavePv(const char* path, const float* b5, const int* ids, int n) try {
    if (!path || (n > 0 && !b5)) return -1;
    std::vector<std::pair<int, Box>> boxes;
    for (int i = 0; i < n; ++i)
        boxes.emplace_back(ids ? ids[i] : i, Box{b5[5 * i], b5[5 * i + 1], b5[5 * i + 2], b5[5 * i + 3], b5[5 * i + 4]});
    return savePv(path, boxes, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdHostRoomMetrics(const float* p, int T, int fs, int onset, PvAmdRoomMetrics* out) try {
    if (!p || !out || T <= 0 || onset < 0 || onset >= T) {
        g_lastError = "PvAmdHostRoomMetrics: an impulse response p[T], T > 0, 0 <= onset < T and an output record";
        return -1;
    }
    static_assert(sizeof(PvAmdRoomMetrics) == kRoomMetricFloats * sizeof(float), "ten floats");
    float v[kRoomMetricFloats];
    roomMetricsOfIr(p, T, fs, onset, v);
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostDecayTimes(const float* p, int T, int fs, int onset, PvAmdDecayTimes* out) try {
    if (!p || !out || T <= 0 || onset < 0 || onset >= T) {
        g_lastError = "decay times: PvAmdHostDecayTimes: an impulse response p[T], T > 0, 0 <= onset < T and an output record";
        return -1;
    }
    static_assert(sizeof(PvAmdDecayTimes) == kDecayFloats * sizeof(float), "eight floats");
    float v[kDecayFloats];
    decayTimesOfIr(p, T, fs, onset, v);
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostLateralFraction(const float* p, const float* vx, const float* vy, int T, int fs, int onset,
                             PvAmdLateralFraction* out) try {
    if (!p || !vx || !vy || !out || T <= 0 || onset < 0 || onset >= T) {
        g_lastError = "lateral fraction: PvAmdHostLateralFraction: an impulse response p[T], vx[T], vy[T], T > 0, 0 <= onset < T and an output record";
        return -1;
    }
    static_assert(sizeof(PvAmdLateralFraction) == kLateralFloats * sizeof(float), "eleven floats");
    float v[kLateralFloats];
    lateralFractionOfIr(p, vx, vy, T, fs, onset, v);
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostEchoCriterion(const float* p, int T, int fs, int onset, PvAmdEchoCriterion* out) try {
    if (!p || !out || T <= 0 || onset < 0 || onset >= T) {
        g_lastError = "echo: PvAmdHostEchoCriterion: an impulse response p[T], T > 0, 0 <= onset < T and an output record";
        return -1;
    }
    if (!echoFsOk(fs)) {
        g_lastError = "echo: the sampling rate gives a speech lag below one step ((int)(0.009f * (float)fs) < 1)";
        return -1;
    }
    static_assert(sizeof(PvAmdEchoCriterion) == kEchoFloats * sizeof(float), "ten floats");
    float v[kEchoFloats];
    echoCriterionOfIr(p, T, fs, onset, v);
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostEchogram(const float* p, const float* vx, const float* vy, int T, int fs, int onset, float slotSeconds, int nSlots,
                      float* out) try {
    if (!p || !vx || !vy || !out || T <= 0 || onset < 0 || onset >= T || nSlots < 1 || nSlots > kEchogramMaxSlots) {
        g_lastError =
            "echogram: PvAmdHostEchogram: an impulse response p[T], vx[T], vy[T], T > 0, 0 <= onset < T, 1 .. 32 slots and an output of "
            "1 + 3 nSlots floats";
        return -1;
    }
    if (!echogramSlotOk(slotSeconds, fs)) {
        g_lastError = "echogram: slotSeconds must be finite and give 1 .. 2^20 steps per slot ((int)(slotSeconds * (float)fs))";
        return -1;
    }
    echogramOfIr(p, vx, vy, T, onset, echogramSlotSteps(slotSeconds, fs), nSlots, out);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostLobes(const float* p, const float* vx, const float* vy, int T, int fs, int onset, const float* edgesSeconds, int nEdges,
                   float* out) try {
    if (!p || !vx || !vy || !out || T <= 0 || onset < 0 || onset >= T || fs <= 0) {
        g_lastError =
            "lobes: PvAmdHostLobes: an impulse response p[T], vx[T], vy[T], T > 0, fs > 0, 0 <= onset < T and an output of 1 + 5 nW floats";
        return -1;
    }
    if (nEdges == 0) {
        edgesSeconds = kLobesDefaultEdges;
        nEdges = 2;
    }
    LobeEdges ed;
    if (!lobesEdgeSteps(edgesSeconds, nEdges, fs, &ed)) {
        g_lastError = kLobesEdgesError;
        return -1;
    }
    lobesOfIr(p, vx, vy, T, onset, ed, nEdges, out);
    return 0;
} PV_API_CATCH(-1)

int PvAmdLobeGains(const float* record, int nWindows, float fwdX, float fwdY, int pattern, float* gains) try {
    if (!record || !gains || nWindows < 1 || nWindows > kLobesMaxWindows || (pattern != 0 && pattern != 1)) {
        g_lastError = "lobes: PvAmdLobeGains: a record of 1 + 5 nWindows floats, 1 <= nWindows <= 8, pattern 0 (omni) or 1 (cardioid)";
        return -1;
    }
    lobeGainsOfRecord(record, nWindows, fwdX, fwdY, pattern, gains);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostBandCoefs(int fs, const float* centreHz, int n, int fraction, float* out10n) try {
    if (const char* e = bandsError(centreHz, n, fraction, fs)) {
        g_lastError = e;
        return -1;
    }
    if (!out10n) {
        g_lastError = "band metrics: PvAmdHostBandCoefs: null output";
        return -1;
    }
    bandCoefs(fs, centreHz, n, fraction, out10n);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostBandMetrics(const float* p, int T, int fs, int onset, const float* coefs10n, int n, PvAmdBandMetrics* out12n) try {
    if (!p || !coefs10n || !out12n || T <= 0 || fs <= 0 || onset < 0 || onset >= T || n < 1 || n > kBandsMax) {
        g_lastError =
            "band metrics: PvAmdHostBandMetrics: an impulse response p[T], T > 0, fs > 0, 0 <= onset < T, 1 .. 8 coefficient sets and an "
            "output of n records";
        return -1;
    }
    for (int j = 0; j < n; ++j)
        bandMetricsOfIr(p, T, fs, onset, coefs10n + (size_t)kBandCoefs * j, reinterpret_cast<float*>(out12n) + (size_t)kBandFloats * j);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostModulationTable(int T, int fs, const float* hz14, float* out28T) try {
    if (T <= 0 || fs <= 0 || !out28T) {
        g_lastError = "modulation: PvAmdHostModulationTable: T > 0, fs > 0 and a table of T * 28 floats";
        return -1;
    }
    if (!hz14) hz14 = kModDefaultHz;
    if (const char* e = modulationFreqsError(hz14, fs)) {
        g_lastError = e;
        return -1;
    }
    modulationTable(T, fs, hz14, out28T);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostModulation(const float* p, int T, int fs, int onset, const float* coefs10n, int n, const float* hz14,
                        PvAmdModulation* out15n) try {
    if (!p || !coefs10n || !out15n || T <= 0 || fs <= 0 || onset < 0 || onset >= T || n < 1 || n > kBandsMax) {
        g_lastError =
            "modulation: PvAmdHostModulation: an impulse response p[T], T > 0, fs > 0, 0 <= onset < T, 1 .. 8 coefficient sets and an "
            "output of n records";
        return -1;
    }
    if (!hz14) hz14 = kModDefaultHz;
    if (const char* e = modulationFreqsError(hz14, fs)) {
        g_lastError = e;
        return -1;
    }
    std::vector<float> tab((size_t)T * kModRowFloats);
    modulationTable(T, fs, hz14, tab.data());
    for (int j = 0; j < n; ++j)
        modulationOfIr(p, T, onset, coefs10n + (size_t)kBandCoefs * j, tab.data(), reinterpret_cast<float*>(out15n) + (size_t)kModFloats * j);
    return 0;
} PV_API_CATCH(-1)

int PvAmdCombineMti(const float* mti, const float* alpha, const float* beta, int n, float* out) try {
    if (!mti || !alpha || !out || n < 1 || n > kBandsMax || (n > 1 && !beta)) {
        g_lastError = "modulation: PvAmdCombineMti: n (1 .. 8) indices and weights alpha, n - 1 weights beta and an output";
        return -1;
    }
    *out = combineMti(mti, alpha, beta, n);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostSpectrumTables(int T, int fs, const float* hz, int n, float* cosTn, float* sinTn) try {
    if (T <= 0 || fs <= 0 || !cosTn || !sinTn) {
        g_lastError = "PvAmdHostSpectrumTables: T > 0, fs > 0 and two tables of T * n floats";
        return -1;
    }
    if (const char* e = spectrumBinsError(hz, n, fs)) {
        g_lastError = e;
        return -1;
    }
    spectrumTables(T, fs, hz, n, cosTn, sinTn);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostSpectrum(const float* p, int T, int fs, int onset, const float* hz, int n, const float* pulseT, float* out3n) try {
    if (!p || !pulseT || !out3n || T <= 0 || fs <= 0 || onset < 0 || onset >= T) {
        g_lastError = "PvAmdHostSpectrum: an impulse response p[T] and a pulse table of T floats, T > 0, fs > 0, 0 <= onset < T and an output of 3 n floats";
        return -1;
    }
    if (const char* e = spectrumBinsError(hz, n, fs)) {
        g_lastError = e;
        return -1;
    }
    std::vector<float> c((size_t)T * n), s((size_t)T * n), src((size_t)3 * n);
    spectrumTables(T, fs, hz, n, c.data(), s.data());
    spectrumSource(pulseT, T, c.data(), s.data(), n, src.data());
    spectrumOfIr(p, T, onset, c.data(), s.data(), n, src.data(), out3n);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostWaterfall(const float* p, int T, int fs, int onset, const float* hz, int n, float sliceSeconds, int nSlices, const float* pulseT,
                       float* outF) try {
    if (!p || !pulseT || !outF || T <= 0 || fs <= 0 || onset < 0 || onset >= T) {
        g_lastError = "waterfall: PvAmdHostWaterfall: an impulse response p[T] and a pulse table of T floats, T > 0, fs > 0, 0 <= onset < T and an output of 2 + 2 n + m n floats";
        return -1;
    }
    if (const char* e = waterfallSettingError(hz, n, fs, sliceSeconds, nSlices)) {
        g_lastError = e;
        return -1;
    }
    std::vector<float> c((size_t)T * n), s((size_t)T * n), src((size_t)3 * n);
    spectrumTables(T, fs, hz, n, c.data(), s.data());
    spectrumSource(pulseT, T, c.data(), s.data(), n, src.data());
    waterfallOfIr(p, T, onset, c.data(), s.data(), n, waterfallSliceSteps(sliceSeconds, fs), nSlices, src.data(), outF);
    return 0;
} PV_API_CATCH(-1)

// source arrays: the taps of one member and the response of one array (pv_arrays.h), as the device computes them
int PvAmdHostArrayTaps(int fs, int T, float gain, float delaySeconds, int interp, int* delay4, float* w4) try {
    if (!delay4 || !w4) {
        g_lastError = "arrays: PvAmdHostArrayTaps: room for four delays and four weights";
        return -1;
    }
    const char* why = nullptr;
    const int n = arrayTaps(fs, T, gain, delaySeconds, interp, delay4, w4, &why);
    if (n < 0) g_lastError = why;
    return n;
} PV_API_CATCH(-1)

int PvAmdHostArrayResponse(const float* pMT, int M, int T, const int* tapMember, const int* tapDelay, const float* tapWeight, int nTaps,
                           float* outT, float* onset) try {
    if (!pMT || !outT || M < 1 || T < 1 || nTaps < 0 || (nTaps > 0 && (!tapMember || !tapDelay || !tapWeight))) {
        g_lastError = "arrays: PvAmdHostArrayResponse: member responses pMT[M][T], M > 0, T > 0, nTaps taps and an output of T floats";
        return -1;
    }
    std::vector<ArrayTap> taps((size_t)nTaps);
    for (int k = 0; k < nTaps; ++k) {
        if (tapMember[k] < 0 || tapMember[k] >= M) {
            g_lastError = "arrays: PvAmdHostArrayResponse: a tap of a member outside 0 .. M - 1";
            return -1;
        }
        taps[(size_t)k] = ArrayTap{tapMember[k], tapDelay[k], tapWeight[k], 0};
    }
    const float on = arrayResponse(pMT, T, taps.data(), nTaps, outT);
    if (onset) *onset = on;
    return 0;
} PV_API_CATCH(-1)

// auralisation: the tables, one response and one output (pv_aural.h), as the device computes them
int PvAmdHostAuralTaps(int fsSigned, int T, int rate, int zeroCrossings, float beta, int* first, float* w, int capN, int* L, int* K) try {
    int l = 0, k = 0;
    const unsigned fs = fsSigned < 1 ? 0u : (unsigned)fsSigned;  // (0: refused below)
    if (const char* e = auralShape(fs, T, rate, zeroCrossings, beta, &l, &k)) {
        g_lastError = e;
        return -1;
    }
    if (L) *L = l;
    if (K) *K = k;
    if (!first && !w) return 0;  // (the shape alone)
    if (!first || !w || capN < l) {
        g_lastError = "aural: PvAmdHostAuralTaps: room for L first steps and L * K weights (capN >= L), or neither table";
        return -1;
    }
    auralTaps(fs, rate, zeroCrossings, beta, l, k, first, w);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostAuralResample(const float* p, int T, const int* first, const float* w, int L, int K, float* outL) try {
    if (!p || !first || !w || !outL || T < 1 || L < 1 || K < 1 || K > kAuralMaxTaps || (long long)L * K > kAuralMaxTableFloats) {
        g_lastError = "aural: PvAmdHostAuralResample: samples p[T], T > 0, tables first[L] and w[L * K] with 1 <= K <= 1024 and L * K <= 2^24, and an output of L floats";
        return -1;
    }
    auralResample(p, T, first, w, L, K, outL);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostAuralConvolve(const float* h, int L, const float* x, int N, float* outM) try {
    if (!h || !x || !outM || L < 1 || N < 1 || L > (int)kAuralMaxTableFloats || N > kAuralMaxSignalSamples) {
        g_lastError = "aural: PvAmdHostAuralConvolve: a response h[L], 1 <= L <= 2^24, a signal x[N], 1 <= N <= 2^20, and an output of N + L - 1 floats";
        return -1;
    }
    auralConvolve(h, L, x, N, outM);
    return 0;
} PV_API_CATCH(-1)

// the accumulate passes of PvAmdSetZoneMaps restated: the step functions of pv_metrics.h / pv_spectrum.h the kernel applies
int PvAmdHostRoomSumsAdvance(const float* p, int T, int fs, int onset, int tA, int tB, float sums6[6]) try {
    if (!p || !sums6 || T <= 0 || onset < 0 || onset >= T || tA < 0 || tB < tA) {
        g_lastError = "zone maps: PvAmdHostRoomSumsAdvance: an impulse response p[T], T > 0, 0 <= onset < T, a pass 0 <= tA <= tB and six sums";
        return -1;
    }
    static_assert(sizeof(RoomSums) == 6 * sizeof(float), "six floats");
    RoomSums s;
    std::memcpy(&s, sums6, sizeof(s));
    roomSumsAdvance(p, T, fs, onset, tA, tB, &s);
    std::memcpy(sums6, &s, sizeof(s));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostRoomMetricsFromSums(const float sums6[6], int fs, PvAmdRoomMetrics* out) try {
    if (!sums6 || !out) {
        g_lastError = "zone maps: PvAmdHostRoomMetricsFromSums: six sums and an output record";
        return -1;
    }
    RoomSums s;
    std::memcpy(&s, sums6, sizeof(s));
    float v[kRoomMetricFloats];
    roomMetricsDerive(s, fs, &v[0], &v[1], &v[2], &v[3]);
    std::memcpy(v + 4, sums6, 6 * sizeof(float));
    std::memcpy(out, v, sizeof(*out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostSpectrumAdvance(const float* p, int T, int onset, int tA, int tB, const float* cosTn, const float* sinTn, int n, float* reim2n) try {
    if (!p || !cosTn || !sinTn || !reim2n || T <= 0 || onset < 0 || onset >= T || tA < 0 || tB < tA || n < 1 || n > kSpectrumMaxBins) {
        g_lastError = "zone maps: PvAmdHostSpectrumAdvance: an impulse response p[T], tables of T x n floats, T > 0, 0 <= onset < T, a pass 0 <= tA <= tB, "
                      "1 .. 32 bins and 2 n sums";
        return -1;
    }
    spectrumAdvance(p, T, onset, tA, tB, cosTn, sinTn, n, reim2n);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneStats(const float* map, int gx, int gy, int planes, const unsigned char* labels, int nZones, PvAmdZoneStat* out) try {
    if (!map || !out || gx < 1 || gy < 1 || planes < 1 || (long long)gx * gy > INT_MAX) {
        g_lastError = "zone statistics: PvAmdHostZoneStats: a map of gx x gy records of `planes` floats, gx, gy, planes >= 1, and an output of nZones x planes records";
        return -1;
    }
    if (const char* e = zoneLabelsError(labels, (long long)gx * gy, nZones)) {
        g_lastError = e;
        return -1;
    }
    static_assert(sizeof(PvAmdZoneStat) == sizeof(ZoneStat), "64 bytes");
    zoneStatsOfMap(map, gx, gy, planes, labels, nZones, reinterpret_cast<ZoneStat*>(out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneDecay(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels, int nZones,
                       int align, PvAmdZoneDecay* out, double* etc, double* edc) try {
    if (!p || !delay || !out || gx < 1 || gy < 1 || T < 1 || fs < 1 || (long long)gx * gy > INT_MAX) {
        g_lastError = "zone decay: PvAmdHostZoneDecay: a history of T planes of gx x gy floats, gx x gy onsets, gx, gy, T, fs >= 1, and an output of nZones records";
        return -1;
    }
    if (!zoneDecayAlign(align)) return -1;
    if (const char* e = zoneLabelsError(labels, (long long)gx * gy, nZones)) {
        g_lastError = std::string("zone decay: ") + (e + sizeof("zone statistics: ") - 1);
        return -1;
    }
    if (const char* e = zoneDecayOnsetsError(delay, labels, (long long)gx * gy, T)) {
        g_lastError = e;
        return -1;
    }
    zoneDecayOfHistory(p, delay, gx, gy, T, fs, labels, nZones, align, reinterpret_cast<ZoneDecay*>(out), etc, edc);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneBandDecay(const float* p, const float* delay, int gx, int gy, int T, int fs, const unsigned char* labels, int nZones,
                           const float* coefs10n, int nBands, int align, PvAmdZoneBandDecay* out, double* etc, double* edc) try {
    if (!p || !delay || !coefs10n || !out || gx < 1 || gy < 1 || T < 1 || fs < 1 || (long long)gx * gy > INT_MAX || nBands < 1 ||
        nBands > kBandsMax) {
        g_lastError =
            "zone band decay: PvAmdHostZoneBandDecay: a history of T planes of gx x gy floats, gx x gy onsets, gx, gy, T, fs >= 1, 1 .. 8 "
            "coefficient sets (PVA_BANDS_MAX), and an output of nZones x nBands records";
        return -1;
    }
    if (!zoneDecayAlign(align, "zone band decay: ")) return -1;
    if (const char* e = zoneLabelsError(labels, (long long)gx * gy, nZones)) {
        g_lastError = std::string("zone band decay: ") + (e + sizeof("zone statistics: ") - 1);
        return -1;
    }
    if (const char* e = zoneDecayOnsetsError(delay, labels, (long long)gx * gy, T)) {
        g_lastError = std::string("zone band decay: ") + (e + sizeof("zone decay: ") - 1);
        return -1;
    }
    zoneBandDecayOfHistory(p, delay, gx, gy, T, fs, labels, nZones, coefs10n, nBands, align, reinterpret_cast<ZoneBandDecay*>(out), etc, edc);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneCurveClarity(const double* etc, int T, int fs, int j0, double out4[4]) try {
    if (!etc || !out4 || T < 1 || fs < 1 || j0 < 0 || j0 >= T) {
        g_lastError = "zone band decay: PvAmdHostZoneCurveClarity: a curve etc[T], T, fs >= 1, 0 <= j0 < T and an output of four doubles";
        return -1;
    }
    zoneCurveClarity(etc, T, fs, j0, out4);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneTiles(const unsigned char* labels, int gx, int gy, int tileRows, int tileCols, unsigned char* flags, int box4[4]) try {
    if (!labels || !flags || !box4 || gx < 1 || gy < 1 || tileRows < 1 || tileCols < 1) {
        g_lastError = "zone curves: PvAmdHostZoneTiles: gx x gy labels, gx, gy, tileRows, tileCols >= 1, ceil(gx / tileRows) x ceil(gy / tileCols) flags and four ints";
        return -1;
    }
    const ZoneTileBox b = zoneTileFlags(labels, gx, gy, tileRows, tileCols, flags);
    box4[0] = b.row0, box4[1] = b.row1, box4[2] = b.blk0, box4[3] = b.blk1;
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneTileUnion(const unsigned char* emitterFlags, const unsigned char* zoneFlags, int ntiles, unsigned char* out) try {
    if (!out || ntiles < 0) {
        g_lastError = "zone curves: PvAmdHostZoneTileUnion: ntiles >= 0 and an output of ntiles bytes";
        return -1;
    }
    zoneTileUnion(emitterFlags, zoneFlags, ntiles, out);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostZoneCurveChunk(int nZones, int rows, long long scratchBytes) try {
    if (nZones < 1 || nZones > kZonesMax || rows < 1 || scratchBytes < 0) {
        g_lastError = "zone curves: PvAmdHostZoneCurveChunk: nZones 1 .. 64, rows >= 1, scratchBytes >= 0";
        return -1;
    }
    return streamZoneCurveChunk(nZones, rows, (size_t)scratchBytes);
} PV_API_CATCH(-1)

int PvAmdHostZoneRects(float dx, int gx, int gy, const float* rect4, int n, unsigned char* labels) try {
    if (!labels || gx < 1 || gy < 1 || n < 0 || n > kZonesMax || (n > 0 && !rect4)) {
        g_lastError = "zone statistics: PvAmdHostZoneRects: gx, gy >= 1, 0 .. 64 rectangles and gx x gy labels";
        return -1;
    }
    zoneLabelsFromRects(dx, gx, gy, rect4, n, labels);
    return 0;
} PV_API_CATCH(-1)

int PvAmdHostCells(float sx, float sy, int res, float x, float z, int* lcx, int* lcy, int* rcx, int* rcy,
                   int* rvalid) try {
    if (res < kLowResolution) return -1;
    const GridSpec g = makeGridSpec(sx, sy, res);
    listenerCell(g, x, z, lcx, lcy);
    int cx = -1, cy = -1;
    *rvalid = resultCell(g, x, z, &cx, &cy) ? 1 : 0;
    *rcx = cx;
    *rcy = cy;
    return 0;
} PV_API_CATCH(-1)

void PvAmdReverbBusGains(float rt60, float wetGain, float* a, float* b, float* c) try {
    reverbBusGains(rt60, wetGain, a, b, c);
} PV_API_CATCH_VOID


#ifndef PVA_HOST_TEST
// ---------------------------------------------------------------------------------------------------------------
// Part 4: baked probe tables (pv_bake.h)
// ---------------------------------------------------------------------------------------------------------------
PvAmdBake* PvAmdBakeCreate(PvAmdSolver* like, int stride, float x0, float z0, float sx, float sz, int nx, int nz) try {
    if (!wholeGrid(like) || !ensure(like)) return nullptr;
    std::unique_ptr<PvAmdBake> h(new PvAmdBake());
    h->b.reset(Bake::create(like->s, stride, x0, z0, sx, sz, nx, nz, &g_lastError));
    return h->b ? h.release() : nullptr;
} PV_API_CATCH(nullptr)

int PvAmdBakeRun(PvAmdBake* b, PvAmdSolver* const* solvers, int n, int rank, int world) try {
    if (!bakeOk(b)) return -1;
    if (!solvers || n < 1) {
        g_lastError = "PvAmdBakeRun: no solvers";
        return -1;
    }
    std::vector<Solver*> sv;
    for (int i = 0; i < n; ++i) {
        PvAmdSolver* h = solvers[i];
        if (h && !h->slabDevices.empty()) {
            g_lastError = "PvAmdBakeRun: solver " + std::to_string(i) + " is a slab group (slab groups cannot bake)";
            return -1;
        }
        if (h && h->opt.slabCount > 1) {
            g_lastError = "PvAmdBakeRun: solver " + std::to_string(i) + " is a slab rank (slab ranks cannot bake)";
            return -1;
        }
        if (!ensure(h)) return -1;
        sv.push_back(h->s);
    }
    return b->b->run(sv.data(), n, rank, world, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdBakeMerge(PvAmdBake* dst, const PvAmdBake* src) try {
    if (!bakeOk(dst) || !bakeOk(src)) return -1;
    return dst->b->merge(*src->b, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

int PvAmdBakeSave(const PvAmdBake* b, const char* path) try {
    if (!bakeOk(b)) return -1;
    if (!path) {
        g_lastError = "PvAmdBakeSave: null path";
        return -1;
    }
    return b->b->save(path, &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)

PvAmdBake* PvAmdBakeLoad(const char* path) try {
    if (!path) {
        g_lastError = "PvAmdBakeLoad: null path";
        return nullptr;
    }
    std::unique_ptr<PvAmdBake> h(new PvAmdBake());
    h->b.reset(Bake::load(path, &g_lastError));
    return h->b ? h.release() : nullptr;
} PV_API_CATCH(nullptr)

void PvAmdBakeDestroy(PvAmdBake* b) try {
    delete b;
} PV_API_CATCH_VOID

int PvAmdBakeGetInfo(const PvAmdBake* b, PvAmdBakeInfo* out) try {
    if (!bakeOk(b) || !out) return -1;
    const BakeHeader& h = b->b->h;
    out->gx = h.gx;
    out->gy = h.gy;
    out->T = h.T;
    out->fs = h.fs;
    out->res = h.res;
    out->dx = h.dx;
    out->stride = h.stride;
    out->x0 = h.x0;
    out->z0 = h.z0;
    out->sx = h.sx;
    out->sz = h.sz;
    out->nx = h.nx;
    out->nz = h.nz;
    b->b->counts(&out->probesBaked, &out->probesInvalid, &out->records);
    out->materialHash = h.materialHash;
    return 0;
} PV_API_CATCH(-1)

int PvAmdBakeProbe(const PvAmdBake* b, int k, int* state5, float* rec9) try {
    if (!bakeOk(b)) return -1;
    if (k < 0 || k >= b->b->probes()) {
        g_lastError = "PvAmdBakeProbe: probe index outside the lattice";
        return -1;
    }
    const int* p = &b->b->probe5[(size_t)5 * k];
    if (state5) std::memcpy(state5, p, 5 * sizeof(int));
    const size_t n = (size_t)p[3] * p[4];
    if (rec9 && n) std::memcpy(rec9, b->b->records(k), n * kBakeRecFloats * 4);
    return (int)n;
} PV_API_CATCH(-1)

int PvAmdBakeQuery(const PvAmdBake* b, const float* listenersXYZ, const float* emittersXYZ, int n, PlaneverbOutput* out) try {
    if (!bakeOk(b)) return -1;
    if (n < 0 || (n > 0 && (!listenersXYZ || !emittersXYZ || !out))) {
        g_lastError = "PvAmdBakeQuery: invalid arguments";
        return -1;
    }
    b->b->query(listenersXYZ, emittersXYZ, n, reinterpret_cast<float*>(out));
    return 0;
} PV_API_CATCH(-1)

int PvAmdBakeQueryDevice(const PvAmdBake* b, int device, const float* listenersXYZ, const float* emittersXYZ, int n,
                         PlaneverbOutput* out) try {
    if (!bakeOk(b)) return -1;
    if (n < 0 || (n > 0 && (!listenersXYZ || !emittersXYZ || !out))) {
        g_lastError = "PvAmdBakeQueryDevice: invalid arguments";
        return -1;
    }
    return b->b->queryDevice(device, listenersXYZ, emittersXYZ, n, reinterpret_cast<float*>(out), &g_lastError) ? 0 : -1;
} PV_API_CATCH(-1)
#endif  // !PVA_HOST_TEST

}  // extern "C"
