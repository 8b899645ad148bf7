// pv_core.h -- host-side grid arithmetic, scene rasteriser and .pv I/O for the MI355X Planeverb solver.
//
// Everything here is index / parameter arithmetic that the reference does on the host in float32 and that must
// be replicated literally: true division where the reference divides, multiplication by the
// reciprocal where it multiplies.  This file is compiled WITHOUT fast-math and with -ffp-contract=off.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace pva {

// reference constants: ProjectPlaneverb/include/PvTypes.h:83-101
constexpr float kC = 343.21f;
constexpr float kAudibleThreshold = 0.00000316f;
constexpr float kDryDirectionLen = 0.005f;
constexpr float kDryGainLen = 0.01f;
constexpr float kWetGainLen = 0.080f;
constexpr float kSqrt2 = 1.4142136f;
constexpr float kPointsPerWavelength = 3.5f;
constexpr float kSchroederOffset = 0.01f;
constexpr float kDistanceGainThreshold = 0.891251f;
constexpr float kDelayCloseThreshold = 5.f;
constexpr float kInvalidDryGain = -1.f;
constexpr int kLowResolution = 275;

struct GridSpec {
    int res = 0;
    float sizeX = 0, sizeY = 0;  // metres
    float dx = 0, dt = 0;
    unsigned fs = 0;
    int T = 0;                   // response length
    float gsx = 0, gsy = 0;      // the reference's float m_gridSize (Grid.cpp:48-49)
    int gx = 0, gy = 0;          // (int)m_gridSize
    int NX = 0, NY = 0;          // cell array = (gx+1) x (gy+1), index x*NY + y (FDTD.cpp:99)
    float courant = 0;           // FDTD.cpp:90
    int nDir = 0, nDry = 0, nWet = 0, nCut = 0;  // Analyzer.cpp:170-171,237,286
    int nFree = 0;               // FreeGrid.cpp:99
};

// Grid.cpp:390-396, Grid.cpp:46-55
GridSpec makeGridSpec(float sizeX, float sizeY, int res);
// same parameters but explicit cell counts (used for the free-field window, FreeGrid.cpp:71-94)
GridSpec makeGridSpecCells(int gx, int gy, int res);
// Grid.cpp:12-27
std::vector<float> gaussianPulse(const GridSpec& g);
// does the host's expf reproduce the reference's pulse table?  (checked once per process, a warning on stderr if not)
bool pulseMatchesReferenceLibm();
void warnIfPulseDiffers();
// FDTD.cpp:97-98 : (int)((pos + offset) / dx)
void listenerCell(const GridSpec& g, float lx, float lz, int* cx, int* cy);
// Analyzer.cpp:200-201 : (int)(pos * (1/dx))
void listenerCellRecip(const GridSpec& g, float lx, float lz, int* cx, int* cy);
// Analyzer.cpp:106-116 ; returns false when the reference returns nullptr (with >= instead of >)
bool resultCell(const GridSpec& g, float ex, float ez, int* cx, int* cy);

struct Box {
    float x, y, w, h, R;  // PvMathTypes.h:31-49 : centre, full extents, absorption parameter
};

// beta / R planes with the reference's rasteriser semantics (Grid.cpp:84-108,136-144,229-296)
class MaterialPlane {
public:
    void init(const GridSpec& g);
    void add(const Box& b);     // Grid::AddAABB
    void remove(const Box& b);  // Grid::RemoveAABB (clears overlaps of other boxes too: SURVEY Q4)
    const std::vector<uint8_t>& beta() const { return beta_; }
    const std::vector<float>& R() const { return R_; }
    // Cell::by (PvTypes.h:113): never read by the solver, but part of the AoS Cell GetImpulseResponse hands out
    const std::vector<uint8_t>& by() const { return by_; }
    // dirty row range [lo, hi) since the last clearDirty(); empty when lo >= hi
    int dirtyLo() const { return dirtyLo_; }
    int dirtyHi() const { return dirtyHi_; }
    void clearDirty();
    void markAllDirty();

private:
    void bounds(const Box& b, int* sx, int* sy, int* ex, int* ey) const;
    GridSpec g_;
    std::vector<uint8_t> beta_, by_;
    std::vector<float> R_;
    int dirtyLo_ = 0, dirtyHi_ = 0;
};

// Shapes (no reference counterpart): convex polygons of 3..kShapeMaxVerts vertices in grid metres (x = grid x, y = grid y),
// counter-clockwise, with an absorption value; rasterised by the cell-centre rule of shapeCovers on top of the AABB layer
// (Solver::applyGeometry, pv_shapes.hip).  Everything here is float32 without contraction, so that a numpy restatement is exact.
constexpr int kShapeMaxVerts = 8;
// Round and concave kinds in the same layer (include/planeverb_amd.h, "Round and concave shapes"): a round shape is a chain of
// n >= 1 points with a radius -- n = 1 a disc, n = 2 a capsule, more a wall path, covered where any of its capsules covers -- and
// a simple polygon is 3..kPolyMaxVerts vertices in either winding under the even-odd crossing rule.
constexpr int kPolyMaxVerts = 64;
enum ShapeKind : int { kShapeConvex = 0, kShapeRound = 1, kShapePolygon = 2 };
// The point list is inline and of the largest size (528 bytes a Shape, 76 before these kinds), also where the live module queues
// a Shape by value beside every change (pv_context.h Change, AABB and grid-edge changes included) and in every table slot: a
// fixed-size record cannot fail to allocate, which keeps the queue's "room first, then push" guarantee under allocation failure
// (tests/host/alloc_fault*.cpp) as simple as it was.  The price is a queue entry about five times the size; the device side has
// the pooled table instead (pv_shapes.h).
struct Shape {
    int kind = kShapeConvex;
    int n = 0;
    float xy[2 * kPolyMaxVerts] = {};  // (a convex shape uses the first kShapeMaxVerts)
    float R = 0.f;
    float r = 0.f;                     // radius of a round shape
};
// validates (finite coordinates and absorption, 3..8 vertices, non-zero area, convex and simple) and orders the list
// counter-clockwise; false + *err on a refusal
bool makeShape(const float* xy, int n, float R, Shape* out, std::string* err);
// a disc / capsule / wall path: finite points and absorption, 1..kPolyMaxVerts points, finite radius > 0, every segment's
// float32 squared length finite; false + *err on a refusal
bool makeRound(const float* xy, int n, float radius, float R, Shape* out, std::string* err);
// a simple polygon: finite vertices and absorption, 3..kPolyMaxVerts vertices, non-zero area, no two edges with a point in
// common other than the vertex two neighbours share (polygonSelfIntersects); the list is kept as given
bool makePolygon(const float* xy, int n, float R, Shape* out, std::string* err);
// O(n^2), in double: a zero-length edge; neighbours that fold back onto each other (o = 0 and (p - v) . (q - v) > 0 at their
// shared vertex v); or two other edges p1p2, p3p4 that cross (o(p3,p4,p1), o(p3,p4,p2) of opposite strict signs and
// o(p1,p2,p3), o(p1,p2,p4) too) or touch (some o = 0 with that point inside the other edge's bounding box), where
// o(p, q, r) = (q.x - p.x) (r.y - p.y) - (q.y - p.y) (r.x - p.x)
bool polygonSelfIntersects(const float* xy, int n);
// the 4 vertices of an oriented box: centre (px, py), full width w along the axis (ax, ay) (any non-zero length), full
// height h along its left normal; counter-clockwise.  false + *err for a zero or non-finite axis or a non-finite input.
bool orientedBoxVertices(float px, float py, float w, float h, float ax, float ay, float out8[8], std::string* err);
// is the centre of cell (x, y) inside the shape?  ((float)x + 0.5f) * dx etc.; convex: every edge a -> b: e.x (P.y - a.y) - e.y (P.x - a.x) >= 0;
// round and polygon: the rules of include/planeverb_amd.h, restated in pv_core.cpp and pv_shapes.hip
bool shapeCovers(const Shape& s, float dx, int x, int y);
// cells [*x0, *x1) x [*y0, *y1) that contain every cell shapeCovers can accept (padded for the rounding of the edge
// function), clipped to the grid's cells 0 <= x < gx, 0 <= y < gy (never the ghost row / column); empty when x0 >= x1 or y0 >= y1
void shapeCellBounds(const Shape& s, const GridSpec& g, int* x0, int* x1, int* y0, int* y1);

// Triangle meshes (include/planeverb_amd.h, "Triangle meshes"; no reference counterpart): sliced at the solver's height and
// rasterised on the device (pv_mesh.h) between the AABB layer and the shape layer.  These are the host's parts: validation, the
// closedness check of a solid mesh and the CPU restatement of slice and coverage -- float32 without contraction, as the kernels.
constexpr int kMeshMax = 64;
constexpr int kMeshMaxTris = 1 << 20;
constexpr int kMeshMaxTrisTotal = 1 << 22;
enum MeshMode : int { kMeshSolid = 0, kMeshShell = 1 };
// finite vertices, absorption and (shell) radius with a finite non-zero float32 square; 1 <= nt <= kMeshMaxTris; indices inside
// [0, nv) and distinct within a triangle; solid: every undirected edge shared by exactly two triangles (a hash over the edges)
bool validateMesh(const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius, std::string* err);
bool validateMeshTransform(const float* m12, std::string* err);
// the section of every triangle at height h: out4[4 i ..] = (a.x, a.z, b.x, b.z) and valid[i] = 1, or valid[i] = 0 and zeros.
// m12 = nullptr: no transform.
void meshSection(const float* verts, const int* tris, int nt, const float* m12, float h, float* out4, uint8_t* valid);
// coverage of the section's segments over the grid's cells (cover[x * NY + y] = 0 / 1, the ghost row and column never): solid by
// the marks-and-suffix-XOR form of the even-odd rule, shell by the capsule rule over each segment's cell bounds
void meshCoverage(const GridSpec& g, const float* seg4, const uint8_t* valid, int nt, int mode, float radius, uint8_t* cover);
// how many cells x in [0, gx) have ((float)x + 0.5f) * dx < xi: the cells one crossing toggles are the prefix [0, k)
int meshCrossingPrefix(float xi, float dx, int gx);

// Graded absorbing layers at the grid edges (pv_layer.h: the model and the layer kernel)
constexpr int kEdgeLayerMaxWidth = 64;
constexpr int kEdgeLayerMinInterior = 8;  // cells between two opposite layers (or a layer and the far edge)
constexpr int kEdgeLayerDefaultWidth = 24;
// the grading rule's design reflection: s_max = (m + 1) * C * ln(1 / R0) / (4 w), m = 2 (tuned by tests/test_host_layer.py)
constexpr double kEdgeLayerR0 = 0.1;
// the split-field model's default design reflection (PVA_EDGE_LAYER_SPLIT_R0; the sweep: profiles/edge_layer.txt)
constexpr double kEdgeLayerSplitR0 = 1e-4;

// The tables of a gx x gy grid (cell array (gx + 1) x (gy + 1)), into out[4 (gx + 1) + 4 (gy + 1)] in this order:
//   apx[gx + 1], bpx[gx + 1], ax[gx + 1], bx[gx + 1], apy[gy + 1], bpy[gy + 1], ay[gy + 1], by[gy + 1]
// For a damping value s: a = (1 - s) / (1 + s), b = 1 / (1 + s), in double, rounded to float.  Cells sit at half depths and
// velocity faces at whole depths: along x with a layer of width w on side 0, face x (between cells x - 1 and x) has depth
// w - x for x <= w and cell x has depth w - x - 1/2 for x < w; on side 1, face x has depth x - (gx - w) for x >= gx - w and
// cell x depth x + 1/2 - (gx - w) for gx - w <= x < gx.  s = s_max (depth / w)^2, 0 outside the layers (depth <= 0, the
// ghost cell x = gx included); y likewise with sides 2 and 3.  courant = the grid's Courant number (GridSpec::courant); r0 =
// the design reflection R0 in s_max (kEdgeLayerR0 for the unsplit model, 0 < r0 < 1).
void edgeLayerTables(int gx, int gy, float courant, const int w4[4], float* out, double r0 = kEdgeLayerR0);
// is r0 a design reflection the split model accepts (finite, 0 < r0 < 1)?
inline bool edgeLayerR0Ok(double r0) { return r0 > 0.0 && r0 < 1.0; }
// why w4 is refused for a gx x gy grid ("" = accepted)
const char* edgeLayerRefusal(int gx, int gy, const int w4[4]);

// .pv scene files: PlaneverbSandbox/src/Editor/Editor.cpp:219-281
bool loadPv(const std::string& path, std::vector<Box>* out, std::string* err);
bool savePv(const std::string& path, const std::vector<std::pair<int, Box>>& boxes, std::string* err);

// PlaneverbDSP/src/PvDSPContext.cpp:165-228
void reverbBusGains(float rt60, float wet, float* a, float* b, float* c);

// Row-streaming air segments (pv_seg.h, PVA_OPT_STREAM_ROWS): cover every tile with air[ti * nty + tj] != 0 by exactly
// one segment.  Tile rows are cut into maximal runs of air tiles and those into chunks of <= wmax tile columns; identical
// chunks of consecutive tile rows form a rectangle; rectangles are cut into pieces of about equal height -- ROW-granular,
// not tile-granular -- of about (total rows / target) rows, at most 7 * rxi (a segment may touch 8 tile rows).  Sorted by
// (first row, tile column).  Pure index arithmetic (no reference counterpart).
struct SegRect {
    int row0, nrows, tj0, w;  // array rows [row0, row0 + nrows) x tile columns [tj0, tj0 + w)
};
std::vector<SegRect> planSegments(const uint8_t* air, int ntx, int nty, int rxi, int wmax, int target);

// Enclosure of a cell (resident-window runs, Solver::windowFor): the 4-connected component of air cells (beta != 0) that
// holds the seed, as long as the TILE WINDOW around it stays small.  beta: NX x NY cells, index x * NY + y.  The window is
// the component's bounding box grown by one cell on every side, clipped to the grid and rounded out to rxi x wi-cell tiles
// (tile (ti, tj) = rows [ti rxi, +rxi) x columns [tj wi, +wi)).  The fill gives up -- found = 0 -- as soon as that window
// holds more than maxTiles tiles, so it visits at most maxTiles * rxi * wi cells whatever the grid's size; a seed outside
// the grid or inside a wall gives found = 0 with no cell visited.
// Why the window bounds a run exactly: the pressure of a non-air cell is identically 0 (beta = 0, FDTD.cpp:139); the face
// between two non-air cells has coefficient 0; the face between a wall cell and an air cell of ANOTHER component multiplies
// two pressures that are both zero for the whole run.  In a run whose pulse enters at the seed, non-zero values therefore live
// only in the component's pressures and in the faces that touch a component cell -- face (x, y) lies between cells (x - 1, y)
// and (x, y), so those are cell indices [min, max + 1] of the bounding box: inside the one-cell ring.  Grid edges need no
// special case: they are ordinary face coefficients.
struct Enclosure {
    int found;            // 1: the component was walked completely and its window holds <= maxTiles tiles
    int cells;            // cells visited (found: the component's size)
    int r0, c0, r1, c1;   // inclusive bounding box of the visited cells
    int ti0, tj0, tis, tjs;  // the tile window (of the visited cells' box: meaningful when found)
};
// visited (optional): the visited cells' indices, ascending
Enclosure findEnclosure(const uint8_t* beta, int NX, int NY, int seedX, int seedY, int rxi, int wi, int maxTiles,
                        std::vector<int>* visited);

// What a reach-eligible run (RunPlan::reach: the reach-bounded launches or a resident-window run) clears in front of its first
// launch (Solver::clearReachPlanes).  Such a run writes only inside its tile rectangle, so both buffer sets must hold zeros
// everywhere else; prevRect = {first tile row, tile rows, first tile column, tile columns} is the only place the previous such run
// left values, and the flags say that something else wrote the planes since (planesDirty: a geometry change, setFields, raw stepping;
// sweptDirty: a run of a sweeping path).  A WINDOW run over the very rectangle of the previous run needs no clear at all: the
// resident kernel starts from zero registers, loads nothing in its first epoch, and every later epoch reads only what the epoch
// before published -- the blocks' interiors tile the window exactly, so a stale value inside it is overwritten before anything
// reads it, in either buffer set and for every step count (pv_resident.hip).  The reach-bounded launches load their tiles from the
// first launch on, and the split planes (an edge layer's, splitPlanes) are not the resident kernel's to overwrite.
//   None: no launch.  Rect: prevRect, in all planes (an empty one: nothing to clear).  All: every plane, whole.
enum class PlaneClear { None = 0, Rect = 1, All = 2 };
PlaneClear planClear(bool windowRun, const int win[4], const int prevRect[4], bool planesDirty, bool sweptDirty, bool splitPlanes);

// ----------------------------------------------------------------------------------------------------------------
// Which path a run takes ("Which path a run takes").  Solver::init resolves a PathCaps once, every run head
// (Solver::beginRun) states a PathRun, and planRun -- pure, no device -- answers with the RunPlan the solver keeps for the
// run in flight.  What needs the device or a counter shared between solvers (the resident budgets, the enclosure lookup, a
// lost graph capture) is applied to the plan afterwards as a demotion to RunPlan::fallback.  Every path computes the same
// bits, so no parity test notices a run on the wrong one: tests/test_host_run_plan.py checks this function instead.
// ----------------------------------------------------------------------------------------------------------------
struct PathCaps {
    // the tile configuration's answers (pv_launch.h)
    bool stacked = false;       // stepConfigStacked
    bool mergedOk = false;      // mergedConfigOk
    bool smallFits = false;     // smallGridFits: the whole grid fits one CU's LDS
    // the options as resolved by init (SolverOptions)
    int useGraph = 0;           // 0 = auto, 1 = always, 2 = never
    int smallGrid = 0;          // 0 = auto, 1 = whenever it fits, 2 = never
    int resident = 0;           // 0 = auto, 1 = also beside the small-grid kernel / with an explicit tile, 2 = never
    int merged = 1;
    int reachBound = -1;        // 0 = full sweeps
    int timeKernels = 0;
    bool streaming = false, denseHistory = false, edgeTiles = false;
    bool explicitTile = false;  // K or rxi given by the caller (any non-zero value)
    // the solver
    bool slab = false;
    int ntiles = 0;
    long long cells = 0;        // NX * NY array cells
    int bands = 1;              // row bands (1 = none)
    bool wholeWindow = false;   // the history window is the whole grid
    // the forms init resolved from all of the above, the device's occupancy answers and the plane size
    bool useSeg = false, usePatch = false, windowOk = false;
    bool useResident = false;   // NOT fixed at init like the rest: Solver::sync() clears it for good when a resident run was given up
};

struct PathRun {
    enum Kind { Run, Raw, Shared };  // a run of this solver alone; raw stepping (runSteps); a member of a batch or a slab group,
    Kind kind = Run;                 // whose caller drives the launches: full sweeps, plain launches
    bool listenerInside = false;     // the pulse enters inside the grid
    bool layerActive = false;        // an edge layer is set ...
    bool layerTiles = false;         // ... and has tiles (numLayer > 0)
    bool windowOff = false;          // a window run was given up on this geometry
    bool segmentsFound = true;       // false: the run's segment plan came out empty (known once prepareDyn has made it)
};

enum class StepPath { Streaming, Window, Resident, SmallGrid, Graph, Launches };

struct RunPlan {
    StepPath path = StepPath::Launches;
    // what the run goes out as when the device says no: Window -> the reach-bounded launches (no enclosure, budget used up, a
    // workgroup gave up), Resident -> the small-grid kernel / the replayed graph / launches (budget used up), Graph -> launches
    // (the capture was lost); = path where nothing can say no
    StepPath fallback = StepPath::Launches;
    // the launch form of enqueueSteps
    bool oneLaunch = false;    // the sweep is one launch per K steps on one stream (else the air kernel, beside the general kernel
                               // on a second stream where general tiles exist)
    bool plainMerged = false;  // ... and it is the plain merged kernel of an unstacked tile: what reach, bands and patch require
    bool banded = false;       // per-band run parameters and lists; the sweep = one launch per row band
    bool segments = false;     // row-streaming air segments
    bool patch = false;        // air tiles by the persistent patch kernel
    bool reach = false;        // only the tiles the pulse can have reached (Window: the planes are cleared as for such a run)
    bool layer = false;        // the layer launch behind every merged launch
    PathRun::Kind kind = PathRun::Run;
    bool oneXcd = false;       // Resident, Window: the one-XCD hand-off (set by the solver: it needs the XCD's budget)
};

// "the plain merged path": what the patch kernel, row bands and the reach bound require
inline bool plainMergedLaunch(const PathCaps& c) { return !c.stacked && c.merged == 1 && c.mergedOk; }
RunPlan planRun(const PathCaps& c, const PathRun& r);

}  // namespace pva
