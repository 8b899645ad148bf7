// pv_launch.h -- host-callable launchers and configuration queries of the kernel translation units (the .hip files of this
// directory that the host code calls into), grouped by the file that implements them
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "pv_device.h"

namespace pva {

// ---- pv_kernels.hip: the stencil
// supported (K steps per launch, interior rows per tile) instantiations of the fused stencil
bool stepConfigSupported(int K, int rxi);
bool mergedConfigOk(int K, int rxi);
// stacked tiles (W waves share one tall tile): always one merged launch; their blocks load
// stepConfigExtraRows() rows beyond rxi + 2K at the bottom, which the guard band must cover
bool stepConfigStacked(int K, int rxi);
int stepConfigExtraRows(int K, int rxi);
// which: bit 0 = air-tile kernel, bit 1 = general-tile kernel (both write disjoint tiles of the same planes);
// 4 = both in ONE merged launch (one block per general tile first, then the air tiles)
// The general kernel goes to stream2 when given (the caller orders the two streams with events).
void launchStep(int K, int rxi, const StepArgs& a, hipStream_t stream, int which = 3, hipStream_t stream2 = nullptr);
// which = 4 | kStepGeneralPacked: the merged launch whose general-tile arm is the packed one also at K = 12 (scenes with many wall tiles)
constexpr int kStepGeneralPacked = 32;
// persistent patch kernel (pv_patch.h): the AIR tiles of one sweep by `blocks` resident workgroups (one per CU, multiple
// of 8); the general tiles of the sweep are launched with launchStep(..., which = 16)
bool patchConfigOk(int K, int rxi);
void launchStepPatch(int K, int rxi, const StepArgs& a, int blocks, hipStream_t stream);
// sparse-emitter mode with the forward sums inside the stencil (pv_stream.h): per K-step launch the classify pass, the merged
// launch with the per-launch tile classes, and the open half tiles
bool openConfigOk(int K, int rxi);
bool unpackedAirOk();
void launchStreamClassify(const ClassifyArgs& c, hipStream_t stream);
void launchStreamIdle(const ClassifyArgs& c, int* idleHost, hipStream_t stream);
void launchStepOpen(int K, int rxi, const StepArgs& a, const OpenArgs& o, hipStream_t stream);
// row-streaming air segments (pv_seg.h): columns per lane of the configuration's segment kernel (0 = it has none), the
// tile columns a segment can span, and the launch (general tiles + a.numSeg segments in one grid)
int segConfigColumns(int K, int rxi);
int segConfigMaxTileColumns(int K, int rxi);
void launchStepSeg(int K, int rxi, const StepArgs& a, hipStream_t stream);
// batched merged launch: ba.n runs (blockIdx.y) of identically configured solvers in one grid; only for
// batchConfigOk() configurations
bool batchConfigOk(int K, int rxi);
bool edgeConfigOk(int K, int rxi);  // the batched kernel of this configuration has the edge-tile arm (tile class 2)
void launchBatch(int K, int rxi, const BatchArgs& ba, hipStream_t stream);
// tile classes: 0 air, 1 general (also appended to `list`), 2 edge tile (only when allowEdge and the configuration
// has the mirror-pair air tile)
void launchTileClass(int K, int rxi, const FaceCoef* coef, uint8_t* tileClass, int* list, int* count,
                     const Geometry& g, hipStream_t stream, bool allowEdge);
// dead tiles (all-wall interior): dead[tile] = 1, *count += number of them
void launchTileDead(const FaceCoef* coef, uint8_t* dead, int* count, const Geometry& g, int K, hipStream_t stream);
void launchCoefs(const float* mat, FaceCoef* coef, const Geometry& g, hipStream_t stream);
void launchLaneSelfTest(float* out128, hipStream_t stream);

// ---- pv_resident.hip: a walled-in room's run as one launch
// resident kernel (pv_resident.hip): one launch per run; a.ntiles workgroups that must all be co-resident
bool residentConfigOk(int K, int rxi);
int residentExtraRows(int K, int rxi);   // rows its blocks load beyond rxi + 2K at the bottom
int residentMaxBlocks(int K, int rxi, int device);
void launchResident(int K, int rxi, const ResidentArgs& a, hipStream_t stream);
#ifdef PV_RESIDENT_TRACE
void residentDumpTrace();  // development builds: the phase stamps of the last launch to stderr
#endif

// ---- pv_probe.hip: queue / clock / bandwidth probes, the run's status words
// do the two (idle) streams share a hardware queue?  stamps = 4 words of pinned host memory (pv_probe.hip)
bool streamsShareQueue(hipStream_t a, hipStream_t b, unsigned long long* stamps);
// shader clock of the moment (pv_probe.hip): MHz by a timed s_sleep, or 0
float clockProbeMHz(int device, float* byMemtime);
// the device's own streaming bandwidth in GB/s: {copy 16 B per lane, copy 4 B per lane, read only, write only} (pv_probe.hip)
bool bandwidthProbeGBs(int device, float out[4]);
// one form of pv_libm.h per input (pv_probe.hip; PVA_LIBM_* of include/planeverb_amd.h): on the current device with the analysis
// kernels' LDS tables, or the same header on the host
enum LibmForm {
    kLibmLog10 = 0,         // pvLog10f
    kLibmLog10NonNeg,       // pvLog10fNonNeg
    kLibmLog10NonNegTab,    // pvLog10fNonNegT<LogTabLds>
    kLibmLog10NormalTab,    // pvLog10fNormalT<LogTabLds>      (normal positive inputs only)
    kLibmLog10NormalBatch,  // pvLog10fNormalBatch<LogTabLds>  (likewise)
    kLibmPow08,             // pvPowf(x, 0.8f)
    kLibmPow23,             // pvPowf(x, (float)(2.0 / 3.0))
    kLibmPowNonNeg08,       // pvPowfNonNeg(x, 0.8f)
    kLibmPowNonNeg23,
    kLibmPowNonNegTab08,    // pvPowfNonNegT<PowTabLds>(x, 0.8f)
    kLibmPowNonNegTab23,
    kLibmForms
};
bool libmProbe(int form, const float* in, float* out, long long n, bool onDevice, std::string* err);
// error flag, {cells of non-zero tiles, cells with an onset}, resident claim counter (or NULL) -> 4 ints of pinned host memory
void launchRunStatus(int* err, int* counts, const unsigned* claims, int* outHost, hipStream_t stream);

// ---- pv_run.hip: start of a run, zeroing, the small grids' one-workgroup kernel
// cells = NX*NY must satisfy smallGridFits()
bool smallGridFits(int NX, int NY);
void launchSmallGrid(const SmallArgs& a, hipStream_t stream);
void launchZero(float* p, long long n, hipStream_t stream);
// rows [r0, r0 + nr) x columns [c0, c0 + nc) of six padded planes set to zero (reach-bounded runs: Solver::clearReachPlanes)
struct ZeroRectArgs {
    float* p[6];
    int pitch, r0, nr, c0, nc;
};
void launchZeroRect(const ZeroRectArgs& z, hipStream_t stream);
void launchBeginRun(const BeginArgs& a, hipStream_t stream);

// ---- pv_analysis.hip: impulse-response analysis, one pass per launch, and its streaming form
void launchAnalysis(const AnalyzeArgs& a, hipStream_t stream);
// the three phases of launchAnalysis separately (slab groups run the middle one per slab, the others on the whole map)
void launchFarCells(const AnalyzeArgs& a, hipStream_t stream);
void launchAnalysisFar(const AnalyzeArgs& a, hipStream_t stream);  // launchAnalysis' first pass (the lazy far frame, or every far cell)
void launchAnalysisCells(const AnalyzeArgs& a, hipStream_t stream);  // = the three below, one after the other
void launchOnset(const AnalyzeArgs& a, hipStream_t stream);   // onsets of the window's cells into the delay map
void launchEncode(const AnalyzeArgs& a, hipStream_t stream);  // dry gain, source direction, low-pass (reads the onsets)
void launchRt60(const AnalyzeArgs& a, hipStream_t stream);    // wet gain, decay time (reads the onsets)
void launchAnalysisDirection(const AnalyzeArgs& a, hipStream_t stream);
// direction planes of the far cells, for whole-map read-backs; delay plane = "no onset" everywhere (solver creation)
void launchFarDirections(float* res, long long n, const FarInfo& far, hipStream_t stream);
void launchFillDelay(float* delay, long long n, hipStream_t stream);
// (zc: the zones' curves of the pass's steps behind its onsets -- launchStreamZoneCurves below --, nullptr: none)
// (zm: the labelled cells' room-metrics / spectrum sums of the pass's steps, likewise behind its onsets -- launchStreamZoneMaps
// below, with the pass's tA / tB --, nullptr: no map kind selected)
struct ZoneRingCurveArgs;
struct ZoneMapArgs;
struct ZoneMapSpecSlice;
void launchStreamAccum(const AnalyzeArgs& a, const uint8_t* hasEmitter, uint8_t* tileOpen, int ntiles,
                       hipStream_t stream, const ZoneRingCurveArgs* zc = nullptr, int zcChunk = 0, const ZoneMapArgs* zm = nullptr,
                       const ZoneMapSpecSlice* zmSlices = nullptr, int zmSliceCount = 0);
void launchStreamFinalize(const AnalyzeArgs& a, hipStream_t stream);

// ---- pv_rt60.hip: wet gain and decay time; results carried over from another solver
// no-onset cells of the window and of the block [srcR0, +srcNR) x [srcC0, +srcNC) (the other solver's last window; srcNR = 0:
// none) take the six persistent result planes (occlusion, wet gain, decay time, lowpass, source direction x / y) from another
// solver's maps (pv_rt60.hip; Solver::run's carryFrom)
void launchCarryResults(const AnalyzeArgs& a, const float* srcOut, int srcR0, int srcC0, int srcNR, int srcNC, hipStream_t stream);
// wet gain + decay time (pv_rt60.hip): sixteen / four lanes per cell in one launch, the lane-per-cell form in a second one where
// AnalyzeArgs::rt60Tile announces it; the form is chosen on the device
void launchRt60Forms(const AnalyzeArgs& a, hipStream_t stream);

// ---- pv_fused.hip: the analysis as one launch (experimental build), the last kernel of a run
// the whole analysis of a grid whose history window is the grid, in one launch (pv_fused.hip); fusedAnalysisOk: its phase
// counters fit; launchRunFinish: a run's output queries + status words in one launch (last kernel of a run)
bool fusedAnalysisBuilt();  // false in the product build: the arm lives in the experimental build only
bool fusedAnalysisOk(const AnalyzeArgs& a);
void launchAnalysisFused(const FusedArgs& f, hipStream_t stream);
// (zeroWords / nZero: words to clear behind everything else -- the resident kernel's flags, for the next run; with them the error flag)
void launchRunFinish(const float* res, long long n, const long long* cellsHost, int nq, float* outHost, const FarInfo& far,
                     int* err, int* counts, const unsigned* claims, int* statusHost, unsigned* zeroWords, int nZero,
                     unsigned long long* stamp, hipStream_t stream);

// ---- pv_metrics.hip: room-acoustic metrics
// room metrics of the last completed run (pv_metrics.hip): out = kRoomMetricFloats planes of a.histPlane floats, indexed by the
// cell's offset inside a history plane; NaN where the cell has no onset in that run
void launchRoomMetrics(const AnalyzeArgs& a, float* out, hipStream_t stream);

// ---- pv_zones.hip: per-zone statistics of a computed map
// the records (pv_zones.h ZoneStat, without std and the empty-zone values: zoneStatFinish) of one chunk of a map's planes for the
// zones of a.labels: four launches, a.rows / a.rowM2 are scratch
struct ZoneArgs;
void launchZoneStats(const ZoneArgs& a, hipStream_t stream);

// ---- pv_zone_decay.hip: per-zone ensemble decay curves
// launchZoneMembers: members, smallest and largest onset of every zone into a.members (a.memberRows is scratch; of the window, the
// onset map and the labels alone).  launchZoneCurves: etc of the chunk of slots a.slot0 .. a.slot0 + a.slots - 1 of every zone into
// a.etc off the kept history (pv_zone_decay.h; a.rows is scratch), slot j = t (onset false) or t - t0 (true)
struct ZoneCurveArgs;
void launchZoneMembers(const ZoneCurveArgs& a, hipStream_t stream);
void launchZoneCurves(const ZoneCurveArgs& a, bool onset, hipStream_t stream);
// sparse-emitter mode: steps [tA, min(tB, T)) of every zone's ABSOLUTE curve into a.c.etc (nZones x T), off the ring, in chunks of
// `chunk` steps (pv_zone_decay.h streamZoneCurveChunk; a.c.slot0 / a.c.slots are the launcher's; a.c.rows is scratch)
void launchStreamZoneCurves(const ZoneRingCurveArgs& a, int tA, int tB, int chunk, hipStream_t stream);

// ---- pv_zone_maps.hip: sparse-emitter mode, the room-metrics and spectrum records of the labelled cells inside the run
// launchStreamZoneMaps: the sums of the steps [a.tA, min(a.tB, a.T)) into the records' own planes (pv_zone_maps.h), one launch for
// the room metrics and one per slice of the bins; launchStreamZoneMapsFinish: the derived planes, NaN where a labelled cell has no
// onset -- behind the finalize pass.  Neither launches anything without a labelled tile
void launchStreamZoneMaps(const ZoneMapArgs& a, const ZoneMapSpecSlice* slices, int nSlices, hipStream_t stream);
void launchStreamZoneMapsFinish(const ZoneMapArgs& a, hipStream_t stream);

// ---- pv_zone_band_decay.hip: per-zone ensemble decay curves per band
// etc of one chunk of (zone, band) pairs -- zones a.zone0 + 1 .. a.zone0 + a.zones, bands a.band0 .. a.band0 + a.bands - 1 -- into
// a.c.etc (nZones x nBands x T; pv_zone_band_decay.h); a.c.rows = a.zones x a.bands x gx x T doubles of scratch the caller has
// cleared to +0.0; slot j = t (onset false) or t - t0 (true).  The members are launchZoneMembers'
struct ZoneBandCurveArgs;
void launchZoneBandCurves(const ZoneBandCurveArgs& a, bool onset, hipStream_t stream);

// ---- pv_decay.hip: per-cell decay times
// decay times (EDT, T20, T30) of the last completed run (pv_decay.hip): out = kDecayFloats planes of a.histPlane floats, indexed
// by the cell's offset inside a history plane; NaN where the cell has no onset in that run.  twoLaunches: the two walks of the
// curve as a launch each (measurement; the records are the same bits)
void launchDecayTimes(const AnalyzeArgs& a, float* out, bool twoLaunches, hipStream_t stream);

// ---- pv_lateral.hip: per-cell lateral energy fraction and early-sound direction
// lateral-fraction records of the last completed run (pv_lateral.hip): out = kLateralFloats planes of a.histPlane floats, indexed
// by the cell's offset inside a history plane; NaN where the cell has no onset in that run.  Whole-grid solvers only (the pass
// does not read a slab's histAbove)
void launchLateralFraction(const AnalyzeArgs& a, float* out, hipStream_t stream);

// ---- pv_echogram.hip: per-cell directional echogram
// echogram records of the last completed run (pv_echogram.hip) for nSlots slots (1 .. kEchogramMaxSlots) of ns >= 1 steps:
// out = 1 + 3 nSlots planes of a.histPlane floats (n, then e, ix, iy of slot j at planes 1 + 3 j ..), indexed by the cell's
// offset inside a history plane; NaN where the cell has no onset in that run.  Whole-grid solvers only, as the lateral fraction
void launchEchogram(const AnalyzeArgs& a, float* out, int ns, int nSlots, hipStream_t stream);

// ---- pv_lobes.hip: per-cell directional energy lobes
// lobe records of the last completed run (pv_lobes.hip) for nW windows (1 .. kLobesMaxWindows) whose nW - 1 edges in steps are
// ed.n[0 .. nW - 2], strictly increasing, the other entries INT_MAX (pv_lobes.h lobesEdgeSteps): out = 1 + 5 nW planes of
// a.histPlane floats (n, then E, XP, XN, YP, YN of window j at planes 1 + 5 j ..), indexed by the cell's offset inside a history
// plane; NaN where the cell has no onset in that run.  Whole-grid solvers only, as the echogram
struct LobeEdges;
void launchLobes(const AnalyzeArgs& a, float* out, const LobeEdges& ed, int nW, hipStream_t stream);

// ---- pv_query_records.hip: the record kinds above for the cells of the registered output queries, inside the run
// one launch (one wave per selected kind, lane i = query i) that writes q.nq records per selected kind straight into pinned host
// memory (pv_query_records.h); the records are bit for bit the whole-map passes' at the same cells
struct QueryRecordArgs;
void launchQueryRecords(const AnalyzeArgs& a, const QueryRecordArgs& q, hipStream_t stream);
// ---- pv_query_spectral.hip: band metrics, modulation and spectrum (below) for the same cells, inside the run, with a launch of
// their own: one wave per work item (a block of bands, a band, a slice of bins) and per 64 queries (pv_query_spectral.h)
struct QuerySpectralArgs;
void launchQuerySpectral(const AnalyzeArgs& a, const QuerySpectralArgs& q, hipStream_t stream);

// ---- pv_bands.hip: per-cell, per-band decay times and clarity
// band records of the last completed run (pv_bands.hip) for n bands: coefs = n x kBandCoefs floats on the HOST (they travel as
// kernel arguments), out = n x kBandFloats planes of a.histPlane floats (band j, float k at plane j * kBandFloats + k), indexed by
// the cell's offset inside a history plane; NaN where the cell has no onset in that run.  One launch per block of
// bandMetricsBlock() bands
void launchBandMetrics(const AnalyzeArgs& a, const float* coefs, int n, float* out, hipStream_t stream);
int bandMetricsBlock();

// ---- pv_modulation.hip: per-cell, per-band modulation transfer function and index
// modulation records of the last completed run (pv_modulation.hip) for n bands: coefs as launchBandMetrics takes them; tab = row 0
// of the twiddle table on the DEVICE (pv_modulation.h: kModRowStride floats from step to step, T rows, kModTablePad zero rows in front
// of row 0); out = n x kModFloats planes of a.histPlane floats (band j, float k at plane j * kModFloats + k), indexed by the cell's
// offset inside a history plane; NaN where the cell has no onset in that run.  One launch per band
void launchModulation(const AnalyzeArgs& a, const float* coefs, int n, const float* tab, float* out, hipStream_t stream);

// ---- pv_echo.hip: per-cell echo criterion (speech and music)
// echo criterion of the last completed run (pv_echo.hip): out = kEchoFloats planes of a.histPlane floats, indexed by the cell's
// offset inside a history plane; NaN where the cell has no onset in that run.  The caller has checked echoFsOk(a.fs)
void launchEchoCriterion(const AnalyzeArgs& a, float* out, hipStream_t stream);

// ---- pv_spectrum.hip: per-cell transfer functions at chosen frequencies
// One pass over the history of the last completed run for `bins` bins held `block` to a lane (spectrumBlockOk(block); bins <=
// block).  tab: the pass's twiddles on the device, row t = {cos, sin} pairs of its `block` bins (2 * block floats, bins past
// `bins` zero), rows 0 .. T - 1 + kSpectrumTablePad (rows past T - 1 zero); spow: the bins' source powers (device); out: the
// pass's 3 * bins planes of a.histPlane floats -- re, im, level of each bin, indexed by the cell's offset inside a history
// plane; NaN where the cell has no onset in that run.
constexpr int kSpectrumTablePad = 64;
bool spectrumBlockOk(int block);
void launchSpectrum(const AnalyzeArgs& a, int block, int bins, const float* tab, const float* spow, float* out, hipStream_t stream);

// ---- pv_waterfall.hip: per-receiver waterfalls (cumulative spectral decay)
// Where a receiver's samples are and what of them may be read: sample t at samples[offset + t * stride], never below tLoad (the
// larger of the onset and the first recorded step of the cell's tile; INT_MAX: nothing); onset < 0: no record (F quiet NaNs)
struct WaterfallRx {
    long long offset, stride;
    int onset, tLoad;
};
struct WaterfallArgs {
    const float* samples;   // the history (a.hist), or the emitter traces of sparse-emitter mode
    const WaterfallRx* rx;  // nPos receivers
    const float* tab;       // per block of 64 bins: kWaterfallTablePad zero rows, then rows 0 .. T - 1, each 64 {cos, sin} pairs
                            // (the bins past n zero)
    const float* spow;      // n source powers
    float* rec;             // nPos records of waterfallFloats(n, m) floats (pv_waterfall.h)
    int nPos, n, m, ns, T;
};
constexpr int kWaterfallTablePad = 128;
// the receiver table of `cells` (result cell X * gy + Y, -1: off the map; device-visible) from the last run's window, onset map and
// tileFirst; trace: receiver i's samples are row i of the emitter traces [nPos][T] instead of the history
void launchWaterfallReceivers(const AnalyzeArgs& a, const long long* cells, int nPos, bool trace, WaterfallRx* rx, hipStream_t stream);
// one pass with `block` receivers to a wave (waterfallBlockOk(block)); waterfallBlockFor: the block the launcher's rule picks on a
// device of `cus` compute units (speed only: a record's bits do not depend on the block)
bool waterfallBlockOk(int block);
int waterfallBlockFor(int n, int nPos, int cus);
void launchWaterfall(const WaterfallArgs& a, int block, hipStream_t stream);

// ---- pv_arrays.hip: source arrays (the combined response of weighted, delayed members; pv_arrays.h)
// Where a member's samples are: sample t at samples[offset + t * stride], never below tLoad (its tile's first recorded step, 0 for
// an emitter trace; INT_MAX: no samples -- a cell outside the run's history window)
struct ArrayRow {
    long long offset, stride;
    int tLoad, pad;
};
struct ArrayTap;
struct ArrayMixArgs {
    const float* samples;  // the history (a.hist), or the emitter traces of sparse-emitter mode
    const ArrayRow* rows;  // one per member of the setting, in the setting's order
    const ArrayTap* taps;  // array a's taps at tapOff[a] .. tapOff[a + 1] - 1, row = the member's index into rows
    const int* tapOff;     // nArrays + 1 entries
    float* mix;            // planes [T][P]: y_a(t) at mix[t * P + a]; columns nArrays .. P - 1 are written as zero
    int nArrays, P, T;     // P = nArrays rounded up to 64
};
// the member rows of `src` (device-visible; per member its result cell X * gy + Y, or with trace the index of the registered emitter
// whose trace it reads) from the last run's window and tileFirst
void launchArrayRows(const AnalyzeArgs& a, const long long* src, int nRows, bool trace, ArrayRow* rows, hipStream_t stream);
void launchArrayMix(const ArrayMixArgs& a, hipStream_t stream);
// onsets[0 .. P): the first step of column a of the mix planes above the onset threshold as a float, FLT_MAX: none (and for a >= nArrays)
void launchArrayOnsets(const float* mix, int T, int P, int nArrays, float* onsets, hipStream_t stream);

// ---- pv_aural.hip: auralisation (audio-rate responses and their convolution with dry signals; pv_aural.h)
// rows[r][0 .. T): receiver r's samples gathered out of `samples` by its ArrayRow (+0.0f below tLoad)
void launchAuralGather(const float* samples, const ArrayRow* src, int R, int T, float* rows, hipStream_t stream);
// resp[r][0 .. L) from rows[r][0 .. T): first[L], wT the weights TRANSPOSED, slot j of sample n at wT[j * L + n]
void launchAuralResample(const float* rows, int R, int T, const int* first, const float* wT, int L, int K, float* resp, hipStream_t stream);
struct AuralConvolveArgs {
    const float* resp;     // [R][L]
    const float* signals;  // [nSignals][N]
    const int* route;      // [R]: the signal of receiver r, -1: not rendered (its output is +0.0f)
    float* out;            // [R][M], M = N + L - 1
    int R, L, N;
};
// the tiling of the tiled form: outputs per block, taps per staged chunk
constexpr int kAuralOutputsPerBlock = 256;
constexpr int kAuralTapsPerChunk = 128;
// form: kAuralTiled or kAuralPlain (pv_aural.h); the same bits either way
void launchAuralConvolve(const AuralConvolveArgs& a, int form, hipStream_t stream);
// mix[m] over the routed receivers in increasing r
void launchAuralMix(const float* out, const int* route, const float* gain, int R, int M, float* mix, hipStream_t stream);

// ---- pv_copy.hip: read-backs and copies
// slab halos: src[i] -> dst[i] for up to six blocks of n floats (n % 4 == 0, 16-byte aligned); dst[i] = NULL skips a block
void launchHaloPush(const float* const src[6], float* const dst[6], long long n, const HaloHandoff& hand, hipStream_t stream);
void launchHistRow(const AnalyzeArgs& a, int X, float* outTxPitch, hipStream_t stream);
void launchCopyBlock(const float* src, long long sstride, int spitch, int sr0, int sc0, float* dst, long long dstride,
                     int dpitch, int dr0, int dc0, int nr, int nc, int nplanes, const int* srcPlanesDev,
                     const int* dstPlanesDev, hipStream_t stream, const unsigned* abortWord = nullptr);  // plane maps: NULL = identity
// (far: where the last run's far cells begin -- their listener direction is computed, not read: pv_device.h FarInfo)
void launchGatherQueries(const float* res, long long n, const long long* cellsHost, int nq, float* outHost, const FarInfo& far,
                         hipStream_t stream);  // nq <= 64
void launchGatherOutput(const float* res, long long n, long long cell, float* out8Host, const FarInfo& far, hipStream_t stream);
void launchPackResults(const float* res, long long n, float* res8, hipStream_t stream);
void launchPackWindow(const float* res, long long n, int gy, int r0, int c0, int nr, int nc, float* out8, const FarInfo& far,
                      hipStream_t stream);
void launchEfree(const float* hist, long long plane, long long cellOff, int n, float r, float* out,
                 hipStream_t stream);
void launchIr(const AnalyzeArgs& a, int X, int Y, float* out3T, hipStream_t stream);
void launchUnpad(const float* padded, float* dense, const Geometry& g, hipStream_t stream);
void launchPad(const float* dense, float* padded, const Geometry& g, hipStream_t stream);
void launchHistPlane(const AnalyzeArgs& a, int t, float* dense, int NX, int NY, int histRows,
                     hipStream_t stream);
void launchSetHistPlane(const AnalyzeArgs& a, int t, const float* dense, int NX, int NY, int histRows, float* hist,
                        hipStream_t stream);

}  // namespace pva
