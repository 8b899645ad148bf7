// pv_bake.h -- baked listener-probe tables (include/planeverb_amd.h Part 4): the query rule, shared by the host (pv_bake.cpp)
// and the device (pv_bake.hip), and the host-side bake.
//
// A bake holds, for every probe k = j * nx + i of a lattice of listener positions (x0 + i sx, 0, z0 + j sz), the block of
// emitter-lattice nodes (result cells (r, c) with r % stride == 0 and c % stride == 0) that the probe's run reached: 9 floats
// per node, the 8 AnalyzerResult members in PvAmdCopyResults order and the onset delay.  INTEGRATION.md documents the rule,
// the file format and the API.
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace pva {

class Solver;

constexpr int kBakeRecFloats = 9;

// what the query rule reads of a bake (host vectors or their device copies)
struct BakeView {
    int gx, gy, stride, nx, nz;
    float dx, x0, z0, sx, sz;
    const int* probe5;        // nx * nz x {state, i0, j0, ni, nj}
    const long long* recOff;  // nx * nz: the probe's first record float in rec
    const float* rec;
};

// The query rule (INTEGRATION.md "Baked probe tables"): float32 throughout, no contraction (the Makefile's -ffp-contract=off),
// correctly rounded division and sqrtf -- the same bits on the host and on the device.
__host__ __device__ inline void bakeQuery(const BakeView& v, float lx, float lz, float ex, float ez, float* out) {
    for (int k = 0; k < 8; ++k) out[k] = 0.f;
    out[0] = -1.f;  // PV_INVALID_DRY_GAIN
    // 1. emitter cell: resultCell's (unsigned)((e + 0) / dx) < gx, with the truncation made explicit (valid for every input)
    const float qr = (ex + 0.f) / v.dx, qc = (ez + 0.f) / v.dx;
    if (!(qr > -1.f && qr < (float)v.gx && qc > -1.f && qc < (float)v.gy)) return;
    const int er = (int)qr, ec = (int)qc, d = v.stride;
    // 2. emitter corners
    const int ei0 = er / d, ej0 = ec / d;
    const float fa = (float)(er - ei0 * d) / (float)d, fb = (float)(ec - ej0 * d) / (float)d;
    // 3. probe corners
    float p = (lx - v.x0) / v.sx, q = (lz - v.z0) / v.sz;
    p = p >= 0.f ? p : 0.f;  // (NaN -> 0)
    q = q >= 0.f ? q : 0.f;
    p = p <= (float)(v.nx - 1) ? p : (float)(v.nx - 1);
    q = q <= (float)(v.nz - 1) ? q : (float)(v.nz - 1);
    int k0 = (int)floorf(p), m0 = (int)floorf(q);
    k0 = v.nx == 1 ? 0 : (k0 < v.nx - 2 ? k0 : v.nx - 2);
    m0 = v.nz == 1 ? 0 : (m0 < v.nz - 2 ? m0 : v.nz - 2);
    const float fp = p - (float)k0, fq = q - (float)m0;
    // 4. contributions in the order probe corner (0,0) (1,0) (0,1) (1,1), inside it emitter corner (0,0) (1,0) (0,1) (1,1)
    int used = 0;
    const float* first = nullptr;
    float S = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, rtDen = 0.f;
    bool anyInf = false;
    for (int pc = 0; pc < 4; ++pc) {
        const int a = pc & 1, b = pc >> 1;
        const int pi = k0 + a, pj = m0 + b;
        const float wp = (a ? fp : 1.f - fp) * (b ? fq : 1.f - fq);
        if (pi >= v.nx || pj >= v.nz) continue;
        const int k = pj * v.nx + pi;
        const int* pr = v.probe5 + 5 * (long long)k;
        if (pr[0] != 1) continue;
        for (int ecn = 0; ecn < 4; ++ecn) {
            const int ea = ecn & 1, eb = ecn >> 1;
            const float we = (ea ? fa : 1.f - fa) * (eb ? fb : 1.f - fb);
            const float w = wp * we;
            if (!(w > 0.f)) continue;
            const int ni = ei0 + ea - pr[1], nj = ej0 + eb - pr[2];
            if (ni < 0 || ni >= pr[3] || nj < 0 || nj >= pr[4]) continue;
            const float* r = v.rec + v.recOff[k] + (long long)(ni * pr[4] + nj) * kBakeRecFloats;
            if (!(r[8] < FLT_MAX)) continue;
            if (used++ == 0) first = r;
            S += w;
            acc[0] += w * r[0];
            acc[1] += w * r[1];
            acc[3] += w * r[3];
            for (int m = 4; m < 8; ++m) acc[m] += w * r[m];
            const float rt = r[2];
            if (rt - rt == 0.f) {  // finite
                acc[2] += w * rt;
                rtDen += w;
            } else if (rt == INFINITY) {
                anyInf = true;
            }
        }
    }
    // 5. result
    if (used == 0) return;
    if (used == 1) {
        for (int m = 0; m < 8; ++m) out[m] = first[m];
        return;
    }
    out[0] = acc[0] / S;
    out[1] = acc[1] / S;
    out[3] = acc[3] / S;
    out[2] = rtDen > 0.f ? acc[2] / rtDen : (anyInf ? INFINITY : NAN);
    for (int m = 4; m < 8; m += 2) {
        float x = acc[m], y = acc[m + 1];
        float len = (x * x) + (y * y);
        if (len != 0.f) {
            len = sqrtf(len);
            x /= len;
            y /= len;
        } else {
            x = 0.f;
            y = 0.f;
        }
        out[m] = x;
        out[m + 1] = y;
    }
}

// per-solver after-run gather (pv_bake.hip): the window's emitter-lattice nodes -> bounding box of the reached ones (device
// words) -> the box's records and the box into pinned staging
struct BakeGatherArgs {
    const float* res;     // 8 SoA result planes of resN cells
    const float* delay;
    long long resN;
    int gy, stride;
    int ni0, nj0, nni, nnj;  // the window's lattice nodes: indices [ni0, ni0 + nni) x [nj0, nj0 + nnj)
    int* box;                // 4 device words {max -i, max -j, max i, max j}, 0x80808080 = empty
    int* stage;              // pinned: 4 ints {i0, j0, ni, nj} (ni = 0: empty), then ni * nj * 9 floats
};
void launchBakeGather(const BakeGatherArgs& a, hipStream_t stream);
void launchBakeQuery(const BakeView& v, const float* lxyz, const float* exyz, int n, float* out8, hipStream_t stream);

struct BakeHeader {
    int gx = 0, gy = 0, T = 0, fs = 0, res = 0;
    float dx = 0.f;
    int stride = 1;
    float x0 = 0.f, z0 = 0.f, sx = 0.f, sz = 0.f;
    int nx = 0, nz = 0;
    unsigned long long materialHash = 0;
};

class Bake {
public:
    BakeHeader h;
    std::vector<int> probe5;      // nx * nz x {state, i0, j0, ni, nj}
    std::vector<long long> recOff;
    std::vector<float> rec;       // records of every probe in probe order

    ~Bake();
    static Bake* create(Solver* like, int stride, float x0, float z0, float sx, float sz, int nx, int nz, std::string* err);
    int probes() const { return h.nx * h.nz; }
    bool run(Solver* const* solvers, int n, int rank, int world, std::string* err);
    bool merge(const Bake& src, std::string* err);
    bool save(const std::string& path, std::string* err) const;
    static Bake* load(const std::string& path, std::string* err);
    void counts(int* baked, int* invalid, long long* records) const;
    BakeView view() const;
    void query(const float* lxyz, const float* exyz, int n, float* out8) const;
    bool queryDevice(int device, const float* lxyz, const float* exyz, int n, float* out8, std::string* err) const;
    // probe k's block (state5) and records (ni * nj * 9 floats)
    const float* records(int k) const { return rec.data() + recOff[(size_t)k]; }

private:
    Bake() = default;
    void setProbes(const std::vector<std::vector<float>>& recs);  // recOff / rec from per-probe record lists
    std::vector<std::vector<float>> split() const;
    bool sameBake(const Bake& o) const;
    // device copies (queryDevice), dropped when run / merge change the bake
    struct DevCopy {
        int* probe5 = nullptr;
        long long* recOff = nullptr;
        float* rec = nullptr;
        float* q = nullptr;  // query staging: 6 n floats in, 8 n out
        size_t qCap = 0;
        hipStream_t stream = nullptr;
        unsigned long long version = ~0ull;
    };
    mutable std::mutex devMu_;
    mutable std::map<int, DevCopy> dev_;
    unsigned long long version_ = 0;
    void dropDevice() const;
};

// FNV-1a 64
unsigned long long fnv1a64(const void* p, size_t n, unsigned long long h = 14695981039346656037ull);

}  // namespace pva
