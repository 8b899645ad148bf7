// pv_bake.cpp -- host side of the baked probe tables (pv_bake.h, include/planeverb_amd.h Part 4): dealing the probes over solvers,
// harvesting the gathered blocks, merging, the file format and the host query.
#include "pv_bake.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>

#include "pv_core.h"
#include "pv_solver.h"

namespace pva {

unsigned long long fnv1a64(const void* p, size_t n, unsigned long long h) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) {
        h ^= b[i];
        h *= 1099511628211ull;
    }
    return h;
}

namespace {

// FNV-1a 64 of the composed material: beta ((gx+1)(gy+1) bytes), then R ((gx+1)(gy+1) float32), then -- only when some side is
// not absorbing (Solver::boundaryAbsorbing) -- the four grid-edge absorptions' bits, so that the hashes of bakes of absorbing
// grids stay what they were
bool materialOf(Solver* s, std::vector<uint8_t>* beta, unsigned long long* hash, std::string* err) {
    const GridSpec& g = s->spec();
    const size_t n = (size_t)g.NX * g.NY;
    beta->resize(n);
    std::vector<float> R(n);
    if (!s->copyMaterial(beta->data(), R.data())) {
        *err = s->lastError();
        return false;
    }
    *hash = fnv1a64(R.data(), n * 4, fnv1a64(beta->data(), n));
    if (!s->boundaryAbsorbing()) {
        float edges[4];
        s->gridBoundary(edges);
        *hash = fnv1a64(edges, sizeof edges, *hash);
    }
    if (s->layerActive()) {  // then -- only when some side has one -- the four edge-layer widths (int32)
        int w[4];
        s->edgeLayer(w);
        *hash = fnv1a64(w, sizeof w, *hash);
        bool split;
        double r0;
        s->edgeLayerModel(&split, &r0);
        if (split) {  // then -- the split-field model only -- a model tag (int32 1) and its r0 (double)
            const int tag = 1;
            *hash = fnv1a64(&tag, sizeof tag, *hash);
            *hash = fnv1a64(&r0, sizeof r0, *hash);
        }
    }
    return true;
}

// lattice nodes along an axis of `cells` result cells: indices 0 .. nodes - 1
int latticeNodes(int cells, int d) { return (cells + d - 1) / d; }

bool finite(float v) { return v - v == 0.f; }

// one solver's gather: device box words, pinned staging sized once by the window's lattice nodes
struct Slot : RunTap {
    Solver* s = nullptr;
    int stride = 1;
    int* box = nullptr;
    int* stage = nullptr;
    long long cap = 0;  // records
    bool overflow = false;
    int probe = -1;     // the probe of the run in flight (-1: none)
    void afterRun(const float* res, const float* delay, long long resN, int gy, int r0, int c0, int nr, int nc,
                  hipStream_t stream) override {
        BakeGatherArgs a{};
        a.res = res;
        a.delay = delay;
        a.resN = resN;
        a.gy = gy;
        a.stride = stride;
        const int ra = std::max(r0, 0), ca = std::max(c0, 0);
        const int rb = r0 + nr, cb = c0 + nc;  // (exclusive; curWindow clips to the map)
        a.ni0 = (ra + stride - 1) / stride;
        a.nj0 = (ca + stride - 1) / stride;
        a.nni = std::max(0, (rb - 1) / stride - a.ni0 + 1);
        a.nnj = std::max(0, (cb - 1) / stride - a.nj0 + 1);
        if (rb <= ra) a.nni = 0;
        if (cb <= ca) a.nnj = 0;
        if ((long long)a.nni * a.nnj > cap) {  // (cannot happen: cap bounds every window; never write past the staging)
            overflow = true;
            a.nni = a.nnj = 0;
        }
        a.box = box;
        a.stage = stage;
        launchBakeGather(a, stream);
    }
    ~Slot() override {
        if (stage) Solver::hostFree(stage);
        if (box) hipFree(box);
    }
};

}  // namespace

Bake::~Bake() { dropDevice(); }

void Bake::dropDevice() const {
    std::lock_guard<std::mutex> lk(devMu_);
    for (auto& kv : dev_) {
        DevCopy& c = kv.second;
        hipSetDevice(kv.first);
        if (c.stream) hipStreamSynchronize(c.stream);
        hipFree(c.probe5);
        hipFree(c.recOff);
        hipFree(c.rec);
        hipFree(c.q);
        if (c.stream) hipStreamDestroy(c.stream);
    }
    dev_.clear();
}

Bake* Bake::create(Solver* like, int stride, float x0, float z0, float sx, float sz, int nx, int nz, std::string* err) {
    if (stride < 1) return *err = "PvAmdBakeCreate: stride must be >= 1", nullptr;
    if (nx < 1 || nz < 1 || (long long)nx * nz > (1 << 24)) return *err = "PvAmdBakeCreate: nx, nz must be >= 1, nx * nz <= 2^24", nullptr;
    if (!finite(x0) || !finite(z0) || !finite(sx) || !finite(sz) || !(sx > 0.f) || !(sz > 0.f))
        return *err = "PvAmdBakeCreate: origin and spacing must be finite, the spacing > 0", nullptr;
    std::unique_ptr<Bake> b(new Bake());
    const GridSpec& g = like->spec();
    b->h.gx = g.gx;
    b->h.gy = g.gy;
    b->h.T = like->T();
    b->h.fs = (int)g.fs;
    b->h.res = g.res;
    b->h.dx = g.dx;
    b->h.stride = stride;
    b->h.x0 = x0;
    b->h.z0 = z0;
    b->h.sx = sx;
    b->h.sz = sz;
    b->h.nx = nx;
    b->h.nz = nz;
    std::vector<uint8_t> beta;
    if (!materialOf(like, &beta, &b->h.materialHash, err)) return nullptr;
    b->probe5.assign((size_t)5 * nx * nz, 0);
    b->recOff.assign((size_t)nx * nz, 0);
    return b.release();
}

void Bake::counts(int* baked, int* invalid, long long* records) const {
    int nb = 0, ni = 0;
    long long nr = 0;
    for (int k = 0; k < probes(); ++k) {
        const int* p = &probe5[(size_t)5 * k];
        nb += p[0] != 0;
        ni += p[0] == 2;
        nr += (long long)p[3] * p[4];
    }
    if (baked) *baked = nb;
    if (invalid) *invalid = ni;
    if (records) *records = nr;
}

std::vector<std::vector<float>> Bake::split() const {
    std::vector<std::vector<float>> r((size_t)probes());
    for (int k = 0; k < probes(); ++k) {
        const size_t n = (size_t)probe5[(size_t)5 * k + 3] * probe5[(size_t)5 * k + 4] * kBakeRecFloats;
        r[(size_t)k].assign(rec.begin() + recOff[(size_t)k], rec.begin() + recOff[(size_t)k] + (long long)n);
    }
    return r;
}

void Bake::setProbes(const std::vector<std::vector<float>>& recs) {
    size_t total = 0;
    for (const auto& v : recs) total += v.size();
    rec.clear();
    rec.reserve(total);
    for (int k = 0; k < probes(); ++k) {
        recOff[(size_t)k] = (long long)rec.size();
        rec.insert(rec.end(), recs[(size_t)k].begin(), recs[(size_t)k].end());
    }
    ++version_;
    dropDevice();
}

bool Bake::run(Solver* const* solvers, int n, int rank, int world, std::string* err) {
    if (!solvers || n < 1) return *err = "PvAmdBakeRun: no solvers", false;
    if (world < 1 || rank < 0 || rank >= world) return *err = "PvAmdBakeRun: rank must lie in [0, world)", false;
    std::vector<uint8_t> beta;
    for (int i = 0; i < n; ++i) {
        Solver* s = solvers[i];
        if (!s) return *err = "PvAmdBakeRun: null solver", false;
        for (int j = 0; j < i; ++j)
            if (solvers[j] == s) return *err = "PvAmdBakeRun: a solver is listed twice", false;
        const GridSpec& g = s->spec();
        if (g.gx != h.gx || g.gy != h.gy || s->T() != h.T || (int)g.fs != h.fs || g.res != h.res || !(g.dx == h.dx))
            return *err = "PvAmdBakeRun: solver " + std::to_string(i) + " has another grid (gx, gy, T, fs, res or dx) than the bake", false;
        SolverOptions& o = s->options();
        if (o.slabCount > 1) return *err = "PvAmdBakeRun: slab solvers cannot bake", false;
        if (o.streaming) return *err = "PvAmdBakeRun: solver " + std::to_string(i) + " is in sparse-emitter mode (no wet gain or RT60 away from registered emitters)", false;
        if (o.skipAnalysis) return *err = "PvAmdBakeRun: solver " + std::to_string(i) + " skips the analysis", false;
        unsigned long long hash = 0;
        if (!materialOf(s, &beta, &hash, err)) return false;
        if (hash != h.materialHash)
            return *err = "PvAmdBakeRun: solver " + std::to_string(i) + "'s material differs from the bake's (material hash)", false;
    }
    // probe validity: the listener cell (FDTD.cpp:97-98) inside the result map and air in the composed material
    const GridSpec& g = solvers[0]->spec();
    std::vector<int> todo;
    std::vector<int> state((size_t)probes(), -1);
    for (int k = rank; k < probes(); k += world) {
        const int i = k % h.nx, j = k / h.nx;
        const float x = h.x0 + (float)i * h.sx, z = h.z0 + (float)j * h.sz;
        const float qx = (x + 0.f) / g.dx, qz = (z + 0.f) / g.dx;
        bool ok = qx >= 0.f && qx < (float)g.gx && qz >= 0.f && qz < (float)g.gy;
        if (ok) {
            int cx, cy;
            listenerCell(g, x, z, &cx, &cy);
            ok = beta[(size_t)cx * g.NY + cy] != 0;
        }
        state[(size_t)k] = ok ? 1 : 2;
        if (ok) todo.push_back(k);
    }
    // one slot per solver; each solver keeps one run in flight
    std::vector<std::unique_ptr<Slot>> slots;
    for (int i = 0; i < n; ++i) {
        std::unique_ptr<Slot> sl(new Slot());
        sl->s = solvers[i];
        sl->stride = h.stride;
        int wr = 0, wc = 0;
        solvers[i]->windowExtent(&wr, &wc);
        // a window of wr rows holds at most ceil(wr / d) lattice rows
        sl->cap = (long long)latticeNodes(wr, h.stride) * latticeNodes(wc, h.stride);
        if (hipSetDevice(solvers[i]->device()) != hipSuccess || hipMalloc((void**)&sl->box, 4 * sizeof(int)) != hipSuccess)
            return *err = "PvAmdBakeRun: hipMalloc of the box words failed", false;
        sl->stage = static_cast<int*>(Solver::hostAlloc(16 + (size_t)sl->cap * kBakeRecFloats * 4));
        if (!sl->stage) return *err = "PvAmdBakeRun: pinned staging allocation failed", false;
        slots.push_back(std::move(sl));
    }
    // whatever happens below: no run of a solver is left in flight with its tap pointing at a slot
    struct Release {
        std::vector<std::unique_ptr<Slot>>& slots;
        ~Release() {
            for (auto& sl : slots) {
                if (sl->probe >= 0) sl->s->sync();
                sl->s->setRunTap(nullptr);
            }
        }
    } release{slots};
    for (auto& sl : slots) sl->s->setRunTap(sl.get());

    std::vector<std::vector<float>> recs = split();
    std::vector<int> block((size_t)5 * probes());
    std::copy(probe5.begin(), probe5.end(), block.begin());
    auto harvest = [&](Slot& sl) -> bool {
        if (sl.probe < 0) return true;
        const int k = sl.probe;
        sl.probe = -1;
        if (!sl.s->sync()) return *err = sl.s->lastError(), false;
        if (sl.overflow) return *err = "PvAmdBakeRun: window larger than the staging slot", false;
        const int* st = sl.stage;
        const int i0 = st[0], j0 = st[1], ni = st[2], nj = st[3];
        if (ni < 0 || nj < 0 || (long long)ni * nj > sl.cap) return *err = "PvAmdBakeRun: gathered block out of range", false;
        int* p = &block[(size_t)5 * k];
        p[0] = 1;
        p[1] = ni ? i0 : 0;
        p[2] = ni ? j0 : 0;
        p[3] = ni;
        p[4] = ni ? nj : 0;
        const float* r = reinterpret_cast<const float*>(st + 4);
        recs[(size_t)k].assign(r, r + (size_t)p[3] * p[4] * kBakeRecFloats);
        return true;
    };
    for (size_t q = 0; q < todo.size(); ++q) {
        Slot& sl = *slots[q % (size_t)n];
        if (!harvest(sl)) return false;
        const int k = todo[q];
        const int i = k % h.nx, j = k / h.nx;
        const float x = h.x0 + (float)i * h.sx, z = h.z0 + (float)j * h.sz;
        sl.probe = k;
        if (!sl.s->run(x, 0.f, z, false)) {
            sl.probe = -1;
            return *err = sl.s->lastError(), false;
        }
    }
    for (auto& sl : slots)
        if (!harvest(*sl)) return false;
    // commit: this rank's probes (invalid ones without records)
    for (int k = rank; k < probes(); k += world) {
        int* p = &block[(size_t)5 * k];
        if (state[(size_t)k] == 2) {
            p[0] = 2;
            p[1] = p[2] = p[3] = p[4] = 0;
            recs[(size_t)k].clear();
        }
    }
    probe5 = block;
    setProbes(recs);
    return true;
}

bool Bake::sameBake(const Bake& o) const {
    return h.gx == o.h.gx && h.gy == o.h.gy && h.T == o.h.T && h.fs == o.h.fs && h.res == o.h.res &&
           std::memcmp(&h.dx, &o.h.dx, 4) == 0 && h.stride == o.h.stride && std::memcmp(&h.x0, &o.h.x0, 4) == 0 &&
           std::memcmp(&h.z0, &o.h.z0, 4) == 0 && std::memcmp(&h.sx, &o.h.sx, 4) == 0 && std::memcmp(&h.sz, &o.h.sz, 4) == 0 &&
           h.nx == o.h.nx && h.nz == o.h.nz && h.materialHash == o.h.materialHash;
}

bool Bake::merge(const Bake& src, std::string* err) {
    if (&src == this) return true;
    if (!sameBake(src)) return *err = "PvAmdBakeMerge: the bakes differ in lattice, grid or material hash", false;
    std::vector<std::vector<float>> recs = split();
    std::vector<int> block = probe5;
    for (int k = 0; k < probes(); ++k) {
        const int* s5 = &src.probe5[(size_t)5 * k];
        if (s5[0] == 0) continue;
        int* d5 = &block[(size_t)5 * k];
        const size_t nf = (size_t)s5[3] * s5[4] * kBakeRecFloats;
        if (d5[0] != 0) {
            const bool same = std::equal(s5, s5 + 5, d5) &&
                              std::memcmp(src.records(k), recs[(size_t)k].data(), nf * 4) == 0;
            if (!same) return *err = "PvAmdBakeMerge: probe " + std::to_string(k) + " is baked in both with different contents", false;
            continue;
        }
        std::copy(s5, s5 + 5, d5);
        recs[(size_t)k].assign(src.records(k), src.records(k) + nf);
    }
    probe5 = block;
    setProbes(recs);
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// file format: little-endian; magic, version, header, probe table, records, FNV-1a 64 of everything before it
// ---------------------------------------------------------------------------------------------------------------------------
namespace {
const char kMagic[8] = {'P', 'V', 'B', 'A', 'K', 'E', '\0', '\1'};
constexpr unsigned kVersion = 1;
constexpr size_t kHeaderBytes = 88, kEntryBytes = 28;

template <typename Tp>
void put(std::vector<unsigned char>& b, Tp v) {
    const size_t o = b.size();
    b.resize(o + sizeof(Tp));
    std::memcpy(b.data() + o, &v, sizeof(Tp));
}
template <typename Tp>
Tp get(const unsigned char* p) {
    Tp v;
    std::memcpy(&v, p, sizeof(Tp));
    return v;
}
}  // namespace

bool Bake::save(const std::string& path, std::string* err) const {
    std::vector<unsigned char> b;
    b.insert(b.end(), kMagic, kMagic + 8);
    put<uint32_t>(b, kVersion);
    for (int v : {h.gx, h.gy, h.T, h.fs, h.res}) put<int32_t>(b, v);
    put<float>(b, h.dx);
    put<int32_t>(b, h.stride);
    for (float v : {h.x0, h.z0, h.sx, h.sz}) put<float>(b, v);
    put<int32_t>(b, h.nx);
    put<int32_t>(b, h.nz);
    int nb = 0, ni = 0;
    long long nr = 0;
    counts(&nb, &ni, &nr);
    put<int32_t>(b, nb);
    put<int32_t>(b, ni);
    put<int64_t>(b, nr);
    put<uint64_t>(b, h.materialHash);
    const uint64_t recStart = kHeaderBytes + kEntryBytes * (uint64_t)probes();
    for (int k = 0; k < probes(); ++k) {
        for (int m = 0; m < 5; ++m) put<int32_t>(b, probe5[(size_t)5 * k + m]);
        put<uint64_t>(b, recStart + 4 * (uint64_t)recOff[(size_t)k]);
    }
    const size_t o = b.size();
    b.resize(o + rec.size() * 4);
    if (!rec.empty()) std::memcpy(b.data() + o, rec.data(), rec.size() * 4);
    put<uint64_t>(b, fnv1a64(b.data(), b.size()));
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return *err = "PvAmdBakeSave: cannot open " + path, false;
    const bool ok = std::fwrite(b.data(), 1, b.size(), f) == b.size();
    if (std::fclose(f) != 0 || !ok) return *err = "PvAmdBakeSave: write to " + path + " failed", false;
    return true;
}

Bake* Bake::load(const std::string& path, std::string* err) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return *err = "PvAmdBakeLoad: cannot open " + path, nullptr;
    std::vector<unsigned char> b;
    unsigned char buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof(buf), f)) > 0) b.insert(b.end(), buf, buf + got);
    std::fclose(f);
    auto bad = [&](const std::string& why) -> Bake* {
        *err = "PvAmdBakeLoad: " + path + ": " + why;
        return nullptr;
    };
    if (b.size() < kHeaderBytes + 8) return bad("truncated (shorter than the header)");
    if (std::memcmp(b.data(), kMagic, 8) != 0) return bad("wrong magic");
    if (get<uint32_t>(&b[8]) != kVersion) return bad("unsupported version " + std::to_string(get<uint32_t>(&b[8])));
    std::unique_ptr<Bake> k(new Bake());
    BakeHeader& h = k->h;
    const unsigned char* p = b.data() + 12;
    h.gx = get<int32_t>(p), h.gy = get<int32_t>(p + 4), h.T = get<int32_t>(p + 8), h.fs = get<int32_t>(p + 12), h.res = get<int32_t>(p + 16);
    h.dx = get<float>(p + 20);
    h.stride = get<int32_t>(p + 24);
    h.x0 = get<float>(p + 28), h.z0 = get<float>(p + 32), h.sx = get<float>(p + 36), h.sz = get<float>(p + 40);
    h.nx = get<int32_t>(p + 44), h.nz = get<int32_t>(p + 48);
    const int nb = get<int32_t>(p + 52), ninv = get<int32_t>(p + 56);
    const long long nrec = get<int64_t>(p + 60);
    h.materialHash = get<uint64_t>(p + 68);
    if (h.gx < 1 || h.gy < 1 || h.T < 1 || h.stride < 1 || h.nx < 1 || h.nz < 1 || (long long)h.nx * h.nz > (1 << 24) ||
        !finite(h.dx) || !(h.dx > 0.f) || !finite(h.x0) || !finite(h.z0) || !finite(h.sx) || !finite(h.sz) || !(h.sx > 0.f) ||
        !(h.sz > 0.f))
        return bad("inconsistent header");
    const uint64_t np = (uint64_t)h.nx * h.nz;
    const uint64_t recStart = kHeaderBytes + kEntryBytes * np;
    if (b.size() < recStart + 8) return bad("truncated (probe table)");
    if (nrec < 0 || (uint64_t)nrec > (b.size() - recStart) / 36) return bad("inconsistent sizes (record count)");
    if ((uint64_t)b.size() != recStart + 36 * (uint64_t)nrec + 8) return bad("inconsistent sizes (file length)");
    if (get<uint64_t>(&b[b.size() - 8]) != fnv1a64(b.data(), b.size() - 8)) return bad("checksum mismatch");
    const int li = latticeNodes(h.gx, h.stride), lj = latticeNodes(h.gy, h.stride);
    k->probe5.resize((size_t)5 * np);
    k->recOff.resize((size_t)np);
    uint64_t next = recStart;
    int cb = 0, ci = 0;
    for (uint64_t q = 0; q < np; ++q) {
        const unsigned char* e = b.data() + kHeaderBytes + kEntryBytes * q;
        int* s5 = &k->probe5[(size_t)5 * q];
        for (int m = 0; m < 5; ++m) s5[m] = get<int32_t>(e + 4 * m);
        const uint64_t off = get<uint64_t>(e + 20);
        const int st = s5[0], i0 = s5[1], j0 = s5[2], ni = s5[3], nj = s5[4];
        if (st < 0 || st > 2) return bad("probe " + std::to_string(q) + ": state " + std::to_string(st));
        const bool empty = ni == 0 && nj == 0 && i0 == 0 && j0 == 0;
        if (st != 1 && !empty) return bad("probe " + std::to_string(q) + ": a block for a probe that is not baked valid");
        if (!empty && (ni < 1 || nj < 1 || i0 < 0 || j0 < 0 || i0 > li - ni || j0 > lj - nj))
            return bad("probe " + std::to_string(q) + ": block outside the lattice");
        if (off != next) return bad("probe " + std::to_string(q) + ": record offset outside the file or out of order");
        const uint64_t bytes = 36 * (uint64_t)ni * (uint64_t)nj;
        if (bytes > b.size() - 8 - next) return bad("probe " + std::to_string(q) + ": records outside the file");
        k->recOff[(size_t)q] = (long long)((next - recStart) / 4);
        next += bytes;
        cb += st != 0;
        ci += st == 2;
    }
    if (next != recStart + 36 * (uint64_t)nrec) return bad("inconsistent sizes (records of the table vs the header)");
    if (cb != nb || ci != ninv) return bad("inconsistent sizes (probe counts of the header)");
    k->rec.resize((size_t)nrec * kBakeRecFloats);
    if (nrec) std::memcpy(k->rec.data(), b.data() + recStart, (size_t)nrec * 36);
    return k.release();
}

// ---------------------------------------------------------------------------------------------------------------------------
// queries
// ---------------------------------------------------------------------------------------------------------------------------
BakeView Bake::view() const {
    BakeView v;
    v.gx = h.gx;
    v.gy = h.gy;
    v.stride = h.stride;
    v.nx = h.nx;
    v.nz = h.nz;
    v.dx = h.dx;
    v.x0 = h.x0;
    v.z0 = h.z0;
    v.sx = h.sx;
    v.sz = h.sz;
    v.probe5 = probe5.data();
    v.recOff = recOff.data();
    v.rec = rec.data();
    return v;
}

void Bake::query(const float* lxyz, const float* exyz, int n, float* out8) const {
    const BakeView v = view();
    for (int q = 0; q < n; ++q)
        bakeQuery(v, lxyz[3 * (size_t)q], lxyz[3 * (size_t)q + 2], exyz[3 * (size_t)q], exyz[3 * (size_t)q + 2], out8 + 8 * (size_t)q);
}

bool Bake::queryDevice(int device, const float* lxyz, const float* exyz, int n, float* out8, std::string* err) const {
    if (n <= 0) return true;
    std::lock_guard<std::mutex> lk(devMu_);
    auto hip = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        *err = std::string("PvAmdBakeQueryDevice: ") + what + ": " + hipGetErrorString(e);
        return false;
    };
    int count = 0;
    if (!hip(hipGetDeviceCount(&count), "hipGetDeviceCount")) return false;
    if (device < 0 || device >= count) return *err = "PvAmdBakeQueryDevice: no HIP device " + std::to_string(device), false;
    if (!hip(hipSetDevice(device), "hipSetDevice")) return false;
    DevCopy& c = dev_[device];
    if (!c.stream && !hip(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking), "hipStreamCreate")) return false;
    if (c.version != version_) {  // the bake once per device, until run / merge change it
        hipFree(c.probe5);
        hipFree(c.recOff);
        hipFree(c.rec);
        c.probe5 = nullptr;
        c.recOff = nullptr;
        c.rec = nullptr;
        const size_t np = (size_t)probes();
        if (!hip(hipMalloc((void**)&c.probe5, np * 5 * 4), "hipMalloc") || !hip(hipMalloc((void**)&c.recOff, np * 8), "hipMalloc") ||
            !hip(hipMalloc((void**)&c.rec, std::max<size_t>(rec.size(), 1) * 4), "hipMalloc"))
            return false;
        if (!hip(hipMemcpyAsync(c.probe5, probe5.data(), np * 5 * 4, hipMemcpyHostToDevice, c.stream), "upload") ||
            !hip(hipMemcpyAsync(c.recOff, recOff.data(), np * 8, hipMemcpyHostToDevice, c.stream), "upload") ||
            (!rec.empty() && !hip(hipMemcpyAsync(c.rec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice, c.stream), "upload")) ||
            !hip(hipStreamSynchronize(c.stream), "upload sync"))
            return false;
        c.version = version_;
    }
    if ((size_t)n > c.qCap) {
        hipFree(c.q);
        c.q = nullptr;
        c.qCap = 0;
        if (!hip(hipMalloc((void**)&c.q, (size_t)n * 14 * 4), "hipMalloc")) return false;
        c.qCap = (size_t)n;
    }
    float* dl = c.q;
    float* de = c.q + (size_t)n * 3;
    float* dout = c.q + (size_t)n * 6;
    BakeView v = view();
    v.probe5 = c.probe5;
    v.recOff = c.recOff;
    v.rec = c.rec;
    if (!hip(hipMemcpyAsync(dl, lxyz, (size_t)n * 12, hipMemcpyHostToDevice, c.stream), "query upload") ||
        !hip(hipMemcpyAsync(de, exyz, (size_t)n * 12, hipMemcpyHostToDevice, c.stream), "query upload"))
        return false;
    launchBakeQuery(v, dl, de, n, dout, c.stream);
    if (!hip(hipGetLastError(), "query launch")) return false;
    return hip(hipMemcpyAsync(out8, dout, (size_t)n * 32, hipMemcpyDeviceToHost, c.stream), "query read-back") &&
           hip(hipStreamSynchronize(c.stream), "query sync");
}

}  // namespace pva
