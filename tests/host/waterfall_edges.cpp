// waterfall_edges.cpp -- the edge cases of the waterfall's host restatement (PvAmdHostWaterfall: csrc/pv_waterfall.h through the
// HIP-less host build of pv_capi.cpp) in a program of their own, to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_host_waterfall.py): every array is sized exactly, so an index outside a response, a table or a record is an ASan report.
//   1  parity with a plain restatement of the definition written here, bit for bit: 1, 64, 65 and 130 bins, 1 and 16 slices,
//      onsets 0 and T - 1, a slice length that puts the last slices past T (-inf levels, a slice count below m);
//   2  the sequential-summation bound against the same sum in double, every slice and every bin;
//   3  a decaying mode: its bin's level falls from slice to slice and is the loudest of every slice;
//   4  the refusals: the bin rule, the slice rule, the caps.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "planeverb_amd.h"
#include "pv_libm.h"

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            std::printf("line %d: %s\n", __LINE__, #c);            \
        }                                                          \
    } while (0)

static bool sameBits(float a, float b) {
    if (a != a || b != b) return (a != a) && (b != b);
    if (a == 0.f && b == 0.f) return true;
    return std::memcmp(&a, &b, 4) == 0;
}

static unsigned rngState = 12345u;
static float rnd() {  // uniform in [-1, 1)
    rngState = rngState * 1664525u + 1013904223u;
    return (float)((rngState >> 8) & 0xffffff) / 8388608.0f - 1.0f;
}

struct Setting {
    int T, fs, n, m;
    float seconds;
    std::vector<float> hz, pulse;
    Setting(int T_, int fs_, int n_, int m_, float sec) : T(T_), fs(fs_), n(n_), m(m_), seconds(sec), hz((size_t)n_), pulse((size_t)T_) {
        for (int j = 0; j < n; ++j) hz[(size_t)j] = n > 1 ? (float)(0.5 * fs * j / (n - 1)) : 61.7f;
        for (int t = 0; t < T; ++t) pulse[(size_t)t] = 0.1f * rnd();
    }
    int floats() const { return 2 + 2 * n + m * n; }
    int ns() const { return (int)(seconds * (float)fs); }
};

// the definition, written out once more: tables by PvAmdHostSpectrumTables, the source by the forward sums of the Spectrum
static void restate(const Setting& s, const std::vector<float>& p, int onset, std::vector<float>& out) {
    const int T = s.T, n = s.n, m = s.m, ns = s.ns();
    std::vector<float> c((size_t)T * n), sn((size_t)T * n);
    {  // (the Spectrum's call caps its bins: the tables in chunks of columns)
        for (int j0 = 0; j0 < n; j0 += PVA_SPECTRUM_MAX_BINS) {
            const int w = n - j0 < PVA_SPECTRUM_MAX_BINS ? n - j0 : PVA_SPECTRUM_MAX_BINS;
            std::vector<float> cc((size_t)T * w), ss((size_t)T * w);
            CHECK(PvAmdHostSpectrumTables(T, s.fs, s.hz.data() + j0, w, cc.data(), ss.data()) == 0);
            for (int t = 0; t < T; ++t)
                for (int j = 0; j < w; ++j) {
                    c[(size_t)t * n + j0 + j] = cc[(size_t)t * w + j];
                    sn[(size_t)t * n + j0 + j] = ss[(size_t)t * w + j];
                }
        }
    }
    out.assign((size_t)s.floats(), 0.f);
    int count = 0;
    for (int k = 0; k < m; ++k)
        if (onset + k * ns < T) ++count;
    out[0] = (float)onset;
    out[1] = (float)count;
    for (int j = 0; j < n; ++j) {
        float sre = 0.f, sim = 0.f;
        for (int t = 0; t < T; ++t) {
            const float a = s.pulse[(size_t)t] * c[(size_t)t * n + j], b = s.pulse[(size_t)t] * sn[(size_t)t * n + j];
            sre = sre + a;
            sim = sim + b;
        }
        const float spow = (sre * sre) + (sim * sim);
        std::vector<float> R((size_t)m, 0.f), I((size_t)m, 0.f);
        float re = 0.f, im = 0.f;
        for (int t = T - 1; t >= onset; --t) {
            const float a = p[(size_t)t] * c[(size_t)t * n + j], b = p[(size_t)t] * sn[(size_t)t * n + j];
            re = re + a;
            im = im + b;
            if ((t - onset) % ns == 0 && (t - onset) / ns < m) {
                R[(size_t)((t - onset) / ns)] = re;
                I[(size_t)((t - onset) / ns)] = im;
            }
        }
        out[(size_t)(2 + j)] = R[0];
        out[(size_t)(2 + n + j)] = I[0];
        for (int k = 0; k < m; ++k)
            out[(size_t)(2 + 2 * n + k * n + j)] = 10.0f * pva::pvLog10f(((R[(size_t)k] * R[(size_t)k]) + (I[(size_t)k] * I[(size_t)k])) / spow);
    }
}

static void parity(int T, int fs, int n, int m, float seconds, int onset, float scale) {
    Setting s(T, fs, n, m, seconds);
    std::vector<float> p((size_t)T);
    for (int t = 0; t < T; ++t) p[(size_t)t] = scale * rnd() * std::exp(-0.01f * (float)t);
    std::vector<float> got((size_t)s.floats(), -7.f), want;
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, onset, s.hz.data(), n, seconds, m, s.pulse.data(), got.data()) == 0);
    restate(s, p, onset, want);
    int bad = 0;
    for (size_t i = 0; i < got.size(); ++i) bad += !sameBits(got[i], want[i]);
    if (bad) std::printf("parity T %d n %d m %d onset %d: %d floats differ\n", T, n, m, onset, bad);
    CHECK(bad == 0);
    const int ns = s.ns();
    for (int k = 0; k < m; ++k)
        if (onset + k * ns >= T)
            for (int j = 0; j < n; ++j) CHECK(std::isinf(got[(size_t)(2 + 2 * n + k * n + j)]) && got[(size_t)(2 + 2 * n + k * n + j)] < 0.f);
}

static void bound() {
    // every slice k = 0 .. 15 (ns = 24) and every bin: slice k's sums are slice 0's of the record whose onset is the slice's first
    // step -- the walk is the same walk --, held to gamma_{N + 1} sum |p w| of the sum in double over the same float32 factors
    const int T = 435, fs = 1443, n = 130, W = PVA_SPECTRUM_MAX_BINS, ns = 24, onset = 17;
    Setting s(T, fs, n, 1, 24.2f / 1443.0f);
    CHECK(s.ns() == ns);
    std::vector<float> p((size_t)T), got((size_t)s.floats());
    for (int t = 0; t < T; ++t) p[(size_t)t] = rnd() * std::exp(-0.01f * (float)t);
    const double u = std::ldexp(1.0, -24);
    for (int k = 0; k < 16; ++k) {
        const int tk = onset + k * ns;
        CHECK(PvAmdHostWaterfall(p.data(), T, fs, tk, s.hz.data(), n, s.seconds, 1, s.pulse.data(), got.data()) == 0);
        const double q = (double)(T - tk + 1), gamma = q * u / (1.0 - q * u);
        for (int j0 = 0; j0 < n; j0 += W) {
            const int w = n - j0 < W ? n - j0 : W;
            std::vector<float> c((size_t)T * w), sn((size_t)T * w);
            CHECK(PvAmdHostSpectrumTables(T, fs, s.hz.data() + j0, w, c.data(), sn.data()) == 0);
            for (int j = 0; j < w; ++j) {
                double re = 0, im = 0, are = 0, aim = 0;
                for (int t = tk; t < T; ++t) {
                    const double a = (double)p[(size_t)t] * (double)c[(size_t)t * w + j], b = (double)p[(size_t)t] * (double)sn[(size_t)t * w + j];
                    re += a, im += b, are += std::fabs(a), aim += std::fabs(b);
                }
                CHECK(std::fabs((double)got[(size_t)(2 + j0 + j)] - re) <= gamma * are);
                CHECK(std::fabs((double)got[(size_t)(2 + n + j0 + j)] - im) <= gamma * aim);
            }
        }
    }
}

static void mode(double delta, int jmode) {
    const int T = 435, fs = 1443, n = 130, m = 32;
    const float seconds = 8.5f / 1443.0f;
    Setting s(T, fs, n, m, seconds);
    CHECK(s.ns() == 8);
    std::fill(s.pulse.begin(), s.pulse.end(), 0.f);
    s.pulse[0] = 1.f;  // (a flat source)
    std::vector<float> p((size_t)T), got((size_t)s.floats());
    for (int t = 0; t < T; ++t) p[(size_t)t] = (float)(std::exp(-delta * t) * std::cos(2.0 * M_PI * (double)s.hz[(size_t)jmode] * t / fs));
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, 0, s.hz.data(), n, seconds, m, s.pulse.data(), got.data()) == 0);
    CHECK(got[0] == 0.f && got[1] == (float)m);
    const float* level = got.data() + 2 + 2 * n;
    for (int k = 0; k < m; ++k) {
        if (k) CHECK(level[k * n + jmode] < level[(k - 1) * n + jmode]);
        for (int j = 0; j < n; ++j) CHECK(j == jmode || level[k * n + j] < level[k * n + jmode]);
    }
}

static void refusals() {
    const int T = 16, fs = 1443;
    std::vector<float> p((size_t)T, 1.f), hz(513, 5.f), out((size_t)(2 + 2 * 512 + 64 * 512));
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    auto call = [&](const float* h, int n, float sec, int m) { return PvAmdHostWaterfall(p.data(), T, fs, 0, h, n, sec, m, p.data(), out.data()); };
    CHECK(call(hz.data(), 512, 0.01f, 64) == 0);
    CHECK(call(hz.data(), 513, 0.01f, 1) == -1 && std::strstr(PvAmdLastError(), "waterfall:"));
    CHECK(call(hz.data(), 0, 0.01f, 1) == -1);
    CHECK(call(nullptr, 1, 0.01f, 1) == -1);
    CHECK(call(hz.data(), 1, 0.01f, 0) == -1 && call(hz.data(), 1, 0.01f, 65) == -1);
    for (float sec : {0.f, 0.5f / 1443.f, -1.f, nan, inf, 800.f}) CHECK(call(hz.data(), 1, sec, 1) == -1);
    CHECK(call(hz.data(), 1, (float)(1 << 20) / 1443.f, 2) == 0);
    for (float bad : {nan, inf, -1.f, 722.f}) {
        std::vector<float> h{10.f, bad};
        CHECK(call(h.data(), 2, 0.01f, 1) == -1);
    }
    std::vector<float> edge{0.f, 721.5f};
    CHECK(call(edge.data(), 2, 0.01f, 1) == 0);
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, T, hz.data(), 1, 0.01f, 1, p.data(), out.data()) == -1);
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, -1, hz.data(), 1, 0.01f, 1, p.data(), out.data()) == -1);
    CHECK(PvAmdHostWaterfall(nullptr, T, fs, 0, hz.data(), 1, 0.01f, 1, p.data(), out.data()) == -1);
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, 0, hz.data(), 1, 0.01f, 1, nullptr, out.data()) == -1);
    CHECK(PvAmdHostWaterfall(p.data(), T, fs, 0, hz.data(), 1, 0.01f, 1, p.data(), nullptr) == -1);
}

int main() {
    const int shapes[5][2] = {{1, 1}, {64, 16}, {65, 16}, {130, 1}, {130, 16}};
    for (const auto& sh : shapes) {
        parity(160, 1443, sh[0], sh[1], 0.0105f, 0, 1.f);        // ns = 15: the slices from k = 11 on start past T
        parity(160, 1443, sh[0], sh[1], 0.0105f, 159, 1.f);      // onset T - 1: one term per sum
        parity(160, 1443, sh[0], sh[1], 0.0105f, 37, 1.0e-36f);  // denormal products are kept
    }
    parity(1, 1443, 3, 4, 0.01f, 0, 1.f);  // T = 1
    parity(64, 12, 5, 64, 0.1f, 3, 1.f);   // ns = 1: a boundary at every step
    bound();
    mode(0.01, 20);
    mode(0.02, 40);
    mode(0.005, 12);
    refusals();
    std::printf("waterfall_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
