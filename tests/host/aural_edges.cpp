// aural_edges.cpp -- the edge cases of the auralisation's host restatements (PvAmdHostAuralTaps, PvAmdHostAuralResample,
// PvAmdHostAuralConvolve: csrc/pv_aural.h through the HIP-less host build of pv_capi.cpp) in a program of their own, to be compiled
// with -fsanitize=address,undefined and run on the CPU (tests/test_host_aural.py): every array is sized exactly, so an index outside
// a table, a sample row, a response or an output is an ASan report.
//   1  tables: the shapes the header states, the first slot and the last inside the window, weights outside it +0, every row's sum
//      near the gain of the filter at 0 Hz, every refusal;
//   2  responses against a plain restatement, bit for bit: random samples, a denormal, -0.0, inf and NaN, tables that reach below
//      t = 0 and past T - 1;
//   3  outputs against a plain restatement, bit for bit, N in {1, 2, L - 1, L, L + 1}, the same special samples.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "planeverb_amd.h"

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

static unsigned rngState = 2463534242u;
static float rnd() {  // uniform in [-1, 1)
    rngState = rngState * 1664525u + 1013904223u;
    return (float)((rngState >> 8) & 0xffffff) / 8388608.0f - 1.0f;
}

static void special(std::vector<float>& v) {  // a denormal, -0.0, inf, NaN, where there is room
    const float s[4] = {1.0e-41f, -0.0f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    for (size_t i = 0; i < 4 && 3 * i + 1 < v.size(); ++i) v[3 * i + 1] = s[i];
}

struct Tables {
    int L = 0, K = 0;
    std::vector<int> first;
    std::vector<float> w;
};

static bool tables(int fs, int T, int rate, int Z, float beta, Tables* t) {
    if (PvAmdHostAuralTaps(fs, T, rate, Z, beta, nullptr, nullptr, 0, &t->L, &t->K) != 0) return false;
    t->first.assign((size_t)t->L, 0);
    t->w.assign((size_t)t->L * t->K, -1.f);
    int L2 = 0, K2 = 0;
    CHECK(PvAmdHostAuralTaps(fs, T, rate, Z, beta, t->first.data(), t->w.data(), t->L, &L2, &K2) == 0);
    CHECK(L2 == t->L && K2 == t->K);
    return true;
}

static void checkTables(int fs, int T, int rate, int Z, float beta) {
    Tables t;
    CHECK(tables(fs, T, rate, Z, beta, &t));
    const double c = rate < fs ? (double)rate / fs : 1.0, half = (double)Z / c;
    CHECK(t.K == 2 * (int)std::floor(half) + 1);
    CHECK(t.L == (int)std::floor(((double)(T - 1) * rate) / fs) + 1);
    CHECK(t.K <= PVA_AURAL_MAX_TAPS);
    for (int n = 0; n < t.L; ++n) {
        const double u = ((double)n * fs) / rate;
        CHECK(t.first[(size_t)n] == (int)std::ceil(u - half));
        double sum = 0.0;
        for (int j = 0; j < t.K; ++j) {
            const float v = t.w[(size_t)n * t.K + j];
            const double d = u - (double)(t.first[(size_t)n] + j);
            CHECK(v == v && std::fabs(v) <= 1.0f);
            if (std::fabs(d) > half) {
                unsigned bitsOf;
                std::memcpy(&bitsOf, &v, 4);
                CHECK(bitsOf == 0u);
            }
            sum += v;
        }
        if (beta >= 6.f && Z >= 8) CHECK(std::fabs(sum - 1.0) < 0.01);  // (a windowed sinc of unit gain at 0 Hz)
    }
}

static void checkResample(int fs, int T, int rate, int Z, float beta, bool shifted) {
    Tables t;
    CHECK(tables(fs, T, rate, Z, beta, &t));
    if (shifted)  // (tables that reach far below 0 and past T - 1: every such sample is +0)
        for (int n = 0; n < t.L; ++n) {
            int& f = t.first[(size_t)n];
            f = n % 3 == 0 ? f - T : n % 3 == 1 ? f + T - 2 : std::numeric_limits<int>::max() - t.K;
        }
    std::vector<float> p((size_t)T), got((size_t)t.L);
    for (float& v : p) v = rnd();
    special(p);
    CHECK(PvAmdHostAuralResample(p.data(), T, t.first.data(), t.w.data(), t.L, t.K, got.data()) == 0);
    for (int n = 0; n < t.L; ++n) {
        float h = 0.f;
        for (int j = 0; j < t.K; ++j) {
            const long long s = (long long)t.first[(size_t)n] + j;
            const volatile float prod = t.w[(size_t)n * t.K + j] * (s >= 0 && s < T ? p[(size_t)s] : 0.f);  // (rounded on its own)
            h = h + prod;
        }
        CHECK(sameBits(got[(size_t)n], h));
    }
}

static void checkConvolve(int L, int N, bool specials) {
    std::vector<float> h((size_t)L), x((size_t)N), got((size_t)(N + L - 1));
    for (float& v : h) v = rnd();
    for (float& v : x) v = rnd();
    if (specials) {
        special(x);
        if (L > 7) h[5] = -0.0f, h[7] = 1.0e-40f;
    }
    CHECK(PvAmdHostAuralConvolve(h.data(), L, x.data(), N, got.data()) == 0);
    for (int m = 0; m < N + L - 1; ++m) {
        float o = 0.f;
        for (int k = m - N + 1 > 0 ? m - N + 1 : 0; k <= (m < L - 1 ? m : L - 1); ++k) {
            const volatile float prod = h[(size_t)k] * x[(size_t)(m - k)];
            o = o + prod;
        }
        CHECK(sameBits(got[(size_t)m], o));
    }
}

int main() {
    const int fs = 1443, T = 435;
    // 1 tables
    for (int rate : {1443, 1000, 8000})
        for (int Z : {2, 4, 16, 64})
            for (float beta : {0.f, 9.f, 20.f}) checkTables(fs, T, rate, Z, beta);
    checkTables(84351, 500, 48000, 16, 9.f);
    {
        int L = 0, K = 0;
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == 0 && L == 2407 && K == 33);
        CHECK(PvAmdHostAuralTaps(fs, T, 1000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == 0 && L == 301 && K == 47);
        CHECK(PvAmdHostAuralTaps(fs, T, 1443, 16, 9.f, nullptr, nullptr, 0, &L, &K) == 0 && L == 435 && K == 33);
        std::vector<int> first((size_t)L);
        std::vector<float> w((size_t)L * K);
        CHECK(PvAmdHostAuralTaps(fs, T, 999, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 384001, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 1, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 65, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 16, -0.5f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 16, 20.5f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 16, std::numeric_limits<float>::quiet_NaN(), nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, T, 8000, 16, std::numeric_limits<float>::infinity(), nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(0, T, 8000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(fs, 0, 8000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);
        CHECK(PvAmdHostAuralTaps(84351, 500, 1000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);   // K = 2699
        CHECK(PvAmdHostAuralTaps(fs, 30000, 384000, 16, 9.f, nullptr, nullptr, 0, &L, &K) == -1);  // L * K above 2^24
        CHECK(PvAmdHostAuralTaps(fs, T, 1443, 16, 9.f, first.data(), w.data(), 434, &L, &K) == -1);  // (capN below L)
        CHECK(PvAmdHostAuralTaps(fs, T, 1443, 16, 9.f, first.data(), nullptr, 435, &L, &K) == -1);
        CHECK(std::strncmp(PvAmdLastError(), "aural:", 6) == 0);
        CHECK(PvAmdHostAuralTaps(fs, T, 1443, 16, 9.f, first.data(), w.data(), 435, nullptr, nullptr) == 0);
    }
    // 2 responses
    for (int rate : {1443, 1000, 8000})
        for (int Z : {2, 16})
            for (bool shifted : {false, true}) checkResample(fs, T, rate, Z, 9.f, shifted);
    checkResample(fs, 1, 8000, 4, 0.f, false);  // (one sample)
    {
        std::vector<float> p(8, 1.f), out(4);
        const int first[4] = {0, 1, 2, 3};
        const float w[4] = {1.f, 1.f, 1.f, 1.f};
        CHECK(PvAmdHostAuralResample(nullptr, 8, first, w, 4, 1, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, nullptr, w, 4, 1, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, nullptr, 4, 1, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, w, 4, 1, nullptr) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 0, first, w, 4, 1, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, w, 0, 1, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, w, 4, 0, out.data()) == -1);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, w, 4, 1025, out.data()) == -1);
        CHECK(std::strncmp(PvAmdLastError(), "aural:", 6) == 0);
        CHECK(PvAmdHostAuralResample(p.data(), 8, first, w, 4, 1, out.data()) == 0 && out[3] == 1.f);
    }
    // 3 outputs
    for (int L : {1, 2, 9, 301})
        for (int N : {1, 2, L - 1, L, L + 1})
            if (N >= 1)
                for (bool specials : {false, true}) checkConvolve(L, N, specials);
    {
        std::vector<float> h(4, 1.f), x(4, 1.f), out(7);
        CHECK(PvAmdHostAuralConvolve(nullptr, 4, x.data(), 4, out.data()) == -1);
        CHECK(PvAmdHostAuralConvolve(h.data(), 4, nullptr, 4, out.data()) == -1);
        CHECK(PvAmdHostAuralConvolve(h.data(), 4, x.data(), 4, nullptr) == -1);
        CHECK(PvAmdHostAuralConvolve(h.data(), 0, x.data(), 4, out.data()) == -1);
        CHECK(PvAmdHostAuralConvolve(h.data(), 4, x.data(), 0, out.data()) == -1);
        CHECK(PvAmdHostAuralConvolve(h.data(), 4, x.data(), PVA_AURAL_MAX_SAMPLES + 1, out.data()) == -1);
        CHECK(std::strncmp(PvAmdLastError(), "aural:", 6) == 0);
        CHECK(PvAmdHostAuralConvolve(h.data(), 4, x.data(), 4, out.data()) == 0 && out[3] == 4.f && out[6] == 1.f);
    }
    std::printf("aural_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
