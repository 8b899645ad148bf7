// arrays_edges.cpp -- the edge cases of the source arrays' host restatements (PvAmdHostArrayTaps, PvAmdHostArrayResponse:
// csrc/pv_arrays.h through the HIP-less host build of pv_capi.cpp) in a program of their own, to be compiled with
// -fsanitize=address,undefined and run on the CPU (tests/test_host_arrays.py): every array is sized exactly, so an index outside a
// member row, a tap list or a response is an ASan report.
//   1  taps: integer delays, mu near 0 and near 1, n = 0 with mu != 0 (refused), d just below T, negative gains, non-finite input
//      (refused), against the rule written out here; the Lagrange weights sum to the gain;
//   2  responses: 1, 2, 17 and 64 members, taps below t = 0 and past T - 1, against a plain restatement, bit for bit;
//   3  the cancelling pair gives +0 everywhere and no onset; the identity array gives p and p's onset;
//   4  the refusals of both calls.
#include <cfloat>
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

// the tap rule of the header, written out once more
static int restateTaps(int fs, int T, float gain, float seconds, int interp, int* d4, float* w4) {
    if (!std::isfinite(gain) || !std::isfinite(seconds) || seconds < 0.f) return -1;
    const double d = (double)seconds * (double)fs;
    if (!(d < (double)T)) return -1;
    if (interp == PVA_ARRAY_NEAREST) {
        const double r = std::floor(d + 0.5);
        if (!(r < (double)T)) return -1;
        d4[0] = (int)r;
        w4[0] = gain;
        return 1;
    }
    const double n = std::floor(d), mu = d - n;
    if (mu == 0.0) {
        d4[0] = (int)n;
        w4[0] = gain;
        return 1;
    }
    if (n < 1.0) return -1;
    const double D = mu + 1.0;
    const double L0 = -(((D - 1.0) * (D - 2.0)) * (D - 3.0)) / 6.0, L1 = ((D * (D - 2.0)) * (D - 3.0)) / 2.0;
    const double L2 = -((D * (D - 1.0)) * (D - 3.0)) / 2.0, L3 = ((D * (D - 1.0)) * (D - 2.0)) / 6.0;
    const double L[4] = {L0, L1, L2, L3};
    for (int j = 0; j < 4; ++j) {
        d4[j] = (int)n - 1 + j;
        w4[j] = (float)((double)gain * L[j]);
    }
    return 4;
}

static void checkTaps(int fs, int T, float gain, float seconds, int interp) {
    int wd[4], gd[4];
    float ww[4], gw[4];
    const int want = restateTaps(fs, T, gain, seconds, interp, wd, ww);
    const int got = PvAmdHostArrayTaps(fs, T, gain, seconds, interp, gd, gw);
    CHECK(got == want);
    if (got != want || got < 0) return;
    double sum = 0.0;
    for (int j = 0; j < got; ++j) {
        CHECK(gd[j] == wd[j]);
        CHECK(sameBits(gw[j], ww[j]));
        CHECK(gd[j] >= 0);
        sum += (double)gw[j];
    }
    // (after the rounding to float32: four roundings of weights of magnitude <= 1.3 |gain|)
    CHECK(std::fabs(sum - (double)gain) <= 8.0 * 1.3 * std::fabs((double)gain) * 5.96e-8 + 1e-300);
}

static void restateResponse(const std::vector<float>& p, int T, const std::vector<int>& tm, const std::vector<int>& td,
                            const std::vector<float>& tw, std::vector<float>& y, float* onset) {
    y.assign((size_t)T, 0.f);
    *onset = FLT_MAX;
    for (int t = 0; t < T; ++t) {
        float acc = 0.f;
        for (size_t k = 0; k < tm.size(); ++k) {
            const long long ts = (long long)t - td[k];
            const float s = ts >= 0 && ts < T ? p[(size_t)tm[k] * T + (size_t)ts] : 0.f;
            const volatile float prod = tw[k] * s;  // (rounded on its own)
            acc = acc + prod;
        }
        y[(size_t)t] = acc;
        if (*onset == FLT_MAX && std::fabs(acc) > 0.00000316f) *onset = (float)t;
    }
}

static void checkResponse(int M, int T, int fs, int interp, bool edges) {
    std::vector<float> p((size_t)M * T);
    for (int m = 0; m < M; ++m) {
        const int t0 = (int)((rnd() + 1.f) * 20.f);
        for (int t = 0; t < T; ++t) p[(size_t)m * T + t] = t < t0 ? 0.f : rnd() * std::exp(-0.01f * (float)(t - t0));
    }
    std::vector<int> tm, td;
    std::vector<float> tw;
    for (int m = 0; m < M; ++m) {
        const float seconds = m % 3 == 0 ? 0.f : m % 3 == 1 ? (float)(2 + m % 38) / (float)fs : (1.01f + 30.f * (rnd() + 1.f)) / (float)fs;
        int d4[4];
        float w4[4];
        const int n = PvAmdHostArrayTaps(fs, T, rnd() * 1.5f, m == M - 1 && edges ? ((float)T - 1.5f) / (float)fs : seconds, interp, d4, w4);
        CHECK(n == 1 || n == 4);
        for (int k = 0; k < n; ++k) {
            tm.push_back(m);
            td.push_back(d4[k]);
            tw.push_back(w4[k]);
        }
    }
    if (edges) {  // below t = 0 and far past T - 1
        for (int d : {-1, -T, -T - 3, T, T + 7, std::numeric_limits<int>::max(), std::numeric_limits<int>::min()}) {
            tm.push_back(0);
            td.push_back(d);
            tw.push_back(0.5f);
        }
    }
    std::vector<float> got((size_t)T), want;
    float gon = -1.f, won = -1.f;
    CHECK(PvAmdHostArrayResponse(p.data(), M, T, tm.data(), td.data(), tw.data(), (int)tm.size(), got.data(), &gon) == 0);
    restateResponse(p, T, tm, td, tw, want, &won);
    for (int t = 0; t < T; ++t) CHECK(sameBits(got[(size_t)t], want[(size_t)t]));
    CHECK(gon == won);
}

int main() {
    const int fs = 1443, T = 435;
    // 1 taps
    const float gains[] = {1.f, -1.f, 0.37f, -2.5e-3f, 0.f, 3.0e20f};
    for (int interp : {PVA_ARRAY_NEAREST, PVA_ARRAY_LAGRANGE3})
        for (float g : gains) {
            for (int n : {0, 1, 2, 17, T - 3, T - 2, T - 1})
                for (double mu : {0.0, 1e-7, 1e-4, 0.25, 0.5, 0.75, 1.0 - 1e-4, 1.0 - 1e-6}) checkTaps(fs, T, g, (float)((n + mu) / fs), interp);
            checkTaps(fs, T, g, std::nextafter((float)T / (float)fs, 0.f), interp);
            checkTaps(fs, T, g, (float)T / (float)fs, interp);
            checkTaps(fs, T, g, ((float)T + 0.5f) / (float)fs, interp);
            checkTaps(fs, T, g, -1e-6f, interp);
            checkTaps(fs, T, g, std::numeric_limits<float>::quiet_NaN(), interp);
            checkTaps(fs, T, g, std::numeric_limits<float>::infinity(), interp);
            checkTaps(fs, T, std::numeric_limits<float>::quiet_NaN(), 0.01f, interp);
            checkTaps(fs, T, -std::numeric_limits<float>::infinity(), 0.01f, interp);
        }
    {
        int d4[4];
        float w4[4];
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, 0.4f / fs, PVA_ARRAY_LAGRANGE3, d4, w4) == -1);  // n = 0, mu != 0
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, 0.4f / fs, PVA_ARRAY_NEAREST, d4, w4) == 1 && d4[0] == 0);
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, ((float)T - 0.25f) / fs, PVA_ARRAY_NEAREST, d4, w4) == -1);  // rounds to T
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, ((float)T - 0.25f) / fs, PVA_ARRAY_LAGRANGE3, d4, w4) == 4 && d4[3] == T + 1);
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, 0.f, 2, d4, w4) == -1);
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, 0.f, 0, nullptr, w4) == -1);
        CHECK(PvAmdHostArrayTaps(fs, T, 1.f, 0.f, 0, d4, nullptr) == -1);
        CHECK(PvAmdHostArrayTaps(0, T, 1.f, 0.f, 0, d4, w4) == -1);
        CHECK(PvAmdHostArrayTaps(fs, 0, 1.f, 0.f, 0, d4, w4) == -1);
        CHECK(std::strncmp(PvAmdLastError(), "arrays:", 7) == 0);
    }
    // 2 responses
    for (int M : {1, 2, 17, 64})
        for (int interp : {PVA_ARRAY_NEAREST, PVA_ARRAY_LAGRANGE3}) {
            checkResponse(M, T, fs, interp, false);
            checkResponse(M, T, fs, interp, true);
        }
    // 3 the cancelling pair and the identity
    {
        std::vector<float> p((size_t)2 * T), y((size_t)T);
        for (int t = 0; t < T; ++t) p[(size_t)t] = p[(size_t)T + t] = t < 9 ? 0.f : rnd();
        for (int d : {0, 5}) {
            const int tm[2] = {0, 1}, td[2] = {d, d};
            const float tw[2] = {0.9f, -0.9f};
            float on = 0.f;
            CHECK(PvAmdHostArrayResponse(p.data(), 2, T, tm, td, tw, 2, y.data(), &on) == 0);
            for (int t = 0; t < T; ++t) {
                unsigned u;
                std::memcpy(&u, &y[(size_t)t], 4);
                CHECK(u == 0u);
            }
            CHECK(on == FLT_MAX);
        }
        const int tm = 0, td = 0;
        const float tw = 1.f;
        float on = 0.f;
        CHECK(PvAmdHostArrayResponse(p.data(), 1, T, &tm, &td, &tw, 1, y.data(), &on) == 0);
        for (int t = 0; t < T; ++t) CHECK(sameBits(y[(size_t)t], p[(size_t)t]));
        int first = -1;
        for (int t = 0; t < T && first < 0; ++t)
            if (std::fabs(p[(size_t)t]) > 0.00000316f) first = t;
        CHECK(first >= 9 && on == (float)first);
        // a NaN sample compares false: no onset from it
        std::vector<float> q((size_t)T, std::numeric_limits<float>::quiet_NaN());
        CHECK(PvAmdHostArrayResponse(q.data(), 1, T, &tm, &td, &tw, 1, y.data(), &on) == 0);
        CHECK(on == FLT_MAX && y[0] != y[0]);
        // no taps: +0 everywhere; the onset pointer is optional
        CHECK(PvAmdHostArrayResponse(p.data(), 1, T, nullptr, nullptr, nullptr, 0, y.data(), nullptr) == 0);
        for (int t = 0; t < T; ++t) CHECK(y[(size_t)t] == 0.f);
    }
    // 4 refusals
    {
        std::vector<float> p(8, 1.f), y(8);
        const int tm[2] = {0, 1}, td[2] = {0, 0};
        const float tw[2] = {1.f, 1.f};
        CHECK(PvAmdHostArrayResponse(nullptr, 1, 8, tm, td, tw, 1, y.data(), nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 8, tm, td, tw, 1, nullptr, nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 0, 8, tm, td, tw, 1, y.data(), nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 0, tm, td, tw, 1, y.data(), nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 8, tm, td, tw, -1, y.data(), nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 8, nullptr, td, tw, 1, y.data(), nullptr) == -1);
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 8, tm, td, tw, 2, y.data(), nullptr) == -1);  // member 1 of 1
        const int neg = -1;
        CHECK(PvAmdHostArrayResponse(p.data(), 1, 8, &neg, td, tw, 1, y.data(), nullptr) == -1);
        CHECK(std::strncmp(PvAmdLastError(), "arrays:", 7) == 0);
    }
    std::printf("arrays_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
