// stream_zone_maps_edges.cpp -- the edge cases of the accumulate passes of PvAmdSetZoneMaps as the host restates them
// (csrc/pv_metrics.h roomSumsAdvance, csrc/pv_spectrum.h spectrumAdvance: the step functions the kernel of csrc/pv_zone_maps.hip
// applies) in a program of their own, to be compiled with -fsanitize=address,undefined and run on the CPU
// (tests/test_host_stream_zone_maps.py): every array is sized exactly, so a sample read past p[T - 1] or a table row read past
// T - 1 is an ASan report.
//   1  onset >= tB: the pass changes nothing, whatever the sums hold;
//   2  tA >= T and a pass that reaches past T: nothing past T - 1 is read;
//   3  an empty pass (tA == tB), in front of, at and behind the onset;
//   4  an onset inside the pass: the sums start from +0.0f and what they held is never read;
//   5  chains of passes against the one-walk definitions (roomMetricsOfIr, spectrumOfIr), levels included, n = 1, 3, 17 and 32,
//      with NaN and inf samples, onsets 0, mid, T - 1 and within n50 of T.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pv_metrics.h"
#include "pv_spectrum.h"

using namespace pva;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            std::printf("line %d: %s\n", __LINE__, #c);            \
        }                                                          \
    } while (0)

static bool sameBits(const float* a, const float* b, int n) {
    for (int i = 0; i < n; ++i) {
        if (std::isnan(a[i]) && std::isnan(b[i])) continue;
        if (std::memcmp(&a[i], &b[i], 4) != 0) return false;
    }
    return true;
}

static unsigned lcg(unsigned& s) { return s = s * 1664525u + 1013904223u; }

static std::vector<float> signal(int T, int onset, unsigned seed, int poison) {
    std::vector<float> p((size_t)T, 0.f);
    for (int t = onset; t < T; ++t) p[(size_t)t] = ((float)(lcg(seed) >> 8) / 8388608.f - 1.f) * std::exp(-0.01f * (float)(t - onset));
    if (p[(size_t)onset] == 0.f) p[(size_t)onset] = 0.25f;
    const float inf = std::numeric_limits<float>::infinity();
    if (poison == 1) p[(size_t)onset] = std::numeric_limits<float>::quiet_NaN();
    if (poison == 2) p[(size_t)(T - 1)] = inf;
    if (poison == 3) p[(size_t)((onset + T) / 2)] = -inf;
    return p;
}

// the passes [0, step), [step, 2 step) .. up to and past T
static void chainRoom(const std::vector<float>& p, int fs, int onset, int step, RoomSums* s) {
    const int T = (int)p.size();
    for (int tA = 0; tA < T; tA += step) roomSumsAdvance(p.data(), T, fs, onset, tA, tA + step, s);
}

int main() {
    const int fs = 1443, n50 = roomMetricsN50(fs), n80 = roomMetricsN80(fs);
    const float junk = 123.5f;
    // 1 .. 4: the room sums
    {
        const int T = 160, onset = 70;
        const std::vector<float> p = signal(T, onset, 7u, 0);
        RoomSums s{junk, junk, junk, junk, junk, junk}, keep = s;
        roomSumsAdvance(p.data(), T, fs, onset, 0, 64, &s);     // onset >= tB
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
        roomSumsAdvance(p.data(), T, fs, onset, 0, onset, &s);  // ... exactly
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
        roomSumsAdvance(p.data(), T, fs, onset, 64, 64, &s);    // empty, in front of the onset
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
        roomSumsAdvance(p.data(), T, fs, onset, 64, 128, &s);   // the onset inside the pass: junk never read
        RoomSums w{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = onset; t < 128; ++t) roomSumsStep(w, p[(size_t)t], t - onset, n50, n80);
        CHECK(std::memcmp(&s, &w, sizeof(s)) == 0 && s.total > 0.f);
        keep = s;
        roomSumsAdvance(p.data(), T, fs, onset, 128, 128, &s);  // empty, behind the onset
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
        roomSumsAdvance(p.data(), T, fs, onset, onset, onset, &s);  // empty, at the onset
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
        roomSumsAdvance(p.data(), T, fs, onset, 128, 4096, &s);  // past T
        float one[kRoomMetricFloats];
        roomMetricsOfIr(p.data(), T, fs, onset, one);
        CHECK(sameBits(&s.e50, one + 4, 6));
        keep = s;
        roomSumsAdvance(p.data(), T, fs, onset, T, T + 64, &s);  // tA >= T
        roomSumsAdvance(p.data(), T, fs, onset, T + 5, T + 5, &s);
        CHECK(std::memcmp(&s, &keep, sizeof(s)) == 0);
    }
    // 5: chains against the one walk
    const int Ts[2] = {435, 160};
    for (int T : Ts) {
        const int onsets[5] = {0, T / 2, T - 1, T - n50 + 3, T - 5};
        for (int onset : onsets)
            for (int poison = 0; poison < 4; ++poison) {
                const std::vector<float> p = signal(T, onset, (unsigned)(T * 31 + onset * 7 + poison), poison);
                float one[kRoomMetricFloats];
                roomMetricsOfIr(p.data(), T, fs, onset, one);
                const int steps[5] = {96, 64, 1, T, 7};
                for (int step : steps) {
                    RoomSums s{junk, junk, junk, junk, junk, junk};
                    chainRoom(p, fs, onset, step, &s);
                    float got[kRoomMetricFloats];
                    roomMetricsDerive(s, fs, &got[0], &got[1], &got[2], &got[3]);
                    std::memcpy(got + 4, &s, sizeof(s));
                    CHECK(sameBits(got, one, kRoomMetricFloats));
                }
                // pass boundaries exactly at the onset, at onset + n50 and at onset + n80
                {
                    RoomSums s{junk, junk, junk, junk, junk, junk};
                    const int cuts[5] = {0, onset, onset + n50, onset + n80, T + 9};
                    for (int i = 0; i + 1 < 5; ++i)
                        if (cuts[i] < cuts[i + 1]) roomSumsAdvance(p.data(), T, fs, onset, cuts[i], cuts[i + 1], &s);
                    CHECK(sameBits(&s.e50, one + 4, 6));
                }
                const int bins[4] = {1, 3, 17, 32};
                for (int n : bins) {
                    std::vector<float> hz((size_t)n), c((size_t)T * n), sn((size_t)T * n), src((size_t)3 * n), want((size_t)3 * n);
                    for (int j = 0; j < n; ++j) hz[(size_t)j] = 20.f + 21.5f * (float)j;
                    CHECK(spectrumBinsError(hz.data(), n, fs) == nullptr);
                    spectrumTables(T, fs, hz.data(), n, c.data(), sn.data());
                    const std::vector<float> pulse = signal(T, 0, 99u, 0);
                    spectrumSource(pulse.data(), T, c.data(), sn.data(), n, src.data());
                    spectrumOfIr(p.data(), T, onset, c.data(), sn.data(), n, src.data(), want.data());
                    const int ssteps[4] = {96, 64, 1, T};
                    for (int step : ssteps) {
                        std::vector<float> reim((size_t)2 * n, junk), got((size_t)3 * n);
                        for (int tA = 0; tA < T; tA += step)
                            spectrumAdvance(p.data(), T, onset, tA, tA + step, c.data(), sn.data(), n, reim.data());
                        for (int j = 0; j < n; ++j) {
                            got[(size_t)3 * j] = reim[(size_t)2 * j];
                            got[(size_t)3 * j + 1] = reim[(size_t)2 * j + 1];
                            got[(size_t)3 * j + 2] = spectrumLevel(reim[(size_t)2 * j], reim[(size_t)2 * j + 1], src[(size_t)3 * j + 2]);
                        }
                        CHECK(sameBits(got.data(), want.data(), 3 * n));
                    }
                    // onset >= tB, tA >= T and the empty pass leave the sums alone
                    std::vector<float> reim((size_t)2 * n, junk), keep = reim;
                    if (onset > 0) spectrumAdvance(p.data(), T, onset, 0, onset, c.data(), sn.data(), n, reim.data());
                    spectrumAdvance(p.data(), T, onset, T, T + 64, c.data(), sn.data(), n, reim.data());
                    spectrumAdvance(p.data(), T, onset, onset, onset, c.data(), sn.data(), n, reim.data());
                    CHECK(reim == keep);
                }
            }
    }
    std::printf("stream_zone_maps_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
