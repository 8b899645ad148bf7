// zone_band_decay_edges.cpp -- the edge cases of the zone band decay's host restatement (csrc/pv_zone_band_decay.h) in a program of
// their own, to be compiled with -fsanitize=address,undefined and run on the CPU (tests/test_zone_band_decay_cpu.py): every array
// is sized exactly, so an index outside a history, a curve, a coefficient set or a label map is an ASan report.
//   1  gy that is no multiple of 64 (70), onsets 0 and T - 1, an empty zone, 8 bands, both alignments;
//   2  T = 1: one sample per member, every clarity window past the curve's end;
//   3  the identity coefficients give the broadband restatement's curves and shared fields;
//   4  the clarity of a curve at j0 = T - 1 and of an all-zero curve; the chunk rule at its corners.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pv_zone_band_decay.h"

using namespace pva;

static int failures = 0;
#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            ++failures;                                            \
            std::printf("line %d: %s\n", __LINE__, #c);            \
        }                                                          \
    } while (0)

struct Case {
    int gx, gy, T, fs, nZones, nBands;
    std::vector<float> p, delay, coefs;
    std::vector<unsigned char> labels;
    std::vector<ZoneBandDecay> out;
    std::vector<double> etc, edc;
    Case(int gx_, int gy_, int T_, int fs_, int nz, int nb) : gx(gx_), gy(gy_), T(T_), fs(fs_), nZones(nz), nBands(nb) {
        p.assign((size_t)T * gx * gy, 1.0e3f);  // (what lies below an onset must never count)
        delay.assign((size_t)gx * gy, FLT_MAX);
        labels.assign((size_t)gx * gy, 0);
        coefs.resize((size_t)kBandCoefs * nb);
        out.resize((size_t)nz * nb);
        etc.resize((size_t)nz * nb * T);
        edc.resize((size_t)nz * nb * T);
    }
    // octave bands from fs / 6 downwards
    void octaves() {
        std::vector<float> hz((size_t)nBands);
        for (int b = 0; b < nBands; ++b) hz[(size_t)b] = (float)fs / 6.0f / (float)(1 << b);
        CHECK(bandsError(hz.data(), nBands, 1, fs) == nullptr);
        bandCoefs(fs, hz.data(), nBands, 1, coefs.data());
    }
    void identity() {
        for (int b = 0; b < nBands; ++b)
            for (int k = 0; k < kBandCoefs; ++k) coefs[(size_t)b * kBandCoefs + k] = k % 5 == 0 ? 1.0f : 0.0f;
    }
    // cell (X, Y): zone z, onset t0, p(t) = a * g^(t - t0) with alternating sign from the onset on
    void cell(int X, int Y, int z, int t0, float a, float g) {
        const size_t s = (size_t)X * gy + Y;
        labels[s] = (unsigned char)z;
        delay[s] = (float)t0;
        float v = a;
        for (int t = t0; t < T; ++t, v *= -g) p[(size_t)t * gx * gy + s] = v;
    }
    void run(int align) {
        CHECK(zoneLabelsError(labels.data(), (long long)gx * gy, nZones) == nullptr);
        CHECK(zoneDecayOnsetsError(delay.data(), labels.data(), (long long)gx * gy, T) == nullptr);
        std::memset(out.data(), 0xff, out.size() * sizeof(ZoneBandDecay));
        zoneBandDecayOfHistory(p.data(), delay.data(), gx, gy, T, fs, labels.data(), nZones, coefs.data(), nBands, align, out.data(),
                               etc.data(), edc.data());
    }
};

static void checkEmpty(const ZoneBandDecay& r) {
    CHECK(r.n_cells == 0 && r.t_first == -1 && r.t_last == -1 && r.n_edt == 0 && r.n_t20 == 0 && r.n_t30 == 0);
    CHECK(r.e0 == 0.0 && !std::signbit(r.e0));
    CHECK(std::isnan(r.edt) && std::isnan(r.t20) && std::isnan(r.t30) && std::isnan(r.depth));
    CHECK(std::isnan(r.c50) && std::isnan(r.c80) && std::isnan(r.d50) && std::isnan(r.ts));
}

int main() {
    for (int align = 0; align < 2; ++align) {
        {  // 1
            Case c(3, 70, 48, 400, 3, 8);
            c.octaves();
            for (int Y = 0; Y < 70; ++Y) {
                c.cell(0, Y, 1, Y % 5, 1.0f + (float)Y, 0.9f);
                c.cell(1, Y, 1 + Y % 2, Y == 69 ? 47 : 0, 0.5f, 0.8f);
            }
            c.labels[(size_t)2 * 70 + 3] = 3;  // unreached: zone 3 is empty
            c.run(align);
            for (int b = 0; b < 8; ++b) {
                const ZoneBandDecay &r1 = c.out[(size_t)b], &r2 = c.out[(size_t)8 + b];
                CHECK(r1.n_cells == 70 + 35 && r1.t_first == 0 && r1.t_last == 4);
                CHECK(r2.n_cells == 35 && r2.t_first == 0 && r2.t_last == 47);
                checkEmpty(c.out[(size_t)16 + b]);
                for (int z = 0; z < 3; ++z) {
                    const size_t at = ((size_t)z * 8 + b) * c.T;
                    CHECK(c.out[(size_t)z * 8 + b].e0 == c.edc[at]);
                    for (int j = 0; j + 1 < c.T; ++j) CHECK(c.edc[at + j] >= c.edc[at + j + 1]);
                    CHECK(c.edc[at + c.T - 1] == c.etc[at + c.T - 1]);
                    for (int j = 0; j < c.T; ++j) CHECK(z == 2 ? c.etc[at + j] == 0.0 : c.etc[at + j] >= 0.0);
                }
                CHECK(r1.e0 > 0.0 && r1.d50 > 0.0 && r1.d50 <= 1.0 && r1.ts >= 0.0);
            }
            // the bands differ
            CHECK(std::memcmp(&c.etc[0], &c.etc[(size_t)c.T], sizeof(double) * (size_t)c.T) != 0);
        }
        {  // 2
            Case c(2, 5, 1, 400, 2, 2);
            c.octaves();
            c.cell(0, 4, 1, 0, 2.0f, 0.5f);
            c.cell(1, 0, 1, 0, 3.0f, 0.5f);
            c.run(align);
            for (int b = 0; b < 2; ++b) {
                const ZoneBandDecay& r = c.out[(size_t)b];
                const float y2 = c.coefs[(size_t)b * kBandCoefs + 5] * (c.coefs[(size_t)b * kBandCoefs] * 2.0f);
                const float y3 = c.coefs[(size_t)b * kBandCoefs + 5] * (c.coefs[(size_t)b * kBandCoefs] * 3.0f);
                CHECK(r.n_cells == 2 && r.t_first == 0 && r.t_last == 0);
                CHECK(c.etc[(size_t)b] == (double)y2 * (double)y2 + (double)y3 * (double)y3);
                CHECK(r.e0 == c.etc[(size_t)b] && std::isnan(r.edt) && std::isnan(r.depth));
                CHECK(std::isinf(r.c50) && r.c50 > 0.0 && r.d50 == 1.0 && r.ts == 0.0);
                checkEmpty(c.out[(size_t)2 + b]);
            }
        }
        {  // 3
            Case c(2, 65, 30, 400, 2, 2);
            c.identity();
            for (int Y = 0; Y < 65; ++Y) c.cell(Y & 1, Y, 1 + Y % 2, Y % 9, 1.0f + (float)Y, 0.7f);
            c.cell(1, 64, 2, 29, 4.0f, 0.5f);
            c.run(align);
            std::vector<ZoneDecay> w(2);
            std::vector<double> wetc((size_t)2 * 30), wedc((size_t)2 * 30);
            zoneDecayOfHistory(c.p.data(), c.delay.data(), c.gx, c.gy, c.T, c.fs, c.labels.data(), 2, align, w.data(), wetc.data(), wedc.data());
            for (int z = 0; z < 2; ++z)
                for (int b = 0; b < 2; ++b) {
                    const size_t at = ((size_t)z * 2 + b) * 30;
                    CHECK(std::memcmp(&c.etc[at], &wetc[(size_t)z * 30], 30 * sizeof(double)) == 0);
                    CHECK(std::memcmp(&c.edc[at], &wedc[(size_t)z * 30], 30 * sizeof(double)) == 0);
                    const ZoneBandDecay& r = c.out[(size_t)z * 2 + b];
                    CHECK(std::memcmp(&r.edt, &w[(size_t)z].edt, 5 * sizeof(double)) == 0);
                    CHECK(std::memcmp(&r.n_edt, &w[(size_t)z].n_edt, 6 * sizeof(int)) == 0);
                }
        }
    }
    {  // 4
        std::vector<double> e(7, 0.0), out(4);
        zoneCurveClarity(e.data(), 7, 400, 0, out.data());
        CHECK(std::isnan(out[0]) && std::isnan(out[1]) && std::isnan(out[2]) && std::isnan(out[3]));
        e[6] = 2.0;
        zoneCurveClarity(e.data(), 7, 400, 6, out.data());
        CHECK(std::isinf(out[0]) && std::isinf(out[1]) && out[2] == 1.0 && out[3] == 0.0);
        zoneCurveClarity(e.data(), 7, 100, 0, out.data());  // n50 = 5, n80 = 8: the sample is late for 50 ms, early for 80 ms
        CHECK(std::isinf(out[0]) && out[0] < 0.0 && std::isinf(out[1]) && out[1] > 0.0 && out[2] == 0.0 && out[3] == 6.0 / 100.0);
        int zp = 0, bp = 0;
        CHECK(zoneBandDecayChunks(64, 128, 5, 3, (size_t)32 << 20, &zp, &bp) == 1 && zp == 5 && bp == 3);
        CHECK(zoneBandDecayChunks(1024, 1024, 5, 3, (size_t)32 << 20, &zp, &bp) == 5 && zp == 1 && bp == 3);  // 8 MiB a pair
        CHECK(zoneBandDecayChunks(1024, 2048, 5, 3, (size_t)32 << 20, &zp, &bp) == 10 && zp == 1 && bp == 2);  // 16 MiB a pair
        CHECK(zoneBandDecayChunks(4096, 4096, 2, 3, (size_t)32 << 20, &zp, &bp) == 6 && zp == 1 && bp == 1);   // 128 MiB a pair
    }
    std::printf("zone_band_decay_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
