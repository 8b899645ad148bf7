// zone_decay_edges.cpp -- the edge cases of the zone decay's host restatement (csrc/pv_zone_decay.h) in a program of their own, to be
// compiled with -fsanitize=address,undefined and run on the CPU (tests/test_zone_decay_cpu.py): every array is sized exactly, so
// an index outside a history, a curve or a label map is an ASan report.
//   1  a zone whose cells are all unreached, and a zone without cells;
//   2  ABSOLUTE with t_first >= T - tailN: nothing before the tail;
//   3  ONSET with t_last >= T - tailN: jEnd <= 0;
//   4  a range with fewer than two points;
//   5  onsets 0 and T - 1, gy of one block and one cell more, both alignments: edc[0] == e0, edc non-increasing.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pv_zone_decay.h"

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
    int gx, gy, T, fs, nZones;
    std::vector<float> p, delay;
    std::vector<unsigned char> labels;
    std::vector<ZoneDecay> out;
    std::vector<double> etc, edc;
    Case(int gx_, int gy_, int T_, int fs_, int nz) : gx(gx_), gy(gy_), T(T_), fs(fs_), nZones(nz) {
        p.assign((size_t)T * gx * gy, 1.0e3f);  // (what lies below an onset must never count)
        delay.assign((size_t)gx * gy, FLT_MAX);
        labels.assign((size_t)gx * gy, 0);
        out.resize((size_t)nz);
        etc.resize((size_t)nz * T);
        edc.resize((size_t)nz * T);
    }
    // cell (X, Y): zone z, onset t0, p(t) = a * g^(t - t0) from the onset on
    void cell(int X, int Y, int z, int t0, float a, float g) {
        const size_t s = (size_t)X * gy + Y;
        labels[s] = (unsigned char)z;
        delay[s] = (float)t0;
        float v = a;
        for (int t = t0; t < T; ++t, v *= g) p[(size_t)t * gx * gy + s] = v;
    }
    void run(int align) {
        CHECK(zoneLabelsError(labels.data(), (long long)gx * gy, nZones) == nullptr);
        CHECK(zoneDecayOnsetsError(delay.data(), labels.data(), (long long)gx * gy, T) == nullptr);
        std::memset(out.data(), 0xff, out.size() * sizeof(ZoneDecay));
        zoneDecayOfHistory(p.data(), delay.data(), gx, gy, T, fs, labels.data(), nZones, align, out.data(), etc.data(), edc.data());
    }
};

static void checkEmpty(const ZoneDecay& r) {
    CHECK(r.n_cells == 0 && r.t_first == -1 && r.t_last == -1 && r.n_edt == 0 && r.n_t20 == 0 && r.n_t30 == 0);
    CHECK(r.e0 == 0.0 && !std::signbit(r.e0));
    CHECK(std::isnan(r.edt) && std::isnan(r.t20) && std::isnan(r.t30) && std::isnan(r.depth));
}

int main() {
    for (int align = 0; align < 2; ++align) {
        {  // 1
            Case c(3, 5, 30, 400, 2);
            c.labels[4] = c.labels[7] = 1;  // unreached; zone 2 has no cell
            c.run(align);
            checkEmpty(c.out[0]);
            checkEmpty(c.out[1]);
            for (double v : c.etc) CHECK(v == 0.0);
            for (double v : c.edc) CHECK(v == 0.0);
        }
        {  // 2, 3: tailN = 4, T = 30: the tail begins at 26
            Case c(2, 65, 30, 400, 1);
            c.cell(0, 64, 1, 26, 1.0f, 0.5f);
            c.cell(1, 0, 1, 29, 2.0f, 0.5f);
            c.run(align);
            const ZoneDecay& r = c.out[0];
            CHECK(r.n_cells == 2 && r.t_first == 26 && r.t_last == 29);
            CHECK(std::isnan(r.edt) && std::isnan(r.t20) && std::isnan(r.t30) && std::isnan(r.depth));
            CHECK(r.n_edt == 0 && r.n_t20 == 0 && r.n_t30 == 0);
            CHECK(r.e0 == c.edc[align == kZoneDecayAbsolute ? 26 : 0] && r.e0 == c.edc[0] && r.e0 > 4.0);
        }
        {  // 4: 12 dB a step: the EDT range holds the first point only; T20 and T30 hold two
            Case c(1, 64, 40, 400, 1);
            c.cell(0, 63, 1, 0, 1.0f, 0.25f);
            c.run(align);
            const ZoneDecay& r = c.out[0];
            CHECK(r.n_edt == 1 && std::isnan(r.edt));
            CHECK(r.n_t20 == 2 && r.t20 > 0.0);
            CHECK(r.n_t30 == 2 && r.t30 > 0.0);
            CHECK(r.depth < -100.0);
        }
        {  // 5
            Case c(3, 65, 36, 400, 3);
            for (int Y = 0; Y < 65; ++Y) {
                c.cell(0, Y, 1, Y % 7, 1.0f + (float)Y, 0.7f);
                c.cell(1, Y, 1 + Y % 3, Y == 64 ? 35 : 0, 0.5f, 0.8f);
                c.cell(2, Y, 2, 35 - Y % 36, 3.0f, 0.6f);
            }
            c.run(align);
            for (int z = 0; z < 3; ++z) {
                const double* e = c.edc.data() + (size_t)z * c.T;
                CHECK(c.out[(size_t)z].e0 == e[0]);
                for (int j = 0; j + 1 < c.T; ++j) CHECK(e[j] >= e[j + 1]);
                CHECK(e[c.T - 1] == c.etc[(size_t)z * c.T + c.T - 1]);
            }
            CHECK(c.out[0].t_first == 0 && c.out[1].t_last == 35);
        }
    }
    // an onset outside the run, a label above nZones
    {
        Case c(1, 3, 10, 400, 1);
        c.labels[1] = 1;
        c.delay[1] = 10.0f;
        CHECK(zoneDecayOnsetsError(c.delay.data(), c.labels.data(), 3, c.T) != nullptr);
        c.delay[1] = -1.0f;
        CHECK(zoneDecayOnsetsError(c.delay.data(), c.labels.data(), 3, c.T) != nullptr);
        c.labels[1] = 2;
        CHECK(zoneLabelsError(c.labels.data(), 3, 1) != nullptr);
    }
    std::printf("zone_decay_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
