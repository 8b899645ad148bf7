// stream_zone_tiles_edges.cpp -- the edge cases of what a sparse-emitter run derives from the zones' labels (csrc/pv_zone_decay.h:
// zoneTileFlags, zoneTileUnion, streamZoneCurveChunk) and the scratch layout of the curve passes (zoneCurveScratch) in a program
// of their own, to be compiled with -fsanitize=address,undefined and run on the CPU (tests/test_host_stream_zone_decay.py): every
// array is sized exactly, so a flag written past the tile plane or a label read past the map is an ASan report.
//   1  no labelled cell: no flag, the empty box;
//   2  one labelled cell in each corner of the grid, on grids that are no multiple of the tile or of 64;
//   3  labels on the last row / column of a tile and on Y = 63 / 64;
//   4  a grid smaller than one tile and smaller than one block;
//   5  the union with either side missing, and with no tile at all;
//   6  the chunk: whole groups within the bound, one group where the bound is below one;
//   7  the scratch of a curve pass: increasing offsets, every region 8-byte aligned (a member record is 12 bytes, so an odd
//      nZones x gx needs the padding), and the total the passes have always asked for.
#include <cstdio>
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
    int gx, gy, rxi, wi, ntx, nty;
    std::vector<unsigned char> labels, flags;
    Case(int gx_, int gy_, int rxi_, int wi_) : gx(gx_), gy(gy_), rxi(rxi_), wi(wi_) {
        ntx = (gx + rxi - 1) / rxi;
        nty = (gy + wi - 1) / wi;
        labels.assign((size_t)gx * gy, 0);
        flags.assign((size_t)ntx * nty, 7);  // (every flag must be written)
    }
    void set(int X, int Y, int z = 1) { labels[(size_t)X * gy + Y] = (unsigned char)z; }
    ZoneTileBox run() { return zoneTileFlags(labels.data(), gx, gy, rxi, wi, flags.data()); }
    int flag(int ti, int tj) const { return flags[(size_t)ti * nty + tj]; }
    int count() const {
        int n = 0;
        for (unsigned char f : flags) {
            CHECK(f <= 1);
            n += f;
        }
        return n;
    }
};

static bool boxIs(const ZoneTileBox& b, int r0, int r1, int b0, int b1) { return b.row0 == r0 && b.row1 == r1 && b.blk0 == b0 && b.blk1 == b1; }

int main() {
    const int shapes[][4] = {{70, 70, 12, 40}, {70, 70, 24, 48}, {252, 280, 12, 36}, {280, 252, 24, 48}, {5, 3, 12, 40}, {64, 64, 8, 24}, {65, 129, 8, 24}};
    for (const auto& s : shapes) {
        const int gx = s[0], gy = s[1], rxi = s[2], wi = s[3];
        {  // 1
            Case c(gx, gy, rxi, wi);
            CHECK(boxIs(c.run(), 0, -1, 0, -1));
            CHECK(c.count() == 0);
        }
        {  // 2
            Case c(gx, gy, rxi, wi);
            c.set(0, 0), c.set(0, gy - 1, 2), c.set(gx - 1, 0, 3), c.set(gx - 1, gy - 1, 64);
            CHECK(boxIs(c.run(), 0, gx - 1, 0, (gy - 1) / 64));
            CHECK(c.flag(0, 0) && c.flag(0, c.nty - 1) && c.flag(c.ntx - 1, 0) && c.flag(c.ntx - 1, c.nty - 1));
            CHECK(c.count() == (c.ntx > 1 ? 2 : 1) * (c.nty > 1 ? 2 : 1));
        }
        if (gx > rxi && gy > 64 && gy > wi) {  // 3
            Case c(gx, gy, rxi, wi);
            c.set(rxi - 1, wi - 1);
            CHECK(boxIs(c.run(), rxi - 1, rxi - 1, (wi - 1) / 64, (wi - 1) / 64));
            CHECK(c.count() == 1 && c.flag(0, 0));
            c.set(rxi, wi);
            CHECK(boxIs(c.run(), rxi - 1, rxi, (wi - 1) / 64, wi / 64));
            CHECK(c.count() == 2 && c.flag(1, 1));
            Case d(gx, gy, rxi, wi);
            d.set(gx / 2, 63);
            CHECK(boxIs(d.run(), gx / 2, gx / 2, 0, 0));
            d.set(gx / 2, 64);
            CHECK(boxIs(d.run(), gx / 2, gx / 2, 0, 1));
            Case e(gx, gy, rxi, wi);
            e.set(gx / 2, 64);
            CHECK(boxIs(e.run(), gx / 2, gx / 2, 1, 1));
        }
        {  // every cell labelled: every tile
            Case c(gx, gy, rxi, wi);
            for (auto& l : c.labels) l = 1;
            CHECK(boxIs(c.run(), 0, gx - 1, 0, (gy - 1) / 64));
            CHECK(c.count() == c.ntx * c.nty);
        }
    }
    {  // 5
        const unsigned char a[4] = {1, 0, 0, 2}, b[4] = {0, 0, 1, 1};
        std::vector<unsigned char> out(4, 9);
        zoneTileUnion(a, b, 4, out.data());
        CHECK(out[0] == 1 && out[1] == 0 && out[2] == 1 && out[3] == 1);
        zoneTileUnion(a, nullptr, 4, out.data());
        CHECK(out[0] == 1 && out[1] == 0 && out[2] == 0 && out[3] == 1);
        zoneTileUnion(nullptr, b, 4, out.data());
        CHECK(out[0] == 0 && out[1] == 0 && out[2] == 1 && out[3] == 1);
        zoneTileUnion(nullptr, nullptr, 4, out.data());
        CHECK(out[0] == 0 && out[1] == 0 && out[2] == 0 && out[3] == 0);
        std::vector<unsigned char> none;
        zoneTileUnion(nullptr, nullptr, 0, none.data());
    }
    {  // 6
        const size_t bound = 32u << 20;
        for (int nz : {1, 5, 64})
            for (int rows : {1, 70, 820, 4096, 16384}) {
                const int c = streamZoneCurveChunk(nz, rows, bound);
                CHECK(c >= kZoneCurveSlots && c % kZoneCurveSlots == 0 && c <= kZoneCurveMaxChunk);
                const size_t bytes = (size_t)c * nz * rows * sizeof(double);
                CHECK(bytes <= bound || c == kZoneCurveSlots);
                if (c < kZoneCurveMaxChunk) CHECK((size_t)(c + kZoneCurveSlots) * nz * rows * sizeof(double) > bound);
            }
        CHECK(streamZoneCurveChunk(64, 4096, bound) == 16);
        CHECK(streamZoneCurveChunk(64, 16384, bound) == 16);  // (one group is more than the bound: one group all the same)
        CHECK(streamZoneCurveChunk(1, 1, 0) == 16);
        CHECK(streamZoneCurveChunk(0, 0, bound) == kZoneCurveMaxChunk);
    }
    {  // 7
        static_assert(sizeof(ZoneMembers) == 12, "the padding below counts on it");
        const int T = 435;
        for (int nz : {1, 5, 64})
            for (int gx : {1, 70, 401}) {
                const size_t curve = (size_t)nz * T * sizeof(double), group = (size_t)kZoneCurveSlots * nz * gx * sizeof(double);
                // zone decay (a chunk of slots), zone band decay with three bands (a chunk of pairs), a sparse-emitter solver (members only)
                const size_t sizes[][2] = {{group, curve}, {(size_t)nz * 3 * gx * T * sizeof(double), 3 * curve}, {0, 0}};
                for (const auto& b : sizes) {
                    const ZoneCurveScratch s = zoneCurveScratch(b[0], b[1], nz, gx);
                    CHECK(s.rows == 0 && s.etc == s.rows + b[0] && s.memberRows == s.etc + b[1]);
                    CHECK(s.rows <= s.etc && s.etc <= s.memberRows && s.memberRows < s.members && s.members < s.total);
                    CHECK(s.rows % 8 == 0 && s.etc % 8 == 0 && s.memberRows % 8 == 0 && s.members % 8 == 0);
                    CHECK(s.members - s.memberRows >= (size_t)nz * gx * sizeof(ZoneMembers));
                    CHECK(s.members - s.memberRows < (size_t)nz * gx * sizeof(ZoneMembers) + 8);
                    const size_t memberRowsBytes = ((size_t)nz * (size_t)gx * sizeof(ZoneMembers) + 7) / 8 * 8;
                    CHECK(s.total == b[0] + b[1] + memberRowsBytes + (size_t)nz * sizeof(ZoneMembers));
                }
            }
        CHECK(zoneCurveScratch(0, 0, 1, 1).members == 16);  // (12 bytes of member rows, padded)
        CHECK(zoneCurveScratch(0, 0, 5, 401).members == 24064);  // (24060, padded)
    }
    std::printf("stream_zone_tiles_edges: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
