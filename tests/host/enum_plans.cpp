// tests/host/enum_plans.cpp -- TEST INFRASTRUCTURE: pva::planRun (pv_core.h) over the product of its inputs' values, for
// tests/test_host_run_plan.py.  The inputs are the digits of a mixed-radix index, least significant first, in the order of
// kFields; every field takes each value a rule of planRun can tell apart.
//   enum_plans fields                  the fields: "name v0 v1 ..." per line, in digit order
//   enum_plans all                     the plans of all indices, in order, as little-endian uint16 on stdout
//   enum_plans plan [name=value ...]   one plan as text, from the defaults of PathCaps / PathRun and the values given
// A plan as 16 bits: path | fallback << 3 | oneLaunch << 6 | plainMerged << 7 | banded << 8 | segments << 9 | patch << 10 |
// reach << 11 | layer << 12.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pv_core.h"

using namespace pva;

static const char* stepPathName(StepPath p) {
    static const char* const names[] = {"Streaming", "Window", "Resident", "SmallGrid", "Graph", "Launches"};
    return names[(int)p];
}

struct Inputs {
    PathCaps c;
    PathRun r;
};
struct Field {
    const char* name;
    std::vector<long long> values;
    void (*set)(Inputs&, long long);
};
#define F(name, member, ...) \
    Field { name, {__VA_ARGS__}, [](Inputs& in, long long v) { in.member = (decltype(in.member))v; } }
static const std::vector<Field> kFields = {
    F("stacked", c.stacked, 0, 1),
    F("mergedOk", c.mergedOk, 0, 1),
    F("merged", c.merged, 0, 1),
    F("timeKernels", c.timeKernels, 0, 1),
    F("streaming", c.streaming, 0, 1),
    F("denseHistory", c.denseHistory, 0, 1),
    F("edgeTiles", c.edgeTiles, 0, 1),
    F("slab", c.slab, 0, 1),
    F("ntiles", c.ntiles, 4096, 4097),
    F("bands", c.bands, 1, 2),
    F("useSeg", c.useSeg, 0, 1),
    F("usePatch", c.usePatch, 0, 1),
    F("useResident", c.useResident, 0, 1),
    F("windowOk", c.windowOk, 0, 1),
    F("explicitTile", c.explicitTile, 0, 1),
    F("smallFits", c.smallFits, 0, 1),
    F("wholeWindow", c.wholeWindow, 0, 1),
    F("cells", c.cells, 1536, 1537),
    F("reachBound", c.reachBound, -1, 0, 1),
    F("useGraph", c.useGraph, 0, 1, 2),
    F("smallGrid", c.smallGrid, 0, 1, 2),
    F("resident", c.resident, 0, 1, 2),
    F("kind", r.kind, 0, 1, 2),
    F("listenerInside", r.listenerInside, 0, 1),
    F("layerActive", r.layerActive, 0, 1),
    F("layerTiles", r.layerTiles, 0, 1),
    F("windowOff", r.windowOff, 0, 1),
    F("segmentsFound", r.segmentsFound, 0, 1),
};

static unsigned code(const RunPlan& p) {
    return (unsigned)p.path | (unsigned)p.fallback << 3 | p.oneLaunch << 6 | p.plainMerged << 7 | p.banded << 8 | p.segments << 9 |
           p.patch << 10 | p.reach << 11 | p.layer << 12;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "fields") {
        for (const Field& f : kFields) {
            std::printf("%s", f.name);
            for (long long v : f.values) std::printf(" %lld", v);
            std::printf("\n");
        }
        return 0;
    }
    if (mode == "all") {
        Inputs in;
        std::vector<size_t> digit(kFields.size(), 0);
        for (const Field& f : kFields) f.set(in, f.values[0]);
        std::vector<uint16_t> out;
        out.reserve(1 << 20);
        for (;;) {
            out.push_back((uint16_t)code(planRun(in.c, in.r)));
            if (out.size() == (1u << 20)) {
                if (std::fwrite(out.data(), 2, out.size(), stdout) != out.size()) return 1;  // (the reader has gone)
                out.clear();
            }
            size_t k = 0;  // the next index: an odometer step
            for (; k < kFields.size(); ++k) {
                digit[k] = digit[k] + 1 < kFields[k].values.size() ? digit[k] + 1 : 0;
                kFields[k].set(in, kFields[k].values[digit[k]]);
                if (digit[k]) break;
            }
            if (k == kFields.size()) break;
        }
        std::fwrite(out.data(), 2, out.size(), stdout);
        return 0;
    }
    if (mode == "plan") {
        Inputs in;
        for (int a = 2; a < argc; ++a) {
            const char* eq = std::strchr(argv[a], '=');
            bool known = false;
            for (const Field& f : kFields)
                if (eq && std::string(argv[a], (size_t)(eq - argv[a])) == f.name) {
                    f.set(in, std::atoll(eq + 1));
                    known = true;
                }
            if (!known) {
                std::fprintf(stderr, "unknown field: %s\n", argv[a]);
                return 2;
            }
        }
        const RunPlan p = planRun(in.c, in.r);
        std::printf("%s fallback=%s oneLaunch=%d plainMerged=%d banded=%d segments=%d patch=%d reach=%d layer=%d code=%u\n",
                    stepPathName(p.path), stepPathName(p.fallback), p.oneLaunch, p.plainMerged, p.banded, p.segments, p.patch, p.reach,
                    p.layer, code(p));
        return 0;
    }
    std::fprintf(stderr, "usage: enum_plans fields | all | plan [name=value ...]\n");
    return 2;
}
