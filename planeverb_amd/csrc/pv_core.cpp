// pv_core.cpp -- see pv_core.h.  Host-side float32 index arithmetic; no fast-math.
#include "pv_core.h"

#include <cstdio>
#include <cstring>

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iomanip>
#include <limits>
#include <sstream>

namespace pva {

static void fillDerived(GridSpec& g) {
    // PvTypes.h:101 : IR seconds = sqrt2 * 12.5 / c + 0.25, a float constant expression
    const float irSeconds = kSqrt2 * 12.5f / kC + 0.25f;
    g.T = (int)(unsigned)((float)g.fs * irSeconds);            // Grid.cpp:55
    g.courant = kC * g.dt / g.dx;                              // FDTD.cpp:90
    g.nDir = (int)(kDryDirectionLen * (float)g.fs);            // Analyzer.cpp:171
    g.nDry = (int)(kDryGainLen * (float)g.fs);                 // Analyzer.cpp:170
    g.nWet = (int)(kWetGainLen * (float)g.fs);                 // Analyzer.cpp:237
    g.nCut = (int)(kSchroederOffset * (float)g.fs);            // Analyzer.cpp:286
    g.nFree = g.nDry + (int)((1.f / kC) * (float)(int)g.fs);   // FreeGrid.cpp:99
    g.NX = g.gx + 1;
    g.NY = g.gy + 1;
}

static void fillResolution(GridSpec& g, int res) {
    g.res = res;
    const float minWavelength = kC / (float)res;  // Grid.cpp:392
    g.dx = minWavelength / kPointsPerWavelength;  // :393
    g.dt = g.dx / (kC * 1.5f);                    // :394
    g.fs = (unsigned)(1.0f / g.dt);               // :395
}

GridSpec makeGridSpec(float sizeX, float sizeY, int res) {
    GridSpec g;
    fillResolution(g, res);
    g.sizeX = sizeX;
    g.sizeY = sizeY;
    g.gsx = (1.f / g.dx) * sizeX;  // Grid.cpp:48
    g.gsy = (1.f / g.dx) * sizeY;  // Grid.cpp:49
    g.gx = (int)g.gsx;
    g.gy = (int)g.gsy;
    fillDerived(g);
    return g;
}

GridSpec makeGridSpecCells(int gx, int gy, int res) {
    GridSpec g;
    fillResolution(g, res);
    g.gx = gx;
    g.gy = gy;
    g.gsx = (float)gx + 0.5f;
    g.gsy = (float)gy + 0.5f;
    g.sizeX = g.gsx * g.dx;
    g.sizeY = g.gsy * g.dx;
    fillDerived(g);
    return g;
}

std::vector<float> gaussianPulse(const GridSpec& g) {
    // Grid.cpp:12-27.  The 0.5 literal is a double, so sigma is evaluated in double and narrowed; pi is
    // acos(-1) narrowed to float BEFORE use.  expf is the host libm's, as in the reference.
    std::vector<float> out((size_t)g.T);
    const float samplingRate = (float)g.fs;
    const float maxFreq = (float)g.res;
    const float pi = (float)std::acos(-1.0);
    const float sigma = (float)(1.0f / (0.5 * pi * maxFreq));
    const float delay = 2 * sigma;
    const float dt = 1.0f / samplingRate;
    for (int i = 0; i < g.T; ++i) {
        const float t = (float)i * dt;
        out[(size_t)i] = std::exp(-(t - delay) * (t - delay) / (sigma * sigma));
    }
    return out;
}

// Bit parity of the pulse rides on the HOST libm's expf (glibc 2.35 in the reference build): a libm whose
// expf rounds differently would shift every field by an ulp and no test on that host would say why.  Checked once per
// process against five samples of the reference's own 275 Hz table (tests/golden/g71_*.npz `pulse`), incl. a denormal.
bool pulseMatchesReferenceLibm() {
    static const struct {
        int i;
        uint32_t bits;
    } kRef[] = {{0, 0x3c960aaeu}, {10, 0x3ebecae4u}, {20, 0x3405f3a0u}, {30, 0x1c4fb297u}, {40, 0x0000002cu}};
    const std::vector<float> p = gaussianPulse(makeGridSpec(25.f, 25.f, 275));
    for (const auto& r : kRef) {
        uint32_t b;
        std::memcpy(&b, &p[(size_t)r.i], 4);
        if (b != r.bits) return false;
    }
    return true;
}

void warnIfPulseDiffers() {
    static const bool ok = [] {
        const bool m = pulseMatchesReferenceLibm();
        if (!m)
            std::fprintf(stderr, "[planeverb_amd] warning: this host's expf does not reproduce the reference's Gaussian pulse "
                                 "table bit for bit (glibc 2.35 expected): fields and outputs may differ from the reference "
                                 "in the last place\n");
        return m;
    }();
    (void)ok;
}

void listenerCell(const GridSpec& g, float lx, float lz, int* cx, int* cy) {
    *cx = (int)((lx + 0.f) / g.dx);
    *cy = (int)((lz + 0.f) / g.dx);
}

void listenerCellRecip(const GridSpec& g, float lx, float lz, int* cx, int* cy) {
    *cx = (int)(lx * (1.f / g.dx));
    *cy = (int)(lz * (1.f / g.dx));
}

bool resultCell(const GridSpec& g, float ex, float ez, int* cx, int* cy) {
    const unsigned px = (unsigned)((ex + 0.f) / g.dx);
    const unsigned py = (unsigned)((ez + 0.f) / g.dx);
    // The reference tests `>` and so admits one row/column past the gx*gy result map; that read
    // is out of bounds there.  Here it is rejected.
    if (px >= (unsigned)g.gx || py >= (unsigned)g.gy) return false;
    *cx = (int)px;
    *cy = (int)py;
    return true;
}

void MaterialPlane::init(const GridSpec& g) {
    g_ = g;
    const size_t n = (size_t)g.NX * g.NY;
    beta_.assign(n, 1);
    by_.assign(n, 1);
    R_.assign(n, 0.f);
    for (int x = 0; x < g.NX; ++x)
        for (int y = 0; y < g.NY; ++y) {
            if (x == g.gx || y == g.gy) beta_[(size_t)x * g.NY + y] = by_[(size_t)x * g.NY + y] = 0;  // Grid.cpp:93-97
            else if (y == 0) by_[(size_t)x * g.NY + y] = 0;                                            // Grid.cpp:98-102
        }
    markAllDirty();
}

// ---------------------------------------------------------------------------------------------------------------
// shapes
// ---------------------------------------------------------------------------------------------------------------

bool makeShape(const float* xy, int n, float R, Shape* out, std::string* err) {
    auto refuse = [&](const char* why) {
        if (err) *err = why;
        return false;
    };
    if (!xy) return refuse("shape: no vertex list");
    if (n < 3 || n > kShapeMaxVerts) return refuse("shape: 3 to 8 vertices");
    if (!std::isfinite(R)) return refuse("shape with a non-finite absorption");
    for (int i = 0; i < 2 * n; ++i)
        if (!std::isfinite(xy[i])) return refuse("shape with a non-finite coordinate");
    // signed area and the turn at every vertex in double: a product of two floats is exact there, differences nearly so
    double area = 0, turnSum = 0;
    int pos = 0, neg = 0;
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1) % n, k = (i + 2) % n;
        const double ax = xy[2 * i], ay = xy[2 * i + 1], bx = xy[2 * j], by = xy[2 * j + 1], cx = xy[2 * k], cy = xy[2 * k + 1];
        area += ax * by - bx * ay;
        const double ux = bx - ax, uy = by - ay, vx = cx - bx, vy = cy - by;
        const double cr = ux * vy - uy * vx;
        pos += cr > 0;
        neg += cr < 0;
        turnSum += std::atan2(cr, ux * vx + uy * vy);
    }
    if (!(area != 0) || !std::isfinite(area)) return refuse("shape with zero area");
    // convex and simple: every turn one way (collinear vertices allowed), and the turns add up to one revolution (a pentagram's
    // add up to two)
    if ((pos && neg) || std::fabs(std::fabs(turnSum) - 2 * M_PI) > 1e-3) return refuse("shape: the vertex list is not convex");
    Shape s;
    s.n = n;
    s.R = R;
    for (int i = 0; i < n; ++i) {
        const int src = area > 0 ? i : n - 1 - i;  // clockwise lists are reversed
        s.xy[2 * i] = xy[2 * src];
        s.xy[2 * i + 1] = xy[2 * src + 1];
    }
    *out = s;
    return true;
}

bool makeRound(const float* xy, int n, float radius, float R, Shape* out, std::string* err) {
    auto refuse = [&](const char* why) {
        if (err) *err = why;
        return false;
    };
    if (!xy) return refuse("round shape: no point list");
    if (n < 1 || n > kPolyMaxVerts) return refuse("round shape: 1 to 64 points");
    if (!std::isfinite(R)) return refuse("round shape with a non-finite absorption");
    if (!std::isfinite(radius)) return refuse("round shape with a non-finite radius");
    if (!(radius > 0.f) || !(radius * radius > 0.f)) return refuse("round shape: the radius must be positive");
    if (!std::isfinite(radius * radius)) return refuse("round shape: the radius is too large");
    for (int i = 0; i < 2 * n; ++i)
        if (!std::isfinite(xy[i])) return refuse("round shape with a non-finite coordinate");
    for (int i = 0; i + 1 < n; ++i) {
        const float ex = xy[2 * i + 2] - xy[2 * i], ey = xy[2 * i + 3] - xy[2 * i + 1];
        if (!std::isfinite((ex * ex) + (ey * ey))) return refuse("round shape: a segment is too long");
    }
    Shape s;
    s.kind = kShapeRound;
    s.n = n;
    s.R = R;
    s.r = radius;
    std::memcpy(s.xy, xy, sizeof(float) * 2 * (size_t)n);
    *out = s;
    return true;
}

bool polygonSelfIntersects(const float* xy, int n) {
    struct P {
        double x, y;
    };
    auto pt = [&](int i) { return P{xy[2 * (i % n)], xy[2 * (i % n) + 1]}; };
    auto o = [](P p, P q, P r) { return (q.x - p.x) * (r.y - p.y) - (q.y - p.y) * (r.x - p.x); };
    auto inBox = [](P p, P q, P r) {
        return std::min(p.x, q.x) <= r.x && r.x <= std::max(p.x, q.x) && std::min(p.y, q.y) <= r.y && r.y <= std::max(p.y, q.y);
    };
    for (int i = 0; i < n; ++i) {
        const P p = pt(i), v = pt(i + 1), q = pt(i + 2);
        if (p.x == v.x && p.y == v.y) return true;  // zero-length edge
        if (o(p, v, q) == 0 && (p.x - v.x) * (q.x - v.x) + (p.y - v.y) * (q.y - v.y) > 0) return true;  // fold-back
    }
    for (int i = 0; i < n; ++i)
        for (int j = i + 2; j < n; ++j) {
            if (i == 0 && j == n - 1) continue;  // neighbours through the closing vertex
            const P p1 = pt(i), p2 = pt(i + 1), p3 = pt(j), p4 = pt(j + 1);
            const double d1 = o(p3, p4, p1), d2 = o(p3, p4, p2), d3 = o(p1, p2, p3), d4 = o(p1, p2, p4);
            if (((d1 > 0 && d2 < 0) || (d1 < 0 && d2 > 0)) && ((d3 > 0 && d4 < 0) || (d3 < 0 && d4 > 0))) return true;
            if ((d1 == 0 && inBox(p3, p4, p1)) || (d2 == 0 && inBox(p3, p4, p2)) || (d3 == 0 && inBox(p1, p2, p3)) ||
                (d4 == 0 && inBox(p1, p2, p4)))
                return true;
        }
    return false;
}

bool makePolygon(const float* xy, int n, float R, Shape* out, std::string* err) {
    auto refuse = [&](const char* why) {
        if (err) *err = why;
        return false;
    };
    if (!xy) return refuse("polygon: no vertex list");
    if (n < 3 || n > kPolyMaxVerts) return refuse("polygon: 3 to 64 vertices");
    if (!std::isfinite(R)) return refuse("polygon with a non-finite absorption");
    for (int i = 0; i < 2 * n; ++i)
        if (!std::isfinite(xy[i])) return refuse("polygon with a non-finite coordinate");
    double area = 0;  // (shoelace in double, as makeShape)
    for (int i = 0; i < n; ++i) {
        const int j = (i + 1) % n;
        area += (double)xy[2 * i] * xy[2 * j + 1] - (double)xy[2 * j] * xy[2 * i + 1];
    }
    if (!(area != 0) || !std::isfinite(area)) return refuse("polygon with zero area");
    if (polygonSelfIntersects(xy, n)) return refuse("polygon: the vertex list intersects itself");
    Shape s;
    s.kind = kShapePolygon;
    s.n = n;
    s.R = R;
    std::memcpy(s.xy, xy, sizeof(float) * 2 * (size_t)n);
    *out = s;
    return true;
}

bool orientedBoxVertices(float px, float py, float w, float h, float ax, float ay, float out8[8], std::string* err) {
    if (!(std::isfinite(px) && std::isfinite(py) && std::isfinite(w) && std::isfinite(h) && std::isfinite(ax) && std::isfinite(ay))) {
        if (err) *err = "oriented box with a non-finite input";
        return false;
    }
    const float len2 = ax * ax + ay * ay;
    if (!(len2 > 0.f) || !std::isfinite(len2)) {
        if (err) *err = "oriented box with a zero (or too long) axis";
        return false;
    }
    const float inv = 1.0f / std::sqrt(len2);
    const float ux = ax * inv, uy = ay * inv;
    const float vx = -uy, vy = ux;
    const float hw = w / 2.f, hh = h / 2.f;
    const float wx = hw * ux, wy = hw * uy, hx = hh * vx, hy = hh * vy;
    // c - w u - h v, c + w u - h v, c + w u + h v, c - w u + h v: counter-clockwise for w, h > 0
    out8[0] = (px - wx) - hx;
    out8[1] = (py - wy) - hy;
    out8[2] = (px + wx) - hx;
    out8[3] = (py + wy) - hy;
    out8[4] = (px + wx) + hx;
    out8[5] = (py + wy) + hy;
    out8[6] = (px - wx) + hx;
    out8[7] = (py - wy) + hy;
    return true;
}

bool shapeCovers(const Shape& s, float dx, int x, int y) {
    const float px = ((float)x + 0.5f) * dx, py = ((float)y + 0.5f) * dx;
    if (s.kind == kShapeRound) {
        const float rr = s.r * s.r;
        const int segs = s.n > 1 ? s.n - 1 : 1;
        for (int i = 0; i < segs; ++i) {
            const int j = i + 1 < s.n ? i + 1 : i;
            const float ax = s.xy[2 * i], ay = s.xy[2 * i + 1];
            const float ex = s.xy[2 * j] - ax, ey = s.xy[2 * j + 1] - ay;
            const float wx = px - ax, wy = py - ay;
            const float ee = (ex * ex) + (ey * ey);
            float t = 0.f;
            if (ee != 0.f) {
                t = ((wx * ex) + (wy * ey)) / ee;
                t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
            }
            const float qx = wx - (t * ex), qy = wy - (t * ey);
            if ((qx * qx) + (qy * qy) <= rr) return true;
        }
        return false;
    }
    if (s.kind == kShapePolygon) {
        bool in = false;
        for (int i = 0; i < s.n; ++i) {
            const int j = i + 1 == s.n ? 0 : i + 1;
            const float ax = s.xy[2 * i], ay = s.xy[2 * i + 1], bx = s.xy[2 * j], by = s.xy[2 * j + 1];
            if ((ay > py) != (by > py) && px < (((bx - ax) * (py - ay)) / (by - ay)) + ax) in = !in;
        }
        return in;
    }
    for (int i = 0; i < s.n; ++i) {
        const int j = i + 1 == s.n ? 0 : i + 1;
        const float ax = s.xy[2 * i], ay = s.xy[2 * i + 1];
        const float ex = s.xy[2 * j] - ax, ey = s.xy[2 * j + 1] - ay;
        if (!((ex * (py - ay)) - (ey * (px - ax)) >= 0.f)) return false;
    }
    return true;
}

void shapeCellBounds(const Shape& s, const GridSpec& g, int* x0, int* x1, int* y0, int* y1) {
    double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL}, m = std::max(g.gsx, g.gsy) * (double)g.dx;
    for (int i = 0; i < s.n; ++i)
        for (int a = 0; a < 2; ++a) {
            lo[a] = std::min(lo[a], (double)s.xy[2 * i + a]);
            hi[a] = std::max(hi[a], (double)s.xy[2 * i + a]);
            m = std::max(m, std::fabs((double)s.xy[2 * i + a]));
        }
    // a round shape reaches r beyond its points: q = w - t e with 0 <= t <= 1 stays within rounding of the segment's box, and
    // q.q <= r r holds |q.x|, |q.y| to r (1 + 2^-22).  A polygon's crossing rule compares P.y with the vertices exactly, and its
    // float32 intersection abscissa leaves the vertices' x range by a few ulp(m) at most.  The pad below covers both.
    if (s.kind == kShapeRound) {
        for (int a = 0; a < 2; ++a) {
            lo[a] -= (double)s.r;
            hi[a] += (double)s.r;
        }
        m += (double)s.r;
    }
    // the float32 edge function can accept a centre up to ~16 ulp(m) outside an edge: 2 cells plus that, in cells
    const double pad = 2.0 + std::ceil(m * 4e-6 / g.dx);
    const int n[2] = {g.gx, g.gy};
    int r[4];
    for (int a = 0; a < 2; ++a) {
        const double c0 = std::floor(lo[a] / g.dx - 0.5 - pad), c1 = std::ceil(hi[a] / g.dx - 0.5 + pad) + 1;
        r[2 * a] = (int)std::max(0.0, std::min((double)n[a], c0));
        r[2 * a + 1] = (int)std::max(0.0, std::min((double)n[a], c1));
    }
    *x0 = r[0];
    *x1 = r[1];
    *y0 = r[2];
    *y1 = r[3];
}

void MaterialPlane::bounds(const Box& b, int* sx, int* sy, int* ex, int* ey) const {
    // Grid.cpp:139-142 : multiply by the reciprocal of dx, truncate toward zero
    const float inv = 1.f / g_.dx;
    *sy = (int)((b.y - b.h / 2.f + 0.f) * inv);
    *sx = (int)((b.x - b.w / 2.f + 0.f) * inv);
    *ey = (int)((b.y + b.h / 2.f + 0.f) * inv);
    *ex = (int)((b.x + b.w / 2.f + 0.f) * inv);
}

void MaterialPlane::add(const Box& b) {
    int sx, sy, ex, ey;
    bounds(b, &sx, &sy, &ex, &ey);
    for (int y = sy; y < ey; ++y) {
        if (!(y >= 0 && (float)y <= g_.gsy)) continue;  // Grid.cpp:231
        for (int x = sx; x < ex; ++x) {
            if (!(x >= 0 && (float)x <= g_.gsx)) continue;  // Grid.cpp:235
            const size_t i = (size_t)x * g_.NY + y;
            R_[i] = b.R;
            beta_[i] = 0;
            by_[i] = 0;  // Grid.cpp:241-242
            dirtyLo_ = std::min(dirtyLo_, x);
            dirtyHi_ = std::max(dirtyHi_, x + 1);
        }
    }
}

void MaterialPlane::remove(const Box& b) {
    int sx, sy, ex, ey;
    bounds(b, &sx, &sy, &ex, &ey);
    for (int y = sy; y < ey; ++y) {
        if (!(y >= 0 && (float)y <= g_.gsy)) continue;
        for (int x = sx; x < ex; ++x) {
            if (!(x >= 0 && (float)x <= g_.gsx)) continue;
            const size_t i = (size_t)x * g_.NY + y;
            R_[i] = 0.f;
            // Grid.cpp:276 tests (y == gx || x == gy); identical to the ghost test on square grids, which
            // are the only self-consistent ones.  The ghost row/column is always beta = 0 here.
            beta_[i] = (x == g_.gx || y == g_.gy) ? 0 : 1;
            // Grid.cpp:281-290: by comes back as 0 on the x == 0 ROW ("j == 0", j being x), not on the y == 0 column
            // the constructor cleared
            by_[i] = (x == g_.gx || y == g_.gy || x == 0) ? 0 : 1;
            dirtyLo_ = std::min(dirtyLo_, x);
            dirtyHi_ = std::max(dirtyHi_, x + 1);
        }
    }
}

void MaterialPlane::clearDirty() {
    dirtyLo_ = g_.NX;
    dirtyHi_ = 0;
}

void MaterialPlane::markAllDirty() {
    dirtyLo_ = 0;
    dirtyHi_ = g_.NX;
}

bool loadPv(const std::string& path, std::vector<Box>* out, std::string* err) {
    std::ifstream f(path);
    if (!f.is_open()) {
        if (err) *err = "cannot open scene file: " + path;
        return false;
    }
    size_t n = 0;
    f >> n;
    out->clear();
    for (size_t i = 0; i < n; ++i) {
        long long id;  // read and discarded, Editor.cpp:271,278
        Box b;
        f >> id >> b.x >> b.y >> b.w >> b.h >> b.R;
        if (!f) {
            if (err) *err = "truncated scene file: " + path;
            return false;
        }
        out->push_back(b);
    }
    return true;
}

bool savePv(const std::string& path, const std::vector<std::pair<int, Box>>& boxes, std::string* err) {
    std::ofstream f(path);
    if (!f.is_open()) {
        if (err) *err = "cannot write scene file: " + path;
        return false;
    }
    // max_digits10: every float survives the text round trip, so a saved scene rasterises to the same cells (the
    // Editor writes 6 significant digits, Editor.cpp:229-241; its operator>> loader reads either form)
    f << std::setprecision(std::numeric_limits<float>::max_digits10);
    f << boxes.size() << std::endl;  // Editor.cpp:229-230
    for (const auto& p : boxes) {
        const Box& b = p.second;
        f << p.first << " " << b.x << " " << b.y << " " << b.w << " " << b.h << " " << b.R << std::endl;
    }
    return true;
}

void reverbBusGains(float rt60, float wet, float* a, float* b, float* c) {
    // three reverb buses with decay times 0.5 / 1.0 / 3.0 s (PvDSPTypes.h:13-15); g(T) = 10^(-3*0.1/T)
    const float t1 = 0.5f, t2 = 1.0f, t3 = 3.0f, tstar = 0.1f;
    auto g = [&](float T) { return std::pow(10.f, -3.f * tstar / T); };
    if (rt60 > t2) *a = 0.f;
    else if (rt60 < t1) *a = 1.f;
    else *a = wet * (g(t2) - g(rt60)) / (g(t2) - g(t1));

    if (rt60 < t1) *b = 0.f;
    else if (rt60 > t2) *b = wet * (g(t3) - g(rt60)) / (g(t3) - g(t2));
    else *b = wet - wet * (g(t2) - g(rt60)) / (g(t2) - g(t1));

    if (rt60 > t3) *c = 1.f;
    else if (rt60 < t2) *c = 0.f;
    else *c = wet - wet * (g(t3) - g(rt60)) / (g(t3) - g(t2));
}

std::vector<SegRect> planSegments(const uint8_t* air, int ntx, int nty, int rxi, int wmax, int target) {
    struct Rect {
        int ti0, nt, tj0, w;
    };
    std::vector<Rect> rects;
    std::vector<SegRect> out;
    if (ntx <= 0 || nty <= 0 || rxi <= 0 || wmax <= 0) return out;
    wmax = std::min(wmax, 7);  // (the chunk key below has 3 bits for the width)
    std::vector<int> open((size_t)nty * 8, -1), next((size_t)nty * 8, -1);
    for (int ti = 0; ti < ntx; ++ti) {
        std::fill(next.begin(), next.end(), -1);
        const uint8_t* row = air + (size_t)ti * nty;
        for (int tj = 0; tj < nty;) {
            if (!row[tj]) {
                ++tj;
                continue;
            }
            int e = tj;
            while (e < nty && row[e]) ++e;
            for (int c = tj; c < e; c += wmax) {
                const int w = std::min(wmax, e - c);
                const size_t key = (size_t)c * 8 + (size_t)w;
                int r = open[key];
                if (r >= 0 && rects[(size_t)r].ti0 + rects[(size_t)r].nt == ti) {
                    ++rects[(size_t)r].nt;
                } else {
                    r = (int)rects.size();
                    rects.push_back({ti, 1, c, w});
                }
                next[key] = r;
            }
            tj = e;
        }
        open.swap(next);
    }
    long long totalRows = 0;
    for (const Rect& r : rects) totalRows += (long long)r.nt * rxi;
    const long long want = (totalRows + std::max(target, 1) - 1) / std::max(target, 1);
    const int Xt = (int)std::min<long long>(7LL * rxi, std::max<long long>(rxi / 2 + 1, want));
    for (const Rect& r : rects) {
        const int rows = r.nt * rxi;
        const int m = (rows + Xt - 1) / Xt;
        for (int k = 0; k < m; ++k) {
            const int r0 = (int)((long long)rows * k / m), r1 = (int)((long long)rows * (k + 1) / m);
            out.push_back(SegRect{r.ti0 * rxi + r0, r1 - r0, r.tj0, r.w});
        }
    }
    std::sort(out.begin(), out.end(), [](const SegRect& x, const SegRect& y) {
        return x.row0 != y.row0 ? x.row0 < y.row0 : x.tj0 < y.tj0;
    });
    return out;
}

// ----------------------------------------------------------------------------------------------------------------
// triangle meshes (pv_core.h; the device side is pv_mesh.hip)
// ----------------------------------------------------------------------------------------------------------------

bool validateMeshTransform(const float* m12, std::string* err) {
    if (!m12) {
        if (err) *err = "mesh: no transform";
        return false;
    }
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(m12[i])) {
            if (err) *err = "mesh with a non-finite transform entry";
            return false;
        }
    return true;
}

bool validateMesh(const float* verts, int nv, const int* tris, int nt, float R, int mode, float radius, std::string* err) {
    auto refuse = [&](const char* why) {
        if (err) *err = why;
        return false;
    };
    if (!verts || !tris) return refuse("mesh: no vertex or triangle list");
    if (mode != kMeshSolid && mode != kMeshShell) return refuse("mesh: unknown mode");
    if (nv < 1) return refuse("mesh: no vertices");
    if (nt < 1) return refuse("mesh: at least one triangle");
    if (nt > kMeshMaxTris) return refuse("mesh: more than 1 << 20 triangles");
    if (!std::isfinite(R)) return refuse("mesh with a non-finite absorption");
    if (mode == kMeshShell) {
        if (!std::isfinite(radius)) return refuse("mesh with a non-finite radius");
        if (!(radius > 0.f) || !(radius * radius > 0.f)) return refuse("mesh: the shell radius must be positive");
        if (!std::isfinite(radius * radius)) return refuse("mesh: the shell radius is too large");
    }
    for (size_t i = 0; i < (size_t)3 * nv; ++i)
        if (!std::isfinite(verts[i])) return refuse("mesh with a non-finite vertex");
    for (int i = 0; i < nt; ++i) {
        const int a = tris[3 * i], b = tris[3 * i + 1], c = tris[3 * i + 2];
        if (a < 0 || a >= nv || b < 0 || b >= nv || c < 0 || c >= nv) return refuse("mesh: a vertex index outside [0, nv)");
        if (a == b || b == c || c == a) return refuse("mesh: a triangle with two equal indices");
    }
    if (mode != kMeshSolid) return true;
    // closedness: every undirected edge in exactly two triangles (open addressing over (min, max) keys)
    size_t cap = 16;
    while (cap < (size_t)6 * nt) cap <<= 1;
    std::vector<uint64_t> keys(cap, ~(uint64_t)0);
    std::vector<uint8_t> count(cap, 0);
    for (int i = 0; i < nt; ++i)
        for (int e = 0; e < 3; ++e) {
            const unsigned a = (unsigned)tris[3 * i + e], b = (unsigned)tris[3 * i + (e + 1) % 3];
            const uint64_t key = ((uint64_t)std::min(a, b) << 32) | std::max(a, b);
            size_t slot = (size_t)((key * 0x9E3779B97F4A7C15ull) >> 20) & (cap - 1);
            while (keys[slot] != key && keys[slot] != ~(uint64_t)0) slot = (slot + 1) & (cap - 1);
            keys[slot] = key;
            if (++count[slot] > 2) return refuse("mesh: a solid mesh's edge is shared by more than two triangles");
        }
    for (size_t s = 0; s < cap; ++s)
        if (count[s] == 1) return refuse("mesh: a solid mesh must be closed (an edge belongs to one triangle only)");
    return true;
}

void meshSection(const float* verts, const int* tris, int nt, const float* m12, float h, float* out4, uint8_t* valid) {
    for (int i = 0; i < nt; ++i) {
        float p[3][3];
        for (int k = 0; k < 3; ++k) {
            const float* v = verts + (size_t)3 * tris[3 * i + k];
            for (int r = 0; r < 3; ++r)
                p[k][r] = m12 ? ((m12[4 * r] * v[0] + m12[4 * r + 1] * v[1]) + m12[4 * r + 2] * v[2]) + m12[4 * r + 3] : v[r];
        }
        const bool up[3] = {p[0][1] > h, p[1][1] > h, p[2][1] > h};
        float* o = out4 + (size_t)4 * i;
        o[0] = o[1] = o[2] = o[3] = 0.f;
        valid[i] = 0;
        if (up[0] == up[1] && up[1] == up[2]) continue;
        int n = 0;
        for (int e = 0; e < 3; ++e) {
            const int e2 = e == 2 ? 0 : e + 1;
            if (up[e] == up[e2]) continue;
            const float* lo = up[e] ? p[e2] : p[e];
            const float* hi = up[e] ? p[e] : p[e2];
            const float t = (h - lo[1]) / (hi[1] - lo[1]);
            o[2 * n] = lo[0] + (t * (hi[0] - lo[0]));
            o[2 * n + 1] = lo[2] + (t * (hi[2] - lo[2]));
            ++n;
        }
        valid[i] = 1;
    }
}

int meshCrossingPrefix(float xi, float dx, int gx) {
    const float kf = std::ceil(xi / dx - 0.5f);
    if (!(kf >= 0.f)) return 0;  // (left of the grid, or NaN)
    int k = kf >= (float)gx ? gx : (int)kf;
    while (k > 0 && !(((float)(k - 1) + 0.5f) * dx < xi)) --k;
    while (k < gx && ((float)k + 0.5f) * dx < xi) ++k;
    return k;
}

void meshCoverage(const GridSpec& g, const float* seg4, const uint8_t* valid, int nt, int mode, float radius, uint8_t* cover) {
    const int NY = g.NY, gx = g.gx, gy = g.gy;
    const float dx = g.dx;
    std::memset(cover, 0, (size_t)g.NX * NY);
    // rows (or columns) n of 0 .. cells whose centre can lie in [lo - pad, hi + pad]; everything when a bound is not finite
    auto range = [&](float lo, float hi, double pad, int cells, int* c0, int* c1) {
        *c0 = 0;
        *c1 = cells;
        if (!std::isfinite(lo) || !std::isfinite(hi)) return;
        const double a = std::floor((double)lo / dx - 0.5 - pad), b = std::ceil((double)hi / dx - 0.5 + pad) + 1;
        *c0 = (int)std::max(0.0, std::min((double)cells, a));
        *c1 = (int)std::max(0.0, std::min((double)cells, b));
    };
    const float rr = radius * radius;
    for (int i = 0; i < nt; ++i) {
        if (!valid[i]) continue;
        const float ax = seg4[4 * (size_t)i], ay = seg4[4 * (size_t)i + 1], bx = seg4[4 * (size_t)i + 2], by = seg4[4 * (size_t)i + 3];
        int x0, x1, y0, y1;
        if (mode == kMeshSolid) {
            range(std::min(ay, by), std::max(ay, by), 1.0, gy, &y0, &y1);
            for (int y = y0; y < y1; ++y) {
                const float py = ((float)y + 0.5f) * dx;
                if ((ay > py) == (by > py)) continue;
                const int k = meshCrossingPrefix((((bx - ax) * (py - ay)) / (by - ay)) + ax, dx, gx);
                if (k > 0) cover[(size_t)(k - 1) * NY + y] ^= 1;  // a mark: the suffix XOR below turns marks into coverage
            }
            continue;
        }
        double m = std::max(g.gsx, g.gsy) * (double)dx;
        for (float c : {ax, ay, bx, by}) m = std::max(m, std::fabs((double)c));
        const double pad = 2.0 + std::ceil((m + radius) * 4e-6 / dx);  // (as shapeCellBounds for a round shape)
        range(std::min(ax, bx) - radius, std::max(ax, bx) + radius, pad, gx, &x0, &x1);
        range(std::min(ay, by) - radius, std::max(ay, by) + radius, pad, gy, &y0, &y1);
        const float ex = bx - ax, ey = by - ay, ee = (ex * ex) + (ey * ey);
        for (int x = x0; x < x1; ++x) {
            const float wx = ((float)x + 0.5f) * dx - ax;
            for (int y = y0; y < y1; ++y) {
                const float wy = ((float)y + 0.5f) * dx - ay;
                float t = 0.f;
                if (ee != 0.f) {
                    t = ((wx * ex) + (wy * ey)) / ee;
                    t = t < 0.f ? 0.f : (t > 1.f ? 1.f : t);
                }
                const float qx = wx - (t * ex), qy = wy - (t * ey);
                if ((qx * qx) + (qy * qy) <= rr) cover[(size_t)x * NY + y] = 1;
            }
        }
    }
    if (mode == kMeshSolid)
        for (int x = gx - 2; x >= 0; --x)
            for (int y = 0; y < gy; ++y) cover[(size_t)x * NY + y] ^= cover[(size_t)(x + 1) * NY + y];
}

const char* edgeLayerRefusal(int gx, int gy, const int w4[4]) {
    for (int k = 0; k < 4; ++k)
        if (w4[k] < 0 || w4[k] > kEdgeLayerMaxWidth) return "edge layer widths run from 0 to 64 cells";
    if ((w4[0] > 0 || w4[1] > 0) && gx - w4[0] - w4[1] < kEdgeLayerMinInterior)
        return "edge layers along x leave fewer than 8 interior cells";
    if ((w4[2] > 0 || w4[3] > 0) && gy - w4[2] - w4[3] < kEdgeLayerMinInterior)
        return "edge layers along y leave fewer than 8 interior cells";
    return "";
}

// one axis of n = g cells (+ the ghost): cell and face tables for layers of widths wlo (index 0 side) and whi (index g side)
static void axisTables(int g, int wlo, int whi, double C, double r0, float* ap, float* bp, float* a, float* b) {
    auto sOf = [&](double depth, int w) {
        if (w <= 0 || depth <= 0.0) return 0.0;
        const double smax = 3.0 * C * std::log(1.0 / r0) / (4.0 * w);
        const double u = depth / w;
        return smax * (u * u);
    };
    for (int x = 0; x <= g; ++x) {
        double sc = 0.0, sf = 0.0;
        if (x < g) {  // (the ghost cell x = g lies outside every layer)
            if (x < wlo) sc += sOf(wlo - x - 0.5, wlo);
            if (x >= g - whi) sc += sOf(x + 0.5 - (g - whi), whi);
        }
        if (x <= wlo) sf += sOf((double)(wlo - x), wlo);
        if (x >= g - whi) sf += sOf((double)(x - (g - whi)), whi);
        ap[x] = (float)((1.0 - sc) / (1.0 + sc));
        bp[x] = (float)(1.0 / (1.0 + sc));
        a[x] = (float)((1.0 - sf) / (1.0 + sf));
        b[x] = (float)(1.0 / (1.0 + sf));
    }
}

void edgeLayerTables(int gx, int gy, float courant, const int w4[4], float* out, double r0) {
    const int nx = gx + 1, ny = gy + 1;
    float* o = out;
    axisTables(gx, w4[0], w4[1], (double)courant, r0, o, o + nx, o + 2 * nx, o + 3 * nx);
    o += 4 * nx;
    axisTables(gy, w4[2], w4[3], (double)courant, r0, o, o + ny, o + 2 * ny, o + 3 * ny);
}

Enclosure findEnclosure(const uint8_t* beta, int NX, int NY, int seedX, int seedY, int rxi, int wi, int maxTiles,
                        std::vector<int>* visited) {
    Enclosure e{};
    if (visited) visited->clear();
    if (seedX < 0 || seedX >= NX || seedY < 0 || seedY >= NY || maxTiles < 1 || !beta[(size_t)seedX * NY + seedY]) return e;
    const long long cap = (long long)maxTiles * rxi * wi;  // cells of the largest window: no component beyond that fits
    // the cells seen so far: an open-addressing table sized for the cap (nothing of the grid's size is touched)
    size_t tab = 1024;
    while ((long long)tab < 2 * cap + 16) tab <<= 1;
    std::vector<int> seen(tab, -1);
    auto mark = [&](int i) {  // true: i was not in the table yet
        size_t h = ((size_t)(unsigned)i * 2654435761u) & (tab - 1);
        while (seen[h] >= 0) {
            if (seen[h] == i) return false;
            h = (h + 1) & (tab - 1);
        }
        seen[h] = i;
        return true;
    };
    std::vector<int> todo;
    todo.push_back(seedX * NY + seedY);
    mark(todo[0]);
    e.r0 = e.r1 = seedX;
    e.c0 = e.c1 = seedY;
    bool fits = true;
    auto window = [&]() {
        const int lo = std::max(e.r0 - 1, 0), hi = std::min(e.r1 + 1, NX - 1);
        const int lc = std::max(e.c0 - 1, 0), hc = std::min(e.c1 + 1, NY - 1);
        e.ti0 = lo / rxi;
        e.tis = hi / rxi - e.ti0 + 1;
        e.tj0 = lc / wi;
        e.tjs = hc / wi - e.tj0 + 1;
        return (long long)e.tis * e.tjs <= maxTiles;
    };
    for (size_t head = 0; head < todo.size() && fits; ++head) {
        const int i = todo[head], x = i / NY, y = i - x * NY;
        if (x < e.r0 || x > e.r1 || y < e.c0 || y > e.c1) {
            e.r0 = std::min(e.r0, x);
            e.r1 = std::max(e.r1, x);
            e.c0 = std::min(e.c0, y);
            e.c1 = std::max(e.c1, y);
            fits = window();
        }
        if (!fits) break;
        const int nb[4] = {x > 0 ? i - NY : -1, x + 1 < NX ? i + NY : -1, y > 0 ? i - 1 : -1, y + 1 < NY ? i + 1 : -1};
        for (int j : nb)
            if (j >= 0 && beta[(size_t)j] && mark(j)) {
                if ((long long)todo.size() >= cap) {  // one cell more than any window holds
                    fits = false;
                    break;
                }
                todo.push_back(j);
            }
    }
    // (the queue's cells are all marked air cells of the component; on a give-up the unprocessed ones count as visited too)
    e.cells = (int)todo.size();
    for (int i : todo) {
        const int x = i / NY, y = i - x * NY;
        e.r0 = std::min(e.r0, x);
        e.r1 = std::max(e.r1, x);
        e.c0 = std::min(e.c0, y);
        e.c1 = std::max(e.c1, y);
    }
    const bool w = window();
    e.found = fits && w ? 1 : 0;
    if (visited) {
        std::sort(todo.begin(), todo.end());
        visited->swap(todo);
    }
    return e;
}

PlaneClear planClear(bool windowRun, const int win[4], const int prevRect[4], bool planesDirty, bool sweptDirty, bool splitPlanes) {
    if (planesDirty || sweptDirty) return PlaneClear::All;
    const bool same = win[1] > 0 && win[3] > 0 && std::equal(win, win + 4, prevRect);
    return (windowRun && same && !splitPlanes) ? PlaneClear::None : PlaneClear::Rect;
}

// ----------------------------------------------------------------------------------------------------------------
// which path a run takes (pv_core.h)
// ----------------------------------------------------------------------------------------------------------------

RunPlan planRun(const PathCaps& c, const PathRun& r) {
    RunPlan p;
    p.kind = r.kind;
    const bool run = r.kind == PathRun::Run;
    // -- the launch form -------------------------------------------------------------------------------------------
    // merged: one launch per K steps on one stream (no cross-stream hand-shake); not with the streaming kernel
    // (a layer: always merged -- setEdgeLayer refused the configurations without a merged kernel)
    p.oneLaunch = c.stacked || ((c.merged == 1 || r.layerTiles) && c.mergedOk);
    p.plainMerged = plainMergedLaunch(c);
    p.layer = r.layerTiles;  // the layer tiles, behind the merged launch on the same stream (disjoint tiles)
    p.patch = c.usePatch && !r.layerTiles;
    // the replayed graph: automatic up to 4096 tiles; it holds no timing events, and the sparse-emitter ring is driven from the host
    const bool graph = !c.timeKernels && !c.streaming && (c.useGraph == 1 || (c.useGraph == 0 && c.ntiles <= 4096));
    // row bands: a run that is not replayed from a graph, and raw stepping; never the callers that drive the launches themselves
    // (a layer: one launch per sweep beside the layer launch)
    const bool bandsWanted = run ? !graph : r.kind == PathRun::Raw;
    p.banded = bandsWanted && c.bands > 1 && !r.layerActive;
    p.segments = c.useSeg && !p.banded && !r.layerActive && r.segmentsFound;
    if (!run) return p;  // (Launches, full sweeps)

    // -- the path --------------------------------------------------------------------------------------------------
    // (an explicit tile configuration means "use the tile kernels")
    // The whole-grid-resident kernel wins where a run is a chain of tiny launches even as a replayed graph: measured on
    // MI355X (profiles/r03_presets.txt) 0.47 vs 0.62 ms at 28^2 and 0.67 vs 0.82 ms at 38^2 -- but 0.81 vs 0.69 ms at 39^2,
    // 0.88 vs 0.71 ms at the Sandbox's 70^2 and 1.60 vs 0.97 ms at 95^2, where its two barriers per step over 5-9 cells per
    // thread are slower than the 4-wave general tiles.  auto = up to 1536 array cells; 1 = whenever the grid fits one CU.
    const bool smallWanted = c.smallGrid == 1 || (c.smallGrid == 0 && c.cells <= 1536);
    const bool small = smallWanted && !c.explicitTile && !c.timeKernels && c.useGraph != 1 && !c.streaming && c.smallFits &&
                       c.wholeWindow && !r.layerActive;
    // reach-bounded (Solver::setReachArgs): the plain merged-launch path of a run whose listener lies inside the grid
    // (DESIGN.md 4.1); every other path sweeps the grid and leaves fields anywhere
    p.reach = c.reachBound != 0 && p.plainMerged && !graph && !small && !c.useResident && !c.streaming && !p.banded && !p.segments &&
              !c.usePatch && !c.denseHistory && !c.edgeTiles && !c.slab && c.timeKernels == 0 && r.listenerInside;
    // resident kernel: one launch per run; it loses to the small-grid kernel unless asked for by name
    const bool resident = c.useResident && !(small && c.resident != 1) && !r.layerActive;
    const StepPath tiles = graph ? StepPath::Graph : StepPath::Launches;
    if (c.streaming) {
        p.path = StepPath::Streaming;  // sparse-emitter mode: ring history; forward sums advanced after every `ring` steps
    } else if (p.reach && c.windowOk && !r.windowOff && !r.layerActive) {
        p.path = StepPath::Window;     // (reach-eligible runs never have useResident; whether the listener is walled in: the solver)
    } else if (resident) {
        p.path = StepPath::Resident;
    } else if (small) {
        p.path = StepPath::SmallGrid;
    } else {
        p.path = tiles;
    }
    p.fallback = p.path == StepPath::Resident ? (small ? StepPath::SmallGrid : tiles)
                 : (p.path == StepPath::Window || p.path == StepPath::Graph) ? StepPath::Launches
                                                                             : p.path;
    return p;
}

}  // namespace pva
