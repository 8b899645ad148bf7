// pv_metrics.h -- room-acoustic metrics of one impulse response (clarity C50 / C80, definition D50, centre time Ts): the
// definition of include/planeverb_amd.h (PvAmdRoomMetrics), shared by the device pass (pv_metrics.hip) and the host
// restatement (PvAmdHostRoomMetrics).  All arithmetic is float32, every product and sum rounded on its own (-ffp-contract=off),
// every sum sequential in increasing t from +0.0f; log10f is glibc's (pv_libm.h, general form: the argument may be +inf).
#pragma once

#include "pv_libm.h"

namespace pva {

constexpr int kRoomMetricFloats = 10;  // c50, c80, d50, ts, e50, l50, e80, l80, total, moment

PV_HD inline int roomMetricsN50(int fs) { return (int)(0.05f * (float)fs); }
PV_HD inline int roomMetricsN80(int fs) { return (int)(0.08f * (float)fs); }

struct RoomSums {
    float e50, l50, e80, l80, total, moment;
};

// the four derived values; nothing is special-cased (an empty late window gives c = +inf, d50 = 1)
PV_HD inline void roomMetricsDerive(const RoomSums& s, int fs, float* c50, float* c80, float* d50, float* ts) {
    *c50 = 10.0f * pvLog10f(s.e50 / s.l50);
    *c80 = 10.0f * pvLog10f(s.e80 / s.l80);
    *d50 = s.e50 / (s.e50 + s.l50);
    *ts = (s.moment / s.total) / (float)fs;
}

// one sample of the definition: what p = p(onset + k) adds to the six sums.  The walk below and the in-run accumulate pass of
// sparse-emitter mode (pv_zone_maps.hip) are both this text
PV_HD inline void roomSumsStep(RoomSums& s, float p, int k, int n50, int n80) {
    const float e = p * p;
    s.e50 = s.e50 + (k < n50 ? e : 0.f);
    s.l50 = s.l50 + (k < n50 ? 0.f : e);
    s.e80 = s.e80 + (k < n80 ? e : 0.f);
    s.l80 = s.l80 + (k < n80 ? 0.f : e);
    s.total = s.total + e;
    const float m = (float)k * e;
    s.moment = s.moment + m;
}

// The sums carried over the steps [max(tA, onset), min(tB, T)) of one accumulate pass [tA, tB): a cell whose onset lies in the
// pass (onset >= tA) starts from +0.0f and never reads *s; one with an earlier onset goes on from what the pass before left
inline void roomSumsAdvance(const float* p, int T, int fs, int onset, int tA, int tB, RoomSums* s) {
    const int n50 = roomMetricsN50(fs), n80 = roomMetricsN80(fs);
    const int tEnd = tB < T ? tB : T;
    if (onset < 0 || onset >= tEnd) return;
    RoomSums r = onset >= tA ? RoomSums{0.f, 0.f, 0.f, 0.f, 0.f, 0.f} : *s;
    for (int t = onset > tA ? onset : tA; t < tEnd; ++t) roomSumsStep(r, p[t], t - onset, n50, n80);
    *s = r;
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T)
inline void roomMetricsOfIr(const float* p, int T, int fs, int onset, float out[kRoomMetricFloats]) {
    const int n50 = roomMetricsN50(fs), n80 = roomMetricsN80(fs);
    RoomSums s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int t = onset; t < T; ++t) roomSumsStep(s, p[t], t - onset, n50, n80);
    roomMetricsDerive(s, fs, &out[0], &out[1], &out[2], &out[3]);
    out[4] = s.e50;
    out[5] = s.l50;
    out[6] = s.e80;
    out[7] = s.l80;
    out[8] = s.total;
    out[9] = s.moment;
}

}  // namespace pva
