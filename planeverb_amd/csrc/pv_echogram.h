// pv_echogram.h -- directional echogram (energy and flux per time slot) of one impulse response with its particle velocity: the
// definition of include/planeverb_amd.h (PvAmdSetEchogram .. PvAmdHostEchogram), shared by the device pass (pv_echogram.hip)
// and the host restatement (PvAmdHostEchogram).  All arithmetic is float32, every product and sum rounded on its own
// (-ffp-contract=off), every slot's three sums sequential in increasing t from +0.0f.
//
// Selects.  The device pass walks wave-uniform time and therefore visits steps outside a lane's [onset, tEnd); it keeps ONE
// triple of running sums per lane, the current slot's, and leaves it unchanged by select at such a step (echogramStep).  That
// gives the definition's bits without the argument pv_lateral.h needs about adding +0.0f: the definition adds nothing at all to
// a slot for a step that is no member of it -- e[j] receives exactly the products of k in [j ns, (j + 1) ns) below tEnd, in
// increasing t, starting from +0.0f -- and the running triple receives exactly those, in that order, between the reset after
// slot j - 1 was written and the write of slot j.  No sum ever sees a value of another slot, selected or added.
#pragma once

#include <cmath>

#include "pv_libm.h"

namespace pva {

constexpr int kEchogramMaxSlots = 32;         // PVA_ECHOGRAM_MAX_SLOTS
constexpr int kEchogramMaxSlotSteps = 1 << 20;

PV_HD inline int echogramFloats(int nSlots) { return 1 + 3 * nSlots; }  // n, then e, ix, iy per slot

// steps per slot: the expression of lateralN5 (pv_lateral.h), so 0.005f gives n5.  Call only with echogramSlotOk(slotSeconds, fs)
PV_HD inline int echogramSlotSteps(float slotSeconds, int fs) { return (int)(slotSeconds * (float)fs); }

// slotSeconds finite and 1 <= ns <= 2^20 (checked on the float product: the conversion to int is then defined)
PV_HD inline bool echogramSlotOk(float slotSeconds, int fs) {
    const float x = slotSeconds * (float)fs;
    return x >= 1.0f && x < (float)(kEchogramMaxSlotSteps + 1);  // (false for NaN; an infinite slotSeconds gives inf or NaN)
}

PV_HD inline float echogramQuietNan() { return pvFloatBits(0x7fc00000u); }

struct EchogramSums {
    float e, ix, iy;
};

// one step of the current slot by selects: `in` = the step lies in [onset, tEnd)
PV_HD inline void echogramStep(EchogramSums& s, bool in, float p, float vx, float vy) {
    const float e = s.e + (p * p), ix = s.ix + (p * vx), iy = s.iy + (p * vy);
    s.e = in ? e : s.e;
    s.ix = in ? ix : s.ix;
    s.iy = in ? iy : s.iy;
}

// the definition applied to one impulse response p[T], vx[T], vy[T] with its onset (0 <= onset < T), ns >= 1 steps per slot and
// 1 <= nSlots <= kEchogramMaxSlots, as it is written down; out: echogramFloats(nSlots) floats
inline void echogramOfIr(const float* p, const float* vx, const float* vy, int T, int onset, int ns, int nSlots, float* out) {
    const long long w = (long long)ns * nSlots;
    const int tEnd = (long long)onset + w < (long long)T ? (int)(onset + w) : T;
    float* e = out + 1;
    for (int j = 0; j < 3 * nSlots; ++j) e[j] = 0.f;
    for (int t = onset; t < tEnd; ++t) {
        const int k = t - onset, j = k / ns;
        e[3 * j] = e[3 * j] + (p[t] * p[t]);
        e[3 * j + 1] = e[3 * j + 1] + (p[t] * vx[t]);
        e[3 * j + 2] = e[3 * j + 2] + (p[t] * vy[t]);
    }
    out[0] = (float)(tEnd - onset);
}

}  // namespace pva
