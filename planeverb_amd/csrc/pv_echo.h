// pv_echo.h -- echo criterion of Dietsch and Kraak (Acustica 60, 1986), speech and music variant, of one impulse response: the
// definition of include/planeverb_amd.h (PvAmdEchoCriterion), shared by the device pass (pv_echo.hip) and the host restatement
// (PvAmdHostEchoCriterion).  All arithmetic is float32, every product, sum and quotient rounded on its own (-ffp-contract=off),
// every sum sequential in increasing k from +0.0f; powf is glibc's (pv_libm.h).
//
// The lagged centre c(k - nD) is not remembered: a second pair of sums, fed with the weight of p(t - nD), makes exactly the
// additions the leading pair made nD steps earlier, so its quotient has the bits of c(k - nD).  echoStep is
// one step of one variant in that form, for device and host alike.
#pragma once

#include "pv_libm.h"

namespace pva {

constexpr int kEchoFloats = 10;  // speech, then music: ek, tk, ekLate, tkLate, ts
constexpr float kEchoSpeechExponent = 0.6666667f;  // (float)(2.0 / 3.0); PVA_ECHO_SPEECH_EXPONENT

PV_HD inline int echoSpeechLag(int fs) { return (int)(0.009f * (float)fs); }
PV_HD inline int echoMusicLag(int fs) { return (int)(0.014f * (float)fs); }
PV_HD inline int echoSpeechLimit(int fs) { return (int)(0.05f * (float)fs); }
PV_HD inline int echoMusicLimit(int fs) { return (int)(0.08f * (float)fs); }
// the sampling rates the criterion is defined for: a speech lag of at least one step
PV_HD inline bool echoFsOk(int fs) { return echoSpeechLag(fs) >= 1; }

PV_HD inline float echoAbs(float p) { return pvFloatBits(pvBitsF(p) & 0x7fffffffu); }  // fabsf

struct EchoVar {
    float A, B;    // the leading sums: A(k), B(k)
    float Al, Bl;  // the same sums nD steps behind: A(k - nD), B(k - nD)
    float ek, ekLate, c;
    int kk, kkLate;
};

PV_HD inline EchoVar echoVarInit() { return EchoVar{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, __builtin_nanf(""), 0, 0}; }

// Step k = t - onset of one variant.  on: the step exists (0 <= k < N; a device lane outside its range changes nothing, by
// select); w: the weight of p(t); wl: the weight of p(t - nD), read only when k >= nD.
PV_HD inline void echoStep(EchoVar& v, bool on, int k, float w, float wl, int nD, float nDf, int nL) {
    const float m = (float)k * w;
    const float a1 = v.A + w, b1 = v.B + m;
    v.A = on ? a1 : v.A;
    v.B = on ? b1 : v.B;
    const bool lag = on && k >= nD;
    const float ml = (float)(k - nD) * wl;
    const float al1 = v.Al + wl, bl1 = v.Bl + ml;
    v.Al = lag ? al1 : v.Al;
    v.Bl = lag ? bl1 : v.Bl;
    const float c = v.B / v.A;
    const float cl = v.Bl / v.Al;
    const float x = (c - (lag ? cl : 0.f)) / nDf;
    const bool up = on && x > v.ek;  // strict: the first maximum wins, a NaN never does
    v.ek = up ? x : v.ek;
    v.kk = up ? k : v.kk;
    const bool upLate = on && k >= nL && x > v.ekLate;
    v.ekLate = upLate ? x : v.ekLate;
    v.kkLate = upLate ? k : v.kkLate;
    v.c = on ? c : v.c;
}

PV_HD inline void echoRecord(const EchoVar& v, int fs, float out[5]) {
    out[0] = v.ek;
    out[1] = (float)v.kk / (float)fs;
    out[2] = v.ekLate;
    out[3] = (float)v.kkLate / (float)fs;
    out[4] = v.c / (float)fs;
}

// the definition applied to one impulse response p[T] with its onset (0 <= onset < T; echoFsOk(fs))
inline void echoCriterionOfIr(const float* p, int T, int fs, int onset, float out[kEchoFloats]) {
    const int nDs = echoSpeechLag(fs), nDm = echoMusicLag(fs), nLs = echoSpeechLimit(fs), nLm = echoMusicLimit(fs);
    EchoVar sp = echoVarInit(), mu = echoVarInit();
    for (int t = onset; t < T; ++t) {
        const int k = t - onset;
        const float a = echoAbs(p[t]);
        const float als = k >= nDs ? echoAbs(p[t - nDs]) : 0.f, alm = k >= nDm ? echoAbs(p[t - nDm]) : 0.f;
        echoStep(sp, true, k, pvPowfNonNeg(a, kEchoSpeechExponent), pvPowfNonNeg(als, kEchoSpeechExponent), nDs, (float)nDs, nLs);
        echoStep(mu, true, k, a, alm, nDm, (float)nDm, nLm);
    }
    echoRecord(sp, fs, out);
    echoRecord(mu, fs, out + 5);
}

}  // namespace pva
