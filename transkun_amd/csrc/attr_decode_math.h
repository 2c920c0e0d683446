// attr_decode_math.h -- the per-row mathematics of the attribute-head readout of transcription (TransKun.transcribeFrames,
// ModelTransformer.py:590-651), shared by the HIP kernel (attr_decode.hip, T = float) and the host kernel behind the CPU dispatch
// key (cpu_ops.cpp, T = double).
//
// Refined onset / offset, from the value logit l (:640-643):
//   ofValue = clamp((m(l) - 0.5) / 0.99, -0.5, 0.5),   m = the ContinuousBernoulli mean as the reference runs it in fp32, i.e. WITH
//   the probability clamp at eps32 = 2^-23 (the convention of attr_loss_math.h's logC):   m(l) - 0.5 = sign(l) h(min(|l|, l*)),
//   h(a) = 0.5 coth(a / 2) - 1 / a,   l* = log((1 - eps32) / eps32).
// torch evaluates m in probability space, p / (2p - 1) + 1 / (log1p(-p) - log p): two terms of size 1 / |l| whose difference loses
// 3.4e-3 in fp32 at the edge of its Taylor window (|l| ~ 0.004).  Here, a = min(|l|, l*), e = exp(-a):
//   a >= 1.5:  0.5 (1 + e) / (1 - e) - 1 / a          -- both terms are below 1.1: their roundings stay absolute
//   a <  1.5:  a/12 - a^3/720 + a^5/30240 - ...         -- the Maclaurin series, coefficients B_2k / (2k)!, seven terms
// The switch point and the number of terms are measured ("Attribute-head readout"): in fp32 against 40-digit arithmetic
// on 20001 points per interval the series errs by at most 1.3e-8 below 1.5 (its truncation there: 1.4e-10), the closed form by at
// most 1.3e-7 above (used further down it would lose 2.4e-7 on [1, 1.5], 5.6e-7 on [0.5, 1] and 2.2e-6 on [0.25, 0.5]).
// Presence (:645): l' > 0, so NaN gives 0.
//
// Velocity (:595-632), from the probabilities p[w] of the row's 128 logits: the window sums of "match" and the decisions are the
// callers' (a wave on the device, a loop on the host); the constants they share are here.
#pragma once
#include "attr_loss_math.h"

namespace semicrf {
namespace attr_decode {

using attr_loss::NVEL;
using attr_loss::LSTAR;

constexpr int CRIT_HAMMING = 0, CRIT_MSE = 1, CRIT_MATCH = 2, CRIT_MAE = 3;     // SEMICRF_VEL_* (include/semicrf_hip.h)
constexpr int MATCH_RADIUS = 12;                            // |w - v| < 0.1 * 128 (ModelTransformer.py:610-611)
constexpr double OF_SERIES_BELOW = 1.5;
constexpr double H_STAR = 0.43727424739728643;              // h(LSTAR): the mean's distance from 0.5 at torch's probability clamp

// h(a) for 0 <= a < LSTAR
template <class T>
ATTR_LOSS_HD T mean_shift(T a)
{
    if (a < (T)OF_SERIES_BELOW) {
        const T s = a * a;
        return a * ((T)8.33333333333333287e-02 + s * ((T)-1.38888888888888894e-03 + s * ((T)3.30687830687830710e-05
               + s * ((T)-8.26719576719576754e-07 + s * ((T)2.08767569878681002e-08 + s * ((T)-5.28419013868749322e-10
               + s * (T)1.33825365306846789e-11))))));
    }
    const T e = attr_loss::exp_(-a);
    return (T)0.5 * ((T)1 + e) / ((T)1 - e) - (T)1 / a;
}

// ofValue of a value logit.  NaN in, NaN out (as torch.clamp); beyond l* the constant h(l*) / 0.99 = 0.4416912.
template <class T>
ATTR_LOSS_HD T of_value(T l)
{
    const T a = attr_loss::abs_(l);
    if (a != a) return a;
    const T h = (double)a < LSTAR ? mean_shift<T>(a) : (T)H_STAR;      // compared in double: LSTAR is no fp32 number
    const T v = (l < (T)0 ? -h : h) / (T)0.99;
    return v < (T)-0.5 ? (T)-0.5 : (v > (T)0.5 ? (T)0.5 : v);
}

ATTR_LOSS_HD unsigned char of_presence(float l) { return l > 0.0f ? 1 : 0; }

}  // namespace attr_decode
}  // namespace semicrf
