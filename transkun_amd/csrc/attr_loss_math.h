// attr_loss_math.h -- the per-row mathematics of the attribute-head training loss (TransKun.log_prob, ModelTransformer.py:284-328),
// shared by the HIP kernels (attr_loss.hip, T = float) and the host kernels behind the CPU dispatch key (cpu_ops.cpp, T = double).
//
// Per target interval, with the heads' raw outputs:
//   lpVel  = logitsVelocity[v] - logsumexp(logitsVelocity)                                   (:291-295; the callers reduce)
//   lpOF   = sum_j  x_j l_j - softplus(l_j) + logC(l_j),   x_j = r_j * 0.99 + 0.5            (:304-313, ContinuousBernoulli)
//   lpPres = sum_j  p_j l'_j - softplus(l'_j)                                                (:315-317, Bernoulli)
// logC is torch's _cont_bern_log_norm as the reference runs it in fp32, i.e. WITH its probability clamp at eps32 = 2^-23:
//   logC(l) = log(l / tanh(l / 2))   for |l| < l* = log((1 - eps32) / eps32),   logC(l*) beyond (derivative 0),   log 2 at 0.
// torch evaluates it in probability space, log|log1p(-p) - log p| - log|1 - 2p|, whose fp32 cancellation costs up to 1e-2 near the
// clamp and 3e-3 (gradient) at the edge of its Taylor window.  Here it is evaluated from the logit, a = |l|, e = exp(-a):
//   a >= 1:  log(a / (1 - e)) + log1p(e)              -- a quotient of two well-conditioned numbers, then a log away from 0
//   a <  1:  log 2 + a^2/12 - 7 a^4/1440 + ...        -- the Maclaurin series (coefficients 2 (2^(2k-1) - 1) |B_2k| / ((2k)! 2k))
//   d/dl:    1/l - 1/sinh l = 1/l - 2e / ((1 - e)(1 + e))   for a >= 1,   l/6 - 7 l^3/360 + ...   below (the closed form cancels)
// The switch point 1 is measured: with nine terms the series' truncation at a = 1 is 2e-9 (value) / 2e-9 (derivative), and the closed
// forms' fp32 rounding at a >= 1 stays below 3 ulp of the result.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ATTR_LOSS_HD __host__ __device__ __forceinline__
#else
#define ATTR_LOSS_HD inline
#endif

namespace semicrf {
namespace attr_loss {

constexpr int NVEL = 128;                                   // velocity classes (ModelTransformer.py:109-115)
constexpr double LSTAR = 15.942385033669446;                // log((1 - 2^-23) / 2^-23): where sigmoid(l) meets torch's clamp
constexpr double LOGC_STAR = 2.7689815262885857;            // log(LSTAR / (1 - 2^-22)) = logC(LSTAR)
constexpr double SERIES_BELOW = 1.0;
constexpr double LOG2 = 0.69314718055994531;

ATTR_LOSS_HD float exp_(float x) { return expf(x); }
ATTR_LOSS_HD double exp_(double x) { return exp(x); }
ATTR_LOSS_HD float log_(float x) { return logf(x); }
ATTR_LOSS_HD double log_(double x) { return log(x); }
ATTR_LOSS_HD float log1p_(float x) { return log1pf(x); }
ATTR_LOSS_HD double log1p_(double x) { return log1p(x); }
ATTR_LOSS_HD float abs_(float x) { return fabsf(x); }
ATTR_LOSS_HD double abs_(double x) { return fabs(x); }

// logC(l): the ContinuousBernoulli log-normaliser, clamped as above.  NaN in, NaN out.
template <class T>
ATTR_LOSS_HD T log_norm(T l)
{
    const T a = abs_(l);
    if (a != a) return a;
    if (!((double)a < LSTAR)) return (T)LOGC_STAR;      // compared in double: LSTAR is no fp32 number
    if (a < (T)SERIES_BELOW) {
        const T s = a * a;
        return (T)LOG2 + s * ((T)8.33333333333333287e-02 + s * ((T)-4.86111111111111119e-03 + s * ((T)3.41710758377425047e-04
               + s * ((T)-2.62483465608465622e-05 + s * ((T)2.13360456416011954e-06 + s * ((T)-1.80278953564888321e-07
               + s * ((T)1.56594795318340298e-08 + s * ((T)-1.38837067837002588e-09 + s * (T)1.25042637753154829e-10))))))));
    }
    const T e = exp_(-a);
    return log_(a / ((T)1 - e)) + log1p_(e);
}

// d logC / d l (0 beyond the clamp)
template <class T>
ATTR_LOSS_HD T log_norm_grad(T l)
{
    const T a = abs_(l);
    if (a != a) return a;
    if (!((double)a < LSTAR)) return (T)0;
    if (a < (T)SERIES_BELOW) {
        const T s = a * a;
        return l * ((T)1.66666666666666657e-01 + s * ((T)-1.94444444444444448e-02 + s * ((T)2.05026455026455006e-03
               + s * ((T)-2.09986772486772498e-04 + s * ((T)2.13360456416011963e-05 + s * ((T)-2.16334744277865964e-06
               + s * ((T)2.19232713445676397e-07 + s * ((T)-2.22139308539204141e-08 + s * (T)2.25076747955678672e-09))))))));
    }
    const T e = exp_(-a);
    const T d = (T)1 / a - ((T)2 * e) / (((T)1 - e) * ((T)1 + e));
    return l < (T)0 ? -d : d;
}

// x l - softplus(l), the Bernoulli / ContinuousBernoulli cross-entropy term for a target x in [0, 1]: the form without the
// cancellation of l against softplus(l) at large |l|
template <class T>
ATTR_LOSS_HD T bern_term(T x, T l)
{
    if (l >= (T)0) return -(((T)1 - x) * l) - log1p_(exp_(-l));
    return x * l - log1p_(exp_(l));
}

template <class T>
ATTR_LOSS_HD T sigmoid(T l)
{
    if (l >= (T)0) return (T)1 / ((T)1 + exp_(-l));
    const T e = exp_(l);
    return e / ((T)1 + e);
}

// The onset/offset part of a row: of = the head's raw output [value0, value1, presence0, presence1] (.chunk(2, -1), :306),
// r = the target refinement in [-0.5, 0.5] (shifted to [0.005, 0.995] here, in fp32 as the reference does at :304), p = presence.
template <class T>
ATTR_LOSS_HD void of_terms(const float of[4], const float r[2], const float p[2], T& lpOF, T& lpPres)
{
    const T x0 = (T)(r[0] * 0.99f + 0.5f), x1 = (T)(r[1] * 0.99f + 0.5f);
    const T t0 = bern_term<T>(x0, (T)of[0]) + log_norm<T>((T)of[0]);
    const T t1 = bern_term<T>(x1, (T)of[1]) + log_norm<T>((T)of[1]);
    lpOF = t0 + t1;
    lpPres = bern_term<T>((T)p[0], (T)of[2]) + bern_term<T>((T)p[1], (T)of[3]);
}

// its derivative with respect to the four raw outputs (to be scaled by the chain's upstream gradient)
template <class T>
ATTR_LOSS_HD void of_grads(const float of[4], const float r[2], const float p[2], T d[4])
{
    const T x0 = (T)(r[0] * 0.99f + 0.5f), x1 = (T)(r[1] * 0.99f + 0.5f);
    d[0] = (x0 - sigmoid<T>((T)of[0])) + log_norm_grad<T>((T)of[0]);
    d[1] = (x1 - sigmoid<T>((T)of[1])) + log_norm_grad<T>((T)of[1]);
    d[2] = (T)p[0] - sigmoid<T>((T)of[2]);
    d[3] = (T)p[1] - sigmoid<T>((T)of[3]);
}

}  // namespace attr_loss
}  // namespace semicrf
