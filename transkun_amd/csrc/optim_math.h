// optim_math.h -- the per-element mathematics of the optimizer step (train.py:242-246: clip_grad_norm_ + torch_optimizer.AdaBelief with
// weight_decouple=True, rectify=True, amsgrad=False), shared by the HIP kernel (optim.hip) and the host kernel behind the CPU dispatch key
// (cpu_ops.cpp).  Both run it in fp32: every operation below is one correctly rounded IEEE operation (no fast-math, no fma
// contraction -- the build flags of both compilers forbid them), in one fixed order, so the two give the same bits.
//
// The scalar factors are computed on the host in float64 and rounded to fp32 ONCE each (semicrf_adabelief_group); t is the step
// counter (1 on the first step), bc1 = 1 - b1^t, bc2 = 1 - b2^t, rho_inf = 2/(1-b2) - 1, rho_t = rho_inf - 2 t b2^t / (1 - b2^t):
//   g  = g * coef                                     coef: the clip coefficient (1 when nothing clips); the gradient buffer is not written
//   p  = p * decay                                    decay = 1 - lr*wd  (decoupled, before the update; decay = 1 is exact)
//   m  = b1*m + omb1*g                                omb1 = 1 - b1
//   r  = g - m
//   s  = (b2*s + omb2*(r*r)) + eps                    omb2 = 1 - b2; eps goes INTO the stored state every step, as the package does
//   rectified (rho_t > 4):   p = p - step * (m / (sqrt(s)/sqrt_bc2 + eps))      step = rt*lr/bc1
//   otherwise:               p = p - step * m                                   step = lr
#pragma once
#include <math.h>
#include "../../include/semicrf_hip.h"

#if defined(__HIPCC__)
#define OPTIM_HD __host__ __device__ __forceinline__
#else
#define OPTIM_HD inline
#endif

namespace semicrf {
namespace optim {

constexpr int SQNORM_BLOCK = 1024;                // threads per workgroup of the norm's first stage
constexpr int SQNORM_PER_BLOCK = 32768;           // elements per workgroup below the cap
constexpr int SQNORM_MAX_PARTIALS = SEMICRF_SQNORM_MAX_PARTIALS;   // the cap (the second stage adds them one after the other): beyond
                                                  // 8 M elements the workgroups stride
constexpr int HISTORY_MAX = SEMICRF_HISTORY_MAX;               // the ring is sorted in LDS: 16384 fp32 = 64 KB

// the number of partial sums semicrf_grad_sqnorm writes: a function of numel only
OPTIM_HD int sqnorm_partials(long long numel)
{
    const long long n = (numel + SQNORM_PER_BLOCK - 1) / SQNORM_PER_BLOCK;
    return n < 1 ? 1 : (n > SQNORM_MAX_PARTIALS ? SQNORM_MAX_PARTIALS : (int)n);
}

OPTIM_HD void adabelief_update(float& p, float g, float& m, float& s, float coef, const semicrf_adabelief_group& k)
{
    g = g * coef;
    float pv = p * k.decay;
    const float mv = k.b1 * m + k.omb1 * g;
    const float r = g - mv;
    const float sv = (k.b2 * s + k.omb2 * (r * r)) + k.eps;
    if (k.rectified) {
        const float denom = sqrtf(sv) / k.sqrt_bc2 + k.eps;
        pv = pv - k.step * (mv / denom);
    } else {
        pv = pv - k.step * mv;
    }
    p = pv; m = mv; s = sv;
}

// clip_grad_norm_'s coefficient: min(1, clip / (norm + 1e-6)), NaN when either is NaN
OPTIM_HD float clip_coef(float clip, float norm)
{
    const float c = clip / (norm + 1e-6f);
    return c > 1.0f ? 1.0f : c;
}

// np.quantile's default (linear) interpolation between the order statistics a <= b at weight t in [0, 1], in double
OPTIM_HD double quantile_lerp(double a, double b, double t)
{
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}

}  // namespace optim
}  // namespace semicrf
