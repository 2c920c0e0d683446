// attr_heads_math.h -- what the HIP kernel of the attribute heads (attr_heads.hip) and its host mirror (cpu_ops.cpp) share: the
// tile constants that fix the order of operations of every output element, and the activation.
//
// Per interval i, x_i = [a | b | a * b] (3 D values, a = ctx[c, begin], b = ctx[c, end]; the product is rounded to fp32 once):
//   h[j]       = fmaf-chain over k = 0 .. 3D-1 ascending from +0 of x[k] * W1[k][j], then + b1[j]          (one fp32 addition)
//   g[j]       = gelu(h[j])                                                                                (below)
//   part[s][n] = fmaf-chain over the hidden columns j of slice s ascending from +0 of g[j] * W2[j][n]
//   out[n]     = ((part[0][n] + part[1][n]) + ...) + b2[n]                                                 (slices ascending, bias last)
// A head's hidden columns are cut into slices of HEADS_SLICE; a slice never holds columns of both heads.  Both chains are padded
// with exact zeros (0 * 0 added: no change to a finite value), so a result depends on its own row and the weights alone.
//
// gelu is the exact erf form, nn.GELU()'s default: 0.5 h (1 + erf(h / sqrt 2)).  For h < 0 that sum cancels (1 + erf -> 0) and
// loses the tail's relative accuracy; there 1 + erf(z) = erfc(-z) is used, which does not.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ATTR_HEADS_HD __host__ __device__ __forceinline__
#else
#define ATTR_HEADS_HD inline
#endif

namespace semicrf {
namespace attr_heads {

constexpr int HEADS_ROWS = 64;       // rows (intervals) per workgroup: SEMICRF_HEADS_ROW_TILE
constexpr int HEADS_SLICE = 64;      // hidden columns per workgroup
constexpr int HEADS_KCHUNK = 32;     // contraction values of layer 1 staged per step

ATTR_HEADS_HD int slices_of(int H) { return (H + HEADS_SLICE - 1) / HEADS_SLICE; }

ATTR_HEADS_HD float erf_(float x) { return erff(x); }
ATTR_HEADS_HD double erf_(double x) { return erf(x); }
ATTR_HEADS_HD float erfc_(float x) { return erfcf(x); }
ATTR_HEADS_HD double erfc_(double x) { return erfc(x); }

template <class T>
ATTR_HEADS_HD T gelu(T h)
{
    const T z = h * (T)0.70710678118654752440;
    const T t = h < (T)0 ? erfc_(-z) : (T)1 + erf_(z);       // NaN takes the second branch and stays NaN
    return ((T)0.5 * h) * t;
}

}  // namespace attr_heads
}  // namespace semicrf
