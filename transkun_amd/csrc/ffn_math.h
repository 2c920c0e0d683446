// ffn_math.h -- what the HIP kernel of the backbone's feed-forward ResBlock (ffn.hip) and its host mirror (cpu_ops.cpp) share: the
// supported set, the tile constants and the order of operations of every output element.
//
// Per token (a row x of D values; W1 [H][D], b1 [H], W2 [D][H], b2 [D], scale [D] as nn.Linear and ResBlock store them):
//   s_q     = fmaf-chain over k = q, q + 4, q + 8, .. ascending from +0 of x[k] * x[k]              q = 0 .. 3
//   ss      = (s_0 + s_1) + (s_2 + s_3)
//   rs      = 1 / sqrt(ss / (float)D + eps)             one division, one addition, one square root, one division, all IEEE fp32
//   xn[k]   = x[k] * rs                                  rounded to fp32 once
//   h[j]    = fmaf-chain over k = 0 .. D-1 ascending from +0 of xn[k] * W1[j][k], then + b1[j]      (one fp32 addition)
//   g[j]    = gelu(h[j])                                 attr_heads_math.h: the exact erf form, erfc below 0
//   p_c[n]  = fmaf-chain over the hidden columns j of chunk c ascending from +0 of g[j] * W2[n][j]; a last chunk of fewer than
//             FFN_CHUNK columns goes on over its padding with 0 * 0 (which leaves every value but -0 as it is, and turns -0 into +0)
//   acc[n]  = ((0 + p_0[n]) + p_1[n]) + ..               the chunks' sums, ascending, one fp32 addition each
//   out[n]  = x[n] + (acc[n] + b2[n]) * scale[n]         one addition, one multiplication, one addition
// The hidden columns are walked in chunks of FFN_CHUNK, ascending.  A chunk's sum starts from +0 and is added to the running total at
// the chunk's end: the rounding error of a chain grows with its length, and at 640 to 1024 hidden columns one chain through all of
// them is several times less accurate than eager PyTorch's blocked sums (both stay in registers for the whole walk).
// A workgroup owns FFN_ROWS token rows; rows past the last token are zeros formed in registers and never stored.  Neither constant
// depends on anything (so not on D either): a token's output depends on its own row and the weights alone, whatever the other tokens,
// their number and the strides are.
#pragma once
#include <math.h>
#include <stdint.h>

#include "attr_heads_math.h"

#if defined(__HIPCC__)
#define FFN_HD __host__ __device__ __forceinline__
#else
#define FFN_HD inline
#endif

namespace semicrf {
namespace ffn {

constexpr int FFN_ROWS = 64;         // token rows per workgroup: SEMICRF_FFN_ROW_TILE
constexpr int FFN_CHUNK = 64;        // hidden columns per step of the walk: SEMICRF_FFN_HIDDEN_CHUNK
constexpr int FFN_MIN_D = 8;
constexpr int FFN_MAX_D = 256;       // SEMICRF_FFN_MAX_D: the [64, D] accumulator is 64 registers per lane there
constexpr int FFN_MIN_H = 8;
constexpr int FFN_MAX_H = 4096;      // SEMICRF_FFN_MAX_HIDDEN

FFN_HD bool supported(int D, int H)
{
    return D >= FFN_MIN_D && D <= FFN_MAX_D && D % 8 == 0 && H >= FFN_MIN_H && H <= FFN_MAX_H && H % 8 == 0;
}

FFN_HD int chunks_of(int H) { return (H + FFN_CHUNK - 1) / FFN_CHUNK; }

// where contraction index k sits inside a row of an operand tile in LDS: every four values are kept as [k0, k2, k1, k3], so that one
// 8-byte read gives half wave 0 (k0, k2) and half wave 1 (k1, k3) -- the k pairs (k0, k1) and (k2, k3) of two 32x32x2 products
FFN_HD int lds_pos(int k) { return (k & ~3) | ((k & 1) << 1) | ((k >> 1) & 1); }

FFN_HD float sumsq_combine(float s0, float s1, float s2, float s3) { return (s0 + s1) + (s2 + s3); }
FFN_HD float rs_of(float ss, int D, float eps) { return 1.0f / sqrtf(ss / (float)D + eps); }
FFN_HD float epilogue(float x, float acc, float b2, float scale) { return x + (acc + b2) * scale; }

}  // namespace ffn
}  // namespace semicrf
