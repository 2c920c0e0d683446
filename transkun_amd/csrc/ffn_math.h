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
//
// Training (semicrf_ffn_residual_train_fwd, semicrf_ffn_residual_bwd: ffn.hip's second mode and ffn_bwd.hip).  i is the token's index
// i0 n1 + i1 in the [n0, n1, D] view, M1[j] = keep(seed, 0, i, j) ? s1 : 0 with s1 = (float)(1 / (1 - p1)), M2[n] = keep(seed, 1, i, n)
// ? s2 : 0; a dropout with p = 0 neither masks nor scales (no multiplication at all).  keep: Philox-4x32-10 (attr_heads_math.h) with
// counter ((i >> 2) & 0xffffffff, column, stream, i >> 34) and the seed as key; element i takes word i & 3 and is kept iff the word
// >= floor(p 2^32).  Forward:
//   z[j]    = h[j]  (after + b1; saved)          a[j] = gelu(z[j]) * M1[j]    takes g's place in p_c
//   y[n]    = acc[n] + b2[n]  (saved)            out[n] = x[n] + (y[n] * M2[n]) * scale[n]
// Backward, g = dout (every product and sum one fp32 operation unless stated):
//   dy[n]   = (g[n] * scale[n]) * M2[n]                                        -> workspace [tokens][D]
//   da[j]   = sum_n dy[n] W2[n][j]: the contraction index n ascending in sub-chains of FFN_BWD_KSUB values, each an fmaf chain from +0
//             (on over its zero padding up to a multiple of FFN_BWD_KSTEP), the sub-chains' sums added in ascending order from +0
//   dz[j]   = (da[j] * M1[j]) * gelu_grad(z[j])                                -> workspace [tokens][H]
//   dxn[k]  = sum_j dz[j] W1[j][k], summed like da
//   t       = sum_k dxn[k] xn[k]: for c = k mod 32 and cw = (k / 32) mod 2 the fmaf chain over k ascending from +0 (ceil(D / 64)
//             terms: 0 * 0 past D), the 32 chains of a cw added as a butterfly (v[c] += v[c ^ 1], then ^ 2, 4, 8, 16), then cw 0 + cw 1
//   dx[k]   = g[k] + rs * (dxn[k] - xn[k] * (t / (float)D))
//   sums over tokens, per chunk of FFN_BWD_ROWS tokens (a plane), the planes added in ascending order starting from plane 0:
//   dW2[n][j] = sum_i dy[i][n] a[i][j], dW1[j][k] = sum_i dz[i][j] xn[i][k]: per plane, sub-chains of FFN_BWD_RSUB tokens (fmaf from +0,
//             on over zero padding up to a multiple of FFN_BWD_RSTEP), their sums added ascending from +0
//   db1[j] = sum_i dz[i][j], db2[n] = sum_i dy[i][n], dscale[n] = sum_i g[i][n] * (y[i][n] * M2[i][n]): per plane FFN_BWD_SUBSUMS sums
//             in double over the tokens i = q (mod FFN_BWD_SUBSUMS), added in ascending q, rounded to fp32 once
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

// ---- training ---------------------------------------------------------------------------------------------------------------------
constexpr int FFN_BWD_ROWS = 512;    // tokens per partial plane of the sums over tokens: SEMICRF_FFN_BWD_ROW_CHUNK
constexpr int FFN_BWD_RSUB = 128;    // tokens per sub-chain inside a plane
constexpr int FFN_BWD_RSTEP = 32;    // tokens staged per step of those kernels
constexpr int FFN_BWD_KSUB = 64;     // contraction values per sub-chain of da and dxn
constexpr int FFN_BWD_KSTEP = 16;    // contraction values staged per step of those kernels
constexpr int FFN_BWD_SUBSUMS = 8;   // a column sum's plane: 8 sums over the tokens i = q (mod 8), added in ascending q (double)

using attr_heads::DropoutParams;     // index 0: the hidden dropout (stream 0), index 1: the output dropout (stream 1)

// the four draws of tokens 4 q .. 4 q + 3 (q = i >> 2 < 2^35) at column j of `stream`
FFN_HD void dropout_draws(unsigned long long seed, uint32_t stream, unsigned long long q, uint32_t j, uint32_t out[4])
{
    attr_heads::philox4x32_10((uint32_t)q, j, stream, (uint32_t)(q >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), out);
}
FFN_HD bool keep(const DropoutParams& d, int stream, long long i, int j)
{
    if (!d.on[stream]) return true;
    uint32_t w[4];
    dropout_draws(d.seed, (uint32_t)stream, (unsigned long long)i >> 2, (uint32_t)j, w);
    return w[i & 3] >= d.thr[stream];
}
// v * M of `stream`, given the element's draw
FFN_HD float masked(const DropoutParams& d, int stream, uint32_t draw, float v)
{
    return d.on[stream] ? (draw >= d.thr[stream] ? v * d.scale[stream] : 0.0f) : v;
}
FFN_HD float dy_of(float g, float scale, const DropoutParams& d, uint32_t draw) { return masked(d, 1, draw, g * scale); }
FFN_HD float dx_of(float g, float rs, float dxn, float xn, float t, int D) { return g + rs * (dxn - xn * (t / (float)D)); }

}  // namespace ffn
}  // namespace semicrf
