// attention_math.h -- what the HIP kernel of the backbone's axial attention (attention.hip) and its host mirror (cpu_ops.cpp) share:
// the supported set, the tile constants that fix the order of operations of every output element, and the scalar pieces.
//
// Per sequence s, head h and query i (q, k, v token-major: a token's H d values contiguous, head h the slice [h d, (h + 1) d)):
//   dot[j]  = fmaf-chain over c = 0 .. d-1 ascending from +0 of k[j][c] * q[i][c]
//   sc[j]   = dot[j] * scale                    scale = (float)(1 / sqrt(d)), one fp32 multiplication
//   m       = max over the keys j < Lk of sc[j] (keys past Lk never take part)
//   p[j]    = exp(sc[j] - m)
//   sum     = S0 + S1,  S_b = the sum of p[j] over the keys with sum_half(j) == b, ascending in j from +0
//   acc[c]  = fmaf-chain over j = 0 .. Lk-1 ascending from +0 of p[j] * v[j][c]
//   out[c]  = acc[c] / sum
// On the device the keys are padded to a multiple of ATT_TILE and the head dimension to 32 or 64 with exact zeros (0 * x added to a
// chain changes nothing for finite x; padded K / V rows are zeros formed in registers, never loaded), so every output depends on its
// own sequence alone.  sum_half is the half wave that holds score row j of a 32 x 32 accumulator block (its rows 4 .. 7 of every 8).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ATTENTION_HD __host__ __device__ __forceinline__
#else
#define ATTENTION_HD inline
#endif

namespace semicrf {
namespace attention {

constexpr int ATT_TILE = 32;         // queries per wave pass, keys per score block
constexpr int ATT_MAX_L = 256;       // SEMICRF_ATTENTION_MAX_L: the longest sequence (8 score blocks of a query tile stay in registers)
constexpr int ATT_MIN_D = 8;
constexpr int ATT_MAX_D = 64;        // SEMICRF_ATTENTION_MAX_D
constexpr int ATT_LDP = 40;          // floats per key row of a wave's probability tile (32 used): the two half waves write disjoint banks

ATTENTION_HD bool supported(int Lq, int Lk, int H, int d)
{
    return Lq >= 1 && Lq <= ATT_MAX_L && Lk >= 1 && Lk <= ATT_MAX_L && H >= 1 && d >= ATT_MIN_D && d <= ATT_MAX_D && d % 8 == 0;
}

ATTENTION_HD float scale_of(int d) { return (float)(1.0 / sqrt((double)d)); }
ATTENTION_HD int sum_half(int key) { return (key >> 2) & 1; }
ATTENTION_HD int key_tiles(int Lk) { return (Lk + ATT_TILE - 1) / ATT_TILE; }

// ---- the backward (attention_bwd.hip, semicrf_cpu::axial_attention_bwd) ----------------------------------------------------------------
// sc, m, p and sum are the forward's, recomputed by its chain (the product k[j][c] * q[i][c] commutes, so the pass that holds a key per
// lane forms the same bits as the pass that holds a query per lane).  Then, per sequence and head:
//   D[i]     = fmaf-chain over c = 0 .. d-1 ascending from +0 of dout[i][c] * out[i][c]          (out as the forward wrote it)
//   dP[i][j] = fmaf-chain over c = 0 .. d-1 ascending from +0 of v[j][c] * dout[i][c]
//   P[i][j]  = p[i][j] / sum[i]                                   one division, not a multiplication by a reciprocal
//   dS[i][j] = P[i][j] * (dP[i][j] - D[i])                        one subtraction, one multiplication
//   dq[i][c] = scale * fmaf-chain from +0 over t = 0 .. of dS[i][j] * k[j][c],    j = bwd_order(t), the j >= Lk left out
//   dk[j][c] = scale * fmaf-chain from +0 over t = 0 .. of dS[i][j] * q[i][c],    i = bwd_order(t), the i >= Lq left out
//   dv[j][c] =         fmaf-chain from +0 over t = 0 .. of P[i][j]  * dout[i][c], i = bwd_order(t), the i >= Lq left out
// bwd_order: blocks of ATT_TILE ascending; inside a block the accumulator-row order of a 32 x 32 matrix-pipe result, whose register r
// holds row (r & 3) + 8 (r >> 2) in lanes 0-31 and that row + 4 in lanes 32-63 -- the two k indices of one 32x32x2 product, so a score
// block's registers feed the next product as they are: 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, ..  It depends on nothing but t.
// On the device the left-out entries take part with exact zeros (a padded key has P = dS = 0, a padded query dout = 0 and D = 0).
ATTENTION_HD int bwd_order(int t)
{
    const int r = (t & (ATT_TILE - 1)) >> 1;
    return (t & ~(ATT_TILE - 1)) + (r & 3) + 8 * (r >> 2) + 4 * (t & 1);
}

}  // namespace attention
}  // namespace semicrf
