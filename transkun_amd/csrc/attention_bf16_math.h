// attention_bf16_math.h -- what the HIP kernels of the bf16 axial attention (attention_bf16.hip, attention_bf16_bwd.hip) and their host
// mirrors (cpu_ops.cpp) share: the chains of operations, the bf16 conversions and the order of the keys inside a matrix instruction's
// k-step.  The forward first, the backward at the end.
//
// Per sequence s, head h and query i (q, k, v, out token-major bf16, head h the slice [h d, (h + 1) d)):
//   s[j]   = (sum over c < d of q[i][c] * k[j][c]) * scale     every product exact in fp32, fp32 accumulation; scale = (float)(1 / sqrt(d))
//   m      = max over the keys j < Lk of s[j]                  keys from Lk to the tile edge are -inf before the maximum
//   p[j]   = expf(s[j] - m)
//   ph[j]  = bf16_rne(p[j])                                    what the second product consumes
//   sum    = S0 + S1,  S_b = the sum of (float)ph[j] over the keys with sum_half(j) == b, ascending in j from +0
//   o[c]   = sum over j < Lk of ph[j] * v[j][c]                fp32 accumulation
//   out[c] = bf16_rne(o[c] / sum)
// The sum is the sum of the ROUNDED weights: the weights of o[c] sum to `sum`, so a V that is constant over the keys comes back exactly.
// On the device the two accumulations are v_mfma_f32_32x32x16_bf16's (16 products per instruction, summed inside the instruction); the
// mirror accumulates in fp32 ascending.  The two agree wherever every partial sum is exact, and to rounding elsewhere.
#pragma once
#include "attention_math.h"

namespace semicrf {
namespace attention {

// round to nearest even, NaN stays NaN (quiet, sign kept), +-inf stays
ATTENTION_HD uint16_t bf16_rne(float x)
{
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

ATTENTION_HD float bf16_to_float(uint16_t b)
{
    const uint32_t u = (uint32_t)b << 16;
    float x;
    __builtin_memcpy(&x, &u, 4);
    return x;
}

// The key that element j (0 .. 7) of half wave hh holds in k-step ks (0, 1) of a 32-key block when a 32 x 32 accumulator block is
// handed to the next product as its operand: accumulator register 8 ks + j, whose row is (r & 3) + 8 (r >> 2) + 4 hh.
ATTENTION_HD int kstep_key(int ks, int j, int hh) { return 16 * ks + 8 * (j >> 2) + 4 * hh + (j & 3); }

constexpr int ATT16_KPAD = 8;        // bf16 elements behind a K row in LDS: rows stay 16-byte aligned and leave the power of two
constexpr int ATT16_VPAD = 4;        // bf16 elements behind a row of V^T in LDS: rows stay 8-byte aligned

ATTENTION_HD int dim_steps(int d) { return (d + 15) / 16; }          // k-steps of the first product: the head dimension padded to 16
ATTENTION_HD int col_blocks(int d) { return d <= 32 ? 1 : 2; }       // 32-column blocks of the output

// LDS of one workgroup: K [32 nkt][16 ks + KPAD] and V^T [32 db][32 nkt + VPAD], bf16
ATTENTION_HD size_t lds_bytes_bf16(int Lk, int d)
{
    const int nkt = key_tiles(Lk);
    return 2 * ((size_t)nkt * ATT_TILE * (16 * dim_steps(d) + ATT16_KPAD) + (size_t)32 * col_blocks(d) * (nkt * ATT_TILE + ATT16_VPAD));
}

// ---- the backward (attention_bf16_bwd.hip, semicrf_cpu::axial_attention_bf16_bwd) -----------------------------------------------------
// s, m, p, ph and sum are the forward's, recomputed by its chain (nothing is saved; the products commute, so the pass that holds a key
// per lane forms the scores of the pass that holds a query per lane).  Then, per sequence and head, dout the bf16 cotangent:
//   P[i][j]  = (float)ph[i][j] / sum[i]                            one fp32 division
//   dP[i][j] = sum over c < d of dout[i][c] * v[j][c]              exact products, fp32 accumulation
//   D[i]     = D0 + D1,  D_b = the sum of P[i][j] * dP[i][j] over the keys with sum_half(j) == b, ascending in j from +0: the order
//              of `sum`.  The softmax form, not dout . out: `out` is not an input, and at Lk = 1 dS is an exact zero
//   dS[i][j] = P[i][j] * (dP[i][j] - D[i])                         fp32
//   dSh = bf16_rne(dS), Ph = bf16_rne(P)                           what the three gradient products consume
//   dq[i][c] = bf16_rne(scale * sum over j of dSh[i][j] k[j][c])   fp32 accumulation, one multiplication by scale, one rounding
//   dk[j][c] = bf16_rne(scale * sum over i of dSh[i][j] q[i][c])
//   dv[j][c] = bf16_rne(        sum over i of Ph[i][j] dout[i][c])
// A key from Lk to the tile edge has P = dS = 0 exactly; a padded query has dout = 0, so D = dS = 0 and it adds exact zeros.
// On the device the five products are v_mfma_f32_32x32x16_bf16's; the mirror accumulates in fp32 ascending.

// LDS of one workgroup of the backward, nt = the tiles of the longer of the two sequences: two token-major images [32 nt][16 ks +
// KPAD] and two transposed ones [32 db][32 nt + VPAD] in bf16 (pass A: K, V, K^T; pass B: Q, dout, Q^T, dout^T), and m, sum, D of
// every query row as fp32
ATTENTION_HD size_t lds_bytes_bf16_bwd(int Lq, int Lk, int d)
{
    const int nt = key_tiles(Lq > Lk ? Lq : Lk);
    return 2 * (2 * (size_t)nt * ATT_TILE * (16 * dim_steps(d) + ATT16_KPAD) + 2 * (size_t)32 * col_blocks(d) * (nt * ATT_TILE + ATT16_VPAD)) +
           3 * (size_t)nt * ATT_TILE * sizeof(float);
}

}  // namespace attention
}  // namespace semicrf
