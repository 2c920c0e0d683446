// attention_bf16_math.h -- what the HIP kernel of the bf16 axial attention (attention_bf16.hip) and its host mirror (cpu_ops.cpp) share:
// the chain of operations, the bf16 conversions and the order of the keys inside a matrix instruction's k-step.
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

}  // namespace attention
}  // namespace semicrf
