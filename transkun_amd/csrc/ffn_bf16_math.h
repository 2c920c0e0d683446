// ffn_bf16_math.h -- what the HIP kernel of the bf16 feed-forward ResBlock (ffn_bf16.hip) and its host mirrors (cpu_ops.cpp) share:
// the tile constants and the order of operations of every output element.  The supported set is ffn_math.h's.
//
// Two forms, one chain.  Form A (semicrf_ffn_residual_bf16): x, out, W1, b1, W2, b2 and scale are bf16 in memory, T = bf16.  Form B
// (semicrf_ffn_residual_bf16_mixed): all of them are fp32 in memory, as an fp32 model under autocast holds them, T = fp32; W1 and W2
// are rounded to bf16 (RNE) on their way into the operand tiles, every call, and b1, b2 and scale are used AS FP32.  That is where
// form B departs from autocast's nn.Linear, which rounds the biases to bf16 as well (and the Linear's output, and the gelu's).
//
// Per token (a row x of D values; W1 [H][D], b1 [H], W2 [D][H], b2 [D], scale [D] as nn.Linear and ResBlock store them):
//   xf[k]   = (float)x[k]                                exact
//   ss, rs  = ffn_math.h's: four strided fmaf chains over xf, (s_0 + s_1) + (s_2 + s_3), rs = 1 / sqrt(ss / (float)D + eps)
//   xh[k]   = bf16_rne(xf[k] * rs)                       one fp32 multiplication, one rounding
//   Wh1     = bf16_rne(W1), Wh2 = bf16_rne(W2)           the identity in form A
//   h[j]    = (sum over k < D of xh[k] * Wh1[j][k]) + (float)b1[j]       exact products, fp32 accumulation from +0, one fp32 addition
//   gh[j]   = bf16_rne(gelu(h[j]))                       attr_heads_math.h: the exact erf form, erfc below 0, in fp32
//   acc[n]  = sum over j < H of gh[j] * Wh2[n][j]        exact products, ONE running fp32 accumulator from +0 over all of hidden
//   out[n]  = round_T(xf[n] + (acc[n] + (float)b2[n]) * (float)scale[n])   one addition, one multiplication, one addition in fp32, ONE
//             rounding to T (none in form B)
// acc is one running accumulator, not the fp32 op's per-chunk sums: with bf16 operands each term already carries a relative error of
// 2^-9, which the length of the fp32 chain does not add to in any way that shows (640 to 1024 terms: a few 2^-24 more), while a
// second set of [rows, D] sums costs the kernel 48 registers per lane.  On the device both sums are v_mfma_f32_32x32x16_bf16's: 16
// products per instruction (hh = 0: k = 16 s .. + 7, hh = 1: k = 16 s + 8 .. + 15), summed inside the instruction and added to the
// running block, k-steps ascending; hidden is walked in chunks of FFN16_CHUNK columns, ascending, whose padding past hidden (and past
// D, in layer 1) adds 0 * 0.  The mirror accumulates in fp32 ascending.  The two agree wherever every partial sum is exact, and to
// rounding elsewhere; erff differs as well.
// A workgroup owns FFN16_ROWS token rows; rows past the last token are zeros formed in registers and never stored.  Neither constant
// depends on anything: a token's output depends on its own row and the weights alone, whatever the other tokens, their number, the
// strides and the alignment are.
#pragma once
#include "ffn_math.h"
#include "attention_bf16_math.h"

namespace semicrf {
namespace ffn {

constexpr int FFN16_ROWS = 64;       // token rows per workgroup: SEMICRF_FFN_BF16_ROW_TILE
constexpr int FFN16_CHUNK = 64;      // hidden columns per step of the walk: SEMICRF_FFN_BF16_HIDDEN_CHUNK
constexpr int FFN16_PAD = 8;         // bf16 elements behind a row of an operand tile in LDS: rows stay 16-byte aligned

using attention::bf16_rne;
using attention::bf16_to_float;

// an element of x or of a parameter as fp32 (exact), and the one rounding of the result
FFN_HD float to_f32(uint16_t v) { return bf16_to_float(v); }
FFN_HD float to_f32(float v) { return v; }
FFN_HD void store_as(uint16_t* p, float v) { *p = bf16_rne(v); }
FFN_HD void store_as(float* p, float v) { *p = v; }
// a weight as the bf16 operand of a product
FFN_HD uint16_t operand_of(uint16_t v) { return v; }
FFN_HD uint16_t operand_of(float v) { return bf16_rne(v); }

// LDS of one workgroup: the W1 tile [CHUNK][D + PAD], the W2 tile [D][CHUNK + PAD] and the gelu tile [ROWS][CHUNK + PAD] in bf16,
// and rs of every row in fp32
FFN_HD size_t lds_bytes_bf16(int D)
{
    return 2 * ((size_t)FFN16_CHUNK * (D + FFN16_PAD) + (size_t)D * (FFN16_CHUNK + FFN16_PAD) + (size_t)FFN16_ROWS * (FFN16_CHUNK + FFN16_PAD)) +
           FFN16_ROWS * sizeof(float);
}

}  // namespace ffn
}  // namespace semicrf
