// ffn_bf16_train_math.h -- what the training route of the bf16 feed-forward ResBlock shares between its kernels (ffn_bf16.hip in
// training mode, ffn_bf16_bwd.hip) and its host mirrors (cpu_ops.cpp): the chain of operations of every element, the layout of the
// saved buffer and the order of every sum.  It builds on ffn_bf16_math.h (the eval chain, the two forms), ffn_math.h (the mask, rs,
// dx_of, the plane size) and attr_heads_math.h (gelu, gelu_grad, Philox).
//
// T is the element type of the form: bf16 in form A (every tensor bf16), fp32 in form B (every tensor fp32, bf16 operands inside).
// round_T is bf16_rne in form A and the identity in form B.  M1[i][j] = keep(seed, 0, i, j) ? (float)(1 / (1 - p_hidden)) : 0 and
// M2[i][n] = keep(seed, 1, i, n) ? (float)(1 / (1 - p_out)) : 0 are the factors of ffn_math.h's mask function (stream 0: hidden,
// stream 1: the output; a dropout with p = 0 neither masks nor multiplies); token i is the index i0 n1 + i1 in the [n0, n1, D] view.
// The same seed gives the same masks on the fp32 and on the bf16 routes: semicrf_ffn_dropout_mask describes both.
//
// Forward, training mode.  Everything up to h[j] is exactly ffn_bf16_math.h (xf, rs, xh, Wh1, Wh2, h):
//   zs[j]  = bf16_rne(h[j])                                  saved
//   a[j]   = bf16_rne(gelu(h[j]) * M1[i][j])                 fp32 product, one rounding; the layer-2 operand
//   acc[n] = sum_j a[j] * Wh2[n][j]                          one running fp32 accumulator, as the eval op
//   y[n]   = acc[n] + (float)b2[n]        ys[n] = round_T(y[n])   saved
//   out[n] = round_T(xf[n] + (y[n] * M2[i][n]) * (float)scale[n])
// With p_hidden = p_out = 0, out has the bits of semicrf_ffn_residual_bf16 / _mixed.
//
// Backward, g = (float)dout:
//   dyf[n] = (g[n] * (float)scale[n]) * M2[i][n]             dyh = bf16_rne(dyf)
//   dscale[n] = sum_tok g[n] * ((float)ys[n] * M2[i][n])     db2[n] = sum_tok dyf[n]
//   da[j]  = sum_n dyh[n] * Wh2[n][j]                        exact products, fp32 accumulation from +0, n ascending
//   zf     = (float)zs[j]
//   dzf[j] = (da[j] * M1[i][j]) * gelu_grad(zf)              dzh = bf16_rne(dzf)
//   ah[j]  = bf16_rne(gelu(zf) * M1[i][j])                   RECOMPUTED from zs, not the forward's a (which saw the unrounded h): it
//                                                            saves the forward a second [tokens, hidden] store; the two agree wherever
//                                                            bf16_rne(h) = h
//   db1[j] = sum_tok (float)dzh[j]
//   dW2[n][j] = sum_tok dyh[n] * ah[j]                       dW1[j][k] = sum_tok dzh[j] * xh[k]        xh as the forward forms it
//   dxn[k] = sum_j dzh[j] * Wh1[j][k]                        one running fp32 accumulator over all of hidden, j ascending
//   xn[k]  = xf[k] * rs                                      fp32, unrounded
//   t      = sum_k dxn[k] * xn[k]: for cw = (k / 32) mod 2 and hh = (k / 4) mod 2 the fmaf chain over that class's k ascending from +0,
//            then (cw, hh = 0) + (cw, hh = 1), then cw 0 + cw 1
//   dx[k]  = round_T(ffn_math.h's dx_of(g[k], rs, dxn[k], xn[k], t, D))
// Sums over tokens run per chunk of FFN_BWD_ROWS (512) tokens, each from +0 with the tokens ascending on one fp32 accumulator (the
// device adds 16 exact products per matrix instruction); a chunk's sum is a plane of the workspace and the planes are added in
// ascending order starting from plane 0.  The column sums (db1, db2, dscale) are FFN_BWD_SUBSUMS sub-sums in double per plane over
// the tokens i = q (mod 8), added in ascending q and rounded to fp32 once, as ffn_bwd.hip forms them.  Every parameter gradient is
// rounded to T once, at the very end.  No atomics, no memset the result depends on: every gradient is bit-identical from run to run,
// and a token's out and dx depend on its own row, its index i, the seed and the weights only.
//
// The saved buffer (written by the forward, read by the backward; its layout depends on (tokens, D, hidden) only):
//   zs  bf16 [tokens][hidden]  at byte 0
//   ys  T    [tokens][D]       at byte train_saved_ys_offset(tokens, hidden); sized for fp32 in both forms
#pragma once
#include "ffn_bf16_math.h"

namespace semicrf {
namespace ffn {

constexpr int FFN16_LDZ = FFN16_CHUNK + FFN16_PAD;    // bf16 per row of the zs tile in LDS (training mode)

FFN_HD size_t train_up256(size_t n) { return (n + 255) / 256 * 256; }
FFN_HD size_t train_saved_ys_offset(long long ntok, int H) { return train_up256((size_t)ntok * (size_t)H * 2); }
FFN_HD size_t train_saved_bytes(long long ntok, int D, int H) { return train_saved_ys_offset(ntok, H) + train_up256((size_t)ntok * (size_t)D * 4); }

// LDS of the forward in training mode: the eval op's tiles and the chunk's zs tile [ROWS][CHUNK + PAD] in bf16
FFN_HD size_t lds_bytes_bf16_train(int D) { return lds_bytes_bf16(D) + 2 * (size_t)FFN16_ROWS * FFN16_LDZ; }

// a value as the form's element holds it (round_T), still as fp32
FFN_HD float round_to(uint16_t, float v) { return bf16_to_float(bf16_rne(v)); }
FFN_HD float round_to(float, float v) { return v; }

}  // namespace ffn
}  // namespace semicrf
