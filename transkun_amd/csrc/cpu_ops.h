// cpu_ops.h -- host kernels behind the CPU dispatch key of torch.ops.semicrf.* (cpu_ops.cpp); argument meaning as the
// entry points of the same name in include/semicrf_hip.h, with host pointers and no stream / workspace.
#pragma once
#include <cstdint>
#include "../../include/semicrf_hip.h"

namespace semicrf_cpu {
void logz_fwd(const float* score, const float* noise, int T, int B, float* logZ, float* v /* [T][B], required */);
// alpha of the semi-CRF restricted to the frames start[c] .. T-1 (semicrf_alpha_from); a start out of range gives a NaN column
void alpha_from(const float* score, const float* noise, const int32_t* start, int T, int B, float* v /* [T][B] */, float* logZ);
void logz_bwd(const float* score, const float* noise, const float* v, const float* logZ, const float* gout, int T, int B,
              float* dScore /* or null: beta only */, float* dNoise /* or null */, float* q /* [T][B], required */);
void viterbi(const float* score, const float* noise, int T, int B, const int32_t* start, int forward, int32_t* pairs, int64_t cap,
             int32_t* offsets);
void sample(const float* score, const float* noise, const float* v, int T, int B, int64_t k0, int nSample, uint64_t key,
            const int32_t* end, int32_t* pairs, int64_t cap, int32_t* offsets);
void viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int32_t* start, int forward, int32_t* pairs,
                   int64_t cap, int32_t* offsets, float* scores /* [k][B] */, int32_t* npaths /* [B] */);
void posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B, float* node,
                float* begin, float* end, float* single, float* noiseP, float* entropy);
void interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int32_t* pairs,
                        const int32_t* offsets, float* out);
void marginal_decode(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                     int tau_stride, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets);
void interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int32_t* pairs,
                            const int32_t* offsets, int tol_begin, int tol_end, float* out);
void marginal_decode_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                         int tau_stride, int tol_begin, int tol_end, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets);
void mbr_select(const int32_t* pairs, const float* weight, const int32_t* offsets, int64_t K, int T, int B, const float* tau,
                int tau_stride, int32_t* pairs_out, float* probs_out, int64_t cap, int32_t* offsets_out, float* gain /* [B] */);
void compare_paths(const int32_t* est_pairs, const int32_t* est_offsets, const int32_t* ref_pairs, const int32_t* ref_offsets, int T,
                   int B, int tol_begin, int tol_end, int32_t* stats /* [B][7] */);
// state: (4 T B + 2 B) doubles, filled by expectation and read by covariance (v64, a, q64, binc [T][B] each, then E, logZ [B])
void expectation(const float* score, const float* noise, const float* weight /* or null: score */, const float* nweight /* or null: 0 */,
                 int T, int B, float* E, float* H, double* state);
void covariance(const float* score, const float* noise, const float* weight, const float* nweight, const float* gout, int T, int B,
                const double* state, float* C, float* Cn /* or null when T = 1 */);
void eval_path(const float* score, const float* noise, int T, int B, const int32_t* pairs, const int32_t* offsets, float* out);
void eval_path_bwd(const float* gout, int T, int B, const int32_t* pairs, const int32_t* offsets, float* dScore, float* dNoise);
// the attribute-head training loss (semicrf_attribute_loss_fwd / _bwd): the formulas of attr_loss_math.h per row in double, each
// row term rounded to fp32, then the pinned fp32 order -- (lpVel + lpOF) + lpPres, rows ascending per chain, base last
void attribute_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int32_t* velocity, const float* ofRefined,
                        const float* ofPresence, int64_t K, const int32_t* offsets, int C, const float* base /* or null */,
                        float* rowLogProb, float* out);
void attribute_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int32_t* velocity,
                        const float* ofRefined, const float* ofPresence, int64_t K, const int32_t* offsets, int C,
                        float* dLogitsVelocity, float* dOfLogits);
// the attribute-head readout (semicrf_attribute_decode): the formulas of attr_decode_math.h per row in double, each result rounded
// to fp32; velocityClass or velocityMean by criterion (the other may be null)
void attribute_decode(const float* logitsVelocity, const float* ofLogits, int64_t K, int criterion, int64_t* velocityClass,
                      float* velocityMean, float* ofValue, unsigned char* ofPresence);
// the two attribute heads (semicrf_attribute_heads): the device kernel's order of operations per output element, in fp32
// (attr_heads_math.h); the weights packed as the C ABI takes them; symIdx / scatterIdx may be null
void attribute_heads(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets, int nSym,
                     const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                     float* logitsVelocity, float* ofLogits, int64_t* symIdx, int64_t* scatterIdx);
// the heads in training (semicrf_attribute_heads_train_fwd / _bwd / _dropout_mask): the same order of operations, in fp32
void attribute_heads_train_fwd(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets,
                               int nSym, const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                               uint64_t seed, double pv, double po, float* logitsVelocity, float* ofLogits, float* z, int64_t* symIdx,
                               int64_t* scatterIdx);
void attribute_heads_bwd(const float* dLv, const float* dOf, const float* z, const float* ctx, int C, int T, int D, int64_t ldc,
                         const int32_t* pairs, int64_t K, const int32_t* offsets, const float* W1, const float* W2, int Hv, int Ho, int Nv,
                         int No, uint64_t seed, double pv, double po, float* dctx, float* dW1, float* db1, float* dW2, float* db2);
void attribute_heads_dropout_mask(uint64_t seed, int64_t K, int Hv, int Ho, double pv, double po, unsigned char* mask);
// the optimizer step (semicrf_grad_sqnorm / semicrf_clip_from_history / semicrf_adabelief_step): the arithmetic of optim_math.h, the
// update in fp32 in the device kernel's order of operations (the same bits); partials: as many as the device writes for this numel
void grad_sqnorm(const float* flat, int64_t numel, double* partials);
void clip_from_history(const double* partials /* or null */, int64_t numel, const float* norm_in /* or null */, double q, float* ring,
                       int capacity, int32_t* state, int append, float* stats);
void adabelief_step(float* p, const float* g, float* m, float* s, int64_t numel, const float* coef /* or null: 1 */,
                    const semicrf_adabelief_groups& groups);
// the backbone's axial attention (semicrf_axial_attention): the device kernel's order of operations per output element, in fp32
// (attention_math.h); strides: the twelve element strides q, k, v, out x (s0, s1, l); the caller has checked the supported set
void axial_attention(const float* q, const float* k, const float* v, float* out, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d,
                     const int64_t* strides);
// the same attention of bfloat16 tensors (semicrf_axial_attention_bf16): the chain of attention_bf16_math.h in plain C++ -- fp32
// accumulation ascending, the conversions to bf16 written out (round to nearest even); strides as above, in bf16 elements
void axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int64_t n0, int64_t n1, int Lq, int Lk, int H,
                          int d, const int64_t* strides);
// its backward (semicrf_axial_attention_bwd): the same chain in the same orders; any of dq, dk, dv may be null; strides: the twenty-four
// element strides q, k, v, out, dout, dq, dk, dv x (s0, s1, l)
void axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk, float* dv,
                         int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, const int64_t* strides);
// the backward of the bf16 attention (semicrf_axial_attention_bf16_bwd): the backward chain of attention_bf16_math.h, fp32 accumulation
// ascending; any of dq, dk, dv may be null; strides: the twenty-one element strides q, k, v, dout, dq, dk, dv x (s0, s1, l)
void axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk, uint16_t* dv,
                              int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, const int64_t* strides);
// the backbone's feed-forward ResBlock (semicrf_ffn_residual): the device kernel's order of operations per output element, in fp32
// (ffn_math.h); x and out [n0, n1, D] with their two element row strides; the caller has checked the supported set
void ffn_residual(const float* x, float* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                  const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps);
// the block in training (semicrf_ffn_residual_train_fwd / _bwd / semicrf_ffn_dropout_mask): the device's order of operations (ffn_math.h)
void ffn_residual_train_fwd(const float* x, float* out, float* z, float* y, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                            int64_t os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale,
                            float eps, uint64_t seed, double p1, double p2);
void ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1,
                      int64_t xs0, int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const float* W1, const float* W2, const float* scale,
                      float eps, uint64_t seed, double p1, double p2, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale);
void ffn_dropout_mask(uint64_t seed, int64_t rows, int D, int H, double p1, double p2, unsigned char* mask_hidden, unsigned char* mask_out);
// the bf16 feed-forward ResBlock (semicrf_ffn_residual_bf16 on bf16 tensors, semicrf_ffn_residual_bf16_mixed on fp32 tensors): the
// chain of ffn_bf16_math.h per output element, both sums in fp32 ascending; the caller has checked the supported set
void ffn_residual_bf16(const uint16_t* x, uint16_t* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                       const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale, float eps);
void ffn_residual_bf16_mixed(const float* x, float* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                             const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps);
// the bf16 block in training (semicrf_ffn_residual_bf16_train_fwd / _bwd and their _mixed forms): the chain of ffn_bf16_train_math.h one
// product at a time in ascending order; `saved` as that header lays it out (semicrf_ffn_residual_bf16_train_saved_bytes bytes)
void ffn_residual_bf16_train_fwd(const uint16_t* x, uint16_t* out, void* saved, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                                 int64_t os1, int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2,
                                 const uint16_t* scale, float eps, uint64_t seed, double p1, double p2);
void ffn_residual_bf16_mixed_train_fwd(const float* x, float* out, void* saved, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                                       int64_t os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                                       const float* scale, float eps, uint64_t seed, double p1, double p2);
void ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1, int64_t xs0,
                           int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const uint16_t* W1, const uint16_t* W2, const uint16_t* scale,
                           float eps, uint64_t seed, double p1, double p2, uint16_t* dx, uint16_t* dW1, uint16_t* db1, uint16_t* dW2, uint16_t* db2,
                           uint16_t* dscale);
void ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1, int64_t xs0,
                                 int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const float* W1, const float* W2, const float* scale, float eps,
                                 uint64_t seed, double p1, double p2, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale);
// the audio front end (semicrf_log_mel): the device kernel's order of operations per output element, in fp32 (logmel_math.h); frames
// by its three element strides, out contiguous [N][to_mono ? 1 : C][nFrame][nMel][nWin]; the caller has checked the supported set
void log_mel(const float* frames, int64_t sn, int64_t sc, int64_t sf, int N, int C, int nFrame, int W, const float* windows, int nWin,
             const float* tw, const int32_t* fb_start, const int32_t* fb_len, const int32_t* fb_off, const float* fb_val, int nMel, int total,
             const float* shift, const float* denom, int log_flag, float eps, int to_mono, float* out);
}  // namespace semicrf_cpu
