// launchers.h -- every function of namespace semicrf that one .hip file defines and another calls: the kernels' host launchers,
// their workspace sizes and support predicates.  Declarations only.  The defining file and every caller include this header,
// so the compiler sees each definition next to its declaration and a call can only name what is declared here.
#pragma once
#include "common.h"

namespace semicrf {

// alpha_from.hip
void launch_alpha_from(const float* score, const float* noise, const int* start, int T, int B, float* v, float* logZ, hipStream_t stream);

// attention.hip
void launch_axial_attention(const float* q, const float* k, const float* v, float* out, long long n0, long long n1, int Lq, int Lk, int H, int d,
                            const long long* strides, hipStream_t stream);

// attention_bf16.hip
void launch_axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, long long n0, long long n1, int Lq, int Lk, int H,
                                 int d, const long long* strides, hipStream_t stream);

// attention_bf16_bwd.hip
void launch_axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk,
                                     uint16_t* dv, long long n0, long long n1, int Lq, int Lk, int H, int d, const long long* strides,
                                     hipStream_t stream);

// attention_bwd.hip
void launch_axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk, float* dv,
                                long long n0, long long n1, int Lq, int Lk, int H, int d, const long long* strides, hipStream_t stream);

// attr_decode.hip
void launch_attr_decode(const float* logitsVelocity, const float* ofLogits, int K, int criterion, long long* velocityClass,
                        float* velocityMean, float* ofValue, unsigned char* ofPresence, hipStream_t stream);

// attr_gather.hip
void launch_interval_features(const float* ctx, int C, int T, int D, long long ldc, const int* pairs, int K,
                              const int* offsets, int nSym, float* out, long long* symIdx, long long* scatterIdx,
                              hipStream_t stream);
void launch_interval_features_bwd(const float* gout, const float* ctx, int C, int T, int D, long long ldc, const int* pairs,
                                  int K, const int* offsets, float* dctx, long long lddc, hipStream_t stream);

// attr_heads.hip
size_t attr_heads_workspace_bytes(long long K, int Hv, int Ho, int Nv, int No);
void launch_attr_heads(const float* ctx, int C, int T, int D, long long ldc, const int* pairs, int K, const int* offsets, int nSym,
                       const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                       float* logitsVelocity, float* ofLogits, long long* symIdx, long long* scatterIdx, float* ws, hipStream_t stream,
                       float* zsave = nullptr, unsigned long long seed = 0, double pv = 0.0, double po = 0.0);

// attr_heads_bwd.hip
size_t attr_heads_bwd_workspace_bytes(long long K, int D, int Hv, int Ho, int Nv, int No);
hipError_t launch_attr_heads_bwd(const float* dLv, const float* dOf, const float* z, const float* ctx, int C, int T, int D, long long ldc,
                                 const int* pairs, int K, const int* offsets, const float* W1, const float* W2, int Hv, int Ho, int Nv, int No,
                                 unsigned long long seed, double pv, double po, float* dctx, float* dW1, float* db1, float* dW2, float* db2,
                                 float* ws, hipStream_t stream);
void launch_attr_heads_mask(unsigned long long seed, long long K, int Hv, int Ho, double pv, double po, unsigned char* mask, hipStream_t stream);

// attr_loss.hip
void launch_attr_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int* velocity, const float* ofRefined,
                          const float* ofPresence, int K, const int* offsets, int C, const float* base, float* rowLogProb, float* out,
                          hipStream_t stream);
void launch_attr_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int* velocity,
                          const float* ofRefined, const float* ofPresence, int K, const int* offsets, int C, float* dLogitsVelocity,
                          float* dOfLogits, hipStream_t stream);

// decode.hip
void launch_backtrack(const int* code, int T, int B, const int* start, int forward, int* region, int* counts,
                      int* pairs, long long cap, int* offsets, hipStream_t stream, const unsigned* err, int nerr, int err_stride);
void launch_pack(const int* region, const int* counts, int T, int B, int forward, int* pairs, long long cap, int* offsets,
                 hipStream_t stream, const unsigned* err, int nerr, int err_stride);

// evalpath.hip
void launch_eval_path(const float* score, const float* noise, int T, int B, int K, const int* pairs,
                      const int* offsets, float* out, hipStream_t stream, const float* sub = nullptr);
void launch_eval_path_bwd(const float* gout, int T, int B, int K, const int* pairs, const int* offsets,
                          float* dScore, float* dNoise, hipStream_t stream, int gstride = 1, float gscale = 1.0f, int noise_term_done = 0);

// expectation.hip
size_t expectation_workspace_bytes(int T, int B);
void launch_expectation(const float* score, const float* noise, const float* weight, const float* nweight, const float* v, const float* q,
                        int T, int B, float* E, float* H, void* ws, hipStream_t stream);
void launch_covariance(const float* score, const float* noise, const float* weight, const float* nweight, const float* gout, int T, int B,
                       float* C, float* Cn, const void* ws, hipStream_t stream);

// ffn.hip
void launch_ffn_residual(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                         int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                         hipStream_t stream);

void launch_ffn_residual_train(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                               long long os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                               const float* scale, float eps, unsigned long long seed, double p1, double p2, float* z, float* y,
                               hipStream_t stream);

// ffn_bwd.hip
size_t ffn_bwd_workspace_bytes(long long ntok, int D, int H);
void launch_ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, long long n0, long long n1, long long gs0,
                             long long gs1, long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const float* W1,
                             const float* W2, const float* scale, float eps, unsigned long long seed, double p1, double p2, float* dx,
                             float* dW1, float* db1, float* dW2, float* db2, float* dscale, float* ws, hipStream_t stream);
void launch_ffn_mask(unsigned long long seed, long long rows, int D, int H, double p1, double p2, unsigned char* mask_hidden,
                     unsigned char* mask_out, hipStream_t stream);

// ffn_bf16.hip
void launch_ffn_residual_bf16(const uint16_t* x, uint16_t* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                              int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale,
                              float eps, hipStream_t stream);
void launch_ffn_residual_bf16_mixed(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                                    int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                                    hipStream_t stream);
// the training mode: `saved` is laid out as ffn_bf16_train_math.h says (zs, then ys)
void launch_ffn_residual_bf16_train(const uint16_t* x, uint16_t* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                                    long long os1, int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2,
                                    const uint16_t* scale, float eps, unsigned long long seed, double p1, double p2, void* saved, hipStream_t stream);
void launch_ffn_residual_bf16_mixed_train(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                                          long long os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                                          const float* scale, float eps, unsigned long long seed, double p1, double p2, void* saved,
                                          hipStream_t stream);

// ffn_bf16_bwd.hip
size_t ffn_bf16_bwd_workspace_bytes(long long ntok, int D, int H);
void launch_ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, long long n0, long long n1, long long gs0, long long gs1,
                                  long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const uint16_t* W1, const uint16_t* W2,
                                  const uint16_t* scale, float eps, unsigned long long seed, double p1, double p2, uint16_t* dx, uint16_t* dW1,
                                  uint16_t* db1, uint16_t* dW2, uint16_t* db2, uint16_t* dscale, void* ws, hipStream_t stream);
void launch_ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, long long n0, long long n1, long long gs0, long long gs1,
                                        long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const float* W1, const float* W2,
                                        const float* scale, float eps, unsigned long long seed, double p1, double p2, float* dx, float* dW1,
                                        float* db1, float* dW2, float* db2, float* dscale, void* ws, hipStream_t stream);

// logmel.hip
void launch_log_mel(const float* frames, long long sn, long long sc, long long sf, int N, int C, int nFrame, int W, const float* windows, int nWin,
                    const float* tw, const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_val, int nMel, int total,
                    const float* shift, const float* denom, int log_flag, float eps, int to_mono, float* out, hipStream_t stream);

// marginal_decode.hip
size_t marginal_decode_workspace_bytes(int T, int B);
void launch_marginal_decode(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                            int tau_stride, int* pairs, float* probs, long long cap, int* offsets, void* ws, hipStream_t stream);
void marginal_decode_scans(int* cnt, int* coltot, int* tot, const float* v, int T, int B, int* offsets, hipStream_t stream);

// marginal_tol.hip
size_t marginal_decode_tol_workspace_bytes(int T, int B);
void launch_interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int* pairs,
                                   int K, const int* offsets, int db, int de, float* out, hipStream_t stream);
void launch_marginal_decode_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                                int tau_stride, int db, int de, int* pairs, float* probs, long long cap, int* offsets, void* ws,
                                hipStream_t stream);

// marginals.hip
void launch_marginals(const float* score, const float* noise, const float* v, const float* q,
                      const float* logZ, const float* gout, int T, int B, float* dScore, float* dNoise,
                      hipStream_t stream, int gstride = 1, float gscale = 1.0f);

// mbr_decode.hip
size_t mbr_select_workspace_bytes(int T, int B);
void launch_mbr_select(const int* pairs, const float* weight, const int* offsets, long long K, int T, int B, const float* tau,
                       int tau_stride, int* pairs_out, float* probs_out, long long cap, int* offsets_out, float* gain, void* ws,
                       hipStream_t stream);

// merge_weights.hip
void launch_merge_weights_fwd(const float* W, const float* bias, int D, int size, int rows, float* Wm, float* bm, float* WmT, hipStream_t stream);
void launch_merge_weights_bwd(const float* W, const float* bias, const float* dWm, const float* dbm, int D, int size, float* dW, float* dbias,
                              float* ws, hipStream_t stream);
size_t merge_weights_bwd_workspace_bytes(int size);
void launch_stage_linear(const float* W, const float* bias, int D, int size, int rows_pad, float* BT, float* Wqd, float* w2, float* b2,
                         hipStream_t stream);

// nbest.hip
size_t nbest_workspace_bytes(int T, int nB);
void launch_viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int* start, int forward, int* pairs,
                          long long cap, int* offsets, float* scores, int* npaths, void* ws, hipStream_t stream);

// optim.hip
void launch_grad_sqnorm(const float* flat, long long numel, double* partials, hipStream_t stream);
void launch_clip_from_history(const double* partials, long long numel, const float* norm_in, double q, float* ring, int capacity,
                              int* state, int append, float* stats, hipStream_t stream);
void launch_adabelief_step(float* p, const float* g, float* m, float* s, long long numel, const float* coef,
                           const semicrf_adabelief_groups& groups, hipStream_t stream);

// pathstats.hip
void launch_compare_paths(const int* est_pairs, const int* est_offsets, const int* ref_pairs, const int* ref_offsets, int T, int B,
                          int tb, int te, int* stats, hipStream_t stream);

// persist.hip
const unsigned* persist_error_words(void* pws, int* n, int* stride);
void launch_zero_upper(float* X, int T, int B, hipStream_t stream);
size_t persist_workspace_bytes(int T, int B);
bool persist_supported(int T, int B);
int launch_persist_sweep(int mode, int dir, const float* score, const float* noise, int T, int B, float* u_out,
                         float* last_out, int* code, void* ws, hipStream_t stream, int lease, unsigned lease_tag);
int persist_set_host_abort_word(unsigned* devptr);
int persist_wg_ticket(int nSpine, int grid, int b);
int read_and_clear_device_status();
int launch_persist_logz_bwd(const float* score, const float* noise, const float* v, const float* logZ,
                            const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out, void* ws,
                            hipStream_t stream, int lease, unsigned lease_tag, int gstride = 1, float gscale = 1.0f, int keep_upper = 0,
                            float noise_add = 0.0f, const int* ptab = nullptr, int* path_folded = nullptr);
int launch_persist_logprob_fwd(const float* score, const float* noise, int T, int B, float* u_out, float* logZ, const int* pairs,
                               int K, const int* offsets, float* logProb, void* ws, hipStream_t stream, int lease, unsigned lease_tag,
                               int* ptab = nullptr);
int persist_path_fold_possible(int T, int B);

// posterior.hip
size_t posterior_workspace_bytes(int T, int B);
void launch_posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                       float* node, float* begin, float* end, float* single, float* noiseP, float* entropy, void* ws,
                       hipStream_t stream);
void launch_interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int* pairs,
                               int K, const int* offsets, float* out, hipStream_t stream);

// proj_gemm.hip
int launch_proj_nn(const float* A, long long lda, long long M, int K, const float* B, long long ldb, int N, float* out, long long ldout,
                   const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, hipStream_t stream);
size_t proj_tn_workspace_bytes(long long M, int R, int N);
int launch_proj_tn(const float* A, long long lda, long long M, int R, int extra_col0, int total_rows, const float* X, long long ldx, int N,
                   float* dW, long long lddw, float* db, void* ws, size_t ws_bytes, hipStream_t stream);
bool proj_gemm_supported(long long M, int K, int N, const void* A, long long lda, const void* B, long long ldb, const void* out,
                         long long ldout);

// proj_gemm3.hip
size_t proj_nn3_workspace_bytes(int K, int N);
int launch_proj_nn3(const float* A, long long lda, long long M, int K, const float* B, long long ldb, int N, float* out, long long ldout,
                    const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, void* ws, size_t ws_bytes,
                    hipStream_t stream);
int launch_proj_tn3_core(const float* A, long long lda, long long M, int R, const float* X, long long ldx, int N, float* part, int Mp,
                         float* pbias, int bias_pitch, int S, int kslice, hipStream_t stream);

// rowseq.hip
void launch_rowseq_sweep(int mode, int dir, const float* score, const float* noise, int T, int B, float* u,
                         int* code, float* out_last, hipStream_t stream);

// sample.hip
size_t sample_workspace_bytes(int T, int nB);
void launch_sample(const float* score, const float* noise, const float* v, int T, int B, long long k0, int nSample,
                   unsigned long long key, const int* end, int* pairs, long long cap, int* offsets, void* ws, hipStream_t stream);

// scorer.hip
void launch_interval_score_naive(const float* q, const float* k, const float* diag, int C, int T, int D,
                                 long long ldq, long long ldk, long long ldd, float qscale, int mode, int full,
                                 float* S, hipStream_t stream);

// scorer_bwd.hip
bool interval_score_bwd_supported(int C, int T, int D);
void launch_interval_score_bwd_fused(const float* S, const float* alpha, const float* beta, const float* logZ,
                                     const float* gout, const float* q, const float* k, int C, int T, int D,
                                     long long ldq, long long ldk, float qscale, int mode, float* dq, float* dk,
                                     float* ddiag, long long lddq, long long lddk, long long lddd, hipStream_t stream);
void launch_interval_score_bwd(const float* dS, const float* q, const float* k, int C, int T, int D, long long ldq,
                               long long ldk, float qscale, int mode, float* dq, float* dk, float* ddiag,
                               long long lddq, long long lddk, long long lddd, hipStream_t stream);
void launch_interval_score_path_bwd(const float* gout, const int* pairs, int K, const int* offsets, const float* q,
                                    const float* k, int C, int T, int D, long long ldq, long long ldk, float qscale, int mode,
                                    float* dq, float* dk, float* ddiag, long long lddq, long long lddk, long long lddd,
                                    hipStream_t stream, int group, int pitch, float* drowc = nullptr, long long lddrc = 1);
void launch_interval_score_bwd_rowsum(const float* dS, const float* const* fused, float* drowc, long long ldrc, int C, int T,
                                      float qscale, int mode, int group, int pitch, hipStream_t stream);
void launch_interval_score_bwd_diag(const float* dS, const float* const* fused, float* ddiag, int C, int T, long long lddd,
                                    int group, int pitch, hipStream_t stream);

// scorer_bwd_gemm.hip
enum { SCORE_BWD_DIRECT = 0, SCORE_BWD_PACKED = 1, SCORE_BWD_PACKED3 = 2 };       // the direct kernels (scorer_bwd.hip) | packed, exact | packed, three-limb
struct ScoreBwdPlan { int path; size_t ws_bytes; };                                // ws_bytes: what the packed path needs (0: it never applies to the shape)
ScoreBwdPlan plan_score_bwd(int C, int T, int D, bool rows_ok, bool ws_ok, size_t ws_bytes, bool want_dq, bool want_drowc,
                            long long lddq, long long lddk, int prec);
size_t interval_score_bwd_ws_bytes(int C, int T, int D);
bool launch_interval_score_bwd_packed(const float* dS, const float* q, const float* k, int C, int T, int D, long long ldq,
                                      long long ldk, float qscale, int mode, float* dq, float* dk, long long lddq,
                                      long long lddk, void* ws, size_t ws_bytes, hipStream_t stream,
                                      const float* const* fused, int group, int pitch, float* drowc, long long lddrc, int prec);

// scorer_mfma.hip
// the forward kernels, in semicrf_debug_score_variant's numbering (0, 2, 32, 64, 128) extended by the plain kernel, the three-limb
// kernel and "refused" (semicrf_debug_score_route returns these)
enum { SCORE_REFUSED = -1, SCORE_REGLOAD = 0, SCORE_NAIVE = 1, SCORE_TILED = 2, SCORE_TILE3 = 3, SCORE_STREAM = 32, SCORE_TILE64 = 64,
       SCORE_TILE128 = 128 };
struct ScoreRoute { int kernel; const char* why; };       // why: the error text of a refusal
ScoreRoute plan_score_route(int C, int T, int D, long long ldq, long long ldk, bool bases_aligned, int prec, int group, int pitch,
                            bool rowc, int forced, int impl);
int launch_interval_score_fwd(int kernel, const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq,
                              long long ldk, long long ldd, float qscale, int mode, int full, float* S, hipStream_t stream, int group,
                              int pitch, const float* rowc, long long ldrc);
void set_score_variant(int v);
int score_variant();

// scorer_tiled.hip
void launch_interval_score_tiled(const float* q, const float* k, const float* diag, const float* rowc, int C, int T, int D,
                                 long long ldq, long long ldk, long long ldd, long long ldrc, float qscale, int mode, int full,
                                 float* S, hipStream_t stream, int group, int pitch);

// segment.hip
void launch_onset_filter(const int* pairs, const int* offsets, int B, int bound, int* pairs_out, long long cap, int* offsets_out,
                         int* counts, hipStream_t stream);
void launch_segment_events(const int* pairs, const int* offsets, int B, int nSym, const float* ofValue, const unsigned char* ofPresence,
                           int lastFrameIdx, double frameDur, const double* beginTime, int stepFrames, double* times, unsigned char* flags,
                           int* lastP, int* nextStart, hipStream_t stream);

}  // namespace semicrf
