/*
 * semicrf_hip.h -- C ABI of the MI355X (gfx950) Neural Semi-CRF interval layer.
 *
 * This is the drop-in boundary: plain pointers, sizes and a HIP stream handle; no torch
 * types.  The reference (Yujia-Yan/Transkun) has no FFI of its own -- its boundary is the
 * pure-Python class transkun/CRF/NeuralSemiCRFInterval.py:553-588 -- so each entry point
 * below cites the reference *function* it replaces; transkun_amd/CRF (ctypes) is the
 * host-side mirror of that class, and INTEGRATION.md shows the binding a Transkun
 * maintainer would add.
 *
 * Conventions
 *   - All pointers are DEVICE pointers (HBM) unless named h_*.  fp32 everywhere.
 *   - score  [T][T][B]  C-contiguous, indexed [end][begin][chain]; only end >= begin is read.
 *   - noise  [T-1][B]   score of "no event between frames t and t+1".
 *   - stream is a hipStream_t passed as void*; every call only ENQUEUES work on it
 *     (no host synchronisation), so calls compose with torch's current stream.
 *   - ws / ws_bytes: caller-owned scratch of at least semicrf_workspace_bytes(op,T,B) bytes,
 *     256-byte aligned (SEMICRF_WS_ALIGN); contents are undefined afterwards.
 *   - Return value: SEMICRF_OK or an error code; semicrf_last_error() gives the message of the
 *     last failing call on this thread.  Nothing is written on SEMICRF_EINVAL.
 *
 * Memory contract of the semi-CRF entry points (semicrf_*; tests/test_memory_contract.py pins every sentence)
 *   - ws: every entry point that takes one refuses a non-NULL ws whose address is not a multiple of SEMICRF_WS_ALIGN with
 *     SEMICRF_EINVAL, together with the other argument checks and ahead of any HIP call -- the entry points that ignore their ws
 *     (semicrf_alpha_from, semicrf_eval_path) included; where an entry point compares ws_bytes before it launches, a ws that is
 *     also too short stays SEMICRF_EWORKSPACE.  The library hands out its sub-buffers at 256-byte offsets from the base, and
 *     64-bit device-scope atomics sit on them.  Exactly semicrf_workspace_bytes(op,T,B) bytes are enough: nothing past ws + ws_bytes
 *     is read or written.  The results do not depend on what an unleased ws held before the call.
 *   - Operands and outputs (score, noise, v, q, logZ, gout, weights, every float / int32 output, start / end / offsets): ANY 4-byte
 *     aligned address.  The kernels' 16-byte accesses to four neighbouring chains are typed for 4-byte alignment (an odd NBatch
 *     puts every row at another phase anyway) and every atomic on them is a 4-byte one; the fixed summation orders name no
 *     alignment: results are bit-identical whatever the bases are modulo 16.  The exceptions are stated where they apply: `pairs`
 *     INPUTS of semicrf_mbr_select and semicrf_compare_paths are 8-byte aligned (one 8-byte load per pair; enforced).
 *   - Nothing outside the elements a call is documented to write is written, and nothing outside the elements it is documented to
 *     read reaches a result.  What a call leaves UNTOUCHED (it keeps the bits it had):
 *       an optional output passed as NULL / "not wanted" (v of semicrf_logz_fwd / _logprob_fwd, q_out of semicrf_logz_bwd);
 *       pairs rows (and probs entries) from min(total, cap) up to cap, total = the last offset, of every packed list;
 *       the cells begin > end of dScore under SEMICRF_GRAD_UPPER_IS_ZERO, where the persistent sweep runs (T >= 2, NBatch >= 2,
 *       implementation 0) -- the flag is a permission: the row-sequential kernels write the +0.0f the caller promised;
 *       semicrf_eval_path_bwd: every cell of dScore that is not a path cell (dNoise: every element is read and written back,
 *       += gout on every gap and -= gout on the covered ones);
 *       out[i] past K of semicrf_interval_marginals[_tol]; Cn / noiseP / dNoise when T = 1 (they have no elements).
 *     Everything else of an output is written by every call: logZ [B], v / beta / q_out [T][B], dScore / C [T][T][B] (zeros
 *     included, without the flag), dNoise / Cn / noiseP [T-1][B], offsets (all B+1, nSample*B+1, k*B+1 entries), scores [k][B],
 *     npaths [B], node / begin / end / single [T][B], entropy / E / H / out / logProb [B].
 *
 *   Accuracy of the sweeps, per element (tests/test_sweep_accuracy.py asserts every sentence against float64 of the same fp32 inputs;
 *   tests/sweep_accuracy_common.py counts the constants operation by operation).  u = 2^-24, natural-log units.  For chain c let A_c
 *   be the largest magnitude among its alpha, beta, logZ, the scores end >= begin and the noise, and P_c its largest
 *   softplus(score[t][t]).  An element of v / alpha, beta / q_out or logZ with n recurrence steps behind it (alpha[t]: t + 1,
 *   beta[t]: T - t, logZ: T) is within
 *       L(n) = u ((a n + b) A_c + s n P_c + c0 n + c1 n^2 / 2)
 *   of the float64 value: a, b count a step's (an output's) roundings at the size of alpha, s those inside softplus, c0 those at
 *   magnitude one (exp2 / log2 at 1 ulp, the linear-domain sums), c1 the serial part of a row's sum.
 *       persistent sweep (implementation 0, T >= 2, NBatch >= 2, T <= 2048): a = 6.25, b = 1.1, s = 3.25, c1 = 0, c0 = 257 for
 *                                  the steps at positions below 64 (no far field) and 655 for the others (c0 n is their sum)
 *       row-sequential kernels and the host kernels:                         a = 3,    b = 0,   s = 4,    c0 = 114, c1 = 0.275
 *   A marginal -- dScore[e][b], e >= b, off the target path; out[i] of semicrf_interval_marginals -- has the sign of its float64
 *   value gout gscale m and |ln|got| - ln|value|| <= L_alpha(b + 1) + L_beta(T - e) + L_logZ(T) + E, with E = u (11 A_c + 6.5 P_c +
 *   |ln m| + 256) in the persistent sweep and u (5 A_c + 8 P_c + 3 |ln m| + 8) elsewhere (semicrf_interval_marginals: the latter,
 *   on top of the L of whatever produced its v, q, logZ).  A path cell of semicrf_logprob_bwd holds gout (1 - m) to within
 *   |gout| (m (e^bound - 1) + 2u); dNoise[t] is ONE term, the marginal of the skip over gap t, to within |g| (m (e^bound - 1) + 3u)
 *   with the bound of alpha[t], beta[t + 1], logZ and E.  Cells begin > end are +0.0f.  Below 2^-100 |gout gscale| a value is only
 *   finite, of the right sign or zero, and below 2^-99 |gout gscale| (fp32 exp2 returns 0 near 2^-126).  One exception: the
 *   persistent gradient sweep forms a far-field marginal (row block k >= 4 of the descending sweep, column tile m <= k - 4) as
 *   (gz 2^(M + arow)) 2^(t - M) around the reference M of its accumulator, which an earlier cell of the same row, chain and column
 *   part (12 tiles) set to 96 above its own term, and v_exp_f32 returns 0 below -126.  Such a cell may be exactly 0 if one of those
 *   earlier cells has a marginal below 2^-220 (the common factor is then 0), or if its own marginal is below 2^-28 of the largest
 *   of them (its own factor is).  Where it is not 0 it is within the bound.  No cell of the `balanced` test inputs qualifies at
 *   any length; on an MI355X the rule was needed for marginals between 2^-100 and 2^-75 of the `model` inputs only.  These are
 *   worst-case bounds: measured errors are 4 to 5000 times smaller ("Accuracy of the sweeps, per element").
 *
 * Memory contract of the scorer entry points (interval_score_*, scorer_*; tests/test_scorer_contract.py pins every sentence, S1 .. S12;
 * the test behind each is named in brackets).  Throughout: nothing outside the elements named as written is written, nothing outside the
 * elements named as read reaches a result, an output passed as NULL is not touched, SEMICRF_EINVAL / SEMICRF_EWORKSPACE write nothing;
 * a leading dimension's pad columns (D .. ld-1 of q / k / dq / dk, N .. of the GEMMs' operands and outputs) are neither read nor written.
 *   S1  interval_score_fwd[_p|_pc] READS the D used columns of the C * T rows of q and k, diag[c][t] at stride ldd and rowc[c][t] at
 *       stride ldrc -- no row past T (the tile kernels round T up to 64 or 128 rows and CLAMP the rows they ask for to T - 1), no chain
 *       past C.  diag, rowc, ldd, ldrc and noise_out take any 4-byte alignment.  [test_forward]
 *   S2  It WRITES S[e][b][slot] for e >= b (full_square 2: the cells e < b keep their bits), the exact +0.0f above the diagonal on top
 *       (full_square 0), or the full square (1); every slot of a written cell is written, the ghost slots of a padded pitch with
 *       +0.0f; noise_out [T-1][Cs] is zero-filled when non-NULL (T == 1: it has no elements).  [test_forward]
 *   S3  Alignment is a matter of the ROUTE, never of correctness (semicrf_debug_score_route states it): with q, k and S 16-byte aligned,
 *       ldq % 4 == 0, ldk % 4 == 0 and T * ld * 4 < 2^31 the LDS-staged kernels run (16-byte loads of the rows, 16-byte stores of S's
 *       chain axis); anything else -- rows of a packed [C][T][2D+1] tensor, an S off 16 bytes -- runs the register-load kernel
 *       (D % 64 == 0: dword loads and stores) or the plain kernel: the same scores to the bound below, not bit for bit (the streaming
 *       kernel sums two accumulators, the register-load kernel one).  A padded pitch or a row constant exists in the
 *       tiled kernels only: D % 64 == 0, T >= 128 and that alignment, else SEMICRF_EINVAL; so are a pitch that is no multiple of 4 and
 *       ldq / ldk < D.  [test_forward_route_table, test_forward_refused, test_forward_S_off_16_bytes_takes_the_register_load_kernel]
 *   S4  interval_score_bwd_ws and _ws_p are _ws_pc with drowc == NULL (and group == pitch == C): the same bits; interval_score_bwd is
 *       the direct kernels.  [test_backward_entry_point_forms]
 *   S5  The backward READS dS[e][b][slot] for e >= b in the slots of real chains only -- the cells e < b and the ghost slots of a
 *       padded pitch may hold anything (the CRF's gradient there is not zero) -- and the D used columns of q and k.  dS takes any 4-byte
 *       alignment (16-byte loads where C % 4 == 0 and it is 16-byte aligned).  [test_backward_direct_kernels,
 *       test_backward_packed_gemms, test_backward_slot_layout]
 *   S6  It WRITES (never adds to) the D used columns of dq[c][t] and dk[c][t], ddiag[c][t] at stride lddd (bit-equal to dS[t][t][c])
 *       and drowc[c][t] at stride lddrc; each output only when its pointer is non-NULL, and with the bits of the call that asks for
 *       all of them.  Outputs take any 4-byte alignment and any leading dimension >= D.  [test_backward_output_subsets]
 *   S7  The packed path runs when D is 64, 128 or 256, T >= 64, q and k are 16-byte aligned with ldq % 4 == 0 and ldk % 4 == 0, ws is
 *       non-NULL, 16-byte aligned and holds interval_score_bwd_workspace_bytes(C, T, D) bytes, dq or dk is wanted, and drowc is not
 *       wanted without dq (its row sums come out of the dq product).  Otherwise the call runs exactly interval_score_bwd (+ a row-sum
 *       kernel for drowc): the same bits as that entry point; with a padded pitch, which only the packed path knows,
 *       SEMICRF_EINVAL.  [test_backward_falls_back_to_the_direct_kernels, test_backward_slot_layout]
 *   S8  ws of the backward: exactly interval_score_bwd_workspace_bytes(C, T, D) bytes (the 4096 bytes of slack for the transposed walk
 *       of the last tile are part of that figure), 16-byte aligned; nothing past ws + ws_bytes is read or written and what it held
 *       before the call does not matter.  [test_backward_workspace_contents_do_not_matter, test_backward_packed_gemms]
 *   S9  interval_score_bwd_fused[_ws[_p|_pc]] read S for e >= b (real slots), alpha and beta [T][Cs], logZ and gout [Cs] instead of dS;
 *       any 4-byte alignment (16-byte loads where Cs % 4 == 0 and S, alpha and beta are 16-byte aligned); outputs, workspace and
 *       fallback as S6 - S8.  [test_backward_fused]
 *   S10 interval_score_path_bwd[_p|_pc] ADDS (4-byte atomics): w k[c][b][:] to dq[c][e][:D], w q[c][e][:] to dk[c][b][:D], w to
 *       drowc[c][e], gout to ddiag[c][e] when b == e, for every interval; every other row and entry keeps its bits; K == 0 launches
 *       nothing.  It reads gout [Cs], offsets [Cs + 1], pairs [K][2] and the rows of q and k that paths name.  [test_path_backward]
 *   S11 scorer_proj_nn / _nn3 READ the K used columns of A's M rows (rows past M and contraction values past K are clamped back into
 *       the matrix), B's Kpad = ceil(K / 32) * 32 rows of N columns -- the caller keeps the rows K .. Kpad-1 ZERO in memory --, bias [N]
 *       (NOT with accumulate: an accumulating call adds the product alone), w2 [2][K], b2 [2]; they WRITE out[m][0 .. N-1] (accumulate:
 *       add to it) and with w2 the two extra columns and zero_cols exact zeros behind them (written, not added).  A, B: 16-byte aligned,
 *       lda % 4 == 0, ldb % 4 == 0, M * lda * 4 < 2^31; N in {64, 128, 256}, K % 4 == 0, ldout >= N (+ 2 + zero_cols): enforced,
 *       SEMICRF_EINVAL before anything is launched.  out, bias, w2, b2, ldout: any 4-byte alignment.  scorer_proj_nn3's ws: exactly
 *       scorer_proj_nn3_workspace_bytes(K, N) bytes, 16-byte aligned, earlier contents do not matter; without it (NULL, short, off 16
 *       bytes, N != 256) the call is scorer_proj_nn, bit for bit.  scorer_proj_tn READS the R main columns of dy's M rows, the columns
 *       extra_col0 and extra_col0 + 1 (>= R; or -1) and the N used columns of x; it WRITES dW[r][0 .. N-1] and db[r] for r <
 *       total_rows, exact zeros from R + 2 (R without extra columns) on.  dy, x: 16-byte aligned with lddy % 4 == 0, ldx % 4 == 0
 *       (enforced); dW, db, lddw: any 4-byte alignment.  Its ws: exactly scorer_proj_tn_workspace_bytes(M, R, N) bytes, 16-byte aligned,
 *       earlier contents do not matter; NULL, short or misaligned: SEMICRF_EWORKSPACE.  With SEMICRF_PROJ_TN_BF16X3 the two extra rows
 *       and db are the exact call's bits.  [test_proj_nn_every_width, test_proj_nn_every_row_count, test_proj_nn3, test_proj_tn,
 *       test_projection_rejections_host, test_projection_rejections_device]
 *   S12 scorer_stage_linear, scorer_merge_weights_fwd / _bwd: contiguous operands and outputs at any 4-byte alignment.  They write every
 *       element of BT [size][2 D], Wqd [rows_pad][size], w2 [2][size], b2 [2]; of Wm [rows][size], bm [rows] and (when non-NULL) WmT
 *       [size][size]; of dW [2 D + 1][size] and dbias [2 D + 1] -- the rows behind the diagonal row exact zeros; _bwd reads the first
 *       size + 2 rows of dWm / entries of dbm.  _bwd's ws: exactly scorer_merge_weights_bwd_workspace_bytes(size) bytes, 4-byte
 *       aligned, earlier contents do not matter; NULL or short: SEMICRF_EWORKSPACE.  [test_stage_linear, test_merge_weights]
 *   Accuracy, per element against float64 (u = 2^-24; derivations: tests/scorer_contract_common.py): forward (D + 8) u (qscale len
 *   (sum_d |q k| + |rowc|) + |diag|); dq / dk (n + 8) u sum |G k| over the n terms of the row; scorer_proj_nn (K + 4) u (sum_k |a b| +
 *   |bias|); scorer_proj_tn (M + 8) u sum_m |dy x|; the three-limb forms add 2^-21 of the same sum.
 */
#ifndef SEMICRF_HIP_H
#define SEMICRF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: rounds 1-4.  2 (round 6; the changes themselves are round 5's): new entry points scorer_proj_nn3 /
 * scorer_proj_nn3_workspace_bytes and the flag bits SEMICRF_LEN_BF16X3, SEMICRF_PROJ_TN_BF16X3; semicrf_workspace_bytes(LOGZ_FWD /
 * LOGZ_BWD / VITERBI) grew by a second u buffer (leased workspaces alternate), B path-score granules and -- for launches of at most
 * 192 chains -- the spine-major band copy K * ceil(B/4) * 4 * 4 KB + its flag words (tens to ~200 MB at T = 1024..2048): callers
 * must size workspaces with semicrf_workspace_bytes of THIS library, never with a constant from an older one.  No entry point of
 * version 1 changed its signature or meaning. */
#define SEMICRF_ABI_VERSION 2

#define SEMICRF_OK 0
#define SEMICRF_EINVAL 1      /* bad shape / null pointer / unsupported size */
#define SEMICRF_EWORKSPACE 2  /* ws_bytes too small */
#define SEMICRF_ELAUNCH 3     /* HIP reported an error at enqueue time */
#define SEMICRF_ETIMEOUT 4    /* an EARLIER sweep gave up on a bounded wait on the device (see semicrf_async_error); nothing enqueued */

/* op ids for semicrf_workspace_bytes */
#define SEMICRF_OP_LOGZ_FWD 0
#define SEMICRF_OP_LOGZ_BWD 1
#define SEMICRF_OP_VITERBI 2
#define SEMICRF_OP_EVAL_PATH 3
#define SEMICRF_OP_INTERVAL_SCORE 4
#define SEMICRF_OP_SAMPLE 5           /* B = nSample * NBatch of the semicrf_sample call */
#define SEMICRF_OP_VITERBI_NBEST 6    /* B = k * NBatch of the semicrf_viterbi_nbest call */
#define SEMICRF_OP_POSTERIORS 7       /* semicrf_posteriors */
#define SEMICRF_OP_MARGINAL_DECODE 8   /* semicrf_marginal_decode */
#define SEMICRF_OP_EXPECTATION 9       /* semicrf_expectation / semicrf_covariance (one workspace for the pair) */
#define SEMICRF_OP_MBR_SELECT 10       /* semicrf_mbr_select */
#define SEMICRF_OP_MARGINAL_DECODE_TOL 11   /* semicrf_marginal_decode_tol */
#define SEMICRF_OP_ATTRIBUTE_HEADS 12       /* semicrf_attribute_heads: T = rows K, B = Hv + Ho (see there) */
#define SEMICRF_OP_ATTRIBUTE_HEADS_BWD 13   /* semicrf_attribute_heads_bwd: T = rows K, B = Hv + Ho (see there) */
#define SEMICRF_OP_FFN_RESIDUAL_BWD 14      /* semicrf_ffn_residual_bwd: T = tokens n0 n1, B = hidden (see there) */

#define SEMICRF_WS_ALIGN 256           /* required alignment of every `ws` of the semicrf_* entry points (enforced: SEMICRF_EINVAL) */

#define SEMICRF_TOL_MAX 8              /* largest onset / offset tolerance (frames) of the *_tol entry points */

/* length scaling of the interval scorer (LayersTransformer.py:416-427) */
#define SEMICRF_LEN_LINEAR 0
#define SEMICRF_LEN_SQRT 1
#define SEMICRF_LEN_NONE 2

/* interval_score_fwd, full_square bit 2 (OR it to 0 / 1 / 2): opt-in contraction on the bf16 matrix instructions.  Default
 * (bit clear) is the exact fp32 contraction.  With the bit every operand is split exactly into three bf16 limbs and six of
 * the nine limb products are accumulated in fp32: |S - S_exact| <= 2^-21 * qscale * len * sum_d |q_d k_d| (measured
 * <= 2^-22; tests/test_gpu_parity.py::test_scorer_bf16x3), i.e. fp32-grade but NOT bit-identical to the default, 1.3-1.4x
 * faster.  Operands must be finite with |x| < 2^127 (the first limb rounds to nearest: larger values round to infinity);
 * limbs below the bf16 normal range (|x| < 2^-110) may be flushed to zero by the matrix instruction. */
#define SEMICRF_SCORE_BF16X3 4
/* The same for the backward: OR it to length_scaling of interval_score_bwd_ws* / interval_score_bwd_fused_ws* (bit 4).  The two
 * products dq = G k, dk = G^T q run on the bf16 matrix instructions with every operand (the scaled cotangent G as well as k and q)
 * split exactly into three limbs: |dq - dq_exact| <= 2^-21 * sum_b |G[e,b] k[b,d]| per element (likewise dk), fp32-grade, not
 * bit-identical to the default.  Honoured where the packed path runs (workspace, D in {64,128,256}, T >= 64, aligned rows);
 * the direct kernels ignore it (exact fp32).  ddiag and drowc are exact fp32 sums either way (drowc in a different fixed order). */
#define SEMICRF_LEN_BF16X3 16

typedef void* semicrf_stream_t;

int semicrf_abi_version(void);
const char* semicrf_last_error(void);
size_t semicrf_workspace_bytes(int op, int T, int B);

/* Optional: LEASED workspaces.  The sweeps (semicrf_logz_fwd / _logz_bwd / _beta / _viterbi) need their scratch to read
 * 0xff when they start and therefore fill a caller-owned buffer in front of every launch (17 MB, 6.8 us at T=1024,
 * NBatch=352).  A buffer the caller registers is filled once; every launch leaves it the way the fill would.  The caller
 * promises, until semicrf_workspace_unregister:
 *   - nothing but this library's sweeps writes to the buffer (pass the registered base pointer as `ws`, unchanged);
 *   - at most one stream uses it at a time (launches into one workspace are ordered by the stream they are enqueued on);
 *   - the calling thread's current device is the buffer's device when it registers.
 * (Stream capture: a sweep enqueued on a capturing stream takes the ordinary path -- its fill becomes a node of the graph --
 *  whatever the workspace; every entry point of this library can be captured into a HIP graph and replayed.)
 * A change of (operation, T, B) costs one fill.  A launch that aborted (see below: NaN outputs / negative decode total)
 * raises a pinned host word; the next launch of ANY lease is preceded by a fill again.  semicrf_workspace_register may
 * synchronise the device (once per device); call it at set-up time.  (No counterpart in the reference: its
 * NeuralSemiCRFInterval.py:207-246, :386-414 allocate their temporaries per call.) */
int semicrf_workspace_register(void* ws, size_t ws_bytes);
int semicrf_workspace_unregister(void* ws);

/* Select kernel implementation: 0 = auto (fastest valid), 1 = row-sequential reference kernels.
 * Process-wide; meant for tests and A/B benchmarking. */
void semicrf_set_impl(int impl);
int semicrf_get_impl(void);

/* Debug/test hook, SYNCHRONISES the device: returns and clears the sticky device-side status word.
 * 0 = no kernel ever gave up on a bounded spin; 2..12 = a hand-off wait timed out (results invalid);
 * -1 = HIP error.  The persistent kernels never hang: every wait is bounded (0.3 - 2 s).
 *
 * What a caller sees WITHOUT this hook when a wait does time out (e.g. the GPU is shared and part of the persistent
 * kernel was not resident in time): the calls still return SEMICRF_OK -- nothing synchronises the host -- but the results
 * are poisoned, not silently wrong: logZ, the last row of v / q_out / beta and the gradient's last diagonal cells are NaN
 * for the chains of every workgroup that saw a timeout, and semicrf_viterbi writes offsets[B] = -1. */
int semicrf_debug_device_status(void);

/* The asynchronous error word, WITHOUT synchronising: nonzero (the device's code, 2..13) when a sweep enqueued earlier by this
 * process has given up on a bounded hand-off wait since the last look; reading clears it.  Every sweep entry point
 * (semicrf_logz_fwd / _logz_bwd / _beta / _viterbi / _logprob_*) looks first and returns SEMICRF_ETIMEOUT -- enqueueing nothing -- so
 * that a time-out is an ERROR on the caller's next call at the latest, not only NaN-poisoned outputs; a caller that synchronises
 * (reads results on the host) can ask here right after its synchronisation.  The word is raised by the device with a
 * system-scope store when the wait gives up, i.e. before the poisoned outputs are written.  (Error convention of the boundary:
 * SURVEY.md 8b -- the reference raises on every failure; it has no asynchronous ones.) */
int semicrf_async_error(void);

/* Host-side view of the sweeps' workgroup -> role map (test hook, no device work): the role ticket of workgroup `block`
 * in a launch of `grid` workgroups of which `n_spine` are ring workgroups.  Tickets < n_spine are rings (ticket = the
 * 4-chain group); the eight rings of a 32-chain panel group get workgroup indices that are equal modulo 8 (one XCD). */
int semicrf_debug_wg_ticket(int n_spine, int grid, int block);

/* Test hook, process-wide: force one of interval_score_fwd's kernels where it applies (0 = register loads, 32 = streaming,
 * 2 = the 64 x 128 tiles with the epilogue inside the contraction loop; 64 / 128 = the earlier shared-operand tiles, compiled into
 * the DEBUG library only -- libsemicrf_hip_debug.so, the same ABI built with -DSEMICRF_DEBUG_BUILD=1, which the parity tests load
 * through ctypes as the bit-level reference of 2; the release library ignores 64 / 128.  The kernels agree to fp32 rounding, not all bit
 * for bit: the register-load kernel sums one accumulator, the streaming kernel two -- tests/test_scorer_contract.py); -1 =
 * automatic choice (the default).  The release library reads no environment variables. */
void semicrf_debug_score_variant(int variant);

/* Host-side view of interval_score_fwd's kernel choice (test hook, no device work, nothing is read from the process's state): the
 * kernel that a call with C chains, T frames, contraction size D, row strides ldq / ldk, 16-byte aligned q, k and S (aligned != 0),
 * precision prec (1 = SEMICRF_SCORE_BF16X3), the slot layout group / pitch, a row constant (rowc != 0), the forced variant
 * (semicrf_debug_score_variant's argument) and the implementation impl (semicrf_set_impl's) would run.  The answer is in
 * semicrf_debug_score_variant's numbering, extended: 0 register loads, 1 the plain kernel, 2 the 64 x 128 tiles, 3 the three-limb
 * bf16 tiles, 32 streaming, 64 / 128 the reference tiles (debug library only), -1 the call is refused with SEMICRF_EINVAL.
 * (A test hook: SEMICRF_ABI_VERSION stays 2, as for the entry points added since round 6.) */
int semicrf_debug_score_route(int C, int T, int D, int64_t ldq, int64_t ldk, int aligned, int prec, int group, int pitch, int rowc,
                              int forced, int impl);

/*
 * Log-partition, forward (alpha) sweep.
 * Replaces: computeLogZ (NeuralSemiCRFInterval.py:207-246) and the un-flipped half of
 * forward_backward (:394-410,:417).
 *   v[0] = softplus(s[0,0]);  v[i] = logaddexp(v[i-1]+n[i-1], logsumexp_{j<i}(v[j]+s[i,j])) + softplus(s[i,i])
 * Outputs: logZ [B] (= v[T-1]);  v [T][B] (may be NULL when no backward will follow).
 */
int semicrf_logz_fwd(const float* score, const float* noise, int T, int B,
                     float* logZ, float* v, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Gradient of sum_c gout[c]*logZ[c] w.r.t. score and noise: the backward (beta) sweep fused with
 * the marginals.  Replaces: the flipped half of forward_backward (:386-414), the marginals
 * (:424-447) and ComputeLogZFasterGrad.backward (:469-472).
 *   dScore[e,b,c] = gout[c] * exp(v[b] + q[e] - logZ + s[e,b])                     e > b
 *   dScore[t,t,c] = gout[c] * exp(v[t] + q[t] - logZ + s[t,t] - 2 softplus(s[t,t]))
 *   dScore[e,b,c] = 0 exactly                                                       e < b
 *   dNoise[t,c]   = gout[c] * exp(v[t] + q[t+1] + n[t] - logZ)
 * Inputs v, logZ come from semicrf_logz_fwd on the same score/noise.  dScore [T][T][B] is fully
 * written (including the zeros).  q_out [T][B] may be NULL.
 */
int semicrf_logz_bwd(const float* score, const float* noise, const float* v, const float* logZ,
                     const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out,
                     void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Viterbi decode.  Replaces: viterbiBackward (:13-104, forward=0, the default of .decode) and
 * viterbi (:107-202, forward=1), including the backtrack that the reference runs on the host.
 *   start: NULL or B ints (forcedStartPos; for forward=1 it is the END position, :161-165).
 *   pairs: int32 [cap][2] (begin,end), chain-major, ascending within a chain (packed).
 *   offsets: int32 [B+1] prefix counts; offsets[B] = total.  If total > cap the pairs content is
 *   truncated but offsets are still exact (callers allocate cap = B*(2T) to be safe, or retry).
 * Decoded indices are bit-identical to the reference's CPU path (first-maximum tie-break in the
 * candidate order [skip, nearest, ..., farthest], single fp32 add per candidate).
 */
int semicrf_viterbi(const float* score, const float* noise, int T, int B, const int32_t* start,
                    int forward, int32_t* pairs, int64_t cap, int32_t* offsets,
                    void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Exact posterior sampling of paths, p(y) = exp(evalPath(y) - logZ) (forward-filtering backward-sampling).  No counterpart in
 * the reference (an extension of its surface, like decode_packed).  Adds nothing to the ABI's existing entry points (version 2).
 *   v: alpha [T][B] of semicrf_logz_fwd on the same score / noise.
 *   Draws k0 .. k0 + nSample - 1.  Draw k of chain c walks from t = T-1 (end == NULL) or end[c] down to frame 0; at a visited
 *   frame t > 0 the predecessor is drawn from [skip, j = t-1, ..., 0] with weights exp(v[t-1] + n[t-1]), exp(v[j] + s[t,j]) by
 *   inverse CDF over the row's own max-shifted sum Z (a candidate of weight 0 is never chosen; a threshold at or past the last
 *   partial sum takes the last candidate of positive weight; a row without one takes the skip); at every visited frame (t,t)
 *   is emitted iff u' < sigmoid(s[t,t]).
 *   Uniforms: u = (splitmix64(idx, key) >> 40) * 2^-24, idx = ((k*B + c)*T + t)*2 + r, r = 0 predecessor, 1 singleton; the
 *   result depends on (inputs, key, k) only -- not on nSample, k0 splits, grid or device.
 *   pairs [cap][2], offsets [nSample*B + 1]: sample-major (chain c of draw k0 + k owns offsets[k*B + c] : offsets[k*B + c + 1]),
 *   ascending by (begin, end) within a path, as semicrf_viterbi(forward = 1).  offsets[nSample*B] = -1 when v holds NaN in its
 *   last row (a sweep that gave up on a bounded wait).
 *   Workspace: semicrf_workspace_bytes(SEMICRF_OP_SAMPLE, T, nSample * B), about 5 * nSample * B * T int32.
 */
int semicrf_sample(const float* score, const float* noise, const float* v, int T, int B, int64_t k0, int nSample,
                   uint64_t key, const int32_t* end, int32_t* pairs, int64_t cap, int32_t* offsets,
                   void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * k-best Viterbi: the k highest-scoring paths of every chain, ranked.  No counterpart in the reference (an extension of its
 * surface, like decode_packed).  Adds nothing to the ABI's existing entry points (version 2).
 *   A path is what semicrf_viterbi returns for a chain; its value is the Viterbi recursion's: one fp32 add per candidate, the
 *   singleton last (u = best + (singleton ? s[t,t] : 0)).  At every frame the partial paths are ordered by (1) value, descending,
 *   (2) value before the singleton, descending, (3) candidate in semicrf_viterbi's tie order (skip first, then the smaller index
 *   of the other endpoint), (4) predecessor rank, ascending, (5) the singleton, "on" first iff s[t,t] > 0; the first k are kept.
 *   The order does not depend on k: k = 1 is semicrf_viterbi bit for bit, and the first m ranks of k are the m-best.
 *   k: 1..16.  start, forward: as semicrf_viterbi (start is the END frame when forward = 1).
 *   pairs [cap][2], offsets [k*B + 1]: rank-major (chain c of rank r owns offsets[r*B + c] : offsets[r*B + c + 1]), each path in
 *   semicrf_viterbi's order.  scores [k][B]: the ranked values; npaths [B]: how many ranks exist (fewer than k paths at tiny T).
 *   An absent rank has no intervals and score -inf; a real path of value -inf (-inf cells) is present.
 *   Workspace: semicrf_workspace_bytes(SEMICRF_OP_VITERBI_NBEST, T, k * B), about 9 * k * B * T int32.
 */
int semicrf_viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int32_t* start, int forward,
                          int32_t* pairs, int64_t cap, int32_t* offsets, float* scores, int32_t* npaths, void* ws, size_t ws_bytes,
                          semicrf_stream_t stream);

/*
 * Posterior marginals and path entropy.  No counterpart in the reference (an extension of its surface, like semicrf_sample).
 * Adds nothing to the ABI's existing entry points (version 2).
 *   v: alpha [T][B] (semicrf_logz_fwd), q: beta [T][B] (semicrf_beta), logZ [B], all on the same score / noise.  q[t], like v[t],
 *   includes softplus(s[t,t]) of its own frame.  sp = softplus (threshold 20), sigma = the logistic sigmoid,
 *   R[t] = v[t] - sp(s[t,t]) (the log row total of alpha's recursion at t), mu[e,b] = dScore of semicrf_logz_bwd with gout = 1.
 *   node   [T][B]   P(frame t is a node of the path, i.e. not strictly inside an interval) = exp(R[t] + q[t] - logZ); 1 at 0, T-1
 *   single [T][B]   P((t,t) on the path) = node[t] sigma(s[t,t]) = mu[t,t]
 *   begin  [T][B]   P(an interval (t,e), e > t, on the path) = sum_{e>t} mu[e,t]
 *   end    [T][B]   P(an interval (b,t), b < t, on the path) = sum_{b<t} mu[t,b]
 *   noiseP [T-1][B] dNoise of semicrf_logz_bwd with gout = 1: exp(v[t] + n[t] + q[t+1] - logZ)   (may be NULL when T = 1)
 *   entropy [B]     H = sum_t node[t] (Hb(s[t,t]) + Hpred[t]) by the chain rule of semicrf_sample's backward walk:
 *                   Hb(x) = sp(x) - x sigma(x) (the singleton's Bernoulli entropy); Hpred[0] = 0, Hpred[t] = -sum p lp over the
 *                   candidates [skip, j = 0..t-1], lp_skip = v[t-1] + n[t-1] - R[t], lp_j = v[j] + s[t,j] - R[t]; a term of p = 0 is 0
 *                   and every lp is clamped to <= 0, so no term is negative and nothing cancels.
 *   Probabilities are clamped to <= 1 (NaN stays NaN).  One read of the lower triangle; no atomics: two calls are bit-identical.
 *   Workspace: semicrf_workspace_bytes(SEMICRF_OP_POSTERIORS, T, B), about 2 * ceil(T/64) * T * B floats.
 */
int semicrf_posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                       float* node, float* begin, float* end, float* single, float* noiseP, float* entropy, void* ws, size_t ws_bytes,
                       semicrf_stream_t stream);

/*
 * Marginals of given intervals: out[i] = mu[e,b] of interval i = (b, e) (pairs / offsets / K as semicrf_eval_path; v, q, logZ as
 * semicrf_posteriors): exp(v[b] + s[e,b] + q[e] - logZ) for b < e, single[t] for b = e, 0 for b > e (never on a path), NaN for an
 * index outside [0, T).  No workspace.
 */
int semicrf_interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B,
                               const int32_t* pairs, int64_t K, const int32_t* offsets, float* out, semicrf_stream_t stream);

/*
 * Marginal-threshold (posterior) decoding: every cell (e, b), b <= e, of chain c with m(e, b, c) >= tau[c * tau_stride], packed.
 * No counterpart in the reference (an extension of its surface, like semicrf_posteriors).  Adds nothing to the ABI's existing
 * entry points (version 2).
 *   v, q, logZ: as semicrf_posteriors.  noise is not read (it is inside v and q); it may be NULL only when T = 1.
 *   m(e, b, c) is the value semicrf_interval_marginals returns for (b, e) of chain c, bit for bit (both evaluate the same inline
 *   functions).  The comparison is m >= tau in fp32; a NaN m or a NaN tau selects nothing.
 *   tau: a DEVICE pointer; tau_stride 0 (one value for all chains) or 1 (per chain: per-symbol calibration).
 *   pairs [cap][2] (begin, end), probs [cap] (probs[i] = m of interval i), offsets [B+1]: chain-major; within a chain ascending by
 *   (begin, end), as semicrf_sample / semicrf_viterbi(forward = 1) order a path.  Two cells that overlap cannot lie on one path, so
 *   their marginals sum to <= 1: for tau > 0.5 the selected cells of a chain are pairwise compatible -- a path in the sense of
 *   semicrf_viterbi (then (begin, end) order is also ascending by end); for tau <= 0.5 they are a candidate lattice that may overlap.
 *   offsets is exact even when offsets[B] > cap; pairs / probs then hold the first cap entries of that order and nothing is written
 *   out of bounds (the semicrf_viterbi convention).  offsets[B] = -1 when v holds NaN in its last row (a sweep that gave up on a
 *   bounded wait; the semicrf_sample convention).
 *   Bound for callers: sum_{e > b} m(e, b) <= 1 for every b, so a chain has at most T * (floor(1 / tau) + 1) selected cells
 *   (singletons included); for tau > 0.5 that is the 2 T of semicrf_viterbi.  T (T+1) / 2 * B must stay below 2^31.
 *   No host synchronisation, no atomics: the result is a pure function of the inputs, two calls are bit-identical.  One read of the
 *   lower triangle plus the rows that hold a selected cell.
 *   Workspace: semicrf_workspace_bytes(SEMICRF_OP_MARGINAL_DECODE, T, B), about (1.5 * ceil(T/64) + 1) * T * B int32.
 */
int semicrf_marginal_decode(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                            const float* tau, int tau_stride, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets,
                            void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Posterior (minimum-Bayes-risk) PATH decoding at any threshold: among all paths of a chain, the one that maximises the sum over
 * its intervals of (m(e, b) - tau) -- the gain 1 - tau per correct and -tau per wrong interval, solved for every tau (for
 * tau > 0.5 it is the set {m > tau} itself).  An interval with m <= tau can be replaced by noise gaps without loss, so the optimum
 * uses only the cells a semicrf_marginal_decode call at the same tau emits: the call is a weighted-interval-scheduling dynamic
 * program over that packed lattice; it reads neither the scores nor a [T][T][B] tensor.  No counterpart in the reference (an
 * extension of its surface, like semicrf_marginal_decode).  Adds nothing to the ABI's existing entry points (version 2).
 *   pairs [K][2] (begin, end), weight [K], offsets [B+1]: a lattice in semicrf_marginal_decode's format (its pairs / probs /
 *   offsets), ascending by (begin, end) within a chain, 0 <= begin <= end < T; K = the lattice's capacity (the `cap` of that call).
 *   tau, tau_stride: as semicrf_marginal_decode; chain c uses tau[c * tau_stride].
 *   Eligibility: entry i is eligible iff weight[i] > tau (a strict fp32 compare; NaN is never eligible; an entry outside
 *   0 <= begin <= end < T is never eligible).  Its gain is g_i = weight[i] - tau, one fp32 subtraction.
 *   gS(t) = g of the eligible entry (t, t), else +0.0f.
 *   Recursion (all fp32, every sum one add):  F[T-1] = gS(T-1);  for t = T-2 .. 0: best = F[t+1], choice "skip"; for the eligible
 *   entries (t, e), e > t, in ascending e: c = g_i + F[e]; if c > best (strict): best = c, choice i;  F[t] = best + gS(t).
 *   Among equal maxima the skip wins, after it the smallest e (the values do not depend on the order the maximum is taken in).
 *   Trace from t = 0: at a visited frame emit (t, t) if it is eligible; stop at t = T-1; on "skip" go to t + 1, otherwise emit
 *   (t, e) and go to e.  The output is ascending by (begin, end), the order of semicrf_viterbi(forward = 1).
 *   pairs_out [cap][2], probs_out [cap]: the selected entries and their weights, bit for bit; offsets_out [B+1], exact even when
 *   offsets_out[B] > cap, nothing is written out of bounds (a path has at most 2 T - 1 cells: cap = 2 T B always suffices);
 *   gain [B] = F[0].
 *   offsets[B] is read on the DEVICE: when it is negative (semicrf_marginal_decode's NaN convention) or exceeds K (a truncated
 *   lattice), offsets_out[B] = -1, the other offsets and gain are 0 and nothing is selected -- the two calls chain without a host
 *   synchronisation in between.
 *   No atomics, fixed order: two calls are bit-identical.  2 T B must stay below 2^31.
 *   Workspace: semicrf_workspace_bytes(SEMICRF_OP_MBR_SELECT, T, B), about 7 T B int32 (8 T B for T > 4096, where the recursion's
 *   values do not stay on chip).  pairs must be 8-byte aligned.
 */
int semicrf_mbr_select(const int32_t* pairs, const float* weight, const int32_t* offsets, int64_t K, int T, int B, const float* tau,
                       int tau_stride, int32_t* pairs_out, float* probs_out, int64_t cap, int32_t* offsets_out, float* gain,
                       void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Onset/offset-tolerant interval posteriors and marginal-threshold decoding.  No counterpart in the reference (an extension of its
 * surface, like semicrf_marginal_decode).  Adds nothing to the ABI's existing entry points (version 2).
 *
 * Tolerances are tol_begin = db and tol_end = de, in frames, with 0 <= db, de <= SEMICRF_TOL_MAX = 8.  For a cell 0 <= b <= e < T
 * of chain c:
 *
 *   row(e') = sum over b' = max(0, b-db) .. min(b+db, e'), ascending, of m(e', b')     (fp32, one add per term)
 *   M(e,b)  = clamp1( sum over e' = max(0, e-de) .. min(T-1, e+de), ascending, of row(e') )
 *
 *   - m(e', b') is the value semicrf_interval_marginals returns for (b', e'), bit for bit.
 *     - That means cell_marginal / cell_marginal_single of posterior_cell.h, each clamped on its own.
 *     - Singletons (t,t) are ordinary cells of the box.
 *   - Rows without a cell (e' < b - db) contribute nothing.
 *   - clamp1 is the existing one: values above 1 become 1 and NaN stays NaN.
 *   - A NaN term makes M NaN, which selects nothing.
 *
 * Meaning: M is the expected number of path intervals whose begin is within db of b and whose end is within de of e, capped at 1.
 *   - For e - b > db + de all cells of the box share an interior frame, so at most one of them lies on a path.  The uncapped sum is
 *     then already a probability: P(some interval of the path matches (b,e) within the tolerance).
 *   - For shorter cells it is the union bound of that probability.
 *   - db = de = 0 gives M = m.
 * The order above is the contract.  It is chosen so that a separable stencil (row sums, then a sum of rows) and a direct gather give
 * the same bits.  Both must sum the 2 db + 1 and 2 de + 1 terms directly, never with a sliding add/subtract.
 *
 * semicrf_interval_marginals_tol: out[i] = M of interval i; arguments as semicrf_interval_marginals; b > e gives 0 and an index
 * outside [0, T) gives NaN.  No workspace.
 * semicrf_marginal_decode_tol: semicrf_marginal_decode with M >= tau in place of m >= tau and probs[i] = M -- chain-major, ascending
 * by (begin, end); offsets exact past cap, nothing written out of bounds; offsets[B] = -1 on a NaN in v's last row; no atomics, no
 * host synchronisation, two calls are bit-identical.  With a tolerance the selected cells of a chain are NOT a path even for
 * tau > 0.5 (neighbouring cells pass together; a box holds up to 2 (2 db + 1)(2 de + 1) of mass per begin): the result is a lattice
 * for semicrf_mbr_select.  The triangle is read once per tile plus the tile's halo of de rows and db columns, plus the boxes of the
 * rows that hold a selected cell.
 * A tolerance outside [0, 8] returns SEMICRF_EINVAL.  With (0, 0) both calls forward to the entry points they extend.
 * Workspace: semicrf_workspace_bytes(SEMICRF_OP_MARGINAL_DECODE_TOL, T, B), the size of SEMICRF_OP_MARGINAL_DECODE.
 */
int semicrf_interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B,
                                   const int32_t* pairs, int64_t K, const int32_t* offsets, int tol_begin, int tol_end, float* out,
                                   semicrf_stream_t stream);
int semicrf_marginal_decode_tol(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                                const float* tau, int tau_stride, int tol_begin, int tol_end, int32_t* pairs, float* probs, int64_t cap,
                                int32_t* offsets, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Posterior expectation of an additive path functional, and its covariance with every cell of the lattice (the Hessian-vector
 * product of logZ).  No counterpart in the reference (an extension of its surface, like semicrf_posteriors); its computeLogZ is
 * plain torch and can be differentiated twice, which is what these two calls provide explicitly.  Adds nothing to the ABI's
 * existing entry points (version 2).
 *   weight [T][T][B] (the layout of score; only begin <= end is read) and noiseWeight [T-1][B] define
 *     W(path) = sum of weight[e,b] over the intervals (b,e) of the path (singletons included) + sum of noiseWeight[t] over the
 *     gaps t .. t+1 that no interval covers.
 *   weight NULL or == score: the weights ARE the scores and the tensor is read once (pass noiseWeight = noise for the entropy:
 *     then W = the path's score S and H = logZ - E_p[S]).  noiseWeight NULL: zeros.
 *   v: alpha (semicrf_logz_fwd), q: beta (semicrf_beta) of the same score / noise.  They serve only as the shift of each row's
 *     sum: the sweeps keep their own per-frame state -- the log-sums and the conditional expectations of W, forward and backward
 *     -- in float64 (fp32 state cannot resolve the cancellation of a covariance; DESIGN.md "Posterior expectations"), every
 *     per-cell exponential stays fp32 on an argument formed in float64.
 * semicrf_expectation: E [B] = E_p[W]; H [B] = logZ - E (the path entropy when the weights are the scores); leaves the state in
 *   ws.  Two reads of the lower triangle (rows forward, columns backward).
 * semicrf_covariance: from the ws a semicrf_expectation call on the SAME score / noise / weight / noiseWeight filled (same T, B,
 *   unchanged in between), one elementwise pass:
 *     C [T][T][B]:  gout[c] Cov(1[(b,e) on path], W) for b <= e; exactly 0.0f for b > e (every element is written)
 *     Cn [T-1][B]:  gout[c] Cov(1[gap t is noise], W)                (may be NULL when T = 1)
 *   i.e. gout[c] dE[c] / dscore and gout[c] dE[c] / dnoise; with the weights = the scores, dH / dscore = -C, dH / dnoise = -Cn.
 * No atomics, fixed summation order: two calls are bit-identical.  T < 65536.
 * Workspace: semicrf_workspace_bytes(SEMICRF_OP_EXPECTATION, T, B), about 4 T B doubles.
 */
int semicrf_expectation(const float* score, const float* noise, const float* weight, const float* noiseWeight, const float* v,
                        const float* q, int T, int B, float* E, float* H, void* ws, size_t ws_bytes, semicrf_stream_t stream);
int semicrf_covariance(const float* score, const float* noise, const float* weight, const float* noiseWeight, const float* gout, int T,
                       int B, float* C, float* Cn, const void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * The alpha sweep from a forced start: alpha of the semi-CRF restricted to the frames start[c] .. T-1 of chain c -- the model whose
 * MAP path semicrf_viterbi(start) returns.  No counterpart in the reference (its forced start exists for decode only); adds nothing
 * to the ABI's existing entry points (version 2).  With d[t] = score[t,t,c], sp = softplus, S[e,b] = score[e,b,c], n[t] = noise[t,c],
 * s = start[c]:
 *     v[t][c] = -inf                                                                          t <  s
 *     v[s][c] = sp(d[s])
 *     v[t][c] = logaddexp(v[t-1] + n[t-1], logsumexp_{s <= b < t}(v[b] + S[t,b])) + sp(d[t])     t >  s
 *     logZ[c] = v[T-1][c]      (= beta[s] of semicrf_beta up to fp32 rounding: beta[t] depends on the frames >= t only)
 * (logZ, v, beta) are what semicrf_posteriors, semicrf_interval_marginals(_tol) and semicrf_marginal_decode(_tol) take: with this v
 * they describe the conditional model, and every marginal of a cell with begin < start[c] is exactly 0.0f.
 *   start [B], device, int32.  A start[c] outside [0, T-1] gives NaN for logZ[c] and for that chain's column of v; it never causes an
 *     out-of-range access.
 *   Reads only cells begin <= end, and nothing in columns before the chain's start.  Any T >= 1, any B >= 1 (odd B: 16-byte
 *     accesses at 4-byte aligned addresses).  fp32 arithmetic (running-maximum log-sum-exp), fixed summation order: two calls are
 *     bit-identical.  No atomics.
 *   No communication between workgroups: a workgroup owns 16 chains for the whole recurrence -- no flags, no spins, no grid barrier,
 *     no lease; nothing in this call can time out or hang, and it never touches semicrf_async_error's word.
 *   Workspace: none (ws may be NULL, ws_bytes 0).
 */
int semicrf_alpha_from(const float* score, const float* noise, const int32_t* start, int T, int B, float* v, float* logZ, void* ws,
                       size_t ws_bytes, semicrf_stream_t stream);

/*
 * Decoded paths against target paths: the counts behind note-level and frame-level precision / recall, per chain.
 * Replaces: the host loops of TransKun.computeStats (ModelTransformer.py:403-438) -- decode() to Python lists, then compareBracket
 * (Evaluation.py:10-18) and compareFramewise (:67-74) chain by chain -- on the packed lists where semicrf_viterbi left them.  Adds
 * nothing to the ABI's existing entry points (version 2).
 *   est_pairs / est_offsets, ref_pairs / ref_offsets: two packed lists in the format of semicrf_viterbi and semicrf_eval_path
 *   (pairs int32 [K][2] (begin, end), chain-major; offsets int32 [B+1], offsets[B] = the total).  A pairs buffer holds at least
 *   offsets[B] entries (the caller's promise: the call has no capacity argument) and is 8-byte aligned -- every pair is one 8-byte
 *   load; it may be NULL when its total is 0.  The two lists may be the same buffers.
 *   stats int32 [B][7], per chain c:
 *     [0] nRef, [1] nEst   the list lengths
 *     [2] nExact           the number of pairs present in both lists (with multiplicity, should a list repeat a pair); on lists
 *                          without repeats -- every decoded path -- compareBracket's nCorrect
 *     [3] nRefFrames, [4] nEstFrames, [5] nBothFrames
 *                          what compareFramewise(est, ref) returns with countZero = True, bit for bit.  A list's frame count is the
 *                          recurrence s += end - begin + (prevEnd < begin), prevEnd = end (prevEnd = -1 at the start): an interval
 *                          that touches its predecessor shares that frame with it.  nBothFrames is the same recurrence over the
 *                          non-empty closed intersections [max(b, b*), min(e, e*)] of a merge walk over the two lists that advances
 *                          the list whose current interval ends first, the reference list on a tie.
 *     [6] nMatchTol        the size of a maximum matching between the two lists where (b, e) and (b*, e*) can be matched iff
 *                          |b - b*| <= tol_begin and |e - e*| <= tol_end; with (0, 0) it is nExact.
 *   tol_begin, tol_end: 0 .. SEMICRF_TOL_MAX frames; anything else returns SEMICRF_EINVAL.
 * Preconditions are checked on the DEVICE (the lists come from other kernels): every index lies in [0, T), begin <= end, and begin
 * and end are each non-decreasing along a chain's list (singletons and touching intervals included), offsets are non-decreasing
 * within [0, offsets[B]].  A chain that violates one gets all seven entries -1; nothing outside [0, offsets[B]) is read.  When
 * est_offsets[B] or ref_offsets[B] is negative (the NaN / time-out marker of semicrf_viterbi and semicrf_marginal_decode) every
 * entry of every chain is -1: a decode and the comparison chain without a host look in between, as semicrf_mbr_select does.
 * All counts are int32: a chain's lists hold fewer than 2^31 / T entries (a path has at most 2 T - 1).
 * No workspace, no atomics, no host synchronisation; one thread per chain.
 */
int semicrf_compare_paths(const int32_t* est_pairs, const int32_t* est_offsets, const int32_t* ref_pairs, const int32_t* ref_offsets,
                          int T, int B, int tol_begin, int tol_end, int32_t* stats /* [B][7] */, semicrf_stream_t stream);

/*
 * Unnormalised path score.  Replaces: evalPath (:508-550).
 *   pairs int32 [K][2] (begin,end), offsets int32 [B+1] (chain c owns pairs[offsets[c]:offsets[c+1]]).
 *   out[c] = sum_path ( s[end,begin,c] - (cum[end]-cum[begin]) ) + cum[T-1],  cum = prefix sums of noise.
 *   K = number of intervals in pairs (= offsets[B]).
 * PRECONDITION (semicrf_eval_path, semicrf_eval_path_bwd, semicrf_logprob_fwd, semicrf_logprob_bwd[_f]): 0 <= begin <= end < T for
 * every pair.  The device code takes pointers and does not check it: a pair with begin > end would read the cell [end][begin] of
 * the upper triangle (which the scorer leaves unwritten) and its gradient would be added there, into cells that
 * SEMICRF_GRAD_UPPER_IS_ZERO promises to be +0.0f.  The host that packs the pairs checks it (the Python entry points raise
 * ValueError naming the pair before anything is launched; the CPU dispatch rejects the packed buffers).
 * semicrf_interval_marginals is different: it accepts begin > end and returns 0 for it.
 */
int semicrf_eval_path(const float* score, const float* noise, int T, int B,
                      const int32_t* pairs, int64_t K, const int32_t* offsets, float* out,
                      void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Gradient of sum_c gout[c]*evalPath[c], ACCUMULATED (+=) into dScore / dNoise (autograd of the
 * gathers at :540-548).  dScore[end,begin,c] += gout[c] per path interval;
 * dNoise[t,c] += gout[c] * [gap t not covered by an interval of the path].
 * K = number of intervals in pairs (= offsets[B], known to the host that packed them).
 * Either output may be NULL.  Callers that want a fresh gradient zero the buffers first.
 */
int semicrf_eval_path_bwd(const float* gout, int T, int B, const int32_t* pairs, int64_t K,
                          const int32_t* offsets, float* dScore, float* dNoise, semicrf_stream_t stream);

/*
 * logProb as ONE call each way.  Replaces: NeuralSemiCRFInterval.logProb (:587-588: evalPath(intervals) - computeLogZ())
 * and its backward (the autograd of :540-548 plus ComputeLogZFasterGrad.backward :469-472).
 *   semicrf_logprob_fwd: logProb[c] = evalPath[c] - logZ[c]; also leaves logZ [B] and (when non-NULL) v [T][B] for the
 *     backward.  Workspace: semicrf_workspace_bytes(SEMICRF_OP_LOGZ_FWD, T, B).
 *   semicrf_logprob_bwd: gradient of sum_c g[c] * logProb[c] with g[c] = gout[c * gout_stride]; gout_stride is 1 or 0 --
 *     0 reads ONE value for every chain, which is what the loss -logProb.sum() / n hands down (an expanded scalar): no
 *     [B] copy of it and no negated copy are made.  dScore [T][T][B] is fully written (marginals times -g, +g on the path
 *     cells, exact zeros for begin > end), dNoise [T-1][B] likewise.  Workspace: SEMICRF_OP_LOGZ_BWD.
 */
int semicrf_logprob_fwd(const float* score, const float* noise, int T, int B, const int32_t* pairs, int64_t K,
                        const int32_t* offsets, float* logProb, float* logZ, float* v, void* ws, size_t ws_bytes,
                        semicrf_stream_t stream);
int semicrf_logprob_bwd(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                        int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets,
                        float* dScore, float* dNoise, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * The two gradient entry points with flags (replacing the same reference lines as semicrf_logz_bwd / semicrf_logprob_bwd).
 */
/* flags of semicrf_logz_bwd_f / semicrf_logprob_bwd_f */
#define SEMICRF_GRAD_UPPER_IS_ZERO 1   /* the caller's promise: every cell begin > end of dScore already holds +0.0f; the call does
                                        * not write them (a third of the bytes the gradient sweep moves).  transkun_amd keeps a pool
                                        * of gradient buffers whose upper triangle this library zeroed and nobody has written since
                                        * (transkun_amd/CRF: _GradPool); the result is the same dense tensor with an exactly-zero
                                        * upper triangle that NeuralSemiCRFInterval.py:436-440, :469-472 hand to autograd. */
int semicrf_logz_bwd_f(const float* score, const float* noise, const float* v, const float* logZ,
                       const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out, int flags,
                       void* ws, size_t ws_bytes, semicrf_stream_t stream);
int semicrf_logprob_bwd_f(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                          int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets,
                          float* dScore, float* dNoise, int flags, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * logProb's backward as ONE launch: the path table.  semicrf_logprob_bwd[_f] runs the gradient sweep and then a second kernel that
 * scatters +g onto the path's cells and -g onto its covered gaps.  With a table of the path, every writer of the sweep adds those
 * terms to what it stores (the same roundings in the same order: the results are bit-identical) and the second kernel is not
 * launched.
 *   ptab int32 [T][B], index f * B + c, one word per (frame, chain):
 *     bits 0..29  the END frame of the path interval that BEGINS at frame f, SEMICRF_PTAB_NONE if none does;
 *     bit 30      SEMICRF_PTAB_COVERED: the gap between frames f and f + 1 lies inside an interval (begin <= f < end).
 *   semicrf_logprob_fwd_t: semicrf_logprob_fwd, and when ptab is non-NULL the launch also writes every word of ptab (no fill
 *     needed, no extra launch).  ptab belongs to the call: keep it with v / logZ for the backward, not in the workspace.  Non-NULL
 *     only where the persistent sweep runs (T >= 2, NBatch >= 2, implementation 0: SEMICRF_EINVAL otherwise);
 *     semicrf_logprob_path_table_supported(T, B) returns 1 where the backward call will also USE the table -- where it returns 0
 *     but the sweep runs (an odd NBatch, a short sequence) the table is written and the backward call ignores it.
 *   semicrf_logprob_bwd_t: semicrf_logprob_bwd_f with the table of the forward call of the SAME pairs (or NULL: exactly
 *     semicrf_logprob_bwd_f).  Launches that cannot use it -- short sequences, whose band is stored by the ring itself; the
 *     row-sequential implementation; more chains than one launch takes -- ignore it and scatter as before.
 * PRECONDITION for a non-NULL ptab, on top of 0 <= begin <= end < T: within a chain the pairs are sorted by begin, begins ascend
 * strictly and end_k <= begin_k+1 -- every frame begins at most one interval and every gap is covered at most once (what the
 * reference's targets are).  The device code does not check it; the host that packs the pairs does (transkun_amd asks its marshal
 * module) and passes NULL for any other path.  A table that breaks it gives wrong gradients, never an access outside dScore.
 * Adds nothing to the ABI's existing entry points (version 2).
 */
#define SEMICRF_PTAB_COVERED (1 << 30)
#define SEMICRF_PTAB_NONE ((1 << 30) - 1)
int semicrf_logprob_path_table_supported(int T, int B);
int semicrf_logprob_fwd_t(const float* score, const float* noise, int T, int B, const int32_t* pairs, int64_t K,
                          const int32_t* offsets, float* logProb, float* logZ, float* v, int32_t* ptab, void* ws, size_t ws_bytes,
                          semicrf_stream_t stream);
int semicrf_logprob_bwd_t(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                          int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets,
                          float* dScore, float* dNoise, int flags, const int32_t* ptab, void* ws, size_t ws_bytes,
                          semicrf_stream_t stream);

/*
 * Interval-score construction.  Replaces: ScaledInnerProductIntervalScorer.forward after the
 * Linear map (LayersTransformer.py:406-441).
 *   q,k: [C][T][D] with row strides ldq/ldk (in floats; >= D); diag: [C][T] with stride ldd between
 *   consecutive t (so the packed Linear output [C][T][2D+1] can be passed without a split copy).
 *   S[e,b,c] = (sum_d (q[c,e,d]*qscale) * k[c,b,d]) * len(|e-b|)  (+ diag[c,t] on e==b)
 *   S is [T][T][C] (chain axis contiguous, the CRF's layout).  full_square: 0 = e >= b is computed and the cells e < b
 *   are set to zero (S needs no initialisation by the caller); 1 = the full square, as the reference materialises it;
 *   2 = e >= b only, the rest of S is left untouched -- for callers that hand S to the sweeps of this library only, which
 *   never read e < b (tests/test_gpu_parity.py::test_upper_triangle_is_never_read): saves the 2 T^2 C bytes of zeros.
 *   | SEMICRF_SCORE_BF16X3: three-limb bf16 contraction (above); honoured where the LDS-tiled kernels run (16-byte
 *   aligned rows, D % 64 == 0), the exact fp32 contraction otherwise.
 *   noise_out [T-1][C] is zero-filled when non-NULL (:436-437).
 */
int interval_score_fwd(const float* q, const float* k, const float* diag, int C, int T, int D,
                       int64_t ldq, int64_t ldk, int64_t ldd, float qscale, int length_scaling,
                       int full_square, float* S, float* noise_out, semicrf_stream_t stream);

/*
 * Backward of interval_score_fwd.  Replaces: the autograd of LayersTransformer.py:410-433 (scale, einsum,
 * length scaling, diag_embed).  dS is [T][T][C] (the CRF's gradient layout; only e >= b is read: the counterpart of
 * interval_score_fwd with full_square == 0):
 *   dq[c,e,:] = qscale * sum_{b<=e} dS[e,b,c] len(e-b) k[c,b,:]
 *   dk[c,b,:] = qscale * sum_{e>=b} dS[e,b,c] len(e-b) q[c,e,:]
 *   ddiag[c,t] = dS[t,t,c]
 * dq/dk: [C][T][D] with row strides lddq/lddk; ddiag: [C][T] with stride lddd.  Any output may be NULL.
 * Requires D % 32 == 0 and D <= 256 (SEMICRF_EINVAL otherwise; the Python mirror then differentiates with torch).
 */
int interval_score_bwd(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                       int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                       int64_t lddq, int64_t lddk, int64_t lddd, semicrf_stream_t stream);

/*
 * The same with a workspace: the cotangent is first repacked into per-chain matrices (scaled, zero above the diagonal)
 * and dq/dk become two batched triangular GEMMs with LDS-shared operands (scorer_bwd_gemm.hip), about 1.7x faster at
 * T=1024, C=352, D=256.  interval_score_bwd_workspace_bytes returns 0 when the packed path does not apply (D not in
 * {64, 128, 256}, T < 64); with ws == NULL, too few bytes or q/k rows that are not 16-byte aligned the call runs
 * exactly interval_score_bwd.
 */
size_t interval_score_bwd_workspace_bytes(int C, int T, int D);
int interval_score_bwd_ws(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                          int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                          int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * SLOT LAYOUT of the chain axis (the *_p entry points): a private layout between this library's scorer and its CRF kernels.
 *
 * The model's chains come in groups of `group` symbols per segment (90: ModelTransformer.py:97); the CRF kernels stream the
 * score tensor in 32-chain pieces of 128 bytes, and a chain count that is not a multiple of 32 makes most pieces straddle two
 * lines (T=691: 90 / 360 chains run 22 - 32 % slower than 96 / 384).  With the slot layout every group owns `pitch` >= group
 * SLOTS of the chain axis: chain c = g * group + p lives in slot g * pitch + p; the slots p = group .. pitch-1 are ghosts.
 *   - S (and dS) is [T][T][Cs], Cs = (C / group) * pitch; the scorer multiplies only the C real chains and writes exact zeros
 *     into the ghost slots (cells e >= b; with full_square == 0 also the zeros above the diagonal);
 *   - the CRF entry points are called with B = Cs: a ghost slot is an ordinary chain of all-zero scores whose results the
 *     caller drops; noise, alpha, beta, logZ, gout and the interval offsets ([Cs + 1], ghost slots empty) are slot-indexed;
 *   - q, k, diag and their gradients stay chain-indexed ([C][T][..]).
 * group == pitch (== any divisor layout) is the plain contiguous layout; a padded pitch must be a multiple of 4 and needs the
 * LDS-tiled kernels (16-byte aligned rows, D % 64 == 0, T >= 128; backward: the workspace path) -- SEMICRF_EINVAL otherwise.
 * The reference has no counterpart: its scorer ends with permute(2,3,0,1).contiguous() (LayersTransformer.py:439) and the
 * glue flattens (N, P) (ModelTransformer.py:215-216); transkun_amd/fused.py and transcribe.py use the slot layout inside and
 * hand out chain-indexed results.
 */
int interval_score_fwd_p(const float* q, const float* k, const float* diag, int C, int T, int D,
                         int64_t ldq, int64_t ldk, int64_t ldd, float qscale, int length_scaling,
                         int full_square, int group, int pitch, float* S, float* noise_out, semicrf_stream_t stream);
int interval_score_bwd_ws_p(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                            int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk,
                            float* ddiag, int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes,
                            semicrf_stream_t stream);
int interval_score_bwd_fused_ws_p(const float* S, const float* alpha, const float* beta, const float* logZ,
                                  const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                  int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk,
                                  float* ddiag, int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes,
                                  semicrf_stream_t stream);
int interval_score_path_bwd_p(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                              const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale, int length_scaling,
                              int group, int pitch, float* dq, float* dk, float* ddiag, int64_t lddq, int64_t lddk,
                              int64_t lddd, semicrf_stream_t stream);

/*
 * MERGED PROJECTION (the *_pc entry points): the scorer with a per-(chain, end) constant inside the contraction,
 *   S[e,b,c] = qscale * ( <q[c,e,:], k[c,b,:]> + rowc[c,e] ) * len(|e-b|)  (+ diag[c,e] on e == b).
 * Why: the reference projects ctx twice, q = ctx Wq^T + bq and k = ctx Wk^T + bk (LayersTransformer.py:388-397, :406-410), and
 * contracts <q_e, k_b>.  Algebraically <q_e, k_b> = <ctx_e A + v, ctx_b> + c_e with A = Wq^T Wk (256 x 256), v = bq Wk,
 * c_e = <ctx_e, Wq^T bk> + <bq, bk>: ONE 256 -> 256 projection z = ctx A + v, the contraction's second operand is ctx ITSELF
 * (no k tensor), and c is a matrix-vector product -- half the Linear's flops forward and backward.  The result is fp32-grade
 * but NOT bit-identical to the reference's operation order (a reassociation; tests/test_gpu_parity.py::test_merged_projection
 * holds it to the scorer tolerance and the segment goldens to logProb 2e-5), so only this package's own fused route and
 * transcription step use it (transkun_amd/fused.py); ScaledInnerProductIntervalScorer.forward keeps the two projections.
 * rowc / drowc: [C][T] with stride ldrc / lddrc between consecutive frames, or NULL (then these are the *_p entry points).
 * drowc[c,e] = qscale * sum_{b<=e} dS[e,b,c] len(e-b) is WRITTEN by the bwd entry points (summed in a fixed order) and ADDED
 * to by interval_score_path_bwd_pc.  Needs the LDS-tiled kernels like the slot layout.
 */
int interval_score_fwd_pc(const float* q, const float* k, const float* diag, const float* rowc, int C, int T, int D,
                          int64_t ldq, int64_t ldk, int64_t ldd, int64_t ldrc, float qscale, int length_scaling,
                          int full_square, int group, int pitch, float* S, float* noise_out, semicrf_stream_t stream);
int interval_score_bwd_ws_pc(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                             int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk,
                             float* ddiag, float* drowc, int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc, void* ws,
                             size_t ws_bytes, semicrf_stream_t stream);
int interval_score_bwd_fused_ws_pc(const float* S, const float* alpha, const float* beta, const float* logZ,
                                   const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                   int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk,
                                   float* ddiag, float* drowc, int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc,
                                   void* ws, size_t ws_bytes, semicrf_stream_t stream);
int interval_score_path_bwd_pc(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                               const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale,
                               int length_scaling, int group, int pitch, float* dq, float* dk, float* ddiag, float* drowc,
                               int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc, semicrf_stream_t stream);

/*
 * The scorer's projection.  Replaces: the nn.Linear of ScaledInnerProductIntervalScorer (LayersTransformer.py:388-397: `self.map`,
 * applied at :406-410) and its autograd, as exact-fp32 matrix-core GEMMs of this library (csrc/proj_gemm.hip: an fp32 fmaf chain per
 * output, v_mfma_f32_32x32x2_f32) -- in the packed forms this package uses: y = [q | diag | 0 0 0] or [z | c | diag | 0 0], i.e. N
 * "main" columns (N in {64, 128, 256}) followed by two extra columns and zero padding.
 *
 *   scorer_proj_nn:  out[M][ldout] (+)= A[M][lda] (K columns used) * B[Kpad][ldb] (N columns)  (+ bias[N])
 *                    B is row-major with the contraction index as ROW and holds whole chunks of 32 rows, zero beyond K (Kpad =
 *                    K rounded up to 32: the caller pads; K % 4 == 0).  Forward: A = x, B = W[:N]^T.  Input gradient: A = dy (K =
 *                    the packed width), B = W (its N = the Linear's input size), accumulate = 1 adds to what out holds.
 *                    w2 != NULL (forward): two more output columns out[m][N + j] = <A[m], w2[j]> + b2[j] (w2 [2][K]), and
 *                    zero_cols columns of zeros behind them.
 *   scorer_proj_tn:  dW[total_rows][lddw] (N columns) = dy[M][lddy]^T x[M][ldx], db[total_rows] = column sums of dy: the R main
 *                    columns of dy through the matrix cores, the two columns extra_col0, extra_col0 + 1 (or -1: none) as dot
 *                    products on the side, rows / entries beyond them zero.  The contraction over M is cut into slices whose
 *                    partial results go through `ws` (scorer_proj_tn_workspace_bytes) and are summed in a fixed order.
 * Rows must be 16-byte aligned (pointers and leading dimensions), M * ld * 4 < 2^31.  SEMICRF_EINVAL for anything else (the
 * Python mirror then uses torch's GEMM).
 */
int scorer_proj_nn(const float* A, int64_t lda, int64_t M, int K, const float* B, int64_t ldb, int N, float* out, int64_t ldout,
                   const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, semicrf_stream_t stream);
/* scorer_proj_nn with the three-limb bf16 contraction (csrc/proj_gemm3.hip; opt-in, fp32-grade: |out - exact| <= 2^-21 sum_k |A[m][k] B[k][n]|
 * per element, not bit-identical): B is split once per call into `ws` (scorer_proj_nn3_workspace_bytes; 16-byte aligned), A in the loop.
 * N == 256 only; any other shape (or ws == NULL / too small) runs scorer_proj_nn's exact kernel.  The two extra columns are fp32 dot
 * products as before (in another fixed order). */
size_t scorer_proj_nn3_workspace_bytes(int K, int N);
int scorer_proj_nn3(const float* A, int64_t lda, int64_t M, int K, const float* B, int64_t ldb, int N, float* out, int64_t ldout,
                    const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, void* ws, size_t ws_bytes,
                    semicrf_stream_t stream);
/* scorer_proj_tn, total_rows | SEMICRF_PROJ_TN_BF16X3: the matrix part of the weight gradient on the three-limb bf16 kernel (N == 256;
 * fp32-grade, not bit-identical; the bias gradient and the two extra rows stay exact fp32 sums).  Other widths ignore the bit. */
#define SEMICRF_PROJ_TN_BF16X3 0x40000000
size_t scorer_proj_tn_workspace_bytes(int64_t M, int R, int N);
int scorer_proj_tn(const float* dy, int64_t lddy, int64_t M, int R, int extra_col0, int total_rows, const float* x, int64_t ldx, int N,
                   float* dW, int64_t lddw, float* db, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * The weights of the MERGED projection and their gradient.  Replaces: nothing the reference computes as such -- its two projections
 * q = x Wq^T + bq, k = x Wk^T + bk (LayersTransformer.py:392-397, applied at :406-410) enter the score only through
 * <q_e, k_b> = <x_e A + v, x_b> + c_e with A = Wq^T Wk, v = bq Wk, c_e = <x_e, Wq^T bk> + <bq, bk>, so ONE size -> size GEMM
 * [z | c | diag | 0 ..] = x Wm^T + bm does (transkun_amd.fused.merged_weights).  W [2 D + 1][size] and bias [2 D + 1] are the
 * Linear's parameters (rows Wq, Wk, the diagonal row); Wm [rows][size], bm [rows] with rows >= size + 2:
 *   Wm[i] = sum_r Wk1[r][i] Wq[r] (i <= size, Wk1 = [Wk | bk]),  Wm[size + 1] = the diagonal row,  zero rows behind;  bm alike.
 * _bwd: dW [2 D + 1][size], dbias [2 D + 1] from dWm, dbm (the autograd of the forward).  size <= 256, contiguous rows.
 */
int scorer_merge_weights_fwd(const float* W, const float* bias, int D, int size, int rows, float* Wm, float* bm, float* WmT,
                             semicrf_stream_t stream);    /* WmT (or NULL): [size][size], WmT[k][n] = Wm[n][k] for n < size -- scorer_proj_nn's B */
/* The Linear's parameters (W [2 D + 1][size], bias) in the layouts scorer_proj_nn reads, one launch: BT [size][2 D] (BT[k][n] = W[n][k] for
 * the q and k rows: B of the two forward products, ldb = 2 D), Wqd [rows_pad][size] = [Wq; diagonal row; zero rows] (B of the input
 * gradient through [q | diag | 0 ..]), w2 [2][size] = [diagonal row; 0], b2 [2] = [its bias, 0] (the forward's two extra columns). */
int scorer_stage_linear(const float* W, const float* bias, int D, int size, int rows_pad, float* BT, float* Wqd, float* w2, float* b2,
                        semicrf_stream_t stream);
size_t scorer_merge_weights_bwd_workspace_bytes(int size);           /* the transpose of dWm's first size + 1 rows */
int scorer_merge_weights_bwd(const float* W, const float* bias, const float* dWm, const float* dbm, int D, int size, int rows, float* dW,
                             float* dbias, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * Backward-direction values only (the beta half of forward_backward, NeuralSemiCRFInterval.py:386-414, without the
 * marginals): beta[t][c] by frame, natural log.  Workspace: semicrf_workspace_bytes(SEMICRF_OP_LOGZ_FWD, T, B).
 * Used by interval_score_bwd_fused, which rebuilds the marginals tile by tile instead of reading a dense gradient.
 */
int semicrf_beta(const float* score, const float* noise, int T, int B, float* beta, void* ws, size_t ws_bytes,
                 semicrf_stream_t stream);

/*
 * Loss gradient fused into the scorer backward: interval_score_bwd with the cotangent
 *   dS[e,b,c] = gout[c] * marginal[e,b,c]      (marginal as in NeuralSemiCRFInterval.py:424-440, e >= b)
 * built on the fly from S (= score [T][T][C]), alpha (= v of semicrf_logz_fwd), beta (semicrf_beta) and logZ --
 * the dense [T][T][C] gradient of ComputeLogZFasterGrad.backward (:469-472) is never written or read.
 * Outputs as interval_score_bwd.  The evalPath part of logProb's gradient (one-hot on the path cells) is sparse and
 * is added by the caller (transkun_amd/fused.py).
 */
int interval_score_bwd_fused(const float* S, const float* alpha, const float* beta, const float* logZ,
                             const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                             int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                             int64_t lddq, int64_t lddk, int64_t lddd, semicrf_stream_t stream);

/*
 * The evalPath half of logProb's gradient (one-hot on the path cells, NeuralSemiCRFInterval.py:540-548) pushed through
 * the scorer, ADDED to dq/dk/ddiag: for every interval (b, e) of chain c (pairs/offsets as in semicrf_eval_path)
 *   dq[c,e,:] += w k[c,b,:],  dk[c,b,:] += w q[c,e,:],  w = gout[c] qscale len(e-b);  ddiag[c,e] += gout[c] if b == e.
 * Completes interval_score_bwd_fused[_ws] to the gradient of logProb = evalPath - logZ.
 */
int interval_score_path_bwd(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                            const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale, int length_scaling,
                            float* dq, float* dk, float* ddiag, int64_t lddq, int64_t lddk, int64_t lddd,
                            semicrf_stream_t stream);

/*
 * interval_score_bwd_fused on the packed path (workspace as interval_score_bwd_ws): the repack kernel evaluates the
 * marginals while it builds the per-chain matrices, the two GEMMs are the same.  Falls back to
 * interval_score_bwd_fused exactly like interval_score_bwd_ws falls back to interval_score_bwd.
 */
int interval_score_bwd_fused_ws(const float* S, const float* alpha, const float* beta, const float* logZ,
                                const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                                int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes,
                                semicrf_stream_t stream);

/*
 * Interval features for the attribute heads.  Replaces: TransKun.fetchIntervalFeaturesBatch
 * (ModelTransformer.py:501-532) and the concatenation that feeds the velocity / onset-offset predictors (:578-582),
 * consuming the packed decode output on the device (pairs [K][2], offsets [C+1] as written by semicrf_viterbi; chain
 * c = segment * nSym + symbol) instead of Python lists:
 *   out[i] = [ ctx[c,begin,:] | ctx[c,end,:] | ctx[c,begin,:] * ctx[c,end,:] ]   ([K][3D]; ctx is [C][T][D], row stride ldc)
 *   symIdx[i] = c % nSym, scatterIdx[i] = c                                       (int64; either may be NULL)
 * The backward ADDS into dctx ([C][T][D], row stride lddc; zero it first for a fresh gradient).
 */
int interval_features_gather(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K,
                             const int32_t* offsets, int nSym, float* out, int64_t* symIdx, int64_t* scatterIdx,
                             semicrf_stream_t stream);
int interval_features_gather_bwd(const float* gout, const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs,
                                 int64_t K, const int32_t* offsets, float* dctx, int64_t lddc, semicrf_stream_t stream);

/*
 * Attribute-head training loss.  Replaces: the part of TransKun.log_prob behind the two heads (ModelTransformer.py:284-328) --
 * the velocity log_softmax + gather, ContinuousBernoulli(logits).log_prob of the refined onset/offset, Bernoulli(logits).log_prob
 * of their presence and the scatter_add into the per-chain logProb -- on the heads' raw outputs.  Rows are the K target intervals
 * in chain order (offsets [C+1]); per row: logitsVelocity [K][128], ofLogits [K][4] (columns 0-1 the value logits, 2-3 the
 * presence logits), velocity int32 [K] in 0..127 (anything else gives NaN, never an access out of bounds), ofRefined [K][2] in
 * [-0.5, 0.5] (shifted to x = r * 0.99 + 0.5 in fp32 here), ofPresence [K][2] in {0, 1}:
 *   lpVel  = logitsVelocity[v] - logsumexp(logitsVelocity)
 *   lpOF   = sum_j x_j l_j - softplus(l_j) + logC(l_j)
 *   lpPres = sum_j p_j l'_j - softplus(l'_j)
 *   rowLogProb[i] = (lpVel + lpOF) + lpPres;   out[c] = (rows of chain c summed in ascending order, fp32) + base[c]
 * logC is torch's ContinuousBernoulli log-normaliser INCLUDING its fp32 probability clamp: log(l / tanh(l / 2)) for
 * |l| < log((1 - 2^-23) / 2^-23) = 15.942..., that value's constant beyond (derivative 0), log 2 at 0 -- evaluated from the logit
 * without the cancellation of torch's probability-space formula (csrc/attr_loss_math.h).
 * No atomics: out[c] depends on the rows of chain c only and is bit-identical from run to run.  base (or NULL: zeros) is the
 * CRF term; out may not alias rowLogProb.  K == 0 launches nothing and leaves out untouched (the result is base itself).
 * Backward, for the upstream gradient g[c] = gout[c * gstride] (gstride 0: one value for every chain, as -logp.sum(-1).mean() gives):
 *   dLogitsVelocity [K][128] = g (onehot(v) - softmax),  dOfLogits [K][4] = g (x_j - sigmoid(l_j) + logC'(l_j)) | g (p_j - sigmoid(l'_j))
 * (d out / d base = 1 is the caller's).  Both calls only enqueue kernels on `stream`: no synchronisation, allocation or workspace.
 * Alignment: logitsVelocity and dLogitsVelocity must be 8-byte aligned (a lane reads / writes two classes at once); anything else is
 * SEMICRF_EINVAL and nothing is launched.  Every other buffer takes any 4-byte aligned base.  Written: rowLogProb[0:K] and
 * out[0:C]; dLogitsVelocity[0:128 K] and dOfLogits[0:4 K]; nothing else (tests/test_step_contract.py).
 */
int semicrf_attribute_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int32_t* velocity, const float* ofRefined,
                               const float* ofPresence, int64_t K, const int32_t* offsets, int C, const float* base, float* rowLogProb,
                               float* out, semicrf_stream_t stream);
int semicrf_attribute_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int32_t* velocity,
                               const float* ofRefined, const float* ofPresence, int64_t K, const int32_t* offsets, int C,
                               float* dLogitsVelocity, float* dOfLogits, semicrf_stream_t stream);

/*
 * Attribute-head readout of transcription.  Replaces: the torch lines behind the two heads in TransKun.transcribeFrames
 * (ModelTransformer.py:590-651) -- softmax and the velocity criterion, ContinuousBernoulli(logits).mean shifted back and clamped,
 * the sign of the presence logits -- on the heads' raw outputs, row-wise (no offsets: the per-chain part stays segment_events).
 * Per row i of K: logitsVelocity [K][128], ofLogits [K][4] (columns 0-1 the value logits, 2-3 the presence logits), p = softmax:
 *   SEMICRF_VEL_HAMMING  velocityClass[i] = the smallest index of the largest logit (= argmax p, exactly)
 *   SEMICRF_VEL_MSE      velocityMean[i]  = sum_w p[w] w
 *   SEMICRF_VEL_MATCH    velocityClass[i] = the smallest v with the largest r[v] = sum of p[w] over |w - v| <= 12 (each r[v] summed
 *                        directly in ascending w: a row with one dominant logit at m gives max(0, m - 12) every time)
 *   SEMICRF_VEL_MAE      velocityClass[i] = the smallest v with p[0] + ... + p[v] > 0.5
 *   ofValue[i][j]    = clamp((mean(l_j) - 0.5) / 0.99, -0.5, 0.5), mean = the ContinuousBernoulli mean INCLUDING torch's fp32
 *                      probability clamp: mean - 0.5 = sign(l) h(min(|l|, l*)), h(a) = 0.5 coth(a / 2) - 1 / a, l* = 15.942...
 *                      (beyond it the constant 0.4416912), evaluated from the logit without the cancellation of torch's
 *                      probability-space formula (csrc/attr_decode_math.h); NaN gives NaN
 *   ofPresence[i][j] = l'_j > 0 (bytes 0 / 1; NaN gives 0)
 * A row whose softmax is not finite (a NaN, a +inf, or all -inf) gives class 0 (torch.argmax of an all-NaN row) and mean NaN.
 * velocityClass (int64 [K]) is required for the three class criteria, velocityMean (float [K]) for SEMICRF_VEL_MSE; the other may be
 * NULL and is not written.  ofValue: float [K][2], ofPresence: bytes [K][2].  SEMICRF_EINVAL for an unknown criterion or a missing
 * output; K == 0 launches nothing.  One launch on `stream`: no synchronisation, allocation, workspace or atomics; a row's result
 * depends on that row alone and is bit-identical from run to run.
 * Alignment: logitsVelocity must be 8-byte aligned (a lane reads two classes at once) and velocityClass is an int64 array, 8-byte
 * aligned as such; a logitsVelocity that is not is SEMICRF_EINVAL and nothing is launched.  ofLogits, velocityMean and ofValue take
 * any 4-byte aligned base, ofPresence any address.  Written: K elements of the criterion's velocity output, ofValue[0:2 K] and
 * exactly 2 K bytes of ofPresence; nothing else (tests/test_step_contract.py).
 */
#define SEMICRF_VEL_HAMMING 0
#define SEMICRF_VEL_MSE 1
#define SEMICRF_VEL_MATCH 2
#define SEMICRF_VEL_MAE 3
int semicrf_attribute_decode(const float* logitsVelocity, const float* ofLogits, int64_t K, int criterion, int64_t* velocityClass,
                             float* velocityMean, float* ofValue, unsigned char* ofPresence, semicrf_stream_t stream);

/*
 * The two attribute heads of transcription, from the packed decode output to their raw outputs (inference only).  Replaces: the
 * gather interval_features_gather, the materialised [K][3D] input and the two nn.Sequential heads (Linear, GELU, Dropout, Linear) of
 * TransKun.transcribeFrames (ModelTransformer.py:578-590, :638; the modules of :112-128) in eval mode.  For interval i of chain c
 * (found from offsets as the gather does), (b, e) = pairs[i]:
 *   x_i               = [ ctx[c][b][:] | ctx[c][e][:] | ctx[c][b][:] * ctx[c][e][:] ]    (3 D values, never written to memory)
 *   logitsVelocity[i] = W2v gelu(W1v x_i + b1v) + b2v        [Nv]
 *   ofLogits[i]       = W2o gelu(W1o x_i + b1o) + b2o        [No]
 * gelu is the exact erf form (csrc/attr_heads_math.h).  ctx: [C][T] rows of ldc >= D floats.  The weights are PACKED, fp32, dense:
 *   W1 [3D][Hv + Ho]   column j < Hv: row j of the velocity head's first Linear weight; column Hv + j: the onset/offset head's
 *   b1 [Hv + Ho]       the two first biases, in the same order
 *   W2 [Hv][Nv] followed by [Ho][No]: the second Linear weights, TRANSPOSED (hidden-major)
 *   b2 [Nv + No]
 * Exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32).  Every output element is ONE fixed chain of operations: the contraction
 * over k = 0 .. 3D-1 ascending, + b1, gelu; per slice of SEMICRF_HEADS_SLICE hidden columns of its head the contraction over the
 * slice's columns ascending; the slices' partial sums added in ascending order, b2 last.  No atomics: a row's outputs are
 * bit-identical whatever K is, wherever the row sits and whatever the other rows hold.  pairs outside [0, T-1] are clamped into it.
 * symIdx[i] = c % nSym and scatterIdx[i] = c (int64 [K]) as the gather writes them; either may be NULL.
 * Workspace: semicrf_attribute_heads_workspace_bytes(K, Hv, Ho, Nv, No), the slices' partial sums (about K * (Nv * ceil(Hv / 64) +
 * No * ceil(Ho / 64)) floats); semicrf_workspace_bytes(SEMICRF_OP_ATTRIBUTE_HEADS, K, Hv + Ho) is an upper bound of it for heads of at
 * most 128 outputs each.  Two launches on `stream` (the tiles; the sum over slices), none for K == 0; no synchronisation or allocation.
 * SEMICRF_EINVAL: a NULL pointer, a size below 1, K < 0, ldc < D; SEMICRF_EWORKSPACE: a workspace that is too small.
 */
#define SEMICRF_HEADS_ROW_TILE 64
#define SEMICRF_HEADS_SLICE 64
size_t semicrf_attribute_heads_workspace_bytes(int64_t K, int Hv, int Ho, int Nv, int No);
int semicrf_attribute_heads(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets,
                            int nSym, const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                            float* logitsVelocity, float* ofLogits, int64_t* symIdx, int64_t* scatterIdx, void* ws, size_t ws_bytes,
                            semicrf_stream_t stream);

/*
 * The attribute heads in TRAINING: the forward with dropout, and the backward of the gather + both heads.  Replaces: the gather, the
 * [K][3D] input and the two nn.Sequential forwards of TransKun.log_prob (ModelTransformer.py:275-281, :290, :306) with their autograd
 * (per Linear two GEMMs, the GELU and dropout backwards, cat / mul backwards and the gather's atomic scatter).  Arguments and packed
 * weights as semicrf_attribute_heads.
 *
 * semicrf_attribute_heads_train_fwd: the arithmetic of semicrf_attribute_heads (the same kernel) with, per row i and packed hidden
 *   column j (0 .. Hv + Ho - 1; the velocity head's columns first),
 *     z[i][j] = (W1 x_i)[j] + b1[j]                       saved to `z` [K][Hv + Ho] for the backward
 *     A[i][j] = keep(seed, i, j) ? gelu(z[i][j]) * scale_head : 0          scale_head = (float)(1 / (1 - p_head))
 *   in gelu's place in layer 2.  A head with p = 0 (pv, po: the heads' dropout probabilities, 0 <= p < 1; pass 0 for a head in eval
 *   mode) is neither masked nor scaled: with pv = po = 0 the outputs are bit-identical to semicrf_attribute_heads'.  Workspace as
 *   semicrf_attribute_heads (semicrf_attribute_heads_train_fwd_workspace_bytes is the same number).
 *
 * The mask is a stateless function of (seed, i, j): Philox-4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as
 *   1, 2, 3", SC 2011; multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds) with
 *     counter = (i >> 2, j, 0, 0) and key = (seed & 0xffffffff, seed >> 32);
 *   element (i, j) takes output word i & 3 and is kept iff word >= floor(p_head * 2^32) (as an unsigned 32-bit number).  i is the
 *   GLOBAL row index, so a row's outputs are bit-identical whatever K is and whatever the other rows hold, in training too.
 *   semicrf_attribute_heads_dropout_mask writes it as bytes (1 = kept) [K][Hv + Ho]; a head with p = 0 is all ones.
 *
 * semicrf_attribute_heads_bwd: given dLogitsVelocity [K][Nv], dOfLogits [K][No] and the forward's z, seed, pv, po; per head, with
 *   M = keep / (1 - p) (1 where p = 0), every contraction a fmaf chain from +0 in the stated order:
 *     dA[i][j]  = sum over n ascending of dOut[i][n] W2[j][n];   dz[i][j] = (dA[i][j] * M) * gelu'(z[i][j])
 *                 gelu'(z) = Phi(z) + z phi(z), the exact erf form (csrc/attr_heads_math.h)
 *     dW2[j][n] = sum_i A[i][j] dOut[i][n]     (A recomputed from z and the mask)         db2[n] = sum_i dOut[i][n]
 *     dW1[k][j] = sum_i x_i[k] dz[i][j]        (x gathered again; matrix pipe)             db1[j] = sum_i dz[i][j]
 *     dx[i][k]  = sum over j ascending of dz[i][j] W1[k][j]      (matrix pipe; never stored)
 *     ga_i = fmaf(dx_ab, ctx[c][e], dx_a),  gb_i = fmaf(dx_ab, ctx[c][b], dx_b)            (the three thirds of dx_i)
 *     dctx[c][b][:] += ga_i, then dctx[c][e][:] += gb_i, rows i in ascending order, on dctx zeroed by the call
 *   Sums over rows: per chunk of SEMICRF_HEADS_BWD_ROW_CHUNK rows one partial (rows ascending; the two bias gradients as 8 sums over
 *   the rows r = q (mod 8) of the chunk added in ascending q, in double, rounded to fp32 once per chunk), the chunks' partials added in ascending order.  No atomics: one wave
 *   per chain (and 256 columns) walks the chain's rows offsets[c] .. offsets[c+1] (the last chain: to K), so every result is
 *   bit-identical from run to run.  Outputs: dctx [C][T][D] dense, dW1 [3D][Hv + Ho], db1 [Hv + Ho], dW2 and db2 in the layout of W2
 *   and b2.  Workspace: semicrf_attribute_heads_bwd_workspace_bytes(K, D, Hv, Ho, Nv, No): dz [K][Hv + Ho], (ga, gb) [K][2][D], the
 *   rows' frames, and ceil(K / chunk) planes of all parameter gradients; semicrf_workspace_bytes(SEMICRF_OP_ATTRIBUTE_HEADS_BWD, K,
 *   Hv + Ho) is an upper bound of it for 3 D <= Hv + Ho and heads of at most 128 outputs each.
 *
 * All three: launches on `stream` only (the backward also one hipMemsetAsync of dctx), no synchronisation, no allocation; K == 0
 * launches nothing and writes nothing.  SEMICRF_EINVAL: a NULL pointer, a size below 1, K < 0, ldc < D, p outside [0, 1), more than
 * 65535 row chunks; SEMICRF_EWORKSPACE: a workspace that is too small.  The seed is a host value: a captured call replays ONE mask.
 */
#define SEMICRF_HEADS_BWD_ROW_CHUNK 512
size_t semicrf_attribute_heads_train_fwd_workspace_bytes(int64_t K, int Hv, int Ho, int Nv, int No);
int semicrf_attribute_heads_train_fwd(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K,
                                      const int32_t* offsets, int nSym, const float* W1, const float* b1, const float* W2, const float* b2,
                                      int Hv, int Ho, int Nv, int No, uint64_t seed, double pv, double po, float* logitsVelocity,
                                      float* ofLogits, float* z, int64_t* symIdx, int64_t* scatterIdx, void* ws, size_t ws_bytes,
                                      semicrf_stream_t stream);
size_t semicrf_attribute_heads_bwd_workspace_bytes(int64_t K, int D, int Hv, int Ho, int Nv, int No);
int semicrf_attribute_heads_bwd(const float* dLogitsVelocity, const float* dOfLogits, const float* z, const float* ctx, int C, int T, int D,
                                int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* W1, const float* W2,
                                int Hv, int Ho, int Nv, int No, uint64_t seed, double pv, double po, float* dctx, float* dW1, float* db1,
                                float* dW2, float* db2, void* ws, size_t ws_bytes, semicrf_stream_t stream);
int semicrf_attribute_heads_dropout_mask(uint64_t seed, int64_t K, int Hv, int Ho, double pv, double po, unsigned char* mask,
                                         semicrf_stream_t stream);

/*
 * Transcription segment loop, on the packed decode output in HBM.
 *
 * segment_onset_filter.  Replaces: the onsetBound filter of TransKun.transcribeFrames (ModelTransformer.py:554-555),
 *   `path = [[e for e in _ if e[0] < onsetBound] for _ in path]`: pairs/offsets (as written by semicrf_viterbi) ->
 *   pairs_out [cap][2] / offsets_out [B+1]; counts_ws: B ints of scratch.  offsets_out[B] is exact even if it exceeds cap.
 *
 * segment_events.  Replaces: the per-interval event assembly of transcribeFrames (:672-718) and the hand-off of
 *   TransKun.transcribe (:789-800), for chains c = segment * nSym + symbol in list order:
 *     start = (begin + ofValue[i][0]) * frameDur, end = (end + ofValue[i][1]) * frameDur   (double, the reference's order)
 *     hasOnset = begin > 0 || ofPresence[i][0];  hasOffset = end < lastFrameIdx || ofPresence[i][1]
 *     start = max(start, lastEnd); end = max(end, start + 1e-8); lastEnd = end            (per chain)
 *     times[i] = the two shifted by beginTime[segment], clamped (start >= 0, end >= start);  flags[i] = {hasOnset, hasOffset}
 *     lastP[c] = end frame of the chain's last interval with hasOffset (0 if none);  nextStart[c] = max(lastP[c] - stepFrames, 0)
 *   ofValue: float [K][2] (already (mean - 0.5) / 0.99 clamped, :650-653), ofPresence: bytes [K][2] (logit > 0, :655),
 *   beginTime: double [B / nSym].  nextStart is what the next semicrf_viterbi takes as `start`.
 */
int segment_onset_filter(const int32_t* pairs, const int32_t* offsets, int B, int bound, int32_t* pairs_out, int64_t cap,
                         int32_t* offsets_out, int32_t* counts_ws, semicrf_stream_t stream);
int segment_events(const int32_t* pairs, int64_t K, const int32_t* offsets, int B, int nSym, const float* ofValue,
                   const unsigned char* ofPresence, int lastFrameIdx, double frameDur, const double* beginTime, int stepFrames,
                   double* times, unsigned char* flags, int32_t* lastP, int32_t* nextStart, semicrf_stream_t stream);

/*
 * The optimizer step on flat fp32 buffers.  Replaces: train.py:239-246 -- the clip value as a quantile of the past gradient norms
 * (TrainUtil.py:12-25, a host deque), clip_grad_norm_, the host read of the norm, and torch_optimizer.AdaBelief(weight_decouple=True,
 * rectify=True) looping over every parameter -- by three launches and no host synchronisation.  csrc/optim_math.h holds the arithmetic.
 *
 * semicrf_grad_sqnorm.  partials[i] = the sum of squares of workgroup i's share of flat[0:numel], squares and sums in double (1e30 does
 *   not overflow).  The number of partials and every order of addition depend on numel (and the alignment of flat) only: no atomics,
 *   the same bits every run.  partials: SEMICRF_SQNORM_MAX_PARTIALS doubles (8-byte aligned), of which the first
 *   min(max(ceil(numel / 32768), 1), SEMICRF_SQNORM_MAX_PARTIALS) are written; the ones past that count are not written (and not read
 *   by semicrf_clip_from_history).  flat is read only, at any 4-byte aligned base; nothing behind flat[numel] is read.
 *
 * semicrf_clip_from_history (one workgroup).  The adaptive clip value and the norm history, MovingBuffer(initValue, maxLen) on the device:
 *   ring [capacity] fp32 (capacity <= SEMICRF_HISTORY_MAX), state = {count, head} (int32; a fresh history is ring[0] = 40, state = {1, 0}).
 *     norm  = fp32(sqrt(partials summed in index order, double))   when partials != NULL (numel: what semicrf_grad_sqnorm was given),
 *             *norm_in                                             when partials == NULL and norm_in != NULL, else there is no norm
 *     clip  = the q-quantile of the count values in the ring BEFORE this call: np.quantile's linear interpolation at q (count - 1),
 *             in double, rounded to fp32; NaN if the ring holds a NaN; skipped when q < 0
 *     coef  = min(1, clip / (norm + 1e-6)) in fp32 (clip_grad_norm_); NaN if either is NaN -- a non-finite norm propagates
 *     stats = {norm, clip, coef}; an entry that was not computed is left alone
 *     append != 0 (and there is a norm): the norm goes into the ring, replacing the oldest value once count == capacity
 *
 * semicrf_adabelief_step.  The update of optim_math.h over p, g, m, s [numel]; g is read only.  groups: up to SEMICRF_OPTIM_MAX_GROUPS
 *   contiguous element ranges [g[i-1].end, g[i].end) with g[n-1].end == numel, each with its own factors, passed by value; ranges may
 *   begin anywhere: an access of four elements that crosses a boundary gives each element its own group's factors.  coef: a device
 *   fp32 (stats + 2 above) or NULL for 1.  16-byte accesses when the four buffers are 16-byte aligned, 4-byte accesses otherwise.
 */
#define SEMICRF_OPTIM_MAX_GROUPS 8
#define SEMICRF_SQNORM_MAX_PARTIALS 256
#define SEMICRF_HISTORY_MAX 16384
typedef struct semicrf_adabelief_group {
    int64_t end;       /* one past the group's last element */
    float decay;       /* 1 - lr*wd */
    float b1, omb1;    /* beta1, 1 - beta1 */
    float b2, omb2;    /* beta2, 1 - beta2 */
    float eps;
    float sqrt_bc2;    /* sqrt(1 - beta2^t) */
    float step;        /* rectified: rt*lr/(1 - beta1^t); otherwise lr */
    int32_t rectified; /* rho_t > 4 */
    int32_t pad_;
} semicrf_adabelief_group;
typedef struct semicrf_adabelief_groups {
    int32_t n;
    int32_t pad_;
    semicrf_adabelief_group g[SEMICRF_OPTIM_MAX_GROUPS];
} semicrf_adabelief_groups;

int semicrf_grad_sqnorm(const float* flat, int64_t numel, double* partials, semicrf_stream_t stream);
int semicrf_clip_from_history(const double* partials, int64_t numel, const float* norm_in, double q, float* ring, int capacity,
                              int32_t* state, int append, float* stats, semicrf_stream_t stream);
int semicrf_adabelief_step(float* p, const float* g, float* m, float* s, int64_t numel, const float* coef,
                           semicrf_adabelief_groups groups, semicrf_stream_t stream);

/*
 * The attention of the backbone's transformer layers for many short, independent sequences (forward only).  Replaces: the head
 * split `unflatten / transpose`, F.scaled_dot_product_attention and the merge `transpose / flatten` of MultiHeadAttentionKernel.forward
 * with kernel = None (LayersTransformer.py:173-186), and with them the transposed copies of BasicBlock's time-axis half (:327-337).
 * For every sequence s = (s0, s1), s0 < n0, s1 < n1, head h < H, query i < Lq:
 *   out[s][i][h][:] = sum over j < Lk of softmax_j(q[s][i][h][:] . k[s][j][h][:] / sqrt(d)) v[s][j][h][:]
 * fp32, no mask, no dropout, no bias.  The layout is TOKEN-MAJOR: a token's H d values are contiguous, head h the slice
 * [h d, (h + 1) d).  Each of q, k, v, out has its own three ELEMENT strides: token (s0, s1, l) starts at
 * base + s0 stride_s0 + s1 stride_s1 + l stride_l.  One [N][T'][F'][H d] buffer serves the frequency axis as n0 = N, n1 = T', L = F'
 * (strides T' F' H d, F' H d, H d) and the time axis as n0 = N, n1 = F', L = T' (strides T' F' H d, H d, F' H d): no transposed copy.
 * q has Lq tokens per sequence, k and v have Lk (cross attention: Lq != Lk).  Strides are >= 0; a 0 repeats a tensor over that dimension
 * (not for out); a token stride stays below 2^28 elements.  All offsets are 64-bit.
 *
 * Supported (semicrf_axial_attention_supported returns 1): 1 <= Lq, Lk <= SEMICRF_ATTENTION_MAX_L; d a multiple of 8 in
 * [8, SEMICRF_ATTENTION_MAX_D]; H >= 1.  n0 n1 H < 2^31 (2^20 sequences and more).  n0 n1 == 0 launches nothing.
 *
 * Exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32), one fixed chain of operations per output element (csrc/attention_math.h):
 * q . k a fmaf chain over the head dimension ascending from +0, times (float)(1 / sqrt(d)); the maximum over the keys j < Lk; exp of
 * the difference; the sum of the exponentials as S0 + S1, S_b over the keys with ((j >> 2) & 1) == b ascending; P V a fmaf chain over
 * the keys ascending from +0; one division by the sum.  Keys from Lk to the tile edge are masked before the maximum and contribute
 * exact zeros; K and V rows past Lk and query rows past Lq are never read (zeros are formed in registers), rows past Lq never stored;
 * the head dimension is padded with zeros in LDS and registers only.  No atomics; tile sizes depend on Lk and d alone: a sequence's
 * result is bit-identical from run to run, whatever n0, n1, its position in the batch and the strides are.
 * One launch on `stream`; no workspace, no synchronisation, no allocation.  16-byte loads of the Q and K rows when q, k are 16-byte
 * aligned and their strides multiples of 4, 4-byte loads otherwise (the same numbers).
 * SEMICRF_EINVAL, with nothing launched and `out` untouched: a shape outside the supported set, a NULL or misaligned pointer, a
 * negative count or stride, n0 n1 H >= 2^31.
 */
#define SEMICRF_ATTENTION_MAX_L 256
#define SEMICRF_ATTENTION_MAX_D 64
int semicrf_axial_attention_supported(int Lq, int Lk, int H, int d);
int semicrf_axial_attention(const float* q, const float* k, const float* v, float* out, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d,
                            int64_t q_stride_s0, int64_t q_stride_s1, int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1,
                            int64_t k_stride_l, int64_t v_stride_s0, int64_t v_stride_s1, int64_t v_stride_l, int64_t out_stride_s0,
                            int64_t out_stride_s1, int64_t out_stride_l, semicrf_stream_t stream);

/*
 * The backward of semicrf_axial_attention: dq, dk, dv from q, k, v, `out` AS THE FORWARD WROTE IT and the cotangent dout.  Per sequence
 * and head, scale = (float)(1 / sqrt(d)), sc, m, p and sum recomputed with the forward's own chain (the forward saves nothing):
 *   P[i][j] = p[i][j] / sum_i     D_i = dout_i . out_i     dP[i][j] = dout_i . v_j     dS[i][j] = P[i][j] (dP[i][j] - D_i)
 *   dv_j = sum_i P[i][j] dout_i   dq_i = scale sum_j dS[i][j] k_j                      dk_j = scale sum_i dS[i][j] q_i
 * Layout and strides as in the forward, three ELEMENT strides for each of the eight tensors (q, dout, out, dq: Lq tokens; k, v, dk, dv:
 * Lk tokens).  Strides of q, k, v are >= 0 (0 repeats); out, dout, dq, dk, dv are real, non-overlapping tensors.  A token stride stays
 * below 2^28 elements; all offsets are 64-bit.  Any of dq, dk, dv may be NULL: nothing is computed or written for it.
 *
 * Supported (semicrf_axial_attention_bwd_supported returns 1): exactly the forward's set -- 1 <= Lq, Lk <= SEMICRF_ATTENTION_MAX_L; d a
 * multiple of 8 in [8, SEMICRF_ATTENTION_MAX_D]; H >= 1.  n0 n1 H < 2^31.  n0 n1 == 0 launches nothing.
 *
 * Exact fp32 on the matrix pipe, one fixed chain per gradient element (csrc/attention_math.h): D_i and dP fmaf chains over the head
 * dimension ascending from +0; P = p / sum (a division); dS = P * (dP - D_i); dq_i, dk_j, dv_j fmaf chains from +0 over the keys
 * (queries) in the order bwd_order -- blocks of 32 ascending, inside a block 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, .. -- then one
 * multiplication by scale for dq and dk.  Rows past Lq / Lk are never read or written, padded keys are masked before the maximum, the
 * head dimension is padded with zeros in registers only.  One workgroup per (sequence, head) forms all of its dk and dv: no atomics,
 * and a sequence's gradients are bit-identical from run to run, whatever n0, n1, its position in the batch and the strides are.
 * One launch on `stream`; no workspace, no synchronisation, no allocation.
 * SEMICRF_EINVAL, with nothing launched and dq / dk / dv untouched: a shape outside the supported set, a NULL q / k / v / out / dout, a
 * misaligned pointer, a negative count or stride, a token stride >= 2^28, n0 n1 H >= 2^31.
 */
int semicrf_axial_attention_bwd_supported(int Lq, int Lk, int H, int d);
int semicrf_axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk,
                                float* dv, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, int64_t q_stride_s0, int64_t q_stride_s1,
                                int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0,
                                int64_t v_stride_s1, int64_t v_stride_l, int64_t out_stride_s0, int64_t out_stride_s1, int64_t out_stride_l,
                                int64_t dout_stride_s0, int64_t dout_stride_s1, int64_t dout_stride_l, int64_t dq_stride_s0,
                                int64_t dq_stride_s1, int64_t dq_stride_l, int64_t dk_stride_s0, int64_t dk_stride_s1, int64_t dk_stride_l,
                                int64_t dv_stride_s0, int64_t dv_stride_s1, int64_t dv_stride_l, semicrf_stream_t stream);

/*
 * semicrf_axial_attention for bfloat16 tensors (forward only): the same sequences, heads, layout and strides, every element of q, k,
 * v and out one bf16 value (uint16_t: the upper half of the fp32 bit pattern).  TOKEN-MAJOR, head h the slice [h d, (h + 1) d); three
 * ELEMENT strides per tensor (s0, s1, token), so both axes of one [N][T'][F'][H d] buffer are served without a copy; strides are >= 0,
 * a 0 repeats a tensor over that dimension (not for out); Lq != Lk is allowed; a token stride stays below 2^28 elements.  All offsets
 * are 64-bit.
 *
 * Supported (semicrf_axial_attention_bf16_supported returns 1): the fp32 op's set -- 1 <= Lq, Lk <= SEMICRF_ATTENTION_MAX_L; d a
 * multiple of 8 in [8, SEMICRF_ATTENTION_MAX_D]; H >= 1.  n0 n1 H < 2^31.  n0 n1 == 0 launches nothing.
 *
 * The chain (csrc/attention_bf16_math.h), per sequence, head and query i:
 *   s_j    = (sum over c of q_ic k_jc) * (float)(1 / sqrt(d))   products of bf16 values are exact in fp32; fp32 accumulation
 *   m      = max over j < Lk of s_j                             keys from Lk to the tile edge are masked to -inf before the maximum
 *   p_j    = expf(s_j - m)                                      fp32
 *   ph_j   = bf16_rne(p_j)                                      the weight the second product consumes
 *   sum    = sum over j of (float)ph_j                          fp32, of the ROUNDED weights, in one fixed order: the keys of a
 *                                                               32-key block whose ((j >> 2) & 1) is 0 ascending, block after block,
 *                                                               then those whose bit is 1, then the two partial sums added
 *   o_c    = sum over j of ph_j v_jc                            fp32 accumulation
 *   out_ic = bf16_rne(o_c / sum)                                one correctly rounded fp32 division, one rounding to bf16
 * so the weights that enter P V sum to `sum`, and a V that is constant over the keys comes back exactly.  NaN and inf propagate to the
 * outputs they belong to (a non-finite q row: that query; a non-finite k row: every query of that sequence and head; a non-finite v
 * element: its column of that sequence and head) and to no other output.
 * On the device both products run on v_mfma_f32_32x32x16_bf16; the head dimension is padded with zeros to a multiple of 16 and the
 * keys to a multiple of 32, in registers and LDS only.  Rows past Lq, rows past Lk and columns behind d are never read, rows past Lq
 * never stored.  No atomics, no workspace, one launch on `stream`; tile sizes depend on Lk and d alone: a sequence's result is
 * bit-identical from run to run, whatever n0, n1, its position in the batch, the strides and the alignment are.
 * The device and the host mirror (the CPU key of torch.ops.semicrf.axial_attention_bf16) are NOT bit-identical to each other: the
 * matrix instruction's internal summation is not the mirror's ascending fp32 chain, and expf differs.  Both answer to the same
 * accuracy gates and give the same exact answers wherever every partial sum is exact.
 * Pointers need 2-byte alignment only.  Q, K and V rows are read with 16-byte loads when q, k, v are 16-byte aligned and all their
 * strides are multiples of 8, with 2-byte loads otherwise; `out` is written with 8-byte stores when it is 8-byte aligned and its
 * strides are multiples of 4, with 2-byte stores otherwise: the same bits either way.
 * SEMICRF_EINVAL, with nothing launched and `out` untouched: a shape outside the supported set, a NULL or misaligned (odd) pointer, a
 * negative count or stride, a token stride >= 2^28, n0 n1 H >= 2^31.
 */
int semicrf_axial_attention_bf16_supported(int Lq, int Lk, int H, int d);
int semicrf_axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int64_t n0, int64_t n1, int Lq, int Lk,
                                 int H, int d, int64_t q_stride_s0, int64_t q_stride_s1, int64_t q_stride_l, int64_t k_stride_s0,
                                 int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0, int64_t v_stride_s1, int64_t v_stride_l,
                                 int64_t out_stride_s0, int64_t out_stride_s1, int64_t out_stride_l, semicrf_stream_t stream);

/*
 * The backward of semicrf_axial_attention_bf16: dq, dk, dv from q, k, v and the cotangent dout, every element one bf16 value.  It is
 * the contract of semicrf_axial_attention_bwd with bf16 elements and WITHOUT `out`: TOKEN-MAJOR, head h the slice [h d, (h + 1) d);
 * two sequence dimensions and three ELEMENT strides for each of the seven tensors (q, dout, dq: Lq tokens; k, v, dk, dv: Lk tokens), so
 * the gradient of the time-axis call lands in the [N][T'][F'][H d] buffer without a transposed copy.  Strides of q, k, v are >= 0 (0
 * repeats); dout, dq, dk, dv are real, non-overlapping tensors.  A token stride stays below 2^28 elements; all offsets are 64-bit.  Any
 * of dq, dk, dv may be NULL: nothing is computed or written for it.
 *
 * Supported (semicrf_axial_attention_bf16_bwd_supported returns 1): exactly the forward's set -- 1 <= Lq, Lk <= SEMICRF_ATTENTION_MAX_L;
 * d a multiple of 8 in [8, SEMICRF_ATTENTION_MAX_D]; H >= 1.  n0 n1 H < 2^31.  n0 n1 == 0 launches nothing.
 *
 * The chain (csrc/attention_bf16_math.h), per sequence and head; s, m, p, ph = bf16_rne(p) and sum are recomputed exactly as the bf16
 * forward forms them (the forward saves nothing), scale = (float)(1 / sqrt(d)):
 *   P[i][j]  = (float)ph[i][j] / sum_i                          one fp32 division
 *   dP[i][j] = sum over c of dout[i][c] v[j][c]                 exact products, fp32 accumulation
 *   D_i      = sum over j of P[i][j] dP[i][j]                   fp32, in the fixed order of `sum`: the keys whose ((j >> 2) & 1) is 0
 *                                                               ascending, then those whose bit is 1, then the two partial sums added
 *   dS[i][j] = P[i][j] (dP[i][j] - D_i)                         fp32
 *   dSh = bf16_rne(dS), Ph = bf16_rne(P)                        what the three gradient products consume
 *   dq[i][c] = bf16_rne(scale * sum over j of dSh[i][j] k[j][c])   fp32 accumulation, one multiplication by scale, one rounding
 *   dk[j][c] = bf16_rne(scale * sum over i of dSh[i][j] q[i][c])
 *   dv[j][c] = bf16_rne(sum over i of Ph[i][j] dout[i][c])
 * D_i is the softmax form, not dout_i . out_i: it is up to 3.4 x closer to float64 on sharp softmaxes, gives dq = dk = 0 exactly at
 * Lk = 1, and needs no `out`.
 * On the device all five products run on v_mfma_f32_32x32x16_bf16.  Keys from Lk to the tile edge are masked to -inf before the maximum
 * and have P = dS = 0 exactly; rows past Lq / Lk are never read and never written; a padded query has dout = 0 in registers and adds
 * exact zeros to dk and dv; the head dimension is padded with zeros in registers and LDS only.  One workgroup per (sequence, head) forms
 * all of its dk and dv: no atomics, no workspace, one launch on `stream`, and a sequence's gradients are bit-identical from run to run,
 * whatever n0, n1, its position in the batch, the strides and the alignment are.
 * The device and the host mirror (the CPU key of torch.ops.semicrf.axial_attention_bf16_bwd) are NOT bit-identical to each other: the
 * matrix instruction's internal summation is not the mirror's ascending fp32 chain, and expf differs.  Both answer to the same
 * accuracy gates and give the same exact answers wherever every partial sum is exact.
 * Pointers need 2-byte alignment only.  Q, K, V and dout rows are read with 16-byte loads when q, k, v, dout are 16-byte aligned and all
 * their strides are multiples of 8, with 2-byte loads otherwise; each of dq, dk, dv is written with 8-byte stores when it is 8-byte
 * aligned and its strides are multiples of 4, with 2-byte stores otherwise: the same bits either way.
 * SEMICRF_EINVAL, with nothing launched and dq / dk / dv untouched: a shape outside the supported set, a NULL q / k / v / dout, a
 * misaligned (odd) pointer, a negative count or stride, a token stride >= 2^28, n0 n1 H >= 2^31.
 */
int semicrf_axial_attention_bf16_bwd_supported(int Lq, int Lk, int H, int d);
int semicrf_axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk,
                                     uint16_t* dv, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, int64_t q_stride_s0, int64_t q_stride_s1,
                                     int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0,
                                     int64_t v_stride_s1, int64_t v_stride_l, int64_t dout_stride_s0, int64_t dout_stride_s1,
                                     int64_t dout_stride_l, int64_t dq_stride_s0, int64_t dq_stride_s1, int64_t dq_stride_l, int64_t dk_stride_s0,
                                     int64_t dk_stride_s1, int64_t dk_stride_l, int64_t dv_stride_s0, int64_t dv_stride_s1, int64_t dv_stride_l,
                                     semicrf_stream_t stream);

/*
 * The feed-forward ResBlock of the backbone's transformer layers in eval mode, as one launch.  Replaces: RMSNorm, Linear, GELU,
 * Linear, the multiplication by the LayerScale and the residual addition of ResBlock around the feed-forward module
 * (LayersTransformer.py), about ten launches and three round trips of the [tokens, hidden] activation.  For every token t = (i0, i1),
 * i0 < n0, i1 < n1, with x_t its D values:
 *   out_t = x_t + (W2 gelu(W1 (x_t / sqrt(mean(x_t^2) + eps)) + b1) + b2) * scale
 * fp32, no dropout.  W1 [hidden][D], b1 [hidden], W2 [D][hidden], b2 [D] and scale [D] are contiguous and read as nn.Linear and
 * ResBlock store them; nothing is repacked or cached between calls.  x and out are [n0, n1, D] VIEWS with a contiguous last dimension
 * and two ELEMENT row strides each: token (i0, i1) starts at base + i0 stride_0 + i1 stride_1.  One [T'][F'][D] buffer goes in as
 * n0 = T', n1 = F' (strides F' D, D) and its transpose(-3, -2) view as n0 = F', n1 = T' (strides D, F' D): no copy; the op is per
 * token, so a caller is free to hand the tokens of a batch over in the order of their addresses.  All offsets are 64-bit.
 *
 * Supported (semicrf_ffn_residual_supported returns 1): D a multiple of 8 in [8, SEMICRF_FFN_MAX_D]; hidden a multiple of 8 in
 * [8, SEMICRF_FFN_MAX_HIDDEN].  1 <= n0, n1 and n0 n1 < 2^37.
 *
 * Exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32), one fixed chain of operations per output element (csrc/ffn_math.h): the sum
 * of squares as four strided fmaf chains added pairwise; 1 / sqrt(ss / D + eps); both products fmaf chains over the ascending
 * contraction index from +0, the second one per hidden chunk of SEMICRF_FFN_HIDDEN_CHUNK columns, the chunks' sums added in ascending
 * order; gelu in its exact erf form (erfc below 0); bias, scale and residual as one addition, one multiplication, one addition.  A workgroup owns
 * SEMICRF_FFN_ROW_TILE rows; rows past the last token, the columns past D and past hidden are zeros formed in registers, never read and
 * never stored.  No atomics, no workspace; the tile sizes depend on nothing: a token's result is bit-identical from run to run, whatever
 * the other tokens, n0, n1 and the strides are.  16-byte loads when the bases are 16-byte aligned and the strides multiples of 4,
 * 4-byte loads otherwise (the same numbers).  One launch on `stream`; no synchronisation, no allocation.
 * SEMICRF_EINVAL, with nothing launched and `out` untouched: a shape outside the supported set, a NULL or misaligned (4 bytes) pointer,
 * n0 or n1 <= 0, n0 n1 >= 2^37, a negative stride or one of 2^40 elements or more, a row stride of `out` below D where that dimension
 * has more than one entry, `out` overlapping `x`.
 */
#define SEMICRF_FFN_ROW_TILE 64
#define SEMICRF_FFN_HIDDEN_CHUNK 64
#define SEMICRF_FFN_MAX_D 256
#define SEMICRF_FFN_MAX_HIDDEN 4096
int semicrf_ffn_residual_supported(int D, int hidden);
int semicrf_ffn_residual(const float* x, float* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                         int64_t out_stride_1, int D, int hidden, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* scale, float eps, semicrf_stream_t stream);

/*
 * The same block in TRAINING: both dropouts in the forward, and its backward (once differentiable).  fp32, exact on the matrix pipe.
 * With i = i0 n1 + i1 the token's index in the [n0, n1, D] view that is handed over (so: the tokens in the order the caller lists
 * them; the Python wrapper lists them in the order of their addresses), M1 = keep(seed, 0, i, j) / (1 - p_hidden) on the hidden
 * activation and M2 = keep(seed, 1, i, n) / (1 - p_out) on the module's output (a dropout with p = 0 neither masks nor scales):
 *   rs  = 1 / sqrt(mean(x^2) + eps)      xn = x * rs
 *   z   = W1 xn + b1                     a  = gelu(z) * M1
 *   y   = W2 a + b2                      out = x + (y * M2) * scale
 *   dscale = sum_tok g * (y * M2)        dy  = (g * scale) * M2   db2 = sum_tok dy                      g = dout
 *   dW2    = sum_tok dy (x) a            da  = W2^T dy            dz  = (da * M1) * gelu'(z)
 *   db1    = sum_tok dz                  dW1 = sum_tok dz (x) xn  dxn = W1^T dz
 *   dx     = g + rs * (dxn - xn * mean(dxn * xn))
 * keep(seed, stream, i, j): Philox-4x32-10 (Salmon et al., SC'11) with counter ((i >> 2) mod 2^32, j, stream, i >> 34) and key (seed mod
 * 2^32, seed >> 32); element i takes output word i & 3 and is KEPT iff that word >= floor(p * 2^32).  stream 0: the hidden dropout
 * (j a hidden column), stream 1: the output dropout (j a column of D).  A stateless function of (seed, stream, i, j): a token's mask
 * does not depend on the number of tokens.  semicrf_ffn_dropout_mask writes both masks as bytes (1 = kept), [rows][hidden] and
 * [rows][D]; a dropout with p = 0 is all ones.
 *
 * semicrf_ffn_residual_train_fwd: semicrf_ffn_residual's kernel in its training mode, the same chain per element; it also stores
 * z [n0 n1][hidden] and y [n0 n1][D] (dense, row i = the token's index) for the backward.  With p_hidden = p_out = 0 `out` has the
 * bits of semicrf_ffn_residual.  One launch, no workspace.
 *
 * semicrf_ffn_residual_bwd: dout, x and dx are [n0, n1, D] views with two ELEMENT row strides each and a contiguous last dimension
 * (dx is laid out by its own strides, e.g. like x); z and y are the forward's; W1, W2, scale as the forward read them; dW1 [hidden][D],
 * db1 [hidden], dW2 [D][hidden], db2 [D], dscale [D] are contiguous and written whole.  Seven launches on `stream`, no atomics, no
 * allocation: the order of operations of every gradient is fixed (csrc/ffn_math.h) -- fmaf chains in sub-chains of 64 contraction
 * values (da, dxn) or 128 tokens (dW1, dW2), one partial plane of all parameter gradients per chunk of SEMICRF_FFN_BWD_ROW_CHUNK tokens
 * (whatever n0 n1 is), the column sums db1, db2, dscale per chunk in double and rounded once, the planes added in ascending order --
 * so every gradient is bit-identical from run to run and a token's dx does not depend on the other tokens.
 * Workspace: semicrf_ffn_residual_bwd_workspace_bytes(n0 n1, D, hidden): rs [tokens], dy [tokens][D], dz [tokens][hidden] and
 * ceil(tokens / chunk) planes of 2 D hidden + hidden + 2 D floats; semicrf_workspace_bytes(SEMICRF_OP_FFN_RESIDUAL_BWD, tokens,
 * hidden) is an upper bound of it for every supported D.  Nothing is written past the size the function names, nor outside dx and the
 * five gradients.  Supported: semicrf_ffn_residual_bwd_supported = the set of semicrf_ffn_residual; n0 n1 <= 65535 chunks.
 * SEMICRF_EINVAL, with nothing launched and nothing written: the cases of semicrf_ffn_residual (dx in the place of out), p outside
 * [0, 1), dx overlapping dout, x, z or y; SEMICRF_EWORKSPACE: a workspace smaller than the function says.
 */
#define SEMICRF_FFN_BWD_ROW_CHUNK 512
int semicrf_ffn_residual_train_fwd(const float* x, float* out, float* z, float* y, int64_t n0, int64_t n1, int64_t x_stride_0,
                                   int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const float* W1,
                                   const float* b1, const float* W2, const float* b2, const float* scale, float eps, uint64_t seed,
                                   double p_hidden, double p_out, semicrf_stream_t stream);
int semicrf_ffn_residual_bwd_supported(int D, int hidden);
size_t semicrf_ffn_residual_bwd_workspace_bytes(int64_t tokens, int D, int hidden);
int semicrf_ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, int64_t n0, int64_t n1, int64_t dout_stride_0,
                             int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0, int64_t dx_stride_1, int D,
                             int hidden, const float* W1, const float* W2, const float* scale, float eps, uint64_t seed, double p_hidden,
                             double p_out, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale, void* ws, size_t ws_bytes,
                             semicrf_stream_t stream);
int semicrf_ffn_dropout_mask(uint64_t seed, int64_t rows, int D, int hidden, double p_hidden, double p_out, unsigned char* mask_hidden,
                             unsigned char* mask_out, semicrf_stream_t stream);

/*
 * The same block with both products on the bf16 matrix instruction (v_mfma_f32_32x32x16_bf16), eval mode, forward only, one launch, no
 * workspace, no atomics: what a bf16 backbone, or an fp32 one under bf16 autocast, runs in place of about ten stock launches.  Two
 * entry points share one kernel body (csrc/ffn_bf16.hip) and one chain of operations (csrc/ffn_bf16_math.h):
 *   semicrf_ffn_residual_bf16        x, out, W1, b1, W2, b2 and scale are bfloat16 in memory (raw 16-bit patterns)
 *   semicrf_ffn_residual_bf16_mixed  all seven are fp32 in memory, as the module holds them.  W1 and W2 are rounded to bf16 (nearest
 *                                    even) while they are staged, on every call: no bf16 copy of the weights exists that could go
 *                                    stale.  b1, b2 and scale are used AS FP32 -- unlike autocast's nn.Linear, which rounds its
 *                                    bias (and its output) to bf16 too -- and `out` is not rounded.
 * Chain: x to fp32; the sum of squares and rs exactly as semicrf_ffn_residual; x rs rounded to bf16; h = W1 xh with exact products
 * and fp32 accumulation, + b1; gelu in fp32 (exact erf form), rounded to bf16; acc = W2 gh on ONE running fp32 accumulator over all
 * of hidden; out = x + (acc + b2) * scale in fp32, rounded ONCE to the output type.  The device sums 16 products inside a matrix
 * instruction and the host mirror one by one: they agree wherever every partial sum is exact, and to rounding elsewhere.
 * Views, strides, the supported set, padding and determinism are semicrf_ffn_residual's: [n0, n1, D] views with two ELEMENT row
 * strides each; D a multiple of 8 in [8, SEMICRF_FFN_MAX_D], hidden a multiple of 8 in [8, SEMICRF_FFN_MAX_HIDDEN], 1 <= n0, n1,
 * n0 n1 < 2^37; a workgroup owns SEMICRF_FFN_BF16_ROW_TILE rows and walks hidden in chunks of SEMICRF_FFN_BF16_HIDDEN_CHUNK columns;
 * rows past the last token, columns past D and past hidden are zeros formed in registers, never read as data and never stored; a
 * token's result is bit-identical whatever the other tokens, n0, n1, the strides and the alignment are.  Pointers need the alignment
 * of an element (2 bytes, 4 bytes for _mixed); 16-byte loads when x, W1 and W2 are 16-byte aligned and x's strides multiples of 16
 * bytes, element loads otherwise (the same bits).  One launch on `stream`; no synchronisation, no allocation.
 * SEMICRF_EINVAL, with nothing launched and `out` untouched: the cases of semicrf_ffn_residual.
 */
#define SEMICRF_FFN_BF16_ROW_TILE 64
#define SEMICRF_FFN_BF16_HIDDEN_CHUNK 64
int semicrf_ffn_residual_bf16_supported(int D, int hidden);
int semicrf_ffn_residual_bf16_mixed_supported(int D, int hidden);
int semicrf_ffn_residual_bf16(const uint16_t* x, uint16_t* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                              int64_t out_stride_1, int D, int hidden, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2,
                              const uint16_t* b2, const uint16_t* scale, float eps, semicrf_stream_t stream);
int semicrf_ffn_residual_bf16_mixed(const float* x, float* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                                    int64_t out_stride_1, int D, int hidden, const float* W1, const float* b1, const float* W2, const float* b2,
                                    const float* scale, float eps, semicrf_stream_t stream);

/*
 * Training through the bf16 block: the forward kernel in a training mode and one backward on the same matrix instruction, in both
 * forms (every tensor bfloat16; every tensor fp32 with bf16 operands inside: _mixed).  The chain of every element, the order of every
 * sum and the layout of the saved buffer are stated in csrc/ffn_bf16_train_math.h; the host mirrors follow it one product at a time.
 *   out = x + ((W2 (gelu(W1 rmsnorm(x) + b1) * M1) + b2) * M2) * scale
 * M1, M2: the masks of semicrf_ffn_dropout_mask (the same seed gives the same masks on the fp32 and the bf16 routes), as factors
 * keep / (1 - p).  With p_hidden = p_out = 0 `out` has the bits of semicrf_ffn_residual_bf16 / _mixed.
 *
 * semicrf_ffn_residual_bf16_train_fwd / _mixed_train_fwd: the eval entry points' contract (views, strides, supported set, rejected
 * calls), one launch, no workspace.  `saved` (16-byte aligned, semicrf_ffn_residual_bf16_train_saved_bytes(n0 n1, D, hidden) bytes) is an
 * opaque buffer for the backward: zs = bf16(h) [tokens][hidden], then ys = y rounded to the form's element [tokens][D].
 *
 * semicrf_ffn_residual_bf16_bwd / _mixed_bwd: dout, x and dx are [n0, n1, D] views with two ELEMENT row strides each; W1, W2, scale and
 * the five gradients lie as nn.Linear and ResBlock store them, in the form's element type.  Five launches on `stream` (the weights as
 * transposed bf16 operands; the per-token part dy, da, dz, dxn, dx in the forward's geometry; dW2 and dW1 per chunk of
 * SEMICRF_FFN_BWD_ROW_CHUNK tokens; the column sums in double; the planes added in ascending order with one rounding), no atomics, no
 * memset, no synchronisation, no allocation: every gradient is bit-identical from run to run, and a token's dx depends on its own row,
 * its index, the seed and the weights only.  ah = bf16(gelu(zs) * M1) is recomputed from zs (the forward's operand saw the unrounded h).
 * Workspace (16-byte aligned): semicrf_ffn_residual_bf16_bwd_workspace_bytes(n0 n1, D, hidden); nothing in it is read before it is
 * written.  16-byte loads of x and dout when both are 16-byte aligned with strides multiples of 16 bytes, element loads otherwise: the
 * same bits.  Supported: semicrf_ffn_residual_bf16_bwd_supported = the set of semicrf_ffn_residual_bf16; n0 n1 <= 65535 chunks.
 * SEMICRF_EINVAL, with nothing launched and nothing written: the cases of semicrf_ffn_residual_bf16 (dx in the place of out, dout and x
 * each in the place of x), p outside [0, 1), a saved buffer that is too small, misaligned or overlaps a view; SEMICRF_EWORKSPACE: a
 * workspace that is too small.
 */
int semicrf_ffn_residual_bf16_bwd_supported(int D, int hidden);
size_t semicrf_ffn_residual_bf16_train_saved_bytes(int64_t tokens, int D, int hidden);
size_t semicrf_ffn_residual_bf16_bwd_workspace_bytes(int64_t tokens, int D, int hidden);
int semicrf_ffn_residual_bf16_train_fwd(const uint16_t* x, uint16_t* out, void* saved, size_t saved_bytes, int64_t n0, int64_t n1, int64_t x_stride_0,
                                        int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const uint16_t* W1,
                                        const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale, float eps, uint64_t seed,
                                        double p_hidden, double p_out, semicrf_stream_t stream);
int semicrf_ffn_residual_bf16_mixed_train_fwd(const float* x, float* out, void* saved, size_t saved_bytes, int64_t n0, int64_t n1, int64_t x_stride_0,
                                              int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const float* W1,
                                              const float* b1, const float* W2, const float* b2, const float* scale, float eps, uint64_t seed,
                                              double p_hidden, double p_out, semicrf_stream_t stream);
int semicrf_ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, size_t saved_bytes, int64_t n0, int64_t n1,
                                  int64_t dout_stride_0, int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0,
                                  int64_t dx_stride_1, int D, int hidden, const uint16_t* W1, const uint16_t* W2, const uint16_t* scale, float eps,
                                  uint64_t seed, double p_hidden, double p_out, uint16_t* dx, uint16_t* dW1, uint16_t* db1, uint16_t* dW2, uint16_t* db2,
                                  uint16_t* dscale, void* ws, size_t ws_bytes, semicrf_stream_t stream);
int semicrf_ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, size_t saved_bytes, int64_t n0, int64_t n1,
                                        int64_t dout_stride_0, int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0,
                                        int64_t dx_stride_1, int D, int hidden, const float* W1, const float* W2, const float* scale, float eps,
                                        uint64_t seed, double p_hidden, double p_out, float* dx, float* dW1, float* db1, float* dW2, float* db2,
                                        float* dscale, void* ws, size_t ws_bytes, semicrf_stream_t stream);

/*
 * The audio front end (Util.py:78-170 behind the gain of ModelTransformer.py:159-164) as one launch.  Replaces: the gain normalisation,
 * the product of the frames with the analysis windows, the orthonormal real transform, |.|^2, the channel mean, the matrix product with
 * the mel filterbank and the log compression -- a dozen launches and two round trips of a [N, C, nFrame, nWin, W] tensor.  For every
 * recording n, channel c, frame t, window w and band m:
 *   x[j]   = frames[n, c, t, j] (with a gain: (x[j] - shift[n]) / denom[n]), times windows[w, j]     j < W
 *   p[k]   = |rfft(x)[k]|^2 / W                                                                     k <= W / 2
 *   p[k]   = mean over c of p[k] when to_mono (the output then has one channel)
 *   mel    = sum over r < fb_len[m] of p[fb_start[m] + r] fb_val[fb_off[m] + r]
 *   out[n, c, t, m, w] = log_flag ? (log(mel + eps) - log eps) / (-log eps) : mel
 * fp32.  `frames` is a VIEW with sample stride 1 and three ELEMENT strides (recording, channel, frame): the overlapping view of padded
 * audio (frame stride = hop) is read in place.  windows [nWin][W] and twiddles [W / 2][2] (cos, -sin of 2 pi k / W, computed in float64
 * and rounded) are contiguous; the library keeps no state.  The filterbank comes column by column: band m weighs the fb_len[m] rows from
 * fb_start[m] with the values from fb_val[fb_off[m]] (zeros inside the range included; fb_len 0 gives 0; `total` values in all; a range
 * that leaves the spectrum or the value array is cut).  shift / denom [N] are both given or both NULL.  out is contiguous
 * [N][to_mono ? 1 : C][nFrame][nMel][nWin].
 *
 * Supported (semicrf_log_mel_supported returns 1): W a power of two in [256, SEMICRF_LOGMEL_MAX_W]; nWin in [1, SEMICRF_LOGMEL_MAX_WINDOWS];
 * C in [1, SEMICRF_LOGMEL_MAX_CHANNELS]; nMel in [1, SEMICRF_LOGMEL_MAX_BANDS]; the longest column support at most W / 2 + 1 and the sum
 * of all supports at most SEMICRF_LOGMEL_MAX_SUPPORT.  N, nFrame >= 1 and N nFrame < 2^31.
 *
 * One fixed chain of operations per output element (csrc/logmel_math.h): a half-length complex radix-2 transform in LDS plus the split
 * pass, channels never share a transform; the band sums are fmaf chains over ascending rows; the logarithm is evaluated in float64 and
 * rounded once.  One workgroup per (recording, frame); no atomics, no workspace: a frame's result is bit-identical from run to run,
 * whatever the batch, its position and the strides are.  One launch on `stream`; no synchronisation, no allocation.
 * SEMICRF_EINVAL, with nothing launched and `out` untouched: a shape outside the supported set, a NULL or misaligned (4 bytes) pointer,
 * only one of shift / denom, a negative stride or one of 2^40 elements or more, eps <= 0 with log_flag, `out` overlapping `frames`.
 */
#define SEMICRF_LOGMEL_MAX_W 4096
#define SEMICRF_LOGMEL_MAX_WINDOWS 8
#define SEMICRF_LOGMEL_MAX_CHANNELS 16
#define SEMICRF_LOGMEL_MAX_BANDS 512
#define SEMICRF_LOGMEL_MAX_SUPPORT 65536
int semicrf_log_mel_supported(int W, int nWin, int C, int nMel, int max_len, int total);
int semicrf_log_mel(const float* frames, int64_t stride_n, int64_t stride_c, int64_t stride_frame, int N, int C, int nFrame, int W,
                    const float* windows, int nWin, const float* twiddles, const int32_t* fb_start, const int32_t* fb_len, const int32_t* fb_off,
                    const float* fb_val, int nMel, int total, const float* shift, const float* denom, int log_flag, float eps, int to_mono,
                    float* out, semicrf_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SEMICRF_HIP_H */
