// scorer_mfma.hip -- scaled-inner-product interval scores on the CDNA4 matrix cores
// (LayersTransformer.py:406-441 after the Linear map).
//
//   S[e,b,c] = qscale * <q[c,e,:], k[c,b,:]> * len(|e-b|)  (+ diag[c,e] when e == b),   layout [T][T][C]
//
// The contraction is exact fp32: v_mfma_f32_32x32x2_f32 (f32 in / f32 accumulate, a k-ordered fmaf chain; no
// xf32/TF32 exists on gfx950), so scores match the reference's fp32 einsum to round-off and the CRF decode
// that consumes them stays comparable.
//
// This file is the ROUTE (which forward kernel runs: plan_score_route, one pure host function) and the launch.  The kernels,
// each with its launcher:
//   scorer_fwd_regload.h    one matrix row per lane, register loads: any alignment, any D % 64 == 0; the work-list cache
//   scorer_fwd_stream.h     LDS-staged operands, persistent and barrier-free: 16-byte aligned rows, T < 256
//   scorer_tiled.hip        64 x 128 tiles with the epilogue inside the contraction loop: the default at T >= 256
//   scorer_fwd_tile3.h      128 x 128 tiles on the bf16 matrix instructions, three exact limbs per operand (opt-in)
//   scorer_fwd_tile_ref.h   the 64- / 128-row shared-operand tiles: the bit-level reference, debug library only
//   scorer.hip              the plain kernel for every other D
#include <atomic>
#include "common.h"
#include "launchers.h"
#include "scorer_fwd_regload.h"
#include "scorer_fwd_stream.h"
#include "scorer_fwd_tile3.h"
#if SEMICRF_HAVE_TILE_REF
#include "scorer_fwd_tile_ref.h"
#endif

namespace semicrf {

// test hook (semicrf_debug_score_variant): force one of the forward kernels where it applies; -1 = automatic
static std::atomic<int> g_score_variant{-1};
void set_score_variant(int v) { g_score_variant.store(v, std::memory_order_relaxed); }
int score_variant() { return g_score_variant.load(std::memory_order_relaxed); }

// Which forward kernel runs.  group / pitch: the slot layout of S's chain axis (SlotGeom; group == pitch == C is the contiguous
// layout), rowc: a row constant is present (the merged projection) -- both live in the tile kernels only ("slots" below).
// bases_aligned: q, k and S are 16-byte aligned (the LDS-staged kernels load q / k rows and store S's chain axis in 16-byte pieces).  forced: the test hook's variant, impl: semicrf_set_impl's.
ScoreRoute plan_score_route(int C, int T, int D, long long ldq, long long ldk, bool bases_aligned, int prec, int group, int pitch,
                            bool rowc, int forced, int impl)
{
    static const char* const need_rows =
        "a padded slot layout / a row constant needs the shared-operand kernels: 16-byte aligned rows, D % 64 == 0, T >= 128";
    static const char* const need_tiled =
        "interval_score_fwd: a padded slot layout / a row constant needs the tiled kernels (D <= 256, D % 64 == 0, T >= 128, "
        "16-byte aligned rows, 32 T Cs floats within 32-bit offsets)";
    const bool slots = !(group == C && pitch == C) || rowc;
    // the LDS-staged kernels' operands: buffer_load ... lds with 32-bit offsets
    const bool rows_ok = bases_aligned && rows_addressable(nullptr, ldq, T) && rows_addressable(nullptr, ldk, T);
    if (impl != 0 || D % 64 != 0) return slots ? ScoreRoute{SCORE_REFUSED, need_rows} : ScoreRoute{SCORE_NAIVE, nullptr};
    if (slots && !(rows_ok && T >= 128)) return {SCORE_REFUSED, need_rows};
    if (!rows_ok) return {SCORE_REGLOAD, nullptr};
    // 64-row reference tiles when they waste less of the last tile row (e.g. T=691: 704 vs 768 rows) -- measured 779 vs 814 us
    int variant = T < 256 ? SCORE_STREAM : ((T + 63) / 64 * 64 < (T + 127) / 128 * 128 ? SCORE_TILE64 : SCORE_TILE128);
    // the tiles with the epilogue inside the contraction loop (scorer_tiled.hip): a tie with the reference tiles at T=1024 x 352
    // (1.115 vs 1.107 ms, a third less written to HBM), faster at the model's shapes (691 x 360: 0.653 vs 0.707 ms, 1024 x 88:
    // 0.312 vs 0.365, 691 x 90: 0.183 vs 0.189)
    const int Cs = (C / group) * pitch;
    const bool tiled_ok = prec == 0 && T >= 128 && D <= 256 && (long long)32 * T * Cs * 4 < (1ll << 31);
    if (tiled_ok && (T >= 256 || slots)) variant = SCORE_TILED;
    if (forced >= 0) variant = forced;
    if (variant == SCORE_TILED && tiled_ok) return {SCORE_TILED, nullptr};
    if (variant == SCORE_TILED) variant = SCORE_TILE128;
    if (slots && variant != SCORE_TILE64) variant = SCORE_TILE128;
    if (prec == 1 && T >= 128) return {SCORE_TILE3, nullptr};
#if SEMICRF_HAVE_TILE_REF
    if (variant == SCORE_TILE128 || variant == SCORE_TILE64) return {variant, nullptr};
#else
    // release library: what the tiled kernel does not take (D > 256, 32 T Cs floats beyond 32-bit offsets) runs on the
    // register-load kernel, which knows no slot layout / row constant
    if (slots) return {SCORE_REFUSED, need_tiled};
#endif
    return {variant == SCORE_STREAM ? SCORE_STREAM : SCORE_REGLOAD, nullptr};
}

static int launch_score_regload(const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq, long long ldk,
                                long long ldd, float qscale, int mode, int full, float* S, int band, hipStream_t stream);

// kernel: plan_score_route's answer for these arguments (not SCORE_REFUSED).  Returns 1 when the work list could not be allocated.
int launch_interval_score_fwd(int kernel, const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq,
                              long long ldk, long long ldd, float qscale, int mode, int full, float* S, hipStream_t stream, int group,
                              int pitch, const float* rowc, long long ldrc)
{
    const int band = 4;                 // tile rows per band of the work list (scorer_fwd_regload.h)
    switch (kernel) {
    case SCORE_NAIVE:
        launch_interval_score_naive(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, stream);
        return 0;
    case SCORE_TILED:
        launch_interval_score_tiled(q, k, diag, rowc, C, T, D, ldq, ldk, ldd, ldrc, qscale, mode, full, S, stream, group, pitch);
        return 0;
    case SCORE_TILE3:
        return launch_score_tile3<128>(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, stream, group, pitch, rowc, ldrc);
#if SEMICRF_HAVE_TILE_REF
    case SCORE_TILE128:
        return launch_score_tile<128>(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, stream, group, pitch, rowc, ldrc);
    case SCORE_TILE64:
        return launch_score_tile<64>(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, stream, group, pitch, rowc, ldrc);
#endif
    case SCORE_STREAM:
        return launch_score_stream(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, band, stream);
    default:
        return launch_score_regload(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, mode, full, S, band, stream);
    }
}

// The register-load kernel's launcher (kernel and work list: scorer_fwd_regload.h).  It stands here, behind the switch, because the
// code object lists template kernels in the order their uses are met: in front of it the ten instantiations would move ahead of
// the three-limb kernel, and the object would no longer compare equal to the one before the split.
// aligned: 16-byte loads (no 32-bit offsets in this kernel, so no limit on T * ld)
static int launch_score_regload(const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq,
                                long long ldk, long long ldd, float qscale, int mode, int full, float* S, int band,
                                hipStream_t stream)
{
    const int nt = (T + ST - 1) / ST;
    const size_t lds = (size_t)ST * ST * SPAD * sizeof(float);
    const bool aligned = ((uintptr_t)q % 16 == 0) && ((uintptr_t)k % 16 == 0) && ldq % 4 == 0 && ldk % 4 == 0;
    const int nch = (D / 64 <= 4) ? D / 64 : 0;
    int ngrid = 0;
    const int2* work = score_work_list(nt, (C + SC - 1) / SC, full ? 1 : 0, band, &ngrid, stream);
    if (!work) return 1;
    const dim3 grid(ngrid), block(256);
#define SEMICRF_FWD_LAUNCH(A, N)                                                                                        \
    do {                                                                                                                \
        static PerDeviceOnce attr_once;                                                                                   \
        if (attr_once.first()) {                                                                                                \
            (void)hipFuncSetAttribute((const void*)interval_score_mfma_kernel<A, N>,                                    \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                           \
        }                                                                                                               \
        hipLaunchKernelGGL((interval_score_mfma_kernel<A, N>), grid, block, lds, stream, q, k, diag, C, T, D, ldq, ldk, \
                           ldd, qscale, mode, full, S, work);                                                           \
    } while (0)
#define SEMICRF_FWD_DISPATCH(A)                                                                                         \
    switch (nch) {                                                                                                      \
    case 1: SEMICRF_FWD_LAUNCH(A, 1); break;                                                                            \
    case 2: SEMICRF_FWD_LAUNCH(A, 2); break;                                                                            \
    case 3: SEMICRF_FWD_LAUNCH(A, 3); break;                                                                            \
    case 4: SEMICRF_FWD_LAUNCH(A, 4); break;                                                                            \
    default: SEMICRF_FWD_LAUNCH(A, 0); break;                                                                           \
    }
    if (aligned) { SEMICRF_FWD_DISPATCH(true) } else { SEMICRF_FWD_DISPATCH(false) }
#undef SEMICRF_FWD_DISPATCH
#undef SEMICRF_FWD_LAUNCH
    return 0;
}

}  // namespace semicrf
