// scorer_bwd_gemm.hip -- backward of the interval scores as two batched triangular GEMMs on a repacked cotangent
// (the autograd of LayersTransformer.py:406-441 after the Linear map; same definition as scorer_bwd.hip).
//
//   G[e,b,c] = dS[e,b,c] * qscale * len(e-b) for e >= b, 0 otherwise
//   dq[c,e,:] = sum_b G[e,b,c] k[c,b,:]           dk[c,b,:] = sum_e G[e,b,c] q[c,e,:]
//
// scorer_bwd.hip multiplies straight out of the CRF's chain-minor gradient layout: a 32-row tile of 8 chains per
// workgroup, the k/q rows of every chain re-read by every row tile -- 16 B/clk/CU of operands at full matrix rate,
// which is what a CU's L1 can deliver at best (see scorer_mfma.hip), and the kernel ends up at a quarter of the fp32
// MFMA rate.  Here the cotangent is repacked ONCE into per-chain block-triangular matrices Gt[c][e][b] (scaled, zero above
// the diagonal inside the 128-aligned diagonal blocks; whole 128-byte lines in, 128-byte rows out), and both products become ordinary tiled GEMMs of one chain
// at a time: a persistent workgroup of 8 waves owns a 128 x D output tile (wave = 32 rows x D/2 columns), the
// operand chunks (32 contraction values: 16 KB of Gt + 32 rows of k or q) arrive by `buffer_load ... lds`, three
// stages deep, one s_barrier per chunk: 6 B/clk/CU.  dq reads Gt rows along the contraction (ds_read_b128, swizzled as
// in scorer_mfma.hip); dk needs the transpose, which is just a different walk of the same LDS stage (ds_read_b32 with
// consecutive lanes on consecutive b): no second copy.  The triangular structure shows up as the contraction range
// of an output tile (dq: b < 128 (i+1); dk: e >= 128 i); items are dealt longest first.
#include "common.h"
#include "launchers.h"
#include "scorer_bwd_pack.h"
#include "scorer_bwd_gemm_exact.h"
#include "scorer_bwd_gemm3.h"

namespace semicrf {

static int round_up32(int T) { return (T + 31) / 32 * 32; }

// Packed path or direct kernels, exact or three-limb: the one statement of it.  rows_ok: q and k are rows_addressable (the LDS
// loads); ws_ok: the workspace is there and 16-byte aligned, ws_bytes: its size.  want_dq / want_drowc: the outputs asked for.
ScoreBwdPlan plan_score_bwd(int C, int T, int D, bool rows_ok, bool ws_ok, size_t ws_bytes, bool want_dq, bool want_drowc,
                            long long lddq, long long lddk, int prec)
{
    ScoreBwdPlan P{SCORE_BWD_DIRECT, 0};
    if (!(D == 64 || D == 128 || D == 256) || T < 64 || C < 1) return P;
    const size_t slab = gt_chain_floats(round_up32(T));
    if (slab * 4 >= (1ull << 31)) return P;                              // 32-bit buffer offsets inside a chain's slab
    P.ws_bytes = (size_t)C * slab * sizeof(float) + 4096;                // + slack for the transposed walk of the last tile
    // the row sums of the packed cotangent come out of the dq GEMM, which then must run
    if ((want_drowc && !want_dq) || !rows_ok || !ws_ok || ws_bytes < P.ws_bytes) return P;
    // (the three-limb kernels address their outputs through buffers: 32-bit offsets inside a chain's [T][ld] block)
    const bool out32 = (long long)T * lddq * 4 < (1ll << 31) && (long long)T * lddk * 4 < (1ll << 31);
    P.path = prec == 1 && out32 ? SCORE_BWD_PACKED3 : SCORE_BWD_PACKED;
    return P;
}

// 0: the packed path does not apply (the caller uses the direct kernels)
size_t interval_score_bwd_ws_bytes(int C, int T, int D) { return plan_score_bwd(C, T, D, true, false, 0, false, false, D, D, 0).ws_bytes; }

// true when the packed path ran
// prec: 0 exact fp32 (v_mfma_f32_32x32x2_f32), 1 the three-limb bf16 contraction (score_bwd_gemm3_kernel)
// fused != nullptr: {alpha, beta, logZ, gout} and dS is the score tensor itself
// drowc (may be NULL): row sums of the packed cotangent, out of the dq GEMM
bool launch_interval_score_bwd_packed(const float* dS, const float* q, const float* k, int C, int T, int D, long long ldq,
                                      long long ldk, float qscale, int mode, float* dq, float* dk, long long lddq,
                                      long long lddk, void* ws, size_t ws_bytes, hipStream_t stream,
                                      const float* const* fused, int group, int pitch, float* drowc, long long lddrc, int prec)
{
    const bool rows_ok = rows_addressable(q, ldq, T) && rows_addressable(k, ldk, T), ws_ok = ws && ((uintptr_t)ws & 15) == 0;
    const ScoreBwdPlan P = plan_score_bwd(C, T, D, rows_ok, ws_ok, ws_bytes, dq != nullptr, drowc != nullptr, lddq, lddk, prec);
    if (P.path == SCORE_BWD_DIRECT) return false;
    const ChainSlots SL{group, pitch};
    const int Cs = (C / group) * pitch;                       // slots: the chain pitch of dS and of the CRF-side vectors
    const int Tp = round_up32(T);
    float* Gt = (float*)ws;
    // (chain groups fastest: see the kernel)
    const dim3 pgrid((Cs + PK_CH - 1) / PK_CH, Tp / PK_B, Tp / PK_E);
    if (fused) {
        const PackFused F{fused[0], fused[1], fused[2], fused[3]};
        hipLaunchKernelGGL(score_bwd_pack_kernel<true>, pgrid, dim3(256), 0, stream, dS, Gt, Cs, T, Tp, qscale, mode, F, SL);
    } else {
        const PackFused F{nullptr, nullptr, nullptr, nullptr};
        hipLaunchKernelGGL(score_bwd_pack_kernel<false>, pgrid, dim3(256), 0, stream, dS, Gt, Cs, T, Tp, qscale, mode, F, SL);
    }
#define SEMICRF_GEMM_DISPATCH(LAUNCH, AT_, OTHER, LDO, OUT, LDOUT)                                                      \
    switch (D) {                                                                                                        \
    case 64: LAUNCH<AT_, 1>(Gt, Tp, OTHER, LDO, OUT, LDOUT, C, T, stream, drowc, lddrc); break;                         \
    case 128: LAUNCH<AT_, 2>(Gt, Tp, OTHER, LDO, OUT, LDOUT, C, T, stream, drowc, lddrc); break;                        \
    default: LAUNCH<AT_, 4>(Gt, Tp, OTHER, LDO, OUT, LDOUT, C, T, stream, drowc, lddrc); break;                         \
    }
    if (P.path == SCORE_BWD_PACKED3) {
        if (dq) { SEMICRF_GEMM_DISPATCH(launch_gemm3, false, k, ldk, dq, lddq) }
        if (dk) { SEMICRF_GEMM_DISPATCH(launch_gemm3, true, q, ldq, dk, lddk) }
    } else {
        if (dq) { SEMICRF_GEMM_DISPATCH(launch_gemm, false, k, ldk, dq, lddq) }
        if (dk) { SEMICRF_GEMM_DISPATCH(launch_gemm, true, q, ldq, dk, lddk) }
    }
#undef SEMICRF_GEMM_DISPATCH
    return true;
}

}  // namespace semicrf
