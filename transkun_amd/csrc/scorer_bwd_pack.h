// scorer_bwd_pack.h -- the repack kernel of the packed interval-score backward: dS [T][T][C] -> Gt.  Included by scorer_bwd_gemm.hip.
#pragma once
#include "scorer_bwd_gemm_common.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// repack: dS [T][T][C] -> Gt [C][block-triangular] (Tp = T rounded up to 32), scaled; zero for b > e and for e >= T
// ---------------------------------------------------------------------------------------------
// One block = 8 end frames x 32 begin frames x 32 chains (whole 128-byte lines in; 128-byte rows out).  Only the
// b tiles up to the end of the row's 128-aligned diagonal block are written: the GEMMs read nothing beyond.
constexpr int PK_CH = 32, PK_E = 8, PK_B = 32;
constexpr int PK_ROW = PK_B + 4;                   // LDS row pitch (floats): 16-byte aligned rows
constexpr int PK_CHS = PK_E * PK_ROW + 4;          // chain pitch

// FUSED: the cotangent is built on the fly from the CRF's own quantities (the dense [T][T][C]
// gradient of ComputeLogZFasterGrad.backward is never written):  dS[e,b,c] = gout[c] * marginal[e,b,c],
//   marginal = exp(alpha[b,c] + beta[e,c] + S[e,b,c] - logZ[c])                         (e > b)
//            = exp(alpha[t,c] + beta[t,c] + S[t,t,c] - 2 softplus(S[t,t,c]) - logZ[c])  (e == b == t)
// (NeuralSemiCRFInterval.py:424-447); `dS` then points at S itself.
struct PackFused {
    const float* alpha;   // [T][C] by frame
    const float* beta;    // [T][C] by frame
    const float* logZ;    // [C]
    const float* gout;    // [C]
};

// C here is the number of SLOTS (the chain pitch of dS, alpha, beta, logZ, gout); a slot's matrix goes to its chain's slab,
// ghost slots are skipped (SL: common.h).
template <bool FUSED>
__global__ __launch_bounds__(256) void score_bwd_pack_kernel(const float* __restrict__ dS, float* __restrict__ Gt, int C,
                                                             int T, int Tp, float qscale, int mode, PackFused F, ChainSlots SL)
{
    __shared__ __attribute__((aligned(16))) float L[PK_CH * PK_CHS];
    // (chain groups fastest: the blocks that run side by side read neighbouring 128-byte pieces of the SAME cells -- whole runs of the
    // chain axis -- instead of one piece each of cells 1.4 KB apart)
    const int cg = blockIdx.x * PK_CH, b0 = blockIdx.y * PK_B, e0 = blockIdx.z * PK_E;
    if (b0 >= (e0 / GM + 1) * GM) return;
    const int tid = threadIdx.x;
    const bool vec = (C % 4 == 0) && (((uintptr_t)dS & 15) == 0) &&
                     (!FUSED || ((((uintptr_t)F.alpha | (uintptr_t)F.beta) & 15) == 0));
    // this thread's four chains are the same in every iteration (the quad depends on tid only)
    float lz[4] = {0.f, 0.f, 0.f, 0.f}, gz[4] = {0.f, 0.f, 0.f, 0.f};
    if (FUSED) {
        const int cq = cg + (tid & 7) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (cq + i < C) { lz[i] = F.logZ[cq + i]; gz[i] = F.gout[cq + i]; }
    }
#pragma unroll
    for (int it = 0; it < (PK_E * PK_B * PK_CH / 4) / 256; ++it) {
        const int idx = tid + it * 256;
        const int quad = idx & 7, cell = idx >> 3;
        const int bl = cell & 31, el = cell >> 5;
        const int e = e0 + el, b = b0 + bl, c4 = cg + quad * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < T && b <= e && c4 < C) {
            const float* src = dS + ((size_t)e * T + b) * C + c4;
            if (vec) {
                v = *(const float4*)src;
            } else {
                v.x = src[0];
                if (c4 + 1 < C) v.y = src[1];
                if (c4 + 2 < C) v.z = src[2];
                if (c4 + 3 < C) v.w = src[3];
            }
            if (FUSED) {
                float al[4] = {0.f, 0.f, 0.f, 0.f}, be[4] = {0.f, 0.f, 0.f, 0.f};
                const float* ap = F.alpha + (size_t)b * C + c4;
                const float* bp = F.beta + (size_t)e * C + c4;
                if (vec) {
                    const float4 a4 = *(const float4*)ap, b4 = *(const float4*)bp;
                    al[0] = a4.x; al[1] = a4.y; al[2] = a4.z; al[3] = a4.w;
                    be[0] = b4.x; be[1] = b4.y; be[2] = b4.z; be[3] = b4.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c4 + i < C) { al[i] = ap[i]; be[i] = bp[i]; }
                }
                float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float x = al[i] + be[i] + vv[i] - lz[i];
                    if (e == b) x -= 2.0f * softplus_f(vv[i]);
                    vv[i] = gz[i] * __expf(x);
                }
                v = make_float4(vv[0], vv[1], vv[2], vv[3]);
            }
            const float sc = qscale * len_scale_pack(e - b, mode);
            v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc;
        }
        float* dst = L + (quad * 4) * PK_CHS + el * PK_ROW + bl;
        dst[0] = v.x; dst[PK_CHS] = v.y; dst[2 * PK_CHS] = v.z; dst[3 * PK_CHS] = v.w;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < (PK_E * PK_B * PK_CH / 4) / 256; ++it) {
        const int idx = tid + it * 256;
        const int j4 = idx & 7, rowid = idx >> 3;
        const int el = rowid & 7, ch = rowid >> 3;
        const int c = cg + ch < C ? chain_of_slot(SL, cg + ch) : -1;
        if (c >= 0) {
            const float4 v = *(const float4*)(L + ch * PK_CHS + el * PK_ROW + 4 * j4);
            const int blk = e0 / GM;                          // the 8 rows of a block lie in one 128-row block
            float* row = Gt + (size_t)c * gt_chain_floats(Tp) + gt_block_off(blk) + (size_t)(e0 + el - blk * GM) * gt_row_len(blk, Tp);
            *(float4*)(row + b0 + 4 * j4) = v;
        }
    }
}

}  // namespace semicrf
