// ffn_bwd.hip -- the backward of the feed-forward ResBlock in training mode (ffn.hip, TRAIN) and its dropout masks as bytes:
// semicrf_ffn_residual_bwd, semicrf_ffn_dropout_mask.  Given dout (g), x, the forward's z [tokens][H] and y [tokens][D] and its
// (seed, p1, p2); the order of operations is stated in csrc/ffn_math.h and mirrored on the host by cpu_ops.cpp.  Seven launches, no
// atomics, no memset; the workspace holds rs [tokens], dy [tokens][D], dz [tokens][H] and one plane of all parameter gradients per
// chunk of FFN_BWD_ROWS tokens:
//   prep      (row tiles of 64): rs from x as the forward forms it; dy = (g * scale) * M2
//   dz        (row tiles of 64) x (slices of 64 hidden columns): da = dy W2 on v_mfma_f32_32x32x2_f32, dz = (da * M1) * gelu'(z)
//   dW2       (tiles of 64 n x 64 j) x (chunks): dy^T a over the chunk's tokens on the matrix pipe, a recomputed from z and M1 while it is
//             staged -> the chunk's plane
//   sums      column sums of dz (db1), dy (db2) and g * (y * M2) (dscale) over the chunk in double, rounded once -> the chunk's plane
//   dW1       (tiles of 64 j x 64 k) x (chunks): dz^T xn over the chunk's tokens, xn = x * rs formed on the way into LDS -> the plane
//   dx        (row tiles of 64, all of D): dxn = dz W1 on the matrix pipe; the row's sum of dxn * xn never leaves the workgroup (a
//             butterfly over the 32 lanes of a half wave, then the two column waves through LDS); dx = g + rs (dxn - xn mean)
//   reduce    the planes added in ascending chunk order -> dW1, db1, dW2, db2, dscale
// dz and dx share one kernel body (rows x contraction in LDS steps of FFN_BWD_KSTEP, A transposed on its way into LDS), dW2 and dW1
// another (contraction over tokens: both operands are token-major = contraction-major).  Tile sizes depend on nothing; ragged edges
// are zeros selected in registers behind clamped, valid addresses.
#include "common.h"
#include "launchers.h"
#include "ffn_math.h"

#include <type_traits>

namespace semicrf {

using namespace ffn;
using attr_heads::gelu;
using attr_heads::gelu_grad;

typedef float fbwd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int FB_LDT = 96;           // floats per contraction row of a 64-wide operand tile (the half waves hit disjoint banks)
static_assert(FFN_BWD_ROWS % FFN_BWD_RSUB == 0 && FFN_BWD_RSUB % FFN_BWD_RSTEP == 0 && FFN_BWD_KSUB % FFN_BWD_KSTEP == 0, "sub-chains are whole steps");
static_assert(FFN_BWD_RSTEP == 32 && FFN_BWD_KSTEP == 16 && FFN_BWD_SUBSUMS == 8, "the lane maps below are written for these");

__device__ __forceinline__ int fbwd_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ uint32_t fbwd_pick(const uint32_t w[4], int u) { return u == 0 ? w[0] : u == 1 ? w[1] : u == 2 ? w[2] : w[3]; }

template <bool VEC>
__device__ __forceinline__ float4 fbwd_load4(const float* p, bool ok)    // the caller clamps p into the tensor
{
    float4 v;
    if (VEC) {
        v = *(const float4*)p;
    } else {
        v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    }
    return make_float4(ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
}

struct FfnBwdPlan {                  // the workspace, in floats from its start
    size_t rs, dy, dz, planes, plane_size, total;
    size_t o_db1, o_dw2, o_db2, o_dscale;   // inside a plane: dW1 at 0
    int nch;
};

static FfnBwdPlan ffn_bwd_plan(long long ntok, int D, int H)
{
    FfnBwdPlan p;
    const size_t k = (size_t)(ntok > 0 ? ntok : 0);
    auto up = [](size_t x) { return (x + 63) / 64 * 64; };
    p.nch = (int)((k + FFN_BWD_ROWS - 1) / FFN_BWD_ROWS);
    p.rs = 0;
    p.dy = up(k);
    p.dz = p.dy + up(k * (size_t)D);
    p.planes = p.dz + up(k * (size_t)H);
    p.o_db1 = (size_t)H * D;
    p.o_dw2 = p.o_db1 + H;
    p.o_db2 = p.o_dw2 + (size_t)D * H;
    p.o_dscale = p.o_db2 + D;
    p.plane_size = up(p.o_dscale + D);
    p.total = p.planes + (size_t)p.nch * p.plane_size;
    return p;
}

size_t ffn_bwd_workspace_bytes(long long ntok, int D, int H) { return align_up(ffn_bwd_plan(ntok, D, H).total * sizeof(float) + 256); }

struct FfnView { long long n1, s0, s1; };
__device__ __forceinline__ long long fbwd_off(const FfnView& v, long long i)
{
    const long long i0 = i / v.n1;
    return i0 * v.s0 + (i - i0 * v.n1) * v.s1;
}

// ---- prep: rs and dy ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffn_bwd_prep_kernel(const float* __restrict__ x, FfnView xv, const float* __restrict__ g, FfnView gv,
                                                           long long ntok, int D, const float* __restrict__ scale, float eps,
                                                           DropoutParams drop, float* __restrict__ rs, float* __restrict__ dy)
{
    __shared__ long long goff[64];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * 64;
    {
        // four threads per row: thread q sums the squares of k = q, q + 4, .. (the forward's chains)
        const int r = tid >> 2, q = tid & 3;
        const long long t = row0 + r;
        float s = 0.0f;
        if (t < ntok) {
            const float* xr = x + fbwd_off(xv, t);
            for (int k = q; k < D; k += 4) s = fmaf(xr[k], xr[k], s);
        }
        const float a = s + __shfl_xor(s, 1);
        const float u = a + __shfl_xor(a, 2);                // (s0 + s1) + (s2 + s3): every q holds the same bits
        if (q == 0 && t < ntok) rs[t] = rs_of(u, D, eps);
    }
    if (tid < 64) goff[tid] = row0 + tid < ntok ? fbwd_off(gv, row0 + tid) : -1;
    __syncthreads();
    for (int idx = tid; idx < 64 * D; idx += 256) {
        const int r = idx / D, n = idx - r * D;
        const long long i = row0 + r;
        if (i >= ntok) break;                                 // (rows ascend with idx)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (drop.on[1]) dropout_draws(drop.seed, 1u, (unsigned long long)i >> 2, (uint32_t)n, w);
        dy[(size_t)i * D + n] = dy_of(g[goff[r] + n], scale[n], drop, fbwd_pick(w, (int)(i & 3)));
    }
}

// ---- dz and dx: C[64 rows][64 NB columns] = A[rows][K] B[K][M] ----------------------------------------------------------------------
// A [tokens][K] and B [K][M] are dense.  A step stages FFN_BWD_KSTEP contraction values: A's 64 rows transposed (Zs[k][row]) and B's
// 64 NB columns as they lie (Ws[k][column]), two LDS stages and a register stage.  Wave (rt, cw): row block rt, column blocks cw,
// cw + 2, ..  A sub-chain of FFN_BWD_KSUB values runs on `part` from +0 and is added to `acc` at its end.
struct FfnDzArgs { const float* z; float* dz; DropoutParams drop; };
struct FfnDxArgs { const float* x; FfnView xv; const float* g; FfnView gv; float* dx; FfnView dv; const float* rs; };

template <int NB, bool DX, bool VEC>
__global__ __launch_bounds__(256) void ffn_bwd_rowgemm_kernel(const float* __restrict__ A, const float* __restrict__ B, long long ntok, int K,
                                                              int M, std::conditional_t<DX, FfnDxArgs, FfnDzArgs> ar)
{
    constexpr int LDW = 64 * NB + 32;                         // 32 (mod 64): the half waves hit disjoint banks
    constexpr int STAGE = FFN_BWD_KSTEP * (FB_LDT + LDW);
    constexpr int QW = 16 * NB;                               // float4 per contraction row of the B tile
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    __shared__ long long offs[DX ? 3 : 1][64];
    __shared__ float psum[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64 * NB;
    const int gr = tid & 63, j4 = tid >> 6;
    const bool rowok = row0 + gr < ntok;
    const float* const arow = A + (size_t)(rowok ? row0 + gr : 0) * K;

    if constexpr (DX) {
        if (tid < 64) {
            const long long t = row0 + tid;
            offs[0][tid] = t < ntok ? fbwd_off(ar.xv, t) : -1;
            offs[1][tid] = t < ntok ? fbwd_off(ar.gv, t) : -1;
            offs[2][tid] = t < ntok ? fbwd_off(ar.dv, t) : -1;
        }
    }

    float4 zr, wr[NB];
    auto load_step = [&](int kc0) {
        const int k = kc0 + 4 * j4;
        zr = fbwd_load4<VEC>(arow + (k < K ? k : 0), rowok && k < K);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + 256 * i;
            const int kk = idx / QW, c4 = idx - kk * QW;
            const bool ok = kc0 + kk < K && c0 + 4 * c4 < M;
            wr[i] = fbwd_load4<VEC>(B + (ok ? (size_t)(kc0 + kk) * M + c0 + 4 * c4 : 0), ok);
        }
    };
    auto store_step = [&](int stage) {
        float* const Zs = smem + stage * STAGE;
        float* const Ws = Zs + FFN_BWD_KSTEP * FB_LDT;
        Zs[(4 * j4 + 0) * FB_LDT + gr] = zr.x;
        Zs[(4 * j4 + 1) * FB_LDT + gr] = zr.y;
        Zs[(4 * j4 + 2) * FB_LDT + gr] = zr.z;
        Zs[(4 * j4 + 3) * FB_LDT + gr] = zr.w;
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int idx = tid + 256 * i;
            const int kk = idx / QW, c4 = idx - kk * QW;
            *(float4*)(Ws + kk * LDW + 4 * c4) = wr[i];
        }
    };

    const int rt = wave & 1, cw = wave >> 1;
    fbwd_f32x16 acc[NB], part[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[i][r] = 0.0f; part[i][r] = 0.0f; }
    const int nst = (K + FFN_BWD_KSTEP - 1) / FFN_BWD_KSTEP;
    constexpr int SUBSTEPS = FFN_BWD_KSUB / FFN_BWD_KSTEP;
    load_step(0);
    store_step(0);
    if (nst > 1) load_step(FFN_BWD_KSTEP);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        if (st + 1 < nst) store_step((st + 1) & 1);           // that stage was last read before the previous barrier
        if (st + 2 < nst) load_step((st + 2) * FFN_BWD_KSTEP);
        const float* za = smem + (st & 1) * STAGE + hh * FB_LDT + rt * 32 + l31;
        const float* wb = smem + (st & 1) * STAGE + FFN_BWD_KSTEP * FB_LDT + hh * LDW + cw * 32 + l31;
#pragma unroll
        for (int m = 0; m < FFN_BWD_KSTEP / 2; ++m) {         // instruction m: k = 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            const float a = za[2 * m * FB_LDT];
#pragma unroll
            for (int i = 0; i < NB; ++i) part[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * m * LDW + 64 * i], part[i], 0, 0, 0);
        }
        if (st % SUBSTEPS == SUBSTEPS - 1 || st + 1 == nst) {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                acc[i] += part[i];                            // sub-chains ascending
#pragma unroll
                for (int r = 0; r < 16; ++r) part[i][r] = 0.0f;
            }
        }
        __syncthreads();
    }

    if constexpr (!DX) {
        // ---- dz = (da * M1) * gelu'(z) -------------------------------------------------------------------------------------------
        static_assert(DX || NB == 1, "the dz kernel owns one column block per wave");
        const int j = c0 + cw * 32 + l31;
        if (j < M) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const long long ib = row0 + rt * 32 + 8 * g4 + 4 * hh;          // a multiple of 4
                uint32_t draw[4] = {0u, 0u, 0u, 0u};
                if (ar.drop.on[0]) dropout_draws(ar.drop.seed, 0u, (unsigned long long)ib >> 2, (uint32_t)j, draw);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ib + u >= ntok) continue;
                    const size_t at = (size_t)(ib + u) * M + j;
                    ar.dz[at] = masked(ar.drop, 0, draw[u], acc[0][4 * g4 + u]) * gelu_grad<float>(ar.z[at]);
                }
            }
        }
    } else {
        // ---- dx = g + rs (dxn - xn mean(dxn xn)) ----------------------------------------------------------------------------------
        float prod[16], rsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long long t = row0 + rt * 32 + fbwd_acc_row(r, hh);
            rsv[r] = t < ntok ? ar.rs[t] : 0.0f;
            prod[r] = 0.0f;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int n = (cw + 2 * i) * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long xo = offs[0][rt * 32 + fbwd_acc_row(r, hh)];
                const float xn = (n < M && xo >= 0) ? ar.x[xo + n] * rsv[r] : 0.0f;
                prod[r] = fmaf(acc[i][r], xn, prod[r]);       // columns past D: 0 * 0
                part[i][r] = xn;
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = prod[r];
            v += __shfl_xor(v, 1);
            v += __shfl_xor(v, 2);
            v += __shfl_xor(v, 4);
            v += __shfl_xor(v, 8);
            v += __shfl_xor(v, 16);
            if (l31 == 0) psum[cw][rt * 32 + fbwd_acc_row(r, hh)] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int n = (cw + 2 * i) * 32 + l31;
            if (n >= M) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + fbwd_acc_row(r, hh);
                const long long go = offs[1][row], xo = offs[2][row];
                if (go < 0) continue;
                const float t = psum[0][row] + psum[1][row];
                ar.dx[xo + n] = dx_of(ar.g[go + n], rsv[r], acc[i][r], part[i][r], t, M);
            }
        }
    }
}

// ---- dW2 and dW1: the chunk's partial of A^T B over its tokens on the matrix pipe ---------------------------------------------------------
// DW1 = false: C[n][j] = sum_i dy[i][n] a[i][j] (a from z and M1 at the store); DW1 = true: C[j][k] = sum_i dz[i][j] (x[i][k] rs[i]).
// A thread stages one column of 8 consecutive tokens per step for both operands (two Philox calls), so the global reads are coalesced
// along the column; no 16-byte loads, so no alignment case.
struct FfnColArgs {
    const float* a_src;              // dy [tokens][D] | dz [tokens][H]
    const float* b_src;              // z [tokens][H]  | x (view)
    FfnView xv;
    const float* rs;
    DropoutParams drop;
};

template <bool DW1>
__global__ __launch_bounds__(256, 2) void ffn_bwd_colgemm_kernel(FfnColArgs ar, long long ntok, int Md, int Nd, int ntn, float* __restrict__ planes,
                                                                 size_t plane_size, size_t o_out)
{
    constexpr int STAGE = 2 * FFN_BWD_RSTEP * FB_LDT;         // the 32 tokens of A, then the 32 tokens of B
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int m0 = (blockIdx.x / ntn) * 64, n0 = (blockIdx.x % ntn) * 64;
    const int chunk = blockIdx.y;
    const long long r_begin = (long long)chunk * FFN_BWD_ROWS, r_end = min(ntok, r_begin + FFN_BWD_ROWS);
    const int c = lane, rb = wave * 8;                        // this thread stages column c of tokens rb .. rb + 7 of a step
    const bool mok = m0 + c < Md, nok = n0 + c < Nd;

    float av[8], bv[8];
    auto load_step = [&](long long row0) {
        long long i0 = 0, i1 = 0;
        if (DW1) {
            i0 = (row0 + rb) / ar.xv.n1;
            i1 = (row0 + rb) - i0 * ar.xv.n1;
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const long long i = row0 + rb + p;
            const bool in = i < r_end;
            av[p] = (mok && in) ? ar.a_src[(size_t)i * Md + m0 + c] : 0.0f;
            if (DW1) {
                bv[p] = (nok && in) ? ar.b_src[i0 * ar.xv.s0 + i1 * ar.xv.s1 + n0 + c] * ar.rs[i] : 0.0f;
                if (++i1 == ar.xv.n1) { i1 = 0; ++i0; }
            } else {
                bv[p] = (nok && in) ? ar.b_src[(size_t)i * Nd + n0 + c] : 0.0f;                 // z for now: gelu and mask at the store
            }
        }
    };
    auto store_step = [&](int stage, long long row0) {
        float* const As = smem + stage * STAGE;
        float* const Bs = As + FFN_BWD_RSTEP * FB_LDT;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const long long ib = row0 + rb + 4 * q;           // a multiple of 4
            uint32_t draw[4] = {0u, 0u, 0u, 0u};
            if (!DW1 && ar.drop.on[0] && nok) dropout_draws(ar.drop.seed, 0u, (unsigned long long)ib >> 2, (uint32_t)(n0 + c), draw);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float b = bv[4 * q + u];
                if (!DW1) b = (nok && ib + u < r_end) ? masked(ar.drop, 0, draw[u], gelu<float>(b)) : 0.0f;
                As[(rb + 4 * q + u) * FB_LDT + c] = av[4 * q + u];
                Bs[(rb + 4 * q + u) * FB_LDT + c] = b;
            }
        }
    };

    const int mt = wave >> 1, nt = wave & 1;                  // wave = block (mt, nt) of the 64 x 64 tile
    fbwd_f32x16 acc, part;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc[r] = 0.0f; part[r] = 0.0f; }
    const int nst = (int)((r_end - r_begin + FFN_BWD_RSTEP - 1) / FFN_BWD_RSTEP);
    constexpr int SUBSTEPS = FFN_BWD_RSUB / FFN_BWD_RSTEP;
    load_step(r_begin);
    store_step(0, r_begin);
    if (nst > 1) load_step(r_begin + FFN_BWD_RSTEP);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        if (st + 1 < nst) store_step((st + 1) & 1, r_begin + (long long)(st + 1) * FFN_BWD_RSTEP);
        if (st + 2 < nst) load_step(r_begin + (long long)(st + 2) * FFN_BWD_RSTEP);
        const float* aa = smem + (st & 1) * STAGE + hh * FB_LDT + mt * 32 + l31;
        const float* bb = smem + (st & 1) * STAGE + FFN_BWD_RSTEP * FB_LDT + hh * FB_LDT + nt * 32 + l31;
#pragma unroll
        for (int m = 0; m < FFN_BWD_RSTEP / 2; ++m)           // instruction m: tokens 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[2 * m * FB_LDT], bb[2 * m * FB_LDT], part, 0, 0, 0);
        if (st % SUBSTEPS == SUBSTEPS - 1 || st + 1 == nst) {
            acc += part;                                      // sub-chains ascending
#pragma unroll
            for (int r = 0; r < 16; ++r) part[r] = 0.0f;
        }
        __syncthreads();
    }
    float* const out = planes + (size_t)chunk * plane_size + o_out;
    const int n = n0 + nt * 32 + l31;
    if (n < Nd) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + mt * 32 + fbwd_acc_row(r, hh);
            if (m < Md) out[(size_t)m * Nd + n] = acc[r];
        }
    }
}

// ---- db1, db2, dscale: column sums of dz, dy and g * (y * M2) over the chunk ------------------------------------------------------------
__global__ __launch_bounds__(256) void ffn_bwd_sums_kernel(const float* __restrict__ dz, const float* __restrict__ dy, const float* __restrict__ g,
                                                           FfnView gv, const float* __restrict__ y, long long ntok, int D, int H,
                                                           DropoutParams drop, float* __restrict__ planes, size_t plane_size, size_t o_db1,
                                                           size_t o_db2, size_t o_dscale)
{
    __shared__ double sub[FFN_BWD_SUBSUMS][32];               // a chunk's sum is formed in double and rounded to fp32 once
    const int tid = threadIdx.x, cl = tid & 31, q = tid >> 5;
    const int col = blockIdx.x * 32 + cl;
    const int chunk = blockIdx.y;
    const long long r_begin = (long long)chunk * FFN_BWD_ROWS, r_end = min(ntok, r_begin + FFN_BWD_ROWS);
    const int kind = col < H ? 0 : col < H + D ? 1 : col < H + 2 * D ? 2 : 3;
    double t = 0.0;
    if (kind == 0) {
        for (long long i = r_begin + q; i < r_end; i += FFN_BWD_SUBSUMS) t += (double)dz[(size_t)i * H + col];
    } else if (kind == 1) {
        for (long long i = r_begin + q; i < r_end; i += FFN_BWD_SUBSUMS) t += (double)dy[(size_t)i * D + (col - H)];
    } else if (kind == 2) {
        const int n = col - H - D;
        for (long long i = r_begin + q; i < r_end; i += FFN_BWD_SUBSUMS) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (drop.on[1]) dropout_draws(drop.seed, 1u, (unsigned long long)i >> 2, (uint32_t)n, w);
            t += (double)(g[fbwd_off(gv, i) + n] * masked(drop, 1, fbwd_pick(w, (int)(i & 3)), y[(size_t)i * D + n]));
        }
    }
    sub[q][cl] = t;
    __syncthreads();
    if (q == 0 && kind < 3) {
        double s = sub[0][cl];
#pragma unroll
        for (int u = 1; u < FFN_BWD_SUBSUMS; ++u) s += sub[u][cl];
        float* plane = planes + (size_t)chunk * plane_size;
        if (kind == 0) plane[o_db1 + col] = (float)s;
        else if (kind == 1) plane[o_db2 + (col - H)] = (float)s;
        else plane[o_dscale + (col - H - D)] = (float)s;
    }
}

// ---- the planes added in ascending chunk order ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffn_bwd_reduce_kernel(const float* __restrict__ planes, size_t plane_size, int nch, size_t n_w, int D, int H,
                                                             float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                             float* __restrict__ db2, float* __restrict__ dscale)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t e1 = n_w, e2 = e1 + H, e3 = e2 + n_w, e4 = e3 + D, e5 = e4 + D;   // (the sections are contiguous from the start of a plane)
    if (idx >= e5) return;
    float t = planes[idx];
    for (int c = 1; c < nch; ++c) t += planes[(size_t)c * plane_size + idx];
    if (idx < e1) dW1[idx] = t;
    else if (idx < e2) db1[idx - e1] = t;
    else if (idx < e3) dW2[idx - e2] = t;
    else if (idx < e4) db2[idx - e3] = t;
    else dscale[idx - e4] = t;
}

template <int NB>
static void ffn_bwd_launch_dx(bool vec, dim3 grid, hipStream_t stream, const float* dz, const float* W1, long long ntok, int H, int D, FfnDxArgs a)
{
    if (vec) hipLaunchKernelGGL((ffn_bwd_rowgemm_kernel<NB, true, true>), grid, dim3(256), 0, stream, dz, W1, ntok, H, D, a);
    else hipLaunchKernelGGL((ffn_bwd_rowgemm_kernel<NB, true, false>), grid, dim3(256), 0, stream, dz, W1, ntok, H, D, a);
}

// the caller (api.hip) has checked the supported set, the pointers, the strides, the workspace and the token count
void launch_ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, long long n0, long long n1, long long gs0,
                             long long gs1, long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const float* W1,
                             const float* W2, const float* scale, float eps, unsigned long long seed, double p1, double p2, float* dx,
                             float* dW1, float* db1, float* dW2, float* db2, float* dscale, float* ws, hipStream_t stream)
{
    const long long ntok = n0 * n1;
    const FfnBwdPlan p = ffn_bwd_plan(ntok, D, H);
    const DropoutParams drop = attr_heads::dropout_params(seed, p1, p2);
    const FfnView xv{n1, xs0, xs1}, gv{n1, gs0, gs1}, dv{n1, ds0, ds1};
    float* rs = ws + p.rs;
    float* dy = ws + p.dy;
    float* dz = ws + p.dz;
    float* planes = ws + p.planes;
    const unsigned ntile = (unsigned)((ntok + 63) / 64);
    hipLaunchKernelGGL(ffn_bwd_prep_kernel, dim3(ntile), dim3(256), 0, stream, x, xv, dout, gv, ntok, D, scale, eps, drop, rs, dy);
    // 16-byte loads: dy and dz start at multiples of 64 floats inside the workspace; D and H are multiples of 8
    const bool vec = (((uintptr_t)ws | (uintptr_t)W1 | (uintptr_t)W2) & 15) == 0;
    const FfnDzArgs za{z, dz, drop};
    const dim3 gz(ntile, (unsigned)((H + 63) / 64));
    if (vec) hipLaunchKernelGGL((ffn_bwd_rowgemm_kernel<1, false, true>), gz, dim3(256), 0, stream, dy, W2, ntok, D, H, za);
    else hipLaunchKernelGGL((ffn_bwd_rowgemm_kernel<1, false, false>), gz, dim3(256), 0, stream, dy, W2, ntok, D, H, za);
    const int tD = (D + 63) / 64, tH = (H + 63) / 64;
    const FfnColArgs c2{dy, z, xv, rs, drop}, c1{dz, x, xv, rs, drop};
    hipLaunchKernelGGL(ffn_bwd_colgemm_kernel<false>, dim3((unsigned)(tD * tH), p.nch), dim3(256), 0, stream, c2, ntok, D, H, tH, planes, p.plane_size,
                       p.o_dw2);
    hipLaunchKernelGGL(ffn_bwd_sums_kernel, dim3((unsigned)((H + 2 * D + 31) / 32), p.nch), dim3(256), 0, stream, dz, dy, dout, gv, y, ntok, D, H, drop,
                       planes, p.plane_size, p.o_db1, p.o_db2, p.o_dscale);
    hipLaunchKernelGGL(ffn_bwd_colgemm_kernel<true>, dim3((unsigned)(tH * tD), p.nch), dim3(256), 0, stream, c1, ntok, H, D, tD, planes, p.plane_size,
                       (size_t)0);
    const FfnDxArgs xa{x, xv, dout, gv, dx, dv, rs};
    const dim3 gx(ntile, 1);
    switch (tD) {
        case 1: ffn_bwd_launch_dx<1>(vec, gx, stream, dz, W1, ntok, H, D, xa); break;
        case 2: ffn_bwd_launch_dx<2>(vec, gx, stream, dz, W1, ntok, H, D, xa); break;
        case 3: ffn_bwd_launch_dx<3>(vec, gx, stream, dz, W1, ntok, H, D, xa); break;
        default: ffn_bwd_launch_dx<4>(vec, gx, stream, dz, W1, ntok, H, D, xa); break;
    }
    const size_t total = 2 * (size_t)H * D + H + 2 * (size_t)D;
    hipLaunchKernelGGL(ffn_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, planes, p.plane_size, p.nch, (size_t)H * D,
                       D, H, dW1, db1, dW2, db2, dscale);
}

// ---- the masks as bytes ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ffn_mask_kernel(DropoutParams drop, long long rows, int D, int H, unsigned char* __restrict__ mh,
                                                       unsigned char* __restrict__ mo)
{
    const int W = H + D;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;          // one thread per (group of 4 tokens, column of either mask)
    const long long q = idx / W;
    const int jj = (int)(idx - q * W);
    if (4 * q >= rows) return;
    const int stream = jj < H ? 0 : 1, j = jj < H ? jj : jj - H;
    uint32_t draw[4] = {0u, 0u, 0u, 0u};
    if (drop.on[stream]) dropout_draws(drop.seed, (uint32_t)stream, (unsigned long long)q, (uint32_t)j, draw);
    unsigned char* const m = stream == 0 ? mh : mo;
    const int ld = stream == 0 ? H : D;
    for (int u = 0; u < 4; ++u)
        if (4 * q + u < rows) m[(size_t)(4 * q + u) * ld + j] = (!drop.on[stream] || draw[u] >= drop.thr[stream]) ? 1 : 0;
}

void launch_ffn_mask(unsigned long long seed, long long rows, int D, int H, double p1, double p2, unsigned char* mask_hidden,
                     unsigned char* mask_out, hipStream_t stream)
{
    const long long total = ((rows + 3) / 4) * ((long long)H + D);
    hipLaunchKernelGGL(ffn_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, attr_heads::dropout_params(seed, p1, p2), rows, D,
                       H, mask_hidden, mask_out);
}

}  // namespace semicrf
