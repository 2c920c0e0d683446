// attr_heads_bwd.hip -- the backward of the attribute heads (attr_heads.hip in training mode) and the dropout mask as bytes:
// semicrf_attribute_heads_bwd, semicrf_attribute_heads_dropout_mask.  Given dLv [K][Nv], dOf [K][No], the forward's z [K][H]
// (H = Hv + Ho, packed as W1's columns) and its (seed, pv, po); the order of operations is stated in include/semicrf_hip.h and
// mirrored on the host by cpu_ops.cpp.  Seven launches and one memset, no atomics:
//   dz        (row tiles of 32) x (slices of 64 hidden columns of a head): dA = dOut W2 (vector code, W2's slice and the rows' dOut in
//             LDS), dz = (dA * M) * gelu'(z) -> workspace [K][H]; slice 0 also writes the rows' two frames c T + b, c T + e
//   dW2       (slices x tiles of 64 outputs) x (row chunks of HEADS_BWD_ROWS): A recomputed from z and the mask, A^T dOut over the chunk
//             on the matrix pipe (the pipeline of dW1) -> the chunk's plane
//   bias      column sums of dz, dLv, dOf over the chunk, accumulated in double and rounded once -> the chunk's plane (db1, db2)
//   dW1       (tiles of 64 k x 64 j) x (row chunks): x^T dz over the chunk on v_mfma_f32_32x32x2_f32, x gathered again per step of
//             32 rows into LDS next to the rows of dz (both are row-major = contraction-major: no transposing stores), two LDS
//             stages and a register stage as in the forward -> the chunk's plane
//   dx        (row tiles of 64) x (tiles of 64 columns d): dz W1^T for the three thirds k = d, D + d, 2 D + d of the SAME d on the
//             matrix pipe (contraction over j in steps of 16, A = dz read once for three products); the epilogue forms
//             ga = dx_a + dx_ab ctx[c][e], gb = dx_b + dx_ab ctx[c][b] -> workspace [K][2][D]; dx itself is never stored
//   scatter   one wave per (chain, 256 columns) walks the chain's rows in ascending order: dctx[c][b] += ga, then dctx[c][e] += gb
//   reduce    the planes added in ascending chunk order -> dW1, db1, dW2, db2
// Tile sizes do not depend on K; ragged edges are padded with exact zeros.
#include "common.h"
#include "launchers.h"
#include "chain_search.h"
#include "attr_heads_math.h"

namespace semicrf {

using namespace attr_heads;

typedef float hbwd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int HB_LDT = 96;           // floats per contraction row of a 64-wide operand tile (the half waves hit disjoint banks)
constexpr int HB_LDW = 224;          // the same for the 192-wide W1 tile of the dx kernel (224 = 32 mod 64)
constexpr int HB_DZ_ROWS = 32;       // rows per workgroup of the dz kernel
constexpr int HB_NB = 128;           // outputs of a head staged per pass of the dz kernel
constexpr int HB_JC = 16;            // contraction values per step of the dx kernel

__device__ __forceinline__ int hbwd_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

struct HeadsBwdPlan {                // the workspace, in floats from its start
    size_t frames, dz, g, planes, plane_size, total;
    size_t o_db1, o_dw2, o_db2;     // inside a plane: dW1 at 0
    int nch;
};

static HeadsBwdPlan heads_bwd_plan(long long K, int D, int Hv, int Ho, int Nv, int No)
{
    HeadsBwdPlan p;
    const size_t k = (size_t)(K > 0 ? K : 0), H = (size_t)Hv + Ho;
    auto up = [](size_t x) { return (x + 63) / 64 * 64; };
    p.nch = (int)((k + HEADS_BWD_ROWS - 1) / HEADS_BWD_ROWS);
    p.frames = 0;
    p.dz = up(2 * k);
    p.g = p.dz + up(k * H);
    p.planes = p.g + up(2 * k * (size_t)D);
    p.o_db1 = 3 * (size_t)D * H;
    p.o_dw2 = p.o_db1 + H;
    p.o_db2 = p.o_dw2 + (size_t)Hv * Nv + (size_t)Ho * No;
    p.plane_size = up(p.o_db2 + (size_t)Nv + No);
    p.total = p.planes + (size_t)p.nch * p.plane_size;
    return p;
}

size_t attr_heads_bwd_workspace_bytes(long long K, int D, int Hv, int Ho, int Nv, int No)
{
    return align_up(heads_bwd_plan(K, D, Hv, Ho, Nv, No).total * sizeof(float) + 256);
}

struct HeadSlice { bool vel; int sl, Hh, N, hcol0, wv, pcol0; };
__device__ __forceinline__ HeadSlice head_slice(int s, int Hv, int Ho, int Nv, int No)
{
    HeadSlice h;
    const int Sv = slices_of(Hv);
    h.vel = s < Sv;
    h.sl = h.vel ? s : s - Sv;
    h.Hh = h.vel ? Hv : Ho;
    h.N = h.vel ? Nv : No;
    h.hcol0 = h.sl * HEADS_SLICE;
    h.wv = min(HEADS_SLICE, h.Hh - h.hcol0);
    h.pcol0 = (h.vel ? 0 : Hv) + h.hcol0;
    return h;
}

// ---- dz ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attr_heads_dz_kernel(const float* __restrict__ dLv, const float* __restrict__ dOf,
                                                            const float* __restrict__ z, const float* __restrict__ W2, int Hv, int Ho, int Nv,
                                                            int No, int K, const int* __restrict__ pairs, const int* __restrict__ offsets,
                                                            int C, int T, DropoutParams drop, float* __restrict__ dz, int* __restrict__ frames)
{
    __shared__ float Ws[HEADS_SLICE * (HB_NB + 1)];           // W2[slice column][n], rows of 129: a wave reads one n of 64 columns
    __shared__ float Ds[HB_DZ_ROWS * HB_NB];                  // dOut[row][n]
    const int tid = threadIdx.x, j = tid & 63, rg = tid >> 6;
    const int row0 = blockIdx.x * HB_DZ_ROWS;
    const HeadSlice h = head_slice(blockIdx.y, Hv, Ho, Nv, No);
    const int N = h.N;
    const size_t H = (size_t)Hv + Ho;
    const float* W2h = (h.vel ? W2 : W2 + (size_t)Hv * Nv) + (size_t)h.hcol0 * N;
    const float* dOut = h.vel ? dLv : dOf;

    if (blockIdx.y == 0 && tid < HB_DZ_ROWS && row0 + tid < K) {
        const int i = row0 + tid;
        const int c = chain_of_interval(offsets, C, i);
        const int b = min(max(pairs[2 * (size_t)i], 0), T - 1), e = min(max(pairs[2 * (size_t)i + 1], 0), T - 1);
        frames[2 * (size_t)i] = c * T + b;
        frames[2 * (size_t)i + 1] = c * T + e;
    }

    float acc[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) acc[r] = 0.0f;
    for (int n0 = 0; n0 < N; n0 += HB_NB) {
        const int nlim = min(HB_NB, N - n0);
        __syncthreads();
        for (int idx = tid; idx < HEADS_SLICE * HB_NB; idx += 256) {
            const int jj = idx >> 7, nn = idx & (HB_NB - 1);
            Ws[jj * (HB_NB + 1) + nn] = (jj < h.wv && nn < nlim) ? W2h[(size_t)jj * N + n0 + nn] : 0.0f;
        }
        for (int idx = tid; idx < HB_DZ_ROWS * HB_NB; idx += 256) {
            const int r = idx >> 7, nn = idx & (HB_NB - 1);
            Ds[idx] = (row0 + r < K && nn < nlim) ? dOut[(size_t)(row0 + r) * N + n0 + nn] : 0.0f;
        }
        __syncthreads();
        for (int nn = 0; nn < nlim; ++nn) {
            const float w = Ws[j * (HB_NB + 1) + nn];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = fmaf(Ds[(rg * 8 + r) * HB_NB + nn], w, acc[r]);
        }
    }
    if (j >= h.wv) return;
    const int head = h.vel ? 0 : 1;
    const bool masked = drop.on[head] != 0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int ib = row0 + rg * 8 + 4 * q;                 // a multiple of 4
        uint32_t draw[4] = {0u, 0u, 0u, 0u};
        if (masked) dropout_draws(drop.seed, (uint32_t)(ib >> 2), (uint32_t)(h.pcol0 + j), draw);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = ib + u;
            if (i >= K) continue;
            float t = acc[4 * q + u];
            if (masked) t = draw[u] >= drop.thr[head] ? t * drop.scale[head] : 0.0f;
            const size_t at = (size_t)i * H + h.pcol0 + j;
            dz[at] = t * gelu_grad<float>(z[at]);
        }
    }
}

// ---- dW2: the chunk's partial of A^T dOut on the matrix pipe -----------------------------------------------------------------------
// The contraction runs over the rows, as in dW1: A (recomputed from z and the mask) and dOut are row-major = contraction-major.
// A workgroup owns 64 hidden columns of a head x 64 outputs; a thread stages one column of 8 consecutive rows per step (two Philox
// calls), so the global reads of z and dOut are coalesced along the column.
__global__ __launch_bounds__(256, 2) void attr_heads_dw2_kernel(const float* __restrict__ dLv, const float* __restrict__ dOf,
                                                                const float* __restrict__ z, int Hv, int Ho, int Nv, int No, int K, int ntn,
                                                                DropoutParams drop, float* __restrict__ planes, size_t plane_size,
                                                                size_t o_dw2)
{
    constexpr int STAGE = 2 * 32 * HB_LDT;                    // the 32 rows of A, then the 32 rows of dOut
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const HeadSlice h = head_slice(blockIdx.x / ntn, Hv, Ho, Nv, No);
    const int N = h.N, head = h.vel ? 0 : 1;
    const int n0 = (blockIdx.x % ntn) * 64;
    if (n0 >= N) return;                                      // (the whole workgroup: before any barrier)
    const size_t H = (size_t)Hv + Ho;
    const float* dOut = h.vel ? dLv : dOf;
    const int chunk = blockIdx.y;
    const int r_begin = chunk * HEADS_BWD_ROWS, r_end = min(K, r_begin + HEADS_BWD_ROWS);
    const bool masked = drop.on[head] != 0;
    const int c = lane, rb = wave * 8;                        // this thread stages column c of rows rb .. rb + 7 of a step
    const bool jok = c < h.wv, nok = n0 + c < N;

    float ar[8], dr[8];
    auto load_step = [&](int row0) {
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int i = row0 + rb + p;
            ar[p] = (jok && i < r_end) ? z[(size_t)i * H + h.pcol0 + c] : 0.0f;               // z for now: gelu and mask at the store
            dr[p] = (nok && i < r_end) ? dOut[(size_t)i * N + n0 + c] : 0.0f;
        }
    };
    auto store_step = [&](int stage, int row0) {
        float* const As = smem + stage * STAGE;
        float* const Ds = As + 32 * HB_LDT;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int ib = row0 + rb + 4 * q;                 // a multiple of 4
            uint32_t draw[4] = {0u, 0u, 0u, 0u};
            if (masked) dropout_draws(drop.seed, (uint32_t)(ib >> 2), (uint32_t)(h.pcol0 + c), draw);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float a = 0.0f;
                if (jok && ib + u < r_end) {
                    a = gelu<float>(ar[4 * q + u]);
                    if (masked) a = draw[u] >= drop.thr[head] ? a * drop.scale[head] : 0.0f;
                }
                As[(rb + 4 * q + u) * HB_LDT + c] = a;
                Ds[(rb + 4 * q + u) * HB_LDT + c] = dr[4 * q + u];
            }
        }
    };

    const int jt = wave >> 1, nt = wave & 1;                  // wave = block (jt, nt) of the 64 x 64 tile of dW2
    hbwd_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nst = (r_end - r_begin + 31) / 32;
    load_step(r_begin);
    store_step(0, r_begin);
    if (nst > 1) load_step(r_begin + 32);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        if (st + 1 < nst) store_step((st + 1) & 1, r_begin + (st + 1) * 32);
        if (st + 2 < nst) load_step(r_begin + (st + 2) * 32);
        const float* aa = smem + (st & 1) * STAGE + hh * HB_LDT + jt * 32 + l31;
        const float* db = smem + (st & 1) * STAGE + 32 * HB_LDT + hh * HB_LDT + nt * 32 + l31;
#pragma unroll
        for (int m = 0; m < 16; ++m)                          // instruction m: rows 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[2 * m * HB_LDT], db[2 * m * HB_LDT], acc, 0, 0, 0);
        __syncthreads();
    }
    float* out = planes + (size_t)chunk * plane_size + o_dw2 + (h.vel ? 0 : (size_t)Hv * Nv) + (size_t)h.hcol0 * N;
    const int n = n0 + nt * 32 + l31;
    if (n < N) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = jt * 32 + hbwd_acc_row(r, hh);
            if (j < h.wv) out[(size_t)j * N + n] = acc[r];
        }
    }
}

// ---- db1, db2: column sums of dz, dLv, dOf over the chunk ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attr_heads_bias_kernel(const float* __restrict__ dLv, const float* __restrict__ dOf,
                                                              const float* __restrict__ dz, int H, int Nv, int No, int K,
                                                              float* __restrict__ planes, size_t plane_size, size_t o_db1, size_t o_db2)
{
    __shared__ double sub[HEADS_BWD_SUBSUMS][32];             // a chunk's sum is formed in double and rounded to fp32 once
    const int tid = threadIdx.x, cl = tid & 31, q = tid >> 5;
    const int col = blockIdx.x * 32 + cl;
    const int chunk = blockIdx.y;
    const int r_begin = chunk * HEADS_BWD_ROWS, r_end = min(K, r_begin + HEADS_BWD_ROWS);
    const float* src = nullptr;
    size_t ld = 0;
    if (col < H) { src = dz + col; ld = (size_t)H; }
    else if (col < H + Nv) { src = dLv + (col - H); ld = (size_t)Nv; }
    else if (col < H + Nv + No) { src = dOf + (col - H - Nv); ld = (size_t)No; }
    double t = 0.0;
    if (src)
        for (int i = r_begin + q; i < r_end; i += HEADS_BWD_SUBSUMS) t += (double)src[(size_t)i * ld];
    sub[q][cl] = t;
    __syncthreads();
    if (q == 0 && src) {
        double s = sub[0][cl];
#pragma unroll
        for (int u = 1; u < HEADS_BWD_SUBSUMS; ++u) s += sub[u][cl];
        float* plane = planes + (size_t)chunk * plane_size;
        if (col < H) plane[o_db1 + col] = (float)s; else plane[o_db2 + (col - H)] = (float)s;
    }
}

// ---- dW1: the chunk's partial of x^T dz on the matrix pipe ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256, 2) void attr_heads_dw1_kernel(const float* __restrict__ ctx, int D, long long ldc,
                                                                const int* __restrict__ frames, const float* __restrict__ dz, int H, int K,
                                                                int ntj, float* __restrict__ planes, size_t plane_size)
{
    constexpr int STAGE = 2 * 32 * HB_LDT;                    // the 32 rows of x, then the 32 rows of dz
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int k0 = (blockIdx.x / ntj) * 64, j0 = (blockIdx.x % ntj) * 64;
    const int chunk = blockIdx.y;
    const int r_begin = chunk * HEADS_BWD_ROWS, r_end = min(K, r_begin + HEADS_BWD_ROWS);
    const int nk = 3 * D;

    float xr[8], zr[8];
    auto x_at = [&](long long ra, long long rb, int k) -> float {
        if (k >= nk) return 0.0f;
        if (k < D) return ctx[ra + k];
        if (k < 2 * D) return ctx[rb + (k - D)];
        return ctx[ra + (k - 2 * D)] * ctx[rb + (k - 2 * D)];
    };
    auto load_step = [&](int row0) {
        if (VEC) {                                            // D % 4 == 0 and H % 4 == 0: four values lie in one third / inside H
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int i = row0 + (tid >> 4) + 16 * p, c4 = 4 * (tid & 15);
                float4 xv = make_float4(0.0f, 0.0f, 0.0f, 0.0f), zv = xv;
                if (i < r_end) {
                    const long long ra = (long long)frames[2 * (size_t)i] * ldc, rb = (long long)frames[2 * (size_t)i + 1] * ldc;
                    const int k = k0 + c4;
                    if (k < D) xv = *(const float4*)(ctx + ra + k);
                    else if (k < 2 * D) xv = *(const float4*)(ctx + rb + (k - D));
                    else if (k < nk) {
                        const float4 a = *(const float4*)(ctx + ra + (k - 2 * D)), b = *(const float4*)(ctx + rb + (k - 2 * D));
                        xv = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
                    }
                    if (j0 + c4 < H) zv = *(const float4*)(dz + (size_t)i * H + j0 + c4);
                }
                xr[4 * p] = xv.x; xr[4 * p + 1] = xv.y; xr[4 * p + 2] = xv.z; xr[4 * p + 3] = xv.w;
                zr[4 * p] = zv.x; zr[4 * p + 1] = zv.y; zr[4 * p + 2] = zv.z; zr[4 * p + 3] = zv.w;
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int i = row0 + (tid >> 6) + 4 * p, c = tid & 63;
                float xv = 0.0f, zv = 0.0f;
                if (i < r_end) {
                    const long long ra = (long long)frames[2 * (size_t)i] * ldc, rb = (long long)frames[2 * (size_t)i + 1] * ldc;
                    xv = x_at(ra, rb, k0 + c);
                    if (j0 + c < H) zv = dz[(size_t)i * H + j0 + c];
                }
                xr[p] = xv; zr[p] = zv;
            }
        }
    };
    auto store_step = [&](int stage) {
        float* const Xs = smem + stage * STAGE;
        float* const Zs = Xs + 32 * HB_LDT;
        if (VEC) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int r = (tid >> 4) + 16 * p, c4 = 4 * (tid & 15);
                *(float4*)(Xs + r * HB_LDT + c4) = make_float4(xr[4 * p], xr[4 * p + 1], xr[4 * p + 2], xr[4 * p + 3]);
                *(float4*)(Zs + r * HB_LDT + c4) = make_float4(zr[4 * p], zr[4 * p + 1], zr[4 * p + 2], zr[4 * p + 3]);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int r = (tid >> 6) + 4 * p, c = tid & 63;
                Xs[r * HB_LDT + c] = xr[p];
                Zs[r * HB_LDT + c] = zr[p];
            }
        }
    };

    const int kt = wave >> 1, jt = wave & 1;                  // wave = block (kt, jt) of the 64 x 64 tile of dW1
    hbwd_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nst = (r_end - r_begin + 31) / 32;
    load_step(r_begin);
    store_step(0);
    if (nst > 1) load_step(r_begin + 32);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        if (st + 1 < nst) store_step((st + 1) & 1);           // that stage was last read before the previous barrier
        if (st + 2 < nst) load_step(r_begin + (st + 2) * 32);
        const float* xa = smem + (st & 1) * STAGE + hh * HB_LDT + kt * 32 + l31;
        const float* zb = smem + (st & 1) * STAGE + 32 * HB_LDT + hh * HB_LDT + jt * 32 + l31;
#pragma unroll
        for (int m = 0; m < 16; ++m)                          // instruction m: rows 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * m * HB_LDT], zb[2 * m * HB_LDT], acc, 0, 0, 0);
        __syncthreads();
    }
    float* plane = planes + (size_t)chunk * plane_size;
    const int j = j0 + jt * 32 + l31;
    if (j < H) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + kt * 32 + hbwd_acc_row(r, hh);
            if (k < nk) plane[(size_t)k * H + j] = acc[r];
        }
    }
}

// ---- dx and the gather's backward per row: (ga, gb) -> workspace ---------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256, 2) void attr_heads_dx_kernel(const float* __restrict__ ctx, int D, long long ldc,
                                                               const int* __restrict__ frames, const float* __restrict__ dz,
                                                               const float* __restrict__ W1, int H, int K, float* __restrict__ gws)
{
    constexpr int STAGE = HB_JC * (HB_LDT + HB_LDW);          // the 16 contraction rows of dz^T [64 rows], then of W1^T [3 x 64 columns]
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.x * 64, d0 = blockIdx.y * 64;
    const int gr = tid & 63, j4 = tid >> 6;
    const bool rowok = row0 + gr < K, colok = d0 + gr < D;

    // element q of a thread's four per operand row is contraction value jj(q) of the step
    auto jj_of = [&](int q) { return VEC ? 4 * j4 + q : j4 + 4 * q; };
    float zr[4], wr[12];
    auto load_step = [&](int jc0) {
        if (VEC) {                                            // H % 4 == 0
            const int j = jc0 + 4 * j4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (rowok && j < H) v = *(const float4*)(dz + (size_t)(row0 + gr) * H + j);
            zr[0] = v.x; zr[1] = v.y; zr[2] = v.z; zr[3] = v.w;
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (colok && j < H) w = *(const float4*)(W1 + ((size_t)t * D + d0 + gr) * H + j);
                wr[4 * t] = w.x; wr[4 * t + 1] = w.y; wr[4 * t + 2] = w.z; wr[4 * t + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = jc0 + j4 + 4 * q;
                zr[q] = (rowok && j < H) ? dz[(size_t)(row0 + gr) * H + j] : 0.0f;
#pragma unroll
                for (int t = 0; t < 3; ++t) wr[4 * t + q] = (colok && j < H) ? W1[((size_t)t * D + d0 + gr) * H + j] : 0.0f;
            }
        }
    };
    auto store_step = [&](int stage) {
        float* const Zs = smem + stage * STAGE;
        float* const Ws = Zs + HB_JC * HB_LDT;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int jj = jj_of(q);
            Zs[jj * HB_LDT + gr] = zr[q];
#pragma unroll
            for (int t = 0; t < 3; ++t) Ws[jj * HB_LDW + t * 64 + gr] = wr[4 * t + q];
        }
    };

    const int rt = wave >> 1, ct = wave & 1;                  // wave = rows rt * 32 .., columns d0 + ct * 32 .. of all three thirds
    hbwd_f32x16 acc0, acc1, acc2;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; acc2[r] = 0.0f; }
    const int nst = (H + HB_JC - 1) / HB_JC;
    load_step(0);
    store_step(0);
    if (nst > 1) load_step(HB_JC);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        if (st + 1 < nst) store_step((st + 1) & 1);
        if (st + 2 < nst) load_step((st + 2) * HB_JC);
        const float* za = smem + (st & 1) * STAGE + hh * HB_LDT + rt * 32 + l31;
        const float* wb = smem + (st & 1) * STAGE + HB_JC * HB_LDT + hh * HB_LDW + ct * 32 + l31;
#pragma unroll
        for (int m = 0; m < HB_JC / 2; ++m) {                 // instruction m: j = 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            const float a = za[2 * m * HB_LDT];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * m * HB_LDW], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * m * HB_LDW + 64], acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, wb[2 * m * HB_LDW + 128], acc2, 0, 0, 0);
        }
        __syncthreads();
    }
    const int d = d0 + ct * 32 + l31;
    if (d < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = row0 + rt * 32 + hbwd_acc_row(r, hh);
            if (i < K) {
                const float ca = ctx[(long long)frames[2 * (size_t)i] * ldc + d], cb = ctx[(long long)frames[2 * (size_t)i + 1] * ldc + d];
                gws[(2 * (size_t)i) * D + d] = fmaf(acc2[r], cb, acc0[r]);
                gws[(2 * (size_t)i + 1) * D + d] = fmaf(acc2[r], ca, acc1[r]);
            }
        }
    }
}

// ---- dctx: one wave per (chain, 256 columns) walks the chain's rows in ascending order ----------------------------------------------
__global__ __launch_bounds__(64) void attr_heads_scatter_kernel(const float* __restrict__ gws, const int* __restrict__ pairs,
                                                                const int* __restrict__ offsets, int C, int T, int D, int K,
                                                                float* __restrict__ dctx)
{
    const int c = blockIdx.x, lane = threadIdx.x;
    const int lo = min(max(offsets[c], 0), K);
    const int hi = c == C - 1 ? K : min(max(offsets[c + 1], 0), K);       // rows past offsets[C] belong to the last chain
    const int dbase = blockIdx.y * 256 + lane;
    for (int i = lo; i < hi; ++i) {
        const int b = min(max(pairs[2 * (size_t)i], 0), T - 1), e = min(max(pairs[2 * (size_t)i + 1], 0), T - 1);
        float* const pb = dctx + ((size_t)c * T + b) * D;
        float* const pe = dctx + ((size_t)c * T + e) * D;
        const float* const g = gws + 2 * (size_t)i * D;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int d = dbase + 64 * q;
            if (d < D) {
                pb[d] = pb[d] + g[d];
                pe[d] = pe[d] + g[D + d];                     // (b == e: reads what the line above wrote)
            }
        }
    }
}

// ---- the planes added in ascending chunk order ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attr_heads_bwd_reduce_kernel(const float* __restrict__ planes, size_t plane_size, int nch, size_t n_dw1,
                                                                    size_t n_db1, size_t n_dw2, size_t n_db2, float* __restrict__ dW1,
                                                                    float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n_dw1 + n_db1 + n_dw2 + n_db2) return;        // (the sections are contiguous from the start of a plane)
    float t = planes[idx];
    for (int c = 1; c < nch; ++c) t += planes[(size_t)c * plane_size + idx];
    if (idx < n_dw1) dW1[idx] = t;
    else if (idx < n_dw1 + n_db1) db1[idx - n_dw1] = t;
    else if (idx < n_dw1 + n_db1 + n_dw2) dW2[idx - n_dw1 - n_db1] = t;
    else db2[idx - n_dw1 - n_db1 - n_dw2] = t;
}

// returns the first HIP error of the enqueued work (the memset; launch errors are read by the caller)
hipError_t launch_attr_heads_bwd(const float* dLv, const float* dOf, const float* z, const float* ctx, int C, int T, int D, long long ldc,
                                 const int* pairs, int K, const int* offsets, const float* W1, const float* W2, int Hv, int Ho, int Nv, int No,
                                 unsigned long long seed, double pv, double po, float* dctx, float* dW1, float* db1, float* dW2, float* db2,
                                 float* ws, hipStream_t stream)
{
    if (K <= 0) return hipSuccess;
    const HeadsBwdPlan p = heads_bwd_plan(K, D, Hv, Ho, Nv, No);
    const DropoutParams drop = dropout_params(seed, pv, po);
    const int H = Hv + Ho, S = slices_of(Hv) + slices_of(Ho);
    int* frames = (int*)(ws + p.frames);
    float* dz = ws + p.dz;
    float* gws = ws + p.g;
    float* planes = ws + p.planes;
    const hipError_t e = hipMemsetAsync(dctx, 0, (size_t)C * T * D * sizeof(float), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(attr_heads_dz_kernel, dim3((K + HB_DZ_ROWS - 1) / HB_DZ_ROWS, S), dim3(256), 0, stream, dLv, dOf, z, W2, Hv, Ho, Nv, No,
                       K, pairs, offsets, C, T, drop, dz, frames);
    const int ntn = (max(Nv, No) + 63) / 64;
    hipLaunchKernelGGL(attr_heads_dw2_kernel, dim3((unsigned)S * ntn, p.nch), dim3(256), 0, stream, dLv, dOf, z, Hv, Ho, Nv, No, K, ntn, drop,
                       planes, p.plane_size, p.o_dw2);
    hipLaunchKernelGGL(attr_heads_bias_kernel, dim3((H + Nv + No + 31) / 32, p.nch), dim3(256), 0, stream, dLv, dOf, dz, H, Nv, No, K, planes,
                       p.plane_size, p.o_db1, p.o_db2);
    const bool vec = (D & 3) == 0 && (ldc & 3) == 0 && (H & 3) == 0 && (((uintptr_t)ctx | (uintptr_t)W1 | (uintptr_t)ws) & 15) == 0;
    const int ntk = (3 * D + 63) / 64, ntj = (H + 63) / 64;
    const dim3 g1((unsigned)ntk * ntj, p.nch), g2((K + 63) / 64, (D + 63) / 64);
    if (vec) {
        hipLaunchKernelGGL(attr_heads_dw1_kernel<true>, g1, dim3(256), 0, stream, ctx, D, ldc, frames, dz, H, K, ntj, planes, p.plane_size);
        hipLaunchKernelGGL(attr_heads_dx_kernel<true>, g2, dim3(256), 0, stream, ctx, D, ldc, frames, dz, W1, H, K, gws);
    } else {
        hipLaunchKernelGGL(attr_heads_dw1_kernel<false>, g1, dim3(256), 0, stream, ctx, D, ldc, frames, dz, H, K, ntj, planes, p.plane_size);
        hipLaunchKernelGGL(attr_heads_dx_kernel<false>, g2, dim3(256), 0, stream, ctx, D, ldc, frames, dz, W1, H, K, gws);
    }
    hipLaunchKernelGGL(attr_heads_scatter_kernel, dim3(C, (D + 255) / 256), dim3(64), 0, stream, gws, pairs, offsets, C, T, D, K, dctx);
    const size_t n_dw1 = p.o_db1, n_db1 = (size_t)H, n_dw2 = p.o_db2 - p.o_dw2, n_db2 = (size_t)Nv + No;
    const size_t total = n_dw1 + n_db1 + n_dw2 + n_db2;
    hipLaunchKernelGGL(attr_heads_bwd_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, planes, p.plane_size, p.nch,
                       n_dw1, n_db1, n_dw2, n_db2, dW1, db1, dW2, db2);
    return hipSuccess;
}

// ---- the mask as bytes ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attr_heads_mask_kernel(DropoutParams drop, long long K, int Hv, int Ho, unsigned char* __restrict__ mask)
{
    const int H = Hv + Ho;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;          // one thread per (group of 4 rows, column)
    const long long q = idx / H;
    const int j = (int)(idx % H);
    if (4 * q >= K) return;
    const int head = j < Hv ? 0 : 1;
    uint32_t draw[4] = {0u, 0u, 0u, 0u};
    if (drop.on[head]) dropout_draws(drop.seed, (uint32_t)q, (uint32_t)j, draw);
    for (int u = 0; u < 4; ++u)
        if (4 * q + u < K) mask[(size_t)(4 * q + u) * H + j] = (!drop.on[head] || draw[u] >= drop.thr[head]) ? 1 : 0;
}

void launch_attr_heads_mask(unsigned long long seed, long long K, int Hv, int Ho, double pv, double po, unsigned char* mask, hipStream_t stream)
{
    if (K <= 0) return;
    const long long total = ((K + 3) / 4) * ((long long)Hv + Ho);
    hipLaunchKernelGGL(attr_heads_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, dropout_params(seed, pv, po), K, Hv,
                       Ho, mask);
}

}  // namespace semicrf
