// ffn_bf16_bwd.hip -- semicrf_ffn_residual_bf16_bwd and semicrf_ffn_residual_bf16_mixed_bwd: the backward of the bf16 feed-forward
// ResBlock in training mode (ffn_bf16.hip, TRAIN), all four products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  Given dout
// (g), x, the forward's saved buffer (zs, ys) and its (seed, p_hidden, p_out); the order of operations is stated in
// csrc/ffn_bf16_train_math.h and mirrored on the host by cpu_ops.cpp.  One kernel body per role, two forms (T = bf16 | fp32 tensors).
// FIVE launches, no atomics, no memset:
//   prep      W1 and W2 as bf16 operands, transposed: W1T [D][hidden], W2T [hidden][D].  The token kernel then stages them exactly as the
//             forward stages W2 and W1 (rows of 8 consecutive contraction values), in both forms alike
//   token     (row tiles of 64, the forward's transposed geometry: a lane is ONE token) dyh from dout, scale and M2 in registers (the
//             forward's x fragments); per hidden chunk of 64: da^T = W2T-tile . dyh on one accumulator, dzh = bf16((da M1) gelu'(zs)) into
//             the LDS tile the forward keeps its gelu values in, dxn^T += W1T-tile . dzh on the running accumulators; epilogue: the row's
//             sum of dxn xn (a chain per lane, the half waves by a shuffle, the two column waves through LDS), dx, one rounding.  x and
//             dout never go through LDS.  On its way it writes the operands of the token-contracted products with the TOKEN index
//             contiguous: dyhT [D][Tp], xhT [D][Tp], dzhT [hidden][Tp], ahT [hidden][Tp] (Tp = tokens up to a multiple of 64; the rows past
//             the last token are written as zeros, so nothing depends on what the workspace held)
//   dW        (tiles of 64 x 64) x (chunks of 512 tokens) x {dW2, dW1}: both operands are 16-byte reads of 8 consecutive tokens, straight
//             from memory into the matrix instruction; k-steps of 16 tokens ascending on one accumulator -> the chunk's plane
//   sums      db1 from dzhT, db2 and dscale from dout, scale, ys and M2, in double sub-sums as ffn_bwd.hip forms them -> the chunk's plane
//   reduce    the planes added in ascending chunk order, one rounding to T -> dW1, db1, dW2, db2, dscale
// The data flow needs the token kernel before the sums over tokens (they read dzh of every token) and the planes before their sum;
// prep is the one launch that could go (by staging the transposes in the token kernel), at the price of 2-byte LDS stores per chunk.
// Tile sizes and token steps depend on nothing; ragged edges are zeros selected in registers behind clamped, valid addresses.
#include "common.h"
#include "launchers.h"
#include "bf16x3.h"
#include "ffn_bf16_dev.h"

namespace semicrf {

using namespace ffn;
using attr_heads::gelu;
using attr_heads::gelu_grad;

struct Ffn16BwdPlan {                // the workspace, in bytes from its start (every section a multiple of 256)
    size_t w1t, w2t, xht, dyht, dzht, aht, planes, total;
    size_t plane_size;               // floats
    size_t o_db1, o_dw2, o_db2, o_dscale;   // floats inside a plane: dW1 at 0
    long long tp;
    int nch;
};

static Ffn16BwdPlan ffn16_bwd_plan(long long ntok, int D, int H)
{
    Ffn16BwdPlan p;
    const size_t k = (size_t)(ntok > 0 ? ntok : 0);
    p.tp = (long long)((k + 63) / 64 * 64);
    p.nch = (int)((k + FFN_BWD_ROWS - 1) / FFN_BWD_ROWS);
    const size_t w = train_up256((size_t)H * D * 2), td = train_up256((size_t)D * p.tp * 2), th = train_up256((size_t)H * p.tp * 2);
    p.w1t = 0;
    p.w2t = p.w1t + w;
    p.xht = p.w2t + w;
    p.dyht = p.xht + td;
    p.dzht = p.dyht + td;
    p.aht = p.dzht + th;
    p.planes = p.aht + th;
    p.o_db1 = (size_t)H * D;
    p.o_dw2 = p.o_db1 + H;
    p.o_db2 = p.o_dw2 + (size_t)D * H;
    p.o_dscale = p.o_db2 + D;
    p.plane_size = (p.o_dscale + D + 63) / 64 * 64;
    p.total = p.planes + (size_t)p.nch * p.plane_size * sizeof(float);
    return p;
}

size_t ffn_bf16_bwd_workspace_bytes(long long ntok, int D, int H) { return align_up(ffn16_bwd_plan(ntok, D, H).total + 256); }

__device__ __forceinline__ int f16b_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
__device__ __forceinline__ uint32_t f16b_pick(const uint32_t w[4], int u) { return u == 0 ? w[0] : u == 1 ? w[1] : u == 2 ? w[2] : w[3]; }

// ---- prep: the weights as bf16 operands, transposed ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ffn16_bwd_prep_kernel(const T* __restrict__ W1, const T* __restrict__ W2, int D, int H,
                                                             uint16_t* __restrict__ W1T, uint16_t* __restrict__ W2T)
{
    const int n = H * D;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n) {                                            // W1T[k][j] = W1[j][k]
        const int k = idx / H, j = idx - k * H;
        W1T[idx] = operand_of(W1[(size_t)j * D + k]);
    } else if (idx < 2 * n) {                                 // W2T[j][c] = W2[c][j]
        const int i2 = idx - n;
        const int j = i2 / D, c = i2 - j * D;
        W2T[i2] = operand_of(W2[(size_t)c * H + j]);
    }
}

// ---- token: dyh, da, dzh, dxn, dx per token --------------------------------------------------------------------------------------------
template <typename T>
struct Ffn16BwdTok {
    const T* x; const T* g; T* dx;
    long long n1, xs0, xs1, gs0, gs1, ds0, ds1, ntok, tp;
    int D, H;
    const uint16_t* W1T; const uint16_t* W2T; const T* scale; const uint16_t* zs;
    float eps;
    int vec, ovec;                   // 16-byte loads of x and dout; the epilogue's four-column reads of x and dout and stores of dx
    DropoutParams drop;
    uint16_t *xhT, *dyhT, *dzhT, *ahT;
};

FFN_HD size_t lds_bytes_bf16_bwd(int D) { return lds_bytes_bf16(D) + 2 * FFN16_ROWS * sizeof(float); }

template <typename T, int DB>
__global__ __launch_bounds__(256, DB <= 5 ? 2 : 1) void ffn16_bwd_token_kernel(const Ffn16BwdTok<T> a)
{
    constexpr int NB = (DB + 1) / 2;                         // column blocks of dxn per wave
    constexpr int KS = 2 * DB;                               // k-steps of da an instantiation can have
    constexpr int NW = DB;                                   // 8-element pieces of a weight tile per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn16b_smem[];
    const int D = a.D, H = a.H;
    const int ldw = D + FFN16_PAD;
    uint16_t* const As = (uint16_t*)ffn16b_smem;                        // [64][ldw]: the chunk's rows of W2T
    uint16_t* const Bs = As + FFN16_CHUNK * ldw;                         // [D][FFN16_LDG]: the chunk's columns of W1T
    uint16_t* const Gs = Bs + D * FFN16_LDG;                             // [64][FFN16_LDG]: the chunk's dzh tile, token-major
    float* const Rs = (float*)(Gs + FFN16_ROWS * FFN16_LDG);             // [64]
    float* const Ps = Rs + FFN16_ROWS;                                   // [2][64]: a column wave's share of the row's sum of dxn xn

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int rt = wave & 1, cw = wave >> 1;
    const long long row0 = (long long)blockIdx.x * FFN16_ROWS;
    const int q8 = D >> 3;
    const int npiece = FFN16_CHUNK * q8;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const long long tp = a.tp;

    // ---- a chunk's weights: the forward's staging, with W2T in the place of W1 and W1T in the place of W2 (always 16-byte loads: the
    // workspace is aligned and D and hidden are multiples of 8)
    u32x4 wr1[NW], wr2[NW];
    auto load_w = [&](int j0) {
        const int wv = min(FFN16_CHUNK, H - j0);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx / q8, c = idx - r * q8;
            const u32x4 u = *(const u32x4*)(a.W2T + (size_t)(j0 + min(r, wv - 1)) * D + 8 * c);
            wr1[i] = idx < npiece && r < wv ? u : zero4;
            const int n = min(idx >> 3, D - 1), c2 = 8 * (idx & 7);
            const bool ok = idx < npiece && j0 + c2 < H;
            const u32x4 v = *(const u32x4*)(a.W1T + (size_t)n * H + (ok ? j0 + c2 : 0));
            wr2[i] = ok ? v : zero4;
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx / q8, c = idx - r * q8;
            if (idx < npiece) {
                *(u32x4*)(As + r * ldw + 8 * c) = wr1[i];
                *(u32x4*)(Bs + (idx >> 3) * FFN16_LDG + 8 * (idx & 7)) = wr2[i];
            }
        }
    };
    load_w(0);
    if (tid < FFN16_CHUNK) *(u32x4*)(As + tid * ldw + D) = zero4;        // the pad columns, once

    // ---- rs of the tile's rows, as the forward forms it ------------------------------------------------------------------------------------
    {
        const int r = tid >> 2, q = tid & 3;
        const long long t = row0 + r;
        float s = 0.0f;
        if (t < a.ntok) {
            const long long i0 = t / a.n1, i1 = t - i0 * a.n1;
            const T* const xr = a.x + i0 * a.xs0 + i1 * a.xs1;
            for (int m0 = 0; m0 < q8; m0 += 4) {
                float v0[4], v1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const Ffn16F8 f = ffn16_load8f<T>(xr + 8 * min(m0 + i, q8 - 1), a.vec);
                    v0[i] = q == 0 ? f.v[0] : q == 1 ? f.v[1] : q == 2 ? f.v[2] : f.v[3];
                    v1[i] = q == 0 ? f.v[4] : q == 1 ? f.v[5] : q == 2 ? f.v[6] : f.v[7];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (m0 + i < q8) {
                        s = fmaf(v0[i], v0[i], s);
                        s = fmaf(v1[i], v1[i], s);
                    }
                }
            }
        }
        const float u = s + __shfl_xor(s, 1);
        const float w = u + __shfl_xor(u, 2);
        if (q == 0) Rs[r] = rs_of(w, D, a.eps);
    }
    __syncthreads();

    // ---- this lane's token: its offsets, dyh as the operand fragments of da, and the token-contiguous copies of dyh and xh ------------------
    const long long tok = row0 + rt * 32 + l31;              // < tp: a tile lies inside the padded token range
    const bool tok_ok = tok < a.ntok;
    long long xo = 0, go = 0, dxo = 0;
    if (tok_ok) {
        const long long i0 = tok / a.n1, i1 = tok - i0 * a.n1;
        xo = i0 * a.xs0 + i1 * a.xs1;
        go = i0 * a.gs0 + i1 * a.gs1;
        dxo = i0 * a.ds0 + i1 * a.ds1;
    }
    const float rs = Rs[rt * 32 + l31];
    u32x4 gf[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int c = 16 * s + 8 * hh;
        gf[s] = zero4;
        if (c < D) {                                         // the same for the four lanes of a quad
            uint32_t w0[4], w1[4];
            ffn16_draws4(a.drop, 1, tok, c, w0);
            ffn16_draws4(a.drop, 1, tok, c + 4, w1);
            if (tok_ok) {
                const Ffn16F8 f = ffn16_load8f<T>(a.g + go + c, a.vec);
                float dy[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) dy[e] = dy_of(f.v[e], to_f32(a.scale[c + e]), a.drop, e < 4 ? w0[e & 3] : w1[e & 3]);
#pragma unroll
                for (int e = 0; e < 4; ++e) gf[s][e] = cvt_pk_bf16(dy[2 * e], dy[2 * e + 1]);
            }
            // the two column waves of a row block hold the same fragments: wave cw = 0 writes dyh, wave cw = 1 forms and writes xh
            u32x4 o = gf[s];
            if (cw == 1) {
                o = zero4;
                if (tok_ok) {
                    const Ffn16F8 f = ffn16_load8f<T>(a.x + xo + c, a.vec);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = cvt_pk_bf16(f.v[2 * e] * rs, f.v[2 * e + 1] * rs);
                }
            }
            uint16_t* const dst = (cw == 1 ? a.xhT : a.dyhT) + (size_t)c * tp + tok;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dst[(size_t)(2 * e) * tp] = (uint16_t)o[e];
                dst[(size_t)(2 * e + 1) * tp] = (uint16_t)(o[e] >> 16);
            }
        }
    }

    f32x16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const uint16_t* const w2a = As + (cw * 32 + l31) * ldw + 8 * hh;             // da's A operand: hidden column cw * 32 + l31 of the chunk
    uint16_t* const grow = Gs + (rt * 32 + l31) * FFN16_LDG;                      // this token's row of the dzh tile
    const uint16_t* w1a[NB];                                                      // dxn's A operand: column k of x
    bool on[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int n = (cw + 2 * i) * 32 + l31;
        on[i] = n < D;
        w1a[i] = Bs + min(n, D - 1) * FFN16_LDG + 8 * hh;
    }
    const uint16_t* const zrow = a.zs + (size_t)(tok_ok ? tok : 0) * H;

    const int nch = (H + FFN16_CHUNK - 1) / FFN16_CHUNK;
    for (int ch = 0; ch < nch; ++ch) {
        const int j0 = ch * FFN16_CHUNK;
        store_w();
        // zs of this lane's 16 hidden columns (register group g: columns jg .. jg + 3), asked for ahead of the next chunk's weights
        uint2 zraw[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int jg = j0 + cw * 32 + 8 * g + 4 * hh;    // a multiple of 4, hidden of 8: all four columns or none
            zraw[g] = *(const uint2*)(zrow + min(jg, H - 4));
        }
        if (ch + 1 < nch) load_w(j0 + FFN16_CHUNK);
        __syncthreads();
        // ---- da^T block cw of the chunk: contraction over n = the columns of dout -----------------------------------------------------------
        f32x16 h;
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (16 * s < D) {
                const u32x4 u = *(const u32x4*)(w2a + 16 * s);
                h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, u), __builtin_bit_cast(bf16x8, gf[s]), h, 0, 0, 0);
            }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int jg = j0 + cw * 32 + 8 * g + 4 * hh;
            const bool real = jg < H;
            uint32_t w[4];
            ffn16_draws4(a.drop, 0, tok, min(jg, H - 4), w);
            float zf[4], dz[4], ah[4];
            zf[0] = __uint_as_float(zraw[g].x << 16); zf[1] = __uint_as_float(zraw[g].x & 0xffff0000u);
            zf[2] = __uint_as_float(zraw[g].y << 16); zf[3] = __uint_as_float(zraw[g].y & 0xffff0000u);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = real && tok_ok;
                dz[e] = ok ? masked(a.drop, 0, w[e], h[4 * g + e]) * gelu_grad<float>(zf[e]) : 0.0f;
                ah[e] = ok ? masked(a.drop, 0, w[e], gelu<float>(zf[e])) : 0.0f;
            }
            const unsigned d0 = cvt_pk_bf16(dz[0], dz[1]), d1 = cvt_pk_bf16(dz[2], dz[3]);
            const unsigned a0 = cvt_pk_bf16(ah[0], ah[1]), a1 = cvt_pk_bf16(ah[2], ah[3]);
            *(uint2*)(grow + cw * 32 + 8 * g + 4 * hh) = make_uint2(d0, d1);
            if (real) {                                      // the token-contiguous copies: 32 lanes write 32 consecutive tokens of a row
                uint16_t* const dzp = a.dzhT + (size_t)jg * tp + tok;
                uint16_t* const ahp = a.ahT + (size_t)jg * tp + tok;
                dzp[0] = (uint16_t)d0; dzp[(size_t)tp] = (uint16_t)(d0 >> 16); dzp[(size_t)2 * tp] = (uint16_t)d1; dzp[(size_t)3 * tp] = (uint16_t)(d1 >> 16);
                ahp[0] = (uint16_t)a0; ahp[(size_t)tp] = (uint16_t)(a0 >> 16); ahp[(size_t)2 * tp] = (uint16_t)a1; ahp[(size_t)3 * tp] = (uint16_t)(a1 >> 16);
            }
        }
        __syncthreads();                                     // the dzh tile is written
        // ---- dxn^T blocks cw, cw + 2, .. on the running accumulators: contraction over the chunk's hidden columns -----------------------------
#pragma unroll
        for (int s = 0; s < FFN16_CHUNK / 16; ++s) {
            const u32x4 b = *(const u32x4*)(grow + 16 * s + 8 * hh);
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (cw + 2 * i < DB) {
                    u32x4 u = *(const u32x4*)(w1a[i] + 16 * s);
                    u = on[i] ? u : zero4;
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, u), __builtin_bit_cast(bf16x8, b), acc[i], 0, 0, 0);
                }
        }
        __syncthreads();                                     // the tiles are free for the next chunk
    }

    // ---- t = sum_k dxn[k] xn[k] and dx: register group g of block i holds the columns (cw + 2 i) * 32 + 8 g + 4 hh .. + 3 of this token --------
    float xn[NB][16];
    float part = 0.0f;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = (cw + 2 * i) * 32 + 8 * g + 4 * hh;
            const bool ok = cw + 2 * i < DB && n < D;
            float xv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (ok && tok_ok) ffn16_load4f(a.x + xo + n, a.ovec, xv);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xn[i][4 * g + e] = xv[e] * rs;
                if (ok) part = fmaf(acc[i][4 * g + e], xn[i][4 * g + e], part);
            }
        }
    part = part + __shfl_xor(part, 32);                      // hh = 0 + hh = 1: the sum commutes, both halves hold the same bits
    if (hh == 0) Ps[cw * FFN16_ROWS + rt * 32 + l31] = part;
    __syncthreads();
    if (tok_ok) {
        const float t = Ps[rt * 32 + l31] + Ps[FFN16_ROWS + rt * 32 + l31];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = (cw + 2 * i) * 32 + 8 * g + 4 * hh;
                if (cw + 2 * i < DB && n < D) {
                    float gv[4], o[4];
                    ffn16_load4f(a.g + go + n, a.ovec, gv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = dx_of(gv[e], rs, acc[i][4 * g + e], xn[i][4 * g + e], t, D);
                    ffn16_store4(a.dx + dxo + n, a.ovec, o);
                }
            }
    }
}

// ---- dW2 and dW1: a chunk's partial of P Q^T over its tokens, P [M][Tp] and Q [N][Tp] with the token index contiguous ---------------------
// blockIdx.z = 0: dW2[n][j] = sum_i dyh[i][n] ah[i][j] (P = dyhT, Q = ahT); 1: dW1[j][k] = sum_i dzh[i][j] xh[i][k] (P = dzhT, Q = xhT).
// Wave (mt, nt) owns block (mt, nt) of the 64 x 64 tile; a k-step is 16 tokens: 8 consecutive tokens per lane, 16 bytes, no LDS.
__global__ __launch_bounds__(256) void ffn16_bwd_dw_kernel(const uint16_t* __restrict__ dyhT, const uint16_t* __restrict__ ahT,
                                                           const uint16_t* __restrict__ dzhT, const uint16_t* __restrict__ xhT, long long tp, int D,
                                                           int H, float* __restrict__ planes, size_t plane_size, size_t o_dw2)
{
    const int which = blockIdx.z;
    const uint16_t* const P = which ? dzhT : dyhT;
    const uint16_t* const Q = which ? xhT : ahT;
    const int M = which ? H : D, N = which ? D : H;
    const int ntn = (N + 63) / 64;
    const int m0 = (blockIdx.x / ntn) * 64, n0 = (blockIdx.x % ntn) * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int mt = wave >> 1, nt = wave & 1;
    const long long t0 = (long long)blockIdx.y * FFN_BWD_ROWS, t1 = min(tp, t0 + FFN_BWD_ROWS);      // both multiples of 64
    const int m = m0 + mt * 32 + l31, n = n0 + nt * 32 + l31;
    const bool mok = m < M, nok = n < N;
    const uint16_t* const pa = P + (size_t)min(m, M - 1) * tp + 8 * hh;
    const uint16_t* const pb = Q + (size_t)min(n, N - 1) * tp + 8 * hh;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (long long t = t0; t < t1; t += 64) {
        u32x4 av[4], bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            av[s] = *(const u32x4*)(pa + t + 16 * s);
            bv[s] = *(const u32x4*)(pb + t + 16 * s);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, mok ? av[s] : zero4), __builtin_bit_cast(bf16x8, nok ? bv[s] : zero4),
                                                          acc, 0, 0, 0);
    }
    float* const out = planes + (size_t)blockIdx.y * plane_size + (which ? (size_t)0 : o_dw2);
    if (nok) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mo = m0 + mt * 32 + f16b_acc_row(r, hh);
            if (mo < M) out[(size_t)mo * N + n] = acc[r];
        }
    }
}

// ---- db1, db2, dscale: column sums over the chunk in double sub-sums ---------------------------------------------------------------------
// blocks 0 .. ceil(hidden / 32) - 1: db1 of 32 hidden columns from dzhT (8 consecutive lanes read 8 consecutive tokens of a column);
// the blocks behind them: db2 and dscale of 32 columns of dout (32 consecutive lanes read 32 consecutive columns of a token)
template <typename T>
__global__ __launch_bounds__(256) void ffn16_bwd_sums_kernel(const uint16_t* __restrict__ dzhT, long long tp, const T* __restrict__ g, long long n1,
                                                             long long gs0, long long gs1, const T* __restrict__ ys, const T* __restrict__ scale,
                                                             long long ntok, int D, int H, DropoutParams drop, float* __restrict__ planes,
                                                             size_t plane_size, size_t o_db1, size_t o_db2, size_t o_dscale)
{
    __shared__ double sub[2][FFN_BWD_SUBSUMS][32];
    const int tid = threadIdx.x;
    const int nb1 = (H + 31) / 32;
    const int chunk = blockIdx.y;
    const long long r_begin = (long long)chunk * FFN_BWD_ROWS, r_end = min(ntok, r_begin + FFN_BWD_ROWS);
    float* const plane = planes + (size_t)chunk * plane_size;
    if ((int)blockIdx.x < nb1) {
        const int q = tid & 7, cl = tid >> 3;
        const int col = blockIdx.x * 32 + cl;
        double t = 0.0;
        if (col < H)
            for (long long i = r_begin + q; i < r_end; i += FFN_BWD_SUBSUMS) t += (double)bf16_to_float(dzhT[(size_t)col * tp + i]);
        sub[0][q][cl] = t;
        __syncthreads();
        if (q == 0 && col < H) {
            double s = sub[0][0][cl];
#pragma unroll
            for (int u = 1; u < FFN_BWD_SUBSUMS; ++u) s += sub[0][u][cl];
            plane[o_db1 + col] = (float)s;
        }
    } else {
        const int cl = tid & 31, q = tid >> 5;
        const int n = ((int)blockIdx.x - nb1) * 32 + cl;
        double t2 = 0.0, ts = 0.0;
        if (n < D) {
            const float sc = to_f32(scale[n]);
            for (long long i = r_begin + q; i < r_end; i += FFN_BWD_SUBSUMS) {
                uint32_t w[4] = {0u, 0u, 0u, 0u};
                if (drop.on[1]) dropout_draws(drop.seed, 1u, (unsigned long long)i >> 2, (uint32_t)n, w);
                const uint32_t draw = f16b_pick(w, (int)(i & 3));
                const long long i0 = i / n1;
                const float gv = to_f32(g[i0 * gs0 + (i - i0 * n1) * gs1 + n]);
                t2 += (double)dy_of(gv, sc, drop, draw);
                ts += (double)(gv * masked(drop, 1, draw, to_f32(ys[(size_t)i * D + n])));
            }
        }
        sub[0][q][cl] = t2;
        sub[1][q][cl] = ts;
        __syncthreads();
        if (q == 0 && n < D) {
            double s2 = sub[0][0][cl], ss = sub[1][0][cl];
#pragma unroll
            for (int u = 1; u < FFN_BWD_SUBSUMS; ++u) { s2 += sub[0][u][cl]; ss += sub[1][u][cl]; }
            plane[o_db2 + n] = (float)s2;
            plane[o_dscale + n] = (float)ss;
        }
    }
}

// ---- the planes added in ascending chunk order, one rounding to T --------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void ffn16_bwd_reduce_kernel(const float* __restrict__ planes, size_t plane_size, int nch, size_t n_w, int D, int H,
                                                               T* __restrict__ dW1, T* __restrict__ db1, T* __restrict__ dW2, T* __restrict__ db2,
                                                               T* __restrict__ dscale)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t e1 = n_w, e2 = e1 + H, e3 = e2 + n_w, e4 = e3 + D, e5 = e4 + D;   // (the sections are contiguous from the start of a plane)
    if (idx >= e5) return;
    float t = planes[idx];
    for (int c = 1; c < nch; ++c) t += planes[(size_t)c * plane_size + idx];
    if (idx < e1) store_as(dW1 + idx, t);
    else if (idx < e2) store_as(db1 + (idx - e1), t);
    else if (idx < e3) store_as(dW2 + (idx - e2), t);
    else if (idx < e4) store_as(db2 + (idx - e3), t);
    else store_as(dscale + (idx - e4), t);
}

template <typename T, int DB>
static void ffn16_bwd_launch_token(const Ffn16BwdTok<T>& a, hipStream_t stream)
{
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)ffn16_bwd_token_kernel<T, DB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_bf16_bwd(DB * 32));
    hipLaunchKernelGGL((ffn16_bwd_token_kernel<T, DB>), dim3((unsigned)((a.ntok + FFN16_ROWS - 1) / FFN16_ROWS)), dim3(256), lds_bytes_bf16_bwd(a.D), stream, a);
}

// the caller (api.hip) has checked the supported set, the pointers, the strides, the saved buffer, the workspace and the token count
template <typename T>
static void ffn16_bwd_launch(const T* dout, const T* x, const void* saved, long long n0, long long n1, long long gs0, long long gs1, long long xs0,
                             long long xs1, long long ds0, long long ds1, int D, int H, const T* W1, const T* W2, const T* scale, float eps,
                             unsigned long long seed, double p1, double p2, T* dx, T* dW1, T* db1, T* dW2, T* db2, T* dscale, void* ws,
                             hipStream_t stream)
{
    const long long ntok = n0 * n1;
    const Ffn16BwdPlan p = ffn16_bwd_plan(ntok, D, H);
    unsigned char* const base = (unsigned char*)ws;
    uint16_t* const W1T = (uint16_t*)(base + p.w1t);
    uint16_t* const W2T = (uint16_t*)(base + p.w2t);
    uint16_t* const xhT = (uint16_t*)(base + p.xht);
    uint16_t* const dyhT = (uint16_t*)(base + p.dyht);
    uint16_t* const dzhT = (uint16_t*)(base + p.dzht);
    uint16_t* const ahT = (uint16_t*)(base + p.aht);
    float* const planes = (float*)(base + p.planes);
    const uint16_t* const zs = (const uint16_t*)saved;
    const T* const ys = (const T*)((const unsigned char*)saved + train_saved_ys_offset(ntok, H));
    const DropoutParams drop = attr_heads::dropout_params(seed, p1, p2);

    hipLaunchKernelGGL(ffn16_bwd_prep_kernel<T>, dim3((unsigned)((2 * H * D + 255) / 256)), dim3(256), 0, stream, W1, W2, D, H, W1T, W2T);

    constexpr long long EL = 16 / sizeof(T);
    Ffn16BwdTok<T> a;
    a.x = x; a.g = dout; a.dx = dx;
    a.n1 = n1; a.xs0 = xs0; a.xs1 = xs1; a.gs0 = gs0; a.gs1 = gs1; a.ds0 = ds0; a.ds1 = ds1; a.ntok = ntok; a.tp = p.tp;
    a.D = D; a.H = H;
    a.W1T = W1T; a.W2T = W2T; a.scale = scale; a.zs = zs;
    a.eps = eps;
    a.vec = ((((uintptr_t)x | (uintptr_t)dout) & 15) == 0) && ((xs0 | xs1 | gs0 | gs1) & (EL - 1)) == 0;
    a.ovec = ((((uintptr_t)x | (uintptr_t)dout | (uintptr_t)dx) & (4 * sizeof(T) - 1)) == 0) && ((xs0 | xs1 | gs0 | gs1 | ds0 | ds1) & 3) == 0;
    a.drop = drop;
    a.xhT = xhT; a.dyhT = dyhT; a.dzhT = dzhT; a.ahT = ahT;
#define SEMICRF_FFN16B_CASE(N) case N: ffn16_bwd_launch_token<T, N>(a, stream); break
    switch ((D + 31) / 32) {
        SEMICRF_FFN16B_CASE(1); SEMICRF_FFN16B_CASE(2); SEMICRF_FFN16B_CASE(3); SEMICRF_FFN16B_CASE(4);
        SEMICRF_FFN16B_CASE(5); SEMICRF_FFN16B_CASE(6); SEMICRF_FFN16B_CASE(7); SEMICRF_FFN16B_CASE(8);
    }
#undef SEMICRF_FFN16B_CASE

    const int tD = (D + 63) / 64, tH = (H + 63) / 64;
    hipLaunchKernelGGL(ffn16_bwd_dw_kernel, dim3((unsigned)(tD * tH), (unsigned)p.nch, 2), dim3(256), 0, stream, dyhT, ahT, dzhT, xhT, p.tp, D, H, planes,
                       p.plane_size, p.o_dw2);
    hipLaunchKernelGGL(ffn16_bwd_sums_kernel<T>, dim3((unsigned)((H + 31) / 32 + (D + 31) / 32), (unsigned)p.nch), dim3(256), 0, stream, dzhT, p.tp, dout,
                       n1, gs0, gs1, ys, scale, ntok, D, H, drop, planes, p.plane_size, p.o_db1, p.o_db2, p.o_dscale);
    const size_t total = 2 * (size_t)H * D + H + 2 * (size_t)D;
    hipLaunchKernelGGL(ffn16_bwd_reduce_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, planes, p.plane_size, p.nch,
                       (size_t)H * D, D, H, dW1, db1, dW2, db2, dscale);
}

void launch_ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, long long n0, long long n1, long long gs0, long long gs1,
                                  long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const uint16_t* W1, const uint16_t* W2,
                                  const uint16_t* scale, float eps, unsigned long long seed, double p1, double p2, uint16_t* dx, uint16_t* dW1,
                                  uint16_t* db1, uint16_t* dW2, uint16_t* db2, uint16_t* dscale, void* ws, hipStream_t stream)
{
    ffn16_bwd_launch<uint16_t>(dout, x, saved, n0, n1, gs0, gs1, xs0, xs1, ds0, ds1, D, H, W1, W2, scale, eps, seed, p1, p2, dx, dW1, db1, dW2, db2,
                               dscale, ws, stream);
}

void launch_ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, long long n0, long long n1, long long gs0, long long gs1,
                                        long long xs0, long long xs1, long long ds0, long long ds1, int D, int H, const float* W1, const float* W2,
                                        const float* scale, float eps, unsigned long long seed, double p1, double p2, float* dx, float* dW1,
                                        float* db1, float* dW2, float* db2, float* dscale, void* ws, hipStream_t stream)
{
    ffn16_bwd_launch<float>(dout, x, saved, n0, n1, gs0, gs1, xs0, xs1, ds0, ds1, D, H, W1, W2, scale, eps, seed, p1, p2, dx, dW1, db1, dW2, db2, dscale,
                            ws, stream);
}

}  // namespace semicrf
