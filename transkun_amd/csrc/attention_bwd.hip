// attention_bwd.hip -- the backward of the backbone's axial attention (attention.hip): dq, dk, dv of
//   out[s, i, h, :] = sum_j softmax_j(q[s,i,h,:] . k[s,j,h,:] / sqrt(d)) v[s,j,h,:]        1 <= Lq, Lk <= 256, d = 8, 16, .. 64
// from q, k, v, out as the forward wrote it, and the cotangent dout.  fp32, TOKEN-MAJOR with three element strides per tensor like the
// forward, so the gradient of the time-axis call lands in the [N, T', F', H d] buffer without a transposed copy.  Nothing is saved by
// the forward: the scores, their maximum, the exponentials and their sum are recomputed with the forward's own chain (attention_math.h).
//
// Workgroup = one (sequence, head), 4 waves, so dk and dv are complete inside it: no atomics, nothing reduced across workgroups.
//   pass A   query-owned.  K and V of the head in LDS, token-major with rows of d + 1 floats.  Wave w takes the query tiles w, w + 4, ..:
//            its Q rows as the B operand straight from memory into registers (a lane = one query, d / 2 values), S^T = K Q^T block kt on
//            its own accumulator exactly as the forward; * scale, mask, maximum, exp, sum = S0 + S1 as the forward.  D_i = dout_i . out_i.
//            m_i, sum_i, D_i of the tile go to LDS for pass B.  Then per key block: dP^T = V dout^T on one accumulator, dS = P (dP - D)
//            in the score block's registers, and those registers ARE the A operand of dq += dS K: register r holds key row(r, 0) in lanes
//            0-31 and key row(r, 1) = row(r, 0) + 4 in lanes 32-63, the two k indices of one v_mfma_f32_32x32x2_f32, with B = the two K
//            rows from LDS.  No LDS round trip; the keys enter dq's chain in the order bwd_order (attention_math.h).
//   barrier, then Q and dout of the head replace K and V in LDS
//   pass B   key-owned.  Wave w takes the key tiles w, w + 4, ..: its K and V rows as B operands from memory into registers, then walks
//            the query tiles ascending: S = Q K^T (rows = queries, a lane = one key; the products q k commute, so the scores carry the
//            bits of pass A), P from the statistics in LDS, dP = dout V^T, dS; dv += P^T dout and dk += dS^T Q with the score block's
//            registers as the A operand again and the two Q / dout rows from LDS as B.  The queries enter in the order bwd_order.
//   store    dq * scale, dk * scale, dv for the rows below Lq / Lk and the columns below d.
// The score blocks are computed twice: the price of fixed orders without atomics.  Tile sizes depend on Lq, Lk and d alone, so a
// sequence's gradients are bit-identical whatever the batch, its position in it and the strides are.
// LDS: 2 * 32 * max(query tiles, key tiles) * (d + 1) + 3 * 256 floats: 56 KB at L = 149, d = 40 (two workgroups per CU), 136 KB at
// the largest shape.  Rows past Lq / Lk are never loaded; padded keys are masked before the maximum; padded head columns are zeros in
// registers; a padded query has dout = 0 and D = 0, so it adds exact zeros to dk and dv.
#include "common.h"
#include "launchers.h"
#include "attention_math.h"

namespace semicrf {

using namespace attention;

typedef float attb_f32x16 __attribute__((ext_vector_type(16)));

struct AttBwdStrides { long long s0, s1, l; };
struct AttBwdTensors { AttBwdStrides q, k, v, o, g, dq, dk, dv; };

__device__ __forceinline__ int attb_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

static size_t attb_lds_bytes(int Lq, int Lk, int d)
{
    const int nt = key_tiles(Lq > Lk ? Lq : Lk);
    return (2 * (size_t)nt * ATT_TILE * (d + 1) + 3 * (size_t)ATT_MAX_L) * sizeof(float);
}

// rows [0, ntiles * 32) x d of a token-major matrix into LDS rows of ld floats, zeros past nrows (those rows are never loaded)
__device__ __forceinline__ void attb_stage(float* dst, int ld, const float* src, long long stride_l, int nrows, int ntiles, int d, int t)
{
    for (int idx = t; idx < ntiles * ATT_TILE * d; idx += 256) {
        const int row = idx / d, c = idx - row * d;
        dst[row * ld + c] = row < nrows ? src[(long long)row * stride_l + c] : 0.0f;
    }
}

// the B operand of a product over the head dimension: row `row` of a token-major matrix, value m = column 2 m + hh; zeros for a row
// past nrows (never loaded) and the columns past d
template <int DB>
__device__ __forceinline__ void attb_load_operand(float (&b)[DB * 16], const float* base, long long stride_l, int row, int nrows, int d, int hh)
{
    // one lane mask for the whole operand: a lane past nrows reads row 0 (always there) and keeps zeros; the column test is uniform
    const bool real = row < nrows;
    const float* p = base + (long long)(real ? row : 0) * stride_l + hh;
#pragma unroll
    for (int m = 0; m < DB * 16; ++m) b[m] = 0.0f;
#pragma unroll
    for (int c8 = 0; c8 < DB * 4; ++c8)                      // d is a multiple of 8: eight columns, four values per lane, at a time
        if (8 * c8 < d) {
#pragma unroll
            for (int m = 4 * c8; m < 4 * c8 + 4; ++m) {
                const float x = p[2 * m];
                b[m] = real ? x : 0.0f;
            }
        }
}

template <int NKT, int DB>
__global__ __launch_bounds__(256, NKT <= 5 ? 2 : 1) void axial_attention_bwd_kernel(const float* q, const float* k, const float* v, const float* out,
                                                                  const float* dout, float* dq, float* dk, float* dv, long long n1,
                                                                  int Lq, int Lk, int H, int d, AttBwdTensors st, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float attb_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int ld = d + 1;
    const int nqt = (Lq + ATT_TILE - 1) / ATT_TILE;
    const int ntl = nqt > NKT ? nqt : NKT;
    float* const Xs = attb_lds;                              // pass A: K [NKT * 32][ld]    pass B: Q [nqt * 32][ld]
    float* const Ys = Xs + ntl * ATT_TILE * ld;              // pass A: V                   pass B: dout
    float* const Ms = Ys + ntl * ATT_TILE * ld;              // [256] row maxima, [256] row sums, [256] D
    float* const Ss = Ms + ATT_MAX_L;
    float* const Ds = Ss + ATT_MAX_L;

    const unsigned blk = blockIdx.x, useq = blk / (unsigned)H;   // n0 n1 H < 2^31: 32-bit divisions
    const int h = (int)(blk - useq * (unsigned)H);
    const long long s0 = useq / (unsigned)n1, s1 = useq - (unsigned)s0 * (unsigned)n1;
    const long long hd = (long long)h * d;
    const float* const qb = q + s0 * st.q.s0 + s1 * st.q.s1 + hd;
    const float* const kb = k + s0 * st.k.s0 + s1 * st.k.s1 + hd;
    const float* const vb = v + s0 * st.v.s0 + s1 * st.v.s1 + hd;
    const float* const ob = out + s0 * st.o.s0 + s1 * st.o.s1 + hd;
    const float* const gb = dout + s0 * st.g.s0 + s1 * st.g.s1 + hd;
    float* const dqb = dq ? dq + s0 * st.dq.s0 + s1 * st.dq.s1 + hd : nullptr;      // a gradient that is not wanted: a null pointer
    float* const dkb = dk ? dk + s0 * st.dk.s0 + s1 * st.dk.s1 + hd : nullptr;
    float* const dvb = dv ? dv + s0 * st.dv.s0 + s1 * st.dv.s1 + hd : nullptr;

    attb_stage(Xs, ld, kb, st.k.l, Lk, NKT, d, tid);
    attb_stage(Ys, ld, vb, st.v.l, Lk, NKT, d, tid);
    __syncthreads();

    // ==== pass A: this wave's query tiles -- the statistics of every query, and dq ========================================================
    for (int qt = wave; qt < nqt; qt += 4) {
        const int i = qt * ATT_TILE + l31;                   // this lane's query
        int lk = Lk;
        asm volatile("" : "+s"(lk));                         // the key masks are this iteration's own: not hoisted into registers
        attb_f32x16 acc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kt][r] = 0.0f;
        {
            float qr[DB * 16];
            attb_load_operand<DB>(qr, qb, st.q.l, i, Lq, d, hh);
            const float* ka = Xs + l31 * ld + hh;
#pragma unroll
            for (int c8 = 0; c8 < DB * 4; ++c8)              // eight columns at a time (d is a multiple of 8)
                if (8 * c8 < d) {
#pragma unroll
                    for (int m = 4 * c8; m < 4 * c8 + 4; ++m)   // instruction m: c = 2 m (lanes 0-31), 2 m + 1 (lanes 32-63), as the forward
#pragma unroll
                        for (int kt = 0; kt < NKT; ++kt)
                            acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kt * ATT_TILE * ld + 2 * m], qr[m], acc[kt], 0, 0, 0);
                }
        }
        // ---- the forward's softmax: * scale, mask, maximum, exp, S0 + S1 ------------------------------------------------------------------
        float mx = SEMICRF_NEG_INF;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool real = kt * ATT_TILE + attb_acc_row(r, hh) < lk;
                acc[kt][r] = real ? acc[kt][r] * scale : SEMICRF_NEG_INF;
                mx = fmaxf(mx, acc[kt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(acc[kt][r] - mx);       // a masked key: exp(-inf) = +0 exactly
                acc[kt][r] = p;
                sum += p;
            }
        {
            const float other = __shfl_xor(sum, 32);
            sum = hh == 0 ? sum + other : other + sum;       // S0 + S1 in both halves
        }
        // ---- D = dout . out, one chain over the head dimension ascending (a padded query: 0) -------------------------------------------
        float D = 0.0f;
        if (i < Lq) {
            const float* go = gb + (long long)i * st.g.l;
            const float* oo = ob + (long long)i * st.o.l;
            for (int c = 0; c < d; ++c) D = fmaf(go[c], oo[c], D);
        }
        if (hh == 0) { Ms[i] = mx; Ss[i] = sum; Ds[i] = D; }
        if (dq == nullptr) continue;

        // ---- per key block: dP^T = V dout^T, dS = P (dP - D), dq += dS K with the block's registers as the A operand ------------------
        // dout's rows are asked for here, after the softmax: requested earlier they would sit in registers through it
        const float* gq = gb;
        asm volatile("" : "+s"(gq));
        float gr[DB * 16];
        attb_load_operand<DB>(gr, gq, st.g.l, i, Lq, d, hh);
        attb_f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            int ldb = ld;                                    // this block's own row length: its 16 K-row addresses are formed here, not
            asm volatile("" : "+s"(ldb));                    // kept in registers from before the tile loop
            attb_f32x16 dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
            const float* va = Ys + (kt * ATT_TILE + l31) * ldb + hh;
#pragma unroll
            for (int c8 = 0; c8 < DB * 4; ++c8)
                if (8 * c8 < d) {
#pragma unroll
                    for (int m = 4 * c8; m < 4 * c8 + 4; ++m) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(va[2 * m], gr[m], dp, 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ds = (acc[kt][r] / sum) * (dp[r] - D);
                const float* krow = Xs + (kt * ATT_TILE + attb_acc_row(r, hh)) * ldb;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int col = db * 32 + l31;
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds, col < d ? krow[col] : 0.0f, o[db], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = qt * ATT_TILE + attb_acc_row(r, hh);
            if (row < Lq) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int col = db * 32 + l31;
                    if (col < d) dqb[(long long)row * st.dq.l + col] = o[db][r] * scale;
                }
            }
        }
    }
    if (dk == nullptr && dv == nullptr) return;

    // ==== pass B: Q and dout replace K and V; this wave's key tiles -- dk and dv =========================================================
    __syncthreads();                                         // every wave has read K and V, and every statistic is in LDS
    attb_stage(Xs, ld, qb, st.q.l, Lq, nqt, d, tid);
    attb_stage(Ys, ld, gb, st.g.l, Lq, nqt, d, tid);
    __syncthreads();

    for (int kt = wave; kt < NKT; kt += 4) {
        const int j = kt * ATT_TILE + l31;                   // this lane's key
        float kr[DB * 16], vr[DB * 16];
        attb_load_operand<DB>(kr, kb, st.k.l, j, Lk, d, hh);
        attb_load_operand<DB>(vr, vb, st.v.l, j, Lk, d, hh);
        attb_f32x16 ak[DB], av[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) { ak[db][r] = 0.0f; av[db][r] = 0.0f; }

        for (int qt = 0; qt < nqt; ++qt) {
            int ldb = ld;                                    // as in pass A: the row addresses are this tile's own
            asm volatile("" : "+s"(ldb));
            attb_f32x16 sc, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = 0.0f; dp[r] = 0.0f; }
            const float* qa = Xs + (qt * ATT_TILE + l31) * ldb + hh;
            const float* ga = Ys + (qt * ATT_TILE + l31) * ldb + hh;
#pragma unroll
            for (int c8 = 0; c8 < DB * 4; ++c8)
                if (8 * c8 < d) {
#pragma unroll
                    for (int m = 4 * c8; m < 4 * c8 + 4; ++m) {
                        sc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[2 * m], kr[m], sc, 0, 0, 0);
                        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * m], vr[m], dp, 0, 0, 0);
                    }
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = qt * ATT_TILE + attb_acc_row(r, hh);
                const float p = j < Lk ? expf(sc[r] * scale - Ms[row]) / Ss[row] : 0.0f;
                const float ds = p * (dp[r] - Ds[row]);
                const float* qrow = Xs + row * ldb;
                const float* grow = Ys + row * ldb;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int col = db * 32 + l31;
                    if (dv != nullptr) av[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(p, col < d ? grow[col] : 0.0f, av[db], 0, 0, 0);
                    if (dk != nullptr) ak[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(ds, col < d ? qrow[col] : 0.0f, ak[db], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = kt * ATT_TILE + attb_acc_row(r, hh);
            if (row < Lk) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int col = db * 32 + l31;
                    if (col < d) {
                        if (dk != nullptr) dkb[(long long)row * st.dk.l + col] = ak[db][r] * scale;
                        if (dv != nullptr) dvb[(long long)row * st.dv.l + col] = av[db][r];
                    }
                }
            }
        }
    }
}

template <int NKT, int DB>
static void attb_launch_one(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk, float* dv,
                            long long nseq, long long n1, int Lq, int Lk, int H, int d, const AttBwdTensors& st, hipStream_t stream)
{
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)axial_attention_bwd_kernel<NKT, DB>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)attb_lds_bytes(ATT_MAX_L, ATT_MAX_L, DB * 32));
    hipLaunchKernelGGL((axial_attention_bwd_kernel<NKT, DB>), dim3((unsigned)(nseq * H)), dim3(256), attb_lds_bytes(Lq, Lk, d), stream, q, k, v,
                       out, dout, dq, dk, dv, n1, Lq, Lk, H, d, st, scale_of(d));
}

template <int DB>
static void attb_launch_kt(int nkt, const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk,
                           float* dv, long long nseq, long long n1, int Lq, int Lk, int H, int d, const AttBwdTensors& st, hipStream_t stream)
{
#define SEMICRF_ATTB_CASE(N) case N: attb_launch_one<N, DB>(q, k, v, out, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, stream); break
    switch (nkt) {
        SEMICRF_ATTB_CASE(1); SEMICRF_ATTB_CASE(2); SEMICRF_ATTB_CASE(3); SEMICRF_ATTB_CASE(4);
        SEMICRF_ATTB_CASE(5); SEMICRF_ATTB_CASE(6); SEMICRF_ATTB_CASE(7); SEMICRF_ATTB_CASE(8);
    }
#undef SEMICRF_ATTB_CASE
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and n0 n1 H < 2^31;
// strides: q, k, v, out, dout, dq, dk, dv x (s0, s1, l)
void launch_axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk, float* dv,
                                long long n0, long long n1, int Lq, int Lk, int H, int d, const long long* s, hipStream_t stream)
{
    AttBwdTensors st;
    AttBwdStrides* each[8] = {&st.q, &st.k, &st.v, &st.o, &st.g, &st.dq, &st.dk, &st.dv};
    for (int i = 0; i < 8; ++i) *each[i] = AttBwdStrides{s[3 * i], s[3 * i + 1], s[3 * i + 2]};
    const int nkt = key_tiles(Lk);
    if (d <= 32) attb_launch_kt<1>(nkt, q, k, v, out, dout, dq, dk, dv, n0 * n1, n1, Lq, Lk, H, d, st, stream);
    else attb_launch_kt<2>(nkt, q, k, v, out, dout, dq, dk, dv, n0 * n1, n1, Lq, Lk, H, d, st, stream);
}

}  // namespace semicrf
