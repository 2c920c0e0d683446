// attention_bf16_bwd.hip -- semicrf_axial_attention_bf16_bwd: dq, dk, dv of the bf16 axial attention (attention_bf16.hip) from q, k, v and
// the cotangent dout, all bfloat16, TOKEN-MAJOR with three element strides per tensor.  Nothing is saved by the forward and `out` is not
// an input: the scores, their maximum, the rounded weights and their sum are recomputed with the forward's own chain, and D_i is the
// softmax form sum_j P dP (attention_bf16_math.h has the chain).  All five products run on v_mfma_f32_32x32x16_bf16.
//
// Workgroup = one (sequence, head), 4 waves, so dk and dv are complete inside it: no atomics, nothing reduced across workgroups.
//   pass A   query-owned.  LDS holds K and V token-major (rows of 16 KS + 8 bf16, as the forward's K) and K^T (rows of 32 nt + 4, as the
//            forward's V^T).  Wave w takes the query tiles w, w + 4, ..: Q and dout fragments straight from memory (a lane = one query),
//            S^T = K Q^T block kt on its own accumulator, * scale, mask, maximum, exp, the rounded weights two per dword and their sum
//            S0 + S1 -- the forward, instruction for instruction.  Then the key blocks are walked twice with dP^T = V dout^T on ONE
//            accumulator: the first walk sums D = D0 + D1 (a lane's registers ascending, then the other half wave: the order of `sum`),
//            the second forms dS = P (dP - D), rounds pairs with v_cvt_pk_bf16_f32, and those dwords ARE the B operand of
//            dq^T = K^T dS^T (key order kstep_key; A = two 8-byte reads of a K^T row).  dP twice costs 2 KS matrix instructions per
//            block and saves the 16 NKT registers that would hold it.  m, sum, D of the tile go to LDS for pass B.
//   barrier, then Q, dout, Q^T, dout^T of the head replace K, V, K^T in LDS
//   pass B   key-owned.  Wave w takes the key tiles w, w + 4, ..: K and V fragments from memory (a lane = one key), then walks the query
//            tiles ascending: S = Q K^T and dP = dout V^T (rows = queries; the products commute, so the scores are pass A's), P and dS
//            from the statistics in LDS, rounded pairwise, and the dwords feed dv^T = dout^T P and dk^T = Q^T dS the same way.
//   store    bf16(dq * scale), bf16(dk * scale), bf16(dv): a lane holds four neighbouring columns of its token -- 8-byte stores where
//            the destination allows, 2-byte stores elsewhere.
// Tile sizes depend on Lq, Lk and d alone and every reduction has one order: a sequence's gradients are bit-identical whatever the
// batch, its position in it, the strides and the alignment are.  Rows past Lq / Lk are never loaded or stored; padded keys are masked
// before the maximum (P = dS = 0); a padded query has dout = 0 (D = dS = 0); padded head columns are zeros in registers and LDS.
// LDS (lds_bytes_bf16_bwd): 79 744 B at L = 149, d = 40 (two workgroups per CU), 143 360 B at L = 256, d = 64.
#include "common.h"
#include "launchers.h"
#include "bf16x3.h"
#include "attention_bf16_math.h"

namespace semicrf {

using namespace attention;

struct Att16BwdStrides { long long s0, s1, l; };
struct Att16BwdTensors { Att16BwdStrides q, k, v, g, dq, dk, dv; };

// 8 consecutive bf16 values as four dwords: one 16-byte load, or eight 2-byte loads put together -- the same bits
__device__ __forceinline__ u32x4 att16b_load8(const uint16_t* p, bool vec)
{
    u32x4 x;
    if (vec) {
        x = *(const u32x4*)p;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (unsigned)p[2 * e] | ((unsigned)p[2 * e + 1] << 16);
    }
    return x;
}

// four neighbouring columns of one token, two per dword
__device__ __forceinline__ void att16b_store4(uint16_t* p, unsigned a, unsigned b, bool vec)
{
    if (vec) {
        *(uint2*)p = make_uint2(a, b);
    } else {
        p[0] = (uint16_t)a; p[1] = (uint16_t)(a >> 16);
        p[2] = (uint16_t)b; p[3] = (uint16_t)(b >> 16);
    }
}

__device__ __forceinline__ float att16b_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float att16b_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }

// the fragments of token `row` for the products over the head dimension: k-step s holds the columns 16 s + 8 hh .. + 8; zeros for a
// row past nrows (never loaded) and the columns past d
template <int KS>
__device__ __forceinline__ void att16b_frag(u32x4 (&f)[KS], const uint16_t* base, long long stride_l, int row, int nrows, int d, int hh, bool vec)
{
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int c = 16 * s + 8 * hh;
        f[s] = (u32x4){0u, 0u, 0u, 0u};
        if (row < nrows && c < d) f[s] = att16b_load8(base + (long long)row * stride_l + c, vec);
    }
}

// rows [0, 32 ntiles) of a token-major matrix into LDS rows of 16 KS + KPAD bf16: a thread per (row, 8 columns); zeros past nrows and d
template <int KS>
__device__ __forceinline__ void att16b_stage_rows(uint16_t* dst, const uint16_t* src, long long stride_l, int nrows, int ntiles, int d, int tid, bool vec)
{
    constexpr int LDK = 16 * KS + ATT16_KPAD;
    for (int idx = tid; idx < ntiles * ATT_TILE * 2 * KS; idx += 256) {
        const int row = idx / (2 * KS), c = 8 * (idx - row * (2 * KS));
        u32x4 x = {0u, 0u, 0u, 0u};
        if (row < nrows && c < d) x = att16b_load8(src + (long long)row * stride_l + c, vec);
        *(u32x4*)(dst + row * LDK + c) = x;
    }
}

// the same rows transposed, [32 DB columns][ldt]: a thread per (row pair, 8 columns) writes 8 dwords, a row pair of one column each
template <int DB>
__device__ __forceinline__ void att16b_stage_cols(uint16_t* dst, int ldt, const uint16_t* src, long long stride_l, int nrows, int ntiles, int d, int tid, bool vec)
{
    for (int idx = tid; idx < ntiles * (ATT_TILE / 2) * 4 * DB; idx += 256) {
        const int pair = idx / (4 * DB), c = 8 * (idx - pair * (4 * DB));
        u32x4 x0 = {0u, 0u, 0u, 0u}, x1 = {0u, 0u, 0u, 0u};
        if (c < d) {
            if (2 * pair < nrows) x0 = att16b_load8(src + (long long)(2 * pair) * stride_l + c, vec);
            if (2 * pair + 1 < nrows) x1 = att16b_load8(src + (long long)(2 * pair + 1) * stride_l + c, vec);
        }
        unsigned* const p = (unsigned*)(dst + c * ldt) + pair;                  // ldt is even: a row pair is one dword
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            p[(2 * e) * (ldt / 2)] = (x0[e] & 0xffffu) | (x1[e] << 16);
            p[(2 * e + 1) * (ldt / 2)] = (x0[e] >> 16) | (x1[e] & 0xffff0000u);
        }
    }
}

// the A operand of a product that sums over the tokens of block `blk`, k-step s: row `row` of a transposed image at the tokens
// kstep_key(s, 0 .. 3, hh) and kstep_key(s, 4 .. 7, hh) -- two 8-byte reads
__device__ __forceinline__ bf16x8 att16b_tr_operand(const uint16_t* img, int ldt, int row, int blk, int s, int hh)
{
    const uint16_t* p = img + row * ldt + blk * ATT_TILE + 16 * s + 4 * hh;
    const uint2 lo = *(const uint2*)p, hi = *(const uint2*)(p + 8);
    const u32x4 a = {lo.x, lo.y, hi.x, hi.y};
    return __builtin_bit_cast(bf16x8, a);
}

// q, k, v, dout are not __restrict__ (attention.hip: an invariant load would be hoisted out of the tile loop into registers)
template <int NKT, int KS>
__global__ __launch_bounds__(256, 2) void axial_attention_bf16_bwd_kernel(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout,
                                                                          uint16_t* dq, uint16_t* dk, uint16_t* dv, long long n1, int Lq, int Lk,
                                                                          int H, int d, Att16BwdTensors st, float scale, int vec, int ovec)
{
    constexpr int DB = KS <= 2 ? 1 : 2;                   // 32-column blocks of a gradient
    constexpr int LDK = 16 * KS + ATT16_KPAD;             // bf16 per row of a token-major image
    extern __shared__ __attribute__((aligned(16))) unsigned char att16b_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int nqt = (Lq + ATT_TILE - 1) / ATT_TILE;
    const int ntl = nqt > NKT ? nqt : NKT;
    const int ldt = ntl * ATT_TILE + ATT16_VPAD;          // bf16 per row of a transposed image
    uint16_t* const Xr = (uint16_t*)att16b_lds;           // pass A: K      pass B: Q         [ntl * 32][LDK]
    uint16_t* const Yr = Xr + ntl * ATT_TILE * LDK;       // pass A: V      pass B: dout
    uint16_t* const Xt = Yr + ntl * ATT_TILE * LDK;       // pass A: K^T    pass B: Q^T       [DB * 32][ldt]
    uint16_t* const Yt = Xt + DB * 32 * ldt;              //                pass B: dout^T
    float* const Ms = (float*)(Yt + DB * 32 * ldt);       // [ntl * 32] row maxima, row sums, D
    float* const Ss = Ms + ntl * ATT_TILE;
    float* const Ds = Ss + ntl * ATT_TILE;

    const unsigned blk = blockIdx.x, useq = blk / (unsigned)H;   // n0 n1 H < 2^31: 32-bit divisions
    const int h = (int)(blk - useq * (unsigned)H);
    const long long s0 = useq / (unsigned)n1, s1 = useq - (unsigned)s0 * (unsigned)n1;
    const long long hd = (long long)h * d;
    const uint16_t* const qb = q + s0 * st.q.s0 + s1 * st.q.s1 + hd;
    const uint16_t* const kb = k + s0 * st.k.s0 + s1 * st.k.s1 + hd;
    const uint16_t* const vb = v + s0 * st.v.s0 + s1 * st.v.s1 + hd;
    const uint16_t* const gb = dout + s0 * st.g.s0 + s1 * st.g.s1 + hd;
    uint16_t* const dqb = dq ? dq + s0 * st.dq.s0 + s1 * st.dq.s1 + hd : nullptr;     // a gradient that is not wanted: a null pointer
    uint16_t* const dkb = dk ? dk + s0 * st.dk.s0 + s1 * st.dk.s1 + hd : nullptr;
    uint16_t* const dvb = dv ? dv + s0 * st.dv.s0 + s1 * st.dv.s1 + hd : nullptr;

    att16b_stage_rows<KS>(Xr, kb, st.k.l, Lk, NKT, d, tid, vec);
    att16b_stage_rows<KS>(Yr, vb, st.v.l, Lk, NKT, d, tid, vec);
    if (dq != nullptr) att16b_stage_cols<DB>(Xt, ldt, kb, st.k.l, Lk, NKT, d, tid, vec);
    __syncthreads();

    // ==== pass A: this wave's query tiles -- the statistics of every query, and dq ========================================================
    for (int qt = wave; qt < nqt; qt += 4) {
        int lk = Lk;
        asm volatile("" : "+s"(lk));                               // the key masks as this iteration's own: not hoisted into registers
        const int i = qt * ATT_TILE + l31;                         // this lane's query
        unsigned pk[NKT][8];                                       // the rounded weights, two per dword, in register order
        float mx = SEMICRF_NEG_INF, sum = 0.0f;
        {
            u32x4 qf[KS];
            att16b_frag<KS>(qf, qb, st.q.l, i, Lq, d, hh, vec);
            // ---- scores and softmax: the forward's --------------------------------------------------------------------------------------
            f32x16 acc[NKT];
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[kt][r] = 0.0f;
#pragma unroll
                for (int s = 0; s < KS; ++s) {
                    const u32x4 ka = *(const u32x4*)(Xr + (kt * ATT_TILE + l31) * LDK + 16 * s + 8 * hh);
                    acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ka), __builtin_bit_cast(bf16x8, qf[s]), acc[kt], 0, 0, 0);
                }
            }
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const bool real = kt * ATT_TILE + (r & 3) + 8 * (r >> 2) + 4 * hh < lk;
                    acc[kt][r] = real ? acc[kt][r] * scale : SEMICRF_NEG_INF;
                    mx = fmaxf(mx, acc[kt][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32));                    // key 0 is real: the maximum is a true score
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const float p0 = expf(acc[kt][r] - mx), p1 = expf(acc[kt][r + 1] - mx);      // a masked key: exp(-inf) = +0 exactly
                    const unsigned u = cvt_pk_bf16(p0, p1);
                    pk[kt][r >> 1] = u;
                    sum += att16b_lo(u);
                    sum += att16b_hi(u);
                }
            const float other = __shfl_xor(sum, 32);
            sum = hh == 0 ? sum + other : other + sum;             // S0 + S1 in both halves
        }

        // ---- D = sum_j P dP: the key blocks once, dP^T = V dout^T on one accumulator --------------------------------------------------
        u32x4 gf[KS];
        att16b_frag<KS>(gf, gb, st.g.l, i, Lq, d, hh, vec);
        float D = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x16 dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 va = *(const u32x4*)(Yr + (kt * ATT_TILE + l31) * LDK + 16 * s + 8 * hh);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, gf[s]), dp, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const unsigned u = pk[kt][r >> 1];
                D += (att16b_lo(u) / sum) * dp[r];
                D += (att16b_hi(u) / sum) * dp[r + 1];
            }
        }
        {
            const float other = __shfl_xor(D, 32);
            D = hh == 0 ? D + other : other + D;                   // D0 + D1 in both halves
        }
        if (hh == 0) { Ms[i] = mx; Ss[i] = sum; Ds[i] = D; }
        if (dq == nullptr) continue;

        // ---- the key blocks again: dS = P (dP - D) rounded pairwise is the B operand of dq^T = K^T dS^T --------------------------------
        int ldb = LDK;                                             // the second walk's own row length: its dP is formed again, not
        asm volatile("" : "+s"(ldb));                              // kept in 16 NKT registers from the first
        f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            f32x16 dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[r] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 va = *(const u32x4*)(Yr + (kt * ATT_TILE + l31) * ldb + 16 * s + 8 * hh);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, gf[s]), dp, 0, 0, 0);
            }
            unsigned dsb[8];
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const unsigned u = pk[kt][r >> 1];
                const float ds0 = (att16b_lo(u) / sum) * (dp[r] - D), ds1 = (att16b_hi(u) / sum) * (dp[r + 1] - D);
                dsb[r >> 1] = cvt_pk_bf16(ds0, ds1);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u32x4 pb = {dsb[4 * s], dsb[4 * s + 1], dsb[4 * s + 2], dsb[4 * s + 3]};
#pragma unroll
                for (int db = 0; db < DB; ++db)
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att16b_tr_operand(Xt, ldt, db * 32 + l31, kt, s, hh),
                                                                    __builtin_bit_cast(bf16x8, pb), o[db], 0, 0, 0);
            }
        }
        if (i < Lq) {
            uint16_t* const di = dqb + (long long)i * st.dq.l;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = db * 32 + 8 * g + 4 * hh;
                    if (col < d)                                     // d is a multiple of 8 and col of 4: all four columns or none
                        att16b_store4(di + col, cvt_pk_bf16(o[db][4 * g] * scale, o[db][4 * g + 1] * scale),
                                      cvt_pk_bf16(o[db][4 * g + 2] * scale, o[db][4 * g + 3] * scale), (ovec & 1) != 0);
                }
        }
    }
    if (dk == nullptr && dv == nullptr) return;

    // ==== pass B: Q and dout replace K and V; this wave's key tiles -- dk and dv =========================================================
    __syncthreads();                                               // every wave has read K, V and K^T, and every statistic is in LDS
    att16b_stage_rows<KS>(Xr, qb, st.q.l, Lq, nqt, d, tid, vec);
    att16b_stage_rows<KS>(Yr, gb, st.g.l, Lq, nqt, d, tid, vec);
    if (dk != nullptr) att16b_stage_cols<DB>(Xt, ldt, qb, st.q.l, Lq, nqt, d, tid, vec);
    if (dv != nullptr) att16b_stage_cols<DB>(Yt, ldt, gb, st.g.l, Lq, nqt, d, tid, vec);
    __syncthreads();

    for (int kt = wave; kt < NKT; kt += 4) {
        const int j = kt * ATT_TILE + l31;                         // this lane's key
        u32x4 kf[KS], vf[KS];
        att16b_frag<KS>(kf, kb, st.k.l, j, Lk, d, hh, vec);
        att16b_frag<KS>(vf, vb, st.v.l, j, Lk, d, hh, vec);
        f32x16 ak[DB], av[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) { ak[db][r] = 0.0f; av[db][r] = 0.0f; }

        for (int qt = 0; qt < nqt; ++qt) {
            f32x16 sc, dp;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sc[r] = 0.0f; dp[r] = 0.0f; }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 qa = *(const u32x4*)(Xr + (qt * ATT_TILE + l31) * LDK + 16 * s + 8 * hh);
                const u32x4 ga = *(const u32x4*)(Yr + (qt * ATT_TILE + l31) * LDK + 16 * s + 8 * hh);
                sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, qa), __builtin_bit_cast(bf16x8, kf[s]), sc, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ga), __builtin_bit_cast(bf16x8, vf[s]), dp, 0, 0, 0);
            }
            unsigned pb[8], dsb[8];                                // Ph and dSh of the block, two queries per dword, in register order
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const int row = qt * ATT_TILE + (r & 3) + 8 * (r >> 2) + 4 * hh;      // register r + 1 holds the query row + 1
                const float p0 = j < Lk ? expf(sc[r] * scale - Ms[row]) : 0.0f;
                const float p1 = j < Lk ? expf(sc[r + 1] * scale - Ms[row + 1]) : 0.0f;
                const unsigned u = cvt_pk_bf16(p0, p1);
                const float P0 = att16b_lo(u) / Ss[row], P1 = att16b_hi(u) / Ss[row + 1];
                pb[r >> 1] = cvt_pk_bf16(P0, P1);
                dsb[r >> 1] = cvt_pk_bf16(P0 * (dp[r] - Ds[row]), P1 * (dp[r + 1] - Ds[row + 1]));
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u32x4 pv = {pb[4 * s], pb[4 * s + 1], pb[4 * s + 2], pb[4 * s + 3]};
                const u32x4 sv = {dsb[4 * s], dsb[4 * s + 1], dsb[4 * s + 2], dsb[4 * s + 3]};
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    if (dv != nullptr)
                        av[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att16b_tr_operand(Yt, ldt, db * 32 + l31, qt, s, hh),
                                                                         __builtin_bit_cast(bf16x8, pv), av[db], 0, 0, 0);
                    if (dk != nullptr)
                        ak[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(att16b_tr_operand(Xt, ldt, db * 32 + l31, qt, s, hh),
                                                                         __builtin_bit_cast(bf16x8, sv), ak[db], 0, 0, 0);
                }
            }
        }
        if (j < Lk) {
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = db * 32 + 8 * g + 4 * hh;
                    if (col < d) {
                        if (dk != nullptr)
                            att16b_store4(dkb + (long long)j * st.dk.l + col, cvt_pk_bf16(ak[db][4 * g] * scale, ak[db][4 * g + 1] * scale),
                                          cvt_pk_bf16(ak[db][4 * g + 2] * scale, ak[db][4 * g + 3] * scale), (ovec & 2) != 0);
                        if (dv != nullptr)
                            att16b_store4(dvb + (long long)j * st.dv.l + col, cvt_pk_bf16(av[db][4 * g], av[db][4 * g + 1]),
                                          cvt_pk_bf16(av[db][4 * g + 2], av[db][4 * g + 3]), (ovec & 4) != 0);
                    }
                }
        }
    }
}

template <int NKT, int KS>
static void att16b_launch_one(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk, uint16_t* dv,
                              long long nseq, long long n1, int Lq, int Lk, int H, int d, const Att16BwdTensors& st, int vec, int ovec,
                              hipStream_t stream)
{
    static PerDeviceOnce once;
    if (once.first())                                              // the instantiation's largest: every query count, Lk and d rounded up
        (void)hipFuncSetAttribute((const void*)axial_attention_bf16_bwd_kernel<NKT, KS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes_bf16_bwd(ATT_MAX_L, NKT * ATT_TILE, 16 * KS));
    hipLaunchKernelGGL((axial_attention_bf16_bwd_kernel<NKT, KS>), dim3((unsigned)(nseq * H)), dim3(256), lds_bytes_bf16_bwd(Lq, Lk, d), stream, q, k,
                       v, dout, dq, dk, dv, n1, Lq, Lk, H, d, st, scale_of(d), vec, ovec);
}

template <int KS>
static void att16b_launch_kt(int nkt, const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk,
                             uint16_t* dv, long long nseq, long long n1, int Lq, int Lk, int H, int d, const Att16BwdTensors& st, int vec, int ovec,
                             hipStream_t stream)
{
#define SEMICRF_ATT16B_CASE(N) case N: att16b_launch_one<N, KS>(q, k, v, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, vec, ovec, stream); break
    switch (nkt) {
        SEMICRF_ATT16B_CASE(1); SEMICRF_ATT16B_CASE(2); SEMICRF_ATT16B_CASE(3); SEMICRF_ATT16B_CASE(4);
        SEMICRF_ATT16B_CASE(5); SEMICRF_ATT16B_CASE(6); SEMICRF_ATT16B_CASE(7); SEMICRF_ATT16B_CASE(8);
    }
#undef SEMICRF_ATT16B_CASE
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and n0 n1 H < 2^31, and that a gradient is wanted;
// strides: q, k, v, dout, dq, dk, dv x (s0, s1, l)
void launch_axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk,
                                     uint16_t* dv, long long n0, long long n1, int Lq, int Lk, int H, int d, const long long* s, hipStream_t stream)
{
    Att16BwdTensors st;
    Att16BwdStrides* each[7] = {&st.q, &st.k, &st.v, &st.g, &st.dq, &st.dk, &st.dv};
    for (int i = 0; i < 7; ++i) *each[i] = Att16BwdStrides{s[3 * i], s[3 * i + 1], s[3 * i + 2]};
    // 16-byte loads of Q, K, V and dout rows: every base 16-byte aligned and every stride a multiple of eight bf16 (d is a multiple of 8)
    bool vec = ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout) & 15) == 0);
    for (int i = 0; i < 12; ++i) vec = vec && (s[i] & 7) == 0;
    // 8-byte stores of four columns, gradient by gradient (a NULL one is never stored)
    const uint16_t* grads[3] = {dq, dk, dv};
    int ovec = 0;
    for (int g = 0; g < 3; ++g) {
        bool ok = (((uintptr_t)grads[g]) & 7) == 0;
        for (int i = 12 + 3 * g; i < 15 + 3 * g; ++i) ok = ok && (s[i] & 3) == 0;
        ovec |= ok ? 1 << g : 0;
    }
    const int nkt = key_tiles(Lk);
    const long long nseq = n0 * n1;
    switch (dim_steps(d)) {
        case 1: att16b_launch_kt<1>(nkt, q, k, v, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, vec, ovec, stream); break;
        case 2: att16b_launch_kt<2>(nkt, q, k, v, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, vec, ovec, stream); break;
        case 3: att16b_launch_kt<3>(nkt, q, k, v, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, vec, ovec, stream); break;
        default: att16b_launch_kt<4>(nkt, q, k, v, dout, dq, dk, dv, nseq, n1, Lq, Lk, H, d, st, vec, ovec, stream); break;
    }
}

}  // namespace semicrf
