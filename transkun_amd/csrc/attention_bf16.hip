// attention_bf16.hip -- semicrf_axial_attention_bf16: the axial attention of attention.hip for bfloat16 tensors, forward only.
//   out[s, i, h, :] = bf16(sum_j bf16(exp(s_ij - m_i)) v[s,j,h,:] / sum_j bf16(exp(s_ij - m_i)))      s_ij = q[s,i,h,:] . k[s,j,h,:] / sqrt(d)
// The contract is attention.hip's (token-major, three element strides per tensor, 1 <= Lq, Lk <= 256, d = 8, 16, .. 64); the chain of
// operations is attention_bf16_math.h's.
//
// Workgroup = one (sequence, head), 4 waves.  All of them stage the head's K and V into LDS once:
//   K    [32 NKT keys][16 KS + 8] bf16, token-major as in memory; zeros for the keys past Lk and the columns past d
//   V^T  [32 DB columns][32 NKT + 4] bf16: a thread takes 8 columns of two neighbouring keys and writes 8 dwords (a key pair of one
//        column each); zeros for the keys past Lk (they meet an exact-zero weight: 0 * 0, never 0 * NaN)
// Wave w then takes the query tiles w, w + 4, .. of 32 queries on its own, with no further LDS writes and no barrier:
//   Q        the lane's fragments straight from memory: lane (r, hh) holds q[query r][16 s + 8 hh .. + 8] for k-step s -- 16 bytes
//   scores   S^T = K Q^T, block kt (32 keys x 32 queries) on its own accumulator: v_mfma_f32_32x32x16_bf16 with A = 8 consecutive bf16
//            of K row (kt, r) from LDS, B = the Q fragment.  A lane holds ONE query's scores: 16 keys per block and half wave
//   softmax  * scale, keys past Lk -inf BEFORE the maximum; maximum over the lane's registers and the other half wave's; p = expf(s - m);
//            pairs of p rounded to bf16 (v_cvt_pk_bf16_f32), and the ROUNDED values summed: registers ascending, then S0 + S1
//   P V      out^T = V^T P^T: the packed registers 8 s .. 8 s + 7 of block kt ARE the B fragment of k-step (kt, s) -- no LDS, no lane
//            movement.  Element j of half wave hh is key kstep_key(s, j, hh) = 16 s + 8 (j >> 2) + 4 hh + (j & 3) of the block, so
//            the A fragment takes V^T[column r] at the keys 16 s + 4 hh .. + 3 and 16 s + 8 + 4 hh .. + 3: two 8-byte LDS reads
//   store    o / sum rounded to bf16; a lane holds its query's columns 8 g + 4 hh .. + 3: 8-byte stores where `out` allows, 2-byte
//            stores elsewhere
// Tile sizes depend on Lk and d alone, there are no atomics and every reduction has one order: a sequence's result is bit-identical
// whatever the batch, its position in it, the strides and the alignment are.  LDS (attention_bf16_math.h: lds_bytes_bf16): 38 KB at
// L = 149, d = 40; 69 KB at L = 256, d = 64.
#include "common.h"
#include "launchers.h"
#include "bf16x3.h"
#include "attention_bf16_math.h"

namespace semicrf {

using namespace attention;

struct Att16Strides { long long s0, s1, l; };

// 8 consecutive bf16 values as four dwords: one 16-byte load, or eight 2-byte loads put together -- the same bits
__device__ __forceinline__ u32x4 att16_load8(const uint16_t* p, bool vec)
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

// v and out are not __restrict__ (attention.hip: an invariant load would be hoisted out of the tile loop into registers)
template <int NKT, int KS>
__global__ __launch_bounds__(256, 2) void axial_attention_bf16_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ k, const uint16_t* v,
                                                                      uint16_t* out, long long n1, int Lq, int Lk, int H, int d, Att16Strides sq,
                                                                      Att16Strides sk, Att16Strides sv, Att16Strides so, float scale, int vec, int ovec)
{
    constexpr int DB = KS <= 2 ? 1 : 2;                   // 32-column blocks of the output
    constexpr int LDK = 16 * KS + ATT16_KPAD;             // bf16 per K row
    constexpr int LDV = NKT * ATT_TILE + ATT16_VPAD;      // bf16 per V^T row
    extern __shared__ __attribute__((aligned(16))) unsigned char att16_lds[];
    uint16_t* const Ks = (uint16_t*)att16_lds;                               // [NKT * 32][LDK]
    uint16_t* const Vt = Ks + NKT * ATT_TILE * LDK;                           // [DB * 32][LDV]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;

    const unsigned blk = blockIdx.x, useq = blk / (unsigned)H;   // n0 n1 H < 2^31: 32-bit divisions
    const int h = (int)(blk - useq * (unsigned)H);
    const long long s0 = useq / (unsigned)n1, s1 = useq - (unsigned)s0 * (unsigned)n1;
    const uint16_t* const qb = q + s0 * sq.s0 + s1 * sq.s1 + (long long)h * d;
    const uint16_t* const kb = k + s0 * sk.s0 + s1 * sk.s1 + (long long)h * d;
    const uint16_t* const vb = v + s0 * sv.s0 + s1 * sv.s1 + (long long)h * d;
    uint16_t* const ob = out + s0 * so.s0 + s1 * so.s1 + (long long)h * d;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- K: a thread per (key, 8 columns) ---------------------------------------------------------------------------------------------
    for (int idx = tid; idx < NKT * ATT_TILE * 2 * KS; idx += 256) {
        const int row = idx / (2 * KS), c = 8 * (idx - row * (2 * KS));
        u32x4 x = zero4;
        if (row < Lk && c < d) x = att16_load8(kb + (long long)row * sk.l + c, vec);
        *(u32x4*)(Ks + row * LDK + c) = x;
    }
    // ---- V^T: a thread per (key pair, 8 columns) ---------------------------------------------------------------------------------------
    for (int idx = tid; idx < NKT * (ATT_TILE / 2) * 4 * DB; idx += 256) {
        const int pair = idx / (4 * DB), c = 8 * (idx - pair * (4 * DB));
        u32x4 x0 = zero4, x1 = zero4;
        if (c < d) {
            if (2 * pair < Lk) x0 = att16_load8(vb + (long long)(2 * pair) * sv.l + c, vec);
            if (2 * pair + 1 < Lk) x1 = att16_load8(vb + (long long)(2 * pair + 1) * sv.l + c, vec);
        }
        unsigned* const dst = (unsigned*)(Vt + c * LDV) + pair;              // LDV is even: a key pair is one dword
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            dst[(2 * e) * (LDV / 2)] = (x0[e] & 0xffffu) | (x1[e] << 16);
            dst[(2 * e + 1) * (LDV / 2)] = (x0[e] >> 16) | (x1[e] & 0xffff0000u);
        }
    }
    __syncthreads();

    const int nqt = (Lq + ATT_TILE - 1) / ATT_TILE;
    for (int qt = wave; qt < nqt; qt += 4) {
        int lk = Lk;
        asm volatile("" : "+s"(lk));                               // the key masks as this iteration's own: not hoisted into registers
        const int i = qt * ATT_TILE + l31;                         // this lane's query

        // ---- Q fragments from memory -------------------------------------------------------------------------------------------------
        u32x4 qf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 16 * s + 8 * hh;
            qf[s] = zero4;
            if (i < Lq && c < d) qf[s] = att16_load8(qb + (long long)i * sq.l + c, vec);
        }

        // ---- scores: block kt = K[kt * 32 ..][:] Q[tile][:]^T, column (lane) = query, rows (registers) = keys ------------------------
        f32x16 acc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kt][r] = 0.0f;
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const u32x4 ka = *(const u32x4*)(Ks + (kt * ATT_TILE + l31) * LDK + 16 * s + 8 * hh);
                acc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ka), __builtin_bit_cast(bf16x8, qf[s]), acc[kt], 0, 0, 0);
            }
        }

        // ---- softmax over the keys of this lane's query: registers, then the other half wave ---------------------------------------
        float mx = SEMICRF_NEG_INF;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool real = kt * ATT_TILE + (r & 3) + 8 * (r >> 2) + 4 * hh < lk;
                acc[kt][r] = real ? acc[kt][r] * scale : SEMICRF_NEG_INF;
                mx = fmaxf(mx, acc[kt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));                        // key 0 is real: the maximum is a true score
        unsigned pk[NKT][8];                                       // the rounded weights, two per dword, in register order
        float sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                const float p0 = expf(acc[kt][r] - mx), p1 = expf(acc[kt][r + 1] - mx);      // a masked key: exp(-inf) = +0 exactly
                const unsigned u = cvt_pk_bf16(p0, p1);
                pk[kt][r >> 1] = u;
                sum += __uint_as_float(u << 16);
                sum += __uint_as_float(u & 0xffff0000u);
            }
        {
            const float other = __shfl_xor(sum, 32);
            sum = hh == 0 ? sum + other : other + sum;             // S0 + S1 in both halves
        }

        // ---- P V: out^T = V^T P^T, the packed score registers as the B operand ------------------------------------------------------------
        f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u32x4 pb = {pk[kt][4 * s], pk[kt][4 * s + 1], pk[kt][4 * s + 2], pk[kt][4 * s + 3]};
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const uint16_t* vr = Vt + (db * 32 + l31) * LDV + kt * ATT_TILE + 16 * s + 4 * hh;      // kstep_key(s, 0, hh)
                    const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 8);                        // kstep_key(s, 4, hh)
                    const u32x4 va = {lo.x, lo.y, hi.x, hi.y};
                    o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), __builtin_bit_cast(bf16x8, pb), o[db], 0, 0, 0);
                }
            }

        // ---- bf16(o / sum) -> out: this lane's query, the columns below d ------------------------------------------------------------------
        if (i < Lq) {
            uint16_t* const oi = ob + (long long)i * so.l;
#pragma unroll
            for (int db = 0; db < DB; ++db)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = db * 32 + 8 * g + 4 * hh;
                    if (col < d) {                                   // d is a multiple of 8 and col of 4: all four columns or none
                        const unsigned a = cvt_pk_bf16(o[db][4 * g] / sum, o[db][4 * g + 1] / sum);
                        const unsigned b = cvt_pk_bf16(o[db][4 * g + 2] / sum, o[db][4 * g + 3] / sum);
                        if (ovec) {
                            *(uint2*)(oi + col) = make_uint2(a, b);
                        } else {
                            oi[col] = (uint16_t)a; oi[col + 1] = (uint16_t)(a >> 16);
                            oi[col + 2] = (uint16_t)b; oi[col + 3] = (uint16_t)(b >> 16);
                        }
                    }
                }
        }
    }
}

template <int NKT, int KS>
static void att16_launch_one(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, long long nseq, long long n1, int Lq, int Lk, int H,
                             int d, Att16Strides sq, Att16Strides sk, Att16Strides sv, Att16Strides so, int vec, int ovec, hipStream_t stream)
{
    static PerDeviceOnce once;
    const size_t lds = lds_bytes_bf16(NKT * ATT_TILE, 16 * KS);               // the instantiation's own size: Lk and d rounded up
    if (once.first())
        (void)hipFuncSetAttribute((const void*)axial_attention_bf16_kernel<NKT, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((axial_attention_bf16_kernel<NKT, KS>), dim3((unsigned)(nseq * H)), dim3(256), lds, stream, q, k, v, out, n1, Lq, Lk, H, d,
                       sq, sk, sv, so, scale_of(d), vec, ovec);
}

template <int KS>
static void att16_launch_kt(int nkt, const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, long long nseq, long long n1, int Lq, int Lk,
                            int H, int d, Att16Strides sq, Att16Strides sk, Att16Strides sv, Att16Strides so, int vec, int ovec, hipStream_t stream)
{
#define SEMICRF_ATT16_CASE(N) case N: att16_launch_one<N, KS>(q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, vec, ovec, stream); break
    switch (nkt) {
        SEMICRF_ATT16_CASE(1); SEMICRF_ATT16_CASE(2); SEMICRF_ATT16_CASE(3); SEMICRF_ATT16_CASE(4);
        SEMICRF_ATT16_CASE(5); SEMICRF_ATT16_CASE(6); SEMICRF_ATT16_CASE(7); SEMICRF_ATT16_CASE(8);
    }
#undef SEMICRF_ATT16_CASE
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and n0 n1 H < 2^31
void launch_axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, long long n0, long long n1, int Lq, int Lk, int H,
                                 int d, const long long* strides, hipStream_t stream)
{
    const Att16Strides sq{strides[0], strides[1], strides[2]}, sk{strides[3], strides[4], strides[5]}, sv{strides[6], strides[7], strides[8]},
        so{strides[9], strides[10], strides[11]};
    // 16-byte loads of Q, K and V rows: every base 16-byte aligned and every stride a multiple of eight bf16 (d is a multiple of 8)
    bool vec = ((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v) & 15) == 0);
    for (int i = 0; i < 9; ++i) vec = vec && (strides[i] & 7) == 0;
    // 8-byte stores of four columns
    bool ovec = (((uintptr_t)out) & 7) == 0;
    for (int i = 9; i < 12; ++i) ovec = ovec && (strides[i] & 3) == 0;
    const int nkt = key_tiles(Lk);
    const long long nseq = n0 * n1;
    switch (dim_steps(d)) {
        case 1: att16_launch_kt<1>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, vec, ovec, stream); break;
        case 2: att16_launch_kt<2>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, vec, ovec, stream); break;
        case 3: att16_launch_kt<3>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, vec, ovec, stream); break;
        default: att16_launch_kt<4>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, vec, ovec, stream); break;
    }
}

}  // namespace semicrf
