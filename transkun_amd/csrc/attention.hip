// attention.hip -- the attention of the backbone's transformer layers (MultiHeadAttentionKernel with kernel = None,
// LayersTransformer.py:162-190: F.scaled_dot_product_attention on head-split views) for hundreds of short, independent sequences:
//   out[s, i, h, :] = sum_j softmax_j(q[s,i,h,:] . k[s,j,h,:] / sqrt(d)) v[s,j,h,:]        1 <= Lq, Lk <= 256, d = 8, 16, .. 64
// fp32, no mask, no dropout.  q, k, v and out are TOKEN-MAJOR (a token's H d values contiguous) and each carries three element
// strides (two sequence dimensions and the token), so the frequency axis and the time axis of one [N, T', F', H d] buffer are two
// calls on the same memory: no transposed copy on the way in or out.
//
// Workgroup = one (sequence, head), 4 waves.  K of the head goes into LDS once, token-major with rows of d + 1 floats (an operand
// read takes 32 tokens at one column: 32 banks).  Wave w then takes the query tiles w, w + 4, .. of 32 queries on its own:
//   Q tile    32 rows into the wave's scratch, the same layout
//   scores    S^T = K Q^T, block kt (32 keys x 32 queries) on its own accumulator: v_mfma_f32_32x32x2_f32 with A = K[key][c],
//             B = Q[query][c], c ascending -- a lane holds ONE query's scores (its column), 16 keys per block and half wave
//   softmax   * scale, keys past Lk masked BEFORE the maximum; maximum and sum over the lane's registers, then across the two half
//             waves (one exchange each); p = exp(s - max), exactly 0 for masked keys.  All in registers: no online rescaling.
//   P V       per key block: p into the wave's LDS tile [key][query] (the accumulator's rows become the next product's k index),
//             read back as the A operand in natural key order; B = V[key][column] straight from memory, a half wave reading 32
//             consecutive floats of one token (coalesced; the head's V is 10 - 64 KB and stays in the L2), zeros formed in
//             registers for keys past Lk and columns past d; block kt + 1 is requested before block kt's products.  One or two
//             accumulators (d <= 32, d <= 64).
//   store     o / sum for the rows below Lq and the columns below d
// No atomics, no workgroup barrier after the K stage; tile sizes depend on Lk and d alone, so a sequence's result is bit-identical
// whatever the batch, its position in it and the strides are.  LDS: 32 kt (d + 1) + 4 (32 max(d + 1, 40) + 32) floats: 48 KB at
// L = 149, d = 40 (two workgroups per CU, which the 256 registers of that instantiation allow), 100 KB at the largest shape.
#include "common.h"
#include "launchers.h"
#include "attention_math.h"

namespace semicrf {

using namespace attention;

typedef float att_f32x16 __attribute__((ext_vector_type(16)));

struct AttStrides { long long s0, s1, l; };

// row of a 32 x 32 result block held in accumulator register r of a lane in half wave hh (the column is lane & 31)
__device__ __forceinline__ int att_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// orders a wave's LDS traffic: what its lanes wrote before is what any of its lanes reads after (the LDS serves one wave's
// instructions in order; this keeps the compiler from moving them across)
__device__ __forceinline__ void att_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__host__ __device__ inline int att_scratch_floats(int d) { return ATT_TILE * (d + 1 > ATT_LDP ? d + 1 : ATT_LDP) + ATT_TILE; }
static size_t att_lds_bytes(int Lk, int d) { return ((size_t)key_tiles(Lk) * ATT_TILE * (d + 1) + 4 * (size_t)att_scratch_floats(d)) * sizeof(float); }

// rows [row0, row0 + 32) x d of a token-major matrix into LDS rows of ldk floats, zeros past nrows; nthr threads, this one `t`
template <bool VEC>
__device__ __forceinline__ void att_stage_rows(float* dst, int ldk, const float* __restrict__ src, long long stride_l, int row0, int nrows,
                                               int ntile_rows, int d, int t, int nthr)
{
    if (VEC) {
        const int d4 = d >> 2;
        for (int idx = t; idx < ntile_rows * d4; idx += nthr) {
            const int row = idx / d4, c = 4 * (idx - row * d4);
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (row0 + row < nrows) x = *(const float4*)(src + (long long)(row0 + row) * stride_l + c);
            float* p = dst + row * ldk + c;
            p[0] = x.x; p[1] = x.y; p[2] = x.z; p[3] = x.w;
        }
    } else {
        for (int idx = t; idx < ntile_rows * d; idx += nthr) {
            const int row = idx / d, c = idx - row * d;
            dst[row * ldk + c] = row0 + row < nrows ? src[(long long)(row0 + row) * stride_l + c] : 0.0f;
        }
    }
}

// v and out are deliberately not __restrict__: V is the same for every query tile of a wave, and as an invariant load the compiler
// hoists a whole head of it out of the tile loop into registers (hundreds of them, then spills)
template <int NKT, int DB, bool VEC>
__global__ __launch_bounds__(256, NKT <= 5 ? 2 : 1) void axial_attention_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                              const float* v, float* out, long long n1, int Lq,
                                                              int Lk, int H, int d, AttStrides sq, AttStrides sk, AttStrides sv,
                                                              AttStrides so, float scale)
{
    extern __shared__ __attribute__((aligned(16))) float att_lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int ldk = d + 1;
    float* const Ks = att_lds;                                                        // [NKT * 32][ldk]
    float* const Ws = att_lds + NKT * ATT_TILE * ldk + wave * att_scratch_floats(d);  // this wave's Q tile [32][ldk] / P tile [32][ATT_LDP]
    float* const Sm = Ws + att_scratch_floats(d) - ATT_TILE;                          // this wave's 32 row sums

    const unsigned blk = blockIdx.x, useq = blk / (unsigned)H;   // n0 n1 H < 2^31: 32-bit divisions
    const int h = (int)(blk - useq * (unsigned)H);
    const long long s0 = useq / (unsigned)n1, s1 = useq - (unsigned)s0 * (unsigned)n1;
    const float* const qb = q + s0 * sq.s0 + s1 * sq.s1 + (long long)h * d;
    const float* const kb = k + s0 * sk.s0 + s1 * sk.s1 + (long long)h * d;
    const float* const vb = v + s0 * sv.s0 + s1 * sv.s1 + (long long)h * d;
    float* const ob = out + s0 * so.s0 + s1 * so.s1 + (long long)h * d;

    att_stage_rows<VEC>(Ks, ldk, kb, sk.l, 0, Lk, NKT * ATT_TILE, d, tid, 256);
    __syncthreads();

    const int nqt = (Lq + ATT_TILE - 1) / ATT_TILE;
    for (int qt = wave; qt < nqt; qt += 4) {
        // V's base and the key count as this iteration's own scalars: the V addresses and the key masks are the same for every query
        // tile, and hoisted out of this loop they occupy hundreds of registers
        const float* vq = vb;
        int lk = Lk;
        asm volatile("" : "+s"(vq), "+s"(lk));
        att_stage_rows<VEC>(Ws, ldk, qb, sq.l, qt * ATT_TILE, Lq, ATT_TILE, d, lane, 64);
        att_wave_sync();

        // ---- scores: block kt = K[kt * 32 ..][:] Q[tile][:]^T, column (lane) = query, rows (registers) = keys ------------------------
        att_f32x16 acc[NKT];
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[kt][r] = 0.0f;
        {
            const float* qa = Ws + l31 * ldk + hh;
            const float* ka = Ks + l31 * ldk + hh;
            for (int m = 0; m < (d >> 1); ++m) {                   // instruction m: c = 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
                const float qv = qa[2 * m];
#pragma unroll
                for (int kt = 0; kt < NKT; ++kt)
                    acc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ka[kt * ATT_TILE * ldk + 2 * m], qv, acc[kt], 0, 0, 0);
            }
        }
        att_wave_sync();                                           // the Q tile has been read: its memory becomes the P tile

        // ---- V of the first key block, requested before the softmax so that its latency hides there -------------------------------------
        // a lane's part of a V address (its key's parity and its column) is a 32-bit offset (stride_l < 2^28, checked by the caller);
        // the even key's row is the same for the whole wave
        const unsigned voff = (unsigned)(hh * sv.l + l31);
        float bv[2][DB][16];
        auto load_v = [&](int kt, float (&b)[DB][16]) {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int key0 = kt * ATT_TILE + 2 * m;
                const float* row = vq + (long long)key0 * sv.l;
#pragma unroll
                for (int db = 0; db < DB; ++db)
                    b[db][m] = (key0 + hh < lk && db * 32 + l31 < d) ? row[voff + db * 32] : 0.0f;
            }
        };
        load_v(0, bv[0]);

        // ---- softmax over the keys of this lane's query: registers, then the other half wave ---------------------------------------
        float mx = SEMICRF_NEG_INF;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool real = kt * ATT_TILE + att_acc_row(r, hh) < lk;
                acc[kt][r] = real ? acc[kt][r] * scale : SEMICRF_NEG_INF;
                mx = fmaxf(mx, acc[kt][r]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 32));                        // key 0 is real: the maximum is a true score
        float sum = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = expf(acc[kt][r] - mx);             // a masked key: exp(-inf) = +0 exactly
                acc[kt][r] = p;
                sum += p;
            }
        {
            const float other = __shfl_xor(sum, 32);
            const float total = hh == 0 ? sum + other : other + sum;      // S0 + S1 in both halves
            if (hh == 0) Sm[l31] = total;
        }

        // ---- P V: per key block, p through the LDS tile into operand layout; V from memory ------------------------------------------
        att_f32x16 o[DB];
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[db][r] = 0.0f;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
            if (kt + 1 < NKT) load_v(kt + 1, bv[(kt + 1) & 1]);    // the next block's V is on its way during this block's products
#pragma unroll
            for (int r = 0; r < 16; ++r) Ws[att_acc_row(r, hh) * ATT_LDP + l31] = acc[kt][r];
            att_wave_sync();
#pragma unroll
            for (int m = 0; m < 16; ++m) {                         // instruction m: keys 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
                const float pa = Ws[(2 * m + hh) * ATT_LDP + l31];
#pragma unroll
                for (int db = 0; db < DB; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa, bv[kt & 1][db][m], o[db], 0, 0, 0);
            }
            att_wave_sync();                                       // the tile has been read before the next block overwrites it
            __builtin_amdgcn_sched_barrier(0);
        }

        // ---- o / sum -> out, rows below Lq and columns below d -------------------------------------------------------------------------
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = att_acc_row(r, hh), i = qt * ATT_TILE + row;
            const float den = Sm[row];
            if (i < Lq) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int col = db * 32 + l31;
                    if (col < d) ob[(long long)i * so.l + col] = o[db][r] / den;
                }
            }
        }
        att_wave_sync();                                           // Sm and the tile are free for the next query tile
    }
}

template <int NKT, int DB, bool VEC>
static void att_launch_one(const float* q, const float* k, const float* v, float* out, long long nseq, long long n1, int Lq, int Lk, int H, int d,
                           AttStrides sq, AttStrides sk, AttStrides sv, AttStrides so, hipStream_t stream)
{
    static PerDeviceOnce once;
    const size_t lds = att_lds_bytes(Lk, d);
    if (once.first())
        (void)hipFuncSetAttribute((const void*)axial_attention_kernel<NKT, DB, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)att_lds_bytes(NKT * ATT_TILE, DB * 32));
    hipLaunchKernelGGL((axial_attention_kernel<NKT, DB, VEC>), dim3((unsigned)(nseq * H)), dim3(256), lds, stream, q, k, v, out, n1, Lq, Lk, H, d,
                       sq, sk, sv, so, scale_of(d));
}

template <int DB, bool VEC>
static void att_launch_kt(int nkt, const float* q, const float* k, const float* v, float* out, long long nseq, long long n1, int Lq, int Lk, int H,
                          int d, AttStrides sq, AttStrides sk, AttStrides sv, AttStrides so, hipStream_t stream)
{
#define SEMICRF_ATT_CASE(N) case N: att_launch_one<N, DB, VEC>(q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, stream); break
    switch (nkt) {
        SEMICRF_ATT_CASE(1); SEMICRF_ATT_CASE(2); SEMICRF_ATT_CASE(3); SEMICRF_ATT_CASE(4);
        SEMICRF_ATT_CASE(5); SEMICRF_ATT_CASE(6); SEMICRF_ATT_CASE(7); SEMICRF_ATT_CASE(8);
    }
#undef SEMICRF_ATT_CASE
}

// the caller (api.hip) has checked the supported set, the pointers and n0 n1 H < 2^31
void launch_axial_attention(const float* q, const float* k, const float* v, float* out, long long n0, long long n1, int Lq, int Lk, int H, int d,
                            const long long* strides, hipStream_t stream)
{
    const AttStrides sq{strides[0], strides[1], strides[2]}, sk{strides[3], strides[4], strides[5]}, sv{strides[6], strides[7], strides[8]},
        so{strides[9], strides[10], strides[11]};
    // 16-byte loads of Q and K rows: every base and every stride a multiple of four floats (d is a multiple of 8)
    bool vec = ((((uintptr_t)q | (uintptr_t)k) & 15) == 0);
    for (int i = 0; i < 6; ++i) vec = vec && (strides[i] & 3) == 0;
    const int nkt = key_tiles(Lk);
    const long long nseq = n0 * n1;
    if (d <= 32) {
        if (vec) att_launch_kt<1, true>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, stream);
        else att_launch_kt<1, false>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, stream);
    } else {
        if (vec) att_launch_kt<2, true>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, stream);
        else att_launch_kt<2, false>(nkt, q, k, v, out, nseq, n1, Lq, Lk, H, d, sq, sk, sv, so, stream);
    }
}

}  // namespace semicrf
