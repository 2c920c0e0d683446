// ffn.hip -- the feed-forward ResBlock of the backbone (ResBlock around Linear, GELU, Dropout, Linear; LayersTransformer.py) in eval
// mode as ONE launch:
//   out = x + (W2 gelu(W1 rmsnorm(x) + b1) + b2) * scale                     per token, ffn_math.h gives the order of operations
// in exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  No workspace, no atomics: the [tokens, hidden]
// activation never exists in memory.  x and out are [n0, n1, D] views with two row strides each and a contiguous last dimension.
//
// A workgroup (4 waves) owns FFN_ROWS = 64 token rows.  LDS (dynamic, sized by D):
//   Xs [64][D + 2]      the rows of x as they are (the epilogue's residual reads them again); the layer-1 A operand is Xs * rs
//   Ws                  the weights of the step at hand, half a chunk's worth: W1's 64 rows of the chunk over half of D
//                       [64][D / 2 + 2], or W2's D rows over 32 of the chunk's columns [D][34]
//   Gs [64][66]         the chunk's gelu tile, the A operand of layer 2
// which is 78.5 KB at D = 160 (two workgroups per CU, so that one's gelu runs beside the other's matrix work) and 115 KB at D = 256.
// Every operand row keeps each four contraction values as [k0, k2, k1, k3] (lds_pos): one 8-byte read feeds two matrix instructions,
// half wave 0 taking (k0, k2) and half wave 1 (k1, k3).  Row pitches are 2 (mod 4) floats: such a read hits 64 different banks.
// The walk over the hidden chunks, ascending, four steps per chunk; the weights of the next TWO steps are on their way from L2 into
// registers during every step (one step does not cover that latency), and every step is "registers -> Ws | barrier | matrix work | barrier":
//   layer 1, k < D / 2 and k >= D / 2: wave (rt, cw) one 32 x 32 block of the [64 x 64] hidden tile, D / 2 instructions in all
//   + b1, gelu -> Gs
//   layer 2, the chunk's columns 0 .. 31 and 32 .. 63: wave (rt, cw) the column blocks cw, cw + 2, .. of row block rt, 32
//   instructions each in all, on the chunk's own accumulators (from +0), which are added at the chunk's end to the running totals;
//   both sets stay in registers for the whole walk
// Epilogue: x + (acc + b2) * scale from Xs, stored by rows.  Ragged edges (rows past the last token, the last chunk of hidden, the
// last column block of D) are exact zeros formed in registers.
//
// TRAIN (semicrf_ffn_residual_train_fwd): the same walk; z = h + b1 is stored [tokens][H] as it leaves the accumulators, a = gelu(z) * M1
// goes to Gs in gelu's place, and the epilogue stores y = acc + b2 [tokens][D] and out = x + (y * M2) * scale.  One Philox call serves
// the four accumulator rows r & 3 of a lane (tokens 4 q .. 4 q + 3 at one column).  The eval instantiations carry none of it.
#include "common.h"
#include "launchers.h"
#include "ffn_math.h"

#include <type_traits>

namespace semicrf {

using namespace ffn;
using attr_heads::gelu;

typedef float ffn_f32x16 __attribute__((ext_vector_type(16)));
typedef float ffn_f32x2 __attribute__((ext_vector_type(2)));

constexpr int FFN_LDG = FFN_CHUNK + 2;   // floats per row of Gs and of the W2 tile
static_assert(FFN_ROWS == 64 && FFN_CHUNK == 64, "the lane maps below are written for 64 x 64");

constexpr int FFN_LDW2 = FFN_CHUNK / 2 + 2;   // floats per row of a W2 half tile

static inline size_t ffn_ws_floats(int D)
{
    const size_t a = (size_t)FFN_ROWS * (D / 2 + 2), b = (size_t)D * FFN_LDW2;
    return a > b ? a : b;
}
static inline size_t ffn_lds_bytes(int D)
{
    return ((size_t)FFN_ROWS * (D + 2) + ffn_ws_floats(D) + (size_t)FFN_ROWS * FFN_LDG + FFN_ROWS) * sizeof(float);
}

// row of a 32 x 32 result block held in accumulator register r of a lane in half wave hh (the column is lane & 31)
__device__ __forceinline__ int ffn_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// four consecutive contraction values into their LDS order
__device__ __forceinline__ void ffn_store4(float* dst, float4 v)
{
    *(float2*)dst = make_float2(v.x, v.z);
    *(float2*)(dst + 2) = make_float2(v.y, v.w);
}

// p[0 .. 3] when `ok`, zeros formed in registers otherwise.  The load is issued either way, without a branch (the compiler then counts
// the loads in flight, and a wait for the older of two sets does not wait for the younger): the caller clamps p into the tensor.
template <bool VEC>
__device__ __forceinline__ float4 ffn_load4(const float* p, bool ok)
{
    float4 v;
    if (VEC) {
        v = *(const float4*)p;
    } else {
        v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = p[3];
    }
    return make_float4(ok ? v.x : 0.0f, ok ? v.y : 0.0f, ok ? v.z : 0.0f, ok ? v.w : 0.0f);
}

// DB: column blocks of 32 that cover D (D in (32 (DB - 1), 32 DB]); up to D = 160 two workgroups share a CU
// VEC: 16-byte loads (every base 16-byte aligned, every stride a multiple of four floats)
struct FfnTrainArgs { float* z; float* y; DropoutParams drop; };
struct FfnNoArgs {};

// TRAIN at DB = 5 does not fit two workgroups' registers without scratch: one workgroup per CU there
template <int DB, bool VEC, bool TRAIN>
__global__ __launch_bounds__(256, DB <= (TRAIN ? 4 : 5) ? 2 : 1) void ffn_residual_kernel(
    const float* __restrict__ x, float* __restrict__ out, long long ntok, long long n1, long long xs0, long long xs1, long long os0,
    long long os1, int D, int H, const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
    const float* __restrict__ b2, const float* __restrict__ scale, float eps, std::conditional_t<TRAIN, FfnTrainArgs, FfnNoArgs> tr)
{
    constexpr int NB = (DB + 1) / 2;                         // column blocks per wave
    constexpr int NW = DB;                                   // float4 of a half tile per thread (64 (D / 2) / 4 / 256 = D / 32 <= DB)
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn_smem[];
    const int ldx = D + 2, kh = D >> 1, ldw1 = kh + 2;
    float* const Xs = (float*)ffn_smem;
    float* const Ws = Xs + FFN_ROWS * ldx;
    float* const Gs = Ws + max(FFN_ROWS * ldw1, D * FFN_LDW2);
    float* const Rs = Gs + FFN_ROWS * FFN_LDG;
    long long* const roff = (long long*)Ws;                  // element offsets of the tile's rows (-1 past the last token), while Ws is free

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const long long row0 = (long long)blockIdx.x * FFN_ROWS;
    const int q4 = D >> 2;                                   // float4 per row of x
    const int q8 = D >> 3;                                   // float4 per row of a W1 half tile
    const int nhalf = FFN_ROWS * q8;                         // float4 of a W1 half tile = of a W2 half tile (D rows of 8)

    auto row_offsets = [&](long long s0, long long s1) {
        if (tid < FFN_ROWS) {
            const long long t = row0 + tid;
            long long o = -1;
            if (t < ntok) {
                const long long i0 = t / n1, i1 = t - i0 * n1;
                o = i0 * s0 + i1 * s1;
            }
            roff[tid] = o;
        }
    };
    row_offsets(xs0, xs1);

    // ---- the weights of a step, from memory into registers: W1's rows j0 .. j0 + 63 over k0 .. k0 + D / 2 - 1 [64][D / 2], or W2's
    // columns j0 .. j0 + 31 [D][32]; thread t moves the float4 t, t + 256, .. of the half tile
    float4 wra[NW], wrb[NW];                                 // two steps ahead: the steps alternate between the two sets
    int w1r[NW], w1c[NW];                                    // row and float4 column of this thread's pieces of a W1 half tile
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int idx = tid + 256 * i;
        w1r[i] = idx / q8;
        w1c[i] = idx - w1r[i] * q8;
    }
    auto load_w1 = [&](float4* wr, int j0, int k0) {
        const int wv = min(FFN_CHUNK, H - j0);
#pragma unroll
        for (int i = 0; i < NW; ++i)                          // rows past the chunk's end (and the threads past the tile's) read its last row
            wr[i] = ffn_load4<VEC>(W1 + (size_t)(j0 + min(w1r[i], wv - 1)) * D + k0 + 4 * w1c[i], tid + 256 * i < nhalf && w1r[i] < wv);
    };
    auto store_w1 = [&](const float4* wr) {
#pragma unroll
        for (int i = 0; i < NW; ++i)
            if (tid + 256 * i < nhalf) ffn_store4(Ws + w1r[i] * ldw1 + 4 * w1c[i], wr[i]);
    };
    auto load_w2 = [&](float4* wr, int j0) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            const int n = min(idx >> 3, D - 1), c = idx & 7;
            const bool ok = idx < nhalf && j0 + 4 * c < H;     // columns past hidden read the row's first four
            wr[i] = ffn_load4<VEC>(W2 + (size_t)n * H + (ok ? j0 + 4 * c : 0), ok);
        }
    };
    auto store_w2 = [&](const float4* wr) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            if (idx < nhalf) ffn_store4(Ws + (idx >> 3) * FFN_LDW2 + 4 * (idx & 7), wr[i]);
        }
    };

    load_w1(wra, 0, 0);
    load_w1(wrb, 0, kh);
    __syncthreads();                                         // roff

    // ---- the tile's rows of x -> Xs ------------------------------------------------------------------------------------------------
    {
        float4 xr[2 * DB];                                   // all of this thread's loads are in flight before the first is stored
#pragma unroll
        for (int i = 0; i < 2 * DB; ++i) {
            const int idx = tid + 256 * i;
            const int r = min(idx / q4, FFN_ROWS - 1), c = idx - (idx / q4) * q4;
            const long long xo = roff[r];
            xr[i] = ffn_load4<VEC>(x + max(xo, 0ll) + 4 * c, idx < FFN_ROWS * q4 && xo >= 0);   // rows past the last token read token 0
        }
#pragma unroll
        for (int i = 0; i < 2 * DB; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx / q4, c = idx - r * q4;
            if (idx < FFN_ROWS * q4) ffn_store4(Xs + r * ldx + 4 * c, xr[i]);
        }
    }
    __syncthreads();
    {
        // four threads per row: thread q sums the squares of k = q, q + 4, .. (lds_pos(4 m + q) = 4 m + lds_pos(q))
        const int r = tid >> 2, q = tid & 3;
        const float* xr = Xs + r * ldx + lds_pos(q);
        float s = 0.0f;
        for (int m = 0; m < q4; m += 2) {                    // q4 is even; two reads in flight
            const float v0 = xr[4 * m], v1 = xr[4 * m + 4];
            s = fmaf(v0, v0, s);
            s = fmaf(v1, v1, s);
        }
        const float t = s + __shfl_xor(s, 1);                // q = 0, 1: s0 + s1;  q = 2, 3: s2 + s3
        const float u = t + __shfl_xor(t, 2);                // (s0 + s1) + (s2 + s3): the sum commutes, so every q holds the same bits
        if (q == 0) Rs[r] = rs_of(u, D, eps);
    }
    __syncthreads();                                         // Rs; the reads of roff are behind, Ws is free

    const int rt = wave & 1, cw = wave >> 1;
    ffn_f32x16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const float* const xa = Xs + (rt * 32 + l31) * ldx + 2 * hh;      // this lane's row of x, its half wave's pair of every four
    const float* const ga = Gs + (rt * 32 + l31) * FFN_LDG + 2 * hh;  // the same row of the gelu tile
    const float* const w1b = Ws + (cw * 32 + l31) * ldw1 + 2 * hh;    // layer 1's B operand: row (hidden column) cw * 32 + l31 of the W1 tile
    const float* w2b[NB];                                    // layer 2's: row (output column) n of the W2 tile
    bool on[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int n = (cw + 2 * i) * 32 + l31;
        on[i] = n < D;
        w2b[i] = Ws + min(n, D - 1) * FFN_LDW2 + 2 * hh;
    }
    ffn_f32x16 h, part[NB];                                  // a chunk's own layer-2 sums: from +0 per chunk, added to acc at its end
    const float rs = Rs[rt * 32 + l31];
    // both loops keep their operand reads two steps ahead of the matrix instructions that take them (an in-order wave would otherwise
    // wait out the LDS latency in front of every pair).  Layer 1: the offset of the read ahead goes through an empty asm, or the
    // compiler proves that it is the address of a later step and reads it there instead; a read past the end is clamped to the last
    // step and never used.  Layer 2 (unrolled): the scheduler is told the order, reads of step m + 2 in front of the products of step m.
    auto lds2 = [](const float* p) -> ffn_f32x2 { return *(const ffn_f32x2*)p; };
    auto layer1 = [&](int k0) {                              // k = k0 .. k0 + D / 2 - 1
        const float* const xk = xa + k0;
        ffn_f32x2 a0 = lds2(xk), b0 = lds2(w1b);
        const int m1 = min(1, q8 - 1);
        ffn_f32x2 a1 = lds2(xk + 4 * m1), b1 = lds2(w1b + 4 * m1);
        for (int m = 0; m < q8; ++m) {
            int off = 4 * min(m + 2, q8 - 1);
            asm volatile("" : "+s"(off));
            const ffn_f32x2 a2 = lds2(xk + off), b2 = lds2(w1b + off);
            h = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x * rs, b0.x, h, 0, 0, 0);
            h = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y * rs, b0.y, h, 0, 0, 0);
            a0 = a1; b0 = b1;
            a1 = a2; b1 = b2;
        }
    };
    // a wave whose last column block lies past D (DB odd, cw = 1) multiplies zeros there while the other waves work on real blocks:
    // the barrier would have it wait that long anyway, and a loop without branches lets the reads run ahead
    auto layer2 = [&](int jj0) {                             // the chunk's columns jj0 .. jj0 + 31
        constexpr int NM = FFN_CHUNK / 8;
        ffn_f32x2 a[3], b[3][NB];
        auto fetch = [&](int m) {
            a[m % 3] = lds2(ga + jj0 + 4 * m);
#pragma unroll
            for (int i = 0; i < NB; ++i) b[m % 3][i] = lds2(w2b[i] + 4 * m);
        };
        fetch(0);
        fetch(1);
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            if (m + 2 < NM) fetch(m + 2);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const ffn_f32x2 v = b[m % 3][i];
                part[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m % 3].x, on[i] ? v.x : 0.0f, part[i], 0, 0, 0);
                part[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[m % 3].y, on[i] ? v.y : 0.0f, part[i], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 2 * (NB + 1), 0);          // LDS reads of steps 0 and 1
#pragma unroll
        for (int m = 0; m < NM; ++m) {
            if (m + 2 < NM) __builtin_amdgcn_sched_group_barrier(0x100, NB + 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x008, 2 * NB, 0);            // the step's matrix instructions
        }
    };

    const int nch = chunks_of(H);
    for (int ch = 0; ch < nch; ++ch) {
        const int j0 = ch * FFN_CHUNK;
        const int wv = min(FFN_CHUNK, H - j0);
        // ---- layer 1: block (rt, cw) of the hidden tile, the two halves of D -------------------------------------------------------
        store_w1(wra);                                       // Ws was last read before the barrier that ends the previous step
        load_w2(wra, j0);
        __syncthreads();
        const int col = cw * 32 + l31;
        const bool real = col < wv;
        const float bias = real ? b1[j0 + col] : 0.0f;       // asked for a whole layer ahead of its use
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = 0.0f;
        layer1(0);
        __syncthreads();
        store_w1(wrb);
        load_w2(wrb, j0 + FFN_CHUNK / 2);
        __syncthreads();
        layer1(kh);
        {
            float* const gw = Gs + lds_pos(col);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint32_t draw[4] = {0u, 0u, 0u, 0u};
                if constexpr (TRAIN) {
                    const long long ib = row0 + rt * 32 + 8 * g4 + 4 * hh;          // a multiple of 4: rows ib .. ib + 3 are r & 3
                    if (tr.drop.on[0] && real) dropout_draws(tr.drop.seed, 0u, (unsigned long long)ib >> 2, (uint32_t)(j0 + col), draw);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = 4 * g4 + u;
                    const int row = rt * 32 + ffn_acc_row(r, hh);
                    if constexpr (TRAIN) {
                        const float zz = h[r] + bias;
                        if (real && row0 + row < ntok) tr.z[(size_t)(row0 + row) * H + j0 + col] = zz;
                        gw[row * FFN_LDG] = real ? masked(tr.drop, 0, draw[u], gelu<float>(zz)) : 0.0f;
                    } else {
                        gw[row * FFN_LDG] = real ? gelu<float>(h[r] + bias) : 0.0f;
                    }
                }
            }
        }
        __syncthreads();                                     // Gs is written, Ws (W1) is read
        // ---- layer 2: the column blocks cw, cw + 2, .. of row block rt, the two halves of the chunk ----------------------------------
        store_w2(wra);
        if (ch + 1 < nch) load_w1(wra, j0 + FFN_CHUNK, 0);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) part[i][r] = 0.0f;
        layer2(0);
        __syncthreads();
        store_w2(wrb);
        if (ch + 1 < nch) load_w1(wrb, j0 + FFN_CHUNK, kh);
        __syncthreads();
        layer2(FFN_CHUNK / 2);
#pragma unroll
        for (int i = 0; i < NB; ++i) acc[i] += part[i];      // chunks ascending: ((p0 + p1) + p2) + ..
        __syncthreads();                                     // Ws and Gs are free for the next chunk
    }

    // ---- x + (acc + b2) * scale -----------------------------------------------------------------------------------------------------
    row_offsets(os0, os1);                                   // into Ws, free since the last barrier
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int n = (cw + 2 * i) * 32 + l31;
        if (cw + 2 * i < DB && n < D) {
            const float bb = b2[n], sc = scale[n];
            const int xp = lds_pos(n);
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                uint32_t draw[4] = {0u, 0u, 0u, 0u};
                if constexpr (TRAIN) {
                    const long long ib = row0 + rt * 32 + 8 * g4 + 4 * hh;
                    if (tr.drop.on[1]) dropout_draws(tr.drop.seed, 1u, (unsigned long long)ib >> 2, (uint32_t)n, draw);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int r = 4 * g4 + u;
                    const int row = rt * 32 + ffn_acc_row(r, hh);
                    const long long oo = roff[row];
                    if constexpr (TRAIN) {
                        if (oo >= 0) {
                            const float yy = acc[i][r] + bb;
                            tr.y[(size_t)(row0 + row) * D + n] = yy;
                            out[oo + n] = Xs[row * ldx + xp] + masked(tr.drop, 1, draw[u], yy) * sc;
                        }
                    } else {
                        if (oo >= 0) out[oo + n] = epilogue(Xs[row * ldx + xp], acc[i][r], bb, sc);
                    }
                }
            }
        }
    }
}

template <int DB, bool VEC, bool TRAIN>
static void ffn_launch_one(const float* x, float* out, long long ntok, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                           int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                           hipStream_t stream, std::conditional_t<TRAIN, FfnTrainArgs, FfnNoArgs> tr)
{
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)ffn_residual_kernel<DB, VEC, TRAIN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)ffn_lds_bytes(DB * 32));
    hipLaunchKernelGGL((ffn_residual_kernel<DB, VEC, TRAIN>), dim3((unsigned)((ntok + FFN_ROWS - 1) / FFN_ROWS)), dim3(256), ffn_lds_bytes(D), stream,
                       x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, tr);
}

template <bool TRAIN>
static void ffn_launch_any(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                           int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                           hipStream_t stream, std::conditional_t<TRAIN, FfnTrainArgs, FfnNoArgs> tr)
{
    // 16-byte loads: every base and every stride a multiple of four floats (D and H are multiples of 8)
    const bool vec = ((((uintptr_t)x | (uintptr_t)W1 | (uintptr_t)W2) & 15) == 0) && ((xs0 | xs1) & 3) == 0;
    const long long ntok = n0 * n1;
#define SEMICRF_FFN_CASE(N)                                                                                                        \
    case N:                                                                                                                        \
        if (vec) ffn_launch_one<N, true, TRAIN>(x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream, tr);  \
        else ffn_launch_one<N, false, TRAIN>(x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream, tr);     \
        break
    switch ((D + 31) / 32) {
        SEMICRF_FFN_CASE(1); SEMICRF_FFN_CASE(2); SEMICRF_FFN_CASE(3); SEMICRF_FFN_CASE(4);
        SEMICRF_FFN_CASE(5); SEMICRF_FFN_CASE(6); SEMICRF_FFN_CASE(7); SEMICRF_FFN_CASE(8);
    }
#undef SEMICRF_FFN_CASE
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and n0 n1 < 2^37
void launch_ffn_residual(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                         int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                         hipStream_t stream)
{
    ffn_launch_any<false>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream, FfnNoArgs{});
}

// the training mode: also z [n0 n1][H] and y [n0 n1][D], dense, and the two dropouts of (seed, p1, p2)
void launch_ffn_residual_train(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                               long long os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                               const float* scale, float eps, unsigned long long seed, double p1, double p2, float* z, float* y,
                               hipStream_t stream)
{
    ffn_launch_any<true>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream,
                         FfnTrainArgs{z, y, attr_heads::dropout_params(seed, p1, p2)});
}

}  // namespace semicrf
