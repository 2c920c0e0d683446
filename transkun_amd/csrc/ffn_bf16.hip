// ffn_bf16.hip -- semicrf_ffn_residual_bf16 and semicrf_ffn_residual_bf16_mixed: the feed-forward ResBlock of ffn.hip with both
// products on the bf16 matrix instruction (v_mfma_f32_32x32x16_bf16), eval mode, forward only, ONE launch:
//   out = x + (W2 gelu(W1 rmsnorm(x) + b1) + b2) * scale                     per token, ffn_bf16_math.h gives the order of operations
// One kernel body, two forms: T = bf16 (form A: every tensor bf16 in memory) and T = fp32 (form B: every tensor fp32 in memory, W1 and
// W2 rounded to bf16 on their way into LDS, b1, b2 and scale used as fp32).  The contract is ffn.hip's: x and out are [n0, n1, D]
// views with two row strides each and a contiguous last dimension; no workspace, no atomics.
//
// A workgroup (4 waves) owns FFN16_ROWS = 64 token rows and walks hidden in chunks of FFN16_CHUNK = 64 columns, ascending.  Both
// products are computed TRANSPOSED, so that a lane of wave (rt, cw) is ONE token (row rt * 32 + (lane & 31)) throughout:
//   x         never in LDS.  Four threads per row sum its squares (ffn_math.h's four chains) from memory; then every lane takes its
//             token's layer-1 operand fragments from memory, 8 consecutive values per k-step (16 s + 8 hh ..), times rs, rounded to
//             bf16 (v_cvt_pk_bf16_f32), and keeps them in registers for the whole walk: D / 4 dwords
//   LDS       W1s [64][D + 8]     the chunk's rows of W1 (zeros past hidden; the 8 pad columns are zeros: D = 8 (mod 16) reads them)
//             W2s [D][64 + 8]     the chunk's columns of W2 (zeros past hidden)
//             Gs  [64][64 + 8]    the chunk's gelu tile, token-major
//             all bf16: 54 KB at D = 160 (two workgroups per CU), 80 KB at D = 256
//   layer 1   H^T block cw of the chunk (32 hidden columns x 32 tokens): A = 8 consecutive bf16 of W1s row cw * 32 + (lane & 31), B =
//             the x fragment; k-steps ascending on one accumulator.  + b1, gelu, pairs rounded to bf16; a lane holds four consecutive
//             hidden columns per register group: 8-byte stores into Gs
//   layer 2   out^T blocks cw, cw + 2, .. (32 output columns x 32 tokens): A = 8 consecutive bf16 of W2s row n, B = 16 bytes of the
//             token's row of Gs; four k-steps per chunk, on ONE running accumulator per block for the whole walk
//   epilogue  a lane holds four consecutive output columns of its token per register group: x is read again from memory (8 or 16
//             bytes), x + (acc + b2) * scale, one rounding to T, 8-byte (bf16) or 16-byte (fp32) stores where `out` allows
// The weights of the NEXT chunk are on their way from L2 into registers during a chunk's matrix work.  Three barriers per chunk.
// Ragged edges: rows past the last token are zero fragments formed in registers (and their gelu values are zeros: no 0 * NaN, nothing
// stored); hidden columns past the last chunk and columns past D are zeros formed in registers; the loads behind them are clamped
// onto real elements and their values dropped.  Tile sizes depend on nothing and every sum has one order: a token's result is
// bit-identical whatever the other tokens, n0, n1, the strides and the alignment are.
//
// Training mode (template parameter TRAIN; semicrf_ffn_residual_bf16_train_fwd / _mixed_train_fwd; the chain: ffn_bf16_train_math.h): the
// same walk with both dropouts from the fp32 route's stateless mask (one Philox call per lane and register group: the four lanes of a
// quad share their draws), zs = bf16(h) written through one more LDS tile [64][64 + 8] as whole 128-byte lines, ys = y rounded to T
// beside `out`.  The eval instantiations compile to the registers they had; with p = 0 the training mode gives their bits.
#include "common.h"
#include "launchers.h"
#include "bf16x3.h"
#include "ffn_bf16_dev.h"

#include <type_traits>

namespace semicrf {

using namespace ffn;
using attr_heads::gelu;

struct Ffn16Eval {};
template <typename T>
struct Ffn16Train { DropoutParams drop; uint16_t* zs; T* ys; };

// T: uint16_t (bf16 tensors) or float (fp32 tensors, bf16 operands)
// TRAIN: the training mode: both dropouts, zs and ys saved (tr); the eval instantiations compile to what they were
// DB: column blocks of 32 that cover D (D in (32 (DB - 1), 32 DB]); up to D = 160 two workgroups share a CU
// vec: 16-byte loads of x, W1 and W2 (launch_ffn_residual_bf16 decides); ovec: the epilogue's four-column reads of x and stores of out
template <typename T, int DB, bool TRAIN = false>
__global__ __launch_bounds__(256, DB <= 5 ? 2 : 1) void ffn_residual_bf16_kernel(const T* x, T* out, long long ntok, long long n1, long long xs0,
                                                                               long long xs1, long long os0, long long os1, int D, int H,
                                                                               const T* __restrict__ W1, const T* __restrict__ b1,
                                                                               const T* __restrict__ W2, const T* __restrict__ b2,
                                                                               const T* __restrict__ scale, float eps, int vec, int ovec,
                                                                               std::conditional_t<TRAIN, Ffn16Train<T>, Ffn16Eval> tr = {})
{
    constexpr int NB = (DB + 1) / 2;                         // column blocks per wave
    constexpr int KS = 2 * DB;                               // k-steps of layer 1 an instantiation can have
    constexpr int NW = DB;                                   // 8-element pieces of a weight tile per thread (64 (D / 8) / 256 = D / 32 <= DB)
    extern __shared__ __attribute__((aligned(16))) unsigned char ffn16_smem[];
    const int ldw1 = D + FFN16_PAD;
    uint16_t* const W1s = (uint16_t*)ffn16_smem;                       // [64][ldw1]
    uint16_t* const W2s = W1s + FFN16_CHUNK * ldw1;                     // [D][FFN16_LDG]
    uint16_t* const Gs = W2s + D * FFN16_LDG;                           // [64][FFN16_LDG]
    float* const Rs = (float*)(Gs + FFN16_ROWS * FFN16_LDG);            // [64]
    uint16_t* const Zs = (uint16_t*)(Rs + FFN16_ROWS);                  // [64][FFN16_LDZ]: the chunk's zs tile (TRAIN)

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hh = lane >> 5;
    const int rt = wave & 1, cw = wave >> 1;
    const long long row0 = (long long)blockIdx.x * FFN16_ROWS;
    const int q8 = D >> 3;                                   // 8-element pieces per row of x and of W1
    const int npiece = FFN16_CHUNK * q8;                     // pieces of a W1 tile = of a W2 tile (D rows of 8)
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- a chunk's weights, from memory into registers as bf16 operands: thread t moves the pieces t, t + 256, .. of each tile.  The
    // loads are issued without a branch (rows and columns past the edges read a real element, and the value is dropped)
    u32x4 wr1[NW], wr2[NW];
    auto load_w = [&](int j0) {
        const int wv = min(FFN16_CHUNK, H - j0);
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx / q8, c = idx - r * q8;
            const u32x4 a = ffn16_load8h<T>(W1 + (size_t)(j0 + min(r, wv - 1)) * D + 8 * c, vec);
            wr1[i] = idx < npiece && r < wv ? a : zero4;
            const int n = min(idx >> 3, D - 1), c2 = 8 * (idx & 7);
            const bool ok = idx < npiece && j0 + c2 < H;      // hidden is a multiple of 8: a piece lies inside it or past it
            const u32x4 b = ffn16_load8h<T>(W2 + (size_t)n * H + (ok ? j0 + c2 : 0), vec);
            wr2[i] = ok ? b : zero4;
        }
    };
    auto store_w = [&]() {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int idx = tid + 256 * i;
            const int r = idx / q8, c = idx - r * q8;
            if (idx < npiece) {
                *(u32x4*)(W1s + r * ldw1 + 8 * c) = wr1[i];
                *(u32x4*)(W2s + (idx >> 3) * FFN16_LDG + 8 * (idx & 7)) = wr2[i];
            }
        }
    };
    load_w(0);
    if (tid < FFN16_CHUNK) *(u32x4*)(W1s + tid * ldw1 + D) = zero4;      // the pad columns, once: no tile store touches them

    // ---- rs of the tile's rows: four threads per row, thread q the chain over k = q, q + 4, .. --------------------------------------------
    {
        const int r = tid >> 2, q = tid & 3;
        const long long t = row0 + r;
        float s = 0.0f;
        if (t < ntok) {
            const long long i0 = t / n1, i1 = t - i0 * n1;
            const T* const xr = x + i0 * xs0 + i1 * xs1;
            for (int m0 = 0; m0 < q8; m0 += 4) {             // four pieces in flight at once; a piece past the row reads its last one
                float v0[4], v1[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const Ffn16F8 f = ffn16_load8f<T>(xr + 8 * min(m0 + i, q8 - 1), vec);
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
        const float u = s + __shfl_xor(s, 1);                // q = 0, 1: s0 + s1;  q = 2, 3: s2 + s3
        const float w = u + __shfl_xor(u, 2);                // (s0 + s1) + (s2 + s3): the sum commutes, so every q holds the same bits
        if (q == 0) Rs[r] = rs_of(w, D, eps);
    }
    __syncthreads();

    // ---- this lane's token: its offsets and its layer-1 operand fragments ------------------------------------------------------------------
    const long long tok = row0 + rt * 32 + l31;
    const bool tok_ok = tok < ntok;
    long long xo = 0, oo = 0;
    if (tok_ok) {
        const long long i0 = tok / n1, i1 = tok - i0 * n1;
        xo = i0 * xs0 + i1 * xs1;
        oo = i0 * os0 + i1 * os1;
    }
    u32x4 xf[KS];
    {
        const float rs = Rs[rt * 32 + l31];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int c = 16 * s + 8 * hh;
            xf[s] = zero4;
            if (tok_ok && c < D) {
                const Ffn16F8 f = ffn16_load8f<T>(x + xo + c, vec);
#pragma unroll
                for (int e = 0; e < 4; ++e) xf[s][e] = cvt_pk_bf16(f.v[2 * e] * rs, f.v[2 * e + 1] * rs);
            }
        }
    }

    f32x16 acc[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;

    const uint16_t* const w1a = W1s + (cw * 32 + l31) * ldw1 + 8 * hh;          // layer 1's A operand: hidden column cw * 32 + l31 of the chunk
    uint16_t* const grow = Gs + (rt * 32 + l31) * FFN16_LDG;                     // this token's row of the gelu tile
    const uint16_t* w2a[NB];                                                     // layer 2's A operand: output column n
    bool on[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int n = (cw + 2 * i) * 32 + l31;
        on[i] = n < D;
        w2a[i] = W2s + min(n, D - 1) * FFN16_LDG + 8 * hh;
    }

    const int nch = (H + FFN16_CHUNK - 1) / FFN16_CHUNK;
    for (int ch = 0; ch < nch; ++ch) {
        const int j0 = ch * FFN16_CHUNK;
        store_w();                                           // the tiles were last read before the barrier that ends the previous chunk
        // b1 of this lane's 16 hidden columns (register r: column cw * 32 + 8 (r >> 2) + 4 hh + (r & 3)), asked for ahead of their use
        // and ahead of the next chunk's weights: loads return in order, and the gelu must not wait for those
        float bias[16];
        bool real[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + cw * 32 + 8 * (r >> 2) + 4 * hh + (r & 3);
            real[r] = j < H;
            if (!TRAIN || r < 4) bias[r] = to_f32(b1[min(j, H - 1)]);
        }
        if (ch + 1 < nch) load_w(j0 + FFN16_CHUNK);
        __syncthreads();
        // ---- layer 1: H^T block cw of the chunk -------------------------------------------------------------------------------------
        f32x16 h;
#pragma unroll
        for (int r = 0; r < 16; ++r) h[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s)
            if (16 * s < D) {
                const u32x4 a = *(const u32x4*)(w1a + 16 * s);
                h = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, xf[s]), h, 0, 0, 0);
            }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float v[4];
            if constexpr (TRAIN) {
                // zs = bf16(h) into the chunk's tile, a = gelu(h) * M1: this lane's token at four consecutive hidden columns
                uint32_t w[4];
                ffn16_draws4(tr.drop, 0, tok, j0 + cw * 32 + 8 * g + 4 * hh, w);
                float z[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    z[e] = h[r] + bias[r];
                    v[e] = real[r] && tok_ok ? masked(tr.drop, 0, w[e], gelu<float>(z[e])) : 0.0f;
                }
                if (g < 3) {                                 // the next group's b1: four values in flight, not sixteen held through the draws
#pragma unroll
                    for (int e = 0; e < 4; ++e) bias[4 * g + 4 + e] = to_f32(b1[min(j0 + cw * 32 + 8 * (g + 1) + 4 * hh + e, H - 1)]);
                }
                *(uint2*)(Zs + (rt * 32 + l31) * FFN16_LDZ + cw * 32 + 8 * g + 4 * hh) = make_uint2(cvt_pk_bf16(z[0], z[1]), cvt_pk_bf16(z[2], z[3]));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    v[e] = real[r] && tok_ok ? gelu<float>(h[r] + bias[r]) : 0.0f;
                }
            }
            *(uint2*)(grow + cw * 32 + 8 * g + 4 * hh) = make_uint2(cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]));
        }
        __syncthreads();                                     // Gs is written
        if constexpr (TRAIN) {
            // the zs tile to memory as whole 128-byte lines: 8 consecutive threads move one token's 64 columns of the chunk
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int idx = tid + 256 * i;
                const int r = idx >> 3, c = 8 * (idx & 7);
                if (row0 + r < ntok && j0 + c < H)            // hidden is a multiple of 8: a piece lies inside it or past it
                    *(u32x4*)(tr.zs + (size_t)(row0 + r) * H + j0 + c) = *(const u32x4*)(Zs + r * FFN16_LDZ + c);
            }
        }
        // ---- layer 2: out^T blocks cw, cw + 2, .. on the running accumulators ----------------------------------------------------------
#pragma unroll
        for (int s = 0; s < FFN16_CHUNK / 16; ++s) {
            const u32x4 b = *(const u32x4*)(grow + 16 * s + 8 * hh);
#pragma unroll
            for (int i = 0; i < NB; ++i)
                if (cw + 2 * i < DB) {                       // wave-uniform: a block past D (DB odd, cw = 1) is skipped
                    u32x4 a = *(const u32x4*)(w2a[i] + 16 * s);
                    a = on[i] ? a : zero4;
                    acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc[i], 0, 0, 0);
                }
        }
        __syncthreads();                                     // the tiles and Gs are free for the next chunk
    }

    // ---- x + (acc + b2) * scale: register group g of block i holds the columns (cw + 2 i) * 32 + 8 g + 4 hh .. + 3 of this token ---------
    if constexpr (TRAIN) {
        // y = acc + b2 (saved, rounded to T), out = x + (y * M2) * scale; the quad shares its draws, so every lane walks the columns
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = (cw + 2 * i) * 32 + 8 * g + 4 * hh;
                if (cw + 2 * i < DB) {                       // wave-uniform
                    uint32_t w[4];
                    ffn16_draws4(tr.drop, 1, tok, min(n, D - 4), w);
                    if (tok_ok && n < D) {
                        float xv[4], y[4], o[4];
                        ffn16_load4f(x + xo + n, ovec, xv);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            y[e] = acc[i][4 * g + e] + to_f32(b2[n + e]);
                            o[e] = xv[e] + masked(tr.drop, 1, w[e], y[e]) * to_f32(scale[n + e]);
                        }
                        ffn16_store4(tr.ys + (size_t)tok * D + n, true, y);      // ys is dense and 256-byte aligned
                        ffn16_store4(out + oo + n, ovec, o);
                    }
                }
            }
    } else if (tok_ok) {
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = (cw + 2 * i) * 32 + 8 * g + 4 * hh;
                if (cw + 2 * i < DB && n < D) {              // D is a multiple of 8 and n of 4: all four columns or none
                    float xv[4], o[4];
                    ffn16_load4f(x + xo + n, ovec, xv);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = epilogue(xv[e], acc[i][4 * g + e], to_f32(b2[n + e]), to_f32(scale[n + e]));
                    ffn16_store4(out + oo + n, ovec, o);
                }
            }
    }
}

template <typename T, int DB>
static void ffn16_launch_one(const T* x, T* out, long long ntok, long long n1, long long xs0, long long xs1, long long os0, long long os1, int D,
                             int H, const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps, int vec, int ovec,
                             hipStream_t stream)
{
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)ffn_residual_bf16_kernel<T, DB>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes_bf16(DB * 32));
    hipLaunchKernelGGL((ffn_residual_bf16_kernel<T, DB>), dim3((unsigned)((ntok + FFN16_ROWS - 1) / FFN16_ROWS)), dim3(256), lds_bytes_bf16(D), stream, x,
                       out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, vec, ovec);
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and n0 n1 < 2^37
template <typename T>
static void ffn16_launch(const T* x, T* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1, int D, int H,
                         const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps, hipStream_t stream)
{
    // 16-byte loads of 8 bf16 / 4 floats: every base 16-byte aligned, every stride a multiple of 16 bytes (D and H are multiples of 8)
    constexpr long long EL = 16 / sizeof(T);
    const int vec = ((((uintptr_t)x | (uintptr_t)W1 | (uintptr_t)W2) & 15) == 0) && ((xs0 | xs1) & (EL - 1)) == 0;
    // the epilogue's four columns: 8 bytes (bf16) or 16 bytes (fp32) of x and of out
    const int ovec = ((((uintptr_t)x | (uintptr_t)out) & (4 * sizeof(T) - 1)) == 0) && ((xs0 | xs1 | os0 | os1) & 3) == 0;
    const long long ntok = n0 * n1;
#define SEMICRF_FFN16_CASE(N) \
    case N: ffn16_launch_one<T, N>(x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, vec, ovec, stream); break
    switch ((D + 31) / 32) {
        SEMICRF_FFN16_CASE(1); SEMICRF_FFN16_CASE(2); SEMICRF_FFN16_CASE(3); SEMICRF_FFN16_CASE(4);
        SEMICRF_FFN16_CASE(5); SEMICRF_FFN16_CASE(6); SEMICRF_FFN16_CASE(7); SEMICRF_FFN16_CASE(8);
    }
#undef SEMICRF_FFN16_CASE
}

// ---- the training mode: the same geometry, the zs tile more in LDS; the saved buffer is laid out as ffn_bf16_train_math.h says -------------
template <typename T, int DB>
static void ffn16_train_launch_one(const T* x, T* out, long long ntok, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                                   int D, int H, const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps, int vec, int ovec,
                                   const Ffn16Train<T>& tr, hipStream_t stream)
{
    static PerDeviceOnce once;
    if (once.first())
        (void)hipFuncSetAttribute((const void*)ffn_residual_bf16_kernel<T, DB, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds_bytes_bf16_train(DB * 32));
    hipLaunchKernelGGL((ffn_residual_bf16_kernel<T, DB, true>), dim3((unsigned)((ntok + FFN16_ROWS - 1) / FFN16_ROWS)), dim3(256),
                       lds_bytes_bf16_train(D), stream, x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, vec, ovec, tr);
}

template <typename T>
static void ffn16_train_launch(const T* x, T* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1, int D,
                               int H, const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps, unsigned long long seed,
                               double p1, double p2, void* saved, hipStream_t stream)
{
    constexpr long long EL = 16 / sizeof(T);
    const int vec = ((((uintptr_t)x | (uintptr_t)W1 | (uintptr_t)W2) & 15) == 0) && ((xs0 | xs1) & (EL - 1)) == 0;
    const int ovec = ((((uintptr_t)x | (uintptr_t)out) & (4 * sizeof(T) - 1)) == 0) && ((xs0 | xs1 | os0 | os1) & 3) == 0;
    const long long ntok = n0 * n1;
    const Ffn16Train<T> tr{attr_heads::dropout_params(seed, p1, p2), (uint16_t*)saved, (T*)((unsigned char*)saved + train_saved_ys_offset(ntok, H))};
#define SEMICRF_FFN16_CASE(N) \
    case N: ffn16_train_launch_one<T, N>(x, out, ntok, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, vec, ovec, tr, stream); break
    switch ((D + 31) / 32) {
        SEMICRF_FFN16_CASE(1); SEMICRF_FFN16_CASE(2); SEMICRF_FFN16_CASE(3); SEMICRF_FFN16_CASE(4);
        SEMICRF_FFN16_CASE(5); SEMICRF_FFN16_CASE(6); SEMICRF_FFN16_CASE(7); SEMICRF_FFN16_CASE(8);
    }
#undef SEMICRF_FFN16_CASE
}

void launch_ffn_residual_bf16_train(const uint16_t* x, uint16_t* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                                    long long os1, int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2,
                                    const uint16_t* scale, float eps, unsigned long long seed, double p1, double p2, void* saved, hipStream_t stream)
{
    ffn16_train_launch<uint16_t>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, seed, p1, p2, saved, stream);
}

void launch_ffn_residual_bf16_mixed_train(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0,
                                          long long os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                                          const float* scale, float eps, unsigned long long seed, double p1, double p2, void* saved,
                                          hipStream_t stream)
{
    ffn16_train_launch<float>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, seed, p1, p2, saved, stream);
}

void launch_ffn_residual_bf16(const uint16_t* x, uint16_t* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                              int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale,
                              float eps, hipStream_t stream)
{
    ffn16_launch<uint16_t>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream);
}

void launch_ffn_residual_bf16_mixed(const float* x, float* out, long long n0, long long n1, long long xs0, long long xs1, long long os0, long long os1,
                                    int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                                    hipStream_t stream)
{
    ffn16_launch<float>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, stream);
}

}  // namespace semicrf
