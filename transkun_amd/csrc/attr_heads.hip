// attr_heads.hip -- the two attribute heads of transcription, from the packed decode output straight to their raw outputs
// (TransKun.transcribeFrames, ModelTransformer.py:578-590, :638; the heads of :112-128): per interval i of chain c, (b, e) = pairs[i],
//   x_i               = [ ctx[c,b,:] | ctx[c,e,:] | ctx[c,b,:] * ctx[c,e,:] ]            3 D values, never written to HBM
//   logitsVelocity[i] = W2v gelu(W1v x_i + b1v) + b2v                                     [Nv]
//   ofLogits[i]       = W2o gelu(W1o x_i + b1o) + b2o                                     [No]
// in exact fp32 on the matrix pipe (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).  TRAIN = false: inference (dropout is the
// identity).  TRAIN = true (semicrf_attribute_heads_train_fwd): the same chain per output element, with z = W1 x + b1 saved for the
// backward (attr_heads_bwd.hip) and, for a head with p > 0, the dropout mask of attr_heads_math.h between gelu and layer 2.
//
// Grid = (row tiles of 64 intervals) x (slices of 64 hidden columns, the velocity head's first): at the model's K = 1400 rows the
// row tiles alone are 22 workgroups, with the 16 slices of Hv = Ho = 512 they are 352.  The slice count depends on Hv and Ho only.
// A workgroup (4 waves, one 32 x 32 block of the 64 x 64 hidden tile each):
//   layer 1   the contraction over k = 0 .. 3D-1 in chunks of 32: the chunk of x is gathered from the rows of ctx (the product third
//             formed on the fly) and the chunk of the packed W1 = [3D][Hv + Ho] is copied, both k-major into LDS (rows of 96 floats:
//             the two half waves of an operand read hit disjoint banks); two LDS stages and one register stage: chunk n multiplies
//             while chunk n + 1 is written to the other stage and chunk n + 2 is on its way from memory, one barrier per chunk;
//             16 matrix instructions per wave and chunk on one accumulator
//   gelu      + b1, gelu (attr_heads_math.h), into LDS as the A operand of layer 2 (the same memory, after a barrier)
//   layer 2   hidden tile [64 x 64] x the slice's rows of W2^T [64 x N]: wave w takes the column blocks w, w + 4, ... of 32 outputs and
//             both row blocks; B comes straight from global memory (L2-resident, coalesced), requested before the gelu
//   partial   [rows x N] into the workspace, plane `slice` of its head
// A second kernel adds a head's planes in ascending slice order and the bias last.  No atomics: every output element is one fixed
// chain of operations -- bit-identical whatever K is, wherever the row sits and whatever other rows hold.  Ragged edges (3D, the
// last slice of a head, the rows past K, N) are padded with exact zeros; rows past K are computed on zeros and never stored.
#include "common.h"
#include "launchers.h"
#include "chain_search.h"
#include "attr_heads_math.h"

namespace semicrf {

using namespace attr_heads;

typedef float heads_f32x16 __attribute__((ext_vector_type(16)));

constexpr int HEADS_LDT = 96;        // floats per k row of the layer-1 operand tiles (64 used)
constexpr int HEADS_LDH = 97;        // floats per hidden column of the gelu tile (64 used)
static_assert(HEADS_ROWS == 64 && HEADS_SLICE == 64 && HEADS_KCHUNK == 32, "the lane maps below are written for 64 x 64 x 32");
constexpr int HEADS_STAGE = 2 * HEADS_KCHUNK * HEADS_LDT;   // floats of one stage: the x chunk, then the W1 chunk
constexpr int HEADS_SMEM = 2 * HEADS_STAGE > HEADS_SLICE * HEADS_LDH ? 2 * HEADS_STAGE : HEADS_SLICE * HEADS_LDH;

// row of a 32 x 32 result block held in accumulator register r of a lane in half wave hh (the column is lane & 31)
__device__ __forceinline__ int heads_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

template <bool VEC, bool TRAIN>
__global__ __launch_bounds__(256, 2) void attr_heads_kernel(const float* __restrict__ ctx, int C, int T, int D, long long ldc,
                                                         const int* __restrict__ pairs, int K, const int* __restrict__ offsets, int nSym,
                                                         const float* __restrict__ W1, const float* __restrict__ b1,
                                                         const float* __restrict__ W2, int Hv, int Ho, int Nv, int No,
                                                         float* __restrict__ ws, long long* __restrict__ symIdx,
                                                         long long* __restrict__ scatterIdx, float* __restrict__ zsave, DropoutParams drop)
{
    __shared__ __attribute__((aligned(16))) float smem[HEADS_SMEM];
    // two stages of {x chunk [32 k][96], W1 chunk [32 k][96]}, k-major; after layer 1 the gelu tile [64 hidden][97] takes their place
    float* const Hs = smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int row0 = blockIdx.x * HEADS_ROWS;
    const int Sv = slices_of(Hv);
    const int s = blockIdx.y;
    const bool vel = s < Sv;
    const int sl = vel ? s : s - Sv;                          // slice within its head
    const int Hh = vel ? Hv : Ho, N = vel ? Nv : No;
    const int hcol0 = sl * HEADS_SLICE;                       // first hidden column, within the head
    const int wv = min(HEADS_SLICE, Hh - hcol0);              // columns of this slice that exist
    const int pcol0 = (vel ? 0 : Hv) + hcol0;                 // the same column in the packed W1 / b1
    const long long ldw = (long long)Hv + Ho;
    const int nk = 3 * D;

    // the row this thread gathers (always the same one): element offsets of its two frames, -1 past K
    const int gr = tid & 63;
    long long ra = -1, rb = -1;
    {
        const int i = row0 + gr;
        if (i < K) {
            const int c = chain_of_interval(offsets, C, i);
            const int b = min(max(pairs[2 * (size_t)i], 0), T - 1), e = min(max(pairs[2 * (size_t)i + 1], 0), T - 1);
            ra = ((long long)c * T + b) * ldc;
            rb = ((long long)c * T + e) * ldc;
            if (s == 0 && wave == 0) {
                if (symIdx) symIdx[i] = c % nSym;
                if (scatterIdx) scatterIdx[i] = c;
            }
        }
    }

    float xr[8], wr[8];
    auto x_at = [&](int k) -> float {
        if (ra < 0 || k >= nk) return 0.0f;
        if (k < D) return ctx[ra + k];
        if (k < 2 * D) return ctx[rb + (k - D)];
        return ctx[ra + (k - 2 * D)] * ctx[rb + (k - 2 * D)];
    };
    auto x4_at = [&](int k) -> float4 {                       // VEC: D % 4 == 0, so the four values lie in one third
        if (ra < 0 || k >= nk) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < D) return *(const float4*)(ctx + ra + k);
        if (k < 2 * D) return *(const float4*)(ctx + rb + (k - D));
        const float4 a = *(const float4*)(ctx + ra + (k - 2 * D)), b = *(const float4*)(ctx + rb + (k - 2 * D));
        return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
    };
    auto load_chunk = [&](int k0) {
        if (VEC) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const float4 v = x4_at(k0 + 4 * ((tid >> 6) + 4 * p));
                xr[4 * p] = v.x; xr[4 * p + 1] = v.y; xr[4 * p + 2] = v.z; xr[4 * p + 3] = v.w;
                const int kk = (tid >> 4) + 16 * p, j = 4 * (tid & 15);
                float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (k0 + kk < nk && j < wv) w = *(const float4*)(W1 + (long long)(k0 + kk) * ldw + pcol0 + j);
                wr[4 * p] = w.x; wr[4 * p + 1] = w.y; wr[4 * p + 2] = w.z; wr[4 * p + 3] = w.w;
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int kk = (tid >> 6) + 4 * p;
                xr[p] = x_at(k0 + kk);
                wr[p] = (k0 + kk < nk && gr < wv) ? W1[(long long)(k0 + kk) * ldw + pcol0 + gr] : 0.0f;
            }
        }
    };
    auto store_chunk = [&](int stage) {
        float* const Xs = smem + stage * HEADS_STAGE;
        float* const Ws = Xs + HEADS_KCHUNK * HEADS_LDT;
        if (VEC) {
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int kg = (tid >> 6) + 4 * p;
#pragma unroll
                for (int j = 0; j < 4; ++j) Xs[(4 * kg + j) * HEADS_LDT + gr] = xr[4 * p + j];
                const int kk = (tid >> 4) + 16 * p;
                *(float4*)(Ws + kk * HEADS_LDT + 4 * (tid & 15)) = make_float4(wr[4 * p], wr[4 * p + 1], wr[4 * p + 2], wr[4 * p + 3]);
            }
        } else {
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int kk = (tid >> 6) + 4 * p;
                Xs[kk * HEADS_LDT + gr] = xr[p];
                Ws[kk * HEADS_LDT + gr] = wr[p];
            }
        }
    };

    // ---- layer 1: wave = block (rt, ct) of the 64 x 64 hidden tile ----------------------------------------------------------
    const int rt = wave >> 1, ct = wave & 1;
    heads_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    const int nch = (nk + HEADS_KCHUNK - 1) / HEADS_KCHUNK;
    // chunk ch multiplies out of stage ch & 1 while chunk ch + 1 (in registers since the previous step) goes into the other stage
    // and chunk ch + 2 is requested from memory: one barrier per chunk, a whole chunk of matrix work behind every global load
    load_chunk(0);
    store_chunk(0);
    if (nch > 1) load_chunk(HEADS_KCHUNK);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        if (ch + 1 < nch) store_chunk((ch + 1) & 1);          // that stage was last read before the previous barrier
        if (ch + 2 < nch) load_chunk((ch + 2) * HEADS_KCHUNK);
        const float* xa = smem + (ch & 1) * HEADS_STAGE + hh * HEADS_LDT + rt * 32 + l31;
        const float* wb = smem + (ch & 1) * HEADS_STAGE + HEADS_KCHUNK * HEADS_LDT + hh * HEADS_LDT + ct * 32 + l31;
#pragma unroll
        for (int m = 0; m < HEADS_KCHUNK / 2; ++m)            // instruction m: k = 2 m (lanes 0-31) and 2 m + 1 (lanes 32-63)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * m * HEADS_LDT], wb[2 * m * HEADS_LDT], acc, 0, 0, 0);
        __syncthreads();                                      // both stages' next use is ordered behind this chunk's reads
    }

    // ---- layer 2's B operand of this wave's first column block, requested before the gelu so that its latency hides there --------
    const float* W2h = (vel ? W2 : W2 + (size_t)Hv * Nv) + (size_t)hcol0 * N;
    float bv[HEADS_SLICE / 2];
    auto load_b = [&](int nb) {
        const int n = nb * 32 + l31;
#pragma unroll
        for (int m = 0; m < HEADS_SLICE / 2; ++m) {
            const int j = 2 * m + hh;
            bv[m] = (n < N && j < wv) ? W2h[(size_t)j * N + n] : 0.0f;
        }
    };
    if (wave * 32 < N) load_b(wave);

    // ---- + b1, gelu -> Hs[hidden column][row] -----------------------------------------------------------------------------------
    {
        const int col = ct * 32 + l31;
        const bool real = col < wv;
        const float bias = real ? b1[pcol0 + col] : 0.0f;
        if (!TRAIN) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * 32 + heads_acc_row(r, hh);
                Hs[col * HEADS_LDH + row] = real ? gelu<float>(acc[r] + bias) : 0.0f;
            }
        } else {
            const int head = vel ? 0 : 1;
            const bool masked = drop.on[head] != 0;
            const unsigned thr = drop.thr[head];
            const float scale = drop.scale[head];
#pragma unroll
            for (int q = 0; q < 4; ++q) {                     // registers 4 q .. 4 q + 3: four consecutive rows from a multiple of 4
                const int rowq = rt * 32 + heads_acc_row(4 * q, hh);
                uint32_t draw[4] = {0u, 0u, 0u, 0u};
                if (masked) dropout_draws(drop.seed, (uint32_t)((row0 + rowq) >> 2), (uint32_t)(pcol0 + col), draw);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int row = rowq + u;
                    const float zz = acc[4 * q + u] + bias;
                    float g = gelu<float>(zz);
                    if (masked) g = draw[u] >= thr ? g * scale : 0.0f;
                    Hs[col * HEADS_LDH + row] = real ? g : 0.0f;
                    if (real && row0 + row < K) zsave[(size_t)(row0 + row) * (size_t)ldw + pcol0 + col] = zz;
                }
            }
        }
    }
    __syncthreads();

    // ---- layer 2: [64 rows x 64 hidden] x W2^T[hidden][N], 32 output columns per pass -----------------------------------------
    float* part = (vel ? ws + (size_t)sl * K * Nv : ws + (size_t)Sv * K * Nv + (size_t)sl * K * No);
    for (int nb = wave; nb * 32 < N; nb += 4) {
        const int n = nb * 32 + l31;
        const bool ncol = n < N;
        heads_f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        if (nb != wave) load_b(nb);
#pragma unroll
        for (int m = 0; m < HEADS_SLICE / 2; ++m) {
            const int j = 2 * m + hh;
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Hs[j * HEADS_LDH + l31], bv[m], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Hs[j * HEADS_LDH + 32 + l31], bv[m], acc1, 0, 0, 0);
            if ((m & 7) == 7) __builtin_amdgcn_sched_barrier(0);              // (keeps the LDS reads of all 32 steps from being hoisted at once)
        }
        if (ncol) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i0 = row0 + heads_acc_row(r, hh), i1 = i0 + 32;
                if (i0 < K) part[(size_t)i0 * N + n] = acc0[r];
                if (i1 < K) part[(size_t)i1 * N + n] = acc1[r];
            }
        }
    }
}

// out = ((plane 0 + plane 1) + ...) + b2, one thread per output element
__global__ __launch_bounds__(256) void attr_heads_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ b2, int K, int Sv,
                                                                int So, int Nv, int No, float* __restrict__ logitsVelocity,
                                                                float* __restrict__ ofLogits)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long nv = (long long)K * Nv, no = (long long)K * No;
    if (idx < nv) {
        float t = ws[idx];
        for (int s = 1; s < Sv; ++s) t += ws[(long long)s * nv + idx];
        logitsVelocity[idx] = t + b2[idx % Nv];
    } else if (idx < nv + no) {
        const long long j = idx - nv;
        const float* w = ws + (long long)Sv * nv;
        float t = w[j];
        for (int s = 1; s < So; ++s) t += w[(long long)s * no + j];
        ofLogits[j] = t + b2[Nv + j % No];
    }
}

size_t attr_heads_workspace_bytes(long long K, int Hv, int Ho, int Nv, int No)
{
    const size_t per_row = (size_t)slices_of(Hv) * Nv + (size_t)slices_of(Ho) * No;
    return align_up((size_t)(K > 0 ? K : 0) * per_row * sizeof(float) + 256);
}

void launch_attr_heads(const float* ctx, int C, int T, int D, long long ldc, const int* pairs, int K, const int* offsets, int nSym,
                       const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                       float* logitsVelocity, float* ofLogits, long long* symIdx, long long* scatterIdx, float* ws, hipStream_t stream,
                       float* zsave, unsigned long long seed, double pv, double po)
{
    if (K <= 0) return;
    const DropoutParams drop = dropout_params(seed, zsave ? pv : 0.0, zsave ? po : 0.0);
    const int Sv = slices_of(Hv), So = slices_of(Ho);
    const dim3 grid((K + HEADS_ROWS - 1) / HEADS_ROWS, Sv + So), block(256);
    const bool vec = (D & 3) == 0 && (ldc & 3) == 0 && (Hv & 3) == 0 && (Ho & 3) == 0 && (((uintptr_t)ctx | (uintptr_t)W1) & 15) == 0;
    // zsave != nullptr: the training forward (z saved, dropout by pv / po)
#define SEMICRF_HEADS_LAUNCH(VEC, TRAIN)                                                                                                  \
    hipLaunchKernelGGL((attr_heads_kernel<VEC, TRAIN>), grid, block, 0, stream, ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, Hv, \
                       Ho, Nv, No, ws, symIdx, scatterIdx, zsave, drop)
    if (zsave) {
        if (vec) SEMICRF_HEADS_LAUNCH(true, true); else SEMICRF_HEADS_LAUNCH(false, true);
    } else {
        if (vec) SEMICRF_HEADS_LAUNCH(true, false); else SEMICRF_HEADS_LAUNCH(false, false);
    }
#undef SEMICRF_HEADS_LAUNCH
    const long long total = (long long)K * ((long long)Nv + No);
    hipLaunchKernelGGL(attr_heads_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, ws, b2, K, Sv, So, Nv, No,
                       logitsVelocity, ofLogits);
}

}  // namespace semicrf
