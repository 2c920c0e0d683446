// sample.hip -- exact posterior sampling of interval paths (forward-filtering backward-sampling).
//
// Given alpha (v [T][B] of semicrf_logz_fwd), the walk from the END towards frame 0 is a Markov chain: at a visited frame t > 0
// the predecessor is drawn from the candidates [skip, j = t-1, t-2, ..., 0] with weights exp(v[t-1] + n[t-1]) and
// exp(v[j] + s[t,j]), and the singleton (t,t) is emitted with probability sigmoid(s[t,t]).  Every frame's draw depends on alpha
// and on that frame's score row only, so the whole code table -- one drawn predecessor per (draw, chain, frame) -- is produced
// in ONE pass over the lower triangle for all draws of the call; the walk itself is decode.hip's launch_backtrack (forward = 1).
//
// code[k*B + c][t] = (pred+1) | (singleton ? CODE_DIAG : 0), pred = -1 for skip: the layout decode.hip reads.
//
// Random numbers: u = (splitmix64(idx, key) >> 40) * 2^-24, idx = ((k*B + c)*T + t)*2 + r (k the global draw index, r = 0 for the
// predecessor, 1 for the singleton) -- the same uniforms as the host kernel (cpu_ops.cpp) and transkun_amd.synth.hash_u64_*.
#include "common.h"
#include "launchers.h"

namespace semicrf {

constexpr int SMP_CODE_DIAG = 0x40000000;      // decode.hip: CODE_DIAG
constexpr int SMP_WAVES = 8;                   // one workgroup = one row t x 64 chains (a lane per chain) x 8 waves
constexpr int SMP_NCH = 128;                   // at most this many chunk summaries per (row, chain): 32 KB of LDS
constexpr int SMP_BATCH = 16;                  // loads in flight per lane; a chunk is a whole number of batches

__host__ __device__ inline uint64_t splitmix64(uint64_t idx, uint64_t key)
{
    uint64_t z = idx + key * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ float uniform24(uint64_t idx, uint64_t key)
{
    return (float)(uint32_t)(splitmix64(idx, key) >> 40) * (1.0f / 16777216.0f);
}

// candidate i of row t (i = 0: skip, i >= 1: the interval (t - i, t)), natural-log weight
__device__ __forceinline__ float cand_logw(const float* __restrict__ score, const float* __restrict__ noise,
                                           const float* __restrict__ v, int T, int B, int t, int c, int i)
{
    if (i == 0) return v[(size_t)(t - 1) * B + c] + noise[(size_t)(t - 1) * B + c];
    const int j = t - i;
    return v[(size_t)j * B + c] + score[((size_t)t * T + j) * B + c];
}

// grid T * ceil(B/64), chain tile fastest, rows from t = T-1 down (longest first).  Phase 1 streams the row once: per chunk of
// CH candidates the log of its weight sum (max-shifted).  Phase 2 turns the chunk sums into prefix sums P (shift M = the row's max).  Phase 3, per
// draw: the chunk by binary search over P, then the candidate by rescanning that chunk only (CH cells, L2).
__global__ __launch_bounds__(64 * SMP_WAVES) void sample_code_kernel(const float* __restrict__ score, const float* __restrict__ noise,
                                                                    const float* __restrict__ v, int T, int B, long long k0,
                                                                    int nSample, unsigned long long key, const int* __restrict__ end,
                                                                    int* __restrict__ code, int* __restrict__ start,
                                                                    unsigned* __restrict__ err)
{
    __shared__ float s_p[SMP_NCH][64];          // chunk log-sums, then their prefix sums exp(L - M)
    __shared__ float s_red[SMP_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntile = (B + 63) / 64;
    const int c = (int)(blockIdx.x % ntile) * 64 + lane;
    const int t = T - 1 - (int)(blockIdx.x / ntile);
    const bool act = c < B;
    const int ncand = t >= 1 ? t + 1 : 0;
    const int CH = SMP_BATCH * ((ncand + SMP_NCH * SMP_BATCH - 1) / (SMP_NCH * SMP_BATCH));
    const int nch = (ncand + CH - 1) / CH;
    // chunks [q0, q1) of this wave (contiguous ranges: the prefix sums below run per wave)
    const int per = (nch + SMP_WAVES - 1) / SMP_WAVES;
    const int q0 = min(nch, wave * per), q1 = min(nch, q0 + per);

    if (t == 0 && act && wave == 0) {
        for (int k = 0; k < nSample; ++k) start[(size_t)k * B + c] = end ? end[c] : T - 1;
        // a sweep that gave up on a bounded wait leaves NaN in the last row of alpha: the total comes back as -1
        if (v[(size_t)(T - 1) * B + c] != v[(size_t)(T - 1) * B + c]) err[0] = 0u;
    }

    // ---- phase 1: chunk log-sums, relative to R = v[t] - softplus(s[t,t]) (alpha's log of the row total, when finite): the stored
    // values are then small numbers, whose float rounding does not move the weights (absolute log-sums ~1e3 would: 6e-5 per ulp)
    const float dg = act ? score[((size_t)t * T + t) * B + c] : 0.0f;
    float R = act ? v[(size_t)t * B + c] - softplus_f(dg) : 0.0f;
    if (!(fabsf(R) < INFINITY)) R = 0.0f;
    float wmax = -INFINITY;
    for (int q = q0; q < q1; ++q) {
        const int i0 = q * CH, i1 = min(ncand, i0 + CH);
        float m = -INFINITY, s = 0.0f;
        for (int b = i0; b < i1; b += SMP_BATCH) {
            float x[SMP_BATCH];
            float bm = -INFINITY;
#pragma unroll
            for (int u = 0; u < SMP_BATCH; ++u) {
                x[u] = (act && b + u < i1) ? cand_logw(score, noise, v, T, B, t, c, b + u) - R : -INFINITY;
                bm = fmaxf(bm, x[u]);
            }
            if (bm == -INFINITY) continue;
            if (bm > m) { s *= expf(m - bm); m = bm; }
#pragma unroll
            for (int u = 0; u < SMP_BATCH; ++u) s += expf(x[u] - m);
        }
        const float L = s > 0.0f ? m + logf(s) : -INFINITY;
        s_p[q][lane] = L;
        wmax = fmaxf(wmax, L);
    }
    s_red[wave][lane] = wmax;
    __syncthreads();
    float M = s_red[0][lane];
#pragma unroll
    for (int w = 1; w < SMP_WAVES; ++w) M = fmaxf(M, s_red[w][lane]);
    __syncthreads();

    // ---- phase 2: prefix sums of exp(L - M), per wave, then the waves' offsets
    float run = 0.0f;
    if (M != -INFINITY)
        for (int q = q0; q < q1; ++q) { run += expf(s_p[q][lane] - M); s_p[q][lane] = run; }
    s_red[wave][lane] = run;
    __syncthreads();
    float off = 0.0f;
#pragma unroll
    for (int w = 0; w < SMP_WAVES; ++w)
        if (w < wave) off += s_red[w][lane];
    if (off != 0.0f)
        for (int q = q0; q < q1; ++q) s_p[q][lane] += off;
    __syncthreads();
    if (!act) return;
    const float Z = nch > 0 && M != -INFINITY ? s_p[nch - 1][lane] : 0.0f;     // the row's own total

    // ---- phase 3: the draws of this (row, chain)
    const float pdiag = 1.0f / (1.0f + expf(-dg));
    for (int k = wave; k < nSample; k += SMP_WAVES) {
        const uint64_t base = ((uint64_t)(k0 + k) * (uint64_t)B + (uint64_t)c) * (uint64_t)T + (uint64_t)t;
        int pred = -1;
        if (ncand > 0 && Z > 0.0f) {
            const float thr = uniform24(base * 2u, key) * Z;
            // first chunk whose prefix exceeds thr; past the end (rounding): the first chunk that reaches the total -- the last
            // chunk of positive weight
            int lo = 0, hi = nch - 1;
            const bool past = !(Z > thr);
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const float p = s_p[mid][lane];
                if (past ? (p >= Z) : (p > thr)) hi = mid; else lo = mid + 1;
            }
            const int q = lo;
            float acc = q > 0 ? s_p[q - 1][lane] : 0.0f;
            const int i0 = q * CH, i1 = min(ncand, i0 + CH);
            int last = -1, hit = -1;
            for (int i = i0; i < i1; ++i) {
                const float w = expf((cand_logw(score, noise, v, T, B, t, c, i) - R) - M);
                if (w > 0.0f) {
                    last = i;
                    acc += w;
                    if (!past && acc > thr) { hit = i; break; }
                }
            }
            const int i = hit >= 0 ? hit : last;
            pred = i <= 0 ? -1 : t - i;
        }
        const bool diag = uniform24(base * 2u + 1u, key) < pdiag;
        code[((size_t)k * B + c) * T + t] = (pred + 1) | (diag ? SMP_CODE_DIAG : 0);
    }
}

size_t sample_workspace_bytes(int T, int nB)
{
    // code [nB][T], region [nB][2T][2], counts [nB], start [nB], the error word
    return align_up((size_t)nB * T * 4) + align_up((size_t)nB * 2 * T * 2 * 4) + align_up((size_t)nB * 4) * 2 + 256 + 4096;
}

void launch_sample(const float* score, const float* noise, const float* v, int T, int B, long long k0, int nSample,
                   unsigned long long key, const int* end, int* pairs, long long cap, int* offsets, void* ws, hipStream_t stream)
{
    const size_t nB = (size_t)nSample * B;
    char* p = (char*)ws;
    int* code = (int*)p;   p += align_up(nB * T * 4);
    int* region = (int*)p; p += align_up(nB * 2 * T * 2 * 4);
    int* counts = (int*)p; p += align_up(nB * 4);
    int* start = (int*)p;  p += align_up(nB * 4);
    unsigned* err = (unsigned*)p;
    (void)hipMemsetAsync(err, 0xff, sizeof(unsigned), stream);
    hipLaunchKernelGGL(sample_code_kernel, dim3((unsigned)T * (unsigned)((B + 63) / 64)), dim3(64 * SMP_WAVES), 0, stream, score, noise, v, T, B, k0,
                       nSample, key, end, code, start, err);
    launch_backtrack(code, T, (int)nB, start, 1, region, counts, pairs, cap, offsets, stream, err, 1, 0);
}

}  // namespace semicrf
