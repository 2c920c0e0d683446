// optim.hip -- the optimizer step on flat fp32 buffers (replaces train.py:239-246: the clip value from the norm history, clip_grad_norm_,
// the host read of the norm and torch_optimizer.AdaBelief's loop over 182 parameters) as three launches:
//   grad_sqnorm        workgroup i sums the squares of its share of the flat gradient in double -> partials[i].  A lane adds its float4s
//                      in ascending order, the lanes of a wave meet by xor-shuffles (every lane ends with the same bits), the 16 waves
//                      are added in wave order: the grid and every order of addition follow from numel alone.  No atomics.
//   clip_from_history  ONE workgroup: thread 0 adds the partials in index order and takes the root (double); all 1024 threads sort a
//                      copy of the norm ring in LDS (bitonic, padded with +inf to a power of two) for the quantile; thread 0
//                      interpolates, forms coef = min(1, clip / (norm + 1e-6)), writes {norm, clip, coef} and appends the norm.
//   adabelief_step     a grid-stride stream over p, g, m, s (28 bytes per element): 16-byte accesses, the update of optim_math.h per
//                      element.  The groups' factors arrive by value; a work item runs over the (at most 8) groups with a compile-time
//                      index -- no table in memory -- and an access that crosses a boundary gives each element its own group.
#include <algorithm>
#include "common.h"
#include "launchers.h"
#include "optim_math.h"

namespace semicrf {

using namespace optim;

__global__ __launch_bounds__(SQNORM_BLOCK) void grad_sqnorm_kernel(const float* __restrict__ flat, long long numel, int head,
                                                                    double* __restrict__ partials)
{
    // flat + head is 16-byte aligned (head < 4 scalar elements in front, fewer than 4 behind the float4 body)
    const int tid = threadIdx.x;
    const long long nq = (numel - head) / 4;
    const int tail = (int)(numel - head - 4 * nq);
    const float4* __restrict__ body = (const float4*)(flat + head);
    double acc = 0.0;
    for (long long q = (long long)blockIdx.x * SQNORM_BLOCK + tid; q < nq; q += (long long)gridDim.x * SQNORM_BLOCK) {
        const float4 v = body[q];
        acc += (double)v.x * (double)v.x;
        acc += (double)v.y * (double)v.y;
        acc += (double)v.z * (double)v.z;
        acc += (double)v.w * (double)v.w;
    }
    if (blockIdx.x == 0) {                                   // the edges: one element per lane of workgroup 0
        if (tid < head) { const double x = flat[tid]; acc += x * x; }
        if (tid >= 64 && tid - 64 < tail) { const double x = flat[head + 4 * nq + (tid - 64)]; acc += x * x; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    __shared__ double wsum[SQNORM_BLOCK / WAVE];
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
#pragma unroll
        for (int w = 1; w < SQNORM_BLOCK / WAVE; ++w) t += wsum[w];
        partials[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void clip_from_history_kernel(const double* __restrict__ partials, int nparts,
                                                                 const float* __restrict__ norm_in, double q, float* __restrict__ ring,
                                                                 int capacity, int* __restrict__ state, int append,
                                                                 float* __restrict__ stats)
{
    __shared__ __attribute__((aligned(16))) float sh[HISTORY_MAX];                       // first the partials (doubles), then the ring's copy
    const int tid = threadIdx.x;
    bool has_norm = false;
    float norm = 0.0f;                                       // (thread 0's)
    if (nparts > 0) {
        double* shd = (double*)sh;
        if (tid < nparts) shd[tid] = partials[tid];
        __syncthreads();
        if (tid == 0) {
            double t = shd[0];
#pragma unroll 8
            for (int i = 1; i < nparts; ++i) t += shd[i];
            norm = (float)sqrt(t);
        }
        has_norm = true;
        __syncthreads();                                     // sh is about to be reused
    } else if (norm_in) {
        norm = *norm_in;
        has_norm = true;
    }
    int count = state[0], head = state[1];
    count = min(max(count, 0), capacity);
    head = min(max(head, 0), capacity - 1);
    float clip = 0.0f;
    const bool want_clip = q >= 0.0;
    if (want_clip) {
        int npad = 2;
        while (npad < count) npad <<= 1;                     // <= HISTORY_MAX: capacity is
        int nan = 0;
        for (int i = tid; i < npad; i += 1024) {             // (the order in the ring does not matter to a sort)
            const float v = i < count ? ring[(head + i) % capacity] : __builtin_huge_valf();
            nan |= v != v;
            sh[i] = v;
        }
        nan = __syncthreads_or(nan);
        for (int k = 2; k <= npad; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < npad; i += 1024) {
                    const int x = i ^ j;
                    if (x > i) {
                        const float a = sh[i], b = sh[x];
                        if ((a > b) == ((i & k) == 0)) { sh[i] = b; sh[x] = a; }
                    }
                }
                __syncthreads();
            }
        }
        if (tid == 0) {
            if (nan || count < 1) {
                clip = __builtin_nanf("");
            } else {
                const double pos = q * (double)(count - 1);
                const int lo = min(max((int)floor(pos), 0), count - 1), hi = min(lo + 1, count - 1);
                clip = (float)quantile_lerp((double)sh[lo], (double)sh[hi], pos - (double)lo);
            }
        }
    } else {
        __syncthreads();                                     // every read of state is done before thread 0 writes it
    }
    if (tid != 0) return;
    if (has_norm) stats[0] = norm;
    if (want_clip) stats[1] = clip;
    if (has_norm && want_clip) stats[2] = clip_coef(clip, norm);
    if (append && has_norm) {
        if (count < capacity) {
            ring[(head + count) % capacity] = norm;
            state[0] = count + 1;
        } else {
            ring[head] = norm;
            state[1] = (head + 1) % capacity;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void adabelief_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ s, long long numel, const float* __restrict__ coef_ptr,
                                                             const semicrf_adabelief_groups G)
{
    const float coef = coef_ptr ? *coef_ptr : 1.0f;
    const long long nwork = VEC ? (numel + 3) / 4 : numel;
    for (long long w = (long long)blockIdx.x * 256 + threadIdx.x; w < nwork; w += (long long)gridDim.x * 256) {
        const long long e0 = VEC ? 4 * w : w;
        const int n = VEC ? (int)min(4ll, numel - e0) : 1;
        float pv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gv[4] = {0.0f, 0.0f, 0.0f, 0.0f}, mv[4] = {0.0f, 0.0f, 0.0f, 0.0f},
              sv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC && n == 4) {
            const float4 a = *(const float4*)(p + e0), b = *(const float4*)(g + e0), c = *(const float4*)(m + e0),
                         d = *(const float4*)(s + e0);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
            gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
            mv[0] = c.x; mv[1] = c.y; mv[2] = c.z; mv[3] = c.w;
            sv[0] = d.x; sv[1] = d.y; sv[2] = d.z; sv[3] = d.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) { pv[j] = p[e0 + j]; gv[j] = g[e0 + j]; mv[j] = m[e0 + j]; sv[j] = s[e0 + j]; }
        }
#pragma unroll
        for (int gi = 0; gi < SEMICRF_OPTIM_MAX_GROUPS; ++gi) {
            if (gi >= G.n) continue;
            const long long lo = gi ? G.g[gi ? gi - 1 : 0].end : 0, hi = G.g[gi].end;
            if (e0 >= hi || e0 + n <= lo) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n && e0 + j >= lo && e0 + j < hi) adabelief_update(pv[j], gv[j], mv[j], sv[j], coef, G.g[gi]);
        }
        if (VEC && n == 4) {
            *(float4*)(p + e0) = make_float4(pv[0], pv[1], pv[2], pv[3]);
            *(float4*)(m + e0) = make_float4(mv[0], mv[1], mv[2], mv[3]);
            *(float4*)(s + e0) = make_float4(sv[0], sv[1], sv[2], sv[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < n) { p[e0 + j] = pv[j]; m[e0 + j] = mv[j]; s[e0 + j] = sv[j]; }
        }
    }
}

void launch_grad_sqnorm(const float* flat, long long numel, double* partials, hipStream_t stream)
{
    const int head = (int)std::min<long long>(numel, (long long)(((16 - ((uintptr_t)flat & 15)) & 15) / 4));
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(sqnorm_partials(numel)), dim3(SQNORM_BLOCK), 0, stream, flat, numel, head, partials);
}

void launch_clip_from_history(const double* partials, long long numel, const float* norm_in, double q, float* ring, int capacity,
                              int* state, int append, float* stats, hipStream_t stream)
{
    hipLaunchKernelGGL(clip_from_history_kernel, dim3(1), dim3(1024), 0, stream, partials, partials ? sqnorm_partials(numel) : 0, norm_in,
                       q, ring, capacity, state, append, stats);
}

void launch_adabelief_step(float* p, const float* g, float* m, float* s, long long numel, const float* coef,
                           const semicrf_adabelief_groups& groups, hipStream_t stream)
{
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)s) & 15) == 0;
    const long long nwork = vec ? (numel + 3) / 4 : numel;
    const int grid = (int)std::min<long long>((nwork + 255) / 256, 2048);
    if (vec)
        hipLaunchKernelGGL(adabelief_step_kernel<true>, dim3(grid), dim3(256), 0, stream, p, g, m, s, numel, coef, groups);
    else
        hipLaunchKernelGGL(adabelief_step_kernel<false>, dim3(grid), dim3(256), 0, stream, p, g, m, s, numel, coef, groups);
}

}  // namespace semicrf
