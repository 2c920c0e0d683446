// attr_loss.hip -- the attribute-head part of the training loss (replaces TransKun.log_prob, ModelTransformer.py:284-328: the
// velocity log-softmax + gather, the ContinuousBernoulli log-density of the refined onset/offset, the Bernoulli log-density of
// their presence, and the scatter_add of the three per-interval terms into the per-chain logProb).
//
// Rows are the K target intervals in chain order (offsets [C+1], the packed layout of the whole library).  Forward:
//   rows kernel   one wave per row: the 128 velocity logits as a float2 per lane, max and sum by xor-shuffles (every lane ends
//                 with the same bits), lane 0 evaluates the four onset/offset logits (attr_loss_math.h) and stores
//                 rowLogProb[i] = (lpVel + lpOF) + lpPres
//   chains kernel one thread per chain: out[c] = (sum of its rows, ascending, fp32) + base[c]
// No atomics: a chain's result depends on its own rows only, in a fixed order.  Backward: one wave per row, the row's chain by
// binary search in offsets, logsumexp recomputed (128 exps per row are cheaper than a saved array is to carry around):
//   dLogitsVelocity = g (onehot(v) - softmax),  dOfLogits = g (x - sigmoid + logC') | g (p - sigmoid)
#include "common.h"
#include "launchers.h"
#include "chain_search.h"
#include "attr_loss_math.h"

namespace semicrf {

using namespace attr_loss;

// max and log(sum exp(x - max)) of the row's 128 logits, identical in all 64 lanes
__device__ __forceinline__ void row_logsumexp(float2 x, float& m, float& logs)
{
    m = fmaxf(x.x, x.y);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float s = expf(x.x - m) + expf(x.y - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    logs = logf(s);
}

__global__ __launch_bounds__(256) void attr_loss_rows_kernel(const float* __restrict__ logitsVelocity, const float* __restrict__ ofLogits,
                                                             const int* __restrict__ velocity, const float* __restrict__ ofRefined,
                                                             const float* __restrict__ ofPresence, int K, float* __restrict__ rowLogProb)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= K) return;                                                      // (whole waves leave)
    const float2 x = *(const float2*)(logitsVelocity + (size_t)i * NVEL + 2 * lane);
    float m, logs;
    row_logsumexp(x, m, logs);
    const int v = velocity[i];
    const float xv = __shfl((v & 1) ? x.y : x.x, (v >> 1) & 63);             // logitsVelocity[i][v] without indexing memory by v
    if (lane != 0) return;
    const float lpVel = (unsigned)v < (unsigned)NVEL ? (xv - m) - logs : __builtin_nanf("");
    const float of[4] = {ofLogits[4 * (size_t)i], ofLogits[4 * (size_t)i + 1], ofLogits[4 * (size_t)i + 2], ofLogits[4 * (size_t)i + 3]};
    const float r[2] = {ofRefined[2 * (size_t)i], ofRefined[2 * (size_t)i + 1]};
    const float p[2] = {ofPresence[2 * (size_t)i], ofPresence[2 * (size_t)i + 1]};
    float lpOF, lpPres;
    of_terms<float>(of, r, p, lpOF, lpPres);
    rowLogProb[i] = (lpVel + lpOF) + lpPres;
}

__global__ __launch_bounds__(256) void attr_loss_chains_kernel(const float* __restrict__ rowLogProb, int K, const int* __restrict__ offsets,
                                                               int C, const float* __restrict__ base, float* __restrict__ out)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int b = max(offsets[c], 0), e = min(offsets[c + 1], K);            // (offsets the caller got wrong read no row outside [0, K))
    if (e <= b) { out[c] = base ? base[c] : 0.0f; return; }
    float acc = rowLogProb[b];
    for (int i = b + 1; i < e; ++i) acc += rowLogProb[i];
    out[c] = base ? acc + base[c] : acc;
}

__global__ __launch_bounds__(256) void attr_loss_bwd_kernel(const float* __restrict__ gout, int gstride, const float* __restrict__ logitsVelocity,
                                                            const float* __restrict__ ofLogits, const int* __restrict__ velocity,
                                                            const float* __restrict__ ofRefined, const float* __restrict__ ofPresence, int K,
                                                            const int* __restrict__ offsets, int C, float* __restrict__ dLogitsVelocity,
                                                            float* __restrict__ dOfLogits)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= K) return;
    const float g = gout[(size_t)chain_of_interval(offsets, C, i) * gstride];
    const float2 x = *(const float2*)(logitsVelocity + (size_t)i * NVEL + 2 * lane);
    float m, logs;
    row_logsumexp(x, m, logs);
    const int v = velocity[i];
    float2 d;
    d.x = g * ((2 * lane == v ? 1.0f : 0.0f) - expf((x.x - m) - logs));
    d.y = g * ((2 * lane + 1 == v ? 1.0f : 0.0f) - expf((x.y - m) - logs));
    *(float2*)(dLogitsVelocity + (size_t)i * NVEL + 2 * lane) = d;
    if (lane != 0) return;
    const float of[4] = {ofLogits[4 * (size_t)i], ofLogits[4 * (size_t)i + 1], ofLogits[4 * (size_t)i + 2], ofLogits[4 * (size_t)i + 3]};
    const float r[2] = {ofRefined[2 * (size_t)i], ofRefined[2 * (size_t)i + 1]};
    const float p[2] = {ofPresence[2 * (size_t)i], ofPresence[2 * (size_t)i + 1]};
    float dd[4];
    of_grads<float>(of, r, p, dd);
#pragma unroll
    for (int j = 0; j < 4; ++j) dOfLogits[4 * (size_t)i + j] = g * dd[j];
}

void launch_attr_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int* velocity, const float* ofRefined,
                          const float* ofPresence, int K, const int* offsets, int C, const float* base, float* rowLogProb, float* out,
                          hipStream_t stream)
{
    if (K <= 0) return;
    hipLaunchKernelGGL(attr_loss_rows_kernel, dim3((K + 3) / 4), dim3(256), 0, stream, logitsVelocity, ofLogits, velocity, ofRefined,
                       ofPresence, K, rowLogProb);
    hipLaunchKernelGGL(attr_loss_chains_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, rowLogProb, K, offsets, C, base, out);
}

void launch_attr_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int* velocity,
                          const float* ofRefined, const float* ofPresence, int K, const int* offsets, int C, float* dLogitsVelocity,
                          float* dOfLogits, hipStream_t stream)
{
    if (K <= 0) return;
    hipLaunchKernelGGL(attr_loss_bwd_kernel, dim3((K + 3) / 4), dim3(256), 0, stream, gout, gstride, logitsVelocity, ofLogits, velocity,
                       ofRefined, ofPresence, K, offsets, C, dLogitsVelocity, dOfLogits);
}

}  // namespace semicrf
