// pathscore.h -- the unnormalised path score of ONE chain by ONE wave (NeuralSemiCRFInterval.py:508-550), shared by the stand-alone
// evalPath kernel (evalpath.hip) and the path role of the forward sweep (persist.hip: semicrf_logprob_fwd as one launch), so that
// logProb == evalPath - logZ bit for bit whichever way it is computed.
//   out[c] = sum_{(b,e) in path_c} ( s[e,b,c] - sum_{t=b}^{e-1} noise[t,c] ) + sum_t noise[t,c]
// The lanes stride over the chain's noise column and over its intervals; sums in double (torch's CPU cumsum does the same), combined
// by a butterfly over the 64 lanes: a fixed order, the result is bit-reproducible run to run and the same in every lane.
#pragma once
#include "common.h"

namespace semicrf {

__device__ __forceinline__ double path_score_wave(const float* __restrict__ score, const float* __restrict__ noise, int T, int B, int K,
                                                  const int* __restrict__ pairs, const int* __restrict__ offsets, int c)
{
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int t = lane; t < T - 1; t += 64) acc += (double)noise[(size_t)t * B + c];          // cum[T-1]
    const int k0 = offsets[c], k1 = offsets[c + 1];
    for (int k = k0 + lane; k < k1 && k < K; k += 64) {
        const int b = pairs[2 * k], e = pairs[2 * k + 1];
        double covered = 0.0;
        for (int t = b; t < e; ++t) covered += (double)noise[(size_t)t * B + c];
        acc += (double)score[((size_t)e * T + b) * B + c] - covered;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    return acc;
}

// The path table of logProb's backward (persist.hip: the gradient sweep applies the path's own +-gout while it stores the
// marginals).  tab[f * B + c], one word per (frame, chain):
//   bits 0..29: the END frame of the path interval that BEGINS at frame f, PTAB_NONE if none does (a row of the gradient sweep is
//               a begin frame, its columns are end frames: the writer of a row's cells looks up ONE word per chain);
//   bit 30:     the gap between frames f and f + 1 is covered by an interval (begin <= f < end).
// Representable paths (the host checks it when it packs, nothing here does): within a chain the begins ascend strictly and no
// interval starts before the previous one has ended -- every frame begins at most one interval, every gap is covered at most once.
// Interval k owns the frames [begin_k, begin_k+1), the first interval also those before it: every word of the chain's column
// is written exactly once on every call, by plain stores (no fill, no atomics).  Indices are clamped into [0, T).
constexpr int PTAB_COVERED = 1 << 30;
constexpr int PTAB_NONE = PTAB_COVERED - 1;

__device__ __forceinline__ void path_table_wave(int* __restrict__ tab, int T, int B, int K, const int* __restrict__ pairs,
                                                const int* __restrict__ offsets, int c)
{
    const int lane = threadIdx.x & 63;
    const int k0 = offsets[c];
    int k1 = offsets[c + 1];
    if (k1 > K) k1 = K;
    int first = k0 < k1 ? pairs[2 * k0] : T;                                          // frames in front of the first interval
    first = first < 0 ? 0 : (first > T ? T : first);
    for (int t = lane; t < first; t += 64) tab[(size_t)t * B + c] = PTAB_NONE;
    for (int k = k0 + lane; k < k1; k += 64) {
        const int b = pairs[2 * k], e = pairs[2 * k + 1];
        int hi = k + 1 < k1 ? pairs[2 * k + 2] : T;
        hi = hi > T ? T : hi;
        for (int t = b < 0 ? 0 : b; t < hi; ++t)
            tab[(size_t)t * B + c] = (t == b ? (e & PTAB_NONE) : PTAB_NONE) | (t < e ? PTAB_COVERED : 0);
    }
}

}  // namespace semicrf
