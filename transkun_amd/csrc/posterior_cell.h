// posterior_cell.h -- what posterior.hip and marginal_decode.hip share: the tiling of the lower triangle, the chain-quad load,
// and the marginal of ONE cell.  semicrf_interval_marginals and semicrf_marginal_decode evaluate cell_marginal /
// cell_marginal_single and nothing else, so the value a threshold is compared with is the value semicrf_interval_marginals
// returns, bit for bit.
#pragma once
#include "common.h"

namespace semicrf {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));     // odd NBatch: 16-byte accesses at 4-byte aligned addresses

// chains c0 .. c0+3 of row `p` (n = how many of them exist; the rest read as `fill`)
__device__ __forceinline__ f4 ld4(const float* __restrict__ p, int n, float fill)
{
    if (n >= 4) return (f4)(*(const f4u*)p);
    f4 r = {fill, fill, fill, fill};
    if (n > 0) r.x = p[0];
    if (n > 1) r.y = p[1];
    if (n > 2) r.z = p[2];
    return r;
}

__device__ __forceinline__ void tile_of(int k, int& i, int& j)      // k-th tile of the lower triangle, row-major: (i, j), j <= i
{
    int r = (int)((sqrtf(8.0f * (float)k + 1.0f) - 1.0f) * 0.5f);
    while ((r + 1) * (r + 2) / 2 <= k) ++r;
    while (r * (r + 1) / 2 > k) --r;
    i = r;
    j = k - r * (r + 1) / 2;
}

__device__ __forceinline__ float clamp1(float x) { return x > 1.0f ? 1.0f : x; }     // rounding above 1; NaN stays NaN

// the singleton's marginal exp(v + q - logZ + d - 2 sp(d)) (semicrf_logz_bwd's diagonal dScore)
__device__ __forceinline__ float single_marg(float v, float q, float lz, float d)
{
    return __expf(v + q - lz + d - 2.0f * softplus_f(d));
}

// m(e, b), b < e: vb = v[b], s = s[e,b], A = q[e] - logZ
__device__ __forceinline__ float cell_marginal(float vb, float s, float A) { return clamp1(__expf((vb + s) + A)); }
// m(t, t): vt = v[t], qt = q[t], d = s[t,t]
__device__ __forceinline__ float cell_marginal_single(float vt, float qt, float lz, float d) { return clamp1(single_marg(vt, qt, lz, d)); }

}  // namespace semicrf
