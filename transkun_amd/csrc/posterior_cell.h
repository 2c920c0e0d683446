// posterior_cell.h -- what posterior.hip, marginal_decode.hip and marginal_tol.hip share: the tiling of the lower triangle, the
// chain-quad loads, and the marginal of ONE cell.  semicrf_interval_marginals and semicrf_marginal_decode evaluate cell_marginal /
// cell_marginal_single and nothing else, so the value a threshold is compared with is the value semicrf_interval_marginals
// returns, bit for bit.  tol_marginal is the tolerance-aware marginal M of include/semicrf_hip.h (semicrf_interval_marginals_tol),
// evaluated literally: the gather kernel and the write pass of semicrf_marginal_decode_tol both call it.
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

// ---- chain quads of int32 words and of thresholds (marginal_decode.hip, marginal_tol.hip) ----
typedef int i4 __attribute__((ext_vector_type(4)));
typedef int i4u __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned long long u64;

__device__ __forceinline__ i4 ldi4(const int* __restrict__ p, int n)
{
    if (n >= 4) return (i4)(*(const i4u*)p);
    i4 r = {0, 0, 0, 0};
    if (n > 0) r.x = p[0];
    if (n > 1) r.y = p[1];
    if (n > 2) r.z = p[2];
    return r;
}
__device__ __forceinline__ void sti4(int* __restrict__ p, int n, i4 x)
{
    if (n >= 4) { *(i4u*)p = (i4u)x; return; }
    if (n > 0) p[0] = x.x;
    if (n > 1) p[1] = x.y;
    if (n > 2) p[2] = x.z;
}
// the thresholds of chains c0 .. c0+3; a chain that does not exist gets +inf (m <= 1 never reaches it)
__device__ __forceinline__ f4 ld_tau(const float* __restrict__ tau, int tau_stride, int c0, int n)
{
    const float inf = __builtin_huge_valf();
    f4 r = {inf, inf, inf, inf};
    if (n > 0) r.x = tau[(size_t)c0 * tau_stride];
    if (n > 1) r.y = tau[(size_t)(c0 + 1) * tau_stride];
    if (n > 2) r.z = tau[(size_t)(c0 + 2) * tau_stride];
    if (n > 3) r.w = tau[(size_t)(c0 + 3) * tau_stride];
    return r;
}

// ---- the tolerance-aware marginal, evaluated literally (the definition of include/semicrf_hip.h) ----
// One template for a lone chain (V = float) and a chain quad (V = f4): per chain the same operations in the same order.
template <typename V> struct ChainVec;
template <> struct ChainVec<float> {
    static __device__ __forceinline__ float ld(const float* __restrict__ p, int, float) { return p[0]; }
    static __device__ __forceinline__ float cell(float vb, float s, float A) { return cell_marginal(vb, s, A); }
    static __device__ __forceinline__ float single(float vt, float qt, float lz, float d) { return cell_marginal_single(vt, qt, lz, d); }
    static __device__ __forceinline__ float clamp(float x) { return clamp1(x); }
};
template <> struct ChainVec<f4> {
    static __device__ __forceinline__ f4 ld(const float* __restrict__ p, int n, float fill) { return ld4(p, n, fill); }
    static __device__ __forceinline__ f4 cell(f4 vb, f4 s, f4 A)
    {
        f4 r;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) r[ch] = cell_marginal(vb[ch], s[ch], A[ch]);
        return r;
    }
    static __device__ __forceinline__ f4 single(f4 vt, f4 qt, f4 lz, f4 d)
    {
        f4 r;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) r[ch] = cell_marginal_single(vt[ch], qt[ch], lz[ch], d[ch]);
        return r;
    }
    static __device__ __forceinline__ f4 clamp(f4 x)
    {
        f4 r;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) r[ch] = clamp1(x[ch]);
        return r;
    }
};

// M(e, b) of the chains at c0 (n of them exist), 0 <= b <= e < T: rows e' ascending, inside a row b' ascending, one fp32 add per
// term; only cells of the triangle (0 <= b' <= e' < T) are loaded.  lz = logZ of those chains.
template <typename V>
__device__ __forceinline__ V tol_marginal(const float* __restrict__ score, const float* __restrict__ v, const float* __restrict__ q, V lz,
                                          int T, size_t Bs, int c0, int n, int b, int e, int db, int de)
{
    typedef ChainVec<V> X;
    const int elo = e - de > 0 ? e - de : 0, ehi = e + de < T - 1 ? e + de : T - 1;
    const int blo = b - db > 0 ? b - db : 0;
    V acc = (V)(0.0f);
    for (int er = elo; er <= ehi; ++er) {
        const int bhi = b + db < er ? b + db : er;
        if (bhi < blo) continue;                                 // a row without a cell
        const V qe = X::ld(q + (size_t)er * Bs + c0, n, SEMICRF_NEG_INF);
        const V A = qe - lz;
        const float* __restrict__ srow = score + (size_t)er * T * Bs + c0;
        V row = (V)(0.0f);
        for (int bc = blo; bc <= bhi; ++bc) {
            const V vb = X::ld(v + (size_t)bc * Bs + c0, n, SEMICRF_NEG_INF);
            const V s = X::ld(srow + (size_t)bc * Bs, n, SEMICRF_NEG_INF);
            row += bc == er ? X::single(vb, qe, lz, s) : X::cell(vb, s, A);
        }
        acc += row;
    }
    return X::clamp(acc);
}

}  // namespace semicrf
