// attr_heads_math.h -- what the HIP kernel of the attribute heads (attr_heads.hip) and its host mirror (cpu_ops.cpp) share: the
// tile constants that fix the order of operations of every output element, and the activation.
//
// Per interval i, x_i = [a | b | a * b] (3 D values, a = ctx[c, begin], b = ctx[c, end]; the product is rounded to fp32 once):
//   h[j]       = fmaf-chain over k = 0 .. 3D-1 ascending from +0 of x[k] * W1[k][j], then + b1[j]          (one fp32 addition)
//   g[j]       = gelu(h[j])                                                                                (below)
//   part[s][n] = fmaf-chain over the hidden columns j of slice s ascending from +0 of g[j] * W2[j][n]
//   out[n]     = ((part[0][n] + part[1][n]) + ...) + b2[n]                                                 (slices ascending, bias last)
// A head's hidden columns are cut into slices of HEADS_SLICE; a slice never holds columns of both heads.  Both chains are padded
// with exact zeros (0 * 0 added: no change to a finite value), so a result depends on its own row and the weights alone.
//
// gelu is the exact erf form, nn.GELU()'s default: 0.5 h (1 + erf(h / sqrt 2)).  For h < 0 that sum cancels (1 + erf -> 0) and
// loses the tail's relative accuracy; there 1 + erf(z) = erfc(-z) is used, which does not.
//
// Training (attribute_heads_train, attr_heads_bwd.hip): z[j] = h[j] (after + b1) is saved; A[j] = keep(seed, i, j) ? gelu(z[j]) * scale
// : 0 takes g's place in layer 2 (scale = (float)(1 / (1 - p)) of the head; a head with p = 0 is not masked and not scaled).  The
// mask, gelu' and the backward's order of operations: below and include/semicrf_hip.h.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ATTR_HEADS_HD __host__ __device__ __forceinline__
#else
#define ATTR_HEADS_HD inline
#endif

namespace semicrf {
namespace attr_heads {

constexpr int HEADS_ROWS = 64;       // rows (intervals) per workgroup: SEMICRF_HEADS_ROW_TILE
constexpr int HEADS_SLICE = 64;      // hidden columns per workgroup
constexpr int HEADS_KCHUNK = 32;     // contraction values of layer 1 staged per step
constexpr int HEADS_BWD_ROWS = 512;  // rows per partial plane of the backward's sums over rows: SEMICRF_HEADS_BWD_ROW_CHUNK
constexpr int HEADS_BWD_SUBSUMS = 8; // a bias gradient's chunk sum: 8 sums over the rows r = q (mod 8), added in ascending q (double)

ATTR_HEADS_HD int slices_of(int H) { return (H + HEADS_SLICE - 1) / HEADS_SLICE; }

ATTR_HEADS_HD float erf_(float x) { return erff(x); }
ATTR_HEADS_HD double erf_(double x) { return erf(x); }
ATTR_HEADS_HD float erfc_(float x) { return erfcf(x); }
ATTR_HEADS_HD double erfc_(double x) { return erfc(x); }

template <class T>
ATTR_HEADS_HD T gelu(T h)
{
    const T z = h * (T)0.70710678118654752440;
    const T t = h < (T)0 ? erfc_(-z) : (T)1 + erf_(z);       // NaN takes the second branch and stays NaN
    return ((T)0.5 * h) * t;
}

ATTR_HEADS_HD float fma_(float a, float b, float c) { return fmaf(a, b, c); }
ATTR_HEADS_HD double fma_(double a, double b, double c) { return fma(a, b, c); }
ATTR_HEADS_HD float exp_(float x) { return expf(x); }
ATTR_HEADS_HD double exp_(double x) { return exp(x); }

// gelu'(h) = Phi(h) + h phi(h), the exact erf form; Phi by erfc below 0, as in gelu
template <class T>
ATTR_HEADS_HD T gelu_grad(T h)
{
    const T z = h * (T)0.70710678118654752440;
    const T cdf = (T)0.5 * (h < (T)0 ? erfc_(-z) : (T)1 + erf_(z));
    const T pdf = (T)0.39894228040143267794 * exp_((T)-0.5 * h * h);
    return fma_(h, pdf, cdf);
}

// ---- the dropout mask: Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) ------------------------
// counter = (i >> 2, j, 0, 0), key = (seed & 0xffffffff, seed >> 32); element (i, j) takes output word i & 3 and is KEPT iff that
// word >= floor(p * 2^32).  i: the global row, j: the packed hidden column 0 .. Hv + Ho - 1.
struct DropoutParams {
    unsigned long long seed;
    unsigned thr[2];                 // floor(p * 2^32) per head (velocity, onset/offset)
    float scale[2];                  // (float)(1 / (1 - p))
    int on[2];                       // p > 0: the head is masked and scaled
};

ATTR_HEADS_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four draws of rows 4 q .. 4 q + 3 (q = i >> 2) at column j
ATTR_HEADS_HD void dropout_draws(unsigned long long seed, uint32_t q, uint32_t j, uint32_t out[4])
{
    philox4x32_10(q, j, 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

inline DropoutParams dropout_params(unsigned long long seed, double pv, double po)
{
    DropoutParams d;
    d.seed = seed;
    const double p[2] = {pv, po};
    for (int h = 0; h < 2; ++h) {
        d.on[h] = p[h] > 0.0;
        d.thr[h] = d.on[h] ? (unsigned)floor(p[h] * 4294967296.0) : 0u;
        d.scale[h] = d.on[h] ? (float)(1.0 / (1.0 - p[h])) : 1.0f;
    }
    return d;
}

}  // namespace attr_heads
}  // namespace semicrf
