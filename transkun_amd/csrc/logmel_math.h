// logmel_math.h -- what the HIP kernel of the audio front end (logmel.hip) and its host mirror (cpu_ops.cpp) share: the supported set
// and the order of operations of every output element.  Everything below is +, -, *, /, fmaf and integer work in IEEE arithmetic (the
// logarithm included: lm_log), so the two sides compute the same bits.
//
// Per (recording n, channel c, frame t, window w), W = 2^LOGW samples, M = W / 2, P = LOGW - 1:
//   x[j]    = frames[n, c, t, j]; with a gain, (x[j] - shift[n]) / denom[n]                 one subtraction, one true division
//   y[j]    = x[j] * windows[w, j]                                                          always, also where the window is 0
//   z[i]    = (y[2 i], y[2 i + 1])  i < M                                                   the half-length complex signal
//   Z       = the length-M transform of z, radix 2, decimation in frequency, in place: P stages with half span h = M / 2, M / 4, .. 1;
//             a stage takes every pair (i, i + h) with (i & h) == 0 through lm_butterfly with the twiddle tw[(i & (h - 1)) * (M / h)];
//             Z[k] ends at position lm_brev(k, P).  tw[k] = exp(-2 pi i k / W), k < M, comes from the caller (float64 rounded to fp32)
//   X[k]    = lm_split(Z[k], Z[M - k], tw[k])   0 < k < M;   X[0] = Zr[0] + Zi[0], X[M] = Zr[0] - Zi[0] (both real)
//   p[k]    = lm_power(X[k], 1 / W)             (re re + im im) (1 / W): the ortho norm, exact
//   mono:     p[k] = ((p_0[k] + p_1[k]) + ..) / C over the channels, ascending, then one division
//   mel[m]  = fmaf-chain over r = fb_start[m] .. fb_start[m] + fb_len[m] - 1 ascending from +0 of p[r] * fb_val[fb_off[m] + r - fb_start[m]]
//   out     = log_flag ? (lm_log(mel + eps) - le) / (-le) : mel                            le = (float)log((double)eps), from the host
// The butterflies of a stage are independent, so the order in which a stage's pairs are visited (the device takes three stages at a
// time in registers) changes nothing.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LM_HD __host__ __device__ __forceinline__
#else
#define LM_HD inline
#endif

namespace semicrf {
namespace logmel {

constexpr int LM_MIN_LOGW = 8;         // W = 256
constexpr int LM_MAX_LOGW = 12;        // W = 4096: SEMICRF_LOGMEL_MAX_W
constexpr int LM_MAX_WIN = 8;          // SEMICRF_LOGMEL_MAX_WINDOWS
constexpr int LM_MAX_C = 16;           // SEMICRF_LOGMEL_MAX_CHANNELS
constexpr int LM_MAX_MEL = 512;        // SEMICRF_LOGMEL_MAX_BANDS: nMel * nWin floats of a frame's features are staged in LDS
constexpr int LM_MAX_TOTAL = 65536;    // SEMICRF_LOGMEL_MAX_SUPPORT: the products of one (frame, channel, window)

struct alignas(8) cf { float re, im; };

LM_HD int log2_of_window(int W)        // LOGW, or -1 outside the supported set
{
    for (int l = LM_MIN_LOGW; l <= LM_MAX_LOGW; ++l)
        if (W == (1 << l)) return l;
    return -1;
}

// max_len: the longest column support; total: the sum of all supports
LM_HD bool supported(int W, int nWin, int C, int nMel, int max_len, int total)
{
    return log2_of_window(W) >= 0 && nWin >= 1 && nWin <= LM_MAX_WIN && C >= 1 && C <= LM_MAX_C && nMel >= 1 && nMel <= LM_MAX_MEL &&
           max_len >= 0 && max_len <= W / 2 + 1 && total >= 0 && total <= LM_MAX_TOTAL;
}

LM_HD float lm_sample(float x, bool gain, float shift, float denom, float win)
{
    if (gain) x = (x - shift) / denom;
    return x * win;
}

// (a, b) <- (a + b, (a - b) w)
LM_HD void lm_butterfly(cf& a, cf& b, cf w)
{
    const float dr = a.re - b.re, di = a.im - b.im;
    a.re = a.re + b.re;
    a.im = a.im + b.im;
    b.re = fmaf(dr, w.re, -(di * w.im));
    b.im = fmaf(dr, w.im, di * w.re);
}

// the low `bits` bits of k in reverse order
LM_HD int lm_brev(int k, int bits)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (int)(__brev((unsigned)k) >> (32 - bits));
#else
    uint32_t v = (uint32_t)k;
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return (int)(v >> (32 - bits));
#endif
}

// bin k of the real transform from bins k and M - k of the half-length one: E + w O with E = (Zk + conj(Zm)) / 2 the transform of the
// even samples and O = -i (Zk - conj(Zm)) / 2 that of the odd ones
LM_HD cf lm_split(cf zk, cf zm, cf w)
{
    const float er = 0.5f * (zk.re + zm.re), ei = 0.5f * (zk.im - zm.im);
    const float pr = 0.5f * (zk.im + zm.im), pi = -0.5f * (zk.re - zm.re);
    cf x;
    x.re = er + fmaf(pr, w.re, -(pi * w.im));
    x.im = ei + fmaf(pr, w.im, pi * w.re);
    return x;
}

LM_HD float lm_power(cf x, float inv_w) { return fmaf(x.re, x.re, x.im * x.im) * inv_w; }

// the natural logarithm of an fp32 value, rounded to fp32 from a float64 evaluation (error below 1e-13 before the rounding):
// x = m 2^e with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s) with s = (m - 1) / (m + 1), |s| < 0.1716, as its series to s^19.
// Plain IEEE float64 operations only: the same bits on the host and on the device.
LM_HD float lm_log(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return x;                        // NaN
    if ((u & 0x7fffffffu) == 0) return -__builtin_huge_valf();            // +-0
    if (u >> 31) return __builtin_nanf("");                               // negative
    if (u == 0x7f800000u) return x;                                       // +inf
    double d = (double)x;                                                 // exact; every fp32 value is a normal float64
    uint64_t q;
    memcpy(&q, &d, 8);
    int e = (int)(q >> 52) - 1023;
    q = (q & 0x000fffffffffffffull) | 0x3ff0000000000000ull;              // m in [1, 2)
    double m;
    memcpy(&m, &q, 8);
    if (m > 1.4142135623730951) { m *= 0.5; e += 1; }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double p = 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    return (float)((double)e * 0.6931471805599453 + 2.0 * s * p);
}

LM_HD float lm_compress(float mel, float eps, float le) { return (lm_log(mel + eps) - le) / (-le); }

// a band's support clamped into the spectrum [0, M] and into the value array: what both sides walk
LM_HD void lm_band(int start, int len, int off, int M, int total, int& s, int& n)
{
    s = start;
    n = len;
    if (s < 0 || off < 0 || n < 0) n = 0;
    if (n > M + 1 - s) n = M + 1 - s > 0 ? M + 1 - s : 0;
    if (n > total - off) n = total - off > 0 ? total - off : 0;
}

}  // namespace logmel
}  // namespace semicrf
