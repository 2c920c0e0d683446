// ffn_bf16_dev.h -- the device helpers that the kernels of the bf16 feed-forward ResBlock share (ffn_bf16.hip, ffn_bf16_bwd.hip):
// loads and stores of 4 and 8 consecutive elements with or without wide accesses (the same bits either way), and the dropout draws
// of a quad of tokens.
#pragma once
#include "common.h"
#include "bf16x3.h"
#include "ffn_bf16_train_math.h"

namespace semicrf {

using namespace ffn;

static_assert(FFN16_ROWS == 64 && FFN16_CHUNK == 64, "the lane maps below are written for 64 x 64");
constexpr int FFN16_LDG = FFN16_CHUNK + FFN16_PAD;          // bf16 per row of Gs and of the W2 tile

struct Ffn16F8 { float v[8]; };

// 8 consecutive elements as fp32 (exact): 16-byte loads, or element loads put together -- the same bits
template <typename T>
__device__ __forceinline__ Ffn16F8 ffn16_load8f(const T* p, bool vec);
template <>
__device__ __forceinline__ Ffn16F8 ffn16_load8f<uint16_t>(const uint16_t* p, bool vec)
{
    u32x4 x;
    if (vec) {
        x = *(const u32x4*)p;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (unsigned)p[2 * e] | ((unsigned)p[2 * e + 1] << 16);
    }
    Ffn16F8 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        r.v[2 * e] = __uint_as_float(x[e] << 16);
        r.v[2 * e + 1] = __uint_as_float(x[e] & 0xffff0000u);
    }
    return r;
}
template <>
__device__ __forceinline__ Ffn16F8 ffn16_load8f<float>(const float* p, bool vec)
{
    Ffn16F8 r;
    if (vec) {
        const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
        r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
        r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) r.v[e] = p[e];
    }
    return r;
}

// 8 consecutive weights as the bf16 operand of a product: as they are (form A), rounded to nearest even (form B)
template <typename T>
__device__ __forceinline__ u32x4 ffn16_load8h(const T* p, bool vec);
template <>
__device__ __forceinline__ u32x4 ffn16_load8h<uint16_t>(const uint16_t* p, bool vec)
{
    u32x4 x;
    if (vec) {
        x = *(const u32x4*)p;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = (unsigned)p[2 * e] | ((unsigned)p[2 * e + 1] << 16);
    }
    return x;
}
template <>
__device__ __forceinline__ u32x4 ffn16_load8h<float>(const float* p, bool vec)
{
    const Ffn16F8 f = ffn16_load8f<float>(p, vec);
    u32x4 x;
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = cvt_pk_bf16(f.v[2 * e], f.v[2 * e + 1]);
    return x;
}

// four consecutive elements as fp32, and four results rounded once to T
__device__ __forceinline__ void ffn16_load4f(const uint16_t* p, bool vec, float* v)
{
    if (vec) {
        const uint2 u = *(const uint2*)p;
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __uint_as_float((unsigned)p[e] << 16);
    }
}
__device__ __forceinline__ void ffn16_load4f(const float* p, bool vec, float* v)
{
    if (vec) {
        const float4 a = *(const float4*)p;
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p[e];
    }
}
__device__ __forceinline__ void ffn16_store4(uint16_t* p, bool vec, const float* v)
{
    const unsigned a = cvt_pk_bf16(v[0], v[1]), b = cvt_pk_bf16(v[2], v[3]);
    if (vec) {
        *(uint2*)p = make_uint2(a, b);
    } else {
        p[0] = (uint16_t)a; p[1] = (uint16_t)(a >> 16);
        p[2] = (uint16_t)b; p[3] = (uint16_t)(b >> 16);
    }
}
__device__ __forceinline__ void ffn16_store4(float* p, bool vec, const float* v)
{
    if (vec) {
        *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = v[e];
    }
}

// ---- training mode (ffn_bf16_train_math.h) ----------------------------------------------------------------------------------------------
// The four lanes of a quad are the tokens 4 q .. 4 q + 3 (a tile starts at a multiple of 64), and one Philox call gives the draws of
// those four tokens at one column.  Lane e of the quad makes the call for the e-th of four columns; the 4 x 4 transpose below hands
// every lane its own token's draw at all four: one call per lane where one per element would be four.
__device__ __forceinline__ void ffn16_quad_transpose(uint32_t w[4], int e)     // in: w[u] = draw of token u at column e; out: w[c] = own token at column c
{
    {
        const bool odd = e & 1;
        const uint32_t s0 = odd ? w[0] : w[1], s1 = odd ? w[2] : w[3];
        const uint32_t r0 = __shfl_xor(s0, 1), r1 = __shfl_xor(s1, 1);
        if (odd) { w[0] = r0; w[2] = r1; } else { w[1] = r0; w[3] = r1; }
    }
    {
        const bool up = e & 2;
        const uint32_t s0 = up ? w[0] : w[2], s1 = up ? w[1] : w[3];
        const uint32_t r0 = __shfl_xor(s0, 2), r1 = __shfl_xor(s1, 2);
        if (up) { w[0] = r0; w[1] = r1; } else { w[2] = r0; w[3] = r1; }
    }
}
// the draws of token `tok` (lane e = tok & 3 of its quad) at the columns c0 .. c0 + 3 of `stream`; every lane of the quad calls it
__device__ __forceinline__ void ffn16_draws4(const DropoutParams& d, int stream, long long tok, int c0, uint32_t w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (d.on[stream]) {
        const int e = (int)(tok & 3);
        dropout_draws(d.seed, (uint32_t)stream, (unsigned long long)tok >> 2, (uint32_t)(c0 + e), w);
        ffn16_quad_transpose(w, e);
    }
}

}  // namespace semicrf
