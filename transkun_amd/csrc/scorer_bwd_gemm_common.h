// scorer_bwd_gemm_common.h -- what the kernels of the packed interval-score backward share (scorer_bwd_gemm.hip): the tile
// constants and the block-triangular layout of the repacked cotangent Gt.
#pragma once
#include "common.h"

#include <type_traits>

namespace semicrf {

typedef __attribute__((address_space(3))) void lds_void_t;

constexpr int GM = 128;            // rows of an output tile
constexpr int GK = 32;             // contraction values per chunk
constexpr int GNS = 3;             // LDS stages
constexpr int GA_BYTES = GM * GK * 4;      // 16 KB: the Gt part of a stage

__device__ __forceinline__ float len_scale_pack(int len, int mode)
{
    if (mode == SEMICRF_LEN_LINEAR) return (float)len;
    if (mode == SEMICRF_LEN_SQRT) return sqrtf((float)len);
    return 1.0f;
}

__device__ __forceinline__ unsigned g_lds_addr(const void* p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---------------------------------------------------------------------------------------------
// Gt layout: per chain a block-triangular matrix.  Rows come in blocks of 128 (GM); the rows of block i hold columns
// 0 .. RL(i)-1 with RL(i) = min(128 (i+1), Tp) -- everything an output tile ever reads (the diagonal block included,
// zero above the diagonal) and nothing else: 56 % of the square at T=1024.
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int gt_row_len(int blk, int Tp) { return (blk + 1) * GM < Tp ? (blk + 1) * GM : Tp; }
// floats before block blk (blocks before it are full: 128 rows of 128 (i+1) columns)
__host__ __device__ __forceinline__ size_t gt_block_off(int blk) { return (size_t)GM * GM * ((size_t)blk * (blk + 1) / 2); }
__host__ __device__ __forceinline__ size_t gt_chain_floats(int Tp)
{
    const int nb = (Tp + GM - 1) / GM;
    return gt_block_off(nb - 1) + (size_t)(Tp - (nb - 1) * GM) * Tp;
}

}  // namespace semicrf
