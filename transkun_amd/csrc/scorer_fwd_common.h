// scorer_fwd_common.h -- what the forward interval-score kernels of scorer_mfma.hip share: the 32 x 32 work-list tile, the length
// scaling, the LDS-DMA chunk of the LDS-staged kernels.
#pragma once
#include "common.h"
#include "scorer_tiles.h"

namespace semicrf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the 64- / 128-row reference tile kernels (scorer_fwd_tile_ref.h) exist in the debug library only
#if defined(SEMICRF_DEBUG_BUILD) && SEMICRF_DEBUG_BUILD
#define SEMICRF_HAVE_TILE_REF 1
#else
#define SEMICRF_HAVE_TILE_REF 0
#endif

constexpr int ST = 32;        // tile edge (positions)
constexpr int SC = 16;        // chains per workgroup
constexpr int SPAD = SC + 1;  // LDS row padding: conflict-free column writes
constexpr int NXCD = 8;       // workgroup b runs on XCD b % 8
constexpr int XTB = 128;      // columns (begin positions) of the shared-operand tiles

__device__ __forceinline__ float len_scale_mfma(int len, int mode)
{
    if (mode == SEMICRF_LEN_LINEAR) return (float)len;
    if (mode == SEMICRF_LEN_SQRT) return sqrtf((float)len);
    return 1.0f;
}

// ---------------------------------------------------------------------------------------------
// LDS-staged operands (16-byte aligned rows, D % 64 == 0)
// ---------------------------------------------------------------------------------------------
// With one matrix row per lane a register load touches 64 different 128-byte lines and the CU's L1 looks them up one
// per clock: the operand loads, not the matrix pipe, set the pace of the register-load kernel (28 % of the fp32 MFMA rate).
// The streaming and tile kernels copy operands with `buffer_load ... lds`: one instruction moves 8 rows x 128 contiguous bytes
// (8 full lines), a chunk is 32 contraction values of every row.  The 16-byte segments of a row are XOR-swizzled by
// the LOADING lanes ((row >> 1) & 7) so that the row-per-lane ds_read_b128 of the MFMA operands is bank-conflict free
// without padding.  LDS reads in the main loops are asm: the compiler would order every DS operation it sees after ALL
// outstanding LDS-DMA (s_waitcnt vmcnt(0)).
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void_t;

constexpr int ZSTAGE = 8192;              // bytes per stage: q chunk (4 KB) + k chunk (4 KB)
constexpr int ZCH = 32;                   // contraction values per chunk

__device__ __forceinline__ unsigned z_lds_addr(const void* p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}

}  // namespace semicrf
