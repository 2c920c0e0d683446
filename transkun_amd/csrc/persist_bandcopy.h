#pragma once
// persist_bandcopy.h -- the COPY role of the persistent sweep (persist.hip, SEMICRF_BANDX): spare waves of the panel workgroups
// copy the band into spine-major order while the sweep runs, so that the spines' loaders read whole 128-byte lines.
#include "persist_spine.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// BAND COPY (SEMICRF_BANDX): the band in spine-major order
// ---------------------------------------------------------------------------------------------
// A spine reads its band as 16-byte pieces (its 4 chains) of 128-byte lines: 64 lines per 1 KB load, 1024 line fills per row
// block through its compute unit's L1.  In the copy a spine's tile is 4 KB contiguous -- [column][row][4 chains], the loader's
// LDS image -- so the same load touches 8 lines.  One copy unit = (row block kr, 32-chain group g, band tile t, column quarter
// q): 64 cells x 128 bytes in, 1 KB to each of the group's 8 spines out; lane = (cell of 8, chain quad): 8 lanes read one whole
// line, and the 8 lanes of a quad write 128 contiguous bytes.  Cells and clamps are exactly the loader's own (bit-identical LDS).
template <int DIR>
__device__ __forceinline__ void band_copy_load(const float* __restrict__ score, int T, int B, int kr, int g, int t, int q, int lane,
                                               v4u_a4 (&v)[8])
{
    const int q8 = lane & 7, cs = lane >> 3;
    const int cbase = (g * (GP / GS) + q8) * GS;             // the batch's spine number x 4
    const size_t Bs = (size_t)B;
    const size_t last4 = (size_t)T * T * Bs - 4;
    const int kc = kr - t > 0 ? kr - t : 0;                  // tile t: column block kr - t (the ring's tiles, newest first)
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int ci = q * 64 + it * 8 + cs;                 // cell of the tile in LDS order: column (ci >> 4), row (ci & 15)
        const int col = ci >> 4, tr = ci & 15;
        const int prow_t = kr * PB + tr < T ? kr * PB + tr : T - 1;
        int pj = kc * PB + col;
        pj = pj < prow_t ? pj : (prow_t > 0 ? prow_t - 1 : 0);
        size_t off = cell_index<DIR>(prow_t, pj, T) * Bs + (cbase < B ? cbase : 0);
        off = off < last4 ? off : last4;
        v[it] = *(const v4u_a4*)(score + off);
    }
}
__device__ __forceinline__ void band_copy_store(float* __restrict__ band, int B, int bandSpines, int kr, int g, int t, int q, int lane,
                                                const v4u_a4 (&v)[8])
{
    const int q8 = lane & 7, cs = lane >> 3;
    const int sgG = g * (GP / GS) + q8;
    if (sgG * GS >= B) return;
    // loader tile index i: column block kr - (RING-1) + i
    const int ti = RING - 1 - t;
    // write-through stores (sc1): the reader is another compute unit of the same launch, possibly on another XCD
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)band, 0, 0x7fffffff, 0x00020000);
    const unsigned voff = (unsigned)(((((size_t)kr * bandSpines + sgG) * RING + ti) * (TILE_BYTES / 4) + (q * 64 + cs) * 4) * 4);
#pragma unroll
    for (int it = 0; it < 8; ++it) __builtin_amdgcn_raw_buffer_store_b128(v[it], rs, voff + it * 128, 0, 16);
}

// COPY role: tasks (row block kr >= bandK0, band tile t, 32-chain group g) in that order from an atomic queue; a task is the tile's
// four quarters, then -- all of its stores acknowledged -- the launch tag in the tile's flag word.
template <int DIR>
__device__ __forceinline__ void copy_role(const SweepParams& P)
{
    const int K = P.K, nG = P.nPanelGroups, g0 = P.c0 / GP;
    const int nTasks = (K - P.bandK0) * RING * nG;
    const int lane = threadIdx.x & 63;
    while (true) {
        int task = 0;
        if (lane == 0) task = (int)(atomicAdd(P.ctrl + CTRL_COPYQ, 1u) + 1u);
        task = __builtin_amdgcn_readfirstlane(task);
        if (task >= nTasks) break;
        const int g = task % nG, t = (task / nG) % RING, kr = P.bandK0 + task / (nG * RING);
        // the tile's four quarters, two of them in flight (a quarter is eight 16-byte loads per lane: a wave with one quarter in flight
        // needs 12 us per tile, and the first row blocks of the copy are wanted 6 us into the sweep)
        v4u_a4 va[8], vb[8];
        band_copy_load<DIR>(P.score, P.T, P.B, kr, g0 + g, t, 0, lane, va);
        band_copy_load<DIR>(P.score, P.T, P.B, kr, g0 + g, t, 1, lane, vb);
        band_copy_store(P.band, P.B, P.bandSpines, kr, g0 + g, t, 0, lane, va);
        band_copy_load<DIR>(P.score, P.T, P.B, kr, g0 + g, t, 2, lane, va);
        band_copy_store(P.band, P.B, P.bandSpines, kr, g0 + g, t, 1, lane, vb);
        band_copy_load<DIR>(P.score, P.T, P.B, kr, g0 + g, t, 3, lane, vb);
        band_copy_store(P.band, P.B, P.bandSpines, kr, g0 + g, t, 2, lane, va);
        band_copy_store(P.band, P.B, P.bandSpines, kr, g0 + g, t, 3, lane, vb);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // (every lane stores the same word: a lane-0 branch here would be threaded into the next draw's, see path_role)
        __builtin_amdgcn_wave_barrier();
        __hip_atomic_store(P.bandFlags + ((size_t)(g0 + g) * (K + 2) + kr) * 8 + t, ((P.tag & 0xffffu) << 16) | (unsigned)kr, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace semicrf
