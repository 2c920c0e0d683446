// scorer_fwd_tile_ref.h -- the 64- / 128-row shared-operand tile kernels: the bit-level reference of the default kernel
// (scorer_tiled.hip), compiled into the debug library only.  Included by scorer_mfma.hip under SEMICRF_HAVE_TILE_REF.
#pragma once
#include "scorer_fwd_common.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// 128x128 variant: operands shared by the whole workgroup through LDS
// ---------------------------------------------------------------------------------------------
// Counters of the streaming kernel (1.8 ms): the L1 waits on L2 80 % of the time and delivers 15 B/clk/CU -- its miss
// queue holds about 8 KB and an L2 round trip is ~600 cycles, so that IS what a CU can pull, whatever the access
// pattern.  32x32 tiles need 32 B/clk/CU to keep the fp32 matrix pipe busy (8 flop per operand byte).  Hence the
// classic answer: the eight waves of a workgroup multiply ONE chain's 128x128 tile together (wave = 32 rows x 64
// columns, two accumulators), the q and k chunks (128 rows x 32 contraction values each, 32 KB per stage, swizzled as
// above) are fetched once per workgroup: 32 flop per byte, 8 B/clk/CU at full rate.  A workgroup item is one tile for
// FOUR adjacent chains: finished blocks stay in registers and every cell leaves as one 16-byte piece.  The eight
// workgroups that cover the 32 chains of a 128-byte output line run side by side on the same XCD (persistent
// workgroups, static schedule: slot % 8 = chain quad), so its L2 assembles whole lines.  One s_barrier per chunk (no
// fence: the prefetch stays in flight); the matrix instructions of a wave alternate between its two accumulators.
constexpr int XNS = 3;                     // LDS stages (4: measured no faster -- 1.32-1.34 against 1.33 ms, and two 64-row workgroups per CU no
                                           // longer fit; raised wave priority during a chunk's matrix instructions: 1.33-1.35 ms, the same.
                                           // profiles/r02_scorer.md)

// XTE = tile rows (end positions): 128 -> 8 waves, one workgroup per CU; 64 -> 4 waves, two (independent) workgroups
// per CU whose barriers and operand reads fall into each other's matrix phases (24 instead of 32 flop per byte).
// C = real chains; Cs = slots (the chain pitch of S); see SlotGeom.
// The 64- / 128-row shared-operand tile kernels: superseded as the default by scorer_tiled.hip (bit-identical results); since
// round 4 they are compiled into the DEBUG library only (libsemicrf_hip_debug.so, -DSEMICRF_DEBUG_BUILD=1), where the parity tests
// load them explicitly as the reference of test_scorer_tiled_bits.  The release library keeps the tiled kernel (default), the
// streaming kernel (T < 256), the register-load kernel (any alignment / contraction size) and the opt-in three-limb kernel.
template <int XTE>
__global__ __launch_bounds__(512, 2) void interval_score_tile_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ diag, int C, int T, int D,
    long long ldq, long long ldk, long long ldd, float qscale, int mode, int full, float* __restrict__ S,
    int ntiles, int nquadp, int Cs, SlotGeom G, const float* __restrict__ rowc, long long ldrc)
{
    constexpr int XW = XTE / 16;                   // waves: (row block of 32, column half of 64)
    constexpr int KP = 16 / XW;                    // k pieces (8 rows x 128 bytes) per wave and chunk; q pieces: 2
    constexpr int XSTAGE = (XTE + XTB) * 128;      // bytes per stage: q chunk | k chunk
    extern __shared__ __attribute__((aligned(16))) char xlds[];    // [XNS][XSTAGE]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = lane & 31, half = lane >> 5;
    const int wer = wave >> 1, wh = wave & 1;                       // this wave: rows 32*wer.., columns 64*wh.. of the tile
    const unsigned lds0 = z_lds_addr(xlds);
    const int nchunk = D / ZCH;
    const int nbt = (T + XTB - 1) / XTB;                            // column tiles
    const int xcd = blockIdx.x % NXCD, slot0 = blockIdx.x / NXCD, nslots = gridDim.x / NXCD;
    const long long nitems = (long long)ntiles * nquadp;            // nquadp: chain quads, padded to a multiple of 8

    // entry u of this XCD's list -> global item n: 8 consecutive entries = the 8 quads of one 128-byte line group
    auto item_of = [&](int u, int& et, int& bt, QuadInfo& qi) -> bool {
        const long long n = (long long)(u >> 3) * (8 * NXCD) + xcd * 8 + (u & 7);
        if (n >= nitems) return false;
        const int t = (int)(n / nquadp);
        qi = quad_info(G, (int)(n % nquadp));
        tile_of_index<XTE == XTB>(t, nbt, full, et, bt);
        return true;
    };

    // reading lanes: lane = (row, half); segment 4*half + m of the row
    unsigned rdq[4], rdk[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const unsigned sw = (unsigned)((((4 * half + m) ^ ((row >> 1) & 7)) * 16));
        rdq[m] = (unsigned)((32 * wer + row) * 128) + sw;
        rdk[m] = (unsigned)(XTE * 128 + (64 * wh + row) * 128) + sw;       // second column block: + 32 rows = + 4096 bytes
    }

    // ---- request side (identical in all waves): (entry, chain of the quad, chunk, stage) ----------------------
    int nx_u = slot0, nx_j = 0, nx_ch = 0, nx_stage = 0;
    QuadInfo nx_q4 = {0, 0, 0, 0};
    bool nx_valid = false;
    unsigned voq[2], vok[4];      // (a [KP] array captured by the lambdas below trips the host compiler)
    const float* nx_q = q;
    const float* nx_k = k;
    // row constants (rowc != NULL, the merged projection): the XTE constants of chain j of a quad ride along with the chain's first
    // chunk -- wave j asks for them (one dword per lane, straight into LDS) right after its operand pieces, so every vmcnt wait
    // below stays at least as strict as without them -- into one of two buffers [chain][row] behind the stages, alternating by
    // REAL item (padding items request nothing).  The epilogue of item n reads buffer n & 1 while the requests of item n + 1 are
    // in flight; those of item n + 2 are issued only after a barrier of item n + 1 (>= 2 chunks per chain: D % 64 == 0), which
    // every wave reaches after its epilogue of item n.
    static_assert(XNS <= 3, "the two row-constant buffers assume requests run at most two chunks ahead");
    constexpr int RC_BYTES = 4 * XTE * 4;
    unsigned vorc[2] = {0u, 0u};
    const float* nx_rc = rowc;
    int nx_cnt = 0;
    auto set_chain = [&]() {
        const int c = nx_q4.ck + nx_j;                                       // nx_j < nx_q4.nr: a real chain
        nx_q = q + (size_t)c * T * ldq;
        nx_k = k + (size_t)c * T * ldk;
        if (rowc) nx_rc = rowc + (size_t)c * T * ldrc;
    };
    auto set_item = [&]() {
        int et = 0, bt = 0;
        // padding items (no real chain) request nothing: the consuming side skips them the same way
        while ((nx_valid = item_of(nx_u, et, bt, nx_q4)) && nx_q4.nr == 0) nx_u += nslots;
        if (nx_valid && rowc) {
#pragma unroll
            for (int h = 0; h < XTE / 64; ++h) {
                const int er = et * XTE + 64 * h + lane < T ? et * XTE + 64 * h + lane : T - 1;
                vorc[h] = (unsigned)((size_t)er * ldrc * 4);
            }
        }
        if (nx_valid) {
            // loading lanes: a piece is 8 rows x 128 bytes; this wave's q pieces 2*wave.. and k pieces KP*wave..
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int lr = 8 * (2 * wave + j) + (lane >> 3);
                const int seg = (lane & 7) ^ ((lr >> 1) & 7);
                const int er = et * XTE + lr < T ? et * XTE + lr : T - 1;     // clamped rows (masked at the write)
                voq[j] = (unsigned)(((size_t)er * ldq + seg * 4) * 4);
            }
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const int lr = 8 * (KP * wave + j) + (lane >> 3);
                const int seg = (lane & 7) ^ ((lr >> 1) & 7);
                const int br = bt * XTB + lr < T ? bt * XTB + lr : T - 1;
                vok[j] = (unsigned)(((size_t)br * ldk + seg * 4) * 4);
            }
            nx_j = 0;
            nx_ch = 0;
            set_chain();
        }
    };
    auto issue_chunk = [&]() {
        char* dq = xlds + nx_stage * XSTAGE + (2 * wave) * 1024;
        char* dk = xlds + nx_stage * XSTAGE + XTE * 128 + (KP * wave) * 1024;
        const auto rq = __builtin_amdgcn_make_buffer_rsrc((void*)nx_q, 0, 0x7fffffff, 0x00020000);
        const auto rk = __builtin_amdgcn_make_buffer_rsrc((void*)nx_k, 0, 0x7fffffff, 0x00020000);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, (lds_void_t*)dq, 16, voq[0], nx_ch * (ZCH * 4), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rq, (lds_void_t*)(dq + 1024), 16, voq[1], nx_ch * (ZCH * 4), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void_t*)dk, 16, vok[0], nx_ch * (ZCH * 4), 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void_t*)(dk + 1024), 16, vok[1], nx_ch * (ZCH * 4), 0, 0);
        if (KP == 4) {
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void_t*)(dk + 2048), 16, vok[KP - 2], nx_ch * (ZCH * 4), 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rk, (lds_void_t*)(dk + 3072), 16, vok[KP - 1], nx_ch * (ZCH * 4), 0, 0);
        }
        if (rowc && nx_ch == 0 && wave == nx_j) {
            const auto rr = __builtin_amdgcn_make_buffer_rsrc((void*)nx_rc, 0, 0x7fffffff, 0x00020000);
            char* dr = xlds + XNS * XSTAGE + (nx_cnt & 1) * RC_BYTES + nx_j * (XTE * 4);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_void_t*)dr, 4, vorc[0], 0, 0, 0);
            if (XTE == 128) __builtin_amdgcn_raw_ptr_buffer_load_lds(rr, (lds_void_t*)(dr + 256), 4, vorc[XTE / 64 - 1], 0, 0, 0);
        }
        nx_stage = nx_stage + 1 == XNS ? 0 : nx_stage + 1;
        if (++nx_ch == nchunk) {
            nx_ch = 0;
            if (++nx_j == nx_q4.nr) {
                nx_u += nslots;
                ++nx_cnt;
                set_item();
            } else {
                set_chain();
            }
        }
    };

    set_item();
    int cur_u = slot0;
    {
        int e0_, b0_; QuadInfo q0_;
        if (!item_of(cur_u, e0_, b0_, q0_)) return;                 // uniform over the workgroup
    }

    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    float hold[3][2][16];

    // prologue: XNS-1 chunks requested
    int inflight = 0;                           // chunks requested and not yet consumed
#pragma unroll
    for (int i = 0; i < XNS - 1; ++i)
        if (nx_valid) { issue_chunk(); ++inflight; }
    int rd_stage = 0;
    int cur_cnt = 0;                            // real items consumed: which row-constant buffer

    while (true) {
        int et, bt;
        QuadInfo qi;
        (void)item_of(cur_u, et, bt, qi);
        const int c4 = qi.c4;
        // 32x32 blocks of this wave that lie entirely above the diagonal are not multiplied (nor written)
        const int erow = et * (XTE / 32) + wer, bcol = bt * (XTB / 32) + 2 * wh;
        const bool on0 = full || bcol <= erow, on1 = full || bcol + 1 <= erow;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int ch = 0; ch < (j < qi.nr ? nchunk : 0); ++ch) {
                // this wave's pieces of the current chunk have landed (a younger request may stay in flight) ...
                if (inflight >= 2) {
                    if (KP == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                // ... and so have everybody's; everybody is also done reading the previous chunk (no fence: the
                // prefetch stays in flight)
                __builtin_amdgcn_s_barrier();
                --inflight;
                if (nx_valid) { issue_chunk(); ++inflight; }        // into the stage of the previous chunk
                v4f qa[4], ka0[4], ka1[4];
                const unsigned sb = lds0 + (unsigned)(rd_stage * XSTAGE);
                rd_stage = rd_stage + 1 == XNS ? 0 : rd_stage + 1;
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %4\n\tds_read_b128 %2, %4 offset:4096"
                                 : "=&v"(qa[m]), "=&v"(ka0[m]), "=&v"(ka1[m])
                                 : "v"(sb + rdq[m]), "v"(sb + rdk[m]));
                }
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(qa[0]), "+v"(qa[1]), "+v"(qa[2]), "+v"(qa[3]), "+v"(ka0[0]), "+v"(ka0[1]), "+v"(ka0[2]),
                               "+v"(ka0[3]), "+v"(ka1[0]), "+v"(ka1[1]), "+v"(ka1[2]), "+v"(ka1[3]));
                __builtin_amdgcn_sched_barrier(0);
                if (on0 && on1) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].x, ka0[m].x, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].x, ka1[m].x, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].y, ka0[m].y, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].y, ka1[m].y, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].z, ka0[m].z, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].z, ka1[m].z, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].w, ka0[m].w, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].w, ka1[m].w, acc1, 0, 0, 0);
                    }
                } else if (on0) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) {
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].x, ka0[m].x, acc0, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].y, ka0[m].y, acc0, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].z, ka0[m].z, acc0, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].w, ka0[m].w, acc0, 0, 0, 0);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            if (j < 3) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    hold[j][0][r] = acc0[r]; hold[j][1][r] = acc1[r];
                    acc0[r] = 0.0f; acc1[r] = 0.0f;
                }
            }
        }
        // ---- write the item's four chains: one 16-byte piece per cell (C/D layout: col = lane & 31,
        //      row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) ----
        {
            const bool vec = (Cs & 3) == 0 && c4 + 3 < Cs;
            // merged projection (interval_score_fwd_pc): the row constants of this wave's rows, four consecutive rows (one row group
            // r >> 2) of the four chains per pass
            const unsigned rb = lds0 + (unsigned)(XNS * XSTAGE + (cur_cnt & 1) * RC_BYTES + (32 * wer + 4 * half) * 4);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                v4f rcv[4];
                if (rowc) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        asm volatile("ds_read_b128 %0, %1" : "=v"(rcv[i]) : "v"(rb + (unsigned)((i * XTE + 8 * g) * 4)));
                    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rcv[0]), "+v"(rcv[1]), "+v"(rcv[2]), "+v"(rcv[3]));
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int b = bt * XTB + 64 * wh + 32 * t + row;
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int r = 4 * g + rr;
                        const int e = et * XTE + 32 * wer + rr + 8 * g + 4 * half;
                        const int len = e > b ? e - b : b - e;
                        const float sc = qscale * len_scale_mfma(len, mode);
                        const float last = t == 0 ? acc0[r] : acc1[r];
                        float v[4] = {hold[0][t][r], hold[1][t][r], hold[2][t][r], last};
                        if (rowc) {
#pragma unroll
                            for (int i = 0; i < 4; ++i)
                                if (i < qi.nr) v[i] += rcv[i][rr];
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] *= sc;
                        // (this write is a copy in each tile kernel: as one function in scorer_tiles.h it changes the three-limb kernel's register allocation)
                        if (e < T && b < T && (full || b <= e) && qi.nr > 0) {
                            if (e == b) {
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    if (i < qi.nr) v[i] += diag[((size_t)(qi.ck + i) * T + e) * ldd];
                            }
                            float* dst = S + ((size_t)e * T + b) * Cs + c4;
                            if (vec) {
                                // (plain stores: L2 merges the eight 16-byte pieces of a line; nontemporal ones do not -- 2.4 ms)
                                *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);      // ghost slots of the quad: exact zeros (hold = 0)
                                for (int z = 4; z <= qi.tz; z += 4) *(float4*)(dst + z) = make_float4(0.f, 0.f, 0.f, 0.f);   // the group's ghost tail
                            } else {
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    if (i < qi.nr) dst[i] = v[i];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
        }
        if (qi.nr > 0) ++cur_cnt;
        cur_u += nslots;
        int e2, b2;
        QuadInfo q2;
        if (!item_of(cur_u, e2, b2, q2)) break;
    }
}

template <int XTE>
static int launch_score_tile(const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq,
                             long long ldk, long long ldd, float qscale, int mode, int full, float* S, hipStream_t stream,
                             int group, int pitch, const float* rowc, long long ldrc)
{
    const SlotGeom G = slot_geom(C, group, pitch);
    const int Cs = (C / group) * pitch;
    const int net = (T + XTE - 1) / XTE, nbt = (T + XTB - 1) / XTB;
    int ntiles = 0;
    if (full) ntiles = net * nbt;
    else
        for (int et = 0; et < net; ++et) ntiles += (et * XTE + XTE - 1) / XTB + 1 < nbt ? (et * XTE + XTE - 1) / XTB + 1 : nbt;
    const int nquadp = (G.nrq + 7) / 8 * 8;
    const size_t lds = (size_t)XNS * (XTE + XTB) * 128 + 2 * (4 * XTE * 4);     // stages + the two row-constant buffers
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute((const void*)interval_score_tile_kernel<XTE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    // persistent workgroups (128 / XTE per CU); per XCD a multiple of 8 slots
    const long long nitems = (long long)ntiles * nquadp;
    const int grid = persistent_grid((long long)device_ncu() * (128 / XTE), 8 * NXCD, (nitems + 8 * NXCD - 1) / (8 * NXCD) * (8 * NXCD));
    hipLaunchKernelGGL(interval_score_tile_kernel<XTE>, dim3(grid), dim3(XTE * 4), lds, stream, q, k, diag, C, T, D, ldq, ldk, ldd,
                       qscale, mode, full, S, ntiles, nquadp, Cs, G, rowc, ldrc);
    return 0;
}

}  // namespace semicrf
