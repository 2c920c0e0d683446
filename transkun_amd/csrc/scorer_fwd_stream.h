// scorer_fwd_stream.h -- the streaming forward kernel (16-byte aligned rows, T < 256 by default).  Included by scorer_mfma.hip.
#pragma once
#include "scorer_fwd_regload.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// Streaming variant: persistent, barrier-free, no output tile
// ---------------------------------------------------------------------------------------------
// A first LDS-staged version kept the output tile of the kernel above (one workgroup per 32x32 tile and 8 chains, 1.85 ms
// at T=1024, C=352, D=256): 19 % of the time no workgroup was resident (133 KB of LDS: the next one starts only when the
// previous one has drained its stores) and a quarter of a workgroup's cycles were pipeline fill, barrier and write-out.
// Here
//   * a wave owns FOUR ADJACENT chains of one 32x32 tile: it multiplies them one after the other, keeps the finished
//     blocks in registers and writes each cell's four chains as one 16-byte piece straight from registers -- the
//     eight waves of a workgroup cover 32 adjacent chains of the same tile, i.e. whole 128-byte lines, which L2 merges;
//     no output tile in LDS, no barrier, waves never wait for each other;
//   * workgroups are persistent (one per CU, 8 waves = 2 per SIMD) and walk their XCD's part of the work list; the
//     operand stream (two 8 KB LDS stages per wave + the register double buffer) runs on across chains and tiles;
//   * consecutive matrix instructions alternate between two accumulators (summed at the end of a chain).
constexpr int YW = 8;                      // waves per workgroup
constexpr int YNS = 2;                     // LDS stages per wave
constexpr int YG = 4 * YW;                 // chains per workgroup item

__global__ __launch_bounds__(64 * YW) void interval_score_stream_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ diag, int C, int T, int D,
    long long ldq, long long ldk, long long ldd, float qscale, int mode, int full, float* __restrict__ S,
    const int2* __restrict__ work, int nlist)
{
    extern __shared__ __attribute__((aligned(16))) char ylds[];    // [YW waves][YNS][ZSTAGE]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int row = lane & 31, half = lane >> 5;
    char* const stage0 = ylds + wave * (YNS * ZSTAGE);
    const unsigned stage0_addr = z_lds_addr(stage0);
    const int nchunk = D / ZCH;                                     // even (D % 64 == 0)
    const int xcd = blockIdx.x % NXCD, slot0 = blockIdx.x / NXCD, nslots = gridDim.x / NXCD;
    const int nper = nlist / NXCD;                                  // entries per XCD (the tail may be padding)

    // reading lanes: lane = (row, half); segment 4*half + m of the row, m = 0..3
    unsigned rd[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) rd[m] = (unsigned)(row * 128 + (((4 * half + m) ^ ((row >> 1) & 7)) * 16));

    // ---- request side: (item, chain of the quad, chunk) walked with counters ---------------------------------
    int nx_item = slot0;                       // index into this XCD's list
    int nx_j = 0, nx_ch = 0, nx_stage = 0;
    bool nx_valid = false;
    unsigned voq[4], vok[4];
    const float* nx_q = q;
    const float* nx_k = k;
    int nx_c4 = 0;
    auto set_chain = [&]() {
        const int c = nx_c4 + nx_j < C ? nx_c4 + nx_j : C - 1;
        nx_q = q + (size_t)c * T * ldq;
        nx_k = k + (size_t)c * T * ldk;
    };
    auto set_item = [&]() {
        nx_valid = false;
        if (nx_item < nper) {
            const int2 wk = work[(size_t)nx_item * NXCD + xcd];
            if (wk.x >= 0) {
                nx_valid = true;
                const int e0 = (wk.x & 0xffff) * ST, b0 = (wk.x >> 16) * ST;
                nx_c4 = wk.y * YG + wave * 4;
                // loading lanes: piece j (0..3) covers rows 8j .. 8j+7, lane = (row within the piece, 16-byte position)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int lr = 8 * j + (lane >> 3);
                    const int seg = (lane & 7) ^ ((lr >> 1) & 7);
                    const int er = e0 + lr < T ? e0 + lr : T - 1;          // clamped rows (masked at the write)
                    const int br = b0 + lr < T ? b0 + lr : T - 1;
                    voq[j] = (unsigned)(((size_t)er * ldq + seg * 4) * 4);
                    vok[j] = (unsigned)(((size_t)br * ldk + seg * 4) * 4);
                }
                nx_j = 0;
                nx_ch = 0;
                set_chain();
            }
        }
    };
    // one 1 KB piece of the next chunk: p < 4 -> q rows 8p.., else k rows 8(p-4)..
    auto issue_piece = [&](int p) {
        char* dst = stage0 + nx_stage * ZSTAGE + p * 1024;
        if (p < 4) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)nx_q, 0, 0x7fffffff, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)dst, 16, voq[p & 3], nx_ch * (ZCH * 4), 0, 0);
        } else {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)nx_k, 0, 0x7fffffff, 0x00020000);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)dst, 16, vok[p & 3], nx_ch * (ZCH * 4), 0, 0);
        }
    };
    auto advance_next = [&]() {
        nx_stage ^= 1;
        if (++nx_ch == nchunk) {
            nx_ch = 0;
            if (++nx_j == 4) {
                nx_item += nslots;
                set_item();
            } else {
                set_chain();
            }
        }
    };
    auto read_chunk = [&](int stage, v4f (&qa)[4], v4f (&ka)[4]) {
        const unsigned sb = stage0_addr + (unsigned)(stage * ZSTAGE);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const unsigned a = sb + rd[m];
            asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:4096" : "=&v"(qa[m]), "=&v"(ka[m]) : "v"(a));
        }
    };
    auto wait_reads = [&](v4f (&qa)[4], v4f (&ka)[4]) {
        asm volatile("s_waitcnt lgkmcnt(0)"
                     : "+v"(qa[0]), "+v"(qa[1]), "+v"(qa[2]), "+v"(qa[3]), "+v"(ka[0]), "+v"(ka[1]), "+v"(ka[2]), "+v"(ka[3]));
    };

    set_item();
    if (!nx_valid) return;
    // the compute side's view of the current item
    int cur_item = nx_item;
    int2 cur_wk = work[(size_t)cur_item * NXCD + xcd];

    f32x16 accA, accB;
#pragma unroll
    for (int r = 0; r < 16; ++r) { accA[r] = 0.0f; accB[r] = 0.0f; }
    float hold[3][16];
    v4f qa0[4], ka0[4], qa1[4], ka1[4];

    // prologue: chunk 0 requested and read into registers, chunk 1 requested
#pragma unroll
    for (int p = 0; p < 8; ++p) issue_piece(p);
    advance_next();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    read_chunk(0, qa0, ka0);
    wait_reads(qa0, ka0);
    if (nx_valid) {
#pragma unroll
        for (int p = 0; p < 8; ++p) issue_piece(p);
        advance_next();
    }
    int rd_stage = 1;

    // step: the current chunk is in registers (qc, kc); the next one (in flight since the previous step) is awaited and
    // read into the other set; the one after it is requested between the matrix instructions
    auto step = [&](v4f (&qc)[4], v4f (&kc)[4], v4f (&qn)[4], v4f (&kn)[4], bool last_of_stream) {
        if (!last_of_stream) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            // the chunk after the next goes into the stage of the current one (which is in registers); all of it is
            // requested NOW so that every piece has the whole step to arrive
            if (nx_valid) {
#pragma unroll
                for (int p = 0; p < 8; ++p) issue_piece(p);
                advance_next();
            }
            read_chunk(rd_stage, qn, kn);
            rd_stage ^= 1;
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            accA = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[m].x, kc[m].x, accA, 0, 0, 0);
            accB = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[m].y, kc[m].y, accB, 0, 0, 0);
            accA = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[m].z, kc[m].z, accA, 0, 0, 0);
            accB = __builtin_amdgcn_mfma_f32_32x32x2f32(qc[m].w, kc[m].w, accB, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (!last_of_stream) wait_reads(qn, kn);
    };

    while (true) {
        // is there an item after this one (for this workgroup)?  the request side knows: it is at most two chunks ahead
        const int e0 = (cur_wk.x & 0xffff) * ST, b0 = (cur_wk.x >> 16) * ST;
        const int c4 = cur_wk.y * YG + wave * 4;
        int nxt_item = cur_item + nslots;
        bool nxt_ok = false;
        int2 nxt_wk = make_int2(-1, 0);
        if (nxt_item < nper) {
            nxt_wk = work[(size_t)nxt_item * NXCD + xcd];
            nxt_ok = nxt_wk.x >= 0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            for (int ch = 0; ch < nchunk; ch += 2) {
                step(qa0, ka0, qa1, ka1, false);
                step(qa1, ka1, qa0, ka0, !nxt_ok && j == 3 && ch + 2 == nchunk);
            }
            if (j < 3) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { hold[j][r] = accA[r] + accB[r]; accA[r] = 0.0f; accB[r] = 0.0f; }
            }
        }
        // ---- write the item's four chains: one 16-byte piece per cell (C/D layout: col = lane & 31,
        //      row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) ----
        {
            const int bj = row, b = b0 + bj;
            const bool vec = (C & 3) == 0 && c4 + 3 < C;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ei = (r & 3) + 8 * (r >> 2) + 4 * half;
                const int e = e0 + ei;
                const int len = e > b ? e - b : b - e;
                const float sc = qscale * len_scale_mfma(len, mode);
                float v[4] = {hold[0][r] * sc, hold[1][r] * sc, hold[2][r] * sc, (accA[r] + accB[r]) * sc};
                accA[r] = 0.0f; accB[r] = 0.0f;
                if (e < T && b < T && (full || b <= e) && c4 < C) {
                    if (e == b) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c4 + i < C) v[i] += diag[((size_t)(c4 + i) * T + e) * ldd];
                    }
                    float* dst = S + ((size_t)e * T + b) * C + c4;
                    if (vec) {
                        *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c4 + i < C) dst[i] = v[i];
                    }
                }
            }
        }
        if (!nxt_ok) break;
        cur_item = nxt_item;
        cur_wk = nxt_wk;
    }
}

static int launch_score_stream(const float* q, const float* k, const float* diag, int C, int T, int D, long long ldq,
                               long long ldk, long long ldd, float qscale, int mode, int full, float* S, int band,
                               hipStream_t stream)
{
    const int nt = (T + ST - 1) / ST;
    const size_t lds = (size_t)YW * YNS * ZSTAGE;
    int nlist = 0;
    const int2* work = score_work_list(nt, (C + YG - 1) / YG, full ? 1 : 0, band, &nlist, stream);
    if (!work) return 1;
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute((const void*)interval_score_stream_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    const int grid = persistent_grid(device_ncu(), NXCD, nlist);      // one workgroup per CU, a whole number per XCD (nlist is a multiple of NXCD)
    hipLaunchKernelGGL(interval_score_stream_kernel, dim3(grid), dim3(64 * YW), lds, stream, q, k, diag, C, T, D, ldq, ldk, ldd,
                       qscale, mode, full, S, work, nlist);
    return 0;
}

}  // namespace semicrf
