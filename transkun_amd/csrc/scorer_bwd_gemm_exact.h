// scorer_bwd_gemm_exact.h -- the two products of the packed interval-score backward, exact fp32.  Included by scorer_bwd_gemm.hip.
#pragma once
#include "scorer_bwd_gemm_common.h"
#include "bf16x3.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// GEMM: out[c][m][:] = sum_k A[m][k] other[c][k][:]   with A = Gt (dq: m = e, k = b) or Gt^T (dk: m = b, k = e)
// ---------------------------------------------------------------------------------------------
// AT: A is read transposed (dk).  NW: 32-column blocks per wave (D = 64 NW; NW in {1, 2, 4}).
// rsum (!AT only, may be NULL): rsum[(c T + m) ldrs] = sum_k A[m][k] -- the gradient of the merged projection's row constant
// (include/semicrf_hip.h: interval_score_bwd_ws_pc) falls out of the A values this kernel reads anyway: every lane adds up the
// contraction values of its row that pass through it (a fixed order: chunk, group, component), the two half-waves are combined at
// the end of the item.
template <bool AT, int NW>
__global__ __launch_bounds__(512, 2) void score_bwd_gemm_kernel(const float* __restrict__ Gt, int Tp,
                                                                const float* __restrict__ other, long long ldo,
                                                                float* __restrict__ out, long long ldout, int C, int T,
                                                                float* __restrict__ rsum, long long ldrs)
{
    constexpr int D = 64 * NW;
    constexpr int GB_BYTES = GK * D * 4;               // the k/q part of a stage: 32 rows
    constexpr int GSTAGE = GA_BYTES + GB_BYTES;
    constexpr int RPP = 4 / NW;                        // k/q rows per 1 KB piece
    constexpr int NLOAD = 2 + NW;                      // pieces per wave and chunk
    extern __shared__ __attribute__((aligned(16))) char glds[];    // [GNS][GSTAGE]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int l31 = lane & 31, half = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;           // this wave: rows 32*wm.., columns 32*NW*wn.. of the tile
    const unsigned lds0 = g_lds_addr(glds);
    const int nm = (T + GM - 1) / GM;                  // output tiles per chain
    const long long nitems = (long long)nm * C;
    const int nkt = Tp / GK;                           // chunks of the whole contraction axis

    // item n: tiles dealt longest first (dq: the last row tile has the longest contraction range, dk: the first)
    auto item_of = [&](long long n, int& c, int& mi, int& kbeg, int& nk) -> bool {
        if (n >= nitems) return false;
        const int r = (int)(n / C);
        c = (int)(n % C);
        mi = AT ? r : nm - 1 - r;
        if (AT) {
            kbeg = mi * (GM / GK);
            nk = nkt - kbeg;
        } else {
            kbeg = 0;
            nk = (mi + 1) * (GM / GK) < nkt ? (mi + 1) * (GM / GK) : nkt;
        }
        return true;
    };

    // ---- LDS read addresses (bytes within a stage) ----------------------------------------------------------
    // contraction order inside a chunk: matrix instruction (mm, comp) takes k = 4 mm + comp from lanes 0-31 and
    // k = 16 + 4 mm + comp from lanes 32-63 -- the same permutation for both operands
    unsigned rdA[4];                                   // !AT: one 16-byte segment per mm (row = m, swizzled)
#pragma unroll
    for (int mm = 0; mm < 4; ++mm) {
        const int row = 32 * wm + l31;
        rdA[mm] = (unsigned)(row * 128 + (((4 * half + mm) ^ ((row >> 1) & 7)) * 16));
    }
    const unsigned rdAT = (unsigned)(half * 16 * (GM * 4) + (32 * wm + l31) * 4);        // AT: stage rows = k, 512 bytes each
    const unsigned rdB = (unsigned)(GA_BYTES + half * 16 * (D * 4) + (32 * NW * wn + l31) * 4);

    // ---- request side (identical in all waves) --------------------------------------------------------------
    long long nx_n = blockIdx.x;
    int nx_c = 0, nx_mi = 0, nx_kbeg = 0, nx_nk = 0, nx_j = 0, nx_stage = 0;
    bool nx_valid = item_of(nx_n, nx_c, nx_mi, nx_kbeg, nx_nk);
    if (!nx_valid) return;                             // uniform
    // per-lane byte offsets of this wave's pieces (relative to the chain slab, without the chunk)
    unsigned voA[2], voB[4];                           // (dependent array bounds captured by lambdas trip the host compiler)
    auto set_offsets = [&]() {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int p = 2 * wave + j;                // Gt piece 0..15
            if (!AT) {
                const int row = 8 * p + (lane >> 3);   // m within the tile; 128 contiguous bytes along k
                const int seg = (lane & 7) ^ ((row >> 1) & 7);
                voA[j] = (unsigned)((gt_block_off(nx_mi) + (size_t)row * gt_row_len(nx_mi, Tp) + seg * 4) * 4);
            } else {
                const int row = 2 * p + (lane >> 5);   // k within the chunk; 512 contiguous bytes along m
                voA[j] = (unsigned)row;                  // the row length depends on the chunk: finished in issue_chunk
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int p = NW * wave + j;               // k/q piece 0 .. 8 NW - 1
            const int row = p * RPP + lane / (16 * NW);
            voB[j] = (unsigned)(((size_t)row * ldo + (lane % (16 * NW)) * 4) * 4);
        }
    };
    set_offsets();
    // A chunk's requests = prep (scalars; the walk over the items moves on) + req(0 .. NLOAD-1), in a block behind the barrier.  (One
    // at a time between the chunk's matrix instructions, the two waves of a SIMD at different places: tried and left out, DESIGN.md
    // section 3 -- 2.19 against 2.125 ms at T=1024 x 352 as straight-line bodies per wave group.)
    // (the pending request as plain locals, the resource words made at the request: through a struct handed to the lambdas the HOST
    // pass drops the kernel's instantiation without a diagnostic and the library fails to load with an undefined kernel symbol)
    const float* rq_pa = Gt; const float* rq_pb = other; int rq_na = 0, rq_nb = 0; unsigned rq_da = 0, rq_db = 0, rq_sa = 0, rq_va0 = 0, rq_va1 = 0, rq_kb = 0;
    auto prep = [&]() __attribute__((always_inline)) {
        const int k0 = (nx_kbeg + nx_j) * GK;
        // bounds-checked buffers over the chain's slab: rows past the end read as zero
        const size_t slab = gt_chain_floats(Tp);
        rq_pa = Gt + (size_t)nx_c * slab; rq_na = (int)(slab * 4);
        rq_pb = other + (size_t)nx_c * T * ldo; rq_nb = (int)((size_t)T * ldo * 4);
        rq_da = (unsigned)(nx_stage * GSTAGE + (2 * wave) * 1024);
        rq_db = (unsigned)(nx_stage * GSTAGE + GA_BYTES + (NW * wave) * 1024);
        // AT: the chunk's 32 rows (k = e) lie in one 128-row block kblk; its row length enters the per-lane offsets
        const int kblk = k0 / GM, krl = gt_row_len(kblk, Tp);
        rq_sa = AT ? (unsigned)((gt_block_off(kblk) + (size_t)(k0 - kblk * GM) * krl) * 4) : (unsigned)(k0 * 4);   // inside the slab
        rq_va0 = AT ? (unsigned)((voA[0] * krl + nx_mi * GM + (lane & 31) * 4) * 4) : voA[0];
        rq_va1 = AT ? (unsigned)((voA[1] * krl + nx_mi * GM + (lane & 31) * 4) * 4) : voA[1];
        // the k/q rows of the last chunk may lie past T: their offset goes into the per-lane part, which is what the
        // buffer's range check looks at (the scalar offset is not checked); such rows keep the stage's old contents
        // and meet Gt == 0 (the stages are cleared once at the start so that they never hold a NaN pattern)
        rq_kb = (unsigned)((size_t)k0 * ldo * 4);
        nx_stage = nx_stage + 1 == GNS ? 0 : nx_stage + 1;
        if (++nx_j == nx_nk) {
            nx_j = 0;
            nx_n += gridDim.x;
            nx_valid = item_of(nx_n, nx_c, nx_mi, nx_kbeg, nx_nk);
            if (nx_valid) set_offsets();
        }
    };
    auto req = [&](int i) __attribute__((always_inline)) {
        // (the destination through a named char*: with the cast applied to `glds + ...` directly the HOST pass drops the kernel's
        // instantiation without a diagnostic and the library fails to load with an undefined kernel symbol)
        if (i < 2) {
            const auto ra = __builtin_amdgcn_make_buffer_rsrc((void*)rq_pa, 0, rq_na, 0x00020000);
            char* dst = glds + rq_da + i * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_void_t*)dst, 16, i == 0 ? rq_va0 : rq_va1, rq_sa, 0, 0);
        } else {
            const auto rb = __builtin_amdgcn_make_buffer_rsrc((void*)rq_pb, 0, rq_nb, 0x00020000);
            char* dst = glds + rq_db + (i - 2) * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, (lds_void_t*)dst, 16, voB[i - 2] + rq_kb, 0, 0, 0);
        }
    };
    auto issue_chunk = [&]() __attribute__((always_inline)) {
        prep();
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) req(i);
    };

    // clear the stages once (see issue_chunk)
    for (int i = threadIdx.x; i < GNS * GSTAGE / 16; i += 512) ((float4*)glds)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < NW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    int inflight = 0;
#pragma unroll
    for (int i = 0; i < GNS - 1; ++i)
        if (nx_valid) { issue_chunk(); ++inflight; }
    int rd_stage = 0;
    float rs = 0.0f;                                    // !AT && rsum: this lane's part of its row's sum
    const bool want_rs = !AT && rsum != nullptr;

    long long cur_n = blockIdx.x;
    while (true) {
        int c, mi, kbeg, nk;
        if (!item_of(cur_n, c, mi, kbeg, nk)) break;
        for (int j = 0; j < nk; ++j) {
            // this wave's pieces of the current chunk have landed (a younger request may stay in flight) ...
            if (inflight >= 2) {
                if (NLOAD == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else if (NLOAD == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            // ... and so have everybody's; everybody is also done reading the previous chunk
            __builtin_amdgcn_s_barrier();
            --inflight;
            const bool doreq = nx_valid;
            if (doreq) {
                issue_chunk();
                ++inflight;
            }
            const unsigned sb = lds0 + (unsigned)(rd_stage * GSTAGE);
            rd_stage = rd_stage + 1 == GNS ? 0 : rd_stage + 1;
            // four groups of four contraction pairs; the operands of group g+1 are read while group g multiplies
            // (the registers an asm read returns must not be touched before the wait that is tied to them: no copies).
            {
            v4f a4[2];                         // !AT: four consecutive contraction values of the row
            float a1[2][4];                    // AT: one value per read
            float bq[2][4][4];
            auto read_group = [&](auto mmc, v4f& av4, float (&av)[4], float (&bv)[4][4]) {
                constexpr int mm = decltype(mmc)::value;
                if (!AT) {
                    const unsigned addr = sb + rdA[mm];
                    asm volatile("ds_read_b128 %0, %1" : "=v"(av4) : "v"(addr));
                } else {
                    static_for<0, 4>([&](auto cc) {
                        constexpr int comp = decltype(cc)::value;
                        float& dst = av[comp];                       // (asm operands alone do not capture)
                        const unsigned addr = sb + rdAT;
                        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"((4 * mm + comp) * (GM * 4)));
                    });
                }
                static_for<0, 4>([&](auto cc) {
                    constexpr int comp = decltype(cc)::value;
                    static_for<0, NW>([&](auto tc) {
                        constexpr int t = decltype(tc)::value;
                        float& dst = bv[comp][t];
                        const unsigned addr = sb + rdB;
                        asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"((4 * mm + comp) * (D * 4) + t * 128));
                    });
                });
            };
            auto wait_group = [&](v4f& av4, float (&av)[4], float (&bv)[4][4]) {
                if (!AT) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av4));
                else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3]));
#pragma unroll
                for (int comp = 0; comp < 4; ++comp)
#pragma unroll
                    for (int t = 0; t < NW; ++t) asm volatile("" : "+v"(bv[comp][t]));
            };
            auto mul_group = [&](const v4f& av4, const float (&av)[4], const float (&bv)[4][4]) __attribute__((always_inline)) {
                static_for<0, 4>([&](auto cc) __attribute__((always_inline)) {
                    constexpr int comp = decltype(cc)::value;
#pragma unroll
                    for (int t = 0; t < NW; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(AT ? av[comp] : av4[comp], bv[comp][t], acc[t], 0, 0, 0);
                });
                if (!AT && want_rs) rs += (av4[0] + av4[1]) + (av4[2] + av4[3]);
            };
            read_group(std::integral_constant<int, 0>{}, a4[0], a1[0], bq[0]);
            wait_group(a4[0], a1[0], bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            read_group(std::integral_constant<int, 1>{}, a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            mul_group(a4[0], a1[0], bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            wait_group(a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            read_group(std::integral_constant<int, 2>{}, a4[0], a1[0], bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            mul_group(a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            wait_group(a4[0], a1[0], bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            read_group(std::integral_constant<int, 3>{}, a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            mul_group(a4[0], a1[0], bq[0]);
            __builtin_amdgcn_sched_barrier(0);
            wait_group(a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            mul_group(a4[1], a1[1], bq[1]);
            __builtin_amdgcn_sched_barrier(0);
            }
        }
        // ---- the item's 128 x D block (C/D layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) ----
        {
            float* ob = out + (size_t)c * T * ldout;
#pragma unroll
            for (int t = 0; t < NW; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mi * GM + 32 * wm + (r & 3) + 8 * (r >> 2) + 4 * half;
                    if (m < T) ob[(size_t)m * ldout + 32 * NW * wn + 32 * t + l31] = acc[t][r];
                    acc[t][r] = 0.0f;
                }
            if (!AT && want_rs) {
                const float tot = rs + __shfl_xor(rs, 32);
                const int m = mi * GM + 32 * wm + l31;
                if (wn == 0 && half == 0 && m < T) rsum[((size_t)c * T + m) * ldrs] = tot;
                rs = 0.0f;
            }
        }
        cur_n += gridDim.x;
    }
}

template <bool AT, int NW>
static void launch_gemm(const float* Gt, int Tp, const float* other, long long ldo, float* out, long long ldout, int C,
                        int T, hipStream_t stream, float* rsum = nullptr, long long ldrs = 1)
{
    const size_t lds = (size_t)GNS * (GA_BYTES + GK * 64 * NW * 4);
    static PerDeviceOnce attr_once;
    if (attr_once.first()) {
        (void)hipFuncSetAttribute((const void*)score_bwd_gemm_kernel<AT, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    const int grid = persistent_grid(device_ncu(), 1, (long long)((T + GM - 1) / GM) * C);      // one workgroup per CU, at most one per item
    hipLaunchKernelGGL((score_bwd_gemm_kernel<AT, NW>), dim3(grid), dim3(512), lds, stream, Gt, Tp, other, ldo, out, ldout, C, T,
                       AT ? nullptr : rsum, ldrs);
}

}  // namespace semicrf
