#pragma once
// persist_grad.h -- the gradient sweep's extra roles in the panel workgroups of the persistent sweep (persist.hip): zero_role
// (the exact zeros of the dense gradient's upper triangle) and band_role (the band's marginals).  Each is described at its section.
#include "persist_common.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// ZERO role (GRAD): the dense gradient's upper triangle (begin > end) is exact zeros.  Spare waves of the panel
// workgroups write it while the sweep runs (row e: columns e+1..T-1, contiguous over all chains); rows are handed
// out in pairs (e, T-2-e) of equal total length.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void zero_row(float* __restrict__ dScore, int e, int T, int B, int lane)
{
    const size_t n = (size_t)(T - 1 - e) * B;                 // floats to clear in this row
    float* rowp = dScore + ((size_t)e * T + e + 1) * B;
    const size_t lead = (4 - (((uintptr_t)rowp >> 2) & 3)) & 3;          // floats up to 16-byte alignment
    const size_t head = lead < n ? lead : n;
    const size_t n4 = (n - head) / 4;
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    f32x4* v = (f32x4*)(rowp + head);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = lane; i < n4; i += 64) __builtin_nontemporal_store(z, v + i);
    if ((size_t)lane < head) rowp[lane] = 0.f;
    const size_t tail0 = head + n4 * 4;
    if (tail0 + lane < n) rowp[tail0 + lane] = 0.f;
}
__device__ __forceinline__ void zero_role(const SweepParams& P)
{
    const int T = P.T, B = P.B;
    float* const dScore = P.dScore;
    unsigned* const ctrl = P.ctrl;
    const int lane = threadIdx.x & 63;
    const int npairs = T / 2;                                  // rows 0 .. T-2 in pairs (e, T-2-e)
    while (true) {
        int p = 0;
        if (lane == 0) p = (int)(atomicAdd(ctrl + 3, 1u) + 1u);
        p = __builtin_amdgcn_readfirstlane(p);
        if (p >= npairs) break;
        const int e2 = T - 2 - p;
        if (p <= e2) zero_row(dScore, p, T, B, lane);
        if (p < e2) zero_row(dScore, e2, T, B, lane);
    }
}

// ---------------------------------------------------------------------------------------------
// BAND role (GRAD): the marginals of the band, written by spare waves of the panel workgroups
// ---------------------------------------------------------------------------------------------
// Until round 5 the ring waves stored the marginals of the cells they read themselves (the band: the diagonal tile and the
// FAR0 - 1 tiles left of it) -- one 4-byte store per lane and cell, 64 store instructions per block in the middle of the
// dependent chain, every one a 16-byte piece of 16 different lines: the ring of the gradient sweep needed 3.1 us per block where
// the forward ring needs 1.4, and the whole head of the sweep ran at that pace (T=1024 x 352: 357 us with, 295 us without
// those stores).  The band's marginals need nothing the ring has not published: marginal(pi, pj) = gz exp2(u[pj] + cell log2e +
// arow[pi]) -- the same expression, bit for bit, the panels evaluate for the far field.  So they are a task of their own:
// (column block m, row block k = m + dk, 32-chain group g, row quarter q4), ready as soon as the ring has published block m,
// handed out in m order to `bandWaves` otherwise idle waves of every panel workgroup.  A wave reads the tile's cells once more
// (+12 % reads: 4 rows x 16 columns x 128 bytes, register loads in 512-byte runs), its 16 x 4 u values and writes whole lines.
// Nobody waits for these waves: the ring's only global stores are u, the diagonal and the noise gradient.
constexpr int CTRL_BANDQ = 32;        // [32]: band task queue head (a line of its own)

template <int DIR>
__device__ __forceinline__ void band_role(const SweepParams& P)
{
    const int T = P.T, B = P.B, K = P.K, c0 = P.c0, c1 = P.c1;
    const size_t Bs = (size_t)B;
    unsigned* const ctrl = P.ctrl;
    const float* __restrict__ score = P.score;
    float* const dScore = P.dScore;
    const int* __restrict__ ptab = P.ptab;
    const int lane = threadIdx.x & 63;
    const int q8 = lane & 7, pjsub = (lane >> 3) & 1, pisub = lane >> 4;
    const int nG = P.nPanelGroups;
    const int nTasks = K * FAR0 * nG * 4;
    const size_t last4 = (size_t)T * T * Bs - 4;
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc((void*)P.ug, 0, (int)((size_t)T * Bs * 4), 0x00020000);
    const bool grad_nt = __builtin_amdgcn_readfirstlane(P.gradNT) != 0;
    while (true) {
        int task = 0;
        if (lane == 0) task = (int)(atomicAdd(ctrl + CTRL_BANDQ, 1u) + 1u);
        task = __builtin_amdgcn_readfirstlane(task);
        if (task >= nTasks) break;
        const int q4 = task & 3, t2 = task >> 2;
        const int g = t2 % nG, t3 = t2 / nG;
        const int dk = t3 % FAR0, m = t3 / FAR0, k = m + dk;
        const int pbase = k * PB + q4 * 4;
        if (k >= K || pbase >= T) continue;
        const int pi = pbase + pisub;
        const bool rowok = pi < T;
        const int pic = rowok ? pi : T - 1;
        const int c = c0 + g * GP + q8 * 4;
        const int cl = c < c1 ? c : c0;
        const bool v0 = c < c1, v1 = c + 1 < c1, v2 = c + 2 < c1, v3 = c + 3 < c1;
        float gz[4], ar[4];
        // the path table (DIR 1: a row is a begin frame): the column position of the path interval that begins in this lane's row, per
        // chain (-1: none, or no table), and what its cell gets on top of the marginal
        float gp[4];
        int pjp[4];
        {
            const int fr = frame_of<DIR>(pic, T);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = c + i < c1;
                const float lz = ok ? P.logZ[c + i] : 0.f;
                const float go = ok ? P.gout[(size_t)(c + i) * P.gstride] : 0.f;
                gz[i] = ok ? go * P.gscale : 0.f;
                ar[i] = ok ? (P.vfwd[(size_t)fr * Bs + c + i] - lz) * LOG2E : 0.f;
                const int pend = (DIR == 1 && ok && rowok && ptab) ? (ptab[(size_t)fr * Bs + c + i] & PTAB_NONE) : PTAB_NONE;
                pjp[i] = pend != PTAB_NONE ? T - 1 - pend : -1;
                gp[i] = P.noiseAdd * go;
            }
        }
        v4u x[8], uu[8];
        size_t off[8];                                               // element offset of the cell (loads: clamped into the tensor)
        unsigned uoff[8];
        bool use[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int pj = m * PB + 2 * e + pjsub;
            use[e] = rowok && pj < pi;
            const int pjc = pj < pic ? pj : (pic > 0 ? pic - 1 : 0);       // the diagonal tile: cells at and above the diagonal are not used
            off[e] = cell_index<DIR>(pic, pjc, T) * Bs + cl;
            uoff[e] = (unsigned)(((size_t)pjc * Bs + cl) * 4);
            const v4u_a4 t = *(const v4u_a4*)(score + (off[e] < last4 ? off[e] : last4));
            x[e] = t;
            uu[e] = __builtin_amdgcn_raw_buffer_load_b128(ursrc, uoff[e], 0, 0);
        }
        // u not published yet (or a stale line of the launch's start): again with device scope until the ring is there
        {
            int spins = 0;
            while (true) {
                bool ok = true;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    ok = ok && (uu[e].x != U_EMPTY || !v0) && (uu[e].y != U_EMPTY || !v1) && (uu[e].z != U_EMPTY || !v2) && (uu[e].w != U_EMPTY || !v3);
                if (__all(ok)) break;
                __builtin_amdgcn_s_sleep(64);
                if (spin_abort(ctrl, spins, SPIN_LIMIT, 14)) break;
#pragma unroll
                for (int e = 0; e < 8; ++e) uu[e] = __builtin_amdgcn_raw_buffer_load_b128(ursrc, uoff[e], 0, 16);     // 16 = sc1
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (!use[e] || !v0) continue;
            v4u gv;
            gv.x = __float_as_uint(gz[0] * fexp2(fmaf(__uint_as_float(x[e].x), LOG2E, __uint_as_float(uu[e].x)) + ar[0]));
            gv.y = __float_as_uint(gz[1] * fexp2(fmaf(__uint_as_float(x[e].y), LOG2E, __uint_as_float(uu[e].y)) + ar[1]));
            gv.z = __float_as_uint(gz[2] * fexp2(fmaf(__uint_as_float(x[e].z), LOG2E, __uint_as_float(uu[e].z)) + ar[2]));
            gv.w = __float_as_uint(gz[3] * fexp2(fmaf(__uint_as_float(x[e].w), LOG2E, __uint_as_float(uu[e].w)) + ar[3]));
            {
                // the cell of a path interval: marginal + noiseAdd * gout, rounded once -- what the scatter's atomicAdd left
                const int pj = m * PB + 2 * e + pjsub;
                if (pj == pjp[0]) gv.x = __float_as_uint(__uint_as_float(gv.x) + gp[0]);
                if (pj == pjp[1]) gv.y = __float_as_uint(__uint_as_float(gv.y) + gp[1]);
                if (pj == pjp[2]) gv.z = __float_as_uint(__uint_as_float(gv.z) + gp[2]);
                if (pj == pjp[3]) gv.w = __float_as_uint(__uint_as_float(gv.w) + gp[3]);
            }
            float* const dst = dScore + off[e];
            if (v3) {
                const v4u_a4 ga = gv;
                if (grad_nt) __builtin_nontemporal_store(ga, (v4u_a4*)dst);
                else *(v4u_a4*)dst = ga;
            }
            else {                                                   // ragged tail of the chain range
                dst[0] = __uint_as_float(gv.x);
                if (v1) dst[1] = __uint_as_float(gv.y);
                if (v2) dst[2] = __uint_as_float(gv.z);
            }
        }
    }
}

}  // namespace semicrf
