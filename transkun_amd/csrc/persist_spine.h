#pragma once
// persist_spine.h -- the SPINE workgroup of the persistent sweep (persist.hip): loader, far and ring roles.
//
// SPINE workgroup, one per 4 chains: a ring of four waves, wave w owns position blocks k = w, w+4, ...; a lane is (row r of the
// block, ONE chain).  Every wave applies each newly finished u[j] to its own block's rows (band = the current block and the next
// three); the owner of the current block finalises one position per step and publishes it through LDS to its ring mates; once per
// block it publishes 16 positions to HBM for the panels.  The T-step dependent chain never leaves one CU.  A lone wave issues one
// plain instruction per ~4.5 cycles and one transcendental per ~16, so the step is kept at ~24 instructions with 4
// transcendentals.  The ring waves never wait for memory: a LOADER wave stages the band cells in LDS with asynchronous
// global->LDS loads several blocks ahead, and a FAR wave collects the panels' partial results into LDS.
#include "persist_common.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// SPINE workgroup: ring waves + loader wave + far-partial wave
// ---------------------------------------------------------------------------------------------
// The ring waves never issue a global LOAD: vector-memory results return in order, so one request queued
// behind a burst of HBM misses (several microseconds while the panels stream) would stall the dependent chain.
//   * the LOADER wave copies the band cells of row block kr -- four 16x16x4-chain tiles -- and its per-row
//     constants into LDS with asynchronous global->LDS loads, running up to NRBUF row blocks ahead of the ring;
//   * the FAR wave polls the panels' partials for the upcoming blocks (its polls are the only requests it has
//     in flight, so they see L2 latency) and leaves one combined value per (row, chain) in LDS;
//   * a ring wave reads its four tiles from LDS into registers at the start of its iteration.
// LDS ring: 128 positions x 4 chains x 8 bytes {u, seq = position+1}.  A position is published with ONE
// 8-byte DS write per lane by the four lanes r == 0 of the owning wave (after the broadcast every lane holds
// u[j] of its chain); consumers read their chain's 8 bytes and check seq.
//
// The step bodies are written for a lone wave (issue-bound):
//   * the diagonal step needs no lane predicates: the broadcast value is what gets published and the
//     next broadcast simply reads the lanes of the next row,
//   * row jj+1 receives its last term through logaddexp2(Vp, u + W) where Vp (everything but that term)
//     is refreshed one step ahead by the (M,S) push that runs beside it.
constexpr int NRBUF = SEMICRF_NRBUF;                  // row-block buffers between the loader and the ring
constexpr int TILE_BYTES = PB * PB * RS * 4;          // 4096: [column u][row r][chain] floats
constexpr int NCONST = 4;                             // per-row constants: diagonal cell, noise, alpha (GRAD), path table word (GRAD)
constexpr int LDS_TILES = 0;
constexpr int LDS_CONST = LDS_TILES + NRBUF * RING * TILE_BYTES;       // [NRBUF][NCONST][64] floats
constexpr int LDS_FAR = LDS_CONST + NRBUF * NCONST * 256;              // [8][64] x {value, key, seq, pad}
constexpr int NFAR = 8;                               // far-partial entries (blocks) between the far wave and the ring (>= RING)
constexpr int NPOS = 128;                             // positions kept in the LDS ring (>= the band, RING blocks)
static_assert(NFAR >= RING && NPOS >= RING * PB, "ring geometry");
constexpr int LDS_RING = LDS_FAR + NFAR * 64 * 16;                     // [NPOS][RS] x {u, seq}
// Far waves per spine workgroup: far wave f takes the blocks k = RING + f, RING + f + NFARW, ...  One far wave needs a device-scope
// round trip per block even when the partial has long been stored (issue the poll, wait for it: ~2 us behind the loader's
// traffic in the same compute unit) -- the block period of every hand-off-bound shape sat exactly there (2.1 - 2.2 us at 88
// chains); two of them take turns.
constexpr int NFARW = SEMICRF_NFARW;
constexpr int LDS_CTL = LDS_RING + NPOS * RS * 8;                      // ready[NRBUF], cons[RING] (ints)
// (reserved: the rest of the 256 bytes -- counters of a retired alternative lived there; LDS_DUMMY keeps its offset)
static_assert(NRBUF + RING <= 64, "control words");
constexpr int LDS_DUMMY = LDS_CTL + 256;                               // sink of the non-writer lanes' ring stores
constexpr int LDS_SPINE_BYTES = LDS_DUMMY + (64 * 2 + PB * 8) * 4;

struct SpineBlk { float v[PB]; };

// lane -> (row of the block, chain of the ring) in the spine workgroup's ring, far and loader-constant code: a chain's 16 rows
// are one DPP row (lanes 16 ch .. 16 ch + 15), so that "row j of my chain" is a row_newbcast operand
__device__ __forceinline__ int spine_row(int lane) { return lane & 15; }
__device__ __forceinline__ int spine_chain(int lane) { return lane >> 4; }


// ---- loader wave ---------------------------------------------------------------------------------------
template <int DIR, bool GRAD>
__device__ __forceinline__ void loader_role(const SweepParams& P, int sg, char* lds)
{
    const int T = P.T, B = P.B, K = P.K;
    unsigned* const ctrl = P.ctrl;
    const size_t Bs = (size_t)B;
    const float* const score = P.score;
    const float* const noise = P.noise;
    const float* const vfwd = P.vfwd;
    const float* const tabw = P.ptab ? (const float*)P.ptab : P.vfwd;
    const int lane = threadIdx.x & 63;
    const int cbase = P.c0 + sg * GS;
    const size_t last4 = (size_t)T * T * Bs - 4;                 // last element offset a 16-byte load may start at
    // tile loads: instruction q covers columns 4q..4q+3, lane = (column within the group, row)
    const int tu = lane >> 4, tr = lane & 15;
    // constants: lane = (row, chain) like the ring waves
    const int cr = spine_row(lane), cch = spine_chain(lane);
    const int cc = cbase + cch < P.c1 ? cbase + cch : cbase;
    int* const ready = (int*)(lds + LDS_CTL);
    int* const cons = ready + NRBUF;
    constexpr int NL = RING * 4 + 2 + (GRAD ? 2 : 0);   // loads per row block (exactly, the waits count them)
    constexpr int LDEPTH = 3 * NL <= 63 ? 3 : 2;
    static_assert(2 * NL <= 63, "loader pipeline");

    const bool useband = SEMICRF_BANDX && P.band != nullptr;
    const float* const bandp = useband ? P.band + (size_t)(cbase / GS) * RING * (TILE_BYTES / 4) + lane * 4 : nullptr;
    const size_t band_kr = (size_t)P.bandSpines * RING * (TILE_BYTES / 4);
    // The copy's hand-off: RING words per (32-chain group, row block), each {launch tag, row block} once its tile is in place.  The
    // loader looks at them with a SCALAR load (its own counter: the vector-memory counter of this wave counts LDS-DMA pieces exactly)
    // that takes two row blocks at once, request and wait in ONE asm statement: the compiler believes an asm's outputs are there when
    // the statement ends -- a first version requested a row block ahead and waited later, and the compiler copied the registers in
    // between and reused them while the load was still on its way (a memory aperture violation a microsecond later).
    typedef unsigned v16u __attribute__((ext_vector_type(16)));
    const int bKpad = K + 2;
    const unsigned* const bflags = useband ? P.bandFlags + (size_t)(cbase / GP) * bKpad * 8 : nullptr;
    const unsigned btag = P.tag;
    int ready_upto = -1;                       // row blocks <= ready_upto are known to be copied
    auto band_ready = [&](int kr) -> bool {
        const uintptr_t fa = (uintptr_t)(bflags + (size_t)kr * 8);                 // wave-uniform by construction; said explicitly for the "s" operand
        const u64 fp = (u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)fa) |
                       ((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(fa >> 32)) << 32);
        v16u f;
        asm volatile("s_load_dwordx16 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=&s"(f) : "s"(fp) : "memory");
        // (a flag word is {launch tag, row block}: neither the fill nor a previous launch's words can pass for this row block's)
        const unsigned want0 = ((btag & 0xffffu) << 16) | (unsigned)kr, want1 = want0 + 1u;
        bool ok0 = true, ok1 = true;
#pragma unroll
        for (int i = 0; i < RING; ++i) { ok0 = ok0 && f[i] == want0; ok1 = ok1 && f[8 + i] == want1; }
        if (ok0) ready_upto = ok1 ? kr + 1 : kr;
        return ok0;
    };
    auto issue = [&](int kr) {
        const int slot = kr % NRBUF;
        const int prow_t = kr * PB + tr < T ? kr * PB + tr : T - 1;
        const bool fromband = useband && kr >= P.bandK0;
        if (fromband) {
            const float* const bk = bandp + (size_t)kr * band_kr;
#pragma unroll
            for (int i = 0; i < RING; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    __builtin_amdgcn_global_load_lds((gbl_void_t*)(bk + i * (TILE_BYTES / 4) + q * 256),
                                                     (lds_void_t*)(lds + LDS_TILES + (slot * RING + i) * TILE_BYTES + q * 1024), 16, 0, SEMICRF_BAND_LOAD_AUX);   // sc1: written by another CU in this launch
        } else
#pragma unroll
        for (int i = 0; i < RING; ++i) {
            const int kc = kr - (RING - 1) + i > 0 ? kr - (RING - 1) + i : 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                int pj = kc * PB + 4 * q + tu;
                pj = pj < prow_t ? pj : (prow_t > 0 ? prow_t - 1 : 0);       // only cells below the diagonal are used
                size_t off = cell_index<DIR>(prow_t, pj, T) * Bs + cbase;
                off = off < last4 ? off : last4;
                __builtin_amdgcn_global_load_lds((gbl_void_t*)(score + off),
                                                 (lds_void_t*)(lds + LDS_TILES + (slot * RING + i) * TILE_BYTES + q * 1024), 16, 0, 0);
            }
        }
        const int prow_c = kr * PB + cr < T ? kr * PB + cr : T - 1;
        const int frow = frame_of<DIR>(prow_c, T);
        char* cb = lds + LDS_CONST + slot * NCONST * 256;
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(score + ((size_t)frow * T + frow) * Bs + cc), (lds_void_t*)cb, 4, 0, 0);
        __builtin_amdgcn_global_load_lds((gbl_void_t*)(noise + (size_t)gap_of<DIR>(prow_c >= 1 ? prow_c : 1, T) * Bs + cc),
                                         (lds_void_t*)(cb + 256), 4, 0, 0);
        if (GRAD) {
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(vfwd + (size_t)frow * Bs + cc), (lds_void_t*)(cb + 512), 4, 0, 0);
            // the path table's word of (frame, chain), indexed like alpha (no table: alpha once more -- the load count is fixed, the ring ignores it)
            __builtin_amdgcn_global_load_lds((gbl_void_t*)(tabw + (size_t)frow * Bs + cc), (lds_void_t*)(cb + 768), 4, 0, 0);
        }
    };
    auto publish = [&](int kr) {
        if (lane == 0) lds_flag_store_asm(ready + kr % NRBUF, kr + 1);
    };

    // the loader keeps LDEPTH row blocks in flight (the counter holds 63 operations)
    int prev2 = -1, prev1 = -1;                    // row blocks issued and not yet published (oldest first)
    for (int kr = 0; kr < K; ++kr) {
        if (kr >= NRBUF) {
            // the buffer's previous row block (kr - NRBUF) must have been read by its ring wave
            const int w = (kr - NRBUF) % RING;
            int spins = 0;
            while (lds_flag_load_asm(cons + w) < kr - NRBUF + 1) {
                __builtin_amdgcn_s_sleep(2);
                if (spin_abort(ctrl, spins, SPIN_LIMIT_LDS, 6)) return;
            }
        }
        if (useband && kr >= P.bandK0 && kr > ready_upto) {
            int spins = 0;
            while (!band_ready(kr)) {
                __builtin_amdgcn_s_sleep(8);
                if (spin_abort(ctrl, spins, SPIN_LIMIT, 16)) return;
                asm volatile("s_dcache_inv" ::: "memory");          // (a line of the scalar cache also holds the next row blocks' words: looked at too early, stale from then on)
            }
        }
        issue(kr);
        if (LDEPTH == 3) {
            if (prev2 >= 0) { wait_vmcnt<2 * NL>(); publish(prev2); }
            prev2 = prev1; prev1 = kr;
        } else {
            if (prev1 >= 0) { wait_vmcnt<NL>(); publish(prev1); }
            prev1 = kr;
        }
    }
    if (LDEPTH == 3 && prev2 >= 0) { wait_vmcnt<NL>(); publish(prev2); }
    wait_vmcnt<0>();
    if (prev1 >= 0) publish(prev1);
}

// ---- far wave -------------------------------------------------------------------------------------------
// Per block k >= RING, one combined value per (row, chain) for the owner's diagonal phase: the panels' partials of the far field
// (tiles 0 .. k-FAR0).
template <int MODE>
__device__ __forceinline__ void far_role(const SweepParams& P, int sg, char* lds, int fw)
{
    const int T = P.T, B = P.B, K = P.K;
    unsigned* const ctrl = P.ctrl;
    const u64* const farg = P.farg;
    const unsigned tag = P.tag;
    const size_t Bs = (size_t)B;
    const int lane = threadIdx.x & 63;
    const int r = spine_row(lane), ch = spine_chain(lane);
    const int c = P.c0 + sg * GS + ch;
    const bool cvalid = c < P.c1;
    float4* const far = (float4*)(lds + LDS_FAR);
    const bool cbase_is_first = sg == 0;
    __builtin_amdgcn_s_setprio(0);     // below the ring's shadow phase (1) and its diagonal phase (3)
    const bool fprobe = SEMICRF_PANEL_PROBES && (DBGF(P) & 16u) && cbase_is_first && lane == 0;
    // (NFARW far waves exist; a launch uses the first P.nfarw of them: SweepParams::nfarw)
    const int nfar = __builtin_amdgcn_readfirstlane(P.nfarw);
    if (fw >= nfar) return;
    for (int k = RING + fw; k < K; k += nfar) {
        if (fprobe && k < 64) P.ts[640 + k] = __builtin_amdgcn_s_memrealtime();
        const int prow = k * PB + r;
        const bool rvalid = cvalid && prow < T;
        float aM = SEMICRF_NEG_INF, aS = 0.f;
        int aK = 0x7fffffff;
        // parts of block k: the panels' column parts of its far tiles 0 .. k-FAR0
        const int nparts = k >= FAR0 ? nparts_of(k - FAR0) : 0;
        // (two stamps of the trace's layout, tools/chain_trace.py: nothing lies between them any more)
        if (fprobe && k < 64) P.ts[704 + k] = __builtin_amdgcn_s_memrealtime();
        if (fprobe && k < 64) P.ts[832 + k] = __builtin_amdgcn_s_memrealtime();
        if (rvalid && nparts > 0) {
            // all parts are requested together (they complete in any order); the poll repeats for the missing ones.  A request
            // is a device-scope round trip of ~2 us from this compute unit -- behind the loader's traffic -- whether or not the
            // partial has long been stored.
            for (int p0 = 0; p0 < nparts; p0 += 4) {
                const int np = nparts - p0 < 4 ? nparts - p0 : 4;
                u64 gq[4];
                bool have[4] = {false, false, false, false};
                int spins = 0;
                while (true) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < np && !have[i]) gq[i] = load_granule(farg + ((size_t)(p0 + i) * T + prow) * Bs + c);
                    bool all = true;
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (i < np && !have[i]) {
                            const bool ok = MODE == 0 ? (unsigned)(gq[i] >> 32) == tag : (unsigned)(gq[i] >> 48) == (tag & 0xffffu);
                            if (ok) have[i] = true;          // gq[i] keeps the granule: it is not requested again
                            else all = false;
                        }
                    if (all) break;
                    __builtin_amdgcn_s_sleep(1);
                    if (spin_abort(ctrl, spins, SPIN_LIMIT, 3)) break;
                }
                // the parts are merged in index order, not in the order they arrived in: the sum's last bit (and a tie
                // between two maxima) must not depend on timing
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < np && have[i]) {
                        if (MODE == 0) acc_push1(aM, aS, __uint_as_float((unsigned)gq[i]));
                        else max_push(aM, aK, __uint_as_float((unsigned)gq[i]), (int)((gq[i] >> 32) & 0xffffu));
                    }
            }
        }
        if (fprobe && k < 64) P.ts[896 + k] = __builtin_amdgcn_s_memrealtime();
        // (LSE: an empty accumulator -- rows past the end, ghost chains -- gives -inf + log2(0) = NaN, which nobody reads)
        const float val = MODE == 0 ? aM + flog2(aS) : aM;
        lds_store128(far + (k % NFAR) * 64 + lane, make_float4(val, __int_as_float(aK), __int_as_float(k + 1), 0.0f));   // one DS write: data + seq
        if (SEMICRF_PANEL_PROBES && (DBGF(P) & 16u) && cbase_is_first && lane == 0) P.ts[128 + k] = __builtin_amdgcn_s_memrealtime();   // chain probe
    }
}

// ---- ring waves -----------------------------------------------------------------------------------------
// The diagonal phase of the LSE sweeps (round 3).  Rows p = own0 .. own0+15 of the owner's block satisfy
//     y[r] = log2( 2^V[r] + sum_{j<r} 2^(y[j] + d[r][j]) ),   u[r] = y[r] + sp[r],
// V[r] = everything outside the block (shadow pushes + far partial, known when the phase starts), d[r][j] = log2 cell
// (r, j) + sp[j] (for j = r-1 the cell with the skip folded in, `wl`).  Walked in the log domain this is 16 dependent
// logaddexp steps of ~240 cycles each for a lone wave (two transcendentals and a cross-lane broadcast per step): 1.6 us per
// block, the pace of the whole head of the sweep.  Now:
//   1. a (max,+) pass over the block gives every row an exponent e[r] = max(Vmax[r], max_j e[j] + d[r][j]): the weight of the
//      best single path into row r, so y[r] - e[r] lies in [0, 16 log2 17];
//   2. with Y[r] = 2^(y[r] - e[r]) the recurrence is LINEAR with coefficients m[r][j] = 2^(e[j] + d[r][j] - e[r]) <= 1
//      (sixteen independent exponentials per lane): Y[r] = a[r] + sum_j Y[j] m[r][j], a[r] = S[r] 2^(Vmax[r] - e[r]) <= #terms;
//      nothing can overflow, what underflows is below 2^-24 of a term of size >= 1;
//   3. y[r] = e[r] + log2 Y[r].
// Both passes are 15 steps of TWO dependent vector instructions: a lane is (row r, chain) with the chain's 16 rows in one DPP
// row, so "the value of row j" is a row_newbcast operand (v_add_f32_dpp / v_mov_b32_dpp), no LDS round trip.
// tools/dpp_probe.hip measures the chains on their own.  The (max,+) sweeps keep their stepwise form (one add and one
// compare per step, bit-exact candidates).

template <int J>
__device__ __forceinline__ float row_bcast(float x)       // lane J of this lane's DPP row: row J of the block, same chain
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x150 + J, 0xf, 0xf, false));
}
template <int J, int N, typename F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (J < N) { f(IC<J>{}); static_for<J + 1, N>(f); }
}

template <int MODE, int DIR, bool GRAD, bool RINGBAND>
__device__ __forceinline__ void spine_role(const SweepParams& P, int sg, int ring_pos, char* lds)
{
    // kernel arguments are copied into locals: lambdas that capture the struct by reference make the
    // compiler spill it to scratch and reload fields inside the step loops
    const int T = P.T, B = P.B, K = P.K;
    const unsigned dbg = DBGF(P);
    unsigned* const ctrl = P.ctrl;
    u64* const ts = P.ts;
    unsigned* const ug = P.ug;
    float* const u_out = P.u_out;
    float* const last_out = P.last_out;
    int* const code = P.code;
    float* const dScore = P.dScore;
    float* const dNoise = P.dNoise;
    const u64* const pathg = P.pathg;
    float* const pathOut = P.pathOut;
    const unsigned ptag = P.tag;
    const int rw = __builtin_amdgcn_readfirstlane(ring_pos);                // position of the wave in the ring
    const int lane = threadIdx.x & 63;
    const int r = spine_row(lane), ch = spine_chain(lane);
    const int c = P.c0 + sg * GS + ch;
    const bool cvalid = c < P.c1;
    const int cc = cvalid ? c : P.c0;
    const size_t Bs = (size_t)B;
    const bool trace = (dbg & 16u) && sg == 0 && lane == 0;
    float* const ring = (float*)(lds + LDS_RING);
    const float* rd_base = ring + ch * 2;                                   // + (j % NPOS) * 8 floats
    const int* const ready = (const int*)(lds + LDS_CTL);
    int* const cons = (int*)(lds + LDS_CTL) + NRBUF;
    const float4* const far = (const float4*)(lds + LDS_FAR);
    float gz = 0.f, lzc = 0.f;
    float nadd = 0.f;     // logProb's backward: + gout on every gap (the path score's cum[T-1] term; the product, then the sum: two
                          // roundings, exactly what a separate `dNoise += gout` pass over the stored marginal gave)
                          // With the path table the same weight goes onto the path's own terms: + on the diagonal cell of a one-frame
                          // interval, - on a covered gap.
    const bool fold = GRAD && P.ptab != nullptr;
    if (GRAD && cvalid) {                                                                                 // the only global loads of a ring wave
        const float go = P.gout[(size_t)c * P.gstride];
        gz = go * P.gscale; lzc = P.logZ[c]; nadd = P.noiseAdd * go;
    }
    // GRAD: who stores the marginals of the band (the cells the ring itself reads)?  The panel workgroups' band waves when the
    // launch has them (band_role: whole lines, off the ring's critical path); the ring waves themselves otherwise (short sequences)
    // (a template parameter: as a run-time flag it put a branch around every cell's store and cut the shadow batch into 16 pieces)
    constexpr int ringBand = GRAD && RINGBAND ? 1 : 0;
    __builtin_amdgcn_s_setprio(1);

    for (int k = rw; k < K; k += RING) {
        u64* ev = ts + T + (size_t)k * 8;          // debug events of this block (8 slots)
        if (trace) ev[0] = __builtin_readcyclecounter();
        const int prow = k * PB + r;
        const bool rvalid = cvalid && prow < T;
        const int prow_c = prow < T ? prow : T - 1;
        const int frow = frame_of<DIR>(prow_c, T);
        const int own0 = k * PB;
        const int slot = k % NRBUF;

        // ---- the row block's cells and constants, staged in LDS by the loader wave ----------------
        {
            int spins = 0;
            while (lds_flag_load(ready + slot) != k + 1) {
                __builtin_amdgcn_s_sleep(1);
                if (spin_abort(ctrl, spins, SPIN_LIMIT_LDS, 7)) break;
            }
        }
        const char* tb = lds + LDS_TILES + slot * RING * TILE_BYTES + (r * RS + ch) * 4;
        auto read_tile = [&](int i) -> SpineBlk {
            SpineBlk o;
#pragma unroll
            for (int u = 0; u < PB; ++u) o.v[u] = *(const float*)(tb + i * TILE_BYTES + u * (PB * RS * 4));
            return o;
        };
        SpineBlk X[RING];        // X[i]: columns of block k - (RING-1) + i (the last one is the own block)
#pragma unroll
        for (int i = 0; i < RING; ++i) X[i] = read_tile(i);
        const float* cst = (const float*)(lds + LDS_CONST + slot * NCONST * 256) + lane;
        const float dcell = cst[0], nzl = cst[64], vfl = cst[128];
        // the path table's word of this lane's frame (pathscore.h): does a one-frame interval sit on the diagonal cell, is the gap
        // behind the frame -- the gap this lane stores in DIR 1 -- covered?
        const int pte = fold ? __float_as_int(cst[192]) : PTAB_NONE;
        const bool pdiag = (pte & PTAB_NONE) == frow, pgap = (pte & PTAB_COVERED) != 0;
        // first sub-diagonal cell of this lane's row: column r-1 of the own tile (last column of the previous tile for row 0)
        const float s1own = *(const float*)(lds + LDS_TILES + (slot * RING + RING - 1) * TILE_BYTES +
                                            ((((r > 0 ? r - 1 : 0) * PB) + r) * RS + ch) * 4);
        const float s1 = r == 0 ? X[RING - 2].v[PB - 1] : s1own;
        if (lane == 0) lds_flag_store(cons + rw, k + 1);          // in-order DS queue: after the reads above

        // GRAD stores: wave-uniform base (SGPR) + one per-lane byte offset
        //   DIR 0: cell(prow, j) = ((own0 + r)*T + j)*B          DIR 1: cell(prow, j) = ((T-1-j)*T + (T-1-prow))*B
        const unsigned bvoff = DIR == 0 ? (unsigned)(((size_t)(prow_c - own0) * T * Bs + cc) * 4)
                                        : (unsigned)(((size_t)(T - 1 - prow_c) * Bs + cc) * 4);
        auto col_off = [&](int j) -> size_t {
            return DIR == 0 ? ((size_t)own0 * T + (size_t)j) * Bs : (size_t)(T - 1 - j) * T * Bs;
        };
        auto grad_store = [&](int j, float v) {
            const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(dScore + col_off(j)), 0, 0x7fffffff, 0x00020000);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, bvoff, 0, 0);
        };

        // ---- per-row constants ----------------------------------------------------------------
        float sp = 0.f;   // LSE: softplus2(diag); MAX: diag
        float nz = 0.f;   // noise between prow-1 and prow
        float wl = 0.f;   // LSE: log2(2^s[prow][prow-1] + 2^n): first sub-diagonal cell with the skip folded in
        float draw = 0.f;
        if (rvalid) {
            draw = dcell * LOG2E;
            sp = MODE == 0 ? softplus2(dcell) : dcell;
            if (prow >= 1) {
                nz = nzl;
                if (MODE == 0) {
                    const float a0 = s1 * LOG2E, b0 = nz * LOG2E;
                    wl = fmaxf(a0, b0) + flog2(1.0f + fexp2(-fabsf(a0 - b0)));
                }
            }
        }
        // GRAD: marginal(prow, j) = gz * exp2(t + arow) with t = u[j] + cell*log2e, arow = (alpha[frame] - logZ)*log2e
        const float arow = (GRAD && rvalid) ? (vfl - lzc) * LOG2E : 0.f;
        // LSE: the block's own triangle as log2 coefficients d[j] = cell(r, j) + sp[j] (column r-1: the cell with the skip
        // folded in; columns >= r: none) -- known at the start of the iteration, long before the phase that needs them
        float d[PB - 1];
        if (MODE == 0) {
            static_for<0, PB - 1>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const float cj = r > j + 1 ? X[RING - 1].v[j] * LOG2E : (r == j + 1 ? wl : SEMICRF_NEG_INF);
                d[j] = (rvalid ? cj : SEMICRF_NEG_INF) + row_bcast<j>(sp);
            });
        }
        if (trace) ev[1] = __builtin_readcyclecounter();

        float aM = SEMICRF_NEG_INF, aS = 0.f;
        int aK = 0x7fffffff;

        // wait for positions j .. j+3 in the ring and return this lane's chain (one check per four positions: a wave that
        // lags behind its ring mate catches up at the cost of the pushes alone).  Every entry is ONE 8-byte word {u, seq},
        // written with one DS store and read with ONE 64-bit load (lds_load64: the compiler splits a plain float2 load into
        // separate loads of value and seq when they are used apart -- the value read BEFORE its seq is a torn read);
        // the LSE owner writes all 16 positions of a block with one instruction, so each entry's own seq is checked.
        auto ring_get4 = [&](int j, float (&uo)[4]) {
            const float* e = rd_base + (j % NPOS) * 8;                         // j % 4 == 0: no wrap inside the group
            u64 w0, w1, w2, w3;
            auto fetch = [&]() { w0 = lds_load64(e); w1 = lds_load64(e + 2 * RS); w2 = lds_load64(e + 4 * RS); w3 = lds_load64(e + 6 * RS); };
            auto ok = [&]() {
                return (int)(w0 >> 32) == j + 1 && (int)(w1 >> 32) == j + 2 && (int)(w2 >> 32) == j + 3 && (int)(w3 >> 32) == j + 4;
            };
            fetch();
            if (!__all(ok())) {
                int spins = 0;
                while (true) {
                    __builtin_amdgcn_s_sleep(1);
                    fetch();
                    if (__all(ok())) break;
                    if (spin_abort(ctrl, spins, SPIN_LIMIT_LDS, 2)) break;
                }
            }
            uo[0] = __uint_as_float((unsigned)w0); uo[1] = __uint_as_float((unsigned)w1);
            uo[2] = __uint_as_float((unsigned)w2); uo[3] = __uint_as_float((unsigned)w3);
        };

        // ---------------- shadow phase: apply a block published by a ring mate ---------------------
        // `last`: block k-1, whose final column own0-1 is the first sub-diagonal cell of row 0 (skip folded in)
        auto shadow = [&](const SpineBlk& X, int b, bool last) {
            if (trace && b >= k - 3) ev[3 + (b - (k - 3))] = __builtin_readcyclecounter();
            if (MODE == 0) {
                // log-sum-exp: the block's 16 terms in one batch -- all terms first, ONE exact maximum, then 16 independent
                // exponentials relative to it (a push per term costs a dependent compare / select chain each: 16 x ~45 cycles of
                // a lone wave; the `last` block's batch sits on the ring's critical path, between a mate's publish and the own
                // diagonal phase)
                float t[PB];
#pragma unroll
                for (int u4 = 0; u4 < PB; u4 += 4) {
                    float uq[4];
                    ring_get4(b * PB + u4, uq);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = u4 + q;
                        const int j = b * PB + u;
                        float p = fmaf(X.v[u], LOG2E, uq[q]);
                        if (GRAD && ringBand && rvalid && j < prow) grad_store(j, gz * fexp2(p + arow));
                        if (last && u == PB - 1 && r == 0) {
                            if (GRAD && rvalid) {     // noise marginal of the gap between prow-1 and prow
                                float nv = gz * fexp2(uq[q] + nz * LOG2E + arow) + nadd;
                                if (pgap) nv = nv - nadd;           // a covered gap: the scatter's atomicAdd(-gout), after the sum above
                                dNoise[(size_t)gap_of<DIR>(prow, T) * Bs + c] = nv;
                            }
                            p = uq[q] + wl;
                        }
                        t[u] = p;
                    }
                }
                float mx = aM;
#pragma unroll
                for (int u = 0; u < PB; u += 2) mx = fmaxf(mx, fmaxf(t[u], t[u + 1]));
                float sum = aS * fexp2(aM - mx);               // empty accumulator: 0 * exp2(-inf) = 0 (mx is finite: the terms are)
#pragma unroll
                for (int u = 0; u < PB; ++u) sum += fexp2(t[u] - mx);
                aM = mx; aS = sum;
            } else {
#pragma unroll
                for (int u4 = 0; u4 < PB; u4 += 4) {
                    float uq[4];
                    ring_get4(b * PB + u4, uq);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int u = u4 + q;
                        const int j = b * PB + u;
                        const float uv = uq[q];
                        const int key = frame_of<DIR>(j, T);
                        if (last && u == PB - 1 && r == 0) max_push_sel(aM, aK, uv + nz, -1);   // the skip candidate (key -1 wins every tie)
                        max_push_sel(aM, aK, uv + X.v[u], key);
                    }
                }
            }
        };

#pragma unroll
        for (int i = 0; i < RING - 1; ++i)
            if (k - (RING - 1) + i >= 0) shadow(X[i], k - (RING - 1) + i, i == RING - 2);

        // ---------------- diagonal phase: finalise the 16 positions of block k ------------------------
        __builtin_amdgcn_s_setprio(3);       // the dependent chain goes before everything else on this SIMD
        if (trace) ev[6] = __builtin_readcyclecounter();
        if (k >= RING && !(dbg & 1u)) {
            // combined far-field partial of this (row, chain), left in LDS by the far wave
            const float4* fe = far + (k % NFAR) * 64 + lane;
            float4 f = lds_load128(fe);                          // one 16-byte read: data and seq together
            if (!__all(__float_as_int(f.z) == k + 1)) {
                int spins = 0;
                while (true) {
                    __builtin_amdgcn_s_sleep(1);
                    f = lds_load128(fe);
                    if (__all(__float_as_int(f.z) == k + 1)) break;
                    if (spin_abort(ctrl, spins, SPIN_LIMIT_LDS, 8)) break;
                }
            }
            if (rvalid) {
                if (MODE == 0) acc_push1(aM, aS, f.x);
                else max_push_sel(aM, aK, f.x, __float_as_int(f.y));
            }
        }

        if (SEMICRF_PANEL_PROBES && trace) { ts[64 + k] = __builtin_amdgcn_s_memrealtime(); ev[2] = __builtin_readcyclecounter(); }   // chain probe: far partial in hand
        int mykey = -1;
        float mine = 0.f;                    // this lane's finished u (log2 units for LSE)
        if (MODE == 0) {
            // everything outside the block: S terms relative to their maximum mx (the first position has the empty path, weight 1;
            // rows past the end and ghost chains run on finite stand-ins, nobody reads them)
            float mx = aM, S = aS;
            if (prow == 0 || !rvalid) { mx = 0.0f; S = 1.0f; }
            // 1. exponents: the best single path into every row
            float e = mx;
            static_for<0, PB - 1>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                e = fmaxf(e, row_bcast<j>(e) + d[j]);      // lane j's e is final: it only ever took terms of rows < j
            });
            // 2. linear solve in units of 2^e.  The coefficient's exponent is formed as (e[j] - e[r]) + d[j]: the difference of
            // the two large numbers first (exact or nearly so), then the small one -- one rounding at the magnitude of d, where
            // the log-domain step rounded every term at the magnitude of u (ulp(1000) ~ 6e-5: 4e-5 relative in the sum)
            float acc = S * fexp2(mx - e);
            static_for<0, PB - 1>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                acc = fmaf(row_bcast<j>(acc), fexp2((row_bcast<j>(e) - e) + d[j]), acc);
            });
            // 3. back to the log domain; one 8-byte DS write per lane publishes the whole block to the ring mates
            mine = e + flog2(acc) + sp;
            lds_store64(ring + ch * 2 + ((own0 + r) % NPOS) * 8, mine, own0 + r + 1);
            __builtin_amdgcn_s_setprio(1);
            if (GRAD) {
                // marginals of the block's own triangle (unless the band waves write them) and of its gaps (off the critical path:
                // the block is out).  The gap in front of row r needs u of row r - 1: ONE row shift and one store for the 15 gaps
                // inside the block (until round 5: fifteen stores with four lanes each)
                if (ringBand) {
                    static_for<0, PB - 1>([&](auto jc) {
                        constexpr int j = decltype(jc)::value;
                        const float uj = row_bcast<j>(mine);
                        if (rvalid && r > j) grad_store(own0 + j, gz * fexp2(fmaf(X[RING - 1].v[j], LOG2E, uj) + arow));
                    });
                }
                const float um1 = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(mine), 0x111, 0xf, 0xf, false));   // row_shr:1
                if (rvalid && r >= 1) {
                    float nv = gz * fexp2(um1 + nz * LOG2E + arow) + nadd;
                    if (pgap) nv = nv - nadd;
                    dNoise[(size_t)gap_of<DIR>(prow, T) * Bs + c] = nv;
                }
            }
        } else {
            // (max,+): the same walk over the block's triangle on DPP row broadcasts.  Row j's value is final after step j-1 (the
            // cells of columns >= r are masked to -inf), so all rows advance together: per step ONE broadcast of u[j] = best[j] +
            // relu-select(diag[j]) and two branch-free candidate selects -- the skip (key -1: it wins every tie) for row j+1 and
            // the interval (j, r) for the rows below.  Candidates are the same single fp32 adds as before (u + noise, u + cell)
            // and ties go to the smaller key: the decode stays bit-identical.  (The stepwise form -- an LDS broadcast, a DS
            // publish and two compare-branch pushes per position -- took 465 cycles per position, 3.1 us per block; the
            // log-sum-exp sweeps need 1.4 since round 3.)
            float best = aM;
            int key = aK;
            if (prow == 0 || !rvalid) { best = 0.0f; key = -1; }      // the first position has the empty path; rows past the end: stand-ins
            const float spr = sp > 0.0f ? sp : 0.0f;                   // s * (s > 0), reference :29, :49-51
            static_for<0, PB - 1>([&](auto jc) {
                constexpr int j = decltype(jc)::value;
                const float uj = row_bcast<j>(best + spr);
                const int keyj = frame_of<DIR>(own0 + j < T ? own0 + j : T - 1, T);
                const float ts = uj + nz;
                const bool c1 = (r == j + 1) & ((ts > best) | ((ts == best) & (key > -1)));
                best = c1 ? ts : best;
                key = c1 ? -1 : key;
                const float tc = uj + (r > j ? X[RING - 1].v[j] : SEMICRF_NEG_INF);
                const bool c2 = (tc > best) | ((tc == best) & (keyj < key));
                best = c2 ? tc : best;
                key = c2 ? keyj : key;
            });
            mine = best + spr;
            mykey = key;
            lds_store64(ring + ch * 2 + ((own0 + r) % NPOS) * 8, mine, own0 + r + 1);
            __builtin_amdgcn_s_setprio(1);
        }
        if (trace) ev[7] = __builtin_readcyclecounter();

        // ---- once per block: publish the 16 finished positions to HBM -----------------------------
        if (rvalid) {
            if (k == K - 1 && lds_flag_load(&s_abort) != 0) mine = __uint_as_float(0x7fc00000u);     // a wait timed out: poison the results
            if (k < K - FAR0 || (GRAD && ringBand == 0)) {      // the far field of block k' ends at block k' - FAR0: only the band waves (GRAD) read the last FAR0 blocks' u
                unsigned ub = __float_as_uint(mine);
                if (ub == U_EMPTY) ub = 0x7fc00000u;            // keep the one reserved pattern free (NaN input scores)
                __hip_atomic_store(ug + (size_t)prow * Bs + c, ub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const float sc = MODE == 0 ? LN2 : 1.0f;
            if (u_out) u_out[(size_t)frow * Bs + c] = mine * sc;
            if (last_out && prow == T - 1) last_out[c] = mine * sc;
            if (MODE == 0 && DIR == 0 && !GRAD && pathg && prow == T - 1) {
                // logProb: the chain's path score was left by a path wave long ago (it needs no u); the only global LOAD of a ring
                // wave, after its last publish
                u64 gr;
                int spins = 0;
                bool ok = true;
                while (true) {
                    gr = load_granule(pathg + c);
                    if ((unsigned)(gr >> 32) == ptag) break;
                    __builtin_amdgcn_s_sleep(8);
                    if (spin_abort(ctrl, spins, SPIN_LIMIT, 15)) { ok = false; break; }
                }
                pathOut[c] = ok ? __uint_as_float((unsigned)gr) - mine * sc : __uint_as_float(0x7fc00000u);
            }
            if (GRAD) {    // diagonal: gout * exp(alpha + beta - logZ + s - 2 softplus(s))
                float dv = gz * fexp2(arow + mine + draw - 2.0f * sp);
                if (pdiag) dv = dv + nadd;                  // a one-frame interval of the path: the scatter's atomicAdd(+gout)
                dScore[((size_t)frow * T + frow) * Bs + c] = dv;
            }
            if (MODE == 1) code[(size_t)c * T + frow] = (mykey + 1) | (sp > 0.0f ? 0x40000000 : 0);
        }
        if (SEMICRF_PANEL_PROBES && trace) ts[k] = __builtin_amdgcn_s_memrealtime();                 // chain probe: u published
    }
}

}  // namespace semicrf
