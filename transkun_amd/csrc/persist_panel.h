#pragma once
// persist_panel.h -- the PANEL role of the persistent sweep (persist.hip): panel geometry, task decode, panel_role.
//
// PANEL waves (four per panel workgroup; every wave pulls its own tasks, no workgroup-level synchronisation): a task is
// (position block k >= FAR0, column part of <= 16 tiles, 32 chains, 4 of the 16 rows).  The wave streams the far field -- cells
// (p in its rows, j < 16(k-FAR0+1)) -- tile by tile through three LDS stages filled by asynchronous global->LDS loads (it counts
// its own outstanding loads), keeps the partial accumulators in registers and hands ONE number per (position, chain, part) to
// the spine.
#include "persist_common.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// PANEL role (per wave)
// ---------------------------------------------------------------------------------------------
constexpr int GRAD_AUX = SEMICRF_GRAD_AUX;   // nt: the gradient is written once
constexpr int CELL_AUX = SEMICRF_CELL_AUX;   // nt: every cell is read once -- keep the stream from evicting the (re-read) u values from L2
constexpr int PNS = SEMICRF_PNS;             // LDS stages per panel wave (tiles fetched ahead)
constexpr int PSTAGE_BYTES = 10240;          // 8 KB of cells + 2 KB of u values
constexpr int PW_MAX = SEMICRF_PW_MAX;       // panel waves per workgroup (LDS: PW_MAX * PNS * PSTAGE_BYTES = 150 KB; four of them run unless the sweep is throughput-bound)
constexpr int LDS_PANEL_BYTES = PW_MAX * PNS * PSTAGE_BYTES;
// A wave owns rows pi = 16k + 4*q4 + rr (rr < 4) of position block k for 32 chains.  lane = slot*8 + q8:
// q8 selects 4 of the 32 chains (8 consecutive lanes read one 128-byte line), slot selects the columns
// pj = 16m + slot + 8h (h < 2) of tile m.  Cells and u values of the next tiles are requested before tile m is
// processed.  The same mapping serves both directions (only cell_index differs).
// slow path of the panel accumulation: move the reference above tm when tm is within RESC_EARLY of the limit (see RESC_LIFT)
__device__ __forceinline__ void acc_lift(float& M, float& S, float tm)
{
    const bool need = tm > M + (RESC_HI - RESC_EARLY);                       // true for the empty accumulator (M = -inf)
    const float newM = need ? floorf(tm) + RESC_LIFT : M;
    const int sh = (int)fmaxf(M - newM, -4096.0f);                            // an integer; 0 when nothing moves
    S = __builtin_ldexpf(S, sh);                                              // exact; empty: S = 0 stays 0
    M = newM;
}

// ---- panel helpers (free functions: a lambda that calls another lambda keeps its closure in scratch once
// the body contains operations the optimiser treats as memory writes -- the global->LDS loads) ----------------
struct PanelGeom {
    int pirow[4];          // rows of the task, clamped to T-1
    unsigned voff;         // per-lane byte offset of the PROCESSING mapping (also the gradient stores)
    unsigned fvoff;        // per-lane byte offset of the FETCH mapping
    unsigned gvoff;        // per-lane byte offset into the u values
};

// element offset of the tile base
template <int DIR>
__device__ __forceinline__ size_t panel_tile_off(const PanelGeom& G, int m, int T, size_t Bs)
{
    return DIR == 0 ? ((size_t)G.pirow[0] * T + (size_t)m * PB) * Bs
                    : ((size_t)(T - 1 - (m * PB + 15)) * T + (size_t)(T - 1 - G.pirow[3])) * Bs;
}
// wave-uniform byte offset of cell group (rr, h) in the processing mapping
template <int DIR>
__device__ __forceinline__ unsigned panel_soff(const PanelGeom& G, int rr, int h, int T, size_t Bs)
{
    return DIR == 0 ? (unsigned)((((size_t)(G.pirow[rr] - G.pirow[0]) * T + 8 * h) * Bs) * 4)
                    : (unsigned)((((size_t)(1 - h) * 8 * T + (G.pirow[3] - G.pirow[rr])) * Bs) * 4);
}
// u of a tile's 16 columns (2 KB: the value is its own flag, U_EMPTY until published).
// COHERENT = false: ordinary cached loads.  u is written once and re-read by every task of the launch;
// device-scope (sc1) loads would fetch it through the fabric every time.  A stale cache line can only show
// U_EMPTY (the launch's fill, visible since the kernel boundary; 4-byte values are written atomically), which
// sends the reader to the COHERENT retry.
template <bool COHERENT>
__device__ __forceinline__ void panel_fetch_gran(__amdgpu_buffer_rsrc_t ursrc, char* stage, unsigned gvoff, int m, int B)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {       // positions 16m + 8h + slot, 4 chains (16 bytes) per lane
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane((m * PB + 8 * h) * B * 4);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ursrc, (lds_void_t*)(stage + 8192 + h * 1024), 16, gvoff, so, 0, COHERENT ? 16 : 0);   // 16 = sc1
    }
}
// FETCH mapping (global -> LDS, 1 KB per instruction, lane-linear in LDS):
//   DIR 0: instruction e = (rr, h) fetches what its lanes process (8 columns x 128 B of one matrix row);
//   DIR 1: instruction e fetches columns pj = 16m + 2e + pjsub for the 4 rows pi (4 x 128 B contiguous per pj):
//          lane = (pisub, pjsub, q8), same tile base, lane part ((1-pjsub)*T + (pi_3 - pi_pisub))*B, soffset (14-2e)*T*B.
//          The processing lane reads its cells back from ((slot>>1) + 4h)*1024 + rr*256 + (slot&1)*128 + q8*16.
template <int DIR, int AUX>
__device__ __forceinline__ void panel_fetch_cells_aux(const float* score, const PanelGeom& G, char* stage, int m, int T, size_t Bs)
{
    // The tile base and the piece offsets are wave-uniform by construction; said explicitly, because a load whose descriptor
    // or offset the compiler takes for divergent (task state that passed a lane-dependent loop exit) is wrapped in a
    // waterfall loop -- ten of them per tile.
    const size_t toff = panel_tile_off<DIR>(G, m, T, Bs);
    const size_t toff_u = (size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)toff) |
                          ((size_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(toff >> 32)) << 32);
    const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)(score + toff_u), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const unsigned so = (unsigned)__builtin_amdgcn_readfirstlane(
            (int)(DIR == 0 ? panel_soff<DIR>(G, e >> 1, e & 1, T, Bs) : (unsigned)(((size_t)(14 - 2 * e) * T * Bs) * 4)));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(stage + e * 1024), 16, G.fvoff, so, 0, AUX);
    }
}
// nt (wave-uniform run-time choice; the cache policy is an immediate of the instruction): see cell_policy_nt
template <int DIR>
__device__ __forceinline__ void panel_fetch_cells(const float* score, const PanelGeom& G, char* stage, int m, int T, size_t Bs, bool nt)
{
    if (nt) panel_fetch_cells_aux<DIR, CELL_AUX>(score, G, stage, m, T, Bs);
    else panel_fetch_cells_aux<DIR, 0>(score, G, stage, m, T, Bs);
}
__device__ __forceinline__ void panel_read_gran(unsigned addr, v4u& g0, v4u& g1)
{
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(g0), "=&v"(g1)
                 : "v"(addr));
}
template <int DIR>
__device__ __forceinline__ void panel_read_cells(unsigned addr, v4u (&o)[8])
{
    constexpr int XR = DIR == 0 ? 2048 : 256, XH = DIR == 0 ? 1024 : 4096;      // LDS offset of (rr, h): rr*XR + h*XH
    asm volatile("ds_read_b128 %0, %8 offset:%9\n\tds_read_b128 %1, %8 offset:%10\n\t"
                 "ds_read_b128 %2, %8 offset:%11\n\tds_read_b128 %3, %8 offset:%12\n\t"
                 "ds_read_b128 %4, %8 offset:%13\n\tds_read_b128 %5, %8 offset:%14\n\t"
                 "ds_read_b128 %6, %8 offset:%15\n\tds_read_b128 %7, %8 offset:%16\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(o[0]), "=&v"(o[1]), "=&v"(o[2]), "=&v"(o[3]), "=&v"(o[4]), "=&v"(o[5]), "=&v"(o[6]), "=&v"(o[7])
                 : "v"(addr), "n"(0 * XR + 0 * XH), "n"(0 * XR + 1 * XH), "n"(1 * XR + 0 * XH), "n"(1 * XR + 1 * XH),
                   "n"(2 * XR + 0 * XH), "n"(2 * XR + 1 * XH), "n"(3 * XR + 0 * XH), "n"(3 * XR + 1 * XH));
}
// wait until at most `younger` vector-memory operations are outstanding (rounded down to an encodable step)
__device__ __forceinline__ void panel_wait_younger(int y)
{
    if (y >= 44) wait_vmcnt<44>();
    else if (y >= 36) wait_vmcnt<36>();
    else if (y >= 28) wait_vmcnt<28>();
    else if (y >= 20) wait_vmcnt<20>();
    else if (y >= 10) wait_vmcnt<10>();
    else wait_vmcnt<0>();
}

// ---- task selection -----------------------------------------------------------------------------------------------
// Block k = FAR0 + q has q + 1 far tiles, cut at fixed columns into FULL parts of TPT tiles and one LAST part (see
// part_tiles), each split in four row quarters and 32-chain groups.  ONE queue in (block, part, chain group, row
// quarter) order: an atomic counter.  (Per-part earliest-deadline queues, full parts handed out early, next-task
// prefetch and "recent-tile" waves on the spine CUs were all measured slower, DESIGN.md section 3 "Round 2".)
struct PanelTask { int k, part, g, q4; };

// (block, part) number tt -> block k and column part
__device__ __forceinline__ void panel_tt_decode(int tt, PanelTask& t)
{
    if (tt < LEADT - 1) { t.part = 0; t.k = FAR0 + tt; return; }      // the first LEADT - 1 blocks: one part
    tt -= LEADT - 1;
    int a = 0;
    while (tt >= TPT * (a + 1) * (a + 2) / 2) ++a;          // group a: blocks with a+1 parts
    tt -= TPT * a * (a + 1) / 2;
    const int q = a * TPT + tt / (a + 1) + LEADT - 1;
    t.part = tt % (a + 1);
    t.k = FAR0 + q;
}
// queue position -> task
__device__ __forceinline__ void panel_task_decode(const SweepParams& P, int task, PanelTask& t)
{
    t.q4 = task & 3;
    const int t2 = task >> 2;
    t.g = t2 % P.nPanelGroups;
    panel_tt_decode(t2 / P.nPanelGroups, t);
}

__device__ __forceinline__ bool panel_next_task(const SweepParams& P, PanelTask& t)
{
    int task = 0;
    if ((threadIdx.x & 63) == 0) task = (int)(atomicAdd(P.ctrl + 2, 1u) + 1u);        // counters start at 0xffffffff (one 0xff fill)
    task = __builtin_amdgcn_readfirstlane(task) + P.taskBase;
    if (task >= P.nTasks) return false;
    panel_task_decode(P, task, t);
    return true;
}

template <int MODE, int DIR, bool GRAD>
__device__ __forceinline__ void panel_role(const SweepParams& P, char* lds, int wslot, int hist_role = 0, int first_task = -1)
{
    const int T = P.T, B = P.B;
    const int c0 = P.c0, c1 = P.c1;
    const unsigned dbg = DBGF(P);
    unsigned* const ctrl = P.ctrl;
    u64* const farg = P.farg;
    const float* const vfwd = P.vfwd;
    const float* const logZp = P.logZ;
    const float* const goutp = P.gout;
    float* const dScore = P.dScore;
    constexpr bool PFOLD = GRAD && DIR == 1;                           // the path table (a row is a begin frame in DIR 1 only)
    const int lane = threadIdx.x & 63;
    const int slot = lane >> 3, q8 = lane & 7;
    const size_t Bs = (size_t)B;
    const float* __restrict__ score = P.score;
    const unsigned tag = P.tag;
    const auto ursrc = __builtin_amdgcn_make_buffer_rsrc((void*)P.ug, 0, (int)((size_t)T * Bs * 4), 0x00020000);
    const bool cell_nt = __builtin_amdgcn_readfirstlane(P.cellNT) != 0, grad_nt = __builtin_amdgcn_readfirstlane(P.gradNT) != 0;

    // geometry of a task's tiles (see "addressing" below)
    auto geom_of = [&](const PanelTask& t, PanelGeom& G) {
        const int pb = t.k * PB + t.q4 * 4;
        const int cc = c0 + t.g * GP + q8 * 4;
        const int ccl = cc < c1 ? cc : c0;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) G.pirow[rr] = pb + rr < T ? pb + rr : T - 1;
        G.voff = DIR == 0 ? (unsigned)((slot * B + ccl) * 4) : (unsigned)(((size_t)(7 - slot) * T * Bs + ccl) * 4);
        const int f_pisub = lane >> 4, f_pjsub = (lane >> 3) & 1;
        const int f_pirow = pb + f_pisub < T ? pb + f_pisub : T - 1;
        G.fvoff = DIR == 0 ? G.voff : (unsigned)((((size_t)(1 - f_pjsub) * T + (G.pirow[3] - f_pirow)) * Bs + ccl) * 4);
        G.gvoff = (unsigned)((slot * B + ccl) * 4);
    };
    // vector-memory operations issued so far by this wave (a lower bound: the waits below may only under-count the operations
    // younger than the fetch they wait for), and its value right after each stage's fetch.  They run on across tasks.
    int issued = 0, mark0 = 0, mark1 = 0, mark2 = 0;
    // task timeline probe (probe build, dbg & 256; tools/task_trace.py): the wave that drew task 0 stamps 5 words per task at ts[3T/2 + 5n]
    bool tracer = false;
    int tn = 0;

    while (true) {
        // ---- next task: (k, part, g, q4); a task only waits on spine progress below k-3 ----
        PanelTask tk;
        if (first_task >= 0 && first_task < P.nTasks) {
            panel_task_decode(P, first_task, tk);
#if SEMICRF_STAGGER > 0
            // Staggered start (round 4): the ~700 panel waves of a launch all know their first task and used to request its first
            // tiles in the same microsecond -- 20 MB that the spines' loaders (and the first hand-offs) queued behind: the first 8
            // blocks took 20 - 27 us where the ring alone needs 11.  A wave whose first task belongs to block k waits roughly
            // until the ring can be there.
            for (int i = 0, n = tk.k - FAR0 < 48 ? tk.k - FAR0 : 48; i < n; ++i) __builtin_amdgcn_s_sleep(SEMICRF_STAGGER);
#endif
        } else if (!panel_next_task(P, tk)) break;
        first_task = -1;
        if (SEMICRF_PROBE_TASKS && (dbg & 256u) && tk.k == RING && tk.part == 0 && tk.g == 0 && tk.q4 == 0) tracer = true;
        u64* const tsp = P.ts + (3 * T) / 2 + 5 * tn;
        const bool tr = SEMICRF_PROBE_TASKS && tracer && lane == 0 && 5 * tn + 5 <= T / 2;
        if (tr) tsp[0] = __builtin_amdgcn_s_memrealtime();
        const int q = tk.k - FAR0;                                  // the newest far tile of this block
        int m0, m1;
        part_tiles(q, tk.part, m0, m1);                             // tiles m0 .. m1-1 of the q+1 panel tiles of block k
        const int k = tk.k, part = tk.part, g = tk.g, q4 = tk.q4;
        const int pbase = k * PB + q4 * 4;
        if (pbase >= T) continue;                               // rows past the end (last block)
        const int c = c0 + g * GP + q8 * 4;
        const bool cvalid = c < c1;
        const int cl = cvalid ? c : c0;                         // clamped chain for addresses

        float aM[4][4], aS[4][4];
        int aK[4][4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int i = 0; i < 4; ++i) { aM[rr][i] = SEMICRF_NEG_INF; aS[rr][i] = 0.f; aK[rr][i] = 0x7fffffff; }

        // GRAD: marginal(pi, pj) = gz * exp2(t + arow[rr]), arow = (alpha[frame(pi)] - logZ) * log2e
        float arow[4][4], gz[4];
        if (GRAD) {
            float lz[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool ok = c + i < c1;
                lz[i] = ok ? logZp[c + i] : 0.f;
                gz[i] = ok ? goutp[(size_t)(c + i) * P.gstride] * P.gscale : 0.f;
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {
                const int pi = pbase + rr;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float vv = (c + i < c1 && pi < T) ? vfwd[(size_t)frame_of<DIR>(pi, T) * Bs + c + i] : 0.f;
                    arow[rr][i] = (vv - lz[i]) * LOG2E;
                }
            }
        }
        int ptab_words[4] = {PTAB_NONE, PTAB_NONE, PTAB_NONE, PTAB_NONE};
        const int* const ptab = PFOLD ? kernarg_again<const int*>(offsetof(SweepParams, ptab)) : nullptr;
        if (PFOLD && ptab != nullptr) {
            // (row and chains clamped into the task's own: a word looked at twice can only raise the flag for a cell that IS the task's)
            const int prow = pbase + (slot & 3) < T ? pbase + (slot & 3) : T - 1;
            const int* const pr = ptab + (size_t)frame_of<DIR>(prow, T) * Bs;
#pragma unroll
            for (int i = 0; i < 4; ++i) ptab_words[i] = pr[c + i < c1 ? c + i : c1 - 1];
        }
        // ---- addressing -----------------------------------------------------------------------------------
        // Buffer addressing: one VGPR byte offset per lane (constant over the task), everything that depends
        // on (tile, rr, h) is wave-uniform and lives in the SGPR base / soffset -- no per-load 64-bit VALU math.
        //   DIR 0: cell(pi, pj) = (pi*T + pj)*B: tile base at (pi_0, 16m), lane part slot*B, soffset ((pi_rr-pi_0)*T + 8h)*B
        //   DIR 1: cell(pi, pj) = ((T-1-pj)*T + (T-1-pi))*B: tile base at (pi_3, 16m+15), lane part (7-slot)*T*B,
        //          soffset ((1-h)*8*T + (pi_3-pi_rr))*B            (pi_rr = min(pbase+rr, T-1))
        PanelGeom G;
        geom_of(tk, G);
        char* const stage0 = lds + wslot * (PNS * PSTAGE_BYTES);
        const unsigned rdbase = lds_addr(stage0) + (DIR == 0 ? (unsigned)lane * 16u
                                                             : (unsigned)((slot >> 1) * 1024 + (slot & 1) * 128 + q8 * 16));
        const unsigned grbase = lds_addr(stage0) + 8192u + (unsigned)lane * 16u;
        const bool probe_stream = SEMICRF_PANEL_PROBES && (dbg & 32u);
        const bool probe_nowait = SEMICRF_PANEL_PROBES && (dbg & 4u);
        const bool probe_nou = SEMICRF_PANEL_PROBES && (dbg & 64u);       // math on whatever the stage holds, no u traffic
        const int nst = GRAD ? 2 * (T - pbase < 4 ? T - pbase : 4) : 0;    // gradient stores per tile (a lower bound)

        // A task that has met an unpublished u runs at the spine's frontier: the u copies it prefetched three tiles ahead
        // are stale by construction.  From then on it fetches the NEXT tile's u again (device scope) while it works on
        // the current tile, so that a published value is found on the first look instead of two round trips later.
        bool frontier = false;
#pragma unroll
        for (int i = 0; i < PNS; ++i)
            if (m0 + i < m1) {
                panel_fetch_cells<DIR>(score, G, stage0 + i * PSTAGE_BYTES, m0 + i, T, Bs, cell_nt);
                if (!probe_stream && !probe_nou) panel_fetch_gran<false>(ursrc, stage0 + i * PSTAGE_BYTES, G.gvoff, m0 + i, B);
                issued += 10;
                if (i == 0) mark0 = issued; else if (i == 1) mark1 = issued; else mark2 = issued;
            }

        // The path table: does a path interval that begins in one of the task's rows end in one of its columns?  One wave-uniform
        // flag, found while the first tiles are on their way (slot s looks at row s & 3 of its four chains; the words were
        // requested in front of the tiles, so the wait for them is part of the wait for the first stage); the words themselves are
        // dropped -- the tile loop knows nothing of the path.
        bool pathfix = false;
        if (PFOLD && ptab != nullptr) {
            bool hit = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int pj = T - 1 - (ptab_words[i] & PTAB_NONE);      // none: far below zero
                hit = hit | ((unsigned)(pj - m0 * PB) < (unsigned)((m1 - m0) * PB));
            }
            pathfix = __any(hit);
        }

        for (int m = m0, s = 0; m < m1; ++m, s = (s + 1 == PNS ? 0 : s + 1)) {
            char* const stage = stage0 + s * PSTAGE_BYTES;
            // ---- wait for the stage, move it to registers ------------------------------------------------
            const bool tprobe = SEMICRF_PANEL_PROBES && (dbg & 16u) && g == 0 && q4 == 0 && m == q && lane == 0 && k < 64 && T >= 1024;
            if (tprobe) P.ts[1536 + k] = __builtin_amdgcn_s_memrealtime();
            panel_wait_younger(issued - (s == 0 ? mark0 : (s == 1 ? mark1 : mark2)));
            if (tprobe) P.ts[1600 + k] = __builtin_amdgcn_s_memrealtime();
            int npoll = 0;
            if (tr && m == m0) tsp[1] = __builtin_amdgcn_s_memrealtime();
            if (SEMICRF_PROBE_HIST && (dbg & 1024u) && lane == 0) {
                // activity histogram (tools/activity_hist.py): tiles taken per 4 us bucket, panel and spare waves apart
                u64* const hb = P.ts + (3 * T) / 2;
                const u64 now = __builtin_amdgcn_s_memrealtime();
                // (s_memrealtime counts per XCD: every XCD's tiles are bucketed against the start of ITS first workgroup)
                const u64 t0 = __hip_atomic_load(hb + 129 + (__builtin_amdgcn_s_getreg(6164) & 7), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                u64 b = now > t0 ? (now - t0) / 400 : 0;
                if (b > 63) b = 63;
                atomicAdd((unsigned long long*)(hb + 1 + 64 * hist_role + b), 1ull);
            }
            v4u xo[8];
            panel_read_cells<DIR>(rdbase + (unsigned)(s * PSTAGE_BYTES), xo);
            const bool refill = m + PNS < m1;
            if (probe_stream) {          // streaming probe: touch the data, nothing else
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    aS[0][0] += __uint_as_float(xo[e].x) + __uint_as_float(xo[e].y) + __uint_as_float(xo[e].z) + __uint_as_float(xo[e].w);
            } else {
                v4u g0, g1;      // [h]: u of 4 chains at position 16m + 8h + slot
                panel_read_gran(grbase + (unsigned)(s * PSTAGE_BYTES), g0, g1);
                // a value that has not been published yet reads as U_EMPTY (from the launch's memset, possibly out of a
                // stale cache line): fetch again with device-scope loads until the spine has published block m
                if (!probe_nowait) {
                    const bool v0 = c < c1, v1 = c + 1 < c1, v2 = c + 2 < c1, v3 = c + 3 < c1;
                    int spins = 0;
                    while (true) {
                        const bool ok = (g0.x != U_EMPTY || !v0) && (g0.y != U_EMPTY || !v1) && (g0.z != U_EMPTY || !v2) &&
                                        (g0.w != U_EMPTY || !v3) && (g1.x != U_EMPTY || !v0) && (g1.y != U_EMPTY || !v1) &&
                                        (g1.z != U_EMPTY || !v2) && (g1.w != U_EMPTY || !v3);
                        if (__all(ok)) break;
                        frontier = true;
                        // The task's newest tile (m == q) is on the spine's critical path: poll tightly.  Waves blocked
                        // further ahead advance one tile per spine block; the forward sweeps want them prompt as well
                        // (lazy: 240 us, prompt: 212 us), the bandwidth-bound gradient sweep wants the fabric quiet
                        // (prompt: 505-525 us, lazy: 465-472 us).
                        if (m == q) __builtin_amdgcn_s_sleep(2);
                        else if (GRAD) {
                            // (round 5: the lazy poll pays only where the gradient sweep is bandwidth-bound; with few chains it is
                            // hand-off-bound like the forward sweep -- T=691 x 96: 122 -> 112 us, T=1024 x 88: 222 -> 216 with the short one)
                            if (P.gradLazyShort) __builtin_amdgcn_s_sleep(16);
                            else __builtin_amdgcn_s_sleep(SEMICRF_GRAD_LAZY);
                        }
                        else __builtin_amdgcn_s_sleep(16);
                        if (spin_abort(ctrl, spins, SPIN_LIMIT, 5)) break;
                        ++npoll;
                        // One round trip per poll: the 2 KB tile is fetched again together with a light probe -- one word per
                        // lane, the block's last position for the first of the lane's four chains (a ring publishes its
                        // 16 positions x 4 chains with one store instruction).  The LDS copy is only read back and checked
                        // when every ring of the tile shows a value in the probe; urgent polls (the task's newest tile)
                        // fetch the tile with every probe, lazy ones only after a successful probe.
                        if (m == q) panel_fetch_gran<true>(ursrc, stage, G.gvoff, m, B);
                        const unsigned pw = __builtin_amdgcn_raw_buffer_load_b32(ursrc, (unsigned)(cl * 4), (unsigned)((m * PB + PB - 1) * B * 4), 16);
                        if (!__all(pw != U_EMPTY || !cvalid)) continue;
                        if (m != q) panel_fetch_gran<true>(ursrc, stage, G.gvoff, m, B);
                        wait_vmcnt<0>();
                        panel_read_gran(grbase + (unsigned)(s * PSTAGE_BYTES), g0, g1);
                    }
                }
                if (frontier && m + 1 < m1) {
                    const int sn = s + 1 == PNS ? 0 : s + 1;
                    panel_fetch_gran<true>(ursrc, stage0 + sn * PSTAGE_BYTES, G.gvoff, m + 1, B);
                    issued += 2;
                    if (sn == 0) mark0 = issued; else if (sn == 1) mark1 = issued; else mark2 = issued;
                }
                if (SEMICRF_PANEL_PROBES && (dbg & 16u) && g == 0 && q4 == 0 && m == q && lane == 0) P.ts[192 + k] = __builtin_amdgcn_s_memrealtime();   // chain probe: newest tile's u seen
                // chains past the end of the batch (a ragged last quad reads the NEXT position's first chains there, published or
                // not; a quad that lies past the end altogether reads the first chains, waited for or not): their u is set to 0,
                // so that what they contribute to the wave-wide rescale test -- and with it the other chains' reference points
                // and the last bits of their sums -- does not depend on timing
                if (c >= c1) { g0.x = 0u; g1.x = 0u; }
                if (c + 1 >= c1) { g0.y = 0u; g1.y = 0u; }
                if (c + 2 >= c1) { g0.z = 0u; g1.z = 0u; }
                if (c + 3 >= c1) { g0.w = 0u; g1.w = 0u; }
                const float uv[2][4] = {{__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z), __uint_as_float(g0.w)},
                                        {__uint_as_float(g1.x), __uint_as_float(g1.y), __uint_as_float(g1.z), __uint_as_float(g1.w)}};

                if (MODE == 0) {
                    // The accumulation with half the vector instructions (the panels are issue- and power-bound next
                    // to their loads): the exponent argument t - M = cell*log2e + (u - M) is ONE packed fma per two chains
                    // on top of one packed subtract, the overflow test is a max3 tree over those arguments, the sums are
                    // packed adds: 17 plain instructions + 8 exps per row of 8 cells instead of 35 + 8.
                    // GRAD (round 5: the same packed form, and ONE exponential per cell): the marginal gz 2^(t + arow) is the
                    // accumulator's own term p = 2^(t - M) times the per-(row, chain) factor gz 2^(M + arow) -- four exponentials
                    // per row of eight cells instead of eight more.  (Until then the gradient sweep ran the unpacked form with
                    // two exponentials per cell: a frontier task's tile took 1.3 us of math against 0.3 in the forward sweep,
                    // and the ring's block period in the head of the sweep IS that task's time per tile.  M + arow <= ~97: M sits
                    // RESC_LIFT above the largest term when it is set and 2^(term + arow) is a marginal; a cell whose term
                    // lies 2^-30 below that one underflows -- as it does in the sum -- where the reference holds a marginal below
                    // 1e-9.  The factor underflows too: M + arow is 96 above log2 of the marginal of the cell that set M, and M
                    // stays where it is until a term of the wave passes M + RESC_HI.  After a cell with a marginal below 2^-221
                    // v_exp_f32 returns 0 for the factor, and every later cell of that row and chain is stored as 0 until the next
                    // lift, marginals up to 2^-18 among them; measured, it took ones below 2^-75 (tests/test_sweep_accuracy.py,
                    // DESIGN.md "Accuracy of the sweeps, per element").)  The beta values are bit-identical to the plain beta
                    // sweep's.
                    typedef float v2f __attribute__((ext_vector_type(2)));
                    const v2f l2e = {LOG2E, LOG2E};
                    const v2f u2[2][2] = {{{uv[0][0], uv[0][1]}, {uv[0][2], uv[0][3]}}, {{uv[1][0], uv[1][1]}, {uv[1][2], uv[1][3]}}};
                    const auto gs = __builtin_amdgcn_make_buffer_rsrc((void*)(GRAD ? dScore + panel_tile_off<DIR>(G, m, T, Bs) : nullptr), 0,
                                                                      0x7fffffff, 0x00020000);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        v2f e[2][2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const v4u xv = xo[rr * 2 + h];
                            const v2f x2[2] = {{__uint_as_float(xv.x), __uint_as_float(xv.y)}, {__uint_as_float(xv.z), __uint_as_float(xv.w)}};
#pragma unroll
                            for (int j = 0; j < 2; ++j) {
                                const v2f mj = {aM[rr][2 * j], aM[rr][2 * j + 1]};
                                e[h][j] = __builtin_elementwise_fma(x2[j], l2e, u2[h][j] - mj);      // M = -inf (empty): +inf
                            }
                        }
                        const float emax = fmaxf(fmaxf(fmaxf(e[0][0].x, e[0][0].y), fmaxf(e[0][1].x, e[0][1].y)),
                                                 fmaxf(fmaxf(e[1][0].x, e[1][0].y), fmaxf(e[1][1].x, e[1][1].y)));
                        if (__any(emax > RESC_HI)) {
                            // some accumulator's reference point is too low (always on the first tile): move it up
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float x0 = __uint_as_float(i == 0 ? xo[rr * 2].x : (i == 1 ? xo[rr * 2].y : (i == 2 ? xo[rr * 2].z : xo[rr * 2].w)));
                                const float x1 = __uint_as_float(i == 0 ? xo[rr * 2 + 1].x : (i == 1 ? xo[rr * 2 + 1].y : (i == 2 ? xo[rr * 2 + 1].z : xo[rr * 2 + 1].w)));
                                const float t0 = fmaf(x0, LOG2E, uv[0][i]), t1 = fmaf(x1, LOG2E, uv[1][i]);
                                acc_lift(aM[rr][i], aS[rr][i], fmaxf(t0, t1));
                                const float e0 = t0 - aM[rr][i], e1 = t1 - aM[rr][i];
                                if (i & 1) { e[0][i >> 1].y = e0; e[1][i >> 1].y = e1; } else { e[0][i >> 1].x = e0; e[1][i >> 1].x = e1; }
                            }
                        }
                        v2f mg[2][2];                                   // GRAD: the marginals of the row's two cell groups
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            v2f sj = {aS[rr][2 * j], aS[rr][2 * j + 1]};
                            const v2f p0 = {fexp2(e[0][j].x), fexp2(e[0][j].y)};
                            const v2f p1 = {fexp2(e[1][j].x), fexp2(e[1][j].y)};
                            sj = (sj + p0) + p1;
                            aS[rr][2 * j] = sj.x; aS[rr][2 * j + 1] = sj.y;
                            if (GRAD) {
                                const v2f mj = {aM[rr][2 * j], aM[rr][2 * j + 1]};
                                const v2f aj = {arow[rr][2 * j], arow[rr][2 * j + 1]};
                                const v2f fa = mj + aj;
                                const v2f gzj = {gz[2 * j], gz[2 * j + 1]};
                                const v2f fx = {fexp2(fa.x), fexp2(fa.y)};
                                const v2f gF = gzj * fx;
                                mg[0][j] = gF * p0;
                                mg[1][j] = gF * p1;
                            }
                        }
                        if (GRAD) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                if (cvalid && pbase + rr < T) {
                                    const unsigned so = panel_soff<DIR>(G, rr, h, T, Bs);
                                    v4u gv;
                                    gv.x = __float_as_uint(mg[h][0].x);
                                    gv.y = __float_as_uint(mg[h][0].y);
                                    gv.z = __float_as_uint(mg[h][1].x);
                                    gv.w = __float_as_uint(mg[h][1].y);
                                    if (c + 3 < c1) {
                                        if (grad_nt) __builtin_amdgcn_raw_buffer_store_b128(gv, gs, G.voff, so, GRAD_AUX);
                                        else __builtin_amdgcn_raw_buffer_store_b128(gv, gs, G.voff, so, 0);
                                    }
                                    else {                                  // ragged tail of the chain range
                                        __builtin_amdgcn_raw_buffer_store_b32(gv.x, gs, G.voff, so, 0);
                                        if (c + 1 < c1) __builtin_amdgcn_raw_buffer_store_b32(gv.y, gs, G.voff + 4, so, 0);
                                        if (c + 2 < c1) __builtin_amdgcn_raw_buffer_store_b32(gv.z, gs, G.voff + 8, so, 0);
                                    }
                                }
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if (GRAD) issued += nst;
                } else {
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const v4u xv = xo[rr * 2 + h];
                            const float xe[4] = {__uint_as_float(xv.x), __uint_as_float(xv.y), __uint_as_float(xv.z), __uint_as_float(xv.w)};
                            const int key = frame_of<DIR>(m * PB + slot + 8 * h, T);
#pragma unroll
                            for (int i = 0; i < 4; ++i) max_push_seq<DIR>(aM[rr][i], aK[rr][i], uv[h][i] + xe[i], key);
                        }
                }
            }
            if (tprobe) { P.ts[1664 + k] = __builtin_amdgcn_s_memrealtime(); P.ts[1792 + k] = (u64)npoll; }
            // ---- refill the stage PNS tiles ahead ----------------------------------------------------------
            if (refill) {
                panel_fetch_cells<DIR>(score, G, stage, m + PNS, T, Bs, cell_nt);
                if (!probe_stream && !probe_nou) panel_fetch_gran<false>(ursrc, stage, G.gvoff, m + PNS, B);
                issued += 10;
                if (s == 0) mark0 = issued; else if (s == 1) mark1 = issued; else mark2 = issued;
            }
        }
        if (tr) { tsp[2] = __builtin_amdgcn_s_memrealtime(); tsp[4] = (u64)(m1 - m0) | ((u64)k << 8) | ((u64)(frontier ? 1 : 0) << 16) | ((u64)part << 20); }
        // Nothing that WRITES LDS is in flight here: every stage of the task was waited for before it was read, the coherent
        // re-fetch of a tile's u is only issued for a tile that is still to come (and waited for there), a refill only for a tile
        // m + PNS < m1.  What may be outstanding are the gradient stores of the last tiles -- and waiting for their
        // acknowledgements (0.7 us, measured) sat in front of the reduction of EVERY newest tile, on the ring's critical path.
        if (!(GRAD && MODE == 0)) wait_vmcnt<0>();
        (void)frontier;
        if (SEMICRF_PANEL_PROBES && (dbg & 16u) && g == 0 && q4 == 0 && m1 == q + 1 && lane == 0 && k < 64 && T >= 1024)
            P.ts[1728 + k] = __builtin_amdgcn_s_memrealtime();

        // ---- reduce over the 8 column slots (lane bits 3..5) --------------------------------------------------------------
        // The task's last tile is the newest one: what follows sits on the ring's critical path (16 hand-off rounds per
        // sweep at T=1024: a microsecond here is 16 in the total).  The 16 accumulators of every lane go
        // through LDS once (the wave's stages are idle now) and each lane merges the 8 slot values of its two results with
        // ONE exact maximum and 8 independent exps, instead of a 3-stage shuffle tree with two dependent exps per stage.
        const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0, b3 = (lane & 8) != 0;
        u64* fbase = farg + (size_t)part * T * Bs;
        const int pi = pbase + (b5 ? 2 : 0) + (b4 ? 1 : 0);
        {
            constexpr int RSTR = 65 * 8;                                  // bytes between accumulators (65 lanes: spreads the banks)
            char* const rb = stage0;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *(float2*)(rb + (rr * 4 + i) * RSTR + lane * 8) =
                        make_float2(aM[rr][i], MODE == 0 ? aS[rr][i] : __int_as_float(aK[rr][i]));
            const int orow = (b5 ? 2 : 0) + (b4 ? 1 : 0);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int oi = (b3 ? 2 : 0) + e;
                const char* src = rb + (orow * 4 + oi) * RSTR + q8 * 8;
                float2 v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = *(const float2*)(src + j * 64);            // slot j, same chain quad
                const int cc = c + oi;
                u64 gr;
                if (MODE == 0) {
                    float mx = v[0].x;
#pragma unroll
                    for (int j = 1; j < 8; ++j) mx = fmaxf(mx, v[j].x);
                    float sum = 0.f;
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum += v[j].y == 0.0f ? 0.0f : v[j].y * fexp2(v[j].x - mx);   // empty: (-inf, 0)
                    gr = make_granule(tag, mx + flog2(sum));
                } else {
                    float bm = v[0].x;
                    int bk = __float_as_int(v[0].y);
#pragma unroll
                    for (int j = 1; j < 8; ++j) max_push(bm, bk, v[j].x, __float_as_int(v[j].y));
                    gr = make_granule_key(tag, bm, bk);
                }
                if (pi < T && cc < c1 && !(SEMICRF_PANEL_PROBES && (dbg & 32u))) store_granule(fbase + (size_t)pi * Bs + cc, gr);
            }
        }
        if (SEMICRF_PANEL_PROBES && (dbg & 16u) && g == 0 && m1 == q + 1 && lane == 0 && k < 64)
            P.ts[256 + 64 * q4 + k] = __builtin_amdgcn_s_memrealtime();     // chain probe: partial stored (per row quarter)
        // ---- the path's cells among this task's (rare: a few thousand cells per call against ~10^5 tasks) --------------------------
        // Behind the hand-off, with the accumulators dead.  The cell (row rr, column pj) was stored by THIS wave -- by the lane whose
        // slot is pj & 7, for its chain quad -- so once the wave's stores are acknowledged that lane reads the marginal back (device
        // scope: past this CU's vector cache) and stores marginal + gout with the policy of the first store: no other wave, no atomics,
        // one rounding as in the scatter kernel.
        if (PFOLD && pathfix) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int* const ptab2 = kernarg_again<const int*>(offsetof(SweepParams, ptab));
            const float* const gout2 = kernarg_again<const float*>(offsetof(SweepParams, gout));
            float* const dScore2 = kernarg_again<float*>(offsetof(SweepParams, dScore));
            const int gstride2 = kernarg_again<int>(offsetof(SweepParams, gstride));
            const float wpath = kernarg_again<float>(offsetof(SweepParams, noiseAdd));
            int f0, f1;
            part_tiles(k - FAR0, part, f0, f1);
#pragma nounroll
            for (int n = 0; n < 16; ++n) {                               // (row n >> 2, chain n & 3 of the quad): a plain loop, it runs rarely
                const int prow = pbase + (n >> 2), ci = c + (n & 3);
                if (prow >= T) break;
                const int fb = frame_of<DIR>(prow, T);
                const int pend = ptab2[(size_t)fb * Bs + (ci < c1 ? ci : c1 - 1)] & PTAB_NONE;
                const int pj = T - 1 - pend;
                if (ci < c1 && (unsigned)(pj - f0 * PB) < (unsigned)((f1 - f0) * PB) && (pj & 7) == (lane >> 3)) {
                    float* const cell = dScore2 + ((size_t)pend * T + fb) * Bs + ci;
                    const float mv = __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const float nv = mv + wpath * gout2[(size_t)ci * gstride2];
                    if (grad_nt) __builtin_nontemporal_store(nv, cell);
                    else *cell = nv;
                }
            }
        }
        if (tr) tsp[3] = __builtin_amdgcn_s_memrealtime();
        ++tn;
    }
}

}  // namespace semicrf
