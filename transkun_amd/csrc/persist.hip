// persist.hip -- persistent blocked sweep for the semi-CRF recurrences on gfx950 (impl 0 / auto).
//
// One launch computes, for every chain, the T-long dependent recurrence
//     u[p] = finalize( (+)_{j<p} ( u[j] (x) cell(p,j) ), skip(p) )        p = 0..T-1 (position order)
// in the (logsumexp,+) semiring (alpha/beta sweeps, NeuralSemiCRFInterval.py:402-410) or the
// (max,+) semiring with argmax (viterbi / viterbiBackward, :27-51, :122-144).  Positions run over
// frames ascending (DIR 0) or descending (DIR 1); cell(p,j) is score[end][begin] of the two frames.
//
// Work decomposition (positions in blocks of 16, workgroups of 10 waves, ONE workgroup per compute unit):
//   * SPINE workgroup, one per 4 chains: a ring of four waves walks the T-step dependent chain inside one CU, fed by a LOADER
//     wave (band cells) and a FAR wave (the panels' partial results) -- persist_spine.h;
//   * PANEL waves stream the far field tile by tile, every wave pulling its own tasks, and hand ONE number per (position, chain,
//     column part) to the spine -- persist_panel.h; in the gradient sweep spare waves of the panel workgroups write the zero
//     upper triangle and the band's marginals (persist_grad.h), in launches with few chains they copy the band into
//     spine-major order (persist_bandcopy.h);
//   * hand-offs carry their own flag, every wait is bounded -- persist_common.h; what -D can vary -- persist_tuning.h.
//     Roles go by workgroup index (wg_ticket: the eight rings of a 32-chain panel group share one XCD).
// This file keeps the path role, the workgroup -> role map, the kernel and the host side (workspace layout, launch plan,
// launcher): one translation unit.
//
// HBM traffic: every lower-triangle cell is read exactly once (128-byte lines, non-temporal, in the panels;
// 16-byte segments in the band).  Algorithmic bytes per sweep: 4*B*(T(T+1)/2 + T-1).
#include <atomic>
#include <stdlib.h>
#include "common.h"
#include "launchers.h"
#include "pathscore.h"

#include "persist_common.h"
#include "persist_spine.h"
#include "persist_panel.h"
#include "persist_grad.h"
#include "persist_bandcopy.h"

namespace semicrf {

// ---------------------------------------------------------------------------------------------
// waves and LDS of a workgroup
// ---------------------------------------------------------------------------------------------
// A spine workgroup: waves 0 .. RING-1 ring, wave RING loader, wave RING+1 far wave 0 -- HWAVES in all -- then its spare waves:
// up to HPW_MAX streaming (hybrid panel) waves, the path wave, and as the workgroup's LAST waves far waves 1 .. NFARW-1 (as wave 6
// a second far wave pushed the two streaming waves from SIMDs 2 and 3 to SIMDs 3 and 0 -- next to ring wave 0 and the loader -- and
// the gradient sweep, whose spare waves stream from block 12 on, lost 2 - 7 % although it uses one far wave).
constexpr int HWAVES = RING + 2;
constexpr int LDS_HYBRID_PANEL = (LDS_SPINE_BYTES + 1023) / 1024 * 1024;     // the spine's LDS, padded: behind it the stages of the workgroup's streaming waves
constexpr int HPW_MAX = (160 * 1024 - 512 - LDS_HYBRID_PANEL) / (PNS * PSTAGE_BYTES) < NT / 64 - HWAVES
                            ? (160 * 1024 - 512 - LDS_HYBRID_PANEL) / (PNS * PSTAGE_BYTES) : NT / 64 - HWAVES;
static_assert(HWAVES <= NT / 64 && LDS_HYBRID_PANEL <= 160 * 1024 - 512, "wave roles");
static_assert(HPW_MAX + 1 + (NFARW - 1) <= NT / 64 - HWAVES, "spare waves of a spine workgroup: streaming waves + path wave + far waves 1..NFARW-1");
constexpr int LDS_HYBRID_BYTES = LDS_HYBRID_PANEL + (HPW_MAX > 0 ? HPW_MAX : 0) * PNS * PSTAGE_BYTES;
constexpr int LDS_DYN_MAX2 = LDS_HYBRID_PANEL > LDS_PANEL_BYTES ? LDS_HYBRID_PANEL : LDS_PANEL_BYTES;
constexpr int LDS_DYN_BYTES = LDS_HYBRID_BYTES > LDS_DYN_MAX2 ? LDS_HYBRID_BYTES : LDS_DYN_MAX2;   // > half of the CU's 160 KB: one workgroup per CU

// ---------------------------------------------------------------------------------------------
// PATH role (forward sweep of logProb): the path scores, by one otherwise idle wave per workgroup
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void path_role(const SweepParams& P)
{
    const int nb = P.c1 - P.c0;
    while (true) {
        int i = 0;
        if ((threadIdx.x & 63) == 0) i = (int)(atomicAdd(P.ctrl + CTRL_PATHQ, 1u) + 1u);
        i = __builtin_amdgcn_readfirstlane(i);
        if (i >= nb) break;
        const int c = P.c0 + i;
        const double r = path_score_wave(P.score, P.noise, P.T, P.B, P.pathK, P.pathPairs, P.pathOffsets, c);
        // Every lane stores the (same) granule.  With `if (lane == 0) store` here the compiler threaded this branch into the next
        // iteration's `if (lane == 0) draw` and ran the readfirstlane of the draw -- and everything behind it -- a second time with
        // lane 0 masked off: an endless loop on chain c0 (gfx950, ROCm 7.2; found as a hang of the whole launch).
        __builtin_amdgcn_wave_barrier();
        store_granule(P.pathg + c, make_granule(P.tag, (float)r));
        // the same walk leaves the path as a table for the backward call (every word of the chain's column, every call)
        if (P.ptabOut) path_table_wave(P.ptabOut, P.T, P.B, P.pathK, P.pathPairs, P.pathOffsets, c);
    }
}

// Workgroup index -> role ticket (spines: tickets < nSpine = the chain group; panel workgroups: nSpine + a dense rank).
// The eight rings of a 32-chain panel group read the 16-byte pieces of the SAME 128-byte lines of the band, and their far
// waves take partials from the same tasks: they belong on ONE XCD (one L2).  Block b is observed to run on XCD b % 8 (a
// placement HIP does not promise: only speed depends on it), so panel group g gets the first blocks of XCD g % 8.  Groups
// dealt to the XCDs by block index alone -- every ring of a group on a different XCD -- cost 216-228 us instead of 185; the
// earlier first-come ticket (an atomic per workgroup) clustered them by luck of arrival.
__host__ __device__ __forceinline__ int wg_ticket(int nSpine, int grid, int b)
{
    constexpr int X = 8, SPG = GP / GS;                      // XCDs, spine workgroups per panel group
    const int ngroups = (nSpine + SPG - 1) / SPG;
    int S[X], W[X];
    bool fits = true;
#pragma unroll
    for (int x = 0; x < X; ++x) {
        W[x] = x < grid ? (grid - x + X - 1) / X : 0;        // workgroups of the launch on XCD x
        int sx = 0;
        for (int g = x; g < ngroups; g += X) sx += nSpine - g * SPG < SPG ? nSpine - g * SPG : SPG;
        S[x] = sx;
        fits = fits && sx <= W[x];
    }
    if (!fits) return b;                                     // too few workgroups per XCD: plain order
    const int x = b % X, slot = b / X;
    int Sx = 0, Px = 0;
#pragma unroll
    for (int i = 0; i < X; ++i) if (i == x) { Sx = S[i]; Px = W[i] - S[i]; }
    (void)Px;
    if (slot < Sx) return (x + X * (slot / SPG)) * SPG + slot % SPG;       // ring slot % SPG of panel group x + 8 (slot / SPG)
    const int ps = slot - Sx;                                // panel workgroups: dense rank, level by level across the XCDs
    int rank = 0;
#pragma unroll
    for (int i = 0; i < X; ++i) {
        const int pn = W[i] - S[i];
        rank += ps < pn ? ps : pn;
        if (i < x && pn > ps) ++rank;
    }
    return nSpine + rank;
}

// ---------------------------------------------------------------------------------------------
// kernel
// ---------------------------------------------------------------------------------------------
// Launched with enough dynamic LDS that only ONE workgroup fits a compute unit, so with grid <= #CUs every
// workgroup is resident.  A SPINE workgroup (ticket < nSpine): waves 0-3 ring, wave 4 loader, wave 5 far wave,
// waves 6.. panel waves (hybridPanelWaves of them), then the path wave, the last wave far wave 1 (see HWAVES); the other
// workgroups: `panelWaves` panel waves, then the zero, band, copy and path waves the launch plan gives them.
template <int MODE, int DIR, bool GRAD>
__global__ __launch_bounds__(NT) void persist_sweep_kernel(SweepParams P)
{
    extern __shared__ __attribute__((aligned(16))) char s_dyn[];
    __shared__ int s_exit;
    // A leased workspace that an earlier launch left with its error word up (the host fills it again as soon as it has seen the
    // pinned abort word, but launches it had already enqueued arrive first): this launch gives up at once -- its waits see the
    // word within a few polls, its outputs are poisoned like the aborted launch's own.
    if (threadIdx.x == 0) {
        const unsigned e1 = __hip_atomic_load(P.ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned gen = P.selfclean ? __hip_atomic_load(P.ctrl + CTRL_GEN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : P.expect_gen;
        s_abort = e1 != CTRL_INIT ? 1 : 0;
        // a "clean" lease that is not in the state its last launch must have left (somebody else wrote to the workspace, or a launch
        // the host never saw): nothing in it can be trusted
        if (gen != P.expect_gen) { set_error(P.ctrl, 13u); s_abort = 1; }
        s_exit = 0;
    }
    // flags and sequence numbers start at 0
    // (the one-trip outer loop is what is left of a loop over the spines of a workgroup; without it the compiler lays one
    // branch of wg_ticket out the other way round, and the shipped code is kept instruction for instruction)
    for (int h = 0; h < 1; ++h)
        for (int i = threadIdx.x; i < (LDS_DUMMY - LDS_FAR) / 4; i += NT) ((int*)(s_dyn + LDS_FAR))[i] = 0;
    __syncthreads();
    // Roles by workgroup index: every workgroup of the launch is resident (one per CU, the grid never exceeds the CUs) and
    // the dispatcher starts them in index order, so a workgroup still only waits on earlier ones.  (An atomic ticket cost
    // every workgroup a device-scope round trip before it could do anything, on a line that hundreds of waves hit with
    // their first task draws at the same moment.)
    const int ticket = wg_ticket(P.nSpine, (int)gridDim.x, (int)blockIdx.x);
    const int wave = (int)(threadIdx.x >> 6);
    if (P.ug_other && wave == NT / 64 - 1) {
        // Leased workspace: the u values of the PREVIOUS launch go back to U_EMPTY here -- the two launches use alternate
        // buffers, so this one's own values can stay until the next launch: nobody has to know when the last reader of a u is
        // through (rounds 2-4: the rings cleared their group's u at the end of the sweep, which ruled out any reader that may
        // finish after the ring).  Every workgroup clears one slice with its last wave, in whole 16-byte pieces, before that wave takes up
        // its role (far wave 1 in a spine workgroup; a band wave, the copy wave or none in a panel workgroup).
        const size_t n = (size_t)P.T * P.B, n4 = n / 4;
        const size_t per = (n4 + gridDim.x - 1) / gridDim.x, i0 = per * blockIdx.x, i1 = i0 + per < n4 ? i0 + per : n4;
        const v4u e = {U_EMPTY, U_EMPTY, U_EMPTY, U_EMPTY};
        for (size_t i = i0 + (threadIdx.x & 63); i < i1; i += 64) ((v4u*)P.ug_other)[i] = e;
        if (blockIdx.x == 0 && (threadIdx.x & 63) < (int)(n - n4 * 4)) P.ug_other[n4 * 4 + (threadIdx.x & 63)] = U_EMPTY;
    }
    // clock probe (probe build, debug flag 128): shader cycles and 100 MHz ticks of one panel workgroup over the launch
    const bool clk = SEMICRF_PANEL_PROBES && (DBGF(P) & 128u) && ticket == P.nSpine + 3 && threadIdx.x == 0;
    if (clk) { P.ts[600] = __builtin_readcyclecounter(); P.ts[601] = __builtin_amdgcn_s_memrealtime(); }
    if (SEMICRF_PROBE_HIST && (DBGF(P) & 1024u) && threadIdx.x == 0) {        // activity histogram: t0 = the first workgroup's start, per XCD
        const unsigned long long now = (unsigned long long)__builtin_amdgcn_s_memrealtime();
        atomicMin((unsigned long long*)(P.ts + (3 * P.T) / 2), now);
        atomicMin((unsigned long long*)(P.ts + (3 * P.T) / 2 + 129 + (__builtin_amdgcn_s_getreg(6164) & 7)), now);     // hwreg(HW_REG_XCC_ID, 0, 4)
    }
    if (ticket < P.nSpine) {
        // chain group = ticket: neighbouring groups read neighbouring 16-byte pieces of the same sectors, and
        // measured fetch traffic is 3x lower this way than with groups spread 8 tickets apart (0.13 vs 0.36 GB for
        // the band at T=1024, NBatch=352)
        // wave -> role: the first HWAVES waves are the spine proper (spare == 0, hw = wave), the others its spare waves.
        // (Written as a division: with one spine per workgroup `spare` is 0 or 1, sg == ticket and lds_h == s_dyn, but the
        // compiler does not fold that, and the register allocation of the whole kernel follows from these few instructions --
        // folding them by hand changes the generated code from end to end.  The shipped code is kept instruction for instruction.)
        const int spare = wave / HWAVES, hw = wave % HWAVES;
        const int sg = ticket + spare;
        char* const lds_h = s_dyn + spare * LDS_HYBRID_PANEL;
        if (spare >= 1) {
            const int xw = wave - HWAVES;
            if (NFARW > 1 && wave >= NT / 64 - (NFARW - 1)) {
                // far waves 1 .. NFARW - 1 (they leave at once in launches that use fewer: far_role)
                if (!(DBGF(P) & 9u)) far_role<MODE>(P, ticket, s_dyn, 1 + wave - (NT / 64 - (NFARW - 1)));
            } else if (!(DBGF(P) & 2u) && xw < P.hybridPanelWaves) {
                // Spare waves stream tiles like the panel workgroups do (their stages lie behind the spines' LDS) -- but only
                // once the sweep is bound by the far field: during the first blocks the ring sets the pace and a streaming
                // wave on its CU only slows it down.  They wait until the (first) ring has taken row block hybridStart.
                {
                    const int* cons = (const int*)(s_dyn + LDS_CTL) + NRBUF;
                    int spins = 0;
                    while (lds_flag_load(cons + (P.hybridStart % RING)) < P.hybridStart + 1 && P.hybridStart < P.K &&
                           !(SEMICRF_PANEL_PROBES && (DBGF(P) & 8u))) {
                        __builtin_amdgcn_s_sleep(127);
                        if (spin_abort(P.ctrl, spins, SPIN_LIMIT_LDS, 10)) break;
                    }
                }
                panel_role<MODE, DIR, GRAD>(P, s_dyn + LDS_HYBRID_PANEL, xw, 1);
            } else if (MODE == 0 && DIR == 0 && !GRAD && P.pathPairs != nullptr && P.pathSpine && xw == P.hybridPanelWaves) {
                path_role(P);
            }
        } else if (sg >= P.nSpine) {
            // (never: sg == ticket here -- see above)
        } else if (hw < RING) {
            if (!(DBGF(P) & 8u)) {
                if (GRAD && P.bandWaves == 0) spine_role<MODE, DIR, GRAD, GRAD>(P, sg, hw, lds_h);
                else spine_role<MODE, DIR, GRAD, false>(P, sg, hw, lds_h);
            }
        } else if (hw < RING + 1) {
            if (!(DBGF(P) & 8u)) loader_role<DIR, GRAD>(P, sg, lds_h);
        } else {
            if (!(DBGF(P) & 9u)) far_role<MODE>(P, sg, lds_h, hw - (RING + 1));
        }
    } else {
        if (!(DBGF(P) & 2u) && wave < P.panelWaves)
            panel_role<MODE, DIR, GRAD>(P, s_dyn, wave, 0, P.taskBase > 0 ? (ticket - P.nSpine) * P.panelWaves + wave : -1);
        else if (GRAD && wave - P.panelWaves >= 0 && wave - P.panelWaves < P.zeroWaves) zero_role(P);
        else if (GRAD && wave - P.panelWaves - P.zeroWaves >= 0 && wave - P.panelWaves - P.zeroWaves < P.bandWaves) band_role<DIR>(P);
        else if (SEMICRF_BANDX && wave >= NT / 64 - P.copyWaves && (ticket - P.nSpine) % SEMICRF_BANDX_WGSTRIDE == 0) copy_role<DIR>(P);
        else if (MODE == 0 && DIR == 0 && !GRAD && P.pathPairs != nullptr && wave == P.panelWaves) path_role(P);
    }
    if (clk) { P.ts[602] = __builtin_readcyclecounter(); P.ts[603] = __builtin_amdgcn_s_memrealtime(); }
    if (P.selfclean) {
        // The last wave out puts the control words back (unless a wait timed out: the error word stays for the backtrack
        // kernel, the host has been told through g_host_abort and fills the workspace before its next use).  Counted per
        // workgroup (LDS first) and in a line of its own: one device-scope atomic per WAVE on the line of the ticket
        // counter -- 1500 idle waves leave at the very start -- delayed every workgroup's ticket: +21 us.
        int left = 0;
        if ((threadIdx.x & 63) == 0) left = atomicAdd(&s_exit, 1) + 1;
        left = __builtin_amdgcn_readfirstlane(left);
        if (left == NT / 64) {
            unsigned before = 0;
            if ((threadIdx.x & 63) == 0) before = atomicAdd(P.ctrl + CTRL_EXIT, 1u) + 1u;      // workgroups that left before this one
            before = (unsigned)__builtin_amdgcn_readfirstlane((int)before);
            if (before + 1u == gridDim.x &&
                __hip_atomic_load(P.ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == CTRL_INIT) {
                for (int i = threadIdx.x & 63; i < (int)CTRL_WORDS; i += 64)
                    __hip_atomic_store(P.ctrl + i, i == CTRL_GEN ? P.tag : CTRL_INIT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// in-sweep band copy: for which problems, and what it needs in the workspace (flags first: they are part of the launch's fill)
static bool band_in_sweep(int T, int B)
{
    const int K = (T + PB - 1) / PB;
    return SEMICRF_BANDX && B <= SEMICRF_BANDX_MAXB && K > SEMICRF_BANDX_K0 + FAR0;
}
static size_t band_flag_bytes(int T, int B)
{
    if (!band_in_sweep(T, B)) return 0;
    return align_up((size_t)((T + PB - 1) / PB + 2) * ((B + GP - 1) / GP) * 8 * sizeof(unsigned));      // [group][K + 2 row blocks][8]
}
static size_t band_copy_bytes(int T, int B)
{
    if (!band_in_sweep(T, B)) return 0;
    return align_up((size_t)((T + PB - 1) / PB) * ((B + GS - 1) / GS) * RING * TILE_BYTES);
}

constexpr size_t CTRL_BYTES = MAX_CHUNKS * CTRL_WORDS * sizeof(unsigned);

// Cache policy of the panels' cell stream (round 6).  Every cell is read once per sweep, so the stream was non-temporal from
// round 1 on (it must not evict the re-read u values from the L2s) -- right for the headline shape (0.74 GB per sweep), wrong in two
// cases, both measured with the sweeps in the order a step runs them (tools/nt_probe.py: forward, gradient sweep, decode on one
// tensor; profiles/r06_nt_policy.md):
//   * the score tensor fits the 256 MB memory-side cache next to what else the step touches (lower triangle <= SEMICRF_NT_MIN_MB):
//     the cells were just written by the scorer or read by the previous sweep of the step, and a non-temporal line is not kept
//     there.  Gradient sweep T=1024 x 88 244 -> 190 us, 691 x 180 210 -> 168, 691 x 192 147 -> 137, 1024 x 96 183 -> 168, 512 x 352 119 ->
//     114; forward 142 -> 132 / 116 -> 105 / 97 -> 96 / 128 -> 123 / 85 -> 85; decode level.  (With 1 GiB of unrelated traffic in front
//     of every step the forward sweep -- then the first reader of cold cells -- loses 5 - 10 us of it again; the gradient sweep keeps
//     its gain.)  Above ~250 MB ordinary loads lose everywhere an aligned tensor was tried (T=691 x 384: forward 129 -> 138,
//     gradient sweep 200 -> 239; T=1024 x 352: 194 -> 216, 331 -> 357).
//   * 4 NBatch is no multiple of 128 bytes (the reference's own chain counts: 88, 90, 360): every 32-chain piece straddles two lines
//     and the neighbour group's task fetches the same two -- rocprofv3 FETCH_SIZE at T=691: 635 MB for 360 chains (1.84 x the
//     algorithmic 345 MB) against 388 MB for 384 (1.05 x).  An ordinary line waits in the L2 / the memory-side cache for its
//     second reader: gradient sweep T=691 x 360 325 -> 269 us (278 -> 255 in a loop of gradient sweeps alone), T=2048 x 88 665 -> 583.
//     Only the gradient sweep: a loop of forward sweeps at T=691 x 360 -- the first reader of a tensor that does not fit the cache --
//     takes 132 us non-temporal and 145 with ordinary loads, the decode sweep 167 and 184.
// The marginals' stores stay non-temporal always (ordinary stores push the score tensor out from under the next sweep: decode
// 159 -> 168 at T=1024 x 88, 98 -> 112 at 512 x 352).
static bool cell_policy_nt(int T, int nb, int min_mb)
{
    const double mb = 4.0 * nb * ((double)T * (T + 1) / 2) / 1e6;       // the lower triangle this launch streams
    return mb >= (double)min_mb;
}

static int max_parts(int T)
{
    const int K = (T + PB - 1) / PB;
    return K > FAR0 ? nparts_of(K - 1 - FAR0) : 1;
}

// writes the exact zeros of the upper triangle (begin > end) of the dense gradient: row e, columns e+1..T-1
__global__ __launch_bounds__(256) void zero_upper_kernel(float* __restrict__ dScore, int T, int B)
{
    const int e = blockIdx.y;
    const size_t n = (size_t)(T - 1 - e) * B;                 // floats to clear in this row
    float* rowp = dScore + ((size_t)e * T + e + 1) * B;
    const size_t lead = (4 - (((uintptr_t)rowp >> 2) & 3)) & 3;          // floats up to 16-byte alignment
    const size_t head = lead < n ? lead : n;
    const size_t n4 = (n - head) / 4;
    float4* v = (float4*)(rowp + head);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
        v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) rowp[threadIdx.x] = 0.f;
        const size_t tail0 = head + n4 * 4;
        if (tail0 + threadIdx.x < n) rowp[tail0 + threadIdx.x] = 0.f;
    }
}

// the workspace fill (see launch_persist_sweep_impl for why it is not hipMemsetAsync)
__global__ __launch_bounds__(256) void fill_ff_kernel(v4u* __restrict__ p, size_t n16)
{
    const v4u e = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = e;
}

// exact zeros above the diagonal (begin > end) of a [T][T][B] tensor
void launch_zero_upper(float* X, int T, int B, hipStream_t stream)
{
    if (T < 2) return;
    int gx = (int)(((size_t)T * B / 4 + 255) / 256);
    if (gx > 8) gx = 8;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(zero_upper_kernel, dim3(gx, T - 1), dim3(256), 0, stream, X, T, B);
}

constexpr int MAX_DEVICES = 64;
static int current_device()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) dev = 0;
    return dev;
}
static int device_cus()
{
    static std::atomic<int> ncu[MAX_DEVICES];                    // 0: not asked yet (per device: a process may drive several)
    const int dev = current_device();
    int n = ncu[dev].load();
    if (n == 0) {
        int v = 0;
        n = 256;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        ncu[dev].store(n);
    }
    return n;
}

// The workspace of a sweep over (T, B), as byte offsets: the one statement of the layout (persist_workspace_bytes, the launcher's
// pointers and the fill all read it).  The control words of the chain chunks come first, at offset 0.
struct WsLayout {
    size_t ts;          // [2T] debug timestamps
    size_t farg;        // [max_parts][T][B] granules of far-field partials
    size_t ug;          // two u buffers of ug_bytes each: consecutive launches into a leased workspace alternate
    size_t ug_bytes;
    size_t pathg;       // [B] path-score granules (logProb as one launch)
    size_t band_flags;  // the in-sweep band copy's flag words (none: band_in_sweep)
    size_t band;        // ... and the spine-major copy itself: not filled, its flag words say what is valid
    size_t total;
    size_t fill() const { return band; }      // what a launch's 0xff fill covers
};
static WsLayout ws_layout(int T, int B)
{
    WsLayout L;
    L.ts = CTRL_BYTES;
    L.farg = L.ts + align_up((size_t)2 * T * sizeof(u64));
    L.ug = L.farg + (size_t)max_parts(T) * align_up((size_t)T * B * sizeof(u64));
    L.ug_bytes = align_up((size_t)T * B * sizeof(unsigned));
    L.pathg = L.ug + 2 * L.ug_bytes;
    L.band_flags = L.pathg + align_up((size_t)B * sizeof(u64));
    L.band = L.band_flags + band_flag_bytes(T, B);
    L.total = L.band + band_copy_bytes(T, B);
    return L;
}

size_t persist_workspace_bytes(int T, int B) { return ws_layout(T, B).total; }

// Even NBatch: the loader's 16-byte global->LDS loads and the panels' 16-byte loads need 8-byte aligned
// addresses (4-byte aligned ones, i.e. odd NBatch, return wrong data); chains past the end of the range are masked.
// (An odd NBatch runs too: the 16-byte accesses to four neighbouring chains are then only 4-byte aligned, which the
// global->LDS loads and the 16-byte stores take -- bit-identical results, 271 vs 184 us at T=1024, NBatch=351 / 352: every
// 128-byte piece straddles two lines -- where a padded copy of the tensor cost 1.0 ms.)
bool persist_supported(int T, int B)
{
    return B >= 2 && T >= 2 && T < 65535 && (long long)T * B * 64 < (1ll << 31) &&      // 32-bit buffer offsets
           (B + GS - 1) / GS <= MAX_CHUNKS * (device_cus() / 2 > 0 ? device_cus() / 2 : 1);      // chain chunks of at most half the CUs' worth of rings
}

static unsigned next_tag()
{
    static std::atomic<unsigned> counter{0};
    const unsigned lo = (counter.fetch_add(1) % 65534u) + 1u;   // 1..65534: never the workspace's fill pattern 0xffff
    return (lo << 16) | lo;                                      // both 16-bit halves nonzero
}

// Launch-geometry knobs of the development tools (tools/bench_sweep.py): the environment is read only by a library built
// with -DSEMICRF_DEBUG_BUILD=1 (once, at the first launch); the release library ignores it (-1 = the built-in choice).
struct Knobs { int hybrid_waves, hybrid_start, panel_waves, zero_waves, band_waves, nfarw; };
constexpr Knobs NO_KNOBS{-1, -1, -1, -1, -1, -1};
static Knobs read_knobs()
{
#if defined(SEMICRF_DEBUG_BUILD) && SEMICRF_DEBUG_BUILD
    auto get = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : -1; };
    return Knobs{get("SEMICRF_HYBRID_PANEL_WAVES"), get("SEMICRF_HYBRID_START"), get("SEMICRF_PANEL_WAVES"), get("SEMICRF_ZERO_WAVES"),
                 get("SEMICRF_BAND_WAVES"), get("SEMICRF_NFARW_RT")};
#else
    return NO_KNOBS;
#endif
}

// ---------------------------------------------------------------------------------------------
// launch plan: chain chunks, and per chunk the waves of every role and the policies
// ---------------------------------------------------------------------------------------------
// Chain chunks: at most half of the CUs host spines in one launch (every workgroup must be resident and the panels need the
// rest of the chip).
struct Chunks { int n, perChunk; };      // launches of the call, spines per launch
static Chunks plan_chunks(int B, int ncu)
{
    const int nSpineTotal = (B + GS - 1) / GS;
    const int maxSpine = ncu / 2 > 0 ? ncu / 2 : 1;          // (more rings per launch instead of a second chunk: no faster, 438 vs 445 us at NBatch=600)
    Chunks C;
    C.n = (nSpineTotal + maxSpine - 1) / maxSpine;
    // chunks start on a panel-group boundary (32 chains = 128 bytes): a chunk that starts in the middle of a line makes every
    // 128-byte piece of its panels straddle two (T=1024, NBatch=600 as 2 x 300 chains: 488 us forward, 1680 us gradient sweep)
    int perChunk = C.n > 0 ? (nSpineTotal + C.n - 1) / C.n : 0;
    perChunk = (perChunk + GP / GS - 1) / (GP / GS) * (GP / GS);
    if (perChunk > maxSpine) perChunk = maxSpine / (GP / GS) * (GP / GS) > 0 ? maxSpine / (GP / GS) * (GP / GS) : maxSpine;
    C.perChunk = perChunk;
    return C;
}

// What a call asks of its launches, as far as the plan depends on it
struct SweepKind {
    bool grad;            // the gradient sweep
    bool keep_upper;      // ... whose caller has the zero upper triangle already
    bool want_fold;       // ... and hands in the forward call's path table
};
// The geometry fields of SweepParams for chain chunk ci, and what the launcher needs beside them
struct ChunkPlan {
    int c0, c1;                                    // c0 >= c1: no such chunk
    int nSpine, nPanelGroups, nTasks, taskBase;
    int panelWaves, hybridPanelWaves, hybridStart, zeroWaves, bandWaves, copyWaves;
    int gradLazyShort, nfarw, cellNT, gradNT, pathSpine;
    bool zeroKernel;                               // the zero upper triangle needs its own kernel (in front of this launch)
    bool pathFold;                                 // the launch applies the path's own terms (SweepParams::ptab)
    bool bandCopy;                                 // the launch copies its band (SweepParams::band, bandFlags, bandK0)
    int grid;
};
static ChunkPlan plan_chunk(int T, int B, const Chunks& C, int ci, const SweepKind& kind, int ncu, const Knobs& knobs)
{
    ChunkPlan Q = {};
    const int K = (T + PB - 1) / PB;
    const bool grad = kind.grad;
    Q.c0 = ci * C.perChunk * GS;
    Q.c1 = Q.c0 + C.perChunk * GS < B ? Q.c0 + C.perChunk * GS : B;
    if (Q.c0 >= Q.c1) return Q;
    const int nb = Q.c1 - Q.c0;
    Q.nSpine = (nb + GS - 1) / GS;
    Q.nPanelGroups = (nb + GP - 1) / GP;
    // panel tasks per chain group: block k = FAR0 + q has nparts_of(q) column parts, each split in 4 row quarters
    long long ntask = 0;
    for (int q = 0; q < K - FAR0; ++q) ntask += nparts_of(q);
    ntask *= 4;
    Q.nTasks = (int)(ntask * Q.nPanelGroups);
    // Panel waves.  Every CU streams (HBM bandwidth is limited per CU by the misses it can keep in flight):
    // a spine workgroup carries NT/64 - RING panel waves, the other workgroups `panelWaves`.  More waves
    // mean longer memory queues, and the spine's band loads and hand-offs wait in the same queues; the far
    // field grows with T^2 and the spine's chain with T, so longer sequences get more panel waves, and
    // the gradient sweep (which also stores a tile per tile loaded) a few more.
    int nPanelWG = ncu - Q.nSpine;
    if (nPanelWG < 0) nPanelWG = 0;
    // The spine workgroups' two spare waves stream tiles too, from row block hybridStart on: while the ring sets
    // the pace (the first third of the blocks) a streaming wave on its CU only slows it down; afterwards the sweep is
    // bound by the far field and every CU helps.  Forward, T=1024: 205 us (start at 24-32) vs 214 (from the start)
    // vs 217 (never); T=691, NBatch=360: 158 vs 177 vs 173; T=2048: 651 vs 677 (from the start) vs 788 (never).
    // The gradient sweep is bandwidth-bound almost from the start.
    int hpw = HPW_MAX > 0 ? HPW_MAX : 0;
    if (knobs.hybrid_waves >= 0 && knobs.hybrid_waves <= HPW_MAX) hpw = knobs.hybrid_waves;
    // (round 2, after the panel math got cheaper: later is better -- T=691: 143-150 us from block 28 vs 160 from 16;
    // T=512: 89 from 20 vs 92 from 12; T=1024: 185 from 40 vs 188 from 32; T=2048: 583-598 from 32-48 vs 602-617 from 64-80)
    int hstart = grad ? SEMICRF_GRAD_HSTART : K * 5 / 8;
    hstart = hstart < 8 ? 8 : (hstart > 40 ? 40 : hstart);
    if (knobs.hybrid_start >= 0) hstart = knobs.hybrid_start;
    Q.hybridStart = hstart;
    Q.hybridPanelWaves = hpw;
    // Five panel waves per workgroup where the sweep is bound by the far field's throughput (long sequences, many
    // chains: T=2048, NBatch=352 forward 612 -> 562 us, gradient sweep 1620 -> 1550; T=1024: 185 -> 178), four where the
    // hand-off chain sets the pace (T=691, 90 chains: 103 vs 115 us with five; T=1024, 88 chains: 151 vs 160).
    // tools/stream_probe.hip shows the same per CU: with the panels' math and task boundaries 4 waves x 3 stages stream
    // 22.7 GB/s, 5 x 3 24.8, 6 x 2 29.6, 8 x 2 35.3 -- more waves, not deeper stages, hide a wave's math and boundaries.
    int pw = (T >= 1024 && nb >= 256) ? PW_MAX : (PW_MAX < 4 ? PW_MAX : 4);
    if (knobs.panel_waves > 0) pw = knobs.panel_waves;
    if (pw < 1) pw = 1;
    if (pw > PW_MAX) pw = PW_MAX;
    Q.panelWaves = pw;
    // the zero upper triangle of the gradient: by spare waves of the first chunk's panel workgroups, or (no
    // panel workgroups: short sequences) by its own kernel
    int zw = 0;
    if (grad && ci == 0 && !kind.keep_upper) {
        zw = 2;
        if (knobs.zero_waves >= 0) zw = knobs.zero_waves;
        if (zw > NT / 64 - pw) zw = NT / 64 - pw;
        if (nPanelWG <= 0 || Q.nTasks == 0) zw = 0;
        Q.zeroKernel = zw == 0 && T > 1;
    }
    Q.zeroWaves = zw;
    // the band's marginals: three spare waves of every panel workgroup (none: the ring waves store them).  One / two / three /
    // four / five waves: 446 / 355 / 344 / 354 / 363 us at T=1024 x 352, 272 / 205 / 184-189 / 189 / 196 at T=691 x 384 (one box).
    int bw = 0;
    if (grad && nPanelWG > 0 && Q.nTasks > 0) {
        bw = 3;
        if (knobs.band_waves >= 0) bw = knobs.band_waves;
        if (bw > NT / 64 - pw - zw) bw = NT / 64 - pw - zw;
    }
    Q.bandWaves = bw;
    // The path's own terms inside this launch: where every cell has ONE writer that knows its row -- band waves for the band (a
    // ring that stores the band itself does so in the middle of its dependent chain: short sequences keep the scatter), panels
    // for the far field -- and the whole batch is one launch.
    Q.pathFold = grad && kind.want_fold && bw > 0 && C.n == 1;
    Q.gradLazyShort = nb < 256 ? 1 : 0;
    // Two far waves taking turns halve the far wave's share of a block's period (one device-scope round trip per block and wave):
    // worth 3 - 4 % where the forward / decode sweeps are hand-off-bound, i.e. with few chains; with many chains, and in the gradient
    // sweep, the second poller costs the fabric more than it returns (T=1024 x 352: 178 vs 176 us, gradient sweep 347 vs 337)
    Q.nfarw = (!grad && nb <= SEMICRF_NFARW2_MAXB && T >= SEMICRF_NFARW2_MINT && NFARW >= 2) ? 2 : 1;
    if (knobs.nfarw >= 1 && knobs.nfarw <= NFARW) Q.nfarw = knobs.nfarw;
    Q.cellNT = cell_policy_nt(T, B, SEMICRF_NT_MIN_MB) ? 1 : 0;          // (by the whole batch: chain chunks stream the same tensor)
    if (grad && B % 32 != 0) Q.cellNT = 0;                                // straddling pieces: the line waits for its second reader
    Q.gradNT = cell_policy_nt(T, B, SEMICRF_GRAD_NT_MIN_MB) ? 1 : 0;
    if (Q.nTasks == 0) nPanelWG = 0;
    Q.pathSpine = nPanelWG == 0 ? 1 : 0;        // no panel workgroups (short sequences): the spine workgroups' spare wave
    // the band as a spine-major copy, made by spare waves of the panel workgroups while the sweep runs
    // (not in the gradient sweep: neutral at 88 - 96 chains, 3 % slower at 176 -- its stores leave the copy no quiet fabric)
    Q.bandCopy = band_in_sweep(T, B) && !grad && C.n == 1 && nPanelWG > 0 && NT / 64 - pw - zw - bw - 1 >= SEMICRF_BANDX_WAVES;
    Q.copyWaves = Q.bandCopy ? SEMICRF_BANDX_WAVES : 0;
    Q.grid = Q.nSpine + nPanelWG;
    // the panel workgroups' waves know their first task (the first draws of ~700 waves all hit one counter at the start)
    Q.taskBase = nPanelWG * Q.panelWaves;
    if (Q.taskBase > Q.nTasks) Q.taskBase = Q.nTasks;
    return Q;
}

struct GradArgs {
    const float* vfwd; const float* logZ; const float* gout; float* dScore; float* dNoise; int gstride; float gscale;
    int keep_upper;       // the cells begin > end of dScore hold zeros already (SEMICRF_GRAD_UPPER_IS_ZERO): not written
    float noise_add;      // dNoise += noise_add * gout on every gap (logProb's backward), 0: nothing
    const int* ptab;      // the forward call's path table (logProb's backward), or nullptr
    int* path_folded;     // ... set to 1 when the launch applied the path's own terms (the caller then skips its scatter)
};
struct PathArgs { const int* pairs; const int* offsets; int K; float* out; int* ptab; };

template <int MODE, int DIR, bool GRAD>
static void launch_one(const SweepParams& P, int grid, hipStream_t stream)
{
    static std::atomic<bool> attr_set[MAX_DEVICES];              // the attribute is per device
    const int dev = current_device();
    if (!attr_set[dev].load()) {
        (void)hipFuncSetAttribute((const void*)persist_sweep_kernel<MODE, DIR, GRAD>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, LDS_DYN_BYTES);
        attr_set[dev].store(true);
    }
    hipLaunchKernelGGL((persist_sweep_kernel<MODE, DIR, GRAD>), dim3(grid), dim3(NT), LDS_DYN_BYTES, stream, P);
}

// mode 0 = LSE, 1 = MAX.  ws must hold persist_workspace_bytes().  Enqueues a fill + one kernel per chain chunk.
// lease: 0 = ordinary workspace (filled here, every launch); 1 = leased, not known to be clean (filled here, the launch
// cleans up after itself); 2 = leased and left clean by the previous launch (no fill).  lease_tag: the workspace's own
// launch count (consecutive launches in one workspace must not share a granule tag), 0 = the process-wide counter.
static int launch_persist_sweep_impl(int mode, int dir, const float* score, const float* noise, int T, int B,
                                     float* u_out, float* last_out, int* code, void* ws, hipStream_t stream,
                                     const GradArgs* grad, int lease, unsigned lease_tag, const PathArgs* path = nullptr)
{
    SweepParams P;
    P.pathPairs = nullptr; P.pathOffsets = nullptr; P.pathK = 0; P.pathOut = nullptr; P.pathg = nullptr; P.pathSpine = 0; P.noiseAdd = 0.0f;
    P.ptabOut = nullptr; P.ptab = nullptr;
    P.vfwd = nullptr; P.logZ = nullptr; P.gout = nullptr; P.dScore = nullptr; P.dNoise = nullptr; P.gstride = 1; P.gscale = 1.0f;
    if (grad) {
        P.vfwd = grad->vfwd; P.logZ = grad->logZ; P.gout = grad->gout; P.dScore = grad->dScore; P.dNoise = grad->dNoise;
        P.gstride = grad->gstride; P.gscale = grad->gscale; P.noiseAdd = grad->noise_add;
    }
    P.score = score; P.noise = noise; P.T = T; P.B = B; P.K = (T + PB - 1) / PB;
    P.band = nullptr; P.bandFlags = nullptr; P.bandSpines = (B + GS - 1) / GS; P.bandGroups = (B + GP - 1) / GP; P.bandK0 = 0; P.copyWaves = 0;
    P.tag = lease_tag ? (lease_tag % 65534u) + 1u : next_tag();
    P.dbg = 0u;
    P.selfclean = 0;
#if SEMICRF_PANEL_PROBES
    // timing ablations (results are wrong when set): only the probe build reads them
    if (const char* dbg = getenv("SEMICRF_DEBUG_FLAGS")) P.dbg = (unsigned)atoi(dbg);
    if (SEMICRF_CT_DBG >= 0) P.dbg = (unsigned)SEMICRF_CT_DBG;
#endif
    // ---- the workspace ------------------------------------------------------------------------------------------------------
    const WsLayout L = ws_layout(T, B);
    char* w = (char*)ws;
    P.ts = (u64*)(w + L.ts);
    P.farg = (u64*)(w + L.farg);
    // leased workspaces: launches alternate between the two u buffers, each puts the other one back to U_EMPTY (see the kernel)
    const unsigned upar = lease != 0 ? (lease_tag & 1u) : 0u;
    P.ug = (unsigned*)(w + L.ug + upar * L.ug_bytes);
    P.ug_other = nullptr;
    if (path && mode == 0 && dir == 0 && !grad) {
        // (offsets is never null here; pairs may be when K == 0 -- the role only looks at pairs[k] for k < K)
        P.pathPairs = path->pairs ? path->pairs : path->offsets; P.pathOffsets = path->offsets; P.pathK = path->K; P.pathOut = path->out;
        P.ptabOut = path->ptab;
        P.pathg = (u64*)(w + L.pathg);
    }
    P.u_out = u_out; P.last_out = last_out; P.code = code;
    // ---- fill and lease -----------------------------------------------------------------------------------------------------
    // ONE fill: every word of the workspace starts as 0xffffffff -- u reads U_EMPTY, far-field granules carry a tag no
    // launch uses, the counters return 0 after their first increment, the error word reads CTRL_INIT
    // (probe build, flag 512: the u values of the previous launch in the same workspace stay -- panels alone on real values)
    // (the band copy's scratch is not filled: its flag words, which are, say what is valid)
    const size_t fill_bytes = (SEMICRF_PANEL_PROBES && (P.dbg & 512u)) ? L.ug : L.fill();
    if (P.dbg != 0u) lease = lease ? 1 : 0;                       // timing ablations leave anything behind
    // (a kernel of our own, not hipMemsetAsync: as fast, and a captured memset node of this size breaks the SECOND replay of an
    // instantiated HIP graph -- wrong results or a memory fault -- while this kernel replays correctly)
    if (lease != 2) hipLaunchKernelGGL(fill_ff_kernel, dim3(1024), dim3(256), 0, stream, (v4u*)ws, (fill_bytes + 15) / 16);
    P.selfclean = lease != 0 && P.dbg == 0u;
    if (P.selfclean) P.ug_other = (unsigned*)(w + L.ug + (1u - upar) * L.ug_bytes);
    // what ctrl[CTRL_GEN] must read when the kernel starts: the previous launch's tag (a clean lease) or the fill
    P.expect_gen = (lease == 2 && P.selfclean) ? ((lease_tag - 1u) % 65534u) + 1u : CTRL_INIT;
    // ---- plan and launch, chunk by chunk --------------------------------------------------------------------------------------
    static const Knobs knobs = read_knobs();
    const int ncu = device_cus();
    const Chunks C = plan_chunks(B, ncu);
    if (C.n > MAX_CHUNKS) return 1;
    const SweepKind kind{grad != nullptr, grad && grad->keep_upper, grad && grad->ptab != nullptr};
    for (int ci = 0; ci < C.n; ++ci) {
        const ChunkPlan Q = plan_chunk(T, B, C, ci, kind, ncu, knobs);
        if (Q.c0 >= Q.c1) break;
        P.c0 = Q.c0; P.c1 = Q.c1; P.nSpine = Q.nSpine; P.nPanelGroups = Q.nPanelGroups; P.nTasks = Q.nTasks; P.taskBase = Q.taskBase;
        P.panelWaves = Q.panelWaves; P.hybridPanelWaves = Q.hybridPanelWaves; P.hybridStart = Q.hybridStart;
        P.zeroWaves = Q.zeroWaves; P.bandWaves = Q.bandWaves; P.gradLazyShort = Q.gradLazyShort; P.nfarw = Q.nfarw;
        P.cellNT = Q.cellNT; P.gradNT = Q.gradNT; P.pathSpine = Q.pathSpine;
        P.ctrl = (unsigned*)w + (size_t)ci * CTRL_WORDS;
        if (Q.zeroKernel) launch_zero_upper(grad->dScore, T, B, stream);
        P.ptab = Q.pathFold ? grad->ptab : nullptr;
        if (grad && grad->path_folded) *grad->path_folded = Q.pathFold ? 1 : 0;
        P.band = nullptr; P.copyWaves = Q.copyWaves;
        if (Q.bandCopy) {
            P.bandFlags = (unsigned*)(w + L.band_flags);
            P.band = (float*)(w + L.band);
            P.bandK0 = SEMICRF_BANDX_K0;
        }
        if (grad) launch_one<0, 1, true>(P, Q.grid, stream);
        else if (mode == 0 && dir == 0) launch_one<0, 0, false>(P, Q.grid, stream);
        else if (mode == 0 && dir == 1) launch_one<0, 1, false>(P, Q.grid, stream);
        else if (mode == 1 && dir == 0) launch_one<1, 0, false>(P, Q.grid, stream);
        else launch_one<1, 1, false>(P, Q.grid, stream);
    }
    return 0;
}


int launch_persist_sweep(int mode, int dir, const float* score, const float* noise, int T, int B, float* u_out,
                         float* last_out, int* code, void* ws, hipStream_t stream, int lease, unsigned lease_tag)
{
    return launch_persist_sweep_impl(mode, dir, score, noise, T, B, u_out, last_out, code, ws, stream, nullptr, lease, lease_tag);
}

// logZ and logProb = path - logZ in one launch (the path scores by spare waves while the sweep runs)
int launch_persist_logprob_fwd(const float* score, const float* noise, int T, int B, float* u_out, float* logZ, const int* pairs,
                               int K, const int* offsets, float* logProb, void* ws, hipStream_t stream, int lease, unsigned lease_tag, int* ptab)
{
    const PathArgs pa{pairs, offsets, K, logProb, ptab};
    return launch_persist_sweep_impl(0, 0, score, noise, T, B, u_out, logZ, nullptr, ws, stream, nullptr, lease, lease_tag, &pa);
}

// Fused backward: beta sweep + marginals (dScore fully written incl. the zero upper triangle, dNoise).
int launch_persist_logz_bwd(const float* score, const float* noise, const float* v, const float* logZ,
                            const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out, void* ws,
                            hipStream_t stream, int lease, unsigned lease_tag, int gstride, float gscale, int keep_upper, float noise_add,
                            const int* ptab, int* path_folded)
{
    if (path_folded) *path_folded = 0;
    GradArgs ga{v, logZ, gout, dScore, dNoise, gstride, gscale, keep_upper, noise_add, ptab, path_folded};
    return launch_persist_sweep_impl(0, 1, score, noise, T, B, q_out, nullptr, nullptr, ws, stream, &ga, lease, lease_tag);
}

// Can a gradient sweep of this shape apply the path's own terms (SweepParams::ptab)?  The launcher's own plan, asked before any
// launch and without a workspace, for the callers that decide up front whether to ask the forward call for a table.
int persist_path_fold_possible(int T, int B)
{
    // (an odd batch keeps the scatter: its 16-byte pieces straddle lines and it is a rare shape -- nothing here is tuned for it)
    if (B % 2 != 0) return 0;
    const int ncu = device_cus();
    const Chunks C = plan_chunks(B, ncu);
    if (C.n != 1) return 0;
    return plan_chunk(T, B, C, 0, SweepKind{true, false, true}, ncu, NO_KNOBS).pathFold ? 1 : 0;
}

// host-side view of the workgroup -> role map (tests/test_abi.py checks that it is a permutation for every launch shape)
int persist_wg_ticket(int nSpine, int grid, int b) { return wg_ticket(nSpine, grid, b); }
int persist_spine_wgs_per_group() { return GP / GS; }

// the error word of every chain chunk of a sweep launched into `pws` (0xffffffff = no wait timed out)
const unsigned* persist_error_words(void* pws, int* n, int* stride)
{
    *n = MAX_CHUNKS; *stride = (int)CTRL_WORDS;
    return (const unsigned*)pws + 1;
}

// Tell the sweep kernels of the current device where the host's abort word lives (pinned, mapped memory).  Synchronises.
int persist_set_host_abort_word(unsigned* devptr)
{
    static std::atomic<bool> done[MAX_DEVICES];
    const int dev = current_device();
    if (done[dev].load()) return 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_host_abort), &devptr, sizeof(devptr)) != hipSuccess) return 1;
    done[dev].store(true);
    return 0;
}

int read_and_clear_device_status()
{
    unsigned v = 0, z = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_dev_status), sizeof(v)) != hipSuccess) return -1;
    if (v != 0 && hipMemcpyToSymbol(HIP_SYMBOL(g_dev_status), &z, sizeof(z)) != hipSuccess) return -1;
    return (int)v;
}

}  // namespace semicrf
