#pragma once
// persist_common.h -- what every role of the persistent sweep (persist.hip) shares: the launch's parameters and control words, the
// hand-off primitives, the accumulators and the bounded waits.
//
// Hand-offs carry their own flag -- u: a float that reads U_EMPTY until published; far-field partials: 8-byte {tag, value}
// granules -- written with relaxed agent-scope atomic stores and polled with tagged loads (no fences, placement independent).
// Every workgroup of a launch is resident (one per CU), every spin is bounded and raises the error word instead of hanging.
#include "common.h"
#include "persist_tuning.h"

namespace semicrf {

constexpr int PB = 16;             // positions per block
constexpr int RING = SEMICRF_RING; // waves per ring; band = RING-1 off-diagonal blocks + the diagonal block
constexpr int FAR0 = RING;         // first block with a far field of its own; the newest far tile of block k is k - FAR0
constexpr int RS = 4;              // chains per ring (one per lane)
constexpr int GS = RS;              // chains per spine workgroup
constexpr int GP = 32;             // chains per panel task (4 per lane)
constexpr int TPT = SEMICRF_TPT;   // tiles (column blocks) per panel task
// Parts of a block with far tiles 0..q: FULL parts of TPT tiles at fixed columns, then the LAST part, which ends with the
// newest tile and is at least LEADT tiles long (when the block has that many): every full part lies LEADT tiles or more
// behind the newest one, i.e. all of its columns are published LEADT + RING blocks before its result is needed.
constexpr int LEADT = SEMICRF_LEADT;
__host__ __device__ inline int nfull_of(int q) { return q + 1 - LEADT >= 0 ? (q + 1 - LEADT) / TPT : 0; }
__host__ __device__ inline int nparts_of(int q) { return nfull_of(q) + 1; }
__host__ __device__ inline void part_tiles(int q, int part, int& m0, int& m1)
{
    m0 = part * TPT;
    m1 = part < nfull_of(q) ? m0 + TPT : q + 1;
}
constexpr int NT = SEMICRF_NT;     // threads per workgroup (10 waves: a spine workgroup = 4 ring + loader + far + 4 spare waves)
constexpr int MAX_CHUNKS = 16;     // chain chunks (launches) per call
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;
constexpr int SPIN_LIMIT = 1 << 20;       // global-memory polls (with s_sleep): ~0.3 s
constexpr int SPIN_LIMIT_LDS = 1 << 24;   // LDS polls (s_sleep 1): ~0.5 s
// Panel accumulators (reference M, sum S of exp2(t - M)).  u grows by ~45 log2 units per tile of 16 positions on N(0,1)
// scores, so the old rule -- "move M when a term exceeds M + 64, to exactly that term" -- moved every accumulator every
// 1.4 tiles, each at its own time; the test is a wave-wide __any over 32 chains x 8 columns, so the slow path ran on EVERY
// tile and cost as much as the accumulation itself (a tile of real values took 1.5 us, one of NaNs 0.9).  Now: M is an
// integer placed RESC_LIFT ABOVE the largest term seen when it is (re)set -- fp32 still holds every term within 2^-24 of
// that one -- the slow path is entered when a term exceeds M + RESC_HI, and it then moves every accumulator of the wave
// that is within RESC_EARLY of that limit, so that the chains stay in step: one visit every ~4 tiles.  A move is exact: S
// is scaled by a power of two (ldexp), no exponential.  Bounds: S <= 32 terms x 2^RESC_HI, 8 such in the final reduction.
constexpr float RESC_LIFT = 96.0f, RESC_HI = 108.0f, RESC_EARLY = 56.0f;
constexpr unsigned CTRL_INIT = 0xffffffffu;  // initial value of every workspace word (one 0xff fill per launch)
constexpr unsigned U_EMPTY = 0xffffffffu;  // not-yet-published u (a NaN pattern the spine never stores): the value is its own flag

// control words of a launch (all start at 0xffffffff).  Separate 128-byte lines: counters that take atomics must
// not share a line with words that are polled (hundreds of idle waves reading a line that others update atomically
// slow every dequeue down to tens of microseconds).
constexpr size_t CTRL_WORDS = 256;   // control words per chain chunk
constexpr int CTRL_EXIT = 64;         // [64]: workgroups that have left (leased workspaces: the last one resets the control words)
constexpr int CTRL_COPYQ = 192;       // [192]: band copy task queue head (a line of its own)
constexpr int CTRL_PATHQ = 160;       // [160]: path task queue head (a line of its own)
constexpr int CTRL_GEN = 96;          // [96]: leased workspaces: the tag of the launch that last cleaned up here (CTRL_INIT after a fill);
                                      // every workgroup of the next launch compares it with what the host expects (error 13)

typedef unsigned long long u64;
typedef unsigned v4u __attribute__((ext_vector_type(4)));
typedef unsigned v4u_a4 __attribute__((ext_vector_type(4), aligned(4)));      // rows of odd multiples of 8 bytes
template <int V>
struct IC { static constexpr int value = V; };

#define DBGF(P) (SEMICRF_CT_DBG >= 0 ? (unsigned)SEMICRF_CT_DBG : (P).dbg)
struct SweepParams {
    const float* score;
    const float* noise;
    int T, B, K;
    int c0, c1;            // chains [c0, c1) of the batch are handled by this launch
    int nSpine, nPanelGroups;
    int nTasks;            // panel tasks (k ascending, then column part, then chain group, then row quarter)
    int taskBase;          // tasks [0, taskBase) are the first tasks of the panel workgroups' waves (no draw); the queue hands out the rest
    int panelWaves;        // waves per non-spine workgroup that work as panels (the rest exit at once)
    int hybridPanelWaves;  // panel waves of a spine workgroup (0..2)
    int hybridStart;       // ... which start once the ring has reached this row block
    int zeroWaves;         // GRAD: waves per panel workgroup that write the zero upper triangle of dScore (0: separate kernel)
    unsigned tag;          // nonzero launch epoch
    int selfclean;         // leased workspace (semicrf_workspace_register): the launch leaves u and its control words as the fill would
    unsigned expect_gen;   // ... and finds ctrl[CTRL_GEN] == expect_gen: the previous launch into this workspace was the one the host
                           // counted, and it finished its clean-up (otherwise: error 13, outputs poisoned)
    unsigned dbg;          // SEMICRF_DEBUG_FLAGS (timing experiments only; results are wrong when set):
                           // 1 spine ignores far partials, 2 panels exit at once, 4 panels do not wait for u,
                           // 8 spine exits at once, 16 spine 0 records per-block timestamps,
                           // 32 panels only stream their cells (no granules, no math)
    unsigned* ctrl;        // [1] error, [2] panel task queue head, [3] zero-fill row queue head, [64] workgroups that have left (leases)
    u64* ts;               // [2T] debug timestamps of spine 0, ring 0 (dbg & 16)
    unsigned* ug;          // [T][B] u as float bits (position-major: index p*B + c); U_EMPTY until the spine publishes it
    unsigned* ug_other;    // leased workspaces: the u buffer of the PREVIOUS launch into this workspace (the two alternate); this launch
                           // puts it back to U_EMPTY, at its start and off every critical path (nullptr: nothing to clean)
    int gradLazyShort;     // GRAD: panel waves poll for a tile that is not their task's newest every ~0.5 us instead of every ~4
    int bandWaves;         // GRAD: waves per panel workgroup that write the band's marginals (band_role); 0: the ring waves do
    u64* farg;             // [parts][T][B] granules of far-field partials (part = column range of TPT tiles)
    float* u_out;          // [T][B] by FRAME (natural-log units for LSE) or nullptr
    float* last_out;       // [B] value at the last position (logZ for DIR 0) or nullptr
    int* code;             // MAX: [B][T] backtrack codes by frame
    // GRAD (LSE, DIR 1 only): marginals are a by-product of the beta sweep (NeuralSemiCRFInterval.py:424-447, :469-472)
    const float* vfwd;     // [T][B] alpha values by frame (natural log)
    const float* logZ;     // [B]
    const float* gout;     // upstream gradient of chain c: gscale * gout[c * gstride] (gstride 0: one value for every chain)
    int gstride;
    float gscale;
    float* dScore;         // [T][T][B]: lower triangle + diagonal written here (the upper triangle by zero_upper_kernel)
    float* dNoise;         // [T-1][B]
    // logProb as ONE launch (round 5; LSE, DIR 0 only): a spare wave of the panel workgroups computes the path score of every chain
    // (path_role, pathscore.h) while the sweep runs and leaves it as a {tag, value} granule; the ring wave that finalises the last
    // position takes it and writes logProb = path - logZ (NeuralSemiCRFInterval.py:587-588)
    const int* pathPairs;  // [K][2] (begin, end) or nullptr: no path role
    const int* pathOffsets;// [B+1]
    int pathK;
    int pathSpine;         // the spine workgroups' spare wave takes path tasks too (launches without panel workgroups)
    float* pathOut;        // [B] logProb
    u64* pathg;            // [B] granules (workspace)
    float noiseAdd;        // GRAD: dNoise gets noiseAdd * gout[c] on top of the marginal (d cum[T-1] / d noise of the path score), 0: nothing
    // logProb's backward as ONE launch: the forward's path role also leaves the path as a table (pathscore.h: path_table_wave), and
    // every writer of the gradient sweep applies the path's own terms to what it stores -- + noiseAdd * gout[c] (the path score's
    // weight) on the cell of a path interval, the same with a minus on a covered gap -- as the scatter kernel's atomics did
    // afterwards (evalpath.hip), rounding for rounding
    int* ptabOut;          // forward: [T][B] table to fill, or nullptr
    const int* ptab;       // GRAD: [T][B] table of the forward call, or nullptr: the caller scatters
    float* band;           // SEMICRF_BANDX: [K][bandSpines][RING][16 columns][16 rows][4 chains]: the band, spine-major (workspace), or nullptr
    unsigned* bandFlags;   // ... [32-chain groups][K + 2][8]: {launch tag, row block} once tile t of (row block, group) has been copied
    int bandSpines;        // ... spines of the whole batch (the copy is indexed by the batch's spine number)
    int bandGroups;        // ... 32-chain groups of the whole batch
    int bandK0;            // ... row blocks < bandK0 are loaded from the score tensor itself
    int copyWaves;         // ... waves per panel workgroup that copy (copy_role)
    int cellNT;            // 1: the panels stream their cells non-temporal (large problems); 0: ordinary loads (see cell_policy_nt)
    int gradNT;            // GRAD: likewise for the marginals' stores
    int nfarw;             // far waves of a spine that take turns on the blocks (1 .. NFARW)
};

// ---------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float flog2(float x) { return __builtin_amdgcn_logf(x); }

__device__ __forceinline__ u64 make_granule(unsigned tag, float v)
{
    return ((u64)tag << 32) | (u64)__float_as_uint(v);
}
__device__ __forceinline__ u64 make_granule_key(unsigned tag, float v, int key)
{
    return ((u64)(((tag & 0xffffu) << 16) | ((unsigned)key & 0xffffu)) << 32) | (u64)__float_as_uint(v);
}
__device__ __forceinline__ void store_granule(u64* p, u64 g)
{
    __hip_atomic_store(p, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 load_granule(const u64* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A field of the kernel's argument, read again where it is needed instead of being carried in registers from the kernel's start
// (the panels have neither a vector nor a scalar register to spare across their tile loop; the empty asm keeps the load in place)
template <typename Tp>
__device__ __forceinline__ Tp kernarg_again(size_t off)
{
    typedef __attribute__((address_space(4))) const char ka_t;
    ka_t* ka = (ka_t*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return *(__attribute__((address_space(4))) const Tp*)(ka + off);
}

template <int DIR>
__device__ __forceinline__ int frame_of(int p, int T) { return DIR == 0 ? p : T - 1 - p; }

// element offset (without the chain) of cell(pi, pj), pj < pi, in score [T][T][B]
template <int DIR>
__device__ __forceinline__ size_t cell_index(int pi, int pj, int T)
{
    return DIR == 0 ? (size_t)pi * T + pj : (size_t)(T - 1 - pj) * T + (T - 1 - pi);
}
// noise row between positions p-1 and p
template <int DIR>
__device__ __forceinline__ int gap_of(int p, int T) { return DIR == 0 ? p - 1 : T - 1 - p; }

// log2-domain accumulator, exact running max, one exp per push: value = M + log2(S); empty = (-inf, 0)
__device__ __forceinline__ void acc_push1(float& M, float& S, float t)
{
    const float d = t - M;                       // M = -inf -> +inf
    const float e = fexp2(-fabsf(d));
    S = d > 0.0f ? fmaf(S, e, 1.0f) : S + e;
    M = fmaxf(M, t);
}
__device__ __forceinline__ void acc_merge(float& M, float& S, float M2, float S2)
{
    if (S2 == 0.0f) return;
    if (M2 > M) {
        S = S * fexp2(M - M2) + S2;   // M = -inf -> S*0 (S = 0)
        M = M2;
    } else {
        S += S2 * fexp2(M2 - M);
    }
}
// (max, key) push for candidates that arrive in position order within one accumulator: frames ascend with the
// positions in DIR 0 (the first maximum stays) and descend in DIR 1 (a later equal candidate has the smaller
// frame and wins) -- one compare instead of the general three (the reference keeps the smallest frame index)
template <int DIR>
__device__ __forceinline__ void max_push_seq(float& best, int& key, float t, int k)
{
    const bool take = DIR == 0 ? t > best : t >= best;
    best = take ? t : best;
    key = take ? k : key;
}
// softplus in log2 units: log2(1 + 2^(x*log2e)), linear above the reference's threshold (20)
__device__ __forceinline__ float softplus2(float x)
{
    const float x2 = x * LOG2E;
    return x > 20.0f ? x2 : flog2(1.0f + fexp2(x2));
}

// sticky device-side status word (0 = fine); read and cleared by semicrf_debug_device_status()
__device__ unsigned g_dev_status = 0;
// set (LDS) by any wave of this workgroup that gave up on a bounded wait or saw another one give up: a spine workgroup
// whose flag is up poisons its final outputs with NaN (every wrong result is preceded by a timed-out wait in the
// workgroup of the affected chains -- a missing far partial, band row or ring entry), so that a caller notices without
// reading the status word: logZ / alpha / beta / the gradient come back NaN, decode returns a negative total.
__shared__ int s_abort;

// pinned host word (or null) that an aborting launch raises: the host looks at it before it trusts a leased workspace again
__device__ unsigned* g_host_abort = nullptr;

__device__ __forceinline__ void set_error(unsigned* ctrl, unsigned code)
{
    __hip_atomic_store(ctrl + 1, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&g_dev_status, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned* const h = g_host_abort;
    if (h) __hip_atomic_store(h, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Bounded waiting: returns true when the caller must give up.  The first waiter to exceed its limit
// raises the error word; everybody else notices it within a few hundred polls and drains, so a
// protocol bug costs well under a second instead of hanging the GPU.
__device__ __forceinline__ bool spin_abort(unsigned* ctrl, int& spins, int limit, unsigned code)
{
    ++spins;
    if (spins > limit) { set_error(ctrl, code); s_abort = 1; return true; }
    if ((spins & 255) == 0 &&
        __hip_atomic_load(ctrl + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != CTRL_INIT) { s_abort = 1; return true; }
    return false;
}

// ---------------------------------------------------------------------------------------------
// LDS and wait primitives
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) const void gbl_void_t;

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N)); }

// LDS word accessors for the flags (every poll must be a fresh DS read)
__device__ __forceinline__ int lds_flag_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_flag_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// The same for the loader wave, as asm: the compiler orders every DS access it can see after ALL outstanding
// global->LDS loads (s_waitcnt vmcnt(0)), which would serialise the loader's pipeline; it counts its loads itself.
__device__ __forceinline__ unsigned lds_addr(const void* p)
{
    return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)p;
}
__device__ __forceinline__ int lds_flag_load_asm(const int* p)
{
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr(p)) : "memory");
    return v;
}
__device__ __forceinline__ void lds_flag_store_asm(int* p, int v)
{
    asm volatile("ds_write_b32 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory");
}
// hand-off entries that carry their own sequence number: the whole entry in ONE access, always a fresh read
__device__ __forceinline__ u64 lds_load64(const void* p)
{
    return __hip_atomic_load((const u64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_store64(void* p, float value, int seq)
{
    __hip_atomic_store((u64*)p, ((u64)(unsigned)seq << 32) | (u64)__float_as_uint(value), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lds_store128(void* p, float4 v)
{
    const f32x4_t w = {v.x, v.y, v.z, v.w};
    asm volatile("ds_write_b128 %0, %1" ::"v"(lds_addr(p)), "v"(w) : "memory");
}
__device__ __forceinline__ float4 lds_load128(const void* p)
{
    f32x4_t w;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(w) : "v"(lds_addr(p)) : "memory");
    return make_float4(w.x, w.y, w.z, w.w);
}

// max_push (common.h) as two selects instead of a compare-and-branch: larger value wins, on ties the smaller key
__device__ __forceinline__ void max_push_sel(float& best, int& key, float t, int k)
{
    const bool take = (t > best) | ((t == best) & (k < key));
    best = take ? t : best;
    key = take ? k : key;
}

}  // namespace semicrf
