// nbest.hip -- k-best Viterbi: the k highest-scoring paths of every chain (include/semicrf_hip.h: semicrf_viterbi_nbest).
//
// The max-plus recursion of semicrf_viterbi with a sorted list of at most K partial paths per (frame, chain) in place of one
// value.  An entry is (value, base, order word): value = base + (singleton ? s[t,t] : 0), base = u[pred][rank] + cell (one fp32
// add each, as in decode), and the order word sorts the rest of the key -- (cidx << 5) | (rank << 1) | singleton, XOR 1 when
// s[t,t] > 0, so the decode's own singleton choice sorts first.  cidx = 0 for the skip, else the other endpoint + 1: decode's
// tie order.  Entries compare by (value desc, base desc, order word asc): a total order that does not depend on K, so a list of
// K >= k entries truncated to k is the k-best list (the launch instantiates K in {1, 2, 4, 8, 16}).
//
// Sweep: rowseq.hip's shape -- one workgroup owns NB_G = 4 consecutive chains (16-byte runs of every cell) and walks the frames
// in order; its 256 threads are 64 column slots x 4 chains.  A slot keeps its own top-K list in registers, fed by its share of
// the candidates; a candidate's ranks are scanned in ascending order and the scan stops at the first rank whose two singleton
// variants both fail to beat the slot's K-th entry.  The 64 lists of a chain are then merged: 16 per wave by XOR shuffles, the
// 4 waves' results through LDS.  A merge of two sorted lists keeps max(A[i], B[K-1-i]) (a bitonic sequence holding the top K)
// and sorts it with a bitonic half-cleaner network -- static register indices only.
//   u    [T][K][B]  the ranked values (-inf for absent ranks)
//   cnt  [T][B]     present ranks (>= 1: every frame has at least the two paths of its singleton)
//   code [B][T][K]  the back-pointer word without the XOR; -1 = absent
// Walk: one workgroup per chain stages the chain's T x k code table in LDS; lane r walks rank r from the start frame, the state
// being (frame, rank), and writes decode.hip's region layout (walk order), so its offsets / pack kernels finish the job.
#include "common.h"
#include "launchers.h"

namespace semicrf {

constexpr int NB_G = 4;                        // chains per workgroup
constexpr int NB_Q = 64;                       // column slots per chain: 16 per wave x 4 waves
constexpr int NB_WAVES = NB_G * NB_Q / WAVE;
constexpr int NB_BATCH = 8;                    // candidates a slot loads before it scans them (K <= 4; 32 / K above)
constexpr int NB_ABSENT = 0x7fffffff;          // order word of an absent entry: after every present one
constexpr int NB_WALK_LDS = 128 * 1024;        // largest code table (T * k int32) the walk stages in LDS

template <int K>
struct NbList {
    float v[K], b[K];
    int o[K];
};

// fp32 -> uint32 that orders as the float does (-0 and +0 map to one key).  The entries compare by these integer keys: with plain
// float comparisons the device ordered a value tie whose bases were one ulp apart the wrong way round (k-best Viterbi).
__device__ __forceinline__ unsigned nb_fkey(float x)
{
    const unsigned b = __float_as_uint(x);
    const unsigned u = (b << 1) ? b : 0u;
    return u ^ ((unsigned)((int)u >> 31) | 0x80000000u);
}

__device__ __forceinline__ bool nb_better(float v, float b, int o, float v2, float b2, int o2)
{
    const unsigned kv = nb_fkey(v), kv2 = nb_fkey(v2), kb = nb_fkey(b), kb2 = nb_fkey(b2);
    return kv > kv2 || (kv == kv2 && (kb > kb2 || (kb == kb2 && o < o2)));
}

template <int K>
__device__ __forceinline__ void nb_clear(NbList<K>& L)
{
#pragma unroll
    for (int i = 0; i < K; ++i) { L.v[i] = SEMICRF_NEG_INF; L.b[i] = SEMICRF_NEG_INF; L.o[i] = NB_ABSENT; }
}

// insert (v, b, o) into the sorted list; false when it does not beat the K-th entry
template <int K>
__device__ __forceinline__ bool nb_insert(NbList<K>& L, float v, float b, int o)
{
    if (!nb_better(v, b, o, L.v[K - 1], L.b[K - 1], L.o[K - 1])) return false;
    bool pc = true;                            // the new entry lies above slot i
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
        const bool c = pc && nb_better(v, b, o, L.v[i - 1], L.b[i - 1], L.o[i - 1]);
        if (c) { L.v[i] = L.v[i - 1]; L.b[i] = L.b[i - 1]; L.o[i] = L.o[i - 1]; }
        else if (pc) { L.v[i] = v; L.b[i] = b; L.o[i] = o; }
        pc = c;
    }
    if (pc) { L.v[0] = v; L.b[0] = b; L.o[0] = o; }
    return true;
}

// A <- the top K of A and P, sorted
template <int K>
__device__ __forceinline__ void nb_merge(NbList<K>& A, const NbList<K>& P)
{
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const int j = K - 1 - i;
        if (nb_better(P.v[j], P.b[j], P.o[j], A.v[i], A.b[i], A.o[i])) { A.v[i] = P.v[j]; A.b[i] = P.b[j]; A.o[i] = P.o[j]; }
    }
#pragma unroll
    for (int s = K / 2; s > 0; s >>= 1) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            if (i & s) continue;
            if (nb_better(A.v[i + s], A.b[i + s], A.o[i + s], A.v[i], A.b[i], A.o[i])) {
                const float tv = A.v[i], tb = A.b[i];
                const int to = A.o[i];
                A.v[i] = A.v[i + s]; A.b[i] = A.b[i + s]; A.o[i] = A.o[i + s];
                A.v[i + s] = tv; A.b[i + s] = tb; A.o[i + s] = to;
            }
        }
    }
}

// DIR 0: forward (frames ascending, candidates skip from t-1 and (j, t) for j < t); DIR 1: backward (frames descending,
// candidates skip to t+1 and (t, e) for e > t).
template <int K, int DIR>
__global__ __launch_bounds__(NB_G * NB_Q) void nbest_sweep_kernel(const float* __restrict__ score, const float* __restrict__ noise,
                                                                 int T, int B, float* u, int* cnt, int* __restrict__ code)
{
    __shared__ float s_v[NB_WAVES][NB_G][K];
    __shared__ float s_b[NB_WAVES][NB_G][K];
    __shared__ int s_o[NB_WAVES][NB_G][K];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int cq = lane & (NB_G - 1);
    const int q = wave * (WAVE / NB_G) + lane / NB_G;
    const int c = blockIdx.x * NB_G + cq;
    const bool valid = c < B;
    const size_t Bs = (size_t)B;

    for (int p = 0; p < T; ++p) {
        const int t = DIR == 0 ? p : T - 1 - p;
        const float d = valid ? score[((size_t)t * T + t) * Bs + c] : 0.0f;
        const int flip = d > 0.0f ? 1 : 0;
        NbList<K> L;
        nb_clear(L);
        // candidate cidx: cell value x, the predecessor's ranked values ur (loaded) and its count np
        auto push = [&](const float x, const float (&ur)[K], const int np, const int cidx) {
#pragma unroll
            for (int r = 0; r < K; ++r) {
                if (r >= np) break;
                const float base = ur[r] + x;
                const int w = (cidx << 5) | (r << 1);
                const float von = base + d, voff = base + 0.0f;
                const bool a = flip ? nb_insert(L, von, base, (w | 1) ^ 1) : nb_insert(L, voff, base, w);
                const bool bb = flip ? nb_insert(L, voff, base, w ^ 1) : nb_insert(L, von, base, w | 1);
                if (!a && !bb) break;
            }
        };
        // every rank of a predecessor is loaded up front: the loads of a batch are independent, one L2 round trip per batch
        auto load = [&](int pf, float (&ur)[K], int& np) {
#pragma unroll
            for (int r = 0; r < K; ++r) ur[r] = u[((size_t)pf * K + r) * Bs + c];
            np = cnt[(size_t)pf * Bs + c];
        };
        if (valid) {
            if (p == 0) {
                if (q == 0) {                  // the terminal frame: the empty path, with or without (t,t)
                    nb_insert(L, flip ? 0.0f + d : 0.0f + 0.0f, 0.0f, 0);
                    nb_insert(L, flip ? 0.0f + 0.0f : 0.0f + d, 0.0f, 1);
                }
            } else {
                if (q == 0) {
                    float ur[K];
                    int np;
                    load(DIR == 0 ? t - 1 : t + 1, ur, np);
                    push(noise[(size_t)(DIR == 0 ? t - 1 : t) * Bs + c], ur, np, 0);
                }
                constexpr int NBB = NB_BATCH * 4 / K < NB_BATCH ? (NB_BATCH * 4 / K > 0 ? NB_BATCH * 4 / K : 1) : NB_BATCH;
                for (int pp0 = q; pp0 < p; pp0 += NB_Q * NBB) {
                    float x[NBB], ur[NBB][K];
                    int np[NBB];
#pragma unroll
                    for (int i = 0; i < NBB; ++i) {
                        const int pp = pp0 + i * NB_Q;
                        const int pf = DIR == 0 ? pp : T - 1 - pp;
                        const size_t cell = DIR == 0 ? (size_t)t * T + pf : (size_t)pf * T + t;
                        np[i] = 0;
                        x[i] = 0.0f;
                        if (pp < p) { x[i] = score[cell * Bs + c]; load(pf, ur[i], np[i]); }
                    }
#pragma unroll
                    for (int i = 0; i < NBB; ++i) {
                        const int pp = pp0 + i * NB_Q;
                        const int pf = DIR == 0 ? pp : T - 1 - pp;
                        if (pp < p) push(x[i], ur[i], np[i], pf + 1);
                    }
                }
            }
        }
        // the 16 slots of this chain in this wave (lanes cq, cq + 4, ..., cq + 60)
#pragma unroll
        for (int m = NB_G; m < WAVE; m <<= 1) {
            NbList<K> P;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                P.v[i] = __shfl_xor(L.v[i], m);
                P.b[i] = __shfl_xor(L.b[i], m);
                P.o[i] = __shfl_xor(L.o[i], m);
            }
            nb_merge(L, P);
        }
        if (lane < NB_G) {
#pragma unroll
            for (int i = 0; i < K; ++i) { s_v[wave][lane][i] = L.v[i]; s_b[wave][lane][i] = L.b[i]; s_o[wave][lane][i] = L.o[i]; }
        }
        __syncthreads();
        if (wave == 0 && lane < NB_G && valid) {
#pragma unroll
            for (int w = 1; w < NB_WAVES; ++w) {
                NbList<K> P;
#pragma unroll
                for (int i = 0; i < K; ++i) { P.v[i] = s_v[w][lane][i]; P.b[i] = s_b[w][lane][i]; P.o[i] = s_o[w][lane][i]; }
                nb_merge(L, P);
            }
            int n = 0;
            int* cw = code + ((size_t)c * T + t) * K;
#pragma unroll
            for (int i = 0; i < K; ++i) {
                const bool present = L.o[i] != NB_ABSENT;
                n += present ? 1 : 0;
                u[((size_t)t * K + i) * Bs + c] = L.v[i];
                cw[i] = present ? (L.o[i] ^ flip) : -1;
            }
            cnt[(size_t)t * Bs + c] = n;
        }
        __syncthreads();
    }
}

// One workgroup per chain; lane r < k walks rank r.  region [k*B][2T][2] (entry r*B + c), counts [k*B], scores [k][B], npaths [B].
__global__ __launch_bounds__(64) void nbest_walk_kernel(const int* __restrict__ code, const float* __restrict__ u,
                                                        const int* __restrict__ cnt, int T, int B, int Kp, int k,
                                                        const int* __restrict__ start, int forward, int in_lds,
                                                        int* __restrict__ region, int* __restrict__ counts,
                                                        float* __restrict__ scores, int* __restrict__ npaths)
{
    extern __shared__ int s_tab[];
    const int c = blockIdx.x, r0 = threadIdx.x;
    const int* cc = code + (size_t)c * T * Kp;
    if (in_lds) {
        for (int i = threadIdx.x; i < T * k; i += 64) s_tab[i] = cc[(size_t)(i / k) * Kp + i % k];
        __syncthreads();
    }
    auto rd = [&](int t, int r) { return in_lds ? s_tab[t * k + r] : cc[(size_t)t * Kp + r]; };
    int st = start ? start[c] : (forward ? T - 1 : 0);
    st = st < 0 ? 0 : (st > T - 1 ? T - 1 : st);
    const int np = min(cnt[(size_t)st * B + c], k);
    if (r0 == 0) npaths[c] = np;
    if (r0 >= k) return;
    const size_t idx = (size_t)r0 * B + c;
    scores[idx] = r0 < np ? u[((size_t)st * Kp + r0) * B + c] : SEMICRF_NEG_INF;
    int* out = region + idx * (size_t)(2 * T) * 2;
    int n = 0;
    if (r0 < np) {
        const int term = forward ? 0 : T - 1;
        int j = st, r = r0;
        for (int step = 0; step < T; ++step) {         // every step moves towards the terminal: at most T of them
            const int w = rd(j, r);
            if (w < 0) break;                          // (absent: never reached from a present rank)
            if (w & 1) { out[2 * n] = j; out[2 * n + 1] = j; ++n; }
            if (j == term) break;
            const int cidx = w >> 5;
            r = (w >> 1) & 15;
            if (r >= k) break;
            if (cidx == 0) { j += forward ? -1 : 1; continue; }
            const int q = cidx - 1;
            if (forward ? !(q < j) : !(q > j && q < T)) break;
            // decode.hip's emission: (j, e) on the backward walk; (b, j) on the forward one, whose list the pack kernel reverses
            out[2 * n] = forward ? q : j; out[2 * n + 1] = forward ? j : q; ++n;
            j = q;
        }
    }
    counts[idx] = n;
}

static int nbest_kp(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16; }

// nB = k * B; the instantiated Kp < 2k covers Kp * B < 2 nB
size_t nbest_workspace_bytes(int T, int nB)
{
    const size_t n2 = (size_t)T * 2 * nB;
    // u, code [T][Kp][B]; cnt [T][B]; region [nB][2T][2]; counts [nB]
    return align_up(n2 * 4) * 2 + align_up((size_t)T * nB * 4) + align_up((size_t)nB * 2 * T * 2 * 4) + align_up((size_t)nB * 4) + 4096;
}

template <int K>
static void launch_sweep(const float* score, const float* noise, int T, int B, int forward, float* u, int* cnt, int* code,
                         hipStream_t stream)
{
    const dim3 grid((B + NB_G - 1) / NB_G), block(NB_G * NB_Q);
    if (forward) hipLaunchKernelGGL((nbest_sweep_kernel<K, 0>), grid, block, 0, stream, score, noise, T, B, u, cnt, code);
    else hipLaunchKernelGGL((nbest_sweep_kernel<K, 1>), grid, block, 0, stream, score, noise, T, B, u, cnt, code);
}

void launch_viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int* start, int forward, int* pairs,
                          long long cap, int* offsets, float* scores, int* npaths, void* ws, hipStream_t stream)
{
    const int Kp = nbest_kp(k);
    const size_t nB = (size_t)k * B;
    char* p = (char*)ws;
    float* u = (float*)p;   p += align_up((size_t)T * 2 * nB * 4);
    int* code = (int*)p;    p += align_up((size_t)T * 2 * nB * 4);
    int* cnt = (int*)p;     p += align_up((size_t)T * nB * 4);
    int* region = (int*)p;  p += align_up(nB * 2 * T * 2 * 4);
    int* counts = (int*)p;
    switch (Kp) {
        case 1: launch_sweep<1>(score, noise, T, B, forward, u, cnt, code, stream); break;
        case 2: launch_sweep<2>(score, noise, T, B, forward, u, cnt, code, stream); break;
        case 4: launch_sweep<4>(score, noise, T, B, forward, u, cnt, code, stream); break;
        case 8: launch_sweep<8>(score, noise, T, B, forward, u, cnt, code, stream); break;
        default: launch_sweep<16>(score, noise, T, B, forward, u, cnt, code, stream); break;
    }
    static PerDeviceOnce attr;
    if (attr.first())
        (void)hipFuncSetAttribute((const void*)nbest_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NB_WALK_LDS);
    const size_t tab = (size_t)T * k * sizeof(int);
    const int in_lds = tab <= (size_t)NB_WALK_LDS ? 1 : 0;
    hipLaunchKernelGGL(nbest_walk_kernel, dim3(B), dim3(64), in_lds ? tab : 0, stream, code, u, cnt, T, B, Kp, k, start, forward,
                       in_lds, region, counts, scores, npaths);
    launch_pack(region, counts, T, (int)nB, forward, pairs, cap, offsets, stream, nullptr, 0, 0);
}

}  // namespace semicrf
