// alpha_from.hip -- the forward (alpha) sweep of the semi-CRF restricted to the frames start[c] .. T-1 of every chain
// (include/semicrf_hip.h: semicrf_alpha_from): the alpha of the model that decode(forcedStartPos) maximises, so that the
// posterior family (posteriors, interval marginals, marginal / MBR decoding) can run from a forced start.
//
//   v[t] = -inf                                                                       t <  s
//   v[s] = sp(d[s])
//   v[t] = log(exp(v[t-1] + n[t-1]) + sum_{s <= b < t} exp(v[b] + S[t,b])) + sp(d[t])   t >  s
//
// One workgroup of 4 waves owns 16 chains (4 chain quads, 64 bytes of every cell) for the whole recurrence: no flags, no
// spins, no grid barrier, no atomics -- nothing here can wait for another workgroup.  It walks the rows in blocks of R = 16
// from the smallest start of its chains; per block
//   far field   predecessors b < t0: they need only alpha of earlier blocks, so every row of the block runs at once.  Wave w takes
//               the rows w, w+4, w+8, w+12 of the block; lane = (quad, predecessor slot of 16); the 16 slots of a row are merged by
//               shuffles.  The result, a (maximum, sum) pair per row and chain, goes through LDS.
//   near field  the R x R triangle, rows in order, in wave 0: lane = (quad, column j of the block) holds the cells of its
//               column and, once row j is done, alpha[t0 + j]; a row merges its 16 lanes by a butterfly of shuffles (every lane
//               then holds the row's alpha, bit for bit the same: the merge is commutative).
// alpha of the group lives in LDS ([T][16] floats) while that fits (T <= 2048), beyond that the far field reads the v this
// workgroup wrote itself, a barrier earlier (as expectation.hip does).
// Chains of one quad may start at different frames: a chain ignores predecessors before its own start by selection (never
// by arithmetic on what was loaded), and where a column lies before the start of some chain of the quad the cells are loaded
// chain by chain -- nothing in a column before a chain's start is read for that chain.
// fp32, running-maximum log-sum-exp on __expf; fixed summation order: two calls are bit-identical.
#include <mutex>
#include "posterior_cell.h"
#include "launchers.h"

namespace semicrf {

namespace {
constexpr int ACH = 16;                      // chains per workgroup
constexpr int AR = 16;                       // rows per block
constexpr int AWAVES = 4;
constexpr int ALDS_MAX_T = 2048;             // [T][16] floats in LDS: 128 KB

struct Quad {                                // the 4 chains of a lane
    int c0, n;                               // first chain, how many exist (<= 0: none)
    int st[4];                               // effective start: T for a chain that never starts (absent, or start out of range)
    int lo, hi;                              // smallest / largest effective start
};

// chains of the quad for which frame b lies at or behind the start
__device__ __forceinline__ void ok_of(const Quad& q, int b, bool ok[4])
{
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) ok[ch] = b >= q.st[ch];
}

// 4 chains at p (column / frame b): one 16-byte access when every chain of the quad has started, else chain by chain
__device__ __forceinline__ f4 ldq(const float* __restrict__ p, const Quad& q, int b, const bool ok[4])
{
    if (b >= q.hi) return (f4)(*(const f4u*)p);           // hi < T implies n == 4 and every start <= b
    f4 r = {SEMICRF_NEG_INF, SEMICRF_NEG_INF, SEMICRF_NEG_INF, SEMICRF_NEG_INF};
    if (ok[0]) r.x = p[0];
    if (ok[1]) r.y = p[1];
    if (ok[2]) r.z = p[2];
    if (ok[3]) r.w = p[3];
    return r;
}

// (M, S) <- (M, S) (+) exp(x); an empty accumulator is (-inf, 0), x = -inf adds nothing
__device__ __forceinline__ void push1(float& M, float& S, float x)
{
    const float nm = fmaxf(M, x);
    const float a = S == 0.0f ? 0.0f : S * __expf(M - nm);
    const float b = x == SEMICRF_NEG_INF ? 0.0f : __expf(x - nm);
    S = a + b;
    M = nm;
}
__device__ __forceinline__ void merge1(float& M, float& S, float M2, float S2)
{
    const float nm = fmaxf(M, M2);
    const float a = S == 0.0f ? 0.0f : S * __expf(M - nm);
    const float b = S2 == 0.0f ? 0.0f : S2 * __expf(M2 - nm);
    S = a + b;
    M = nm;
}
// the 16 slots of a (quad, row): lanes that differ in bits 2..5; every lane ends with the same bits
__device__ __forceinline__ void butterfly(f4& M, f4& S)
{
#pragma unroll
    for (int d = 4; d < 64; d <<= 1) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const float m2 = __shfl_xor(M[ch], d), s2 = __shfl_xor(S[ch], d);
            float m = M[ch], s = S[ch];
            merge1(m, s, m2, s2);
            M[ch] = m; S[ch] = s;
        }
    }
}
__device__ __forceinline__ f4 bcast(f4 x, int src)
{
    f4 r;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) r[ch] = __shfl(x[ch], src);
    return r;
}
}  // namespace

// grid ceil(B / 16), block 256; LDSA: alpha of the group in dynamic LDS ([T][16] floats)
template <bool LDSA>
__global__ __launch_bounds__(64 * AWAVES) void alpha_from_kernel(const float* __restrict__ score, const float* __restrict__ noise,
                                                                 const int* __restrict__ start, int T, int B, float* v,
                                                                 float* __restrict__ logZ)
{
    extern __shared__ __attribute__((aligned(16))) float s_alpha[];      // LDSA: [T][ACH]
    __shared__ float s_fm[AR][ACH], s_fs[AR][ACH];         // the far field of the block's rows: (maximum, sum) per chain
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, qd = lane & 3, slot = lane >> 2;
    const int cbase = (int)blockIdx.x * ACH;
    const size_t Bs = (size_t)B;
    const float ninf = SEMICRF_NEG_INF, qnan = __builtin_nanf("");

    // the starts of the group; smin: where the group's recurrence begins (T: no chain of it ever starts)
    int smin = T;
    Quad q;
    q.c0 = cbase + 4 * qd;
    q.n = B - q.c0 < 4 ? B - q.c0 : 4;
    q.lo = T; q.hi = 0;
    bool bad[4];
#pragma unroll
    for (int cc = 0; cc < ACH; ++cc) {
        const int c = cbase + cc;
        int s = T;
        bool bd = false;
        if (c < B) {
            s = start[c];
            bd = s < 0 || s > T - 1;
            if (bd) s = T;
        }
        smin = s < smin ? s : smin;
        if ((cc >> 2) == qd) {
            q.st[cc & 3] = s;
            bad[cc & 3] = bd;
            q.lo = s < q.lo ? s : q.lo;
            q.hi = s > q.hi ? s : q.hi;
        }
    }

    // rows before the group's first start: -inf (NaN for a start out of range)
    for (size_t i = (size_t)tid; i < (size_t)smin * ACH; i += 64 * AWAVES) {
        const int t = (int)(i / ACH), cc = (int)(i % ACH), c = cbase + cc;
        if (c < B) {
            const int s = start[c];
            v[(size_t)t * Bs + c] = (s < 0 || s > T - 1) ? qnan : ninf;
        }
    }

    f4 aprev = {ninf, ninf, ninf, ninf};                   // wave 0: alpha of the previous row (every lane of a quad holds it)
    for (int t0 = smin; t0 < T; t0 += AR) {
        // ---- wave 0: the block's own cells, loaded ahead of the far field (column tj of the triangle, the diagonal, the gap) ----
        f4 tri[AR], spd = {0.0f, 0.0f, 0.0f, 0.0f}, nz = {ninf, ninf, ninf, ninf};
        const int tj = t0 + slot;
        bool okj[4];
        ok_of(q, tj, okj);
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < AR; ++r) {
                tri[r] = (f4){ninf, ninf, ninf, ninf};
                if (r > slot && t0 + r < T && tj >= q.lo) tri[r] = ldq(score + ((size_t)(t0 + r) * T + tj) * Bs + q.c0, q, tj, okj);
            }
            if (tj < T && tj >= q.lo) {
                const f4 d = ldq(score + ((size_t)tj * T + tj) * Bs + q.c0, q, tj, okj);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) spd[ch] = okj[ch] ? softplus_f(d[ch]) : 0.0f;
                if (tj - 1 >= q.lo) {                       // the gap tj-1 .. tj, for the chains that have started by tj-1
                    bool okp[4];
                    ok_of(q, tj - 1, okp);
                    nz = ldq(noise + (size_t)(tj - 1) * Bs + q.c0, q, tj - 1, okp);
                }
            }
        }

        // ---- far field: rows t0 + wave + 4 i, predecessors q.lo <= b < t0, 16 slots per (quad, row) ----
        f4 fM[4], fS[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { fM[i] = (f4){ninf, ninf, ninf, ninf}; fS[i] = (f4){0.0f, 0.0f, 0.0f, 0.0f}; }
        for (int b = q.lo + slot; b < t0; b += 16) {
            bool ok[4];
            ok_of(q, b, ok);
            f4 ab;
            if (LDSA) ab = *(const f4*)&s_alpha[(size_t)b * ACH + 4 * qd];
            else ab = ldq(v + (size_t)b * Bs + q.c0, q, b, ok);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = t0 + wave + 4 * i;
                if (t < T) {
                    const f4 s = ldq(score + ((size_t)t * T + b) * Bs + q.c0, q, b, ok);
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        const float x = ok[ch] ? ab[ch] + s[ch] : ninf;
                        float m = fM[i][ch], sm = fS[i][ch];
                        push1(m, sm, x);
                        fM[i][ch] = m; fS[i][ch] = sm;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            butterfly(fM[i], fS[i]);
            if (slot == 0) {
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) { s_fm[wave + 4 * i][4 * qd + ch] = fM[i][ch]; s_fs[wave + 4 * i][4 * qd + ch] = fS[i][ch]; }
            }
        }
        __syncthreads();

        // ---- near field: the block's triangle, rows in order (wave 0) ----
        if (wave == 0) {
            f4 aj = {ninf, ninf, ninf, ninf};              // alpha[tj] once row `slot` is done
#pragma unroll
            for (int r = 0; r < AR; ++r) {
                const int t = t0 + r;
                if (t < T) {                                // (uniform)
                    const f4 spr = bcast(spd, (r << 2) | qd), nzr = bcast(nz, (r << 2) | qd);
                    f4 M, S;
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        float m, s;
                        if (slot == AR - 1) {               // (column 15 is no predecessor inside the block) the far field and the gap
                            m = s_fm[r][4 * qd + ch]; s = s_fs[r][4 * qd + ch];
                            push1(m, s, t - 1 >= q.st[ch] ? aprev[ch] + nzr[ch] : ninf);
                        } else {
                            m = (slot < r && okj[ch]) ? aj[ch] + tri[r][ch] : ninf;
                            s = m == ninf ? 0.0f : 1.0f;
                        }
                        M[ch] = m; S[ch] = s;
                    }
                    butterfly(M, S);
                    f4 a;
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch)
                        a[ch] = t < q.st[ch] ? ninf : (t == q.st[ch] ? spr[ch] : M[ch] + logf(S[ch]) + spr[ch]);
                    if (slot == r) aj = a;
                    aprev = a;
                }
            }
            if (tj < T) {                                   // lane (quad, j) writes row t0 + j of its 4 chains
                if (LDSA) *(f4*)&s_alpha[(size_t)tj * ACH + 4 * qd] = aj;
                f4 o;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) o[ch] = bad[ch] ? qnan : aj[ch];
                float* p = v + (size_t)tj * Bs + q.c0;
                if (q.n >= 4) *(f4u*)p = (f4u)o;
                else {
                    if (q.n > 0) p[0] = o.x;
                    if (q.n > 1) p[1] = o.y;
                    if (q.n > 2) p[2] = o.z;
                }
            }
        }
        __syncthreads();
    }

    if (wave == 0 && slot == 0) {                           // logZ = alpha[T-1] (aprev after the last block)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch)
            if (ch < q.n) logZ[q.c0 + ch] = bad[ch] ? qnan : aprev[ch];
    }
}

// Per device: may alpha_from_kernel<true> take more than the default 64 KB of dynamic LDS?  0 = not asked yet, 1 = yes, 2 = no.
// Asked under a lock, so that no thread launches with a large LDS size before the attribute is set on that device.
static std::mutex g_alpha_from_mu;
static int g_alpha_from_lds[64];

static bool alpha_from_large_lds()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    std::lock_guard<std::mutex> lk(g_alpha_from_mu);
    if (g_alpha_from_lds[dev] == 0) {
        const bool ok = hipFuncSetAttribute((const void*)alpha_from_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            ALDS_MAX_T * ACH * (int)sizeof(float)) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        g_alpha_from_lds[dev] = ok ? 1 : 2;
    }
    return g_alpha_from_lds[dev] == 1;
}

void launch_alpha_from(const float* score, const float* noise, const int* start, int T, int B, float* v, float* logZ, hipStream_t stream)
{
    const unsigned grid = (unsigned)((B + ACH - 1) / ACH);
    const size_t lds = (size_t)T * ACH * sizeof(float);
    if (T <= ALDS_MAX_T) {
        if (lds <= 48 * 1024 || alpha_from_large_lds()) {
            alpha_from_kernel<true><<<grid, 64 * AWAVES, lds, stream>>>(score, noise, start, T, B, v, logZ);
            return;
        }
    }
    alpha_from_kernel<false><<<grid, 64 * AWAVES, 0, stream>>>(score, noise, start, T, B, v, logZ);
}

}  // namespace semicrf
