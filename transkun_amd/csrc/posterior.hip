// posterior.hip -- posterior marginals and path entropy of the semi-CRF (include/semicrf_hip.h: semicrf_posteriors,
// semicrf_interval_marginals).
//
// With alpha (v, semicrf_logz_fwd), beta (q, semicrf_beta) and logZ known, every summary is a dependence-free function of one
// read of the lower triangle of the score.  With R[e] = v[e] - sp(s[e,e]) (the log row total of alpha's recursion at e) and
// A[e] = q[e] - logZ, the cell (e, b), b < e, of chain c has
//   y = v[b] + s[e,b],  mu = exp(y + A[e])            (the marginal: dScore of semicrf_logz_bwd with gout = 1)
//   and the entropy term  mu * (R[e] - y)            (= -node[e] p lp of the backward walk's predecessor draw; >= 0, clamped)
// so one exp per cell gives end[e] += mu, begin[b] += mu and the entropy together.
//
// Three kernels:
//   posterior_stream_kernel  one 64 x 64 (end x begin) tile of the triangle x 32 chains per workgroup of 4 waves (16 rows each).
//                            Lane = (chain quad qd: 4 neighbouring chains read as one 16-byte piece, column slot bs): it owns the
//                            columns b0 + bs + 8k, k < 8, whose v[b] it loads once per tile; the rows' R / A are staged in LDS
//                            once per tile.  Per row: the 8 column slots of a quad are summed by shuffles and written as the
//                            tile's row partial; per tile: the column sums (over the 4 waves, in LDS, fixed order) and the
//                            entropy (one value per chain) are written.  No atomics: every partial has one writer.
//   posterior_epilogue_kernel  per (frame, chain): end / begin as the sum of the row / column partials in tile order, node,
//                            single, noise, the singleton's Bernoulli entropy and the skip's entropy term; per chain the
//                            entropy partial of 16 frames (plus, once per row band, the band's tiles), in a fixed order.
//   posterior_entropy_kernel  per chain the sum of those partials, in frame order.
// The result is a pure function of the inputs (two calls are bit-identical).
#include "common.h"
#include "launchers.h"
#include "posterior_cell.h"

namespace semicrf {

namespace {
constexpr int PT = 64;                      // tile edge (frames), rows and columns
constexpr int PQ = 8;                       // chain quads per wave (32 chains)
constexpr int PCH = 4 * PQ;
constexpr int PK = PT / 8;                  // columns per lane
constexpr int PWAVES = 4;                   // waves per workgroup; each takes PT / PWAVES rows of the tile
constexpr int PROWS = PT / PWAVES;
constexpr int PSUB = 4;                     // epilogue: workgroups per row band (16 frames each)

__device__ __forceinline__ void st4(float* __restrict__ p, int n, f4 x)
{
    if (n >= 4) { *(f4u*)p = (f4u)x; return; }
    if (n > 0) p[0] = x.x;
    if (n > 1) p[1] = x.y;
    if (n > 2) p[2] = x.z;
}

// (clamp1, single_marg and the cell marginals shared with marginal_decode.hip: posterior_cell.h)
// Bernoulli entropy of sigmoid(d), in the form that is symmetric in d and has no cancellation: sp(-|d|) + |d| sigmoid(-|d|)
__device__ __forceinline__ float bern_entropy(float d)
{
    const float a = fabsf(d), ea = __expf(-a);
    return log1pf(ea) + (ea > 0.0f ? a * ea / (1.0f + ea) : 0.0f);
}
// one entropy term mu * (-lp), lp = y - R clamped to <= 0; a cell of zero probability adds exactly 0 (even with lp = -inf)
__device__ __forceinline__ float ent_term(float mu, float R, float y)
{
    return mu > 0.0f ? mu * fmaxf(R - y, 0.0f) : 0.0f;
}

}  // namespace

// grid (ceil(B/32), nI (nI+1)/2), block 256.  rowp [nI][T][B]: rowp[j][e] = sum over the columns of tile (e/64, j);
// colp [nI][T][B]: colp[i][b] = sum over the rows of tile (i, b/64); htile [ntiles][B]: the tile's entropy terms.
__global__ __launch_bounds__(64 * PWAVES, 2) void posterior_stream_kernel(const float* __restrict__ score, const float* __restrict__ v,
                                                                          const float* __restrict__ q, const float* __restrict__ logZ,
                                                                          int T, int B, float* __restrict__ rowp,
                                                                          float* __restrict__ colp, float* __restrict__ htile)
{
    __shared__ __attribute__((aligned(16))) float s_R[PT][PCH];
    __shared__ __attribute__((aligned(16))) float s_A[PT][PCH];
    __shared__ f4 s_col[PWAVES - 1][PK][64];
    __shared__ f4 s_h[PWAVES - 1][64];
    const int tile = (int)blockIdx.y;
    int ti, tj;
    tile_of(tile, ti, tj);
    const int e0 = ti * PT, b0 = tj * PT;
    const int cbase = (int)blockIdx.x * PCH;
    const size_t Bs = (size_t)B;

    for (int k = (int)threadIdx.x; k < PT * PCH; k += 64 * PWAVES) {
        const int r = k / PCH, cc = k % PCH, e = e0 + r, c = cbase + cc;
        float R = 0.0f, A = SEMICRF_NEG_INF;
        if (e < T && c < B) {
            R = v[(size_t)e * Bs + c] - softplus_f(score[((size_t)e * T + e) * Bs + c]);
            A = q[(size_t)e * Bs + c] - logZ[c];
        }
        s_R[r][cc] = R;
        s_A[r][cc] = A;
    }
    __syncthreads();

    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int qd = lane & (PQ - 1), bs = lane >> 3;
    const int c0 = cbase + 4 * qd;
    const int nc = B - c0 < 0 ? 0 : (B - c0 > 4 ? 4 : B - c0);
    const bool diag = ti == tj;

    f4 vb[PK], col[PK];
#pragma unroll
    for (int k = 0; k < PK; ++k) {
        const int b = b0 + bs + 8 * k;
        vb[k] = b < T ? ld4(v + (size_t)b * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
        col[k] = (f4)(0.0f);
    }
    f4 h = (f4)(0.0f);

    const int r0 = wave * PROWS;
    for (int r = r0; r < r0 + PROWS; ++r) {
        const int e = e0 + r;
        if (e >= T) break;                                   // wave-uniform
        const float* row = score + (size_t)e * T * Bs + c0;
        f4 x[PK];
#pragma unroll
        for (int k = 0; k < PK; ++k) {
            const int b = b0 + bs + 8 * k;
            x[k] = (!diag || b < e) ? ld4(row + (size_t)b * Bs, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
        }
        const f4 R = *(const f4*)&s_R[r][4 * qd];
        const f4 A = *(const f4*)&s_A[r][4 * qd];
        f4 racc = (f4)(0.0f);
#pragma unroll
        for (int k = 0; k < PK; ++k) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const float y = vb[k][ch] + x[k][ch];
                const float mu = __expf(y + A[ch]);
                racc[ch] += mu;
                col[k][ch] += mu;
                h[ch] += ent_term(mu, R[ch], y);
            }
        }
#pragma unroll
        for (int m = 8; m < 64; m <<= 1)
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) racc[ch] += __shfl_xor(racc[ch], m);
        if (bs == 0 && nc > 0) st4(rowp + ((size_t)tj * T + e) * Bs + c0, nc, racc);
    }

    // the entropy over the column slots (shuffles), then over the waves (LDS, wave order)
#pragma unroll
    for (int m = 8; m < 64; m <<= 1)
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) h[ch] += __shfl_xor(h[ch], m);
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < PK; ++k) s_col[wave - 1][k][lane] = col[k];
        s_h[wave - 1][lane] = h;
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < PWAVES - 1; ++w) {
#pragma unroll
            for (int k = 0; k < PK; ++k) col[k] += s_col[w][k][lane];
            h += s_h[w][lane];
        }
        if (nc > 0) {
#pragma unroll
            for (int k = 0; k < PK; ++k) {
                const int b = b0 + bs + 8 * k;
                if (b < T) st4(colp + ((size_t)ti * T + b) * Bs + c0, nc, col[k]);
            }
            if (bs == 0) st4(htile + (size_t)tile * Bs + c0, nc, h);
        }
    }
}

// grid (ceil(B/64), nI * PSUB), block 256: 64 chains (a lane each) x 4 waves over the 16 frames of sub-band `sub` of row band i.
// epart [nI * PSUB][B]; the tiles' entropy of band i is added by its sub-band 0.
__global__ __launch_bounds__(256) void posterior_epilogue_kernel(const float* __restrict__ score, const float* __restrict__ noise,
                                                                 const float* __restrict__ v, const float* __restrict__ q,
                                                                 const float* __restrict__ logZ, int T, int B, int nI,
                                                                 const float* __restrict__ rowp, const float* __restrict__ colp,
                                                                 const float* __restrict__ htile, float* __restrict__ node,
                                                                 float* __restrict__ begin, float* __restrict__ end,
                                                                 float* __restrict__ single, float* __restrict__ noiseP,
                                                                 float* __restrict__ epart)
{
    __shared__ float s_h[4][64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int c = (int)blockIdx.x * 64 + lane;
    const int i = (int)blockIdx.y / PSUB, sub = (int)blockIdx.y % PSUB;
    const size_t Bs = (size_t)B;
    float h = 0.0f;
    if (c < B) {
        const float lz = logZ[c];
        for (int r = sub * (PT / PSUB) + wave; r < (sub + 1) * (PT / PSUB); r += 4) {
            const int t = i * PT + r;
            if (t >= T) break;
            const size_t tc = (size_t)t * Bs + c;
            const float vt = v[tc], qt = q[tc], d = score[((size_t)t * T + t) * Bs + c];
            const float sp = softplus_f(d), R = vt - sp;
            const float nd = clamp1(__expf(R + qt - lz));
            node[tc] = nd;
            single[tc] = clamp1(single_marg(vt, qt, lz, d));
            if (t + 1 < T) noiseP[tc] = clamp1(__expf(vt + noise[tc] + q[tc + Bs] - lz));
            float en = 0.0f, bg = 0.0f;
#pragma unroll 8
            for (int j = 0; j <= i; ++j) en += rowp[((size_t)j * T + t) * Bs + c];
#pragma unroll 8
            for (int k = i; k < nI; ++k) bg += colp[((size_t)k * T + t) * Bs + c];
            end[tc] = clamp1(en);
            begin[tc] = clamp1(bg);
            h += nd > 0.0f ? nd * bern_entropy(d) : 0.0f;
            if (t > 0) {
                const size_t pc = tc - Bs;
                const float y = v[pc] + noise[pc];
                h += ent_term(__expf(y + qt - lz), R, y);
            }
        }
    }
    s_h[wave][lane] = h;
    __syncthreads();
    if (wave == 0 && c < B) {
        float acc = ((s_h[0][lane] + s_h[1][lane]) + s_h[2][lane]) + s_h[3][lane];
        if (sub == 0) {
            const int k0 = i * (i + 1) / 2;
            for (int j = 0; j <= i; ++j) acc += htile[(size_t)(k0 + j) * Bs + c];
        }
        epart[(size_t)blockIdx.y * Bs + c] = acc;
    }
}

__global__ void posterior_entropy_kernel(const float* __restrict__ epart, int n, int B, float* __restrict__ entropy)
{
    const int c = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= B) return;
    float acc = 0.0f;
#pragma unroll 8
    for (int i = 0; i < n; ++i) acc += epart[(size_t)i * B + c];          // (unrolled: the loads of a batch are in flight together)
    entropy[c] = acc;
}

// one thread per interval; the chain by binary search over offsets.  b > e: 0 (never on a path); an index out of range: NaN.
__global__ void interval_marginals_kernel(const float* __restrict__ score, const float* __restrict__ v, const float* __restrict__ q,
                                          const float* __restrict__ logZ, int T, int B, const int* __restrict__ pairs, int K,
                                          const int* __restrict__ offsets, float* __restrict__ out)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= K) return;
    int lo = 0, hi = B;                     // the chain c with offsets[c] <= k < offsets[c+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    const int c = lo, b = pairs[2 * k], e = pairs[2 * k + 1];
    const size_t Bs = (size_t)B;
    float r;
    if (b < 0 || e < 0 || b >= T || e >= T) r = __builtin_nanf("");
    else if (b > e) r = 0.0f;
    else if (b == e) r = cell_marginal_single(v[(size_t)e * Bs + c], q[(size_t)e * Bs + c], logZ[c], score[((size_t)e * T + e) * Bs + c]);
    else r = cell_marginal(v[(size_t)b * Bs + c], score[((size_t)e * T + b) * Bs + c], q[(size_t)e * Bs + c] - logZ[c]);
    out[k] = r;
}

static inline int band_count(int T) { return (T + PT - 1) / PT; }

size_t posterior_workspace_bytes(int T, int B)
{
    const size_t nI = (size_t)band_count(T), Bs = (size_t)B;
    return align_up(nI * T * Bs * 4) * 2 + align_up(nI * (nI + 1) / 2 * Bs * 4) + align_up(nI * PSUB * Bs * 4);
}

void launch_posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                       float* node, float* begin, float* end, float* single, float* noiseP, float* entropy, void* ws,
                       hipStream_t stream)
{
    const int nI = band_count(T);
    const size_t Bs = (size_t)B, part = align_up((size_t)nI * T * Bs * 4);
    char* w = (char*)ws;
    float* rowp = (float*)w;
    float* colp = (float*)(w + part);
    float* htile = (float*)(w + 2 * part);
    float* epart = (float*)(w + 2 * part + align_up((size_t)nI * (nI + 1) / 2 * Bs * 4));
    posterior_stream_kernel<<<dim3((B + PCH - 1) / PCH, nI * (nI + 1) / 2), 64 * PWAVES, 0, stream>>>(score, v, q, logZ, T, B, rowp,
                                                                                                   colp, htile);
    posterior_epilogue_kernel<<<dim3((B + 63) / 64, nI * PSUB), 256, 0, stream>>>(score, noise, v, q, logZ, T, B, nI, rowp, colp, htile, node,
                                                                         begin, end, single, noiseP, epart);
    posterior_entropy_kernel<<<(B + 255) / 256, 256, 0, stream>>>(epart, nI * PSUB, B, entropy);
}

void launch_interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int* pairs,
                               int K, const int* offsets, float* out, hipStream_t stream)
{
    if (K <= 0) return;
    interval_marginals_kernel<<<(K + 255) / 256, 256, 0, stream>>>(score, v, q, logZ, T, B, pairs, K, offsets, out);
}

}  // namespace semicrf
