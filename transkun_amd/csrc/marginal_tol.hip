// marginal_tol.hip -- onset/offset-tolerant interval posteriors (include/semicrf_hip.h: semicrf_interval_marginals_tol,
// semicrf_marginal_decode_tol).  M(e, b) is the sum of the cell marginals m over the box |b' - b| <= db, |e' - e| <= de, capped at 1:
// row sums in ascending b', then the sum of the rows in ascending e', every sum one fp32 add per term.  That order is the contract: a
// separable stencil (here) and a literal gather (posterior_cell.h: tol_marginal) then give the same bits, because a cell outside the
// triangle enters the stencil as +0.0f and x + 0.0f == x for every x >= 0 and for NaN.
//
//   mtol_gather_kernel   one thread per interval: tol_marginal, at most (2 db + 1)(2 de + 1) <= 289 cells.
//   mtol_count_kernel    marginal_decode.hip's count pass with M in place of m, in the same geometry: one 64 x 64 (end x begin) tile x
//                        32 chains per workgroup of 4 waves, lane = (chain quad, column slot), a lane owns 2 columns and walks all
//                        rows of them.  The tile is walked with its halo: rows e0 - de .. e0 + 63 + de, columns b0 - db .. b0 + 63 + db.
//                        Per row: every m of the row (64 + 2 db columns x 32 chains) is formed ONCE and staged in LDS (two buffers,
//                        so one barrier per row); then a lane sums the 2 db + 1 staged values around each of its columns (ascending)
//                        and keeps that row sum in an LDS ring of 2 de + 1 rows; once row e + de is in the ring, M(e, .) is the sum
//                        of the ring in ascending row order.  The ring is lane-private (a lane reads only what it wrote): no barrier
//                        for it.  LDS = 2 (64 + 2 db) x 128 B + (2 de + 1) x 8 KB: 24 KB at (0, 0), 57 KB at (2, 2), 156 KB at
//                        (8, 8) -- dynamic, so a small tolerance keeps several workgroups per CU.  Quads are 16-byte pieces, a wave
//                        reads 1 KB of consecutive LDS per access: no bank conflict.
//                        Halo guard: a cell with b' < 0, e' < 0, e' >= T or b' > e' is never loaded and enters as +0.0f; the
//                        singleton of a halo row takes v, q of its own frame (the staging lane holds v[b'], the row's q[e']).
//   mtol_write_kernel    marginal_decode.hip's write pass with tol_marginal: the rows of the masks are re-evaluated with the
//                        gather's function, so the count pass and the write pass agree because the two evaluations are bit-identical.
// The scans and the offsets kernel of marginal_decode.hip are reused (marginal_decode_scans); the workspace is that of
// semicrf_marginal_decode.  No atomics: every word has one writer and every sum a fixed order.
#include "common.h"
#include "launchers.h"
#include "posterior_cell.h"

namespace semicrf {

namespace {
constexpr int XT = 64;                      // tile edge (frames): marginal_decode.hip's, the masks are 64-bit row words
constexpr int XQ = 8;                       // chain quads per workgroup (32 chains)
constexpr int XCH = 4 * XQ;
constexpr int XWAVES = 4;
constexpr int XTHREADS = 64 * XWAVES;
constexpr int XCOLS = XT / XWAVES;          // columns of the tile per wave
constexpr int XK = XCOLS / 8;               // columns per lane
constexpr int XTOL = 8;                     // SEMICRF_TOL_MAX
constexpr int XSTAGE = ((XT + 2 * XTOL) * XQ + XTHREADS - 1) / XTHREADS;     // staged (column, quad) items per thread: 3
}  // namespace

// one thread per interval; the chain by binary search over offsets.  b > e: 0; an index out of range: NaN.
__global__ void mtol_gather_kernel(const float* __restrict__ score, const float* __restrict__ v, const float* __restrict__ q,
                                   const float* __restrict__ logZ, int T, int B, const int* __restrict__ pairs, int K,
                                   const int* __restrict__ offsets, int db, int de, float* __restrict__ out)
{
    const int k = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= K) return;
    int lo = 0, hi = B;                     // the chain c with offsets[c] <= k < offsets[c+1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= k) lo = mid; else hi = mid;
    }
    const int c = lo, b = pairs[2 * k], e = pairs[2 * k + 1];
    float r;
    if (b < 0 || e < 0 || b >= T || e >= T) r = __builtin_nanf("");
    else if (b > e) r = 0.0f;
    else r = tol_marginal<float>(score, v, q, logZ[c], T, (size_t)B, c, 1, b, e, db, de);
    out[k] = r;
}

// grid (ceil(B/32), nI (nI+1)/2), block 256, dynamic LDS (2 (64 + 2 db) + 64 (2 de + 1)) * 128 bytes.  cnt / mask: marginal_decode.hip.
__global__ __launch_bounds__(XTHREADS) void mtol_count_kernel(const float* __restrict__ score, const float* __restrict__ v,
                                                              const float* __restrict__ q, const float* __restrict__ logZ, int T, int B,
                                                              const float* __restrict__ tau, int tau_stride, int NQ, int db, int de,
                                                              int* __restrict__ cnt, u64* __restrict__ mask)
{
    extern __shared__ __attribute__((aligned(16))) float s_lds[];
    const int W = XT + 2 * db, R = 2 * de + 1;
    float* const s_stage = s_lds;                                // [2][W][XCH]: the m of one row, columns b0 - db .. b0 + 63 + db
    float* const s_ring = s_lds + (size_t)2 * W * XCH;           // [R][XT][XCH]: the row sums of the last R rows
    int ti, tj;
    tile_of((int)blockIdx.y, ti, tj);
    const int e0 = ti * XT, b0 = tj * XT;
    const int cbase = (int)blockIdx.x * XCH;
    const size_t Bs = (size_t)B;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qd = lane & (XQ - 1), bs = lane >> 3;              // (tid & 7 == qd: a thread stages its own chain quad)
    const int c0 = cbase + 4 * qd;
    const int nc = B - c0 < 0 ? 0 : (B - c0 > 4 ? 4 : B - c0);
    const f4 tq = ld_tau(tau, tau_stride, c0, nc);
    const f4 lz = ld4(logZ + c0, nc, 0.0f);

    // staging: item i = tid + 256 j is (column b0 - db + (i >> 3), quad qd); v of that column is loaded once
    int sb[XSTAGE];
    bool sv[XSTAGE];
    f4 svb[XSTAGE];
#pragma unroll
    for (int j = 0; j < XSTAGE; ++j) {
        const int ci = (tid + XTHREADS * j) >> 3;
        sb[j] = b0 - db + ci;
        sv[j] = ci < W && sb[j] >= 0 && sb[j] < T;
        svb[j] = sv[j] ? ld4(v + (size_t)sb[j] * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
    }
    // the lane's columns of the tile
    int col[XK], bk[XK];
    i4 cn[XK];
    u64 mk[XK];
#pragma unroll
    for (int k = 0; k < XK; ++k) {
        col[k] = wave * XCOLS + bs + 8 * k;
        bk[k] = b0 + col[k];
        cn[k] = (i4)(0);
        mk[k] = 0ull;
    }

    const int rows = T - e0 < XT ? T - e0 : XT;                  // rows of this band
    const int nrr = rows + 2 * de;                               // rows walked: e0 - de .. e0 + rows - 1 + de
    f4 x[XSTAGE], qe;
    {                                                            // the loads of the first row
        const int er = e0 - de;
        const bool rok = er >= 0 && er < T;
        qe = rok ? ld4(q + (size_t)er * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
#pragma unroll
        for (int j = 0; j < XSTAGE; ++j)
            x[j] = (rok && sv[j] && sb[j] <= er) ? ld4(score + ((size_t)er * T + sb[j]) * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
    }
    int slot = 0;
    for (int rr = 0; rr < nrr; ++rr) {                           // (workgroup-uniform bounds)
        const int er = e0 - de + rr;
        const bool rok = er >= 0 && er < T;
        float* const stage = s_stage + (size_t)(rr & 1) * W * XCH;
        // every m of the row, once
#pragma unroll
        for (int j = 0; j < XSTAGE; ++j) {
            const int ci = (tid + XTHREADS * j) >> 3;
            if (ci >= W) break;
            f4 m = (f4)(0.0f);
            if (rok && sv[j] && sb[j] <= er) {                   // a cell of the triangle
                if (sb[j] == er) m = ChainVec<f4>::single(svb[j], qe, lz, x[j]);
                else m = ChainVec<f4>::cell(svb[j], x[j], qe - lz);
            }
            *(f4*)(stage + (size_t)ci * XCH + 4 * qd) = m;
        }
        // the next row's loads are in flight across the barrier and the sums
        if (rr + 1 < nrr) {
            const int en = er + 1;
            const bool nok = en >= 0 && en < T;
            qe = nok ? ld4(q + (size_t)en * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
#pragma unroll
            for (int j = 0; j < XSTAGE; ++j)
                x[j] = (nok && sv[j] && sb[j] <= en) ? ld4(score + ((size_t)en * T + sb[j]) * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
        }
        __syncthreads();                                         // one barrier per row: the buffer written now is read below and not
                                                                 // written again before the barrier after the next one
        float* const ring = s_ring + (size_t)slot * XT * XCH;
#pragma unroll
        for (int k = 0; k < XK; ++k) {
            const float* p = stage + (size_t)col[k] * XCH + 4 * qd;            // column bk - db of the staged row
            f4 row = (f4)(0.0f);
            for (int j = 0; j < 2 * db + 1; ++j) row += *(const f4*)(p + (size_t)j * XCH);
            *(f4*)(ring + (size_t)col[k] * XCH + 4 * qd) = row;
        }
        if (rr >= 2 * de) {                                      // rows e - de .. e + de are in the ring: oldest first
            const int r = rr - 2 * de, e = e0 + r;
#pragma unroll
            for (int k = 0; k < XK; ++k) {
                f4 acc = (f4)(0.0f);
                int s = slot + 1 == R ? 0 : slot + 1;
                for (int i = 0; i < R; ++i) {
                    acc += *(const f4*)(s_ring + ((size_t)s * XT + col[k]) * XCH + 4 * qd);
                    s = s + 1 == R ? 0 : s + 1;
                }
                const f4 M = ChainVec<f4>::clamp(acc);
                const bool cell = bk[k] <= e;
                bool any = false;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const bool sel = cell && M[ch] >= tq[ch];    // NaN on either side: not selected
                    cn[k][ch] += sel ? 1 : 0;
                    any = any || sel;
                }
                mk[k] |= (u64)(any ? 1 : 0) << r;
            }
        }
        slot = slot + 1 == R ? 0 : slot + 1;
    }

    if (nc > 0) {
#pragma unroll
        for (int k = 0; k < XK; ++k)
            if (bk[k] < T) {
                sti4(cnt + ((size_t)ti * T + bk[k]) * Bs + c0, nc, cn[k]);
                mask[((size_t)ti * T + bk[k]) * NQ + (c0 >> 2)] = mk[k];
            }
    }
}

// grid (ceil(64 NQ / 256), ntiles), block 256: thread = (column of the tile, chain quad), the quad fastest
__global__ __launch_bounds__(256) void mtol_write_kernel(const float* __restrict__ score, const float* __restrict__ v,
                                                         const float* __restrict__ q, const float* __restrict__ logZ, int T, int B,
                                                         const float* __restrict__ tau, int tau_stride, int NQ, int db, int de,
                                                         const int* __restrict__ cntx, const int* __restrict__ colbase,
                                                         const u64* __restrict__ mask, const int* __restrict__ offsets,
                                                         int* __restrict__ pairs, float* __restrict__ probs, long long cap)
{
    const int id = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (id >= XT * NQ) return;
    const int quad = id % NQ, colt = id / NQ;
    int ti, tj;
    tile_of((int)blockIdx.y, ti, tj);
    const int b = tj * XT + colt;
    if (b >= T) return;
    u64 mk = mask[((size_t)ti * T + b) * NQ + quad];
    if (mk == 0ull) return;
    const size_t Bs = (size_t)B;
    const int c0 = 4 * quad;
    const int nc = B - c0 > 4 ? 4 : B - c0;
    const f4 lz = ld4(logZ + c0, nc, 0.0f);
    const f4 tq = ld_tau(tau, tau_stride, c0, nc);
    const i4 o = ldi4(offsets + c0, nc), cb = ldi4(colbase + (size_t)b * Bs + c0, nc), cx = ldi4(cntx + ((size_t)ti * T + b) * Bs + c0, nc);
    long long pos[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) pos[ch] = (long long)o[ch] + cb[ch] + cx[ch];
    while (mk) {
        const int r = __ffsll((long long)mk) - 1;
        mk &= mk - 1ull;
        const int e = ti * XT + r;
        const f4 M = tol_marginal<f4>(score, v, q, lz, T, Bs, c0, nc, b, e, db, de);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch >= nc) break;
            if (M[ch] >= tq[ch]) {
                const long long p = pos[ch]++;
                if (p >= 0 && p < cap) {
                    pairs[2 * p] = b;
                    pairs[2 * p + 1] = e;
                    probs[p] = M[ch];
                }
            }
        }
    }
}

void launch_interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int* pairs,
                                   int K, const int* offsets, int db, int de, float* out, hipStream_t stream)
{
    if (K <= 0) return;
    mtol_gather_kernel<<<(K + 255) / 256, 256, 0, stream>>>(score, v, q, logZ, T, B, pairs, K, offsets, db, de, out);
}

// the workspace of semicrf_marginal_decode: cnt [nI][T][B] i32, mask [nI][T][ceil(B/4)] u64, coltot [T][B] i32, tot [B] i32
size_t marginal_decode_tol_workspace_bytes(int T, int B) { return marginal_decode_workspace_bytes(T, B); }

void launch_marginal_decode_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                                int tau_stride, int db, int de, int* pairs, float* probs, long long cap, int* offsets, void* ws,
                                hipStream_t stream)
{
    const int nI = (T + XT - 1) / XT, ntiles = nI * (nI + 1) / 2, NQ = (B + 3) / 4;
    const size_t Bs = (size_t)B;
    char* w = (char*)ws;
    int* cnt = (int*)w;
    w += align_up((size_t)nI * T * Bs * 4);
    u64* mask = (u64*)w;
    w += align_up((size_t)nI * T * NQ * 8);
    int* coltot = (int*)w;
    w += align_up((size_t)T * Bs * 4);
    int* tot = (int*)w;
    static PerDeviceOnce attr_once;
    if (attr_once.first())
        (void)hipFuncSetAttribute((const void*)mtol_count_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (2 * (XT + 2 * XTOL) + XT * (2 * XTOL + 1)) * XCH * 4);
    const size_t lds = (size_t)(2 * (XT + 2 * db) + XT * (2 * de + 1)) * XCH * 4;
    mtol_count_kernel<<<dim3((B + XCH - 1) / XCH, ntiles), XTHREADS, lds, stream>>>(score, v, q, logZ, T, B, tau, tau_stride, NQ, db, de, cnt,
                                                                                   mask);
    marginal_decode_scans(cnt, coltot, tot, v, T, B, offsets, stream);
    mtol_write_kernel<<<dim3((XT * NQ + 255) / 256, ntiles), 256, 0, stream>>>(score, v, q, logZ, T, B, tau, tau_stride, NQ, db, de, cnt,
                                                                              coltot, mask, offsets, pairs, probs, cap);
}

}  // namespace semicrf
