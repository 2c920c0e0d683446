// marginal_decode.hip -- marginal-threshold (posterior) decoding of the semi-CRF (include/semicrf_hip.h: semicrf_marginal_decode):
// every cell (e, b), b <= e, whose marginal m(e, b) is >= tau, packed chain-major and ascending by (begin, end) -- a deterministic
// stream compaction of the lower triangle.  m is posterior_cell.h's cell_marginal / cell_marginal_single, the functions
// semicrf_interval_marginals evaluates: the compared value is that entry point's value bit for bit.
//
// The triangle is read ONCE.  Pass 1 streams it in posterior.hip's tiles and leaves, per (row band ti, column b), the number of
// selected cells of every chain and -- per chain quad -- a 64-bit row mask "some chain of the quad selected (ti * 64 + r, b)";
// the scans turn the counts into positions; pass 2 visits only the rows of the masks (of the order of 1e-3 of the triangle at
// tau >= 0.3), re-evaluates those cells with the same functions and writes them.
//
//   mdec_count_kernel    one 64 x 64 (end x begin) tile x 32 chains per workgroup of 4 waves.  Lane = (chain quad qd: 4 neighbouring
//                        chains read as one 16-byte piece, column slot bs); wave w owns the 16 columns b0 + 16 w + bs + 8 k, k < 2,
//                        and walks ALL 64 rows of them (2 rows of loads in flight), so the count and the mask of a tile column are
//                        lane-local: no cross-lane or cross-wave step, one writer per word.  A[e] = q[e] - logZ is staged in LDS
//                        once per tile, v[b] loaded once per tile.  The diagonal tiles take the singletons (b == e).
//   mdec_colscan_kernel  per (column b, chain): the exclusive prefix of the counts over the row bands, in place; the column's total.
//   mdec_rowscan_kernel  per chain: the exclusive prefix of the column totals over b, in place (64 segments of b per chain, combined
//                        in segment order through LDS); the chain's total.
//   mdec_offsets_kernel  offsets = the exclusive prefix of the chains' totals (one workgroup); offsets[B] = -1 if alpha's last row
//                        holds NaN.
//   mdec_write_kernel    one thread per (tile, column, chain quad) with a non-empty mask: position of chain c's first cell of that
//                        tile column = offsets[c] + prefix[b][c] + bandprefix[ti][b][c]; the rows of the mask in ascending order.
// The order (begin, end) -- not (end, begin) -- is what makes the rank inside a tile column a running count of one lane.
// No atomics: every word has one writer and every sum a fixed order; the result is a pure function of the inputs.
// marginal_tol.hip (semicrf_marginal_decode_tol) reuses the scans and the workspace layout with a count and a write pass of its own.
#include "common.h"
#include "launchers.h"
#include "posterior_cell.h"

namespace semicrf {

namespace {
constexpr int MT = 64;                      // tile edge (frames), rows and columns
constexpr int MQ = 8;                       // chain quads per wave (32 chains)
constexpr int MCH = 4 * MQ;
constexpr int MWAVES = 4;                   // waves per workgroup; each takes MT / MWAVES columns of the tile
constexpr int MCOLS = MT / MWAVES;
constexpr int MK = MCOLS / 8;               // columns per lane
constexpr int MRB = 2;                      // rows whose loads are issued together
constexpr int MSEG = 64;                    // rowscan: segments of b per chain
constexpr int MRC = 16;                     // rowscan: chains per workgroup

// (f4, ld4, tile_of, i4, u64, ldi4, sti4, ld_tau: posterior_cell.h)
}  // namespace

// grid (ceil(B/32), nI (nI+1)/2), block 256.  cnt [nI][T][B]: cnt[i][b] = selected cells of tile column (i, b);
// mask [nI][T][NQ], NQ = ceil(B/4): bit r of mask[i][b][quad] = some chain of the quad selected the cell (64 i + r, b).
__global__ __launch_bounds__(64 * MWAVES) void mdec_count_kernel(const float* __restrict__ score, const float* __restrict__ v,
                                                                 const float* __restrict__ q, const float* __restrict__ logZ, int T, int B,
                                                                 const float* __restrict__ tau, int tau_stride, int NQ,
                                                                 int* __restrict__ cnt, u64* __restrict__ mask)
{
    __shared__ __attribute__((aligned(16))) float s_A[MT][MCH];
    int ti, tj;
    tile_of((int)blockIdx.y, ti, tj);
    const int e0 = ti * MT, b0 = tj * MT;
    const int cbase = (int)blockIdx.x * MCH;
    const size_t Bs = (size_t)B;

    for (int k = (int)threadIdx.x; k < MT * MCH; k += 64 * MWAVES) {
        const int r = k / MCH, cc = k % MCH, e = e0 + r, c = cbase + cc;
        s_A[r][cc] = (e < T && c < B) ? q[(size_t)e * Bs + c] - logZ[c] : SEMICRF_NEG_INF;
    }
    __syncthreads();

    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int qd = lane & (MQ - 1), bs = lane >> 3;
    const int c0 = cbase + 4 * qd;
    const int nc = B - c0 < 0 ? 0 : (B - c0 > 4 ? 4 : B - c0);
    const bool diag = ti == tj;
    const f4 tq = ld_tau(tau, tau_stride, c0, nc);

    int bk[MK];
    f4 vb[MK];
    i4 cn[MK];
    u64 mk[MK];
#pragma unroll
    for (int k = 0; k < MK; ++k) {
        bk[k] = b0 + wave * MCOLS + bs + 8 * k;
        vb[k] = bk[k] < T ? ld4(v + (size_t)bk[k] * Bs + c0, nc, SEMICRF_NEG_INF) : (f4)(SEMICRF_NEG_INF);
        cn[k] = (i4)(0);
        mk[k] = 0ull;
    }

    const int rend = T - e0 < MT ? T - e0 : MT;              // rows of this band
    const int rbeg = diag ? wave * MCOLS : 0;                // diagonal tile: the rows above the wave's first column hold no cell
    for (int r = rbeg; r < rend; r += MRB) {                 // (wave-uniform bounds; rbeg is a multiple of MRB)
        f4 x[MRB][MK];
#pragma unroll
        for (int i = 0; i < MRB; ++i) {
            const int e = e0 + r + i;
#pragma unroll
            for (int k = 0; k < MK; ++k)                     // b <= e < T: a cell of the triangle
                x[i][k] = (r + i < rend && bk[k] <= e) ? ld4(score + ((size_t)e * T + bk[k]) * Bs + c0, nc, SEMICRF_NEG_INF)
                                                       : (f4)(SEMICRF_NEG_INF);
        }
#pragma unroll
        for (int i = 0; i < MRB; ++i) {
            if (r + i >= rend) break;
            const int e = e0 + r + i;
            const f4 A = *(const f4*)&s_A[r + i][4 * qd];
#pragma unroll
            for (int k = 0; k < MK; ++k) {
                f4 m;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) m[ch] = cell_marginal(vb[k][ch], x[i][k][ch], A[ch]);
                if (diag && bk[k] == e) {                    // the singleton: one column of one wave per row of a diagonal tile
                    const f4 qe = ld4(q + (size_t)e * Bs + c0, nc, SEMICRF_NEG_INF), lz = ld4(logZ + c0, nc, 0.0f);
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) m[ch] = cell_marginal_single(vb[k][ch], qe[ch], lz[ch], x[i][k][ch]);
                }
                const bool cell = bk[k] <= e;
                bool any = false;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const bool sel = cell && m[ch] >= tq[ch];           // NaN on either side: not selected
                    cn[k][ch] += sel ? 1 : 0;
                    any = any || sel;
                }
                mk[k] |= (u64)(any ? 1 : 0) << (r + i);
            }
        }
    }

    if (nc > 0) {
#pragma unroll
        for (int k = 0; k < MK; ++k)
            if (bk[k] < T) {
                sti4(cnt + ((size_t)ti * T + bk[k]) * Bs + c0, nc, cn[k]);
                mask[((size_t)ti * T + bk[k]) * NQ + (c0 >> 2)] = mk[k];
            }
    }
}

// one thread per (b, chain): cnt[i][b][c], i >= b / 64, becomes its exclusive prefix over i; coltot[b][c] = the column's total
__global__ __launch_bounds__(256) void mdec_colscan_kernel(int* __restrict__ cnt, int T, int B, int nI, int* __restrict__ coltot)
{
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, TB = (size_t)T * B;
    if (idx >= TB) return;
    const int b = (int)(idx / (size_t)B);
    int run = 0;
    for (int i = b / MT; i < nI; ++i) {
        int* p = cnt + (size_t)i * TB + idx;
        const int n = *p;
        *p = run;
        run += n;
    }
    coltot[idx] = run;
}

// grid ceil(B/MRC), block MRC * MSEG: thread = (segment of b, chain), the chain fastest (64-byte pieces of a row).
// coltot[b][c] becomes its exclusive prefix over b; tot[c]
__global__ __launch_bounds__(MRC * MSEG) void mdec_rowscan_kernel(int* __restrict__ coltot, int T, int B, int* __restrict__ tot)
{
    __shared__ int s_part[MSEG][MRC];
    const int cc = (int)threadIdx.x % MRC, seg = (int)threadIdx.x / MRC;
    const int c = (int)blockIdx.x * MRC + cc;
    const int L = (T + MSEG - 1) / MSEG;
    const int lo = seg * L < T ? seg * L : T, hi = lo + L < T ? lo + L : T;
    int sum = 0;
    if (c < B) {
#pragma unroll 8
        for (int b = lo; b < hi; ++b) sum += coltot[(size_t)b * B + c];
    }
    s_part[seg][cc] = sum;
    __syncthreads();
    int run = 0;
    for (int s = 0; s < seg; ++s) run += s_part[s][cc];
    if (c < B) {
        if (seg == MSEG - 1) tot[c] = run + sum;
#pragma unroll 8
        for (int b = lo; b < hi; ++b) {
            int* p = coltot + (size_t)b * B + c;
            const int n = *p;
            *p = run;
            run += n;
        }
    }
}

// one workgroup of 1024: offsets[c] = sum of tot[< c]; offsets[B] = the total, or -1 when alpha's last row holds NaN
__global__ __launch_bounds__(1024) void mdec_offsets_kernel(const int* __restrict__ tot, const float* __restrict__ v, int T, int B,
                                                            int* __restrict__ offsets)
{
    __shared__ int s_x[1024];
    __shared__ int s_carry, s_bad;
    const int tid = (int)threadIdx.x;
    if (tid == 0) { s_carry = 0; s_bad = 0; }
    __syncthreads();
    for (int base = 0; base < B; base += 1024) {
        const int c = base + tid;
        const int x = c < B ? tot[c] : 0;
        if (c < B) {
            const float vl = v[(size_t)(T - 1) * B + c];
            if (vl != vl) s_bad = 1;                         // (every writer stores the same value)
        }
        s_x[tid] = x;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            const int y = tid >= d ? s_x[tid - d] : 0;
            __syncthreads();
            s_x[tid] += y;
            __syncthreads();
        }
        const int incl = s_x[tid], carry = s_carry;
        if (c < B) offsets[c] = carry + incl - x;
        __syncthreads();
        if (tid == 1023) s_carry = carry + incl;
        __syncthreads();
    }
    if (tid == 0) offsets[B] = s_bad ? -1 : s_carry;
}

// grid (ceil(64 NQ / 256), ntiles), block 256: thread = (column of the tile, chain quad), the quad fastest
__global__ __launch_bounds__(256) void mdec_write_kernel(const float* __restrict__ score, const float* __restrict__ v,
                                                         const float* __restrict__ q, const float* __restrict__ logZ, int T, int B,
                                                         const float* __restrict__ tau, int tau_stride, int NQ,
                                                         const int* __restrict__ cntx, const int* __restrict__ colbase,
                                                         const u64* __restrict__ mask, const int* __restrict__ offsets,
                                                         int* __restrict__ pairs, float* __restrict__ probs, long long cap)
{
    const int id = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (id >= MT * NQ) return;
    const int quad = id % NQ, col = id / NQ;
    int ti, tj;
    tile_of((int)blockIdx.y, ti, tj);
    const int b = tj * MT + col;
    if (b >= T) return;
    u64 mk = mask[((size_t)ti * T + b) * NQ + quad];
    if (mk == 0ull) return;
    const size_t Bs = (size_t)B;
    const int c0 = 4 * quad;
    const int nc = B - c0 > 4 ? 4 : B - c0;
    const f4 vb = ld4(v + (size_t)b * Bs + c0, nc, SEMICRF_NEG_INF), lz = ld4(logZ + c0, nc, 0.0f);
    const f4 tq = ld_tau(tau, tau_stride, c0, nc);
    const i4 o = ldi4(offsets + c0, nc), cb = ldi4(colbase + (size_t)b * Bs + c0, nc), cx = ldi4(cntx + ((size_t)ti * T + b) * Bs + c0, nc);
    long long pos[4];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) pos[ch] = (long long)o[ch] + cb[ch] + cx[ch];
    while (mk) {
        const int r = __ffsll((long long)mk) - 1;
        mk &= mk - 1ull;
        const int e = ti * MT + r;
        const f4 x = ld4(score + ((size_t)e * T + b) * Bs + c0, nc, SEMICRF_NEG_INF), qe = ld4(q + (size_t)e * Bs + c0, nc, SEMICRF_NEG_INF);
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            if (ch >= nc) break;
            const float m = b == e ? cell_marginal_single(vb[ch], qe[ch], lz[ch], x[ch]) : cell_marginal(vb[ch], x[ch], qe[ch] - lz[ch]);
            if (m >= tq[ch]) {
                const long long p = pos[ch]++;
                if (p >= 0 && p < cap) {
                    pairs[2 * p] = b;
                    pairs[2 * p + 1] = e;
                    probs[p] = m;
                }
            }
        }
    }
}

static inline int band_count(int T) { return (T + MT - 1) / MT; }

// cnt [nI][T][B] i32, mask [nI][T][ceil(B/4)] u64, coltot [T][B] i32, tot [B] i32
size_t marginal_decode_workspace_bytes(int T, int B)
{
    const size_t nI = (size_t)band_count(T), Bs = (size_t)B, NQ = (Bs + 3) / 4;
    return align_up(nI * T * Bs * 4) + align_up(nI * T * NQ * 8) + align_up((size_t)T * Bs * 4) + align_up(Bs * 4);
}

// the scans between a count pass and a write pass (also marginal_tol.hip's): cnt and coltot become exclusive prefixes, offsets is final
void marginal_decode_scans(int* cnt, int* coltot, int* tot, const float* v, int T, int B, int* offsets, hipStream_t stream)
{
    mdec_colscan_kernel<<<(unsigned)(((size_t)T * B + 255) / 256), 256, 0, stream>>>(cnt, T, B, band_count(T), coltot);
    mdec_rowscan_kernel<<<(B + MRC - 1) / MRC, MRC * MSEG, 0, stream>>>(coltot, T, B, tot);
    mdec_offsets_kernel<<<1, 1024, 0, stream>>>(tot, v, T, B, offsets);
}

void launch_marginal_decode(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                            int tau_stride, int* pairs, float* probs, long long cap, int* offsets, void* ws, hipStream_t stream)
{
    const int nI = band_count(T), ntiles = nI * (nI + 1) / 2, NQ = (B + 3) / 4;
    const size_t Bs = (size_t)B;
    char* w = (char*)ws;
    int* cnt = (int*)w;
    w += align_up((size_t)nI * T * Bs * 4);
    u64* mask = (u64*)w;
    w += align_up((size_t)nI * T * NQ * 8);
    int* coltot = (int*)w;
    w += align_up((size_t)T * Bs * 4);
    int* tot = (int*)w;
    mdec_count_kernel<<<dim3((B + MCH - 1) / MCH, ntiles), 64 * MWAVES, 0, stream>>>(score, v, q, logZ, T, B, tau, tau_stride, NQ, cnt, mask);
    marginal_decode_scans(cnt, coltot, tot, v, T, B, offsets, stream);
    mdec_write_kernel<<<dim3((MT * NQ + 255) / 256, ntiles), 256, 0, stream>>>(score, v, q, logZ, T, B, tau, tau_stride, NQ, cnt, coltot, mask,
                                                                             offsets, pairs, probs, cap);
}

}  // namespace semicrf
