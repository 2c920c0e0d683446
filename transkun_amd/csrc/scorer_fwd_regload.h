// scorer_fwd_regload.h -- the register-load forward kernel (any alignment, any D % 64 == 0) and the XCD-aware work list it shares
// with the streaming kernel.  Included by scorer_mfma.hip.
#pragma once
#include "scorer_fwd_common.h"

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace semicrf {

// Work list (XCD-aware): workgroups are dispatched round-robin over the 8 XCDs, each with its own 4 MB L2, and the
// operands are heavy (a 32-row tile of q or k for 16 chains is 512 KB at D=256) while HBM delivers only ~10 B/clk/CU --
// a third of what the matrix pipe consumes with 32x32 tiles.  So the host orders the tiles such that the workgroups
// resident on ONE XCD at a time work on a band of SBAND tile rows of one chain group, column by column: the band's q
// tiles stay in that L2 and each k tile is fetched once for the SBAND workgroups that use it back to back.
// work[blockIdx.x] = {et | bt << 16, chain group} (et < 0: padding).
// NCH = chunks of 32 contraction values per half-wave (D / 64) when known at compile time (<= 4), else 0: with a
// compile-time trip count the two-stage load/multiply pipeline unrolls without branches and every wait is exact
template <bool ALIGNED, int NCH>
__global__ __launch_bounds__(256) void interval_score_mfma_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ diag, int C, int T, int D,
    long long ldq, long long ldk, long long ldd, float qscale, int mode, int full, float* __restrict__ S,
    const int2* __restrict__ work)
{
    extern __shared__ __attribute__((aligned(16))) float tile[];   // [ST*ST][SPAD]
    const int2 wk = work[blockIdx.x];
    if (wk.x < 0) return;
    const int et = wk.x & 0xffff, bt = wk.x >> 16;
    const int e0 = et * ST, b0 = bt * ST;
    const int cg = wk.y * SC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = lane & 31, half = lane >> 5;
    const int Dh = D >> 1;                                  // d range of this half-wave: [half*Dh, half*Dh + Dh)
    const int er = e0 + row < T ? e0 + row : T - 1;         // clamped rows (masked at the write)
    const int br = b0 + row < T ? b0 + row : T - 1;

    for (int round = 0; round < SC / 4; ++round) {
        const int ci = wave + 4 * round;
        const int c = cg + ci < C ? cg + ci : C - 1;
        const float* qp = q + ((size_t)c * T + er) * ldq + (size_t)half * Dh;
        const float* kp = k + ((size_t)c * T + br) * ldk + (size_t)half * Dh;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
        // chunks of 32 d-values per half-wave: 8 float4 of q and of k per lane; the next chunk is requested
        // before the 32 MFMAs of the current one so that the loads hide under the matrix pipe
        auto load_chunk = [&](float4 (&qa)[8], float4 (&ka)[8], int d0) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const float* qq = qp + d0 + 4 * m;
                const float* kk = kp + d0 + 4 * m;
                if (ALIGNED) {
                    qa[m] = *(const float4*)qq;
                    ka[m] = *(const float4*)kk;
                } else {                      // rows only 4-byte aligned (packed Linear output, ld = 2D+1)
                    qa[m] = make_float4(qq[0], qq[1], qq[2], qq[3]);
                    ka[m] = make_float4(kk[0], kk[1], kk[2], kk[3]);
                }
            }
        };
        auto mma_chunk = [&](const float4 (&qa)[8], const float4 (&ka)[8]) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].x, ka[m].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].y, ka[m].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].z, ka[m].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m].w, ka[m].w, acc, 0, 0, 0);
            }
        };
        float4 qa0[8], ka0[8], qa1[8], ka1[8];
        load_chunk(qa0, ka0, 0);
        if (NCH > 0) {
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                if (ch & 1) {
                    if (ch + 1 < NCH) load_chunk(qa0, ka0, (ch + 1) * 32);
                    __builtin_amdgcn_sched_barrier(0);
                    mma_chunk(qa1, ka1);
                } else {
                    if (ch + 1 < NCH) load_chunk(qa1, ka1, (ch + 1) * 32);
                    __builtin_amdgcn_sched_barrier(0);
                    mma_chunk(qa0, ka0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        } else {
            for (int d0 = 0; d0 < Dh; d0 += 64) {
                if (d0 + 32 < Dh) load_chunk(qa1, ka1, d0 + 32);
                mma_chunk(qa0, ka0);
                if (d0 + 32 >= Dh) break;
                if (d0 + 64 < Dh) load_chunk(qa0, ka0, d0 + 64);
                mma_chunk(qa1, ka1);
            }
        }
        // C/D layout of 32x32: col j = lane & 31, row i = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
        const int bj = lane & 31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ei = (r & 3) + 8 * (r >> 2) + 4 * half;
            const int e = e0 + ei, b = b0 + bj;
            float v = acc[r] * qscale;
            const int len = e > b ? e - b : b - e;
            v *= len_scale_mfma(len, mode);
            if (e == b && e < T) v += diag[((size_t)c * T + e) * ldd];
            tile[(ei * ST + bj) * SPAD + ci] = v;
        }
    }
    __syncthreads();
    // write out: 4 threads per cell (4 chains each), chain axis contiguous
    const int nq = SC / 4;
    for (int idx = threadIdx.x; idx < ST * ST * nq; idx += 256) {
        const int cell = idx / nq, qd = idx % nq;
        const int ei = cell / ST, bj = cell % ST;
        const int e = e0 + ei, b = b0 + bj;
        if (e >= T || b >= T || (!full && b > e)) continue;
        float* dst = S + ((size_t)e * T + b) * C + cg + qd * 4;
        const float* src = tile + cell * SPAD + qd * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (cg + qd * 4 + i < C) dst[i] = src[i];
    }
}

// builds (once per device and shape) the device-resident work list described above.  The cache holds the SCORE_WL_MAX most
// recently used lists (least recently used one freed first), the upload is enqueued on the caller's stream (from a pageable
// staging vector kept alive in the cache entry), and a failed upload frees the allocation.  The first call for a shape
// allocates (hipMalloc: not stream-capturable); later calls only look the list up.
constexpr size_t SCORE_WL_MAX = 16;
struct ScoreWorkList { int2* dev = nullptr; int n = 0; unsigned long long stamp = 0; std::vector<int2> host; };

static const int2* score_work_list(int nt, int ngroups, int full, int band, int* grid_out, hipStream_t stream)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int, int>, ScoreWorkList> cache;
    static unsigned long long clock = 0;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(dev, nt, ngroups, full, band);
    auto it = cache.find(key);
    if (it != cache.end()) { it->second.stamp = ++clock; *grid_out = it->second.n; return it->second.dev; }
    // units: (chain group, pair of bands p and nb-1-p) -- equal work per unit in the triangle
    const int nb = (nt + band - 1) / band;
    std::vector<std::vector<int2>> per(NXCD);
    int u = 0;
    auto add_band = [&](std::vector<int2>& out, int g, int j) {
        const int r0 = j * band, r1 = (r0 + band < nt) ? r0 + band : nt;
        const int ncol = full ? nt : r1;                 // columns 0 .. r1-1 (bt <= et)
        for (int bt = 0; bt < ncol; ++bt)
            for (int et = r0; et < r1; ++et)
                if (full || bt <= et) out.push_back(make_int2(et | (bt << 16), g));
    };
    for (int g = 0; g < ngroups; ++g)
        for (int p = 0; p < (nb + 1) / 2; ++p, ++u) {
            std::vector<int2>& out = per[u % NXCD];
            add_band(out, g, p);
            if (nb - 1 - p != p) add_band(out, g, nb - 1 - p);
        }
    size_t longest = 0;
    for (auto& v : per) longest = v.size() > longest ? v.size() : longest;
    ScoreWorkList e;
    e.host.assign(longest * NXCD, make_int2(-1, 0));
    for (int x = 0; x < NXCD; ++x)
        for (size_t i = 0; i < per[x].size(); ++i) e.host[i * NXCD + x] = per[x][i];
    if (cache.size() >= SCORE_WL_MAX) {                  // evict the least recently used list of this process
        auto lru = cache.begin();
        for (auto c = cache.begin(); c != cache.end(); ++c)
            if (c->second.stamp < lru->second.stamp) lru = c;
        // kernels that still read the list were enqueued before this call: free after they have drained
        (void)hipStreamSynchronize(stream);
        (void)hipFree(lru->second.dev);
        cache.erase(lru);
    }
    if (hipMalloc((void**)&e.dev, e.host.size() * sizeof(int2)) != hipSuccess) return nullptr;
    e.n = (int)e.host.size();
    e.stamp = ++clock;
    auto ins = cache.emplace(key, std::move(e)).first;          // the staging vector lives on in the cache entry
    if (hipMemcpyAsync(ins->second.dev, ins->second.host.data(), ins->second.host.size() * sizeof(int2), hipMemcpyHostToDevice,
                       stream) != hipSuccess) {
        (void)hipFree(ins->second.dev);
        cache.erase(ins);
        return nullptr;
    }
    *grid_out = ins->second.n;
    return ins->second.dev;
}

}  // namespace semicrf
