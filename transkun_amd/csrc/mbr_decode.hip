// mbr_decode.hip -- posterior (minimum-Bayes-risk) PATH decoding at any threshold (include/semicrf_hip.h: semicrf_mbr_select): among
// all paths of a chain the one that maximises the sum over its intervals of (m - tau), by a weighted-interval-scheduling dynamic
// program over the packed lattice semicrf_marginal_decode emits (pairs / probs / offsets, ascending by (begin, end)).  Neither the
// scores nor a [T][T][B] tensor are read: the input is at most T (floor(1 / tau) + 1) cells per chain.
//
//   F[T-1] = gS(T-1);  F[t] = max(F[t+1], max over the eligible (t, e), e > t, of g + F[e]) + gS(t)     (fp32, one add per sum)
//   g = weight - tau of an eligible entry (weight > tau), gS(t) = g of the eligible (t, t) or +0; ties: the skip, then the smallest e.
//
//   mbr_dp_kernel     one wave per chain.  The recursion is a T-long dependent chain with a handful of candidates per frame:
//                     latency-bound, not byte-bound.  F lives in LDS (4 bytes per frame; in the workspace for T > MBR_LDS_T); the
//                     chain's lattice slice is streamed BACKWARDS 64 entries at a time, one entry per lane (coalesced 8- and 4-byte
//                     loads).  Only frames that hold an eligible entry are visited one by one: the next one is the begin of the
//                     highest remaining lane (a ballot), the frames in between have F = F of the frame above them (x + 0 is exact)
//                     and are filled 64 at a time.  At a visited frame the lanes of its entries read F[e] together; the maximum is
//                     then taken over those lanes from the highest index down -- "take if larger, or equal and the holder is not
//                     the skip" -- which leaves the skip, then the smallest e among equal maxima, also when a frame's entries
//                     straddle two 64-entry pieces (the state of the open frame is wave-uniform and carried across).
//                     Per frame it leaves code[c][t] = (e + 1 of the chosen interval, 0 = skip) | (singleton ? CODE_DIAG : 0) --
//                     the layout decode.hip walks -- and idx[c][t] = the lattice indices of (the chosen interval, the singleton).
//   the trace         decode.hip's launch_backtrack (forward = 0): the walk from frame 0, the offsets over the chains and the packing
//                     of pairs_out, with offsets_out[B] = -1 through its error word when the lattice is invalid.
//   mbr_probs_kernel  probs_out[i] = weight[idx of the packed pair i]: the selected entries' weights, bit for bit.
// No atomics: every word has one writer and every comparison a fixed order; the result is a pure function of the inputs.
//
// Registers / scratch (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): see DESIGN.md §3 "MBR path decoding".
#include "common.h"
#include "launchers.h"

namespace semicrf {

namespace {
constexpr int MBR_CODE_DIAG = 0x40000000;   // decode.hip: CODE_DIAG
constexpr int MBR_LDS_T = 4096;             // F in LDS up to this many frames (16 KB per chain: ten chains per CU)

typedef unsigned long long u64;

__device__ __forceinline__ int lane_i(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ float lane_f(float x, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), l)); }
__device__ __forceinline__ int top_bit(u64 m) { return 63 - __clzll((long long)m); }
}  // namespace

// grid B, block 64.  gF: [B][T] floats when !IN_LDS.  flag: decode.hip's error word (0xffffffff = fine).
template <bool IN_LDS>
__global__ __launch_bounds__(64) void mbr_dp_kernel(const int* __restrict__ pairs, const float* __restrict__ weight,
                                                    const int* __restrict__ offsets, long long K, int T, int B,
                                                    const float* __restrict__ tau, int tau_stride, float* __restrict__ gF,
                                                    int* __restrict__ code, int2* __restrict__ idx, unsigned* __restrict__ flag,
                                                    float* __restrict__ gain)
{
    extern __shared__ float s_F[];
    const int c = (int)blockIdx.x, lane = (int)threadIdx.x;
    float* const F = IN_LDS ? s_F : gF + (size_t)c * T;
    int* const cd = code + (size_t)c * T;
    int2* const ix = idx + (size_t)c * T;

    const int total = offsets[B];
    const bool ok = total >= 0 && (long long)total <= K;     // negative: the sweeps' NaN convention; > K: a truncated lattice
    if (c == 0 && lane == 0) *flag = ok ? 0xffffffffu : 0u;
    int lo = ok ? offsets[c] : 0, hi = ok ? offsets[c + 1] : 0;
    lo = lo < 0 ? 0 : (lo > total ? total : lo);             // (a well-formed lattice is untouched; nothing is read past `total`)
    hi = hi < lo ? lo : (hi > total ? total : hi);
    const float th = tau[(size_t)c * tau_stride];

    // the open frame t: best / key over the candidates seen so far (key = e of the holder, -1 = the skip), kidx its lattice
    // index, gs / sidx the singleton; everything below is wave-uniform.  "F[T]" = +0: F[T-1] = 0 + gS(T-1) = gS(T-1).
    int t = T - 1, key = -1, kidx = -1, sidx = -1;
    float best = 0.0f, gs = 0.0f;

    // closes the open frame and fills the frames down to (not including) tn with its F; opens tn
    auto close_to = [&](int tn) {
        const float Ft = best + gs;
        for (int u = t - lane; u > tn; u -= 64) {
            const bool own = u == t;
            F[u] = Ft;
            cd[u] = own ? (key + 1) | (sidx >= 0 ? MBR_CODE_DIAG : 0) : 0;
            ix[u] = own ? make_int2(kidx, sidx) : make_int2(-1, -1);
        }
        t = tn; best = Ft; key = -1; kidx = -1; sidx = -1; gs = 0.0f;
    };

    for (int top = hi; top > lo; top -= 64) {                // the piece [max(lo, top - 64), top), one entry per lane
        const int base = top - 64, i = base + lane;
        const bool valid = i >= lo;
        int b = -1, e = -1;
        float w = 0.0f;
        if (valid) {
            const int2 p = ((const int2*)pairs)[i];
            b = p.x; e = p.y; w = weight[i];
        }
        const bool el = valid && w > th && b >= 0 && b <= e && e < T;      // NaN on either side: not eligible
        const float g = w - th;
        u64 m = __ballot(el && b <= t);                      // (sorted input: every eligible lane)
        while (m) {
            const int tn = lane_i(b, top_bit(m));            // the next frame that holds an eligible entry
            if (tn > t) {                                    // (an unsorted lattice: the entry is dropped, every jump stays forward)
                m &= ~(1ull << top_bit(m));
                continue;
            }
            if (tn < t) close_to(tn);
            const u64 fm = __ballot(el && b == tn) & m;
            const u64 sm = __ballot(el && b == tn && e == tn) & m;
            if (sm) {
                const int ls = __ffsll((long long)sm) - 1;
                gs = lane_f(g, ls);
                sidx = base + ls;
            }
            u64 im = fm & ~sm;
            if (im) {
                __syncthreads();                             // one wave: orders the fills above against the reads of F[e]
                const float cand = ((im >> lane) & 1ull) ? g + F[e] : 0.0f;
                while (im) {
                    const int l2 = top_bit(im);
                    const float cv = lane_f(cand, l2);
                    if (cv > best || (cv == best && key >= 0)) {
                        best = cv;
                        key = lane_i(e, l2);
                        kidx = base + l2;
                    }
                    im &= ~(1ull << l2);
                }
            }
            m &= ~fm;
        }
    }
    close_to(-1);
    if (lane == 0) gain[c] = best;                           // (close_to left F[0] there)
}

// grid B, block 256: probs_out of the packed pairs of chain c
__global__ __launch_bounds__(256) void mbr_probs_kernel(const float* __restrict__ weight, const int2* __restrict__ idx, int T,
                                                        const int* __restrict__ pairs_out, const int* __restrict__ offsets_out,
                                                        float* __restrict__ probs_out, long long cap)
{
    const int c = (int)blockIdx.x;
    const long long lo = offsets_out[c];
    long long hi = offsets_out[c + 1];
    if (hi < 0) return;                                      // the invalid-lattice total; every count is 0 then
    if (hi > cap) hi = cap;
    const int2* ix = idx + (size_t)c * T;
    for (long long d = lo + (int)threadIdx.x; d < hi; d += 256) {
        const int b = pairs_out[2 * d], e = pairs_out[2 * d + 1];
        const int2 k = ix[b];
        probs_out[d] = weight[b == e ? k.y : k.x];
    }
}

// code [B][T] i32, idx [B][T] int2, region [B][2T][2] i32, counts [B] i32, the error word; F [B][T] f32 for T > MBR_LDS_T
size_t mbr_select_workspace_bytes(int T, int B)
{
    const size_t TB = (size_t)T * B;
    return align_up(TB * 4) + align_up(TB * 8) + align_up(TB * 2 * 2 * 4) + align_up((size_t)B * 4) + 256 +
           (T > MBR_LDS_T ? align_up(TB * 4) : 0);
}

void launch_mbr_select(const int* pairs, const float* weight, const int* offsets, long long K, int T, int B, const float* tau,
                       int tau_stride, int* pairs_out, float* probs_out, long long cap, int* offsets_out, float* gain, void* ws,
                       hipStream_t stream)
{
    const size_t TB = (size_t)T * B;
    char* w = (char*)ws;
    int* code = (int*)w;
    w += align_up(TB * 4);
    int2* idx = (int2*)w;
    w += align_up(TB * 8);
    int* region = (int*)w;
    w += align_up(TB * 2 * 2 * 4);
    int* counts = (int*)w;
    w += align_up((size_t)B * 4);
    unsigned* flag = (unsigned*)w;
    w += 256;
    float* gF = (float*)w;
    if (T <= MBR_LDS_T)
        mbr_dp_kernel<true><<<B, 64, (size_t)T * sizeof(float), stream>>>(pairs, weight, offsets, K, T, B, tau, tau_stride, nullptr, code,
                                                                          idx, flag, gain);
    else
        mbr_dp_kernel<false><<<B, 64, 0, stream>>>(pairs, weight, offsets, K, T, B, tau, tau_stride, gF, code, idx, flag, gain);
    launch_backtrack(code, T, B, nullptr, 0, region, counts, pairs_out, cap, offsets_out, stream, flag, 1, 0);
    mbr_probs_kernel<<<B, 256, 0, stream>>>(weight, idx, T, pairs_out, offsets_out, probs_out, cap);
}

}  // namespace semicrf
