// pathstats.hip -- decoded paths against target paths on the device (include/semicrf_hip.h: semicrf_compare_paths).
//
// The reference's validation statistic (TransKun.computeStats, ModelTransformer.py:403-438) decodes, builds the Python lists and
// walks them chain by chain on the host: compareBracket (Evaluation.py:10-18, exact matches through a set) and compareFramewise
// (:21-74, interval length sums and the intersection of the two lists).  Here both lists stay packed in HBM, where semicrf_viterbi
// and the target's upload left them, and one kernel writes seven counts per chain:
//   nRef, nEst                            the list lengths
//   nExact                                pairs present in both lists
//   nRefFrames, nEstFrames, nBothFrames   the three numbers of compareFramewise(est, ref), countZero = True
//   nMatchTol                             the size of a maximum matching under an onset / offset tolerance
//
// The arithmetic, restated.  Every length sum -- of a list or of the intersection -- is one recurrence over (l, r) pieces in order:
//     s += r - l + (prevEnd < l);  prevEnd = r          (prevEnd = -1 in front of the first piece)
// i.e. an interval's frame count minus the frame it shares with a predecessor that touches it.  The reference merges an
// intersection piece into the previous one when it starts where that one ended and then sums the merged list; a merged piece is
// exactly a piece that gets no "+ 1", so the recurrence above over the UNMERGED pieces gives the same number for any input and no
// list of pieces is kept.  The intersection walk takes the closed intersection of the two heads, emits it when it is not empty and
// advances the list whose head ends first -- the reference list on a tie.
// Both lists of a chain are non-decreasing in begin and in end (checked), hence sorted by (begin, end).  Matching under a
// tolerance (tb, te) is then one merge walk: match the two heads when |b - b*| <= tb and |e - e*| <= te; otherwise drop the
// estimate's head if the reference's head is too late for it in either coordinate (so is every later reference entry), else drop
// the reference's head (it is too early for the estimate's head in some coordinate, and for every later estimate).  Two crossing
// matches can be uncrossed, so matching the heads whenever they are compatible loses nothing: the walk finds a maximum matching.
// With (0, 0) it counts the pairs the lists share, which is nExact.
//
// One thread per chain (DESIGN.md "Path comparison"): each walk is a recurrence whose next load depends on the last comparison; the
// three walks of a chain are independent of one another and advance in ONE loop, so their loads overlap.  Every pair is one 8-byte
// load.  A chain's lists are validated in full before anything is counted; no workspace, no atomics, no host synchronisation.
#include "common.h"
#include "launchers.h"

namespace semicrf {

// One list of a chain: validates it and returns its frame count.  ok stays true iff every pair has 0 <= begin <= end < T and both
// coordinates are non-decreasing along the list.
__device__ __forceinline__ unsigned scan_list(const int2* __restrict__ l, int lo, int hi, int T, bool& ok)
{
    unsigned s = 0;
    int pb = 0, pe = -1;
#pragma unroll 4
    for (int i = lo; i < hi; ++i) {
        const int2 p = l[i];
        ok = ok && p.x >= pb && p.x <= p.y && p.y < T && p.y >= pe;
        s += (unsigned)(p.y - p.x) + (pe < p.x ? 1u : 0u);
        pb = p.x; pe = p.y;
    }
    return s;
}

// a merge walk over the two lists of a chain: i / a the estimate's cursor and head, j / r the reference's
struct Walk {
    int i, j;
    int2 a, r;
};

__device__ __forceinline__ void walk_advance(Walk& w, bool adv_est, bool adv_ref, const int2* __restrict__ est, int e1,
                                             const int2* __restrict__ ref, int r1)
{
    if (adv_est) { ++w.i; if (w.i < e1) w.a = est[w.i]; }
    if (adv_ref) { ++w.j; if (w.j < r1) w.r = ref[w.j]; }
}

template <bool TOL>
__global__ __launch_bounds__(64) void compare_paths_kernel(const int2* __restrict__ est, const int* __restrict__ eoff,
                                                           const int2* __restrict__ ref, const int* __restrict__ roff, int T, int B,
                                                           int tb, int te, int* __restrict__ stats)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= B) return;
    int* out = stats + 7 * (size_t)c;
    const int etot = eoff[B], rtot = roff[B];
    const int e0 = eoff[c], e1 = eoff[c + 1], r0 = roff[c], r1 = roff[c + 1];
    // a negative total is the NaN / time-out marker of the call that produced the list; ranges outside [0, total] are never read
    bool ok = etot >= 0 && rtot >= 0 && e0 >= 0 && e0 <= e1 && e1 <= etot && r0 >= 0 && r0 <= r1 && r1 <= rtot;
    unsigned nEstF = 0, nRefF = 0;
    if (ok) nEstF = scan_list(est, e0, e1, T, ok);
    if (ok) nRefF = scan_list(ref, r0, r1, T, ok);
    if (!ok) {
#pragma unroll
        for (int k = 0; k < 7; ++k) out[k] = -1;
        return;
    }
    int nExact = 0, nTol = 0, ce = -1;
    unsigned nBothF = 0;
    Walk f, x, t;                                   // framewise intersection, exact matches, tolerant matches
    f.i = e0; f.j = r0;
    f.a = e0 < e1 ? est[e0] : make_int2(0, 0);
    f.r = r0 < r1 ? ref[r0] : make_int2(0, 0);
    x = f; t = f;
    const bool both = e0 < e1 && r0 < r1;
    bool fa = both, xa = both, ta = TOL && both;
    while (fa || xa || ta) {
        if (fa) {
            const int l = max(f.a.x, f.r.x), r = min(f.a.y, f.r.y);
            if (r >= l) { nBothF += (unsigned)(r - l) + (ce < l ? 1u : 0u); ce = r; }
            const bool adv_est = f.a.y < f.r.y;     // the list whose head ends first; a tie advances the reference
            walk_advance(f, adv_est, !adv_est, est, e1, ref, r1);
            fa = f.i < e1 && f.j < r1;
        }
        if (xa) {
            const bool eq = x.a.x == x.r.x && x.a.y == x.r.y;
            const bool late = x.r.x > x.a.x || x.r.y > x.a.y;
            nExact += eq ? 1 : 0;
            walk_advance(x, eq || late, eq || !late, est, e1, ref, r1);
            xa = x.i < e1 && x.j < r1;
        }
        if (TOL && ta) {
            const bool m = abs(t.a.x - t.r.x) <= tb && abs(t.a.y - t.r.y) <= te;
            const bool late = t.r.x > t.a.x + tb || t.r.y > t.a.y + te;
            nTol += m ? 1 : 0;
            walk_advance(t, m || late, m || !late, est, e1, ref, r1);
            ta = t.i < e1 && t.j < r1;
        }
    }
    out[0] = r1 - r0;
    out[1] = e1 - e0;
    out[2] = nExact;
    out[3] = (int)nRefF;
    out[4] = (int)nEstF;
    out[5] = (int)nBothF;
    out[6] = TOL ? nTol : nExact;
}

void launch_compare_paths(const int* est_pairs, const int* est_offsets, const int* ref_pairs, const int* ref_offsets, int T, int B,
                          int tb, int te, int* stats, hipStream_t stream)
{
    const int2* est = reinterpret_cast<const int2*>(est_pairs);
    const int2* ref = reinterpret_cast<const int2*>(ref_pairs);
    const dim3 grid((B + 63) / 64), block(64);      // one wave per workgroup: 352 chains spread over 6 compute units, not 2
    if (tb == 0 && te == 0)
        hipLaunchKernelGGL(compare_paths_kernel<false>, grid, block, 0, stream, est, est_offsets, ref, ref_offsets, T, B, 0, 0, stats);
    else
        hipLaunchKernelGGL(compare_paths_kernel<true>, grid, block, 0, stream, est, est_offsets, ref, ref_offsets, T, B, tb, te, stats);
}

}  // namespace semicrf
