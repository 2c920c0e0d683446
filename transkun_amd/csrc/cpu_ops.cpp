// cpu_ops.cpp -- the semi-CRF entry points for CPU tensors (dispatch key CPU of torch.ops.semicrf.*).
//
// The reference class runs wherever its tensors live (NeuralSemiCRFInterval.py:553-588; crfMinimalExample.py:28-38 is
// BASELINE config #1, "plumbing, no GPU").  These are the product's own host kernels for that case: plain C++, written
// for this layout ([T][T][B], chain axis contiguous: every inner loop runs over chains), OpenMP over chain blocks.  They
// are NOT a fallback: a GPU tensor never reaches them (the dispatcher selects by device), and nothing here includes or
// links the test suite's CPU checker (tests/test_abi.py::test_product_never_imports_oracle).
//
// Arithmetic: fp32 values as in the reference, sums of exponentials accumulated in double; decode is exact: one fp32 add
// per candidate, first maximum in the reference's candidate order.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "attr_loss_math.h"
#include "optim_math.h"
#include "attr_decode_math.h"
#include "attr_heads_math.h"
#include "attention_math.h"
#include "attention_bf16_math.h"
#include "ffn_math.h"
#include "ffn_bf16_math.h"
#include "ffn_bf16_train_math.h"
#include "logmel_math.h"
#include "cpu_ops.h"

namespace semicrf_cpu {

namespace {
constexpr int CB = 16;                          // chains per block: one 64-byte line of every cell (a thread owns whole lines of what it writes)

inline float softplus(float x) { return x > 20.0f ? x : log1pf(expf(x)); }      // F.softplus, threshold 20 (reference :218,:395)
inline float relu_sel(float x) { return x > 0.0f ? x : 0.0f; }                   // s * (s > 0), reference :29, :49-51

struct Lse {                                    // running log-sum-exp with exact maximum
    float m;
    double s;
    inline void push(float x)
    {
        if (x == -INFINITY) return;             // a masked cell adds nothing (and -inf - -inf would poison the sum with NaN)
        if (x <= m) s += (double)expf(x - m);
        else { s = s * (double)expf(m - x) + 1.0; m = x; }
    }
    inline float value() const { return s == 0.0 ? -INFINITY : m + (float)log(s); }   // nothing pushed: logsumexp of the empty set
};
}  // namespace

// alpha sweep (computeLogZ :207-246; forward_backward :394-410, :417): v [T][B], logZ [B]
void logz_fwd(const float* score, const float* noise, int T, int B, float* logZ, float* v)
{
    // Row by row with the chain blocks spread over the threads INSIDE a row: all threads stream the same 4 B T bytes of row i at
    // the same time.  (A thread per chain block walking the whole tensor on its own -- 64 bytes out of every 4 B -- touched a new
    // page every third cell: 4.9 s per step at T=1024 x 352 on 16 threads where the torch op loop takes 2.3.)
    const size_t Bs = (size_t)B;
    const int nblk = (B + CB - 1) / CB;
#pragma omp parallel
    for (int i = 0; i < T; ++i) {
        const float* row = score + (size_t)i * T * Bs;
#pragma omp for schedule(static) nowait
        for (int blk = 0; blk < nblk; ++blk) {
            const int c0 = blk * CB;
            const int nc = B - c0 < CB ? B - c0 : CB;
            float* vi = v + (size_t)i * Bs + c0;
            if (i == 0) {
                for (int c = 0; c < nc; ++c) vi[c] = softplus(row[c0 + c]);
            } else {
                const float* vp = v + (size_t)(i - 1) * Bs + c0;
                const float* nz = noise + (size_t)(i - 1) * Bs + c0;
                float m[CB];
                double s[CB];
                for (int c = 0; c < nc; ++c) m[c] = vp[c] + nz[c];
                for (int j = 0; j < i; ++j) {
                    const float* vj = v + (size_t)j * Bs + c0;
                    const float* cell = row + (size_t)j * Bs + c0;
                    for (int c = 0; c < nc; ++c) { const float x = vj[c] + cell[c]; m[c] = x > m[c] ? x : m[c]; }
                }
                // every candidate -inf (masked cells, torch.logsumexp gives -inf): the reference point is 0, every term exp(-inf) = 0
                float mm[CB];
                for (int c = 0; c < nc; ++c) mm[c] = m[c] == -INFINITY ? 0.0f : m[c];
                for (int c = 0; c < nc; ++c) s[c] = (double)expf(vp[c] + nz[c] - mm[c]);
                for (int j = 0; j < i; ++j) {
                    const float* vj = v + (size_t)j * Bs + c0;
                    const float* cell = row + (size_t)j * Bs + c0;
                    for (int c = 0; c < nc; ++c) s[c] += (double)expf(vj[c] + cell[c] - mm[c]);
                }
                const float* dg = row + (size_t)i * Bs + c0;
                for (int c = 0; c < nc; ++c) vi[c] = (s[c] == 0.0 ? -INFINITY : mm[c] + (float)log(s[c])) + softplus(dg[c]);
            }
            if (i == T - 1)
                for (int c = 0; c < nc; ++c) logZ[c0 + c] = vi[c];
        }                                               // (no barrier: the blocks are independent; a static schedule keeps a thread on ITS blocks, and threads with
                                                        // equal work stay within a few rows of each other -- a barrier per row cost seconds in the autograd thread)
    }
}

// alpha sweep from a forced start (semicrf_alpha_from): chain c runs on the frames start[c] .. T-1, v = -inf before.
// A thread owns whole chains (the recurrence of a chain is sequential and short next to logz_fwd's: no row-wise sharing).
void alpha_from(const float* score, const float* noise, const int32_t* start, int T, int B, float* v, float* logZ)
{
    const size_t Bs = (size_t)B;
#pragma omp parallel for schedule(static)
    for (int c = 0; c < B; ++c) {
        const int s = start[c];
        if (s < 0 || s > T - 1) {
            for (int t = 0; t < T; ++t) v[(size_t)t * Bs + c] = NAN;
            logZ[c] = NAN;
            continue;
        }
        for (int t = 0; t < s; ++t) v[(size_t)t * Bs + c] = -INFINITY;
        for (int t = s; t < T; ++t) {
            const float* row = score + (size_t)t * T * Bs + c;
            float a = softplus(row[(size_t)t * Bs]);
            if (t > s) {
                Lse acc{-INFINITY, 0.0};
                acc.push(v[(size_t)(t - 1) * Bs + c] + noise[(size_t)(t - 1) * Bs + c]);
                for (int b = s; b < t; ++b) acc.push(v[(size_t)b * Bs + c] + row[(size_t)b * Bs]);
                a += acc.value();
            }
            v[(size_t)t * Bs + c] = a;
        }
        logZ[c] = v[(size_t)(T - 1) * Bs + c];
    }
}

// beta sweep by frames (the flipped half of forward_backward :386-414) and, when dScore is given, the marginals
// (:424-447) times gout (:469-472).  Row e is visited once, right after q[e] is final: its cells are pushed into the
// accumulators of the frames t < e and turned into marginals in the same pass.
void logz_bwd(const float* score, const float* noise, const float* v, const float* logZ, const float* gout, int T, int B,
              float* dScore, float* dNoise, float* q)
{
    const size_t Bs = (size_t)B;
    const int nblk = (B + CB - 1) / CB;
    std::vector<Lse> acc_all((size_t)nblk * T * CB, Lse{-INFINITY, 0.0});      // per chain block: the accumulators of the frames t < e
#pragma omp parallel
    for (int e = T - 1; e >= 0; --e) {                    // row by row, the chain blocks spread over the threads inside a row (see logz_fwd)
        const float* row = score + (size_t)e * T * Bs;
#pragma omp for schedule(static) nowait
        for (int blk = 0; blk < nblk; ++blk) {
            const int c0 = blk * CB;
            const int nc = B - c0 < CB ? B - c0 : CB;
            Lse* const acc = acc_all.data() + (size_t)blk * T * CB;
            const float* dg = row + (size_t)e * Bs + c0;
            float* qe = q + (size_t)e * Bs + c0;
            if (e == T - 1) {
                for (int c = 0; c < nc; ++c) qe[c] = softplus(dg[c]);
            } else {
                const float* qn = q + (size_t)(e + 1) * Bs + c0;
                const float* nz = noise + (size_t)e * Bs + c0;
                for (int c = 0; c < nc; ++c) {
                    Lse a = acc[(size_t)e * CB + c];
                    a.push(qn[c] + nz[c]);
                    qe[c] = a.value() + softplus(dg[c]);
                }
                if (dNoise) {
                    const float* ve = v + (size_t)e * Bs + c0;
                    for (int c = 0; c < nc; ++c)
                        dNoise[(size_t)e * Bs + c0 + c] = gout[c0 + c] * expf(ve[c] + qn[c] + nz[c] - logZ[c0 + c]);
                }
            }
            float* drow = dScore ? dScore + (size_t)e * T * Bs : nullptr;
            for (int t = 0; t < e; ++t) {
                const float* cell = row + (size_t)t * Bs + c0;
                Lse* a = &acc[(size_t)t * CB];
                for (int c = 0; c < nc; ++c) a[c].push(qe[c] + cell[c]);
                if (drow) {
                    const float* vt = v + (size_t)t * Bs + c0;
                    float* d = drow + (size_t)t * Bs + c0;
                    for (int c = 0; c < nc; ++c) d[c] = gout[c0 + c] * expf(vt[c] + qe[c] + cell[c] - logZ[c0 + c]);
                }
            }
            if (drow) {
                const float* ve = v + (size_t)e * Bs + c0;
                float* d = drow + (size_t)e * Bs + c0;
                for (int c = 0; c < nc; ++c)
                    d[c] = gout[c0 + c] * expf(ve[c] + qe[c] + dg[c] - 2.0f * softplus(dg[c]) - logZ[c0 + c]);
                for (int t = e + 1; t < T; ++t) memset(drow + (size_t)t * Bs + c0, 0, (size_t)nc * sizeof(float));   // begin > end: exact zeros
            }
        }
    }
}

// Viterbi + backtrack (viterbiBackward :13-104, forward == 0; viterbi :107-202, forward == 1).  Candidates are single fp32
// adds; ties: skip first, then the nearest frame (forward == 0: smallest end; forward == 1: smallest begin) -- the first
// maximum of the reference's concatenation.  pairs [cap][2] chain-major, offsets [B+1].
void viterbi(const float* score, const float* noise, int T, int B, const int32_t* start, int forward, int32_t* pairs, int64_t cap,
             int32_t* offsets)
{
    const size_t Bs = (size_t)B;
    std::vector<int32_t> ptr((size_t)T * B, -1);           // [frame][chain]: -1 skip, else the partner frame
    std::vector<float> u((size_t)T * B);
    if (forward) {
#pragma omp parallel for schedule(dynamic, 1)
        for (int c0 = 0; c0 < B; c0 += CB) {
            const int nc = B - c0 < CB ? B - c0 : CB;
            for (int i = 0; i < T; ++i) {
                const float* row = score + (size_t)i * T * Bs;
                const float* dg = row + (size_t)i * Bs + c0;
                float* ui = &u[(size_t)i * Bs + c0];
                if (i == 0) { for (int c = 0; c < nc; ++c) ui[c] = relu_sel(dg[c]); continue; }
                float m[CB];
                int32_t a[CB];
                for (int c = 0; c < nc; ++c) { m[c] = u[(size_t)(i - 1) * Bs + c0 + c] + noise[(size_t)(i - 1) * Bs + c0 + c]; a[c] = -1; }
                for (int j = 0; j < i; ++j) {
                    const float* uj = &u[(size_t)j * Bs + c0];
                    const float* cell = row + (size_t)j * Bs + c0;
                    for (int c = 0; c < nc; ++c) { const float x = uj[c] + cell[c]; if (x > m[c]) { m[c] = x; a[c] = j; } }
                }
                for (int c = 0; c < nc; ++c) { ui[c] = m[c] + relu_sel(dg[c]); ptr[(size_t)i * Bs + c0 + c] = a[c]; }
            }
        }
    } else {
#pragma omp parallel for schedule(dynamic, 1)
        for (int c0 = 0; c0 < B; c0 += CB) {
            const int nc = B - c0 < CB ? B - c0 : CB;
            std::vector<float> m((size_t)T * CB, -INFINITY);
            std::vector<int32_t> a((size_t)T * CB, -1);
            for (int e = T - 1; e >= 0; --e) {
                const float* row = score + (size_t)e * T * Bs;
                const float* dg = row + (size_t)e * Bs + c0;
                float* ue = &u[(size_t)e * Bs + c0];
                if (e == T - 1) {
                    for (int c = 0; c < nc; ++c) ue[c] = relu_sel(dg[c]);
                } else {
                    for (int c = 0; c < nc; ++c) {
                        // ends arrived farthest first: a later equal candidate (nearer end) won with >=; the skip goes in front of all
                        const float xs = u[(size_t)(e + 1) * Bs + c0 + c] + noise[(size_t)e * Bs + c0 + c];
                        float mm = m[(size_t)e * CB + c];
                        int32_t aa = a[(size_t)e * CB + c];
                        if (xs >= mm) { mm = xs; aa = -1; }
                        ue[c] = mm + relu_sel(dg[c]);
                        ptr[(size_t)e * Bs + c0 + c] = aa;
                    }
                }
                for (int t = 0; t < e; ++t) {
                    const float* cell = row + (size_t)t * Bs + c0;
                    float* mt = &m[(size_t)t * CB];
                    int32_t* at = &a[(size_t)t * CB];
                    for (int c = 0; c < nc; ++c) { const float x = ue[c] + cell[c]; if (x >= mt[c]) { mt[c] = x; at[c] = e; } }
                }
            }
        }
    }
    // backtrack, chain by chain (:61-102, :161-196)
    std::vector<std::vector<int32_t>> out((size_t)B);
#pragma omp parallel for schedule(dynamic, 8)
    for (int c = 0; c < B; ++c) {
        std::vector<int32_t>& o = out[(size_t)c];
        auto diag = [&](int t) { return score[((size_t)t * T + t) * Bs + c] > 0.0f; };
        if (!forward) {
            int j = start ? start[c] : 0;
            while (j < T - 1) {
                if (diag(j)) { o.push_back(j); o.push_back(j); }
                const int32_t p = ptr[(size_t)j * Bs + c];
                if (p < 0) ++j;
                else { o.push_back(j); o.push_back(p); j = p; }
            }
            if (diag(T - 1)) { o.push_back(T - 1); o.push_back(T - 1); }
        } else {
            int j = start ? start[c] : T - 1;
            std::vector<int32_t> rev;
            while (j > 0) {
                if (diag(j)) { rev.push_back(j); rev.push_back(j); }
                const int32_t p = ptr[(size_t)j * Bs + c];
                if (p < 0) --j;
                else { rev.push_back(p); rev.push_back(j); j = p; }
            }
            if (diag(0)) { rev.push_back(0); rev.push_back(0); }
            for (size_t i = rev.size(); i >= 2; i -= 2) { o.push_back(rev[i - 2]); o.push_back(rev[i - 1]); }
        }
    }
    int64_t k = 0;
    for (int c = 0; c < B; ++c) {
        offsets[c] = (int32_t)k;
        const std::vector<int32_t>& o = out[(size_t)c];
        for (size_t i = 0; i + 1 < o.size(); i += 2, ++k)
            if (k < cap) { pairs[2 * k] = o[i]; pairs[2 * k + 1] = o[i + 1]; }
    }
    offsets[B] = (int32_t)k;
}

// Posterior sampling (include/semicrf_hip.h: semicrf_sample; the device kernel is sample.hip).  Per (frame, chain) the candidate
// weights exp(x - max) in double and their running sums are built once; every draw that visits the frame takes the first candidate
// whose running sum exceeds u * Z (binary search), or -- u * Z at or past the total -- the last one of positive weight.  The
// uniforms are the device's: (splitmix64(((k*B + c)*T + t)*2 + r, key) >> 40) * 2^-24.
namespace {
inline uint64_t splitmix64(uint64_t idx, uint64_t key)
{
    uint64_t z = idx + key * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline double uniform24(uint64_t idx, uint64_t key) { return (double)(splitmix64(idx, key) >> 40) * (1.0 / 16777216.0); }
}  // namespace

void sample(const float* score, const float* noise, const float* v, int T, int B, int64_t k0, int nSample, uint64_t key,
            const int32_t* end, int32_t* pairs, int64_t cap, int32_t* offsets)
{
    const size_t Bs = (size_t)B;
    const int64_t nB = (int64_t)nSample * B;
    std::vector<std::vector<int32_t>> out((size_t)nB);
#pragma omp parallel for schedule(dynamic, 1)
    for (int c = 0; c < B; ++c) {
        // cum[t][i]: running sums of the candidates of frame t (i = 0 skip, i >= 1 the interval (t - i, t)), built on first visit
        std::vector<std::vector<double>> cum((size_t)T);
        auto row = [&](int t) -> const std::vector<double>& {
            std::vector<double>& r = cum[(size_t)t];
            if (!r.empty() || t == 0) return r;
            std::vector<float> x((size_t)t + 1);
            x[0] = v[(size_t)(t - 1) * Bs + c] + noise[(size_t)(t - 1) * Bs + c];
            for (int i = 1; i <= t; ++i) x[(size_t)i] = v[(size_t)(t - i) * Bs + c] + score[((size_t)t * T + (t - i)) * Bs + c];
            float m = -INFINITY;
            for (float xi : x) m = xi > m ? xi : m;
            r.resize((size_t)t + 1);
            double acc = 0.0;
            for (int i = 0; i <= t; ++i) {
                acc += m == -INFINITY ? 0.0 : exp((double)x[(size_t)i] - (double)m);
                r[(size_t)i] = acc;
            }
            return r;
        };
        for (int k = 0; k < nSample; ++k) {
            std::vector<int32_t> rev;
            int t = end ? end[c] : T - 1;
            for (;;) {
                const uint64_t base = ((uint64_t)(k0 + k) * (uint64_t)B + (uint64_t)c) * (uint64_t)T + (uint64_t)t;
                const double sg = 1.0 / (1.0 + exp(-(double)score[((size_t)t * T + t) * Bs + c]));
                if (uniform24(2 * base + 1, key) < sg) { rev.push_back(t); rev.push_back(t); }
                if (t == 0) break;
                const std::vector<double>& r = row(t);
                const double Z = r.back();
                int pick = 0;                                       // no candidate of positive weight: the skip
                if (Z > 0.0) {
                    const double thr = uniform24(2 * base, key) * Z;
                    if (thr < Z) pick = (int)(std::upper_bound(r.begin(), r.end(), thr) - r.begin());
                    else pick = (int)(std::lower_bound(r.begin(), r.end(), Z) - r.begin());   // the last candidate of positive weight
                }
                if (pick == 0) t -= 1;
                else { rev.push_back(t - pick); rev.push_back(t); t -= pick; }
            }
            std::vector<int32_t>& o = out[(size_t)k * Bs + c];
            for (size_t i = rev.size(); i >= 2; i -= 2) { o.push_back(rev[i - 2]); o.push_back(rev[i - 1]); }
        }
    }
    int64_t n = 0;
    for (int64_t p = 0; p < nB; ++p) {
        offsets[p] = (int32_t)n;
        const std::vector<int32_t>& o = out[(size_t)p];
        for (size_t i = 0; i + 1 < o.size(); i += 2, ++n)
            if (n < cap) { pairs[2 * n] = o[i]; pairs[2 * n + 1] = o[i + 1]; }
    }
    offsets[nB] = (int32_t)n;
}

// posterior marginals and path entropy (include/semicrf_hip.h: semicrf_posteriors; the device kernels are posterior.hip), every
// sum and exponential in double from the fp32 v / q / logZ.
namespace {
inline double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }
inline double bern_entropy_d(double d)
{
    const double a = fabs(d), ea = exp(-a);
    return log1p(ea) + (ea > 0.0 ? a * ea / (1.0 + ea) : 0.0);
}
inline double ent_term_d(double mu, double R, double y) { return mu > 0.0 ? mu * (R - y > 0.0 ? R - y : 0.0) : 0.0; }
inline float clamp1(double x) { return x > 1.0 ? 1.0f : (float)x; }
inline double single_d(double v, double q, double lz, double d) { return exp(v + q - lz + d - 2.0 * softplus_d(d)); }
// the marginal of ONE cell, rounded to fp32: what interval_marginals returns and what marginal_decode compares with its threshold
inline float cell_marginal(float vb, float s, float qe, float lz) { return clamp1(exp((double)vb + (double)s + (double)qe - lz)); }
inline float cell_marginal_single(float vt, float qt, float lz, float d) { return clamp1(single_d(vt, qt, lz, d)); }
}  // namespace

void posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B, float* node,
                float* begin, float* end, float* single, float* noiseP, float* entropy)
{
    const size_t Bs = (size_t)B;
    const int nblk = (B + CB - 1) / CB;
#pragma omp parallel for schedule(dynamic, 1)
    for (int blk = 0; blk < nblk; ++blk) {
        const int c0 = blk * CB;
        const int nc = B - c0 < CB ? B - c0 : CB;
        std::vector<double> bg((size_t)T * CB, 0.0);
        double H[CB] = {0.0};
        for (int e = 0; e < T; ++e) {
            const float* row = score + (size_t)e * T * Bs;
            for (int c = 0; c < nc; ++c) {
                const size_t ec = (size_t)e * Bs + c0 + c;
                const double lz = logZ[c0 + c], d = row[(size_t)e * Bs + c0 + c];
                const double R = (double)v[ec] - softplus_d(d), A = (double)q[ec] - lz;
                double en = 0.0, h = 0.0;
                for (int b = 0; b < e; ++b) {
                    const double y = (double)v[(size_t)b * Bs + c0 + c] + (double)row[(size_t)b * Bs + c0 + c];
                    const double mu = exp(y + A);
                    en += mu;
                    bg[(size_t)b * CB + c] += mu;
                    h += ent_term_d(mu, R, y);
                }
                const double nd = exp(R + A);
                if (nd > 0.0) h += nd * bern_entropy_d(d);
                if (e > 0) {
                    const size_t pc = ec - Bs;
                    const double y = (double)v[pc] + (double)noise[pc];
                    h += ent_term_d(exp(y + A), R, y);
                }
                if (e + 1 < T) noiseP[ec] = clamp1(exp((double)v[ec] + (double)noise[ec] + (double)q[ec + Bs] - lz));
                node[ec] = clamp1(nd);
                single[ec] = clamp1(single_d(v[ec], q[ec], lz, d));
                end[ec] = clamp1(en);
                H[c] += h;
            }
        }
        for (int t = 0; t < T; ++t)
            for (int c = 0; c < nc; ++c) begin[(size_t)t * Bs + c0 + c] = clamp1(bg[(size_t)t * CB + c]);
        for (int c = 0; c < nc; ++c) entropy[c0 + c] = (float)H[c];
    }
}

// posterior expectations and covariances (include/semicrf_hip.h: semicrf_expectation, semicrf_covariance; the device kernels are
// expectation.hip), everything in double: the per-frame log-sums v64 / q64 and the conditional expectations
//   a[t]    = E[W of the prefix up to node t, its singleton included | t is a node]
//   binc[t] = E[W of the suffix from node t on, its singleton included | t is a node]
// by rows (forward) and by columns (backward), chain blocks in parallel; then one pass over the triangle.
namespace {
inline double sigmoid_d(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }      // d softplus_d / dx

// one direction for the chains c0 .. c0 + nc: fwd: frame t = k, cell (t, p) = s[t][p]; else t = T-1-k, cell = s[p][t]
void expectation_sweep(const float* score, const float* noise, const float* weight, const float* nweight, int T, int B, int c0, int nc,
                       bool fwd, double* L, double* X)
{
    const size_t Bs = (size_t)B;
    for (int k = 0; k < T; ++k) {
        const int t = fwd ? k : T - 1 - k;
        double m[CB], Z[CB], A[CB];
        if (k > 0) {
            const int pn = fwd ? t - 1 : t + 1;
            const size_t gc = (size_t)(fwd ? t - 1 : t) * Bs + c0;
            for (int c = 0; c < nc; ++c) m[c] = L[(size_t)pn * Bs + c0 + c] + (double)noise[gc + c];
            for (int j = 0; j < k; ++j) {
                const int p = fwd ? j : T - 1 - j;
                const float* cell = score + (fwd ? (size_t)t * T + p : (size_t)p * T + t) * Bs + c0;
                const double* Lp = L + (size_t)p * Bs + c0;
                for (int c = 0; c < nc; ++c) { const double x = Lp[c] + (double)cell[c]; m[c] = x > m[c] ? x : m[c]; }
            }
            for (int c = 0; c < nc; ++c) {
                if (!(m[c] > -INFINITY)) m[c] = 0.0;
                const double ex = exp(L[(size_t)pn * Bs + c0 + c] + (double)noise[gc + c] - m[c]);
                Z[c] = ex;
                A[c] = ex * (X[(size_t)pn * Bs + c0 + c] + (nweight ? (double)nweight[gc + c] : 0.0));
            }
            for (int j = 0; j < k; ++j) {
                const int p = fwd ? j : T - 1 - j;
                const size_t off = (fwd ? (size_t)t * T + p : (size_t)p * T + t) * Bs + c0;
                const float* cell = score + off;
                const float* wc = weight + off;
                const double* Lp = L + (size_t)p * Bs + c0;
                const double* Xp = X + (size_t)p * Bs + c0;
                for (int c = 0; c < nc; ++c) {
                    const double ex = exp(Lp[c] + (double)cell[c] - m[c]);
                    Z[c] += ex;
                    A[c] += ex * (Xp[c] + (double)wc[c]);
                }
            }
        }
        const size_t dc = ((size_t)t * T + t) * Bs + c0;
        for (int c = 0; c < nc; ++c) {
            const double d = score[dc + c];
            double Lt = softplus_d(d), Xt = sigmoid_d(d) * (double)weight[dc + c];
            if (k > 0) {
                Lt += m[c] + log(Z[c]);
                Xt += Z[c] > 0.0 ? A[c] / Z[c] : 0.0;
            }
            L[(size_t)t * Bs + c0 + c] = Lt;
            X[(size_t)t * Bs + c0 + c] = Xt;
        }
    }
}
}  // namespace

void expectation(const float* score, const float* noise, const float* weight, const float* nweight, int T, int B, float* E, float* H,
                 double* state)
{
    if (!weight) weight = score;
    const size_t TB = (size_t)T * B;
    double *v64 = state, *a = state + TB, *q64 = state + 2 * TB, *binc = state + 3 * TB, *E64 = state + 4 * TB, *lz64 = E64 + B;
    const int nblk = (B + CB - 1) / CB;
#pragma omp parallel for schedule(dynamic, 1)
    for (int job = 0; job < 2 * nblk; ++job) {
        const int c0 = (job >> 1) * CB;
        const int nc = B - c0 < CB ? B - c0 : CB;
        if (job & 1) expectation_sweep(score, noise, weight, nweight, T, B, c0, nc, false, q64, binc);
        else expectation_sweep(score, noise, weight, nweight, T, B, c0, nc, true, v64, a);
    }
    for (int c = 0; c < B; ++c) {
        E64[c] = a[(size_t)(T - 1) * B + c];
        lz64[c] = v64[(size_t)(T - 1) * B + c];
        E[c] = (float)E64[c];
        H[c] = (float)(lz64[c] - E64[c]);
    }
}

void covariance(const float* score, const float* noise, const float* weight, const float* nweight, const float* gout, int T, int B,
                const double* state, float* C, float* Cn)
{
    if (!weight) weight = score;
    const size_t TB = (size_t)T * B, Bs = (size_t)B;
    const double *v64 = state, *a = state + TB, *q64 = state + 2 * TB, *binc = state + 3 * TB, *E64 = state + 4 * TB, *lz64 = E64 + B;
#pragma omp parallel for schedule(dynamic, 4)
    for (int e = 0; e < T; ++e) {
        const size_t row = (size_t)e * T * Bs;
        for (int b = 0; b < e; ++b)
            for (int c = 0; c < B; ++c) {
                const size_t cell = row + (size_t)b * Bs + c, bc = (size_t)b * Bs + c, ec = (size_t)e * Bs + c;
                const double mu = exp(v64[bc] + (double)score[cell] + q64[ec] - lz64[c]);
                C[cell] = (float)(mu * (a[bc] + (double)weight[cell] + binc[ec] - E64[c]) * (double)gout[c]);
            }
        for (int c = 0; c < B; ++c) {                                   // the singleton: P = node sigma(d), given weight w[t,t]
            const size_t ec = (size_t)e * Bs + c, cell = row + ec;
            const double d = score[cell], w = weight[cell];
            const double mu = exp(v64[ec] + q64[ec] - 2.0 * softplus_d(d) + d - lz64[c]);
            C[cell] = (float)(mu * (a[ec] + binc[ec] + (1.0 - 2.0 * sigmoid_d(d)) * w - E64[c]) * (double)gout[c]);
        }
        if (e + 1 < T) {
            memset(C + row + (size_t)(e + 1) * Bs, 0, (size_t)(T - 1 - e) * Bs * sizeof(float));        // begin > end: exact zeros
            for (int c = 0; c < B; ++c) {
                const size_t ec = (size_t)e * Bs + c;
                const double mu = exp(v64[ec] + (double)noise[ec] + q64[ec + Bs] - lz64[c]);
                Cn[ec] = (float)(mu * (a[ec] + (nweight ? (double)nweight[ec] : 0.0) + binc[ec + Bs] - E64[c]) * (double)gout[c]);
            }
        }
    }
}

// interval marginals (semicrf_interval_marginals): b > e gives 0; the caller has checked the indices
void interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int32_t* pairs,
                        const int32_t* offsets, float* out)
{
    const size_t Bs = (size_t)B;
    for (int c = 0; c < B; ++c)
        for (int32_t k = offsets[c]; k < offsets[c + 1]; ++k) {
            const int b = pairs[2 * k], e = pairs[2 * k + 1];
            const size_t ec = (size_t)e * Bs + c;
            if (b > e) out[k] = 0.0f;
            else if (b == e) out[k] = cell_marginal_single(v[ec], q[ec], logZ[c], score[((size_t)e * T + e) * Bs + c]);
            else out[k] = cell_marginal(v[(size_t)b * Bs + c], score[((size_t)e * T + b) * Bs + c], q[ec], logZ[c]);
        }
}

// marginal-threshold decoding (include/semicrf_hip.h: semicrf_marginal_decode; the device kernels are marginal_decode.hip): every
// cell b <= e with cell_marginal >= tau[c * tau_stride], chain-major, ascending by (begin, end).  Chain blocks in parallel, each
// walking the triangle row by row (the chain axis is the contiguous one) into per-column lists; packed in order afterwards.
void marginal_decode(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                     int tau_stride, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets)
{
    const size_t Bs = (size_t)B;
    struct Hit { int32_t e; float m; };
    std::vector<std::vector<Hit>> hits((size_t)T * Bs);            // [b][c]: the column's selected cells, e ascending
    const int nblk = (B + CB - 1) / CB;
#pragma omp parallel for schedule(dynamic, 1)
    for (int blk = 0; blk < nblk; ++blk) {
        const int c0 = blk * CB;
        const int nc = B - c0 < CB ? B - c0 : CB;
        for (int e = 0; e < T; ++e) {
            const float* row = score + (size_t)e * T * Bs;
            for (int b = 0; b <= e; ++b)
                for (int c = c0; c < c0 + nc; ++c) {
                    const size_t ec = (size_t)e * Bs + c;
                    const float m = b == e ? cell_marginal_single(v[ec], q[ec], logZ[c], row[(size_t)e * Bs + c])
                                           : cell_marginal(v[(size_t)b * Bs + c], row[(size_t)b * Bs + c], q[ec], logZ[c]);
                    if (m >= tau[(size_t)c * tau_stride]) hits[(size_t)b * Bs + c].push_back(Hit{(int32_t)e, m});
                }
        }
    }
    int64_t n = 0;
    bool bad = false;
    for (int c = 0; c < B; ++c) {
        offsets[c] = (int32_t)n;
        for (int b = 0; b < T; ++b)
            for (const Hit& h : hits[(size_t)b * Bs + c]) {
                if (n < cap) { pairs[2 * n] = b; pairs[2 * n + 1] = h.e; probs[n] = h.m; }
                ++n;
            }
        const float vl = v[(size_t)(T - 1) * Bs + c];
        bad = bad || vl != vl;
    }
    offsets[B] = bad ? -1 : (int32_t)n;
}

// tolerance-aware interval marginals (include/semicrf_hip.h: semicrf_interval_marginals_tol), the definition evaluated literally:
// rows e' ascending, inside a row b' ascending, one fp32 add per term.  b > e gives 0; the caller has checked the indices
void interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const int32_t* pairs,
                            const int32_t* offsets, int db, int de, float* out)
{
    const size_t Bs = (size_t)B;
#pragma omp parallel for schedule(dynamic, 1)
    for (int c = 0; c < B; ++c)
        for (int32_t k = offsets[c]; k < offsets[c + 1]; ++k) {
            const int b = pairs[2 * k], e = pairs[2 * k + 1];
            if (b > e) { out[k] = 0.0f; continue; }
            const int elo = std::max(0, e - de), ehi = std::min(T - 1, e + de), blo = std::max(0, b - db);
            float acc = 0.0f;
            for (int er = elo; er <= ehi; ++er) {
                const int bhi = std::min(b + db, er);
                if (bhi < blo) continue;
                const size_t ec = (size_t)er * Bs + c;
                float row = 0.0f;
                for (int bc = blo; bc <= bhi; ++bc)
                    row += bc == er ? cell_marginal_single(v[ec], q[ec], logZ[c], score[((size_t)er * T + er) * Bs + c])
                                    : cell_marginal(v[(size_t)bc * Bs + c], score[((size_t)er * T + bc) * Bs + c], q[ec], logZ[c]);
                acc += row;
            }
            out[k] = acc > 1.0f ? 1.0f : acc;
        }
}

// tolerance-aware marginal-threshold decoding (include/semicrf_hip.h: semicrf_marginal_decode_tol; the device kernels are
// marginal_tol.hip): marginal_decode with M in place of m.  Per chain block the triangle is walked row by row: the row's m, then its
// row sums around every column (ascending b'; a cell outside the triangle is +0.0f, and x + 0.0f == x for x >= 0 and NaN) into a
// ring of 2 de + 1 rows; M(e, .) is the sum of the ring in ascending row order once row e + de is in it.
void marginal_decode_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B, const float* tau,
                         int tau_stride, int db, int de, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets)
{
    const size_t Bs = (size_t)B;
    struct Hit { int32_t e; float m; };
    std::vector<std::vector<Hit>> hits((size_t)T * Bs);            // [b][c]: the column's selected cells, e ascending
    const int nblk = (B + CB - 1) / CB, R = 2 * de + 1;
#pragma omp parallel for schedule(dynamic, 1)
    for (int blk = 0; blk < nblk; ++blk) {
        const int c0 = blk * CB;
        const int nc = B - c0 < CB ? B - c0 : CB;
        std::vector<float> mrow((size_t)T * CB), ring((size_t)R * T * CB, 0.0f);
        for (int er = 0; er < T + de; ++er) {
            float* rs = ring.data() + (size_t)(er % R) * T * CB;
            if (er < T) {
                const float* row = score + (size_t)er * T * Bs;
                for (int b = 0; b <= er; ++b)
                    for (int cc = 0; cc < nc; ++cc) {
                        const int c = c0 + cc;
                        const size_t ec = (size_t)er * Bs + c;
                        mrow[(size_t)b * CB + cc] = b == er ? cell_marginal_single(v[ec], q[ec], logZ[c], row[(size_t)er * Bs + c])
                                                            : cell_marginal(v[(size_t)b * Bs + c], row[(size_t)b * Bs + c], q[ec], logZ[c]);
                    }
                for (int b = 0; b < T; ++b) {
                    const int blo = std::max(0, b - db), bhi = std::min(b + db, er);
                    for (int cc = 0; cc < nc; ++cc) {
                        float a = 0.0f;
                        for (int bc = blo; bc <= bhi; ++bc) a += mrow[(size_t)bc * CB + cc];
                        rs[(size_t)b * CB + cc] = a;
                    }
                }
            } else {
                std::fill(rs, rs + (size_t)T * CB, 0.0f);          // a row past the last frame
            }
            const int e = er - de;
            if (e < 0) continue;
            const int elo = std::max(0, e - de), ehi = std::min(T - 1, e + de);
            for (int b = 0; b <= e; ++b)
                for (int cc = 0; cc < nc; ++cc) {
                    float a = 0.0f;
                    for (int x = elo; x <= ehi; ++x) a += ring[((size_t)(x % R) * T + b) * CB + cc];
                    const float M = a > 1.0f ? 1.0f : a;
                    const int c = c0 + cc;
                    if (M >= tau[(size_t)c * tau_stride]) hits[(size_t)b * Bs + c].push_back(Hit{(int32_t)e, M});
                }
        }
    }
    int64_t n = 0;
    bool bad = false;
    for (int c = 0; c < B; ++c) {
        offsets[c] = (int32_t)n;
        for (int b = 0; b < T; ++b)
            for (const Hit& h : hits[(size_t)b * Bs + c]) {
                if (n < cap) { pairs[2 * n] = b; pairs[2 * n + 1] = h.e; probs[n] = h.m; }
                ++n;
            }
        const float vl = v[(size_t)(T - 1) * Bs + c];
        bad = bad || vl != vl;
    }
    offsets[B] = bad ? -1 : (int32_t)n;
}

// MBR path decoding (include/semicrf_hip.h: semicrf_mbr_select; the device kernels are mbr_decode.hip): per chain the recursion
// F[t] = max(F[t+1], max over the eligible (t, e), e > t, of g + F[e]) + gS(t) over the packed lattice, walked backwards, then the
// trace from frame 0.  Ties: the skip, then the smallest e (the strict compare in ascending order).  Chains in parallel; packed in
// chain order afterwards.
void mbr_select(const int32_t* pairs, const float* weight, const int32_t* offsets, int64_t K, int T, int B, const float* tau,
                int tau_stride, int32_t* pairs_out, float* probs_out, int64_t cap, int32_t* offsets_out, float* gain)
{
    const int64_t total = offsets[B];
    if (total < 0 || total > K) {                                   // the NaN convention of the sweeps / a truncated lattice
        for (int c = 0; c < B; ++c) { offsets_out[c] = 0; gain[c] = 0.0f; }
        offsets_out[B] = -1;
        return;
    }
    std::vector<std::vector<int32_t>> sel((size_t)B);               // the selected lattice indices of every chain, in path order
#pragma omp parallel for schedule(dynamic, 4)
    for (int c = 0; c < B; ++c) {
        const float th = tau[(size_t)c * tau_stride];
        int64_t lo = std::min<int64_t>(std::max<int64_t>(offsets[c], 0), total);
        int64_t hi = std::min<int64_t>(std::max<int64_t>(offsets[c + 1], lo), total);
        std::vector<float> F((size_t)T + 1, 0.0f);                  // F[T] = +0: F[T-1] = 0 + gS(T-1)
        std::vector<int32_t> ch((size_t)T, -1), sg((size_t)T, -1), nx((size_t)T, 0);
        int64_t i = hi;
        for (int t = T - 1; t >= 0; --t) {
            while (i > lo && pairs[2 * (i - 1)] > t) --i;           // (an unsorted lattice: entries above the frame are dropped)
            int64_t j = i;
            while (j > lo && pairs[2 * (j - 1)] == t) --j;          // the frame's entries: [j, i), ascending by end
            float best = F[t + 1], gs = 0.0f;
            int32_t key = -1;
            for (int64_t k = j; k < i; ++k) {
                const int32_t e = pairs[2 * k + 1];
                const float w = weight[k];
                if (!(w > th) || e < t || e >= T) continue;         // NaN on either side: not eligible
                const float g = w - th;
                if (e == t) {
                    if (sg[t] < 0) { sg[t] = (int32_t)k; gs = g; }
                    continue;
                }
                const float cv = g + F[e];
                if (cv > best) { best = cv; key = (int32_t)k; }
            }
            ch[t] = key;
            nx[t] = key < 0 ? t + 1 : pairs[2 * key + 1];
            F[t] = best + gs;
            i = j;
        }
        gain[c] = F[0];
        std::vector<int32_t>& out = sel[(size_t)c];
        for (int t = 0;; t = nx[t]) {
            if (sg[t] >= 0) out.push_back(sg[t]);
            if (t == T - 1) break;
            if (ch[t] >= 0) out.push_back(ch[t]);
        }
    }
    int64_t n = 0;
    for (int c = 0; c < B; ++c) {
        offsets_out[c] = (int32_t)n;
        for (const int32_t k : sel[(size_t)c]) {
            if (n < cap) { pairs_out[2 * n] = pairs[2 * k]; pairs_out[2 * n + 1] = pairs[2 * k + 1]; probs_out[n] = weight[k]; }
            ++n;
        }
    }
    offsets_out[B] = (int32_t)n;
}

// Path comparison (include/semicrf_hip.h: semicrf_compare_paths; the device kernel is pathstats.hip): per chain the list lengths,
// the exact matches, the three frame counts of the reference's compareFramewise and the maximum matching under a tolerance.  The
// walks are written one after the other here (the device kernel runs them in one loop); the tolerant walk at (0, 0) is the exact one.
namespace {
struct PairList {
    const int32_t* p;
    int64_t lo, hi;
    int64_t size() const { return hi - lo; }
    int32_t b(int64_t i) const { return p[2 * (lo + i)]; }
    int32_t e(int64_t i) const { return p[2 * (lo + i) + 1]; }
};
bool list_valid(const PairList& l, int T)
{
    int32_t pb = 0, pe = -1;
    for (int64_t i = 0; i < l.size(); ++i) {
        if (l.b(i) < pb || l.b(i) > l.e(i) || l.e(i) >= T || l.e(i) < pe) return false;
        pb = l.b(i); pe = l.e(i);
    }
    return true;
}
// s += end - begin, + 1 unless the piece starts at or before the previous piece's end
struct FrameSum {
    uint32_t s = 0;
    int32_t prev_end = -1;
    void add(int32_t l, int32_t r) { s += (uint32_t)(r - l) + (prev_end < l ? 1u : 0u); prev_end = r; }
};
int32_t list_frames(const PairList& l)
{
    FrameSum f;
    for (int64_t i = 0; i < l.size(); ++i) f.add(l.b(i), l.e(i));
    return (int32_t)f.s;
}
int32_t both_frames(const PairList& est, const PairList& ref)
{
    FrameSum f;                                     // (a piece that the reference merges into its predecessor is one without the + 1)
    int64_t i = 0, j = 0;
    while (i < est.size() && j < ref.size()) {
        const int32_t l = std::max(est.b(i), ref.b(j)), r = std::min(est.e(i), ref.e(j));
        if (r >= l) f.add(l, r);
        if (est.e(i) < ref.e(j)) ++i; else ++j;
    }
    return (int32_t)f.s;
}
int32_t match_count(const PairList& est, const PairList& ref, int tb, int te)
{
    int32_t n = 0;
    int64_t i = 0, j = 0;
    while (i < est.size() && j < ref.size()) {
        const int32_t b = est.b(i), e = est.e(i), rb = ref.b(j), re = ref.e(j);
        if (std::abs(b - rb) <= tb && std::abs(e - re) <= te) { ++n; ++i; ++j; }
        else if (rb > b + tb || re > e + te) ++i;   // the reference's head is too late for this estimate: so is all that follows it
        else ++j;                                   // it is too early for this estimate and for every later one
    }
    return n;
}
}  // namespace

void compare_paths(const int32_t* est_pairs, const int32_t* est_offsets, const int32_t* ref_pairs, const int32_t* ref_offsets, int T,
                   int B, int tol_begin, int tol_end, int32_t* stats)
{
    const int64_t etot = est_offsets[B], rtot = ref_offsets[B];
#pragma omp parallel for schedule(dynamic, 8)
    for (int c = 0; c < B; ++c) {
        int32_t* out = stats + (size_t)7 * c;
        const PairList est{est_pairs, est_offsets[c], est_offsets[c + 1]}, ref{ref_pairs, ref_offsets[c], ref_offsets[c + 1]};
        const bool ok = etot >= 0 && rtot >= 0 && est.lo >= 0 && est.lo <= est.hi && est.hi <= etot && ref.lo >= 0 && ref.lo <= ref.hi &&
                        ref.hi <= rtot && list_valid(est, T) && list_valid(ref, T);
        if (!ok) {
            for (int k = 0; k < 7; ++k) out[k] = -1;
            continue;
        }
        out[0] = (int32_t)ref.size();
        out[1] = (int32_t)est.size();
        out[2] = match_count(est, ref, 0, 0);
        out[3] = list_frames(ref);
        out[4] = list_frames(est);
        out[5] = both_frames(est, ref);
        out[6] = tol_begin == 0 && tol_end == 0 ? out[2] : match_count(est, ref, tol_begin, tol_end);
    }
}

// k-best Viterbi (include/semicrf_hip.h: semicrf_viterbi_nbest; the device kernel is nbest.hip).  Per frame and chain a sorted
// list of at most k partial paths, each (value, base, order word); a candidate's ranks are tried in ascending order and the scan of
// a candidate stops at the first rank whose two singleton variants both fail to beat the list's k-th entry (later ranks of the
// same candidate are no better).  Back-pointer word: (cidx << 5) | (rank << 1) | singleton, cidx 0 = skip, else the other
// endpoint + 1; the order word is that ^ (s[t,t] > 0), so "on" sorts first exactly when decode would take it; -1 = absent rank.
namespace {
struct NbItem {
    float v, b;
    int32_t o;
};
inline bool nb_better(const NbItem& x, const NbItem& y)
{
    return x.v > y.v || (x.v == y.v && (x.b > y.b || (x.b == y.b && x.o < y.o)));
}
// insert into the sorted list L[0..n) of capacity k; false when x does not make the list
inline bool nb_insert(NbItem* L, int& n, int k, const NbItem& x)
{
    if (n == k && !nb_better(x, L[k - 1])) return false;
    int i = n < k ? n++ : k - 1;
    while (i > 0 && nb_better(x, L[i - 1])) { L[i] = L[i - 1]; --i; }
    L[i] = x;
    return true;
}
}  // namespace

void viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int32_t* start, int forward, int32_t* pairs,
                   int64_t cap, int32_t* offsets, float* scores, int32_t* npaths)
{
    const size_t Bs = (size_t)B, K = (size_t)k;
    std::vector<float> u((size_t)T * K * Bs);             // [frame][rank][chain]
    std::vector<int32_t> code((size_t)T * K * Bs);
    std::vector<int32_t> cnt((size_t)T * Bs);
#pragma omp parallel for schedule(dynamic, 1)
    for (int c0 = 0; c0 < B; c0 += CB) {
        const int nc = B - c0 < CB ? B - c0 : CB;
        NbItem L[CB][16];
        int n[CB];
        for (int p = 0; p < T; ++p) {
            const int t = forward ? p : T - 1 - p;
            const float* dg = score + ((size_t)t * T + t) * Bs + c0;
            for (int c = 0; c < nc; ++c) n[c] = 0;
            // candidate cidx with predecessor frame q and cell value x, for chain c of the block
            auto push = [&](int c, int q, float x, int32_t cidx) {
                const float d = dg[c];
                const int32_t flip = d > 0.0f ? 1 : 0;
                const int np = cnt[(size_t)q * Bs + c0 + c];
                for (int r = 0; r < np; ++r) {
                    const float base = u[((size_t)q * K + r) * Bs + c0 + c] + x;
                    const int32_t w = (cidx << 5) | (r << 1);
                    const NbItem on{base + d, base, (w | 1) ^ flip}, off{base + 0.0f, base, w ^ flip};
                    const bool a = nb_insert(L[c], n[c], k, flip ? on : off);
                    const bool b = nb_insert(L[c], n[c], k, flip ? off : on);
                    if (!a && !b) break;
                }
            };
            if (p == 0) {                                  // the terminal frame: the empty path, with or without (t,t)
                for (int c = 0; c < nc; ++c) {
                    const float d = dg[c];
                    const int32_t flip = d > 0.0f ? 1 : 0;
                    const NbItem on{0.0f + d, 0.0f, 1 ^ flip}, off{0.0f + 0.0f, 0.0f, 0 ^ flip};
                    nb_insert(L[c], n[c], k, flip ? on : off);
                    nb_insert(L[c], n[c], k, flip ? off : on);
                }
            } else if (forward) {
                for (int c = 0; c < nc; ++c) push(c, t - 1, noise[(size_t)(t - 1) * Bs + c0 + c], 0);
                for (int j = 0; j < t; ++j) {
                    const float* cell = score + ((size_t)t * T + j) * Bs + c0;
                    for (int c = 0; c < nc; ++c) push(c, j, cell[c], j + 1);
                }
            } else {
                for (int c = 0; c < nc; ++c) push(c, t + 1, noise[(size_t)t * Bs + c0 + c], 0);
                for (int e = t + 1; e < T; ++e) {
                    const float* cell = score + ((size_t)e * T + t) * Bs + c0;
                    for (int c = 0; c < nc; ++c) push(c, e, cell[c], e + 1);
                }
            }
            for (int c = 0; c < nc; ++c) {
                const int32_t flip = dg[c] > 0.0f ? 1 : 0;
                cnt[(size_t)t * Bs + c0 + c] = n[c];
                for (int r = 0; r < k; ++r) {
                    const size_t at = ((size_t)t * K + r) * Bs + c0 + c;
                    u[at] = r < n[c] ? L[c][r].v : -INFINITY;
                    code[at] = r < n[c] ? (L[c][r].o ^ flip) : -1;
                }
            }
        }
    }
    // the walks, one per (rank, chain), in decode's emission order
    const int64_t nB = (int64_t)k * B;
    std::vector<std::vector<int32_t>> out((size_t)nB);
#pragma omp parallel for schedule(dynamic, 8)
    for (int64_t idx = 0; idx < nB; ++idx) {
        const int r0 = (int)(idx / B), c = (int)(idx % B);
        const int st = start ? start[c] : (forward ? T - 1 : 0);
        if (r0 == 0) npaths[c] = cnt[(size_t)st * Bs + c];
        const bool present = r0 < cnt[(size_t)st * Bs + c];
        scores[idx] = present ? u[((size_t)st * K + r0) * Bs + c] : -INFINITY;
        if (!present) continue;
        std::vector<int32_t>& o = out[(size_t)idx];
        const int term = forward ? 0 : T - 1;
        int j = st, r = r0;
        for (;;) {
            const int32_t w = code[((size_t)j * K + r) * Bs + c];
            if (w & 1) { o.push_back(j); o.push_back(j); }
            if (j == term) break;
            const int32_t cidx = w >> 5;
            r = (w >> 1) & 15;
            if (cidx == 0) j += forward ? -1 : 1;
            else {
                const int q = cidx - 1;
                o.push_back(forward ? q : j);
                o.push_back(forward ? j : q);
                j = q;
            }
        }
        if (forward) {                                     // emitted descending: ascending like decode's
            std::vector<int32_t> a;
            for (size_t i = o.size(); i >= 2; i -= 2) { a.push_back(o[i - 2]); a.push_back(o[i - 1]); }
            o.swap(a);
        }
    }
    int64_t m = 0;
    for (int64_t idx = 0; idx < nB; ++idx) {
        offsets[idx] = (int32_t)m;
        const std::vector<int32_t>& o = out[(size_t)idx];
        for (size_t i = 0; i + 1 < o.size(); i += 2, ++m)
            if (m < cap) { pairs[2 * m] = o[i]; pairs[2 * m + 1] = o[i + 1]; }
    }
    offsets[nB] = (int32_t)m;
}

// evalPath (:508-550): sum of the path's interval scores plus the noise of every gap no interval covers
void eval_path(const float* score, const float* noise, int T, int B, const int32_t* pairs, const int32_t* offsets, float* out)
{
    const size_t Bs = (size_t)B;
#pragma omp parallel for schedule(dynamic, 8)
    for (int c = 0; c < B; ++c) {
        std::vector<double> cum((size_t)T, 0.0);
        for (int t = 1; t < T; ++t) cum[(size_t)t] = cum[(size_t)t - 1] + (double)noise[(size_t)(t - 1) * Bs + c];
        double acc = T > 0 ? cum[(size_t)T - 1] : 0.0;
        for (int i = offsets[c]; i < offsets[c + 1]; ++i) {
            const int b = pairs[2 * i], e = pairs[2 * i + 1];
            acc += (double)score[((size_t)e * T + b) * Bs + c] - (cum[(size_t)e] - cum[(size_t)b]);
        }
        out[c] = (float)acc;
    }
}

// gradient of sum_c gout[c] evalPath[c], ADDED to dScore / dNoise (either may be null)
void eval_path_bwd(const float* gout, int T, int B, const int32_t* pairs, const int32_t* offsets, float* dScore, float* dNoise)
{
    const size_t Bs = (size_t)B;
#pragma omp parallel for schedule(dynamic, 8)
    for (int c = 0; c < B; ++c) {
        // the derivative of eval_path above, which is LINEAR in the noise: every gap counts once (cum[T-1]) and once less per
        // interval that covers it -- also for overlapping intervals, where a 0/1 "covered" flag is not the derivative of the
        // forward (the reference's gathers :540-548 and evalpath.hip's eval_path_bwd_pairs_kernel agree)
        if (dNoise)
            for (int t = 0; t + 1 < T; ++t) dNoise[(size_t)t * Bs + c] += gout[c];
        for (int i = offsets[c]; i < offsets[c + 1]; ++i) {
            const int b = pairs[2 * i], e = pairs[2 * i + 1];
            if (dScore) dScore[((size_t)e * T + b) * Bs + c] += gout[c];
            if (dNoise)
                for (int t = b; t < e; ++t) dNoise[(size_t)t * Bs + c] -= gout[c];
        }
    }
}

// ---- attribute-head training loss (ModelTransformer.py:284-328) -------------------------------------------------------------
namespace {
// max and log(sum exp(x - max)) of a row's velocity logits, in double
inline void row_logsumexp(const float* x, double& m, double& logs)
{
    using semicrf::attr_loss::NVEL;
    m = x[0];
    for (int k = 1; k < NVEL; ++k) m = std::max(m, (double)x[k]);
    double sum = 0.0;
    for (int k = 0; k < NVEL; ++k) sum += exp((double)x[k] - m);
    logs = log(sum);
}
}  // namespace

void attribute_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int32_t* velocity, const float* ofRefined,
                        const float* ofPresence, int64_t K, const int32_t* offsets, int C, const float* base, float* rowLogProb, float* out)
{
    using namespace semicrf::attr_loss;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < K; ++i) {
        const float* x = logitsVelocity + (size_t)i * NVEL;
        double m, logs, lpOF, lpPres;
        row_logsumexp(x, m, logs);
        const int v = velocity[i];
        const float lpVel = v >= 0 && v < NVEL ? (float)(((double)x[v] - m) - logs) : NAN;
        of_terms<double>(ofLogits + 4 * (size_t)i, ofRefined + 2 * (size_t)i, ofPresence + 2 * (size_t)i, lpOF, lpPres);
        rowLogProb[i] = (lpVel + (float)lpOF) + (float)lpPres;
    }
#pragma omp parallel for schedule(static)
    for (int c = 0; c < C; ++c) {
        const int64_t b = std::max<int64_t>(offsets[c], 0), e = std::min<int64_t>(offsets[c + 1], K);
        if (e <= b) { out[c] = base ? base[c] : 0.0f; continue; }
        float acc = rowLogProb[b];
        for (int64_t i = b + 1; i < e; ++i) acc += rowLogProb[i];
        out[c] = base ? acc + base[c] : acc;
    }
}

void attribute_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int32_t* velocity,
                        const float* ofRefined, const float* ofPresence, int64_t K, const int32_t* offsets, int C, float* dLogitsVelocity,
                        float* dOfLogits)
{
    using namespace semicrf::attr_loss;
#pragma omp parallel for schedule(dynamic, 8)
    for (int c = 0; c < C; ++c) {
        const double g = gout[(size_t)c * gstride];
        const int64_t b = std::max<int64_t>(offsets[c], 0), e = std::min<int64_t>(offsets[c + 1], K);
        for (int64_t i = b; i < e; ++i) {
            const float* x = logitsVelocity + (size_t)i * NVEL;
            float* d = dLogitsVelocity + (size_t)i * NVEL;
            double m, logs, dd[4];
            row_logsumexp(x, m, logs);
            const int v = velocity[i];
            for (int k = 0; k < NVEL; ++k) d[k] = (float)(g * ((k == v ? 1.0 : 0.0) - exp(((double)x[k] - m) - logs)));
            of_grads<double>(ofLogits + 4 * (size_t)i, ofRefined + 2 * (size_t)i, ofPresence + 2 * (size_t)i, dd);
            for (int j = 0; j < 4; ++j) dOfLogits[4 * (size_t)i + j] = (float)(g * dd[j]);
        }
    }
}

// ---- attribute-head readout of transcription (ModelTransformer.py:590-651) ----------------------------------------------------
void attribute_decode(const float* logitsVelocity, const float* ofLogits, int64_t K, int criterion, int64_t* velocityClass,
                      float* velocityMean, float* ofValue, unsigned char* ofPresence)
{
    using namespace semicrf::attr_decode;
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < K; ++i) {
        const float* x = logitsVelocity + (size_t)i * NVEL;
        double p[NVEL];
        double m = x[0];
        int first = 0;                                                        // the smallest index of the largest logit
        bool nan = x[0] != x[0];
        for (int w = 1; w < NVEL; ++w) {
            nan = nan || x[w] != x[w];
            if ((double)x[w] > m) { m = x[w]; first = w; }
        }
        double sum = 0.0;
        for (int w = 0; w < NVEL; ++w) { p[w] = exp((double)x[w] - m); sum += p[w]; }
        const bool finite = !nan && sum < INFINITY;                           // (a +inf or all -inf: inf - inf = NaN in the sum)
        for (int w = 0; w < NVEL; ++w) p[w] /= sum;
        int cls = 0;
        if (criterion == CRIT_HAMMING) {
            cls = first;
        } else if (criterion == CRIT_MSE) {
            double t = 0.0;
            for (int w = 0; w < NVEL; ++w) t += p[w] * w;
            velocityMean[i] = finite ? (float)t : NAN;
        } else if (criterion == CRIT_MATCH) {
            double best = -1.0;
            for (int v = 0; v < NVEL; ++v) {
                double r = 0.0;                                               // summed directly, ascending w: equal windows tie exactly
                for (int w = std::max(v - MATCH_RADIUS, 0); w <= std::min(v + MATCH_RADIUS, NVEL - 1); ++w) r += p[w];
                if (r > best) { best = r; cls = v; }
            }
        } else {
            double c = 0.0;
            cls = 0;
            for (int v = 0; v < NVEL; ++v) {
                c += p[v];
                if (c > 0.5) { cls = v; break; }
            }
        }
        if (criterion != CRIT_MSE) velocityClass[i] = finite ? cls : 0;
        const float* of = ofLogits + 4 * (size_t)i;
        ofValue[2 * (size_t)i] = (float)of_value<double>((double)of[0]);
        ofValue[2 * (size_t)i + 1] = (float)of_value<double>((double)of[1]);
        ofPresence[2 * (size_t)i] = of_presence(of[2]);
        ofPresence[2 * (size_t)i + 1] = of_presence(of[3]);
    }
}

// the dropout mask of the training heads (attr_heads_math.h): element (row i, packed column j) of `head`
static inline bool dropout_keep(const semicrf::attr_heads::DropoutParams& drop, int64_t i, int j, int head)
{
    if (!drop.on[head]) return true;
    uint32_t draw[4];
    semicrf::attr_heads::dropout_draws(drop.seed, (uint32_t)(i >> 2), (uint32_t)j, draw);
    return draw[i & 3] >= drop.thr[head];
}
static inline float dropout_apply(const semicrf::attr_heads::DropoutParams& drop, int64_t i, int j, int head, float g)
{
    if (!drop.on[head]) return g;
    return dropout_keep(drop, i, j, head) ? g * drop.scale[head] : 0.0f;
}

// ---- the two attribute heads (semicrf_attribute_heads; ModelTransformer.py:578-590, :638) ---------------------------------------
// The order of operations of attr_heads.hip per output element, in fp32: the k chain of layer 1 ascending from +0 (fmaf), + b1, gelu,
// per slice of HEADS_SLICE hidden columns the chain of layer 2 ascending from +0, the slices' sums added in ascending order, b2 last.
// zsave != nullptr: the training forward (z saved; a head with drop.on masked and scaled between gelu and layer 2)
static void attribute_heads_impl(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets,
                                 int nSym, const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                                 float* logitsVelocity, float* ofLogits, int64_t* symIdx, int64_t* scatterIdx, float* zsave,
                                 const semicrf::attr_heads::DropoutParams& drop)
{
    using namespace semicrf::attr_heads;
    const int nk = 3 * D, H = Hv + Ho;
#pragma omp parallel
    {
        std::vector<float> x((size_t)nk), h((size_t)H);
#pragma omp for schedule(dynamic, 4)
        for (int64_t i = 0; i < K; ++i) {
            int lo = 0, hi = C;                                               // chain_of_interval (chain_search.h)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (offsets[mid] <= i) lo = mid; else hi = mid;
            }
            const int c = lo;
            const int b = std::min(std::max(pairs[2 * i], 0), T - 1), e = std::min(std::max(pairs[2 * i + 1], 0), T - 1);
            const float* pa = ctx + ((size_t)c * T + b) * ldc;
            const float* pb = ctx + ((size_t)c * T + e) * ldc;
            for (int d = 0; d < D; ++d) { x[d] = pa[d]; x[D + d] = pb[d]; x[2 * D + d] = pa[d] * pb[d]; }
            std::fill(h.begin(), h.end(), 0.0f);
            for (int k = 0; k < nk; ++k) {
                const float xv = x[k];
                const float* w = W1 + (size_t)k * H;
                for (int j = 0; j < H; ++j) h[j] = fmaf(xv, w[j], h[j]);
            }
            if (!zsave) {
                for (int j = 0; j < H; ++j) h[j] = gelu<float>(h[j] + b1[j]);
            } else {
                for (int j = 0; j < H; ++j) {
                    const float zz = h[j] + b1[j];
                    zsave[(size_t)i * H + j] = zz;
                    h[j] = dropout_apply(drop, i, j, j < Hv ? 0 : 1, gelu<float>(zz));
                }
            }
            for (int head = 0; head < 2; ++head) {
                const int Hh = head ? Ho : Hv, N = head ? No : Nv;
                const float* g = h.data() + (head ? Hv : 0);
                const float* w2 = head ? W2 + (size_t)Hv * Nv : W2;
                const float* bias = head ? b2 + Nv : b2;
                float* out = head ? ofLogits + (size_t)i * No : logitsVelocity + (size_t)i * Nv;
                for (int n = 0; n < N; ++n) {
                    float t = 0.0f;
                    for (int j0 = 0; j0 < Hh; j0 += HEADS_SLICE) {
                        float p = 0.0f;
                        for (int j = j0; j < std::min(j0 + HEADS_SLICE, Hh); ++j) p = fmaf(g[j], w2[(size_t)j * N + n], p);
                        t = j0 == 0 ? p : t + p;
                    }
                    out[n] = t + bias[n];
                }
            }
            if (symIdx) symIdx[i] = c % nSym;
            if (scatterIdx) scatterIdx[i] = c;
        }
    }
}

void attribute_heads(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets, int nSym,
                     const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                     float* logitsVelocity, float* ofLogits, int64_t* symIdx, int64_t* scatterIdx)
{
    attribute_heads_impl(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits, symIdx, scatterIdx,
                         nullptr, semicrf::attr_heads::dropout_params(0, 0.0, 0.0));
}

void attribute_heads_train_fwd(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets,
                               int nSym, const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                               uint64_t seed, double pv, double po, float* logitsVelocity, float* ofLogits, float* z, int64_t* symIdx,
                               int64_t* scatterIdx)
{
    attribute_heads_impl(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits, symIdx, scatterIdx,
                         z, semicrf::attr_heads::dropout_params(seed, pv, po));
}

void attribute_heads_dropout_mask(uint64_t seed, int64_t K, int Hv, int Ho, double pv, double po, unsigned char* mask)
{
    using namespace semicrf::attr_heads;
    const DropoutParams drop = dropout_params(seed, pv, po);
    const int H = Hv + Ho;
#pragma omp parallel for
    for (int64_t i = 0; i < K; ++i)
        for (int j = 0; j < H; ++j) mask[(size_t)i * H + j] = dropout_keep(drop, i, j, j < Hv ? 0 : 1) ? 1 : 0;
}

// The backward of the heads in the order of operations of attr_heads_bwd.hip (include/semicrf_hip.h), in fp32.
void attribute_heads_bwd(const float* dLv, const float* dOf, const float* z, const float* ctx, int C, int T, int D, int64_t ldc,
                         const int32_t* pairs, int64_t K, const int32_t* offsets, const float* W1, const float* W2, int Hv, int Ho, int Nv,
                         int No, uint64_t seed, double pv, double po, float* dctx, float* dW1, float* db1, float* dW2, float* db2)
{
    using namespace semicrf::attr_heads;
    const DropoutParams drop = dropout_params(seed, pv, po);
    const int H = Hv + Ho, nk = 3 * D;
    const int64_t nch = (K + HEADS_BWD_ROWS - 1) / HEADS_BWD_ROWS;
    std::fill(dctx, dctx + (size_t)C * T * D, 0.0f);
    if (K <= 0) return;
    std::vector<int64_t> fa((size_t)K), fb((size_t)K);       // the rows' two frames c T + b, c T + e
    std::vector<float> dz((size_t)K * H), g((size_t)K * 2 * D);
    auto head_of = [&](int j) { return j < Hv ? 0 : 1; };
    // dz = (dOut W2 * M) * gelu'(z), the contraction over n ascending
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t i = 0; i < K; ++i) {
        int lo = 0, hi = C;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= i) lo = mid; else hi = mid;
        }
        const int b = std::min(std::max(pairs[2 * i], 0), T - 1), e = std::min(std::max(pairs[2 * i + 1], 0), T - 1);
        fa[i] = (int64_t)lo * T + b;
        fb[i] = (int64_t)lo * T + e;
        for (int j = 0; j < H; ++j) {
            const int head = head_of(j), N = head ? No : Nv;
            const float* w = head ? W2 + (size_t)Hv * Nv + (size_t)(j - Hv) * No : W2 + (size_t)j * Nv;
            const float* d = head ? dOf + (size_t)i * No : dLv + (size_t)i * Nv;
            float t = 0.0f;
            for (int n = 0; n < N; ++n) t = fmaf(d[n], w[n], t);
            if (drop.on[head]) t = dropout_keep(drop, i, j, head) ? t * drop.scale[head] : 0.0f;
            dz[(size_t)i * H + j] = t * gelu_grad<float>(z[(size_t)i * H + j]);
        }
    }
    // sums over rows: one partial per chunk (rows ascending), the chunks' partials added in ascending order
    auto chunk_end = [&](int64_t ch) { return std::min<int64_t>(K, (ch + 1) * HEADS_BWD_ROWS); };
    // the bias gradients: per chunk 8 sums over r = q (mod 8) added in ascending q, all in double, rounded to fp32 once
    auto column_sum = [&](const float* src, size_t ld) {
        float total = 0.0f;
        for (int64_t ch = 0; ch < nch; ++ch) {
            double sub[HEADS_BWD_SUBSUMS];
            for (int q = 0; q < HEADS_BWD_SUBSUMS; ++q) {
                double t = 0.0;
                for (int64_t i = ch * HEADS_BWD_ROWS + q; i < chunk_end(ch); i += HEADS_BWD_SUBSUMS) t += (double)src[(size_t)i * ld];
                sub[q] = t;
            }
            double s = sub[0];
            for (int q = 1; q < HEADS_BWD_SUBSUMS; ++q) s += sub[q];
            total = ch == 0 ? (float)s : total + (float)s;
        }
        return total;
    };
#pragma omp parallel
    {
        std::vector<float> acc((size_t)std::max(std::max(Nv, No), H)), tot(acc.size());
#pragma omp for schedule(dynamic, 4) nowait
        for (int j = 0; j < H; ++j) {                         // dW2 row j, db1[j]
            const int head = head_of(j), N = head ? No : Nv;
            const float* dOut = head ? dOf : dLv;
            float* out = head ? dW2 + (size_t)Hv * Nv + (size_t)(j - Hv) * No : dW2 + (size_t)j * Nv;
            for (int64_t ch = 0; ch < nch; ++ch) {
                std::fill(acc.begin(), acc.begin() + N, 0.0f);
                for (int64_t i = ch * HEADS_BWD_ROWS; i < chunk_end(ch); ++i) {
                    const float a = dropout_apply(drop, i, j, head, gelu<float>(z[(size_t)i * H + j]));
                    const float* d = dOut + (size_t)i * N;
                    for (int n = 0; n < N; ++n) acc[n] = fmaf(a, d[n], acc[n]);
                }
                for (int n = 0; n < N; ++n) tot[n] = ch == 0 ? acc[n] : tot[n] + acc[n];
            }
            std::copy(tot.begin(), tot.begin() + N, out);
            db1[j] = column_sum(dz.data() + j, (size_t)H);
        }
#pragma omp for schedule(static) nowait
        for (int n = 0; n < Nv + No; ++n) db2[n] = n < Nv ? column_sum(dLv + n, (size_t)Nv) : column_sum(dOf + (n - Nv), (size_t)No);
#pragma omp for schedule(dynamic, 4)
        for (int k = 0; k < nk; ++k) {                        // dW1 row k = x[:, k]^T dz
            for (int64_t ch = 0; ch < nch; ++ch) {
                std::fill(acc.begin(), acc.begin() + H, 0.0f);
                for (int64_t i = ch * HEADS_BWD_ROWS; i < chunk_end(ch); ++i) {
                    const float* pa = ctx + (size_t)fa[i] * ldc;
                    const float* pb = ctx + (size_t)fb[i] * ldc;
                    const float xv = k < D ? pa[k] : k < 2 * D ? pb[k - D] : pa[k - 2 * D] * pb[k - 2 * D];
                    const float* d = dz.data() + (size_t)i * H;
                    for (int j = 0; j < H; ++j) acc[j] = fmaf(xv, d[j], acc[j]);
                }
                for (int j = 0; j < H; ++j) tot[j] = ch == 0 ? acc[j] : tot[j] + acc[j];
            }
            std::copy(tot.begin(), tot.begin() + H, dW1 + (size_t)k * H);
        }
        // dx = dz W1^T (j ascending), folded into (ga, gb) per row
#pragma omp for schedule(dynamic, 4)
        for (int64_t i = 0; i < K; ++i) {
            const float* pa = ctx + (size_t)fa[i] * ldc;
            const float* pb = ctx + (size_t)fb[i] * ldc;
            const float* d = dz.data() + (size_t)i * H;
            for (int dd = 0; dd < D; ++dd) {
                float dx[3];
                for (int t = 0; t < 3; ++t) {
                    const float* w = W1 + ((size_t)t * D + dd) * H;
                    float s = 0.0f;
                    for (int j = 0; j < H; ++j) s = fmaf(d[j], w[j], s);
                    dx[t] = s;
                }
                g[(2 * (size_t)i) * D + dd] = fmaf(dx[2], pb[dd], dx[0]);
                g[(2 * (size_t)i + 1) * D + dd] = fmaf(dx[2], pa[dd], dx[1]);
            }
        }
        // dctx: per chain its rows in ascending order, ga before gb
#pragma omp for schedule(dynamic, 1)
        for (int c = 0; c < C; ++c) {
            const int64_t lo = std::min<int64_t>(std::max<int64_t>(offsets[c], 0), K);
            const int64_t hi = c == C - 1 ? K : std::min<int64_t>(std::max<int64_t>(offsets[c + 1], 0), K);
            for (int64_t i = lo; i < hi; ++i) {
                const int b = std::min(std::max(pairs[2 * i], 0), T - 1), e = std::min(std::max(pairs[2 * i + 1], 0), T - 1);
                float* qb = dctx + ((size_t)c * T + b) * D;
                float* qe = dctx + ((size_t)c * T + e) * D;
                const float* gi = g.data() + 2 * (size_t)i * D;
                for (int dd = 0; dd < D; ++dd) { qb[dd] += gi[dd]; qe[dd] += gi[D + dd]; }
            }
        }
    }
}

// ---- the optimizer step (semicrf_grad_sqnorm / semicrf_clip_from_history / semicrf_adabelief_step; optim_math.h) ---------------------
// The norm's partial sums: blocks of SQNORM_PER_BLOCK consecutive elements, each summed in ascending order in double, block b into
// partial b % n (ascending b): a fixed order for a given numel.
void grad_sqnorm(const float* flat, int64_t numel, double* partials)
{
    using namespace semicrf::optim;
    const int n = sqnorm_partials(numel);
    const int64_t nblk = (numel + SQNORM_PER_BLOCK - 1) / SQNORM_PER_BLOCK;
    std::vector<double> blk((size_t)nblk);
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < nblk; ++b) {
        const int64_t lo = b * SQNORM_PER_BLOCK, hi = std::min<int64_t>(lo + SQNORM_PER_BLOCK, numel);
        double acc = 0.0;
        for (int64_t i = lo; i < hi; ++i) acc += (double)flat[i] * (double)flat[i];
        blk[(size_t)b] = acc;
    }
    for (int i = 0; i < n; ++i) partials[i] = 0.0;
    for (int64_t b = 0; b < nblk; ++b) partials[b % n] += blk[(size_t)b];
}

void clip_from_history(const double* partials, int64_t numel, const float* norm_in, double q, float* ring, int capacity, int32_t* state,
                       int append, float* stats)
{
    using namespace semicrf::optim;
    bool has_norm = false;
    float norm = 0.0f;
    if (partials) {
        const int n = sqnorm_partials(numel);
        double t = partials[0];
        for (int i = 1; i < n; ++i) t += partials[i];
        norm = (float)std::sqrt(t);
        has_norm = true;
    } else if (norm_in) {
        norm = *norm_in;
        has_norm = true;
    }
    const int count = std::min(std::max((int)state[0], 0), capacity), head = std::min(std::max((int)state[1], 0), capacity - 1);
    const bool want_clip = q >= 0.0;
    float clip = 0.0f;
    if (want_clip) {
        std::vector<float> v((size_t)count);
        bool nan = false;
        for (int i = 0; i < count; ++i) { v[(size_t)i] = ring[(head + i) % capacity]; nan = nan || v[(size_t)i] != v[(size_t)i]; }
        if (nan || count < 1) {
            clip = std::numeric_limits<float>::quiet_NaN();
        } else {
            std::sort(v.begin(), v.end());
            const double pos = q * (double)(count - 1);
            const int lo = std::min(std::max((int)std::floor(pos), 0), count - 1), hi = std::min(lo + 1, count - 1);
            clip = (float)quantile_lerp((double)v[(size_t)lo], (double)v[(size_t)hi], pos - (double)lo);
        }
    }
    if (has_norm) stats[0] = norm;
    if (want_clip) stats[1] = clip;
    if (has_norm && want_clip) stats[2] = clip_coef(clip, norm);
    if (append && has_norm) {
        if (count < capacity) {
            ring[(head + count) % capacity] = norm;
            state[0] = count + 1;
        } else {
            ring[head] = norm;
            state[1] = (head + 1) % capacity;
        }
    }
}

void adabelief_step(float* p, const float* g, float* m, float* s, int64_t numel, const float* coef_ptr,
                    const semicrf_adabelief_groups& groups)
{
    const float coef = coef_ptr ? *coef_ptr : 1.0f;
    for (int gi = 0; gi < groups.n; ++gi) {
        const int64_t lo = gi ? groups.g[gi - 1].end : 0, hi = std::min<int64_t>(groups.g[gi].end, numel);
        const semicrf_adabelief_group k = groups.g[gi];
#pragma omp parallel for schedule(static) if (hi - lo > 65536)
        for (int64_t i = lo; i < hi; ++i) semicrf::optim::adabelief_update(p[i], g[i], m[i], s[i], coef, k);
    }
}

// ---- the backbone's axial attention (semicrf_axial_attention; LayersTransformer.py:173-186) ------------------------------------------
// The order of operations of attention.hip per output element, in fp32 (attention_math.h): the chain of q . k over the head dimension
// ascending from +0 (fmaf), * scale, the maximum over the keys below Lk, exp of the difference, the sum as S0 + S1 (the keys of each
// half wave ascending), the chain of P V over the keys ascending from +0, / sum.  Only the exponential differs from the device's.
void axial_attention(const float* q, const float* k, const float* v, float* out, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d,
                     const int64_t* st)
{
    using namespace semicrf::attention;
    const float scale = scale_of(d);
    const int64_t nwork = n0 * n1 * H;
#pragma omp parallel
    {
        std::vector<float> p((size_t)Lk), acc((size_t)d);
#pragma omp for schedule(static)
        for (int64_t w = 0; w < nwork; ++w) {
            const int h = (int)(w % H);
            const int64_t s = w / H, s0 = s / n1, s1 = s % n1;
            const float* qb = q + s0 * st[0] + s1 * st[1] + (int64_t)h * d;
            const float* kb = k + s0 * st[3] + s1 * st[4] + (int64_t)h * d;
            const float* vb = v + s0 * st[6] + s1 * st[7] + (int64_t)h * d;
            float* ob = out + s0 * st[9] + s1 * st[10] + (int64_t)h * d;
            for (int i = 0; i < Lq; ++i) {
                const float* qi = qb + (int64_t)i * st[2];
                float mx = -std::numeric_limits<float>::infinity();
                for (int j = 0; j < Lk; ++j) {
                    const float* kj = kb + (int64_t)j * st[5];
                    float t = 0.0f;
                    for (int c = 0; c < d; ++c) t = fmaf(kj[c], qi[c], t);
                    p[j] = t * scale;
                    mx = std::max(mx, p[j]);
                }
                float half[2] = {0.0f, 0.0f};
                for (int j = 0; j < Lk; ++j) {
                    p[j] = expf(p[j] - mx);
                    half[sum_half(j)] += p[j];
                }
                const float sum = half[0] + half[1];
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int j = 0; j < Lk; ++j) {
                    const float* vj = vb + (int64_t)j * st[8];
                    const float pj = p[j];
                    for (int c = 0; c < d; ++c) acc[c] = fmaf(pj, vj[c], acc[c]);
                }
                float* oi = ob + (int64_t)i * st[11];
                for (int c = 0; c < d; ++c) oi[c] = acc[c] / sum;
            }
        }
    }
}

// semicrf_axial_attention_bf16: the chain of attention_bf16_math.h.  The products of bf16 values are exact in fp32; both sums over them
// are plain fp32 additions ascending from +0 (the device sums 16 products inside one matrix instruction: equal wherever the partial
// sums are exact, equal to rounding elsewhere); the weights are rounded to bf16 BEFORE they are summed and before they meet V.
void axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int64_t n0, int64_t n1, int Lq, int Lk, int H,
                          int d, const int64_t* st)
{
    using namespace semicrf::attention;
    const float scale = scale_of(d);
    const int64_t nwork = n0 * n1 * H;
#pragma omp parallel
    {
        std::vector<float> p((size_t)Lk), acc((size_t)d), qf((size_t)d);
#pragma omp for schedule(static)
        for (int64_t w = 0; w < nwork; ++w) {
            const int h = (int)(w % H);
            const int64_t s = w / H, s0 = s / n1, s1 = s % n1;
            const uint16_t* qb = q + s0 * st[0] + s1 * st[1] + (int64_t)h * d;
            const uint16_t* kb = k + s0 * st[3] + s1 * st[4] + (int64_t)h * d;
            const uint16_t* vb = v + s0 * st[6] + s1 * st[7] + (int64_t)h * d;
            uint16_t* ob = out + s0 * st[9] + s1 * st[10] + (int64_t)h * d;
            for (int i = 0; i < Lq; ++i) {
                const uint16_t* qi = qb + (int64_t)i * st[2];
                for (int c = 0; c < d; ++c) qf[c] = bf16_to_float(qi[c]);
                float mx = -std::numeric_limits<float>::infinity();
                for (int j = 0; j < Lk; ++j) {
                    const uint16_t* kj = kb + (int64_t)j * st[5];
                    float t = 0.0f;
                    for (int c = 0; c < d; ++c) t += bf16_to_float(kj[c]) * qf[c];
                    p[j] = t * scale;
                    mx = fmaxf(mx, p[j]);                            // as the device: a NaN score does not become the maximum
                }
                float half[2] = {0.0f, 0.0f};
                for (int j = 0; j < Lk; ++j) {
                    p[j] = bf16_to_float(bf16_rne(expf(p[j] - mx)));
                    half[sum_half(j)] += p[j];
                }
                const float sum = half[0] + half[1];
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int j = 0; j < Lk; ++j) {
                    const uint16_t* vj = vb + (int64_t)j * st[8];
                    const float pj = p[j];
                    for (int c = 0; c < d; ++c) acc[c] += pj * bf16_to_float(vj[c]);
                }
                uint16_t* oi = ob + (int64_t)i * st[11];
                for (int c = 0; c < d; ++c) oi[c] = bf16_rne(acc[c] / sum);
            }
        }
    }
}

// The order of operations of attention_bwd.hip per gradient element (attention_math.h): the forward's sc, m, p, sum; D and dP chains
// over the head dimension ascending; P = p / sum; dS = P (dP - D); dq, dk, dv chains in bwd_order, * scale for dq and dk.  P and dS of
// one (sequence, head) are kept [Lq][Lk] so that dk and dv walk the queries in their fixed order.  st: q, k, v, out, dout, dq, dk, dv.
void axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk, float* dv,
                         int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, const int64_t* st)
{
    using namespace semicrf::attention;
    const float scale = scale_of(d);
    const int64_t nwork = n0 * n1 * H;
    const int Lqp = key_tiles(Lq) * ATT_TILE, Lkp = key_tiles(Lk) * ATT_TILE;
#pragma omp parallel
    {
        std::vector<float> P((size_t)Lq * Lk), dS((size_t)Lq * Lk), acc((size_t)d), acc2((size_t)d);
#pragma omp for schedule(static)
        for (int64_t w = 0; w < nwork; ++w) {
            const int h = (int)(w % H);
            const int64_t s = w / H, s0 = s / n1, s1 = s % n1, hd = (int64_t)h * d;
            auto base = [&](auto* p, int t) { return p + s0 * st[3 * t] + s1 * st[3 * t + 1] + hd; };
            const float *qb = base(q, 0), *kb = base(k, 1), *vb = base(v, 2), *ob = base(out, 3), *gb = base(dout, 4);
            for (int i = 0; i < Lq; ++i) {
                const float* qi = qb + (int64_t)i * st[2];
                const float* gi = gb + (int64_t)i * st[14];
                const float* oi = ob + (int64_t)i * st[11];
                float* p = &P[(size_t)i * Lk];
                float* ds = &dS[(size_t)i * Lk];
                float mx = -std::numeric_limits<float>::infinity();
                for (int j = 0; j < Lk; ++j) {
                    const float* kj = kb + (int64_t)j * st[5];
                    float t = 0.0f;
                    for (int c = 0; c < d; ++c) t = fmaf(kj[c], qi[c], t);
                    p[j] = t * scale;
                    mx = std::max(mx, p[j]);
                }
                float half[2] = {0.0f, 0.0f};
                for (int j = 0; j < Lk; ++j) {
                    p[j] = expf(p[j] - mx);
                    half[sum_half(j)] += p[j];
                }
                const float sum = half[0] + half[1];
                float D = 0.0f;
                for (int c = 0; c < d; ++c) D = fmaf(gi[c], oi[c], D);
                for (int j = 0; j < Lk; ++j) {
                    const float* vj = vb + (int64_t)j * st[8];
                    float dp = 0.0f;
                    for (int c = 0; c < d; ++c) dp = fmaf(vj[c], gi[c], dp);
                    p[j] = p[j] / sum;
                    ds[j] = p[j] * (dp - D);
                }
                if (dq) {
                    std::fill(acc.begin(), acc.end(), 0.0f);
                    for (int t = 0; t < Lkp; ++t) {
                        const int j = bwd_order(t);
                        if (j >= Lk) continue;
                        const float* kj = kb + (int64_t)j * st[5];
                        for (int c = 0; c < d; ++c) acc[c] = fmaf(ds[j], kj[c], acc[c]);
                    }
                    float* dqi = base(dq, 5) + (int64_t)i * st[17];
                    for (int c = 0; c < d; ++c) dqi[c] = acc[c] * scale;
                }
            }
            if (!dk && !dv) continue;
            for (int j = 0; j < Lk; ++j) {
                std::fill(acc.begin(), acc.end(), 0.0f);
                std::fill(acc2.begin(), acc2.end(), 0.0f);
                for (int t = 0; t < Lqp; ++t) {
                    const int i = bwd_order(t);
                    if (i >= Lq) continue;
                    const float* qi = qb + (int64_t)i * st[2];
                    const float* gi = gb + (int64_t)i * st[14];
                    const float dsij = dS[(size_t)i * Lk + j], pij = P[(size_t)i * Lk + j];
                    for (int c = 0; c < d; ++c) {
                        acc[c] = fmaf(dsij, qi[c], acc[c]);
                        acc2[c] = fmaf(pij, gi[c], acc2[c]);
                    }
                }
                if (dk) {
                    float* dkj = base(dk, 6) + (int64_t)j * st[20];
                    for (int c = 0; c < d; ++c) dkj[c] = acc[c] * scale;
                }
                if (dv) {
                    float* dvj = base(dv, 7) + (int64_t)j * st[23];
                    for (int c = 0; c < d; ++c) dvj[c] = acc2[c];
                }
            }
        }
    }
}

// semicrf_axial_attention_bf16_bwd: the backward chain of attention_bf16_math.h.  s, m, ph and sum as axial_attention_bf16 forms them;
// P = ph / sum; dP and the three gradient sums plain fp32 additions of exact products ascending from +0; D as the two half-wave
// chains of `sum`; dS and P rounded to bf16 before they meet k, q and dout.  P and dS of one (sequence, head) are kept [Lq][Lk] in
// their rounded form.  st: q, k, v, dout, dq, dk, dv.
void axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk, uint16_t* dv,
                              int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, const int64_t* st)
{
    using namespace semicrf::attention;
    const float scale = scale_of(d);
    const int64_t nwork = n0 * n1 * H;
#pragma omp parallel
    {
        std::vector<float> Ph((size_t)Lq * Lk), dSh((size_t)Lq * Lk), p((size_t)Lk), dp((size_t)Lk), acc((size_t)d), acc2((size_t)d), qf((size_t)d),
            gf((size_t)d);
#pragma omp for schedule(static)
        for (int64_t w = 0; w < nwork; ++w) {
            const int h = (int)(w % H);
            const int64_t s = w / H, s0 = s / n1, s1 = s % n1, hd = (int64_t)h * d;
            auto base = [&](auto* x, int t) { return x + s0 * st[3 * t] + s1 * st[3 * t + 1] + hd; };
            const uint16_t *qb = base(q, 0), *kb = base(k, 1), *vb = base(v, 2), *gb = base(dout, 3);
            for (int i = 0; i < Lq; ++i) {
                const uint16_t* qi = qb + (int64_t)i * st[2];
                const uint16_t* gi = gb + (int64_t)i * st[11];
                for (int c = 0; c < d; ++c) { qf[c] = bf16_to_float(qi[c]); gf[c] = bf16_to_float(gi[c]); }
                float mx = -std::numeric_limits<float>::infinity();
                for (int j = 0; j < Lk; ++j) {
                    const uint16_t* kj = kb + (int64_t)j * st[5];
                    float t = 0.0f;
                    for (int c = 0; c < d; ++c) t += bf16_to_float(kj[c]) * qf[c];
                    p[j] = t * scale;
                    mx = fmaxf(mx, p[j]);
                }
                float half[2] = {0.0f, 0.0f};
                for (int j = 0; j < Lk; ++j) {
                    p[j] = bf16_to_float(bf16_rne(expf(p[j] - mx)));
                    half[sum_half(j)] += p[j];
                }
                const float sum = half[0] + half[1];
                float dhalf[2] = {0.0f, 0.0f};
                for (int j = 0; j < Lk; ++j) {
                    const uint16_t* vj = vb + (int64_t)j * st[8];
                    float t = 0.0f;
                    for (int c = 0; c < d; ++c) t += bf16_to_float(vj[c]) * gf[c];
                    dp[j] = t;
                    p[j] = p[j] / sum;
                    dhalf[sum_half(j)] += p[j] * t;
                }
                const float D = dhalf[0] + dhalf[1];
                for (int j = 0; j < Lk; ++j) {
                    Ph[(size_t)i * Lk + j] = bf16_to_float(bf16_rne(p[j]));
                    dSh[(size_t)i * Lk + j] = bf16_to_float(bf16_rne(p[j] * (dp[j] - D)));
                }
                if (dq) {
                    std::fill(acc.begin(), acc.end(), 0.0f);
                    for (int j = 0; j < Lk; ++j) {
                        const uint16_t* kj = kb + (int64_t)j * st[5];
                        const float ds = dSh[(size_t)i * Lk + j];
                        for (int c = 0; c < d; ++c) acc[c] += ds * bf16_to_float(kj[c]);
                    }
                    uint16_t* dqi = base(dq, 4) + (int64_t)i * st[14];
                    for (int c = 0; c < d; ++c) dqi[c] = bf16_rne(acc[c] * scale);
                }
            }
            if (!dk && !dv) continue;
            for (int j = 0; j < Lk; ++j) {
                std::fill(acc.begin(), acc.end(), 0.0f);
                std::fill(acc2.begin(), acc2.end(), 0.0f);
                for (int i = 0; i < Lq; ++i) {
                    const uint16_t* qi = qb + (int64_t)i * st[2];
                    const uint16_t* gi = gb + (int64_t)i * st[11];
                    const float ds = dSh[(size_t)i * Lk + j], ph = Ph[(size_t)i * Lk + j];
                    for (int c = 0; c < d; ++c) {
                        acc[c] += ds * bf16_to_float(qi[c]);
                        acc2[c] += ph * bf16_to_float(gi[c]);
                    }
                }
                if (dk) {
                    uint16_t* dkj = base(dk, 5) + (int64_t)j * st[17];
                    for (int c = 0; c < d; ++c) dkj[c] = bf16_rne(acc[c] * scale);
                }
                if (dv) {
                    uint16_t* dvj = base(dv, 6) + (int64_t)j * st[20];
                    for (int c = 0; c < d; ++c) dvj[c] = bf16_rne(acc2[c]);
                }
            }
        }
    }
}

// ---- the backbone's feed-forward ResBlock (semicrf_ffn_residual) --------------------------------------------------------------------
// The order of operations of ffn.hip per output element, in fp32 (ffn_math.h): the sum of squares as four strided chains added pairwise,
// rs = 1 / sqrt(ss / D + eps), xn = x rs, the chain of W1 xn over k ascending from +0 (fmaf), + b1, gelu, per hidden chunk the chain of
// W2 g over its columns ascending from +0 (on over the zero padding of the last chunk), the chunks' sums added in ascending order from
// +0, (+ b2) * scale, + x.  Only erf and erfc differ from the device's.
// drop / zs / ys: the training mode (z and y saved, both dropouts), NULL in eval mode
static void ffn_residual_any(const float* x, float* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                             const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps,
                             const semicrf::ffn::DropoutParams* drop, float* zs, float* ys)
{
    using namespace semicrf::ffn;
    const int64_t ntok = n0 * n1;
#pragma omp parallel
    {
        std::vector<float> xn((size_t)D), g((size_t)FFN_CHUNK), acc((size_t)D);
#pragma omp for schedule(static)
        for (int64_t t = 0; t < ntok; ++t) {
            const int64_t i0 = t / n1, i1 = t % n1;
            const float* xt = x + i0 * xs0 + i1 * xs1;
            float* ot = out + i0 * os0 + i1 * os1;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < D; ++k) s[k & 3] = fmaf(xt[k], xt[k], s[k & 3]);
            const float rs = rs_of(sumsq_combine(s[0], s[1], s[2], s[3]), D, eps);
            for (int k = 0; k < D; ++k) xn[k] = xt[k] * rs;
            std::fill(acc.begin(), acc.end(), 0.0f);
            for (int j0 = 0; j0 < H; j0 += FFN_CHUNK) {
                const int wv = std::min(FFN_CHUNK, H - j0);
                for (int j = 0; j < wv; ++j) {
                    const float* w = W1 + (int64_t)(j0 + j) * D;
                    float h = 0.0f;
                    for (int k = 0; k < D; ++k) h = fmaf(xn[k], w[k], h);
                    if (drop) {
                        const float zz = h + b1[j0 + j];
                        zs[t * H + j0 + j] = zz;
                        const float a = semicrf::attr_heads::gelu<float>(zz);
                        g[j] = keep(*drop, 0, t, j0 + j) ? (drop->on[0] ? a * drop->scale[0] : a) : 0.0f;
                    } else {
                        g[j] = semicrf::attr_heads::gelu<float>(h + b1[j0 + j]);
                    }
                }
                for (int n = 0; n < D; ++n) {
                    const float* w = W2 + (int64_t)n * H + j0;
                    float a = 0.0f;                          // the chunk's own sum, from +0
                    for (int j = 0; j < wv; ++j) a = fmaf(g[j], w[j], a);
                    if (wv < FFN_CHUNK) a = fmaf(0.0f, 0.0f, a);          // the device's zero padding: -0 becomes +0, nothing else changes
                    acc[n] += a;                             // chunks ascending
                }
            }
            if (drop) {
                for (int n = 0; n < D; ++n) {
                    const float yy = acc[n] + b2[n];
                    ys[t * D + n] = yy;
                    ot[n] = xt[n] + (keep(*drop, 1, t, n) ? (drop->on[1] ? yy * drop->scale[1] : yy) : 0.0f) * scale[n];
                }
            } else {
                for (int n = 0; n < D; ++n) ot[n] = epilogue(xt[n], acc[n], b2[n], scale[n]);
            }
        }
    }
}

void ffn_residual(const float* x, float* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                  const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps)
{
    ffn_residual_any(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, nullptr, nullptr, nullptr);
}

// ---- the block in training (semicrf_ffn_residual_train_fwd / _bwd / semicrf_ffn_dropout_mask) ----------------------------------------------
void ffn_residual_train_fwd(const float* x, float* out, float* z, float* y, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                            int64_t os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2, const float* scale,
                            float eps, uint64_t seed, double p1, double p2)
{
    const semicrf::ffn::DropoutParams drop = semicrf::attr_heads::dropout_params(seed, p1, p2);
    ffn_residual_any(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, &drop, z, y);
}

void ffn_dropout_mask(uint64_t seed, int64_t rows, int D, int H, double p1, double p2, unsigned char* mask_hidden, unsigned char* mask_out)
{
    using namespace semicrf::ffn;
    const DropoutParams drop = semicrf::attr_heads::dropout_params(seed, p1, p2);
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < rows; ++i) {
        for (int j = 0; j < H; ++j) mask_hidden[i * H + j] = keep(drop, 0, i, j) ? 1 : 0;
        for (int n = 0; n < D; ++n) mask_out[i * D + n] = keep(drop, 1, i, n) ? 1 : 0;
    }
}

// The backward in the order of operations of ffn_bwd.hip (ffn_math.h), in fp32; only erf, erfc and exp differ from the device's.
void ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1,
                      int64_t xs0, int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const float* W1, const float* W2, const float* scale,
                      float eps, uint64_t seed, double p1, double p2, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale)
{
    using namespace semicrf::ffn;
    using semicrf::attr_heads::gelu;
    using semicrf::attr_heads::gelu_grad;
    const DropoutParams drop = semicrf::attr_heads::dropout_params(seed, p1, p2);
    const int64_t ntok = n0 * n1;
    auto off = [&](int64_t i, int64_t s0, int64_t s1) { return (i / n1) * s0 + (i % n1) * s1; };
    auto m1 = [&](int64_t i, int j, float v) { return keep(drop, 0, i, j) ? (drop.on[0] ? v * drop.scale[0] : v) : 0.0f; };
    auto m2 = [&](int64_t i, int n, float v) { return keep(drop, 1, i, n) ? (drop.on[1] ? v * drop.scale[1] : v) : 0.0f; };
    std::vector<float> rs((size_t)ntok), dy((size_t)ntok * D), dz((size_t)ntok * H), xn((size_t)ntok * D), av((size_t)ntok * H);
    // a chain over the contraction values k of `term`, in sub-chains of FFN_BWD_KSUB, padded with 0 * 0 up to a multiple of FFN_BWD_KSTEP
    auto chain = [&](int K, auto term) {
        float acc = 0.0f;
        for (int k0 = 0; k0 < K; k0 += FFN_BWD_KSUB) {
            const int k1 = std::min(K, k0 + FFN_BWD_KSUB);
            float part = 0.0f;
            for (int k = k0; k < k1; ++k) part = term(k, part);
            if (k1 == K && K % FFN_BWD_KSTEP) part = fmaf(0.0f, 0.0f, part);
            acc += part;
        }
        return acc;
    };
#pragma omp parallel for schedule(static)
    for (int64_t i = 0; i < ntok; ++i) {
        const float* xt = x + off(i, xs0, xs1);
        const float* gt = dout + off(i, gs0, gs1);
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < D; ++k) s[k & 3] = fmaf(xt[k], xt[k], s[k & 3]);
        rs[i] = rs_of(sumsq_combine(s[0], s[1], s[2], s[3]), D, eps);
        for (int k = 0; k < D; ++k) xn[i * D + k] = xt[k] * rs[i];
        for (int n = 0; n < D; ++n) dy[i * D + n] = m2(i, n, gt[n] * scale[n]);
        for (int j = 0; j < H; ++j) {
            const float da = chain(D, [&](int n, float p) { return fmaf(dy[i * D + n], W2[(int64_t)n * H + j], p); });
            dz[i * H + j] = m1(i, j, da) * gelu_grad<float>(z[i * H + j]);
            av[i * H + j] = m1(i, j, gelu<float>(z[i * H + j]));
        }
        // dx
        std::vector<float> dxn((size_t)D);
        for (int k = 0; k < D; ++k) dxn[k] = chain(H, [&](int j, float p) { return fmaf(dz[i * H + j], W1[(int64_t)j * D + k], p); });
        const int NB = (D + 63) / 64;
        float T[2];
        for (int cw = 0; cw < 2; ++cw) {
            float v[32], w[32];
            for (int c = 0; c < 32; ++c) {
                float p = 0.0f;
                for (int b = 0; b < NB; ++b) {
                    const int col = (cw + 2 * b) * 32 + c;
                    p = col < D ? fmaf(dxn[col], xn[i * D + col], p) : fmaf(0.0f, 0.0f, p);
                }
                v[c] = p;
            }
            for (int st = 1; st < 32; st <<= 1) {
                for (int c = 0; c < 32; ++c) w[c] = v[c] + v[c ^ st];
                for (int c = 0; c < 32; ++c) v[c] = w[c];
            }
            T[cw] = v[0];
        }
        const float t = T[0] + T[1];
        float* dt = dx + off(i, ds0, ds1);
        for (int k = 0; k < D; ++k) dt[k] = dx_of(gt[k], rs[i], dxn[k], xn[i * D + k], t, D);
    }
    // the sums over tokens: per chunk a plane, the planes added in ascending order starting from plane 0
    const int64_t nch = (ntok + FFN_BWD_ROWS - 1) / FFN_BWD_ROWS;
    // C[m][n] = sum_i A[i][m] B[i][n] into out [Md][Nd]
    auto colgemm = [&](const float* A, int Md, const float* B, int Nd, float* out) {
#pragma omp parallel for schedule(static)
        for (int m = 0; m < Md; ++m) {
            std::vector<float> acc((size_t)Nd), part((size_t)Nd);
            for (int64_t ch = 0; ch < nch; ++ch) {
                const int64_t r0 = ch * FFN_BWD_ROWS, r1 = std::min(ntok, r0 + FFN_BWD_ROWS);
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int64_t s0 = r0; s0 < r1; s0 += FFN_BWD_RSUB) {
                    const int64_t s1 = std::min(r1, s0 + FFN_BWD_RSUB);
                    std::fill(part.begin(), part.end(), 0.0f);
                    for (int64_t i = s0; i < s1; ++i) {
                        const float a = A[i * Md + m];
                        const float* b = B + i * Nd;
                        for (int n = 0; n < Nd; ++n) part[n] = fmaf(a, b[n], part[n]);
                    }
                    const bool pad = (s1 - r0) % FFN_BWD_RSTEP != 0;
                    for (int n = 0; n < Nd; ++n) acc[n] += pad ? fmaf(0.0f, 0.0f, part[n]) : part[n];
                }
                float* o = out + (int64_t)m * Nd;
                if (ch == 0) for (int n = 0; n < Nd; ++n) o[n] = acc[n];
                else for (int n = 0; n < Nd; ++n) o[n] += acc[n];
            }
        }
    };
    colgemm(dy.data(), D, av.data(), H, dW2);
    colgemm(dz.data(), H, xn.data(), D, dW1);
    auto colsum = [&](int ncol, float* out, auto value) {
#pragma omp parallel for schedule(static)
        for (int c = 0; c < ncol; ++c) {
            float total = 0.0f;
            for (int64_t ch = 0; ch < nch; ++ch) {
                const int64_t r0 = ch * FFN_BWD_ROWS, r1 = std::min(ntok, r0 + FFN_BWD_ROWS);
                double sub[FFN_BWD_SUBSUMS];
                for (int q = 0; q < FFN_BWD_SUBSUMS; ++q) {
                    double t = 0.0;
                    for (int64_t i = r0 + q; i < r1; i += FFN_BWD_SUBSUMS) t += (double)value(i, c);
                    sub[q] = t;
                }
                double s = sub[0];
                for (int q = 1; q < FFN_BWD_SUBSUMS; ++q) s += sub[q];
                total = ch == 0 ? (float)s : total + (float)s;
            }
            out[c] = total;
        }
    };
    colsum(H, db1, [&](int64_t i, int j) { return dz[i * H + j]; });
    colsum(D, db2, [&](int64_t i, int n) { return dy[i * D + n]; });
    colsum(D, dscale, [&](int64_t i, int n) { return dout[off(i, gs0, gs1) + n] * m2(i, n, y[i * D + n]); });
}

// ---- the bf16 feed-forward ResBlock (semicrf_ffn_residual_bf16, semicrf_ffn_residual_bf16_mixed) ----------------------------------------
// The chain of ffn_bf16_math.h per output element, T = uint16_t (bf16 tensors) or float (fp32 tensors, bf16 operands): the products of
// two bf16 values are exact in fp32, so each fmaf below is the exact product added with one rounding; both sums ascend one term at a
// time where the device adds 16 products per matrix instruction.  Only that and erf / erfc differ from the device's.
template <typename T>
static void ffn_residual_bf16_any(const T* x, T* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                                  const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps)
{
    using namespace semicrf::ffn;
    const int64_t ntok = n0 * n1;
    std::vector<float> w1h((size_t)H * D), w2h((size_t)D * H);           // the operands as fp32 values, rounded once per call
    for (size_t i = 0; i < w1h.size(); ++i) w1h[i] = bf16_to_float(operand_of(W1[i]));
    for (size_t i = 0; i < w2h.size(); ++i) w2h[i] = bf16_to_float(operand_of(W2[i]));
#pragma omp parallel
    {
        std::vector<float> xh((size_t)D), gh((size_t)H);
#pragma omp for schedule(static)
        for (int64_t t = 0; t < ntok; ++t) {
            const int64_t i0 = t / n1, i1 = t % n1;
            const T* xt = x + i0 * xs0 + i1 * xs1;
            T* ot = out + i0 * os0 + i1 * os1;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < D; ++k) s[k & 3] = fmaf(to_f32(xt[k]), to_f32(xt[k]), s[k & 3]);
            const float rs = rs_of(sumsq_combine(s[0], s[1], s[2], s[3]), D, eps);
            for (int k = 0; k < D; ++k) xh[k] = bf16_to_float(bf16_rne(to_f32(xt[k]) * rs));
            for (int j = 0; j < H; ++j) {
                const float* w = w1h.data() + (size_t)j * D;
                float h = 0.0f;
                for (int k = 0; k < D; ++k) h = fmaf(xh[k], w[k], h);
                gh[j] = bf16_to_float(bf16_rne(semicrf::attr_heads::gelu<float>(h + to_f32(b1[j]))));
            }
            for (int n = 0; n < D; ++n) {
                const float* w = w2h.data() + (size_t)n * H;
                float a = 0.0f;                              // one running accumulator over all of hidden
                for (int j = 0; j < H; ++j) a = fmaf(gh[j], w[j], a);
                store_as(ot + n, epilogue(to_f32(xt[n]), a, to_f32(b2[n]), to_f32(scale[n])));
            }
        }
    }
}
void ffn_residual_bf16(const uint16_t* x, uint16_t* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                       const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale, float eps)
{
    ffn_residual_bf16_any<uint16_t>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps);
}
void ffn_residual_bf16_mixed(const float* x, float* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D, int H,
                             const float* W1, const float* b1, const float* W2, const float* b2, const float* scale, float eps)
{
    ffn_residual_bf16_any<float>(x, out, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps);
}

// ---- the bf16 block in training (semicrf_ffn_residual_bf16_train_fwd / _bwd and their _mixed forms) -------------------------------------
// The chain of ffn_bf16_train_math.h, one product at a time in ascending order; `saved` is laid out as the header says.
template <typename T>
static void ffn_residual_bf16_train_fwd_any(const T* x, T* out, void* saved, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                                            int64_t os1, int D, int H, const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, float eps,
                                            uint64_t seed, double p1, double p2)
{
    using namespace semicrf::ffn;
    const DropoutParams drop = semicrf::attr_heads::dropout_params(seed, p1, p2);
    const int64_t ntok = n0 * n1;
    uint16_t* const zs = (uint16_t*)saved;
    T* const ys = (T*)((unsigned char*)saved + train_saved_ys_offset(ntok, H));
    auto mk = [&](int stream, int64_t i, int j, float v) { return keep(drop, stream, i, j) ? (drop.on[stream] ? v * drop.scale[stream] : v) : 0.0f; };
    std::vector<float> w1h((size_t)H * D), w2h((size_t)D * H);
    for (size_t i = 0; i < w1h.size(); ++i) w1h[i] = bf16_to_float(operand_of(W1[i]));
    for (size_t i = 0; i < w2h.size(); ++i) w2h[i] = bf16_to_float(operand_of(W2[i]));
#pragma omp parallel
    {
        std::vector<float> xh((size_t)D), ah((size_t)H);
#pragma omp for schedule(static)
        for (int64_t t = 0; t < ntok; ++t) {
            const int64_t i0 = t / n1, i1 = t % n1;
            const T* xt = x + i0 * xs0 + i1 * xs1;
            T* ot = out + i0 * os0 + i1 * os1;
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < D; ++k) s[k & 3] = fmaf(to_f32(xt[k]), to_f32(xt[k]), s[k & 3]);
            const float rs = rs_of(sumsq_combine(s[0], s[1], s[2], s[3]), D, eps);
            for (int k = 0; k < D; ++k) xh[k] = bf16_to_float(bf16_rne(to_f32(xt[k]) * rs));
            for (int j = 0; j < H; ++j) {
                const float* w = w1h.data() + (size_t)j * D;
                float h = 0.0f;
                for (int k = 0; k < D; ++k) h = fmaf(xh[k], w[k], h);
                h += to_f32(b1[j]);
                zs[t * H + j] = bf16_rne(h);
                ah[j] = bf16_to_float(bf16_rne(mk(0, t, j, semicrf::attr_heads::gelu<float>(h))));
            }
            for (int n = 0; n < D; ++n) {
                const float* w = w2h.data() + (size_t)n * H;
                float a = 0.0f;
                for (int j = 0; j < H; ++j) a = fmaf(ah[j], w[j], a);
                const float y = a + to_f32(b2[n]);
                store_as(ys + t * D + n, y);
                store_as(ot + n, to_f32(xt[n]) + mk(1, t, n, y) * to_f32(scale[n]));
            }
        }
    }
}

template <typename T>
static void ffn_residual_bf16_bwd_any(const T* dout, const T* x, const void* saved, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1, int64_t xs0,
                                      int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const T* W1, const T* W2, const T* scale, float eps,
                                      uint64_t seed, double p1, double p2, T* dx, T* dW1, T* db1, T* dW2, T* db2, T* dscale)
{
    using namespace semicrf::ffn;
    using semicrf::attr_heads::gelu;
    using semicrf::attr_heads::gelu_grad;
    const DropoutParams drop = semicrf::attr_heads::dropout_params(seed, p1, p2);
    const int64_t ntok = n0 * n1;
    const uint16_t* const zs = (const uint16_t*)saved;
    const T* const ys = (const T*)((const unsigned char*)saved + train_saved_ys_offset(ntok, H));
    auto off = [&](int64_t i, int64_t s0, int64_t s1) { return (i / n1) * s0 + (i % n1) * s1; };
    auto mk = [&](int stream, int64_t i, int j, float v) { return keep(drop, stream, i, j) ? (drop.on[stream] ? v * drop.scale[stream] : v) : 0.0f; };
    auto r16 = [](float v) { return bf16_to_float(bf16_rne(v)); };
    std::vector<float> w1h((size_t)H * D), w2t((size_t)H * D);           // Wh1 [H][D]; Wh2 transposed [H][D]
    for (int j = 0; j < H; ++j)
        for (int k = 0; k < D; ++k) {
            w1h[(size_t)j * D + k] = bf16_to_float(operand_of(W1[(size_t)j * D + k]));
            w2t[(size_t)j * D + k] = bf16_to_float(operand_of(W2[(size_t)k * H + j]));
        }
    std::vector<float> dyf((size_t)ntok * D), dyh((size_t)ntok * D), xh((size_t)ntok * D), dzh((size_t)ntok * H), ah((size_t)ntok * H);
#pragma omp parallel
    {
        std::vector<float> xn((size_t)D), dxn((size_t)D);
#pragma omp for schedule(static)
        for (int64_t i = 0; i < ntok; ++i) {
            const T* xt = x + off(i, xs0, xs1);
            const T* gt = dout + off(i, gs0, gs1);
            float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < D; ++k) s[k & 3] = fmaf(to_f32(xt[k]), to_f32(xt[k]), s[k & 3]);
            const float rs = rs_of(sumsq_combine(s[0], s[1], s[2], s[3]), D, eps);
            for (int k = 0; k < D; ++k) {
                xn[k] = to_f32(xt[k]) * rs;
                xh[i * D + k] = r16(xn[k]);
                dyf[i * D + k] = mk(1, i, k, to_f32(gt[k]) * to_f32(scale[k]));
                dyh[i * D + k] = r16(dyf[i * D + k]);
            }
            for (int j = 0; j < H; ++j) {
                const float* w = w2t.data() + (size_t)j * D;
                float da = 0.0f;
                for (int n = 0; n < D; ++n) da = fmaf(dyh[i * D + n], w[n], da);
                const float zf = bf16_to_float(zs[i * H + j]);
                dzh[i * H + j] = r16(mk(0, i, j, da) * gelu_grad<float>(zf));
                ah[i * H + j] = r16(mk(0, i, j, gelu<float>(zf)));
            }
            std::fill(dxn.begin(), dxn.end(), 0.0f);
            for (int j = 0; j < H; ++j) {                    // every dxn[k] is its own chain over j ascending
                const float d = dzh[i * H + j];
                const float* w = w1h.data() + (size_t)j * D;
                for (int k = 0; k < D; ++k) dxn[k] = fmaf(d, w[k], dxn[k]);
            }
            float P[2][2] = {{0.0f, 0.0f}, {0.0f, 0.0f}};
            for (int k = 0; k < D; ++k) P[(k >> 5) & 1][(k >> 2) & 1] = fmaf(dxn[k], xn[k], P[(k >> 5) & 1][(k >> 2) & 1]);
            const float t = (P[0][0] + P[0][1]) + (P[1][0] + P[1][1]);
            T* dt = dx + off(i, ds0, ds1);
            for (int k = 0; k < D; ++k) store_as(dt + k, dx_of(to_f32(gt[k]), rs, dxn[k], xn[k], t, D));
        }
    }
    // the sums over tokens: per chunk a plane from +0 with the tokens ascending, the planes added in ascending order, one rounding to T
    const int64_t nch = (ntok + FFN_BWD_ROWS - 1) / FFN_BWD_ROWS;
    auto colgemm = [&](const float* A, int Md, const float* B, int Nd, T* o) {
#pragma omp parallel for schedule(static)
        for (int m = 0; m < Md; ++m) {
            std::vector<float> acc((size_t)Nd), total((size_t)Nd);
            for (int64_t ch = 0; ch < nch; ++ch) {
                const int64_t r0 = ch * FFN_BWD_ROWS, r1 = std::min(ntok, r0 + FFN_BWD_ROWS);
                std::fill(acc.begin(), acc.end(), 0.0f);
                for (int64_t i = r0; i < r1; ++i) {
                    const float a = A[i * Md + m];
                    const float* b = B + i * Nd;
                    for (int n = 0; n < Nd; ++n) acc[n] = fmaf(a, b[n], acc[n]);
                }
                if (ch == 0) total = acc;
                else for (int n = 0; n < Nd; ++n) total[n] += acc[n];
            }
            for (int n = 0; n < Nd; ++n) store_as(o + (int64_t)m * Nd + n, total[n]);
        }
    };
    colgemm(dyh.data(), D, ah.data(), H, dW2);
    colgemm(dzh.data(), H, xh.data(), D, dW1);
    auto colsum = [&](int ncol, T* o, auto value) {
#pragma omp parallel for schedule(static)
        for (int c = 0; c < ncol; ++c) {
            float total = 0.0f;
            for (int64_t ch = 0; ch < nch; ++ch) {
                const int64_t r0 = ch * FFN_BWD_ROWS, r1 = std::min(ntok, r0 + FFN_BWD_ROWS);
                double sub[FFN_BWD_SUBSUMS];
                for (int q = 0; q < FFN_BWD_SUBSUMS; ++q) {
                    double t = 0.0;
                    for (int64_t i = r0 + q; i < r1; i += FFN_BWD_SUBSUMS) t += (double)value(i, c);
                    sub[q] = t;
                }
                double sacc = sub[0];
                for (int q = 1; q < FFN_BWD_SUBSUMS; ++q) sacc += sub[q];
                total = ch == 0 ? (float)sacc : total + (float)sacc;
            }
            store_as(o + c, total);
        }
    };
    colsum(H, db1, [&](int64_t i, int j) { return dzh[i * H + j]; });
    colsum(D, db2, [&](int64_t i, int n) { return dyf[i * D + n]; });
    colsum(D, dscale, [&](int64_t i, int n) { return to_f32(dout[off(i, gs0, gs1) + n]) * mk(1, i, n, to_f32(ys[i * D + n])); });
}

void ffn_residual_bf16_train_fwd(const uint16_t* x, uint16_t* out, void* saved, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                                 int64_t os1, int D, int H, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2, const uint16_t* b2,
                                 const uint16_t* scale, float eps, uint64_t seed, double p1, double p2)
{
    ffn_residual_bf16_train_fwd_any<uint16_t>(x, out, saved, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, seed, p1, p2);
}
void ffn_residual_bf16_mixed_train_fwd(const float* x, float* out, void* saved, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0,
                                       int64_t os1, int D, int H, const float* W1, const float* b1, const float* W2, const float* b2,
                                       const float* scale, float eps, uint64_t seed, double p1, double p2)
{
    ffn_residual_bf16_train_fwd_any<float>(x, out, saved, n0, n1, xs0, xs1, os0, os1, D, H, W1, b1, W2, b2, scale, eps, seed, p1, p2);
}
void ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1, int64_t xs0,
                           int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const uint16_t* W1, const uint16_t* W2, const uint16_t* scale,
                           float eps, uint64_t seed, double p1, double p2, uint16_t* dx, uint16_t* dW1, uint16_t* db1, uint16_t* dW2, uint16_t* db2,
                           uint16_t* dscale)
{
    ffn_residual_bf16_bwd_any<uint16_t>(dout, x, saved, n0, n1, gs0, gs1, xs0, xs1, ds0, ds1, D, H, W1, W2, scale, eps, seed, p1, p2, dx, dW1, db1,
                                        dW2, db2, dscale);
}
void ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, int64_t n0, int64_t n1, int64_t gs0, int64_t gs1, int64_t xs0,
                                 int64_t xs1, int64_t ds0, int64_t ds1, int D, int H, const float* W1, const float* W2, const float* scale, float eps,
                                 uint64_t seed, double p1, double p2, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale)
{
    ffn_residual_bf16_bwd_any<float>(dout, x, saved, n0, n1, gs0, gs1, xs0, xs1, ds0, ds1, D, H, W1, W2, scale, eps, seed, p1, p2, dx, dW1, db1, dW2,
                                     db2, dscale);
}

// ---- the audio front end (semicrf_log_mel) -------------------------------------------------------------------------------------------
// The order of operations of logmel.hip per output element, in fp32 (logmel_math.h): gain and window, the half-length radix-2 transform
// in place (decimation in frequency, one stage at a time: the device's three stages per step visit the same pairs), the split pass, the
// power, the channel mean, the band chains, the log compression.  Nothing differs from the device's arithmetic.
void log_mel(const float* frames, int64_t sn, int64_t sc, int64_t sf, int N, int C, int nFrame, int W, const float* windows, int nWin,
             const float* tw, const int32_t* fb_start, const int32_t* fb_len, const int32_t* fb_off, const float* fb_val, int nMel, int total,
             const float* shift, const float* denom, int log_flag, float eps, int to_mono, float* out)
{
    using namespace semicrf::logmel;
    const int M = W / 2, P = log2_of_window(W) - 1;
    const bool gain = shift != nullptr;
    const float inv_w = 1.0f / (float)W, fC = (float)C, le = (float)std::log((double)eps);
    auto twc = [tw](int k) { cf w; w.re = tw[2 * k]; w.im = tw[2 * k + 1]; return w; };
    const int64_t row = (int64_t)nMel * nWin, nf = (int64_t)N * nFrame;
    const int Cout = to_mono ? 1 : C;
#pragma omp parallel
    {
        std::vector<cf> Z((size_t)M);
        std::vector<float> PW((size_t)M + 1);
        auto spectrum = [&](const float* x, const float* win, float sh, float dn, bool first, bool last) {
            for (int i = 0; i < M; ++i) {
                Z[i].re = lm_sample(x[2 * i], gain, sh, dn, win[2 * i]);
                Z[i].im = lm_sample(x[2 * i + 1], gain, sh, dn, win[2 * i + 1]);
            }
            for (int b = P - 1; b >= 0; --b) {
                const int h = 1 << b, step = P - b;
                for (int i = 0; i < M; ++i)
                    if (!(i & h)) lm_butterfly(Z[i], Z[i + h], twc((i & (h - 1)) << step));
            }
            for (int k = 0; k <= M; ++k) {
                cf v;
                if (k == 0 || k == M) {
                    v.re = k == 0 ? Z[0].re + Z[0].im : Z[0].re - Z[0].im;
                    v.im = 0.0f;
                } else {
                    v = lm_split(Z[lm_brev(k, P)], Z[lm_brev(M - k, P)], twc(k));
                }
                float p = lm_power(v, inv_w);
                if (!first) p = PW[k] + p;
                if (last) p = p / fC;
                PW[k] = p;
            }
        };
        auto bands = [&](int w, float* o) {
            for (int m = 0; m < nMel; ++m) {
                int s, len;
                const int off = fb_off[m];
                lm_band(fb_start[m], fb_len[m], off, M, total, s, len);
                float acc = 0.0f;
                for (int r = 0; r < len; ++r) acc = fmaf(PW[s + r], fb_val[off + r], acc);
                o[(int64_t)m * nWin + w] = log_flag ? lm_compress(acc, eps, le) : acc;
            }
        };
#pragma omp for schedule(static)
        for (int64_t f = 0; f < nf; ++f) {
            const int n = (int)(f / nFrame), t = (int)(f % nFrame);
            const float sh = gain ? shift[n] : 0.0f, dn = gain ? denom[n] : 1.0f;
            const float* xn = frames + n * sn + t * sf;
            if (to_mono) {
                float* o = out + ((int64_t)n * nFrame + t) * row;
                for (int w = 0; w < nWin; ++w) {
                    for (int c = 0; c < C; ++c) spectrum(xn + c * sc, windows + (int64_t)w * W, sh, dn, c == 0, c == C - 1);
                    bands(w, o);
                }
            } else {
                for (int c = 0; c < C; ++c) {
                    float* o = out + (((int64_t)n * Cout + c) * nFrame + t) * row;
                    for (int w = 0; w < nWin; ++w) {
                        spectrum(xn + c * sc, windows + (int64_t)w * W, sh, dn, true, false);
                        bands(w, o);
                    }
                }
            }
        }
    }
}

}  // namespace semicrf_cpu
