// expectation.hip -- posterior expectations of additive path functionals and their covariances with the cells of the lattice
// (include/semicrf_hip.h: semicrf_expectation, semicrf_covariance): the first-order expectation semiring on the semi-CRF lattice.
//
// For W(path) = sum of weight[e,b] over the intervals of the path + sum of noiseWeight[t] over its noise gaps:
//   E = E_p[W],  C[e,b] = Cov(1[(b,e) on path], W) = dE / dscore[e,b] = (Hessian of logZ) . (weight, noiseWeight).
// Per frame t, with P the transition probabilities of alpha's / beta's recursion:
//   a[t]    = E[W of the prefix up to node t, its singleton included | t is a node]
//           = sum_pred P(pred -> t) (a[pred] + w_pred) + sigma(s[t,t]) w[t,t]
//   binc[t] = E[W of the suffix from node t on, its singleton included | t is a node]
//           = sum_succ P(t -> succ) (w_succ + binc[succ]) + sigma(s[t,t]) w[t,t]
// and then every covariance is mu(cell) * (E[W | cell on path] - E), one elementwise pass.
//
// PRECISION.  An fp32 alpha of magnitude ~1e3 has an ulp of 6e-5, so every transition probability formed from it carries a 1e-4
// relative error; that error multiplies conditional expectations of size T |w| which then cancel against E: fp32 state gives
// covariances good to 1e-2 only.  The per-frame state here (the log-sums v64 / q64 and a / binc) is therefore float64 and is
// computed by these sweeps themselves; the fp32 v / q of semicrf_logz_fwd / semicrf_beta serve only as the SHIFT of each row's
// sum (known up front, accurate to 1e-4: no running maximum, partial sums are plainly additive).  The per-cell exponential stays
// fp32 on an argument formed in float64: float(v64[b] - shift[e] + s).
//
// Kernels:
//   expectation_sweep_kernel  one workgroup (4 waves) owns 16 chains and walks the frames in order; blockIdx.y = 0 walks the rows
//                             forward (v64, a), 1 walks the columns backward (q64, binc): both directions run side by side.
//                             Lane = (chain, predecessor slot of 16); the 16 slots of a chain are summed by shuffles (4 per wave)
//                             and through LDS in wave order; every thread of the chain then holds the frame's state, the next
//                             frame takes it from registers and older frames from memory (written two barriers earlier).
//   covariance_stream_kernel  one thread per cell of the dense [T][T][B] output, rows in grid.y: C for b <= e, exact zeros above.
//   covariance_noise_kernel   Cn, one thread per (gap, chain).
// No atomics, fixed summation order: two calls are bit-identical.
#include "common.h"
#include "launchers.h"

namespace semicrf {

namespace {
constexpr int ECH = 16;                     // chains per workgroup (64 bytes of every cell)
constexpr int ESL = 16;                     // predecessor slots per chain
constexpr int EWAVES = ECH * ESL / 64;

__device__ __forceinline__ double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double sigmoid_d(double x) { return x > 20.0 ? 1.0 : 1.0 / (1.0 + exp(-x)); }   // d softplus_d / dx

struct ExpState {                           // the workspace: float64 [T][B] each, then [B] each
    double *v64, *a, *q64, *binc, *E64, *lz64;
};
__host__ __device__ inline size_t state_bytes(int T, int B) { return (size_t)T * B * sizeof(double); }
inline ExpState carve(void* ws, int T, int B)
{
    char* w = (char*)ws;
    const size_t tb = align_up(state_bytes(T, B)), b = align_up((size_t)B * sizeof(double));
    ExpState s;
    s.v64 = (double*)w; s.a = (double*)(w + tb); s.q64 = (double*)(w + 2 * tb); s.binc = (double*)(w + 3 * tb);
    s.E64 = (double*)(w + 4 * tb); s.lz64 = (double*)(w + 4 * tb + b);
    return s;
}

// One direction of the sweep for the chains cbase .. cbase + 15.  FWD: frame t = k, predecessors are the frames before it, the
// cell of (t, p) is s[t][p]; else t = T-1-k, the "predecessors" are the frames after it and the cell is s[p][t].
// L / X: the float64 log-sum and conditional expectation of every frame ([T][B]), shift: the fp32 v (FWD) or q.
template <bool FWD>
__device__ __forceinline__ void sweep(const float* __restrict__ score, const float* __restrict__ noise,
                                      const float* __restrict__ weight, const float* __restrict__ nweight,
                                      const float* __restrict__ shift, int T, int B, int cbase, double* L, double* X,
                                      double (*s_z)[EWAVES][ECH], double (*s_a)[EWAVES][ECH], double& Lout, double& Xout)
{
    const int tid = (int)threadIdx.x, cc = tid & (ECH - 1), slot = tid / ECH, wave = tid >> 6, lane = tid & 63;
    const int c = cbase + cc;
    const bool valid = c < B, same = weight == score;
    const size_t Bs = (size_t)B;
    double Lp = 0.0, Xp = 0.0;              // the previous frame's state (every thread of the chain holds it)
    // the frame's own diagonal score / weight and shift are loaded one frame ahead: off the dependent chain
    float d_nx = 0.0f, wd_nx = 0.0f, sh_nx = 0.0f;
    if (valid) {
        const int t0 = FWD ? 0 : T - 1;
        const size_t dc = ((size_t)t0 * T + t0) * Bs + c;
        d_nx = score[dc];
        wd_nx = same ? d_nx : weight[dc];
        sh_nx = shift[(size_t)t0 * Bs + c];
    }
    for (int k = 0; k < T; ++k) {
        const int t = FWD ? k : T - 1 - k;
        const float d = d_nx, wd = wd_nx;
        const float rf = sh_nx - softplus_f(d);
        const double Rf = isfinite(rf) ? (double)rf : 0.0;
        double Z = 0.0, A = 0.0;
        if (valid) {
            if (k + 1 < T) {
                const int tn = FWD ? t + 1 : t - 1;
                const size_t dc = ((size_t)tn * T + tn) * Bs + c;
                d_nx = score[dc];
                wd_nx = same ? d_nx : weight[dc];
                sh_nx = shift[(size_t)tn * Bs + c];
            }
            if (k > 0) {
#pragma unroll 4
                for (int j = slot; j < k - 1; j += ESL) {               // frames written at least two barriers ago
                    const int p = FWD ? j : T - 1 - j;
                    const size_t cell = (FWD ? (size_t)t * T + p : (size_t)p * T + t) * Bs + c;
                    const float x = score[cell];
                    const float wv = same ? x : weight[cell];
                    const size_t pc = (size_t)p * Bs + c;
                    const float ex = __expf((float)(L[pc] - Rf + (double)x));
                    Z += (double)ex;
                    A += (double)ex * (X[pc] + (double)wv);
                }
                if (slot == ESL - 1) {                                  // the neighbouring frame: its interval cell and the skip
                    const int p = FWD ? t - 1 : t + 1;
                    const size_t cell = (FWD ? (size_t)t * T + p : (size_t)p * T + t) * Bs + c;
                    const float x = score[cell];
                    const float wv = same ? x : weight[cell];
                    float ex = __expf((float)(Lp - Rf + (double)x));
                    Z += (double)ex;
                    A += (double)ex * (Xp + (double)wv);
                    const size_t gc = (size_t)(FWD ? t - 1 : t) * Bs + c;
                    const float nz = noise[gc];
                    const float wn = nweight ? nweight[gc] : 0.0f;
                    ex = __expf((float)(Lp - Rf + (double)nz));
                    Z += (double)ex;
                    A += (double)ex * (Xp + (double)wn);
                }
            }
        }
        const double spd = softplus_d((double)d), sw = sigmoid_d((double)d) * (double)wd;      // (before the barrier: not on the chain)
        // the 16 slots of a chain: 4 inside the wave (lanes cc, cc + 16, cc + 32, cc + 48), then the 4 waves in order
        Z += __shfl_xor(Z, 16); A += __shfl_xor(A, 16);
        Z += __shfl_xor(Z, 32); A += __shfl_xor(A, 32);
        const int buf = k & 1;              // two buffers: one barrier per frame
        if (lane < ECH) { s_z[buf][wave][cc] = Z; s_a[buf][wave][cc] = A; }
        __syncthreads();
        Z = ((s_z[buf][0][cc] + s_z[buf][1][cc]) + s_z[buf][2][cc]) + s_z[buf][3][cc];
        A = ((s_a[buf][0][cc] + s_a[buf][1][cc]) + s_a[buf][2][cc]) + s_a[buf][3][cc];
        double Lt = spd, Xt = sw;
        if (k > 0) {
            Lt += Rf + log(Z);
            Xt += Z > 0.0 ? A / Z : 0.0;
        }
        if (valid && slot == 0) { L[(size_t)t * Bs + c] = Lt; X[(size_t)t * Bs + c] = Xt; }
        Lp = Lt; Xp = Xt;
    }
    Lout = Lp; Xout = Xp;
}
static_assert(EWAVES == 4, "the reduction above is written for 4 waves");

}  // namespace

// grid (ceil(B/16), 2), block 256
__global__ __launch_bounds__(64 * EWAVES) void expectation_sweep_kernel(const float* __restrict__ score, const float* __restrict__ noise,
                                                                        const float* __restrict__ weight,
                                                                        const float* __restrict__ nweight, const float* __restrict__ v,
                                                                        const float* __restrict__ q, int T, int B, double* v64, double* a,
                                                                        double* q64, double* binc, double* E64, double* lz64,
                                                                        float* __restrict__ E, float* __restrict__ H)
{
    __shared__ double s_z[2][EWAVES][ECH];
    __shared__ double s_a[2][EWAVES][ECH];
    const int cbase = (int)blockIdx.x * ECH;
    double Lf, Xf;
    if (blockIdx.y == 0) {
        sweep<true>(score, noise, weight, nweight, v, T, B, cbase, v64, a, s_z, s_a, Lf, Xf);
        const int c = cbase + ((int)threadIdx.x & (ECH - 1));
        if (c < B && (int)threadIdx.x < ECH) {
            E64[c] = Xf;
            lz64[c] = Lf;
            E[c] = (float)Xf;
            H[c] = (float)(Lf - Xf);
        }
    } else {
        sweep<false>(score, noise, weight, nweight, q, T, B, cbase, q64, binc, s_z, s_a, Lf, Xf);
    }
}

// grid (ceil(T B / 256), T), block 256: row e = blockIdx.y, element i = b * B + c of the row.
__global__ __launch_bounds__(256) void covariance_stream_kernel(const float* __restrict__ score, const float* __restrict__ weight,
                                                                const float* __restrict__ gout, int T, int B,
                                                                const double* __restrict__ v64, const double* __restrict__ a,
                                                                const double* __restrict__ q64, const double* __restrict__ binc,
                                                                const double* __restrict__ E64, const double* __restrict__ lz64,
                                                                float* __restrict__ C)
{
    const int e = (int)blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, Bs = (size_t)B;
    if (i >= (size_t)T * Bs) return;
    const int b = (int)(i / Bs), c = (int)(i - (size_t)b * Bs);
    const size_t cell = (size_t)e * T * Bs + i;
    float out = 0.0f;                                                   // b > e: never on a path
    if (b <= e) {
        const size_t ec = (size_t)e * Bs + c;
        const float s = score[cell];
        const double w = weight == score ? s : weight[cell];
        const double lz = lz64[c], Ex = E64[c];
        double val;
        if (b < e) {
            const float mu = __expf((float)(v64[i] + (double)s + q64[ec] - lz));
            val = (double)mu * (a[i] + w + binc[ec] - Ex);
        } else {                                                        // the singleton: P = node sigma(d), given weight w[t,t]
            const double sp = softplus_d((double)s), sg = sigmoid_d((double)s);
            const float mu = __expf((float)(v64[ec] + q64[ec] - 2.0 * sp + (double)s - lz));
            val = (double)mu * (a[ec] + binc[ec] + (1.0 - 2.0 * sg) * w - Ex);
        }
        out = (float)(val * (double)gout[c]);
    }
    C[cell] = out;
}

__global__ __launch_bounds__(256) void covariance_noise_kernel(const float* __restrict__ noise, const float* __restrict__ nweight,
                                                               const float* __restrict__ gout, int T, int B,
                                                               const double* __restrict__ v64, const double* __restrict__ a,
                                                               const double* __restrict__ q64, const double* __restrict__ binc,
                                                               const double* __restrict__ E64, const double* __restrict__ lz64,
                                                               float* __restrict__ Cn)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, Bs = (size_t)B;
    if (i >= (size_t)(T - 1) * Bs) return;
    const int c = (int)(i % Bs);
    const double wn = nweight ? (double)nweight[i] : 0.0;
    const float mu = __expf((float)(v64[i] + (double)noise[i] + q64[i + Bs] - lz64[c]));
    Cn[i] = (float)((double)mu * (a[i] + wn + binc[i + Bs] - E64[c]) * (double)gout[c]);
}

size_t expectation_workspace_bytes(int T, int B)
{
    return 4 * align_up(state_bytes(T, B)) + 2 * align_up((size_t)B * sizeof(double));
}

void launch_expectation(const float* score, const float* noise, const float* weight, const float* nweight, const float* v, const float* q,
                        int T, int B, float* E, float* H, void* ws, hipStream_t stream)
{
    const ExpState s = carve(ws, T, B);
    expectation_sweep_kernel<<<dim3((B + ECH - 1) / ECH, 2), 64 * EWAVES, 0, stream>>>(score, noise, weight, nweight, v, q, T, B, s.v64, s.a,
                                                                                      s.q64, s.binc, s.E64, s.lz64, E, H);
}

void launch_covariance(const float* score, const float* noise, const float* weight, const float* nweight, const float* gout, int T, int B,
                       float* C, float* Cn, const void* ws, hipStream_t stream)
{
    const ExpState s = carve((void*)ws, T, B);
    const size_t row = (size_t)T * B;
    covariance_stream_kernel<<<dim3((unsigned)((row + 255) / 256), T), 256, 0, stream>>>(score, weight, gout, T, B, s.v64, s.a, s.q64, s.binc,
                                                                                        s.E64, s.lz64, C);
    if (T > 1) {
        const size_t n = (size_t)(T - 1) * B;
        covariance_noise_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(noise, nweight, gout, T, B, s.v64, s.a, s.q64, s.binc, s.E64,
                                                                                s.lz64, Cn);
    }
}

}  // namespace semicrf
