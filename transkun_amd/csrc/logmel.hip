// logmel.hip -- the audio front end (Util.py:78-170 behind ModelTransformer.py:159-164) as ONE launch: gain, the analysis windows, the
// real transform of every window, the power spectrum, the channel mean, the mel bands and the log compression; logmel_math.h gives the
// order of operations.  No workspace, no atomics: neither the windowed frames nor a spectrum ever exist in memory, and the overlapping
// frames are read where they lie.
//
// A workgroup owns one (recording, frame) and walks its channels and windows; NT = max(64, W / 16) threads.  LDS:
//   Z  [M + M / 8] complex     the half-length transform in place (M = W / 2), element i at i + (i >> 3)
//   TW [M + M / 8] complex     the caller's twiddles, padded likewise
//   PW [M + 1]                 the power spectrum of the window at hand (the channel sum when mixing down)
//   O  [nMel nWin]             a frame's features as they go to memory, the window index minor (dynamic)
// 44.3 KB + O at W = 4096: three workgroups per CU.
// The transform takes three radix-2 stages at a time on eight elements in registers (the last step takes the one or two stages left),
// from the widest span down, so Z is read and written P / 3 times, not P times; the first step takes its elements from memory through
// the gain and the window.  Stage bits s0 .. s0 + 2: a thread's eight elements lie 2^s0 apart.  Banks (8-byte reads, bank = dword
// address mod 64 per half wave): with the padding a half wave's 32 reads of one step touch 0, 18, 36, .. (s0 = 0), or 2 l + 2 (l >> 3)
// (top step): no conflict but for two lanes of the top step that wrap; twiddle reads are 2-way at worst.  The split pass reads Z in
// bit-reversed order (8-way, one pass in P / 3 + 2).
#include "common.h"
#include "launchers.h"
#include "logmel_math.h"

namespace semicrf {

using namespace logmel;

__device__ __forceinline__ int lm_pad(int i) { return i + (i >> 3); }

struct LogMelArgs {
    const float* frames;
    long long sn, sc, sf;
    int N, C, nFrame, nWin, nMel, total;
    const float *windows, *tw;
    const int *fb_start, *fb_len, *fb_off;
    const float* fb_val;
    const float *shift, *denom;
    int log_flag, to_mono;
    float eps, le;
    float* out;
};

// S stages (bits s0 + S - 1 down to s0) of the transform on the groups of 2^S elements that differ in those bits; `get(i)` yields
// element i (from Z, or from memory for the first step)
template <int P, int S, int NT, typename Get>
__device__ __forceinline__ void lm_step(cf* Z, const cf* TW, int s0, int tid, Get get)
{
    constexpr int M = 1 << P, R = 1 << S;
    for (int g = tid; g < (M >> S); g += NT) {
        const int lo = g & ((1 << s0) - 1);
        const int base = ((g >> s0) << (s0 + S)) | lo;
        cf v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = get(base + (r << s0));
#pragma unroll
        for (int q = S - 1; q >= 0; --q) {
            const int sh = P - (s0 + q);                      // M / h, h = 2^(s0 + q)
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (r & (1 << q)) continue;
                const int j = lo + ((r & ((1 << q) - 1)) << s0);
                lm_butterfly(v[r], v[r | (1 << q)], TW[lm_pad(j << sh)]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) Z[lm_pad(base + (r << s0))] = v[r];
    }
}

template <int P, int NT>
__device__ __forceinline__ void lm_transform(cf* Z, const cf* TW, int tid, const float* __restrict__ x, const float* __restrict__ win, bool gain,
                                             float shift, float denom)
{
    auto from_memory = [&](int i) {
        cf v;
        v.re = lm_sample(x[2 * i], gain, shift, denom, win[2 * i]);
        v.im = lm_sample(x[2 * i + 1], gain, shift, denom, win[2 * i + 1]);
        return v;
    };
    auto from_lds = [&](int i) { return Z[lm_pad(i)]; };
    lm_step<P, 3, NT>(Z, TW, P - 3, tid, from_memory);
    __syncthreads();
    constexpr int REST = (P - 3) % 3;                         // the stages the last step takes, when not three
#pragma unroll
    for (int s0 = P - 6; s0 >= REST; s0 -= 3) {
        lm_step<P, 3, NT>(Z, TW, s0, tid, from_lds);
        __syncthreads();
    }
    if (REST == 2) {
        lm_step<P, 2, NT>(Z, TW, 0, tid, from_lds);
        __syncthreads();
    } else if (REST == 1) {
        lm_step<P, 1, NT>(Z, TW, 0, tid, from_lds);
        __syncthreads();
    }
}

template <int LOGW>
__global__ __launch_bounds__((1 << (LOGW - 4)) < 64 ? 64 : (1 << (LOGW - 4))) void log_mel_kernel(const LogMelArgs a)
{
    constexpr int W = 1 << LOGW, M = W / 2, P = LOGW - 1;
    constexpr int NT = (W / 16) < 64 ? 64 : (W / 16);
    __shared__ cf Z[M + M / 8];
    __shared__ cf TW[M + M / 8];
    __shared__ float PW[M + 1];
    extern __shared__ float lm_out_tile[];
    float* const O = lm_out_tile;

    const int tid = threadIdx.x;
    const long long frame = blockIdx.x;
    const int n = (int)(frame / a.nFrame), t = (int)(frame - (long long)n * a.nFrame);
    const bool gain = a.shift != nullptr;
    const float shift = gain ? a.shift[n] : 0.0f, denom = gain ? a.denom[n] : 1.0f;
    const float inv_w = 1.0f / (float)W, fC = (float)a.C;
    const int nWin = a.nWin, nMel = a.nMel, C = a.C;
    const int row = nMel * nWin;

    for (int i = tid; i < M; i += NT) {
        cf w;
        w.re = a.tw[2 * i];
        w.im = a.tw[2 * i + 1];
        TW[lm_pad(i)] = w;
    }
    __syncthreads();

    const float* const xn = a.frames + (long long)n * a.sn + (long long)t * a.sf;

    // the power spectrum of (channel c, window w) into PW: stored when `first`, else added to the channels before; divided by C when `last`
    auto spectrum = [&](int c, int w, int first, int last) {
        lm_transform<P, NT>(Z, TW, tid, xn + (long long)c * a.sc, a.windows + (size_t)w * W, gain, shift, denom);
        for (int k = tid; k <= M; k += NT) {
            cf x;
            if (k == 0 || k == M) {
                const cf z = Z[0];
                x.re = k == 0 ? z.re + z.im : z.re - z.im;
                x.im = 0.0f;
            } else {
                x = lm_split(Z[lm_pad(lm_brev(k, P))], Z[lm_pad(lm_brev(M - k, P))], TW[lm_pad(k)]);
            }
            float p = lm_power(x, inv_w);
            if (!first) p = PW[k] + p;
            if (last) p = p / fC;
            PW[k] = p;
        }
        __syncthreads();
    };
    // the bands of window w from PW into the frame's tile
    auto bands = [&](int w) {
        for (int m = tid; m < nMel; m += NT) {
            int s, len;
            const int off = a.fb_off[m];
            lm_band(a.fb_start[m], a.fb_len[m], off, M, a.total, s, len);
            const float* const val = a.fb_val + off;
            float acc = 0.0f;
            int r = 0;
            for (; r + 4 <= len; r += 4) {                   // the four weights are asked for together; the chain stays one chain
                const float v0 = val[r], v1 = val[r + 1], v2 = val[r + 2], v3 = val[r + 3];
                acc = fmaf(PW[s + r], v0, acc);
                acc = fmaf(PW[s + r + 1], v1, acc);
                acc = fmaf(PW[s + r + 2], v2, acc);
                acc = fmaf(PW[s + r + 3], v3, acc);
            }
            for (; r < len; ++r) acc = fmaf(PW[s + r], val[r], acc);
            O[m * nWin + w] = a.log_flag ? lm_compress(acc, a.eps, a.le) : acc;
        }
    };
    auto store = [&](int c_out, int c_count) {
        __syncthreads();                                     // O is complete
        float* const o = a.out + (((long long)n * c_count + c_out) * a.nFrame + t) * (long long)row;
        for (int i = tid; i < row; i += NT) o[i] = O[i];
        __syncthreads();                                     // O is free
    };

    if (a.to_mono) {
        for (int w = 0; w < nWin; ++w) {
            for (int c = 0; c < C; ++c) spectrum(c, w, c == 0, c == C - 1);
            bands(w);                                        // PW is written again only behind the next transform's barriers
        }
        store(0, 1);
    } else {
        for (int c = 0; c < C; ++c) {
            for (int w = 0; w < nWin; ++w) {
                spectrum(c, w, 1, 0);
                bands(w);
            }
            store(c, C);
        }
    }
}

template <int LOGW>
static void log_mel_launch_one(const LogMelArgs& a, hipStream_t stream)
{
    constexpr int NT = ((1 << LOGW) / 16) < 64 ? 64 : ((1 << LOGW) / 16);
    const size_t dyn = (size_t)a.nMel * a.nWin * sizeof(float);
    hipLaunchKernelGGL((log_mel_kernel<LOGW>), dim3((unsigned)((long long)a.N * a.nFrame)), dim3(NT), dyn, stream, a);
}

// the caller (api.hip) has checked the supported set, the pointers, the strides and N nFrame < 2^31
void launch_log_mel(const float* frames, long long sn, long long sc, long long sf, int N, int C, int nFrame, int W, const float* windows, int nWin,
                    const float* tw, const int* fb_start, const int* fb_len, const int* fb_off, const float* fb_val, int nMel, int total,
                    const float* shift, const float* denom, int log_flag, float eps, int to_mono, float* out, hipStream_t stream)
{
    LogMelArgs a;
    a.frames = frames; a.sn = sn; a.sc = sc; a.sf = sf;
    a.N = N; a.C = C; a.nFrame = nFrame; a.nWin = nWin; a.nMel = nMel; a.total = total;
    a.windows = windows; a.tw = tw;
    a.fb_start = fb_start; a.fb_len = fb_len; a.fb_off = fb_off; a.fb_val = fb_val;
    a.shift = shift; a.denom = denom;
    a.log_flag = log_flag; a.to_mono = to_mono;
    a.eps = eps; a.le = (float)log((double)eps);
    a.out = out;
    switch (log2_of_window(W)) {
        case 8: log_mel_launch_one<8>(a, stream); break;
        case 9: log_mel_launch_one<9>(a, stream); break;
        case 10: log_mel_launch_one<10>(a, stream); break;
        case 11: log_mel_launch_one<11>(a, stream); break;
        case 12: log_mel_launch_one<12>(a, stream); break;
    }
}

}  // namespace semicrf
