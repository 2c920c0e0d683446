// attr_decode.hip -- the attribute-head readout of transcription (replaces the torch lines behind the two heads in
// TransKun.transcribeFrames, ModelTransformer.py:590-651: softmax and the velocity criterion, ContinuousBernoulli(logits).mean
// shifted back and clamped, the presence logits' sign) on the heads' raw outputs, in ONE launch.
//
// One wave per row, four rows per 256-thread workgroup (the shape of attr_loss_rows_kernel).  The 128 velocity logits are a float2
// per lane (classes 2 lane, 2 lane + 1); maximum and sum by xor-shuffles, so every lane holds the same bits; p = exp(x - max) / sum.
//   hamming  the smallest index of the largest LOGIT (no softmax involved: exact)
//   mse      sum_w p[w] w, the lane's two products added, then the xor tree
//   match    r[v] = sum of p[w], |w - v| <= 12, every r[v] summed DIRECTLY in ascending w from the neighbours' p (13 shuffles; a term
//            outside 0..127 is an exact + 0) -- never a difference of prefix sums, so windows that hold the same terms tie exactly --
//            then the smallest v with the largest r[v]
//   mae      inclusive cumulative sums in a fixed order (the lane's pair, then a Hillis-Steele scan over lanes), the first class whose
//            sum exceeds 0.5 by ballot + find-first (a parallel fp32 scan need not be monotone: nothing is counted)
// A row whose softmax is not finite (a NaN, a +inf, or all -inf: the sum of exp(x - max) is then NaN) yields class 0 / mean NaN, what
// torch.argmax of an all-NaN row gives.  Lane 0 evaluates the four onset/offset logits (attr_decode_math.h) and stores the row.
// No atomics, no LDS, nothing shared between rows: a row's result depends on that row alone and is bit-identical from run to run.
// Memory is never indexed by a computed class.
#include "common.h"
#include "launchers.h"
#include "attr_decode_math.h"

namespace semicrf {

using namespace attr_decode;

// the larger value, on a tie the smaller index -- over the wave; every lane ends with the same pair
__device__ __forceinline__ void wave_argmax_first(float& val, int& idx)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(val, o);
        const int oi = __shfl_xor(idx, o);
        if (ov > val || (ov == val && oi < idx)) { val = ov; idx = oi; }
    }
}

template <int CRIT>
__global__ __launch_bounds__(256) void attr_decode_kernel(const float* __restrict__ logitsVelocity, const float* __restrict__ ofLogits, int K,
                                                          long long* __restrict__ velocityClass, float* __restrict__ velocityMean,
                                                          float* __restrict__ ofValue, unsigned char* __restrict__ ofPresence)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= K) return;                                                      // (whole waves leave)
    const float2 x = *(const float2*)(logitsVelocity + (size_t)i * NVEL + 2 * lane);
    float m = fmaxf(x.x, x.y);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float2 p;
    p.x = expf(x.x - m); p.y = expf(x.y - m);
    float s = p.x + p.y;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const bool finite = s < __builtin_inff();                                // false for NaN; a finite row has 1 <= s <= 128
    p.x = p.x / s; p.y = p.y / s;

    int cls = 0;
    float mean = __builtin_nanf("");
    if (CRIT == CRIT_HAMMING) {
        float v = x.y > x.x ? x.y : x.x;
        int idx = x.y > x.x ? 2 * lane + 1 : 2 * lane;
        wave_argmax_first(v, idx);
        cls = idx;
    } else if (CRIT == CRIT_MSE) {
        float t = p.x * (float)(2 * lane) + p.y * (float)(2 * lane + 1);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
        mean = t;
    } else if (CRIT == CRIT_MATCH) {
        // lane's classes v0 = 2 lane and v1 = v0 + 1: r[v0] takes w = v0 - 12 .. v0 + 12, r[v1] takes w = v0 - 11 .. v0 + 13, i.e. the
        // pairs of lanes lane - 6 .. lane + 6, r[v1] without the even class of lane - 6 and r[v0] without the odd class of lane + 6
        float r0 = 0.0f, r1 = 0.0f;
#pragma unroll
        for (int d = -(MATCH_RADIUS / 2); d <= MATCH_RADIUS / 2; ++d) {
            const int src = lane + d;
            const float qx = __shfl(p.x, src & 63), qy = __shfl(p.y, src & 63);
            const bool in = (unsigned)src < 64u;
            const float ax = in ? qx : 0.0f, ay = in ? qy : 0.0f;
            r0 += ax;                                                        // w = 2 src
            if (d > -(MATCH_RADIUS / 2)) r1 += ax;                           //   (2 (lane - 6) = v1 - 13 is outside r[v1])
            if (d < MATCH_RADIUS / 2) r0 += ay;                              // w = 2 src + 1  (2 (lane + 6) + 1 = v0 + 13 is outside r[v0])
            r1 += ay;
        }
        float v = r1 > r0 ? r1 : r0;
        int idx = r1 > r0 ? 2 * lane + 1 : 2 * lane;
        wave_argmax_first(v, idx);
        cls = idx;
    } else {
        const float pair = p.x + p.y;
        float incl = pair;                                                   // inclusive scan of the lanes' pair sums
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        float excl = __shfl_up(incl, 1);
        if (lane == 0) excl = 0.0f;
        const float c0 = excl + p.x, c1 = excl + pair;                       // cum[2 lane], cum[2 lane + 1]
        const unsigned long long b0 = __ballot(c0 > 0.5f), b1 = __ballot(c1 > 0.5f);
        const unsigned long long any = b0 | b1;
        if (any) {
            const int l = __ffsll((long long)any) - 1;
            cls = 2 * l + (((b0 >> l) & 1ull) ? 0 : 1);
        }
    }
    if (lane != 0) return;
    if (CRIT == CRIT_MSE) velocityMean[i] = finite ? mean : __builtin_nanf("");
    else velocityClass[i] = finite ? (long long)cls : 0ll;
    const float* of = ofLogits + 4 * (size_t)i;
    ofValue[2 * (size_t)i] = of_value<float>(of[0]);
    ofValue[2 * (size_t)i + 1] = of_value<float>(of[1]);
    ofPresence[2 * (size_t)i] = of_presence(of[2]);
    ofPresence[2 * (size_t)i + 1] = of_presence(of[3]);
}

void launch_attr_decode(const float* logitsVelocity, const float* ofLogits, int K, int criterion, long long* velocityClass,
                        float* velocityMean, float* ofValue, unsigned char* ofPresence, hipStream_t stream)
{
    if (K <= 0) return;
    const dim3 grid((K + 3) / 4), block(256);
    switch (criterion) {
    case CRIT_HAMMING:
        hipLaunchKernelGGL(attr_decode_kernel<CRIT_HAMMING>, grid, block, 0, stream, logitsVelocity, ofLogits, K, velocityClass, velocityMean,
                           ofValue, ofPresence);
        break;
    case CRIT_MSE:
        hipLaunchKernelGGL(attr_decode_kernel<CRIT_MSE>, grid, block, 0, stream, logitsVelocity, ofLogits, K, velocityClass, velocityMean,
                           ofValue, ofPresence);
        break;
    case CRIT_MATCH:
        hipLaunchKernelGGL(attr_decode_kernel<CRIT_MATCH>, grid, block, 0, stream, logitsVelocity, ofLogits, K, velocityClass, velocityMean,
                           ofValue, ofPresence);
        break;
    default:
        hipLaunchKernelGGL(attr_decode_kernel<CRIT_MAE>, grid, block, 0, stream, logitsVelocity, ofLogits, K, velocityClass, velocityMean,
                           ofValue, ofPresence);
        break;
    }
}

}  // namespace semicrf
