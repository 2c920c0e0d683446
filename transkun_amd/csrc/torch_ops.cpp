// torch_ops.cpp -- LibTorch stable-ABI shim: registers the C ABI of include/semicrf_hip.h as torch ops (namespace
// `semicrf`, dispatch key CUDA = HIP tensors on ROCm), so that the Python mirror of the reference class calls
// torch.ops.semicrf.* -- dispatcher, stream and device handling by torch -- instead of ctypes.  Built into its own
// library (libsemicrf_torch.so) that links libsemicrf_hip.so: the C ABI itself stays free of torch.
//
// Only torch/csrc/stable/* and the aoti C shim are used (no ATen/c10 C++ ABI): the binary does not depend on the
// libtorch C++ ABI of the build.  Every op runs on the tensors' device (device guard) and enqueues on torch's current
// stream of that device; outputs and the workspace are allocated by the caller (the Python mirror) and passed in.
#define USE_ROCM 1
#include <torch/csrc/stable/accelerator.h>
#include <torch/csrc/stable/library.h>
#include <torch/csrc/stable/tensor.h>

#include "../../include/semicrf_hip.h"
#include "cpu_ops.h"

#include <optional>
#include <vector>

using torch::stable::Tensor;
using torch::headeronly::ScalarType;

namespace {

// Every op is dispatcher-visible: arguments are checked here (dtype, contiguity, element counts against T / B / K), not only
// in the Python mirror -- a wrong dtype or a short buffer is an error, never an out-of-bounds access.
inline void want(const Tensor& t, ScalarType st, int64_t min_numel, const char* name)
{
    STD_TORCH_CHECK(t.defined(), "semicrf: `", name, "` is undefined");
    STD_TORCH_CHECK(t.scalar_type() == st, "semicrf: `", name, "` has the wrong dtype");
    STD_TORCH_CHECK(t.is_contiguous(), "semicrf: `", name, "` must be contiguous");
    STD_TORCH_CHECK(t.numel() >= min_numel, "semicrf: `", name, "` holds ", t.numel(), " elements, the call needs ", min_numel);
}
inline const float* f32(const Tensor& t, int64_t n, const char* name) { want(t, ScalarType::Float, n, name); return n > 0 || t.numel() > 0 ? (const float*)t.data_ptr() : nullptr; }
inline float* f32w(const Tensor& t, int64_t n, const char* name) { return (float*)f32(t, n, name); }
inline int32_t* i32(const Tensor& t, int64_t n, const char* name) { want(t, ScalarType::Int, n, name); return n > 0 || t.numel() > 0 ? (int32_t*)t.data_ptr() : nullptr; }
inline void* bytes(const Tensor& t, const char* name) { want(t, ScalarType::Byte, 0, name); return t.numel() > 0 ? t.data_ptr() : nullptr; }

struct Dims { int T, B; };
inline Dims crf_dims(const Tensor& score, const Tensor& noise)
{
    STD_TORCH_CHECK(score.dim() == 3 && score.size(0) == score.size(1), "semicrf: score must be [T, T, B]");
    const int64_t T = score.size(0), B = score.size(2);
    STD_TORCH_CHECK(T >= 1 && B >= 1 && T < (1 << 29) && B < (1ll << 31), "semicrf: bad score shape");
    want(score, ScalarType::Float, T * T * B, "score");
    want(noise, ScalarType::Float, (T - 1) * B, "noise");
    return Dims{(int)T, (int)B};
}

struct Ctx {
    torch::stable::accelerator::DeviceGuard guard;
    void* stream = nullptr;
    static int32_t index_of(const Tensor& t)
    {
        STD_TORCH_CHECK(t.is_cuda(), "semicrf: this overload takes GPU tensors");
        return t.get_device_index();
    }
    explicit Ctx(const Tensor& t) : guard(index_of(t))          // is_cuda is checked BEFORE the guard is built
    {
        TORCH_ERROR_CODE_CHECK(aoti_torch_get_current_cuda_stream(t.get_device_index(), &stream));
    }
    // every tensor of a call lives on the device of the first one
    template <typename... Ts>
    void same(const Tensor& a, const Ts&... rest) const
    {
        const Tensor* ts[] = {&rest...};
        for (const Tensor* t : ts)
            STD_TORCH_CHECK(!t->defined() || t->numel() == 0 || (t->is_cuda() && t->get_device_index() == a.get_device_index()),
                            "semicrf: all tensors of a call must share one device");
    }
};
template <typename... Ts>
inline void all_cpu(const Ts&... ts)
{
    const Tensor* a[] = {&ts...};
    for (const Tensor* t : a)
        STD_TORCH_CHECK(!t->defined() || t->numel() == 0 || t->is_cpu(), "semicrf: all tensors of a call must share one device");
}

inline void check(int rc, const char* what)
{
    STD_TORCH_CHECK(rc == SEMICRF_OK, what, " failed (code ", rc, "): ", semicrf_last_error());
}
inline float* fp(const Tensor& t) { return t.defined() && t.numel() > 0 ? (float*)t.data_ptr() : nullptr; }
inline const float* cfp(const Tensor& t) { return t.defined() && t.numel() > 0 ? (const float*)t.data_ptr() : nullptr; }
inline int32_t* ip(const Tensor& t) { return t.defined() && t.numel() > 0 ? (int32_t*)t.data_ptr() : nullptr; }

// ---- semi-CRF: the ops registered for both dispatch keys ----------------------------------------------------------------
// Per op ONE `*_args` function performs every check that does not depend on where the tensors live and returns the raw pointers
// and sizes; the two twins follow it.  The GPU twin (dispatch key CUDA = HIP tensors) adds the device handling (Ctx / same), the
// workspace and the call of the C ABI.  The `_cpu` twin (dispatch key CPU) adds all_cpu, the checks that read the tensors'
// contents (offsets, intervals, forced frames: host-readable only here) and the product's own host kernels (cpu_ops.cpp) --
// selected by the tensors' device, never a fallback for GPU tensors; its workspace argument is ignored (pass an empty tensor).
// A check that only one twin makes is written in that twin.
inline int64_t pairs_cap(const Tensor& pairs)
{
    STD_TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, "semicrf: pairs must be [cap, 2]");
    return pairs.size(0);
}
inline int64_t pairs_cap1(const Tensor& pairs)
{
    STD_TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2 && pairs.size(0) >= 1, "semicrf: pairs must be [cap, 2], cap >= 1");
    return pairs.size(0);
}
// host-readable checks of the `_cpu` twins
inline void frames_in_range(const int32_t* f, const Dims& d, const char* what)       // forced start / end frames (null: none)
{
    if (f)
        for (int c = 0; c < d.B; ++c) STD_TORCH_CHECK(f[c] >= 0 && f[c] < d.T, "semicrf: ", what, " out of range");
}
inline void check_offsets_cover(const int32_t* offsets, int64_t K, int B)
{
    STD_TORCH_CHECK(offsets[0] == 0 && offsets[B] == K, "semicrf: offsets do not match the interval count");
    for (int c = 0; c < B; ++c) STD_TORCH_CHECK(offsets[c] <= offsets[c + 1], "semicrf: offsets must ascend");
}
inline void check_path(const int32_t* pairs, int64_t K, const int32_t* offsets, int T, int B)      // 0 <= begin <= end < T
{
    check_offsets_cover(offsets, K, B);
    for (int64_t i = 0; i < K; ++i)
        STD_TORCH_CHECK(pairs[2 * i] >= 0 && pairs[2 * i] <= pairs[2 * i + 1] && pairs[2 * i + 1] < T, "semicrf: interval out of range");
}
inline void check_cells(const int32_t* pairs, int64_t K, const int32_t* offsets, int T, int B)     // any order of begin and end
{
    check_offsets_cover(offsets, K, B);
    for (int64_t i = 0; i < 2 * K; ++i) STD_TORCH_CHECK(pairs[i] >= 0 && pairs[i] < T, "semicrf: interval out of range");
}

struct LogzFwdArgs { Dims d; const float *score, *noise; float *logZ, *v; };                  // v: null when not wanted
inline LogzFwdArgs logz_fwd_args(const Tensor& score, const Tensor& noise, const Tensor& logZ, const Tensor& v, bool want_v)
{
    const Dims d = crf_dims(score, noise);
    return LogzFwdArgs{d, cfp(score), cfp(noise), f32w(logZ, d.B, "logZ"), want_v ? f32w(v, (int64_t)d.T * d.B, "v") : nullptr};
}
void logz_fwd(Tensor score, Tensor noise, Tensor logZ, Tensor v, bool want_v, Tensor ws)
{
    Ctx c(score); c.same(score, noise, logZ, v, ws);
    const LogzFwdArgs a = logz_fwd_args(score, noise, logZ, v, want_v);
    check(semicrf_logz_fwd(a.score, a.noise, a.d.T, a.d.B, a.logZ, a.v, bytes(ws, "ws"), (size_t)ws.numel(), c.stream), "semicrf_logz_fwd");
}
void logz_fwd_cpu(Tensor score, Tensor noise, Tensor logZ, Tensor v, bool want_v, Tensor ws)
{
    all_cpu(score, noise, logZ, v);
    const LogzFwdArgs a = logz_fwd_args(score, noise, logZ, v, want_v);
    std::vector<float> scratch;
    if (!want_v) scratch.resize((size_t)a.d.T * a.d.B);
    semicrf_cpu::logz_fwd(a.score, a.noise, a.d.T, a.d.B, a.logZ, want_v ? a.v : scratch.data());
}

struct LogzBwdArgs { Dims d; const float *score, *noise, *v, *logZ, *gout; float *dScore, *dNoise, *q; };      // q: null when not wanted
inline LogzBwdArgs logz_bwd_args(const Tensor& score, const Tensor& noise, const Tensor& v, const Tensor& logZ, const Tensor& gout,
                                 const Tensor& dScore, const Tensor& dNoise, const Tensor& q, bool want_q)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    return LogzBwdArgs{d, cfp(score), cfp(noise), f32(v, TB, "v"), f32(logZ, d.B, "logZ"), f32(gout, d.B, "gout"),
                       f32w(dScore, TB * d.T, "dScore"), f32w(dNoise, TB - d.B, "dNoise"), want_q ? f32w(q, TB, "q") : nullptr};
}
void logz_bwd(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, Tensor dScore, Tensor dNoise, Tensor q, bool want_q,
              int64_t flags, Tensor ws)
{
    Ctx c(score); c.same(score, noise, v, logZ, gout, dScore, dNoise, q, ws);
    const LogzBwdArgs a = logz_bwd_args(score, noise, v, logZ, gout, dScore, dNoise, q, want_q);
    check(semicrf_logz_bwd_f(a.score, a.noise, a.v, a.logZ, a.gout, a.d.T, a.d.B, a.dScore, a.dNoise, a.q, (int)flags, bytes(ws, "ws"),
                             (size_t)ws.numel(), c.stream),
          "semicrf_logz_bwd");
}
void logz_bwd_cpu(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, Tensor dScore, Tensor dNoise, Tensor q, bool want_q,
                  int64_t flags, Tensor ws)       // flags: a permission (SEMICRF_GRAD_UPPER_IS_ZERO); the host kernels write everything
{
    all_cpu(score, noise, v, logZ, gout, dScore, dNoise, q);
    const LogzBwdArgs a = logz_bwd_args(score, noise, v, logZ, gout, dScore, dNoise, q, want_q);
    std::vector<float> scratch;
    if (!want_q) scratch.resize((size_t)a.d.T * a.d.B);
    semicrf_cpu::logz_bwd(a.score, a.noise, a.v, a.logZ, a.gout, a.d.T, a.d.B, a.dScore, a.dNoise, want_q ? a.q : scratch.data());
}

struct BetaArgs { Dims d; const float *score, *noise; float* beta; };
inline BetaArgs beta_args(const Tensor& score, const Tensor& noise, const Tensor& out)
{
    const Dims d = crf_dims(score, noise);
    return BetaArgs{d, cfp(score), cfp(noise), f32w(out, (int64_t)d.T * d.B, "beta")};
}
void beta(Tensor score, Tensor noise, Tensor out, Tensor ws)
{
    Ctx c(score); c.same(score, noise, out, ws);
    const BetaArgs a = beta_args(score, noise, out);
    check(semicrf_beta(a.score, a.noise, a.d.T, a.d.B, a.beta, bytes(ws, "ws"), (size_t)ws.numel(), c.stream), "semicrf_beta");
}
void beta_cpu(Tensor score, Tensor noise, Tensor out, Tensor ws)
{
    all_cpu(score, noise, out);
    const BetaArgs a = beta_args(score, noise, out);
    semicrf_cpu::logz_bwd(a.score, a.noise, nullptr, nullptr, nullptr, a.d.T, a.d.B, nullptr, nullptr, a.beta);
}

struct AlphaFromArgs { Dims d; const float *score, *noise; const int32_t* start; float *v, *logZ; };
inline AlphaFromArgs alpha_from_args(const Tensor& score, const Tensor& noise, const Tensor& start, const Tensor& v, const Tensor& logZ)
{
    const Dims d = crf_dims(score, noise);
    return AlphaFromArgs{d, cfp(score), cfp(noise), i32(start, d.B, "start"), f32w(v, (int64_t)d.T * d.B, "v"), f32w(logZ, d.B, "logZ")};
}
void alpha_from(Tensor score, Tensor noise, Tensor start, Tensor v, Tensor logZ, Tensor ws)
{
    Ctx c(score); c.same(score, noise, start, v, logZ, ws);
    const AlphaFromArgs a = alpha_from_args(score, noise, start, v, logZ);
    check(semicrf_alpha_from(a.score, a.noise, a.start, a.d.T, a.d.B, a.v, a.logZ, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_alpha_from");
}
void alpha_from_cpu(Tensor score, Tensor noise, Tensor start, Tensor v, Tensor logZ, Tensor ws)
{
    all_cpu(score, noise, start, v, logZ);
    const AlphaFromArgs a = alpha_from_args(score, noise, start, v, logZ);
    semicrf_cpu::alpha_from(a.score, a.noise, a.start, a.d.T, a.d.B, a.v, a.logZ);
}

struct ViterbiArgs { Dims d; const float *score, *noise; const int32_t* start; int32_t* pairs; int64_t cap; int32_t* offsets; };
inline ViterbiArgs viterbi_args(const Tensor& score, const Tensor& noise, const Tensor& start, bool has_start, const Tensor& pairs,
                                const Tensor& offsets)
{
    const Dims d = crf_dims(score, noise);
    const int64_t cap = pairs_cap(pairs);
    return ViterbiArgs{d, cfp(score), cfp(noise), has_start ? i32(start, d.B, "start") : nullptr, i32(pairs, 0, "pairs"), cap,
                       i32(offsets, d.B + 1, "offsets")};
}
void viterbi(Tensor score, Tensor noise, Tensor start, bool has_start, bool forward, Tensor pairs, Tensor offsets, Tensor ws)
{
    Ctx c(score); c.same(score, noise, pairs, offsets, ws);
    if (has_start) c.same(score, start);
    const ViterbiArgs a = viterbi_args(score, noise, start, has_start, pairs, offsets);
    check(semicrf_viterbi(a.score, a.noise, a.d.T, a.d.B, a.start, forward ? 1 : 0, a.pairs, a.cap, a.offsets, bytes(ws, "ws"),
                          (size_t)ws.numel(), c.stream),
          "semicrf_viterbi");
}
void viterbi_cpu(Tensor score, Tensor noise, Tensor start, bool has_start, bool forward, Tensor pairs, Tensor offsets, Tensor ws)
{
    all_cpu(score, noise, pairs, offsets);
    if (has_start) all_cpu(start);
    const ViterbiArgs a = viterbi_args(score, noise, start, has_start, pairs, offsets);
    frames_in_range(a.start, a.d, "forcedStartPos");
    semicrf_cpu::viterbi(a.score, a.noise, a.d.T, a.d.B, a.start, forward ? 1 : 0, a.pairs, a.cap, a.offsets);
}

// posterior sampling (semicrf_sample): key is the 64-bit key as a signed int (two's complement); end: B ints when has_end
struct SampleArgs { Dims d; const float *score, *noise, *v; const int32_t* end; int32_t* pairs; int64_t cap; int32_t* offsets; };
inline SampleArgs sample_args(const Tensor& score, const Tensor& noise, const Tensor& v, int64_t k0, int64_t nSample, const Tensor& end,
                              bool has_end, const Tensor& pairs, const Tensor& offsets)
{
    const Dims d = crf_dims(score, noise);
    STD_TORCH_CHECK(nSample >= 1 && nSample < (1 << 30) && k0 >= 0, "semicrf: bad nSample / k0");
    const int64_t cap = pairs_cap(pairs);
    return SampleArgs{d, cfp(score), cfp(noise), f32(v, (int64_t)d.T * d.B, "v"), has_end ? i32(end, d.B, "end") : nullptr,
                      i32(pairs, 0, "pairs"), cap, i32(offsets, nSample * d.B + 1, "offsets")};
}
void sample(Tensor score, Tensor noise, Tensor v, int64_t k0, int64_t nSample, int64_t key, Tensor end, bool has_end, Tensor pairs,
            Tensor offsets, Tensor ws)
{
    Ctx c(score); c.same(score, noise, v, pairs, offsets, ws);
    if (has_end) c.same(score, end);
    const SampleArgs a = sample_args(score, noise, v, k0, nSample, end, has_end, pairs, offsets);
    check(semicrf_sample(a.score, a.noise, a.v, a.d.T, a.d.B, k0, (int)nSample, (uint64_t)key, a.end, a.pairs, a.cap, a.offsets,
                         bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_sample");
}
void sample_cpu(Tensor score, Tensor noise, Tensor v, int64_t k0, int64_t nSample, int64_t key, Tensor end, bool has_end, Tensor pairs,
                Tensor offsets, Tensor ws)
{
    all_cpu(score, noise, v, pairs, offsets);
    if (has_end) all_cpu(end);
    const SampleArgs a = sample_args(score, noise, v, k0, nSample, end, has_end, pairs, offsets);
    STD_TORCH_CHECK(nSample * a.d.B * 2 * a.d.T < (1ll << 31), "semicrf: nSample*B*2T exceeds int32 offsets");      // this twin only
    frames_in_range(a.end, a.d, "forcedEndPos");
    semicrf_cpu::sample(a.score, a.noise, a.v, a.d.T, a.d.B, k0, (int)nSample, (uint64_t)key, a.end, a.pairs, a.cap, a.offsets);
}

// k-best Viterbi (semicrf_viterbi_nbest): rank-major offsets [k*B+1], scores [k][B], npaths [B]
struct NbestArgs { Dims d; const float *score, *noise; const int32_t* start; int32_t* pairs; int64_t cap; int32_t* offsets; float* scores; int32_t* npaths; };
inline NbestArgs viterbi_nbest_args(const Tensor& score, const Tensor& noise, int64_t k, const Tensor& start, bool has_start,
                                    const Tensor& pairs, const Tensor& offsets, const Tensor& scores, const Tensor& npaths)
{
    const Dims d = crf_dims(score, noise);
    STD_TORCH_CHECK(k >= 1 && k <= 16, "semicrf: k must be in [1, 16]");
    const int64_t cap = pairs_cap(pairs);
    return NbestArgs{d, cfp(score), cfp(noise), has_start ? i32(start, d.B, "start") : nullptr, i32(pairs, 0, "pairs"), cap,
                     i32(offsets, k * d.B + 1, "offsets"), f32w(scores, k * d.B, "scores"), i32(npaths, d.B, "npaths")};
}
void viterbi_nbest(Tensor score, Tensor noise, int64_t k, Tensor start, bool has_start, bool forward, Tensor pairs, Tensor offsets,
                   Tensor scores, Tensor npaths, Tensor ws)
{
    Ctx c(score); c.same(score, noise, pairs, offsets, scores, npaths, ws);
    if (has_start) c.same(score, start);
    const NbestArgs a = viterbi_nbest_args(score, noise, k, start, has_start, pairs, offsets, scores, npaths);
    check(semicrf_viterbi_nbest(a.score, a.noise, a.d.T, a.d.B, (int)k, a.start, forward ? 1 : 0, a.pairs, a.cap, a.offsets, a.scores,
                                a.npaths, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_viterbi_nbest");
}
void viterbi_nbest_cpu(Tensor score, Tensor noise, int64_t k, Tensor start, bool has_start, bool forward, Tensor pairs, Tensor offsets,
                       Tensor scores, Tensor npaths, Tensor ws)
{
    all_cpu(score, noise, pairs, offsets, scores, npaths);
    if (has_start) all_cpu(start);
    const NbestArgs a = viterbi_nbest_args(score, noise, k, start, has_start, pairs, offsets, scores, npaths);
    STD_TORCH_CHECK(k * a.d.B * 2 * a.d.T < (1ll << 31), "semicrf: k*B*2T exceeds int32 offsets");                  // this twin only
    frames_in_range(a.start, a.d, "forcedStartPos");
    semicrf_cpu::viterbi_nbest(a.score, a.noise, a.d.T, a.d.B, (int)k, a.start, forward ? 1 : 0, a.pairs, a.cap, a.offsets, a.scores,
                               a.npaths);
}

// posterior marginals and entropy (semicrf_posteriors): v, q, logZ of the same score / noise
struct PosteriorsArgs { Dims d; const float *score, *noise, *v, *q, *logZ; float *node, *begin, *end, *single, *noiseP, *entropy; };
inline PosteriorsArgs posteriors_args(const Tensor& score, const Tensor& noise, const Tensor& v, const Tensor& q, const Tensor& logZ,
                                      const Tensor& node, const Tensor& begin, const Tensor& end, const Tensor& single,
                                      const Tensor& noiseP, const Tensor& entropy)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    return PosteriorsArgs{d, cfp(score), cfp(noise), f32(v, TB, "v"), f32(q, TB, "q"), f32(logZ, d.B, "logZ"), f32w(node, TB, "node"),
                          f32w(begin, TB, "begin"), f32w(end, TB, "end"), f32w(single, TB, "single"), f32w(noiseP, TB - d.B, "noiseP"),
                          f32w(entropy, d.B, "entropy")};
}
void posteriors(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor node, Tensor begin, Tensor end, Tensor single,
                Tensor noiseP, Tensor entropy, Tensor ws)
{
    Ctx c(score); c.same(score, noise, v, q, logZ, node, begin, end, single, noiseP, entropy, ws);
    const PosteriorsArgs a = posteriors_args(score, noise, v, q, logZ, node, begin, end, single, noiseP, entropy);
    check(semicrf_posteriors(a.score, a.noise, a.v, a.q, a.logZ, a.d.T, a.d.B, a.node, a.begin, a.end, a.single, a.noiseP, a.entropy,
                             bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_posteriors");
}
void posteriors_cpu(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor node, Tensor begin, Tensor end, Tensor single,
                    Tensor noiseP, Tensor entropy, Tensor ws)
{
    all_cpu(score, noise, v, q, logZ, node, begin, end, single, noiseP, entropy);
    const PosteriorsArgs a = posteriors_args(score, noise, v, q, logZ, node, begin, end, single, noiseP, entropy);
    semicrf_cpu::posteriors(a.score, a.noise, a.v, a.q, a.logZ, a.d.T, a.d.B, a.node, a.begin, a.end, a.single, a.noiseP, a.entropy);
}

// posterior expectation / covariance (semicrf_expectation, semicrf_covariance): weight may BE score (read once); nweight is
// read when has_nw.  ws: the state the pair shares (semicrf_workspace_bytes(SEMICRF_OP_EXPECTATION); the host kernels:
// (4 T B + 2 B) doubles)
inline const float* weight_of(const Tensor& weight, const Tensor& score, int64_t n)
{
    const float* w = f32(weight, n, "weight");
    STD_TORCH_CHECK(weight.numel() == score.numel(), "semicrf: weight must have the shape of score");
    return w;
}
inline double* state_cpu(const Tensor& ws, const Dims& d)
{
    want(ws, ScalarType::Byte, (int64_t)((4 * (int64_t)d.T * d.B + 2 * d.B) * sizeof(double)), "ws");
    STD_TORCH_CHECK(((uintptr_t)ws.data_ptr() & 7) == 0, "semicrf: `ws` must be 8-byte aligned");
    return (double*)ws.data_ptr();
}
struct ExpectationArgs { Dims d; const float *score, *noise, *weight, *nweight; float *E, *H; };
inline ExpectationArgs expectation_args(const Tensor& score, const Tensor& noise, const Tensor& weight, const Tensor& nweight, bool has_nw,
                                        const Tensor& E, const Tensor& H)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    return ExpectationArgs{d, cfp(score), cfp(noise), weight_of(weight, score, TB * d.T), has_nw ? f32(nweight, TB - d.B, "noiseWeight") : nullptr,
                           f32w(E, d.B, "E"), f32w(H, d.B, "H")};
}
void expectation(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor v, Tensor q, Tensor E, Tensor H, Tensor ws)
{
    Ctx c(score); c.same(score, noise, weight, v, q, E, H, ws);
    if (has_nw) c.same(score, nweight);
    const ExpectationArgs a = expectation_args(score, noise, weight, nweight, has_nw, E, H);
    const int64_t TB = (int64_t)a.d.T * a.d.B;
    check(semicrf_expectation(a.score, a.noise, a.weight, a.nweight, f32(v, TB, "v"), f32(q, TB, "q"),        // v, q: this twin only
                              a.d.T, a.d.B, a.E, a.H, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_expectation");
}
void expectation_cpu(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor v, Tensor q, Tensor E, Tensor H,
                     Tensor ws)
{
    all_cpu(score, noise, weight, nweight, v, q, E, H, ws);       // the host kernels keep their own alpha / beta: v, q are not read
    const ExpectationArgs a = expectation_args(score, noise, weight, nweight, has_nw, E, H);
    semicrf_cpu::expectation(a.score, a.noise, a.weight, a.nweight, a.d.T, a.d.B, a.E, a.H, state_cpu(ws, a.d));
}
struct CovarianceArgs { Dims d; const float *score, *noise, *weight, *nweight, *gout; float *C, *Cn; };
inline CovarianceArgs covariance_args(const Tensor& score, const Tensor& noise, const Tensor& weight, const Tensor& nweight, bool has_nw,
                                      const Tensor& gout, const Tensor& C, const Tensor& Cn)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    return CovarianceArgs{d, cfp(score), cfp(noise), weight_of(weight, score, TB * d.T), has_nw ? f32(nweight, TB - d.B, "noiseWeight") : nullptr,
                          f32(gout, d.B, "gout"), f32w(C, TB * d.T, "C"), f32w(Cn, TB - d.B, "Cn")};
}
void covariance(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor gout, Tensor C, Tensor Cn, Tensor ws)
{
    Ctx c(score); c.same(score, noise, weight, gout, C, Cn, ws);
    if (has_nw) c.same(score, nweight);
    const CovarianceArgs a = covariance_args(score, noise, weight, nweight, has_nw, gout, C, Cn);
    check(semicrf_covariance(a.score, a.noise, a.weight, a.nweight, a.gout, a.d.T, a.d.B, a.C, a.Cn, bytes(ws, "ws"), (size_t)ws.numel(),
                             c.stream),
          "semicrf_covariance");
}
void covariance_cpu(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor gout, Tensor C, Tensor Cn, Tensor ws)
{
    all_cpu(score, noise, weight, nweight, gout, C, Cn, ws);
    const CovarianceArgs a = covariance_args(score, noise, weight, nweight, has_nw, gout, C, Cn);
    semicrf_cpu::covariance(a.score, a.noise, a.weight, a.nweight, a.gout, a.d.T, a.d.B, state_cpu(ws, a.d), a.C, a.Cn);
}

// interval marginals (semicrf_interval_marginals[_tol]): pairs / offsets as eval_path; tol_begin, tol_end in 0 .. SEMICRF_TOL_MAX
inline void check_tol(int64_t tb, int64_t te)
{
    STD_TORCH_CHECK(tb >= 0 && tb <= SEMICRF_TOL_MAX && te >= 0 && te <= SEMICRF_TOL_MAX, "semicrf: tolerance (", tb, ", ", te,
                    ") outside [0, ", SEMICRF_TOL_MAX, "]");
}
struct MarginalsArgs { Dims d; const float *score, *v, *q, *logZ; const int32_t *pairs, *offsets; float* out; };
inline MarginalsArgs interval_marginals_args(const Tensor& score, const Tensor& v, const Tensor& q, const Tensor& logZ, const Tensor& pairs,
                                             int64_t K, const Tensor& offsets, const Tensor& out, int64_t tol_begin = 0, int64_t tol_end = 0)
{
    STD_TORCH_CHECK(score.dim() == 3 && score.size(0) == score.size(1), "semicrf: score must be [T, T, B]");
    const int64_t T = score.size(0), B = score.size(2);
    STD_TORCH_CHECK(T >= 1 && B >= 1 && T < (1 << 29) && B < (1ll << 31), "semicrf: bad score shape");
    want(score, ScalarType::Float, T * T * B, "score");
    want(v, ScalarType::Float, T * B, "v");
    want(q, ScalarType::Float, T * B, "q");
    want(logZ, ScalarType::Float, B, "logZ");
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    check_tol(tol_begin, tol_end);
    return MarginalsArgs{Dims{(int)T, (int)B}, cfp(score), cfp(v), cfp(q), cfp(logZ), i32(pairs, 2 * K, "pairs"), i32(offsets, B + 1, "offsets"),
                         f32w(out, K, "out")};
}
void interval_marginals(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int64_t K, Tensor offsets, Tensor out)
{
    Ctx c(score); c.same(score, v, q, logZ, pairs, offsets, out);
    const MarginalsArgs a = interval_marginals_args(score, v, q, logZ, pairs, K, offsets, out);
    check(semicrf_interval_marginals(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.pairs, K, a.offsets, a.out, c.stream),
          "semicrf_interval_marginals");
}
void interval_marginals_cpu(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int64_t K, Tensor offsets, Tensor out)
{
    all_cpu(score, v, q, logZ, pairs, offsets, out);
    const MarginalsArgs a = interval_marginals_args(score, v, q, logZ, pairs, K, offsets, out);
    check_cells(a.pairs, K, a.offsets, a.d.T, a.d.B);
    semicrf_cpu::interval_marginals(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.pairs, a.offsets, a.out);
}
void interval_marginals_tol(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int64_t K, Tensor offsets, int64_t tol_begin,
                            int64_t tol_end, Tensor out)
{
    Ctx c(score); c.same(score, v, q, logZ, pairs, offsets, out);
    const MarginalsArgs a = interval_marginals_args(score, v, q, logZ, pairs, K, offsets, out, tol_begin, tol_end);
    check(semicrf_interval_marginals_tol(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.pairs, K, a.offsets, (int)tol_begin, (int)tol_end, a.out,
                                         c.stream),
          "semicrf_interval_marginals_tol");
}
void interval_marginals_tol_cpu(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int64_t K, Tensor offsets, int64_t tol_begin,
                                int64_t tol_end, Tensor out)
{
    all_cpu(score, v, q, logZ, pairs, offsets, out);
    const MarginalsArgs a = interval_marginals_args(score, v, q, logZ, pairs, K, offsets, out, tol_begin, tol_end);
    check_cells(a.pairs, K, a.offsets, a.d.T, a.d.B);
    if (tol_begin == 0 && tol_end == 0)
        semicrf_cpu::interval_marginals(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.pairs, a.offsets, a.out);
    else
        semicrf_cpu::interval_marginals_tol(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.pairs, a.offsets, (int)tol_begin, (int)tol_end, a.out);
}

// marginal-threshold decoding (semicrf_marginal_decode[_tol]): tau holds 1 value (all chains) or B (per chain); pairs [cap, 2], probs [cap]
inline int tau_stride_of(const Tensor& tau, int B)
{
    want(tau, ScalarType::Float, 1, "tau");
    STD_TORCH_CHECK(tau.numel() == 1 || tau.numel() == B, "semicrf: tau must hold 1 value or one per chain (", B, "), got ", tau.numel());
    return tau.numel() == B && B > 1 ? 1 : 0;
}
struct MarginalDecodeArgs { Dims d; const float *score, *noise, *v, *q, *logZ, *tau; int tau_stride; int32_t* pairs; float* probs; int64_t cap; int32_t* offsets; };
inline MarginalDecodeArgs marginal_decode_args(const Tensor& score, const Tensor& noise, const Tensor& v, const Tensor& q, const Tensor& logZ,
                                               const Tensor& tau, const Tensor& pairs, const Tensor& probs, const Tensor& offsets,
                                               int64_t tol_begin = 0, int64_t tol_end = 0)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    const int64_t cap = pairs_cap1(pairs);
    check_tol(tol_begin, tol_end);
    return MarginalDecodeArgs{d, cfp(score), cfp(noise), f32(v, TB, "v"), f32(q, TB, "q"), f32(logZ, d.B, "logZ"), cfp(tau), tau_stride_of(tau, d.B),
                              i32(pairs, 2 * cap, "pairs"), f32w(probs, cap, "probs"), cap, i32(offsets, d.B + 1, "offsets")};
}
// (the `_cpu` twins only) the host kernels count cells in int32
inline void check_cell_count(const Dims& d)
{
    STD_TORCH_CHECK((int64_t)d.T * (d.T + 1) / 2 * d.B < (1ll << 31), "semicrf: T (T+1) / 2 * B exceeds int32 offsets");
}
void marginal_decode(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, Tensor pairs, Tensor probs, Tensor offsets,
                     Tensor ws)
{
    Ctx c(score); c.same(score, noise, v, q, logZ, tau, pairs, probs, offsets, ws);
    const MarginalDecodeArgs a = marginal_decode_args(score, noise, v, q, logZ, tau, pairs, probs, offsets);
    check(semicrf_marginal_decode(a.score, a.noise, a.v, a.q, a.logZ, a.d.T, a.d.B, a.tau, a.tau_stride, a.pairs, a.probs, a.cap, a.offsets,
                                  bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_marginal_decode");
}
void marginal_decode_cpu(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, Tensor pairs, Tensor probs,
                         Tensor offsets, Tensor ws)
{
    all_cpu(score, noise, v, q, logZ, tau, pairs, probs, offsets);
    const MarginalDecodeArgs a = marginal_decode_args(score, noise, v, q, logZ, tau, pairs, probs, offsets);
    check_cell_count(a.d);
    semicrf_cpu::marginal_decode(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.tau, a.tau_stride, a.pairs, a.probs, a.cap, a.offsets);
}
void marginal_decode_tol(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, int64_t tol_begin, int64_t tol_end,
                         Tensor pairs, Tensor probs, Tensor offsets, Tensor ws)
{
    Ctx c(score); c.same(score, noise, v, q, logZ, tau, pairs, probs, offsets, ws);
    const MarginalDecodeArgs a = marginal_decode_args(score, noise, v, q, logZ, tau, pairs, probs, offsets, tol_begin, tol_end);
    check(semicrf_marginal_decode_tol(a.score, a.noise, a.v, a.q, a.logZ, a.d.T, a.d.B, a.tau, a.tau_stride, (int)tol_begin, (int)tol_end,
                                      a.pairs, a.probs, a.cap, a.offsets, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_marginal_decode_tol");
}
void marginal_decode_tol_cpu(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, int64_t tol_begin, int64_t tol_end,
                             Tensor pairs, Tensor probs, Tensor offsets, Tensor ws)
{
    all_cpu(score, noise, v, q, logZ, tau, pairs, probs, offsets);
    const MarginalDecodeArgs a = marginal_decode_args(score, noise, v, q, logZ, tau, pairs, probs, offsets, tol_begin, tol_end);
    check_cell_count(a.d);
    if (tol_begin == 0 && tol_end == 0)
        semicrf_cpu::marginal_decode(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.tau, a.tau_stride, a.pairs, a.probs, a.cap, a.offsets);
    else
        semicrf_cpu::marginal_decode_tol(a.score, a.v, a.q, a.logZ, a.d.T, a.d.B, a.tau, a.tau_stride, (int)tol_begin, (int)tol_end, a.pairs,
                                         a.probs, a.cap, a.offsets);
}

// MBR path decoding (semicrf_mbr_select) over a lattice of marginal_decode: pairs [K, 2], weight [K], offsets [B + 1]; tau as above;
// pairs_out [cap, 2], probs_out [cap], offsets_out [B + 1], gain [B]
struct MbrArgs { int64_t K, cap; int B; const int32_t* pairs; const float* weight; const int32_t* offsets; const float* tau; int tau_stride;
                 int32_t* pairs_out; float* probs_out; int32_t* offsets_out; float* gain; };
inline MbrArgs mbr_select_args(const Tensor& pairs, const Tensor& weight, const Tensor& offsets, int64_t T, const Tensor& tau,
                               const Tensor& pairs_out, const Tensor& probs_out, const Tensor& offsets_out, const Tensor& gain)
{
    STD_TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, "semicrf: pairs must be [K, 2]");
    STD_TORCH_CHECK(pairs_out.dim() == 2 && pairs_out.size(1) == 2 && pairs_out.size(0) >= 1, "semicrf: pairs_out must be [cap, 2], cap >= 1");
    const int64_t K = pairs.size(0), cap = pairs_out.size(0), B = offsets.numel() - 1;
    STD_TORCH_CHECK(T >= 1 && B >= 1 && T < (1 << 29) && 2 * T * B < (1ll << 31), "semicrf: bad T / offsets size");
    want(pairs, ScalarType::Int, 2 * K, "pairs");
    want(weight, ScalarType::Float, K, "weight");
    want(offsets, ScalarType::Int, B + 1, "offsets");
    want(pairs_out, ScalarType::Int, 2 * cap, "pairs_out");
    want(probs_out, ScalarType::Float, cap, "probs_out");
    want(offsets_out, ScalarType::Int, B + 1, "offsets_out");
    want(gain, ScalarType::Float, B, "gain");
    return MbrArgs{K, cap, (int)B, ip(pairs), cfp(weight), ip(offsets), cfp(tau), tau_stride_of(tau, (int)B), ip(pairs_out), fp(probs_out),
                   ip(offsets_out), fp(gain)};
}
void mbr_select(Tensor pairs, Tensor weight, Tensor offsets, int64_t T, Tensor tau, Tensor pairs_out, Tensor probs_out, Tensor offsets_out,
                Tensor gain, Tensor ws)
{
    Ctx c(offsets); c.same(offsets, pairs, weight, tau, pairs_out, probs_out, offsets_out, gain, ws);
    const MbrArgs a = mbr_select_args(pairs, weight, offsets, T, tau, pairs_out, probs_out, offsets_out, gain);
    check(semicrf_mbr_select(a.pairs, a.weight, a.offsets, a.K, (int)T, a.B, a.tau, a.tau_stride, a.pairs_out, a.probs_out, a.cap,
                             a.offsets_out, a.gain, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_mbr_select");
}
void mbr_select_cpu(Tensor pairs, Tensor weight, Tensor offsets, int64_t T, Tensor tau, Tensor pairs_out, Tensor probs_out,
                    Tensor offsets_out, Tensor gain, Tensor ws)
{
    all_cpu(pairs, weight, offsets, tau, pairs_out, probs_out, offsets_out, gain);
    const MbrArgs a = mbr_select_args(pairs, weight, offsets, T, tau, pairs_out, probs_out, offsets_out, gain);
    semicrf_cpu::mbr_select(a.pairs, a.weight, a.offsets, a.K, (int)T, a.B, a.tau, a.tau_stride, a.pairs_out, a.probs_out, a.cap,
                            a.offsets_out, a.gain);
}

// path comparison (semicrf_compare_paths): two packed lists, pairs [K, 2] / offsets [B + 1] each; stats [B, 7].  The pairs buffers
// must hold offsets[B] entries -- the total lives on the device, so the caller vouches for it (the Python mirror does)
struct ComparePathsArgs { int B; const int32_t *est_pairs, *est_offsets, *ref_pairs, *ref_offsets; int32_t* stats; };
inline ComparePathsArgs compare_paths_args(const Tensor& est_pairs, const Tensor& est_offsets, const Tensor& ref_pairs,
                                           const Tensor& ref_offsets, int64_t T, int64_t tol_begin, int64_t tol_end, const Tensor& stats)
{
    STD_TORCH_CHECK(est_pairs.dim() == 2 && est_pairs.size(1) == 2 && ref_pairs.dim() == 2 && ref_pairs.size(1) == 2,
                    "semicrf: pairs must be [K, 2]");
    const int64_t B = est_offsets.numel() - 1;
    STD_TORCH_CHECK(T >= 1 && B >= 1 && T < (1 << 29) && 7 * B < (1ll << 31), "semicrf: bad T / offsets size");
    STD_TORCH_CHECK(ref_offsets.numel() == B + 1, "semicrf: est_offsets and ref_offsets must have the same length");
    want(est_pairs, ScalarType::Int, 0, "est_pairs");
    want(ref_pairs, ScalarType::Int, 0, "ref_pairs");
    want(est_offsets, ScalarType::Int, B + 1, "est_offsets");
    want(ref_offsets, ScalarType::Int, B + 1, "ref_offsets");
    want(stats, ScalarType::Int, 7 * B, "stats");
    check_tol(tol_begin, tol_end);
    STD_TORCH_CHECK((((uintptr_t)ip(est_pairs) | (uintptr_t)ip(ref_pairs)) & 7) == 0, "semicrf: pairs must be 8-byte aligned");
    return ComparePathsArgs{(int)B, ip(est_pairs), ip(est_offsets), ip(ref_pairs), ip(ref_offsets), ip(stats)};
}
void compare_paths(Tensor est_pairs, Tensor est_offsets, Tensor ref_pairs, Tensor ref_offsets, int64_t T, int64_t tol_begin,
                   int64_t tol_end, Tensor stats)
{
    Ctx c(est_offsets); c.same(est_offsets, est_pairs, ref_pairs, ref_offsets, stats);
    const ComparePathsArgs a = compare_paths_args(est_pairs, est_offsets, ref_pairs, ref_offsets, T, tol_begin, tol_end, stats);
    check(semicrf_compare_paths(a.est_pairs, a.est_offsets, a.ref_pairs, a.ref_offsets, (int)T, a.B, (int)tol_begin, (int)tol_end, a.stats,
                                c.stream),
          "semicrf_compare_paths");
}
void compare_paths_cpu(Tensor est_pairs, Tensor est_offsets, Tensor ref_pairs, Tensor ref_offsets, int64_t T, int64_t tol_begin,
                       int64_t tol_end, Tensor stats)
{
    all_cpu(est_pairs, est_offsets, ref_pairs, ref_offsets, stats);
    const ComparePathsArgs a = compare_paths_args(est_pairs, est_offsets, ref_pairs, ref_offsets, T, tol_begin, tol_end, stats);
    // on the host the totals can be looked at: the promise the device entry point takes from its caller is checked here
    STD_TORCH_CHECK(a.est_offsets[a.B] <= est_pairs.size(0) && a.ref_offsets[a.B] <= ref_pairs.size(0),
                    "semicrf: offsets[B] exceeds the pairs buffer");
    semicrf_cpu::compare_paths(a.est_pairs, a.est_offsets, a.ref_pairs, a.ref_offsets, (int)T, a.B, (int)tol_begin, (int)tol_end, a.stats);
}

struct EvalPathArgs { Dims d; const float *score, *noise; const int32_t *pairs, *offsets; float* out; };
inline EvalPathArgs eval_path_args(const Tensor& score, const Tensor& noise, const Tensor& pairs, int64_t K, const Tensor& offsets,
                                   const Tensor& out)
{
    const Dims d = crf_dims(score, noise);
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    return EvalPathArgs{d, cfp(score), cfp(noise), i32(pairs, 2 * K, "pairs"), i32(offsets, d.B + 1, "offsets"), f32w(out, d.B, "out")};
}
void eval_path(Tensor score, Tensor noise, Tensor pairs, int64_t K, Tensor offsets, Tensor out, Tensor ws)
{
    Ctx c(score); c.same(score, noise, pairs, offsets, out);
    const EvalPathArgs a = eval_path_args(score, noise, pairs, K, offsets, out);
    check(semicrf_eval_path(a.score, a.noise, a.d.T, a.d.B, a.pairs, K, a.offsets, a.out, ws.numel() > 0 ? ws.data_ptr() : nullptr,
                            (size_t)ws.numel(), c.stream),
          "semicrf_eval_path");
}
void eval_path_cpu(Tensor score, Tensor noise, Tensor pairs, int64_t K, Tensor offsets, Tensor out, Tensor ws)
{
    all_cpu(score, noise, pairs, offsets, out);
    const EvalPathArgs a = eval_path_args(score, noise, pairs, K, offsets, out);
    check_path(a.pairs, K, a.offsets, a.d.T, a.d.B);
    semicrf_cpu::eval_path(a.score, a.noise, a.d.T, a.d.B, a.pairs, a.offsets, a.out);
}
struct EvalPathBwdArgs { const float* gout; const int32_t *pairs, *offsets; float *dScore, *dNoise; };      // dScore / dNoise: null when absent
inline EvalPathBwdArgs eval_path_bwd_args(const Tensor& gout, int64_t T, int64_t B, const Tensor& pairs, int64_t K, const Tensor& offsets,
                                          const Tensor& dScore, bool has_ds, const Tensor& dNoise, bool has_dn)
{
    STD_TORCH_CHECK(T >= 1 && B >= 1 && K >= 0 && T < (1 << 29) && B < (1ll << 31), "semicrf: bad sizes");
    return EvalPathBwdArgs{f32(gout, B, "gout"), i32(pairs, 2 * K, "pairs"), i32(offsets, B + 1, "offsets"),
                           has_ds ? f32w(dScore, T * T * B, "dScore") : nullptr, has_dn ? f32w(dNoise, (T - 1) * B, "dNoise") : nullptr};
}
void eval_path_bwd(Tensor gout, int64_t T, int64_t B, Tensor pairs, int64_t K, Tensor offsets, Tensor dScore, bool has_ds, Tensor dNoise,
                   bool has_dn)
{
    Ctx c(gout); c.same(gout, pairs, offsets);
    if (has_ds) c.same(gout, dScore);
    if (has_dn) c.same(gout, dNoise);
    const EvalPathBwdArgs a = eval_path_bwd_args(gout, T, B, pairs, K, offsets, dScore, has_ds, dNoise, has_dn);
    check(semicrf_eval_path_bwd(a.gout, (int)T, (int)B, a.pairs, K, a.offsets, a.dScore, a.dNoise, c.stream), "semicrf_eval_path_bwd");
}
void eval_path_bwd_cpu(Tensor gout, int64_t T, int64_t B, Tensor pairs, int64_t K, Tensor offsets, Tensor dScore, bool has_ds, Tensor dNoise,
                       bool has_dn)
{
    all_cpu(gout, pairs, offsets);                                 // (unlike the GPU twin, dScore / dNoise are not in this list)
    const EvalPathBwdArgs a = eval_path_bwd_args(gout, T, B, pairs, K, offsets, dScore, has_ds, dNoise, has_dn);
    check_path(a.pairs, K, a.offsets, (int)T, (int)B);
    semicrf_cpu::eval_path_bwd(a.gout, (int)T, (int)B, a.pairs, a.offsets, a.dScore, a.dNoise);
}

// logProb as one call each way (semicrf_logprob_fwd / _bwd): gout holds B values (gstride 1) or ONE (gstride 0)
// ptab / has_ptab: the path table of semicrf_logprob_fwd_t / _bwd_t (int32 [T][B]; has_ptab false: none, pass any int32 tensor).
// It belongs to the GPU twins: the CPU kernels scatter the path's terms themselves, a path table is refused there, not ignored.
struct LogprobFwdArgs { Dims d; const float *score, *noise; const int32_t *pairs, *offsets; float *logProb, *logZ, *v; };
inline LogprobFwdArgs logprob_fwd_args(const Tensor& score, const Tensor& noise, const Tensor& pairs, int64_t K, const Tensor& offsets,
                                       const Tensor& logProb, const Tensor& logZ, const Tensor& v, bool want_v)
{
    const Dims d = crf_dims(score, noise);
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    return LogprobFwdArgs{d, cfp(score), cfp(noise), i32(pairs, 2 * K, "pairs"), i32(offsets, d.B + 1, "offsets"), f32w(logProb, d.B, "logProb"),
                          f32w(logZ, d.B, "logZ"), want_v ? f32w(v, (int64_t)d.T * d.B, "v") : nullptr};
}
void logprob_fwd(Tensor score, Tensor noise, Tensor pairs, int64_t K, Tensor offsets, Tensor logProb, Tensor logZ, Tensor v, bool want_v,
                 Tensor ws, Tensor ptab, bool has_ptab)
{
    Ctx c(score); c.same(score, noise, pairs, offsets, logProb, logZ, v, ws);
    if (has_ptab) c.same(score, ptab);
    const LogprobFwdArgs a = logprob_fwd_args(score, noise, pairs, K, offsets, logProb, logZ, v, want_v);
    check(semicrf_logprob_fwd_t(a.score, a.noise, a.d.T, a.d.B, a.pairs, K, a.offsets, a.logProb, a.logZ, a.v,
                                has_ptab ? i32(ptab, (int64_t)a.d.T * a.d.B, "ptab") : nullptr, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_logprob_fwd");
}
void logprob_fwd_cpu(Tensor score, Tensor noise, Tensor pairs, int64_t K, Tensor offsets, Tensor logProb, Tensor logZ, Tensor v, bool want_v,
                     Tensor ws, Tensor ptab, bool has_ptab)
{
    STD_TORCH_CHECK(!has_ptab, "semicrf: the path table belongs to the GPU sweeps");
    all_cpu(score, noise, logZ, v, pairs, offsets, logProb);
    const LogprobFwdArgs a = logprob_fwd_args(score, noise, pairs, K, offsets, logProb, logZ, v, want_v);
    check_path(a.pairs, K, a.offsets, a.d.T, a.d.B);
    std::vector<float> scratch;
    if (!want_v) scratch.resize((size_t)a.d.T * a.d.B);
    semicrf_cpu::logz_fwd(a.score, a.noise, a.d.T, a.d.B, a.logZ, want_v ? a.v : scratch.data());
    semicrf_cpu::eval_path(a.score, a.noise, a.d.T, a.d.B, a.pairs, a.offsets, a.logProb);
    for (int c = 0; c < a.d.B; ++c) a.logProb[c] -= a.logZ[c];
}
struct LogprobBwdArgs { Dims d; const float *score, *noise, *v, *logZ, *gout; const int32_t *pairs, *offsets; float *dScore, *dNoise; };
inline LogprobBwdArgs logprob_bwd_args(const Tensor& score, const Tensor& noise, const Tensor& v, const Tensor& logZ, const Tensor& gout,
                                       int64_t gstride, const Tensor& pairs, int64_t K, const Tensor& offsets, const Tensor& dScore,
                                       const Tensor& dNoise)
{
    const Dims d = crf_dims(score, noise);
    const int64_t TB = (int64_t)d.T * d.B;
    STD_TORCH_CHECK(K >= 0 && (gstride == 0 || gstride == 1), "semicrf: bad interval count / gout stride");
    return LogprobBwdArgs{d, cfp(score), cfp(noise), f32(v, TB, "v"), f32(logZ, d.B, "logZ"), f32(gout, gstride ? d.B : 1, "gout"),
                          i32(pairs, 2 * K, "pairs"), i32(offsets, d.B + 1, "offsets"), f32w(dScore, TB * d.T, "dScore"),
                          f32w(dNoise, TB - d.B, "dNoise")};
}
void logprob_bwd(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, int64_t gstride, Tensor pairs, int64_t K, Tensor offsets,
                 Tensor dScore, Tensor dNoise, int64_t flags, Tensor ws, Tensor ptab, bool has_ptab)
{
    Ctx c(score); c.same(score, noise, v, logZ, gout, pairs, offsets, dScore, dNoise, ws);
    if (has_ptab) c.same(score, ptab);
    const LogprobBwdArgs a = logprob_bwd_args(score, noise, v, logZ, gout, gstride, pairs, K, offsets, dScore, dNoise);
    check(semicrf_logprob_bwd_t(a.score, a.noise, a.v, a.logZ, a.gout, (int)gstride, a.d.T, a.d.B, a.pairs, K, a.offsets, a.dScore, a.dNoise,
                                (int)flags, has_ptab ? i32(ptab, (int64_t)a.d.T * a.d.B, "ptab") : nullptr, bytes(ws, "ws"),
                                (size_t)ws.numel(), c.stream),
          "semicrf_logprob_bwd");
}
void logprob_bwd_cpu(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, int64_t gstride, Tensor pairs, int64_t K, Tensor offsets,
                     Tensor dScore, Tensor dNoise, int64_t flags, Tensor ws, Tensor ptab, bool has_ptab)
{
    STD_TORCH_CHECK(!has_ptab, "semicrf: the path table belongs to the GPU sweeps");
    all_cpu(score, noise, v, logZ, gout, pairs, offsets, dScore, dNoise);
    const LogprobBwdArgs a = logprob_bwd_args(score, noise, v, logZ, gout, gstride, pairs, K, offsets, dScore, dNoise);
    check_path(a.pairs, K, a.offsets, a.d.T, a.d.B);
    std::vector<float> gp((size_t)a.d.B), gn((size_t)a.d.B), q((size_t)a.d.T * a.d.B);
    for (int c = 0; c < a.d.B; ++c) { gp[(size_t)c] = a.gout[(size_t)c * gstride]; gn[(size_t)c] = -gp[(size_t)c]; }
    semicrf_cpu::logz_bwd(a.score, a.noise, a.v, a.logZ, gn.data(), a.d.T, a.d.B, a.dScore, a.dNoise, q.data());
    semicrf_cpu::eval_path_bwd(gp.data(), a.d.T, a.d.B, a.pairs, a.offsets, a.dScore, a.dNoise);
}

// ---- interval scorer ---------------------------------------------------------------------------------------------------
// q / k / diag (and their gradients) are strided views ([C][T][D] rows of ld floats): dtype and the device are checked, the
// strides are the caller's statement; everything dense is checked for its element count.
inline const float* f32s(const Tensor& t, const char* name)
{
    STD_TORCH_CHECK(t.defined() && t.scalar_type() == ScalarType::Float, "semicrf: `", name, "` must be a float32 tensor");
    return t.numel() > 0 ? (const float*)t.data_ptr() : nullptr;
}
inline float* f32so(const Tensor& t, const char* name) { return t.defined() && t.numel() > 0 ? (float*)f32s(t, name) : nullptr; }
inline void score_dims(int64_t C, int64_t T, int64_t D)
{
    STD_TORCH_CHECK(C >= 1 && T >= 1 && D >= 1 && C < (1ll << 31) && T < (1 << 29) && D < (1 << 20), "semicrf: bad C / T / D");
}
inline int64_t slots_of(int64_t C, int64_t group, int64_t pitch)
{
    STD_TORCH_CHECK(group >= 1 && pitch >= group && C % group == 0 && group < (1ll << 31) && pitch < (1ll << 31), "semicrf: bad slot layout");
    return C / group * pitch;
}
// rowc / drowc (merged projection, *_pc entry points): strided [C][T] views, stride ldrc; ldrc == 0: none
void interval_score_fwd_op(Tensor q, Tensor k, Tensor diag, Tensor rowc, int64_t C, int64_t T, int64_t D, int64_t ldq, int64_t ldk,
                           int64_t ldd, int64_t ldrc, double qscale, int64_t mode, int64_t full, int64_t group, int64_t pitch, Tensor S,
                           Tensor noise)
{
    Ctx c(q); c.same(q, k, diag, rowc, S, noise);
    score_dims(C, T, D);
    const int64_t Cs = slots_of(C, group, pitch);
    check(interval_score_fwd_pc(f32s(q, "q"), f32s(k, "k"), f32s(diag, "diag"), ldrc > 0 ? f32s(rowc, "rowc") : nullptr, (int)C, (int)T, (int)D,
                                ldq, ldk, ldd, ldrc > 0 ? ldrc : 1, (float)qscale, (int)mode, (int)full, (int)group, (int)pitch,
                                f32w(S, T * T * Cs, "S"), noise.numel() > 0 ? f32w(noise, (T - 1) * Cs, "noise") : nullptr, c.stream),
          "interval_score_fwd");
}
void interval_score_bwd_ws_op(Tensor dS, Tensor q, Tensor k, int64_t C, int64_t T, int64_t D, int64_t ldq, int64_t ldk, double qscale,
                              int64_t mode, int64_t group, int64_t pitch, Tensor dq, Tensor dk, Tensor ddiag, Tensor drowc, int64_t lddq,
                              int64_t lddk, int64_t lddd, int64_t lddrc, Tensor ws)
{
    Ctx c(dS); c.same(dS, q, k, dq, dk, ddiag, drowc, ws);
    score_dims(C, T, D);
    const int64_t Cs = slots_of(C, group, pitch);
    check(interval_score_bwd_ws_pc(f32(dS, T * T * Cs, "dS"), f32s(q, "q"), f32s(k, "k"), (int)C, (int)T, (int)D, ldq, ldk, (float)qscale,
                                   (int)mode, (int)group, (int)pitch, f32so(dq, "dq"), f32so(dk, "dk"), f32so(ddiag, "ddiag"),
                                   lddrc > 0 ? f32so(drowc, "drowc") : nullptr, lddq, lddk, lddd, lddrc > 0 ? lddrc : 1, bytes(ws, "ws"),
                                   (size_t)ws.numel(), c.stream),
          "interval_score_bwd_ws");
}
void interval_score_bwd_fused_ws_op(Tensor S, Tensor alpha, Tensor beta_, Tensor logZ, Tensor gout, Tensor q, Tensor k, int64_t C, int64_t T,
                                    int64_t D, int64_t ldq, int64_t ldk, double qscale, int64_t mode, int64_t group, int64_t pitch, Tensor dq,
                                    Tensor dk, Tensor ddiag, Tensor drowc, int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc, Tensor ws)
{
    Ctx c(S); c.same(S, alpha, beta_, logZ, gout, q, k, dq, dk, ddiag, drowc, ws);
    score_dims(C, T, D);
    const int64_t Cs = slots_of(C, group, pitch);
    check(interval_score_bwd_fused_ws_pc(f32(S, T * T * Cs, "S"), f32(alpha, T * Cs, "alpha"), f32(beta_, T * Cs, "beta"),
                                         f32(logZ, Cs, "logZ"), f32(gout, Cs, "gout"), f32s(q, "q"), f32s(k, "k"), (int)C, (int)T, (int)D, ldq,
                                         ldk, (float)qscale, (int)mode, (int)group, (int)pitch, f32so(dq, "dq"), f32so(dk, "dk"),
                                         f32so(ddiag, "ddiag"), lddrc > 0 ? f32so(drowc, "drowc") : nullptr, lddq, lddk, lddd,
                                         lddrc > 0 ? lddrc : 1, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "interval_score_bwd_fused_ws");
}
void interval_score_path_bwd_op(Tensor gout, Tensor pairs, int64_t K, Tensor offsets, Tensor q, Tensor k, int64_t C, int64_t T, int64_t D,
                                int64_t ldq, int64_t ldk, double qscale, int64_t mode, int64_t group, int64_t pitch, Tensor dq, Tensor dk,
                                Tensor ddiag, Tensor drowc, int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc)
{
    Ctx c(gout); c.same(gout, pairs, offsets, q, k, dq, dk, ddiag, drowc);
    score_dims(C, T, D);
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    const int64_t Cs = slots_of(C, group, pitch);
    check(interval_score_path_bwd_pc(f32(gout, Cs, "gout"), i32(pairs, 2 * K, "pairs"), K, i32(offsets, Cs + 1, "offsets"), f32s(q, "q"),
                                     f32s(k, "k"), (int)C, (int)T, (int)D, ldq, ldk, (float)qscale, (int)mode, (int)group, (int)pitch,
                                     f32so(dq, "dq"), f32so(dk, "dk"), f32so(ddiag, "ddiag"), lddrc > 0 ? f32so(drowc, "drowc") : nullptr, lddq,
                                     lddk, lddd, lddrc > 0 ? lddrc : 1, c.stream),
          "interval_score_path_bwd");
}

// ---- attribute-head features ------------------------------------------------------------------------------------------
// the scorer's projection (csrc/proj_gemm.hip): strided row-major matrices, the strides are the caller's statement
void proj_nn_op(Tensor A, int64_t lda, int64_t M, int64_t K, Tensor B, int64_t ldb, int64_t N, Tensor out, int64_t ldout, Tensor bias,
                bool has_bias, Tensor w2, Tensor b2, bool has_w2, int64_t zero_cols, bool accumulate)
{
    Ctx c(A); c.same(A, B, out);
    if (has_bias) c.same(A, bias);
    if (has_w2) c.same(A, w2, b2);
    STD_TORCH_CHECK(M >= 1 && K >= 4 && N >= 1 && M < (1ll << 31) && K < (1 << 20) && N <= 256, "semicrf: bad M / K / N");
    STD_TORCH_CHECK(A.numel() >= (M - 1) * lda + K && out.numel() >= (M - 1) * ldout + N + (has_w2 ? 2 + zero_cols : 0), "semicrf: A / out too small");
    STD_TORCH_CHECK(B.numel() >= ((K + 31) / 32 * 32 - 1) * ldb + N, "semicrf: B must hold whole chunks of 32 rows (zero beyond K)");
    check(scorer_proj_nn(f32s(A, "A"), lda, M, (int)K, f32s(B, "B"), ldb, (int)N, f32so(out, "out"), ldout, has_bias ? f32(bias, N, "bias") : nullptr,
                         has_w2 ? f32(w2, 2 * K, "w2") : nullptr, has_w2 ? f32(b2, 2, "b2") : nullptr, (int)zero_cols, accumulate ? 1 : 0, c.stream),
          "scorer_proj_nn");
}
void proj_nn3_op(Tensor A, int64_t lda, int64_t M, int64_t K, Tensor B, int64_t ldb, int64_t N, Tensor out, int64_t ldout, Tensor bias,
                 bool has_bias, Tensor w2, Tensor b2, bool has_w2, int64_t zero_cols, bool accumulate, Tensor ws)
{
    Ctx c(A); c.same(A, B, out, ws);
    if (has_bias) c.same(A, bias);
    if (has_w2) c.same(A, w2, b2);
    STD_TORCH_CHECK(M >= 1 && K >= 4 && N >= 1 && M < (1ll << 31) && K < (1 << 20) && N <= 256, "semicrf: bad M / K / N");
    STD_TORCH_CHECK(A.numel() >= (M - 1) * lda + K && out.numel() >= (M - 1) * ldout + N + (has_w2 ? 2 + zero_cols : 0), "semicrf: A / out too small");
    STD_TORCH_CHECK(B.numel() >= ((K + 31) / 32 * 32 - 1) * ldb + N, "semicrf: B must hold whole chunks of 32 rows (zero beyond K)");
    check(scorer_proj_nn3(f32s(A, "A"), lda, M, (int)K, f32s(B, "B"), ldb, (int)N, f32so(out, "out"), ldout, has_bias ? f32(bias, N, "bias") : nullptr,
                          has_w2 ? f32(w2, 2 * K, "w2") : nullptr, has_w2 ? f32(b2, 2, "b2") : nullptr, (int)zero_cols, accumulate ? 1 : 0,
                          ws.numel() ? ws.data_ptr() : nullptr, (size_t)ws.numel() * ws.element_size(), c.stream),
          "scorer_proj_nn3");
}
void proj_tn_op(Tensor dy, int64_t lddy, int64_t M, int64_t R, int64_t extra_col0, int64_t total_rows, Tensor x, int64_t ldx, int64_t N, Tensor dW,
                int64_t lddw, Tensor db, Tensor ws)
{
    Ctx c(dy); c.same(dy, x, dW, db, ws);
    const int64_t x3flag = total_rows & SEMICRF_PROJ_TN_BF16X3;  // opt-in: the matrix part on the three-limb bf16 kernel
    total_rows &= ~(int64_t)SEMICRF_PROJ_TN_BF16X3;
    STD_TORCH_CHECK(M >= 1 && R >= 1 && N >= 1 && N <= 256 && M < (1ll << 31) && total_rows >= R && total_rows < (1 << 20), "semicrf: bad sizes");
    STD_TORCH_CHECK(dy.numel() >= (M - 1) * lddy + R && x.numel() >= (M - 1) * ldx + N && dW.numel() >= (total_rows - 1) * lddw + N,
                    "semicrf: dy / x / dW too small");
    check(scorer_proj_tn(f32s(dy, "dy"), lddy, M, (int)R, (int)extra_col0, (int)(total_rows | x3flag), f32s(x, "x"), ldx, (int)N, f32so(dW, "dW"), lddw,
                         f32w(db, total_rows, "db"), bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "scorer_proj_tn");
}

void stage_linear_op(Tensor W, Tensor bias, int64_t D, int64_t size, int64_t rows_pad, Tensor BT, Tensor Wqd, Tensor w2, Tensor b2)
{
    Ctx c(W); c.same(W, bias, BT, Wqd); c.same(W, w2, b2);
    STD_TORCH_CHECK(D >= 1 && size >= 1 && rows_pad >= D + 1 && rows_pad < (1 << 20) && D < (1 << 20) && size < (1 << 20), "semicrf: bad D / size / rows_pad");
    check(scorer_stage_linear(f32(W, (2 * D + 1) * size, "W"), f32(bias, 2 * D + 1, "bias"), (int)D, (int)size, (int)rows_pad,
                              f32w(BT, size * 2 * D, "BT"), f32w(Wqd, rows_pad * size, "Wqd"), f32w(w2, 2 * size, "w2"), f32w(b2, 2, "b2"), c.stream),
          "scorer_stage_linear");
}
void merge_weights_fwd_op(Tensor W, Tensor bias, int64_t D, int64_t size, int64_t rows, Tensor Wm, Tensor bm, Tensor WmT, bool has_t)
{
    Ctx c(W); c.same(W, bias, Wm, bm);
    if (has_t) c.same(W, WmT);
    STD_TORCH_CHECK(D >= 1 && size >= 1 && size <= 256 && rows >= size + 2 && rows < (1 << 20), "semicrf: bad D / size / rows");
    check(scorer_merge_weights_fwd(f32(W, (2 * D + 1) * size, "W"), f32(bias, 2 * D + 1, "bias"), (int)D, (int)size, (int)rows,
                                   f32w(Wm, rows * size, "Wm"), f32w(bm, rows, "bm"), has_t ? f32w(WmT, size * size, "WmT") : nullptr, c.stream),
          "scorer_merge_weights_fwd");
}
void merge_weights_bwd_op(Tensor W, Tensor bias, Tensor dWm, Tensor dbm, int64_t D, int64_t size, int64_t rows, Tensor dW, Tensor dbias, Tensor ws)
{
    Ctx c(W); c.same(W, bias, dWm, dbm); c.same(W, dW, dbias, ws);
    STD_TORCH_CHECK(D >= 1 && size >= 1 && size <= 256 && rows >= size + 2 && rows < (1 << 20), "semicrf: bad D / size / rows");
    check(scorer_merge_weights_bwd(f32(W, (2 * D + 1) * size, "W"), f32(bias, 2 * D + 1, "bias"), f32(dWm, rows * size, "dWm"),
                                   f32(dbm, rows, "dbm"), (int)D, (int)size, (int)rows, f32w(dW, (2 * D + 1) * size, "dW"),
                                   f32w(dbias, 2 * D + 1, "dbias"), bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "scorer_merge_weights_bwd");
}

void interval_features_gather_op(Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K, Tensor offsets,
                                 int64_t nSym, Tensor out, Tensor symIdx, Tensor scatterIdx)
{
    Ctx c(ctx); c.same(ctx, pairs, offsets, out, symIdx, scatterIdx);
    score_dims(C, T, D);
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    want(symIdx, ScalarType::Long, K, "symIdx"); want(scatterIdx, ScalarType::Long, K, "scatterIdx");
    check(interval_features_gather(f32s(ctx, "ctx"), (int)C, (int)T, (int)D, ldc, i32(pairs, 2 * K, "pairs"), K, i32(offsets, C + 1, "offsets"),
                                   (int)nSym, f32w(out, K * 3 * D, "out"), K > 0 ? (int64_t*)symIdx.data_ptr() : nullptr,
                                   K > 0 ? (int64_t*)scatterIdx.data_ptr() : nullptr, c.stream),
          "interval_features_gather");
}
void interval_features_gather_bwd_op(Tensor gout, Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K,
                                     Tensor offsets, Tensor dctx, int64_t lddc)
{
    Ctx c(gout); c.same(gout, ctx, pairs, offsets, dctx);
    score_dims(C, T, D);
    STD_TORCH_CHECK(K >= 0, "semicrf: negative interval count");
    check(interval_features_gather_bwd(f32(gout, K * 3 * D, "gout"), f32s(ctx, "ctx"), (int)C, (int)T, (int)D, ldc, i32(pairs, 2 * K, "pairs"),
                                       K, i32(offsets, C + 1, "offsets"), (float*)f32s(dctx, "dctx"), lddc, c.stream),
          "interval_features_gather_bwd");
}

// ---- attribute-head training loss (semicrf_attribute_loss_fwd / _bwd) ---------------------------------------------------
struct AttrLossArgs { const float *lv, *of, *r, *p; const int32_t *vel, *off; };
inline AttrLossArgs attr_loss_args(const Tensor& logitsVelocity, const Tensor& ofLogits, const Tensor& velocity, const Tensor& ofRefined,
                                   const Tensor& ofPresence, int64_t K, const Tensor& offsets, int64_t C)
{
    STD_TORCH_CHECK(K >= 0 && K < (1ll << 31) && C >= 1 && C < (1ll << 31), "semicrf: bad interval / chain count");
    return AttrLossArgs{f32(logitsVelocity, K * 128, "logitsVelocity"), f32(ofLogits, K * 4, "ofLogits"), f32(ofRefined, K * 2, "ofRefined"),
                        f32(ofPresence, K * 2, "ofPresence"), i32(velocity, K, "velocity"), i32(offsets, C + 1, "offsets")};
}
void attribute_loss_fwd_op(Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined, Tensor ofPresence, int64_t K,
                           Tensor offsets, int64_t C, Tensor base, bool has_base, Tensor rowLogProb, Tensor out)
{
    Ctx c(out); c.same(out, logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, rowLogProb);
    if (has_base) c.same(out, base);
    const AttrLossArgs a = attr_loss_args(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, K, offsets, C);
    check(semicrf_attribute_loss_fwd(a.lv, a.of, a.vel, a.r, a.p, K, a.off, (int)C, has_base ? f32(base, C, "base") : nullptr,
                                     f32w(rowLogProb, K, "rowLogProb"), f32w(out, C, "out"), c.stream),
          "semicrf_attribute_loss_fwd");
}
void attribute_loss_bwd_op(Tensor gout, int64_t gstride, Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined,
                           Tensor ofPresence, int64_t K, Tensor offsets, int64_t C, Tensor dLogitsVelocity, Tensor dOfLogits)
{
    Ctx c(gout); c.same(gout, logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, dLogitsVelocity, dOfLogits);
    STD_TORCH_CHECK(gstride == 0 || gstride == 1, "semicrf: bad gout stride");
    const AttrLossArgs a = attr_loss_args(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, K, offsets, C);
    check(semicrf_attribute_loss_bwd(f32(gout, gstride ? C : 1, "gout"), (int)gstride, a.lv, a.of, a.vel, a.r, a.p, K, a.off, (int)C,
                                     f32w(dLogitsVelocity, K * 128, "dLogitsVelocity"), f32w(dOfLogits, K * 4, "dOfLogits"), c.stream),
          "semicrf_attribute_loss_bwd");
}
// the same two on CPU tensors (cpu_ops.cpp); the offsets are checked here: the host kernels index with them
inline void check_offsets(const int32_t* off, int64_t K, int64_t C)
{
    STD_TORCH_CHECK(off[0] == 0 && off[C] == K, "semicrf: offsets must run from 0 to K");
    for (int64_t c = 0; c < C; ++c) STD_TORCH_CHECK(off[c] <= off[c + 1], "semicrf: offsets must not decrease");
}
void attribute_loss_fwd_cpu(Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined, Tensor ofPresence, int64_t K,
                            Tensor offsets, int64_t C, Tensor base, bool has_base, Tensor rowLogProb, Tensor out)
{
    all_cpu(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, rowLogProb, out);
    if (has_base) all_cpu(base);
    const AttrLossArgs a = attr_loss_args(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, K, offsets, C);
    const float* b = has_base ? f32(base, C, "base") : nullptr;
    float* rows = f32w(rowLogProb, K, "rowLogProb");
    float* o = f32w(out, C, "out");
    if (K == 0) return;
    check_offsets(a.off, K, C);
    semicrf_cpu::attribute_loss_fwd(a.lv, a.of, a.vel, a.r, a.p, K, a.off, (int)C, b, rows, o);
}
void attribute_loss_bwd_cpu(Tensor gout, int64_t gstride, Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined,
                            Tensor ofPresence, int64_t K, Tensor offsets, int64_t C, Tensor dLogitsVelocity, Tensor dOfLogits)
{
    all_cpu(gout, logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, dLogitsVelocity, dOfLogits);
    STD_TORCH_CHECK(gstride == 0 || gstride == 1, "semicrf: bad gout stride");
    const AttrLossArgs a = attr_loss_args(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, K, offsets, C);
    const float* g = f32(gout, gstride ? C : 1, "gout");
    float* dlv = f32w(dLogitsVelocity, K * 128, "dLogitsVelocity");
    float* dof = f32w(dOfLogits, K * 4, "dOfLogits");
    if (K == 0) return;
    check_offsets(a.off, K, C);
    semicrf_cpu::attribute_loss_bwd(g, (int)gstride, a.lv, a.of, a.vel, a.r, a.p, K, a.off, (int)C, dlv, dof);
}

// ---- the optimizer step (semicrf_grad_sqnorm / semicrf_clip_from_history / semicrf_adabelief_step) ---------------------------------
// table: a HOST tensor, float64 [n_groups][10] = {end, decay, b1, 1-b1, b2, 1-b2, eps, sqrt_bc2, step, rectified}, the factors already
// rounded to fp32 by the caller (a double holds an fp32 and an element count exactly): it becomes the by-value struct of the C ABI
inline semicrf_adabelief_groups optim_groups(const Tensor& table, int64_t numel)
{
    STD_TORCH_CHECK(table.defined() && table.is_cpu() && table.scalar_type() == ScalarType::Double && table.is_contiguous() &&
                    table.dim() == 2 && table.size(1) == 10, "semicrf: the group table must be a contiguous host float64 [n][10] tensor");
    const int64_t n = table.size(0);
    STD_TORCH_CHECK(n >= 1 && n <= SEMICRF_OPTIM_MAX_GROUPS, "semicrf: ", n, " parameter groups, at most ", SEMICRF_OPTIM_MAX_GROUPS, " fit");
    semicrf_adabelief_groups G{};
    G.n = (int32_t)n;
    const double* t = (const double*)table.data_ptr();
    int64_t last = 0;
    for (int64_t i = 0; i < n; ++i, t += 10) {
        semicrf_adabelief_group& k = G.g[i];
        k.end = (int64_t)t[0];
        STD_TORCH_CHECK(k.end > last, "semicrf: parameter group ", i, " is empty or out of order");
        last = k.end;
        k.decay = (float)t[1]; k.b1 = (float)t[2]; k.omb1 = (float)t[3]; k.b2 = (float)t[4]; k.omb2 = (float)t[5]; k.eps = (float)t[6];
        k.sqrt_bc2 = (float)t[7]; k.step = (float)t[8]; k.rectified = t[9] != 0.0;
    }
    STD_TORCH_CHECK(last == numel, "semicrf: the groups cover ", last, " elements, the buffers hold ", numel);
    return G;
}
inline double* f64w(const Tensor& t, int64_t n, const char* name) { want(t, ScalarType::Double, n, name); return (double*)t.data_ptr(); }
inline void numel_ok(int64_t numel) { STD_TORCH_CHECK(numel >= 1 && numel < (1ll << 40), "semicrf: bad element count"); }
inline void history_ok(const Tensor& ring, int64_t capacity, const Tensor& state, const Tensor& stats)
{
    STD_TORCH_CHECK(capacity >= 1 && capacity <= SEMICRF_HISTORY_MAX, "semicrf: the history holds 1 to ", SEMICRF_HISTORY_MAX, " values");
    want(ring, ScalarType::Float, capacity, "ring"); want(state, ScalarType::Int, 2, "state"); want(stats, ScalarType::Float, 3, "stats");
}
void grad_sqnorm_op(Tensor flat, int64_t numel, Tensor partials)
{
    Ctx c(flat); c.same(flat, partials);
    numel_ok(numel);
    check(semicrf_grad_sqnorm(f32(flat, numel, "flat"), numel, f64w(partials, SEMICRF_SQNORM_MAX_PARTIALS, "partials"), c.stream),
          "semicrf_grad_sqnorm");
}
void clip_from_history_op(Tensor partials, bool has_partials, int64_t numel, Tensor norm_in, bool has_norm, double q, Tensor ring,
                          int64_t capacity, Tensor state, bool append, Tensor stats)
{
    Ctx c(ring); c.same(ring, state, stats);
    if (has_partials) { c.same(ring, partials); numel_ok(numel); }
    if (has_norm) c.same(ring, norm_in);
    history_ok(ring, capacity, state, stats);
    check(semicrf_clip_from_history(has_partials ? f64w(partials, SEMICRF_SQNORM_MAX_PARTIALS, "partials") : nullptr, numel,
                                    has_norm ? f32(norm_in, 1, "norm_in") : nullptr, q, f32w(ring, capacity, "ring"), (int)capacity,
                                    i32(state, 2, "state"), append ? 1 : 0, f32w(stats, 3, "stats"), c.stream),
          "semicrf_clip_from_history");
}
void adabelief_step_op(Tensor p, Tensor g, Tensor m, Tensor s, int64_t numel, Tensor coef, bool has_coef, Tensor table)
{
    Ctx c(p); c.same(p, g, m, s);
    if (has_coef) c.same(p, coef);
    numel_ok(numel);
    const semicrf_adabelief_groups G = optim_groups(table, numel);
    check(semicrf_adabelief_step(f32w(p, numel, "p"), f32(g, numel, "g"), f32w(m, numel, "m"), f32w(s, numel, "s"), numel,
                                 has_coef ? f32(coef, 1, "coef") : nullptr, G, c.stream),
          "semicrf_adabelief_step");
}
void grad_sqnorm_cpu(Tensor flat, int64_t numel, Tensor partials)
{
    all_cpu(flat, partials);
    numel_ok(numel);
    semicrf_cpu::grad_sqnorm(f32(flat, numel, "flat"), numel, f64w(partials, SEMICRF_SQNORM_MAX_PARTIALS, "partials"));
}
void clip_from_history_cpu(Tensor partials, bool has_partials, int64_t numel, Tensor norm_in, bool has_norm, double q, Tensor ring,
                           int64_t capacity, Tensor state, bool append, Tensor stats)
{
    all_cpu(ring, state, stats);
    if (has_partials) { all_cpu(partials); numel_ok(numel); }
    if (has_norm) all_cpu(norm_in);
    history_ok(ring, capacity, state, stats);
    STD_TORCH_CHECK(q < 0.0 || q <= 1.0, "semicrf: the quantile must lie in [0, 1]");
    semicrf_cpu::clip_from_history(has_partials ? f64w(partials, SEMICRF_SQNORM_MAX_PARTIALS, "partials") : nullptr, numel,
                                   has_norm ? f32(norm_in, 1, "norm_in") : nullptr, q, f32w(ring, capacity, "ring"), (int)capacity,
                                   i32(state, 2, "state"), append ? 1 : 0, f32w(stats, 3, "stats"));
}
void adabelief_step_cpu(Tensor p, Tensor g, Tensor m, Tensor s, int64_t numel, Tensor coef, bool has_coef, Tensor table)
{
    all_cpu(p, g, m, s);
    if (has_coef) all_cpu(coef);
    numel_ok(numel);
    const semicrf_adabelief_groups G = optim_groups(table, numel);
    semicrf_cpu::adabelief_step(f32w(p, numel, "p"), f32(g, numel, "g"), f32w(m, numel, "m"), f32w(s, numel, "s"), numel,
                                has_coef ? f32(coef, 1, "coef") : nullptr, G);
}

// ---- attribute-head readout of transcription (semicrf_attribute_decode) ---------------------------------------------------
// velocityClass (int64 [K]) for the class criteria, velocityMean (fp32 [K]) for mse; the other is passed empty and not written
struct AttrDecodeArgs { const float *lv, *of; int64_t* cls; float *mean, *val; unsigned char* pres; };
inline AttrDecodeArgs attr_decode_args(const Tensor& logitsVelocity, const Tensor& ofLogits, int64_t K, int64_t criterion, const Tensor& velocityClass,
                                       const Tensor& velocityMean, const Tensor& ofValue, const Tensor& ofPresence)
{
    STD_TORCH_CHECK(K >= 0 && K < (1ll << 31), "semicrf: bad row count");
    STD_TORCH_CHECK(criterion >= SEMICRF_VEL_HAMMING && criterion <= SEMICRF_VEL_MAE, "semicrf: unknown velocity criterion");
    const bool mse = criterion == SEMICRF_VEL_MSE;
    want(velocityClass, ScalarType::Long, mse ? 0 : K, "velocityClass");
    want(ofPresence, ScalarType::Byte, 2 * K, "ofPresence");
    return AttrDecodeArgs{f32(logitsVelocity, K * 128, "logitsVelocity"), f32(ofLogits, K * 4, "ofLogits"),
                          mse ? nullptr : (int64_t*)velocityClass.data_ptr(), mse ? f32w(velocityMean, K, "velocityMean") : nullptr,
                          f32w(ofValue, 2 * K, "ofValue"), (unsigned char*)ofPresence.data_ptr()};
}
void attribute_decode_op(Tensor logitsVelocity, Tensor ofLogits, int64_t K, int64_t criterion, Tensor velocityClass, Tensor velocityMean,
                         Tensor ofValue, Tensor ofPresence)
{
    Ctx c(ofValue); c.same(ofValue, logitsVelocity, ofLogits, ofPresence);
    const AttrDecodeArgs a = attr_decode_args(logitsVelocity, ofLogits, K, criterion, velocityClass, velocityMean, ofValue, ofPresence);
    if (K == 0) return;
    check(semicrf_attribute_decode(a.lv, a.of, K, (int)criterion, a.cls, a.mean, a.val, a.pres, c.stream), "semicrf_attribute_decode");
}
void attribute_decode_cpu(Tensor logitsVelocity, Tensor ofLogits, int64_t K, int64_t criterion, Tensor velocityClass, Tensor velocityMean,
                          Tensor ofValue, Tensor ofPresence)
{
    all_cpu(logitsVelocity, ofLogits, velocityClass, velocityMean, ofValue, ofPresence);
    const AttrDecodeArgs a = attr_decode_args(logitsVelocity, ofLogits, K, criterion, velocityClass, velocityMean, ofValue, ofPresence);
    if (K == 0) return;
    semicrf_cpu::attribute_decode(a.lv, a.of, K, (int)criterion, a.cls, a.mean, a.val, a.pres);
}

// ---- the two attribute heads (semicrf_attribute_heads) --------------------------------------------------------------------------
// ctx is a [C, T, D] tensor, possibly a view with rows of ldc >= D floats (its strides are checked against ldc); the packed
// weights and every output are dense and checked for their element counts.  symIdx / scatterIdx: int64 [K], or empty (not written).
struct AttrHeadsArgs { const float *ctx, *W1, *b1, *W2, *b2; const int32_t *pairs, *off; float *lv, *of; int64_t *sym, *sc; };
inline AttrHeadsArgs attr_heads_args(const Tensor& ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, const Tensor& pairs, int64_t K,
                                     const Tensor& offsets, int64_t nSym, const Tensor& W1, const Tensor& b1, const Tensor& W2, const Tensor& b2,
                                     int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, const Tensor& logitsVelocity, const Tensor& ofLogits,
                                     const Tensor& symIdx, const Tensor& scatterIdx)
{
    score_dims(C, T, D);
    STD_TORCH_CHECK(K >= 0 && K < (1ll << 31), "semicrf: bad interval count");
    STD_TORCH_CHECK(nSym >= 1 && ldc >= D, "semicrf: bad nSym / row stride");
    STD_TORCH_CHECK(Hv >= 1 && Ho >= 1 && Nv >= 1 && No >= 1 && Hv < (1 << 21) && Ho < (1 << 21) && Nv < (1 << 20) && No < (1 << 20),
                    "semicrf: bad head sizes");
    STD_TORCH_CHECK(ctx.dim() == 3 && ctx.size(0) == C && ctx.size(1) == T && ctx.size(2) == D, "semicrf: `ctx` must be [C, T, D]");
    STD_TORCH_CHECK((D == 1 || ctx.stride(2) == 1) && (T == 1 || ctx.stride(1) == ldc) && (C == 1 || ctx.stride(0) == T * ldc),
                    "semicrf: `ctx` must be [C][T] rows of ldc floats with unit stride inside a row");
    if (symIdx.numel() > 0) want(symIdx, ScalarType::Long, K, "symIdx");
    if (scatterIdx.numel() > 0) want(scatterIdx, ScalarType::Long, K, "scatterIdx");
    return AttrHeadsArgs{f32s(ctx, "ctx"), f32(W1, 3 * D * (Hv + Ho), "W1"), f32(b1, Hv + Ho, "b1"), f32(W2, Hv * Nv + Ho * No, "W2"),
                         f32(b2, Nv + No, "b2"), i32(pairs, 2 * K, "pairs"), i32(offsets, C + 1, "offsets"),
                         f32w(logitsVelocity, K * Nv, "logitsVelocity"), f32w(ofLogits, K * No, "ofLogits"),
                         symIdx.numel() > 0 ? (int64_t*)symIdx.data_ptr() : nullptr,
                         scatterIdx.numel() > 0 ? (int64_t*)scatterIdx.data_ptr() : nullptr};
}
void attribute_heads_op(Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K, Tensor offsets, int64_t nSym,
                        Tensor W1, Tensor b1, Tensor W2, Tensor b2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, Tensor logitsVelocity,
                        Tensor ofLogits, Tensor symIdx, Tensor scatterIdx, Tensor ws)
{
    Ctx c(ctx); c.same(ctx, pairs, offsets, W1, b1, W2, b2, logitsVelocity, ofLogits, symIdx, scatterIdx, ws);
    const AttrHeadsArgs a = attr_heads_args(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                                            symIdx, scatterIdx);
    if (K == 0) return;
    check(semicrf_attribute_heads(a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, (int)nSym, a.W1, a.b1, a.W2, a.b2, (int)Hv, (int)Ho,
                                  (int)Nv, (int)No, a.lv, a.of, a.sym, a.sc, bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_attribute_heads");
}
void attribute_heads_cpu(Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K, Tensor offsets, int64_t nSym,
                         Tensor W1, Tensor b1, Tensor W2, Tensor b2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, Tensor logitsVelocity,
                         Tensor ofLogits, Tensor symIdx, Tensor scatterIdx, Tensor ws)
{
    all_cpu(ctx, pairs, offsets, W1, b1, W2, b2, logitsVelocity, ofLogits, symIdx, scatterIdx, ws);
    const AttrHeadsArgs a = attr_heads_args(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                                            symIdx, scatterIdx);
    if (K == 0) return;
    semicrf_cpu::attribute_heads(a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, (int)nSym, a.W1, a.b1, a.W2, a.b2, (int)Hv, (int)Ho,
                                 (int)Nv, (int)No, a.lv, a.of, a.sym, a.sc);
}

// ---- the backbone's axial attention (semicrf_axial_attention) ----------------------------------------------------------------------
// q, out: [n0, n1, Lq, H d]; k, v: [n0, n1, Lk, H d]: VIEWS -- the three element strides of every tensor are read from the tensor
// itself (so an access can never leave it); only the last dimension must be contiguous.  Sizes of 1 may carry any stride.
// (the bf16 op, semicrf_axial_attention_bf16, takes the same views of bfloat16 tensors: `dtype` is the one all four must have)
struct AttentionArgs { const void *q, *k, *v; void* out; int64_t n0, n1; int Lq, Lk, H, d; int64_t st[12]; };
inline AttentionArgs attention_args(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out, int64_t H,
                                    ScalarType dtype = ScalarType::Float)
{
    const Tensor* ts[4] = {&q, &k, &v, &out};
    const char* names[4] = {"q", "k", "v", "out"};
    AttentionArgs a{};
    STD_TORCH_CHECK(q.defined() && q.dim() == 4, "semicrf: `q` must be [n0, n1, Lq, H * d]");
    a.n0 = q.size(0); a.n1 = q.size(1);
    const int64_t Lq = q.size(2), Lk = k.defined() && k.dim() == 4 ? k.size(2) : -1, HD = q.size(3);
    STD_TORCH_CHECK(H >= 1 && H < (1 << 20) && HD % H == 0, "semicrf: the last dimension must be H * d");
    for (int i = 0; i < 4; ++i) {
        const Tensor& t = *ts[i];
        STD_TORCH_CHECK(t.defined() && t.scalar_type() == dtype && t.dim() == 4, "semicrf: `", names[i], "` must be a 4-d ",
                        dtype == ScalarType::Float ? "float32" : "bfloat16", " tensor");
        STD_TORCH_CHECK(t.size(0) == a.n0 && t.size(1) == a.n1 && t.size(3) == HD && t.size(2) == (i == 0 || i == 3 ? Lq : Lk),
                        "semicrf: `", names[i], "` does not have the shape of the call");
        STD_TORCH_CHECK(HD == 1 || t.stride(3) == 1, "semicrf: `", names[i], "` must have a contiguous last dimension");
        for (int j = 0; j < 3; ++j) {
            const int64_t s = t.size(j) > 1 ? t.stride(j) : 0;
            STD_TORCH_CHECK(s >= 0, "semicrf: negative stride");
            a.st[3 * i + j] = s;
        }
    }
    for (int j = 0; j < 3; ++j) STD_TORCH_CHECK(out.size(j) == 1 || a.st[9 + j] > 0, "semicrf: `out` must not repeat over a dimension");
    STD_TORCH_CHECK(Lq < (1 << 20) && Lk < (1 << 20), "semicrf: sequence too long");
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H; a.d = (int)(HD / H);
    STD_TORCH_CHECK(semicrf_axial_attention_supported(a.Lq, a.Lk, a.H, a.d),
                    "semicrf: axial_attention does not support Lq=", Lq, " Lk=", Lk, " H=", H, " d=", HD / H,
                    " (semicrf_axial_attention_supported)");
    a.q = q.data_ptr(); a.k = k.data_ptr(); a.v = v.data_ptr(); a.out = out.data_ptr();      // defined and of `dtype`: checked above
    return a;
}
void axial_attention_op(Tensor q, Tensor k, Tensor v, Tensor out, int64_t H)
{
    Ctx c(q); c.same(q, k, v, out);
    const AttentionArgs a = attention_args(q, k, v, out, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    check(semicrf_axial_attention((const float*)a.q, (const float*)a.k, (const float*)a.v, (float*)a.out, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5],
                                  a.st[6], a.st[7], a.st[8], a.st[9], a.st[10], a.st[11], c.stream),
          "semicrf_axial_attention");
}
void axial_attention_cpu(Tensor q, Tensor k, Tensor v, Tensor out, int64_t H)
{
    all_cpu(q, k, v, out);
    const AttentionArgs a = attention_args(q, k, v, out, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    semicrf_cpu::axial_attention((const float*)a.q, (const float*)a.k, (const float*)a.v, (float*)a.out, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, a.st);
}
void axial_attention_bf16_op(Tensor q, Tensor k, Tensor v, Tensor out, int64_t H)
{
    Ctx c(q); c.same(q, k, v, out);
    const AttentionArgs a = attention_args(q, k, v, out, H, ScalarType::BFloat16);
    if (a.n0 == 0 || a.n1 == 0) return;
    check(semicrf_axial_attention_bf16((const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.out, a.n0, a.n1, a.Lq, a.Lk,
                                       a.H, a.d, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5], a.st[6], a.st[7], a.st[8], a.st[9], a.st[10],
                                       a.st[11], c.stream),
          "semicrf_axial_attention_bf16");
}
void axial_attention_bf16_cpu(Tensor q, Tensor k, Tensor v, Tensor out, int64_t H)
{
    all_cpu(q, k, v, out);
    const AttentionArgs a = attention_args(q, k, v, out, H, ScalarType::BFloat16);
    if (a.n0 == 0 || a.n1 == 0) return;
    semicrf_cpu::axial_attention_bf16((const uint16_t*)a.q, (const uint16_t*)a.k, (const uint16_t*)a.v, (uint16_t*)a.out, a.n0, a.n1, a.Lq, a.Lk, a.H,
                                      a.d, a.st);
}

// ---- the backbone's feed-forward ResBlock (semicrf_ffn_residual) --------------------------------------------------------------------
// x, out: [n0, n1, D] VIEWS with a contiguous last dimension (their two row strides are read from the tensors); W1 [hidden, D],
// b1 [hidden], W2 [D, hidden], b2 [D], scale [D] contiguous, as nn.Linear and ResBlock store them
struct FfnArgs { const void *x, *W1, *b1, *W2, *b2, *scale; void* out; int64_t n0, n1, st[4]; int D, H; };   // elements of `dtype`
inline FfnArgs ffn_args(const Tensor& x, const Tensor& W1, const Tensor& b1, const Tensor& W2, const Tensor& b2, const Tensor& scale,
                        const Tensor& out, ScalarType dtype = ScalarType::Float)
{
    const char* const dname = dtype == ScalarType::Float ? "float32" : "bfloat16";
    auto ptr = [&](const Tensor& t, int64_t n, const char* name) -> const void* { want(t, dtype, n, name); return t.data_ptr(); };
    FfnArgs a{};
    STD_TORCH_CHECK(x.defined() && x.dim() == 3 && out.defined() && out.dim() == 3, "semicrf: `x` and `out` must be [n0, n1, D]");
    STD_TORCH_CHECK(x.scalar_type() == dtype && out.scalar_type() == dtype, "semicrf: `x` and `out` must be ", dname);
    STD_TORCH_CHECK(W1.defined() && W1.dim() == 2 && W2.defined() && W2.dim() == 2, "semicrf: `W1` must be [hidden, D], `W2` [D, hidden]");
    const int64_t D = x.size(2), H = W1.size(0);
    a.n0 = x.size(0); a.n1 = x.size(1);
    STD_TORCH_CHECK(out.size(0) == a.n0 && out.size(1) == a.n1 && out.size(2) == D, "semicrf: `out` does not have the shape of `x`");
    STD_TORCH_CHECK(D >= 1 && D < (1 << 20) && H >= 1 && H < (1 << 20) && W1.size(1) == D && W2.size(0) == D && W2.size(1) == H,
                    "semicrf: `W1` / `W2` do not have the shape of the call");
    STD_TORCH_CHECK(semicrf_ffn_residual_supported((int)D, (int)H), "semicrf: ffn_residual does not support D=", D, " hidden=", H,
                    " (semicrf_ffn_residual_supported)");
    STD_TORCH_CHECK(x.stride(2) == 1 && out.stride(2) == 1, "semicrf: `x` and `out` must have a contiguous last dimension");
    for (int j = 0; j < 2; ++j) {
        a.st[j] = x.size(j) > 1 ? x.stride(j) : 0;
        a.st[2 + j] = out.size(j) > 1 ? out.stride(j) : 0;
        STD_TORCH_CHECK(a.st[j] >= 0 && a.st[2 + j] >= 0, "semicrf: negative stride");
        STD_TORCH_CHECK(out.size(j) == 1 || a.st[2 + j] >= D, "semicrf: `out` must not repeat or interleave its rows");
    }
    a.D = (int)D; a.H = (int)H;
    a.W1 = ptr(W1, H * D, "W1"); a.b1 = ptr(b1, H, "b1"); a.W2 = ptr(W2, D * H, "W2"); a.b2 = ptr(b2, D, "b2"); a.scale = ptr(scale, D, "scale");
    STD_TORCH_CHECK(b1.numel() == H && b2.numel() == D && scale.numel() == D, "semicrf: `b1` / `b2` / `scale` do not have the shape of the call");
    a.x = x.numel() > 0 ? x.data_ptr() : nullptr;
    a.out = out.numel() > 0 ? out.data_ptr() : nullptr;
    return a;
}
// one body per entry point: E the element type of the C ABI, `overlap` the element ranges of the two views
template <typename E, typename F>
void ffn_on_device(const FfnArgs& a, double eps, semicrf_stream_t stream, F entry, const char* name)
{
    check(entry((const E*)a.x, (E*)a.out, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H, (const E*)a.W1, (const E*)a.b1, (const E*)a.W2,
                (const E*)a.b2, (const E*)a.scale, (float)eps, stream),
          name);
}
template <typename E, typename F>
void ffn_on_host(const FfnArgs& a, double eps, F mirror, const char* name)
{
    const int64_t xext = (a.n0 - 1) * a.st[0] + (a.n1 - 1) * a.st[1] + a.D, oext = (a.n0 - 1) * a.st[2] + (a.n1 - 1) * a.st[3] + a.D;
    const E *x = (const E*)a.x, *o = (const E*)a.out;
    STD_TORCH_CHECK(x + xext <= o || o + oext <= x, "semicrf: ", name, ": `out` overlaps `x`");
    mirror(x, (E*)a.out, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H, (const E*)a.W1, (const E*)a.b1, (const E*)a.W2, (const E*)a.b2,
           (const E*)a.scale, (float)eps);
}
void ffn_residual_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    Ctx c(x); c.same(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_device<float>(a, eps, c.stream, &semicrf_ffn_residual, "semicrf_ffn_residual");
}
void ffn_residual_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    all_cpu(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_host<float>(a, eps, &semicrf_cpu::ffn_residual, "ffn_residual");
}
// ---- the block in training (semicrf_ffn_residual_train_fwd / _bwd / semicrf_ffn_dropout_mask) -------------------------------------------
// z [n0 n1, hidden], y [n0 n1, D] dense; seed: the 64 bits of an int
void ffn_residual_train_fwd_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed, double p_hidden,
                               double p_out, Tensor out, Tensor z, Tensor y)
{
    Ctx c(x); c.same(x, W1, b1, W2, b2, scale, out, z, y);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    float* zp = f32w(z, a.n0 * a.n1 * a.H, "z");
    float* yp = f32w(y, a.n0 * a.n1 * a.D, "y");
    if (a.n0 == 0 || a.n1 == 0) return;
    check(semicrf_ffn_residual_train_fwd((const float*)a.x, (float*)a.out, zp, yp, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H,
                                         (const float*)a.W1, (const float*)a.b1, (const float*)a.W2, (const float*)a.b2, (const float*)a.scale,
                                         (float)eps, (uint64_t)seed, p_hidden, p_out, c.stream),
          "semicrf_ffn_residual_train_fwd");
}
void ffn_residual_train_fwd_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed, double p_hidden,
                                double p_out, Tensor out, Tensor z, Tensor y)
{
    all_cpu(x, W1, b1, W2, b2, scale, out, z, y);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    float* zp = f32w(z, a.n0 * a.n1 * a.H, "z");
    float* yp = f32w(y, a.n0 * a.n1 * a.D, "y");
    STD_TORCH_CHECK(p_hidden >= 0.0 && p_hidden < 1.0 && p_out >= 0.0 && p_out < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    if (a.n0 == 0 || a.n1 == 0) return;
    const int64_t xext = (a.n0 - 1) * a.st[0] + (a.n1 - 1) * a.st[1] + a.D, oext = (a.n0 - 1) * a.st[2] + (a.n1 - 1) * a.st[3] + a.D;
    const float *xp = (const float*)a.x, *op = (const float*)a.out;
    STD_TORCH_CHECK(xp + xext <= op || op + oext <= xp, "semicrf: ffn_residual_train_fwd: `out` overlaps `x`");
    semicrf_cpu::ffn_residual_train_fwd(xp, (float*)a.out, zp, yp, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H, (const float*)a.W1,
                                        (const float*)a.b1, (const float*)a.W2, (const float*)a.b2, (const float*)a.scale, (float)eps,
                                        (uint64_t)seed, p_hidden, p_out);
}

struct FfnBwdArgs {
    const float *g, *x, *z, *y, *W1, *W2, *scale;
    float *dx, *dW1, *db1, *dW2, *db2, *dscale;
    int64_t n0, n1, st[6];           // dout, x, dx: two element row strides each
    int D, H;
};
inline FfnBwdArgs ffn_bwd_args(const Tensor& dout, const Tensor& x, const Tensor& z, const Tensor& y, const Tensor& W1, const Tensor& W2,
                               const Tensor& scale, double p_hidden, double p_out, const Tensor& dx, const Tensor& dW1, const Tensor& db1,
                               const Tensor& dW2, const Tensor& db2, const Tensor& dscale)
{
    FfnBwdArgs a{};
    const Tensor* views[3] = {&dout, &x, &dx};
    STD_TORCH_CHECK(x.defined() && x.dim() == 3, "semicrf: `x` must be [n0, n1, D]");
    STD_TORCH_CHECK(W1.defined() && W1.dim() == 2 && W2.defined() && W2.dim() == 2, "semicrf: `W1` must be [hidden, D], `W2` [D, hidden]");
    const int64_t D = x.size(2), H = W1.size(0);
    a.n0 = x.size(0); a.n1 = x.size(1);
    STD_TORCH_CHECK(D >= 1 && D < (1 << 20) && H >= 1 && H < (1 << 20) && W1.size(1) == D && W2.size(0) == D && W2.size(1) == H,
                    "semicrf: `W1` / `W2` do not have the shape of the call");
    STD_TORCH_CHECK(semicrf_ffn_residual_bwd_supported((int)D, (int)H), "semicrf: ffn_residual_bwd does not support D=", D, " hidden=", H,
                    " (semicrf_ffn_residual_bwd_supported)");
    STD_TORCH_CHECK(p_hidden >= 0.0 && p_hidden < 1.0 && p_out >= 0.0 && p_out < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    for (int v = 0; v < 3; ++v) {
        const Tensor& t = *views[v];
        STD_TORCH_CHECK(t.defined() && t.dim() == 3 && t.scalar_type() == ScalarType::Float, "semicrf: `dout`, `x` and `dx` must be float32 [n0, n1, D]");
        STD_TORCH_CHECK(t.size(0) == a.n0 && t.size(1) == a.n1 && t.size(2) == D && t.stride(2) == 1,
                        "semicrf: `dout`, `x` and `dx` must share one shape and have a contiguous last dimension");
        for (int j = 0; j < 2; ++j) {
            a.st[2 * v + j] = t.size(j) > 1 ? t.stride(j) : 0;
            STD_TORCH_CHECK(a.st[2 * v + j] >= 0, "semicrf: negative stride");
        }
    }
    STD_TORCH_CHECK((a.n0 <= 1 || a.st[4] >= D) && (a.n1 <= 1 || a.st[5] >= D), "semicrf: `dx` must not repeat or interleave its rows");
    a.D = (int)D; a.H = (int)H;
    const int64_t ntok = a.n0 * a.n1;
    a.z = f32(z, ntok * H, "z"); a.y = f32(y, ntok * D, "y");
    a.W1 = f32(W1, H * D, "W1"); a.W2 = f32(W2, D * H, "W2"); a.scale = f32(scale, D, "scale");
    a.dW1 = f32w(dW1, H * D, "dW1"); a.db1 = f32w(db1, H, "db1"); a.dW2 = f32w(dW2, D * H, "dW2"); a.db2 = f32w(db2, D, "db2");
    a.dscale = f32w(dscale, D, "dscale");
    a.g = ntok > 0 ? (const float*)dout.data_ptr() : nullptr;
    a.x = ntok > 0 ? (const float*)x.data_ptr() : nullptr;
    a.dx = ntok > 0 ? (float*)dx.data_ptr() : nullptr;
    return a;
}
void ffn_residual_bwd_op(Tensor dout, Tensor x, Tensor z, Tensor y, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                         double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    Ctx c(x); c.same(x, dout, z, y, W1, W2, scale, dx, dW1, db1, dW2, db2, dscale, ws);
    const FfnBwdArgs a = ffn_bwd_args(dout, x, z, y, W1, W2, scale, p_hidden, p_out, dx, dW1, db1, dW2, db2, dscale);
    if (a.n0 == 0 || a.n1 == 0) return;
    check(semicrf_ffn_residual_bwd(a.g, a.x, a.z, a.y, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5], a.D, a.H, a.W1, a.W2,
                                   a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out, a.dx, a.dW1, a.db1, a.dW2, a.db2, a.dscale,
                                   bytes(ws, "ws"), (size_t)ws.numel(), c.stream),
          "semicrf_ffn_residual_bwd");
}
void ffn_residual_bwd_cpu(Tensor dout, Tensor x, Tensor z, Tensor y, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                          double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    all_cpu(x, dout, z, y, W1, W2, scale, dx, dW1, db1, dW2, db2, dscale, ws);
    const FfnBwdArgs a = ffn_bwd_args(dout, x, z, y, W1, W2, scale, p_hidden, p_out, dx, dW1, db1, dW2, db2, dscale);
    if (a.n0 == 0 || a.n1 == 0) return;
    auto ext = [&](int v) { return (a.n0 - 1) * a.st[2 * v] + (a.n1 - 1) * a.st[2 * v + 1] + a.D; };
    auto apart = [](const float* p, int64_t np, const float* q, int64_t nq) { return p + np <= q || q + nq <= p; };
    const int64_t ntok = a.n0 * a.n1;
    STD_TORCH_CHECK(apart(a.dx, ext(2), a.g, ext(0)) && apart(a.dx, ext(2), a.x, ext(1)) && apart(a.dx, ext(2), a.z, ntok * a.H) &&
                    apart(a.dx, ext(2), a.y, ntok * a.D), "semicrf: ffn_residual_bwd: `dx` overlaps dout, x, z or y");
    semicrf_cpu::ffn_residual_bwd(a.g, a.x, a.z, a.y, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5], a.D, a.H, a.W1, a.W2,
                                  a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out, a.dx, a.dW1, a.db1, a.dW2, a.db2, a.dscale);
}

inline void ffn_mask_args(const Tensor& mh, const Tensor& mo, int64_t rows, int64_t D, int64_t H, double p_hidden, double p_out)
{
    STD_TORCH_CHECK(rows >= 0 && rows < (1ll << 37) && D >= 1 && D < (1 << 20) && H >= 1 && H < (1 << 20), "semicrf: bad mask shape");
    STD_TORCH_CHECK(p_hidden >= 0.0 && p_hidden < 1.0 && p_out >= 0.0 && p_out < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    want(mh, ScalarType::Byte, rows * H, "mask_hidden");
    want(mo, ScalarType::Byte, rows * D, "mask_out");
}
void ffn_dropout_mask_op(Tensor mh, Tensor mo, int64_t seed, int64_t rows, int64_t D, int64_t H, double p_hidden, double p_out)
{
    Ctx c(mh); c.same(mh, mo);
    ffn_mask_args(mh, mo, rows, D, H, p_hidden, p_out);
    if (rows == 0) return;
    check(semicrf_ffn_dropout_mask((uint64_t)seed, rows, (int)D, (int)H, p_hidden, p_out, (unsigned char*)mh.data_ptr(),
                                   (unsigned char*)mo.data_ptr(), c.stream),
          "semicrf_ffn_dropout_mask");
}
void ffn_dropout_mask_cpu(Tensor mh, Tensor mo, int64_t seed, int64_t rows, int64_t D, int64_t H, double p_hidden, double p_out)
{
    all_cpu(mh, mo);
    ffn_mask_args(mh, mo, rows, D, H, p_hidden, p_out);
    if (rows == 0) return;
    semicrf_cpu::ffn_dropout_mask((uint64_t)seed, rows, (int)D, (int)H, p_hidden, p_out, (unsigned char*)mh.data_ptr(), (unsigned char*)mo.data_ptr());
}

// the bf16 forms: `ffn_residual_bf16` on bfloat16 tensors, `ffn_residual_bf16_mixed` on float32 tensors (bf16 operands inside)
void ffn_residual_bf16_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    Ctx c(x); c.same(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out, ScalarType::BFloat16);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_device<uint16_t>(a, eps, c.stream, &semicrf_ffn_residual_bf16, "semicrf_ffn_residual_bf16");
}
void ffn_residual_bf16_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    all_cpu(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out, ScalarType::BFloat16);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_host<uint16_t>(a, eps, &semicrf_cpu::ffn_residual_bf16, "ffn_residual_bf16");
}
void ffn_residual_bf16_mixed_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    Ctx c(x); c.same(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_device<float>(a, eps, c.stream, &semicrf_ffn_residual_bf16_mixed, "semicrf_ffn_residual_bf16_mixed");
}
void ffn_residual_bf16_mixed_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, Tensor out)
{
    all_cpu(x, W1, b1, W2, b2, scale, out);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out);
    if (a.n0 == 0 || a.n1 == 0) return;
    ffn_on_host<float>(a, eps, &semicrf_cpu::ffn_residual_bf16_mixed, "ffn_residual_bf16_mixed");
}

// ---- the bf16 block in training: four ops, E the element type of the form (uint16_t: bfloat16 tensors, float: the _mixed form) ------------
// saved: uint8, contiguous, at least semicrf_ffn_residual_bf16_train_saved_bytes(n0 n1, D, hidden) bytes, 16-byte aligned; seed: 64 bits
template <typename E>
constexpr ScalarType ffn16_dtype() { return sizeof(E) == 2 ? ScalarType::BFloat16 : ScalarType::Float; }
inline void ffn16_p_ok(double p_hidden, double p_out)
{
    STD_TORCH_CHECK(p_hidden >= 0.0 && p_hidden < 1.0 && p_out >= 0.0 && p_out < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
}
inline bool ffn16_apart(const void* p, size_t np, const void* q, size_t nq)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a + np <= b || b + nq <= a;
}
inline void* ffn16_saved(const Tensor& saved, const FfnArgs& a, size_t* need)
{
    *need = semicrf_ffn_residual_bf16_train_saved_bytes(a.n0 * a.n1, a.D, a.H);
    void* p = bytes(saved, "saved");
    if (a.n0 == 0 || a.n1 == 0) return p;
    STD_TORCH_CHECK((size_t)saved.numel() >= *need, "semicrf: `saved` holds ", saved.numel(), " bytes, the call needs ", *need);
    STD_TORCH_CHECK(((uintptr_t)p & 15) == 0, "semicrf: `saved` must be 16-byte aligned");
    return p;
}
template <typename E, typename F>
void ffn16_train_fwd_device(F entry, const char* name, const Tensor& x, const Tensor& W1, const Tensor& b1, const Tensor& W2, const Tensor& b2,
                            const Tensor& scale, double eps, int64_t seed, double p_hidden, double p_out, const Tensor& out, const Tensor& saved)
{
    Ctx c(x); c.same(x, W1, b1, W2, b2, scale, out, saved);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out, ffn16_dtype<E>());
    void* sp = bytes(saved, "saved");
    if (a.n0 == 0 || a.n1 == 0) return;
    check(entry((const E*)a.x, (E*)a.out, sp, (size_t)saved.numel(), a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H, (const E*)a.W1,
                (const E*)a.b1, (const E*)a.W2, (const E*)a.b2, (const E*)a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out, c.stream),
          name);
}
template <typename E, typename F>
void ffn16_train_fwd_host(F mirror, const char* name, const Tensor& x, const Tensor& W1, const Tensor& b1, const Tensor& W2, const Tensor& b2,
                          const Tensor& scale, double eps, int64_t seed, double p_hidden, double p_out, const Tensor& out, const Tensor& saved)
{
    all_cpu(x, W1, b1, W2, b2, scale, out, saved);
    const FfnArgs a = ffn_args(x, W1, b1, W2, b2, scale, out, ffn16_dtype<E>());
    ffn16_p_ok(p_hidden, p_out);
    size_t need = 0;
    void* sp = ffn16_saved(saved, a, &need);
    if (a.n0 == 0 || a.n1 == 0) return;
    const size_t xext = (size_t)((a.n0 - 1) * a.st[0] + (a.n1 - 1) * a.st[1] + a.D) * sizeof(E);
    const size_t oext = (size_t)((a.n0 - 1) * a.st[2] + (a.n1 - 1) * a.st[3] + a.D) * sizeof(E);
    STD_TORCH_CHECK(ffn16_apart(a.x, xext, a.out, oext), "semicrf: ", name, ": `out` overlaps `x`");
    STD_TORCH_CHECK(ffn16_apart(sp, need, a.x, xext) && ffn16_apart(sp, need, a.out, oext), "semicrf: ", name, ": saved overlaps x or out");
    mirror((const E*)a.x, (E*)a.out, sp, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.D, a.H, (const E*)a.W1, (const E*)a.b1, (const E*)a.W2,
           (const E*)a.b2, (const E*)a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out);
}

struct Ffn16BwdArgs {
    const void *g, *x, *W1, *W2, *scale;
    void *dx, *dW1, *db1, *dW2, *db2, *dscale;
    int64_t n0, n1, st[6];           // dout, x, dx: two element row strides each
    int D, H;
};
inline Ffn16BwdArgs ffn16_bwd_args(ScalarType dtype, const Tensor& dout, const Tensor& x, const Tensor& W1, const Tensor& W2, const Tensor& scale,
                                   double p_hidden, double p_out, const Tensor& dx, const Tensor& dW1, const Tensor& db1, const Tensor& dW2,
                                   const Tensor& db2, const Tensor& dscale)
{
    Ffn16BwdArgs a{};
    const char* const dname = dtype == ScalarType::Float ? "float32" : "bfloat16";
    const Tensor* views[3] = {&dout, &x, &dx};
    STD_TORCH_CHECK(x.defined() && x.dim() == 3, "semicrf: `x` must be [n0, n1, D]");
    STD_TORCH_CHECK(W1.defined() && W1.dim() == 2 && W2.defined() && W2.dim() == 2, "semicrf: `W1` must be [hidden, D], `W2` [D, hidden]");
    const int64_t D = x.size(2), H = W1.size(0);
    a.n0 = x.size(0); a.n1 = x.size(1);
    STD_TORCH_CHECK(D >= 1 && D < (1 << 20) && H >= 1 && H < (1 << 20) && W1.size(1) == D && W2.size(0) == D && W2.size(1) == H,
                    "semicrf: `W1` / `W2` do not have the shape of the call");
    STD_TORCH_CHECK(semicrf_ffn_residual_bf16_bwd_supported((int)D, (int)H), "semicrf: ffn_residual_bf16_bwd does not support D=", D, " hidden=", H,
                    " (semicrf_ffn_residual_bf16_bwd_supported)");
    ffn16_p_ok(p_hidden, p_out);
    for (int v = 0; v < 3; ++v) {
        const Tensor& t = *views[v];
        STD_TORCH_CHECK(t.defined() && t.dim() == 3 && t.scalar_type() == dtype, "semicrf: `dout`, `x` and `dx` must be ", dname, " [n0, n1, D]");
        STD_TORCH_CHECK(t.size(0) == a.n0 && t.size(1) == a.n1 && t.size(2) == D && t.stride(2) == 1,
                        "semicrf: `dout`, `x` and `dx` must share one shape and have a contiguous last dimension");
        for (int j = 0; j < 2; ++j) {
            a.st[2 * v + j] = t.size(j) > 1 ? t.stride(j) : 0;
            STD_TORCH_CHECK(a.st[2 * v + j] >= 0, "semicrf: negative stride");
        }
    }
    STD_TORCH_CHECK((a.n0 <= 1 || a.st[4] >= D) && (a.n1 <= 1 || a.st[5] >= D), "semicrf: `dx` must not repeat or interleave its rows");
    a.D = (int)D; a.H = (int)H;
    auto ptr = [&](const Tensor& t, int64_t n, const char* name) -> void* { want(t, dtype, n, name); return t.data_ptr(); };
    a.W1 = ptr(W1, H * D, "W1"); a.W2 = ptr(W2, D * H, "W2"); a.scale = ptr(scale, D, "scale");
    a.dW1 = ptr(dW1, H * D, "dW1"); a.db1 = ptr(db1, H, "db1"); a.dW2 = ptr(dW2, D * H, "dW2"); a.db2 = ptr(db2, D, "db2");
    a.dscale = ptr(dscale, D, "dscale");
    const int64_t ntok = a.n0 * a.n1;
    a.g = ntok > 0 ? dout.data_ptr() : nullptr;
    a.x = ntok > 0 ? x.data_ptr() : nullptr;
    a.dx = ntok > 0 ? dx.data_ptr() : nullptr;
    return a;
}
template <typename E, typename F>
void ffn16_bwd_device(F entry, const char* name, const Tensor& dout, const Tensor& x, const Tensor& saved, const Tensor& W1, const Tensor& W2,
                      const Tensor& scale, double eps, int64_t seed, double p_hidden, double p_out, const Tensor& dx, const Tensor& dW1,
                      const Tensor& db1, const Tensor& dW2, const Tensor& db2, const Tensor& dscale, const Tensor& ws)
{
    Ctx c(x); c.same(x, dout, saved, W1, W2, scale, dx, dW1, db1, dW2, db2, dscale, ws);
    const Ffn16BwdArgs a = ffn16_bwd_args(ffn16_dtype<E>(), dout, x, W1, W2, scale, p_hidden, p_out, dx, dW1, db1, dW2, db2, dscale);
    void* sp = bytes(saved, "saved");
    void* wp = bytes(ws, "ws");
    if (a.n0 == 0 || a.n1 == 0) return;
    check(entry((const E*)a.g, (const E*)a.x, sp, (size_t)saved.numel(), a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5], a.D, a.H,
                (const E*)a.W1, (const E*)a.W2, (const E*)a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out, (E*)a.dx, (E*)a.dW1, (E*)a.db1, (E*)a.dW2,
                (E*)a.db2, (E*)a.dscale, wp, (size_t)ws.numel(), c.stream),
          name);
}
template <typename E, typename F>
void ffn16_bwd_host(F mirror, const char* name, const Tensor& dout, const Tensor& x, const Tensor& saved, const Tensor& W1, const Tensor& W2,
                    const Tensor& scale, double eps, int64_t seed, double p_hidden, double p_out, const Tensor& dx, const Tensor& dW1,
                    const Tensor& db1, const Tensor& dW2, const Tensor& db2, const Tensor& dscale, const Tensor& ws)
{
    all_cpu(x, dout, saved, W1, W2, scale, dx, dW1, db1, dW2, db2, dscale, ws);
    const Ffn16BwdArgs a = ffn16_bwd_args(ffn16_dtype<E>(), dout, x, W1, W2, scale, p_hidden, p_out, dx, dW1, db1, dW2, db2, dscale);
    void* sp = bytes(saved, "saved");
    if (a.n0 == 0 || a.n1 == 0) return;
    const size_t need = semicrf_ffn_residual_bf16_train_saved_bytes(a.n0 * a.n1, a.D, a.H);
    STD_TORCH_CHECK((size_t)saved.numel() >= need, "semicrf: `saved` holds ", saved.numel(), " bytes, the call needs ", need);
    auto ext = [&](int v) { return (size_t)((a.n0 - 1) * a.st[2 * v] + (a.n1 - 1) * a.st[2 * v + 1] + a.D) * sizeof(E); };
    STD_TORCH_CHECK(ffn16_apart(a.dx, ext(2), a.g, ext(0)) && ffn16_apart(a.dx, ext(2), a.x, ext(1)) && ffn16_apart(a.dx, ext(2), sp, need),
                    "semicrf: ", name, ": `dx` overlaps dout, x or saved");
    mirror((const E*)a.g, (const E*)a.x, sp, a.n0, a.n1, a.st[0], a.st[1], a.st[2], a.st[3], a.st[4], a.st[5], a.D, a.H, (const E*)a.W1,
           (const E*)a.W2, (const E*)a.scale, (float)eps, (uint64_t)seed, p_hidden, p_out, (E*)a.dx, (E*)a.dW1, (E*)a.db1, (E*)a.dW2, (E*)a.db2,
           (E*)a.dscale);
}

void ffn_residual_bf16_train_fwd_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed, double p_hidden,
                                    double p_out, Tensor out, Tensor saved)
{
    ffn16_train_fwd_device<uint16_t>(&semicrf_ffn_residual_bf16_train_fwd, "semicrf_ffn_residual_bf16_train_fwd", x, W1, b1, W2, b2, scale, eps, seed,
                                     p_hidden, p_out, out, saved);
}
void ffn_residual_bf16_train_fwd_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed, double p_hidden,
                                     double p_out, Tensor out, Tensor saved)
{
    ffn16_train_fwd_host<uint16_t>(&semicrf_cpu::ffn_residual_bf16_train_fwd, "ffn_residual_bf16_train_fwd", x, W1, b1, W2, b2, scale, eps, seed,
                                   p_hidden, p_out, out, saved);
}
void ffn_residual_bf16_mixed_train_fwd_op(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed,
                                          double p_hidden, double p_out, Tensor out, Tensor saved)
{
    ffn16_train_fwd_device<float>(&semicrf_ffn_residual_bf16_mixed_train_fwd, "semicrf_ffn_residual_bf16_mixed_train_fwd", x, W1, b1, W2, b2, scale, eps,
                                  seed, p_hidden, p_out, out, saved);
}
void ffn_residual_bf16_mixed_train_fwd_cpu(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, double eps, int64_t seed,
                                           double p_hidden, double p_out, Tensor out, Tensor saved)
{
    ffn16_train_fwd_host<float>(&semicrf_cpu::ffn_residual_bf16_mixed_train_fwd, "ffn_residual_bf16_mixed_train_fwd", x, W1, b1, W2, b2, scale, eps,
                                seed, p_hidden, p_out, out, saved);
}
void ffn_residual_bf16_bwd_op(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                              double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    ffn16_bwd_device<uint16_t>(&semicrf_ffn_residual_bf16_bwd, "semicrf_ffn_residual_bf16_bwd", dout, x, saved, W1, W2, scale, eps, seed, p_hidden, p_out,
                               dx, dW1, db1, dW2, db2, dscale, ws);
}
void ffn_residual_bf16_bwd_cpu(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                               double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    ffn16_bwd_host<uint16_t>(&semicrf_cpu::ffn_residual_bf16_bwd, "ffn_residual_bf16_bwd", dout, x, saved, W1, W2, scale, eps, seed, p_hidden, p_out, dx,
                             dW1, db1, dW2, db2, dscale, ws);
}
void ffn_residual_bf16_mixed_bwd_op(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                                    double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    ffn16_bwd_device<float>(&semicrf_ffn_residual_bf16_mixed_bwd, "semicrf_ffn_residual_bf16_mixed_bwd", dout, x, saved, W1, W2, scale, eps, seed,
                            p_hidden, p_out, dx, dW1, db1, dW2, db2, dscale, ws);
}
void ffn_residual_bf16_mixed_bwd_cpu(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, double eps, int64_t seed, double p_hidden,
                                     double p_out, Tensor dx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor dscale, Tensor ws)
{
    ffn16_bwd_host<float>(&semicrf_cpu::ffn_residual_bf16_mixed_bwd, "ffn_residual_bf16_mixed_bwd", dout, x, saved, W1, W2, scale, eps, seed, p_hidden,
                          p_out, dx, dW1, db1, dW2, db2, dscale, ws);
}

// ---- the audio front end (semicrf_log_mel) -------------------------------------------------------------------------------------------
// frames: a [N, C, nFrame, W] VIEW with sample stride 1 (its three other strides are read from the tensor: the overlapping unfold view
// goes in as it is); windows [nWin, W], tw [W / 2, 2], fb_start / fb_len / fb_off [nMel] int32, fb_val [total], shift / denom [N] when
// has_gain, out [N, to_mono ? 1 : C, nFrame, nMel, nWin], all contiguous
struct LogMelCall {
    const float *frames, *windows, *tw, *fb_val, *shift, *denom; const int32_t *fb_start, *fb_len, *fb_off; float* out;
    int64_t st[3]; int N, C, nFrame, W, nWin, nMel, total;
};
inline LogMelCall log_mel_args(const Tensor& frames, const Tensor& windows, const Tensor& tw, const Tensor& fb_start, const Tensor& fb_len,
                               const Tensor& fb_off, const Tensor& fb_val, int64_t max_len, const Tensor& shift, const Tensor& denom,
                               bool has_gain, bool to_mono, const Tensor& out)
{
    LogMelCall a{};
    STD_TORCH_CHECK(frames.defined() && frames.dim() == 4, "semicrf: `frames` must be [N, C, nFrame, W]");
    STD_TORCH_CHECK(frames.scalar_type() == ScalarType::Float, "semicrf: `frames` must be float32");
    STD_TORCH_CHECK(windows.defined() && windows.dim() == 2, "semicrf: `windows` must be [nWin, W]");
    const int64_t N = frames.size(0), C = frames.size(1), nFrame = frames.size(2), W = frames.size(3), nWin = windows.size(0);
    const int64_t nMel = fb_start.numel(), total = fb_val.numel();
    STD_TORCH_CHECK(windows.size(1) == W && N < (1ll << 31) && C < (1 << 20) && nFrame < (1ll << 31) && W < (1 << 20) && nWin < (1 << 20) &&
                    nMel < (1 << 20) && total < (1ll << 31) && max_len >= 0 && max_len < (1ll << 31), "semicrf: log_mel: bad shape");
    STD_TORCH_CHECK(semicrf_log_mel_supported((int)W, (int)nWin, (int)C, (int)nMel, (int)max_len, (int)total), "semicrf: log_mel does not support W=", W,
                    " nWin=", nWin, " C=", C, " nMel=", nMel, " max_len=", max_len, " total=", total, " (semicrf_log_mel_supported)");
    STD_TORCH_CHECK(W == 1 || frames.stride(3) == 1, "semicrf: `frames` must have sample stride 1");
    for (int j = 0; j < 3; ++j) {
        a.st[j] = frames.size(j) > 1 ? frames.stride(j) : 0;
        STD_TORCH_CHECK(a.st[j] >= 0, "semicrf: negative stride");
    }
    a.N = (int)N; a.C = (int)C; a.nFrame = (int)nFrame; a.W = (int)W; a.nWin = (int)nWin; a.nMel = (int)nMel; a.total = (int)total;
    a.windows = f32(windows, nWin * W, "windows");
    a.tw = f32(tw, W, "tw");
    STD_TORCH_CHECK(tw.numel() == W, "semicrf: `tw` must be [W / 2, 2]");
    a.fb_start = i32(fb_start, nMel, "fb_start"); a.fb_len = i32(fb_len, nMel, "fb_len"); a.fb_off = i32(fb_off, nMel, "fb_off");
    STD_TORCH_CHECK(fb_len.numel() == nMel && fb_off.numel() == nMel, "semicrf: `fb_start` / `fb_len` / `fb_off` must have one entry per band");
    a.fb_val = f32(fb_val, total, "fb_val");
    if (has_gain) {
        a.shift = f32(shift, N, "shift"); a.denom = f32(denom, N, "denom");
        STD_TORCH_CHECK(shift.numel() == N && denom.numel() == N, "semicrf: `shift` / `denom` must have one entry per recording");
    }
    const int64_t on = N * (to_mono ? 1 : C) * nFrame * nMel * nWin;
    a.out = f32w(out, on, "out");
    STD_TORCH_CHECK(out.numel() == on, "semicrf: `out` must be [N, C or 1, nFrame, nMel, nWin]");
    a.frames = frames.numel() > 0 ? (const float*)frames.data_ptr() : nullptr;
    return a;
}
void log_mel_op(Tensor frames, Tensor windows, Tensor tw, Tensor fb_start, Tensor fb_len, Tensor fb_off, Tensor fb_val, int64_t max_len,
                Tensor shift, Tensor denom, bool has_gain, bool log_flag, double eps, bool to_mono, Tensor out)
{
    Ctx c(frames); c.same(frames, windows, tw, fb_start, fb_len, fb_off, fb_val, out);
    if (has_gain) c.same(frames, shift, denom);
    const LogMelCall a = log_mel_args(frames, windows, tw, fb_start, fb_len, fb_off, fb_val, max_len, shift, denom, has_gain, to_mono, out);
    if (a.N == 0 || a.nFrame == 0) return;
    check(semicrf_log_mel(a.frames, a.st[0], a.st[1], a.st[2], a.N, a.C, a.nFrame, a.W, a.windows, a.nWin, a.tw, a.fb_start, a.fb_len, a.fb_off,
                          a.fb_val, a.nMel, a.total, a.shift, a.denom, log_flag ? 1 : 0, (float)eps, to_mono ? 1 : 0, a.out, c.stream),
          "semicrf_log_mel");
}
void log_mel_cpu(Tensor frames, Tensor windows, Tensor tw, Tensor fb_start, Tensor fb_len, Tensor fb_off, Tensor fb_val, int64_t max_len,
                 Tensor shift, Tensor denom, bool has_gain, bool log_flag, double eps, bool to_mono, Tensor out)
{
    all_cpu(frames, windows, tw, fb_start, fb_len, fb_off, fb_val, out);
    if (has_gain) all_cpu(shift, denom);
    const LogMelCall a = log_mel_args(frames, windows, tw, fb_start, fb_len, fb_off, fb_val, max_len, shift, denom, has_gain, to_mono, out);
    if (a.N == 0 || a.nFrame == 0) return;
    STD_TORCH_CHECK(!log_flag || eps > 0.0, "semicrf: log_mel: eps must be positive for the log compression");
    const int64_t fext = (a.N - 1) * a.st[0] + (a.C - 1) * a.st[1] + (a.nFrame - 1) * a.st[2] + a.W;
    STD_TORCH_CHECK(a.frames + fext <= a.out || a.out + out.numel() <= a.frames, "semicrf: log_mel: `out` overlaps `frames`");
    semicrf_cpu::log_mel(a.frames, a.st[0], a.st[1], a.st[2], a.N, a.C, a.nFrame, a.W, a.windows, a.nWin, a.tw, a.fb_start, a.fb_len, a.fb_off,
                         a.fb_val, a.nMel, a.total, a.shift, a.denom, log_flag ? 1 : 0, (float)eps, to_mono ? 1 : 0, a.out);
}

// its backward (semicrf_axial_attention_bwd): q, out, dout, dq [n0, n1, Lq, H d]; k, v, dk, dv [n0, n1, Lk, H d], all views with their
// own strides; a gradient that is not wanted is None (a NULL pointer: nothing is computed for it)
struct AttentionBwdArgs { const float *q, *k, *v, *out, *dout; float *dq, *dk, *dv; int64_t n0, n1; int Lq, Lk, H, d; int64_t st[24]; };
inline AttentionBwdArgs attention_bwd_args(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& out, const Tensor& dout,
                                           const std::optional<Tensor>& dq, const std::optional<Tensor>& dk, const std::optional<Tensor>& dv,
                                           int64_t H)
{
    const Tensor* ts[8] = {&q, &k, &v, &out, &dout, dq ? &*dq : nullptr, dk ? &*dk : nullptr, dv ? &*dv : nullptr};
    const char* names[8] = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"};
    const bool on_q[8] = {true, false, false, true, true, true, false, false};
    AttentionBwdArgs a{};
    STD_TORCH_CHECK(q.defined() && q.dim() == 4, "semicrf: `q` must be [n0, n1, Lq, H * d]");
    a.n0 = q.size(0); a.n1 = q.size(1);
    const int64_t Lq = q.size(2), Lk = k.defined() && k.dim() == 4 ? k.size(2) : -1, HD = q.size(3);
    STD_TORCH_CHECK(H >= 1 && H < (1 << 20) && HD % H == 0, "semicrf: the last dimension must be H * d");
    for (int i = 0; i < 8; ++i) {
        if (!ts[i]) continue;
        const Tensor& t = *ts[i];
        STD_TORCH_CHECK(t.defined() && t.scalar_type() == ScalarType::Float && t.dim() == 4, "semicrf: `", names[i], "` must be a 4-d float32 tensor");
        STD_TORCH_CHECK(t.size(0) == a.n0 && t.size(1) == a.n1 && t.size(3) == HD && t.size(2) == (on_q[i] ? Lq : Lk),
                        "semicrf: `", names[i], "` does not have the shape of the call");
        STD_TORCH_CHECK(HD == 1 || t.stride(3) == 1, "semicrf: `", names[i], "` must have a contiguous last dimension");
        for (int j = 0; j < 3; ++j) {
            const int64_t s = t.size(j) > 1 ? t.stride(j) : 0;
            STD_TORCH_CHECK(s >= 0, "semicrf: negative stride");
            STD_TORCH_CHECK(i < 3 || t.size(j) == 1 || s > 0, "semicrf: `", names[i], "` must not repeat over a dimension");
            a.st[3 * i + j] = s;
        }
    }
    STD_TORCH_CHECK(Lq < (1 << 20) && Lk < (1 << 20), "semicrf: sequence too long");
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H; a.d = (int)(HD / H);
    STD_TORCH_CHECK(semicrf_axial_attention_bwd_supported(a.Lq, a.Lk, a.H, a.d),
                    "semicrf: axial_attention_bwd does not support Lq=", Lq, " Lk=", Lk, " H=", H, " d=", HD / H,
                    " (semicrf_axial_attention_bwd_supported)");
    a.q = f32s(q, "q"); a.k = f32s(k, "k"); a.v = f32s(v, "v"); a.out = f32s(out, "out"); a.dout = f32s(dout, "dout");
    a.dq = dq ? f32so(*dq, "dq") : nullptr; a.dk = dk ? f32so(*dk, "dk") : nullptr; a.dv = dv ? f32so(*dv, "dv") : nullptr;
    return a;
}
void axial_attention_bwd_op(Tensor q, Tensor k, Tensor v, Tensor out, Tensor dout, std::optional<Tensor> dq, std::optional<Tensor> dk,
                            std::optional<Tensor> dv, int64_t H)
{
    Ctx c(q); c.same(q, k, v, out, dout);
    if (dq) c.same(q, *dq);
    if (dk) c.same(q, *dk);
    if (dv) c.same(q, *dv);
    const AttentionBwdArgs a = attention_bwd_args(q, k, v, out, dout, dq, dk, dv, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    const int64_t* s = a.st;
    check(semicrf_axial_attention_bwd(a.q, a.k, a.v, a.out, a.dout, a.dq, a.dk, a.dv, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, s[0], s[1], s[2], s[3],
                                      s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15], s[16], s[17], s[18],
                                      s[19], s[20], s[21], s[22], s[23], c.stream),
          "semicrf_axial_attention_bwd");
}
void axial_attention_bwd_cpu(Tensor q, Tensor k, Tensor v, Tensor out, Tensor dout, std::optional<Tensor> dq, std::optional<Tensor> dk,
                             std::optional<Tensor> dv, int64_t H)
{
    all_cpu(q, k, v, out, dout);
    if (dq) all_cpu(*dq);
    if (dk) all_cpu(*dk);
    if (dv) all_cpu(*dv);
    const AttentionBwdArgs a = attention_bwd_args(q, k, v, out, dout, dq, dk, dv, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    semicrf_cpu::axial_attention_bwd(a.q, a.k, a.v, a.out, a.dout, a.dq, a.dk, a.dv, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, a.st);
}

// the backward of the bf16 op (semicrf_axial_attention_bf16_bwd): the views and checks of axial_attention_bwd with bfloat16 tensors and
// without `out` -- q, dout, dq [n0, n1, Lq, H d]; k, v, dk, dv [n0, n1, Lk, H d]
struct AttentionBf16BwdArgs { const uint16_t *q, *k, *v, *dout; uint16_t *dq, *dk, *dv; int64_t n0, n1; int Lq, Lk, H, d; int64_t st[21]; };
inline AttentionBf16BwdArgs attention_bf16_bwd_args(const Tensor& q, const Tensor& k, const Tensor& v, const Tensor& dout,
                                                    const std::optional<Tensor>& dq, const std::optional<Tensor>& dk,
                                                    const std::optional<Tensor>& dv, int64_t H)
{
    const Tensor* ts[7] = {&q, &k, &v, &dout, dq ? &*dq : nullptr, dk ? &*dk : nullptr, dv ? &*dv : nullptr};
    const char* names[7] = {"q", "k", "v", "dout", "dq", "dk", "dv"};
    const bool on_q[7] = {true, false, false, true, true, false, false};
    AttentionBf16BwdArgs a{};
    STD_TORCH_CHECK(q.defined() && q.dim() == 4, "semicrf: `q` must be [n0, n1, Lq, H * d]");
    a.n0 = q.size(0); a.n1 = q.size(1);
    const int64_t Lq = q.size(2), Lk = k.defined() && k.dim() == 4 ? k.size(2) : -1, HD = q.size(3);
    STD_TORCH_CHECK(H >= 1 && H < (1 << 20) && HD % H == 0, "semicrf: the last dimension must be H * d");
    const void* ptrs[7] = {};
    for (int i = 0; i < 7; ++i) {
        if (!ts[i]) continue;
        const Tensor& t = *ts[i];
        STD_TORCH_CHECK(t.defined() && t.scalar_type() == ScalarType::BFloat16 && t.dim() == 4, "semicrf: `", names[i],
                        "` must be a 4-d bfloat16 tensor");
        STD_TORCH_CHECK(t.size(0) == a.n0 && t.size(1) == a.n1 && t.size(3) == HD && t.size(2) == (on_q[i] ? Lq : Lk),
                        "semicrf: `", names[i], "` does not have the shape of the call");
        STD_TORCH_CHECK(HD == 1 || t.stride(3) == 1, "semicrf: `", names[i], "` must have a contiguous last dimension");
        for (int j = 0; j < 3; ++j) {
            const int64_t s = t.size(j) > 1 ? t.stride(j) : 0;
            STD_TORCH_CHECK(s >= 0, "semicrf: negative stride");
            STD_TORCH_CHECK(i < 3 || t.size(j) == 1 || s > 0, "semicrf: `", names[i], "` must not repeat over a dimension");
            a.st[3 * i + j] = s;
        }
        ptrs[i] = t.numel() > 0 ? t.data_ptr() : nullptr;
    }
    STD_TORCH_CHECK(Lq < (1 << 20) && Lk < (1 << 20), "semicrf: sequence too long");
    a.Lq = (int)Lq; a.Lk = (int)Lk; a.H = (int)H; a.d = (int)(HD / H);
    STD_TORCH_CHECK(semicrf_axial_attention_bf16_bwd_supported(a.Lq, a.Lk, a.H, a.d),
                    "semicrf: axial_attention_bf16_bwd does not support Lq=", Lq, " Lk=", Lk, " H=", H, " d=", HD / H,
                    " (semicrf_axial_attention_bf16_bwd_supported)");
    a.q = (const uint16_t*)ptrs[0]; a.k = (const uint16_t*)ptrs[1]; a.v = (const uint16_t*)ptrs[2]; a.dout = (const uint16_t*)ptrs[3];
    a.dq = (uint16_t*)ptrs[4]; a.dk = (uint16_t*)ptrs[5]; a.dv = (uint16_t*)ptrs[6];
    return a;
}
void axial_attention_bf16_bwd_op(Tensor q, Tensor k, Tensor v, Tensor dout, std::optional<Tensor> dq, std::optional<Tensor> dk,
                                 std::optional<Tensor> dv, int64_t H)
{
    Ctx c(q); c.same(q, k, v, dout);
    if (dq) c.same(q, *dq);
    if (dk) c.same(q, *dk);
    if (dv) c.same(q, *dv);
    const AttentionBf16BwdArgs a = attention_bf16_bwd_args(q, k, v, dout, dq, dk, dv, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    const int64_t* s = a.st;
    check(semicrf_axial_attention_bf16_bwd(a.q, a.k, a.v, a.dout, a.dq, a.dk, a.dv, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, s[0], s[1], s[2], s[3], s[4],
                                           s[5], s[6], s[7], s[8], s[9], s[10], s[11], s[12], s[13], s[14], s[15], s[16], s[17], s[18], s[19],
                                           s[20], c.stream),
          "semicrf_axial_attention_bf16_bwd");
}
void axial_attention_bf16_bwd_cpu(Tensor q, Tensor k, Tensor v, Tensor dout, std::optional<Tensor> dq, std::optional<Tensor> dk,
                                  std::optional<Tensor> dv, int64_t H)
{
    all_cpu(q, k, v, dout);
    if (dq) all_cpu(*dq);
    if (dk) all_cpu(*dk);
    if (dv) all_cpu(*dv);
    const AttentionBf16BwdArgs a = attention_bf16_bwd_args(q, k, v, dout, dq, dk, dv, H);
    if (a.n0 == 0 || a.n1 == 0) return;
    semicrf_cpu::axial_attention_bf16_bwd(a.q, a.k, a.v, a.dout, a.dq, a.dk, a.dv, a.n0, a.n1, a.Lq, a.Lk, a.H, a.d, a.st);
}

// ---- the attribute heads in training (semicrf_attribute_heads_train_fwd / _bwd / _dropout_mask) -------------------------------------
// seed: the 64 bits of an int; z [K, Hv + Ho] and the gradients are dense and checked for their element counts
void attribute_heads_train_fwd_op(Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K, Tensor offsets, int64_t nSym,
                                  Tensor W1, Tensor b1, Tensor W2, Tensor b2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, int64_t seed,
                                  double pv, double po, Tensor logitsVelocity, Tensor ofLogits, Tensor z, Tensor symIdx, Tensor scatterIdx,
                                  Tensor ws)
{
    Ctx c(ctx); c.same(ctx, pairs, offsets, W1, b1, W2, b2, logitsVelocity, ofLogits, z, symIdx, scatterIdx, ws);
    const AttrHeadsArgs a = attr_heads_args(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                                            symIdx, scatterIdx);
    float* zp = f32w(z, K * (Hv + Ho), "z");
    if (K == 0) return;
    check(semicrf_attribute_heads_train_fwd(a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, (int)nSym, a.W1, a.b1, a.W2, a.b2, (int)Hv,
                                            (int)Ho, (int)Nv, (int)No, (uint64_t)seed, pv, po, a.lv, a.of, zp, a.sym, a.sc, bytes(ws, "ws"),
                                            (size_t)ws.numel(), c.stream),
          "semicrf_attribute_heads_train_fwd");
}
void attribute_heads_train_fwd_cpu(Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K, Tensor offsets, int64_t nSym,
                                   Tensor W1, Tensor b1, Tensor W2, Tensor b2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, int64_t seed,
                                   double pv, double po, Tensor logitsVelocity, Tensor ofLogits, Tensor z, Tensor symIdx, Tensor scatterIdx,
                                   Tensor ws)
{
    all_cpu(ctx, pairs, offsets, W1, b1, W2, b2, logitsVelocity, ofLogits, z, symIdx, scatterIdx, ws);
    const AttrHeadsArgs a = attr_heads_args(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                                            symIdx, scatterIdx);
    float* zp = f32w(z, K * (Hv + Ho), "z");
    STD_TORCH_CHECK(pv >= 0.0 && pv < 1.0 && po >= 0.0 && po < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    if (K == 0) return;
    semicrf_cpu::attribute_heads_train_fwd(a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, (int)nSym, a.W1, a.b1, a.W2, a.b2, (int)Hv,
                                           (int)Ho, (int)Nv, (int)No, (uint64_t)seed, pv, po, a.lv, a.of, zp, a.sym, a.sc);
}

struct AttrHeadsBwdArgs { const float *dlv, *dof, *z, *ctx, *W1, *W2; const int32_t *pairs, *off; float *dctx, *dW1, *db1, *dW2, *db2; };
inline AttrHeadsBwdArgs attr_heads_bwd_args(const Tensor& dLv, const Tensor& dOf, const Tensor& z, const Tensor& ctx, int64_t C, int64_t T,
                                            int64_t D, int64_t ldc, const Tensor& pairs, int64_t K, const Tensor& offsets, const Tensor& W1,
                                            const Tensor& W2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, double pv, double po,
                                            const Tensor& dctx, const Tensor& dW1, const Tensor& db1, const Tensor& dW2, const Tensor& db2)
{
    score_dims(C, T, D);
    STD_TORCH_CHECK(K >= 0 && K < (1ll << 31) && ldc >= D && C * T < (1ll << 31), "semicrf: bad interval count / row stride / C * T");
    STD_TORCH_CHECK(Hv >= 1 && Ho >= 1 && Nv >= 1 && No >= 1 && Hv < (1 << 21) && Ho < (1 << 21) && Nv < (1 << 20) && No < (1 << 20),
                    "semicrf: bad head sizes");
    STD_TORCH_CHECK(pv >= 0.0 && pv < 1.0 && po >= 0.0 && po < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    STD_TORCH_CHECK(ctx.dim() == 3 && ctx.size(0) == C && ctx.size(1) == T && ctx.size(2) == D, "semicrf: `ctx` must be [C, T, D]");
    STD_TORCH_CHECK((D == 1 || ctx.stride(2) == 1) && (T == 1 || ctx.stride(1) == ldc) && (C == 1 || ctx.stride(0) == T * ldc),
                    "semicrf: `ctx` must be [C][T] rows of ldc floats with unit stride inside a row");
    const int64_t H = Hv + Ho;
    return AttrHeadsBwdArgs{f32(dLv, K * Nv, "dLogitsVelocity"), f32(dOf, K * No, "dOfLogits"), f32(z, K * H, "z"), f32s(ctx, "ctx"),
                            f32(W1, 3 * D * H, "W1"), f32(W2, Hv * Nv + Ho * No, "W2"), i32(pairs, 2 * K, "pairs"),
                            i32(offsets, C + 1, "offsets"), f32w(dctx, C * T * D, "dctx"), f32w(dW1, 3 * D * H, "dW1"), f32w(db1, H, "db1"),
                            f32w(dW2, Hv * Nv + Ho * No, "dW2"), f32w(db2, Nv + No, "db2")};
}
void attribute_heads_bwd_op(Tensor dLv, Tensor dOf, Tensor z, Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K,
                            Tensor offsets, Tensor W1, Tensor W2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, int64_t seed, double pv,
                            double po, Tensor dctx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor ws)
{
    Ctx c(ctx); c.same(ctx, dLv, dOf, z, pairs, offsets, W1, W2, dctx, dW1, db1, dW2, db2, ws);
    const AttrHeadsBwdArgs a = attr_heads_bwd_args(dLv, dOf, z, ctx, C, T, D, ldc, pairs, K, offsets, W1, W2, Hv, Ho, Nv, No, pv, po, dctx, dW1,
                                                   db1, dW2, db2);
    if (K == 0) return;
    check(semicrf_attribute_heads_bwd(a.dlv, a.dof, a.z, a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, a.W1, a.W2, (int)Hv, (int)Ho,
                                      (int)Nv, (int)No, (uint64_t)seed, pv, po, a.dctx, a.dW1, a.db1, a.dW2, a.db2, bytes(ws, "ws"),
                                      (size_t)ws.numel(), c.stream),
          "semicrf_attribute_heads_bwd");
}
void attribute_heads_bwd_cpu(Tensor dLv, Tensor dOf, Tensor z, Tensor ctx, int64_t C, int64_t T, int64_t D, int64_t ldc, Tensor pairs, int64_t K,
                             Tensor offsets, Tensor W1, Tensor W2, int64_t Hv, int64_t Ho, int64_t Nv, int64_t No, int64_t seed, double pv,
                             double po, Tensor dctx, Tensor dW1, Tensor db1, Tensor dW2, Tensor db2, Tensor ws)
{
    all_cpu(ctx, dLv, dOf, z, pairs, offsets, W1, W2, dctx, dW1, db1, dW2, db2, ws);
    const AttrHeadsBwdArgs a = attr_heads_bwd_args(dLv, dOf, z, ctx, C, T, D, ldc, pairs, K, offsets, W1, W2, Hv, Ho, Nv, No, pv, po, dctx, dW1,
                                                   db1, dW2, db2);
    if (K == 0) return;
    semicrf_cpu::attribute_heads_bwd(a.dlv, a.dof, a.z, a.ctx, (int)C, (int)T, (int)D, ldc, a.pairs, K, a.off, a.W1, a.W2, (int)Hv, (int)Ho,
                                     (int)Nv, (int)No, (uint64_t)seed, pv, po, a.dctx, a.dW1, a.db1, a.dW2, a.db2);
}

inline unsigned char* mask_args(const Tensor& mask, int64_t K, int64_t Hv, int64_t Ho, double pv, double po)
{
    STD_TORCH_CHECK(K >= 0 && K < (1ll << 31) && Hv >= 1 && Ho >= 1 && Hv < (1 << 21) && Ho < (1 << 21), "semicrf: bad mask shape");
    STD_TORCH_CHECK(pv >= 0.0 && pv < 1.0 && po >= 0.0 && po < 1.0, "semicrf: dropout probabilities must lie in [0, 1)");
    want(mask, ScalarType::Byte, K * (Hv + Ho), "mask");
    return K > 0 ? (unsigned char*)mask.data_ptr() : nullptr;
}
void attribute_heads_dropout_mask_op(Tensor mask, int64_t seed, int64_t K, int64_t Hv, int64_t Ho, double pv, double po)
{
    Ctx c(mask);
    unsigned char* m = mask_args(mask, K, Hv, Ho, pv, po);
    if (K == 0) return;
    check(semicrf_attribute_heads_dropout_mask((uint64_t)seed, K, (int)Hv, (int)Ho, pv, po, m, c.stream), "semicrf_attribute_heads_dropout_mask");
}
void attribute_heads_dropout_mask_cpu(Tensor mask, int64_t seed, int64_t K, int64_t Hv, int64_t Ho, double pv, double po)
{
    all_cpu(mask);
    unsigned char* m = mask_args(mask, K, Hv, Ho, pv, po);
    if (K == 0) return;
    semicrf_cpu::attribute_heads_dropout_mask((uint64_t)seed, K, (int)Hv, (int)Ho, pv, po, m);
}

// ---- transcription segment loop ----------------------------------------------------------------------------------------
void segment_onset_filter_op(Tensor pairs, Tensor offsets, int64_t B, int64_t bound, Tensor pairs_out, Tensor offsets_out, Tensor counts_ws)
{
    Ctx c(offsets); c.same(offsets, pairs, pairs_out, offsets_out, counts_ws);
    STD_TORCH_CHECK(B >= 1 && B < (1ll << 31), "semicrf: bad B");
    check(segment_onset_filter(i32(pairs, 0, "pairs"), i32(offsets, B + 1, "offsets"), (int)B, (int)bound, i32(pairs_out, 0, "pairs_out"),
                               pairs_out.numel() / 2, i32(offsets_out, B + 1, "offsets_out"), i32(counts_ws, B, "counts_ws"), c.stream),
          "segment_onset_filter");
}
void segment_events_op(Tensor pairs, int64_t K, Tensor offsets, int64_t B, int64_t nSym, Tensor ofValue, Tensor ofPresence,
                       int64_t lastFrameIdx, double frameDur, Tensor beginTime, int64_t stepFrames, Tensor times, Tensor flags, Tensor lastP,
                       Tensor nextStart)
{
    Ctx c(offsets); c.same(offsets, pairs, ofValue, ofPresence, beginTime, times, flags, lastP, nextStart);
    STD_TORCH_CHECK(B >= 1 && B < (1ll << 31) && nSym >= 1 && K >= 0, "semicrf: bad B / nSym / K");
    want(ofPresence, ScalarType::Byte, 2 * K, "ofPresence"); want(flags, ScalarType::Byte, 2 * K, "flags");
    want(beginTime, ScalarType::Double, B / nSym, "beginTime"); want(times, ScalarType::Double, 2 * K, "times");
    check(segment_events(i32(pairs, 2 * K, "pairs"), K, i32(offsets, B + 1, "offsets"), (int)B, (int)nSym, f32(ofValue, 2 * K, "ofValue"),
                         K > 0 ? (const unsigned char*)ofPresence.data_ptr() : nullptr, (int)lastFrameIdx, frameDur,
                         (const double*)beginTime.data_ptr(), (int)stepFrames, K > 0 ? (double*)times.data_ptr() : nullptr,
                         K > 0 ? (unsigned char*)flags.data_ptr() : nullptr, i32(lastP, B, "lastP"), i32(nextStart, B, "nextStart"), c.stream),
          "segment_events");
}

}  // namespace

STABLE_TORCH_LIBRARY(semicrf, m)
{
    m.def("logz_fwd(Tensor score, Tensor noise, Tensor(a!) logZ, Tensor(b!) v, bool want_v, Tensor(c!) ws) -> ()");
    m.def("logz_bwd(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, Tensor(a!) dScore, Tensor(b!) dNoise, Tensor(c!) q, "
          "bool want_q, int flags, Tensor(d!) ws) -> ()");
    m.def("beta(Tensor score, Tensor noise, Tensor(a!) out, Tensor(b!) ws) -> ()");
    m.def("alpha_from(Tensor score, Tensor noise, Tensor start, Tensor(a!) v, Tensor(b!) logz, Tensor(c!) ws) -> ()");
    m.def("viterbi(Tensor score, Tensor noise, Tensor start, bool has_start, bool forward, Tensor(a!) pairs, Tensor(b!) offsets, "
          "Tensor(c!) ws) -> ()");
    m.def("sample(Tensor score, Tensor noise, Tensor v, int k0, int nSample, int key, Tensor end, bool has_end, Tensor(a!) pairs, "
          "Tensor(b!) offsets, Tensor(c!) ws) -> ()");
    m.def("viterbi_nbest(Tensor score, Tensor noise, int k, Tensor start, bool has_start, bool forward, Tensor(a!) pairs, "
          "Tensor(b!) offsets, Tensor(c!) scores, Tensor(d!) npaths, Tensor(e!) ws) -> ()");
    m.def("posteriors(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor(a!) node, Tensor(b!) begin, Tensor(c!) end, "
          "Tensor(d!) single, Tensor(e!) noiseP, Tensor(f!) entropy, Tensor(g!) ws) -> ()");
    m.def("expectation(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor v, Tensor q, Tensor(a!) E, Tensor(b!) H, "
          "Tensor(c!) ws) -> ()");
    m.def("covariance(Tensor score, Tensor noise, Tensor weight, Tensor nweight, bool has_nw, Tensor gout, Tensor(a!) C, Tensor(b!) Cn, "
          "Tensor ws) -> ()");
    m.def("interval_marginals(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int K, Tensor offsets, Tensor(a!) out) -> ()");
    m.def("marginal_decode(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, Tensor(a!) pairs, Tensor(b!) probs, "
          "Tensor(c!) offsets, Tensor(d!) ws) -> ()");
    m.def("interval_marginals_tol(Tensor score, Tensor v, Tensor q, Tensor logZ, Tensor pairs, int K, Tensor offsets, int tol_begin, "
          "int tol_end, Tensor(a!) out) -> ()");
    m.def("marginal_decode_tol(Tensor score, Tensor noise, Tensor v, Tensor q, Tensor logZ, Tensor tau, int tol_begin, int tol_end, "
          "Tensor(a!) pairs, Tensor(b!) probs, Tensor(c!) offsets, Tensor(d!) ws) -> ()");
    m.def("mbr_select(Tensor pairs, Tensor weight, Tensor offsets, int T, Tensor tau, Tensor(a!) pairs_out, Tensor(b!) probs_out, "
          "Tensor(c!) offsets_out, Tensor(d!) gain, Tensor(e!) ws) -> ()");
    m.def("compare_paths(Tensor est_pairs, Tensor est_offsets, Tensor ref_pairs, Tensor ref_offsets, int T, int tol_begin, int tol_end, "
          "Tensor(a!) stats) -> ()");
    m.def("eval_path(Tensor score, Tensor noise, Tensor pairs, int K, Tensor offsets, Tensor(a!) out, Tensor(b!) ws) -> ()");
    m.def("eval_path_bwd(Tensor gout, int T, int B, Tensor pairs, int K, Tensor offsets, Tensor(a!) dScore, bool has_ds, Tensor(b!) dNoise, "
          "bool has_dn) -> ()");
    m.def("logprob_fwd(Tensor score, Tensor noise, Tensor pairs, int K, Tensor offsets, Tensor(a!) logProb, Tensor(b!) logZ, Tensor(c!) v, "
          "bool want_v, Tensor(d!) ws, Tensor(e!) ptab, bool has_ptab) -> ()");
    m.def("logprob_bwd(Tensor score, Tensor noise, Tensor v, Tensor logZ, Tensor gout, int gstride, Tensor pairs, int K, Tensor offsets, "
          "Tensor(a!) dScore, Tensor(b!) dNoise, int flags, Tensor(c!) ws, Tensor ptab, bool has_ptab) -> ()");
    // (group, pitch): the slot layout of the chain axis (include/semicrf_hip.h, *_p entry points); group == pitch: contiguous
    // rowc / drowc, ldrc / lddrc: the merged projection's per-(chain, end) constant (*_pc entry points); stride 0: none (pass any tensor)
    m.def("interval_score_fwd(Tensor q, Tensor k, Tensor diag, Tensor rowc, int C, int T, int D, int ldq, int ldk, int ldd, int ldrc, "
          "float qscale, int mode, int full, int group, int pitch, Tensor(a!) S, Tensor(b!) noise) -> ()");
    m.def("interval_score_bwd_ws(Tensor dS, Tensor q, Tensor k, int C, int T, int D, int ldq, int ldk, float qscale, int mode, int group, "
          "int pitch, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) ddiag, Tensor(d!) drowc, int lddq, int lddk, int lddd, int lddrc, "
          "Tensor(e!) ws) -> ()");
    m.def("interval_score_bwd_fused_ws(Tensor S, Tensor alpha, Tensor beta, Tensor logZ, Tensor gout, Tensor q, Tensor k, int C, int T, int D, "
          "int ldq, int ldk, float qscale, int mode, int group, int pitch, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) ddiag, Tensor(d!) drowc, "
          "int lddq, int lddk, int lddd, int lddrc, Tensor(e!) ws) -> ()");
    m.def("interval_score_path_bwd(Tensor gout, Tensor pairs, int K, Tensor offsets, Tensor q, Tensor k, int C, int T, int D, int ldq, int ldk, "
          "float qscale, int mode, int group, int pitch, Tensor(a!) dq, Tensor(b!) dk, Tensor(c!) ddiag, Tensor(d!) drowc, int lddq, int lddk, "
          "int lddd, int lddrc) -> ()");
    m.def("proj_nn(Tensor A, int lda, int M, int K, Tensor B, int ldb, int N, Tensor(a!) out, int ldout, Tensor bias, bool has_bias, Tensor w2, "
          "Tensor b2, bool has_w2, int zero_cols, bool accumulate) -> ()");
    m.def("proj_nn3(Tensor A, int lda, int M, int K, Tensor B, int ldb, int N, Tensor(a!) out, int ldout, Tensor bias, bool has_bias, Tensor w2, "
          "Tensor b2, bool has_w2, int zero_cols, bool accumulate, Tensor(b!) ws) -> ()");
    m.def("stage_linear(Tensor W, Tensor bias, int D, int size, int rows_pad, Tensor(a!) BT, Tensor(b!) Wqd, Tensor(c!) w2, Tensor(d!) b2) -> ()");
    m.def("merge_weights_fwd(Tensor W, Tensor bias, int D, int size, int rows, Tensor(a!) Wm, Tensor(b!) bm, Tensor(c!) WmT, bool has_t) -> ()");
    m.def("merge_weights_bwd(Tensor W, Tensor bias, Tensor dWm, Tensor dbm, int D, int size, int rows, Tensor(a!) dW, Tensor(b!) dbias, Tensor(c!) ws) -> ()");
    m.def("proj_tn(Tensor dy, int lddy, int M, int R, int extra_col0, int total_rows, Tensor x, int ldx, int N, Tensor(a!) dW, int lddw, "
          "Tensor(b!) db, Tensor(c!) ws) -> ()");
    m.def("interval_features_gather(Tensor ctx, int C, int T, int D, int ldc, Tensor pairs, int K, Tensor offsets, int nSym, Tensor(a!) out, "
          "Tensor(b!) symIdx, Tensor(c!) scatterIdx) -> ()");
    m.def("interval_features_gather_bwd(Tensor gout, Tensor ctx, int C, int T, int D, int ldc, Tensor pairs, int K, Tensor offsets, "
          "Tensor(a!) dctx, int lddc) -> ()");
    m.def("attribute_loss_fwd(Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined, Tensor ofPresence, int K, "
          "Tensor offsets, int C, Tensor base, bool has_base, Tensor(a!) rowLogProb, Tensor(b!) out) -> ()");
    m.def("attribute_loss_bwd(Tensor gout, int gstride, Tensor logitsVelocity, Tensor ofLogits, Tensor velocity, Tensor ofRefined, "
          "Tensor ofPresence, int K, Tensor offsets, int C, Tensor(a!) dLogitsVelocity, Tensor(b!) dOfLogits) -> ()");
    m.def("attribute_decode(Tensor logitsVelocity, Tensor ofLogits, int K, int criterion, Tensor(a!) velocityClass, Tensor(b!) velocityMean, "
          "Tensor(c!) ofValue, Tensor(d!) ofPresence) -> ()");
    m.def("attribute_heads(Tensor ctx, int C, int T, int D, int ldc, Tensor pairs, int K, Tensor offsets, int nSym, Tensor W1, Tensor b1, "
          "Tensor W2, Tensor b2, int Hv, int Ho, int Nv, int No, Tensor(a!) logitsVelocity, Tensor(b!) ofLogits, Tensor(c!) symIdx, "
          "Tensor(d!) scatterIdx, Tensor(e!) ws) -> ()");
    m.def("attribute_heads_train_fwd(Tensor ctx, int C, int T, int D, int ldc, Tensor pairs, int K, Tensor offsets, int nSym, Tensor W1, "
          "Tensor b1, Tensor W2, Tensor b2, int Hv, int Ho, int Nv, int No, int seed, float pv, float po, Tensor(a!) logitsVelocity, "
          "Tensor(b!) ofLogits, Tensor(c!) z, Tensor(d!) symIdx, Tensor(e!) scatterIdx, Tensor(f!) ws) -> ()");
    m.def("attribute_heads_bwd(Tensor dLogitsVelocity, Tensor dOfLogits, Tensor z, Tensor ctx, int C, int T, int D, int ldc, Tensor pairs, "
          "int K, Tensor offsets, Tensor W1, Tensor W2, int Hv, int Ho, int Nv, int No, int seed, float pv, float po, Tensor(a!) dctx, "
          "Tensor(b!) dW1, Tensor(c!) db1, Tensor(d!) dW2, Tensor(e!) db2, Tensor(f!) ws) -> ()");
    m.def("attribute_heads_dropout_mask(Tensor(a!) mask, int seed, int K, int Hv, int Ho, float pv, float po) -> ()");
    m.def("axial_attention(Tensor q, Tensor k, Tensor v, Tensor(a!) out, int H) -> ()");
    m.def("axial_attention_bf16(Tensor q, Tensor k, Tensor v, Tensor(a!) out, int H) -> ()");
    m.def("axial_attention_bwd(Tensor q, Tensor k, Tensor v, Tensor out, Tensor dout, Tensor(a!)? dq, Tensor(b!)? dk, Tensor(c!)? dv, int H) -> ()");
    m.def("axial_attention_bf16_bwd(Tensor q, Tensor k, Tensor v, Tensor dout, Tensor(a!)? dq, Tensor(b!)? dk, Tensor(c!)? dv, int H) -> ()");
    m.def("ffn_residual(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, Tensor(a!) out) -> ()");
    m.def("ffn_residual_train_fwd(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, int seed, float p_hidden, "
          "float p_out, Tensor(a!) out, Tensor(b!) z, Tensor(c!) y) -> ()");
    m.def("ffn_residual_bwd(Tensor dout, Tensor x, Tensor z, Tensor y, Tensor W1, Tensor W2, Tensor scale, float eps, int seed, float p_hidden, "
          "float p_out, Tensor(a!) dx, Tensor(b!) dW1, Tensor(c!) db1, Tensor(d!) dW2, Tensor(e!) db2, Tensor(f!) dscale, Tensor ws) -> ()");
    m.def("ffn_dropout_mask(Tensor(a!) mask_hidden, Tensor(b!) mask_out, int seed, int rows, int D, int hidden, float p_hidden, float p_out) "
          "-> ()");
    m.def("ffn_residual_bf16(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, Tensor(a!) out) -> ()");
    m.def("ffn_residual_bf16_mixed(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, Tensor(a!) out) -> ()");
    m.def("ffn_residual_bf16_train_fwd(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, int seed, float p_hidden, "
          "float p_out, Tensor(a!) out, Tensor(b!) saved) -> ()");
    m.def("ffn_residual_bf16_mixed_train_fwd(Tensor x, Tensor W1, Tensor b1, Tensor W2, Tensor b2, Tensor scale, float eps, int seed, "
          "float p_hidden, float p_out, Tensor(a!) out, Tensor(b!) saved) -> ()");
    m.def("ffn_residual_bf16_bwd(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, float eps, int seed, float p_hidden, "
          "float p_out, Tensor(a!) dx, Tensor(b!) dW1, Tensor(c!) db1, Tensor(d!) dW2, Tensor(e!) db2, Tensor(f!) dscale, Tensor(g!) ws) -> ()");
    m.def("ffn_residual_bf16_mixed_bwd(Tensor dout, Tensor x, Tensor saved, Tensor W1, Tensor W2, Tensor scale, float eps, int seed, "
          "float p_hidden, float p_out, Tensor(a!) dx, Tensor(b!) dW1, Tensor(c!) db1, Tensor(d!) dW2, Tensor(e!) db2, Tensor(f!) dscale, "
          "Tensor(g!) ws) -> ()");
    m.def("log_mel(Tensor frames, Tensor windows, Tensor tw, Tensor fb_start, Tensor fb_len, Tensor fb_off, Tensor fb_val, int max_len, "
          "Tensor shift, Tensor denom, bool has_gain, bool log_flag, float eps, bool to_mono, Tensor(a!) out) -> ()");
    m.def("grad_sqnorm(Tensor flat, int numel, Tensor(a!) partials) -> ()");
    m.def("clip_from_history(Tensor partials, bool has_partials, int numel, Tensor norm_in, bool has_norm, float q, Tensor(a!) ring, "
          "int capacity, Tensor(b!) state, bool append, Tensor(c!) stats) -> ()");
    m.def("adabelief_step(Tensor(a!) p, Tensor g, Tensor(b!) m, Tensor(c!) s, int numel, Tensor coef, bool has_coef, Tensor table) -> ()");
    m.def("segment_onset_filter(Tensor pairs, Tensor offsets, int B, int bound, Tensor(a!) pairs_out, Tensor(b!) offsets_out, "
          "Tensor(c!) counts_ws) -> ()");
    m.def("segment_events(Tensor pairs, int K, Tensor offsets, int B, int nSym, Tensor ofValue, Tensor ofPresence, int lastFrameIdx, "
          "float frameDur, Tensor beginTime, int stepFrames, Tensor(a!) times, Tensor(b!) flags, Tensor(c!) lastP, Tensor(d!) nextStart) -> ()");
}

STABLE_TORCH_LIBRARY_IMPL(semicrf, CPU, m)
{
    m.impl("logz_fwd", TORCH_BOX(&logz_fwd_cpu));
    m.impl("logz_bwd", TORCH_BOX(&logz_bwd_cpu));
    m.impl("beta", TORCH_BOX(&beta_cpu));
    m.impl("alpha_from", TORCH_BOX(&alpha_from_cpu));
    m.impl("viterbi", TORCH_BOX(&viterbi_cpu));
    m.impl("sample", TORCH_BOX(&sample_cpu));
    m.impl("viterbi_nbest", TORCH_BOX(&viterbi_nbest_cpu));
    m.impl("posteriors", TORCH_BOX(&posteriors_cpu));
    m.impl("interval_marginals", TORCH_BOX(&interval_marginals_cpu));
    m.impl("expectation", TORCH_BOX(&expectation_cpu));
    m.impl("covariance", TORCH_BOX(&covariance_cpu));
    m.impl("marginal_decode", TORCH_BOX(&marginal_decode_cpu));
    m.impl("interval_marginals_tol", TORCH_BOX(&interval_marginals_tol_cpu));
    m.impl("marginal_decode_tol", TORCH_BOX(&marginal_decode_tol_cpu));
    m.impl("mbr_select", TORCH_BOX(&mbr_select_cpu));
    m.impl("compare_paths", TORCH_BOX(&compare_paths_cpu));
    m.impl("eval_path", TORCH_BOX(&eval_path_cpu));
    m.impl("eval_path_bwd", TORCH_BOX(&eval_path_bwd_cpu));
    m.impl("logprob_fwd", TORCH_BOX(&logprob_fwd_cpu));
    m.impl("logprob_bwd", TORCH_BOX(&logprob_bwd_cpu));
    m.impl("attribute_loss_fwd", TORCH_BOX(&attribute_loss_fwd_cpu));
    m.impl("attribute_loss_bwd", TORCH_BOX(&attribute_loss_bwd_cpu));
    m.impl("attribute_decode", TORCH_BOX(&attribute_decode_cpu));
    m.impl("attribute_heads", TORCH_BOX(&attribute_heads_cpu));
    m.impl("attribute_heads_train_fwd", TORCH_BOX(&attribute_heads_train_fwd_cpu));
    m.impl("attribute_heads_bwd", TORCH_BOX(&attribute_heads_bwd_cpu));
    m.impl("attribute_heads_dropout_mask", TORCH_BOX(&attribute_heads_dropout_mask_cpu));
    m.impl("axial_attention", TORCH_BOX(&axial_attention_cpu));
    m.impl("axial_attention_bf16", TORCH_BOX(&axial_attention_bf16_cpu));
    m.impl("axial_attention_bwd", TORCH_BOX(&axial_attention_bwd_cpu));
    m.impl("axial_attention_bf16_bwd", TORCH_BOX(&axial_attention_bf16_bwd_cpu));
    m.impl("ffn_residual", TORCH_BOX(&ffn_residual_cpu));
    m.impl("ffn_residual_train_fwd", TORCH_BOX(&ffn_residual_train_fwd_cpu));
    m.impl("ffn_residual_bwd", TORCH_BOX(&ffn_residual_bwd_cpu));
    m.impl("ffn_dropout_mask", TORCH_BOX(&ffn_dropout_mask_cpu));
    m.impl("ffn_residual_bf16", TORCH_BOX(&ffn_residual_bf16_cpu));
    m.impl("ffn_residual_bf16_mixed", TORCH_BOX(&ffn_residual_bf16_mixed_cpu));
    m.impl("ffn_residual_bf16_train_fwd", TORCH_BOX(&ffn_residual_bf16_train_fwd_cpu));
    m.impl("ffn_residual_bf16_mixed_train_fwd", TORCH_BOX(&ffn_residual_bf16_mixed_train_fwd_cpu));
    m.impl("ffn_residual_bf16_bwd", TORCH_BOX(&ffn_residual_bf16_bwd_cpu));
    m.impl("ffn_residual_bf16_mixed_bwd", TORCH_BOX(&ffn_residual_bf16_mixed_bwd_cpu));
    m.impl("log_mel", TORCH_BOX(&log_mel_cpu));
    m.impl("grad_sqnorm", TORCH_BOX(&grad_sqnorm_cpu));
    m.impl("clip_from_history", TORCH_BOX(&clip_from_history_cpu));
    m.impl("adabelief_step", TORCH_BOX(&adabelief_step_cpu));
}

STABLE_TORCH_LIBRARY_IMPL(semicrf, CUDA, m)
{
    m.impl("logz_fwd", TORCH_BOX(&logz_fwd));
    m.impl("logz_bwd", TORCH_BOX(&logz_bwd));
    m.impl("beta", TORCH_BOX(&beta));
    m.impl("alpha_from", TORCH_BOX(&alpha_from));
    m.impl("viterbi", TORCH_BOX(&viterbi));
    m.impl("sample", TORCH_BOX(&sample));
    m.impl("viterbi_nbest", TORCH_BOX(&viterbi_nbest));
    m.impl("posteriors", TORCH_BOX(&posteriors));
    m.impl("interval_marginals", TORCH_BOX(&interval_marginals));
    m.impl("expectation", TORCH_BOX(&expectation));
    m.impl("covariance", TORCH_BOX(&covariance));
    m.impl("marginal_decode", TORCH_BOX(&marginal_decode));
    m.impl("interval_marginals_tol", TORCH_BOX(&interval_marginals_tol));
    m.impl("marginal_decode_tol", TORCH_BOX(&marginal_decode_tol));
    m.impl("mbr_select", TORCH_BOX(&mbr_select));
    m.impl("compare_paths", TORCH_BOX(&compare_paths));
    m.impl("eval_path", TORCH_BOX(&eval_path));
    m.impl("eval_path_bwd", TORCH_BOX(&eval_path_bwd));
    m.impl("logprob_fwd", TORCH_BOX(&logprob_fwd));
    m.impl("logprob_bwd", TORCH_BOX(&logprob_bwd));
    m.impl("interval_score_fwd", TORCH_BOX(&interval_score_fwd_op));
    m.impl("interval_score_bwd_ws", TORCH_BOX(&interval_score_bwd_ws_op));
    m.impl("interval_score_bwd_fused_ws", TORCH_BOX(&interval_score_bwd_fused_ws_op));
    m.impl("interval_score_path_bwd", TORCH_BOX(&interval_score_path_bwd_op));
    m.impl("proj_nn", TORCH_BOX(&proj_nn_op));
    m.impl("proj_nn3", TORCH_BOX(&proj_nn3_op));
    m.impl("proj_tn", TORCH_BOX(&proj_tn_op));
    m.impl("merge_weights_fwd", TORCH_BOX(&merge_weights_fwd_op));
    m.impl("stage_linear", TORCH_BOX(&stage_linear_op));
    m.impl("merge_weights_bwd", TORCH_BOX(&merge_weights_bwd_op));
    m.impl("interval_features_gather", TORCH_BOX(&interval_features_gather_op));
    m.impl("interval_features_gather_bwd", TORCH_BOX(&interval_features_gather_bwd_op));
    m.impl("attribute_loss_fwd", TORCH_BOX(&attribute_loss_fwd_op));
    m.impl("attribute_loss_bwd", TORCH_BOX(&attribute_loss_bwd_op));
    m.impl("attribute_decode", TORCH_BOX(&attribute_decode_op));
    m.impl("attribute_heads", TORCH_BOX(&attribute_heads_op));
    m.impl("attribute_heads_train_fwd", TORCH_BOX(&attribute_heads_train_fwd_op));
    m.impl("attribute_heads_bwd", TORCH_BOX(&attribute_heads_bwd_op));
    m.impl("attribute_heads_dropout_mask", TORCH_BOX(&attribute_heads_dropout_mask_op));
    m.impl("axial_attention", TORCH_BOX(&axial_attention_op));
    m.impl("axial_attention_bf16", TORCH_BOX(&axial_attention_bf16_op));
    m.impl("axial_attention_bwd", TORCH_BOX(&axial_attention_bwd_op));
    m.impl("axial_attention_bf16_bwd", TORCH_BOX(&axial_attention_bf16_bwd_op));
    m.impl("ffn_residual", TORCH_BOX(&ffn_residual_op));
    m.impl("ffn_residual_train_fwd", TORCH_BOX(&ffn_residual_train_fwd_op));
    m.impl("ffn_residual_bwd", TORCH_BOX(&ffn_residual_bwd_op));
    m.impl("ffn_dropout_mask", TORCH_BOX(&ffn_dropout_mask_op));
    m.impl("ffn_residual_bf16", TORCH_BOX(&ffn_residual_bf16_op));
    m.impl("ffn_residual_bf16_mixed", TORCH_BOX(&ffn_residual_bf16_mixed_op));
    m.impl("ffn_residual_bf16_train_fwd", TORCH_BOX(&ffn_residual_bf16_train_fwd_op));
    m.impl("ffn_residual_bf16_mixed_train_fwd", TORCH_BOX(&ffn_residual_bf16_mixed_train_fwd_op));
    m.impl("ffn_residual_bf16_bwd", TORCH_BOX(&ffn_residual_bf16_bwd_op));
    m.impl("ffn_residual_bf16_mixed_bwd", TORCH_BOX(&ffn_residual_bf16_mixed_bwd_op));
    m.impl("log_mel", TORCH_BOX(&log_mel_op));
    m.impl("grad_sqnorm", TORCH_BOX(&grad_sqnorm_op));
    m.impl("clip_from_history", TORCH_BOX(&clip_from_history_op));
    m.impl("adabelief_step", TORCH_BOX(&adabelief_step_op));
    m.impl("segment_onset_filter", TORCH_BOX(&segment_onset_filter_op));
    m.impl("segment_events", TORCH_BOX(&segment_events_op));
}
