// api.hip -- extern "C" entry points declared in include/semicrf_hip.h: argument checks,
// workspace carving and dispatch to the kernels.  Nothing here synchronises the host.
#include <stdarg.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <unordered_map>
#include "common.h"
#include "launchers.h"
#include "attention_math.h"
#include "ffn_math.h"
#include "ffn_bf16_train_math.h"
#include "logmel_math.h"

namespace semicrf {

static thread_local char g_err[512] = "";
static std::atomic<int> g_impl{0};

void set_error(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// the kernels' launchers (defined in the other translation units): launchers.h

static bool use_persist(int T, int B) { return g_impl.load() == 0 && persist_supported(T, B); }

struct Carver {
    char* p;
    size_t left;
    bool ok = true;
    Carver(void* ws, size_t n) : p((char*)ws), left(n) {}
    template <typename U>
    U* take(size_t count)
    {
        size_t bytes = align_up(count * sizeof(U));
        if (bytes > left) { ok = false; return nullptr; }
        U* r = (U*)p;
        p += bytes;
        left -= bytes;
        return r;
    }
};

static size_t tb(int T, int B) { return align_up((size_t)T * (size_t)B * 4); }

// ---- leased workspaces (semicrf_workspace_register) ------------------------------------------------------------------
// A sweep needs its scratch to read 0xff everywhere when it starts: u values are their own "not published yet" flag.  For a
// caller-owned buffer that means one fill (17 MB at T=1024, NBatch=352: 6.8 us) in front of every launch.  A workspace
// that the caller REGISTERS -- promising that nothing but sweeps of this library writes to it, that at most one stream
// uses it at a time -- is filled once; every launch then leaves it the way the fill would (persist.hip: the rings put
// their u values back, the last wave resets the control words, far partials carry the workspace's own launch count).
// A launch that timed out raises a pinned host word; the host then distrusts every lease and fills again.
struct Lease { size_t bytes; int op, T, B; bool clean; unsigned count; };
static std::mutex g_lease_mu;
static std::unordered_map<void*, Lease> g_leases;
static unsigned* g_abort_word = nullptr;                 // pinned + mapped: the device address equals the host address
static std::atomic<bool> g_abort_on_device[64];          // the kernels of device d know the word's address

// The pinned abort word exists for EVERY caller of the sweeps (round 4; until then only for leased workspaces): a bounded wait
// that timed out on the device raises it with a system-scope store, and the NEXT sweep entry point of this library reports it as
// SEMICRF_ETIMEOUT instead of launching -- a time-out is loud on every path (the poisoned outputs of the launch that aborted have
// been handed out by then: nothing synchronises the host; semicrf_async_error lets a caller that does synchronise ask earlier).
static int ensure_abort_word(hipStream_t stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (g_abort_on_device[dev].load()) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) return 0;   // not now: the set-up synchronises
    {
        std::lock_guard<std::mutex> lk(g_lease_mu);
        if (!g_abort_word) {
            void* p = nullptr;
            if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) return 1;
            memset(p, 0, 64);
            g_abort_word = (unsigned*)p;
        }
    }
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, g_abort_word, 0) != hipSuccess || persist_set_host_abort_word((unsigned*)dp)) return 1;
    g_abort_on_device[dev].store(true);
    return 0;
}

// the code a device-side time-out left behind (0: none); clears it and distrusts every lease
static unsigned take_async_error()
{
    if (!g_abort_word) return 0u;
    const unsigned code = __atomic_exchange_n(g_abort_word, 0u, __ATOMIC_RELAXED);
    if (code != 0u) {
        std::lock_guard<std::mutex> lk(g_lease_mu);
        for (auto& kv : g_leases) kv.second.clean = false;          // some launch gave up: its workspace is in an unknown state
    }
    return code;
}

// first thing in every sweep entry point
static int sweep_prologue(const char* what, hipStream_t stream)
{
    if (ensure_abort_word(stream)) { set_error("%s: could not set up the device's abort word", what); return SEMICRF_ELAUNCH; }
    if (const unsigned code = take_async_error()) {
        set_error("%s: an earlier sweep on this GPU gave up on a bounded hand-off wait (device code %u: the GPU is shared with work that "
                  "kept part of the persistent kernel from running, or a CU mask hides compute units); the results of that launch "
                  "and of launches enqueued behind it are invalid (NaN-poisoned).  Nothing was enqueued by this call.", what, code);
        return SEMICRF_ETIMEOUT;
    }
    return SEMICRF_OK;
}

// what the next sweep into `ws` has to do: 0 ordinary, 1 fill + self-clean, 2 clean already; tag = the lease's launch count
static int lease_acquire(void* ws, int op, int T, int B, unsigned* tag, hipStream_t stream)
{
    *tag = 0;
    std::lock_guard<std::mutex> lk(g_lease_mu);
    if (g_leases.empty()) return 0;
    auto it = g_leases.find(ws);
    if (it == g_leases.end()) return 0;
    {
        // A launch that is being CAPTURED into a graph is replayed with the parameters of the capture -- the same granule tag
        // every time, which a lease must never repeat (the rings would run ahead on the previous replay's partials and clear u
        // under the panels).  Captured launches take the ordinary path: the fill is a node of the graph and resets everything
        // on every replay; the lease no longer counts as clean.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone) {
            it->second.clean = false;
            return 0;
        }
    }
    // (an abort word raised since the entry point's prologue is left for the next prologue: it reports AND distrusts the leases)
    Lease& L = it->second;
    const bool clean = L.clean && L.op == op && L.T == T && L.B == B;
    L.op = op; L.T = T; L.B = B; L.clean = true;                    // the launch enqueued next leaves it clean
    *tag = ++L.count;
    if (L.count == 0u) { *tag = ++L.count; return 1; }              // the count wrapped: the kernel's generation check expects count - 1
    return clean ? 2 : 1;
}
// a sweep that could not be enqueued leaves nothing behind, and a launch of the row-sequential kernels (impl 1) carves its
// scratch out of the same buffer: either way the lease no longer counts as clean
static void lease_failed(void* ws)
{
    std::lock_guard<std::mutex> lk(g_lease_mu);
    auto it = g_leases.find(ws);
    if (it != g_leases.end()) it->second.clean = false;
}

// The argument checks of the two bf16 feed-forward entry points: semicrf_ffn_residual's cases in its words, on elements of T.  The
// strides of the dimensions that count come back in st.
template <typename T>
static int ffn_bf16_check(const char* op, const T* x, T* out, int64_t n0, int64_t n1, int64_t xs0, int64_t xs1, int64_t os0, int64_t os1, int D,
                          int hidden, const T* W1, const T* b1, const T* W2, const T* b2, const T* scale, long long* st, const char* sup = nullptr)
{
    SEMICRF_CHECK_ARG(ffn::supported(D, hidden),
                      "%s: D=%d hidden=%d is outside the supported set (D a multiple of 8 in [%d, %d]; hidden a multiple of 8 in "
                      "[%d, %d]): see semicrf_%s_supported", op, D, hidden, ffn::FFN_MIN_D, ffn::FFN_MAX_D, ffn::FFN_MIN_H, ffn::FFN_MAX_H,
                      sup ? sup : op);
    SEMICRF_CHECK_ARG(n0 >= 1 && n1 >= 1, "%s: n0=%lld n1=%lld must be >= 1", op, (long long)n0, (long long)n1);
    SEMICRF_CHECK_ARG(n0 < (1ll << 37) && n1 < (1ll << 37) && n0 * n1 < (1ll << 37), "%s: n0 * n1 = %lld * %lld must stay below 2^37", op,
                      (long long)n0, (long long)n1);
    SEMICRF_CHECK_ARG(x && out && W1 && b1 && W2 && b2 && scale, "%s: x/out/W1/b1/W2/b2/scale must be non-NULL", op);
    SEMICRF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)W1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)b2 | (uintptr_t)scale) &
                       (sizeof(T) - 1)) == 0,
                      "%s: every pointer must be %d-byte aligned", op, (int)sizeof(T));
    st[0] = n0 > 1 ? xs0 : 0; st[1] = n1 > 1 ? xs1 : 0; st[2] = n0 > 1 ? os0 : 0; st[3] = n1 > 1 ? os1 : 0;
    for (int i = 0; i < 4; ++i) SEMICRF_CHECK_ARG(st[i] >= 0 && st[i] < (1ll << 40), "%s: stride %d = %lld must be in [0, 2^40)", op, i, st[i]);
    SEMICRF_CHECK_ARG((n0 == 1 || st[2] >= D) && (n1 == 1 || st[3] >= D), "%s: a row stride of `out` (%lld, %lld) is below D=%d", op, st[2], st[3], D);
    // the element ranges the two views span (strides below 2^40, counts below 2^37: no overflow)
    const long long xext = (n0 - 1) * st[0] + (n1 - 1) * st[1] + D, oext = (n0 - 1) * st[2] + (n1 - 1) * st[3] + D;
    const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
    SEMICRF_CHECK_ARG(xb + (uintptr_t)xext * sizeof(T) <= ob || ob + (uintptr_t)oext * sizeof(T) <= xb, "%s: `out` overlaps `x`", op);
    return SEMICRF_OK;
}

// ---- the training route of the bf16 feed-forward op: one body per call, both forms (T = uint16_t | float) -------------------------------
static bool ffn16_bytes_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return !(pa + na <= pb || pb + nb <= pa);
}

template <typename T, typename L>
static int ffn_bf16_train_fwd_any(const char* op, L launch, const T* x, T* out, void* saved, size_t saved_bytes, int64_t n0, int64_t n1, int64_t xs0,
                                  int64_t xs1, int64_t os0, int64_t os1, int D, int hidden, const T* W1, const T* b1, const T* W2, const T* b2,
                                  const T* scale, float eps, uint64_t seed, double p1, double p2, semicrf_stream_t stream)
{
    long long st[4];
    const int rc = ffn_bf16_check<T>(op, x, out, n0, n1, xs0, xs1, os0, os1, D, hidden, W1, b1, W2, b2, scale, st, "ffn_residual_bf16_bwd");
    if (rc != SEMICRF_OK) return rc;
    SEMICRF_CHECK_ARG(p1 >= 0.0 && p1 < 1.0 && p2 >= 0.0 && p2 < 1.0, "%s: dropout probabilities p_hidden=%g p_out=%g must lie in [0, 1)", op, p1, p2);
    const long long ntok = n0 * n1;
    const size_t need = ffn::train_saved_bytes(ntok, D, hidden);
    SEMICRF_CHECK_ARG(saved && ((uintptr_t)saved & 15) == 0, "%s: saved must be non-NULL and 16-byte aligned", op);
    SEMICRF_CHECK_ARG(saved_bytes >= need, "%s: saved buffer too small: %zu bytes given, semicrf_ffn_residual_bf16_train_saved_bytes says %zu", op,
                      saved_bytes, need);
    const long long xext = (n0 - 1) * st[0] + (n1 - 1) * st[1] + D, oext = (n0 - 1) * st[2] + (n1 - 1) * st[3] + D;
    SEMICRF_CHECK_ARG(!ffn16_bytes_overlap(saved, need, x, (size_t)xext * sizeof(T)) && !ffn16_bytes_overlap(saved, need, out, (size_t)oext * sizeof(T)),
                      "%s: saved overlaps x or out", op);
    launch(x, out, n0, n1, st[0], st[1], st[2], st[3], D, hidden, W1, b1, W2, b2, scale, eps, seed, p1, p2, saved, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH(op);
    return SEMICRF_OK;
}

template <typename T, typename L>
static int ffn_bf16_bwd_any(const char* op, L launch, const T* dout, const T* x, const void* saved, size_t saved_bytes, int64_t n0, int64_t n1,
                            int64_t gs0, int64_t gs1, int64_t xs0, int64_t xs1, int64_t ds0, int64_t ds1, int D, int hidden, const T* W1, const T* W2,
                            const T* scale, float eps, uint64_t seed, double p1, double p2, T* dx, T* dW1, T* db1, T* dW2, T* db2, T* dscale, void* ws,
                            size_t ws_bytes, semicrf_stream_t stream)
{
    // the cases of the eval op, in its words: once with dout, once with x in the place of `x`, dx in the place of `out`
    long long sg[4], sx[4];
    int rc = ffn_bf16_check<T>(op, dout, dx, n0, n1, gs0, gs1, ds0, ds1, D, hidden, W1, W1, W2, W2, scale, sg, "ffn_residual_bf16_bwd");
    if (rc != SEMICRF_OK) return rc;
    rc = ffn_bf16_check<T>(op, x, dx, n0, n1, xs0, xs1, ds0, ds1, D, hidden, W1, W1, W2, W2, scale, sx, "ffn_residual_bf16_bwd");
    if (rc != SEMICRF_OK) return rc;
    SEMICRF_CHECK_ARG(p1 >= 0.0 && p1 < 1.0 && p2 >= 0.0 && p2 < 1.0, "%s: dropout probabilities p_hidden=%g p_out=%g must lie in [0, 1)", op, p1, p2);
    const long long ntok = n0 * n1;
    SEMICRF_CHECK_ARG(ntok <= 65535ll * SEMICRF_FFN_BWD_ROW_CHUNK, "%s: n0 * n1 = %lld: more than 65535 row chunks", op, ntok);
    SEMICRF_CHECK_ARG(dW1 && db1 && dW2 && db2 && dscale, "%s: dW1/db1/dW2/db2/dscale must be non-NULL", op);
    SEMICRF_CHECK_ARG((((uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)dW2 | (uintptr_t)db2 | (uintptr_t)dscale) & (sizeof(T) - 1)) == 0,
                      "%s: every pointer must be %d-byte aligned", op, (int)sizeof(T));
    const size_t need_saved = ffn::train_saved_bytes(ntok, D, hidden);
    SEMICRF_CHECK_ARG(saved && ((uintptr_t)saved & 15) == 0, "%s: saved must be non-NULL and 16-byte aligned", op);
    SEMICRF_CHECK_ARG(saved_bytes >= need_saved, "%s: saved buffer too small: %zu bytes given, semicrf_ffn_residual_bf16_train_saved_bytes says %zu",
                      op, saved_bytes, need_saved);
    const size_t dext = (size_t)((n0 - 1) * sg[2] + (n1 - 1) * sg[3] + D) * sizeof(T);
    SEMICRF_CHECK_ARG(!ffn16_bytes_overlap(dx, dext, saved, need_saved), "%s: `dx` overlaps saved", op);
    const size_t need = ffn_bf16_bwd_workspace_bytes(ntok, D, hidden);
    SEMICRF_CHECK_ARG(ws && ((uintptr_t)ws & 15) == 0, "%s: ws must be non-NULL and 16-byte aligned", op);
    if (ws_bytes < need) {
        set_error("workspace too small for %s: %zu bytes given, semicrf_ffn_residual_bf16_bwd_workspace_bytes says %zu", op, ws_bytes, need);
        return SEMICRF_EWORKSPACE;
    }
    launch(dout, x, saved, n0, n1, sg[0], sg[1], sx[0], sx[1], sg[2], sg[3], D, hidden, W1, W2, scale, eps, seed, p1, p2, dx, dW1, db1, dW2, db2,
           dscale, ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH(op);
    return SEMICRF_OK;
}

}  // namespace semicrf

using namespace semicrf;

extern "C" {

int semicrf_abi_version(void) { return SEMICRF_ABI_VERSION; }
const char* semicrf_last_error(void) { return g_err; }
void semicrf_set_impl(int impl) { g_impl.store(impl); }
int semicrf_get_impl(void) { return g_impl.load(); }
int semicrf_debug_device_status(void) { return read_and_clear_device_status(); }
int semicrf_async_error(void) { return (int)take_async_error(); }
int semicrf_debug_wg_ticket(int n_spine, int grid, int block) { return persist_wg_ticket(n_spine, grid, block); }
void semicrf_debug_score_variant(int variant) { set_score_variant(variant); }
int semicrf_debug_score_route(int C, int T, int D, int64_t ldq, int64_t ldk, int aligned, int prec, int group, int pitch, int rowc,
                              int forced, int impl)
{
    if (C < 1 || T < 1 || D < 1 || group < 1 || pitch < group || C % group != 0) return SCORE_REFUSED;
    if (pitch == group) group = pitch = C;                     // as the entry points normalise it
    return plan_score_route(C, T, D, ldq, ldk, aligned != 0, prec, group, pitch, rowc != 0, forced, impl).kernel;
}

int semicrf_workspace_register(void* ws, size_t ws_bytes)
{
    SEMICRF_CHECK_ARG(ws != nullptr && ws_bytes > 0, "workspace is NULL or empty");
    if (ensure_abort_word(nullptr)) { set_error("could not hand the abort word to the device"); return SEMICRF_ELAUNCH; }
    std::lock_guard<std::mutex> lk(g_lease_mu);
    g_leases[ws] = Lease{ws_bytes, -1, 0, 0, false, 0u};
    return SEMICRF_OK;
}

int semicrf_workspace_unregister(void* ws)
{
    std::lock_guard<std::mutex> lk(g_lease_mu);
    g_leases.erase(ws);
    return SEMICRF_OK;
}

size_t semicrf_workspace_bytes(int op, int T, int B)
{
    if (T <= 0 || B <= 0) return 0;
    switch (op) {
        case SEMICRF_OP_LOGZ_FWD: return tb(T, B) + persist_workspace_bytes(T, B) + 4096;
        case SEMICRF_OP_LOGZ_BWD: return tb(T, B) + persist_workspace_bytes(T, B) + 4096;
        case SEMICRF_OP_VITERBI:
            // u [T][B] f32, code [B][T] i32, region [B][2T][2] i32, counts [B] i32, persistent-sweep scratch
            return tb(T, B) * 2 + align_up((size_t)B * 2 * T * 2 * 4) + align_up((size_t)B * 4) +
                   persist_workspace_bytes(T, B) + 4096;
        case SEMICRF_OP_EVAL_PATH: return 4096;
        case SEMICRF_OP_INTERVAL_SCORE: return 4096;
        case SEMICRF_OP_SAMPLE: return sample_workspace_bytes(T, B);
        case SEMICRF_OP_POSTERIORS: return posterior_workspace_bytes(T, B);
        case SEMICRF_OP_VITERBI_NBEST: return nbest_workspace_bytes(T, B);
        case SEMICRF_OP_MARGINAL_DECODE: return marginal_decode_workspace_bytes(T, B);
        case SEMICRF_OP_EXPECTATION: return expectation_workspace_bytes(T, B);
        case SEMICRF_OP_MBR_SELECT: return mbr_select_workspace_bytes(T, B);
        case SEMICRF_OP_MARGINAL_DECODE_TOL: return marginal_decode_tol_workspace_bytes(T, B);
        // T = rows, B = Hv + Ho: the two heads have at most (B + 63) / 64 + 1 slices between them, 128 outputs a plane at the most
        case SEMICRF_OP_ATTRIBUTE_HEADS: return attr_heads_workspace_bytes(T, 64 * ((B + 63) / 64 + 1), 1, 128, 1);
        // T = rows, B = Hv + Ho: a bound for 3 D <= B and at most 128 outputs a head (every term grows with D, the hidden sizes, the outputs)
        case SEMICRF_OP_ATTRIBUTE_HEADS_BWD: return attr_heads_bwd_workspace_bytes(T, (B + 2) / 3, B, 1, 128, 128);
        // T = tokens, B = hidden: a bound for every supported D (every term grows with D)
        case SEMICRF_OP_FFN_RESIDUAL_BWD: return ffn_bwd_workspace_bytes(T, ffn::FFN_MAX_D, B);
        default: return 0;
    }
}

static int check_common(const float* score, const float* noise, int T, int B)
{
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG((long long)T * T * B < (1ll << 40), "T*T*B too large");
    SEMICRF_CHECK_ARG(T < (1 << 29), "T too large");
    SEMICRF_CHECK_ARG(score != nullptr, "score is NULL");
    SEMICRF_CHECK_ARG(noise != nullptr || T == 1, "noise is NULL");
    return SEMICRF_OK;
}

// ws of the semi-CRF entry points: Carver hands out sub-buffers at aligned OFFSETS from the base, and 64-bit device-scope atomics
// sit on them -- a base below the alignment the header promises (SEMICRF_WS_ALIGN) is refused with the other argument checks, ahead
// of any HIP call.  A NULL ws is not looked at here: the entry points that need one say so themselves.
static int check_ws(const void* ws, const char* what)
{
    SEMICRF_CHECK_ARG(((uintptr_t)ws & (uintptr_t)(SEMICRF_WS_ALIGN - 1)) == 0, "%s: ws must be %d-byte aligned (it is %p)", what,
                      SEMICRF_WS_ALIGN, ws);
    return SEMICRF_OK;
}

// the intervals of semicrf_logprob_fwd, when the sweep's launch can compute the path scores on the side (*folded = 1)
struct PathFold { const int32_t* pairs; int64_t K; const int32_t* offsets; float* logProb; int folded; int32_t* ptab; };

static int logz_fwd_impl(const float* score, const float* noise, int T, int B, float* logZ, float* v, void* ws,
                         size_t ws_bytes, semicrf_stream_t stream, PathFold* pf)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(logZ != nullptr, "logZ is NULL");
    if (int rc = check_ws(ws, "semicrf_logz_fwd")) return rc;
    if (int rc = sweep_prologue("semicrf_logz_fwd", (hipStream_t)stream)) return rc;
    Carver cv(ws, ws_bytes);
    // the sweep's own workspace comes FIRST: a leased ws is only clean where the previous launch left it clean, so its place
    // must not depend on which optional outputs the caller passes (v == NULL used to move it behind the scratch alpha: a
    // logProb without gradient followed by one with, same lease -> NaN)
    const bool fast = use_persist(T, B);
    void* pws = fast ? cv.take<char>(persist_workspace_bytes(T, B)) : nullptr;
    float* vv = v ? v : cv.take<float>((size_t)T * B);
    if (!cv.ok || !ws) { set_error("workspace too small for logz_fwd"); return SEMICRF_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    if (fast) {
        unsigned ltag = 0;
        const int lease = lease_acquire(ws, SEMICRF_OP_LOGZ_FWD, T, B, &ltag, st);
        const int rc = pf ? launch_persist_logprob_fwd(score, noise, T, B, vv, logZ, pf->pairs, (int)pf->K, pf->offsets, pf->logProb, pws, st, lease, ltag, pf->ptab)
                          : launch_persist_sweep(0, 0, score, noise, T, B, vv, logZ, nullptr, pws, st, lease, ltag);
        if (rc) {
            lease_failed(ws);
            set_error("persistent sweep could not be enqueued (too many chain chunks for this device)"); return SEMICRF_ELAUNCH;
        }
        if (pf) pf->folded = 1;
    } else {
        lease_failed(ws);
        launch_rowseq_sweep(0, 0, score, noise, T, B, vv, nullptr, logZ, st);
    }
    SEMICRF_CHECK_LAUNCH("semicrf_logz_fwd");
    return SEMICRF_OK;
}

int semicrf_logz_fwd(const float* score, const float* noise, int T, int B, float* logZ, float* v, void* ws,
                     size_t ws_bytes, semicrf_stream_t stream)
{
    return logz_fwd_impl(score, noise, T, B, logZ, v, ws, ws_bytes, stream, nullptr);
}

static int logz_bwd_impl(const float* score, const float* noise, const float* v, const float* logZ,
                         const float* gout, int gstride, float gscale, int T, int B, float* dScore, float* dNoise, float* q_out,
                         int flags, void* ws, size_t ws_bytes, semicrf_stream_t stream, float noise_add = 0.0f, int* noise_folded = nullptr,
                         const int32_t* ptab = nullptr, int* path_folded = nullptr)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG((flags & ~SEMICRF_GRAD_UPPER_IS_ZERO) == 0, "unknown flags %d", flags);
    if (int rc = check_ws(ws, "semicrf_logz_bwd")) return rc;
    if (int rc = sweep_prologue("semicrf_logz_bwd", (hipStream_t)stream)) return rc;
    const int keep_upper = (flags & SEMICRF_GRAD_UPPER_IS_ZERO) ? 1 : 0;
    SEMICRF_CHECK_ARG(v && logZ && gout && dScore, "v/logZ/gout/dScore must be non-NULL");
    SEMICRF_CHECK_ARG(dNoise != nullptr || T == 1, "dNoise is NULL");
    SEMICRF_CHECK_ARG(gstride == 0 || gstride == 1, "gout stride must be 0 (one value for all chains) or 1");
    Carver cv(ws, ws_bytes);
    const bool fast = use_persist(T, B);
    void* pws = fast ? cv.take<char>(persist_workspace_bytes(T, B)) : nullptr;      // first: see semicrf_logz_fwd
    float* q = q_out ? q_out : cv.take<float>((size_t)T * B);
    if (!cv.ok || !ws) { set_error("workspace too small for logz_bwd"); return SEMICRF_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    if (fast) {
        // beta sweep fused with the marginals: score is read once, dScore written once
        unsigned ltag = 0;
        const int lease = lease_acquire(ws, SEMICRF_OP_LOGZ_BWD, T, B, &ltag, st);
        if (launch_persist_logz_bwd(score, noise, v, logZ, gout, T, B, dScore, dNoise, q, pws, st, lease, ltag, gstride, gscale, keep_upper, noise_add, ptab, path_folded)) {
            lease_failed(ws);
            set_error("persistent sweep could not be enqueued (too many chain chunks for this device)"); return SEMICRF_ELAUNCH;
        }
        if (noise_folded) *noise_folded = 1;        // the ring waves added noise_add * gout to every gap
    } else {
        lease_failed(ws);
        launch_rowseq_sweep(0, 1, score, noise, T, B, q, nullptr, nullptr, st);
        launch_marginals(score, noise, v, q, logZ, gout, T, B, dScore, dNoise, st, gstride, gscale);
    }
    return SEMICRF_OK;
}

int semicrf_logz_bwd_f(const float* score, const float* noise, const float* v, const float* logZ,
                       const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out, int flags, void* ws,
                       size_t ws_bytes, semicrf_stream_t stream)
{
    if (int rc = logz_bwd_impl(score, noise, v, logZ, gout, 1, 1.0f, T, B, dScore, dNoise, q_out, flags, ws, ws_bytes, stream)) return rc;
    SEMICRF_CHECK_LAUNCH("semicrf_logz_bwd");
    return SEMICRF_OK;
}

int semicrf_logz_bwd(const float* score, const float* noise, const float* v, const float* logZ,
                     const float* gout, int T, int B, float* dScore, float* dNoise, float* q_out, void* ws,
                     size_t ws_bytes, semicrf_stream_t stream)
{
    return semicrf_logz_bwd_f(score, noise, v, logZ, gout, T, B, dScore, dNoise, q_out, 0, ws, ws_bytes, stream);
}

int semicrf_logprob_fwd(const float* score, const float* noise, int T, int B, const int32_t* pairs, int64_t K,
                        const int32_t* offsets, float* logProb, float* logZ, float* v, void* ws, size_t ws_bytes,
                        semicrf_stream_t stream)
{
    return semicrf_logprob_fwd_t(score, noise, T, B, pairs, K, offsets, logProb, logZ, v, nullptr, ws, ws_bytes, stream);
}

int semicrf_logprob_path_table_supported(int T, int B)
{
    return (T >= 1 && B >= 1 && use_persist(T, B) && persist_path_fold_possible(T, B)) ? 1 : 0;
}

int semicrf_logprob_fwd_t(const float* score, const float* noise, int T, int B, const int32_t* pairs, int64_t K,
                          const int32_t* offsets, float* logProb, float* logZ, float* v, int32_t* ptab, void* ws, size_t ws_bytes,
                          semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(offsets && logProb && logZ, "offsets/logProb/logZ must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || pairs), "bad interval count");
    // the table is written by the sweep's path role: no sweep launch, no table (the caller asks semicrf_logprob_path_table_supported)
    SEMICRF_CHECK_ARG(ptab == nullptr || (T >= 1 && B >= 1 && use_persist(T, B)), "a path table needs the persistent sweep (T=%d, B=%d)", T, B);
    // ONE launch where the persistent sweep runs (round 5): spare waves of the sweep's launch compute the path scores while it runs,
    // the ring wave that finalises logZ subtracts (persist.hip: path_role); the row-sequential fallback keeps the path kernel
    PathFold pf{pairs, K, offsets, logProb, 0, ptab};
    if (int rc = logz_fwd_impl(score, noise, T, B, logZ, v, ws, ws_bytes, stream, &pf)) return rc;
    if (!pf.folded) launch_eval_path(score, noise, T, B, (int)K, pairs, offsets, logProb, (hipStream_t)stream, logZ);
    SEMICRF_CHECK_LAUNCH("semicrf_logprob_fwd");
    return SEMICRF_OK;
}

int semicrf_logprob_bwd(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                        int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets, float* dScore,
                        float* dNoise, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return semicrf_logprob_bwd_f(score, noise, v, logZ, gout, gout_stride, T, B, pairs, K, offsets, dScore, dNoise, 0, ws, ws_bytes, stream);
}

int semicrf_logprob_bwd_f(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                          int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets, float* dScore,
                          float* dNoise, int flags, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return semicrf_logprob_bwd_t(score, noise, v, logZ, gout, gout_stride, T, B, pairs, K, offsets, dScore, dNoise, flags, nullptr, ws, ws_bytes,
                                 stream);
}

int semicrf_logprob_bwd_t(const float* score, const float* noise, const float* v, const float* logZ, const float* gout,
                          int gout_stride, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets, float* dScore,
                          float* dNoise, int flags, const int32_t* ptab, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(offsets, "offsets must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || pairs), "bad interval count");
    // d logProb = d evalPath - d logZ: the marginals with -gout, then +gout on the path's cells and uncovered gaps
    // (round 5: the path score's `+ gout on every gap` is added by the gradient sweep's ring waves as they store the noise marginals;
    // what is left for a second launch is the scatter onto the path's own cells and covered gaps -- and with the forward call's path
    // table, in a launch whose band has writers of its own, not even that: every writer of the sweep adds the path's term to what it
    // stores.  The scatter stays for short sequences, the row-sequential implementation, chain chunks and callers without a table.)
    int noise_folded = 0, path_folded = 0;
    if (int rc = logz_bwd_impl(score, noise, v, logZ, gout, gout_stride, -1.0f, T, B, dScore, dNoise, nullptr, flags, ws, ws_bytes, stream,
                               1.0f, &noise_folded, ptab, &path_folded)) return rc;
    if (!path_folded)
        launch_eval_path_bwd(gout, T, B, (int)K, pairs, offsets, dScore, dNoise, (hipStream_t)stream, gout_stride, 1.0f, noise_folded);
    SEMICRF_CHECK_LAUNCH("semicrf_logprob_bwd");
    return SEMICRF_OK;
}

int semicrf_beta(const float* score, const float* noise, int T, int B, float* beta, void* ws, size_t ws_bytes,
                 semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(beta, "beta must be non-NULL");
    if (int rc = check_ws(ws, "semicrf_beta")) return rc;
    if (int rc = sweep_prologue("semicrf_beta", (hipStream_t)stream)) return rc;
    Carver cv(ws, ws_bytes);
    const bool fast = use_persist(T, B);
    void* pws = fast ? cv.take<char>(persist_workspace_bytes(T, B)) : nullptr;
    if (!cv.ok || (fast && !ws)) { set_error("workspace too small for beta"); return SEMICRF_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    if (fast) {
        unsigned ltag = 0;
        const int lease = lease_acquire(ws, SEMICRF_OP_LOGZ_FWD + 100, T, B, &ltag, st);
        if (launch_persist_sweep(0, 1, score, noise, T, B, beta, nullptr, nullptr, pws, st, lease, ltag)) {
            lease_failed(ws);
            set_error("persistent sweep could not be enqueued (too many chain chunks for this device)"); return SEMICRF_ELAUNCH;
        }
    } else {
        lease_failed(ws);
        launch_rowseq_sweep(0, 1, score, noise, T, B, beta, nullptr, nullptr, st);
    }
    SEMICRF_CHECK_LAUNCH("semicrf_beta");
    return SEMICRF_OK;
}

int semicrf_viterbi(const float* score, const float* noise, int T, int B, const int32_t* start, int forward,
                    int32_t* pairs, int64_t cap, int32_t* offsets, void* ws, size_t ws_bytes,
                    semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(pairs && offsets && cap >= 0, "pairs/offsets must be non-NULL");
    SEMICRF_CHECK_ARG((long long)B * 2 * T < (1ll << 31), "B*2T exceeds int32 offsets");
    if (int rc = check_ws(ws, "semicrf_viterbi")) return rc;
    if (int rc = sweep_prologue("semicrf_viterbi", (hipStream_t)stream)) return rc;
    Carver cv(ws, ws_bytes);
    float* u = cv.take<float>((size_t)T * B);
    int* code = cv.take<int>((size_t)T * B);
    int* region = cv.take<int>((size_t)B * 2 * T * 2);
    int* counts = cv.take<int>((size_t)B);
    const bool fast = use_persist(T, B);
    void* pws = fast ? cv.take<char>(persist_workspace_bytes(T, B)) : nullptr;
    if (!cv.ok || !ws) { set_error("workspace too small for viterbi"); return SEMICRF_EWORKSPACE; }
    hipStream_t st = (hipStream_t)stream;
    if (fast) {
        unsigned ltag = 0;
        const int lease = lease_acquire(ws, SEMICRF_OP_VITERBI, T, B, &ltag, st);
        if (launch_persist_sweep(1, forward ? 0 : 1, score, noise, T, B, nullptr, nullptr, code, pws, st, lease, ltag)) {
            lease_failed(ws);
            set_error("persistent sweep could not be enqueued (too many chain chunks for this device)"); return SEMICRF_ELAUNCH;
        }
    } else {
        lease_failed(ws);
        launch_rowseq_sweep(1, forward ? 0 : 1, score, noise, T, B, u, code, nullptr, st);
    }
    int nerr = 0, estride = 0;
    const unsigned* err = fast ? persist_error_words(pws, &nerr, &estride) : nullptr;
    launch_backtrack(code, T, B, start, forward ? 1 : 0, region, counts, pairs, (long long)cap, offsets, st, err, nerr, estride);
    SEMICRF_CHECK_LAUNCH("semicrf_viterbi");
    return SEMICRF_OK;
}

int semicrf_sample(const float* score, const float* noise, const float* v, int T, int B, int64_t k0, int nSample, uint64_t key,
                   const int32_t* end, int32_t* pairs, int64_t cap, int32_t* offsets, void* ws, size_t ws_bytes,
                   semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(v != nullptr, "v (alpha) is NULL");
    SEMICRF_CHECK_ARG(nSample >= 1 && k0 >= 0, "nSample=%d must be >= 1 and k0=%lld >= 0", nSample, (long long)k0);
    SEMICRF_CHECK_ARG(pairs && offsets && cap >= 0, "pairs/offsets must be non-NULL");
    SEMICRF_CHECK_ARG((long long)nSample * B * 2 * T < (1ll << 31), "nSample*B*2T exceeds int32 offsets");
    SEMICRF_CHECK_ARG((long long)T * ((B + 63) / 64) < (1ll << 31), "T*ceil(B/64) exceeds the grid");
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < sample_workspace_bytes(T, nSample * B)) { set_error("workspace too small for sample"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_sample")) return rc;
    launch_sample(score, noise, v, T, B, (long long)k0, nSample, (unsigned long long)key, end, pairs, (long long)cap, offsets, ws,
                  (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_sample");
    return SEMICRF_OK;
}

int semicrf_viterbi_nbest(const float* score, const float* noise, int T, int B, int k, const int32_t* start, int forward,
                          int32_t* pairs, int64_t cap, int32_t* offsets, float* scores, int32_t* npaths, void* ws, size_t ws_bytes,
                          semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(k >= 1 && k <= 16, "k=%d must be in [1, 16]", k);
    SEMICRF_CHECK_ARG(pairs && offsets && cap >= 0, "pairs/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(scores && npaths, "scores/npaths must be non-NULL");
    SEMICRF_CHECK_ARG((long long)k * B * 2 * T < (1ll << 31), "k*B*2T exceeds int32 offsets");
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < nbest_workspace_bytes(T, k * B)) { set_error("workspace too small for viterbi_nbest"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_viterbi_nbest")) return rc;
    launch_viterbi_nbest(score, noise, T, B, k, start, forward ? 1 : 0, pairs, (long long)cap, offsets, scores, npaths, ws,
                         (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_viterbi_nbest");
    return SEMICRF_OK;
}

int semicrf_posteriors(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                       float* node, float* begin, float* end, float* single, float* noiseP, float* entropy, void* ws, size_t ws_bytes,
                       semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(v && q && logZ, "v (alpha), q (beta) and logZ must be non-NULL");
    SEMICRF_CHECK_ARG(node && begin && end && single && entropy && (noiseP || T == 1), "an output is NULL");
    SEMICRF_CHECK_ARG((long long)((T + 63) / 64) * ((T + 63) / 64 + 1) / 2 < 65536, "T=%d too large for the posterior pass", T);
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < posterior_workspace_bytes(T, B)) { set_error("workspace too small for posteriors"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_posteriors")) return rc;
    launch_posteriors(score, noise, v, q, logZ, T, B, node, begin, end, single, noiseP, entropy, ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_posteriors");
    return SEMICRF_OK;
}

int semicrf_expectation(const float* score, const float* noise, const float* weight, const float* noiseWeight, const float* v,
                        const float* q, int T, int B, float* E, float* H, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(v && q, "v (alpha) and q (beta) must be non-NULL");
    SEMICRF_CHECK_ARG(E && H, "an output is NULL");
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < expectation_workspace_bytes(T, B)) { set_error("workspace too small for expectation"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_expectation")) return rc;
    launch_expectation(score, noise, weight ? weight : score, noiseWeight, v, q, T, B, E, H, ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_expectation");
    return SEMICRF_OK;
}

int semicrf_alpha_from(const float* score, const float* noise, const int32_t* start, int T, int B, float* v, float* logZ, void* ws,
                       size_t ws_bytes, semicrf_stream_t stream)
{
    (void)ws; (void)ws_bytes;                      // no workspace: NULL is fine
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(start != nullptr, "start is NULL");
    SEMICRF_CHECK_ARG(v && logZ, "an output is NULL");
    if (int rc = check_ws(ws, "semicrf_alpha_from")) return rc;
    launch_alpha_from(score, noise, start, T, B, v, logZ, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_alpha_from");
    return SEMICRF_OK;
}

int semicrf_covariance(const float* score, const float* noise, const float* weight, const float* noiseWeight, const float* gout, int T,
                       int B, float* C, float* Cn, const void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(gout != nullptr, "gout is NULL");
    SEMICRF_CHECK_ARG(C && (Cn || T == 1), "an output is NULL");
    SEMICRF_CHECK_ARG(T < 65536, "T=%d too large for the covariance pass", T);
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < expectation_workspace_bytes(T, B)) { set_error("workspace too small for covariance"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_covariance")) return rc;
    launch_covariance(score, noise, weight ? weight : score, noiseWeight, gout, T, B, C, Cn, ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_covariance");
    return SEMICRF_OK;
}

int semicrf_interval_marginals(const float* score, const float* v, const float* q, const float* logZ, int T, int B,
                               const int32_t* pairs, int64_t K, const int32_t* offsets, float* out, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG((long long)T * T * B < (1ll << 40), "T*T*B too large");
    SEMICRF_CHECK_ARG(score && v && q && logZ && offsets, "score / v / q / logZ / offsets must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || (pairs && out)), "bad interval count");
    launch_interval_marginals(score, v, q, logZ, T, B, pairs, (int)K, offsets, out, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_interval_marginals");
    return SEMICRF_OK;
}

int semicrf_marginal_decode(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                            const float* tau, int tau_stride, int32_t* pairs, float* probs, int64_t cap, int32_t* offsets, void* ws,
                            size_t ws_bytes, semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(v && q && logZ && tau, "v (alpha), q (beta), logZ and tau must be non-NULL");
    SEMICRF_CHECK_ARG(tau_stride == 0 || tau_stride == 1, "tau stride must be 0 (one value for all chains) or 1");
    SEMICRF_CHECK_ARG(pairs && probs && offsets && cap >= 0, "pairs/probs/offsets must be non-NULL and cap >= 0");
    SEMICRF_CHECK_ARG((long long)T * (T + 1) / 2 * B < (1ll << 31), "T (T+1) / 2 * B exceeds int32 offsets");
    SEMICRF_CHECK_ARG((long long)((T + 63) / 64) * ((T + 63) / 64 + 1) / 2 < 65536, "T=%d too large for the marginal decode", T);
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < marginal_decode_workspace_bytes(T, B)) { set_error("workspace too small for marginal_decode"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_marginal_decode")) return rc;
    launch_marginal_decode(score, v, q, logZ, T, B, tau, tau_stride, pairs, probs, (long long)cap, offsets, ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_marginal_decode");
    return SEMICRF_OK;
}

int semicrf_interval_marginals_tol(const float* score, const float* v, const float* q, const float* logZ, int T, int B,
                                   const int32_t* pairs, int64_t K, const int32_t* offsets, int tol_begin, int tol_end, float* out,
                                   semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(tol_begin >= 0 && tol_begin <= SEMICRF_TOL_MAX && tol_end >= 0 && tol_end <= SEMICRF_TOL_MAX,
                      "tolerance (%d, %d) outside [0, %d]", tol_begin, tol_end, SEMICRF_TOL_MAX);
    if (tol_begin == 0 && tol_end == 0) return semicrf_interval_marginals(score, v, q, logZ, T, B, pairs, K, offsets, out, stream);
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG((long long)T * T * B < (1ll << 40), "T*T*B too large");
    SEMICRF_CHECK_ARG(score && v && q && logZ && offsets, "score / v / q / logZ / offsets must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || (pairs && out)), "bad interval count");
    launch_interval_marginals_tol(score, v, q, logZ, T, B, pairs, (int)K, offsets, tol_begin, tol_end, out, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_interval_marginals_tol");
    return SEMICRF_OK;
}

int semicrf_marginal_decode_tol(const float* score, const float* noise, const float* v, const float* q, const float* logZ, int T, int B,
                                const float* tau, int tau_stride, int tol_begin, int tol_end, int32_t* pairs, float* probs, int64_t cap,
                                int32_t* offsets, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(tol_begin >= 0 && tol_begin <= SEMICRF_TOL_MAX && tol_end >= 0 && tol_end <= SEMICRF_TOL_MAX,
                      "tolerance (%d, %d) outside [0, %d]", tol_begin, tol_end, SEMICRF_TOL_MAX);
    if (tol_begin == 0 && tol_end == 0)
        return semicrf_marginal_decode(score, noise, v, q, logZ, T, B, tau, tau_stride, pairs, probs, cap, offsets, ws, ws_bytes, stream);
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(v && q && logZ && tau, "v (alpha), q (beta), logZ and tau must be non-NULL");
    SEMICRF_CHECK_ARG(tau_stride == 0 || tau_stride == 1, "tau stride must be 0 (one value for all chains) or 1");
    SEMICRF_CHECK_ARG(pairs && probs && offsets && cap >= 0, "pairs/probs/offsets must be non-NULL and cap >= 0");
    SEMICRF_CHECK_ARG((long long)T * (T + 1) / 2 * B < (1ll << 31), "T (T+1) / 2 * B exceeds int32 offsets");
    SEMICRF_CHECK_ARG((long long)((T + 63) / 64) * ((T + 63) / 64 + 1) / 2 < 65536, "T=%d too large for the marginal decode", T);
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < marginal_decode_tol_workspace_bytes(T, B)) { set_error("workspace too small for marginal_decode_tol"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_marginal_decode_tol")) return rc;
    launch_marginal_decode_tol(score, v, q, logZ, T, B, tau, tau_stride, tol_begin, tol_end, pairs, probs, (long long)cap, offsets, ws,
                               (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_marginal_decode_tol");
    return SEMICRF_OK;
}

int semicrf_mbr_select(const int32_t* pairs, const float* weight, const int32_t* offsets, int64_t K, int T, int B, const float* tau,
                       int tau_stride, int32_t* pairs_out, float* probs_out, int64_t cap, int32_t* offsets_out, float* gain, void* ws,
                       size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG(T < (1 << 29) && (long long)2 * T * B < (1ll << 31), "2 T B exceeds int32 offsets");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || (pairs && weight)), "bad lattice capacity");
    SEMICRF_CHECK_ARG(((uintptr_t)pairs & 7) == 0, "pairs must be 8-byte aligned");
    SEMICRF_CHECK_ARG(offsets && tau, "offsets and tau must be non-NULL");
    SEMICRF_CHECK_ARG(tau_stride == 0 || tau_stride == 1, "tau stride must be 0 (one value for all chains) or 1");
    SEMICRF_CHECK_ARG(pairs_out && probs_out && offsets_out && gain && cap >= 0, "pairs_out/probs_out/offsets_out/gain must be non-NULL and cap >= 0");
    SEMICRF_CHECK_ARG(ws != nullptr, "workspace is NULL");
    if (ws_bytes < mbr_select_workspace_bytes(T, B)) { set_error("workspace too small for mbr_select"); return SEMICRF_EWORKSPACE; }
    if (int rc = check_ws(ws, "semicrf_mbr_select")) return rc;
    launch_mbr_select(pairs, weight, offsets, (long long)K, T, B, tau, tau_stride, pairs_out, probs_out, (long long)cap, offsets_out, gain,
                      ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_mbr_select");
    return SEMICRF_OK;
}

int semicrf_compare_paths(const int32_t* est_pairs, const int32_t* est_offsets, const int32_t* ref_pairs, const int32_t* ref_offsets,
                          int T, int B, int tol_begin, int tol_end, int32_t* stats, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG(T < (1 << 29) && (long long)7 * B < (1ll << 31), "T or B too large");
    SEMICRF_CHECK_ARG(tol_begin >= 0 && tol_begin <= SEMICRF_TOL_MAX && tol_end >= 0 && tol_end <= SEMICRF_TOL_MAX,
                      "tolerance (%d, %d) outside 0..%d", tol_begin, tol_end, SEMICRF_TOL_MAX);
    SEMICRF_CHECK_ARG(est_offsets && ref_offsets && stats, "est_offsets/ref_offsets/stats must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)est_pairs | (uintptr_t)ref_pairs) & 7) == 0, "pairs must be 8-byte aligned");
    SEMICRF_CHECK_ARG((((uintptr_t)est_offsets | (uintptr_t)ref_offsets | (uintptr_t)stats) & 3) == 0, "offsets/stats must be 4-byte aligned");
    launch_compare_paths(est_pairs, est_offsets, ref_pairs, ref_offsets, T, B, tol_begin, tol_end, stats, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_compare_paths");
    return SEMICRF_OK;
}

int semicrf_eval_path(const float* score, const float* noise, int T, int B, const int32_t* pairs, int64_t K,
                      const int32_t* offsets, float* out, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    if (int rc = check_common(score, noise, T, B)) return rc;
    SEMICRF_CHECK_ARG(offsets && out, "offsets/out must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || pairs), "bad interval count");
    (void)ws; (void)ws_bytes;
    if (int rc = check_ws(ws, "semicrf_eval_path")) return rc;
    launch_eval_path(score, noise, T, B, (int)K, pairs, offsets, out, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_eval_path");
    return SEMICRF_OK;
}

int semicrf_eval_path_bwd(const float* gout, int T, int B, const int32_t* pairs, int64_t K, const int32_t* offsets,
                          float* dScore, float* dNoise, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(T >= 1 && B >= 1, "T=%d, B=%d must be >= 1", T, B);
    SEMICRF_CHECK_ARG(gout && offsets, "gout/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || pairs), "bad interval count");
    launch_eval_path_bwd(gout, T, B, (int)K, pairs, offsets, dScore, dNoise, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_eval_path_bwd");
    return SEMICRF_OK;
}

// ---- the interval scorer ---------------------------------------------------------------------------------------------------------
// Every entry point comes in three forms: plain, _p (slot layout) and _pc (slot layout + the merged projection's row constant).
// The _pc form is the implementation; the other two forward to it.

// The argument checks the scorer's entry points start with, in the order in which a bad call's first error is reported.
// operands: the non-NULL test of the pointers `names` lists; lds: the test of the leading dimensions.
static int check_score_operands(int C, int T, int D, bool operands, const char* names, bool lds, int length_scaling)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1, "C=%d T=%d D=%d must be >= 1", C, T, D);
    SEMICRF_CHECK_ARG(operands, "%s must be non-NULL", names);
    SEMICRF_CHECK_ARG(lds, "bad leading dimensions");
    SEMICRF_CHECK_ARG(length_scaling >= 0 && length_scaling <= 2, "bad length_scaling %d", length_scaling);
    return SEMICRF_OK;
}

// the slot layout, normalised: without ghosts it is ONE group (quads must not straddle a group's end).  Its own function because
// the entry points report another error (full_square, the backward's D) between the operands' and this one.
static int check_slots(int C, int& group, int& pitch)
{
    SEMICRF_CHECK_ARG(group >= 1 && pitch >= group && C % group == 0, "bad slot layout: C=%d group=%d pitch=%d", C, group, pitch);
    SEMICRF_CHECK_ARG(pitch == group || pitch % 4 == 0, "a padded slot pitch must be a multiple of 4 (pitch=%d)", pitch);
    SEMICRF_CHECK_ARG((long long)(C / group) * pitch < (1ll << 31), "too many slots");
    if (pitch == group) group = pitch = C;
    return SEMICRF_OK;
}

int interval_score_fwd_pc(const float* q, const float* k, const float* diag, const float* rowc, int C, int T, int D, int64_t ldq,
                          int64_t ldk, int64_t ldd, int64_t ldrc, float qscale, int length_scaling, int full_square, int group,
                          int pitch, float* S, float* noise_out, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(!rowc || ldrc >= 1, "bad row-constant stride");
    if (int rc = check_score_operands(C, T, D, q && k && diag && S, "q/k/diag/S", ldq >= D && ldk >= D && ldd >= 1, length_scaling)) return rc;
    SEMICRF_CHECK_ARG(full_square >= 0 && (full_square & 3) <= 2 && (full_square & ~7) == 0, "bad full_square %d", full_square);
    if (int rc = check_slots(C, group, pitch)) return rc;
    const int Cs = (C / group) * pitch;
    const int prec = (full_square & SEMICRF_SCORE_BF16X3) ? 1 : 0;   // opt-in: three-limb bf16 contraction (scorer_fwd_tile3.h)
    full_square &= 3;
    // (S too: the LDS-staged kernels write 16-byte pieces of the chain axis; the register-load and plain kernels store dword by dword)
    const ScoreRoute route = plan_score_route(C, T, D, ldq, ldk, (((uintptr_t)q | (uintptr_t)k | (uintptr_t)S) & 15) == 0, prec, group, pitch,
                                              rowc != nullptr, score_variant(), g_impl.load());
    SEMICRF_CHECK_ARG(route.kernel != SCORE_REFUSED, "%s", route.why);
    hipStream_t st = (hipStream_t)stream;
    if (full_square == 0) launch_zero_upper(S, T, Cs, st);     // begin > end: defined (zero), half the bytes of a full fill
    const int full_kernel = full_square == 1 ? 1 : 0;           // 2: lower triangle only, the rest of S is left as it is
    if (launch_interval_score_fwd(route.kernel, q, k, diag, C, T, D, ldq, ldk, ldd, qscale, length_scaling, full_kernel, S, st, group, pitch,
                                  rowc, ldrc) != 0) {
        set_error("interval_score_fwd: work list allocation failed");
        return SEMICRF_ELAUNCH;
    }
    if (noise_out && T > 1) {
        if (hipMemsetAsync(noise_out, 0, (size_t)(T - 1) * Cs * sizeof(float), st) != hipSuccess) {
            set_error("hipMemsetAsync failed");
            return SEMICRF_ELAUNCH;
        }
    }
    SEMICRF_CHECK_LAUNCH("interval_score_fwd");
    return SEMICRF_OK;
}

int interval_score_fwd_p(const float* q, const float* k, const float* diag, int C, int T, int D, int64_t ldq,
                         int64_t ldk, int64_t ldd, float qscale, int length_scaling, int full_square, int group, int pitch,
                         float* S, float* noise_out, semicrf_stream_t stream)
{
    return interval_score_fwd_pc(q, k, diag, nullptr, C, T, D, ldq, ldk, ldd, 1, qscale, length_scaling, full_square, group, pitch, S,
                                 noise_out, stream);
}

int interval_score_fwd(const float* q, const float* k, const float* diag, int C, int T, int D, int64_t ldq,
                       int64_t ldk, int64_t ldd, float qscale, int length_scaling, int full_square, float* S,
                       float* noise_out, semicrf_stream_t stream)
{
    return interval_score_fwd_p(q, k, diag, C, T, D, ldq, ldk, ldd, qscale, length_scaling, full_square, C > 0 ? C : 1, C > 0 ? C : 1, S,
                                noise_out, stream);
}

// the leading dimensions of a backward call
static bool bwd_lds_ok(int D, int64_t ldq, int64_t ldk, const float* dq, const float* dk, const float* ddiag, int64_t lddq, int64_t lddk,
                       int64_t lddd)
{
    return ldq >= D && ldk >= D && (!dq || lddq >= D) && (!dk || lddk >= D) && (!ddiag || lddd >= 1);
}

int interval_score_bwd(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq, int64_t ldk,
                       float qscale, int length_scaling, float* dq, float* dk, float* ddiag, int64_t lddq,
                       int64_t lddk, int64_t lddd, semicrf_stream_t stream)
{
    if (int rc = check_score_operands(C, T, D, dS && q && k, "dS/q/k", bwd_lds_ok(D, ldq, ldk, dq, dk, ddiag, lddq, lddk, lddd), length_scaling)) return rc;
    SEMICRF_CHECK_ARG(interval_score_bwd_supported(C, T, D), "interval_score_bwd needs D %% 32 == 0 and D <= 256 (D=%d)", D);
    launch_interval_score_bwd(dS, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, ddiag, lddq, lddk, lddd,
                              (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("interval_score_bwd");
    return SEMICRF_OK;
}

size_t interval_score_bwd_workspace_bytes(int C, int T, int D) { return interval_score_bwd_ws_bytes(C, T, D); }

int interval_score_bwd_ws_pc(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq, int64_t ldk,
                             float qscale, int length_scaling, int group, int pitch, float* dq, float* dk, float* ddiag, float* drowc,
                             int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(!drowc || lddrc >= 1, "bad row-constant stride");
    const int prec = (length_scaling & SEMICRF_LEN_BF16X3) ? 1 : 0;   // opt-in: the two products on the three-limb bf16 kernels (scorer_bwd_gemm3.h)
    length_scaling &= ~SEMICRF_LEN_BF16X3;
    if (int rc = check_score_operands(C, T, D, dS && q && k, "dS/q/k", bwd_lds_ok(D, ldq, ldk, dq, dk, ddiag, lddq, lddk, lddd), length_scaling)) return rc;
    SEMICRF_CHECK_ARG(interval_score_bwd_supported(C, T, D), "interval_score_bwd needs D %% 32 == 0 and D <= 256 (D=%d)", D);
    if (int rc = check_slots(C, group, pitch)) return rc;
    const bool slots = pitch != group;
    hipStream_t st = (hipStream_t)stream;
    if (g_impl.load() == 0 && (dq || dk) &&
        launch_interval_score_bwd_packed(dS, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, lddq, lddk, ws, ws_bytes, st, nullptr,
                                         group, pitch, drowc, lddrc, prec)) {
        if (ddiag) launch_interval_score_bwd_diag(dS, nullptr, ddiag, C, T, lddd, group, pitch, st);      // (drowc: out of the dq GEMM)
    } else {
        SEMICRF_CHECK_ARG(!slots, "a padded slot layout needs the packed path (workspace, D in {64,128,256}, T >= 64, aligned rows)");
        launch_interval_score_bwd(dS, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, ddiag, lddq, lddk, lddd, st);
        if (drowc) launch_interval_score_bwd_rowsum(dS, nullptr, drowc, lddrc, C, T, qscale, length_scaling, group, pitch, st);
    }
    SEMICRF_CHECK_LAUNCH("interval_score_bwd_ws");
    return SEMICRF_OK;
}

int interval_score_bwd_ws_p(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq, int64_t ldk,
                            float qscale, int length_scaling, int group, int pitch, float* dq, float* dk, float* ddiag, int64_t lddq,
                            int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return interval_score_bwd_ws_pc(dS, q, k, C, T, D, ldq, ldk, qscale, length_scaling, group, pitch, dq, dk, ddiag, nullptr, lddq, lddk, lddd,
                                    1, ws, ws_bytes, stream);
}

int interval_score_bwd_ws(const float* dS, const float* q, const float* k, int C, int T, int D, int64_t ldq, int64_t ldk,
                          float qscale, int length_scaling, float* dq, float* dk, float* ddiag, int64_t lddq,
                          int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return interval_score_bwd_ws_p(dS, q, k, C, T, D, ldq, ldk, qscale, length_scaling, C > 0 ? C : 1, C > 0 ? C : 1, dq, dk, ddiag, lddq, lddk,
                                   lddd, ws, ws_bytes, stream);
}

int interval_score_bwd_fused(const float* S, const float* alpha, const float* beta, const float* logZ,
                             const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                             int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                             int64_t lddq, int64_t lddk, int64_t lddd, semicrf_stream_t stream)
{
    if (int rc = check_score_operands(C, T, D, S && alpha && beta && logZ && gout && q && k, "S/alpha/beta/logZ/gout/q/k", bwd_lds_ok(D, ldq, ldk, dq, dk, ddiag, lddq, lddk, lddd),
                                      length_scaling))
        return rc;
    SEMICRF_CHECK_ARG(interval_score_bwd_supported(C, T, D), "interval_score_bwd_fused needs D %% 32 == 0 and D <= 256 (D=%d)", D);
    launch_interval_score_bwd_fused(S, alpha, beta, logZ, gout, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk,
                                    ddiag, lddq, lddk, lddd, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("interval_score_bwd_fused");
    return SEMICRF_OK;
}

int interval_score_bwd_fused_ws_pc(const float* S, const float* alpha, const float* beta, const float* logZ,
                                   const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                   int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk, float* ddiag,
                                   float* drowc, int64_t lddq, int64_t lddk, int64_t lddd, int64_t lddrc, void* ws, size_t ws_bytes,
                                   semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(!drowc || lddrc >= 1, "bad row-constant stride");
    const int prec = (length_scaling & SEMICRF_LEN_BF16X3) ? 1 : 0;   // opt-in: the two products on the three-limb bf16 kernels (scorer_bwd_gemm3.h)
    length_scaling &= ~SEMICRF_LEN_BF16X3;
    if (int rc = check_score_operands(C, T, D, S && alpha && beta && logZ && gout && q && k, "S/alpha/beta/logZ/gout/q/k", bwd_lds_ok(D, ldq, ldk, dq, dk, ddiag, lddq, lddk, lddd),
                                      length_scaling))
        return rc;
    SEMICRF_CHECK_ARG(interval_score_bwd_supported(C, T, D), "interval_score_bwd_fused needs D %% 32 == 0 and D <= 256 (D=%d)", D);
    if (int rc = check_slots(C, group, pitch)) return rc;
    const bool slots = pitch != group;
    hipStream_t st = (hipStream_t)stream;
    const float* fused[4] = {alpha, beta, logZ, gout};
    if (g_impl.load() == 0 && (dq || dk) &&
        launch_interval_score_bwd_packed(S, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, lddq, lddk, ws, ws_bytes, st, fused,
                                         group, pitch, drowc, lddrc, prec)) {
        if (ddiag) launch_interval_score_bwd_diag(S, fused, ddiag, C, T, lddd, group, pitch, st);
    } else {
        SEMICRF_CHECK_ARG(!slots, "a padded slot layout needs the packed path (workspace, D in {64,128,256}, T >= 64, aligned rows)");
        launch_interval_score_bwd_fused(S, alpha, beta, logZ, gout, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, ddiag, lddq,
                                        lddk, lddd, st);
        if (drowc) launch_interval_score_bwd_rowsum(S, fused, drowc, lddrc, C, T, qscale, length_scaling, group, pitch, st);
    }
    SEMICRF_CHECK_LAUNCH("interval_score_bwd_fused_ws");
    return SEMICRF_OK;
}

int interval_score_bwd_fused_ws_p(const float* S, const float* alpha, const float* beta, const float* logZ,
                                  const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                  int64_t ldk, float qscale, int length_scaling, int group, int pitch, float* dq, float* dk, float* ddiag,
                                  int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return interval_score_bwd_fused_ws_pc(S, alpha, beta, logZ, gout, q, k, C, T, D, ldq, ldk, qscale, length_scaling, group, pitch, dq, dk,
                                          ddiag, nullptr, lddq, lddk, lddd, 1, ws, ws_bytes, stream);
}

int interval_score_bwd_fused_ws(const float* S, const float* alpha, const float* beta, const float* logZ,
                                const float* gout, const float* q, const float* k, int C, int T, int D, int64_t ldq,
                                int64_t ldk, float qscale, int length_scaling, float* dq, float* dk, float* ddiag,
                                int64_t lddq, int64_t lddk, int64_t lddd, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return interval_score_bwd_fused_ws_p(S, alpha, beta, logZ, gout, q, k, C, T, D, ldq, ldk, qscale, length_scaling, C > 0 ? C : 1,
                                         C > 0 ? C : 1, dq, dk, ddiag, lddq, lddk, lddd, ws, ws_bytes, stream);
}

int interval_score_path_bwd_pc(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                               const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale, int length_scaling,
                               int group, int pitch, float* dq, float* dk, float* ddiag, float* drowc, int64_t lddq, int64_t lddk,
                               int64_t lddd, int64_t lddrc, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(!drowc || lddrc >= 1, "bad row-constant stride");
    // (its own sequence: the interval count is reported between the operands and the leading dimensions)
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1, "C=%d T=%d D=%d must be >= 1", C, T, D);
    SEMICRF_CHECK_ARG(gout && offsets && q && k, "gout/offsets/q/k must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || pairs), "bad interval count");
    SEMICRF_CHECK_ARG(bwd_lds_ok(D, ldq, ldk, dq, dk, ddiag, lddq, lddk, lddd), "bad leading dimensions");
    SEMICRF_CHECK_ARG(length_scaling >= 0 && length_scaling <= 2, "bad length_scaling %d", length_scaling);
    if (int rc = check_slots(C, group, pitch)) return rc;
    launch_interval_score_path_bwd(gout, pairs, (int)K, offsets, q, k, C, T, D, ldq, ldk, qscale, length_scaling, dq, dk, ddiag,
                                   lddq, lddk, lddd, (hipStream_t)stream, group, pitch, drowc, lddrc);
    SEMICRF_CHECK_LAUNCH("interval_score_path_bwd");
    return SEMICRF_OK;
}

int interval_score_path_bwd_p(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                              const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale, int length_scaling,
                              int group, int pitch, float* dq, float* dk, float* ddiag, int64_t lddq, int64_t lddk, int64_t lddd,
                              semicrf_stream_t stream)
{
    return interval_score_path_bwd_pc(gout, pairs, K, offsets, q, k, C, T, D, ldq, ldk, qscale, length_scaling, group, pitch, dq, dk, ddiag,
                                      nullptr, lddq, lddk, lddd, 1, stream);
}

int interval_score_path_bwd(const float* gout, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* q,
                            const float* k, int C, int T, int D, int64_t ldq, int64_t ldk, float qscale, int length_scaling,
                            float* dq, float* dk, float* ddiag, int64_t lddq, int64_t lddk, int64_t lddd,
                            semicrf_stream_t stream)
{
    return interval_score_path_bwd_p(gout, pairs, K, offsets, q, k, C, T, D, ldq, ldk, qscale, length_scaling, C > 0 ? C : 1, C > 0 ? C : 1,
                                     dq, dk, ddiag, lddq, lddk, lddd, stream);
}

int scorer_proj_nn(const float* A, int64_t lda, int64_t M, int K, const float* B, int64_t ldb, int N, float* out, int64_t ldout,
                   const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(A && B && out, "A/B/out must be non-NULL");
    SEMICRF_CHECK_ARG(M >= 1 && K >= 4 && lda >= K && ldb >= N && zero_cols >= 0 && (!w2 || b2), "bad sizes");
    SEMICRF_CHECK_ARG(ldout >= N + (w2 ? 2 + zero_cols : 0), "ldout too small for the packed output");
    SEMICRF_CHECK_ARG(launch_proj_nn(A, lda, M, K, B, ldb, N, out, ldout, bias, w2, b2, zero_cols, accumulate, (hipStream_t)stream) == 0,
                      "scorer_proj_nn: N must be 64, 128 or 256, K %% 4 == 0, rows 16-byte aligned, M * ld * 4 < 2^31 (N=%d K=%d)", N, K);
    SEMICRF_CHECK_LAUNCH("scorer_proj_nn");
    return SEMICRF_OK;
}

size_t scorer_proj_nn3_workspace_bytes(int K, int N) { return proj_nn3_workspace_bytes(K, N); }

int scorer_proj_nn3(const float* A, int64_t lda, int64_t M, int K, const float* B, int64_t ldb, int N, float* out, int64_t ldout,
                    const float* bias, const float* w2, const float* b2, int zero_cols, int accumulate, void* ws, size_t ws_bytes,
                    semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(A && B && out, "A/B/out must be non-NULL");
    SEMICRF_CHECK_ARG(M >= 1 && K >= 4 && lda >= K && ldb >= N && zero_cols >= 0 && (!w2 || b2), "bad sizes");
    SEMICRF_CHECK_ARG(ldout >= N + (w2 ? 2 + zero_cols : 0), "ldout too small for the packed output");
    if (launch_proj_nn3(A, lda, M, K, B, ldb, N, out, ldout, bias, w2, b2, zero_cols, accumulate, ws, ws_bytes, (hipStream_t)stream) != 0)
        return scorer_proj_nn(A, lda, M, K, B, ldb, N, out, ldout, bias, w2, b2, zero_cols, accumulate, stream);      // not this kernel's shape: exact
    SEMICRF_CHECK_LAUNCH("scorer_proj_nn3");
    return SEMICRF_OK;
}

size_t scorer_proj_tn_workspace_bytes(int64_t M, int R, int N) { return M >= 1 && R >= 1 ? proj_tn_workspace_bytes(M, R, N) : 0; }

int scorer_proj_tn(const float* dy, int64_t lddy, int64_t M, int R, int extra_col0, int total_rows, const float* x, int64_t ldx, int N,
                   float* dW, int64_t lddw, float* db, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(dy && x && dW, "dy/x/dW must be non-NULL");
    const int x3flag = total_rows & SEMICRF_PROJ_TN_BF16X3;       // opt-in: the matrix part on the three-limb bf16 kernel
    total_rows &= ~SEMICRF_PROJ_TN_BF16X3;
    SEMICRF_CHECK_ARG(M >= 1 && R >= 1 && total_rows >= R && lddy >= R && ldx >= N && lddw >= N, "bad sizes");
    SEMICRF_CHECK_ARG(extra_col0 < 0 || (extra_col0 >= R && extra_col0 + 2 <= total_rows && extra_col0 + 2 <= lddy), "bad extra columns");
    const int rc = launch_proj_tn(dy, lddy, M, R, extra_col0, total_rows | x3flag, x, ldx, N, dW, lddw, db, ws, ws_bytes, (hipStream_t)stream);
    if (rc == 2) { set_error("scorer_proj_tn: workspace missing or too small"); return SEMICRF_EWORKSPACE; }
    SEMICRF_CHECK_ARG(rc == 0, "scorer_proj_tn: N must be 64, 128 or 256, rows 16-byte aligned, M * ld * 4 < 2^31 (N=%d)", N);
    SEMICRF_CHECK_LAUNCH("scorer_proj_tn");
    return SEMICRF_OK;
}

int scorer_merge_weights_fwd(const float* W, const float* bias, int D, int size, int rows, float* Wm, float* bm, float* WmT,
                             semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(W && bias && Wm && bm, "W/bias/Wm/bm must be non-NULL");
    SEMICRF_CHECK_ARG(D >= 1 && size >= 1 && size <= 256 && rows >= size + 2, "scorer_merge_weights: D=%d size=%d (<= 256) rows=%d (>= size + 2)", D, size, rows);
    launch_merge_weights_fwd(W, bias, D, size, rows, Wm, bm, WmT, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("scorer_merge_weights_fwd");
    return SEMICRF_OK;
}

int scorer_stage_linear(const float* W, const float* bias, int D, int size, int rows_pad, float* BT, float* Wqd, float* w2, float* b2,
                        semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(W && bias && BT && Wqd && w2 && b2, "W/bias/BT/Wqd/w2/b2 must be non-NULL");
    SEMICRF_CHECK_ARG(D >= 1 && size >= 1 && rows_pad >= D + 1 && rows_pad < (1 << 20), "scorer_stage_linear: D=%d size=%d rows_pad=%d (>= D + 1)", D, size, rows_pad);
    launch_stage_linear(W, bias, D, size, rows_pad, BT, Wqd, w2, b2, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("scorer_stage_linear");
    return SEMICRF_OK;
}

size_t scorer_merge_weights_bwd_workspace_bytes(int size) { return size >= 1 ? merge_weights_bwd_workspace_bytes(size) : 0; }

int scorer_merge_weights_bwd(const float* W, const float* bias, const float* dWm, const float* dbm, int D, int size, int rows, float* dW,
                             float* dbias, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(W && bias && dWm && dbm && dW && dbias, "W/bias/dWm/dbm/dW/dbias must be non-NULL");
    SEMICRF_CHECK_ARG(D >= 1 && size >= 1 && size <= 256 && rows >= size + 2, "scorer_merge_weights: D=%d size=%d (<= 256) rows=%d (>= size + 2)", D, size, rows);
    if (!ws || ws_bytes < merge_weights_bwd_workspace_bytes(size) || ((uintptr_t)ws & 3)) { set_error("scorer_merge_weights_bwd: workspace missing or too small"); return SEMICRF_EWORKSPACE; }
    launch_merge_weights_bwd(W, bias, dWm, dbm, D, size, dW, dbias, (float*)ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("scorer_merge_weights_bwd");
    return SEMICRF_OK;
}

int interval_features_gather(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K,
                             const int32_t* offsets, int nSym, float* out, int64_t* symIdx, int64_t* scatterIdx,
                             semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1 && nSym >= 1, "C=%d T=%d D=%d nSym=%d must be >= 1", C, T, D, nSym);
    SEMICRF_CHECK_ARG(ctx && offsets, "ctx/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(ldc >= D, "bad row stride");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || (pairs && out)), "bad interval count / buffers");
    launch_interval_features(ctx, C, T, D, ldc, pairs, (int)K, offsets, nSym, out, (long long*)symIdx, (long long*)scatterIdx,
                             (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("interval_features_gather");
    return SEMICRF_OK;
}

int interval_features_gather_bwd(const float* gout, const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs,
                                 int64_t K, const int32_t* offsets, float* dctx, int64_t lddc, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1, "C=%d T=%d D=%d must be >= 1", C, T, D);
    SEMICRF_CHECK_ARG(ctx && offsets && dctx, "ctx/offsets/dctx must be non-NULL");
    SEMICRF_CHECK_ARG(ldc >= D && lddc >= D, "bad row stride");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31) && (K == 0 || (pairs && gout)), "bad interval count / buffers");
    launch_interval_features_bwd(gout, ctx, C, T, D, ldc, pairs, (int)K, offsets, dctx, lddc, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("interval_features_gather_bwd");
    return SEMICRF_OK;
}

int semicrf_attribute_loss_fwd(const float* logitsVelocity, const float* ofLogits, const int32_t* velocity, const float* ofRefined,
                               const float* ofPresence, int64_t K, const int32_t* offsets, int C, const float* base, float* rowLogProb,
                               float* out, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1, "C=%d must be >= 1", C);
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31), "bad interval count");
    if (K == 0) return SEMICRF_OK;                         // nothing to add: the caller's base IS the result (ModelTransformer.py:273)
    SEMICRF_CHECK_ARG(logitsVelocity && ofLogits && velocity && ofRefined && ofPresence && offsets && rowLogProb && out,
                      "logitsVelocity/ofLogits/velocity/ofRefined/ofPresence/offsets/rowLogProb/out must be non-NULL");
    SEMICRF_CHECK_ARG(((uintptr_t)logitsVelocity & 7) == 0, "logitsVelocity must be 8-byte aligned");
    launch_attr_loss_fwd(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, (int)K, offsets, C, base, rowLogProb, out,
                         (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_loss_fwd");
    return SEMICRF_OK;
}

int semicrf_attribute_loss_bwd(const float* gout, int gstride, const float* logitsVelocity, const float* ofLogits, const int32_t* velocity,
                               const float* ofRefined, const float* ofPresence, int64_t K, const int32_t* offsets, int C,
                               float* dLogitsVelocity, float* dOfLogits, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1, "C=%d must be >= 1", C);
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31), "bad interval count");
    SEMICRF_CHECK_ARG(gstride == 0 || gstride == 1, "gout stride must be 0 (one value for all chains) or 1");
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(gout && logitsVelocity && ofLogits && velocity && ofRefined && ofPresence && offsets && dLogitsVelocity && dOfLogits,
                      "gout/logitsVelocity/ofLogits/velocity/ofRefined/ofPresence/offsets/dLogitsVelocity/dOfLogits must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)logitsVelocity | (uintptr_t)dLogitsVelocity) & 7) == 0, "logitsVelocity/dLogitsVelocity must be 8-byte aligned");
    launch_attr_loss_bwd(gout, gstride, logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, (int)K, offsets, C, dLogitsVelocity,
                         dOfLogits, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_loss_bwd");
    return SEMICRF_OK;
}

int semicrf_attribute_decode(const float* logitsVelocity, const float* ofLogits, int64_t K, int criterion, int64_t* velocityClass,
                             float* velocityMean, float* ofValue, unsigned char* ofPresence, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(criterion >= SEMICRF_VEL_HAMMING && criterion <= SEMICRF_VEL_MAE, "criterion=%d is none of SEMICRF_VEL_*", criterion);
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31), "bad row count");
    SEMICRF_CHECK_ARG(criterion == SEMICRF_VEL_MSE ? velocityMean != nullptr : velocityClass != nullptr,
                      "velocityClass (class criteria) / velocityMean (SEMICRF_VEL_MSE) must be non-NULL");
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(logitsVelocity && ofLogits && ofValue && ofPresence, "logitsVelocity/ofLogits/ofValue/ofPresence must be non-NULL");
    SEMICRF_CHECK_ARG(((uintptr_t)logitsVelocity & 7) == 0, "logitsVelocity must be 8-byte aligned");
    launch_attr_decode(logitsVelocity, ofLogits, (int)K, criterion, (long long*)velocityClass, velocityMean, ofValue, ofPresence,
                       (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_decode");
    return SEMICRF_OK;
}

size_t semicrf_attribute_heads_workspace_bytes(int64_t K, int Hv, int Ho, int Nv, int No)
{
    if (K < 0 || Hv < 1 || Ho < 1 || Nv < 1 || No < 1) return 0;
    return attr_heads_workspace_bytes(K, Hv, Ho, Nv, No);
}

int semicrf_attribute_heads(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets,
                            int nSym, const float* W1, const float* b1, const float* W2, const float* b2, int Hv, int Ho, int Nv, int No,
                            float* logitsVelocity, float* ofLogits, int64_t* symIdx, int64_t* scatterIdx, void* ws, size_t ws_bytes,
                            semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1 && nSym >= 1, "C=%d T=%d D=%d nSym=%d must be >= 1", C, T, D, nSym);
    SEMICRF_CHECK_ARG(Hv >= 1 && Ho >= 1 && Nv >= 1 && No >= 1, "Hv=%d Ho=%d Nv=%d No=%d must be >= 1", Hv, Ho, Nv, No);
    SEMICRF_CHECK_ARG(D < (1 << 20) && Hv < (1 << 21) && Ho < (1 << 21) && Nv < (1 << 20) && No < (1 << 20), "D / hidden / output sizes too large");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31), "bad interval count K=%lld", (long long)K);
    SEMICRF_CHECK_ARG(ldc >= D, "bad row stride ldc=%lld < D=%d", (long long)ldc, D);
    SEMICRF_CHECK_ARG(ctx && offsets, "ctx/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(W1 && b1 && W2 && b2, "W1/b1/W2/b2 must be non-NULL");
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(pairs && logitsVelocity && ofLogits, "pairs/logitsVelocity/ofLogits must be non-NULL");
    SEMICRF_CHECK_ARG((long long)K * ((long long)Nv + No) < (1ll << 38), "K * (Nv + No) too large");
    const size_t need = attr_heads_workspace_bytes(K, Hv, Ho, Nv, No);
    SEMICRF_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "ws must be non-NULL and 4-byte aligned");
    if (ws_bytes < need) {
        set_error("workspace too small for attribute_heads: %zu bytes given, semicrf_attribute_heads_workspace_bytes says %zu", ws_bytes, need);
        return SEMICRF_EWORKSPACE;
    }
    launch_attr_heads(ctx, C, T, D, ldc, pairs, (int)K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                      (long long*)symIdx, (long long*)scatterIdx, (float*)ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_heads");
    return SEMICRF_OK;
}

size_t semicrf_attribute_heads_train_fwd_workspace_bytes(int64_t K, int Hv, int Ho, int Nv, int No)
{
    return semicrf_attribute_heads_workspace_bytes(K, Hv, Ho, Nv, No);
}

// the checks the three training entry points share with semicrf_attribute_heads
static int check_heads_sizes(int Hv, int Ho, int Nv, int No, int64_t K, double pv, double po)
{
    SEMICRF_CHECK_ARG(Hv >= 1 && Ho >= 1 && Nv >= 1 && No >= 1, "Hv=%d Ho=%d Nv=%d No=%d must be >= 1", Hv, Ho, Nv, No);
    SEMICRF_CHECK_ARG(Hv < (1 << 21) && Ho < (1 << 21) && Nv < (1 << 20) && No < (1 << 20), "hidden / output sizes too large");
    SEMICRF_CHECK_ARG(K >= 0 && K < (1ll << 31), "bad interval count K=%lld", (long long)K);
    SEMICRF_CHECK_ARG(pv >= 0.0 && pv < 1.0 && po >= 0.0 && po < 1.0, "dropout probabilities pv=%g po=%g must lie in [0, 1)", pv, po);
    return SEMICRF_OK;
}

int semicrf_attribute_heads_train_fwd(const float* ctx, int C, int T, int D, int64_t ldc, const int32_t* pairs, int64_t K,
                                      const int32_t* offsets, int nSym, const float* W1, const float* b1, const float* W2, const float* b2,
                                      int Hv, int Ho, int Nv, int No, uint64_t seed, double pv, double po, float* logitsVelocity,
                                      float* ofLogits, float* z, int64_t* symIdx, int64_t* scatterIdx, void* ws, size_t ws_bytes,
                                      semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1 && nSym >= 1, "C=%d T=%d D=%d nSym=%d must be >= 1", C, T, D, nSym);
    if (const int rc = check_heads_sizes(Hv, Ho, Nv, No, K, pv, po)) return rc;
    SEMICRF_CHECK_ARG(D < (1 << 20), "D too large");
    SEMICRF_CHECK_ARG(ldc >= D, "bad row stride ldc=%lld < D=%d", (long long)ldc, D);
    SEMICRF_CHECK_ARG(ctx && offsets, "ctx/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(W1 && b1 && W2 && b2, "W1/b1/W2/b2 must be non-NULL");
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(pairs && logitsVelocity && ofLogits && z, "pairs/logitsVelocity/ofLogits/z must be non-NULL");
    SEMICRF_CHECK_ARG((long long)K * ((long long)Nv + No) < (1ll << 38), "K * (Nv + No) too large");
    const size_t need = attr_heads_workspace_bytes(K, Hv, Ho, Nv, No);
    SEMICRF_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "ws must be non-NULL and 4-byte aligned");
    if (ws_bytes < need) {
        set_error("workspace too small for attribute_heads_train_fwd: %zu bytes given, semicrf_attribute_heads_train_fwd_workspace_bytes says %zu",
                  ws_bytes, need);
        return SEMICRF_EWORKSPACE;
    }
    launch_attr_heads(ctx, C, T, D, ldc, pairs, (int)K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, logitsVelocity, ofLogits,
                      (long long*)symIdx, (long long*)scatterIdx, (float*)ws, (hipStream_t)stream, z, seed, pv, po);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_heads_train_fwd");
    return SEMICRF_OK;
}

size_t semicrf_attribute_heads_bwd_workspace_bytes(int64_t K, int D, int Hv, int Ho, int Nv, int No)
{
    if (K < 0 || D < 1 || Hv < 1 || Ho < 1 || Nv < 1 || No < 1) return 0;
    return attr_heads_bwd_workspace_bytes(K, D, Hv, Ho, Nv, No);
}

int semicrf_attribute_heads_bwd(const float* dLogitsVelocity, const float* dOfLogits, const float* z, const float* ctx, int C, int T, int D,
                                int64_t ldc, const int32_t* pairs, int64_t K, const int32_t* offsets, const float* W1, const float* W2,
                                int Hv, int Ho, int Nv, int No, uint64_t seed, double pv, double po, float* dctx, float* dW1, float* db1,
                                float* dW2, float* db2, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(C >= 1 && T >= 1 && D >= 1, "C=%d T=%d D=%d must be >= 1", C, T, D);
    if (const int rc = check_heads_sizes(Hv, Ho, Nv, No, K, pv, po)) return rc;
    SEMICRF_CHECK_ARG(D < (1 << 20) && (long long)C * T < (1ll << 31), "D or C * T too large");
    SEMICRF_CHECK_ARG(3ll * D * ((long long)Hv + Ho) < (1ll << 36), "3 D (Hv + Ho) too large");
    SEMICRF_CHECK_ARG(ldc >= D, "bad row stride ldc=%lld < D=%d", (long long)ldc, D);
    SEMICRF_CHECK_ARG(K <= 65535ll * SEMICRF_HEADS_BWD_ROW_CHUNK, "K=%lld: more than 65535 row chunks", (long long)K);
    SEMICRF_CHECK_ARG(ctx && offsets, "ctx/offsets must be non-NULL");
    SEMICRF_CHECK_ARG(W1 && W2, "W1/W2 must be non-NULL");
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(pairs && dLogitsVelocity && dOfLogits && z, "pairs/dLogitsVelocity/dOfLogits/z must be non-NULL");
    SEMICRF_CHECK_ARG(dctx && dW1 && db1 && dW2 && db2, "dctx/dW1/db1/dW2/db2 must be non-NULL");
    const size_t need = attr_heads_bwd_workspace_bytes(K, D, Hv, Ho, Nv, No);
    SEMICRF_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "ws must be non-NULL and 4-byte aligned");
    if (ws_bytes < need) {
        set_error("workspace too small for attribute_heads_bwd: %zu bytes given, semicrf_attribute_heads_bwd_workspace_bytes says %zu", ws_bytes,
                  need);
        return SEMICRF_EWORKSPACE;
    }
    const hipError_t e = launch_attr_heads_bwd(dLogitsVelocity, dOfLogits, z, ctx, C, T, D, ldc, pairs, (int)K, offsets, W1, W2, Hv, Ho, Nv, No,
                                               seed, pv, po, dctx, dW1, db1, dW2, db2, (float*)ws, (hipStream_t)stream);
    if (e != hipSuccess) {
        set_error("semicrf_attribute_heads_bwd: %s", hipGetErrorString(e));
        return SEMICRF_ELAUNCH;
    }
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_heads_bwd");
    return SEMICRF_OK;
}

int semicrf_attribute_heads_dropout_mask(uint64_t seed, int64_t K, int Hv, int Ho, double pv, double po, unsigned char* mask,
                                         semicrf_stream_t stream)
{
    if (const int rc = check_heads_sizes(Hv, Ho, 1, 1, K, pv, po)) return rc;
    if (K == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(mask, "mask must be non-NULL");
    launch_attr_heads_mask(seed, K, Hv, Ho, pv, po, mask, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_attribute_heads_dropout_mask");
    return SEMICRF_OK;
}

int segment_onset_filter(const int32_t* pairs, const int32_t* offsets, int B, int bound, int32_t* pairs_out, int64_t cap,
                         int32_t* offsets_out, int32_t* counts_ws, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(B >= 1, "B=%d must be >= 1", B);
    SEMICRF_CHECK_ARG(offsets && offsets_out && counts_ws && cap >= 0 && (cap == 0 || (pairs && pairs_out)), "NULL buffer");
    launch_onset_filter(pairs, offsets, B, bound, pairs_out, (long long)cap, offsets_out, counts_ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("segment_onset_filter");
    return SEMICRF_OK;
}

int segment_events(const int32_t* pairs, int64_t K, const int32_t* offsets, int B, int nSym, const float* ofValue,
                   const unsigned char* ofPresence, int lastFrameIdx, double frameDur, const double* beginTime, int stepFrames,
                   double* times, unsigned char* flags, int32_t* lastP, int32_t* nextStart, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(B >= 1 && nSym >= 1 && B % nSym == 0, "B=%d must be a positive multiple of nSym=%d", B, nSym);
    SEMICRF_CHECK_ARG(offsets && beginTime && lastP && nextStart, "offsets/beginTime/lastP/nextStart must be non-NULL");
    SEMICRF_CHECK_ARG(K >= 0 && (K == 0 || (pairs && ofValue && ofPresence && times && flags)), "bad interval count / buffers");
    launch_segment_events(pairs, offsets, B, nSym, ofValue, ofPresence, lastFrameIdx, frameDur, beginTime, stepFrames, times, flags,
                          lastP, nextStart, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("segment_events");
    return SEMICRF_OK;
}

int semicrf_grad_sqnorm(const float* flat, int64_t numel, double* partials, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(numel >= 1 && numel < (1ll << 40), "numel=%lld must be in [1, 2^40)", (long long)numel);
    SEMICRF_CHECK_ARG(flat && partials, "flat/partials must be non-NULL");
    SEMICRF_CHECK_ARG(((uintptr_t)flat & 3) == 0 && ((uintptr_t)partials & 7) == 0, "flat must be 4-byte, partials 8-byte aligned");
    launch_grad_sqnorm(flat, numel, partials, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_grad_sqnorm");
    return SEMICRF_OK;
}

int semicrf_clip_from_history(const double* partials, int64_t numel, const float* norm_in, double q, float* ring, int capacity,
                              int32_t* state, int append, float* stats, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(capacity >= 1 && capacity <= SEMICRF_HISTORY_MAX, "capacity=%d must be in [1, %d]", capacity, SEMICRF_HISTORY_MAX);
    SEMICRF_CHECK_ARG(ring && state && stats, "ring/state/stats must be non-NULL");
    SEMICRF_CHECK_ARG(!partials || (numel >= 1 && numel < (1ll << 40)), "numel=%lld must be in [1, 2^40) when partials are given", (long long)numel);
    SEMICRF_CHECK_ARG(q < 0.0 || q <= 1.0, "the quantile q=%g must lie in [0, 1] (negative: none)", q);
    SEMICRF_CHECK_ARG(((uintptr_t)partials & 7) == 0, "partials must be 8-byte aligned");
    launch_clip_from_history(partials, numel, norm_in, q, ring, capacity, state, append, stats, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_clip_from_history");
    return SEMICRF_OK;
}

int semicrf_adabelief_step(float* p, const float* g, float* m, float* s, int64_t numel, const float* coef,
                           semicrf_adabelief_groups groups, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(numel >= 1 && numel < (1ll << 40), "numel=%lld must be in [1, 2^40)", (long long)numel);
    SEMICRF_CHECK_ARG(p && g && m && s, "p/g/m/s must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)s) & 3) == 0, "p/g/m/s must be 4-byte aligned");
    SEMICRF_CHECK_ARG(groups.n >= 1 && groups.n <= SEMICRF_OPTIM_MAX_GROUPS, "groups.n=%d must be in [1, %d]", groups.n, SEMICRF_OPTIM_MAX_GROUPS);
    int64_t last = 0;
    for (int i = 0; i < groups.n; ++i) {
        SEMICRF_CHECK_ARG(groups.g[i].end > last, "group %d is empty or out of order (end=%lld)", i, (long long)groups.g[i].end);
        last = groups.g[i].end;
    }
    SEMICRF_CHECK_ARG(last == numel, "the last group ends at %lld, not at numel=%lld", (long long)last, (long long)numel);
    launch_adabelief_step(p, g, m, s, numel, coef, groups, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_adabelief_step");
    return SEMICRF_OK;
}

int semicrf_axial_attention_supported(int Lq, int Lk, int H, int d) { return attention::supported(Lq, Lk, H, d) ? 1 : 0; }

int semicrf_axial_attention(const float* q, const float* k, const float* v, float* out, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d,
                            int64_t q_stride_s0, int64_t q_stride_s1, int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1,
                            int64_t k_stride_l, int64_t v_stride_s0, int64_t v_stride_s1, int64_t v_stride_l, int64_t out_stride_s0,
                            int64_t out_stride_s1, int64_t out_stride_l, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(attention::supported(Lq, Lk, H, d),
                      "axial_attention: Lq=%d Lk=%d H=%d d=%d is outside the supported set (1 <= Lq, Lk <= %d; d a multiple of 8 in [%d, %d]; "
                      "H >= 1): see semicrf_axial_attention_supported", Lq, Lk, H, d, attention::ATT_MAX_L, attention::ATT_MIN_D,
                      attention::ATT_MAX_D);
    SEMICRF_CHECK_ARG(n0 >= 0 && n1 >= 0, "axial_attention: n0=%lld n1=%lld must be >= 0", (long long)n0, (long long)n1);
    if (n0 == 0 || n1 == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(n0 < (1ll << 31) && n1 < (1ll << 31) && n0 * n1 * H < (1ll << 31),
                      "axial_attention: n0 * n1 * H = %lld * %lld * %d must stay below 2^31", (long long)n0, (long long)n1, H);
    SEMICRF_CHECK_ARG(q && k && v && out, "axial_attention: q/k/v/out must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 3) == 0, "axial_attention: q/k/v/out must be 4-byte aligned");
    const long long strides[12] = {q_stride_s0, q_stride_s1, q_stride_l, k_stride_s0, k_stride_s1, k_stride_l,
                                   v_stride_s0, v_stride_s1, v_stride_l, out_stride_s0, out_stride_s1, out_stride_l};
    for (int i = 0; i < 12; ++i) SEMICRF_CHECK_ARG(strides[i] >= 0, "axial_attention: stride %d is negative (%lld)", i, strides[i]);
    for (int i = 2; i < 12; i += 3)
        SEMICRF_CHECK_ARG(strides[i] < (1ll << 28), "axial_attention: token stride %lld must stay below 2^28 elements", strides[i]);
    launch_axial_attention(q, k, v, out, n0, n1, Lq, Lk, H, d, strides, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_axial_attention");
    return SEMICRF_OK;
}

int semicrf_axial_attention_bf16_supported(int Lq, int Lk, int H, int d) { return attention::supported(Lq, Lk, H, d) ? 1 : 0; }

int semicrf_axial_attention_bf16(const uint16_t* q, const uint16_t* k, const uint16_t* v, uint16_t* out, int64_t n0, int64_t n1, int Lq, int Lk,
                                 int H, int d, int64_t q_stride_s0, int64_t q_stride_s1, int64_t q_stride_l, int64_t k_stride_s0,
                                 int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0, int64_t v_stride_s1, int64_t v_stride_l,
                                 int64_t out_stride_s0, int64_t out_stride_s1, int64_t out_stride_l, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(attention::supported(Lq, Lk, H, d),
                      "axial_attention_bf16: Lq=%d Lk=%d H=%d d=%d is outside the supported set (1 <= Lq, Lk <= %d; d a multiple of 8 in "
                      "[%d, %d]; H >= 1): see semicrf_axial_attention_bf16_supported", Lq, Lk, H, d, attention::ATT_MAX_L, attention::ATT_MIN_D,
                      attention::ATT_MAX_D);
    SEMICRF_CHECK_ARG(n0 >= 0 && n1 >= 0, "axial_attention_bf16: n0=%lld n1=%lld must be >= 0", (long long)n0, (long long)n1);
    if (n0 == 0 || n1 == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(n0 < (1ll << 31) && n1 < (1ll << 31) && n0 * n1 * H < (1ll << 31),
                      "axial_attention_bf16: n0 * n1 * H = %lld * %lld * %d must stay below 2^31", (long long)n0, (long long)n1, H);
    SEMICRF_CHECK_ARG(q && k && v && out, "axial_attention_bf16: q/k/v/out must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) & 1) == 0,
                      "axial_attention_bf16: q/k/v/out must be 2-byte aligned");
    const long long strides[12] = {q_stride_s0, q_stride_s1, q_stride_l, k_stride_s0, k_stride_s1, k_stride_l,
                                   v_stride_s0, v_stride_s1, v_stride_l, out_stride_s0, out_stride_s1, out_stride_l};
    for (int i = 0; i < 12; ++i) SEMICRF_CHECK_ARG(strides[i] >= 0, "axial_attention_bf16: stride %d is negative (%lld)", i, strides[i]);
    for (int i = 2; i < 12; i += 3)
        SEMICRF_CHECK_ARG(strides[i] < (1ll << 28), "axial_attention_bf16: token stride %lld must stay below 2^28 elements", strides[i]);
    launch_axial_attention_bf16(q, k, v, out, n0, n1, Lq, Lk, H, d, strides, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_axial_attention_bf16");
    return SEMICRF_OK;
}

int semicrf_axial_attention_bf16_bwd_supported(int Lq, int Lk, int H, int d) { return attention::supported(Lq, Lk, H, d) ? 1 : 0; }

int semicrf_axial_attention_bf16_bwd(const uint16_t* q, const uint16_t* k, const uint16_t* v, const uint16_t* dout, uint16_t* dq, uint16_t* dk,
                                     uint16_t* dv, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, int64_t q_stride_s0, int64_t q_stride_s1,
                                     int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0,
                                     int64_t v_stride_s1, int64_t v_stride_l, int64_t dout_stride_s0, int64_t dout_stride_s1,
                                     int64_t dout_stride_l, int64_t dq_stride_s0, int64_t dq_stride_s1, int64_t dq_stride_l, int64_t dk_stride_s0,
                                     int64_t dk_stride_s1, int64_t dk_stride_l, int64_t dv_stride_s0, int64_t dv_stride_s1, int64_t dv_stride_l,
                                     semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(attention::supported(Lq, Lk, H, d),
                      "axial_attention_bf16_bwd: Lq=%d Lk=%d H=%d d=%d is outside the supported set (1 <= Lq, Lk <= %d; d a multiple of 8 in "
                      "[%d, %d]; H >= 1): see semicrf_axial_attention_bf16_bwd_supported", Lq, Lk, H, d, attention::ATT_MAX_L,
                      attention::ATT_MIN_D, attention::ATT_MAX_D);
    SEMICRF_CHECK_ARG(n0 >= 0 && n1 >= 0, "axial_attention_bf16_bwd: n0=%lld n1=%lld must be >= 0", (long long)n0, (long long)n1);
    if (n0 == 0 || n1 == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(n0 < (1ll << 31) && n1 < (1ll << 31) && n0 * n1 * H < (1ll << 31),
                      "axial_attention_bf16_bwd: n0 * n1 * H = %lld * %lld * %d must stay below 2^31", (long long)n0, (long long)n1, H);
    SEMICRF_CHECK_ARG(q && k && v && dout, "axial_attention_bf16_bwd: q/k/v/dout must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 1) == 0,
                      "axial_attention_bf16_bwd: every pointer must be 2-byte aligned");
    const long long strides[21] = {q_stride_s0, q_stride_s1, q_stride_l, k_stride_s0, k_stride_s1, k_stride_l, v_stride_s0, v_stride_s1,
                                   v_stride_l, dout_stride_s0, dout_stride_s1, dout_stride_l, dq_stride_s0, dq_stride_s1, dq_stride_l,
                                   dk_stride_s0, dk_stride_s1, dk_stride_l, dv_stride_s0, dv_stride_s1, dv_stride_l};
    for (int i = 0; i < 21; ++i) SEMICRF_CHECK_ARG(strides[i] >= 0, "axial_attention_bf16_bwd: stride %d is negative (%lld)", i, strides[i]);
    for (int i = 2; i < 21; i += 3)
        SEMICRF_CHECK_ARG(strides[i] < (1ll << 28), "axial_attention_bf16_bwd: token stride %lld must stay below 2^28 elements", strides[i]);
    if (!dq && !dk && !dv) return SEMICRF_OK;
    launch_axial_attention_bf16_bwd(q, k, v, dout, dq, dk, dv, n0, n1, Lq, Lk, H, d, strides, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_axial_attention_bf16_bwd");
    return SEMICRF_OK;
}

int semicrf_axial_attention_bwd_supported(int Lq, int Lk, int H, int d) { return attention::supported(Lq, Lk, H, d) ? 1 : 0; }

int semicrf_axial_attention_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout, float* dq, float* dk,
                                float* dv, int64_t n0, int64_t n1, int Lq, int Lk, int H, int d, int64_t q_stride_s0, int64_t q_stride_s1,
                                int64_t q_stride_l, int64_t k_stride_s0, int64_t k_stride_s1, int64_t k_stride_l, int64_t v_stride_s0,
                                int64_t v_stride_s1, int64_t v_stride_l, int64_t out_stride_s0, int64_t out_stride_s1, int64_t out_stride_l,
                                int64_t dout_stride_s0, int64_t dout_stride_s1, int64_t dout_stride_l, int64_t dq_stride_s0,
                                int64_t dq_stride_s1, int64_t dq_stride_l, int64_t dk_stride_s0, int64_t dk_stride_s1, int64_t dk_stride_l,
                                int64_t dv_stride_s0, int64_t dv_stride_s1, int64_t dv_stride_l, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(attention::supported(Lq, Lk, H, d),
                      "axial_attention_bwd: Lq=%d Lk=%d H=%d d=%d is outside the supported set (1 <= Lq, Lk <= %d; d a multiple of 8 in "
                      "[%d, %d]; H >= 1): see semicrf_axial_attention_bwd_supported", Lq, Lk, H, d, attention::ATT_MAX_L, attention::ATT_MIN_D,
                      attention::ATT_MAX_D);
    SEMICRF_CHECK_ARG(n0 >= 0 && n1 >= 0, "axial_attention_bwd: n0=%lld n1=%lld must be >= 0", (long long)n0, (long long)n1);
    if (n0 == 0 || n1 == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(n0 < (1ll << 31) && n1 < (1ll << 31) && n0 * n1 * H < (1ll << 31),
                      "axial_attention_bwd: n0 * n1 * H = %lld * %lld * %d must stay below 2^31", (long long)n0, (long long)n1, H);
    SEMICRF_CHECK_ARG(q && k && v && out && dout, "axial_attention_bwd: q/k/v/out/dout must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk |
                        (uintptr_t)dv) & 3) == 0, "axial_attention_bwd: every pointer must be 4-byte aligned");
    const long long strides[24] = {q_stride_s0, q_stride_s1, q_stride_l, k_stride_s0, k_stride_s1, k_stride_l, v_stride_s0, v_stride_s1,
                                   v_stride_l, out_stride_s0, out_stride_s1, out_stride_l, dout_stride_s0, dout_stride_s1, dout_stride_l,
                                   dq_stride_s0, dq_stride_s1, dq_stride_l, dk_stride_s0, dk_stride_s1, dk_stride_l, dv_stride_s0,
                                   dv_stride_s1, dv_stride_l};
    for (int i = 0; i < 24; ++i) SEMICRF_CHECK_ARG(strides[i] >= 0, "axial_attention_bwd: stride %d is negative (%lld)", i, strides[i]);
    for (int i = 2; i < 24; i += 3)
        SEMICRF_CHECK_ARG(strides[i] < (1ll << 28), "axial_attention_bwd: token stride %lld must stay below 2^28 elements", strides[i]);
    if (!dq && !dk && !dv) return SEMICRF_OK;
    launch_axial_attention_bwd(q, k, v, out, dout, dq, dk, dv, n0, n1, Lq, Lk, H, d, strides, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_axial_attention_bwd");
    return SEMICRF_OK;
}

int semicrf_ffn_residual_supported(int D, int hidden) { return ffn::supported(D, hidden) ? 1 : 0; }

int semicrf_ffn_residual(const float* x, float* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                         int64_t out_stride_1, int D, int hidden, const float* W1, const float* b1, const float* W2, const float* b2,
                         const float* scale, float eps, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(ffn::supported(D, hidden),
                      "ffn_residual: D=%d hidden=%d is outside the supported set (D a multiple of 8 in [%d, %d]; hidden a multiple of 8 in "
                      "[%d, %d]): see semicrf_ffn_residual_supported", D, hidden, ffn::FFN_MIN_D, ffn::FFN_MAX_D, ffn::FFN_MIN_H, ffn::FFN_MAX_H);
    SEMICRF_CHECK_ARG(n0 >= 1 && n1 >= 1, "ffn_residual: n0=%lld n1=%lld must be >= 1", (long long)n0, (long long)n1);
    SEMICRF_CHECK_ARG(n0 < (1ll << 37) && n1 < (1ll << 37) && n0 * n1 < (1ll << 37), "ffn_residual: n0 * n1 = %lld * %lld must stay below 2^37",
                      (long long)n0, (long long)n1);
    SEMICRF_CHECK_ARG(x && out && W1 && b1 && W2 && b2 && scale, "ffn_residual: x/out/W1/b1/W2/b2/scale must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)W1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)b2 | (uintptr_t)scale) & 3) == 0,
                      "ffn_residual: every pointer must be 4-byte aligned");
    const long long st[4] = {n0 > 1 ? x_stride_0 : 0, n1 > 1 ? x_stride_1 : 0, n0 > 1 ? out_stride_0 : 0, n1 > 1 ? out_stride_1 : 0};
    for (int i = 0; i < 4; ++i)
        SEMICRF_CHECK_ARG(st[i] >= 0 && st[i] < (1ll << 40), "ffn_residual: stride %d = %lld must be in [0, 2^40)", i, st[i]);
    SEMICRF_CHECK_ARG((n0 == 1 || st[2] >= D) && (n1 == 1 || st[3] >= D), "ffn_residual: a row stride of `out` (%lld, %lld) is below D=%d", st[2],
                      st[3], D);
    // the element ranges the two views span (strides below 2^40, counts below 2^37: no overflow)
    const long long xext = (n0 - 1) * st[0] + (n1 - 1) * st[1] + D, oext = (n0 - 1) * st[2] + (n1 - 1) * st[3] + D;
    const uintptr_t xb = (uintptr_t)x, ob = (uintptr_t)out;
    SEMICRF_CHECK_ARG(xb + (uintptr_t)xext * 4 <= ob || ob + (uintptr_t)oext * 4 <= xb, "ffn_residual: `out` overlaps `x`");
    launch_ffn_residual(x, out, n0, n1, st[0], st[1], st[2], st[3], D, hidden, W1, b1, W2, b2, scale, eps, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_residual");
    return SEMICRF_OK;
}

// the checks the fp32 entry points share: sizes, pointers, the two views `in` (read) and `out` (written) -- `what` names the call
static int ffn_f32_check(const char* what, int64_t n0, int64_t n1, int D, int hidden, const long long st_in[2], const long long st_out[2])
{
    SEMICRF_CHECK_ARG(ffn::supported(D, hidden),
                      "%s: D=%d hidden=%d is outside the supported set (D a multiple of 8 in [%d, %d]; hidden a multiple of 8 in "
                      "[%d, %d]): see semicrf_ffn_residual_supported", what, D, hidden, ffn::FFN_MIN_D, ffn::FFN_MAX_D, ffn::FFN_MIN_H,
                      ffn::FFN_MAX_H);
    SEMICRF_CHECK_ARG(n0 >= 1 && n1 >= 1, "%s: n0=%lld n1=%lld must be >= 1", what, (long long)n0, (long long)n1);
    SEMICRF_CHECK_ARG(n0 < (1ll << 37) && n1 < (1ll << 37) && n0 * n1 < (1ll << 37), "%s: n0 * n1 = %lld * %lld must stay below 2^37", what,
                      (long long)n0, (long long)n1);
    for (int i = 0; i < 2; ++i)
        SEMICRF_CHECK_ARG(st_in[i] >= 0 && st_in[i] < (1ll << 40) && st_out[i] >= 0 && st_out[i] < (1ll << 40),
                          "%s: stride %lld / %lld must be in [0, 2^40)", what, st_in[i], st_out[i]);
    SEMICRF_CHECK_ARG((n0 == 1 || st_out[0] >= D) && (n1 == 1 || st_out[1] >= D), "%s: a row stride of the output view (%lld, %lld) is below D=%d",
                      what, st_out[0], st_out[1], D);
    return SEMICRF_OK;
}
static bool ffn_ranges_overlap(const void* a, long long na, const void* b, long long nb)     // element counts of fp32
{
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return !(pa + (uintptr_t)na * 4 <= pb || pb + (uintptr_t)nb * 4 <= pa);
}
static int ffn_p_check(const char* what, double p1, double p2)
{
    SEMICRF_CHECK_ARG(p1 >= 0.0 && p1 < 1.0 && p2 >= 0.0 && p2 < 1.0, "%s: dropout probabilities p_hidden=%g p_out=%g must lie in [0, 1)", what, p1,
                      p2);
    return SEMICRF_OK;
}

int semicrf_ffn_residual_train_fwd(const float* x, float* out, float* z, float* y, int64_t n0, int64_t n1, int64_t x_stride_0,
                                   int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const float* W1,
                                   const float* b1, const float* W2, const float* b2, const float* scale, float eps, uint64_t seed,
                                   double p_hidden, double p_out, semicrf_stream_t stream)
{
    const long long si[2] = {n0 > 1 ? x_stride_0 : 0, n1 > 1 ? x_stride_1 : 0}, so[2] = {n0 > 1 ? out_stride_0 : 0, n1 > 1 ? out_stride_1 : 0};
    if (const int rc = ffn_f32_check("ffn_residual_train_fwd", n0, n1, D, hidden, si, so)) return rc;
    if (const int rc = ffn_p_check("ffn_residual_train_fwd", p_hidden, p_out)) return rc;
    SEMICRF_CHECK_ARG(x && out && z && y && W1 && b1 && W2 && b2 && scale, "ffn_residual_train_fwd: x/out/z/y/W1/b1/W2/b2/scale must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)x | (uintptr_t)out | (uintptr_t)z | (uintptr_t)y | (uintptr_t)W1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)b2 |
                        (uintptr_t)scale) & 3) == 0, "ffn_residual_train_fwd: every pointer must be 4-byte aligned");
    const long long ntok = n0 * n1;
    const long long xext = (n0 - 1) * si[0] + (n1 - 1) * si[1] + D, oext = (n0 - 1) * so[0] + (n1 - 1) * so[1] + D;
    SEMICRF_CHECK_ARG(!ffn_ranges_overlap(x, xext, out, oext) && !ffn_ranges_overlap(x, xext, z, ntok * hidden) &&
                      !ffn_ranges_overlap(x, xext, y, ntok * D) && !ffn_ranges_overlap(out, oext, z, ntok * hidden) &&
                      !ffn_ranges_overlap(out, oext, y, ntok * D) && !ffn_ranges_overlap(z, ntok * hidden, y, ntok * D),
                      "ffn_residual_train_fwd: x, out, z and y must not overlap");
    launch_ffn_residual_train(x, out, n0, n1, si[0], si[1], so[0], so[1], D, hidden, W1, b1, W2, b2, scale, eps, seed, p_hidden, p_out, z, y,
                              (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_residual_train_fwd");
    return SEMICRF_OK;
}

int semicrf_ffn_residual_bwd_supported(int D, int hidden) { return ffn::supported(D, hidden) ? 1 : 0; }

size_t semicrf_ffn_residual_bwd_workspace_bytes(int64_t tokens, int D, int hidden)
{
    if (tokens < 1 || tokens >= (1ll << 37) || !ffn::supported(D, hidden)) return 0;
    return ffn_bwd_workspace_bytes(tokens, D, hidden);
}

int semicrf_ffn_residual_bwd(const float* dout, const float* x, const float* z, const float* y, int64_t n0, int64_t n1, int64_t dout_stride_0,
                             int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0, int64_t dx_stride_1, int D,
                             int hidden, const float* W1, const float* W2, const float* scale, float eps, uint64_t seed, double p_hidden,
                             double p_out, float* dx, float* dW1, float* db1, float* dW2, float* db2, float* dscale, void* ws, size_t ws_bytes,
                             semicrf_stream_t stream)
{
    const long long sg[2] = {n0 > 1 ? dout_stride_0 : 0, n1 > 1 ? dout_stride_1 : 0}, sx[2] = {n0 > 1 ? x_stride_0 : 0, n1 > 1 ? x_stride_1 : 0};
    const long long sd[2] = {n0 > 1 ? dx_stride_0 : 0, n1 > 1 ? dx_stride_1 : 0};
    if (const int rc = ffn_f32_check("ffn_residual_bwd", n0, n1, D, hidden, sg, sd)) return rc;
    if (const int rc = ffn_f32_check("ffn_residual_bwd", n0, n1, D, hidden, sx, sd)) return rc;
    if (const int rc = ffn_p_check("ffn_residual_bwd", p_hidden, p_out)) return rc;
    const long long ntok = n0 * n1;
    SEMICRF_CHECK_ARG(ntok <= 65535ll * SEMICRF_FFN_BWD_ROW_CHUNK, "ffn_residual_bwd: n0 * n1 = %lld: more than 65535 row chunks", ntok);
    SEMICRF_CHECK_ARG(dout && x && z && y && W1 && W2 && scale, "ffn_residual_bwd: dout/x/z/y/W1/W2/scale must be non-NULL");
    SEMICRF_CHECK_ARG(dx && dW1 && db1 && dW2 && db2 && dscale, "ffn_residual_bwd: dx/dW1/db1/dW2/db2/dscale must be non-NULL");
    SEMICRF_CHECK_ARG((((uintptr_t)dout | (uintptr_t)x | (uintptr_t)z | (uintptr_t)y | (uintptr_t)W1 | (uintptr_t)W2 | (uintptr_t)scale | (uintptr_t)dx |
                        (uintptr_t)dW1 | (uintptr_t)db1 | (uintptr_t)dW2 | (uintptr_t)db2 | (uintptr_t)dscale) & 3) == 0,
                      "ffn_residual_bwd: every pointer must be 4-byte aligned");
    const long long gext = (n0 - 1) * sg[0] + (n1 - 1) * sg[1] + D, xext = (n0 - 1) * sx[0] + (n1 - 1) * sx[1] + D;
    const long long dext = (n0 - 1) * sd[0] + (n1 - 1) * sd[1] + D;
    SEMICRF_CHECK_ARG(!ffn_ranges_overlap(dx, dext, dout, gext) && !ffn_ranges_overlap(dx, dext, x, xext) &&
                      !ffn_ranges_overlap(dx, dext, z, ntok * hidden) && !ffn_ranges_overlap(dx, dext, y, ntok * D),
                      "ffn_residual_bwd: `dx` overlaps dout, x, z or y");
    const size_t need = ffn_bwd_workspace_bytes(ntok, D, hidden);
    SEMICRF_CHECK_ARG(ws && ((uintptr_t)ws & 3) == 0, "ffn_residual_bwd: ws must be non-NULL and 4-byte aligned");
    if (ws_bytes < need) {
        set_error("workspace too small for ffn_residual_bwd: %zu bytes given, semicrf_ffn_residual_bwd_workspace_bytes says %zu", ws_bytes, need);
        return SEMICRF_EWORKSPACE;
    }
    launch_ffn_residual_bwd(dout, x, z, y, n0, n1, sg[0], sg[1], sx[0], sx[1], sd[0], sd[1], D, hidden, W1, W2, scale, eps, seed, p_hidden, p_out, dx,
                            dW1, db1, dW2, db2, dscale, (float*)ws, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_residual_bwd");
    return SEMICRF_OK;
}

int semicrf_ffn_dropout_mask(uint64_t seed, int64_t rows, int D, int hidden, double p_hidden, double p_out, unsigned char* mask_hidden,
                             unsigned char* mask_out, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(D >= 1 && D < (1 << 20) && hidden >= 1 && hidden < (1 << 20), "ffn_dropout_mask: D=%d hidden=%d out of range", D, hidden);
    SEMICRF_CHECK_ARG(rows >= 0 && rows < (1ll << 37) && (rows + 3) / 4 * ((long long)D + hidden) < (1ll << 38),
                      "ffn_dropout_mask: rows=%lld too large", (long long)rows);
    if (const int rc = ffn_p_check("ffn_dropout_mask", p_hidden, p_out)) return rc;
    if (rows == 0) return SEMICRF_OK;
    SEMICRF_CHECK_ARG(mask_hidden && mask_out, "ffn_dropout_mask: mask_hidden/mask_out must be non-NULL");
    launch_ffn_mask(seed, rows, D, hidden, p_hidden, p_out, mask_hidden, mask_out, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_dropout_mask");
    return SEMICRF_OK;
}

int semicrf_ffn_residual_bf16_supported(int D, int hidden) { return ffn::supported(D, hidden) ? 1 : 0; }
int semicrf_ffn_residual_bf16_mixed_supported(int D, int hidden) { return ffn::supported(D, hidden) ? 1 : 0; }

int semicrf_ffn_residual_bf16(const uint16_t* x, uint16_t* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                              int64_t out_stride_1, int D, int hidden, const uint16_t* W1, const uint16_t* b1, const uint16_t* W2,
                              const uint16_t* b2, const uint16_t* scale, float eps, semicrf_stream_t stream)
{
    long long st[4];
    const int rc = ffn_bf16_check<uint16_t>("ffn_residual_bf16", x, out, n0, n1, x_stride_0, x_stride_1, out_stride_0, out_stride_1, D, hidden, W1,
                                            b1, W2, b2, scale, st);
    if (rc != SEMICRF_OK) return rc;
    launch_ffn_residual_bf16(x, out, n0, n1, st[0], st[1], st[2], st[3], D, hidden, W1, b1, W2, b2, scale, eps, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_residual_bf16");
    return SEMICRF_OK;
}

int semicrf_ffn_residual_bf16_mixed(const float* x, float* out, int64_t n0, int64_t n1, int64_t x_stride_0, int64_t x_stride_1, int64_t out_stride_0,
                                    int64_t out_stride_1, int D, int hidden, const float* W1, const float* b1, const float* W2, const float* b2,
                                    const float* scale, float eps, semicrf_stream_t stream)
{
    long long st[4];
    const int rc = ffn_bf16_check<float>("ffn_residual_bf16_mixed", x, out, n0, n1, x_stride_0, x_stride_1, out_stride_0, out_stride_1, D, hidden,
                                         W1, b1, W2, b2, scale, st);
    if (rc != SEMICRF_OK) return rc;
    launch_ffn_residual_bf16_mixed(x, out, n0, n1, st[0], st[1], st[2], st[3], D, hidden, W1, b1, W2, b2, scale, eps, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_ffn_residual_bf16_mixed");
    return SEMICRF_OK;
}

int semicrf_ffn_residual_bf16_bwd_supported(int D, int hidden) { return ffn::supported(D, hidden) ? 1 : 0; }

size_t semicrf_ffn_residual_bf16_train_saved_bytes(int64_t tokens, int D, int hidden)
{
    if (tokens < 1 || tokens >= (1ll << 37) || !ffn::supported(D, hidden)) return 0;
    return ffn::train_saved_bytes(tokens, D, hidden);
}

size_t semicrf_ffn_residual_bf16_bwd_workspace_bytes(int64_t tokens, int D, int hidden)
{
    if (tokens < 1 || tokens >= (1ll << 37) || !ffn::supported(D, hidden)) return 0;
    return ffn_bf16_bwd_workspace_bytes(tokens, D, hidden);
}

int semicrf_ffn_residual_bf16_train_fwd(const uint16_t* x, uint16_t* out, void* saved, size_t saved_bytes, int64_t n0, int64_t n1, int64_t x_stride_0,
                                        int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const uint16_t* W1,
                                        const uint16_t* b1, const uint16_t* W2, const uint16_t* b2, const uint16_t* scale, float eps, uint64_t seed,
                                        double p_hidden, double p_out, semicrf_stream_t stream)
{
    return ffn_bf16_train_fwd_any<uint16_t>("ffn_residual_bf16_train_fwd", &launch_ffn_residual_bf16_train, x, out, saved, saved_bytes, n0, n1,
                                            x_stride_0, x_stride_1, out_stride_0, out_stride_1, D, hidden, W1, b1, W2, b2, scale, eps, seed, p_hidden,
                                            p_out, stream);
}

int semicrf_ffn_residual_bf16_mixed_train_fwd(const float* x, float* out, void* saved, size_t saved_bytes, int64_t n0, int64_t n1, int64_t x_stride_0,
                                              int64_t x_stride_1, int64_t out_stride_0, int64_t out_stride_1, int D, int hidden, const float* W1,
                                              const float* b1, const float* W2, const float* b2, const float* scale, float eps, uint64_t seed,
                                              double p_hidden, double p_out, semicrf_stream_t stream)
{
    return ffn_bf16_train_fwd_any<float>("ffn_residual_bf16_mixed_train_fwd", &launch_ffn_residual_bf16_mixed_train, x, out, saved, saved_bytes, n0, n1,
                                         x_stride_0, x_stride_1, out_stride_0, out_stride_1, D, hidden, W1, b1, W2, b2, scale, eps, seed, p_hidden, p_out,
                                         stream);
}

int semicrf_ffn_residual_bf16_bwd(const uint16_t* dout, const uint16_t* x, const void* saved, size_t saved_bytes, int64_t n0, int64_t n1,
                                  int64_t dout_stride_0, int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0,
                                  int64_t dx_stride_1, int D, int hidden, const uint16_t* W1, const uint16_t* W2, const uint16_t* scale, float eps,
                                  uint64_t seed, double p_hidden, double p_out, uint16_t* dx, uint16_t* dW1, uint16_t* db1, uint16_t* dW2, uint16_t* db2,
                                  uint16_t* dscale, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return ffn_bf16_bwd_any<uint16_t>("ffn_residual_bf16_bwd", &launch_ffn_residual_bf16_bwd, dout, x, saved, saved_bytes, n0, n1, dout_stride_0,
                                      dout_stride_1, x_stride_0, x_stride_1, dx_stride_0, dx_stride_1, D, hidden, W1, W2, scale, eps, seed, p_hidden,
                                      p_out, dx, dW1, db1, dW2, db2, dscale, ws, ws_bytes, stream);
}

int semicrf_ffn_residual_bf16_mixed_bwd(const float* dout, const float* x, const void* saved, size_t saved_bytes, int64_t n0, int64_t n1,
                                        int64_t dout_stride_0, int64_t dout_stride_1, int64_t x_stride_0, int64_t x_stride_1, int64_t dx_stride_0,
                                        int64_t dx_stride_1, int D, int hidden, const float* W1, const float* W2, const float* scale, float eps,
                                        uint64_t seed, double p_hidden, double p_out, float* dx, float* dW1, float* db1, float* dW2, float* db2,
                                        float* dscale, void* ws, size_t ws_bytes, semicrf_stream_t stream)
{
    return ffn_bf16_bwd_any<float>("ffn_residual_bf16_mixed_bwd", &launch_ffn_residual_bf16_mixed_bwd, dout, x, saved, saved_bytes, n0, n1, dout_stride_0,
                                   dout_stride_1, x_stride_0, x_stride_1, dx_stride_0, dx_stride_1, D, hidden, W1, W2, scale, eps, seed, p_hidden, p_out,
                                   dx, dW1, db1, dW2, db2, dscale, ws, ws_bytes, stream);
}

int semicrf_log_mel_supported(int W, int nWin, int C, int nMel, int max_len, int total)
{
    return logmel::supported(W, nWin, C, nMel, max_len, total) ? 1 : 0;
}

int semicrf_log_mel(const float* frames, int64_t stride_n, int64_t stride_c, int64_t stride_frame, int N, int C, int nFrame, int W,
                    const float* windows, int nWin, const float* twiddles, const int32_t* fb_start, const int32_t* fb_len, const int32_t* fb_off,
                    const float* fb_val, int nMel, int total, const float* shift, const float* denom, int log_flag, float eps, int to_mono,
                    float* out, semicrf_stream_t stream)
{
    SEMICRF_CHECK_ARG(logmel::supported(W, nWin, C, nMel, 0, total),
                      "log_mel: W=%d nWin=%d C=%d nMel=%d total=%d is outside the supported set (W a power of two in [256, 4096]; nWin in [1, %d]; "
                      "C in [1, %d]; nMel in [1, %d]; total support in [0, %d]): see semicrf_log_mel_supported", W, nWin, C, nMel, total,
                      logmel::LM_MAX_WIN, logmel::LM_MAX_C, logmel::LM_MAX_MEL, logmel::LM_MAX_TOTAL);
    SEMICRF_CHECK_ARG(N >= 1 && nFrame >= 1 && (long long)N * nFrame < (1ll << 31), "log_mel: N=%d nFrame=%d must be >= 1 and N nFrame < 2^31", N, nFrame);
    SEMICRF_CHECK_ARG(frames && windows && twiddles && fb_start && fb_len && fb_off && out && (fb_val || total == 0),
                      "log_mel: frames/windows/twiddles/fb_start/fb_len/fb_off/fb_val/out must be non-NULL");
    SEMICRF_CHECK_ARG((shift == nullptr) == (denom == nullptr), "log_mel: shift and denom come together or not at all");
    SEMICRF_CHECK_ARG((((uintptr_t)frames | (uintptr_t)windows | (uintptr_t)twiddles | (uintptr_t)fb_start | (uintptr_t)fb_len | (uintptr_t)fb_off |
                        (uintptr_t)fb_val | (uintptr_t)shift | (uintptr_t)denom | (uintptr_t)out) & 3) == 0,
                      "log_mel: every pointer must be 4-byte aligned");
    const long long st[3] = {N > 1 ? stride_n : 0, C > 1 ? stride_c : 0, nFrame > 1 ? stride_frame : 0};
    for (int i = 0; i < 3; ++i)
        SEMICRF_CHECK_ARG(st[i] >= 0 && st[i] < (1ll << 40), "log_mel: stride %d = %lld must be in [0, 2^40)", i, st[i]);
    SEMICRF_CHECK_ARG(!log_flag || eps > 0.0f, "log_mel: eps=%g must be positive for the log compression", (double)eps);
    // the element ranges the input view and the output span (strides below 2^40, counts below 2^31: no overflow)
    const long long fext = (N - 1) * st[0] + (C - 1) * st[1] + (nFrame - 1) * st[2] + W;
    const long long oext = (long long)N * (to_mono ? 1 : C) * nFrame * nMel * nWin;
    const uintptr_t fb = (uintptr_t)frames, ob = (uintptr_t)out;
    SEMICRF_CHECK_ARG(fb + (uintptr_t)fext * 4 <= ob || ob + (uintptr_t)oext * 4 <= fb, "log_mel: `out` overlaps `frames`");
    launch_log_mel(frames, st[0], st[1], st[2], N, C, nFrame, W, windows, nWin, twiddles, fb_start, fb_len, fb_off, fb_val, nMel, total, shift, denom,
                   log_flag ? 1 : 0, eps, to_mono ? 1 : 0, out, (hipStream_t)stream);
    SEMICRF_CHECK_LAUNCH("semicrf_log_mel");
    return SEMICRF_OK;
}

}  // extern "C"
