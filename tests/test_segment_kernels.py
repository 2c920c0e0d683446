"""The kernels between `decode` and the note list, at their edges: `attr_gather.hip` (`interval_features_kernel`,
`interval_features_bwd_kernel`) and `segment.hip` (`onset_count_kernel`, `offsets_scan_kernel`, `onset_pack_kernel`,
`segment_events_kernel`), called through `_lib.ops()` so that strides, `cap` and `K` are the test's, and through
`transkun_amd.attributes` where the wrapper is the subject.

References are numpy / plain Python written here, plus `oracle.segment_events` (pinned to the reference's loop by the goldens);
none of them calls the library.  Inputs are `synth.hash_normal` and `gen_lists`, a seeded pure-Python generator of per-chain
interval lists.  `test_inputs_bite` (no GPU) proves on the references alone that the lists and event inputs contain what the
device tests rely on.

The backward's bound is derived, not measured.  An element of `dctx` is the fp32 sum, by atomics in no fixed order, of n
contributions `g + g_ab * ctx`.  One contribution carries at most two roundings (one if contracted), error <= 2u(|g| + |g_ab*ctx|)
with u = 2**-24; the first add into the zeroed buffer is exact and each of the other n - 1 rounds a partial sum of magnitude
<= A(1 + O(nu)), A the sum of |g| + |g_ab*ctx| over the contributions.  Together (n + 1) u A to first order; the tests allow
2 (n + 1) u A per element and exact zeros where n == 0.

Untested: interval counts K >= 2**30, where `2 * i` overflows an `int` in these kernels; not reachable at test sizes.
"""
import functools

import numpy as np
import pytest
import torch

SENT_F = -777.0
SENT_I = -7777
GUARD = 8
FRAME_DUR = 1024 / 44100
U = 2.0 ** -24


# ---- seeded pure-Python list generator -----------------------------------------------------------------------------

_M64 = (1 << 64) - 1


class Rng:
    """splitmix64"""

    def __init__(self, seed):
        self.s = (seed * 0x9E3779B97F4A7C15 + 0x1234567) & _M64

    def u64(self):
        self.s = (self.s + 0x9E3779B97F4A7C15) & _M64
        z = self.s
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)

    def below(self, n):
        return self.u64() % n

    def unit(self):
        return (self.u64() >> 11) * (1.0 / (1 << 53))

    def chance(self, p):
        return self.unit() < p


def gen_lists(C, T, seed, p_empty=0.2, head=0, mid=None, tail=0, p_single=0.3, p_repeat=0.5, p_touch=0.4, p_last=0.1, p_zero=0.3,
              p_start_last=0.0, p_late=0.0, p_stop=0.0, max_len=6, gap=4):
    """Per-chain lists ascending in begin, every begin >= the previous end (what decode emits).  Rates: p_empty a chain is empty
    (besides the forced runs of `head` / `tail` chains and `mid` = (first, length)); p_single a singleton (t, t) at the current
    frame, p_repeat that an interval (t, e) follows it at the same begin; p_touch the next begin is the last end; p_last an interval
    ends on frame T - 1; p_zero the chain begins at frame 0, p_start_last at frame T - 1, p_late at any frame
    (otherwise within `gap` frames of 0); p_stop the chain ends after an entry."""
    rng = Rng(seed)
    out = []
    for c in range(C):
        cur = []
        forced = c < head or c >= C - tail or (mid is not None and mid[0] <= c < mid[0] + mid[1])
        if forced or rng.chance(p_empty):
            out.append(cur)
            continue
        u = rng.unit()
        t = 0 if u < p_zero else T - 1 if u < p_zero + p_start_last else rng.below(T) if u < p_zero + p_start_last + p_late else 1 + rng.below(gap)
        while t < T:
            if rng.chance(p_single):
                cur.append((t, t))
                if t == T - 1 or not rng.chance(p_repeat):
                    if rng.chance(p_stop):
                        break
                    t += 1 + rng.below(gap)
                    continue
            if t >= T - 1:
                break
            e = T - 1 if rng.chance(p_last) else min(T - 1, t + 1 + rng.below(max_len))
            cur.append((t, e))
            if rng.chance(p_stop):
                break
            t = e if rng.chance(p_touch) else e + 1 + rng.below(gap)
        out.append(cur)
    return out


def truncate(lists, K):
    out, left = [], K
    for l in lists:
        out.append(l[:left])
        left -= len(out[-1])
    assert left == 0
    return out


def pack(lists):
    flat = [p for l in lists for p in l]
    pairs = np.asarray(flat, np.int32).reshape(-1, 2)
    offsets = np.zeros(len(lists) + 1, np.int32)
    offsets[1:] = np.cumsum([len(l) for l in lists])
    return pairs, offsets


def list_facts(lists, T):
    """what a list set contains (and that it is well formed)"""
    f = dict(repeat=0, touch=0, last=0, zero=0, single=0, K=sum(len(l) for l in lists))
    for l in lists:
        for j, (b, e) in enumerate(l):
            assert 0 <= b <= e < T
            f["single"] += b == e
            f["last"] += e == T - 1 and b < e
            f["zero"] += b == 0
            if j:
                pb, pe = l[j - 1]
                assert b >= pe and b >= pb and (pb, pe) != (b, e)
                f["repeat"] += pb == pe == b and e > b
                f["touch"] += pb < pe == b and e > b
    ne = [i for i, l in enumerate(lists) if l]
    f["nonempty"] = len(ne)
    f["empty_head"] = ne[0] if ne else len(lists)
    f["empty_tail"] = len(lists) - 1 - ne[-1] if ne else len(lists)
    f["empty_mid"] = max([b - a - 1 for a, b in zip(ne, ne[1:])], default=0)
    return f


# ---- the list sets --------------------------------------------------------------------------------------------------

GATHER_SETS = {
    # name: (C, nSym, T, generator arguments)
    "C1": (1, 1, 2, dict(seed=1, p_empty=0.0, p_zero=1.0, p_single=1.0, p_repeat=1.0, p_touch=1.0)),
    "C7": (7, 7, 13, dict(seed=2, p_empty=0.0, head=1, mid=(3, 2), tail=1, p_touch=0.6, gap=2)),
    "C24": (24, 8, 33, dict(seed=3, p_empty=0.15, head=2, mid=(9, 3), tail=2, p_touch=0.5)),
    "C270": (270, 90, 33, dict(seed=4, p_empty=0.3, head=3, mid=(100, 40), tail=5)),
    "C1000": (1000, 8, 97, dict(seed=5, p_empty=0.5, head=10, mid=(400, 130), tail=20)),
}
ONSET_T = 40
ONSET_B = (1, 46, 255, 256, 257, 513, 700)
ONSET_RATES = dict(p_empty=0.15, p_single=0.5, p_repeat=0.7, p_touch=0.5, p_zero=0.3, p_start_last=0.15, p_late=0.3, p_stop=0.25, p_last=0.15)
EVENT_T = 40
EVENT_LAST = EVENT_T - 3                     # lastFrameIdx: the end of some intervals, above most
EVENT_STEPS = (5, 30)                        # stepFrames below and above a typical lastP
EVENT_CASES = ((1, 1), (5, 5), (135, 5), (360, 90), (258, 1))
EVENT_RATES = dict(p_empty=0.15, p_single=0.4, p_repeat=0.6, p_touch=0.5, p_zero=0.6, p_stop=0.12, p_last=0.25)


@functools.lru_cache(maxsize=None)
def gather_set(name):
    C, nSym, T, kw = GATHER_SETS[name]
    return gen_lists(C, T, **kw)


@functools.lru_cache(maxsize=None)
def onset_set(B):
    head, tail = (2, 3) if B >= 46 else (0, 0)
    mid = (B // 2, 5) if B >= 46 else None
    rates = dict(ONSET_RATES, p_empty=ONSET_RATES["p_empty"] if B > 1 else 0.0, p_stop=ONSET_RATES["p_stop"] if B > 1 else 0.0)
    return gen_lists(B, ONSET_T, seed=100 + B, head=head, mid=mid, tail=tail, **rates)


def contended_lists():
    """not paths (the ABI takes any pairs): 64 intervals of chain 0 share begin frame 5, 64 of chain 1 share end frame 75, and
    40 singletons of chain 2 hit frame 9 twice each"""
    return [[(5, 6 + j) for j in range(64)], [(j, 75) for j in range(64)], [(9, 9)] * 40], 80


@functools.lru_cache(maxsize=None)
def event_inputs(B, nSym):
    """(lists, ofValue [K,2] float32, ofPresence [K,2] bool, beginTime [B / nSym])"""
    lists = gen_lists(B, EVENT_T, seed=200 + B, p_empty=EVENT_RATES["p_empty"] if B > 1 else 0.0,
                      **{k: v for k, v in EVENT_RATES.items() if k != "p_empty"})
    rng = Rng(300 + B)

    def draw():
        u = rng.unit()
        return -0.5 if u < 0.25 else 0.5 if u < 0.5 else rng.unit() - 0.5

    ofv, ofp = [], []
    for l in lists:
        k0 = len(ofv)
        for (b, e) in l:
            v = [draw(), draw()]
            if b == e and rng.chance(0.6):
                v = [0.5, -0.5]                                  # end < start + 1e-8
            ofv.append(v)
            ofp.append([rng.chance(0.5), rng.chance(0.5)])
        for j in range(1, len(l)):
            if l[j][0] == l[j - 1][1] and rng.chance(0.6):       # touching: the next start falls before lastEnd
                ofv[k0 + j - 1][1] = 0.5
                ofv[k0 + j][0] = -0.5
    nseg = B // nSym
    begin = [s * 26624 / 44100 - 0.6 for s in range(nseg)]      # segment 0 negative like the reference's -pad_t, the others non-dyadic
    return lists, np.asarray(ofv, np.float32).reshape(-1, 2), np.asarray(ofp, bool).reshape(-1, 2), begin


def event_branches(lists, nSym, ofValue, ofPresence, lastFrameIdx, frameDur, beginTime, stepFrames):
    """which branches of the event recurrence (ModelTransformer.py:684-718, transcribe :789-800) the inputs take"""
    n = 0
    cnt = dict.fromkeys(("start_clamped", "end_raised", "s2_clamped", "en2_raised", "onset_presence_only", "onset_b_only",
                         "offset_presence_only", "offset_e_only", "offset_false", "next_clamped"), 0)
    for c, cur in enumerate(lists):
        bt = beginTime[c // nSym]
        lastEnd, lastP = 0.0, 0
        for (b, e) in cur:
            start = (b + float(ofValue[n][0])) * frameDur
            end = (e + float(ofValue[n][1])) * frameDur
            p0, p1 = bool(ofPresence[n][0]), bool(ofPresence[n][1])
            cnt["onset_presence_only"] += b == 0 and p0
            cnt["onset_b_only"] += b > 0 and not p0
            cnt["offset_presence_only"] += e >= lastFrameIdx and p1
            cnt["offset_e_only"] += e < lastFrameIdx and not p1
            cnt["offset_false"] += e >= lastFrameIdx and not p1 and lastP > 0
            cnt["start_clamped"] += start < lastEnd
            start = max(start, lastEnd)
            cnt["end_raised"] += end < start + 1e-8
            end = max(end, start + 1e-8)
            lastEnd = end
            if e < lastFrameIdx or p1:
                lastP = e
            cnt["s2_clamped"] += start + bt < 0
            cnt["en2_raised"] += end + bt < max(start + bt, 0)
            n += 1
        cnt["next_clamped"] += bool(cur) and lastP - stepFrames < 0
    return cnt


# ---- references ----------------------------------------------------------------------------------------------------

def chain_index(offsets):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))


def gather_ref(ctx, pairs, offsets, nSym):
    """ctx numpy float32 [C, T, D] -> (out [K, 3D] float32 with the product rounded once in float32, symIdx, scatterIdx)"""
    c = chain_index(offsets)
    a, b = ctx[c, pairs[:, 0]], ctx[c, pairs[:, 1]]
    assert a.dtype == np.float32
    return np.concatenate([a, b, a * b], axis=1), (c % nSym).astype(np.int64), c.astype(np.int64)


def gather_bwd_ref(ctx, pairs, offsets, gout):
    """float64 scatter-add; returns (dctx [C,T,D], A [C,T,D] = sum of |g| + |g_ab * ctx| per element, n [C,T] contributions)"""
    C, T, D = ctx.shape
    x = ctx.astype(np.float64)
    g = gout.astype(np.float64)
    ga, gb, gab = g[:, :D], g[:, D:2 * D], g[:, 2 * D:]
    c = chain_index(offsets)
    b, e = pairs[:, 0], pairs[:, 1]
    ref, A, n = np.zeros((C, T, D)), np.zeros((C, T, D)), np.zeros((C, T), np.int64)
    np.add.at(ref, (c, b), ga + gab * x[c, e]); np.add.at(A, (c, b), np.abs(ga) + np.abs(gab * x[c, e])); np.add.at(n, (c, b), 1)
    np.add.at(ref, (c, e), gb + gab * x[c, b]); np.add.at(A, (c, e), np.abs(gb) + np.abs(gab * x[c, b])); np.add.at(n, (c, e), 1)
    return ref, A, n


def bwd_bound(A, n):
    return 2.0 * (n[:, :, None] + 1) * U * A


def check_bwd(got, ref, A, n):
    got = np.asarray(got)
    assert got.dtype == np.float32
    untouched = np.broadcast_to((n == 0)[:, :, None], got.shape)
    assert np.all(got[untouched] == 0.0)
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > bwd_bound(A, n)
    assert not bad.any(), (int(bad.sum()), float((err / np.maximum(bwd_bound(A, n), 1e-300))[bad].max()))


def bf16_ulp(x):
    """spacing of bfloat16 (8 significant bits) at |x|"""
    _, e = np.frexp(np.abs(x))
    return np.ldexp(1.0, e - 8)


def ctx_of(C, T, D, seed, storage_D=None, col0=0):
    """ctx [C, T, D] float32 on the CPU as columns [col0 : col0 + D] of a [C, T, storage_D] tensor (contiguous if not given)"""
    from transkun_amd import synth
    S = storage_D or D
    full = synth.hash_normal(C * T * S, seed).view(C, T, S)
    return full[:, :, col0:col0 + D]


CTX_LAYOUTS = {
    # name: (storage row length or None, first column)        for D = 64
    "contiguous": (None, 0),
    "base_off1_ld68": (68, 1),       # base 4 bytes off a 16-byte boundary, ldc % 4 == 0
    "ld67": (67, 0),                 # ldc % 4 != 0
}


def wrapper_case(kind):
    """inputs of the two `attribute_input_packed` tests on the CPU: (ctxBatch [N,SYM,T,D], lists, gout [K,3D])"""
    from transkun_amd import synth
    if kind == "bf16":
        N, SYM, T, D = 2, 3, 12, 8
        x = synth.hash_normal(N * SYM * T * D, 61).view(N, SYM, T, D).bfloat16()
    else:
        N, SYM, T, D = 2, 5, 20, 64
        x = synth.hash_normal(N * T * SYM * D, 62).view(N, T, SYM, D).permute(0, 2, 1, 3)      # [N, T, SYM, D] storage
    lists = gen_lists(N * SYM, T, seed=63 if kind == "bf16" else 64, p_empty=0.2, p_touch=0.5)
    K = sum(len(l) for l in lists)
    gout = synth.hash_normal(K * 3 * D, 65).view(K, 3 * D)
    return x, lists, gout


# ---- 5. the inputs are proven to bite (no GPU) ----------------------------------------------------------------------

def test_inputs_bite():
    """Conditions on the generators' outputs, evaluated with the references alone."""
    for name, (C, nSym, T, _) in GATHER_SETS.items():
        f = list_facts(gather_set(name), T)
        assert len(gather_set(name)) == C and C % nSym == 0
        assert f["repeat"] >= 1 and f["single"] >= 1, (name, f)
        if C == 1:
            assert f["K"] >= 2 and f["zero"] >= 1 and f["last"] >= 1
            continue
        assert f["touch"] >= 1 and f["zero"] >= 1 and f["last"] >= 1, (name, f)
        assert f["empty_head"] >= 1 and f["empty_tail"] >= 1 and f["empty_mid"] >= 2, (name, f)      # runs at start, middle, end
    assert list_facts(gather_set("C7"), 13)["K"] >= 9                                               # the K cases cut this set
    assert list_facts(gather_set("C24"), 33)["K"] >= 40
    assert list_facts(gather_set("C1000"), 97)["nonempty"] <= 500
    assert list_facts(gather_set("C270"), 33)["empty_mid"] >= 40

    T = ONSET_T
    for B in ONSET_B:
        lists = onset_set(B)
        f = list_facts(lists, T)
        assert len(lists) == B and f["K"] >= 1
        if B < 46:
            continue
        assert f["repeat"] >= B // 8 and f["touch"] >= 1, (B, f)                                     # many repeated begins
        assert f["empty_head"] >= 2 and f["empty_tail"] >= 3 and f["empty_mid"] >= 5, (B, f)
        for bound in (1, T // 2, T - 1):
            kept = [sum(p[0] < bound for p in l) for l in lists if l]
            size = [len(l) for l in lists if l]
            assert any(k == s for k, s in zip(kept, size)), (B, bound, "no chain fully kept")
            assert any(k == 0 for k in kept), (B, bound, "no chain fully dropped")
            assert any(0 < k < s for k, s in zip(kept, size)), (B, bound, "no chain cut in the middle")
        assert sum(sum(p[0] < T // 2 for p in l) for l in lists) >= 4                                # room for cap = kept - 3

    total = {}
    for (B, nSym) in EVENT_CASES:
        lists, ofv, ofp, begin = event_inputs(B, nSym)
        list_facts(lists, EVENT_T)
        assert len(ofv) == sum(len(l) for l in lists) >= 1 and len(begin) == B // nSym
        assert begin[0] < 0 and len(set(begin)) == len(begin)
        assert np.all(np.abs(ofv) <= 0.5)
        if B > 1:
            assert any(not l for l in lists)
        for step in EVENT_STEPS:
            cnt = event_branches(lists, nSym, ofv, ofp, EVENT_LAST, FRAME_DUR, begin, step)
            if B >= 135:                                   # the small cases cannot hold five of everything
                seg0 = ("s2_clamped", "en2_raised")        # only segment 0 begins before 0: nSym chains
                assert min(v for k, v in cnt.items() if k not in seg0) >= 5, (B, step, cnt)
                assert min(cnt[k] for k in seg0) >= (5 if nSym >= 5 else 1), (B, step, cnt)
            for k, v in cnt.items():
                total[(k, step)] = total.get((k, step), 0) + v
    assert min(total.values()) >= 5, total
    lastPs = [max([e for (b, e) in l] or [0]) for (B, nSym) in EVENT_CASES for l in event_inputs(B, nSym)[0] if l]
    assert sum(p < EVENT_STEPS[1] for p in lastPs) >= 5 and sum(p > EVENT_STEPS[0] for p in lastPs) >= 5

    lists, T = contended_lists()
    pairs, offsets = pack(lists)
    ctx = ctx_of(3, T, 6, 70).numpy()
    gout = ctx_of(1, len(pairs), 18, 71).numpy()[0]
    _, _, n = gather_bwd_ref(ctx, pairs, offsets, gout)
    assert n.max() >= 64 and n[0, 5] == 64 and n[1, 75] == 64 and n[2, 9] == 80

    # bfloat16 through the wrapper: where the derived fp32 bound is at most half a bf16 step of the rounded reference, the cast
    # of any fp32 value within the bound lands within one bf16 step of it (rounding is monotone)
    x, lists, gout = wrapper_case("bf16")
    N, SYM, T, D = x.shape
    pairs, offsets = pack(lists)
    ref, A, n = gather_bwd_ref(x.float().numpy().reshape(N * SYM, T, D), pairs, offsets, gout.numpy())
    ref_bf = torch.from_numpy(ref).float().bfloat16().double().numpy()
    hit = np.broadcast_to((n > 0)[:, :, None], ref.shape)
    assert hit.sum() >= 100 and (n >= 2).any()
    assert np.all(bwd_bound(A, n)[hit] <= 0.5 * bf16_ulp(ref_bf[hit]))


# ---- device side ---------------------------------------------------------------------------------------------------

def run_gather(gpu, ctx, pairs_h, offsets_h, K, nSym, out_misaligned=False):
    """ctx: GPU float32 [C, T, D] view with unit last stride.  Returns numpy (out, symIdx, scatterIdx); checks the guard rows."""
    from transkun_amd import _lib
    C, T, D = ctx.shape
    assert ctx.stride(2) == 1 and ctx.stride(0) == T * ctx.stride(1)
    lead = 1 if out_misaligned else 0
    big = torch.full((lead + (K + GUARD) * 3 * D,), SENT_F, dtype=torch.float32, device=gpu)
    out = big[lead:lead + K * 3 * D].view(K, 3 * D)
    assert (out.data_ptr() % 16 != 0) == out_misaligned
    sym = torch.full((K + GUARD,), SENT_I, dtype=torch.int64, device=gpu)
    sc = torch.full((K + GUARD,), SENT_I, dtype=torch.int64, device=gpu)
    pairs = torch.from_numpy(pairs_h).to(gpu)
    offsets = torch.from_numpy(offsets_h).to(gpu)
    _lib.ops().interval_features_gather(ctx, C, T, D, ctx.stride(1), pairs, K, offsets, nSym, out, sym[:K], sc[:K])
    assert torch.all(big[:lead] == SENT_F) and torch.all(big[lead + K * 3 * D:] == SENT_F)
    assert torch.all(sym[K:] == SENT_I) and torch.all(sc[K:] == SENT_I)
    return out.cpu().numpy(), sym[:K].cpu().numpy(), sc[:K].cpu().numpy()


def check_gather(gpu, ctx_h, lists, nSym, **kw):
    pairs, offsets = pack(lists)
    K = len(pairs)
    want, wsym, wsc = gather_ref(ctx_h.numpy(), pairs, offsets, nSym)
    out, sym, sc = run_gather(gpu, ctx_h.to(gpu) if ctx_h.is_contiguous() else to_gpu_view(ctx_h, gpu), pairs, offsets, K, nSym, **kw)
    assert np.array_equal(out, want)
    assert np.array_equal(sym, wsym) and np.array_equal(sc, wsc)
    assert np.array_equal(sym, sc % nSym) and np.all(np.diff(sc) >= 0)
    return out


def to_gpu_view(view_h, gpu):
    """the same view of a copy of the whole storage on the GPU"""
    base = view_h._base if view_h._base is not None else view_h
    while base._base is not None:
        base = base._base
    g = base.to(gpu)
    return torch.as_strided(g, view_h.shape, view_h.stride(), view_h.storage_offset())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [4, 64, 256, 260, 512, 1, 6, 130])
def test_gather_forward_widths(gpu, D):
    """vector path (D % 4 == 0; 260 and 512 take the loop's second trip) and scalar path (D = 1, 6, 130), bit for bit"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C24"]
    check_gather(gpu, ctx_of(C, T, D, 10 + D), gather_set("C24"), nSym)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["base_off1_ld68", "ld67", "out_misaligned"])
def test_gather_forward_scalar_fallback_layouts(gpu, layout):
    """D = 64 forced onto the scalar path by the base address, by the row stride or by `out`; same bits as the vector path"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C24"]
    S, col0 = CTX_LAYOUTS.get(layout, (None, 0))
    view = ctx_of(C, T, 64, 20, S, col0)
    if layout == "base_off1_ld68":
        assert view.storage_offset() == 1 and view.stride(1) % 4 == 0
    if layout == "ld67":
        assert view.storage_offset() == 0 and view.stride(1) % 4 != 0
    got = check_gather(gpu, view, gather_set("C24"), nSym, out_misaligned=layout == "out_misaligned")
    same = check_gather(gpu, view.contiguous(), gather_set("C24"), nSym)
    assert np.array_equal(got, same)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 6])
@pytest.mark.parametrize("K", [1, 3, 4, 5, 9])
def test_gather_forward_interval_counts(gpu, K, D):
    """K % 4 != 0 leaves waves of the last block idle; cutting the lists leaves a run of empty chains at the end"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C7"]
    check_gather(gpu, ctx_of(C, T, D, 30 + D), truncate(gather_set("C7"), K), nSym)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_gather_forward_no_intervals(gpu):
    """K = 0 returns success and writes nothing"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C7"]
    pairs, offsets = pack(gather_set("C7"))
    out, sym, sc = run_gather(gpu, ctx_of(C, T, 64, 40).to(gpu), pairs, np.zeros_like(offsets), 0, nSym)
    assert out.shape == (0, 192) and len(sym) == 0 and len(sc) == 0              # run_gather checked the sentinels behind
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["C1", "C7", "C270", "C1000"])
def test_gather_forward_chain_counts(gpu, name):
    """the binary search of `chain_of_interval` over runs of empty chains at the start, in the middle and at the end"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS[name]
    check_gather(gpu, ctx_of(C, T, 64, 50 + C), gather_set(name), nSym)
    assert _lib.device_status() == 0


def run_gather_bwd(gpu, ctx, pairs_h, offsets_h, gout_h, lddc=None):
    """returns dctx [C, T, D] numpy; with `lddc` the gradient is columns [0:D] of a [C, T, lddc] buffer whose other columns stay 0"""
    from transkun_amd import _lib
    C, T, D = ctx.shape
    K = len(pairs_h)
    big = torch.zeros(C, T, lddc or D, dtype=torch.float32, device=gpu)
    dctx = big[:, :, :D]
    _lib.ops().interval_features_gather_bwd(torch.from_numpy(gout_h).to(gpu), ctx, C, T, D, ctx.stride(1), torch.from_numpy(pairs_h).to(gpu),
                                            K, torch.from_numpy(offsets_h).to(gpu), dctx, dctx.stride(1))
    assert torch.all(big[:, :, D:] == 0.0)
    return dctx.cpu().numpy()


def check_gather_bwd(gpu, view_h, lists, seed, lddc=None):
    from transkun_amd import synth
    C, T, D = view_h.shape
    pairs, offsets = pack(lists)
    gout = synth.hash_normal(len(pairs) * 3 * D, seed).view(-1, 3 * D).numpy()
    ref, A, n = gather_bwd_ref(view_h.numpy(), pairs, offsets, gout)
    got = run_gather_bwd(gpu, view_h.to(gpu) if view_h.is_contiguous() else to_gpu_view(view_h, gpu), pairs, offsets, gout, lddc)
    check_bwd(got, ref, A, n)
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("D", [6, 64, 260])
def test_gather_backward_paths(gpu, D):
    """path-like lists: singletons add twice into one address, touching intervals share a frame"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C24"]
    n = check_gather_bwd(gpu, ctx_of(C, T, D, 80 + D), gather_set("C24"), 90 + D)
    assert n.max() >= 2
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("D", [6, 64])
def test_gather_backward_contended(gpu, D):
    """64 intervals of one chain on one begin frame, 64 on one end frame, 40 singletons on one frame: the atomics"""
    from transkun_amd import _lib
    lists, T = contended_lists()
    n = check_gather_bwd(gpu, ctx_of(3, T, D, 100 + D), lists, 110 + D)
    assert n.max() >= 64
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout,lddc", [("base_off1_ld68", 72), ("ld67", 65), ("contiguous", 67)])
def test_gather_backward_strided(gpu, layout, lddc):
    """strided `ctx` and `dctx` with lddc != ldc; the columns of the gradient buffer beyond D stay zero"""
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C24"]
    S, col0 = CTX_LAYOUTS[layout]
    view = ctx_of(C, T, 64, 20, S, col0)
    assert view.stride(1) != lddc
    check_gather_bwd(gpu, view, gather_set("C24"), 120, lddc)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 5])
def test_gather_backward_interval_counts(gpu, K):
    from transkun_amd import _lib
    C, nSym, T, _ = GATHER_SETS["C7"]
    check_gather_bwd(gpu, ctx_of(C, T, 64, 130), truncate(gather_set("C7"), K), 131 + K)
    assert _lib.device_status() == 0


def _capture_fp32_grad(out):
    """hook the dtype-cast node behind `out` in the autograd graph: its incoming gradient is the fp32 dctx before the cast"""
    seen, todo, box = set(), [out.grad_fn], []
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        if node.name().startswith("ToCopyBackward"):
            node.register_hook(lambda gin, gout: box.append(gout[0].detach().clone()))
            return box
        todo.extend(f for f, _ in node.next_functions)
    raise AssertionError("no dtype cast between the input and the gather")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bf16", "permuted"])
def test_attribute_input_packed_wrapper(gpu, kind):
    """`attributes.attribute_input_packed` on a bfloat16 ctx and on a permuted [N, T, SYM, D] storage: forward bit-identical to the
    call on `.float().contiguous()` and to numpy; the gradient arrives with the input's dtype and shape, within the derived bound in
    fp32 (for bfloat16: before the cast) and, cast, within one bfloat16 step of the rounded float64 reference."""
    from transkun_amd import _lib, attributes
    x_h, lists, gout_h = wrapper_case(kind)
    N, SYM, T, D = x_h.shape
    pairs_h, offsets_h = pack(lists)
    K = len(pairs_h)
    pairs, offsets = torch.from_numpy(pairs_h).to(gpu), torch.from_numpy(offsets_h).to(gpu)
    x = (x_h.to(gpu) if kind == "bf16" else to_gpu_view(x_h, gpu)).requires_grad_()
    assert x.dtype == x_h.dtype and x.stride() == x_h.stride() and (kind == "bf16" or not x.is_contiguous())

    out, sym, sc = attributes.attribute_input_packed(x, pairs, offsets, K)
    plain, sym2, sc2 = attributes.attribute_input_packed(x.detach().float().contiguous(), pairs, offsets)      # K from offsets[-1]
    flat = x_h.detach().float().contiguous().view(N * SYM, T, D).numpy()
    want, wsym, wsc = gather_ref(flat, pairs_h, offsets_h, SYM)
    assert out.dtype == torch.float32 and np.array_equal(out.detach().cpu().numpy(), want)
    assert torch.equal(out.detach(), plain) and torch.equal(sym, sym2) and torch.equal(sc, sc2)
    assert np.array_equal(sym.cpu().numpy(), wsym) and np.array_equal(sc.cpu().numpy(), wsc)

    box = _capture_fp32_grad(out) if kind == "bf16" else None
    out.backward(gout_h.to(gpu))
    ref, A, n = gather_bwd_ref(flat, pairs_h, offsets_h, gout_h.numpy())
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    if kind == "bf16":
        assert len(box) == 1 and box[0].dtype == torch.float32
        check_bwd(box[0].cpu().numpy().reshape(N * SYM, T, D), ref, A, n)
        ref_bf = torch.from_numpy(ref).float().bfloat16().double().numpy()
        got = x.grad.double().cpu().numpy().reshape(N * SYM, T, D)
        assert np.all(got[np.broadcast_to((n == 0)[:, :, None], got.shape)] == 0.0)
        assert np.all(np.abs(got - ref_bf) <= bf16_ulp(ref_bf))
    else:
        check_bwd(x.grad.cpu().numpy().reshape(N * SYM, T, D), ref, A, n)
    assert _lib.device_status() == 0


def run_onset_filter(gpu, pairs_h, offsets_h, bound, cap):
    """returns numpy (all rows of the over-allocated pairs buffer, offsets_out, counts); the op sees its first `cap` rows"""
    from transkun_amd import _lib
    B, K = len(offsets_h) - 1, len(pairs_h)
    big = torch.full((K + GUARD, 2), SENT_I, dtype=torch.int32, device=gpu)
    o2 = torch.full((B + 1 + GUARD,), SENT_I, dtype=torch.int32, device=gpu)
    cnt = torch.full((B + GUARD,), SENT_I, dtype=torch.int32, device=gpu)
    _lib.ops().segment_onset_filter(torch.from_numpy(pairs_h).to(gpu), torch.from_numpy(offsets_h).to(gpu), B, bound, big[:cap], o2[:B + 1], cnt[:B])
    assert torch.all(o2[B + 1:] == SENT_I) and torch.all(cnt[B:] == SENT_I)
    return big.cpu().numpy(), o2[:B + 1].cpu().numpy(), cnt[:B].cpu().numpy()


def onset_ref(lists, bound):
    want = [[p for p in l if p[0] < bound] for l in lists]
    counts = np.asarray([len(l) for l in want], np.int32)
    return pack(want)[0], np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), counts


ONSET_BOUNDS = (-1, 0, 1, ONSET_T // 2, ONSET_T - 1, ONSET_T, ONSET_T + 50)


@pytest.mark.gpu
@pytest.mark.parametrize("B", ONSET_B)
def test_onset_filter_chain_counts(gpu, B):
    """one, two and three blocks of the 256-wide scan with carry and a ragged last block; every bound"""
    from transkun_amd import _lib
    lists = onset_set(B)
    pairs, offsets = pack(lists)
    K = len(pairs)
    for bound in ONSET_BOUNDS:
        want, woff, wcnt = onset_ref(lists, bound)
        got, off, cnt = run_onset_filter(gpu, pairs, offsets, bound, K)
        assert np.array_equal(cnt, wcnt), bound
        assert np.array_equal(off, woff), bound
        assert np.array_equal(got[:len(want)], want), bound
        assert np.all(got[len(want):] == SENT_I), bound
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [46, 257, 700])
@pytest.mark.parametrize("cut", ["kept_minus_3", "zero_rows"])
def test_onset_filter_cap(gpu, B, cut):
    """a `pairs_out` shorter than what is kept: rows below `cap` are the reference's, the rows behind it (part of the test's own
    larger buffer) keep their sentinel, and `offsets_out` holds the full counts"""
    from transkun_amd import _lib
    lists = onset_set(B)
    pairs, offsets = pack(lists)
    want, woff, wcnt = onset_ref(lists, ONSET_T // 2)
    cap = len(want) - 3 if cut == "kept_minus_3" else 0
    assert 0 <= cap < len(want) <= len(pairs)
    got, off, cnt = run_onset_filter(gpu, pairs, offsets, ONSET_T // 2, cap)
    assert np.array_equal(got[:cap], want[:cap])
    assert np.all(got[cap:] == SENT_I)
    assert np.array_equal(off, woff) and np.array_equal(cnt, wcnt)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B", [46, 513])
def test_onset_filter_hands_on_timeout_marker(gpu, B):
    """a negative total in the source offsets (decode's time-out marker) comes out as the new total"""
    from transkun_amd import _lib
    pairs, offsets = pack(onset_set(B))
    marked = offsets.copy()
    marked[-1] = -1
    _, off, _ = run_onset_filter(gpu, pairs, marked, ONSET_T // 2, len(pairs))
    assert off[B] == -1
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,nSym", EVENT_CASES)
def test_segment_events(gpu, oracle, B, nSym):
    """every clamp of the event recurrence, per-segment begin times with up to 258 segments, two blocks from B > 128"""
    from transkun_amd import _lib
    lists, ofv, ofp, begin = event_inputs(B, nSym)
    pairs_h, offsets_h = pack(lists)
    K = len(pairs_h)
    pairs, offsets = torch.from_numpy(pairs_h).to(gpu), torch.from_numpy(offsets_h).to(gpu)
    ofValue, ofPresence = torch.from_numpy(ofv).to(gpu), torch.from_numpy(ofp).to(gpu).view(torch.uint8)
    beginTime = torch.tensor(begin, dtype=torch.float64, device=gpu)
    for step in EVENT_STEPS:
        ev, lastP, nextStart = oracle.segment_events(lists, nSym, ofv.tolist(), ofp.tolist(), EVENT_LAST, FRAME_DUR, begin, step)
        times = torch.full((K + GUARD, 2), SENT_F, dtype=torch.float64, device=gpu)
        flags = torch.full((K + GUARD, 2), 77, dtype=torch.uint8, device=gpu)
        lp = torch.full((B + GUARD,), SENT_I, dtype=torch.int32, device=gpu)
        ns = torch.full((B + GUARD,), SENT_I, dtype=torch.int32, device=gpu)
        _lib.ops().segment_events(pairs, K, offsets, B, nSym, ofValue, ofPresence, EVENT_LAST, FRAME_DUR, beginTime, step, times[:K], flags[:K],
                                  lp[:B], ns[:B])
        want_t = np.asarray([[e[0], e[1]] for c in ev for e in c], np.float64).reshape(-1, 2)
        want_f = np.asarray([[e[2], e[3]] for c in ev for e in c], np.uint8).reshape(-1, 2)
        got_t = times.cpu().numpy()
        assert np.array_equal(got_t[:K].view(np.int64), want_t.view(np.int64)), step                 # the doubles' bits
        assert np.array_equal(flags[:K].cpu().numpy(), want_f), step
        lp_h, ns_h = lp[:B].cpu().tolist(), ns[:B].cpu().tolist()
        assert lp_h == lastP and ns_h == nextStart, step
        for c, l in enumerate(lists):
            if not l:
                assert lp_h[c] == 0 and ns_h[c] == 0
        assert np.all(got_t[K:] == SENT_F) and torch.all(flags[K:] == 77) and torch.all(lp[B:] == SENT_I) and torch.all(ns[B:] == SENT_I)
    assert _lib.device_status() == 0
