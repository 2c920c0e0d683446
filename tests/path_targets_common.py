"""Shared by the CPU and GPU halves of tests/test_path_targets.py: inputs with full 24-bit mantissas, the target-path families,
the cotangents, and float64 expected values of evalPath / logProb and of their gradients.

Everything here is a deterministic function of (T, B, seed); nothing is read from a fixture.  Expected values come from numpy
float64 sums (the path side) and from the C oracle in float64 (logZ and the marginals), never from the code under test."""
import numpy as np
import torch

KINDS = ("randn", "model", "cancel")

IN_CONTRACT = ("empty_all", "only_first_chain", "only_last_chain", "full_span", "all_singletons", "touching_chain", "ragged_counts",
               "long_mixed", "unsorted", "boundary")
FAMILIES = IN_CONTRACT + ("overlap_dup",)
COVERING = ("full_span", "touching_chain")          # every gap covered: with the "cancel" inputs the covered sum cancels cum[T-1]

SCALAR_W = -0.625                                    # the expanded-scalar cotangent (exact in fp32, not +-1)


# ------------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------------

def make_inputs(T, B, seed, kind, base_device="cpu"):
    """(score [T,T,B], noise [T-1,B]) fp32 on the CPU.  synth.crf_inputs values are multiples of 2**-16 (randn) or 2**-20 (model,
    with an all-zero noise): any sum of a few thousand of them is exact in fp32, so they cannot tell one accumulator or one
    summation order from another.  Here they are scaled by an irrational-looking factor and perturbed in float64 with a seeded
    CPU generator, then rounded ONCE to fp32: full 24-bit mantissas, non-zero noise for every kind.
      randn / model: score * 1.2345678901 + 1e-3 N(0,1); noise * 0.987654321 + sigma N(0,1), sigma = 1 (randn) / 30 (model).
      cancel: randn's score; noise = +-1e3 (1 + 0.25 N(0,1)) with hashed signs: a path that covers every gap (COVERING) sums
              ~T values of size 1e3 twice with opposite signs -- a float accumulator loses ~1e-1 there, a double one nothing.
    base_device: where the hash of synth.crf_inputs runs (bit-identical on either device: test_generator_same_bits_on_gpu)."""
    from transkun_amd import synth
    g = torch.Generator(device="cpu")
    g.manual_seed(1000003 * seed + 7919 * T + B + 17 * KINDS.index(kind))
    s0, n0 = synth.crf_inputs(T, B, seed, base_device, "model" if kind == "model" else "randn")
    s0, n0 = s0.cpu(), n0.cpu()
    score = torch.empty(T, T, B, dtype=torch.float32)
    rows = max(1, (1 << 24) // max(T * B, 1))                        # float64 temporaries of at most 128 MB
    for r in range(0, T, rows):
        blk = s0[r:r + rows].double() * 1.2345678901
        blk += 1e-3 * torch.randn(blk.shape, generator=g, dtype=torch.float64)
        score[r:r + rows] = blk.float()
    z = torch.randn((max(T - 1, 0), B), generator=g, dtype=torch.float64)
    if kind == "cancel":
        sign = torch.where(n0 >= 0, 1.0, -1.0).double()
        noise = sign * 1e3 * (1.0 + 0.25 * z)
    else:
        noise = n0.double() * 0.987654321 + (30.0 if kind == "model" else 1.0) * z
    return score.contiguous(), noise.float().contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# target families
# ------------------------------------------------------------------------------------------------------------------------------

def _long_mixed_chain(T, rs):
    """Lengths from {0, 1, 2, 7, 33, T//3+1}, gaps 0..2 (0: the next interval begins on this one's end frame -- it is then longer
    than a singleton, and a singleton is never touched)."""
    lens = (0, 1, 2, 7, 33, T // 3 + 1)
    out, t, touching = [], int(rs.randint(0, 3)), False
    while t <= T - 1:
        ln = lens[int(rs.randint(1 if touching else 0, len(lens)))]
        e = min(t + ln, T - 1)
        out.append((t, e))
        gap = int(rs.randint(0, 3))
        touching = gap == 0 and e > t and e < T - 1
        t = e + (gap if touching or gap > 0 else 1)
    return out


def family(name, T, B, seed):
    """List (len B) of lists of (begin, end)."""
    rs = np.random.RandomState((seed * 7919 + T * 31 + B) % (2 ** 31 - 1))
    if name == "empty_all":
        return [[] for _ in range(B)]
    if name in ("only_first_chain", "only_last_chain"):
        out = [[] for _ in range(B)]
        out[0 if name == "only_first_chain" else B - 1] = _long_mixed_chain(T, rs)
        return out
    if name == "full_span":
        return [[(0, T - 1)] for _ in range(B)]
    if name == "all_singletons":
        return [[(t, t) for t in range(T)] for _ in range(B)]
    if name == "touching_chain":
        return [[(t, t + 1) for t in range(T - 1)] for _ in range(B)]
    if name == "ragged_counts":
        counts = (0, 1, 63, 64, 65, 127, 128, 129, T)                 # both sides of path_score_wave's 64-lane stride
        out = []
        for c in range(B):
            n = min(counts[c % len(counts)], T)
            fr = np.sort(rs.choice(T, size=n, replace=False)) if n else []
            out.append([(int(t), int(t)) for t in fr])
        return out
    if name == "long_mixed":
        return [_long_mixed_chain(T, rs) for _ in range(B)]
    if name == "unsorted":
        out = []
        for c in range(B):
            lst = _long_mixed_chain(T, rs)
            out.append(lst[::-1] if c % 2 == 0 else [lst[i] for i in rs.permutation(len(lst))])
        return out
    if name == "boundary":
        singles = [[(0, 0)], [(0, 1)], [(T - 2, T - 1)], [(T - 1, T - 1)]]
        combos = singles + ([[(0, 0), (T - 1, T - 1)], [(0, 1), (T - 2, T - 1)], [(0, 0), (T - 2, T - 1)]] if T >= 4 else [])
        combos = [[(b, e) for b, e in lst if 0 <= b <= e < T] for lst in combos]
        return [list(combos[c % len(combos)]) for c in range(B)]
    if name == "overlap_dup":                                        # outside evalPath's contract; the forward is linear, so defined
        out = []
        for c in range(B):
            base = [(2, 5), (2, 5), (3, 8), (0, T - 1), (4, 4), (4, 4), (4, 4), (1, T - 2), (0, T - 1)]
            lst = [(b, e) for b, e in base if 0 <= b <= e < T]
            for _ in range(int(rs.randint(0, 6))):
                b = int(rs.randint(0, T)); e = min(T - 1, b + int(rs.randint(0, 12)))
                lst += [(b, e)] * int(rs.randint(1, 3))
            out.append(lst)
        return out
    raise ValueError(name)


def packed(iv):
    """(b, e, c) int64 numpy arrays over all intervals."""
    cnt = [len(x) for x in iv]
    K = sum(cnt)
    flat = np.asarray([p for lst in iv for p in lst], dtype=np.int64).reshape(K, 2)
    return flat[:, 0], flat[:, 1], np.repeat(np.arange(len(iv), dtype=np.int64), cnt)


# ------------------------------------------------------------------------------------------------------------------------------
# cotangents
# ------------------------------------------------------------------------------------------------------------------------------

def chain_weights(B, seed):
    """Per-chain cotangent, float64 numpy holding fp32 values: distinct in every chain, mixed signs, exactly 0.0 in one chain of
    every 32-chain panel group, one value of -1000.  (B == 1 has room for one of the two special values only: -1000.)"""
    rs = np.random.RandomState(4099 + seed)
    w = rs.uniform(0.25, 2.0, B) * np.where(np.arange(B) % 3 == 1, -1.0, 1.0)
    w = w.astype(np.float32).astype(np.float64)
    for g in range((B + 31) // 32):
        n = min(32, B - 32 * g)
        w[32 * g + (5 * g + 3) % n] = 0.0
    big = B // 2
    while w[big] == 0.0 and B > 1:
        big = (big + 1) % B
    w[big] = -1000.0
    nz = w[w != 0.0]
    assert len(set(nz.tolist())) == len(nz) and (B < 3 or ((w > 0).any() and (w < 0).any()))
    return w


def sampled_chains(B):
    """All chains up to 72; beyond, the first 32, the last 32 and 8 in the middle (test_persist_model_chain_counts_full_length)."""
    if B <= 72:
        return list(range(B))
    return sorted(set(list(range(32)) + list(range(B - 32, B)) + [B // 2 + i for i in range(8)]))


# ------------------------------------------------------------------------------------------------------------------------------
# float64 expectations
# ------------------------------------------------------------------------------------------------------------------------------

def path_reference(score, noise, iv):
    """(path64 [B], abs_terms [B]) in float64 numpy: path64[c] = sum_t n[t,c] + sum_(b,e) (s[e,b,c] - sum_{t=b}^{e-1} n[t,c]);
    abs_terms the same sum over absolute values (the scale of the accumulation error).  Prefix sums in long double."""
    T, B = score.shape[0], score.shape[2]
    n = noise.numpy().astype(np.longdouble)
    cum = np.concatenate([np.zeros((1, B), np.longdouble), np.cumsum(n, axis=0)])          # cum[t] = sum_{u<t} n[u]
    cua = np.concatenate([np.zeros((1, B), np.longdouble), np.cumsum(np.abs(n), axis=0)])
    path, terms = cum[-1].copy(), cua[-1].copy()
    b, e, c = packed(iv)
    if len(b):
        s = score[torch.from_numpy(e), torch.from_numpy(b), torch.from_numpy(c)].numpy().astype(np.longdouble)
        np.add.at(path, c, s - (cum[e, c] - cum[b, c]))
        np.add.at(terms, c, np.abs(s) + (cua[e, c] - cua[b, c]))
    return path.astype(np.float64), terms.astype(np.float64)


def eval_path_bound(path64, terms):
    """The kernels accumulate in double and round once: |got - path64| <= 2**-23 |path64| + 2**-40 sum|terms|."""
    return 2.0 ** -23 * np.abs(path64) + 2.0 ** -40 * terms


def cover_counts(iv, T, B):
    """cover[t, c] = number of intervals of chain c with b <= t < e (int64 numpy [T-1, B])."""
    d = np.zeros((T + 1, B), np.int64)
    b, e, c = packed(iv)
    np.add.at(d, (b, c), 1)
    np.add.at(d, (e, c), -1)
    return np.cumsum(d, axis=0)[:max(T - 1, 0)]


class Oracle64:
    """The float64 truth of one (shape, kind): logZ and marginals of the sampled chains from the C oracle, kept where the
    gradients will be compared (`dev`)."""

    def __init__(self, oracle, score, noise, dev):
        T, B = score.shape[0], score.shape[2]
        self.T, self.B, self.dev = T, B, dev
        self.idx = sampled_chains(B)
        ix = torch.tensor(self.idx)
        lz, grad, gn, _, _ = oracle.forward_backward_f64(score.index_select(2, ix).numpy(), noise.index_select(1, ix).numpy())
        self.lz64 = lz                                               # numpy [n]
        self.ix = ix.to(dev)
        self.grad64 = torch.from_numpy(grad).to(dev)                 # [T,T,n] float64
        self.gn64 = torch.from_numpy(gn).to(dev)                     # [T-1,n]
        self.lut = np.full(B, -1, np.int64)
        self.lut[self.idx] = np.arange(len(self.idx))

    def want_grads(self, iv, w):
        """(dS64 [T,T,n], dN64 [T-1,n]) of sum_c w[c] logProb[c] for the sampled chains: w_c (count - grad64), w_c (1 - cover - gn64)."""
        T, dev = self.T, self.dev
        wj = torch.from_numpy(np.asarray(w, np.float64)[self.idx]).to(dev)
        dS = self.grad64 * (-wj)
        b, e, c = packed(iv)
        keep = self.lut[c] >= 0
        if keep.any():
            jt = torch.from_numpy(self.lut[c[keep]]).to(dev)
            dS.index_put_((torch.from_numpy(e[keep]).to(dev), torch.from_numpy(b[keep]).to(dev), jt), wj[jt], accumulate=True)
        cover = torch.from_numpy(cover_counts(iv, T, self.B)[:, self.idx]).to(dev).double()
        dN = (1.0 - cover - self.gn64) * wj
        return dS, dN
