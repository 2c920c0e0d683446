"""Shared by the CPU and GPU halves of tests/test_sample.py: the float64 restatement of semicrf_sample's contract, the flat-row input
family, and a checker that takes a sampler's packed draws apart into their steps and tests each step against the float64 CDF of
its row.

A draw is a pure function of (inputs, alpha, key): at a visited row t the predecessor is the first candidate whose normalised
running sum exceeds the uniform u0, and the singleton (t, t) is emitted iff u1 < sigmoid(score[t, t]).  A sampler working in fp32
can differ from that only where u0 lies within rounding of a CDF boundary.  The checker therefore accepts a pick i iff
[C64[i-1], C64[i]] meets [u0 - delta, u0 + delta]; `delta` comes from the plain-fp32 restatement's own error against float64 on
the rows a case visits (StepCase), never from the sampler under test.

Everything here is a function of its arguments; nothing is read from a fixture or from a global random generator."""
import math

import numpy as np

from transkun_amd import synth

# sample.hip: candidates per chunk of row t = SMP_BATCH * ceil((t + 1) / (SMP_NCH * SMP_BATCH))
SMP_NCH, SMP_BATCH = 128, 16

DELTA_FACTOR = 4                        # the margin for the same fp32 sums formed in another order (chunks, prefix sums of chunk sums)
DELTA_FLOOR = 2.0 ** -22                # the 24-bit uniform and the fp32 product u * Z
COIN_BAND = 8 * 2.0 ** -24              # a few fp32 ulps of 1 / (1 + expf(-x)) against a 24-bit uniform
AMBIGUOUS_CAP = 0.05


def _segments(pairs, offsets):
    return [[tuple(int(x) for x in p) for p in pairs[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]


def _check_valid(pairs, offsets, T, ends=None, B=None):
    """Every segment is a path a walk can produce: 0 <= b <= e < T (e <= forced end), strictly ascending (begin, end), intervals
    that at most touch, and no singleton strictly inside an interval."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    K = int(offsets[-1])
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and pairs.shape[0] == K
    if K == 0:
        return
    b, e = pairs[:, 0], pairs[:, 1]
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    assert (b >= 0).all() and (b <= e).all() and (e < T).all()
    if ends is not None:
        lim = np.asarray(ends, np.int64)[seg % B]
        assert (e <= lim).all()
    same = seg[1:] == seg[:-1]
    asc = (b[1:] > b[:-1]) | ((b[1:] == b[:-1]) & (e[1:] > e[:-1]))
    assert asc[same].all(), "not strictly ascending within a path"
    # the last interval (b < e) before each entry, in the same path: its end must not pass the entry's begin
    idx = np.where(b < e, np.arange(K), -1)
    last = np.maximum.accumulate(idx)
    prev = np.concatenate([[-1], last[:-1]])
    ok = prev >= 0
    ok &= seg[np.maximum(prev, 0)] == seg
    assert (e[prev[ok]] <= b[ok]).all(), "overlapping intervals or a singleton inside an interval"


# ---- float64 restatement of the contract ---------------------------------------------------------------------------------

def _u(idx, key):
    return (synth.hash_u64_numpy(np.asarray(idx, np.uint64), key) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def _uniforms(T, B, nSample, key, k0=0):
    """(u0, u1) [nSample, B, T]: the predecessor's and the singleton's uniform of draw k0 + k, chain c, row t"""
    k = np.arange(k0, k0 + nSample, dtype=np.uint64)[:, None, None]
    c = np.arange(B, dtype=np.uint64)[None, :, None]
    t = np.arange(T, dtype=np.uint64)[None, None, :]
    base = (k * np.uint64(B) + c) * np.uint64(T) + t
    return _u(np.uint64(2) * base, key), _u(np.uint64(2) * base + np.uint64(1), key)


def _alpha64(s, n):
    T, B = s.shape[0], s.shape[2]
    v = np.zeros((T, B))
    sp = lambda x: np.logaddexp(0.0, np.asarray(x, np.float64))       # (fp32 inputs are taken to float64 first, here and below)
    v[0] = sp(s[0, 0])
    for t in range(1, T):
        cand = np.concatenate([(v[t - 1] + n[t - 1])[None], v[:t] + s[t, :t]], 0)
        v[t] = np.logaddexp.reduce(cand, 0) + sp(s[t, t])
    return v


def _row_cums(s, n, v, t, c, cums):
    """Running sums of exp(x - max) over the candidates of row t >= 1 of chain c in the kernels' order (skip, then (t-1, t) ..
    (0, t)), in float64 from whatever precision the inputs have.  Built on first use, for all chains of the row at once (each
    chain's sum is still sequential: np.cumsum along the last axis)."""
    cs = cums.get(t)
    if cs is None:
        x = np.concatenate([(v[t - 1].astype(np.float64) + n[t - 1].astype(np.float64))[None],
                            v[t - 1::-1].astype(np.float64) + s[t, t - 1::-1].astype(np.float64)], 0)
        x = np.ascontiguousarray(x.T)                                     # [B, t + 1]
        m = x.max(1, keepdims=True)
        with np.errstate(invalid="ignore"):
            w = np.where(m > -np.inf, np.exp(x - m), 0.0)
        cs = cums[t] = np.cumsum(w, axis=1)
    return cs[c]


def _restated_walk(s, n, v, u0, u1, c, start, cums):
    """One draw of chain c from `start` down to frame 0 (u0, u1: that draw's uniforms per row): [(row, pick, singleton)] in walk
    order, pick = 0 for the skip, i >= 1 for the interval (row - i, row), None at row 0."""
    t = start
    steps = []
    while True:
        single = bool(u1[t] < 1.0 / (1.0 + math.exp(-float(s[t, t, c]))))
        if t == 0:
            steps.append((0, None, single))
            return steps
        cs = _row_cums(s, n, v, t, c, cums)
        Z = cs[-1]
        pick = 0
        if Z > 0:
            thr = u0[t] * Z
            pick = int(np.searchsorted(cs, thr, side="right")) if thr < Z else int(np.searchsorted(cs, Z, side="left"))
        steps.append((t, pick, single))
        t -= max(pick, 1)


def _steps_to_path(steps):
    out = []
    for t, pick, single in steps:
        if single:
            out.append((t, t))
        if pick:
            out.append((t - pick, t))
    return sorted(out)


def _restated_sample(s, n, v, nSample, key, ends=None, k0=0, cums=None):
    """List of nSample*B paths (sample-major) from the contract: float64, sequential running sums, first sum > u*Z."""
    T, B = s.shape[0], s.shape[2]
    u0, u1 = _uniforms(T, B, nSample, key, k0)
    cums = {} if cums is None else cums
    return [_steps_to_path(_restated_walk(s, n, v, u0[k, c], u1[k, c], c, T - 1 if ends is None else int(ends[c]), cums))
            for k in range(nSample) for c in range(B)]


def pack_paths(paths):
    """(pairs int32 [K, 2], offsets int32 [len(paths) + 1]) of a list of paths, the layout sample_packed returns"""
    pairs = np.asarray([p for path in paths for p in path], np.int32).reshape(-1, 2)
    offsets = np.concatenate([[0], np.cumsum([len(path) for path in paths])]).astype(np.int32)
    return pairs, offsets


# ---- flat rows -----------------------------------------------------------------------------------------------------------

def flat_inputs(T, B, seed):
    """(score [T, T, B], noise [T-1, B], alpha [T, B]) as fp32 numpy, built so that EVERY candidate of a row has comparable weight:
    with g ~ N(0, 1) per candidate, noise[t-1] = fl32(g[0] - v[t-1]) and score[t, j] = fl32(g[1 + j] - v[j]), so the log-weights
    v[j] + score[t, j] are g itself; v continues in float64 from the rounded fp32 values, i.e. it is _alpha64 of the returned
    inputs, and is returned rounded to fp32.  A walk then jumps to a frame drawn almost uniformly below it: the picks land in
    every chunk of the row, which the peaked families (picks among the first few candidates) never do.  |v| stays near log T.
    g comes from synth.hash_normal_numpy: the inputs are a function of (T, B, seed).  The upper triangle is zero."""
    score = np.zeros((T, T, B), np.float32)
    noise = np.zeros((max(T - 1, 0), B), np.float32)
    v = np.zeros((T, B))
    sp = lambda x: np.logaddexp(0.0, x)
    g = synth.hash_normal_numpy(2 * B, seed).reshape(2, B)
    score[0, 0] = g[1]
    v[0] = sp(score[0, 0].astype(np.float64))
    off = 2 * B
    for t in range(1, T):
        g = synth.hash_normal_numpy((t + 2) * B, seed, off).reshape(t + 2, B).astype(np.float64)
        off += (t + 2) * B
        noise[t - 1] = (g[0] - v[t - 1]).astype(np.float32)
        score[t, :t] = (g[1:t + 1] - v[:t]).astype(np.float32)
        score[t, t] = g[t + 1].astype(np.float32)
        cand = np.concatenate([(v[t - 1] + noise[t - 1])[None], v[:t] + score[t, :t]], 0)
        v[t] = np.logaddexp.reduce(cand, 0) + sp(score[t, t].astype(np.float64))
    return score, noise, v.astype(np.float32)


def chunk_of(t, pick):
    """the chunk of sample.hip's row t that holds candidate `pick`"""
    ch = SMP_BATCH * ((t + 1 + SMP_NCH * SMP_BATCH - 1) // (SMP_NCH * SMP_BATCH))
    return pick // ch


# ---- the step checker ----------------------------------------------------------------------------------------------------

def _fp32_row_error(s, n, v, t, cs):
    """Per chain, the largest deviation from the float64 CDF cs / cs[:, -1] of row t's CDF in plain fp32: log-weights
    fl32(fl32(v + s) - R) with R = fl32(v[t] - softplus(s[t, t])), fp32 exp, a sequential fp32 running sum (np.cumsum of float32
    accumulates in float32)."""
    f32 = np.float32
    R = v[t] - np.logaddexp(f32(0.0), s[t, t])
    R = np.where(np.isfinite(R), R, f32(0.0))
    x = np.concatenate([(v[t - 1] + n[t - 1])[None], v[t - 1::-1] + s[t, t - 1::-1]], 0) - R
    assert x.dtype == np.float32
    with np.errstate(over="ignore"):
        run = np.cumsum(np.exp(np.ascontiguousarray(x.T)), axis=1, dtype=f32)
    assert run.dtype == np.float32
    ok = (cs[:, -1] > 0) & (run[:, -1] > 0) & np.isfinite(run[:, -1])
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(run.astype(np.float64) / run[:, -1:].astype(np.float64) - cs / cs[:, -1:]).max(1)
    return np.where(ok, err, 0.0)


def _walk_of_path(path, start):
    """[(row, pick, singleton)] of a valid path walked from `start` (unique: at row t at most one interval ends), or None when
    the path holds two intervals with the same end or an entry the walk does not reach"""
    pred, single = {}, set()
    for b, e in path:
        if b == e:
            single.add(e)
        elif e in pred:
            return None
        else:
            pred[e] = b
    steps, t, used = [], start, 0
    while True:
        sg = t in single
        used += sg
        if t == 0:
            steps.append((0, None, sg))
            break
        j = pred.get(t)
        used += j is not None
        steps.append((t, 0 if j is None else t - j, sg))
        t = t - 1 if j is None else j
    return steps if used == len(path) else None


def _all_cums(s, n, v, t, cums):
    _row_cums(s, n, v, t, 0, cums)
    return cums[t]                                                         # [B, t + 1]


def _restated_walks(s, n, v, key, k0, nSample, ends=None, cums=None):
    """_restated_walk for all nSample * B draws at once (sample-major list of step lists): the walks advance in lockstep, row by
    row from the top, and the draws standing on a row take their picks in one numpy call -- the same float64 running sums, the
    same comparisons (np.searchsorted side="right" is the count of sums <= u Z, side="left" the count of sums < Z)."""
    T, B = s.shape[0], s.shape[2]
    u0, u1 = _uniforms(T, B, nSample, key, k0)
    cums = {} if cums is None else cums
    kk, cc = np.repeat(np.arange(nSample), B), np.tile(np.arange(B), nSample)
    pos = np.full(nSample * B, T - 1) if ends is None else np.asarray(ends, np.int64)[cc]
    with np.errstate(over="ignore"):
        pdiag = 1.0 / (1.0 + np.exp(-np.diagonal(s).astype(np.float64)))   # [B, T]
    walks = [[] for _ in range(nSample * B)]
    for t in range(int(pos.max()), -1, -1):
        act = np.nonzero(pos == t)[0]
        if not len(act):
            continue
        k, c = kk[act], cc[act]
        single = u1[k, c, t] < pdiag[c, t]
        if t == 0:
            for w, sg in zip(act, single):
                walks[w].append((0, None, bool(sg)))
            break
        rows = _all_cums(s, n, v, t, cums)[c]
        Z = rows[:, -1]
        thr = u0[k, c, t] * Z
        pick = np.where(thr < Z, (rows <= thr[:, None]).sum(1), (rows < Z[:, None]).sum(1))
        pick = np.where(Z > 0, pick, 0)
        pos[act] = t - np.maximum(pick, 1)
        for w, pk, sg in zip(act, pick, single):
            walks[w].append((t, int(pk), bool(sg)))
    return walks


def check_steps(score, noise, v, key, k0, nSample, ends, pairs, offsets, delta, cums=None):
    """Every step of every draw in (pairs, offsets) -- draws k0 .. k0 + nSample - 1 of semicrf_sample on fp32 numpy (score, noise)
    with the fp32 alpha `v` -- against the float64 CDF of its row.  Returns (violations, steps, ambiguous):
      violations  [(k, c, row, "pick" | "coin" | "path", detail)]: a predecessor whose CDF interval [C64[i-1], C64[i]] does not
                  meet [u0 - delta, u0 + delta]; a singleton that disagrees with u1 < sigmoid(score[t, t]) further than COIN_BAND
                  from the boundary; a path that is not a walk from its start;
      steps       visited rows, row 0 (coin only) included;
      ambiguous   steps at which more than one candidate is admissible or the coin is inside its band.
    The row CDFs are cached in `cums` per row, and the steps are tested row by row, all draws that visit a row in one numpy call."""
    T, B = score.shape[0], score.shape[2]
    assert score.dtype == noise.dtype == v.dtype == np.float32
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    assert len(offsets) == nSample * B + 1
    _check_valid(pairs, offsets, T, ends, B)
    u0, u1 = _uniforms(T, B, nSample, key, k0)
    with np.errstate(over="ignore"):
        pdiag = 1.0 / (1.0 + np.exp(-np.diagonal(score).astype(np.float64)))       # [B, T]
    cums = {} if cums is None else cums
    paths = _segments(pairs, offsets)
    bad, flat = [], []
    for i, path in enumerate(paths):
        k, c = divmod(i, B)
        steps = _walk_of_path(path, T - 1 if ends is None else int(ends[c]))
        if steps is None:
            bad.append((k, c, -1, "path", path))
        else:
            flat += [(k, c, t, -1 if pick is None else pick, sg) for t, pick, sg in steps]
    if not flat:
        return bad, 0, 0
    k, c, t, pick, single = (np.asarray(x) for x in zip(*flat))
    # the coin
    p, uc = pdiag[c, t], u1[k, c, t]
    amb = np.abs(uc - p) <= COIN_BAND
    wrong = ~amb & (single.astype(bool) != (uc < p))
    bad += [(int(k[i]), int(c[i]), int(t[i]), "coin", (bool(single[i]), float(uc[i]), float(p[i]))) for i in np.nonzero(wrong)[0]]
    # the predecessor, row by row
    order = np.argsort(t, kind="stable")
    cuts = np.nonzero(np.diff(t[order]))[0] + 1
    for grp in np.split(order, cuts):
        row = int(t[grp[0]])
        if row == 0:
            continue
        rows = _all_cums(score, noise, v, row, cums)[c[grp]]
        Z, u = rows[:, -1], u0[k[grp], c[grp], row]
        lo = (rows < ((u - delta) * Z)[:, None]).sum(1)                    # first i with C64[i] >= u0 - delta
        hi = np.minimum((rows <= ((u + delta) * Z)[:, None]).sum(1), row)  # last i with C64[i-1] <= u0 + delta
        lo, hi = np.where(Z > 0, lo, 0), np.where(Z > 0, hi, 0)            # no candidate of positive weight: the skip
        amb[grp] |= hi > lo
        for j in np.nonzero((pick[grp] < lo) | (pick[grp] > hi))[0]:
            i = grp[j]
            bad.append((int(k[i]), int(c[i]), row, "pick", (int(pick[i]), int(lo[j]), int(hi[j]), float(u[j]))))
    return bad, len(flat), int(amb.sum())


class StepCase:
    """The reference side of one sampler case, computed once from (inputs, alpha, key) alone: the float64 restatement's draws,
    eps (the plain-fp32 restatement's largest CDF error over the rows those draws visit), delta = max(DELTA_FACTOR * eps,
    DELTA_FLOOR), and the share of the restatement's own steps that are ambiguous at that delta, which must stay below
    AMBIGUOUS_CAP.  check() then runs a sampler's draws of the same case through check_steps."""

    def __init__(self, name, score, noise, v, key, k0, nSample, ends=None):
        assert score.dtype == noise.dtype == v.dtype == np.float32
        self.name, self.score, self.noise, self.v = name, score, noise, v
        self.key, self.k0, self.nSample, self.ends = key, k0, nSample, ends
        T, B = score.shape[0], score.shape[2]
        self.T, self.B = T, B
        self.cums = {}
        self.walks = _restated_walks(score, noise, v, key, k0, nSample, ends, self.cums)
        self.paths = [_steps_to_path(w) for w in self.walks]
        visited = np.zeros((T, B), bool)
        for i, w in enumerate(self.walks):
            visited[[t for t, _, _ in w if t > 0], i % B] = True
        self.eps = max([float(_fp32_row_error(score, noise, v, t, self.cums[t])[visited[t]].max())
                        for t in np.nonzero(visited.any(1))[0]], default=0.0)
        self.delta = max(DELTA_FACTOR * self.eps, DELTA_FLOOR)
        bad, self.steps, self.ambiguous = self.check(*pack_paths(self.paths), quiet=True)
        assert not bad, (name, bad[:5])                                   # the restatement is admissible by construction
        self.share = self.ambiguous / max(self.steps, 1)
        print(f"{name}: T={T} B={B} N={nSample} eps {self.eps:.3g} delta {self.delta:.3g} steps {self.steps} "
              f"ambiguous {self.ambiguous} ({100 * self.share:.3g} %)")
        assert self.share <= AMBIGUOUS_CAP, (name, self.share)

    def check(self, pairs, offsets, quiet=False):
        bad, steps, amb = check_steps(self.score, self.noise, self.v, self.key, self.k0, self.nSample, self.ends, pairs, offsets,
                                      self.delta, self.cums)
        if not quiet:
            print(f"{self.name}: checked {steps} steps, {amb} ambiguous, {len(bad)} violations")
        return bad, steps, amb

    def far_chunk_share(self, first_row=2048):
        """(share, count): of the restatement's picks on rows >= first_row, the share that lies in another chunk than the first"""
        picks = [(t, p) for w in self.walks for t, p, _ in w if t >= first_row]
        far = sum(chunk_of(t, p) > 0 for t, p in picks)
        return far / max(len(picks), 1), len(picks)

    def chunks_hit(self, first_row=2048):
        return len({(chunk_of(t, p)) for w in self.walks for t, p, _ in w if t >= first_row})
