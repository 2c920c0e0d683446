"""Shared by the CPU and GPU tests of tests/test_forced_start.py: start patterns, the float64 reference of the forced-start
posterior (the oracle's forward_backward_f64 on the slice score[s:, s:, c], noise[s:, c], shifted by s) and the comparison.

Everything here is a function of its arguments."""
import numpy as np
import torch

from conftest import edge_inputs
from test_posteriors import FIELDS, _dense_reference, _grad_tol

KINDS = {  # name -> (synth kind, transform of conftest.edge_inputs)
    "randn": ("randn", None), "model": ("model", None), "ties": ("ties", None), "huge": ("model", "huge"),
}


def inputs(T, B, kind, seed):
    k, tr = KINDS[kind]
    return edge_inputs(T, B, k, seed, tr)


def cycle_starts(T, B):
    """0, 1, T//2, T-2, T-1 over the chains (clipped into [0, T-1])."""
    base = [0, 1, T // 2, T - 2, T - 1]
    return [min(max(base[c % 5], 0), T - 1) for c in range(B)]


def segment_loop_starts(T, B, seed):
    """As the segment loop produces them: half the chains 0, half uniform in [0, T/2]."""
    rng = np.random.RandomState(seed)
    st = rng.randint(0, T // 2 + 1, size=B)
    st[rng.permutation(B)[:B // 2]] = 0
    return [int(x) for x in st]


def _softplus(x):
    return np.logaddexp(0.0, x)


def slice_reference(oracle, s, n, starts, chains=None):
    """float64 truth of posteriors(s, n, forcedStartPos=starts): per chain the unconditional reference on the slice from its
    start, shifted by the start, zeros before it.  Chains with one start share an oracle call; a slice of ONE frame is the closed
    form logZ = sp(d), single = sigmoid(d), node = 1.  Returns a dict of [T(, -1), B] arrays plus "marg" [T, T, B] (the dense
    marginal, marg[e, b, c]); chains not in `chains` (default all) stay NaN."""
    T, B = s.shape[0], s.shape[2]
    chains = list(range(B)) if chains is None else list(chains)
    r = {k: np.full((T, B), np.nan) for k in ("node", "begin", "end", "single")}
    r["noise"] = np.full((max(T - 1, 0), B), np.nan)
    r["logZ"] = np.full(B, np.nan); r["entropy"] = np.full(B, np.nan)
    r["marg"] = np.full((T, T, B), np.nan)
    for a in sorted({int(starts[c]) for c in chains}):
        idx = [c for c in chains if int(starts[c]) == a]
        for k in ("node", "begin", "end", "single"):
            r[k][:a, idx] = 0.0
        r["noise"][:a, idx] = 0.0
        r["marg"][:, :, idx] = 0.0
        if a == T - 1:
            d = s[a, a, idx].double().numpy()
            sg = 1.0 / (1.0 + np.exp(-d))
            r["logZ"][idx] = _softplus(d)
            r["single"][a, idx] = sg; r["node"][a, idx] = 1.0
            r["begin"][a, idx] = 0.0; r["end"][a, idx] = 0.0
            r["entropy"][idx] = _softplus(d) - sg * d
            r["marg"][a, a, idx] = sg
            continue
        ss = s[a:, a:, idx].contiguous(); ns = n[a:, idx].contiguous()
        ref = _dense_reference(oracle, ss, ns)
        for k in ("node", "begin", "end", "single"):
            r[k][a:, idx] = ref[k]
        r["noise"][a:, idx] = ref["noise"]
        r["logZ"][idx] = ref["logZ"]; r["entropy"][idx] = ref["entropy"]
        _, grad, _, _, _ = oracle.forward_backward_f64(ss.numpy(), ns.numpy())
        low = np.tril(np.ones((T - a, T - a), bool))[:, :, None]
        for j, c in enumerate(idx):
            r["marg"][a:, a:, c] = np.where(low[:, :, 0], grad[:, :, j], 0.0)
    return r


def np_fields(P):
    return {k: getattr(P, k).cpu().double().numpy() for k in ("logZ", "entropy") + FIELDS}


def check_against_f64(P, r, starts, what, chains=None, entropy=True, scale=1.0):
    """Every Posteriors field of chain c against the slice reference at the project's tolerances; exact zeros before the start."""
    T, B = P["node"].shape
    chains = list(range(B)) if chains is None else list(chains)
    lz = r["logZ"][chains]
    tol = scale * _grad_tol(lz)
    worst = {}
    for c in chains:
        a = int(starts[c])
        assert abs(P["logZ"][c] - r["logZ"][c]) <= scale * 1e-5 * max(1.0, abs(r["logZ"][c])), (what, c, P["logZ"][c], r["logZ"][c])
        for k in FIELDS:
            assert np.all(P[k][:a, c] == 0.0), f"{what}: {k} of chain {c} is not exactly 0 before its start {a}"
            err = float(np.max(np.abs(P[k][:, c] - r[k][:, c]))) if P[k].shape[0] else 0.0
            worst[k] = max(worst.get(k, 0.0), err)
            assert err <= tol, f"{what}: {k} chain {c} start {a}: {err} > {tol}"
        if entropy:
            np.testing.assert_allclose(P["entropy"][c], r["entropy"][c], rtol=1e-4, atol=T * tol, err_msg=f"{what}: entropy chain {c}")
    return worst


def random_path(T, a, rng):
    """A valid path from frame a: singletons and intervals as decode lists them, ascending."""
    path, t = [], a
    while True:
        if rng.rand() < 0.4:
            path.append((t, t))
        if t == T - 1:
            return path
        if rng.rand() < 0.5:
            t += 1
        else:
            e = int(rng.randint(t + 1, min(T, t + 12)))
            path.append((t, e))
            t = e


def peaked_inputs(T, starts, seed):
    """score +12 on the cells of a random path per chain (from its start) and -12 on every other cell with begin <= end, noise 0:
    every other path differs in at least one cell at a cost of e^-12 each, fewer than 2500 cells per chain at T = 70, so every path
    interval has marginal > 0.95 and every other cell < 0.05."""
    rng = np.random.RandomState(seed)
    B = len(starts)
    s = torch.full((T, T, B), -12.0)
    paths = []
    for c, a in enumerate(starts):
        p = random_path(T, int(a), rng)
        for b, e in p:
            s[e, b, c] = 12.0
        paths.append(p)
    return s.contiguous(), torch.zeros(T - 1, B), paths
