"""Shared by tests/test_path_stats.py: the fixture of reference counts, generators of valid interval lists and a brute-force
maximum bipartite matching (test infrastructure; nothing here is used by the product)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOLERANCES = [(0, 0), (1, 0), (0, 2), (2, 2), (8, 8)]


def load_groups():
    """tests/golden/pathstats_small.npz (tools/make_pathstats_golden.py) as (edge names, [group dicts])."""
    g = np.load(os.path.join(GOLDEN, "pathstats_small.npz"), allow_pickle=False)
    n = len([k for k in g.files if k.endswith("_T")])
    groups = [{k: g[f"g{i}_{k}"] for k in ("T", "est_pairs", "est_offsets", "ref_pairs", "ref_offsets", "counts")} for i in range(n)]
    return [str(x) for x in g["edge_names"]], groups


def pack(lists):
    """List[List[(b, e)]] -> (pairs int32 [max(K, 1), 2], offsets int32 [B + 1]) CPU tensors; no validation (the tests pack invalid
    lists on purpose)."""
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(x) for x in lists], out=off[1:])
    flat = [p for l in lists for p in l] or [(0, 0)]
    return torch.tensor(flat, dtype=torch.int32).reshape(-1, 2), torch.from_numpy(off)


def unpack(pairs, offsets):
    p, o = np.asarray(pairs).reshape(-1, 2), [int(x) for x in offsets]
    return [[(int(b), int(e)) for b, e in p[o[c]:o[c + 1]]] for c in range(len(o) - 1)]


def random_path(rng, T, density):
    """A path in the decoder's sense: maybe a singleton at a frame, then an interval to a later frame (touching the next one) or a
    step ahead."""
    out, t = [], 0
    while t < T:
        if rng.random() < 0.3 * density:
            out.append((t, t))
        if t == T - 1:
            break
        if rng.random() < density:
            e = min(T - 1, t + 1 + int(rng.integers(0, 6)))
            out.append((t, e))
            t = e
        else:
            t += 1
    return out


def jitter(rng, path, T, amount):
    """Every interval moved by up to `amount` frames at either end (some dropped), then made non-decreasing in begin and in end again:
    a list the comparison accepts (it need not be a path) that is close to `path` without being equal to it."""
    out, pb, pe = [], 0, 0
    for b, e in path:
        if rng.random() < 0.1:
            continue
        b = min(max(b + int(rng.integers(-amount, amount + 1)), pb), T - 1)
        e = min(max(e + int(rng.integers(-amount, amount + 1)), pe, b), T - 1)
        out.append((b, e))
        pb, pe = b, e
    return out


def related_lists(T, B, seed, density=0.5, amount=2):
    """(est, ref): ref random paths; est alternately a jittered copy of ref and an independent path."""
    rng = np.random.default_rng(seed)
    ref = [random_path(rng, T, density * (0.3 + 0.7 * rng.random())) for _ in range(B)]
    est = [jitter(rng, r, T, amount) if c % 3 else random_path(rng, T, density) for c, r in enumerate(ref)]
    return est, ref


def max_matching(est, ref, tb, te):
    """Size of a maximum matching of the compatibility graph, by augmenting paths (Kuhn); no use of the lists' order."""
    adj = [[j for j, (rb, re) in enumerate(ref) if abs(b - rb) <= tb and abs(e - re) <= te] for b, e in est]
    owner = [-1] * len(ref)

    def augment(i, seen):
        for j in adj[i]:
            if j in seen:
                continue
            seen.add(j)
            if owner[j] < 0 or augment(owner[j], seen):
                owner[j] = i
                return True
        return False
    return sum(1 for i in range(len(est)) if augment(i, set()))
