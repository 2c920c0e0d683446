#!/usr/bin/env python3
"""Generate tests/golden/pathstats_small.npz: packed pairs of interval lists and the six counts the REFERENCE's own
compareBracket / compareFramewise (transkun/Evaluation.py) give for every chain.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_pathstats_golden.py --reference <checkout of Yujia-Yan/Transkun>

Evaluation.py imports mir_eval at module level, which need not be installed: the two functions and their helpers are lifted out of
the source file with ast at run time (as tools/make_golden.py lifts the transcription loop) and run as they are.  Nothing of the
reference is copied into this repository; the fixture holds data only -- per group g of chains that share a frame count:
    g<k>_T, g<k>_est_pairs [K, 2], g<k>_est_offsets [B + 1], g<k>_ref_pairs, g<k>_ref_offsets   (int32, decode_packed's format)
    g<k>_counts [B, 6]   nGT, nEst, nCorrect (compareBracket), nGT, nEst, nIntersected (compareFramewise, countZero = True)
                         -- the first six columns of semicrf_compare_paths' stats
and `edge_names`, the names of the hand-built chains of group 0 in order.

Groups: 0 hand-built edge cases (T = 16); 1 every pair of paths at T = 2; 2, 3 decoded pairs (the reference list is the Viterbi
path of a random score tensor on the CPU kernels of this package, the estimate the path of the same scores plus small noise)
at T = 24 and T = 48; 4 random valid paths at T = 33.  The shares the tests assert are checked here before anything is written.
"""
from __future__ import annotations

import argparse
import ast
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

OUT = os.path.join(ROOT, "tests", "golden", "pathstats_small.npz")
NAMES = ["_listOfListToTuple", "compareBracket", "intersectTwoInterval", "findIntersectListOfIntervals", "computeIntervalLengthSum",
         "compareFramewise"]


def lift(reference: str):
    path = os.path.join(reference, "transkun", "Evaluation.py")
    tree = ast.parse(open(path).read())
    found = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES}
    assert set(found) == set(NAMES), sorted(found)
    ns = {}
    exec(compile(ast.Module(body=[found[n] for n in NAMES], type_ignores=[]), path, "exec"), ns)
    return ns["compareBracket"], ns["compareFramewise"]


def pack(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([len(x) for x in lists], out=off[1:])
    pairs = np.asarray([p for l in lists for p in l], dtype=np.int32).reshape(-1, 2)
    return pairs, off


def random_path(rng, T: int, density: float):
    """A valid path: from frame 0 on, maybe a singleton at the frame, then an interval to a later frame or a step ahead."""
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


def decoded_pairs(T: int, B: int, seed: int, scale: float, jitter: float):
    import torch
    from transkun_amd import CRF
    g = torch.Generator().manual_seed(seed)
    score = torch.randn(T, T, B, generator=g) * scale - 0.5
    noise = torch.randn(T - 1, B, generator=g) * 0.5
    ref = CRF.NeuralSemiCRFInterval(score, noise).decode()
    est = CRF.NeuralSemiCRFInterval(score + jitter * torch.randn(T, T, B, generator=g), noise).decode()
    return est, ref


EDGES = [   # (name, estimate, reference), T = 16
    ("empty_estimate", [], [(0, 3), (5, 5), (7, 9)]),
    ("empty_reference", [(0, 3), (5, 5), (7, 9)], []),
    ("both_empty", [], []),
    ("singleton_and_interval_share_begin", [(2, 2), (2, 6), (9, 9)], [(2, 2), (2, 7), (9, 9), (9, 12)]),
    ("touching_intervals", [(1, 4), (4, 8), (8, 8), (8, 11)], [(1, 4), (4, 7), (7, 11)]),
    ("estimate_inside_reference", [(4, 6)], [(2, 9)]),
    ("reference_inside_estimate", [(2, 9)], [(4, 6)]),
    ("equal_ends_tie", [(0, 5), (5, 9), (12, 15)], [(2, 5), (5, 5), (6, 9), (9, 15)]),
    ("identical", [(0, 0), (0, 15), (15, 15)], [(0, 0), (0, 15), (15, 15)]),
    ("disjoint", [(0, 2), (8, 9)], [(3, 7), (10, 15)]),
    ("full_span_against_singletons", [(0, 15)], [(t, t) for t in range(16)]),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TRANSKUN_REFERENCE"), help="a checkout of the reference (holds transkun/Evaluation.py)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or TRANSKUN_REFERENCE) is required")
    compareBracket, compareFramewise = lift(args.reference)

    groups = [(16, [e for _, e, _ in EDGES], [r for _, _, r in EDGES])]
    cells = [(0, 0), (0, 1), (1, 1)]
    paths2 = [[c for c, k in zip(cells, keep) if k] for keep in itertools.product((0, 1), repeat=3)]
    groups.append((2, [a for a in paths2 for _ in paths2], [b for _ in paths2 for b in paths2]))
    for T, B, seed in ((24, 128, 11), (48, 128, 12)):
        est, ref = decoded_pairs(T, B, seed, 1.5, 0.6)
        groups.append((T, est, ref))
    rng = np.random.default_rng(5)
    groups.append((33, [random_path(rng, 33, 0.5) for _ in range(96)], [random_path(rng, 33, 0.5) for _ in range(96)]))

    out, rows = {"edge_names": np.asarray([n for n, _, _ in EDGES])}, []
    for k, (T, est, ref) in enumerate(groups):
        counts = np.asarray([list(compareBracket(list(e), list(r))) + list(compareFramewise(list(e), list(r))) for e, r in zip(est, ref)],
                            dtype=np.int32)
        ep, eo = pack(est)
        rp, ro = pack(ref)
        out.update({f"g{k}_T": np.int32(T), f"g{k}_est_pairs": ep, f"g{k}_est_offsets": eo, f"g{k}_ref_pairs": rp, f"g{k}_ref_offsets": ro,
                    f"g{k}_counts": counts})
        rows.append(counts)
        assert (counts[:, 0] == [len(r) for r in ref]).all() and (counts[:, 1] == [len(e) for e in est]).all()
    allc = np.concatenate(rows)
    n = len(allc)
    part_exact = int(((allc[:, 2] > 0) & (allc[:, 2] < allc[:, 0])).sum())
    part_frames = int(((allc[:, 5] > 0) & (allc[:, 5] < allc[:, 3])).sum())
    print(f"{n} chains; 0 < nExact < nRef: {part_exact}; 0 < nBothFrames < nRefFrames: {part_frames}; intervals: "
          f"{int(allc[:, 0].sum())} reference, {int(allc[:, 1].sum())} estimated")
    assert 4 * part_exact >= n and 4 * part_frames >= n, "the fixture would be vacuous: change the seeds / the jitter"
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
