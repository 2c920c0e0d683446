#!/usr/bin/env python3
"""Generate tests/golden/expect_*.npz: the float64 truth of the posterior expectations (NeuralSemiCRFInterval.expectation /
entropy / covariance), obtained by differentiating the REFERENCE's own computeLogZ twice in float64.

Run where the reference checkout is available: `PYTHONDONTWRITEBYTECODE=1 python tools/make_expectation_golden.py --ref DIR`.
The fixtures hold arrays only.  Inputs are regenerated from seeds (transkun_amd.synth: exact integer hash, same bits everywhere):
scores as tests/conftest.py:edge_inputs / CASES below, the random weighting as `weights()` below.

For W(path) = sum weight[e,b] over the path's intervals + sum noiseWeight[t] over its noise gaps,
    g = d logZ / d(score, noise)  (the marginals),   E = <g, (weight, noiseWeight)>,   (C, Cn) = dE / d(score, noise)
with create_graph on the first differentiation.  Two weightings per fixture: "s" (weight = score, noiseWeight = noise: E_p[S],
H = logZ - E) and "r" (seeded random).  Every case also records err_ref_fp32: the error of the same double backward run in
float32 (the reference's own precision) under the metric of tests/test_expectation.py -- information only.

Small cases (the twelve edge cases) store C densely as its packed lower triangle (rows e, columns b <= e).  The larger shapes run
the reference on a seeded subset of 8 chains (chains are independent) and store E, H, Cn, the row and column sums of C and the
per-chain maximum in full, and C itself at 16384 seeded (e, b, chain) cells.

The covariance arrays are rounded to 36 mantissa bits (relative 1.5e-11, six orders below the tests' bound) so that the
compressed files stay below 1 MiB; E and H are stored as computed.
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from transkun_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# name, T, B, kind, seed: the larger shapes (must match tests/test_expectation.py LARGE_CASES)
LARGE_CASES = [
    ("T256_B90_model", 256, 90, "model", 131),
    ("T256_B90_randn", 256, 90, "randn", 132),
    ("T1024_B88_randn", 1024, 88, "randn", 133),
]
NSUB = 8
NCELLS = 16384


def weights(T, B, seed):
    """The seeded random weighting of a case: (weight [T,T,B], noiseWeight [T-1,B]), float32."""
    w, wn = synth.crf_inputs(T, B, seed + 7919, "cpu", "randn")
    return w.contiguous(), wn.contiguous()


def subset_chains(B, seed):
    return np.sort(np.random.RandomState(seed).permutation(B)[:NSUB]).astype(np.int64)


def sample_cells(T, n, seed):
    """n seeded (e, b, k) triples, b <= e, k < NSUB."""
    rs = np.random.RandomState(seed + 1)
    e = rs.randint(0, T, size=n)
    b = (rs.random_sample(n) * (e + 1)).astype(np.int64)
    k = rs.randint(0, NSUB, size=n)
    return e.astype(np.int64), np.minimum(b, e), k.astype(np.int64)


def chop(x):
    """float64 rounded to 36 mantissa bits (the low 16 bits zero)."""
    a = np.ascontiguousarray(x, np.float64).copy()
    u = a.view(np.uint64)
    u += np.uint64(1 << 15)
    u &= ~np.uint64(0xFFFF)
    return a


def double_backward(logz_fn, s, n, w, wn):
    """(logZ, E, C, Cn) in the dtype of s, by differentiating logz_fn twice."""
    s = s.clone().requires_grad_()
    n = n.clone().requires_grad_()
    with torch.jit.optimized_execution(False):      # plain autograd through the scripted ops: the optimised graphs of the
        lz = logz_fn(s, n)                          # profiling executor are not differentiated twice reliably (seen at T = 2)
    T = s.shape[0]
    if T == 1:
        (gs,) = torch.autograd.grad(lz.sum(), [s], create_graph=True)
        E = (gs * w).sum((0, 1))
        (C,) = torch.autograd.grad(E.sum(), [s])
        return lz.detach(), E.detach(), C, torch.zeros_like(n)
    gs, gn = torch.autograd.grad(lz.sum(), [s, n], create_graph=True)
    E = (gs * w).sum((0, 1)) + (gn * wn).sum(0)
    C, Cn = torch.autograd.grad(E.sum(), [s, n])
    return lz.detach(), E.detach(), C, Cn


def metric(C, Cn, C64, Cn64, w, wn):
    """max|X - X64| / max(max|X64|, 1e-3 max|w|) per chain over C and Cn together; the worst chain."""
    num = (C - C64).abs().amax((0, 1))
    den = C64.abs().amax((0, 1))
    mw = w.abs().amax((0, 1))
    if Cn.numel():
        num = torch.maximum(num, (Cn - Cn64).abs().amax(0))
        den = torch.maximum(den, Cn64.abs().amax(0))
        mw = torch.maximum(mw, wn.abs().amax(0))
    return float((num / torch.maximum(den, 1e-3 * mw)).max())


def run(logz_fn, s, n, wr, wnr):
    """Both weightings of one (score, noise) [float32]: dict of float64 torch tensors + err_ref_fp32 [2]."""
    low = torch.tril(torch.ones(s.shape[0], s.shape[0], dtype=torch.bool))[:, :, None]
    out, errs = {}, []
    for tag, w, wn in (("s", s, n), ("r", wr, wnr)):
        w = torch.where(low, w, torch.zeros_like(w))                 # the upper triangle is never read
        lz, E, C, Cn = double_backward(logz_fn, s.double(), n.double(), w.double(), wn.double())
        _, _, C32, Cn32 = double_backward(logz_fn, s, n, w, wn)
        errs.append(metric(C32.double(), Cn32.double(), C, Cn, w.double(), wn.double()))
        out["E_" + tag], out["C_" + tag], out["Cn_" + tag] = E, C, Cn
        if tag == "s":
            out["logZ"], out["H"] = lz, lz - E
    out["err_ref_fp32"] = torch.tensor(errs, dtype=torch.float64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("TRANSKUN_REFERENCE"), required="TRANSKUN_REFERENCE" not in os.environ,
                    help="checkout of the reference (default: $TRANSKUN_REFERENCE)")
    ap.add_argument("--only", default=None, help="substring of the case names to write")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.ref, "transkun"))
    sys.path.insert(0, args.ref)
    refmod = importlib.import_module("CRF.NeuralSemiCRFInterval")     # the reference package, imported at run time
    logz_fn = refmod.computeLogZ
    from conftest import EDGE_CASES, edge_inputs

    for name, T, B, kind, seed, tr in EDGE_CASES:
        if args.only and args.only not in name:
            continue
        s, n = edge_inputs(T, B, kind, seed, tr)
        wr, wnr = weights(T, B, seed)
        r = run(logz_fn, s, n, wr, wnr)
        ee, bb = np.tril_indices(T)
        arrays = {"logZ": r["logZ"].numpy(), "H": r["H"].numpy(), "err_ref_fp32": r["err_ref_fp32"].numpy()}
        for tag in ("s", "r"):
            arrays["E_" + tag] = r["E_" + tag].numpy()
            arrays["Ctril_" + tag] = chop(r["C_" + tag].numpy()[ee, bb])           # [T (T+1) / 2, B], rows e then b <= e
            arrays["Cn_" + tag] = chop(r["Cn_" + tag].numpy())
            assert float(torch.triu(r["C_" + tag].permute(2, 0, 1), 1).abs().max()) == 0.0
        path = os.path.join(OUT, f"expect_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(name, "err_ref_fp32", arrays["err_ref_fp32"], os.path.getsize(path), "bytes", flush=True)

    for name, T, B, kind, seed in LARGE_CASES:
        if args.only and args.only not in name:
            continue
        s, n = synth.crf_inputs(T, B, seed, "cpu", kind)
        wr, wnr = weights(T, B, seed)
        ch = subset_chains(B, seed)
        ce, cb, ck = sample_cells(T, NCELLS, seed)
        r = run(logz_fn, s[:, :, ch].contiguous(), n[:, ch].contiguous(), wr[:, :, ch].contiguous(), wnr[:, ch].contiguous())
        arrays = {"chains": ch, "cell_e": ce, "cell_b": cb, "cell_k": ck, "logZ": r["logZ"].numpy(), "H": r["H"].numpy(),
                  "err_ref_fp32": r["err_ref_fp32"].numpy()}
        for tag in ("s", "r"):
            C = r["C_" + tag].numpy()
            arrays["E_" + tag] = r["E_" + tag].numpy()
            arrays["Cn_" + tag] = chop(r["Cn_" + tag].numpy())
            arrays["rowsum_" + tag] = chop(C.sum(1))                                # [T, NSUB]: sum over b of C[e, b]
            arrays["colsum_" + tag] = chop(C.sum(0))                                # [T, NSUB]: sum over e of C[e, b]
            arrays["cmax_" + tag] = np.abs(C).max((0, 1))                           # [NSUB]
            arrays["cells_" + tag] = chop(C[ce, cb, ck])
        path = os.path.join(OUT, f"expect_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(name, "err_ref_fp32", arrays["err_ref_fp32"], os.path.getsize(path), "bytes", flush=True)


if __name__ == "__main__":
    main()
