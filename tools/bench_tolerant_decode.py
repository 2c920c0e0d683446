"""Device time of tolerance-aware marginal decoding at T = 1024 x 352, "model" inputs, threshold 0.5, tolerances (0, 0), (2, 2) and
(8, 8), two figures per tolerance from the same run:

  * semicrf_marginal_decode_tol (halo count pass + scans + gather write pass) against semicrf_marginal_decode, the tolerance-free
    call it extends, timed by device events with the two calls ALTERNATING;
  * the whole decode_mbr_packed(threshold, tolerance) call (alpha and beta sweeps, the lattice, semicrf_mbr_select, the copies
    back; host wall clock) against the route available without it: forward_backward's dense [T, T, B] marginals, a pooling pass
    over the (2 de + 1) x (2 db + 1) box and nonzero (device events; that route stops at the lattice and never selects a path).

    python tools/bench_tolerant_decode.py [--reps 10] [--tau 0.5] [--out FILE.json]      (GPU box)
"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352)]
TOLS = [(0, 0), (2, 2), (8, 8)]


def dense_route(CRF, s, nz, tau, tol):
    """forward_backward + a box sum of the dense marginals + nonzero, sorted into (chain, begin, end) order (device tensors)."""
    import torch
    T, B = s.shape[0], s.shape[2]
    db, de = tol
    _, grad, _ = CRF.forward_backward(s, nz)                 # [end, begin, chain]; zeros above the diagonal
    g = grad.permute(2, 0, 1).unsqueeze(1)                   # [B, 1, end, begin]
    M = torch.nn.functional.avg_pool2d(g, (2 * de + 1, 2 * db + 1), stride=1, padding=(de, db), divisor_override=1).squeeze(1)
    M = torch.tril(M.clamp_(max=1.0))
    idx = torch.nonzero(M >= tau)                            # rows (c, e, b)
    key = (idx[:, 0] * T + idx[:, 2]) * T + idx[:, 1]
    idx = idx[torch.argsort(key)]
    return idx[:, [2, 1]], torch.bincount(idx[:, 0], minlength=B).cumsum(0), M[idx[:, 0], idx[:, 1], idx[:, 2]]


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        lz, v, q = nsci._marginal_inputs(s, nz)
        tau = torch.full((1,), args.tau, dtype=torch.float32, device=dev)
        for tol in TOLS:
            first = nsci._marginal_decode_raw(s, nz, tau, None, (lz, v, q), tol)
            selected = int(first[1][-1])
            cap = max(selected, 1)

            def op():
                return nsci._marginal_decode_raw(s, nz, tau, cap, (lz, v, q), tol)

            def plain():
                return nsci._marginal_decode_raw(s, nz, tau, None, (lz, v, q))
            for _ in range(args.warmup):
                op(); plain(); CRF.decode_mbr_packed(s, nz, args.tau, tolerance=tol); dense_route(CRF, s, nz, args.tau, tol)
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps + 1)]
            ev[0].record()
            for r in range(args.reps):                      # alternating: plain, tolerant, plain, ...
                plain()
                ev[2 * r + 1].record()
                op()
                ev[2 * r + 2].record()
            torch.cuda.synchronize()
            plain_ms = sum(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(args.reps)) / args.reps
            op_ms = sum(ev[2 * r + 1].elapsed_time(ev[2 * r + 2]) for r in range(args.reps)) / args.reps
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            for _ in range(args.reps):
                dense_route(CRF, s, nz, args.tau, tol)
            e[1].record()
            torch.cuda.synchronize()
            dense_ms = e[0].elapsed_time(e[1]) / args.reps
            t0 = time.perf_counter()
            for _ in range(args.reps):
                out = CRF.decode_mbr_packed(s, nz, args.tau, tolerance=tol)      # host wall clock: it ends with the copies back
            call_ms = (time.perf_counter() - t0) / args.reps * 1e3
            row = dict(T=T, B=B, tau=args.tau, tol_begin=tol[0], tol_end=tol[1], lattice_cells=selected, path_intervals=int(out[1][-1]),
                       marginal_decode_op_ms=round(plain_ms, 4), marginal_decode_tol_op_ms=round(op_ms, 4),
                       ratio_to_marginal_decode=round(op_ms / plain_ms, 3), decode_mbr_packed_call_ms=round(call_ms, 4),
                       dense_route_ms=round(dense_ms, 4), speedup_vs_dense=round(dense_ms / call_ms, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--out", default="")
    run(ap.parse_args())
