"""Device time of marginal-threshold decoding (NeuralSemiCRFInterval.decode_marginal_packed) at the model's shapes, "model"
inputs, threshold 0.5: semicrf_marginal_decode (count + scans + write kernels) against its yardstick semicrf_posteriors -- the
same bytes and the same exponential per cell -- timed by device events in the same run, the two calls ALTERNATING; the whole
decode_marginal_packed call (alpha and beta sweeps, the decode, the copies back); and today's route to the same set:
forward_backward (the dense [T, T, B] marginals) + nonzero + the sort into (chain, begin, end) order.

    python tools/bench_marginal_decode.py [--reps 10] [--tau 0.5] [--out FILE.json]      event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mdec -- python tools/bench_marginal_decode.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_marginal_decode.py --reps 5 --warmup 2 --trace DIR/.../mdec_kernel_trace.csv      kernel split (any machine)

The trace pass runs semicrf_marginal_decode on every shape warmup + reps times in the order below and nothing else; --trace
assigns the dispatches of each kernel to the shapes in that order and prints the per-kernel mean, and for the count kernel the
bytes it must read (the lower triangle, 4 B T (T+1) / 2) over its time, as a fraction of 8 TB/s."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352), (691, 360), (691, 90), (2048, 88)]
PEAK = 8.0e12
KERNELS = {"count": "mdec_count_kernel", "colscan": "mdec_colscan_kernel", "rowscan": "mdec_rowscan_kernel",
           "offsets": "mdec_offsets_kernel", "write": "mdec_write_kernel"}


def tri_bytes(T, B):
    return 4.0 * B * T * (T + 1) / 2


def dense_route(CRF, s, nz, tau):
    """forward_backward + nonzero + the sort decode_marginal_packed replaces (device tensors; no copy back)."""
    import torch
    T, B = s.shape[0], s.shape[2]
    _, grad, _ = CRF.forward_backward(s, nz)
    idx = torch.nonzero(grad >= tau)                      # rows (e, b, c), ascending by (e, b, c)
    key = (idx[:, 2] * T + idx[:, 1]) * T + idx[:, 0]
    order = torch.argsort(key)
    idx = idx[order]
    return idx[:, 1:3].flip(1), torch.bincount(idx[:, 2], minlength=B).cumsum(0), grad[idx[:, 0], idx[:, 1], idx[:, 2]]


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

        def op():
            return nsci._marginal_decode_raw(s, nz, tau, None, (lz, v, q))

        def post():
            return nsci._posteriors_raw(s, nz, (lz, v, q))
        if args.trace_pass:
            for _ in range(args.warmup + args.reps):
                op()
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            op(); post(); CRF.decode_marginal_packed(s, nz, args.tau); dense_route(CRF, s, nz, args.tau)
        torch.cuda.synchronize()
        selected = int(op()[1][-1])
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps + 1)]
        ev[0].record()
        for r in range(args.reps):                          # alternating: posteriors, decode, posteriors, ...
            post()
            ev[2 * r + 1].record()
            op()
            ev[2 * r + 2].record()
        torch.cuda.synchronize()
        post_ms = sum(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(args.reps)) / args.reps
        op_ms = sum(ev[2 * r + 1].elapsed_time(ev[2 * r + 2]) for r in range(args.reps)) / args.reps
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record()
        for _ in range(args.reps):
            dense_route(CRF, s, nz, args.tau)
        e[1].record()
        torch.cuda.synchronize()
        dense_ms = e[0].elapsed_time(e[1]) / args.reps
        t0 = time.perf_counter()
        for _ in range(args.reps):
            CRF.decode_marginal_packed(s, nz, args.tau)     # host wall clock: it ends with the copies back
        call_ms = (time.perf_counter() - t0) / args.reps * 1e3
        row = dict(T=T, B=B, tau=args.tau, selected=selected, tri_GB=round(tri_bytes(T, B) / 1e9, 3),
                   posteriors_op_ms=round(post_ms, 4), marginal_decode_op_ms=round(op_ms, 4),
                   ratio_to_posteriors=round(op_ms / post_ms, 3), decode_marginal_packed_call_ms=round(call_ms, 4),
                   dense_route_ms=round(dense_ms, 4), speedup_vs_dense=round(dense_ms / call_ms, 2),
                   marginal_decode_op_tri_frac_of_8TBs=round(tri_bytes(T, B) / (op_ms * 1e-3) / PEAK, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    disp = {k: [] for k in KERNELS}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in KERNELS.items():
                if pat in name:
                    disp[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = args.warmup + args.reps
    out = []
    for i, (T, B) in enumerate(SHAPES):
        row = dict(T=T, B=B, tri_GB=round(tri_bytes(T, B) / 1e9, 3))
        for k, lst in disp.items():
            lst.sort()
            mine = lst[i * per:(i + 1) * per][args.warmup:]
            row[k + "_us"] = round(sum(e - s for s, e in mine) / max(len(mine), 1) / 1e3, 2)
        row["count_frac_of_8TBs"] = round(tri_bytes(T, B) / (row["count_us"] * 1e-6) / PEAK, 3) if row["count_us"] else None
        out.append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tau", type=float, default=0.5)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    parse_trace(a) if a.trace else run(a)
