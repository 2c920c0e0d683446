"""Device time of the posterior summaries (NeuralSemiCRFInterval.posteriors) at the model's shapes: the alpha sweep, the beta
sweep, semicrf_posteriors (stream + epilogue + entropy kernels), the whole posteriors() call, and -- in the same run -- today's
route to the same numbers: forward_backward (the dense [T, T, B] marginals) plus the torch reductions.

    python tools/bench_posteriors.py [--reps 10] [--out FILE.json]            event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o post -- python tools/bench_posteriors.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_posteriors.py --reps 5 --warmup 2 --trace DIR/.../post_kernel_trace.csv     kernel split (any machine)

The trace pass runs semicrf_posteriors on every shape warmup + reps times in the order below and nothing else; --trace assigns
the dispatches of each kernel to the shapes in that order and prints the per-kernel mean, and for the stream kernel the bytes it
must read (the lower triangle, 4 B T (T+1) / 2) over its time, as a fraction of 8 TB/s."""
import argparse
import csv
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352), (691, 360), (691, 90), (2048, 88)]
PEAK = 8.0e12


def tri_bytes(T, B):
    return 4.0 * B * T * (T + 1) / 2


def dense_route(CRF, s, nz):
    """forward_backward + the torch reductions posteriors() replaces."""
    import torch
    T = s.shape[0]
    logz, grad, gn = CRF.forward_backward(s, nz)
    single = torch.diagonal(grad, dim1=0, dim2=1).t()
    off = grad * torch.tril(torch.ones(T, T, device=s.device), -1)[:, :, None]
    end, begin = off.sum(1), off.sum(0)
    node = torch.cat([torch.ones_like(end[:1]), gn + end[1:]], 0)
    return logz, node, begin, end, single, gn


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        lz, v, q = nsci._marginal_inputs(s, nz)

        def op():
            return nsci._posteriors_raw(s, nz, (lz, v, q))
        if args.trace_pass:
            for _ in range(args.warmup + args.reps):
                op()
            torch.cuda.synchronize()
            continue
        for _ in range(args.warmup):
            op(); nsci._marginal_inputs(s, nz); CRF.posteriors(s, nz); dense_route(CRF, s, nz)
        torch.cuda.synchronize()
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        e[0].record()
        for _ in range(args.reps):
            nsci._logz_fwd_raw(s, nz, True)
        e[1].record()
        for _ in range(args.reps):
            nsci._beta_raw(s, nz)
        e[2].record()
        for _ in range(args.reps):
            op()
        e[3].record()
        for _ in range(args.reps):
            CRF.posteriors(s, nz)
        e[4].record()
        for _ in range(args.reps):
            dense_route(CRF, s, nz)
        e[5].record()
        torch.cuda.synchronize()
        ms = [e[i].elapsed_time(e[i + 1]) / args.reps for i in range(5)]
        row = dict(T=T, B=B, tri_GB=round(tri_bytes(T, B) / 1e9, 3), alpha_ms=round(ms[0], 4), beta_ms=round(ms[1], 4),
                   posteriors_op_ms=round(ms[2], 4), posteriors_call_ms=round(ms[3], 4),
                   dense_route_ms=round(ms[4], 4), speedup_vs_dense=round(ms[4] / ms[3], 2),
                   posteriors_op_tri_frac_of_8TBs=round(tri_bytes(T, B) / (ms[2] * 1e-3) / PEAK, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    want = {"stream": "posterior_stream_kernel", "epilogue": "posterior_epilogue_kernel", "entropy": "posterior_entropy_kernel"}
    disp = {k: [] for k in want}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in want.items():
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
        row["stream_frac_of_8TBs"] = round(tri_bytes(T, B) / (row["stream_us"] * 1e-6) / PEAK, 3) if row["stream_us"] else None
        out.append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    parse_trace(a) if a.trace else run(a)
