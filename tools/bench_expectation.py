"""Device time of the posterior expectations (NeuralSemiCRFInterval.entropy / expectation / covariance) at T=1024 x 352, "randn"
inputs, in one process and by device events: entropy forward + backward, expectation under no_grad, their kernels alone
(semicrf_expectation: the two float64-state sweeps; semicrf_covariance: the stream), a bare forward_backward, and the yardstick --
what a user of the library WITHOUT these entry points can do for the same quantities: a central-difference Hessian product from
two forward_backward calls plus the elementwise combine (inexact), and a third forward_backward plus a reduction for E / H.
With --errors the device errors of every fixture (tests/golden/expect_*.npz, the metric of tests/test_expectation.py) are
measured as well.

    python tools/bench_expectation.py [--reps 10] [--errors] [--out profiles/expectation_bench.json]     event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o expect -- python tools/bench_expectation.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_expectation.py --reps 5 --warmup 2 --trace DIR/.../expect_kernel_trace.csv          kernel split (any machine)

The algorithmic bytes of entropy forward + backward are two sweep reads of the lower triangle plus one read and one write of it
in the stream, 4 * 4 B T (T+1) / 2; the fraction of 8 TB/s is those bytes over the time of the two ops."""
import argparse
import csv
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, B = 1024, 352
PEAK = 8.0e12
KERNELS = {"sweep": "expectation_sweep_kernel", "stream": "covariance_stream_kernel", "noise": "covariance_noise_kernel"}


def tri_bytes(T, B):
    return 4.0 * B * T * (T + 1) / 2


def parent_composition(CRF, s, n, h=1e-3):
    """(H, dH/dscore, dH/dnoise) with forward_backward alone: central differences of the marginals along (score, noise)."""
    _, gp, gnp = CRF.forward_backward(s * (1 + h), n * (1 + h))
    _, gm, gnm = CRF.forward_backward(s * (1 - h), n * (1 - h))
    C = (gp - gm) / (2 * h)
    Cn = (gnp - gnm) / (2 * h)
    lz, g, gn = CRF.forward_backward(s, n)
    E = (g * s).sum((0, 1)) + (gn * n).sum(0)
    return lz - E, -C, -Cn


def timed(torch, f, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for r in range(reps):
        f()
        ev[r + 1].record()
    torch.cuda.synchronize()
    return sum(ev[r].elapsed_time(ev[r + 1]) for r in range(reps)) / reps


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    s, n = synth.crf_inputs(T, B, 1234, dev, "randn")
    ones = torch.ones(B, dtype=torch.float32, device=dev)
    state = {}

    def op_expect():
        state["s"] = nsci._expect_fwd(s, n, s, n)[2]

    def op_cov():
        return nsci._expect_cov(state["s"], ones)

    if args.trace_pass:
        for _ in range(args.warmup + args.reps):
            op_expect(); op_cov()
        torch.cuda.synchronize()
        return
    sg, ng = s.clone().requires_grad_(), n.clone().requires_grad_()

    def entropy_fb():
        sg.grad = None; ng.grad = None
        CRF.entropy(sg, ng).sum().backward()

    def expectation_ng():
        with torch.no_grad():
            return CRF.expectation(s, n, s, n)

    calls = {"entropy_fwd_bwd_ms": entropy_fb, "expectation_no_grad_ms": expectation_ng,
             "parent_composition_ms": lambda: parent_composition(CRF, s, n), "forward_backward_ms": lambda: CRF.forward_backward(s, n),
             "sweeps_alpha_beta_ms": lambda: nsci._marginal_inputs(s, n), "expect_fwd_ms": op_expect, "covariance_op_ms": op_cov}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    row = dict(T=T, B=B, tri_GB=round(tri_bytes(T, B) / 1e9, 3))
    for k, f in calls.items():
        row[k] = round(timed(torch, f, args.reps), 4)
    row["expectation_op_ms"] = round(row["expect_fwd_ms"] - row["sweeps_alpha_beta_ms"], 4)     # semicrf_expectation alone
    row["entropy_over_parent"] = round(row["entropy_fwd_bwd_ms"] / row["parent_composition_ms"], 3)
    ops_ms = row["expectation_op_ms"] + row["covariance_op_ms"]
    row["ops_frac_of_8TBs"] = round(4 * tri_bytes(T, B) / (ops_ms * 1e-3) / PEAK, 4)
    # how far the inexact yardstick is from the kernels' result (the metric of tests/test_expectation.py, all chains)
    H, dS, dN = parent_composition(CRF, s, n)
    _, C, Cn = CRF.covariance(s, n, s, n)
    num = torch.maximum((dS + C).abs().amax((0, 1)), (dN + Cn).abs().amax(0))
    den = torch.maximum(C.abs().amax((0, 1)), Cn.abs().amax(0))
    row["parent_composition_err"] = float((num / den).max())
    del dS, C
    print(json.dumps(row), flush=True)
    out = {"timing": row}
    if args.errors:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        te = importlib.import_module("test_expectation")
        errs = {}
        for case in te.EDGE_CASES:
            errs[case[0]] = te._edge_fixture(case, dev)
        for case in te.LARGE_CASES:
            errs[case[0]] = te._large_fixture(case, dev, full=True)
        out["device_err_per_fixture"] = errs
        print(json.dumps(errs), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


def parse_trace(args):
    disp = {k: [] for k in KERNELS}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in KERNELS.items():
                if pat in name:
                    disp[k].append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    row = dict(T=T, B=B, tri_GB=round(tri_bytes(T, B) / 1e9, 3))
    for k, lst in disp.items():
        mine = lst[args.warmup:]
        row[k + "_us"] = round(sum(mine) / max(len(mine), 1) / 1e3, 2)
    if row["sweep_us"] and row["stream_us"]:
        row["sweep_frac_of_8TBs"] = round(2 * tri_bytes(T, B) / (row["sweep_us"] * 1e-6) / PEAK, 4)
        row["stream_frac_of_8TBs"] = round(2 * tri_bytes(T, B) / (row["stream_us"] * 1e-6) / PEAK, 4)
    print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    parse_trace(a) if a.trace else run(a)
