"""Time and memory of the feed-forward ResBlock in TRAINING, forward + backward: the fused training route (feedForwardTrain = "fused":
csrc/ffn.hip in its training mode + csrc/ffn_bwd.hip) against the stock route it replaces (about ten stock forward launches, two
dropouts and their autograd) on IDENTICAL inputs, the two routes ALTERNATING in one process.

    python tools/bench_feed_forward_train.py [--reps 30] [--warmup 5] [--out profiles/feed_forward_train_bench.json]      (GPU box)

Steps, each in a fresh child process under its own time limit (a step that fails or hangs stops the run):
  op       feed_forward_residual forward + backward at D = 160, hidden = 640, p = 0.1 / 0.1, 13 261 and 53 044 tokens: wall clock around
           a device synchronisation and device time between two events, medians; the fraction of the fp32 matrix rate (157.3 TFLOP/s)
           that the fused route's device time amounts to (6 x 2 x tokens x D x hidden operations: each product once forward, twice backward)
  kernels  the fused route's kernels one by one (torch.profiler, device durations, medians over the repetitions) at both token counts
  blocks   BasicBlock [1, 89, 149, 160] and [4, ...] forward + backward, training mode, and torch.cuda.max_memory_allocated of one
           un-checkpointed forward + backward on either route
  model    the whole Backbone step at [1, 691, 229, 6]: training mode, useGradientCheckpoint = True, attention = "fused-train" in
           both arms
Nothing is promised in advance: whatever comes out is written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS = (("op", 240), ("kernels", 240), ("blocks", 240), ("model", 420))          # (name, time limit in seconds)
TOKENS = (13261, 53044)
D, HIDDEN, P = 160, 640, 0.1
PEAK_FP32_MATRIX = 157.3e12


def op_case(torch, backbone, dev, ntok):
    g = torch.Generator().manual_seed(ntok)
    x = torch.randn(ntok, D, generator=g).to(dev).requires_grad_()
    G = torch.randn(ntok, D, generator=g).to(dev)
    blk = backbone.ResBlock(backbone._feed_forward(D, HIDDEN, P), size=D).to(dev).train()
    blk.dropout.p = P
    with torch.no_grad():
        blk.scale.fill_(1.0)                                      # LayerScale of a trained model, not the 1e-2 of initialisation
    blk.feedForward = "fused"

    def run(kind):
        def f():
            blk.feedForwardTrain = kind
            blk.zero_grad(set_to_none=True)
            x.grad = None
            blk(x).backward(G)
        return f
    return blk, run


def step_op(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import alternate, row_of
    rows = []
    for ntok in TOKENS:
        blk, run = op_case(torch, backbone, dev, ntok)
        before = dict(backbone.FEED_FORWARD_TRAIN_ROUTES)
        run("fused")()
        assert backbone.FEED_FORWARD_TRAIN_ROUTES["fused"] == before["fused"] + 1 and backbone.FEED_FORWARD_TRAIN_ROUTES["bwd"] == before["bwd"] + 1
        wf, wt, df, dt = alternate(run("fused"), run("torch"), args.reps, args.warmup, args.inner, torch)
        flop = 6.0 * 2.0 * ntok * D * HIDDEN
        ws = int(backbone._lib.load().semicrf_ffn_residual_bwd_workspace_bytes(ntok, D, HIDDEN))
        rows.append(row_of(f"ResBlock forward + backward, {ntok} tokens", 'feedForwardTrain = "torch"', wf, wt, df, dt,
                           {"tokens": ntok, "D": D, "hidden": HIDDEN, "p": [P, P], "gflop": round(flop * 1e-9, 2),
                            "fused_fraction_of_fp32_matrix_peak": round(flop / df / PEAK_FP32_MATRIX, 4),
                            "other_fraction_of_fp32_matrix_peak": round(flop / dt / PEAK_FP32_MATRIX, 4), "backward_workspace_bytes": ws}))
    return rows


def step_kernels(args, torch, backbone, dev):
    from torch.profiler import ProfilerActivity, profile
    rows = []
    for ntok in TOKENS:
        blk, run = op_case(torch, backbone, dev, ntok)
        f = run("fused")
        for _ in range(args.warmup):
            f()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(args.reps):
                f()
            torch.cuda.synchronize()
        times = {}
        for ev in prof.events():
            if "ffn_" in ev.name:
                times.setdefault(ev.name.split("(")[0], []).append(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0))
        flops = {"rowgemm": 2.0 * ntok * D * HIDDEN, "colgemm": 2.0 * ntok * D * HIDDEN, "ffn_residual_kernel": 4.0 * ntok * D * HIDDEN}
        for name, ts in sorted(times.items()):
            us = statistics.median(ts)
            row = {"tokens": ntok, "kernel": name, "launches_per_step": round(len(ts) / args.reps, 2), "device_us": round(us, 2)}
            for key, fl in flops.items():
                if key in name:
                    row["fraction_of_fp32_matrix_peak"] = round(fl / (us * 1e-6) / PEAK_FP32_MATRIX, 4)
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def train_model(torch, backbone, dev, checkpoint):
    from bench_feed_forward_bf16 import MODEL
    torch.manual_seed(3)
    model = backbone.Backbone(**dict(MODEL, useGradientCheckpoint=checkpoint))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".scale"):
                p.fill_(1.0)
    model = model.to(dev).train()
    model.attention, model.feedForward = "fused-train", "fused"
    return model


def step_blocks(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import MODEL, alternate, row_of
    model = train_model(torch, backbone, dev, False)
    blk = model.encoderLayers[0]
    rows = []
    for N in (1, 4):
        h = torch.randn(N, 89, 149, 4 * MODEL["baseSize"], device=dev).requires_grad_()

        def run(kind):
            def f():
                blk.feedForwardTrain = kind
                blk.zero_grad(set_to_none=True)
                h.grad = None
                blk(h).square().sum().backward()
            return f

        peak = {}
        for kind in ("fused", "torch"):
            run(kind)()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            run(kind)()
            torch.cuda.synchronize()
            peak[kind] = torch.cuda.max_memory_allocated() - base
        wf, wt, df, dt = alternate(run("fused"), run("torch"), args.reps, args.warmup, max(args.inner // 2, 1), torch)
        rows.append(row_of(f"BasicBlock N={N} forward + backward", 'feedForwardTrain = "torch"', wf, wt, df, dt,
                           {"shape": list(h.shape), "attention": "fused-train", "dropoutProb": MODEL["dropoutProb"],
                            "peak_bytes_above_the_resident_set": {"fused": peak["fused"], "torch": peak["torch"]}}))
    return rows


def step_model(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import alternate, row_of
    model = train_model(torch, backbone, dev, True)
    idx = torch.arange(90, device=dev)
    x = torch.randn(1, 691, 229, 6, device=dev)

    def run(kind):
        def f():
            model.feedForwardTrain = kind
            model.zero_grad(set_to_none=True)
            model(x, idx).square().sum().backward()
        return f

    before = dict(backbone.FEED_FORWARD_TRAIN_ROUTES)
    run("fused")()
    n_ff = len(model.feed_forward_blocks())
    assert backbone.FEED_FORWARD_TRAIN_ROUTES["bwd"] == before["bwd"] + n_ff and backbone.FEED_FORWARD_TRAIN_ROUTES["torch"] == before["torch"]
    wf, wt, df, dt = alternate(run("fused"), run("torch"), args.reps, 2, 2, torch)
    return [row_of("Backbone training step N=1", 'feedForwardTrain = "torch"', wf, wt, df, dt,
                   {"x": list(x.shape), "attention": "fused-train", "useGradientCheckpoint": True, "feed_forward_blocks": n_ff})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_forward_train_bench.json"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process and print its rows as one JSON line")
    args = ap.parse_args()
    if args.step:
        import torch
        from transkun_amd import backbone
        dev = torch.device("cuda:0")
        rows = {"op": step_op, "kernels": step_kernels, "blocks": step_blocks, "model": step_model}[args.step](args, torch, backbone, dev)
        print("ROWS " + json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}), flush=True)
        return 0
    res = {"reps": args.reps, "warmup": args.warmup, "inner": args.inner,
           "unit": "ms per forward + backward, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    for step, limit in STEPS:                                     # a fresh process per step, each under its own limit; stop at the first failure
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--inner", str(args.inner)]
        try:
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {limit} s; stopping", file=sys.stderr)
            return 124
        sys.stdout.write(done.stdout)
        if done.returncode != 0:
            print(f"step {step}: exit status {done.returncode}; stopping", file=sys.stderr)
            return done.returncode
        got = json.loads([line for line in done.stdout.splitlines() if line.startswith("ROWS ")][-1][5:])
        res["device"] = got["device"]
        res[step] = got["rows"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
