"""Time and memory of the bf16 feed-forward ResBlock in TRAINING, forward + backward: the fused bf16 training route
(feedForwardBf16Train = "fused": csrc/ffn_bf16.hip in its training mode + csrc/ffn_bf16_bwd.hip) against the stock route it replaces on
IDENTICAL inputs, the two routes ALTERNATING in one process.  Form A: bfloat16 modules; form B: float32 modules under
torch.autocast(bfloat16).  The protocol is tools/bench_feed_forward_train.py's.

    python tools/bench_feed_forward_bf16_train.py [--reps 30] [--warmup 5] [--out profiles/feed_forward_bf16_train_bench.json]      (GPU box)

Steps, each in a fresh child process under its own time limit (a step that fails or hangs stops the run):
  op       a ResBlock forward + backward at D = 160, hidden = 640, p = 0.1 / 0.1, 13 261 and 53 044 tokens: form A against the stock bf16
           modules, form B against the stock fp32 modules under autocast, and form B against the fp32 fused training route (outside
           autocast); wall clock around a device synchronisation and device time between two events, medians
  kernels  the fused route's kernels one by one (torch.profiler, device durations, medians over the repetitions), both forms
  blocks   a bf16 BasicBlock [1, 89, 149, 160] and [4, ...] forward + backward, training mode, and torch.cuda.max_memory_allocated of one
           un-checkpointed forward + backward on either route
  model    the whole Backbone step at [1, 691, 229, 6], training mode, useGradientCheckpoint = True, under torch.autocast(bfloat16), the
           bf16 attention training route on in both arms; in the same run the step with the stock attention and feed-forward under
           autocast, and the fp32 fused step outside autocast (the figures the earlier sections of DESIGN.md quote, measured again)
Nothing is promised in advance: whatever comes out is written down."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STEPS = (("op", 300), ("kernels", 240), ("blocks", 240), ("model", 480))          # (name, time limit in seconds)
TOKENS = (13261, 53044)
D, HIDDEN, P = 160, 640, 0.1


def _autocast(torch, on):
    return torch.autocast("cuda", dtype=torch.bfloat16) if on else contextlib.nullcontext()


def op_case(torch, backbone, dev, ntok, form):
    """run(kind): kind = "fused" (the bf16 training route), "torch" (the stock route of the form), "fp32" (the fp32 fused training
    route outside autocast; form B's tensors)."""
    dt = torch.bfloat16 if form == "A" else torch.float32
    g = torch.Generator().manual_seed(ntok)
    x = torch.randn(ntok, D, generator=g).to(dt).to(dev).requires_grad_()
    G = torch.randn(ntok, D, generator=g).to(dt).to(dev)
    blk = backbone.ResBlock(backbone._feed_forward(D, HIDDEN, P), size=D).train()
    blk.dropout.p = P
    with torch.no_grad():
        blk.scale.fill_(1.0)                                      # LayerScale of a trained model, not the 1e-2 of initialisation
    blk = blk.to(dt).to(dev)
    blk.feedForward, blk.feedForwardTrain, blk.feedForwardBf16 = "fused", "fused", "fused"

    def run(kind):
        def f():
            blk.feedForwardBf16Train = "fused" if kind == "fused" else "torch"
            blk.zero_grad(set_to_none=True)
            x.grad = None
            with _autocast(torch, form == "B" and kind != "fp32"):
                out = blk(x)
            out.backward(G)
        return f
    return blk, run


def step_op(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import alternate, row_of
    rows = []
    for ntok in TOKENS:
        for form, others in (("A", ("torch",)), ("B", ("torch", "fp32"))):
            blk, run = op_case(torch, backbone, dev, ntok, form)
            before = dict(backbone.FEED_FORWARD_BF16_TRAIN_ROUTES)
            run("fused")()
            after = backbone.FEED_FORWARD_BF16_TRAIN_ROUTES
            assert after["fused"] == before["fused"] + 1 and after["bwd"] == before["bwd"] + 1 and after["torch"] == before["torch"]
            lib = backbone._lib.load()
            extra = {"tokens": ntok, "D": D, "hidden": HIDDEN, "p": [P, P], "form": form,
                     "saved_bytes": int(lib.semicrf_ffn_residual_bf16_train_saved_bytes(ntok, D, HIDDEN)),
                     "backward_workspace_bytes": int(lib.semicrf_ffn_residual_bf16_bwd_workspace_bytes(ntok, D, HIDDEN))}
            for other in others:
                before = dict(backbone.FEED_FORWARD_TRAIN_ROUTES), dict(backbone.FEED_FORWARD_BF16_TRAIN_ROUTES)
                run(other)()
                if other == "fp32":                               # the fp32 kernels answered, not the bf16 ones
                    assert backbone.FEED_FORWARD_TRAIN_ROUTES["bwd"] == before[0]["bwd"] + 1
                    assert backbone.FEED_FORWARD_BF16_TRAIN_ROUTES == before[1]
                wf, wt, df, dt_ = alternate(run("fused"), run(other), args.reps, args.warmup, args.inner, torch)
                against = {"torch": 'feedForwardBf16Train = "torch"' + (" (stock bf16 modules)" if form == "A" else " (stock fp32 modules under autocast)"),
                           "fp32": 'the fp32 fused training route (feedForwardTrain = "fused", outside autocast)'}[other]
                rows.append(row_of(f"ResBlock forward + backward, {ntok} tokens, form {form}", against, wf, wt, df, dt_, extra))
    return rows


def step_kernels(args, torch, backbone, dev):
    from torch.profiler import ProfilerActivity, profile
    rows = []
    for ntok in TOKENS:
        for form in ("A", "B"):
            blk, run = op_case(torch, backbone, dev, ntok, form)
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
                if "ffn" in ev.name:
                    times.setdefault(ev.name.split("(")[0], []).append(getattr(ev, "device_time", None) or getattr(ev, "cuda_time", 0.0))
            for name, ts in sorted(times.items()):
                row = {"tokens": ntok, "form": form, "kernel": name, "launches_per_step": round(len(ts) / args.reps, 2),
                       "device_us": round(statistics.median(ts), 2)}
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def train_model(torch, backbone, dev, checkpoint, dtype=None):
    from bench_feed_forward_bf16 import MODEL
    torch.manual_seed(3)
    model = backbone.Backbone(**dict(MODEL, useGradientCheckpoint=checkpoint))
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(".scale"):
                p.fill_(1.0)
    if dtype is not None:
        model = model.to(dtype)
    model = model.to(dev).train()
    model.attention, model.attentionBf16, model.attentionBf16Train = "fused-train", "fused", "fused"
    model.feedForward, model.feedForwardTrain, model.feedForwardBf16 = "fused", "fused", "fused"
    return model


def step_blocks(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import MODEL, alternate, row_of
    model = train_model(torch, backbone, dev, False, torch.bfloat16)
    blk = model.encoderLayers[0]
    rows = []
    for N in (1, 4):
        h = torch.randn(N, 89, 149, 4 * MODEL["baseSize"], device=dev).to(torch.bfloat16).requires_grad_()

        def run(kind):
            def f():
                blk.feedForwardBf16Train = kind
                blk.zero_grad(set_to_none=True)
                h.grad = None
                blk(h).float().square().sum().backward()
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
        wf, wt, df, dt_ = alternate(run("fused"), run("torch"), args.reps, args.warmup, max(args.inner // 2, 1), torch)
        rows.append(row_of(f"bf16 BasicBlock N={N} forward + backward", 'feedForwardBf16Train = "torch"', wf, wt, df, dt_,
                           {"shape": list(h.shape), "attention": "fused-train, bf16 training route", "dropoutProb": MODEL["dropoutProb"],
                            "peak_bytes_above_the_resident_set": {"fused": peak["fused"], "torch": peak["torch"]}}))
    return rows


def step_model(args, torch, backbone, dev):
    from bench_feed_forward_bf16 import alternate, row_of
    model = train_model(torch, backbone, dev, True)
    idx = torch.arange(90, device=dev)
    x = torch.randn(1, 691, 229, 6, device=dev)
    n_ff = len(model.feed_forward_blocks())

    def run(kind):
        """"fused" | "torch": the new knob under autocast; "stock": attention and feed-forward stock under autocast; "fp32": the fp32
        fused step outside autocast."""
        def f():
            model.attention = "torch" if kind == "stock" else "fused-train"
            model.feedForward = "torch" if kind == "stock" else "fused"
            model.feedForwardBf16Train = "fused" if kind == "fused" else "torch"
            model.zero_grad(set_to_none=True)
            with _autocast(torch, kind != "fp32"):
                out = model(x, idx)
            out.float().square().sum().backward()
        return f

    before = dict(backbone.FEED_FORWARD_BF16_TRAIN_ROUTES)
    run("fused")()
    after = backbone.FEED_FORWARD_BF16_TRAIN_ROUTES
    assert after["bwd"] == before["bwd"] + n_ff and after["fused"] == before["fused"] + 2 * n_ff and after["torch"] == before["torch"]
    extra = {"x": list(x.shape), "useGradientCheckpoint": True, "feed_forward_blocks": n_ff, "autocast": "bfloat16"}
    rows = []
    wf, wt, df, dt_ = alternate(run("fused"), run("torch"), args.reps, 2, 2, torch)
    rows.append(row_of("Backbone training step N=1 under autocast", 'feedForwardBf16Train = "torch" (bf16 attention training route on)', wf, wt, df,
                       dt_, extra))
    wf, wt, df, dt_ = alternate(run("fused"), run("stock"), args.reps, 2, 2, torch)
    rows.append(row_of("Backbone training step N=1 under autocast", "stock attention and feed-forward under autocast", wf, wt, df, dt_, extra))
    wf, wt, df, dt_ = alternate(run("fused"), run("fp32"), args.reps, 2, 2, torch)
    rows.append(row_of("Backbone training step N=1 under autocast", "the fp32 fused step outside autocast (fused-train, feedForwardTrain)", wf, wt,
                       df, dt_, extra))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_forward_bf16_train_bench.json"))
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
