"""Time of the bf16 feed-forward ResBlock (backbone.feed_forward_residual with bf16 = "fused", csrc/ffn_bf16.hip) against the stock
routes it replaces, on IDENTICAL inputs, the routes ALTERNATING in one process.

    python tools/bench_feed_forward_bf16.py [--reps 30] [--warmup 5] [--out profiles/feed_forward_bf16_bench.json]          (GPU box)

Steps, each a child process of its own under its own time limit (the first that fails ends the run):
  op      form A (bf16 tensors) against the stock bf16 expression and against the fp32 fused op on the same values, and form B (fp32
          tensors under bfloat16 autocast) against the stock block under autocast, at the model's shape (D = 160, hidden = 640) for
          13 261 tokens (one segment) and 53 044; the stock route's count of dispatched non-view ops per block
  blocks  one bf16 BasicBlock forward at [N, 89, 149, 160], N = 1 and 4, attention and attentionBf16 fused in both arms, feedForward =
          "fused", feedForwardBf16 "fused" against "torch"
  model   the bf16 Backbone forward at [1, 691, 229, 6] (the model's configuration, 90 output indices), likewise
Per case: the wall clock per call around a device synchronisation and the device time between two events around `inner` back-to-back
calls, medians over the repetitions.  For the op also the fraction of the bf16 matrix rate (2.5 PFLOP/s; 4 D hidden operations per
token) and of the HBM bandwidth (8 TB/s; x read once, out written once) that its device time amounts to.  Nothing is promised in
advance: whatever comes out is written down."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_MATRIX = 2.5e15
PEAK_HBM = 8.0e12
STEPS = (("op", 240), ("blocks", 240), ("model", 300))          # (name, time limit in seconds)
MODEL = dict(inputSize=6, baseSize=40, posEmbedInitGamma=1, nHead=4, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4,
             dropoutProb=0.1, nLayers=6, enabledAttn=["F", "T"], useGradientCheckpoint=False, downsampleF=True)
VIEW_OPS = {"view", "_unsafe_view", "reshape", "transpose", "t", "permute", "expand", "unsqueeze", "squeeze", "as_strided", "slice", "select",
            "detach", "alias", "unbind", "split", "chunk"}


def alternate(fa, fb, reps, warmup, inner, torch):
    """(wall a, wall b, device a, device b) in seconds per call, medians.  The first call after the event pair of the repetition
    before is slow on the host, whichever route it is (measured on a BasicBlock: 0.85 ms where the same call takes 0.54 ms in a
    plain loop): a call that is not timed takes that place, and which route goes first changes from one repetition to the next."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    wall, devt = ([], []), ([], [])
    for rep in range(reps):
        order = ((0, fa), (1, fb)) if rep % 2 == 0 else ((1, fb), (0, fa))
        order[1][1]()
        torch.cuda.synchronize()
        for i, f in order:
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[i].append(time.perf_counter() - t0)
        for i, f in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            devt[i].append(e0.elapsed_time(e1) * 1e-3 / inner)
    return tuple(statistics.median(x) for x in wall + devt)


def row_of(tag, other, wf, wt, df, dt, extra):
    row = {"case": tag, "against": other, "fused_wall_ms": round(wf * 1e3, 4), "other_wall_ms": round(wt * 1e3, 4),
           "fused_device_ms": round(df * 1e3, 4), "other_device_ms": round(dt * 1e3, 4), "ratio_other_over_fused_wall": round(wt / wf, 2),
           "ratio_other_over_fused_device": round(dt / df, 2)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def dispatched_ops(fn, torch):
    """The non-view ops a call dispatches: the stock route's launches, counted where they are asked for."""
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.names = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.overloadpacket.__name__
            if name not in VIEW_OPS:
                self.names.append(name)
            return func(*args, **(kwargs or {}))

    with Count() as c:
        fn()
    return c.names


def step_op(args, torch, backbone, dev):
    rows = []
    Tp, Fp, D, hidden = 89, 149, 160, 640
    BF16 = torch.bfloat16
    for N in (1, 4):
        g = torch.Generator().manual_seed(100 + N)
        x = torch.randn(N, Tp, Fp, D, generator=g).to(dev)
        p32 = [(torch.randn(hidden, D, generator=g) / D ** 0.5).to(dev), (torch.randn(hidden, generator=g) * 0.5).to(dev),
               (torch.randn(D, hidden, generator=g) / hidden ** 0.5).to(dev), (torch.randn(D, generator=g) * 0.5).to(dev),
               torch.randn(D, generator=g).to(dev)]
        x16, p16 = x.to(BF16), [p.to(BF16) for p in p32]
        xr, pr = x16.float(), [p.float() for p in p16]              # the fp32 fused op on the values form A sees
        tokens = N * Tp * Fp
        flop = 4.0 * tokens * D * hidden

        def extra(nbytes, df, diff, names=None):
            e = {"tokens": tokens, "D": D, "hidden": hidden, "gflop": round(flop * 1e-9, 3), "mbyte": round(nbytes * 1e-6, 3),
                 "fused_fraction_of_bf16_matrix_peak": round(flop / df / PEAK_BF16_MATRIX, 4),
                 "fused_fraction_of_hbm_bandwidth": round(nbytes / df / PEAK_HBM, 4), "max_abs_difference_between_routes": diff}
            if names is not None:
                e["other_dispatched_ops"] = len(names)
                e["other_ops"] = names
            return e

        form_a = lambda: backbone.feed_forward_residual(x16, *p16, route="fused", bf16="fused")
        stock_a = lambda: backbone.feed_forward_residual(x16, *p16, route="torch")
        fp32_op = lambda: backbone.feed_forward_residual(xr, *pr, route="fused")
        before = backbone.FEED_FORWARD_BF16_ROUTES["fused"]
        diff = float((form_a().float() - stock_a().float()).abs().max())
        assert backbone.FEED_FORWARD_BF16_ROUTES["fused"] == before + 1 and diff < 0.25, diff
        wf, wt, df, dt = alternate(form_a, stock_a, args.reps, args.warmup, args.inner, torch)
        rows.append(row_of(f"form A N={N}", "stock bf16 expression", wf, wt, df, dt, extra(2.0 * 2 * tokens * D, df, diff,
                                                                                           dispatched_ops(stock_a, torch))))
        diff = float((form_a().float() - fp32_op()).abs().max())
        wf, wt, df, dt = alternate(form_a, fp32_op, args.reps, args.warmup, args.inner, torch)
        rows.append(row_of(f"form A N={N}", "fp32 fused op (semicrf_ffn_residual)", wf, wt, df, dt, extra(2.0 * 2 * tokens * D, df, diff)))

        def under_autocast(fn):
            def run():
                with torch.autocast("cuda", dtype=BF16):
                    return fn()
            return run
        form_b = under_autocast(lambda: backbone.feed_forward_residual(x, *p32, route="fused", bf16="fused"))
        stock_b = under_autocast(lambda: backbone.feed_forward_residual(x, *p32, route="torch"))
        before = backbone.FEED_FORWARD_BF16_ROUTES["fused"]
        diff = float((form_b() - stock_b().float()).abs().max())
        assert backbone.FEED_FORWARD_BF16_ROUTES["fused"] == before + 1 and diff < 0.25, diff
        wf, wt, df, dt = alternate(form_b, stock_b, args.reps, args.warmup, args.inner, torch)
        rows.append(row_of(f"form B N={N}", "stock expression under bfloat16 autocast", wf, wt, df, dt,
                           extra(2.0 * 4 * tokens * D, df, diff, dispatched_ops(stock_b, torch))))
    return rows


def bf16_model(torch, backbone, dev):
    torch.manual_seed(11)
    model = backbone.Backbone(**MODEL).eval()
    with torch.no_grad():
        for name, p in model.named_parameters():                  # LayerScale of a trained model, not the 1e-2 of initialisation
            if name.endswith(".scale"):
                p.fill_(1.0)
    model = model.to(torch.bfloat16).to(dev)
    model.attention, model.attentionBf16, model.feedForward = "fused", "fused", "fused"
    return model


def with_kind(m, kind, fn):
    def run():
        m.feedForwardBf16 = kind
        return fn()
    return run


def step_blocks(args, torch, backbone, dev):
    model = bf16_model(torch, backbone, dev)
    blk = model.encoderLayers[0]
    rows = []
    for N in (1, 4):
        h = torch.randn(N, 89, 149, 4 * MODEL["baseSize"], device=dev).to(torch.bfloat16)
        fa, fb = with_kind(blk, "fused", lambda: blk(h)), with_kind(blk, "torch", lambda: blk(h))
        before = dict(backbone.FEED_FORWARD_BF16_ROUTES)
        diff = float((fa().float() - fb().float()).abs().max())
        assert backbone.FEED_FORWARD_BF16_ROUTES == {"fused": before["fused"] + 2, "torch": before["torch"]}
        wf, wt, df, dt = alternate(fa, fb, args.reps, args.warmup, max(args.inner // 2, 1), torch)
        rows.append(row_of(f"bf16 BasicBlock N={N}", 'feedForwardBf16 = "torch"', wf, wt, df, dt,
                           {"shape": list(h.shape), "attention": "fused", "attentionBf16": "fused", "max_abs_difference_between_routes": diff}))
    return rows


def step_model(args, torch, backbone, dev):
    model = bf16_model(torch, backbone, dev)
    idx = torch.arange(90, device=dev)
    x = torch.randn(1, 691, 229, 6, device=dev).to(torch.bfloat16)
    fa, fb = with_kind(model, "fused", lambda: model(x, idx)), with_kind(model, "torch", lambda: model(x, idx))
    a, t = fa(), fb()
    diff = float((a.float() - t.float()).abs().max())
    wf, wt, df, dt = alternate(fa, fb, args.reps, 2, 2, torch)
    return [row_of("bf16 Backbone N=1", 'feedForwardBf16 = "torch"', wf, wt, df, dt,
                   {"x": list(x.shape), "ctx": list(a.shape), "attention": "fused", "attentionBf16": "fused",
                    "max_abs_difference_between_routes": diff})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_forward_bf16_bench.json"))
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="run one step in this process and print its rows as one JSON line")
    args = ap.parse_args()
    if args.step:
        import torch
        from transkun_amd import backbone
        dev = torch.device("cuda:0")
        with torch.no_grad():
            rows = {"op": step_op, "blocks": step_blocks, "model": step_model}[args.step](args, torch, backbone, dev)
        print("ROWS " + json.dumps({"device": torch.cuda.get_device_name(0), "rows": rows}), flush=True)
        return 0
    res = {"reps": args.reps, "warmup": args.warmup, "inner": args.inner,
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
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
