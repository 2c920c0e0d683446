"""Time of the backbone's fused feed-forward ResBlock (backbone.feed_forward_residual, csrc/ffn.hip) against the stock route it
replaces (backbone.feed_forward_torch: RMSNorm, Linear, GELU, Linear, LayerScale and the residual addition as eager ops) on IDENTICAL
inputs, the two routes ALTERNATING in one process.

    python tools/bench_feed_forward.py [--reps 30] [--warmup 5] [--out profiles/feed_forward_bench.json]          (GPU box)

Cases: the op at the model's shape (one segment is 89 x 149 = 13 261 tokens of width 160, 640 hidden columns) at N = 1 and 4; one
BasicBlock forward at [N, 89, 149, 160] (N = 1, 4) and the whole Backbone forward at [1, 691, 229, 6] (the model's configuration, 90
output indices), both with attention = "fused" and feedForward "fused" against "torch".  Per case: the wall clock per call around a
device synchronisation and the device time between two events around `inner` back-to-back calls, medians over the repetitions.  For
the op also the fraction of the fp32 matrix rate (157.3 TFLOP/s; 4 D hidden operations per token) and of the HBM bandwidth (8 TB/s;
x read once, out written once) that its device time amounts to.  Nothing is promised in advance: whatever comes out is written down."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX = 157.3e12
PEAK_HBM = 8.0e12
MODEL = dict(inputSize=6, baseSize=40, posEmbedInitGamma=1, nHead=4, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4,
             dropoutProb=0.1, nLayers=6, enabledAttn=["F", "T"], useGradientCheckpoint=False, downsampleF=True)


def alternate(fa, fb, reps, warmup, inner, torch):
    """(wall a, wall b, device a, device b) in seconds per call, medians."""
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    wall, devt = ([], []), ([], [])
    for _ in range(reps):
        for i, f in enumerate((fa, fb)):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[i].append(time.perf_counter() - t0)
        for i, f in enumerate((fa, fb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            devt[i].append(e0.elapsed_time(e1) * 1e-3 / inner)
    return tuple(statistics.median(x) for x in wall + devt)


def row_of(tag, wf, wt, df, dt, extra):
    row = {"case": tag, "fused_wall_ms": round(wf * 1e3, 4), "torch_route_wall_ms": round(wt * 1e3, 4), "fused_device_ms": round(df * 1e3, 4),
           "torch_route_device_ms": round(dt * 1e3, 4), "ratio_torch_over_fused_wall": round(wt / wf, 2),
           "ratio_torch_over_fused_device": round(dt / df, 2)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "feed_forward_bench.json"))
    ap.add_argument("--no-modules", action="store_true", help="skip the BasicBlock and Backbone parts")
    args = ap.parse_args()
    import torch
    from transkun_amd import backbone
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    Tp, Fp, D, hidden = 89, 149, 160, 640
    with torch.no_grad():
        for N in (1, 4):
            g = torch.Generator().manual_seed(100 + N)
            x = torch.randn(N, Tp, Fp, D, generator=g).to(dev)
            w1, b1 = (torch.randn(hidden, D, generator=g) / D ** 0.5).to(dev), (torch.randn(hidden, generator=g) * 0.5).to(dev)
            w2, b2 = (torch.randn(D, hidden, generator=g) / hidden ** 0.5).to(dev), (torch.randn(D, generator=g) * 0.5).to(dev)
            scale = torch.randn(D, generator=g).to(dev)
            fused = lambda: backbone.feed_forward_residual(x, w1, b1, w2, b2, scale, route="fused")
            stock = lambda: backbone.feed_forward_residual(x, w1, b1, w2, b2, scale, route="torch")
            diff = float((fused() - stock()).abs().max())
            assert diff < 1e-4, diff
            wf, wt, df, dt = alternate(fused, stock, args.reps, args.warmup, args.inner, torch)
            tokens = N * Tp * Fp
            flop, nbytes = 4.0 * tokens * D * hidden, 2.0 * 4 * tokens * D
            res["op"].append(row_of(f"op N={N}", wf, wt, df, dt, {
                "tokens": tokens, "D": D, "hidden": hidden, "gflop": round(flop * 1e-9, 3), "mbyte": round(nbytes * 1e-6, 3),
                "fused_fraction_of_fp32_matrix_peak": round(flop / df / PEAK_FP32_MATRIX, 4),
                "fused_fraction_of_hbm_bandwidth": round(nbytes / df / PEAK_HBM, 4),
                "torch_route_fraction_of_fp32_matrix_peak": round(flop / dt / PEAK_FP32_MATRIX, 4),
                "max_abs_difference_between_routes": diff}))
        if not args.no_modules:
            torch.manual_seed(11)
            model = backbone.Backbone(**MODEL).to(dev).eval()
            model.attention = "fused"
            for name, p in model.named_parameters():              # LayerScale of a trained model, not the 1e-2 of initialisation
                if name.endswith(".scale"):
                    p.fill_(1.0)
            blk = model.encoderLayers[0]

            def with_kind(m, kind, fn):
                def run():
                    m.feedForward = kind
                    return fn()
                return run
            res["modules"] = []
            for N in (1, 4):
                h = torch.randn(N, Tp, Fp, 4 * MODEL["baseSize"], device=dev)
                a, t = with_kind(blk, "fused", lambda: blk(h))(), with_kind(blk, "torch", lambda: blk(h))()
                diff = float((a - t).abs().max())
                wf, wt, df, dt = alternate(with_kind(blk, "fused", lambda: blk(h)), with_kind(blk, "torch", lambda: blk(h)), args.reps,
                                           args.warmup, max(args.inner // 2, 1), torch)
                res["modules"].append(row_of(f"BasicBlock N={N}", wf, wt, df, dt, {"shape": list(h.shape), "attention": "fused",
                                                                                    "max_abs_difference_between_routes": diff}))
            idx = torch.arange(90, device=dev)
            x = torch.randn(1, 691, 229, 6, device=dev)
            a, t = with_kind(model, "fused", lambda: model(x, idx))(), with_kind(model, "torch", lambda: model(x, idx))()
            diff = float((a - t).abs().max())
            wf, wt, df, dt = alternate(with_kind(model, "fused", lambda: model(x, idx)), with_kind(model, "torch", lambda: model(x, idx)),
                                       args.reps, 2, 2, torch)
            res["modules"].append(row_of("Backbone N=1", wf, wt, df, dt, {"x": list(x.shape), "ctx": list(a.shape), "attention": "fused",
                                                                          "max_abs_difference_between_routes": diff}))
            model.feedForward = backbone.DEFAULT_FEED_FORWARD
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
