"""Time of the backbone's fused axial attention (backbone.axial_attention, csrc/attention.hip) against the stock route it replaces
(backbone.attention_torch: the reference's call -- head-split transposed views into F.scaled_dot_product_attention, with whatever
copies eager makes) on IDENTICAL inputs, the two routes ALTERNATING in one process.

    python tools/bench_attention.py [--reps 30] [--warmup 5] [--out profiles/attention_bench.json]          (GPU box)

Cases: the model's two shapes (one segment is 89 x 149 tokens: 89 sequences of L = 149 along the frequency axis, 149 sequences of
L = 89 along the time axis, read from the same [N, 89, 149, H d] buffers by strides) at N = 1 and 4, H = 4, d = 40; the same lengths at
d = 64; one BasicBlock forward (N = 1, 4) and the whole Backbone forward at [N, 691, 229, 6] (N = 1, 2; the model's configuration,
90 output indices), attention "fused" against "torch".  Per case: the wall clock per call around a device synchronisation and the device time between
two events around `inner` back-to-back calls, medians over the repetitions.  For the op also the fraction of the fp32 matrix rate
(157.3 TFLOP/s; 4 Lq Lk d operations per sequence and head) and of the HBM bandwidth (8 TB/s; q, k, v read once, out written once)
that its device time amounts to.  Nothing is promised in advance: whatever comes out is written down."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bench.json"))
    ap.add_argument("--no-modules", action="store_true", help="skip the BasicBlock and Backbone parts")
    args = ap.parse_args()
    import torch
    from transkun_amd import backbone
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    Tp, Fp, H = 89, 149, 4
    with torch.no_grad():
        for d in (40, 64):
            for N in (1, 4):
                g = torch.Generator().manual_seed(100 * d + N)
                q, k, v = (torch.randn(N, Tp, Fp, H * d, generator=g).to(dev) for _ in range(3))
                for axis, view in (("frequency", lambda t: t), ("time", lambda t: t.transpose(1, 2))):
                    qa, ka, va = view(q), view(k), view(v)
                    a, t = backbone.axial_attention(qa, ka, va, H), backbone.attention_torch(qa, ka, va, H)
                    diff = float((a - t).abs().max())
                    assert diff < 1e-4, diff
                    wf, wt, df, dt = alternate(lambda: backbone.axial_attention(qa, ka, va, H), lambda: backbone.attention_torch(qa, ka, va, H),
                                               args.reps, args.warmup, args.inner, torch)
                    nseq, L = qa.shape[0] * qa.shape[1], qa.shape[2]
                    flop, nbytes = 4.0 * nseq * H * L * L * d, 4.0 * 4 * nseq * L * H * d
                    res["op"].append(row_of(f"{axis} axis N={N} d={d}", wf, wt, df, dt, {
                        "sequences": nseq, "L": L, "H": H, "d": d, "gflop": round(flop * 1e-9, 3), "mbyte": round(nbytes * 1e-6, 3),
                        "fused_fraction_of_fp32_matrix_peak": round(flop / df / PEAK_FP32_MATRIX, 4),
                        "fused_fraction_of_hbm_bandwidth": round(nbytes / df / PEAK_HBM, 4),
                        "torch_route_fraction_of_fp32_matrix_peak": round(flop / dt / PEAK_FP32_MATRIX, 4),
                        "max_abs_difference_between_routes": diff}))
        if not args.no_modules:
            torch.manual_seed(11)
            model = backbone.Backbone(**MODEL).to(dev).eval()
            for name, p in model.named_parameters():              # LayerScale of a trained model, not the 1e-2 of initialisation
                if name.endswith(".scale"):
                    p.fill_(1.0)
            blk = model.encoderLayers[0]

            def with_route(m, route, fn):
                def run():
                    m.attention = route
                    return fn()
                return run
            res["modules"] = []
            for N in (1, 4):
                h = torch.randn(N, Tp, Fp, 4 * MODEL["baseSize"], device=dev)
                a, t = with_route(blk, "fused", lambda: blk(h))(), with_route(blk, "torch", lambda: blk(h))()
                diff = float((a - t).abs().max())
                wf, wt, df, dt = alternate(with_route(blk, "fused", lambda: blk(h)), with_route(blk, "torch", lambda: blk(h)), args.reps,
                                           args.warmup, max(args.inner // 2, 1), torch)
                res["modules"].append(row_of(f"BasicBlock N={N}", wf, wt, df, dt, {"shape": list(h.shape), "max_abs_difference_between_routes": diff}))
            idx = torch.arange(90, device=dev)
            for N in (1, 2):
                x = torch.randn(N, 691, 229, 6, device=dev)
                a, t = with_route(model, "fused", lambda: model(x, idx))(), with_route(model, "torch", lambda: model(x, idx))()
                diff = float((a - t).abs().max())
                wf, wt, df, dt = alternate(with_route(model, "fused", lambda: model(x, idx)), with_route(model, "torch", lambda: model(x, idx)),
                                           max(args.reps // 3, 3), 2, 2, torch)
                res["modules"].append(row_of(f"Backbone N={N}", wf, wt, df, dt, {"x": list(x.shape), "ctx": list(a.shape),
                                                                                  "max_abs_difference_between_routes": diff}))
            model.attention = backbone.DEFAULT_ATTENTION
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
