"""Time of training through the backbone's fused axial attention (backbone.axial_attention(route="fused-train"): csrc/attention.hip
forward, csrc/attention_bwd.hip backward) against the stock route under autograd (backbone.attention_torch: the reference's call --
head-split transposed views into F.scaled_dot_product_attention, with whatever copies eager makes, and torch's own backward) on
IDENTICAL inputs, the two routes ALTERNATING in one process.

    python tools/bench_attention_bwd.py [--reps 30] [--warmup 5] [--out profiles/attention_bwd_bench.json]          (GPU box)

Cases: forward + backward of the op at the model's two shapes (one segment is 89 x 149 tokens: 89 sequences of L = 149 along the
frequency axis, 149 sequences of L = 89 along the time axis, read from the same [N, 89, 149, H d] buffers by strides) at N = 1 and 4,
H = 4, d = 40 and 64; the backward kernel alone at the same shapes; one BasicBlock forward + backward at [N, 89, 149, 160]; the whole
Backbone forward + backward at [1, 691, 229, 6] (the model's configuration, 90 output indices) in training mode with
useGradientCheckpoint = True, as the reference trains.  Per case: the wall clock per call around a device synchronisation and the
device time between two events around `inner` back-to-back calls, medians over the repetitions.  For the backward kernel also the
fraction of the fp32 matrix rate (157.3 TFLOP/s) that its device time amounts to, counted twice: by the 14 Lq Lk d operations per
sequence and head it executes (the score and dP blocks are formed in both passes) and by the 10 Lq Lk d a backward needs.
Nothing is promised in advance: whatever comes out is written down."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MATRIX = 157.3e12
MODEL = dict(inputSize=6, baseSize=40, posEmbedInitGamma=1, nHead=4, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4,
             dropoutProb=0.0, nLayers=6, enabledAttn=["F", "T"], useGradientCheckpoint=True, downsampleF=True)


def alternate(fa, fb, reps, warmup, inner, torch):
    """(wall a, wall b, device a, device b) in seconds per call, medians; fb may be None."""
    fns = [f for f in (fa, fb) if f is not None]
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    wall, devt = ([], []), ([], [])
    for _ in range(reps):
        for i, f in enumerate(fns):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            wall[i].append(time.perf_counter() - t0)
        for i, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            devt[i].append(e0.elapsed_time(e1) * 1e-3 / inner)
    return tuple(statistics.median(x) if x else None for x in wall + devt)


def row_of(tag, wf, wt, df, dt, extra):
    row = {"case": tag, "fused_train_wall_ms": round(wf * 1e3, 4), "torch_route_wall_ms": round(wt * 1e3, 4),
           "fused_train_device_ms": round(df * 1e3, 4), "torch_route_device_ms": round(dt * 1e3, 4),
           "ratio_torch_over_fused_train_wall": round(wt / wf, 2), "ratio_torch_over_fused_train_device": round(dt / df, 2)}
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bwd_bench.json"))
    ap.add_argument("--no-modules", action="store_true", help="skip the BasicBlock and Backbone parts")
    args = ap.parse_args()
    import torch
    from transkun_amd import _lib, backbone
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [], "kernel": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    Tp, Fp, H = 89, 149, 4
    for d in (40, 64):
        for N in (1, 4):
            g = torch.Generator().manual_seed(100 * d + N)
            q, k, v, go = (torch.randn(N, Tp, Fp, H * d, generator=g).to(dev) for _ in range(4))
            for axis, view in (("frequency", lambda t: t), ("time", lambda t: t.transpose(1, 2))):
                qa, ka, va = (view(t.detach()).requires_grad_() for t in (q, k, v))
                ga = view(go)

                def step(route):
                    def run():
                        out = backbone.axial_attention(qa, ka, va, H, route=route)
                        return torch.autograd.grad(out, (qa, ka, va), ga)
                    return run
                a, t = step("fused-train")(), step("torch")()
                diff = max(float((x - y).abs().max()) for x, y in zip(a, t))
                assert diff < 1e-3, diff
                wf, wt, df, dt = alternate(step("fused-train"), step("torch"), args.reps, args.warmup, args.inner, torch)
                nseq, L = qa.shape[0] * qa.shape[1], qa.shape[2]
                res["op"].append(row_of(f"forward + backward, {axis} axis N={N} d={d}", wf, wt, df, dt, {
                    "sequences": nseq, "L": L, "H": H, "d": d, "max_abs_gradient_difference_between_routes": diff}))
                # the backward kernel alone, on the views the route hands it
                with torch.no_grad():
                    q4, k4, v4 = (x.detach() for x in (qa, ka, va))
                    o4 = backbone.axial_attention(q4, k4, v4, H, route="fused")
                    dq, dk, dv = (torch.empty_like(x) for x in (q4, k4, v4))
                    kern = lambda: _lib.ops().axial_attention_bwd(q4, k4, v4, o4, ga, dq, dk, dv, H)
                    wk, _, dk_s, _ = alternate(kern, None, args.reps, args.warmup, args.inner, torch)
                executed, needed = 14.0 * nseq * H * L * L * d, 10.0 * nseq * H * L * L * d
                row = {"case": f"backward kernel, {axis} axis N={N} d={d}", "wall_ms": round(wk * 1e3, 4), "device_ms": round(dk_s * 1e3, 4),
                       "gflop_executed": round(executed * 1e-9, 3), "fraction_of_fp32_matrix_peak_executed": round(executed / dk_s / PEAK_FP32_MATRIX, 4),
                       "fraction_of_fp32_matrix_peak_needed": round(needed / dk_s / PEAK_FP32_MATRIX, 4)}
                print(json.dumps(row), flush=True)
                res["kernel"].append(row)
    if not args.no_modules:
        torch.manual_seed(11)
        model = backbone.Backbone(**MODEL).to(dev).train()
        with torch.no_grad():
            for name, p in model.named_parameters():              # LayerScale of a trained model, not the 1e-2 of initialisation
                if name.endswith(".scale"):
                    p.fill_(1.0)
        blk = model.encoderLayers[0]
        params = [p for p in model.parameters()]

        def train_step(m, route, fn, ps):
            def run():
                m.attention = route
                return torch.autograd.grad(fn().square().sum(), ps, allow_unused=True)
            return run
        res["modules"] = []
        bps = [p for p in blk.parameters()]
        for N in (1, 4):
            h = torch.randn(N, Tp, Fp, 4 * MODEL["baseSize"], device=dev)
            fa, ft = train_step(blk, "fused-train", lambda: blk(h), bps), train_step(blk, "torch", lambda: blk(h), bps)
            a, t = fa(), ft()
            diff = max(float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for x, y in zip(a, t))
            wf, wt, df, dt = alternate(fa, ft, args.reps, args.warmup, max(args.inner // 2, 1), torch)
            res["modules"].append(row_of(f"BasicBlock forward + backward N={N}", wf, wt, df, dt, {
                "shape": list(h.shape), "max_relative_gradient_difference_between_routes": diff}))
        idx = torch.arange(90, device=dev)
        x = torch.randn(1, 691, 229, 6, device=dev)
        fa, ft = train_step(model, "fused-train", lambda: model(x, idx), params), train_step(model, "torch", lambda: model(x, idx), params)
        a, t = fa(), ft()
        diff = max(float((p - r).abs().max() / r.abs().max().clamp_min(1e-30)) for p, r in zip(a, t) if p is not None)
        wf, wt, df, dt = alternate(fa, ft, max(args.reps // 3, 3), 2, 2, torch)
        res["modules"].append(row_of("Backbone forward + backward N=1, training mode, gradient checkpoint", wf, wt, df, dt, {
            "x": list(x.shape), "max_relative_gradient_difference_between_routes": diff}))
        model.attention = backbone.DEFAULT_ATTENTION
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
