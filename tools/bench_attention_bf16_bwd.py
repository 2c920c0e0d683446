"""Time of training through the bf16 axial attention (backbone.axial_attention(route="fused-train", bf16="fused", bf16_train="fused"):
csrc/attention_bf16.hip forward, csrc/attention_bf16_bwd.hip backward) against the stock bf16 route under autograd (the same call with
bf16_train="torch": head-split transposed views into F.scaled_dot_product_attention and torch's own backward) and against the fp32
"fused-train" route on the upcast tensors, on IDENTICAL inputs, the three candidates ALTERNATING in one process.

    python tools/bench_attention_bf16_bwd.py [--reps 30] [--warmup 5] [--out profiles/attention_bf16_bwd_bench.json]          (GPU box)

Cases: forward + backward of the op at the eight shapes of tools/bench_attention_bwd.py (one segment is 89 x 149 tokens: the frequency
axis and the time axis of the same [N, 89, 149, H d] buffers, N = 1 and 4, H = 4, d = 40 and 64); the backward kernel alone at the same
shapes; one BasicBlock forward + backward at [1, 89, 149, 160] (bf16 weights; the fp32 candidate is the same block in fp32); the whole
Backbone forward + backward at [1, 691, 229, 6] (the model's configuration, 90 output indices) in training mode with
useGradientCheckpoint = True under torch.autocast(bfloat16) (the fp32 candidate: the same step without autocast).  Per case: the wall
clock per call around a device synchronisation and the device time between two events around `inner` back-to-back calls, medians over
the repetitions.  Nothing is promised in advance: whatever comes out is written down, and the aim -- the new route no slower on the
device than the stock bf16 route under autograd at the four d = 40 shapes and in the Backbone step -- is reported as met or missed."""
import argparse
import contextlib
import copy
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODEL = dict(inputSize=6, baseSize=40, posEmbedInitGamma=1, nHead=4, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4,
             dropoutProb=0.0, nLayers=6, enabledAttn=["F", "T"], useGradientCheckpoint=True, downsampleF=True)
NAMES = ("bf16_fused_train", "bf16_torch_route", "fp32_fused_train")


def alternate(fns, reps, warmup, inner, torch):
    """([wall], [device]) in seconds per call, medians, of the candidates `fns` run in turn."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    wall, devt = [[] for _ in fns], [[] for _ in fns]
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
    return [statistics.median(x) for x in wall], [statistics.median(x) for x in devt]


def row_of(tag, wall, devt, extra):
    row = {"case": tag}
    for name, w, d in zip(NAMES, wall, devt):
        row[name + "_wall_ms"], row[name + "_device_ms"] = round(w * 1e3, 4), round(d * 1e3, 4)
    row["ratio_torch_route_over_bf16_fused_train_device"] = round(devt[1] / devt[0], 2)
    row["ratio_fp32_fused_train_over_bf16_fused_train_device"] = round(devt[2] / devt[0], 2)
    row.update(extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bf16_bwd_bench.json"))
    ap.add_argument("--no-modules", action="store_true", help="skip the BasicBlock and Backbone parts")
    args = ap.parse_args()
    import torch
    from transkun_amd import _lib, backbone
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [], "kernel": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    Tp, Fp, H = 89, 149, 4
    for d in (40, 64):
        for N in (1, 4):
            g = torch.Generator().manual_seed(100 * d + N)
            q, k, v, go = (torch.randn(N, Tp, Fp, H * d, generator=g).to(bf).to(dev) for _ in range(4))
            for axis, view in (("frequency", lambda t: t), ("time", lambda t: t.transpose(1, 2))):
                qa, ka, va = (view(t.detach()).requires_grad_() for t in (q, k, v))
                qf, kf, vf = (view(t.detach().float()).requires_grad_() for t in (q, k, v))
                ga, gf = view(go), view(go.float())

                def step(ins, cot, **kw):
                    def run():
                        return torch.autograd.grad(backbone.axial_attention(*ins, H, route="fused-train", **kw), ins, cot)
                    return run
                fns = [step((qa, ka, va), ga, bf16="fused", bf16_train="fused"), step((qa, ka, va), ga, bf16="fused"), step((qf, kf, vf), gf)]
                before = dict(backbone.ATTENTION_BF16_TRAIN_ROUTES)
                a, t = fns[0](), fns[1]()
                assert backbone.ATTENTION_BF16_TRAIN_ROUTES == {"fused": before["fused"] + 1, "torch": before["torch"], "bwd": before["bwd"] + 1}
                diff = max(float((x.float() - y.float()).abs().max()) for x, y in zip(a, t))
                assert diff < 0.25, diff
                wall, devt = alternate(fns, args.reps, args.warmup, args.inner, torch)
                nseq, L = qa.shape[0] * qa.shape[1], qa.shape[2]
                res["op"].append(row_of(f"forward + backward, {axis} axis N={N} d={d}", wall, devt, {
                    "sequences": nseq, "L": L, "H": H, "d": d, "max_abs_gradient_difference_between_bf16_routes": diff}))
                # the backward kernel alone, on the views the route hands it
                with torch.no_grad():
                    q4, k4, v4 = (x.detach() for x in (qa, ka, va))
                    dq, dk, dv = (torch.empty_like(x) for x in (q4, k4, v4))
                    (wk,), (dk_s,) = alternate([lambda: _lib.ops().axial_attention_bf16_bwd(q4, k4, v4, ga, dq, dk, dv, H)], args.reps,
                                               args.warmup, args.inner, torch)
                row = {"case": f"backward kernel, {axis} axis N={N} d={d}", "wall_ms": round(wk * 1e3, 4), "device_ms": round(dk_s * 1e3, 4),
                       "gflop_executed": round(16.0 * nseq * H * L * L * d * 1e-9, 3)}      # S, dP twice, dq in pass A; S, dP, dk, dv in pass B
                print(json.dumps(row), flush=True)
                res["kernel"].append(row)
    if not args.no_modules:
        torch.manual_seed(11)
        model = backbone.Backbone(**MODEL).to(dev).train()
        with torch.no_grad():
            for name, p in model.named_parameters():              # LayerScale of a trained model, not the 1e-2 of initialisation
                if name.endswith(".scale"):
                    p.fill_(1.0)
        model.attention, model.attentionBf16 = "fused-train", "fused"
        blk32 = model.encoderLayers[0]
        blk16 = copy.deepcopy(blk32).to(bf)

        def train_step(m, kind, fn, ps, autocast):
            def run():
                m.attentionBf16Train = kind
                with torch.autocast(device_type="cuda", dtype=bf) if autocast else contextlib.nullcontext():
                    out = fn()
                return torch.autograd.grad(out.float().square().sum(), ps, allow_unused=True)
            return run
        res["modules"] = []
        h16 = torch.randn(1, Tp, Fp, 4 * MODEL["baseSize"], device=dev).to(bf)
        h32 = h16.float()
        p16, p32 = list(blk16.parameters()), list(blk32.parameters())
        fns = [train_step(blk16, "fused", lambda: blk16(h16), p16, False), train_step(blk16, "torch", lambda: blk16(h16), p16, False),
               train_step(blk32, "torch", lambda: blk32(h32), p32, False)]
        a, t = fns[0](), fns[1]()
        diff = max(float((x.float() - y.float()).abs().max() / y.float().abs().max().clamp_min(1e-30)) for x, y in zip(a, t))
        wall, devt = alternate(fns, args.reps, args.warmup, max(args.inner // 2, 1), torch)
        res["modules"].append(row_of("BasicBlock forward + backward N=1, bf16 weights", wall, devt, {
            "shape": list(h16.shape), "max_relative_gradient_difference_between_bf16_routes": diff}))
        idx = torch.arange(90, device=dev)
        x = torch.randn(1, 691, 229, 6, device=dev)
        params = list(model.parameters())
        fns = [train_step(model, "fused", lambda: model(x, idx), params, True), train_step(model, "torch", lambda: model(x, idx), params, True),
               train_step(model, "torch", lambda: model(x, idx), params, False)]
        before = dict(backbone.ATTENTION_BF16_TRAIN_ROUTES)
        a = fns[0]()
        launches = backbone.ATTENTION_BF16_TRAIN_ROUTES["bwd"] - before["bwd"]
        assert launches > 0 and backbone.ATTENTION_BF16_TRAIN_ROUTES["torch"] == before["torch"]
        t = fns[1]()
        diff = max(float((p - r).abs().max() / r.abs().max().clamp_min(1e-30)) for p, r in zip(a, t) if p is not None)
        wall, devt = alternate(fns, max(args.reps // 3, 3), 2, 2, torch)
        res["modules"].append(row_of("Backbone forward + backward N=1, training mode, gradient checkpoint, autocast(bfloat16)", wall, devt, {
            "x": list(x.shape), "bf16_backward_launches_per_step": launches, "max_relative_gradient_difference_between_bf16_routes": diff}))
        model.attentionBf16Train = backbone.DEFAULT_ATTENTION_BF16_TRAIN
    d40 = [r for r in res["op"] if r["d"] == 40]
    met = all(r["bf16_fused_train_device_ms"] <= r["bf16_torch_route_device_ms"] for r in d40)
    if "modules" in res:
        met = met and res["modules"][1]["bf16_fused_train_device_ms"] <= res["modules"][1]["bf16_torch_route_device_ms"]
    res["aim"] = {"statement": "the new route is no slower on the device than the stock bf16 route under autograd at the four d = 40 shapes"
                               + (" and in the Backbone step" if "modules" in res else " (modules not run)"), "met": bool(met)}
    print(json.dumps(res["aim"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
