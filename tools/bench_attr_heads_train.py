"""Time of the attribute heads in training, forward + backward: attributes.attribute_heads_train (csrc/attr_heads.hip in its training mode
+ csrc/attr_heads_bwd.hip) against the route it replaces (attributes.attribute_heads_torch under autograd: the gather kernel, the
[K, 3D] input in memory, the two torch modules with dropout and their stock backward, the gather's atomic scatter) on IDENTICAL
inputs, the two routes ALTERNATING in one process, both heads in training mode with p = 0.1.

    python tools/bench_attr_heads_train.py [--reps 30] [--warmup 5] [--out profiles/attr_heads_train_bench.json]      (GPU box)

Shapes: K = 512, 1400, 4096 and 16384 rows at D = 256, Hv = Ho = 512, over 360 chains of T = 691 frames.  Per K: the wall clock per
forward + backward around a device synchronisation and the device time between two events around `inner` back-to-back
forward + backward pairs, medians over the repetitions; the fraction of the fp32 matrix rate (157.3 TFLOP/s) that the fused op's
device time amounts to, from the operations forward and backward need (2 K (3 . 3D (Hv + Ho) + 3 (Hv Nv + Ho No)): layer 1 once
forward and twice backward, layer 2 likewise).  Also SegmentTranscriber.log_prob forward + backward at 4 x 90 x 691 (size 256) with
attributeHeads "fused" against "torch" (training mode, the fused loss op in both), and the gradient-gate ratios of
tests/test_attr_heads_train.py on the device.  Nothing is promised in advance: whatever comes out is written down."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KS = [512, 1400, 4096, 16384]
PEAK_FP32_MATRIX = 157.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back forward + backward pairs between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_heads_train_bench.json"))
    ap.add_argument("--no-segment", action="store_true", help="skip the SegmentTranscriber.log_prob part")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the gate ratios")
    args = ap.parse_args()
    import torch
    from bench_attr_heads import alternate
    from transkun_amd import attributes, synth
    from transkun_amd.transcribe import SegmentTranscriber, _head
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [],
           "unit": "ms per forward + backward, median; wall = host clock around a device synchronisation, device = events around `inner` pairs"}
    N, P, T, D, Hv, Ho, Nv, No = 4, 90, 691, 256, 512, 512, 128, 4
    C = N * P
    torch.manual_seed(7)
    vp, op = _head(3 * D, Hv, Nv, 0.1).to(dev).train(), _head(3 * D, Ho, No, 0.1).to(dev).train()
    params = list(vp.parameters()) + list(op.parameters())
    ctx = (synth.hash_normal(C * T * D, 95, dev).view(N, P, T, D) * 0.5).requires_grad_()
    for K in KS:
        g = torch.Generator().manual_seed(K)
        b = torch.randint(0, T, (K,), generator=g)
        e = torch.minimum(b + torch.randint(0, 40, (K,), generator=g), torch.tensor(T - 1))
        pairs = torch.stack([b, e], dim=1).to(torch.int32).to(dev)
        counts = torch.full((C,), K // C, dtype=torch.int64)
        counts[:K - int(counts.sum())] += 1
        offsets = torch.zeros(C + 1, dtype=torch.int32)
        offsets[1:] = counts.cumsum(0)
        offsets = offsets.to(dev)
        dlv = synth.hash_normal(K * Nv, 11, dev).view(K, Nv)
        dof = synth.hash_normal(K * No, 12, dev).view(K, No)

        def step(fn):
            def run():
                for p in params:
                    p.grad = None
                ctx.grad = None
                lv, of, _, _ = fn(ctx, pairs, offsets, vp, op, K)
                torch.autograd.backward([lv, of], [dlv, dof])
            return run

        wf, wt, df, dt = alternate(step(attributes.attribute_heads_train), step(attributes.attribute_heads_torch), args.reps, args.warmup,
                                   args.inner, torch)
        flop = 2.0 * K * 3 * (3 * D * (Hv + Ho) + Hv * Nv + Ho * No)
        row = {"K": K, "fused_wall_ms": round(wf * 1e3, 4), "torch_route_wall_ms": round(wt * 1e3, 4), "fused_device_ms": round(df * 1e3, 4),
               "torch_route_device_ms": round(dt * 1e3, 4), "ratio_torch_over_fused_wall": round(wt / wf, 2),
               "ratio_torch_over_fused_device": round(dt / df, 2), "gflop": round(flop * 1e-9, 3),
               "fused_fraction_of_fp32_matrix_peak": round(flop / df / PEAK_FP32_MATRIX, 4),
               "torch_route_fraction_of_fp32_matrix_peak": round(flop / dt / PEAK_FP32_MATRIX, 4),
               "launches": {"fused": "2 forward + 7 and a memset backward (+ torch's packing and transposing copies)"}}
        print(json.dumps(row), flush=True)
        res["op"].append(row)
    if not args.no_segment:
        model = SegmentTranscriber(size=D).to(dev).train()
        c = (synth.hash_normal(N * P * T * D, 97, dev).view(N, P, T, D) * 0.5).requires_grad_()
        iv = synth.synthetic_intervals(T, N * P, seed=6)
        batch = [iv[n * P:(n + 1) * P] for n in range(N)]
        K = sum(len(x) for x in iv)
        vel = [(i * 37 + 5) % 128 for i in range(K)]
        refined = (synth.hash_normal(K * 2, 98, "cpu").view(K, 2) / 8).clamp(-0.5, 0.5)
        pres = (synth.hash_normal(K * 2, 99, "cpu").view(K, 2) > 0).float()

        def seg(route):
            def run():
                model.zero_grad(set_to_none=True)
                c.grad = None
                lp = model.log_prob(c, batch, vel, refined, pres, attributeHeads=route)
                (-lp.sum(-1).mean()).backward()
            return run

        wf, wt, _, _ = alternate(seg("fused"), seg("torch"), max(args.reps // 2, 3), max(args.warmup // 2, 2), 1, torch)
        res["segment_log_prob"] = {"shape": [N, P, T, D], "K": K, "mode": "train, p = 0.1", "fused_heads_ms": round(wf * 1e3, 3),
                                   "torch_heads_ms": round(wt * 1e3, 3), "ratio_torch_over_fused": round(wt / wf, 3)}
        print(json.dumps(res["segment_log_prob"]), flush=True)
    if not args.no_accuracy:
        import attr_heads_common as common
        import attr_heads_train_common as tc
        res["accuracy"] = []
        names = ("logitsVelocity", "ofLogits") + tc.NAMES
        for (d, hv, ho) in common.SHAPES:
            for (scale, pv, po) in ((1.0, 0.1, 0.1), (8.0, 0.1, 0.1), (1.0, 0.1, 0.5)):
                cs = tc.gate_case(d, hv, ho, scale, pv, po)
                lv, of, grads = tc.run_op(dev, cs)
                ratios = {}
                for name, got, t, e in zip(names, [lv, of] + grads, cs["truth"], cs["e32"]):
                    err = float((got.detach().cpu().double() - t).abs().max())
                    ratios[name] = round(err / max(e, common.U * float(t.abs().max())), 3)
                row = {"D": d, "Hv": hv, "Ho": ho, "scale": scale, "pv": pv, "po": po, "K": cs["K"], "ratio": ratios, "gate": common.GATE}
                print(json.dumps(row), flush=True)
                res["accuracy"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
