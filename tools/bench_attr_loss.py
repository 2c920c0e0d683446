"""Device time of the attribute-head training loss, forward + backward: the fused op (attributes.attribute_log_prob, csrc/attr_loss.hip)
against the torch-call route (attributes.attribute_log_prob_torch: ModelTransformer.py:291-328 as the torch calls the reference makes,
ContinuousBernoulli's synchronising argument check included) on IDENTICAL head outputs, the two routes ALTERNATING in one run.

    python tools/bench_attr_loss.py [--reps 20] [--warmup 5] [--out profiles/attr_loss_bench.json]          (GPU box)

Shapes: K = 512, 4096 and 16384 target intervals over C = 360 chains (rows dealt to the chains by the integer hash, some chains empty).
Also SegmentTranscriber.log_prob forward + backward at 4 x 90 x 691 (size 256), with the op and with the torch-call route.  Times are
wall-clock per call around a device synchronisation (the torch-call route synchronises by itself; device events would not see its host
side), median over the repetitions.  Whatever comes out is written down."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C = 360
KS = [512, 4096, 16384]


def make_case(K, dev):
    import numpy as np
    import torch
    from transkun_amd import synth
    chain = np.sort((synth.hash_u64_numpy(np.arange(K, dtype=np.uint64), 91) % np.uint64(C)).astype(np.int64))
    counts = np.bincount(chain, minlength=C)
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32, device=dev)
    lv = synth.hash_normal(K * 128, 92, dev).view(K, 128) * 2
    of = synth.hash_normal(K * 4, 93, dev).view(K, 4) * 2
    vel = ((torch.arange(K, device=dev) * 37 + 5) % 128).to(torch.int32)
    refined = (synth.hash_normal(K * 2, 94, dev).view(K, 2) / 8).clamp(-0.5, 0.5)
    pres = (synth.hash_normal(K * 2, 95, dev).view(K, 2) > 0).float()
    base = synth.hash_normal(C, 96, dev) * 50
    return lv, of, vel, refined, pres, offsets, base


def alternate(fa, fb, reps, warmup, torch):
    for _ in range(warmup):
        fa(); fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, acc in ((fa, ta), (fb, tb)):
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            acc.append(time.perf_counter() - t0)
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attr_loss_bench.json"))
    ap.add_argument("--no-segment", action="store_true", help="skip the SegmentTranscriber.log_prob part")
    args = ap.parse_args()
    import torch
    from transkun_amd import attributes, synth
    from transkun_amd.transcribe import SegmentTranscriber
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "C": C, "op": [], "unit": "ms per forward + backward, median"}
    for K in KS:
        lv, of, vel, refined, pres, offsets, base = make_case(K, dev)
        lv.requires_grad_(); of.requires_grad_(); base.requires_grad_()

        def step(fn):
            def run():
                lv.grad = of.grad = base.grad = None
                out = fn(lv, of, vel, refined, pres, offsets, base=base)
                (-out.sum() / 4).backward()
            return run

        t_op, t_torch = alternate(step(attributes.attribute_log_prob), step(attributes.attribute_log_prob_torch), args.reps, args.warmup, torch)
        row = {"K": K, "fused_ms": round(t_op * 1e3, 4), "torch_route_ms": round(t_torch * 1e3, 4), "ratio_torch_over_fused": round(t_torch / t_op, 2)}
        print(json.dumps(row))
        res["op"].append(row)
    if not args.no_segment:
        N, P, T, D = 4, 90, 691, 256
        model = SegmentTranscriber(size=D).to(dev).train()
        ctx = (synth.hash_normal(N * P * T * D, 97, dev).view(N, P, T, D) * 0.5).requires_grad_()
        iv = synth.synthetic_intervals(T, N * P, seed=6)
        batch = [iv[n * P:(n + 1) * P] for n in range(N)]
        K = sum(len(x) for x in iv)
        vel = [(i * 37 + 5) % 128 for i in range(K)]
        refined = (synth.hash_normal(K * 2, 98, "cpu").view(K, 2) / 8).clamp(-0.5, 0.5)
        pres = (synth.hash_normal(K * 2, 99, "cpu").view(K, 2) > 0).float()

        def seg(route):
            def run():
                model.zero_grad(set_to_none=True)
                ctx.grad = None
                lp = model.log_prob(ctx, batch, vel, refined, pres, attributeRoute=route)
                (-lp.sum(-1).mean()).backward()
            return run

        t_op, t_torch = alternate(seg("fused"), seg("torch"), max(args.reps // 2, 3), max(args.warmup // 2, 2), torch)
        res["segment_log_prob"] = {"shape": [N, P, T, D], "K": K, "fused_ms": round(t_op * 1e3, 3), "torch_route_ms": round(t_torch * 1e3, 3)}
        print(json.dumps(res["segment_log_prob"]))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
