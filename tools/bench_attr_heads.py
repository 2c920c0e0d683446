"""Time and accuracy of the fused attribute heads (attributes.attribute_heads, csrc/attr_heads.hip) against the route they replace
(attributes.attribute_heads_torch: the gather kernel, the [K, 3D] input in memory and the two torch modules) on IDENTICAL inputs,
the two routes ALTERNATING in one process.

    python tools/bench_attr_heads.py [--reps 50] [--warmup 10] [--out profiles/attr_heads_bench.json]          (GPU box)

Shapes: K = 512, 1400, 4096 and 16384 rows at D = 256, Hv = Ho = 512, over 360 chains of T = 691 frames.  Per K: the wall clock per call
around a device synchronisation and the device time between two events around `inner` back-to-back calls (the launch cost of a
single call hides what the device does), medians over the repetitions; the fraction of the fp32 matrix rate (157.3 TFLOP/s) that
the fused op's device time amounts to, from the operations the shapes need (2 K (3D (Hv + Ho) + Hv Nv + Ho No)).  Also
SegmentTranscriber.decode_step at T = 691 x 90 chains with one and with four recordings, attributeHeads "fused" against "torch",
attributeDecode "fused" in both.  And the accuracy cases of tests/test_attr_heads.py: the ratio of the op's maximum error to torch's
fp32 modules' (CPU), both against the float64 modules, per shape and input scale.  Nothing is promised in advance: whatever comes out
is written down."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KS = [512, 1400, 4096, 16384]
PEAK_FP32_MATRIX = 157.3e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attr_heads_bench.json"))
    ap.add_argument("--no-segment", action="store_true", help="skip the SegmentTranscriber.decode_step part")
    ap.add_argument("--no-accuracy", action="store_true", help="skip the accuracy ratios")
    args = ap.parse_args()
    import torch
    from transkun_amd import attributes, synth
    from transkun_amd.transcribe import SegmentTranscriber, _head
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    N, P, T, D, Hv, Ho, Nv, No = 4, 90, 691, 256, 512, 512, 128, 4
    C = N * P
    torch.manual_seed(7)
    vp, op = _head(3 * D, Hv, Nv, 0.1).to(dev).eval(), _head(3 * D, Ho, No, 0.1).to(dev).eval()
    ctx = synth.hash_normal(C * T * D, 95, dev).view(N, P, T, D) * 0.5
    with torch.no_grad():
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
            a = attributes.attribute_heads(ctx, pairs, offsets, vp, op, K)
            t = attributes.attribute_heads_torch(ctx, pairs, offsets, vp, op, K)
            diff = max(float((a[0] - t[0]).abs().max()), float((a[1] - t[1]).abs().max()))
            assert torch.equal(a[2], t[2]) and torch.equal(a[3], t[3]) and diff < 1e-4, diff
            wf, wt, df, dt = alternate(lambda: attributes.attribute_heads(ctx, pairs, offsets, vp, op, K),
                                       lambda: attributes.attribute_heads_torch(ctx, pairs, offsets, vp, op, K), args.reps, args.warmup, args.inner,
                                       torch)
            flop = 2.0 * K * (3 * D * (Hv + Ho) + Hv * Nv + Ho * No)
            row = {"K": K, "fused_wall_ms": round(wf * 1e3, 4), "torch_route_wall_ms": round(wt * 1e3, 4), "fused_device_ms": round(df * 1e3, 4),
                   "torch_route_device_ms": round(dt * 1e3, 4), "ratio_torch_over_fused_wall": round(wt / wf, 2),
                   "ratio_torch_over_fused_device": round(dt / df, 2), "gflop": round(flop * 1e-9, 3),
                   "fused_fraction_of_fp32_matrix_peak": round(flop / df / PEAK_FP32_MATRIX, 4),
                   "torch_route_fraction_of_fp32_matrix_peak": round(flop / dt / PEAK_FP32_MATRIX, 4),
                   "max_abs_difference_between_routes": diff, "launches": {"fused": 2, "torch_route": "gather + 6 stock + 2 BLAS"}}
            print(json.dumps(row), flush=True)
            res["op"].append(row)
    if not args.no_segment:
        model = SegmentTranscriber(size=D).to(dev).eval()
        model.attributeDecode = "fused"
        res["decode_step"] = []
        for n in (1, 4):
            c = synth.hash_normal(n * P * T * D, 97, dev).view(n, P, T, D) * 0.5
            begin = torch.zeros(n, dtype=torch.float64, device=dev)
            counts = {}

            def step(route):
                def run():
                    model.attributeHeads = route
                    counts[route] = model.decode_step(c, None, begin, T - 1, 0)["K"]
                return run

            try:
                wf, wt, _, _ = alternate(step("fused"), step("torch"), args.reps, args.warmup, 1, torch)
            finally:
                model.attributeHeads = "torch"
            assert counts["fused"] == counts["torch"]
            row = {"shape": [n, P, T, D], "K": counts["fused"], "fused_ms": round(wf * 1e3, 3), "torch_route_ms": round(wt * 1e3, 3),
                   "ratio_torch_over_fused": round(wt / wf, 3), "attributeDecode": "fused"}
            print(json.dumps(row), flush=True)
            res["decode_step"].append(row)
    if not args.no_accuracy:
        import attr_heads_common as common
        res["accuracy"] = []
        for (d, hv, ho) in common.SHAPES:
            for scale in common.SCALES:
                cs = common.gate_case(d, hv, ho, scale)
                v, o, x, pr, off = common.to_device(dev, cs["vp"], cs["op"], cs["ctx"], cs["pairs"], cs["offsets"])
                lv, of, _, _ = common.fused(x, pr, off, v, o, cs["K"])
                ev = float((lv.cpu().double() - cs["truth"][0]).abs().max()); eo = float((of.cpu().double() - cs["truth"][1]).abs().max())
                row = {"D": d, "Hv": hv, "Ho": ho, "scale": scale, "K": cs["K"], "logitsVelocity_error": ev, "ofLogits_error": eo,
                       "torch_fp32_cpu_error": list(cs["e32"]), "ratio": [round(ev / cs["e32"][0], 3), round(eo / cs["e32"][1], 3)], "gate": common.GATE}
                print(json.dumps(row), flush=True)
                res["accuracy"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
