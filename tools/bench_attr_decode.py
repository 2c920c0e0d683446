"""Device time of the attribute-head readout of transcription: the fused op (attributes.attribute_decode, csrc/attr_decode.hip) against
the torch-call route (attributes.attribute_decode_torch: ModelTransformer.py:590-651 as the torch calls the reference makes) on
IDENTICAL head outputs, the two routes ALTERNATING in one run.

    python tools/bench_attr_decode.py [--reps 20] [--warmup 5] [--out profiles/attr_decode_bench.json]          (GPU box)

Shapes: K = 512, 4096 and 16384 rows, each of the four velocity criteria.  Also SegmentTranscriber.decode_step (scorer, Viterbi, gather,
the two heads, the readout, segment_events; one host synchronisation for the interval count) at T = 691 x 90 chains with one and with
four recordings, attributeDecode "torch" against "fused".  Times are wall-clock per call around a device synchronisation, median over
the repetitions.  Nothing is promised in advance: whatever comes out is written down."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = [512, 4096, 16384]
CRITERIA = ["hamming", "mse", "match", "mae"]


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "attr_decode_bench.json"))
    ap.add_argument("--no-segment", action="store_true", help="skip the SegmentTranscriber.decode_step part")
    args = ap.parse_args()
    import torch
    from transkun_amd import attributes, synth
    from transkun_amd.transcribe import SegmentTranscriber
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "op": [], "unit": "ms per call, median"}
    for K in KS:
        lv = synth.hash_normal(K * 128, 92, dev).view(K, 128) * 2
        of = synth.hash_normal(K * 4, 93, dev).view(K, 4) * 2
        for crit in CRITERIA:
            t_op, t_torch = alternate(lambda: attributes.attribute_decode(lv, of, crit), lambda: attributes.attribute_decode_torch(lv, of, crit),
                                      args.reps, args.warmup, torch)
            row = {"K": K, "criterion": crit, "fused_ms": round(t_op * 1e3, 4), "torch_route_ms": round(t_torch * 1e3, 4),
                   "ratio_torch_over_fused": round(t_torch / t_op, 2)}
            print(json.dumps(row))
            res["op"].append(row)
    if not args.no_segment:
        P, T, D = 90, 691, 256
        model = SegmentTranscriber(size=D).to(dev).eval()
        res["decode_step"] = []
        for N in (1, 4):
            ctx = synth.hash_normal(N * P * T * D, 97, dev).view(N, P, T, D) * 0.5
            begin = torch.zeros(N, dtype=torch.float64, device=dev)
            counts = {}

            def step(route):
                def run():
                    model.attributeDecode = route
                    counts[route] = model.decode_step(ctx, None, begin, T - 1, 0)["K"]
                return run

            try:
                t_op, t_torch = alternate(step("fused"), step("torch"), args.reps, args.warmup, torch)
            finally:
                model.attributeDecode = "torch"
            row = {"shape": [N, P, T, D], "K": counts["fused"], "fused_ms": round(t_op * 1e3, 3), "torch_route_ms": round(t_torch * 1e3, 3),
                   "ratio_torch_over_fused": round(t_torch / t_op, 3)}
            assert counts["fused"] == counts["torch"]
            print(json.dumps(row))
            res["decode_step"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
