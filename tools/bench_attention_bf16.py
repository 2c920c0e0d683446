"""Time of the bf16 axial attention (backbone.axial_attention(bf16="fused"), csrc/attention_bf16.hip) against the stock bf16 route
(backbone.attention_torch on the same bf16 tensors) and against the fp32 fused op on the upcast tensors, on IDENTICAL inputs, the
three candidates ALTERNATING in one process.

    python tools/bench_attention_bf16.py [--reps 30] [--warmup 5] [--out profiles/attention_bf16_bench.json]          (GPU box)

Cases: the eight shapes of tools/bench_attention.py (one segment is 89 x 149 tokens: the frequency axis and the time axis of the same
[N, 89, 149, H d] buffers, N = 1 and 4, H = 4, d = 40 and 64); then one bf16 BasicBlock forward and the whole bf16 Backbone forward at
[1, 691, 229, 6] (the model's configuration, 90 output indices), attentionBf16 "fused" against "torch".  Per case: the wall clock per
call around a device synchronisation and the device time between two events around `inner` back-to-back calls, medians over the
repetitions.  For the new op also the fraction of the bf16 matrix rate (2.5 PFLOP/s dense; 4 Lq Lk d operations per sequence and
head) and of the HBM bandwidth (8 TB/s; q, k, v read once, out written once, 2 bytes each) that its device time amounts to, and which
of the two is the nearer bound.  Nothing is promised in advance: whatever comes out is written down, and the aim -- the new op no
slower on the device than the stock bf16 route at the four d = 40 shapes and in the BasicBlock -- is reported as met or missed."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_MATRIX = 2.5e15
PEAK_HBM = 8.0e12
MODEL = dict(inputSize=6, baseSize=40, posEmbedInitGamma=1, nHead=4, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4,
             dropoutProb=0.1, nLayers=6, enabledAttn=["F", "T"], useGradientCheckpoint=False, downsampleF=True)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back calls between the two device events")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_bf16_bench.json"))
    ap.add_argument("--no-modules", action="store_true", help="skip the BasicBlock and Backbone parts")
    args = ap.parse_args()
    import torch
    from transkun_amd import backbone
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "inner": args.inner, "op": [],
           "unit": "ms per call, median; wall = host clock around a device synchronisation, device = events around `inner` calls"}
    Tp, Fp, H = 89, 149, 4
    ms = lambda x: round(x * 1e3, 4)
    with torch.no_grad():
        for d in (40, 64):
            for N in (1, 4):
                g = torch.Generator().manual_seed(100 * d + N)
                q, k, v = (torch.randn(N, Tp, Fp, H * d, generator=g).to(bf).to(dev) for _ in range(3))
                q32, k32, v32 = q.float(), k.float(), v.float()
                for axis, view in (("frequency", lambda t: t), ("time", lambda t: t.transpose(1, 2))):
                    qa, ka, va = view(q), view(k), view(v)
                    qf, kf, vf = view(q32), view(k32), view(v32)
                    before = backbone.ATTENTION_BF16_ROUTES["fused"]
                    a, t = backbone.axial_attention(qa, ka, va, H, bf16="fused"), backbone.attention_torch(qa, ka, va, H)
                    assert backbone.ATTENTION_BF16_ROUTES["fused"] == before + 1
                    diff = float((a.float() - t.float()).abs().max())
                    assert diff < 0.1, diff
                    (wn, wt, w32), (dn, dt, d32) = alternate(
                        [lambda: backbone.axial_attention(qa, ka, va, H, bf16="fused"), lambda: backbone.attention_torch(qa, ka, va, H),
                         lambda: backbone.axial_attention(qf, kf, vf, H)], args.reps, args.warmup, args.inner, torch)
                    nseq, L = qa.shape[0] * qa.shape[1], qa.shape[2]
                    flop, nbytes = 4.0 * nseq * H * L * L * d, 2.0 * 4 * nseq * L * H * d
                    fm, fh = flop / dn / PEAK_BF16_MATRIX, nbytes / dn / PEAK_HBM
                    row = {"case": f"{axis} axis N={N} d={d}", "bf16_fused_wall_ms": ms(wn), "bf16_torch_route_wall_ms": ms(wt),
                           "fp32_fused_wall_ms": ms(w32), "bf16_fused_device_ms": ms(dn), "bf16_torch_route_device_ms": ms(dt),
                           "fp32_fused_device_ms": ms(d32), "ratio_torch_route_over_bf16_fused_device": round(dt / dn, 2),
                           "ratio_fp32_fused_over_bf16_fused_device": round(d32 / dn, 2), "sequences": nseq, "L": L, "H": H, "d": d,
                           "gflop": round(flop * 1e-9, 3), "mbyte": round(nbytes * 1e-6, 3),
                           "bf16_fused_fraction_of_bf16_matrix_peak": round(fm, 4), "bf16_fused_fraction_of_hbm_bandwidth": round(fh, 4),
                           "nearer_bound": "matrix" if fm > fh else "hbm", "max_abs_difference_between_bf16_routes": diff}
                    print(json.dumps(row), flush=True)
                    res["op"].append(row)
        if not args.no_modules:
            torch.manual_seed(11)
            model = backbone.Backbone(**MODEL).to(dev).eval()
            for name, p in model.named_parameters():              # LayerScale of a trained model, not the 1e-2 of initialisation
                if name.endswith(".scale"):
                    p.fill_(1.0)
            model = model.to(bf)
            blk = model.encoderLayers[0]

            def with_kind(m, kind, fn):
                def run():
                    m.attentionBf16 = kind
                    return fn()
                return run
            res["modules"] = []
            idx = torch.arange(90, device=dev)
            h = torch.randn(1, Tp, Fp, 4 * MODEL["baseSize"], device=dev).to(bf)
            x = torch.randn(1, 691, 229, 6, device=dev).to(bf)
            for tag, m, fn, reps, inner in (("BasicBlock N=1", blk, lambda: blk(h), args.reps, max(args.inner // 2, 1)),
                                            ("Backbone N=1", model, lambda: model(x, idx), max(args.reps // 3, 3), 2)):
                stock0 = backbone.ATTENTION_ROUTES["torch"]
                a = with_kind(m, "fused", fn)()
                stock_calls = backbone.ATTENTION_ROUTES["torch"] - stock0      # attention_torch calls of the "fused" forward
                t = with_kind(m, "torch", fn)()
                diff = float((a.float() - t.float()).abs().max())
                (wn, wt), (dn, dt) = alternate([with_kind(m, "fused", fn), with_kind(m, "torch", fn)], reps, 2, inner, torch)
                row = {"case": "bf16 " + tag, "bf16_fused_wall_ms": ms(wn), "bf16_torch_route_wall_ms": ms(wt), "bf16_fused_device_ms": ms(dn),
                       "bf16_torch_route_device_ms": ms(dt), "ratio_torch_route_over_bf16_fused_wall": round(wt / wn, 2),
                       "ratio_torch_route_over_bf16_fused_device": round(dt / dn, 2), "attention_torch_calls_with_fused": stock_calls,
                       "output": list(a.shape), "max_abs_difference_between_bf16_routes": diff}
                print(json.dumps(row), flush=True)
                res["modules"].append(row)
            model.attentionBf16 = backbone.DEFAULT_ATTENTION_BF16
    d40 = [r for r in res["op"] if r["d"] == 40]
    met = all(r["bf16_fused_device_ms"] <= r["bf16_torch_route_device_ms"] for r in d40)
    if "modules" in res:
        met = met and res["modules"][0]["bf16_fused_device_ms"] <= res["modules"][0]["bf16_torch_route_device_ms"]
    res["aim"] = {"statement": "the bf16 op is no slower on the device than the stock bf16 route at the four d = 40 shapes"
                               + (" and in the BasicBlock" if "modules" in res else " (modules not run)"), "met": bool(met)}
    print(json.dumps(res["aim"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
