"""Device time of the forced-start alpha sweep (semicrf_alpha_from) and of the segment loop's step with decoder = "mbr", "model"
inputs, one run:
  (a) semicrf_alpha_from with every start 0 next to the existing forward sweep (semicrf_logz_fwd with alpha), the two ALTERNATING,
      one pair of device events per launch, at T=691 x 90, 691 x 360 and 1024 x 352;
  (b) semicrf_alpha_from with the starts the segment loop produces (half the chains 0, half uniform in [0, T/2]), same shapes;
  (c) SegmentTranscriber.decode_step with decoder = "viterbi" next to decoder = "mbr" (threshold 0.5, no tolerance) at T=691 with one
      and with four recordings, alternating, by the host's clock (a step ends with its interval count on the host).
Every figure is reported as the minimum and the mean over the timed launches (after the warm-up).

    python tools/bench_forced_start.py [--reps 20] [--warmup 3] [--out profiles/forced_start_bench.json]
"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(691, 90), (691, 360), (1024, 352)]
STEP_RECORDINGS = [1, 4]


def segment_starts(T, B, seed, dev):
    import numpy as np
    import torch
    rng = np.random.RandomState(seed)
    st = rng.randint(0, T // 2 + 1, size=B)
    st[rng.permutation(B)[:B // 2]] = 0
    return torch.tensor(st, dtype=torch.int32, device=dev)


def timed(fns, reps, warmup):
    """Device events around every launch of each of `fns`, the functions alternating; per function (min ms, mean ms)."""
    import torch
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in fns]
    for r in range(reps):
        for i, f in enumerate(fns):
            ev[i][r][0].record()
            f()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    out = []
    for per in ev:
        ms = [a.elapsed_time(b) for a, b in per]
        out.append((min(ms), sum(ms) / len(ms)))
    return out


def run(args):
    import torch
    from transkun_amd import synth
    from transkun_amd.transcribe import SegmentTranscriber
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    res = {"reps": args.reps, "warmup": args.warmup, "alpha_from": [], "decode_step": []}
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        seg = segment_starts(T, B, 7, dev)
        (a0, a0m), (f0, f0m), (a1, a1m) = timed([lambda: nsci._alpha_from_raw(s, nz, zero), lambda: nsci._logz_fwd_raw(s, nz, True),
                                                 lambda: nsci._alpha_from_raw(s, nz, seg)], args.reps, args.warmup)
        row = dict(T=T, B=B, alpha_from_start0_min_ms=round(a0, 4), alpha_from_start0_mean_ms=round(a0m, 4),
                   logz_fwd_min_ms=round(f0, 4), logz_fwd_mean_ms=round(f0m, 4), ratio_start0_to_logz_fwd=round(a0 / f0, 2),
                   alpha_from_segment_starts_min_ms=round(a1, 4), alpha_from_segment_starts_mean_ms=round(a1m, 4))
        res["alpha_from"].append(row)
        print(json.dumps(row), flush=True)
        del s, nz
    T, P, D = 691, 90, 256
    tr = SegmentTranscriber(D).to(dev).eval()
    for Fn in STEP_RECORDINGS:
        ctx = synth.hash_normal(Fn * P * T * D, 77 + Fn, dev).view(Fn, P, T, D) * 0.5
        start = segment_starts(T, Fn * P, 9, dev)
        bt = torch.zeros(Fn, dtype=torch.float64, device=dev)
        times = {"viterbi": [], "mbr": []}
        K = {}
        for r in range(args.warmup + args.reps):
            for dec in ("viterbi", "mbr"):
                tr.decoder = dec
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step = tr.decode_step(ctx, start, bt, T - 1, T // 2)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                K[dec] = step["K"]
                if r >= args.warmup:
                    times[dec].append((t1 - t0) * 1e3)
        tr.decoder = "viterbi"
        v, m = times["viterbi"], times["mbr"]
        row = dict(T=T, recordings=Fn, chains=Fn * P, viterbi_min_ms=round(min(v), 4), viterbi_mean_ms=round(sum(v) / len(v), 4),
                   mbr_min_ms=round(min(m), 4), mbr_mean_ms=round(sum(m) / len(m), 4), ratio_mbr_to_viterbi=round(min(m) / min(v), 2),
                   intervals_viterbi=K["viterbi"], intervals_mbr=K["mbr"])
        res["decode_step"].append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "forced_start_bench.json"))
    run(ap.parse_args())
