"""Device time of posterior sampling (NeuralSemiCRFInterval.sample) at the model's shapes: the alpha sweep, semicrf_sample (the
sampler kernel, then the walk + packing of decode.hip), the copies + list building on the host, and the whole sample() call.

    python tools/bench_sample.py [--reps 10] [--out FILE.json]            event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sample -- python tools/bench_sample.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_sample.py --reps 5 --warmup 2 --trace DIR/.../sample_kernel_trace.csv     kernel split (any machine)

The trace pass runs every (shape, n) config warmup + reps times in the order below and nothing else; --trace assigns the
dispatches of each kernel to the configs in that order and prints the per-kernel mean, and for the sampler kernel the bytes it
must read (the lower triangle, 4 B T (T+1) / 2) over its time, as a fraction of 8 TB/s."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352), (691, 360)]
NS = [1, 8, 32]
PEAK = 8.0e12


def configs():
    return [(T, B, n) for T, B in SHAPES for n in NS]


def tri_bytes(T, B):
    return 4.0 * B * T * (T + 1) / 2


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        _, v = nsci._logz_fwd_raw(s, nz, True)
        for n in NS:
            key = int(torch.randint(0, 2 ** 63 - 1, (1,), generator=gen))
            def op():
                return nsci._sample_raw(s, nz, v, 0, n, key, None)
            if args.trace_pass:
                for _ in range(args.warmup + args.reps):
                    op()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                op(); nsci._logz_fwd_raw(s, nz, True)
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            for _ in range(args.reps):
                nsci._logz_fwd_raw(s, nz, True)
            e[1].record()
            for _ in range(args.reps):
                pairs, offsets = op()
            e[2].record()
            torch.cuda.synchronize()
            alpha_ms = e[0].elapsed_time(e[1]) / args.reps
            sample_ms = e[1].elapsed_time(e[2]) / args.reps
            t0 = time.perf_counter()
            for _ in range(args.reps):
                off_h = offsets.cpu()
                total = int(off_h[-1])
                ph = pairs[:total].cpu()
                flat = nsci.unpack_intervals(ph, off_h, T)
            host_ms = (time.perf_counter() - t0) / args.reps * 1e3
            crf = CRF.NeuralSemiCRFInterval(s, nz)
            crf.sample(n, generator=gen)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                crf.sample(n, generator=gen)
            torch.cuda.synchronize()
            call_ms = (time.perf_counter() - t0) / args.reps * 1e3
            row = dict(T=T, B=B, n=n, alpha_ms=round(alpha_ms, 4), sample_op_ms=round(sample_ms, 4),
                       host_copy_unpack_ms=round(host_ms, 3), sample_call_ms=round(call_ms, 3), intervals=total,
                       sample_op_tri_frac_of_8TBs=round(tri_bytes(T, B) / (sample_ms * 1e-3) / PEAK, 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    want = {"sampler": "sample_code_kernel", "backtrack": "backtrack", "offsets": "offsets_kernel", "pack": "pack_kernel"}
    disp = {k: [] for k in want}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in want.items():
                if pat in name:
                    disp[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = args.warmup + args.reps
    out = []
    for i, (T, B, n) in enumerate(configs()):
        row = dict(T=T, B=B, n=n)
        for k, lst in disp.items():
            lst.sort()
            mine = lst[i * per:(i + 1) * per][args.warmup:]
            row[k + "_us"] = round(sum(e - s for s, e in mine) / max(len(mine), 1) / 1e3, 2)
        row["sampler_frac_of_8TBs"] = round(tri_bytes(T, B) / (row["sampler_us"] * 1e-6) / PEAK, 3) if row["sampler_us"] else None
        out.append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace", default="")
    a = ap.parse_args()
    parse_trace(a) if a.trace else run(a)
