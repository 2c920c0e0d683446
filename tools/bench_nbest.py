"""Device time of k-best Viterbi (NeuralSemiCRFInterval.decode_nbest) at the model's shapes, against semicrf_viterbi (decode)
measured in the same run: semicrf_viterbi_nbest (sweep, walk, offsets + packing), the copies + list building on the host, and the
whole decode_nbest() call.

    python tools/bench_nbest.py [--reps 10] [--out FILE.json]            event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o nbest -- python tools/bench_nbest.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_nbest.py --reps 5 --warmup 2 --trace DIR/.../nbest_kernel_trace.csv     kernel split (any machine)

The trace pass runs every (shape, k) config's semicrf_viterbi_nbest warmup + reps times in the order below and nothing else;
--trace assigns the dispatches of each kernel to the configs in that order and prints the per-kernel mean."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352), (691, 360), (691, 90)]
KS = [1, 4, 16]


def configs():
    return [(T, B, k) for T, B in SHAPES for k in KS]


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        for k in KS:
            def op():
                return nsci._nbest_raw(s, nz, k, None, False)
            if args.trace_pass:
                for _ in range(args.warmup + args.reps):
                    op()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                op(); nsci._viterbi_raw(s, nz, None, False)
            torch.cuda.synchronize()
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            for _ in range(args.reps):
                nsci._viterbi_raw(s, nz, None, False)
            e[1].record()
            for _ in range(args.reps):
                pairs, meta = op()
            e[2].record()
            torch.cuda.synchronize()
            viterbi_ms = e[0].elapsed_time(e[1]) / args.reps
            nbest_ms = e[1].elapsed_time(e[2]) / args.reps
            nB = k * B
            t0 = time.perf_counter()
            for _ in range(args.reps):
                meta_h = meta.cpu().numpy()
                total = int(meta_h[nB])
                ph = pairs[:total].cpu()
            copy_ms = (time.perf_counter() - t0) / args.reps * 1e3
            t0 = time.perf_counter()
            for _ in range(args.reps):
                flat = nsci.unpack_intervals(ph, torch.from_numpy(meta_h[:nB + 1].copy()), T)
                npaths = meta_h[nB + 1:nB + 1 + B]
                _ = [[flat[r * B + c] if r < npaths[c] else None for c in range(B)] for r in range(k)]
            lists_ms = (time.perf_counter() - t0) / args.reps * 1e3
            crf = CRF.NeuralSemiCRFInterval(s, nz)
            crf.decode_nbest(k)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                crf.decode_nbest(k)
            torch.cuda.synchronize()
            call_ms = (time.perf_counter() - t0) / args.reps * 1e3
            row = dict(T=T, B=B, k=k, viterbi_op_ms=round(viterbi_ms, 4), nbest_op_ms=round(nbest_ms, 4),
                       nbest_over_viterbi=round(nbest_ms / viterbi_ms, 2), host_copy_ms=round(copy_ms, 3),
                       python_lists_ms=round(lists_ms, 3), decode_nbest_call_ms=round(call_ms, 3), intervals=total)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    want = {"sweep": "nbest_sweep_kernel", "walk": "nbest_walk_kernel", "offsets": "offsets_kernel", "pack": "pack_kernel"}
    disp = {k: [] for k in want}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in want.items():
                if pat in name:
                    disp[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = args.warmup + args.reps
    out = []
    for i, (T, B, k) in enumerate(configs()):
        row = dict(T=T, B=B, k=k)
        for name, lst in disp.items():
            lst.sort()
            mine = lst[i * per:(i + 1) * per][args.warmup:]
            row[name + "_us"] = round(sum(e - s for s, e in mine) / max(len(mine), 1) / 1e3, 2)
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
