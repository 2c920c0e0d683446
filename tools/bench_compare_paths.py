"""Time of the validation statistic's path comparison (NeuralSemiCRFInterval.decode_stats) at T=2048 x 352 and T=691 x 360 chains,
"model" inputs, against the route a caller has without it: decode() to Python lists, then a Python comparison of the same lists (the
exact matches through a set and the three frame counts by a merge walk -- what the reference's computeStats does per chain).

  device route   decode_stats(target).sum(0).cpu(): the Viterbi sweep, the on-device backtrack, semicrf_compare_paths, one copy back
  list route     decode() (the same sweep and backtrack, the copies back, the Python lists), then the Python walk over both lists
  kernel         semicrf_compare_paths alone on a decode left in HBM, by device events; with a tolerance of (2, 2) as well

Both routes by the host's clock, ALTERNATING in one run; both end with their results on the host.

    python tools/bench_compare_paths.py [--reps 10] [--out profiles/path_stats_bench.json]             timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o cmp -- python tools/bench_compare_paths.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_compare_paths.py --reps 5 --warmup 2 --trace DIR/.../cmp_kernel_trace.csv [--out FILE] [--merge]   kernel time (any machine)

The trace pass runs the comparison kernel warmup + reps times per (shape, tolerance) in the order below and nothing else after the
decodes; --trace assigns the dispatches to them in that order.  --merge adds the kernel times to the rows of an existing --out file."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(2048, 352), (691, 360)]
TOLS = [(0, 0), (2, 2)]
KERNEL = "compare_paths_kernel"


def frames(lst):
    s, prev = 0, -1
    for b, e in lst:
        s += e - b + (1 if prev < b else 0)
        prev = e
    return s


def python_compare(est, ref):
    """Per chain, then summed: the list lengths, the pairs in both lists, the frame counts of either list and of their intersection."""
    tot = [0] * 6
    for a, r in zip(est, ref):
        both, i, j = [], 0, 0
        while i < len(a) and j < len(r):
            lo, hi = max(a[i][0], r[j][0]), min(a[i][1], r[j][1])
            if hi >= lo:
                both.append((lo, hi))
            if a[i][1] < r[j][1]:
                i += 1
            else:
                j += 1
        row = (len(r), len(a), len(r) + len(a) - len(set(a + r)), frames(r), frames(a), frames(both))
        tot = [x + y for x, y in zip(tot, row)]
    return tot


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        target = synth.synthetic_intervals(T, B, seed=7)
        crf = CRF.NeuralSemiCRFInterval(s, nz)
        rp, ro = nsci.pack_intervals(target, T, B, dev)
        pairs, offsets = nsci._viterbi_raw(s, nz, None, False)
        torch.cuda.synchronize()

        def kernel(tol):
            return nsci._compare_paths_raw(pairs, offsets, rp, ro, T, tol)
        if args.trace_pass:
            for tol in TOLS:
                for _ in range(args.warmup + args.reps):
                    kernel(tol)
            torch.cuda.synchronize()
            continue

        def device_route():
            return crf.decode_stats(target).sum(0).cpu().tolist()

        def list_route():
            return python_compare(crf.decode(), target)
        for _ in range(args.warmup):
            a, b = device_route(), list_route()
            assert a[:6] == b, (a, b)
        kern_ms = {}
        for tol in TOLS:
            for _ in range(args.warmup):
                kernel(tol)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.reps + 1)]
            ev[0].record()
            for r in range(args.reps):
                kernel(tol)
                ev[r + 1].record()
            torch.cuda.synchronize()
            kern_ms[tol] = sum(ev[r].elapsed_time(ev[r + 1]) for r in range(args.reps)) / args.reps
        dev_ms = list_ms = dec_ms = 0.0
        for r in range(args.reps):
            t0 = time.perf_counter()
            device_route()
            t1 = time.perf_counter()
            est = crf.decode()
            t2 = time.perf_counter()
            python_compare(est, target)
            t3 = time.perf_counter()
            dev_ms += (t1 - t0) * 1e3 / args.reps
            dec_ms += (t2 - t1) * 1e3 / args.reps
            list_ms += (t3 - t1) * 1e3 / args.reps
        row = dict(T=T, B=B, decoded_intervals=int(offsets[-1]), target_intervals=int(ro[-1]), device_route_ms=round(dev_ms, 4),
                   list_route_ms=round(list_ms, 4), list_route_decode_ms=round(dec_ms, 4), speedup=round(list_ms / dev_ms, 2),
                   compare_op_ms=round(kern_ms[(0, 0)], 4), compare_op_tol22_ms=round(kern_ms[(2, 2)], 4))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    disp = []
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            if KERNEL in r.get("Kernel_Name", ""):
                disp.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    disp.sort()
    per = args.warmup + args.reps
    out, i = [], 0
    for T, B in SHAPES:
        row = dict(T=T, B=B)
        for tol in TOLS:
            mine = disp[i * per:(i + 1) * per][args.warmup:]
            row["kernel_us" if tol == (0, 0) else "kernel_tol22_us"] = round(sum(e - s for s, e in mine) / max(len(mine), 1) / 1e3, 2)
            i += 1
        out.append(row)
        print(json.dumps(row))
    if args.out:
        if args.merge and os.path.exists(args.out):
            rows = json.load(open(args.out))
            for row, extra in zip(rows, out):
                assert (row["T"], row["B"]) == (extra["T"], extra["B"])
                row.update(extra)
            out = rows
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-pass", action="store_true")
    ap.add_argument("--trace", default="")
    ap.add_argument("--merge", action="store_true")
    a = ap.parse_args()
    parse_trace(a) if a.trace else run(a)
