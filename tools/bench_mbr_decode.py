"""Device time of MBR path decoding (NeuralSemiCRFInterval.decode_mbr_packed) at the model's shapes, "model" inputs, thresholds
0.5 / 0.2 / 0.05:
  (a) semicrf_mbr_select (the dynamic program over the packed lattice + decode.hip's backtrack and packing + the probs gather)
      against semicrf_marginal_decode, the call that produces its input -- device events in the same run, the two ALTERNATING;
  (b) the whole decode_mbr_packed call (alpha and beta sweeps, the lattice, the selection, the copies back) against the dense
      route to the same path: forward_backward (the dense [T, T, B] marginals), a torch-built gain tensor m - tau, and the Viterbi
      decode of it with zero noise -- both by the host's clock, both end with their copies back.

    python tools/bench_mbr_decode.py [--reps 10] [--out FILE.json]                          event timing (GPU box)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mbr -- python tools/bench_mbr_decode.py --reps 5 --warmup 2 --trace-pass
    python tools/bench_mbr_decode.py --reps 5 --warmup 2 --trace DIR/.../mbr_kernel_trace.csv      kernel split (any machine)

The trace pass runs semicrf_mbr_select on every (shape, threshold) warmup + reps times in the order below and nothing else after
the lattices are built; --trace assigns the dispatches of each kernel to them in that order and prints the per-kernel mean."""
import argparse
import csv
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(1024, 352), (691, 360), (691, 90), (2048, 88)]
TAUS = [0.5, 0.2, 0.05]
KERNELS = {"dp": "mbr_dp_kernel", "backtrack": "backtrack_par_kernel", "offsets": "semicrf::offsets_kernel", "pack": "pack_kernel",
           "probs": "mbr_probs_kernel"}


def dense_route(CRF, s, nz, tau):
    """forward_backward + the gain tensor + Viterbi with zero noise: the same path from the dense [T, T, B] marginals."""
    import torch
    _, grad, _ = CRF.forward_backward(s, nz)
    gain = grad - tau
    zero = torch.zeros_like(nz)
    return CRF.NeuralSemiCRFInterval(gain, zero).decode_packed()


def run(args):
    import torch
    from transkun_amd import CRF, synth
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    dev = torch.device("cuda:0")
    rows = []
    for T, B in SHAPES:
        s, nz = synth.crf_inputs(T, B, 1234, dev, "model")
        lz, v, q = nsci._marginal_inputs(s, nz)
        for tv in TAUS:
            tau = torch.full((1,), tv, dtype=torch.float32, device=dev)
            cap = (int(1.0 / tv) + 1) * T * B

            def lattice():
                return nsci._marginal_decode_raw(s, nz, tau, cap, (lz, v, q))
            lat = lattice()

            def op():
                return nsci._mbr_select_raw(lat[0], lat[2], lat[1], T, tau)
            if args.trace_pass:
                torch.cuda.synchronize()
                for _ in range(args.warmup + args.reps):
                    op()
                torch.cuda.synchronize()
                continue
            for _ in range(args.warmup):
                op(); lattice(); CRF.decode_mbr_packed(s, nz, tv); dense_route(CRF, s, nz, tv)
            torch.cuda.synchronize()
            cells, selected = int(lat[1][-1]), int(op()[1][-1])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * args.reps + 1)]
            ev[0].record()
            for r in range(args.reps):                      # alternating: lattice, selection, lattice, ...
                lattice()
                ev[2 * r + 1].record()
                op()
                ev[2 * r + 2].record()
            torch.cuda.synchronize()
            lat_ms = sum(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(args.reps)) / args.reps
            op_ms = sum(ev[2 * r + 1].elapsed_time(ev[2 * r + 2]) for r in range(args.reps)) / args.reps
            call_ms = dense_ms = 0.0
            for r in range(args.reps):                      # alternating as well; host wall clock: both end with copies back
                t0 = time.perf_counter()
                CRF.decode_mbr_packed(s, nz, tv)
                t1 = time.perf_counter()
                dense_route(CRF, s, nz, tv)
                t2 = time.perf_counter()
                call_ms += (t1 - t0) * 1e3 / args.reps
                dense_ms += (t2 - t1) * 1e3 / args.reps
            row = dict(T=T, B=B, tau=tv, lattice_cells=cells, selected=selected, marginal_decode_op_ms=round(lat_ms, 4),
                       mbr_select_op_ms=round(op_ms, 4), ratio_to_marginal_decode=round(op_ms / lat_ms, 3),
                       decode_mbr_packed_call_ms=round(call_ms, 4), dense_route_ms=round(dense_ms, 4),
                       speedup_vs_dense=round(dense_ms / call_ms, 2))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out and rows:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def parse_trace(args):
    disp = {k: [] for k in KERNELS}
    with open(args.trace) as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "")
            for k, pat in KERNELS.items():
                if pat in name:
                    disp[k].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    per = args.warmup + args.reps
    out = []
    i = 0
    for T, B in SHAPES:
        for tv in TAUS:
            row = dict(T=T, B=B, tau=tv)
            for k, lst in disp.items():
                lst.sort()
                mine = lst[i * per:(i + 1) * per][args.warmup:]
                row[k + "_us"] = round(sum(e - s for s, e in mine) / max(len(mine), 1) / 1e3, 2)
            out.append(row)
            print(json.dumps(row))
            i += 1
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
