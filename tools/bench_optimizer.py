"""The optimizer step: the fused route (transkun_amd.optim.FusedAdaBelief.step: three launches, csrc/optim.hip) against the torch-fp32
per-parameter route of the reference (train.py:239-246: np.quantile over a host deque, clip_grad_norm_, totalNorm.item(), and
torch_optimizer.AdaBelief's tensor calls per parameter -- restated in tests/optimizer_common.py, the package itself is not needed), the
two routes ALTERNATING in one process on identical gradients.

    python tools/bench_optimizer.py [--reps 20] [--warmup 5] [--out profiles/optimizer_bench.json]          (GPU box)

Layout: 182 tensors summing to 13.61 M fp32 parameters in two groups (decay / no decay), clip_quantile = 0.8, norm histories of 1, 1000
and 10000 values.  Per step: wall clock around a device synchronisation and device time between two events, medians.  The three kernels
alone: device time per launch (20 launches back to back between two events), and the update kernel's bytes per second (28 bytes per element) against 8 TB/s and the 6.3 TB/s copy
rate.  train_step at 4 x 90 x 691 per rank with and without optimizer=.  The ONE gate: the fused step is not slower than the torch
route (exit status 1 otherwise); everything else is written down as it comes out."""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TOTAL = 13_610_000
N_TENSORS = 182
HISTORIES = [1, 1000, 10000]


def layout():
    """182 sizes summing to 13.61 M: one large matrix-like tensor, the others between 64 and 262144 elements, seeded."""
    import numpy as np
    rng = np.random.default_rng(182)
    small = (2 ** rng.uniform(6, 18, N_TENSORS - 1)).astype(np.int64)
    small = (small * ((TOTAL * 0.6) / small.sum())).astype(np.int64) + 1
    sizes = [int(TOTAL - small.sum())] + [int(x) for x in small]
    assert len(sizes) == N_TENSORS and sum(sizes) == TOTAL and min(sizes) >= 1
    return sizes


def timed(fn, reps, warmup, torch):
    """Median wall clock (around a synchronisation) and median device time (events) of fn, seconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    wall, devt = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        devt.append(e0.elapsed_time(e1) * 1e-3)
    return statistics.median(wall), statistics.median(devt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_bench.json"))
    ap.add_argument("--no-train-step", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import optimizer_common as oc
    from transkun_amd import _lib, synth
    from transkun_amd.optim import FusedAdaBelief, GradNormHistory

    dev = torch.device("cuda:0")
    sizes = layout()
    split = N_TENSORS // 2
    lr, wd, betas, eps, q = 2e-4, 1e-4, (0.9, 0.999), 1e-8, 0.8
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "numel": TOTAL, "tensors": N_TENSORS,
           "clip_quantile": q, "unit": "ms per step, median", "steps": []}
    grads = [synth.hash_normal(n, 300 + i, dev) * 0.01 for i, n in enumerate(sizes)]
    slow = False
    for H in HISTORIES:
        rng = np.random.default_rng(H)
        past = rng.lognormal(0.0, 0.5, H).astype(np.float32)
        # fused
        fp = [torch.nn.Parameter(synth.hash_normal(n, 100 + i, dev) * 0.05) for i, n in enumerate(sizes)]
        hist = GradNormHistory(device=dev)
        ring = torch.zeros(hist.capacity)
        ring[:H] = torch.from_numpy(past)
        hist.load_state_dict({"capacity": hist.capacity, "ring": ring, "state": torch.tensor([H, 0], dtype=torch.int32)})
        opt = FusedAdaBelief([{"params": fp[:split]}, {"params": fp[split:], "weight_decay": 0.0}], lr=lr, betas=betas, eps=eps,
                             weight_decay=wd, clip_quantile=q, history=hist)
        opt.zero_grad()
        for p, g in zip(fp, grads):
            p.grad.copy_(g)
        # torch route
        tp = [torch.nn.Parameter(p.detach().clone()) for p in fp]
        for p, g in zip(tp, grads):
            p.grad = g.clone()
        keep = [g.clone() for g in grads]
        states = [{"exp_avg": torch.zeros_like(p), "exp_avg_var": torch.zeros_like(p)} for p in tp]
        groups = [(tp[:split], lr, wd, betas, eps), (tp[split:], lr, 0.0, betas, eps)]
        host = collections.deque((float(x) for x in past), maxlen=10000)
        count = {"t": 0}

        def torch_step():
            count["t"] += 1
            clip = float(np.quantile(host, q))                                   # train.py:239
            norm = oc.torch_route_step(tp, states, groups, count["t"], max_norm=clip)        # train.py:242, :246
            host.append(norm.item())                                             # train.py:244

        def torch_restore():                                                     # clip_grad_norm_ rescales the gradients in place: every
            for p, g in zip(tp, keep):                                           # step gets fresh ones, outside the timed region
                p.grad.copy_(g)

        tw_f, td_f = [], []
        tw_t, td_t = [], []
        for _ in range(args.warmup):
            opt.step()
            torch_restore(); torch_step()
        torch.cuda.synchronize()
        for _ in range(args.reps):                                               # alternating
            w, d = timed(opt.step, 1, 0, torch); tw_f.append(w); td_f.append(d)
            torch_restore()
            w, d = timed(torch_step, 1, 0, torch); tw_t.append(w); td_t.append(d)
        row = {"history": H, "fused_wall_ms": round(statistics.median(tw_f) * 1e3, 4), "fused_device_ms": round(statistics.median(td_f) * 1e3, 4),
               "torch_route_wall_ms": round(statistics.median(tw_t) * 1e3, 3), "torch_route_device_ms": round(statistics.median(td_t) * 1e3, 3)}
        row["ratio_torch_over_fused_wall"] = round(row["torch_route_wall_ms"] / row["fused_wall_ms"], 1)
        slow = slow or row["fused_wall_ms"] > row["torch_route_wall_ms"]
        # the three kernels alone
        ops = _lib.ops()
        stats = torch.empty(3, device=dev)
        table = opt._table()
        coef = stats[2:3]

        def batch(f, n=20):                                                      # n launches back to back between the two events
            return lambda: [f() for _ in range(n)]

        t_norm = timed(batch(lambda: ops.grad_sqnorm(opt.bucket.flat, opt.numel, opt._partials)), args.reps, args.warmup, torch)[1] / 20
        t_clip = timed(batch(lambda: hist._launch(opt._partials, opt.numel, None, q, False, stats)), args.reps, args.warmup, torch)[1] / 20
        t_upd = timed(batch(lambda: ops.adabelief_step(opt.flat, opt.bucket.flat, opt.exp_avg, opt.exp_avg_var, opt.numel, coef, True, table)),
                      args.reps, args.warmup, torch)[1] / 20
        bps = 28.0 * TOTAL / t_upd
        row["kernels_us"] = {"grad_sqnorm": round(t_norm * 1e6, 2), "clip_from_history": round(t_clip * 1e6, 2),
                             "adabelief_step": round(t_upd * 1e6, 2)}
        row["update_TBps"] = round(bps / 1e12, 3)
        row["update_fraction_of_8TBps"] = round(bps / 8e12, 3)
        row["update_fraction_of_6.3TBps_copy"] = round(bps / 6.3e12, 3)
        print(json.dumps(row), flush=True)
        res["steps"].append(row)
        del opt, fp, tp, states, keep
    if not args.no_train_step:
        from transkun_amd.optim import optimizer_groups
        from transkun_amd.trainstep import SegmentModel, train_step
        N, P, T, D = 4, 90, 691, 256
        ctx = synth.hash_normal(N * P * T * D, 21, dev).view(N, P, T, D) * 0.5
        iv = synth.synthetic_intervals(T, N * P, seed=21)
        from transkun_amd.dist import FlatGradBucket
        m0 = SegmentModel(D).to(dev)
        b0 = FlatGradBucket(m0.parameters())
        m1 = SegmentModel(D).to(dev)
        o1 = FusedAdaBelief(optimizer_groups(m1), lr=lr, weight_decay=wd, eps=eps, clip_quantile=q)
        w0, w1 = [], []
        for _ in range(max(args.warmup // 2, 2)):
            train_step(m0, ctx, iv, bucket=b0); train_step(m1, ctx, iv, optimizer=o1)
        torch.cuda.synchronize()
        for _ in range(max(args.reps // 2, 5)):
            w0.append(timed(lambda: train_step(m0, ctx, iv, bucket=b0), 1, 0, torch)[0])
            w1.append(timed(lambda: train_step(m1, ctx, iv, optimizer=o1), 1, 0, torch)[0])
        res["train_step"] = {"shape": [N, P, T, D], "bucket_only_wall_ms": round(statistics.median(w0) * 1e3, 3),
                             "with_optimizer_wall_ms": round(statistics.median(w1) * 1e3, 3)}
        print(json.dumps(res["train_step"]), flush=True)
    res["gate_fused_not_slower"] = not slow
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if slow:
        print("GATE FAILED: the fused step is slower than the torch route", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
