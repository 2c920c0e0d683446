"""The optimizer step (transkun_amd.optim: FusedAdaBelief, GradNormHistory, optimizer_groups; csrc/optim.hip, csrc/optim_math.h).

Every numerical case runs on the CPU path (the shim's host kernels, unmarked) and on the device (@pytest.mark.gpu).  The yardstick is
the float64 numpy restatement in tests/optimizer_common.py; the tolerance rule is stated there.

Which steps take the SGD-style branch (rho_t <= 4), from the float64 host scalars:
    b2 = 0.999: rho_inf = 1999, rho_4 = 3.99750, rho_5 = 4.99600  -> steps 1..4 are SGD-style, step 5 is the first rectified one
    b2 = 0.9:   rho_inf = 19,   rho_4 = 3.73742, rho_5 = 4.58057  -> steps 1..4 as well
so steps 1 to 8 cover both branches and the switch for either value.

Measured worst |op - yardstick| / bound over the teacher-forced cases (1 passes), CPU path and device alike (they are bit-identical):
0.53 / 0.59 for randn gradients (454 / 3.4 M elements), 0.45 with exact zeros, 0.24 at |g| = 1e30, 0.96 at |g| = 1e-30 (m at step 2,
where b1*m and (1-b1)*g cancel; DESIGN.md, "Optimizer step").
"""
import copy

import numpy as np
import pytest
import torch

import optimizer_common as oc
from transkun_amd.optim import FusedAdaBelief, GradNormHistory, adabelief_scalars, optimizer_groups

CPU = torch.device("cpu")


def _dev(request, which):
    return CPU if which == "cpu" else request.getfixturevalue("gpu")


DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


# ---- 1. the update, teacher-forced, steps 1 to 8 --------------------------------------------------------------------------------------
def test_branch_boundaries_of_the_host_scalars():
    for b2 in (0.999, 0.9):
        rect = [adabelief_scalars(t, 1e-3, 1e-2, (0.9, b2), 1e-8)["rectified"] for t in range(1, 9)]
        assert rect == [False] * 4 + [True] * 4, (b2, rect)
        assert not adabelief_scalars(4, 1e-3, 0, (0.9, b2), 1e-8)["rho_t"] > 4
        assert adabelief_scalars(5, 1e-3, 0, (0.9, b2), 1e-8)["rho_t"] > 4
    assert adabelief_scalars(3, 1e-3, 0.0, (0.9, 0.999), 1e-8)["decay"] == 1.0            # wd = 0: the decay multiply is exact


UPDATE_CASES = [("A", "randn", 0.999, 0.8), ("A", "randn", 0.9, 0.8), ("A", "zeros", 0.999, 0.8), ("A", "zeros", 0.9, 0.8),
                ("A", "tiny", 0.999, None), ("A", "huge", 0.999, None), ("A", "huge", 0.9, None), ("B", "randn", 0.999, 0.8),
                ("B", "huge", 0.999, None), ("C", "randn", 0.9, 0.8), ("C", "zeros", 0.999, None), ("D", "randn", 0.999, 0.8)]


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("layout,family,b2,clipq", UPDATE_CASES)
def test_update_against_float64(request, which, layout, family, b2, clipq):
    dev = _dev(request, which)
    worst = oc.teacher_forced_steps(layout, dev, family, (0.9, b2), steps=8, clip_quantile=clipq)
    print(f"worst ratio {layout}/{family}/b2={b2} on {which}: {worst:.3f}")


@pytest.mark.parametrize("which", DEVICES)
def test_huge_gradients_overflow_s_like_fp32(request, which):
    dev = _dev(request, which)
    opt, _ = oc.make_optimizer("A", dev)
    oc.set_grads(opt, oc.gradient("huge", opt.numel, 1))
    opt.step()
    assert bool(torch.isinf(opt.exp_avg_var).all()) and bool(torch.isfinite(opt.exp_avg).all()) and bool(torch.isfinite(opt.flat).all())


@pytest.mark.parametrize("which", DEVICES)
def test_no_decay_leaves_the_bits_alone(request, which):
    """wd = 0 and m = 0 (zero gradients, or gradients whose (1 - b1) g underflows): p keeps its bits, denormals and signed zeros included."""
    dev = _dev(request, which)
    opt, params = oc.make_optimizer("A", dev, wd=0.0)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-40, 3e38, -1.17549435e-38, 1.0, -2.5], device=dev)
    with torch.no_grad():
        opt.flat[60:68].copy_(special)                       # across the group boundary at 67
    before = opt.flat.clone().view(torch.int32)
    g = torch.zeros(opt.numel)
    g[1::2] = 1e-45                                          # the smallest denormal: 0.1 * g rounds to zero
    for _ in range(8):
        oc.set_grads(opt, g)
        opt.step()
    assert torch.equal(opt.flat.view(torch.int32), before)
    assert float(opt.exp_avg.abs().max()) == 0.0


# ---- 2. device equals host, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["A", "D"])
def test_device_equals_host_bitwise(gpu, layout):
    host, _ = oc.make_optimizer(layout, CPU, clip_quantile=0.8, history=GradNormHistory(8))
    devo, _ = oc.make_optimizer(layout, gpu)
    assert torch.equal(host.flat, devo.flat.cpu())
    clipped = 0
    for t in range(1, 7):
        g = oc.gradient("randn", host.numel, t) * (50.0 if t % 2 else 1.0)          # some steps clip, some do not
        oc.set_grads(host, g); oc.set_grads(devo, g)
        host.step()
        devo.step(coef=host.last_coef.to(gpu))
        for a, b, name in ((host.flat, devo.flat, "p"), (host.exp_avg, devo.exp_avg, "m"), (host.exp_avg_var, devo.exp_avg_var, "s")):
            assert torch.equal(a, b.cpu()), (layout, t, name)
        clipped += float(host.last_coef) < 1.0
    assert clipped > 0


# ---- 3. the norm --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("layout,family", [("A", "randn"), ("B", "randn"), ("D", "randn"), ("A", "huge"), ("D", "huge")])
def test_norm(request, which, layout, family):
    dev = _dev(request, which)
    g = oc.gradient(family, sum(sum(s) for s in oc.LAYOUTS[layout]), 3)
    norm64 = oc.yardstick_norm(g.numpy())
    bits = []
    for _ in range(2):
        opt, _ = oc.make_optimizer(layout, dev, clip_quantile=0.8)
        oc.set_grads(opt, g)
        tail = opt.bucket.flat[opt.numel:]
        assert layout == "D" or tail.numel() > 0
        tail.fill_(float("nan"))                             # the bucket's padding is neither read nor written
        before = opt.bucket.flat[:opt.numel].clone()
        opt.step()
        norm = float(opt.last_norm)
        print(f"norm {layout}/{family} on {which}: {norm!r} against {norm64!r}")
        assert np.isfinite(norm) and abs(norm - norm64) <= 2 * oc.EPS32 * norm64
        assert bool(torch.isnan(opt.bucket.flat[opt.numel:]).all())
        assert torch.equal(opt.bucket.flat[:opt.numel], before)
        bits.append(np.float32(norm).view(np.int32))
    assert bits[0] == bits[1]


# ---- 4. history and quantile ----------------------------------------------------------------------------------------------------------------
QS = [0.0, 0.5, 0.8, 1.0]


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("ties", [False, True])
def test_history_quantile_small(request, which, ties):
    dev = _dev(request, which)
    h = GradNormHistory(capacity=8, device=dev)
    ref = oc.HostHistory(8)
    assert h.values().tolist() == [40.0] and float(h.quantile(0.8)) == 40.0            # n = 1 before any append
    rng = np.random.default_rng(5)
    vals = rng.uniform(1.0, 300.0, 20).astype(np.float32)
    if ties:
        vals = np.round(vals / 100.0).astype(np.float32) * 100.0
    for i, v in enumerate(vals):
        for q in QS:
            got, want = float(h.quantile(q)), ref.quantile(q)
            assert oc.ulp_close(got, want), (i, q, got, want)
        if i % 2:
            h.append(float(v))
        else:
            h.append(torch.tensor(v, device=dev))
        ref.append(v)
        assert h.values().tolist() == list(ref.values), i
        assert len(h) == min(i + 2, 8)
    for q in QS:
        assert oc.ulp_close(float(h.quantile(q)), ref.quantile(q))


@pytest.mark.parametrize("which", DEVICES)
def test_history_at_capacity_10000(request, which):
    dev = _dev(request, which)
    h = GradNormHistory(device=dev)
    assert h.capacity == 10000
    rng = np.random.default_rng(6)
    vals = rng.lognormal(3.0, 1.0, 10000).astype(np.float32)
    vals[::7] = vals[3]                                      # ties
    head = 1234
    h.load_state_dict({"capacity": 10000, "ring": torch.from_numpy(vals), "state": torch.tensor([10000, head], dtype=torch.int32)})
    ref = oc.HostHistory(10000, init=None)
    for v in np.roll(vals, -head):
        ref.append(v)
    for q in QS + [0.3337]:
        got, want = float(h.quantile(q)), ref.quantile(q)
        assert oc.ulp_close(got, want), (q, got, want)
    h.append(17.5); ref.append(17.5)
    assert h.values().tolist() == list(ref.values)
    assert oc.ulp_close(float(h.quantile(0.8)), ref.quantile(0.8))
    with pytest.raises(ValueError):
        GradNormHistory(capacity=16385, device=dev)


# ---- 5. clip semantics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
def test_clip_semantics(request, which):
    dev = _dev(request, which)
    opt, params = oc.make_optimizer("A", dev, clip_quantile=0.8, history=GradNormHistory(8, device=dev))
    ref = oc.HostHistory(8)
    clipped = 0
    for t in range(1, 13):
        g = oc.gradient("randn", opt.numel, t) * (30.0 if t % 3 else 0.5)
        oc.set_grads(opt, g)
        before = opt.bucket.flat.clone()
        want_clip = ref.quantile(0.8)                        # the history BEFORE this step's norm
        if dev.type == "cuda":
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")          # step() may not wait for the device
        try:
            opt.step()
        finally:
            if dev.type == "cuda":
                torch.cuda.set_sync_debug_mode("default")
        for x in (opt.last_norm, opt.last_clip, opt.last_coef):
            assert isinstance(x, torch.Tensor) and x.device == opt.flat.device and x.dim() == 0
        norm, clip, coef = float(opt.last_norm), float(opt.last_clip), float(opt.last_coef)
        assert oc.ulp_close(clip, want_clip), (t, clip, want_clip)
        want = oc.yardstick_coef(clip, norm)
        assert abs(coef - want) <= 2 * oc.EPS32 * want, (t, coef, want)
        assert abs(norm - oc.yardstick_norm(g.numpy())) <= 2 * oc.EPS32 * norm
        assert torch.equal(opt.bucket.flat, before)          # the gradient buffer is not rescaled
        ref.append(norm)
        assert opt.history.values().tolist() == list(ref.values)
        clipped += coef < 1.0
    assert 0 < clipped < 12                                  # both sides of the min were seen


@pytest.mark.parametrize("which", DEVICES)
def test_nonfinite_norm_propagates(request, which):
    dev = _dev(request, which)
    opt, _ = oc.make_optimizer("B", dev, clip_quantile=0.8, history=GradNormHistory(8, device=dev))
    g = oc.gradient("randn", opt.numel, 1)
    g[2] = float("inf")
    oc.set_grads(opt, g)
    opt.step()
    assert np.isinf(float(opt.last_norm)) and float(opt.last_coef) == 0.0              # 40 / inf: the reference's own arithmetic
    g[2] = float("nan")
    oc.set_grads(opt, g)
    opt.step()
    assert np.isnan(float(opt.last_norm)) and np.isnan(float(opt.last_coef)) and bool(torch.isnan(opt.flat).all())
    oc.set_grads(opt, oc.gradient("randn", opt.numel, 2))
    opt.step()
    assert np.isnan(float(opt.last_clip))                    # np.quantile of a history that holds a NaN


# ---- 6. aliasing and versions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
def test_aliasing_versions_and_rebinding(request, which):
    dev = _dev(request, which)
    opt, params = oc.make_optimizer("C", dev, clip_quantile=0.8)
    twin, tparams = oc.make_optimizer("C", dev, clip_quantile=0.8)
    lo, hi = opt.flat.data_ptr(), opt.flat.data_ptr() + 4 * opt.numel
    for t in range(1, 4):
        g = oc.gradient("randn", opt.numel, t)
        oc.set_grads(opt, g); oc.set_grads(twin, g)
        versions = [p._version for p in params]
        if t == 2:
            victim = params[2]
            with torch.no_grad():
                victim.data = victim.data.clone()
                victim.data.add_(1.0)                         # a value written while the parameter lived elsewhere is not lost
                tparams[2].data.add_(1.0)
            assert not lo <= victim.data_ptr() < hi
        opt.step(); twin.step()
        assert all(p._version > v for p, v in zip(params, versions))
        assert all(lo <= p.data_ptr() < hi for p in params)
        assert opt.rebound == (1 if t >= 2 else 0) and twin.rebound == 0
        assert all(torch.equal(a, b) for a, b in zip(params, tparams))
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(opt.bucket.params, opt.bucket._views))


@pytest.mark.parametrize("which", DEVICES)
def test_packed_head_weights_follow_the_step(request, which):
    """attributes.attribute_heads caches the packed head weights keyed on the parameters' _version: after a step it must equal freshly
    built modules that hold the same values."""
    import attr_heads_common as hc
    from transkun_amd import attributes
    dev = _dev(request, which)
    D, Hv, Ho = 8, 16, 16
    vp, op = hc.make_heads(D, Hv, Ho, 3)
    vp, op = vp.to(dev), op.to(dev)
    pairs, offsets = hc.pack_rows(hc.make_rows(20, 4))
    ctx = hc.make_ctx(D, 1.0, 5).to(dev)
    pairs, offsets = pairs.to(dev), offsets.to(dev)
    opt = FusedAdaBelief(optimizer_groups(torch.nn.ModuleList([vp, op])), lr=1e-2, weight_decay=1e-2)
    with torch.no_grad():
        first = attributes.attribute_heads(ctx, pairs, offsets, vp, op, 20)            # fills the cache
    for t in range(1, 3):
        oc.set_grads(opt, oc.gradient("randn", opt.numel, t))
        opt.step()
        fresh_v, fresh_o = hc.make_heads(D, Hv, Ho, 99)
        fresh_v.load_state_dict({k: v.detach().cpu().clone() for k, v in vp.state_dict().items()})
        fresh_o.load_state_dict({k: v.detach().cpu().clone() for k, v in op.state_dict().items()})
        fresh_v, fresh_o = fresh_v.to(dev), fresh_o.to(dev)
        with torch.no_grad():
            got = attributes.attribute_heads(ctx, pairs, offsets, vp, op, 20)
            want = attributes.attribute_heads(ctx, pairs, offsets, fresh_v, fresh_o, 20)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert not torch.equal(got[0], first[0])


# ---- 7. checkpointing ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
def test_state_dict_round_trip(request, which):
    dev = _dev(request, which)
    a, pa = oc.make_optimizer("A", dev, clip_quantile=0.8, history=GradNormHistory(8, device=dev))
    for t in range(1, 6):
        oc.set_grads(a, oc.gradient("randn", a.numel, t) * (20.0 if t % 2 else 1.0))
        a.step()
    sd = copy.deepcopy(a.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_var"} and sd["state"][0]["step"] == 5
    b, pb = oc.make_optimizer("A", dev, seed=9, lr=5e-2, clip_quantile=0.8, history=GradNormHistory(8, device=dev))
    with torch.no_grad():
        for x, y in zip(pb, pa):
            x.copy_(y)
    b.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == a.param_groups[0]["lr"]
    for t in range(6, 9):
        g = oc.gradient("randn", a.numel, t) * (20.0 if t % 2 else 1.0)
        oc.set_grads(a, g); oc.set_grads(b, g)
        a.step(); b.step()
        assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_var, b.exp_avg_var)
        assert torch.equal(a.last_clip, b.last_clip) and torch.equal(a.last_coef, b.last_coef)
    assert torch.equal(a.history.values(), b.history.values()) and b.rebound == 0
    off = 0
    for p in pb:                                             # the views still alias the flat buffers
        st = b.state[p]
        assert st["step"] == 8
        assert st["exp_avg"].data_ptr() == b.exp_avg.data_ptr() + 4 * off and st["exp_avg_var"].data_ptr() == b.exp_avg_var.data_ptr() + 4 * off
        assert p.data_ptr() == b.flat.data_ptr() + 4 * off
        off += p.numel()


# ---- 8. scheduler -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
def test_one_cycle_lr_drives_the_step(request, which):
    dev = _dev(request, which)
    lrs = []

    def schedule(opt):
        # (40 total steps: with 20, pct_start * total_steps - 1 = 0 and torch's warm-up phase divides by its zero length)
        s = torch.optim.lr_scheduler.OneCycleLR(opt, 2e-4, 40, pct_start=0.05, cycle_momentum=False, final_div_factor=2, div_factor=20)
        step = s.step
        s.step = lambda: (step(), lrs.append(opt.param_groups[0]["lr"]))[0]
        return s

    oc.teacher_forced_steps("A", dev, "randn", (0.9, 0.999), steps=10, schedule=schedule, lr=2e-4)
    assert len(set(lrs)) == 10                               # the rate did change from step to step (and each step matched its own)


# ---- 9. groups ----------------------------------------------------------------------------------------------------------------------------------
def test_optimizer_groups():
    class Pos(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.table = torch.nn.Parameter(torch.zeros(4, 6))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp = torch.nn.Linear(6, 6)
            self.norm = torch.nn.LayerNorm(6)
            self.pos = Pos()
            self.body = torch.nn.Sequential(torch.nn.Conv1d(6, 6, 3), torch.nn.GroupNorm(2, 6), torch.nn.Linear(6, 3, bias=False))
            self.scale = torch.nn.Parameter(torch.zeros(3))

    net = Net()
    decay, no_decay = optimizer_groups(net, no_decay_modules=[net.pos])
    assert "weight_decay" not in decay and no_decay["weight_decay"] == 0.0
    names = {id(p): n for n, p in net.named_parameters()}
    assert [names[id(p)] for p in decay["params"]] == ["scale", "inp.weight", "body.0.weight", "body.2.weight"]
    assert [names[id(p)] for p in no_decay["params"]] == ["inp.bias", "norm.weight", "norm.bias", "pos.table", "body.0.bias",
                                                          "body.1.weight", "body.1.bias"]
    order = [id(p) for p in net.parameters()]
    for grp in (decay, no_decay):
        idx = [order.index(id(p)) for p in grp["params"]]
        assert idx == sorted(idx)
    without = optimizer_groups(net)
    assert "pos.table" in [names[id(p)] for p in without[0]["params"]]
    opt = FusedAdaBelief(optimizer_groups(net, no_decay_modules=[net.pos]), lr=1e-3, weight_decay=1e-4)
    assert [g["weight_decay"] for g in opt.param_groups] == [1e-4, 0.0]


# ---- 10. train_step(..., optimizer=opt) ---------------------------------------------------------------------------------------------------------
def _cpu_log_prob(scorer, ctx, intervals):
    y = scorer.map[0](ctx)
    return -(y ** 2).mean(dim=(-1, -2)).reshape(-1)


def test_train_step_with_optimizer():
    from transkun_amd import synth
    from transkun_amd.trainstep import SegmentModel, train_step
    torch.manual_seed(0)
    model = SegmentModel(size=8, total_params=5000)
    with torch.no_grad():
        model.rest.copy_(synth.hash_normal(model.rest.numel(), 3, "cpu"))
    plain = SegmentModel(size=8, total_params=5000)
    plain.load_state_dict(model.state_dict())
    again = SegmentModel(size=8, total_params=5000)
    again.load_state_dict(model.state_dict())
    N, P, T = 2, 3, 10
    ctx = synth.hash_normal(N * P * T * 8, 50, "cpu").view(N, P, T, 8)
    # without the optimizer: bit-identical to what it was (two runs, with and without a bucket, agree; parameters untouched)
    stats0, n0 = train_step(plain, ctx, None, log_prob=_cpu_log_prob)
    stats1, n1 = train_step(again, ctx, None, log_prob=_cpu_log_prob, optimizer=None)
    assert torch.equal(stats0, stats1) and n0 == n1 == 0
    assert all(torch.equal(a, b) and torch.equal(a.grad, b.grad) for a, b in zip(plain.parameters(), again.parameters()))
    assert all(torch.equal(a, b) for a, b in zip(plain.parameters(), model.parameters()))
    # with it
    opt = FusedAdaBelief(optimizer_groups(model), lr=1e-3, weight_decay=1e-2, eps=1e-8, clip_quantile=0.8)
    p0 = opt.flat.clone()
    stats, ncoll = train_step(model, ctx, None, log_prob=_cpu_log_prob, optimizer=opt)
    assert torch.equal(stats, stats0) and ncoll == 0
    order = [p for g in opt.param_groups for p in g["params"]]
    by_id = {id(p): q for p, q in zip(model.parameters(), plain.parameters())}
    g = torch.cat([by_id[id(p)].grad.reshape(-1) for p in order])
    assert torch.equal(opt.bucket.flat[:opt.numel], g)
    norm64 = oc.yardstick_norm(g.numpy())
    assert abs(float(opt.last_norm) - norm64) <= 2 * oc.EPS32 * norm64 and float(opt.last_clip) == 40.0
    coef = float(opt.last_coef)
    assert abs(coef - oc.yardstick_coef(40.0, float(opt.last_norm))) <= 2 * oc.EPS32
    zeros = torch.zeros(opt.numel)
    for (lo, hi), pg in zip(oc.group_ranges(opt), opt.param_groups):
        k = adabelief_scalars(1, pg["lr"], pg["weight_decay"], pg["betas"], pg["eps"])
        yp, _, _ = oc.yardstick_update(p0[lo:hi].numpy(), g[lo:hi].numpy(), zeros[lo:hi].numpy(), zeros[lo:hi].numpy(), coef, k)
        tp, _, _ = oc.torch_route_flat(p0[lo:hi], g[lo:hi], zeros[lo:hi], zeros[lo:hi], coef, 1, pg["lr"], pg["weight_decay"], pg["betas"],
                                       pg["eps"])
        oc.check_against_yardstick(opt.flat[lo:hi].numpy(), yp, tp.numpy(), "train_step/p")
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(order, opt._views))
    with pytest.raises(ValueError):
        from transkun_amd.dist import FlatGradBucket
        train_step(model, ctx, None, log_prob=_cpu_log_prob, optimizer=opt, bucket=FlatGradBucket(plain.parameters()))


# ---- 11. arguments ------------------------------------------------------------------------------------------------------------------------------
def test_arguments():
    p = lambda n=3, **kw: torch.nn.Parameter(torch.zeros(n, **kw))
    for bad in ({"weight_decouple": False}, {"rectify": False}, {"amsgrad": True}):
        with pytest.raises(NotImplementedError):
            FusedAdaBelief([p()], **bad)
    with pytest.raises(ValueError):
        FusedAdaBelief([p(dtype=torch.float64)])
    with pytest.raises(ValueError):
        FusedAdaBelief([p(), p(dtype=torch.bfloat16)])
    with pytest.raises(ValueError):
        FusedAdaBelief([p(), p(device="meta")])              # two devices
    with pytest.raises(ValueError):
        FusedAdaBelief([{"params": [p()]}, {"params": []}])
    with pytest.raises(ValueError):
        FusedAdaBelief([{"params": [p()]} for _ in range(9)])
    FusedAdaBelief([{"params": [p()]} for _ in range(8)])
    with pytest.raises(ValueError):
        FusedAdaBelief([p()], clip_quantile=1.5)
    opt = FusedAdaBelief([p()])
    with pytest.raises(ValueError):
        opt.step(coef=torch.ones(1, dtype=torch.float64))
    import inspect
    sig = inspect.signature(FusedAdaBelief.__init__)
    assert list(sig.parameters)[:11] == ["self", "params", "lr", "betas", "eps", "weight_decay", "weight_decouple", "rectify",
                                         "clip_quantile", "history", "group"]
    assert sig.parameters["eps"].default == 1e-3 and sig.parameters["lr"].default == 1e-3


@pytest.mark.gpu
def test_mixed_devices_raise(gpu):
    with pytest.raises(ValueError):
        FusedAdaBelief([torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(3, device=gpu))])


def test_c_abi_rejects_bad_groups():
    import ctypes
    from transkun_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)                             # never dereferenced: the argument checks come first
    G = _lib.AdaBeliefGroups()
    G.n = 2
    G.g[0].end = 8; G.g[1].end = 8                           # an empty second group
    assert lib.semicrf_adabelief_step(fake, fake, fake, fake, 8, None, G, None) == 1 and b"empty" in lib.semicrf_last_error()
    G.n = 9
    assert lib.semicrf_adabelief_step(fake, fake, fake, fake, 8, None, G, None) == 1
    G.n = 1; G.g[0].end = 7
    assert lib.semicrf_adabelief_step(fake, fake, fake, fake, 8, None, G, None) == 1 and b"numel" in lib.semicrf_last_error()
    assert lib.semicrf_clip_from_history(None, 0, None, 0.5, fake, 16385, fake, 0, fake, None) == 1
    assert lib.semicrf_grad_sqnorm(None, 8, fake, None) == 1
