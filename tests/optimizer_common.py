"""Shared by the CPU and GPU tests of the optimizer step (tests/test_optimizer.py): the parameter layouts, the float64 yardstick
(a numpy restatement of the update rule and of the norm / clip / history rules, on fp32 inputs and the op's own host scalars), and
the second route: torch's fp32 tensor calls in the order of clip_grad_norm_ and torch_optimizer.AdaBelief.

Tolerance of a quantity (p, m or s after a step) against the yardstick, per element: the larger of
    (a) 2 x the worst error of the torch-fp32 route for that quantity on the same inputs, and
    (b) 4 eps32 max(|yardstick|, smallest normal).
The margin of 2: the op rounds each scalar factor to fp32 once where torch applies Python doubles to fp32 tensors -- at most one more
rounding per operation.
"""
import collections
import math

import numpy as np
import torch

from transkun_amd.optim import FusedAdaBelief, GradNormHistory, adabelief_scalars

EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)


def _layout_d():
    g = torch.Generator().manual_seed(20240)
    sizes = [3 * 2 ** 20 + 5] + [int(x) for x in torch.randint(1, 4097, (181,), generator=g)]
    return [sizes[:100], sizes[100:]]


# groups of tensor sizes.  A: unaligned starts, a 4-element access across the group boundary (67 = 3 mod 4), a one-element tail;
# B: less than one vector; C: a group that is one scalar; D: many workgroups, the norm's second stage, a 182-tensor table
LAYOUTS = {
    "A": [[1, 3, 63], [64, 65, 257, 1]],
    "B": [[5]],
    "C": [[7, 33], [1], [130, 2]],
    "D": _layout_d(),
}
GROUP_WD = [1e-2, 0.0, 3e-2]                  # per group, in order (the second group is the reference's no-decay group)


def make_optimizer(layout, device, seed=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=None, p_scale=1.0, **kw):
    """Seeded parameters in the layout's groups and a FusedAdaBelief over them.  Returns (optimizer, parameters)."""
    g = torch.Generator().manual_seed(seed)
    groups, params = [], []
    for gi, sizes in enumerate(LAYOUTS[layout] if isinstance(layout, str) else layout):
        ps = [torch.nn.Parameter((torch.randn(n, generator=g) * p_scale).to(device)) for n in sizes]
        groups.append({"params": ps, "weight_decay": GROUP_WD[gi] if wd is None else wd})
        params.extend(ps)
    return FusedAdaBelief(groups, lr=lr, betas=betas, eps=eps, **kw), params


def group_ranges(opt):
    lo = 0
    for end in opt._ends:
        yield lo, end
        lo = end


def set_grads(opt, flat_grad):
    """Write a flat fp32 gradient (host tensor, opt.numel elements) into the optimizer's bucket."""
    opt.zero_grad()
    opt.bucket.flat[:opt.numel].copy_(flat_grad)


def gradient(family, n, step, seed=1):
    g = torch.Generator().manual_seed(1000 * seed + step)
    if family == "randn":
        return torch.randn(n, generator=g) * 3.0
    if family == "zeros":                      # the same half of the elements is exactly zero at every step: m = 0, s = eps accumulating
        keep = (torch.arange(n) % 2 == 0).float()
        return torch.randn(n, generator=g) * keep
    if family == "tiny":
        return torch.full((n,), 1e-30) * torch.sign(torch.randn(n, generator=g))
    if family == "huge":
        return torch.full((n,), 1e30) * torch.sign(torch.randn(n, generator=g))
    raise ValueError(family)


# ---- the yardstick: float64 numpy ------------------------------------------------------------------------------------------------------
def yardstick_update(p, g, m, s, coef, k):
    """One step of the update rule on fp32 arrays, in float64.  k: adabelief_scalars(...) (fp32-rounded factors as Python floats)."""
    p, g, m, s = (np.asarray(x, np.float64) for x in (p, g, m, s))
    with np.errstate(all="ignore"):
        g = g * float(coef)
        p = p * k["decay"]
        m = k["b1"] * m + k["omb1"] * g
        r = g - m
        s = k["b2"] * s + k["omb2"] * r * r + k["eps"]
        if k["rectified"]:
            denom = np.sqrt(s) / k["sqrt_bc2"] + k["eps"]
            p = p - k["step"] * m / denom
        else:
            p = p - k["step"] * m
    return p, m, s


def yardstick_norm(flat_grad):
    g = np.asarray(flat_grad, np.float64)
    return math.sqrt(float(np.sum(g * g)))


def yardstick_quantile(values, q):
    """np.quantile of the history (float64), rounded to fp32."""
    return float(np.float32(np.quantile(np.asarray(list(values), np.float64), q)))


def yardstick_coef(clip32, norm32):
    return min(1.0, float(clip32) / (float(np.float32(norm32)) + 1e-6))


# ---- the second route: torch fp32, per parameter ---------------------------------------------------------------------------------------
def torch_adabelief_(p, grad, exp_avg, exp_avg_var, t, lr, wd, betas, eps):
    """torch_optimizer.AdaBelief.step for one parameter (weight_decouple, rectify, no amsgrad): the package's in-place tensor calls."""
    beta1, beta2 = betas
    p.mul_(1.0 - lr * wd)
    bias_correction1 = 1 - beta1 ** t
    bias_correction2 = 1 - beta2 ** t
    exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
    grad_residual = grad - exp_avg
    exp_avg_var.mul_(beta2).addcmul_(grad_residual, grad_residual, value=1 - beta2)
    denom = (exp_avg_var.add_(eps).sqrt() / math.sqrt(bias_correction2)).add_(eps)
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    rho_t = rho_inf - 2 * t * beta2 ** t / (1.0 - beta2 ** t)
    if rho_t > 4:
        rt = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / (rho_inf - 4.0) / (rho_inf - 2.0) / rho_t)
        p.addcdiv_(exp_avg, denom, value=-(rt * lr / bias_correction1))
    else:
        p.add_(exp_avg, alpha=-lr)


def torch_route_step(params, states, groups, t, max_norm=None):
    """train.py:242 + :246 on a list of parameters with .grad set: clip_grad_norm_ at max_norm (None: no clipping), then the package's
    update per parameter.  states: {"exp_avg", "exp_avg_var"} per parameter; groups: (parameters, lr, wd, betas, eps).  Returns the norm."""
    norm = None
    if max_norm is not None:
        norm = torch.nn.utils.clip_grad_norm_(params, max_norm)
    with torch.no_grad():
        i = 0
        for ps, lr, wd, betas, eps in groups:
            for p in ps:
                torch_adabelief_(p, p.grad, states[i]["exp_avg"], states[i]["exp_avg_var"], t, lr, wd, betas, eps)
                i += 1
    return norm


def torch_route_flat(p, g, m, s, coef, t, lr, wd, betas, eps):
    """The same calls on flat fp32 copies of one group (the update is element-wise: the result per element is the per-parameter one);
    the clip is clip_grad_norm_'s `grad.mul_(coef)` with the given fp32 coefficient."""
    p, m, s = p.clone(), m.clone(), s.clone()
    g = g.clone().mul_(torch.tensor(float(coef), dtype=torch.float32))
    torch_adabelief_(p, g, m, s, t, lr, wd, betas, eps)
    return p, m, s


def check_against_yardstick(got, yard, torch_res, what):
    """got / torch_res: fp32 numpy; yard: float64.  Returns the worst ratio error / bound (<= 1 passes) after asserting it."""
    got = np.asarray(got, np.float64); tr = np.asarray(torch_res, np.float64)
    with np.errstate(all="ignore"):
        y32 = yard.astype(np.float32)
    fin = np.isfinite(y32)
    # where the yardstick, rounded to fp32, is not finite the op must say the same
    assert np.array_equal(got[~fin], y32[~fin].astype(np.float64), equal_nan=True), what + ": non-finite elements differ"
    if not fin.any():
        return 0.0
    y, gf, tf = yard[fin], got[fin], tr[fin]
    assert np.all(np.isfinite(gf)), what + ": the op is not finite where the yardstick is"
    torch_err = float(np.max(np.abs(tf - y))) if np.all(np.isfinite(tf)) else 0.0
    bound = np.maximum(2.0 * torch_err, 4.0 * EPS32 * np.maximum(np.abs(y), TINY32))
    ratio = np.abs(gf - y) / bound
    worst = float(ratio.max())
    print(f"{what}: worst |op - yardstick| / bound = {worst:.3f} (torch route's worst error {torch_err:.3e})")
    assert worst <= 1.0, f"{what}: element {int(ratio.argmax())} is off by {worst:.2f} x the bound"
    return worst


def teacher_forced_steps(layout, device, family, betas, steps=8, clip_quantile=0.8, wd=None, eps=1e-8, lr=1e-3, schedule=None):
    """Steps 1..steps of the op; at each, the op's own fp32 state before the step goes to the yardstick and to the torch route.
    schedule: an optional callable(opt) -> lr scheduler, stepped after every optimizer step.  Returns the worst ratio."""
    opt, _ = make_optimizer(layout, device, betas=betas, clip_quantile=clip_quantile, wd=wd, eps=eps, lr=lr,
                            history=GradNormHistory(8, device=device) if clip_quantile is not None else None)
    sched = schedule(opt) if schedule else None
    worst = 0.0
    for t in range(1, steps + 1):
        g = gradient(family, opt.numel, t)
        p0, m0, s0 = opt.flat.cpu().clone(), opt.exp_avg.cpu().clone(), opt.exp_avg_var.cpu().clone()
        lrs = [float(pg["lr"]) for pg in opt.param_groups]
        set_grads(opt, g)
        opt.step()
        coef = float(opt.last_coef)
        p1, m1, s1 = opt.flat.cpu().numpy(), opt.exp_avg.cpu().numpy(), opt.exp_avg_var.cpu().numpy()
        for gi, ((lo, hi), pg) in enumerate(zip(group_ranges(opt), opt.param_groups)):
            k = adabelief_scalars(t, lrs[gi], pg["weight_decay"], pg["betas"], pg["eps"])
            yp, ym, ys = yardstick_update(p0[lo:hi].numpy(), g[lo:hi].numpy(), m0[lo:hi].numpy(), s0[lo:hi].numpy(), coef, k)
            tp, tm, ts = torch_route_flat(p0[lo:hi], g[lo:hi], m0[lo:hi], s0[lo:hi], coef, t, lrs[gi], pg["weight_decay"], pg["betas"],
                                          pg["eps"])
            with np.errstate(all="ignore"):           # s overflows fp32 in this very step and the step divides by it
                ok = ~(k["rectified"] & ~np.isfinite(ys.astype(np.float32)) & np.isfinite(s0[lo:hi].numpy()))
            tag = f"{layout}/{family}/b2={betas[1]}/t={t}/group{gi}"
            worst = max(worst, check_against_yardstick(m1[lo:hi], ym, tm.numpy(), tag + "/m"))
            worst = max(worst, check_against_yardstick(s1[lo:hi], ys, ts.numpy(), tag + "/s"))
            # p is compared where the yardstick is finite: a float64 s that is finite where the fp32 one has just overflowed gives another p
            worst = max(worst, check_against_yardstick(p1[lo:hi][ok], yp[ok], tp.numpy()[ok], tag + "/p"))
        if sched is not None:
            sched.step()
    return worst


class HostHistory:
    """MovingBuffer of the reference: a deque and np.quantile."""

    def __init__(self, capacity, init=40.0):
        self.values = collections.deque(maxlen=capacity)
        if init is not None:
            self.values.append(float(np.float32(init)))

    def quantile(self, q):
        return yardstick_quantile(self.values, q)

    def append(self, v):
        self.values.append(float(np.float32(v)))


def ulp_close(got, want, ulps=1):
    got, want = np.float32(got), np.float32(want)
    return abs(float(got) - float(want)) <= ulps * float(np.spacing(np.abs(want)))
