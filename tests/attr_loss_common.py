"""The yardstick of the attribute-head training loss (transkun_amd.attributes.attribute_log_prob) and what its tests share.

`yardstick_rows` is the definition itself in float64 torch -- per target interval

    lpVel  = logitsVelocity[v] - logsumexp(logitsVelocity)
    lpOF   = sum_j  x_j l_j - softplus(l_j) + logC(l_j),     x_j = r_j * 0.99 + 0.5
    lpPres = sum_j  p_j l'_j - softplus(l'_j)

with logC the ContinuousBernoulli log-normaliser as torch evaluates it for fp32 tensors, i.e. with the probability clamp at
eps32 = 2^-23 written out: log(l / tanh(l / 2)) for |l| < l* = log((1 - eps32) / eps32), logC(l*) beyond (so autograd gives it
a zero derivative there), log 2 at 0.  Gradients come from autograd.  The CPU tests at the end of this file tie it to the
reference twice: to the float64 arrays of tests/golden/attr_loss_small.npz (tools/make_attr_loss_golden.py: the reference's own
expressions in float64) and to torch.distributions.ContinuousBernoulli in float64 where float64's own clamp is inactive.

`torch_route` is the reference's formulation (ModelTransformer.py:290-328) as torch calls, in the dtype of its inputs: the
route a caller would otherwise take, and the first half of the tolerance rule (`check_bound`)."""
import math

import numpy as np
import pytest
import torch

EPS32 = 2.0 ** -23
LSTAR = math.log((1.0 - EPS32) / EPS32)


def log_norm64(l: torch.Tensor, lstar=LSTAR) -> torch.Tensor:
    """logC of the module docstring; l float64.  lstar=None: without the clamp (the comparison with torch's float64 evaluation)."""
    assert l.dtype == torch.float64
    a = l.abs()
    if lstar is not None:
        a = torch.where(a < lstar, a, torch.full_like(a, lstar))           # the clamp: a constant beyond l*
    s = a * a
    # Maclaurin series below 1e-2 (next term 2e-6 a^10 < 1e-25); the closed form above (autograd's 1/a - 1/sinh a loses 2e-14 there)
    series = math.log(2.0) + s * (1.0 / 12 + s * (-7.0 / 1440 + s * (31.0 / 90720 + s * (-127.0 / 4838400))))
    safe = torch.where(a < 1e-2, torch.ones_like(a), a)
    closed = torch.log(safe / torch.tanh(safe / 2))
    return torch.where(a < 1e-2, series, closed)


def _softplus64(l):
    return -torch.nn.functional.logsigmoid(-l)                               # (F.softplus switches to the identity above 20)


def yardstick_rows(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence):
    """(lpVel, lpOF, lpPres), float64 [K] each, differentiable w.r.t. the first two arguments if they are float64 leaves."""
    lv, of = logitsVelocity.double(), ofLogits.double()
    lpVel = (lv.gather(-1, velocity.long().unsqueeze(-1)).squeeze(-1) - torch.logsumexp(lv, -1)) if lv.shape[0] else lv.sum(-1)
    x = ofRefined.double() * 0.99 + 0.5
    l, lp = of[:, :2], of[:, 2:]
    lpOF = (x * l - _softplus64(l) + log_norm64(l)).sum(-1)
    lpPres = (ofPresence.double() * lp - _softplus64(lp)).sum(-1)
    return lpVel, lpOF, lpPres


def scatter_index(offsets):
    counts = (offsets[1:] - offsets[:-1]).long()
    return torch.repeat_interleave(torch.arange(counts.numel(), device=offsets.device), counts)


def yardstick(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, base=None, gout=None):
    """out [C] in float64 (the rows summed exactly enough: float64), the three row terms, and -- with gout [C] -- the gradients
    of (out * gout).sum() w.r.t. the two raw head outputs."""
    lv = logitsVelocity.detach().double().requires_grad_(gout is not None)
    of = ofLogits.detach().double().requires_grad_(gout is not None)
    terms = yardstick_rows(lv, of, velocity, ofRefined, ofPresence)
    C = offsets.numel() - 1
    out = torch.zeros(C, dtype=torch.float64, device=lv.device) if base is None else base.detach().double().reshape(C).clone()
    out = out.index_add(0, scatter_index(offsets), terms[0] + terms[1] + terms[2])
    res = dict(out=out.detach(), lpVel=terms[0].detach(), lpOF=terms[1].detach(), lpPres=terms[2].detach())
    if gout is not None:
        (out * gout.double().expand(C)).sum().backward()
        res["dLogitsVelocity"], res["dOfLogits"] = lv.grad, of.grad
    return res


def torch_route(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, base=None):
    """ModelTransformer.py:290-328 on the heads' raw outputs, written as the torch calls the reference makes; differentiable."""
    C = offsets.numel() - 1
    logProb = torch.zeros(C, dtype=logitsVelocity.dtype, device=logitsVelocity.device) if base is None else base.reshape(C)
    if logitsVelocity.shape[0] == 0:                                           # :273
        return logProb
    logits = torch.nn.functional.log_softmax(logitsVelocity, dim=-1)                                     # :291
    logProbVelocity = torch.gather(logits, dim=-1, index=velocity.long().unsqueeze(-1)).squeeze(-1)      # :295
    refined = ofRefined.to(logitsVelocity.dtype) * 0.99 + 0.5                                            # :304
    ofValue, ofPres = ofLogits.chunk(2, dim=-1)                                                          # :306
    logProbOF = torch.distributions.ContinuousBernoulli(logits=ofValue).log_prob(refined).sum(-1)        # :311-313
    logProbOFPresence = torch.distributions.Bernoulli(logits=ofPres).log_prob(ofPresence.to(logitsVelocity.dtype)).sum(-1)   # :315-317
    return logProb.scatter_add(-1, scatter_index(offsets), logProbVelocity + logProbOF + logProbOFPresence)   # :328


def torch_route_grads(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, gout, base=None):
    lv = logitsVelocity.detach().clone().requires_grad_()
    of = ofLogits.detach().clone().requires_grad_()
    out = torch_route(lv, of, velocity, ofRefined, ofPresence, offsets, base)
    (out * gout.expand_as(out)).sum().backward()
    return out.detach(), lv.grad, of.grad


FLOOR = 8 * EPS32          # per row term: seven roundings of a 128-term tree plus one


def value_floor(y, offsets):
    """[C]: 8 eps32 max(1, |term|), summed over the three terms of every row of the chain (rows add linearly)."""
    f = sum(FLOOR * t.abs().clamp(min=1.0) for t in (y["lpVel"], y["lpOF"], y["lpPres"]))
    return torch.zeros(offsets.numel() - 1, dtype=torch.float64, device=f.device).index_add(0, scatter_index(offsets), f)


def grad_floor(want, gout_rows=None):
    """8 eps32 max(1, |value|) per element, times |g| of the element's chain (the gradient is g times a row quantity)."""
    f = FLOOR * want.abs().clamp(min=1.0)
    return f if gout_rows is None else torch.maximum(f, FLOOR * gout_rows.abs().double().unsqueeze(-1).expand_as(f))


def check_bound(name, got, want, torch_got, floor):
    """The tolerance rule: |got - want| <= max(error of the torch-fp32 route over the same family, floor), elementwise.
    Prints both routes' worst errors (the figures of DESIGN.md) before asserting; returns them."""
    err = (got.double() - want).abs()
    e_torch = float((torch_got.double() - want).abs().max()) if want.numel() else 0.0
    e_op = float(err.max()) if want.numel() else 0.0
    print(f"{name}: op {e_op:.3e}  torch-fp32 {e_torch:.3e}  floor {float(floor.max()) if floor.numel() else 0.0:.3e}")
    bound = floor.clamp(min=e_torch)
    assert bool((err <= bound).all()), (name, e_op, e_torch, float(floor.max()))
    return e_op, e_torch


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _hash(n, seed, device="cpu"):
    from transkun_amd import synth
    return synth.hash_normal(n, seed, device)


TAYLOR = [0.0, 1e-4, 3e-3, 0.0039, 0.0040, 0.0041, 0.01]
CLAMP = [15.0, 15.9, 16.0, 16.7, 20.0, 30.0, 60.0]
FAMILIES = ["taylor", "sweep12", "clamp", "presence", "vel_equal", "vel_peak", "vel_noise"]


def family(name, device="cpu"):
    """One row per chain (C = K), so every output is one row's three terms.  Returns (logitsVelocity, ofLogits, velocity, ofRefined,
    ofPresence, offsets).  The parts a family does not vary are tame hash noise (|.| < 4)."""
    if name == "taylor":
        vals = [s * v for v in TAYLOR for s in (1.0, -1.0)][1:]
    elif name == "sweep12":
        vals = [-12.0 + 24.0 * i / 96 for i in range(97)]
    elif name == "clamp":
        vals = [s * v for v in CLAMP for s in (1.0, -1.0)]
    else:
        vals = [0.7 * i - 3.0 for i in range(9)]
    # every value logit with every refinement (-0.5, 0, 0.5), in both columns (column 1 runs through the values in reverse)
    l0 = [v for v in vals for _ in range(3)]
    l1 = [v for v in reversed(vals) for _ in range(3)]
    r0 = [(-0.5, 0.0, 0.5)[i % 3] for i in range(len(l0))]
    r1 = [(0.5, -0.5, 0.0)[i % 3] for i in range(len(l0))]
    K = len(l0)
    pres = _hash(2 * K, 31).view(K, 2)
    ptar = (_hash(2 * K, 32).view(K, 2) > 0).float()
    if name == "presence":
        K = 6 * 3
        l0, l1, r0, r1 = l0[:K], l1[:K], r0[:K], r1[:K]
        pl = [-50.0, 0.0, 50.0]
        pres = torch.tensor([[pl[i % 3], pl[(i // 3) % 3]] for i in range(K)])
        ptar = torch.tensor([[float(i // 9), float((i // 3) % 2)] for i in range(K)])
    lv = _hash(K * 128, 33).view(K, 128)
    vel = (torch.arange(K) * 37 + 5) % 128
    if name == "vel_equal":
        lv = torch.full((K, 128), 2.5)
    elif name == "vel_peak":
        lv = lv.clone()
        lv[torch.arange(K), (torch.arange(K) * 5) % 128] += 80.0               # one logit 80 above the rest
        vel = torch.where(torch.arange(K) % 2 == 0, (torch.arange(K) * 5) % 128, vel)       # the peak itself, or another class
    elif name == "vel_noise":
        lv = lv * (6.0 / 1.1547)                                             # N(0, 6^2)
    if name.startswith("vel_"):
        vel = vel.clone()
        vel[0], vel[1] = 0, 127                                              # first and last lane
    of = torch.cat([torch.tensor([l0, l1], dtype=torch.float32).t(), pres[:K].float()], dim=1).contiguous()
    refined = torch.tensor([r0, r1], dtype=torch.float32).t().contiguous()
    offsets = torch.arange(K + 1, dtype=torch.int32)
    return tuple(t.to(device) for t in (lv.float().contiguous(), of, vel.to(torch.int32), refined, ptar[:K].contiguous(), offsets))


def hash_counts(C):
    from transkun_amd import synth
    return [int(h % np.uint64(7)) for h in synth.hash_u64_numpy(np.arange(C, dtype=np.uint64), 77)]


SHAPES = {"C1_K1": [1], "C3_K0": [0, 0, 0], "C5": [0, 3, 0, 1, 0], "C65": [1] * 65, "C2_long": [130, 1], "C360": None}


def shape_case(name, device="cpu", seed=50):
    """Tame rows (value logits N(0, 2.3^2), everything else N(0, 1.15^2)) for the chain counts of SHAPES[name]; + base and gout."""
    counts = SHAPES[name] if SHAPES[name] is not None else hash_counts(360)
    C, K = len(counts), sum(counts)
    lv = _hash(K * 128, seed).view(K, 128)
    of = _hash(K * 4, seed + 1).view(K, 4) * torch.tensor([2.0, 2.0, 1.0, 1.0])
    vel = ((torch.arange(K) * 37 + 5) % 128).to(torch.int32)
    refined = (_hash(K * 2, seed + 2).view(K, 2) / 8).clamp(-0.5, 0.5)
    pres = (_hash(K * 2, seed + 3).view(K, 2) > 0).float()
    offsets = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)
    base = _hash(C, seed + 4) * 50
    gout = _hash(C, seed + 5)
    return tuple(t.to(device) for t in (lv.contiguous(), of.contiguous(), vel, refined.contiguous(), pres.contiguous(), offsets, base, gout))


# ---- the golden's shape (tools/make_attr_loss_golden.py builds the same inputs) -----------------------------------------------
GOLDEN_CASE = dict(N=2, P=5, T=40, D=32, H=48, seed=21, hop=1024, fs=44100, pitches=[-64, 60, 61, 62, 63])


def golden_inputs(device="cpu"):
    """ctx [N, P, T, D], the scorer's Linear (W, bias) and the two heads' weights, from the integer hash (nothing of it is stored)."""
    c = GOLDEN_CASE
    N, P, T, D, H, seed = c["N"], c["P"], c["T"], c["D"], c["H"], c["seed"]
    ctx = _hash(N * P * T * D, 200 + seed, device).view(N, P, T, D) * 0.5
    W = _hash((2 * D + 1) * D, 300 + seed, device).view(2 * D + 1, D) * (0.3 / D ** 0.5)
    bias = _hash(2 * D + 1, 400 + seed, device) * 0.1
    heads = {}
    for nm, nout, sd, scale in (("velocity", 128, 820, 2.0), ("of", 4, 830, 3.0)):       # value logits within about +-8
        heads[nm] = (_hash(H * 3 * D, sd + seed, device).view(H, 3 * D) * (1.0 / (3 * D) ** 0.5), _hash(H, sd + 1 + seed, device) * 0.1,
                     _hash(nout * H, sd + 2 + seed, device).view(nout, H) * (scale / H ** 0.5), _hash(nout, sd + 3 + seed, device) * 0.1)
    return ctx, W, bias, heads


def golden_transcriber(device="cpu"):
    """A SegmentTranscriber with the golden's weights, in eval mode."""
    from transkun_amd.transcribe import SegmentTranscriber
    c = GOLDEN_CASE
    ctx, W, bias, heads = golden_inputs(device)
    m = SegmentTranscriber(size=c["D"], velocityPredictorHiddenSize=c["H"], refinedOFPredictorHiddenSize=c["H"], hopSize=c["hop"], fs=c["fs"],
                           targetMIDIPitch=c["pitches"]).to(device)
    with torch.no_grad():
        m.scorer.map[0].weight.copy_(W); m.scorer.map[0].bias.copy_(bias)
        for mod, w in ((m.velocityPredictor, heads["velocity"]), (m.refinedOFPredictor, heads["of"])):
            mod[0].weight.copy_(w[0]); mod[0].bias.copy_(w[1]); mod[3].weight.copy_(w[2]); mod[3].bias.copy_(w[3])
    return m.eval(), ctx


def golden_targets(g):
    """(intervalsBatch [N][P] lists, velocity, ofRefined, ofPresence flat in chain order) from the fixture."""
    c = GOLDEN_CASE
    off = [int(x) for x in g["offsets"]]
    flat = [[(int(b), int(e)) for b, e in g["pairs"][off[i]:off[i + 1]]] for i in range(len(off) - 1)]
    batch = [flat[n * c["P"]:(n + 1) * c["P"]] for n in range(c["N"])]
    return batch, torch.from_numpy(g["velocity"]), torch.from_numpy(g["ofRefined"]), torch.from_numpy(g["ofPresence"])


# ---- the yardstick against the reference ---------------------------------------------------------------------------------
def test_yardstick_matches_golden_float64():
    """The float64 arrays of the fixture are the reference's own expressions (log_softmax, ContinuousBernoulli, Bernoulli,
    scatter_add) evaluated in float64 on the stored head outputs; |logits| <= 8 there, far inside either clamp."""
    from conftest import load_golden
    g = load_golden("attr_loss_small")
    t = {k: torch.from_numpy(g[k]) for k in ("logitsVelocity", "ofLogits", "velocity", "ofRefined", "ofPresence")}
    offsets = torch.from_numpy(g["offsets"].astype(np.int32))
    C = offsets.numel() - 1
    y = yardstick(t["logitsVelocity"], t["ofLogits"], t["velocity"], t["ofRefined"], t["ofPresence"], offsets,
                  gout=torch.full((C,), -1.0 / GOLDEN_CASE["N"], dtype=torch.float64))
    for got, key in ((y["lpVel"], "lpVel64"), (y["lpOF"], "lpOF64"), (y["lpPres"], "lpPres64"), (y["out"], "attr64"),
                     (y["dLogitsVelocity"], "dLogitsVelocity64"), (y["dOfLogits"], "dOfLogits64")):
        want = torch.from_numpy(g[key]).reshape(got.shape)
        err = float(((got - want).abs() / want.abs().clamp(min=1.0)).max())
        assert err <= 1e-12, (key, err)


def test_yardstick_matches_continuous_bernoulli_float64():
    """|l| <= 30, where float64's own clamp (eps64) is inactive: the yardstick WITHOUT its eps32 clamp is torch's float64
    ContinuousBernoulli.log_prob, value and gradient.  The bound is torch's own error there: it works from p = sigmoid(l), and
    towards l = +30 the 1 - p inside log1p(-p) carries sigmoid's rounding (~1 ulp of 1) relative to 1 - p = exp(-l), which
    log|log1p(-p) - log p| divides by |l|: 2 eps64 exp(|l|) / |l|; just outside its Taylor window (|l| > 0.004) its closed form
    subtracts two terms of size 1/|l| whose derivatives are of size 1/l^2: eps64 / l^2 (1.3e-11 at 0.0041, measured 4.2e-12); and
    1e-12 for everything else (measured: 1.3e-13 below |l| = 1, 1.9e-12 up to 12, 6.3e-11 at 15.6).
    With the clamp: constant beyond l*, zero derivative."""
    eps64 = 2.0 ** -52
    l = torch.cat([torch.linspace(-30, 30, 2401, dtype=torch.float64), torch.tensor([s * v for v in TAYLOR + CLAMP for s in (1.0, -1.0)], dtype=torch.float64)])
    l = l[l.abs() <= 30]
    x = torch.linspace(0.005, 0.995, l.numel(), dtype=torch.float64)
    lt = l.clone().requires_grad_()
    want = torch.distributions.ContinuousBernoulli(logits=lt).log_prob(x)
    want.sum().backward()
    ly = l.clone().requires_grad_()
    got = x * ly - _softplus64(ly) + log_norm64(ly, lstar=None)
    got.sum().backward()
    tol = 1e-12 + 2 * eps64 * torch.exp(l.abs()) / l.abs().clamp(min=1.0) + eps64 / (l * l).clamp(min=0.004 ** 2)
    assert bool(((got - want).detach().abs() <= tol).all())
    assert bool(((ly.grad - lt.grad).abs() <= tol).all())
    print("yardstick vs torch float64, |l| <= 12: %.2e" % float((got - want).detach().abs()[l.abs() <= 12].max()))
    # the clamp written out
    lc = torch.tensor([-60.0, -16.0, -LSTAR, LSTAR, 15.95, 30.0], dtype=torch.float64, requires_grad=True)
    c = log_norm64(lc)
    c.sum().backward()
    assert float((c.detach() - math.log(LSTAR / (1 - 2 * EPS32))).abs().max()) <= 1e-14 and float(lc.grad.abs().max()) == 0.0
    below = torch.tensor([LSTAR - 1e-9], dtype=torch.float64)
    assert abs(float(log_norm64(below)) - float(c[0].detach())) <= 1e-9                 # continuous at l*
