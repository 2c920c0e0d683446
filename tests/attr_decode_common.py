"""The yardstick of the attribute-head readout (transkun_amd.attributes.attribute_decode) and what its tests share.

The definitions in float64 torch on the fp32 inputs:

    p        = softmax(logitsVelocity)                                   (float64)
    hamming  the smallest index of the largest fp32 logit
    mse      sum_w p[w] w
    match    r[v] = sum of p[w], |w - v| <= 12; any v is judged by its slack  max r - r[v]
    mae      cum[v] = p[0] + ... + p[v]; any v is judged by its slack  max(0, 0.5 - cum[v], cum[v - 1] - 0.5)
    ofValue  clamp(sign(l) h(min(|l|, l*)) / 0.99, -0.5, 0.5),  h(a) = 0.5 coth(a / 2) - 1 / a,  l* = log((1 - eps32) / eps32)
    presence l' > 0

`of_value64` is tied to torch.distributions.ContinuousBernoulli(logits=l.double()).mean for |l| <= 12 and to the clamp constant beyond l*
(the two tests at the end of this file, collected by test_attr_decode.py)."""
import math

import torch

from attr_loss_common import EPS32, FLOOR, LSTAR

NVEL = 128
RADIUS = 12                                      # |w - v| < 0.1 * 128
SLACK_MAX = 72 * EPS32                           # an fp32 sum of <= 128 non-negative terms with total <= 1: 128 * 2^-24 = 64 eps32; the terms: 8 eps32
CRITERIA = ("hamming", "mse", "match", "mae")
OF_CONSTANT = 0.4416912                          # h(l*) / 0.99


def mean_shift64(a: torch.Tensor) -> torch.Tensor:
    """h(a), a >= 0 float64: the Maclaurin series below 0.05 (next term 5.3e-10 a^11 < 1e-24), the closed form above (it loses
    eps64 / a <= 5e-15 there)."""
    assert a.dtype == torch.float64
    s = a * a
    series = a * (1.0 / 12 + s * (-1.0 / 720 + s * (1.0 / 30240 + s * (-1.0 / 1209600 + s * (1.0 / 47900160)))))
    safe = torch.where(a < 0.05, torch.ones_like(a), a)
    closed = 0.5 / torch.tanh(safe / 2) - 1.0 / safe
    return torch.where(a < 0.05, series, closed)


def of_value64(l: torch.Tensor, lstar=LSTAR) -> torch.Tensor:
    """ofValue of the module docstring for value logits l (any float dtype; evaluated in float64).  NaN gives NaN.  lstar=None:
    without the probability clamp (the comparison with torch's float64 evaluation)."""
    l = l.double()
    a = l.abs()
    if lstar is not None:
        a = torch.where(a < lstar, a, torch.full_like(a, lstar))
    h = mean_shift64(torch.where(a == a, a, torch.zeros_like(a)))
    v = torch.clamp(torch.where(l < 0, -h, h) / 0.99, -0.5, 0.5)
    return torch.where(l == l, v, torch.full_like(v, float("nan")))


def window_matrix(device="cpu"):
    w = torch.arange(NVEL, device=device)
    return ((w.unsqueeze(1) - w.unsqueeze(0)).abs() <= RADIUS).double()


def finite_rows(lv: torch.Tensor) -> torch.Tensor:
    """Rows whose softmax is finite: no NaN, no +inf, not all -inf."""
    return ~(torch.isnan(lv).any(-1) | (lv == float("inf")).any(-1) | (lv == float("-inf")).all(-1))


def velocity64(lv: torch.Tensor) -> dict:
    """p, r (window sums), cum (float64), the mean, and hamming's exact answer, for the fp32 logits lv [K, 128]."""
    lv = lv.float().cpu()
    p = torch.softmax(lv.double(), -1)
    idx = torch.arange(NVEL).expand_as(lv)
    first = torch.where(lv == lv.max(-1, keepdim=True).values, idx, torch.full_like(idx, NVEL)).min(-1).values
    ok = finite_rows(lv)
    first = torch.where(ok, first, torch.zeros_like(first))
    return dict(p=p, r=p @ window_matrix(), cum=p.cumsum(-1), mean=(p * torch.arange(NVEL, dtype=torch.float64)).sum(-1), hamming=first, finite=ok)


def slack(y: dict, criterion: str, v: torch.Tensor) -> torch.Tensor:
    """How far the classes v [K] are from optimal under the float64 probabilities (0: a maximiser / the median itself)."""
    v = v.long().cpu().unsqueeze(-1)
    if criterion == "match":
        return y["r"].max(-1).values - y["r"].gather(-1, v).squeeze(-1)
    if criterion == "hamming":
        return y["p"].max(-1).values - y["p"].gather(-1, v).squeeze(-1)
    assert criterion == "mae"
    cum = y["cum"]
    here = cum.gather(-1, v).squeeze(-1)
    before = torch.where(v.squeeze(-1) > 0, cum.gather(-1, (v - 1).clamp(min=0)).squeeze(-1), torch.zeros_like(here))
    return torch.maximum(torch.maximum(0.5 - here, before - 0.5), torch.zeros_like(here))


def value_floor(want: torch.Tensor) -> torch.Tensor:
    return FLOOR * want.abs().clamp(min=1.0)


def check_values(name, got, want, torch_got, floor=None):
    """The tolerance rule for values (ofValue, mse): |got - want| <= max(what the torch-fp32 route errs over the same inputs, the floor
    8 eps32 max(1, |value|)), elementwise; NaN exactly where the yardstick has NaN.  Prints the worst errors first; returns them."""
    got, want, torch_got = got.detach().double().cpu(), want.detach().double().cpu(), torch_got.detach().double().cpu()
    floor = value_floor(want) if floor is None else floor
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), (name, "NaN pattern")
    ok = ~nan
    err = (got - want).abs()[ok]
    t_err = (torch_got - want).abs()[ok]
    t_err = t_err[~torch.isnan(t_err)]
    e_op = float(err.max()) if err.numel() else 0.0
    e_torch = float(t_err.max()) if t_err.numel() else 0.0
    fl = floor[ok]
    print(f"{name}: op {e_op:.3e}  torch-fp32 {e_torch:.3e}  floor {float(fl.max()) if fl.numel() else 0.0:.3e}")
    assert bool((err <= fl.clamp(min=e_torch)).all()), (name, e_op, e_torch)
    return e_op, e_torch


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


SWITCH = 1.5                                     # attr_decode_math.h: OF_SERIES_BELOW


def of_value_logits() -> torch.Tensor:
    """The issue's list: 0; the Taylor-window neighbourhood; the sweep -12 .. 12 (97 points); one fp32 step to each side of the
    op's switch point; the clamp neighbourhood and beyond; NaN."""
    small = [1e-4, 3e-3, 0.0039, 0.0040, 0.0041, 0.01]
    big = [15.0, 15.9, 16.0, 16.7, 20.0, 30.0, 60.0]
    sw = torch.tensor([SWITCH], dtype=torch.float32)
    around = [float(torch.nextafter(sw, torch.tensor([0.0]))), SWITCH, float(torch.nextafter(sw, torch.tensor([9.0])))]
    vals = [0.0, -0.0] + [s * v for v in small + around + big for s in (1.0, -1.0)] + [-12.0 + 24.0 * i / 96 for i in range(97)] + [float("nan")]
    return torch.tensor(vals, dtype=torch.float32)


PRESENCE_LOGITS = [50.0, -50.0, 0.0, -0.0, 1e-30, float("nan")]
PEAKS = [0, 5, 12, 13, 64, 115, 127]
VELOCITY_FAMILIES = ["n1", "n6", "n001", "equal", "two_max", "peak80", "bump", "minus_inf"]


def velocity_rows(name: str) -> torch.Tensor:
    """fp32 [K, 128] rows with a finite softmax."""
    if name == "n1":
        return _randn(130, NVEL, seed=1)
    if name == "n6":
        return _randn(130, NVEL, seed=2) * 6.0
    if name == "n001":
        return _randn(130, NVEL, seed=3) * 0.01
    if name == "equal":                          # hamming gives 0
        return torch.tensor([2.5, 0.0, -7.25, 80.0]).unsqueeze(-1).expand(4, NVEL).contiguous()
    if name == "two_max":                        # the first wins
        x = _randn(8, NVEL, seed=4)
        for r, (a, b) in enumerate([(0, 127), (3, 4), (63, 64), (64, 65), (1, 126), (31, 95), (126, 127), (0, 1)]):
            x[r, a] = x[r, b] = 6.0
        return x
    if name == "peak80":                         # one logit at +80: match gives max(0, m - 12), hamming and mae give m, all exactly
        x = _randn(len(PEAKS), NVEL, seed=5)
        for r, m in enumerate(PEAKS):
            x[r, m] = 80.0
        return x
    if name == "bump":                           # a smooth bump plus noise
        c = torch.tensor([0.0, 3.5, 12.0, 40.25, 64.0, 90.5, 120.0, 127.0]).repeat(8).unsqueeze(-1)
        w = torch.arange(NVEL, dtype=torch.float32)
        return -((w - c) / 8) ** 2 + 0.1 * _randn(64, NVEL, seed=6)
    assert name == "minus_inf"                   # some -inf entries, a finite maximum: an ordinary row
    x = _randn(6, NVEL, seed=7)
    x[0, :100] = float("-inf"); x[1, 1::2] = float("-inf"); x[2, 5:] = float("-inf"); x[3, :127] = float("-inf")
    x[4, 64] = float("-inf"); x[5, 0] = float("-inf")
    return x


def nonfinite_rows() -> torch.Tensor:
    """Rows whose softmax is not finite: a NaN (first, middle, last lane), +inf, NaN and +inf, all -inf -- and one ordinary row last."""
    x = _randn(8, NVEL, seed=8)
    x[0, 0] = float("nan"); x[1, 77] = float("nan"); x[2, 127] = float("nan")
    x[3, 9] = float("inf"); x[4, 9] = float("inf"); x[4, 10] = float("inf")
    x[5, 3] = float("nan"); x[5, 4] = float("inf")
    x[6, :] = float("-inf")
    return x


def mixed_rows(K: int):
    """K rows of tame velocity logits (N(0, 6^2)) and head outputs (value logits N(0, 2^2), presence N(0, 1))."""
    lv = _randn(K, NVEL, seed=11) * 6.0
    of = _randn(K, 4, seed=12) * torch.tensor([2.0, 2.0, 1.0, 1.0])
    return lv.contiguous(), of.contiguous()


# ---- the yardstick against torch ---------------------------------------------------------------------------------------
def test_yardstick_matches_continuous_bernoulli_float64():
    """|l| <= 12: the yardstick WITHOUT its eps32 clamp is torch's float64 ContinuousBernoulli.mean, shifted and scaled, to 5e-12
    (torch's own closed form subtracts two terms of size 1 / |l| just outside its Taylor window: eps64 / l^2 = 1.4e-11 / 0.99 at 0.004)."""
    l = torch.cat([torch.linspace(-12, 12, 4801, dtype=torch.float64), of_value_logits().double()])
    l = l[(l.abs() <= 12)]
    want = torch.clamp((torch.distributions.ContinuousBernoulli(logits=l, validate_args=False).mean - 0.5) / 0.99, -0.5, 0.5)
    got = of_value64(l, lstar=None)
    err = float((got - want).abs().max())
    print(f"yardstick vs torch float64 ContinuousBernoulli.mean, |l| <= 12: {err:.2e}")
    assert err <= 5e-12
    assert torch.equal(of_value64(l), got)                                   # the clamp is inactive there


def test_yardstick_clamp_constant():
    """Beyond l* the value is the constant h(l*) / 0.99 = 0.4416912 -- not the unclamped 0.488 at l = 60; continuous at l*; NaN
    stays NaN; 0 gives 0."""
    l = torch.tensor([LSTAR, 15.95, 16.0, 16.7, 20.0, 30.0, 60.0], dtype=torch.float64)
    v = of_value64(torch.cat([l, -l]))
    assert float((v[:7] - v[0]).abs().max()) == 0.0 and torch.equal(v[7:], -v[:7])
    assert abs(float(v[0]) - OF_CONSTANT) <= 5e-8
    assert abs(float(v[0]) - (0.5 / math.tanh(LSTAR / 2) - 1 / LSTAR) / 0.99) <= 1e-15
    assert abs(float(of_value64(torch.tensor([LSTAR - 1e-9], dtype=torch.float64))) - float(v[0])) <= 1e-9
    assert abs(float(of_value64(torch.tensor([60.0]), lstar=None)) - 0.488) < 1e-3
    assert bool(torch.isnan(of_value64(torch.tensor([float("nan")])))[0]) and float(of_value64(torch.tensor([0.0]))) == 0.0
