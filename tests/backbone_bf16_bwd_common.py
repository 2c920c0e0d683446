"""Shared by the CPU and GPU tests of the bf16 axial attention's backward (tests/test_backbone_bf16_bwd.py): the cases, the float64
truths, torch's own bf16 autograd on identical inputs, the gate, the closed-form cotangents of the exact-answer tests and the calls
under test.

Inputs: backbone_common.op_case rounded to bf16; dout ~ N(0, 1) rounded to bf16, seeded as backbone_bwd_common.bwd_case seeds it.
Truth: float64 autograd through backbone_common.sdpa on float64 copies of the ROUNDED tensors, on the CPU.  Yardstick per gradient g in
{dq, dk, dv}: e16_g, the maximum absolute error of torch's own bf16 CPU autograd through the same call on the same bf16 tensors.  Gate:
max(GATE x e16_g, 4 x 2^-9 x max|truth_g|) with GATE = 8 -- the fp32 backward's gate with bf16's half-ulp 2^-9 in place of 2^-24; the
floor is needed where e16 is 0.  Where max|truth_g| is 0 (dq and dk at Lk = 1) the gradient must be exactly zero.
"""
import functools

import torch

import backbone_common as common
import backbone_bf16_common as c16

GATE = common.GATE
HALF_ULP = 2.0 ** -9
BF16 = torch.bfloat16
NAMES = ("dq", "dk", "dv")

# the query count is no template parameter of the kernel: partial query tiles, a wave's second query pass (Lq > 128) and a key tile
# whose owner walks eight query tiles (Lq = 256)
QUERY_SIDE = [(Lq, Lk, d) for Lq in (1, 32, 33, 64, 65, 129, 256) for Lk in (100, 256) for d in (32, 64)]
EXACT_SHAPES = c16.EXACT_SHAPES + [(33, 32, 2, 8), (65, 128, 2, 24)]
KNOBS = dict(route="fused-train", bf16="fused", bf16_train="fused")


def _grads(q, k, v, dout, H):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    return torch.autograd.grad(common.sdpa(q, k, v, H), (q, k, v), dout)


def finish(q, k, v, dout, H):
    truth = _grads(q.double(), k.double(), v.double(), dout.double(), H)
    t16 = _grads(q, k, v, dout, H)
    e16 = [float((a.double() - b).abs().max()) for a, b in zip(t16, truth)]
    gate = [max(GATE * e, 4 * HALF_ULP * float(t.abs().max())) for e, t in zip(e16, truth)]
    return dict(q=q, k=k, v=v, dout=dout, H=H, truth_g=truth, e16_g=e16, gate_g=gate)


@functools.lru_cache(maxsize=None)
def case(Lq, Lk, H, d, lead=(3,), scale=1.0, kind="randn"):
    """One case of the gate, computed once and shared by the CPU and GPU forms (kept unchanged on the CPU)."""
    c = common.op_case(Lq, Lk, H, d, lead, scale, kind)
    g = torch.Generator().manual_seed(9000 + 131 * Lq + 17 * Lk + 5 * H + d + sum(lead))
    dout = torch.randn(*lead, Lq, H * d, generator=g).bfloat16()
    out = finish(c["q"].bfloat16(), c["k"].bfloat16(), c["v"].bfloat16(), dout, H)
    for name in ("logit_min", "logit_max"):
        if name in c:
            out[name] = c[name]
    return out


def train_counts():
    from transkun_amd import backbone
    return dict(backbone.ATTENTION_BF16_TRAIN_ROUTES), dict(backbone.ATTENTION_ROUTES), dict(backbone.ATTENTION_BF16_ROUTES)


def moved(before):
    """The counters that moved since `before`, as three dicts (train, all routes, bf16)."""
    return tuple({n: now[n] - old[n] for n in now if now[n] != old[n]} for now, old in zip(train_counts(), before))


def route_grads(q, k, v, dout, H, needs=(True, True, True), **knobs):
    """(out, dq, dk, dv) of backbone.axial_attention under autograd, all three knobs set unless said otherwise; None for an input that
    does not require grad."""
    from transkun_amd import backbone
    ins = [t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), needs)]
    out = backbone.axial_attention(*ins, H, **dict(KNOBS, **knobs))
    out.backward(dout)
    return (out.detach(),) + tuple(t.grad for t in ins)


def fused_grads(q, k, v, dout, H, needs=(True, True, True)):
    """route_grads, and the counters say that the Function answered and its backward launched the op once."""
    before = train_counts()
    got = route_grads(q, k, v, dout, H, needs)
    assert moved(before) == ({"fused": 1, "bwd": 1}, {"fused-train": 1}, {"fused": 1}), moved(before)
    return got


def check_gate(dev, c, tag, grads=None):
    """The gradients of the Python route (or `grads`) against the case's truths, printed and gated per gradient -> the worst
    error / gate."""
    if grads is None:
        grads = fused_grads(*(c[n].to(dev) for n in ("q", "k", "v", "dout")), c["H"])[1:]
    worst = 0.0
    for name, got, truth, e16, gate in zip(NAMES, grads, c["truth_g"], c["e16_g"], c["gate_g"]):
        assert got.shape == truth.shape and got.dtype == BF16 and got.device.type == dev.type, (tag, name)
        assert bool(torch.isfinite(got).all()), (tag, name)
        e = float((got.cpu().double() - truth).abs().max())
        print(f"axial_attention_bf16_bwd [{dev.type}] {tag} {name}: error {e:.3e}  torch bf16 {e16:.3e}  gate {gate:.3e}  "
              f"ratio {e / e16 if e16 > 0 else float('nan'):.2f}  error / gate {e / gate if gate > 0 else float('nan'):.3f}")
        if float(truth.abs().max()) == 0.0:
            assert e == 0.0, (tag, name, e)                       # a truth of zero: exactly zero
        else:
            assert e <= gate, (tag, name, e, e16, gate)
            worst = max(worst, e / gate)
    return worst


def as4(t):
    """[..., L, HD] contiguous -> the op's 4-d form [n0, 1, L, HD] (a view)."""
    return t.reshape(-1, 1, t.shape[-2], t.shape[-1])


def raw_bwd(q4, k4, v4, g4, H, dq=True, dk=True, dv=True):
    """torch.ops.semicrf.axial_attention_bf16_bwd on 4-d views; dq / dk / dv: True (a fresh dense tensor), None, or a tensor to write."""
    from transkun_amd import _lib
    fresh = lambda like: torch.full(like.shape, float("nan"), dtype=like.dtype, device=like.device)
    dq = fresh(q4) if dq is True else dq
    dk = fresh(k4) if dk is True else dk
    dv = fresh(v4) if dv is True else dv
    _lib.ops().axial_attention_bf16_bwd(q4, k4, v4, g4, dq, dk, dv, H)
    return dq, dk, dv


def raw_case(dev, c, off=False):
    """The backward of a case through the raw op; off: all seven tensors one bf16 element off 16 bytes, with an odd token stride."""
    q4, k4, v4, g4 = (as4(c[n]).to(dev) for n in ("q", "k", "v", "dout"))
    if not off:
        return raw_bwd(q4, k4, v4, g4, c["H"])
    q4, k4, v4, g4 = (c16.one_off(t) for t in (q4, k4, v4, g4))
    grads = [c16.one_off(torch.zeros_like(t.contiguous())) for t in (q4, k4, v4)]
    assert all(t.stride(2) % 2 == 1 for t in (q4, k4, v4, g4, *grads))
    return raw_bwd(q4, k4, v4, g4, c["H"], *grads)


# ---- the exact-answer inputs -------------------------------------------------------------------------------------------------------
def _heads(t, H):
    return common.split_heads(t, H)                               # [S, L, H d] -> [S, H, L, d]


@functools.lru_cache(maxsize=None)
def one_hot_bwd_case(Lq, Lk, H, d):
    """backbone_bf16_common.one_hot_case with dout integers in [-3, 3]: P is exactly one-hot, so dS = 0 (dq, dk all +0 or -0) and dv_j is
    the exact integer sum of dout over the queries that selected j; every |sum| <= 256, so it is a bf16 value and one dropped or
    doubled query shows."""
    c = c16.one_hot_case(Lq, Lk, H, d)
    S = c["q"].shape[0]
    g = torch.Generator().manual_seed(1733 + 7 * Lq + 3 * Lk + H + d)
    dout = torch.randint(-3, 4, (S, Lq, H * d), generator=g).double()
    scores = _heads(c["q"].double(), H) @ _heads(c["k"].double(), H).transpose(-1, -2)       # [S, H, Lq, Lk]
    sel = scores.argmax(dim=-1)
    assert bool((scores.gather(-1, sel[..., None]) == 512.0 * d).all())                        # the selected key's own code
    onehot = torch.zeros_like(scores).scatter_(-1, sel[..., None], 1.0)
    dv = (onehot.transpose(-1, -2) @ _heads(dout, H)).transpose(-2, -3).flatten(-2, -1)        # [S, Lk, H d], exact integers
    assert float(dv.abs().max()) <= 256.0
    return dict(q=c["q"], k=c["k"], v=c["v"], dout=dout.bfloat16(), dv=dv.bfloat16())


@functools.lru_cache(maxsize=None)
def uniform_bwd_case(Lq, Lk, H, d, constant_v=False):
    """backbone_bf16_common.uniform_case (q = 0: every weight 1, P = 1 / Lk) with dout integers in [-8, 8]:
    dv_j = bf16((float)bf16(1.0f / (float)Lk) * sum_i dout_i) for every j, every product and partial sum exact.  constant_v: V the same
    integer row for every key; with Lk a power of two dP is constant over the keys and D equals it exactly, so dq = dk = 0."""
    c = c16.uniform_case(Lq, Lk, H, d)
    S = c["q"].shape[0]
    g = torch.Generator().manual_seed(2311 + 7 * Lq + 3 * Lk + H + d)
    dout = torch.randint(-8, 9, (S, Lq, H * d), generator=g).float()
    ph = (torch.tensor(1.0) / torch.tensor(float(Lk))).bfloat16().float()
    dv = (ph * dout.sum(dim=1, keepdim=True)).bfloat16().expand(S, Lk, H * d).contiguous()
    v = c["v"][:, :1].expand(S, Lk, H * d).contiguous() if constant_v else c["v"]
    return dict(q=c["q"], k=c["k"], v=v, dout=dout.bfloat16(), dv=dv)


def all_zero(t):
    return bool((t.float() == 0.0).all())                         # +0 or -0


# ---- the modules ---------------------------------------------------------------------------------------------------------------------
def training_backbone(name, checkpoint):
    """(the fixture's Backbone with dropoutProb = 0 in training mode, the fixture): float32, on the CPU."""
    from transkun_amd import backbone
    fx = common.fixture(name)
    m = backbone.Backbone(**dict(fx["cfg"], useGradientCheckpoint=checkpoint, dropoutProb=0.0))
    m.load_state_dict(fx["sd"], strict=True)
    return m.train(), fx


def set_knobs(m, fused):
    m.attention = "fused-train" if fused else "torch"
    m.attentionBf16 = "fused" if fused else "torch"
    m.attentionBf16Train = "fused" if fused else "torch"


def flat_grad(m):
    assert all(p.grad is not None for p in m.parameters())
    return torch.cat([p.grad.flatten() for p in m.parameters()]).cpu().double()
