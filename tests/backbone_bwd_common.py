"""Shared by the CPU and GPU tests of the axial attention's backward (tests/test_backbone_bwd.py): the cases of backbone_common with a
fixed cotangent, the float64 truths, torch's own fp32 autograd on identical inputs, the gate, and the calls under test.

Truth: float64 autograd through backbone_common.sdpa with dout ~ N(0, 1), on the CPU.  Yardstick per gradient g in {dq, dk, dv}:
e32_g, the maximum absolute error of torch's own fp32 CPU autograd through the same call.  Gate: max(GATE x e32_g,
4 x 2^-24 x max|truth_g|) with backbone_common's GATE = 8 -- the floor is the one gate_of uses; it is needed because e32 is exactly 0
for dv at Lk = 1 (P = 1, dv = the sum of dout's rows in both) while the kernel's sum over the queries runs in another order.
"""
import functools

import torch

import backbone_common as common

U, GATE = common.U, common.GATE
NAMES = ("dq", "dk", "dv")

# the backward kernel's instantiations <NKT = ceil(Lk / 32), DB = 1 (d <= 32) | 2>: MATRIX_D x MATRIX_LK of backbone_common at
# Lq = MATRIX_LQ, aligned and one float off 16 bytes.  The query side -- partial query tiles, a wave's second query pass (Lq > 128),
# and a key tile whose owner walks eight query tiles (Lq = 256):
QUERY_SIDE = [(Lq, Lk, d) for Lq in (1, 32, 33, 64, 65, 129, 256) for Lk in (100, 256) for d in (32, 64)]


def _grads(q, k, v, dout, H):
    q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
    return torch.autograd.grad(common.sdpa(q, k, v, H), (q, k, v), dout)


@functools.lru_cache(maxsize=None)
def bwd_case(Lq, Lk, H, d, lead=(3,), scale=1.0, kind="randn"):
    """backbone_common.op_case with a cotangent: truth, e32 and gate per gradient, computed once and kept unchanged on the CPU."""
    c = common.op_case(Lq, Lk, H, d, lead, scale, kind)
    g = torch.Generator().manual_seed(9000 + 131 * Lq + 17 * Lk + 5 * H + d + sum(lead))
    dout = torch.randn(*lead, Lq, H * d, generator=g)
    truth = _grads(c["q"].double(), c["k"].double(), c["v"].double(), dout.double(), H)
    t32 = _grads(c["q"], c["k"], c["v"], dout, H)
    e32 = [float((a.double() - b).abs().max()) for a, b in zip(t32, truth)]
    gate = [max(GATE * e, 4 * U * float(t.abs().max())) for e, t in zip(e32, truth)]
    out = dict(c)
    out.update(dout=dout, truth_g=truth, e32_g=e32, gate_g=gate)
    return out


def route_grads(q, k, v, dout, H, route="fused-train", needs=(True, True, True)):
    """(out, dq, dk, dv) of backbone.axial_attention under autograd; None for an input that does not require grad."""
    from transkun_amd import backbone
    ins = [t.detach().clone().requires_grad_(n) for t, n in zip((q, k, v), needs)]
    out = backbone.axial_attention(*ins, H, route=route)
    out.backward(dout)
    return (out.detach(),) + tuple(t.grad for t in ins)


def check_gate(dev, c, tag, grads=None):
    """The gradients of the Python route (or `grads`) against the case's truths, printed and gated per gradient."""
    if grads is None:
        grads = route_grads(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), c["dout"].to(dev), c["H"])[1:]
    worst = 0.0
    for name, got, truth, e32, gate in zip(NAMES, grads, c["truth_g"], c["e32_g"], c["gate_g"]):
        assert got.shape == truth.shape and got.dtype == torch.float32 and got.device.type == dev.type, (tag, name)
        assert bool(torch.isfinite(got).all()), (tag, name)
        e = float((got.cpu().double() - truth).abs().max())
        print(f"axial_attention_bwd [{dev.type}] {tag} {name}: error {e:.3e}  torch fp32 {e32:.3e}  gate {gate:.3e}  "
              f"ratio {e / e32 if e32 > 0 else float('nan'):.2f}")
        assert e <= gate, (tag, name, e, e32, gate)
        worst = max(worst, e / gate)
    return worst


def as4(t):
    """[..., L, HD] contiguous -> the op's 4-d form [n0, 1, L, HD] (a view)."""
    return t.reshape(-1, 1, t.shape[-2], t.shape[-1])


def raw_fwd(q4, k4, v4, H, out=None):
    if out is None:
        out = torch.empty_like(q4.contiguous())
    return common.raw_op(q4, k4, v4, out, H)


def raw_bwd(q4, k4, v4, o4, g4, H, dq=True, dk=True, dv=True):
    """torch.ops.semicrf.axial_attention_bwd on 4-d views; dq / dk / dv: True (a fresh dense tensor), None, or a tensor to write."""
    from transkun_amd import _lib
    fresh = lambda like: torch.full(like.shape, float("nan"), dtype=like.dtype, device=like.device)
    dq = fresh(q4) if dq is True else dq
    dk = fresh(k4) if dk is True else dk
    dv = fresh(v4) if dv is True else dv
    _lib.ops().axial_attention_bwd(q4, k4, v4, o4, g4, dq, dk, dv, H)
    return dq, dk, dv


def raw_case(dev, c, off=False):
    """Forward and backward of a case through the raw ops; off: every tensor, the gradients included, one float off 16 bytes."""
    q4, k4, v4, g4 = (as4(c[n]).to(dev) for n in ("q", "k", "v", "dout"))
    if off:
        q4, k4, v4, g4 = (common.one_float_off(t) for t in (q4, k4, v4, g4))
    o4 = common.one_float_off(torch.zeros_like(q4.contiguous())) if off else None
    o4 = raw_fwd(q4, k4, v4, c["H"], o4)
    grads = [common.one_float_off(torch.zeros_like(t.contiguous())) if off else True for t in (q4, k4, v4)]
    return raw_bwd(q4, k4, v4, o4, g4, c["H"], *grads)
