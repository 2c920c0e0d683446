"""Shared by the CPU and GPU tests of the attribute heads in training (tests/test_attr_heads_train.py): seeded cases on the shapes of
attr_heads_common, the float64 yardstick of the forward and of the nine gradients, and torch's own fp32 modules under autograd.

Yardstick: the same modules in float64 on the CPU, dropout written as an explicit multiplication by the op's own mask
(attributes.attribute_heads_dropout_mask, host mirror): Linear -> GELU -> * mask / (1 - p) -> Linear on x = [a | b | a * b] formed in
float64 from the fp32 ctx; seeded random cotangents dLv, dOf through torch.autograd.grad.  Gate per tensor (the forward's two outputs,
dctx and the eight parameter gradients): max abs error <= GATE x max(error of torch's fp32 modules under autograd on the CPU with the
identical mask and inputs, u max|truth|), GATE = 8 and its reasoning from attr_heads_common, u = 2^-24: the second term is the
result's own representation error and keeps a tensor that torch happens to get exactly from gating at zero."""
import copy
import functools

import torch

import attr_heads_common as common

NAMES = ("dctx", "v1.weight", "v1.bias", "v2.weight", "v2.bias", "o1.weight", "o1.bias", "o2.weight", "o2.bias")


def params_of(vp, op):
    return [vp[0].weight, vp[0].bias, vp[-1].weight, vp[-1].bias, op[0].weight, op[0].bias, op[-1].weight, op[-1].bias]


def make_train_heads(D, Hv, Ho, seed, pv=0.1, po=0.1, Nv=128, No=4):
    """attr_heads_common.make_heads in TRAINING mode, with the two dropout probabilities."""
    vp, op = common.make_heads(D, Hv, Ho, seed, Nv, No)
    vp, op = copy.deepcopy(vp), copy.deepcopy(op)
    vp[2].p, op[2].p = pv, po
    return vp.train(), op.train()


def mask_of(seed, K, Hv, Ho, pv, po, device="cpu"):
    from transkun_amd import attributes
    return attributes.attribute_heads_dropout_mask(seed, K, Hv, Ho, pv, po, device)


def modules_with_mask(ctx, pairs, offsets, K, vp, op, mask, pv, po, dlv, dof, dtype):
    """The modules in `dtype` on the CPU, dropout as a multiplication by mask / (1 - p): (logitsVelocity, ofLogits) and the nine
    gradients of the cotangents (dlv, dof), in the order of NAMES."""
    vp2, op2 = copy.deepcopy(vp).to(dtype), copy.deepcopy(op).to(dtype)
    Hv = vp2[0].out_features
    c = ctx.detach().float().to(dtype).requires_grad_()
    a, b, _ = common.gather_ab(c, pairs, offsets, K)
    x = torch.cat([a, b, a * b], dim=-1)
    outs = []
    for head, m, p in ((vp2, mask[:, :Hv], pv), (op2, mask[:, Hv:], po)):
        h = torch.nn.functional.gelu(head[0](x))
        if p > 0:
            h = h * (m.to(dtype) / (1.0 - p))
        outs.append(head[-1](h))
    grads = torch.autograd.grad(outs, [c] + params_of(vp2, op2), [dlv.to(dtype), dof.to(dtype)])
    return outs[0].detach(), outs[1].detach(), [g.detach() for g in grads]


def make_case(D, Hv, Ho, scale, pv, po, K, seed, Nv=128, No=4, layout=None):
    """layout: (pairs int32 [K, 2] inside [0, T - 1], offsets int32 [C + 1]) in place of the seeded rows of make_rows (rows past
    offsets[-1] belong to the last chain).  The case keeps torch's fp32 results ("f32") next to their errors ("e32")."""
    vp, op = make_train_heads(D, Hv, Ho, seed, pv, po, Nv, No)
    ctx = common.make_ctx(D, scale, seed + 1)
    pairs, offsets = common.pack_rows(common.make_rows(K, seed + 2)) if layout is None else layout
    g = torch.Generator().manual_seed(seed + 3)
    dlv, dof = torch.randn(K, Nv, generator=g), torch.randn(K, No, generator=g)
    mseed = 0x9E3779B97F4A7C15 ^ (seed * 1000003)            # (above 2^63: the whole 64 bits travel)
    mask = mask_of(mseed, K, Hv, Ho, pv, po)
    tv, to, tg = modules_with_mask(ctx, pairs, offsets, K, vp, op, mask, pv, po, dlv, dof, torch.float64)
    fv, fo, fg = modules_with_mask(ctx, pairs, offsets, K, vp, op, mask, pv, po, dlv, dof, torch.float32)
    truth = [tv, to] + tg
    e32 = [float((f.double() - t).abs().max()) for f, t in zip([fv, fo] + fg, truth)]
    return dict(vp=vp, op=op, ctx=ctx, pairs=pairs, offsets=offsets, K=K, dlv=dlv, dof=dof, seed=mseed, mask=mask, truth=truth, e32=e32,
                pv=pv, po=po, f32=[fv, fo] + fg)


@functools.lru_cache(maxsize=None)
def gate_case(D, Hv, Ho, scale, pv=0.1, po=0.1):
    """One case of the gate at K = 97, computed once and shared by the CPU and GPU forms."""
    return make_case(D, Hv, Ho, scale, pv, po, common.K_GATE, 2000 + 7 * D + Hv + int(scale) + int(100 * po))


@functools.lru_cache(maxsize=None)
def chunk_case(D, Hv, Ho, K):
    """Rows across the backward's row chunks (K: three chunks and a ragged remainder)."""
    return make_case(D, Hv, Ho, 1.0, 0.1, 0.1, K, 3000 + D)


def run_op(dev, c, seed=None, train=True):
    """The op on `dev` on a case's inputs: (logitsVelocity, ofLogits, [dctx + the eight parameter gradients])."""
    from transkun_amd import attributes
    vp, op = copy.deepcopy(c["vp"]).to(dev), copy.deepcopy(c["op"]).to(dev)
    vp.train(train); op.train(train)
    ctx = c["ctx"].detach().to(dev).requires_grad_()            # a leaf of its own: the cached case stays as it is
    lv, of, sym, sc = attributes.attribute_heads_train(ctx, c["pairs"].to(dev), c["offsets"].to(dev), vp, op, c["K"],
                                                       seed=c["seed"] if seed is None else seed)
    grads = torch.autograd.grad([lv, of], [ctx] + params_of(vp, op), [c["dlv"].to(dev), c["dof"].to(dev)])
    return lv.detach(), of.detach(), list(grads)


def check_gate(tag, names, got, truth, e32):
    """Prints every ratio, then asserts the gate per tensor."""
    bad = []
    for name, g, t, e in zip(names, got, truth, e32):
        assert g.shape == t.shape, (name, g.shape, t.shape)
        err = float((g.detach().cpu().double() - t).abs().max())
        floor = max(e, common.U * float(t.abs().max()))
        print(f"{tag} {name}: error {err:.3e}  torch fp32 {e:.3e}  u max|truth| {common.U * float(t.abs().max()):.3e}  "
              f"ratio {err / floor:.2f} (gate {common.GATE:g})")
        if not err <= common.GATE * floor:
            bad.append((name, err, floor))
    assert not bad, bad
