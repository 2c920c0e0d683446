"""Shared by the CPU and GPU tests of the fused feed-forward ResBlock's training route (tests/test_feed_forward_train.py): seeded
cases, the float64 yardstick with the op's own dropout masks as explicit multiplications, the stock fp32 modules under autograd on
identical inputs and masks, and the gate.

Yardstick: out = x + ((W2 (gelu(W1 rmsnorm(x) + b1) * M1) + b2) * M2) * scale in float64 on the CPU under autograd, M1 = keep1 / (1 - p1)
and M2 = keep2 / (1 - p2) from feed_forward_dropout_mask (the op's own mask; row i = token i in the order of the addresses), loss =
sum(out * G) for a fixed G (so dout = G).  Gate per tensor (the GATE = 8 idiom of ffn_common and attr_heads_train_common): the maximum
absolute error is at most GATE x max(e32, 2^-24 x max|truth|), e32 being the error of the same expression on torch's fp32 modules under
autograd on the CPU with the same masks.

Cases are built once on the CPU (lru_cache) and never modified; the GPU tests move copies.
"""
import functools
import math

import torch

import ffn_common

U = 2.0 ** -24
GATE = 8.0
NAMES = ("out", "dx", "dW1", "db1", "dW2", "db2", "dscale")
ROWS = [1, 63, 64, 65, 129]
SHAPES = [(8, 8), (40, 72), (160, 640), (256, 1032)]


def masks_for(seed, x, hidden, p1, p2):
    """The op's two masks laid out like x: ([..., hidden], [..., D]) as float64 factors keep / (1 - p).  Row i of the op's mask is
    token i in the order of the addresses of x's tokens."""
    from transkun_amd import backbone
    D = x.shape[-1]
    rows = x.numel() // D
    mh, mo = backbone.feed_forward_dropout_mask(seed, rows, D, hidden, p1, p2, "cpu")
    order = sorted(range(x.dim() - 1), key=lambda i: -x.stride(i))
    inv = [order.index(i) for i in range(x.dim() - 1)]
    lead = [x.shape[i] for i in order]
    f1 = mh.view(*lead, hidden).permute(*inv, -1).double() / (1.0 - p1)
    f2 = mo.view(*lead, D).permute(*inv, -1).double() / (1.0 - p2)
    return f1, f2


def expression(x, w1, b1, w2, b2, scale, eps, f1, f2, act=None):
    """The block with explicit masks in the dtype of its arguments (torch's own ops: F.linear, F.gelu)."""
    import torch.nn.functional as F
    act = F.gelu if act is None else act
    xn = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    return x + (F.linear(act(F.linear(xn, w1, b1)) * f1.to(x.dtype), w2, b2) * f2.to(x.dtype)) * scale


def reference(x, params, eps, f1, f2, G, dtype, act=None):
    """(out, dx, dW1, db1, dW2, db2, dscale) of the expression under autograd in `dtype` on the CPU, as float64."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in (x, *params)]
    out = expression(*leaves, eps, f1, f2, act)
    grads = torch.autograd.grad((out * G.to(dtype)).sum(), leaves)
    return [out.detach().double()] + [g.double() for g in grads]


@functools.lru_cache(maxsize=None)
def case(rows, D, hidden, scale_kind="randn", mult=1.0, p1=0.1, p2=0.5, seed=1234):
    g = torch.Generator().manual_seed(77000 + 7 * rows + 131 * D + 17 * hidden + (1 if scale_kind == "init" else 0) + int(10 * mult))
    blk = ffn_common.stock_modules(D, hidden, g)
    if scale_kind == "randn":
        with torch.no_grad():
            blk.scale.copy_(torch.randn(D, generator=g))
    x = torch.randn(rows, D, generator=g) * mult
    G = torch.randn(rows, D, generator=g)
    params = tuple(p.detach().clone() for p in (blk.module[0].weight, blk.module[0].bias, blk.module[3].weight, blk.module[3].bias, blk.scale))
    f1, f2 = masks_for(seed, x, hidden, p1, p2)
    truth = reference(x, params, blk.norm.eps, f1, f2, G, torch.float64)
    t32 = reference(x, params, blk.norm.eps, f1, f2, G, torch.float32)
    e32 = [float((a - b).abs().max()) for a, b in zip(t32, truth)]
    gates = [GATE * max(e, U * float(t.abs().max())) for e, t in zip(e32, truth)]
    return dict(x=x, G=G, params=params, eps=blk.norm.eps, truth=truth, e32=e32, gates=gates, D=D, hidden=hidden, p1=p1, p2=p2, seed=seed)


def run(c, dev, x=None, G=None, seed=None):
    """The fused training route on the case (the host mirrors for the CPU): [out, dx, dW1, db1, dW2, db2, dscale] on the CPU."""
    from transkun_amd import backbone
    x = (c["x"] if x is None else x).to(dev).detach().clone().requires_grad_()
    G = (c["G"] if G is None else G).to(dev)
    params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
    before = dict(backbone.FEED_FORWARD_TRAIN_ROUTES)
    out = backbone.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", p_hidden=c["p1"], p_out=c["p2"],
                                         seed=c["seed"] if seed is None else seed)
    grads = torch.autograd.grad((out * G).sum(), [x] + params)
    after = backbone.FEED_FORWARD_TRAIN_ROUTES
    assert (after["fused"] - before["fused"], after["torch"] - before["torch"], after["bwd"] - before["bwd"]) == (1, 0, 1)
    return [out.detach().cpu()] + [g.cpu() for g in grads]


def worst(got, c):
    """(ratio, name): the largest error / gate over the seven tensors."""
    ratios = [(float((a.double() - t).abs().max()) / gate, n) for a, t, gate, n in zip(got, c["truth"], c["gates"], NAMES)]
    return max(ratios)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- exact answers -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_case(rows, D, hidden, seed=99):
    """Inputs on which every intermediate of forward and backward is exactly representable whatever the order of summation: eps = 0,
    x = +-1 (rs = 1, xn = x), W1 in {-1, 0, 1} with at most 8 non-zeros a row, b1 = +-32 (z = +-32 + a small integer: gelu(z) = z or 0
    and gelu'(z) = 1 or 0 in fp32 and fp64 alike), W2 in {-1, 0, 1}, b2 small integers, scale = 2^-6, dout small integers, p = (0.5, 0.5)
    (masks 0 or 2).  With |z| >= 24 the fp32 gelu IS max(z, 0) and its derivative IS 0 or 1 (erfc and exp underflow), while float64
    still sees 1e-126: the truth takes max(z, 0) for gelu, and `exact` says whether that and the integrality of every result hold."""
    g = torch.Generator().manual_seed(4242 + rows + 3 * D + 5 * hidden)
    x = (torch.randint(0, 2, (rows, D), generator=g) * 2 - 1).float()
    w1 = torch.zeros(hidden, D)
    for j in range(hidden):
        cols = torch.randperm(D, generator=g)[:8]
        w1[j, cols] = (torch.randint(0, 2, (cols.numel(),), generator=g) * 2 - 1).float()
    b1 = (torch.randint(0, 2, (hidden,), generator=g) * 2 - 1).float() * 32
    nz = (torch.rand(D, hidden, generator=g) < min(1.0, 8.0 / hidden)).float()
    w2 = nz * (torch.randint(0, 2, (D, hidden), generator=g) * 2 - 1).float()
    b2 = torch.randint(-2, 3, (D,), generator=g).float()
    scale = torch.full((D,), 2.0 ** -6)
    G = torch.randint(-2, 3, (rows, D), generator=g).float()
    params = (w1, b1, w2, b2, scale)
    f1, f2 = masks_for(seed, x, hidden, 0.5, 0.5)
    truth = reference(x, params, 0.0, f1, f2, G, torch.float64, act=torch.relu)
    # every result is an integer over its own 2^k (k <= 14) of at most 23 bits: sums of such terms are exact in any order
    def small_integers(t):
        for k in range(15):
            q = t * 2.0 ** k
            if bool((q == q.round()).all()):
                return float(q.abs().max()) < 2.0 ** 23
        return False

    exact = all(small_integers(t) for t in truth)
    # the intermediates: z = W1 x + b1 is an integer with |z| >= 24; gelu is max(z, 0) in fp32 exactly and in float64 to 1e-100
    z = x.double() @ w1.double().T + b1.double()
    a = 0.5 * z * torch.special.erfc(-z / math.sqrt(2.0))
    exact = exact and bool(((a - torch.relu(z)).abs() < 1e-100).all()) and bool((z.abs() >= 24).all()) and bool((z == z.round()).all())
    exact = exact and bool((torch.nn.functional.gelu(z.float()) == torch.relu(z.float())).all())
    return dict(x=x, G=G, params=params, eps=0.0, truth=truth, exact=exact, D=D, hidden=hidden, p1=0.5, p2=0.5, seed=seed,
                gates=[0.0] * 7, e32=[0.0] * 7)


# ---- the modules -------------------------------------------------------------------------------------------------------------------------
def patch_reference_blocks(model, p):
    """Every feed-forward ResBlock of `model` (any dtype, on the CPU) answers with the expression above: it draws the seed as the fused
    route does (two 32-bit words from torch's CPU default generator per call, in call order) and multiplies the op's own masks."""
    import types

    def fwd(self, x, *args):
        assert not args
        lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
        m = self.module
        f1, f2 = masks_for((hi << 32) | lo, x, m[0].weight.shape[0], p, p)
        return expression(x, m[0].weight, m[0].bias, m[3].weight, m[3].bias, self.scale, self.norm.eps, f1, f2)

    n = 0
    for blk in model.feed_forward_blocks():
        blk.forward = types.MethodType(fwd, blk)
        n += 1
    return n


def set_ffn_dropout(model, p):
    for blk in model.feed_forward_blocks():
        blk.module[2].p = p
        blk.dropout.p = p
