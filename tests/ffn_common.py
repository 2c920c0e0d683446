"""Shared by the CPU and GPU tests of the backbone's fused feed-forward ResBlock (tests/test_feed_forward.py): seeded cases, the
float64 yardstick, the stock fp32 modules on identical inputs, the gate, and an independent emulation of the op's order of operations.

Yardstick: the block's formula x + (W2 gelu(W1 rmsnorm(x) + b1) + b2) * scale in float64 on the CPU.  Gate (the GATE = 8 idiom of
attr_heads_common and backbone_common): the op's maximum absolute error is at most max(GATE x e32, 4 x 2^-24 x max|truth|), e32 being
the error of the stock fp32 modules (RMSNorm, nn.Linear, nn.GELU, nn.Linear, scale, residual) on the CPU on identical inputs.  The
floor is a few ulps of the largest output: with scale at its initial 1e-2 the residual addition's rounding is the whole error of both.

Cases are built once on the CPU (lru_cache) and never modified; the GPU tests move copies.
"""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
GATE = 8.0


def tiles():
    """(R, C): the op's row tile and hidden chunk, read from the constants exported next to it."""
    from transkun_amd import backbone
    return backbone.FEED_FORWARD_ROW_TILE, backbone.FEED_FORWARD_HIDDEN_CHUNK


def row_counts():
    R, _ = tiles()
    return [1, R - 1, R, R + 1, 2 * R + 1]


def hidden_sizes():
    _, C = tiles()
    return [8, C - 8, C, C + 8, 320, 640, 1024]


WIDTHS = [8, 32, 80, 160, 256]
SCALE_KINDS = ["init", "randn"]                # LayerScale at its initial 1e-2 / ~ N(0, 1)
INPUT_SCALES = [1.0, 4.0]
# one width per instantiation of the kernel (column blocks 1 .. 8 of 32), each on aligned tensors and one float off 16 bytes
MATRIX_WIDTHS = [8, 64, 96, 128, 160, 192, 224, 256]
# set by a test to run the host mirror WITHOUT the last hidden chunk (when there is more than one): the mutation the gate must catch
SKIP_LAST_CHUNK = False


def stock_modules(D, hidden, g):
    """The modules of a feed-forward ResBlock as BasicBlock builds them, with seeded parameters of a trained model's size."""
    from transkun_amd import backbone
    blk = backbone.ResBlock(backbone._feed_forward(D, hidden, 0.0), size=D).eval()
    with torch.no_grad():
        blk.module[0].weight.copy_(torch.randn(hidden, D, generator=g) / math.sqrt(D))
        blk.module[0].bias.copy_(torch.randn(hidden, generator=g) * 0.5)
        blk.module[3].weight.copy_(torch.randn(D, hidden, generator=g) / math.sqrt(hidden))
        blk.module[3].bias.copy_(torch.randn(D, generator=g) * 0.5)
    return blk


def formula64(x, w1, b1, w2, b2, scale, eps):
    x, w1, b1, w2, b2, scale = (t.double() for t in (x, w1, b1, w2, b2, scale))
    xn = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    h = xn @ w1.T + b1
    g = 0.5 * h * torch.special.erfc(-h / math.sqrt(2.0))
    return x + (g @ w2.T + b2) * scale


@functools.lru_cache(maxsize=None)
def case(rows, D, hidden, scale_kind="randn", mult=1.0, lead=None):
    """One case of the gate: x [rows, D] (or [*lead, D]), the parameters, the float64 truth, e32 and the gate."""
    g = torch.Generator().manual_seed(9000 + 7 * rows + 131 * D + 17 * hidden + (1 if scale_kind == "init" else 0) + int(10 * mult))
    blk = stock_modules(D, hidden, g)
    if scale_kind == "randn":
        with torch.no_grad():
            blk.scale.copy_(torch.randn(D, generator=g))
    shape = (rows, D) if lead is None else (*lead, D)
    x = torch.randn(*shape, generator=g) * mult
    params = tuple(p.detach() for p in (blk.module[0].weight, blk.module[0].bias, blk.module[3].weight, blk.module[3].bias, blk.scale))
    with torch.no_grad():
        truth = formula64(x, *params, blk.norm.eps)
        t32 = blk(x)
    e32 = float((t32.double() - truth).abs().max())
    gate = max(GATE * e32, 4 * U * float(truth.abs().max()))
    return dict(x=x, params=params, eps=blk.norm.eps, truth=truth, e32=e32, gate=gate, block=blk, D=D, hidden=hidden)


def run(c, dev, x=None):
    """The fused op on the case's parameters (the host mirror for the CPU); x defaults to the case's own."""
    from transkun_amd import backbone
    x = c["x"] if x is None else x
    w1, b1, w2, b2, scale = c["params"]
    _, C = tiles()
    if SKIP_LAST_CHUNK and c["hidden"] > C:                 # the mutation: the walk stops one chunk early
        keep = (c["hidden"] + C - 1) // C * C - C
        w1, b1, w2 = w1[:keep], b1[:keep], w2[:, :keep].contiguous()
    with torch.no_grad():
        return backbone.feed_forward_residual(x.to(dev), *(p.to(dev) for p in (w1, b1, w2, b2, scale)), eps=c["eps"], route="fused")


def raw_op(x3, params, eps, out3):
    """The torch op itself on [n0, n1, D] views (what backbone.feed_forward_residual calls)."""
    from transkun_amd import _lib
    _lib.ops().ffn_residual(x3, *params, float(eps), out3)
    return out3


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def same_bits_mask(a, b):
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


def one_float_off(x):
    """The values of x in a view one float off a 16-byte boundary (rows of one float more than x's)."""
    view = torch.cat([torch.zeros(*x.shape[:-1], 1, dtype=x.dtype, device=x.device), x], dim=-1)[..., 1:]
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
    return view


# ---- an independent emulation of the op's order of operations (csrc/ffn_math.h), numpy ----------------------------------------------
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64; the sum is rounded to 53 bits and then to 24, which
    differs from one rounding only when the 53-bit result lands on a float32 tie (not at the seeds used here: the tests compare)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(c):
    """The op per ffn_math.h with gelu's erf / erfc taken in float64 and rounded to float32 once: what a correctly rounded fp32 math
    library would give.  x [rows, D] -> float32 [rows, D]."""
    _, C = tiles()
    f32 = np.float32
    x = c["x"].numpy().astype(f32)
    w1, b1, w2, b2, scale = (p.numpy().astype(f32) for p in c["params"])
    rows, D = x.shape
    H = w1.shape[0]
    s = [np.zeros(rows, f32) for _ in range(4)]
    for k in range(D):
        s[k & 3] = _fma32(x[:, k], x[:, k], s[k & 3])
    ss = (s[0] + s[1]) + (s[2] + s[3])
    rs = f32(1.0) / np.sqrt(ss / f32(D) + f32(c["eps"]))
    xn = x * rs[:, None]
    h = np.zeros((rows, H), f32)
    for k in range(D):
        h = _fma32(xn[:, k, None], w1[None, :, k], h)
    h = h + b1[None, :]
    z = h * f32(0.70710678118654752440)
    z64 = torch.from_numpy(z.astype(np.float64))
    erfc_neg = torch.special.erfc(-z64).numpy().astype(f32)              # h < 0:  erfc(-z)
    erf_pos = (f32(1.0) + torch.special.erf(z64).numpy().astype(f32)).astype(f32)     # else: 1 + erf(z), one fp32 addition
    t = np.where(h < 0, erfc_neg, erf_pos).astype(f32)
    g = (f32(0.5) * h) * t
    acc = np.zeros((rows, D), f32)
    for j0 in range(0, H, C):                               # a chunk's sum from +0, the chunks added in ascending order
        part = np.zeros((rows, D), f32)
        for j in range(j0, min(j0 + C, H)):
            part = _fma32(g[:, j, None], w2[None, :, j], part)
        if H - j0 < C:
            part = part + f32(0.0)                          # the zero padding of a short last chunk: -0 becomes +0
        acc = acc + part
    return torch.from_numpy(x + (acc + b2[None, :]) * scale[None, :])
