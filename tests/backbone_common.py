"""Shared by the CPU and GPU tests of the backbone and its axial attention (tests/test_backbone.py): seeded inputs, the float64
yardstick, torch's own fp32 call on identical inputs, the gate, and the fixtures of tools/make_backbone_golden.py.

Yardstick of the op: F.scaled_dot_product_attention on float64 copies, on the CPU.  Gate (the GATE = 8 idiom of attr_heads_common): the
maximum absolute error over the output is at most GATE x e32, e32 being the error of torch's own fp32 CPU call against the same truth
on identical inputs.  With min(Lq, Lk) >= 64 that is the whole gate (the maximum is then a stable statistic).  Below -- where torch is
exact or nearly so: Lk = 1 returns v itself, a handful of keys round a handful of times -- the gate is
max(GATE x e32, 4 x 2^-24 x max|v|): an output is a convex combination of v's rows, so the floor is a few ulps of the largest value
an output can take.

Yardstick of the modules: the reference's own float64 output stored in the fixture; gate GATE x the reference's own fp32 error
against it, also from the fixture.
"""
import functools
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
GATE = 8.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the op's cases -----------------------------------------------------------------------------------------------------------------
EDGE_L = [1, 2, 31, 32, 33, 63, 64, 65, 89, 149, 255, 256]          # the tile edges and the model's own lengths, d = 40, H = 4
SCALES = [1.0, 4.0]                                                   # 4: a sharp softmax
HEAD_CASES = [(L, H, d) for L in (33, 149) for d in (8, 16, 24, 64) for H in (1, 2, 3)]
CROSS = [(1, 149), (149, 1), (65, 33), (89, 149)]                     # (Lq, Lk)
BATCHES = [((1,), 33), ((3,), 33), ((7, 10), 33), ((7, 10), 89)]      # (leading shape, L): 1, 3 and 70 = 7 x 10 sequences

# every instantiation <NKT = ceil(Lk / 32), DB = 1 (d <= 32) | 2, VEC> of the kernel: both edges of every key tile at every head
# dimension, H = 2, three sequences, both SCALES, on aligned tensors (VEC) and with q and k one float off 16 bytes (4-byte loads)
MATRIX_D = [8, 16, 24, 32, 40, 48, 56, 64]
MATRIX_LK = [1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256]
MATRIX_LQ = 33                                                        # a full query tile on wave 0, a one-row tile on wave 1
MATRIX_H = 2
# the second query pass of a wave (Lq > 128) and partial query tiles at NKT = 4, 6, 7, 8; H = 2, three sequences, scale 1
PASSES = [(Lq, Lk, d) for Lq in (1, 127, 128, 129, 160, 256) for Lk in (100, 180, 210, 256) for d in (32, 64)]
LARGEST = (256, 256, 4, 64, (3,))                                     # (Lq, Lk, H, d, leading shape): 100 KB of LDS, the most registers
CORESIDENT = (149, 149, 8, 64, (7, 10))                               # 560 workgroups of 75 KB of LDS: two of them share a CU
HEAD_COUNTS = [(40, 70, 64, 8), (40, 70, 1, 64)]                      # (Lq, Lk, H, d): many heads, one head
CONTRACT = (65, 97, 2, 24, (3,))                                      # the strided contract's shape: NKT = 4, DB = 1
TOKEN_STRIDE_LIMIT = 1 << 28                                          # elements: the C entry point takes token strides below it


def split_heads(t, H):
    return t.unflatten(-1, (H, t.shape[-1] // H)).transpose(-2, -3)


def sdpa(q, k, v, H):
    """The reference's call on head-split views; q [..., Lq, H d] -> [..., Lq, H d]."""
    return F.scaled_dot_product_attention(split_heads(q, H), split_heads(k, H), split_heads(v, H)).transpose(-2, -3).flatten(-2, -1)


def gate_of(Lq, Lk, e32, v):
    if min(Lq, Lk) >= 64:
        return GATE * e32
    return max(GATE * e32, 4 * U * float(v.abs().max()))


def finish_case(q, k, v, H):
    with torch.no_grad():
        truth = sdpa(q.double(), k.double(), v.double(), H)
        t32 = sdpa(q, k, v, H)
    e32 = float((t32.double() - truth).abs().max())
    Lq, Lk = q.shape[-2], k.shape[-2]
    return dict(q=q, k=k, v=v, H=H, truth=truth, e32=e32, gate=gate_of(Lq, Lk, e32, v))


@functools.lru_cache(maxsize=None)
def op_case(Lq, Lk, H, d, lead=(3,), scale=1.0, kind="randn"):
    """One case of the gate, computed once and shared by the CPU and GPU forms (kept unchanged on the CPU).
    kind "randn": q, k, v ~ N(0, scale^2) (v unit scale);  "huge": q and k times 30, logits in the thousands;
    "negative": every true score <= -50 (a padded zero column would win the maximum)."""
    g = torch.Generator().manual_seed(7000 + 131 * Lq + 17 * Lk + 5 * H + d + int(10 * scale) + 1000 * len(lead) + sum(lead))
    q = torch.randn(*lead, Lq, H * d, generator=g)
    k = torch.randn(*lead, Lk, H * d, generator=g)
    v = torch.randn(*lead, Lk, H * d, generator=g)
    if kind == "randn":
        q, k = q * scale, k * scale
    elif kind == "huge":
        q, k = q * 30.0, k * 30.0
    elif kind == "negative":
        q, k = q.abs() + 3.0, -(k.abs() + 3.0)
    else:
        raise ValueError(kind)
    c = finish_case(q, k, v, H)
    if kind != "randn":
        logits = split_heads(q.double(), H) @ split_heads(k.double(), H).transpose(-1, -2) / (d ** 0.5)
        c["logit_min"], c["logit_max"] = float(logits.min()), float(logits.max())
    return c


def fused(q, k, v, H):
    from transkun_amd import backbone
    with torch.no_grad():
        return backbone.axial_attention(q, k, v, H, route="fused")


def raw_op(q4, k4, v4, o4, H):
    """The torch op itself on 4-d views [n0, n1, L, H d] (what backbone.axial_attention calls)."""
    from transkun_amd import _lib
    _lib.ops().axial_attention(q4, k4, v4, o4, H)
    return o4


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def one_float_off(x):
    """The values of x in a view one float off a 16-byte boundary (rows of one float more than x's): the construction of
    _check_strided_views."""
    view = torch.cat([torch.zeros(*x.shape[:-1], 1, dtype=x.dtype, device=x.device), x], dim=-1)[..., 1:]
    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
    return view


def same_bits_mask(a, b):
    """Elementwise: the same 32 bits (NaN payloads included)."""
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


# ---- the fixtures -------------------------------------------------------------------------------------------------------------------
FIXTURES = ["backbone_small", "backbone_d40"]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """NAME.npz and its NAME.part*.npz as one dict; `sd`: the state_dict (fp32 tensors); `cfg`: the constructor arguments."""
    data = {}
    paths = [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".part*.npz")))
    for p in paths:
        data.update(np.load(p, allow_pickle=False))
    out = {k: torch.from_numpy(np.asarray(v)) for k, v in data.items() if not k.startswith(("sd/", "cfg_"))}
    out["sd"] = {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in data.items() if k.startswith("sd/")}
    cfg = {}
    for k, v in data.items():
        if k.startswith("cfg_"):
            v = np.asarray(v)
            cfg[k[4:]] = [str(s) for s in v] if v.dtype.kind == "U" else (bool(v) if v.dtype.kind == "b" else v.item())
    out["cfg"] = cfg
    return out


def make_backbone(name, dev, attention):
    from transkun_amd import backbone
    fx = fixture(name)
    m = backbone.Backbone(**fx["cfg"]).eval()
    m.load_state_dict(fx["sd"], strict=True)
    m.attention = attention
    return m.to(dev), fx
