"""Shared by the CPU and GPU tests of the bf16 axial attention (tests/test_backbone_bf16.py): the cases, the float64 yardstick, torch's
own bf16 call on identical inputs, the two accuracy conditions and the closed-form inputs of the exact-answer tests.

Inputs: the cases of backbone_common.op_case rounded to bf16 (so the fp32 tests' generator is shared).  Truth: F.scaled_dot_product_
attention on float64 copies of the ROUNDED inputs, on the CPU.  Two conditions:
  (i)  always: |out - truth| <= 2^-7 colmax elementwise, colmax the maximum over that sequence's keys of |v| in that head column.
       Rounding the weights to bf16 (relative 2^-9 each, numerator and denominator) moves a weighted mean of values bounded by
       colmax by at most 2 * 2^-9 colmax, the final rounding adds 2^-9 |out| <= 2^-9 colmax; the rest of 2^-7 = 4 * 2^-9 covers the
       fp32 terms.
  (ii) where min(Lq, Lk) >= 64: the maximum error is at most GATE = 8 times e16, the error of torch's own bf16 CPU call on identical
       inputs against the same truth (the gate idiom of backbone_common).
"""
import functools

import torch

import backbone_common as common

GATE = common.GATE
COL_BOUND = 2.0 ** -7

# (Lq, Lk, H, d) of the exact-answer tests: one key; one partial tile; the model's shape; the largest; NKT = 8 at d = 24 (KS = 2, DB = 1);
# cross attention at the model's shape; a 40-query pass over all 256 keys at d = 56
EXACT_SHAPES = [(33, 1, 2, 8), (33, 33, 2, 8), (149, 149, 4, 40), (256, 256, 4, 64), (65, 225, 2, 24), (89, 149, 4, 40), (40, 256, 1, 56)]
KINDS = [(65, 97, 2, 24, "huge"), (65, 97, 2, 24, "negative"), (149, 149, 4, 40, "huge"), (149, 149, 4, 40, "negative")]


@functools.lru_cache(maxsize=None)
def case(Lq, Lk, H, d, lead=(3,), scale=1.0, kind="randn"):
    """One case of the gate, computed once and shared by the CPU and GPU forms (kept unchanged on the CPU)."""
    c = common.op_case(Lq, Lk, H, d, lead, scale, kind)
    q, k, v = (c[n].bfloat16() for n in "qkv")
    return finish(q, k, v, H)


def finish(q, k, v, H):
    with torch.no_grad():
        truth = common.sdpa(q.double(), k.double(), v.double(), H)
        t16 = common.sdpa(q, k, v, H)
    e16 = float((t16.double() - truth).abs().max())
    colmax = v.double().abs().amax(dim=-2, keepdim=True)          # [..., 1, H d]: per sequence and head column, over the keys
    return dict(q=q, k=k, v=v, H=H, truth=truth, e16=e16, colmax=colmax, Lq=q.shape[-2], Lk=k.shape[-2])


def gated(got, c, tag):
    """Both conditions, the figures printed before they are asserted."""
    assert got.dtype == torch.bfloat16 and got.shape == c["truth"].shape, tag
    err = (got.cpu().double() - c["truth"]).abs()
    assert bool(torch.isfinite(err).all()), tag
    frac = float((err / (COL_BOUND * c["colmax"]).clamp_min(1e-300)).max()) if float(err.max()) > 0 else 0.0
    e = float(err.max())
    both = min(c["Lq"], c["Lk"]) >= 64
    ratio = e / c["e16"] if c["e16"] > 0 else float("nan")
    print(f"axial_attention_bf16 [{got.device.type}] {tag}: error {e:.3e}  {frac:.2f} of 2^-7 colmax  torch bf16 {c['e16']:.3e}  "
          f"ratio {ratio:.2f}{' (gate ' + format(GATE, 'g') + ')' if both else ''}")
    assert bool((err <= COL_BOUND * c["colmax"]).all()), (tag, e, frac)
    if both:
        assert e <= GATE * c["e16"], (tag, e, c["e16"])


def fused16(q, k, v, H, route="fused"):
    """backbone.axial_attention with bf16 = "fused", and the counters say that the bf16 op answered (never the stock route)."""
    from transkun_amd import backbone
    before = dict(backbone.ATTENTION_BF16_ROUTES), backbone.ATTENTION_ROUTES["torch"]
    with torch.no_grad():
        out = backbone.axial_attention(q, k, v, H, route=route, bf16="fused")
    assert backbone.ATTENTION_BF16_ROUTES["fused"] == before[0]["fused"] + 1 and backbone.ATTENTION_BF16_ROUTES["torch"] == before[0]["torch"]
    assert backbone.ATTENTION_ROUTES["torch"] == before[1]
    return out


def raw_op16(q4, k4, v4, o4, H):
    """The torch op itself on 4-d views [n0, n1, L, H d]."""
    from transkun_amd import _lib
    _lib.ops().axial_attention_bf16(q4, k4, v4, o4, H)
    return o4


def bits(t):
    return t.contiguous().view(torch.int16)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16 and torch.equal(bits(a), bits(b))


def same_bits_mask(a, b):
    return bits(a) == bits(b)


def one_off(x):
    """The values of x in a view one bf16 element off a 16-byte boundary (rows one element longer than x's: an odd token stride too)."""
    view = torch.cat([torch.zeros(*x.shape[:-1], 1, dtype=x.dtype, device=x.device), x], dim=-1)[..., 1:]
    assert view.data_ptr() % 16 == 2
    return view


# ---- the exact-answer inputs -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_hot_case(Lq, Lk, H, d, S=3):
    """Key j of every head carries in column c the sign of bit (c mod 8) of j; q_i = 512 x the code of sel(i), sel drawn per (sequence,
    head, query); v random bf16.  The selected key's score exceeds every other by at least 2 * 512 / sqrt(d) >= 128: every other weight
    is exp(-128 or less) = 0 exactly in fp32, the selected one exp(0) = 1, so out[i] = v[sel(i)] bit for bit."""
    g = torch.Generator().manual_seed(515 + 7 * Lq + 3 * Lk + H + d)
    j = torch.arange(Lk)
    code = (((j[:, None] >> (torch.arange(d)[None, :] % 8)) & 1) * 2 - 1).float()            # [Lk, d], +-1
    k = code.repeat(1, H).expand(S, Lk, H * d).contiguous()
    sel = torch.randint(0, Lk, (S, H, Lq), generator=g)
    q = (512.0 * code[sel]).permute(0, 2, 1, 3).reshape(S, Lq, H * d)                       # [S, H, Lq, d] -> [S, Lq, H d]
    v = torch.randn(S, Lk, H * d, generator=g).bfloat16()
    vh = v.view(S, Lk, H, d).permute(0, 2, 1, 3)                                             # [S, H, Lk, d]
    want = torch.gather(vh, 2, sel[..., None].expand(S, H, Lq, d)).permute(0, 2, 1, 3).reshape(S, Lq, H * d)
    return dict(q=q.bfloat16(), k=k.bfloat16(), v=v, want=want.contiguous())


@functools.lru_cache(maxsize=None)
def uniform_case(Lq, Lk, H, d, S=3):
    """q = 0, k arbitrary and finite, v integers in [-8, 8]: every weight is exactly 1, every partial sum an exact integer, so
    out = bf16((float)sum_j v_j / (float)Lk): one dropped, doubled or padded key changes a column sum by an integer."""
    g = torch.Generator().manual_seed(929 + 7 * Lq + 3 * Lk + H + d)
    q = torch.zeros(S, Lq, H * d).bfloat16()
    k = (torch.randn(S, Lk, H * d, generator=g) * 50.0).bfloat16()
    v = torch.randint(-8, 9, (S, Lk, H * d), generator=g).float()
    mean = v.sum(dim=1, keepdim=True) / torch.tensor(float(Lk))                               # exact sums, one fp32 division
    want = mean.bfloat16().expand(S, Lq, H * d).contiguous()
    return dict(q=q, k=k, v=v.bfloat16(), want=want)


# ---- the modules ---------------------------------------------------------------------------------------------------------------------
def bf16_backbone(name, dev):
    """(the fixture's Backbone cast to bf16, the same module in float64 with the bf16 weights upcast, the fixture)."""
    import copy
    m, fx = common.make_backbone(name, "cpu", "fused")
    m16 = m.to(torch.bfloat16)
    m64 = copy.deepcopy(m16).double()
    return m16.to(dev), m64, fx
