"""The backbone of the transcriber: the module that turns the spectrogram features of a segment into `ctx`, with its attention as a
fused HIP op.

Mirrors the reference's `Backbone` and the modules it is built from (LayersTransformer.py:12-372, :444-660) under the reference's
constructor arguments and parameter names, so `load_state_dict(reference_state_dict, strict=True)` works:

    RMSNorm, TiedDropout, LearnableSpatialPositionEmbedding, ResBlock, MultiHeadAttentionKernel (kernel = None only), BasicBlock, Backbone

What is native here is the attention.  Every layer attends along the frequency axis and along the time axis of one [N, T', F', D]
hidden state: hundreds of independent sequences of at most a few hundred tokens, head dimension 40 at the model's size.
`axial_attention` runs them through `torch.ops.semicrf.axial_attention` (csrc/attention.hip on a GPU, the host mirror in
csrc/cpu_ops.cpp on the CPU), whose contract is token-major with three strides per tensor: both axes read the SAME buffer, so
`BasicBlock` keeps the hidden state [N, T', F', D] and contiguous from its input to its output -- no `transpose(-3, -2)` around the
time-axis half, and none of the copies eager PyTorch makes for the projections and the attention of a transposed tensor.

`attention = "fused" | "fused-train" | "torch"` on every attention module, and on `Backbone` for all of its layers, picks the route.
"fused" (the default) is forward only: under autograd (gradients enabled and an input requiring grad) it takes the stock route --
`F.scaled_dot_product_attention` on head-split views, exactly the reference's call -- so training works as before, bit for bit.
"fused-train" is "fused" wherever no gradient is wanted, and under autograd a `torch.autograd.Function` around the same forward op
whose backward is `torch.ops.semicrf.axial_attention_bwd` (csrc/attention_bwd.hip, the host mirror on the CPU): dq, dk and dv are
written by strides into tensors laid out like q, k and v, so `BasicBlock` keeps its no-transpose form in training too.  The backward
recomputes the softmax from q and k and takes `out` as the forward wrote it; nothing else is saved, and a second derivative raises.
Every route answers by the stock call for dtypes other than float32 (bfloat16 has a knob of its own, below), for shapes outside the
op's supported set, for broadcasting keys and for device views whose tokens lie 2^28 elements apart or more.  `ATTENTION_ROUTES`
counts which way the calls went.

bfloat16 tensors (a model cast to bf16, or run under `torch.autocast(dtype=torch.bfloat16)`) have a fused forward of their own,
`torch.ops.semicrf.axial_attention_bf16` (csrc/attention_bf16.hip: both products on the bf16 matrix instruction, the same token-major
strided contract; the host mirror on the CPU).  It is a separate knob: `attentionBf16 = "torch" | "fused"` on every attention module,
and on `BasicBlock` and `Backbone` for all of theirs; the default is "torch", under which bf16 tensors take the stock route as they
always have.  "fused" sends bf16 calls to the op wherever the fp32 op would apply (route not "torch", no gradient wanted, supported
shape, no broadcasting keys, token strides within the limit); it is forward only, so under autograd both "fused" and "fused-train"
answer by the stock route for bf16.  `ATTENTION_BF16_ROUTES` counts the bf16 calls made with the knob at "fused".

Training in bf16 has a third knob, `attentionBf16Train = "torch" | "fused"` (default "torch": everything above, unchanged).  With
`attention = "fused-train"`, `attentionBf16 = "fused"` AND `attentionBf16Train = "fused"`, a bf16 call under autograd is a
`torch.autograd.Function` around the same bf16 forward op whose backward is `torch.ops.semicrf.axial_attention_bf16_bwd`
(csrc/attention_bf16_bwd.hip: all five products on the bf16 matrix instruction; the host mirror on the CPU).  It saves the q, k, v views
only -- the backward recomputes the softmax and needs no `out` -- writes dq, dk, dv by strides in the layouts of q, k, v, and is once
differentiable.  `ATTENTION_BF16_TRAIN_ROUTES` counts the bf16 calls under autograd made with the knob at "fused", and the launches
of the backward.

The feed-forward half of a layer has a fused route too.  `feedForward = "fused" | "torch"` on a `ResBlock`, and on `BasicBlock` and
`Backbone` for all of their feed-forward blocks, picks it; the default is "torch", the stock expression.  "fused" runs a block whose
module is the `Linear, GELU, Dropout, Linear` sequence through `feed_forward_residual`: RMSNorm, both Linears, the GELU, the LayerScale
and the residual addition as ONE op, `torch.ops.semicrf.ffn_residual` (csrc/ffn.hip on a GPU, the host mirror on the CPU), on the
hidden state as it lies in memory -- the [tokens, hidden] activation is never written.  It is forward only and eval only: under
autograd, with an active dropout, for dtypes other than float32, for shapes outside the op's supported set, for any other module and
for extra arguments the block runs the stock expression.  `FEED_FORWARD_ROUTES` counts which way the calls went.

bfloat16 has a knob of its own beside it, as the attention has: `feedForwardBf16 = "torch" | "fused"` on `ResBlock`, `BasicBlock` and
`Backbone` (default "torch": everything above, unchanged).  It takes effect only where `feedForward = "fused"` and the conditions above
hold.  Then a block whose input and five parameters are all bfloat16 is `torch.ops.semicrf.ffn_residual_bf16` (csrc/ffn_bf16.hip: both
products on the bf16 matrix instruction), and a float32 block called under `torch.autocast(dtype=torch.bfloat16)` is
`torch.ops.semicrf.ffn_residual_bf16_mixed`: the same kernel on the float32 tensors as the module holds them, the weights rounded to
bf16 inside the launch, the biases and the LayerScale used as float32, a float32 result.  A float32 call outside autocast stays the
float32 op; any other mix of dtypes, and autocast to any other dtype, takes the stock expression.  `FEED_FORWARD_BF16_ROUTES` counts the
calls made with the knob at "fused" that were bfloat16 or under bfloat16 autocast; a fused answer counts in `FEED_FORWARD_ROUTES` too.

Training in float32 has a third knob, `feedForwardTrain = "torch" | "fused"` (default "torch": everything above, unchanged, counters
included).  With `feedForward = "fused"` AND `feedForwardTrain = "fused"`, a float32 call outside autocast that wants a gradient -- its
two dropouts active or not -- is `torch.ops.semicrf.ffn_residual_train_fwd` (csrc/ffn.hip in its training mode: both dropouts from a
stateless Philox mask, z and y saved) with `torch.ops.semicrf.ffn_residual_bwd` (csrc/ffn_bwd.hip) as its backward, once
differentiable, every gradient bit-identical from run to run.  bfloat16, autocast, extra arguments and an unsupported shape take the
stock expression.  `FEED_FORWARD_TRAIN_ROUTES` counts the gradient-wanting calls made with the knob at "fused" (and, under "bwd", the
launches of the HIP backward); a fused answer counts in `FEED_FORWARD_ROUTES` too.

Training in bfloat16 has a fourth knob, `feedForwardBf16Train = "torch" | "fused"` (default "torch": everything above, unchanged,
counters included).  With `feedForward`, `feedForwardTrain`, `feedForwardBf16` AND `feedForwardBf16Train` at "fused", a gradient-wanting
call on bfloat16 tensors (form A), or on float32 tensors under bfloat16 autocast (form B: float32 parameters and gradients, which is what
FusedAdaBelief and FlatGradBucket work on), is `torch.ops.semicrf.ffn_residual_bf16_train_fwd` / `_mixed_train_fwd` (csrc/ffn_bf16.hip
in its training mode: the fp32 route's masks, bf16(h) and y saved in one opaque buffer) with `torch.ops.semicrf.ffn_residual_bf16_bwd` /
`_mixed_bwd` (csrc/ffn_bf16_bwd.hip: five launches, every product on the bf16 matrix instruction) as its backward, once differentiable,
every gradient bit-identical from run to run.  `FEED_FORWARD_BF16_TRAIN_ROUTES` counts the gradient-wanting bfloat16 / bfloat16-autocast
calls made with all four at "fused"; a fused answer counts in the three other dicts too.

Hidden size and head dimension come from the constructor as in the reference: head_dim = ceil(ceil(hiddenFactor * embed_dim) /
num_heads), hidden size = head_dim * num_heads (the model: embed_dim 160, 4 heads, hiddenFactorAttn 1 -> d = 40).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint

from . import _lib

ROUTES = ("fused", "fused-train", "torch")
DEFAULT_ATTENTION = "fused"
# calls of axial_attention by the way they went ("fused": the forward op alone; "fused-train": the autograd Function; "torch": the stock
# call) and, under "bwd", the launches of the HIP backward; tests read it
ATTENTION_ROUTES = {"fused": 0, "fused-train": 0, "torch": 0, "bwd": 0}
BF16_KINDS = ("torch", "fused")
DEFAULT_ATTENTION_BF16 = "torch"
# calls of axial_attention on bfloat16 tensors with bf16 = "fused", by the way they went; tests read it
ATTENTION_BF16_ROUTES = {"fused": 0, "torch": 0}
BF16_TRAIN_KINDS = ("torch", "fused")
DEFAULT_ATTENTION_BF16_TRAIN = "torch"
# calls of axial_attention on bfloat16 tensors under autograd with bf16_train = "fused", by the way they went ("fused": the autograd
# Function around the bf16 op; "torch": the stock call) and, under "bwd", the launches of the bf16 HIP backward; tests read it
ATTENTION_BF16_TRAIN_ROUTES = {"fused": 0, "torch": 0, "bwd": 0}


# ---- the attention ------------------------------------------------------------------------------------------------------------------
def attention_supported(Lq: int, Lk: int, num_heads: int, head_dim: int) -> bool:
    """semicrf_axial_attention_supported: 1 <= Lq, Lk <= 256, head_dim a multiple of 8 in [8, 64], num_heads >= 1."""
    return bool(_lib.load().semicrf_axial_attention_supported(int(Lq), int(Lk), int(num_heads), int(head_dim)))


def attention_bf16_supported(Lq: int, Lk: int, num_heads: int, head_dim: int) -> bool:
    """semicrf_axial_attention_bf16_supported: the fp32 op's set."""
    return bool(_lib.load().semicrf_axial_attention_bf16_supported(int(Lq), int(Lk), int(num_heads), int(head_dim)))


def attention_bf16_bwd_supported(Lq: int, Lk: int, num_heads: int, head_dim: int) -> bool:
    """semicrf_axial_attention_bf16_bwd_supported: the forward's set."""
    return bool(_lib.load().semicrf_axial_attention_bf16_bwd_supported(int(Lq), int(Lk), int(num_heads), int(head_dim)))


def attention_bwd_supported(Lq: int, Lk: int, num_heads: int, head_dim: int) -> bool:
    """semicrf_axial_attention_bwd_supported: the forward's set."""
    return bool(_lib.load().semicrf_axial_attention_bwd_supported(int(Lq), int(Lk), int(num_heads), int(head_dim)))


def attention_torch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int) -> torch.Tensor:
    """The stock route: the reference's call (LayersTransformer.py:173-186) -- heads split off the last dimension and moved in front of
    the sequence as views, F.scaled_dot_product_attention, heads merged back."""
    d = q.shape[-1] // num_heads
    qh, kh, vh = (t.unflatten(-1, (num_heads, d)).transpose(-2, -3) for t in (q, k, v))
    return F.scaled_dot_product_attention(qh, kh, vh).transpose(-2, -3).flatten(-2, -1)


def _merge(sizes, strides):
    """(size, stride) of the dimensions merged into one, or None when they do not lie evenly spaced in memory."""
    dims = [(n, s) for n, s in zip(sizes, strides) if n != 1]
    if not dims:
        return 1, 0
    n, s = dims[-1]
    for m, t in reversed(dims[:-1]):
        if t != s * n:
            return None
        n *= m
    return n, s


def _as_sequences(t: torch.Tensor, split: int):
    """t [..., L, HD] as the op's 4-d view [n0, n1, L, HD] with the leading dimensions cut at `split`, or None (no copy is made)."""
    if t.shape[-1] != 1 and t.stride(-1) != 1:
        return None
    lead, lst = t.shape[:-2], t.stride()[:-2]
    a, b = _merge(lead[:split], lst[:split]), _merge(lead[split:], lst[split:])
    if a is None or b is None:
        return None
    return torch.as_strided(t, (a[0], b[0], t.shape[-2], t.shape[-1]), (a[1], b[1], t.stride(-2), 1), t.storage_offset())


ATTENTION_TOKEN_STRIDE_LIMIT = 1 << 28                          # elements: semicrf_axial_attention takes token strides below it


def _token_strides_fit(*tensors) -> bool:
    """Every tensor's token stride is below the device op's limit (the stride of a single token counts for nothing)."""
    return all(t.shape[-2] <= 1 or t.stride(-2) < ATTENTION_TOKEN_STRIDE_LIMIT for t in tensors)


def _wants_grad(q, k, v) -> bool:
    return torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)


def _fused_applies(q, k, v, num_heads, train=False, dtype=torch.float32) -> bool:
    if not (q.dtype == k.dtype == v.dtype == dtype) or not (q.device == k.device == v.device):
        return False
    if q.device.type not in ("cuda", "cpu") or q.dim() < 2 or k.shape != v.shape or q.numel() == 0 or k.numel() == 0:
        return False
    if k.shape[:-2] != q.shape[:-2] or k.shape[-1] != q.shape[-1] or q.shape[-1] % num_heads != 0:
        return False                                            # broadcasting batch dimensions: the stock route
    if not train and _wants_grad(q, k, v):
        return False                                            # forward only
    if q.device.type == "cuda" and not _token_strides_fit(q, k, v):
        return False                                            # tokens 2^28 elements apart or more: outside the device op's addressing
    dims = (q.shape[-2], k.shape[-2], num_heads, q.shape[-1] // num_heads)
    if dtype == torch.bfloat16:
        return attention_bf16_supported(*dims) and (not train or attention_bf16_bwd_supported(*dims))
    return attention_supported(*dims) and (not train or attention_bwd_supported(*dims))


def _fused_forward(q, k, v, num_heads):
    """The forward op (the bf16 op for bfloat16 tensors) on q, k, v as they lie in memory -> (out, split, (q4, k4, v4)): the 4-d views
    the op was given."""
    nlead = q.dim() - 2
    best = None
    for split in range(nlead + 1):
        views = [_as_sequences(t, split) for t in (q, k, v)]
        copies = sum(x is None for x in views)
        if best is None or copies < best[0]:
            best = (copies, split, views)
        if copies == 0:
            break
    _, split, views = best
    q4, k4, v4 = (x if x is not None else _as_sequences(t.contiguous(), split) for x, t in zip(views, (q, k, v)))
    out = torch.empty_like(q)                                   # q's own layout when q is dense
    o4 = _as_sequences(out, split) if views[0] is not None else None
    if o4 is None:
        out = torch.empty(q.shape, dtype=q.dtype, device=q.device)
        o4 = _as_sequences(out, split)
    if q.dtype == torch.bfloat16:
        _lib.ops().axial_attention_bf16(q4, k4, v4, o4, num_heads)
    else:
        _lib.ops().axial_attention(q4, k4, v4, o4, num_heads)
    return out, split, (q4, k4, v4)


def _layout_of(t):
    """(shape, strides) of empty_like(t): t's own layout when t is dense, contiguous otherwise (nothing is allocated)."""
    e = torch.empty_like(t, device="meta")
    return tuple(e.shape), tuple(e.stride())


def _real_strides(x4) -> bool:
    return all(n == 1 or s > 0 for n, s in zip(x4.shape[:3], x4.stride()[:3]))


def _backward_views(ctx, dout):
    """What a backward op is handed -> (dout's 4-d view, the gradients, their 4-d views): dout by its strides under the forward's
    split (made contiguous only where that cannot be said), the gradients allocated in the layouts of q, k, v; None for an input
    that needs none."""
    split = ctx.split
    g4 = _as_sequences(dout, split)
    if g4 is None or not _real_strides(g4) or (dout.device.type == "cuda" and not _token_strides_fit(g4)):
        g4 = _as_sequences(dout.contiguous(), split)
    grads, grads4 = [], []
    for need, (shape, strides) in zip(ctx.needs_input_grad[:3], ctx.layouts):
        g = x4 = None
        if need:
            g = torch.empty_strided(shape, strides, dtype=dout.dtype, device=dout.device)
            x4 = _as_sequences(g, split)
            if x4 is None:
                g = torch.empty(shape, dtype=dout.dtype, device=dout.device)
                x4 = _as_sequences(g, split)
        grads.append(g)
        grads4.append(x4)
    return g4, grads, grads4


class _AxialAttentionTrain(torch.autograd.Function):
    """The forward op, and axial_attention_bwd as its backward (route "fused-train")."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads):
        out, split, (q4, k4, v4) = _fused_forward(q, k, v, num_heads)
        ctx.save_for_backward(q4, k4, v4, out)
        ctx.split, ctx.num_heads = split, num_heads
        ctx.layouts = [_layout_of(t) for t in (q, k, v)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q4, k4, v4, out = ctx.saved_tensors
        o4 = _as_sequences(out, ctx.split)
        g4, grads, grads4 = _backward_views(ctx, dout)
        _lib.ops().axial_attention_bwd(q4, k4, v4, o4, g4, grads4[0], grads4[1], grads4[2], ctx.num_heads)
        ATTENTION_ROUTES["bwd"] += 1
        return grads[0], grads[1], grads[2], None


class _AxialAttentionBf16Train(torch.autograd.Function):
    """The bf16 forward op, and axial_attention_bf16_bwd as its backward (bf16_train = "fused").  Only the q, k, v views are saved."""

    @staticmethod
    def forward(ctx, q, k, v, num_heads):
        out, split, views = _fused_forward(q, k, v, num_heads)
        ctx.save_for_backward(*views)
        ctx.split, ctx.num_heads = split, num_heads
        ctx.layouts = [_layout_of(t) for t in (q, k, v)]
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        q4, k4, v4 = ctx.saved_tensors
        g4, grads, grads4 = _backward_views(ctx, dout)
        _lib.ops().axial_attention_bf16_bwd(q4, k4, v4, g4, grads4[0], grads4[1], grads4[2], ctx.num_heads)
        ATTENTION_BF16_TRAIN_ROUTES["bwd"] += 1
        return grads[0], grads[1], grads[2], None


def axial_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, num_heads: int, route: str = "fused",
                    bf16: str = "torch", bf16_train: str = "torch") -> torch.Tensor:
    """softmax(q k^T / sqrt(d)) v per head and sequence.  q [..., Lq, H d], k and v [..., Lk, H d], arbitrary strided views whose last
    dimension is contiguous: the leading dimensions are handed to the op as its two sequence dimensions by strides alone (a tensor
    whose leading dimensions cannot be expressed that way is made contiguous first, that tensor only).  Returns [..., Lq, H d], laid
    out in memory like q (so the result of a transposed view transposes back into a contiguous tensor).

    route = "fused": the HIP op (the host kernel for CPU tensors) whenever it applies; the stock route (attention_torch) when the
    shape is outside the supported set, the dtype is not float32, k / v broadcast against q, gradients are enabled and an input
    requires grad, or -- on the device -- q, k or v has more than one token and a token stride of 2^28 elements or more (the kernel
    forms V addresses from a 32-bit lane offset).  route = "fused-train": "fused", except that under autograd the op runs inside an
    autograd Function whose backward is the HIP op axial_attention_bwd (once differentiable; gradients laid out like q, k, v; None
    for an input that needs none) wherever the forward applies and semicrf_axial_attention_bwd_supported holds, and the stock route
    elsewhere.  route = "torch": always the stock route.  Always usable, always differentiable.

    bf16 = "torch" (the default): bfloat16 tensors take the stock route, as every dtype other than float32 does.  bf16 = "fused": when
    q, k and v are all bfloat16, route is not "torch" and no gradient is wanted, the call is the HIP op axial_attention_bf16 (the host
    kernel for CPU tensors) under the same conditions as the fp32 op -- same device, no broadcasting keys, a supported shape, token
    strides within the limit -- and returns bf16 laid out like q; in every other case, under autograd with either fused route
    included, the call is what it is with bf16 = "torch".

    bf16_train = "torch" (the default): all of the above.  bf16_train = "fused" has an effect only when q, k and v are all bfloat16,
    route is "fused-train", bf16 is "fused", a gradient is wanted, the bf16 op applies to the call and
    semicrf_axial_attention_bf16_bwd_supported holds: the call is then an autograd Function around the bf16 forward op whose backward
    is the HIP op axial_attention_bf16_bwd (once differentiable; only the q, k, v views are saved; bf16 gradients laid out like q, k,
    v; None for an input that needs none).  In every other case the call is exactly what it is with bf16_train = "torch"."""
    if route not in ROUTES:
        raise ValueError(f"route must be one of {ROUTES}, not {route!r}")
    if bf16 not in BF16_KINDS:
        raise ValueError(f"bf16 must be one of {BF16_KINDS}, not {bf16!r}")
    if bf16_train not in BF16_TRAIN_KINDS:
        raise ValueError(f"bf16_train must be one of {BF16_TRAIN_KINDS}, not {bf16_train!r}")
    if bf16_train == "fused" and q.dtype == k.dtype == v.dtype == torch.bfloat16 and _wants_grad(q, k, v):
        if route == "fused-train" and bf16 == "fused" and _fused_applies(q, k, v, num_heads, True, torch.bfloat16):
            ATTENTION_BF16_TRAIN_ROUTES["fused"] += 1
            ATTENTION_BF16_ROUTES["fused"] += 1
            ATTENTION_ROUTES["fused-train"] += 1
            return _AxialAttentionBf16Train.apply(q, k, v, num_heads)
        ATTENTION_BF16_TRAIN_ROUTES["torch"] += 1
    if bf16 == "fused" and q.dtype == k.dtype == v.dtype == torch.bfloat16:
        if route != "torch" and _fused_applies(q, k, v, num_heads, dtype=torch.bfloat16):
            ATTENTION_BF16_ROUTES["fused"] += 1
            ATTENTION_ROUTES["fused"] += 1
            return _fused_forward(q, k, v, num_heads)[0]
        ATTENTION_BF16_ROUTES["torch"] += 1
    train = route == "fused-train" and _wants_grad(q, k, v)
    if route == "torch" or not _fused_applies(q, k, v, num_heads, train):
        ATTENTION_ROUTES["torch"] += 1
        return attention_torch(q, k, v, num_heads)
    if train:
        ATTENTION_ROUTES["fused-train"] += 1
        return _AxialAttentionTrain.apply(q, k, v, num_heads)
    ATTENTION_ROUTES["fused"] += 1
    return _fused_forward(q, k, v, num_heads)[0]


# ---- the feed-forward block -----------------------------------------------------------------------------------------------------------
FEED_FORWARD_KINDS = ("fused", "torch")
DEFAULT_FEED_FORWARD = "torch"
# calls of feed_forward_residual, and of the ResBlocks set to "fused", by the way they went; tests read it
FEED_FORWARD_ROUTES = {"fused": 0, "torch": 0}
FEED_FORWARD_ROW_TILE = _lib.FFN_ROW_TILE                       # token rows per workgroup of the op
FEED_FORWARD_HIDDEN_CHUNK = _lib.FFN_HIDDEN_CHUNK               # hidden columns per step of its walk
FEED_FORWARD_BF16_KINDS = ("torch", "fused")
DEFAULT_FEED_FORWARD_BF16 = "torch"
# calls made with bf16 = "fused" on bfloat16 tensors or under bfloat16 autocast, by the way they went; tests read it
FEED_FORWARD_BF16_ROUTES = {"fused": 0, "torch": 0}
FEED_FORWARD_BF16_ROW_TILE = _lib.FFN_BF16_ROW_TILE             # token rows per workgroup of the bf16 op
FEED_FORWARD_BF16_HIDDEN_CHUNK = _lib.FFN_BF16_HIDDEN_CHUNK     # hidden columns per step of its walk
FEED_FORWARD_TRAIN_KINDS = ("torch", "fused")
DEFAULT_FEED_FORWARD_TRAIN = "torch"
# gradient-wanting calls made with train = "fused", by the way they went ("bwd": launches of the HIP backward); tests read it
FEED_FORWARD_TRAIN_ROUTES = {"fused": 0, "torch": 0, "bwd": 0}
FEED_FORWARD_BWD_ROW_CHUNK = _lib.FFN_BWD_ROW_CHUNK             # tokens per partial plane of the backward's sums over tokens
# what the last fused training forward / backward handed to the op: (data_ptr, shape, strides) of its x view; tests read it
FEED_FORWARD_TRAIN_LAST = {"fwd": None, "bwd": None}
FEED_FORWARD_BF16_TRAIN_KINDS = ("torch", "fused")
DEFAULT_FEED_FORWARD_BF16_TRAIN = "torch"
# gradient-wanting calls on bfloat16 tensors or under bfloat16 autocast made with route, train, bf16 AND bf16_train = "fused", by the way
# they went ("bwd": launches of the bf16 HIP backward); tests read it
FEED_FORWARD_BF16_TRAIN_ROUTES = {"fused": 0, "torch": 0, "bwd": 0}
# what the last fused bf16 training forward / backward handed to the op, as FEED_FORWARD_TRAIN_LAST
FEED_FORWARD_BF16_TRAIN_LAST = {"fwd": None, "bwd": None}


def feed_forward_supported(D: int, hidden: int) -> bool:
    """semicrf_ffn_residual_supported: D a multiple of 8 in [8, 256], hidden a multiple of 8 in [8, 4096]."""
    return bool(_lib.load().semicrf_ffn_residual_supported(int(D), int(hidden)))


def feed_forward_bf16_supported(D: int, hidden: int) -> bool:
    """semicrf_ffn_residual_bf16_supported (both forms): the set of feed_forward_supported."""
    lib = _lib.load()
    return bool(lib.semicrf_ffn_residual_bf16_supported(int(D), int(hidden))
                and lib.semicrf_ffn_residual_bf16_mixed_supported(int(D), int(hidden)))


def feed_forward_torch(x, w1, b1, w2, b2, scale, eps=1e-6):
    """The stock route: ResBlock's expression around Linear, GELU, Linear in eval mode, op for op."""
    xn = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    return x + F.linear(F.gelu(F.linear(xn, w1, b1)), w2, b2) * scale


def _as_rows(t: torch.Tensor, order):
    """t [..., D] as the op's view [n0, n1, D] with the leading dimensions taken in `order` (the op is per token), or None."""
    lead = [(t.shape[i], t.stride(i)) for i in order if t.shape[i] != 1]
    merged = []
    for n, s in lead:                                           # merge what lies evenly spaced
        if merged and merged[-1][1] == s * n:
            merged[-1] = (merged[-1][0] * n, s)
        else:
            merged.append((n, s))
    if len(merged) > 2:
        return None
    while len(merged) < 2:
        merged.insert(0, (1, 0))
    (n0, s0), (n1, s1) = merged
    return torch.as_strided(t, (n0, n1, t.shape[-1]), (s0, s1, 1), t.storage_offset())


def _ffn_applies(x, w1, b1, w2, b2, scale, dtype=torch.float32) -> bool:
    ts = (x, w1, b1, w2, b2, scale)
    if any(t.dtype != dtype for t in ts) or any(t.device != x.device for t in ts):
        return False
    if x.device.type not in ("cuda", "cpu") or x.dim() < 1 or x.numel() == 0 or w1.dim() != 2 or w2.dim() != 2:
        return False
    D, hidden = x.shape[-1], w1.shape[0]
    if w1.shape != (hidden, D) or w2.shape != (D, hidden) or b1.shape != (hidden,) or b2.shape != (D,) or scale.shape != (D,):
        return False
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return False                                            # forward only
    return feed_forward_supported(D, hidden) if dtype == torch.float32 else feed_forward_bf16_supported(D, hidden)


def _ffn_pick(ts, bf16):
    """(op, is16): the torch op that answers the call -- "ffn_residual", "ffn_residual_bf16" (form A), "ffn_residual_bf16_mixed"
    (form B) or None for the stock expression -- and whether FEED_FORWARD_BF16_ROUTES counts it (the knob at "fused", and x
    bfloat16 or bfloat16 autocast on for x's device type)."""
    if bf16 != "fused":
        return ("ffn_residual" if _ffn_applies(*ts) else None), False
    x = ts[0]
    kind = x.device.type
    ac = torch.get_autocast_dtype(kind) if kind in ("cuda", "cpu") and torch.is_autocast_enabled(kind) else None
    is16 = x.dtype == torch.bfloat16 or ac == torch.bfloat16
    op = None
    if x.dtype == torch.bfloat16:
        if ac in (None, torch.bfloat16) and _ffn_applies(*ts, dtype=torch.bfloat16):
            op = "ffn_residual_bf16"
    elif ac is None:
        if _ffn_applies(*ts):
            op = "ffn_residual"
    elif ac == torch.bfloat16 and _ffn_applies(*ts):
        op = "ffn_residual_bf16_mixed"
    return op, is16


def _ffn_count(op, is16):
    FEED_FORWARD_ROUTES["torch" if op is None else "fused"] += 1
    if is16:
        FEED_FORWARD_BF16_ROUTES["torch" if op is None else "fused"] += 1


def _ffn_fused(x, w1, b1, w2, b2, scale, eps, op="ffn_residual"):
    if x.shape[-1] != 1 and x.stride(-1) != 1:
        x = x.contiguous()
    order = sorted(range(x.dim() - 1), key=lambda i: -x.stride(i))          # the tokens in the order of their addresses
    out = torch.empty_like(x)                                   # x's own layout when x is dense
    x3, o3 = _as_rows(x, order), _as_rows(out, order)
    if x3 is None or o3 is None or x3.shape != o3.shape:
        x = x.contiguous()
        out = torch.empty_like(x)
        order = list(range(x.dim() - 1))
        x3, o3 = _as_rows(x, order), _as_rows(out, order)
    getattr(_lib.ops(), op)(x3, w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(), scale.contiguous(), float(eps), o3)
    return out


def _seed_arg(seed) -> int:
    """A seed (any int; its low 64 bits count) as the signed 64-bit value the torch ops carry."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def feed_forward_dropout_mask(seed: int, rows: int, D: int, hidden: int, p_hidden: float, p_out: float, device="cpu"):
    """The two dropout masks of the fused training route as tensors: (bool [rows, hidden], bool [rows, D]), True = kept; the first
    belongs to the hidden activation (probability p_hidden), the second to the module's output (p_out); p = 0 keeps everything.  Row
    i is token i of the [n0, n1, D] view the wrapper hands to the op: the tokens in the order of their addresses (for a contiguous
    x: x.reshape(-1, D)'s rows).  A stateless function of (seed, stream, i, column) (Philox-4x32-10, include/semicrf_hip.h): the
    first rows of a larger `rows` are the same rows.  On a GPU by semicrf_ffn_dropout_mask, on the CPU by the host mirror: the same
    bits."""
    dev = torch.device(device)
    mh = torch.empty(int(rows), int(hidden), dtype=torch.uint8, device=dev)
    mo = torch.empty(int(rows), int(D), dtype=torch.uint8, device=dev)
    _lib.ops().ffn_dropout_mask(mh, mo, _seed_arg(seed), int(rows), int(D), int(hidden), float(p_hidden), float(p_out))
    return mh.view(torch.bool), mo.view(torch.bool)


def _rows_views(ts, order):
    """Tensors of one shape [..., D] as [n0, n1, D] views with one (n0, n1) that list the tokens in the same order (the leading
    dimensions taken in `order`), or None."""
    lead = [(ts[0].shape[i], [t.stride(i) for t in ts]) for i in order if ts[0].shape[i] != 1]
    merged = []
    for n, ss in lead:                                          # merge what lies evenly spaced in every tensor
        if merged and all(p == s * n for p, s in zip(merged[-1][1], ss)):
            merged[-1] = (merged[-1][0] * n, ss)
        else:
            merged.append((n, ss))
    if len(merged) > 2:
        return None
    while len(merged) < 2:
        merged.insert(0, (1, [0] * len(ts)))
    (n0, s0), (n1, s1) = merged
    return [torch.as_strided(t, (n0, n1, t.shape[-1]), (s0[k], s1[k], 1), t.storage_offset()) for k, t in enumerate(ts)]


def _ffn_train_applies(x, w1, b1, w2, b2, scale, p_hidden=0.0, p_out=0.0) -> bool:
    """The fused training route answers: float32 everywhere, one device, no autocast for it, a supported shape, p < 1."""
    ts = (x, w1, b1, w2, b2, scale)
    if any(t.dtype != torch.float32 for t in ts) or any(t.device != x.device for t in ts):
        return False
    kind = x.device.type
    if kind not in ("cuda", "cpu") or torch.is_autocast_enabled(kind) or x.dim() < 1 or x.numel() == 0 or w1.dim() != 2 or w2.dim() != 2:
        return False
    D, hidden = x.shape[-1], w1.shape[0]
    if w1.shape != (hidden, D) or w2.shape != (D, hidden) or b1.shape != (hidden,) or b2.shape != (D,) or scale.shape != (D,):
        return False
    if not (0.0 <= p_hidden < 1.0 and 0.0 <= p_out < 1.0):
        return False
    return bool(_lib.load().semicrf_ffn_residual_bwd_supported(int(D), int(hidden)))


class _FeedForwardTrain(torch.autograd.Function):
    """The op behind train = "fused": semicrf_ffn_residual_train_fwd and semicrf_ffn_residual_bwd."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, scale, eps, seed, p1, p2):
        xd = x.detach()
        if xd.shape[-1] != 1 and xd.stride(-1) != 1:
            xd = xd.contiguous()
        order = sorted(range(xd.dim() - 1), key=lambda i: -xd.stride(i))       # the tokens in the order of their addresses
        out = torch.empty_like(xd)
        views = _rows_views((xd, out), order)
        if views is None:
            xd = xd.contiguous()
            out = torch.empty_like(xd)
            order = list(range(xd.dim() - 1))
            views = _rows_views((xd, out), order)
        x3, o3 = views
        ntok, D, hidden = x3.shape[0] * x3.shape[1], x3.shape[2], w1.shape[0]
        z = torch.empty(ntok, hidden, dtype=torch.float32, device=xd.device)
        y = torch.empty(ntok, D, dtype=torch.float32, device=xd.device)
        w1, b1, w2, b2, scale = (t.detach().contiguous() for t in (w1, b1, w2, b2, scale))
        FEED_FORWARD_TRAIN_LAST["fwd"] = (x3.data_ptr(), tuple(x3.shape), tuple(x3.stride()))
        _lib.ops().ffn_residual_train_fwd(x3, w1, b1, w2, b2, scale, float(eps), seed, p1, p2, o3, z, y)
        ctx.save_for_backward(xd, z, y, w1, w2, scale)
        ctx.geom = (order, float(eps), seed, p1, p2)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xd, z, y, w1, w2, scale = ctx.saved_tensors
        order, eps, seed, p1, p2 = ctx.geom
        dev = xd.device
        hidden, D = w1.shape
        dx = torch.empty_like(xd)
        views = None
        if dout.dtype == torch.float32 and (dout.shape[-1] == 1 or dout.stride(-1) == 1):
            views = _rows_views((xd, dout, dx), order)
        if views is None:                                       # dout laid out like dx: then the three merge as x and out did
            dout = torch.empty_like(xd).copy_(dout)
            views = _rows_views((xd, dout, dx), order)
        x3, g3, d3 = views
        ntok = x3.shape[0] * x3.shape[1]
        flat = torch.empty(2 * hidden * D + hidden + 2 * D, dtype=torch.float32, device=dev)
        e1, e2, e3, e4 = hidden * D, hidden * D + hidden, 2 * hidden * D + hidden, 2 * hidden * D + hidden + D
        dW1, db1, dW2, db2, dscale = flat[:e1].view(hidden, D), flat[e1:e2], flat[e2:e3].view(D, hidden), flat[e3:e4], flat[e4:]
        if dev.type == "cpu":
            ws = torch.empty(0, dtype=torch.uint8)
        else:
            ws = torch.empty(int(_lib.load().semicrf_ffn_residual_bwd_workspace_bytes(ntok, D, hidden)), dtype=torch.uint8, device=dev)
        FEED_FORWARD_TRAIN_ROUTES["bwd"] += 1
        FEED_FORWARD_TRAIN_LAST["bwd"] = (x3.data_ptr(), tuple(x3.shape), tuple(x3.stride()), g3.data_ptr(), tuple(g3.stride()))
        _lib.ops().ffn_residual_bwd(g3, x3, z, y, w1, w2, scale, eps, seed, p1, p2, d3, dW1, db1, dW2, db2, dscale, ws)
        need = ctx.needs_input_grad
        grads = (dx, dW1, db1, dW2, db2, dscale)
        return tuple(g if need[i] else None for i, g in enumerate(grads)) + (None, None, None, None)


def _ffn_train(x, w1, b1, w2, b2, scale, eps, p_hidden, p_out, seed):
    if seed is None:
        if p_hidden > 0 or p_out > 0:
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()       # the CPU default generator: no device sync
            seed = (hi << 32) | lo
        else:
            seed = 0
    return _FeedForwardTrain.apply(x, w1, b1, w2, b2, scale, float(eps), _seed_arg(seed), float(p_hidden), float(p_out))


def _autocast_dtype(kind):
    return torch.get_autocast_dtype(kind) if kind in ("cuda", "cpu") and torch.is_autocast_enabled(kind) else None


def _ffn_bf16_train_form(x, w1, b1, w2, b2, scale, p_hidden=0.0, p_out=0.0):
    """(form, is16): "A" (bfloat16 tensors, outside autocast or under bfloat16 autocast), "B" (float32 tensors under bfloat16 autocast)
    or None where the fused bf16 training route does not answer; is16: x bfloat16 or bfloat16 autocast on (what the counter counts)."""
    ts = (x, w1, b1, w2, b2, scale)
    kind = x.device.type
    ac = _autocast_dtype(kind)
    is16 = x.dtype == torch.bfloat16 or ac == torch.bfloat16
    if any(t.device != x.device for t in ts) or kind not in ("cuda", "cpu"):
        return None, is16
    if all(t.dtype == torch.bfloat16 for t in ts) and ac in (None, torch.bfloat16):
        form = "A"
    elif all(t.dtype == torch.float32 for t in ts) and ac == torch.bfloat16:
        form = "B"
    else:
        return None, is16
    if x.dim() < 1 or x.numel() == 0 or w1.dim() != 2 or w2.dim() != 2:
        return None, is16
    D, hidden = x.shape[-1], w1.shape[0]
    if w1.shape != (hidden, D) or w2.shape != (D, hidden) or b1.shape != (hidden,) or b2.shape != (D,) or scale.shape != (D,):
        return None, is16
    if not (0.0 <= p_hidden < 1.0 and 0.0 <= p_out < 1.0):
        return None, is16
    if not _lib.load().semicrf_ffn_residual_bf16_bwd_supported(int(D), int(hidden)):
        return None, is16
    return form, is16


class _FeedForwardBf16Train(torch.autograd.Function):
    """The op behind bf16_train = "fused": semicrf_ffn_residual_bf16_train_fwd / _bwd (form A) and their _mixed forms (form B)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, scale, eps, seed, p1, p2, form):
        xd = x.detach()
        if xd.shape[-1] != 1 and xd.stride(-1) != 1:
            xd = xd.contiguous()
        order = sorted(range(xd.dim() - 1), key=lambda i: -xd.stride(i))       # the tokens in the order of their addresses
        out = torch.empty_like(xd)
        views = _rows_views((xd, out), order)
        if views is None:
            xd = xd.contiguous()
            out = torch.empty_like(xd)
            order = list(range(xd.dim() - 1))
            views = _rows_views((xd, out), order)
        x3, o3 = views
        ntok, D, hidden = x3.shape[0] * x3.shape[1], x3.shape[2], w1.shape[0]
        saved = torch.empty(int(_lib.load().semicrf_ffn_residual_bf16_train_saved_bytes(ntok, D, hidden)), dtype=torch.uint8, device=xd.device)
        w1, b1, w2, b2, scale = (t.detach().contiguous() for t in (w1, b1, w2, b2, scale))
        FEED_FORWARD_BF16_TRAIN_LAST["fwd"] = (x3.data_ptr(), tuple(x3.shape), tuple(x3.stride()))
        ops = _lib.ops()
        (ops.ffn_residual_bf16_train_fwd if form == "A" else ops.ffn_residual_bf16_mixed_train_fwd)(
            x3, w1, b1, w2, b2, scale, float(eps), seed, p1, p2, o3, saved)
        ctx.save_for_backward(xd, saved, w1, w2, scale)
        ctx.geom = (order, float(eps), seed, p1, p2, form)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dout):
        xd, saved, w1, w2, scale = ctx.saved_tensors
        order, eps, seed, p1, p2, form = ctx.geom
        dev = xd.device
        hidden, D = w1.shape
        dx = torch.empty_like(xd)
        views = None
        if dout.dtype == xd.dtype and (dout.shape[-1] == 1 or dout.stride(-1) == 1):
            views = _rows_views((xd, dout, dx), order)
        if views is None:                                       # dout laid out like dx: then the three merge as x and out did
            dout = torch.empty_like(xd).copy_(dout)
            views = _rows_views((xd, dout, dx), order)
        x3, g3, d3 = views
        ntok = x3.shape[0] * x3.shape[1]
        flat = torch.empty(2 * hidden * D + hidden + 2 * D, dtype=xd.dtype, device=dev)
        e1, e2, e3, e4 = hidden * D, hidden * D + hidden, 2 * hidden * D + hidden, 2 * hidden * D + hidden + D
        dW1, db1, dW2, db2, dscale = flat[:e1].view(hidden, D), flat[e1:e2], flat[e2:e3].view(D, hidden), flat[e3:e4], flat[e4:]
        if dev.type == "cpu":
            ws = torch.empty(0, dtype=torch.uint8)
        else:
            ws = torch.empty(int(_lib.load().semicrf_ffn_residual_bf16_bwd_workspace_bytes(ntok, D, hidden)), dtype=torch.uint8, device=dev)
        FEED_FORWARD_BF16_TRAIN_ROUTES["bwd"] += 1
        FEED_FORWARD_TRAIN_ROUTES["bwd"] += 1
        FEED_FORWARD_BF16_TRAIN_LAST["bwd"] = (x3.data_ptr(), tuple(x3.shape), tuple(x3.stride()), g3.data_ptr(), tuple(g3.stride()))
        ops = _lib.ops()
        (ops.ffn_residual_bf16_bwd if form == "A" else ops.ffn_residual_bf16_mixed_bwd)(
            g3, x3, saved, w1, w2, scale, eps, seed, p1, p2, d3, dW1, db1, dW2, db2, dscale, ws)
        need = ctx.needs_input_grad
        grads = (dx, dW1, db1, dW2, db2, dscale)
        return tuple(g if need[i] else None for i, g in enumerate(grads)) + (None, None, None, None, None)


def _ffn_bf16_train(form, x, w1, b1, w2, b2, scale, eps, p_hidden, p_out, seed):
    """The fused bf16 training call, counted: the seed rule of _ffn_train (a host value from the CPU generator)."""
    FEED_FORWARD_BF16_TRAIN_ROUTES["fused"] += 1
    FEED_FORWARD_TRAIN_ROUTES["fused"] += 1
    FEED_FORWARD_ROUTES["fused"] += 1
    FEED_FORWARD_BF16_ROUTES["fused"] += 1
    if seed is None:
        if p_hidden > 0 or p_out > 0:
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()       # the CPU default generator: no device sync
            seed = (hi << 32) | lo
        else:
            seed = 0
    return _FeedForwardBf16Train.apply(x, w1, b1, w2, b2, scale, float(eps), _seed_arg(seed), float(p_hidden), float(p_out), form)


def feed_forward_residual(x, w1, b1, w2, b2, scale, eps=1e-6, route="fused", bf16=DEFAULT_FEED_FORWARD_BF16,
                          train=DEFAULT_FEED_FORWARD_TRAIN, p_hidden=0.0, p_out=0.0, seed=None,
                          bf16_train=DEFAULT_FEED_FORWARD_BF16_TRAIN):
    """x + (W2 gelu(W1 rmsnorm(x) + b1) + b2) * scale per token: the feed-forward ResBlock in eval mode.  x [..., D] with a contiguous
    last dimension, any strides in front (a tensor whose rows cannot be handed over as two strides is made contiguous first); w1
    [hidden, D], b1 [hidden], w2 [D, hidden], b2 [D], scale [D] as nn.Linear and ResBlock hold them.  Returns [..., D], laid out in
    memory like x.

    route = "fused": the HIP op (the host kernel for CPU tensors) whenever it applies; the stock route (feed_forward_torch) when a
    dtype is not float32, the shape is outside the supported set (feed_forward_supported), or gradients are enabled and an input or
    a parameter requires grad.  route = "torch": always the stock route.  Always usable, always differentiable.

    bf16 = "torch" (the default): the above.  bf16 = "fused", with route = "fused": bfloat16 x and parameters take the bf16 HIP op
    (form A); float32 x and parameters under torch.autocast(dtype=torch.bfloat16) take the same kernel on the float32 tensors
    (form B: bf16 operands, float32 biases, LayerScale and result); float32 outside autocast stays the float32 op; any other mix of
    dtypes, and autocast to another dtype, is the stock route.

    train = "torch" (the default): the above.  train = "fused", with route = "fused": a call that wants a gradient (grad mode on, x or
    a parameter requires grad) on float32 tensors of one device, outside autocast, with a supported shape is the HIP op in its training
    mode and its HIP backward (semicrf_ffn_residual_train_fwd / _bwd; the host mirrors on the CPU): once differentiable (a second
    differentiation raises) w.r.t. x, w1, b1, w2, b2 and scale, every gradient bit-identical from run to run.  FEED_FORWARD_TRAIN_ROUTES
    counts the gradient-wanting calls made with train = "fused".

    p_hidden, p_out (default 0): the block in TRAINING mode, out = x + dropout(W2 dropout(gelu(..)) + b2) * scale.  On the fused
    training route element (token i, column j) is kept iff feed_forward_dropout_mask(seed, ...)[.][i, j]: a stateless function of
    (seed, i, j), so a token's output does not depend on the other tokens.  seed = None draws one value per call from torch's CPU
    default generator when something drops (torch.manual_seed makes runs reproducible, and torch.utils.checkpoint's RNG preservation
    reproduces the mask on recomputation; nothing waits for the device); an explicit seed makes the call reproducible.  The seed is a
    HOST value: a call captured in a HIP graph replays one and the same mask.  On every other route the two dropouts are
    F.dropout's.

    bf16_train = "torch" (the default): the above.  bf16_train = "fused", with route, train AND bf16 = "fused": a call that wants a
    gradient on bfloat16 x and parameters (outside autocast or under bfloat16 autocast: form A) or on float32 x and parameters under
    bfloat16 autocast (form B: float32 parameters and gradients, bf16 operands inside the launch) is the bf16 HIP op in its training
    mode and its HIP backward (semicrf_ffn_residual_bf16_train_fwd / _bwd and their _mixed forms; the host mirrors on the CPU): once
    differentiable, the same masks and the same seed rule as train = "fused", every gradient bit-identical from run to run.  float32
    outside autocast stays the float32 training route; every other case is what it was.  FEED_FORWARD_BF16_TRAIN_ROUTES counts the
    gradient-wanting bfloat16 / bfloat16-autocast calls made with all four at "fused"; a fused answer counts in
    FEED_FORWARD_TRAIN_ROUTES, FEED_FORWARD_ROUTES and FEED_FORWARD_BF16_ROUTES too."""
    if route not in FEED_FORWARD_KINDS:
        raise ValueError(f"route must be one of {FEED_FORWARD_KINDS}, not {route!r}")
    if bf16 not in FEED_FORWARD_BF16_KINDS:
        raise ValueError(f"bf16 must be one of {FEED_FORWARD_BF16_KINDS}, not {bf16!r}")
    if train not in FEED_FORWARD_TRAIN_KINDS:
        raise ValueError(f"train must be one of {FEED_FORWARD_TRAIN_KINDS}, not {train!r}")
    if bf16_train not in FEED_FORWARD_BF16_TRAIN_KINDS:
        raise ValueError(f"bf16_train must be one of {FEED_FORWARD_BF16_TRAIN_KINDS}, not {bf16_train!r}")
    drops = p_hidden > 0 or p_out > 0

    def stock():
        if not drops:
            return feed_forward_torch(x, w1, b1, w2, b2, scale, eps)
        xn = x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
        return x + F.dropout(F.linear(F.dropout(F.gelu(F.linear(xn, w1, b1)), p_hidden), w2, b2), p_out) * scale

    if route == "torch":
        FEED_FORWARD_ROUTES["torch"] += 1
        return stock()
    ts = (x, w1, b1, w2, b2, scale)
    if train == "fused" and torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        if _ffn_train_applies(*ts, p_hidden, p_out):
            FEED_FORWARD_TRAIN_ROUTES["fused"] += 1
            FEED_FORWARD_ROUTES["fused"] += 1
            return _ffn_train(*ts, eps, p_hidden, p_out, seed)
        if bf16_train == "fused" and bf16 == "fused":
            form, is16 = _ffn_bf16_train_form(*ts, p_hidden, p_out)
            if form is not None:
                return _ffn_bf16_train(form, *ts, eps, p_hidden, p_out, seed)
            if is16:
                FEED_FORWARD_BF16_TRAIN_ROUTES["torch"] += 1
        FEED_FORWARD_TRAIN_ROUTES["torch"] += 1
    op, is16 = _ffn_pick(ts, bf16)
    if drops:
        op = None
    _ffn_count(op, is16)
    if op is None:
        return stock()
    return _ffn_fused(x, w1, b1, w2, b2, scale, eps, op)


# ---- the modules --------------------------------------------------------------------------------------------------------------------
class RMSNorm(nn.Module):
    """x / sqrt(mean(x^2) + eps) over the last dimension; no parameters."""

    def __init__(self, eps=1e-6):
        super().__init__()
        self.eps = eps

    def forward(self, x):
        return x * torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + self.eps)


class TiedDropout(nn.Module):
    """Dropout whose mask is shared along `axis` (training only)."""

    def __init__(self, dropoutProb, axis):
        super().__init__()
        self.dropout = nn.Dropout(dropoutProb)
        self.axis = axis

    def forward(self, x):
        if not self.training:
            return x
        shape = list(x.shape)
        shape[self.axis] = 1
        return self.dropout(torch.ones(*shape, device=x.device)) * x


class LearnableSpatialPositionEmbedding(nn.Module):
    """Random-Fourier-feature position embedding with a learnable projection: mlp(cos(proj(coord)) / sqrt(embedSize / 2))."""

    def __init__(self, embedSize, coordDim, gamma=10.0, dropoutProb=0.0):
        super().__init__()
        self.gamma = gamma
        self.proj = nn.Linear(coordDim, embedSize)
        self.mlp = nn.Sequential(nn.Linear(embedSize, 4 * embedSize), nn.GELU(), nn.Dropout(dropoutProb),
                                 nn.Linear(4 * embedSize, embedSize))
        self.dropout = nn.Dropout(dropoutProb)
        self._reset_parameters()

    def _reset_parameters(self):
        nn.init.normal_(self.proj.weight, std=1 / self.gamma)
        nn.init.uniform_(self.proj.bias, a=-math.pi, b=math.pi)

    def forwardWithCoordVec(self, coord):
        """coord [..., coordDim] -> [..., embedSize] (coordinates are taken in the projection's dtype)."""
        phi = self.proj(coord.to(self.proj.weight.dtype))
        return self.mlp(torch.cos(phi) / math.sqrt(phi.shape[-1] / 2))

    def forward(self, *coords):
        """One 1-d coordinate vector per dimension -> the embedding of their grid [len(c0), len(c1), .., embedSize]."""
        return self.forwardWithCoordVec(torch.stack(torch.meshgrid(coords, indexing="ij"), dim=-1))


class ResBlock(nn.Module):
    """x + dropout(module(norm(x), *args)) * scale: pre-norm residual with LayerScale (initialised to 1e-2).  Only x is normalised.

    feedForward: "torch" (the default: the expression above as it stands) or "fused": when the module is the `Linear, GELU, Dropout,
    Linear` sequence of a feed-forward block, no extra arguments are passed and no dropout is active (eval mode or p = 0), the block
    is feed_forward_residual's one op wherever that applies (float32, a supported shape, no gradient wanted); the expression above
    in every other case.
    feedForwardBf16: "torch" (the default: the above) or "fused": where feedForward = "fused" and its conditions hold, a block whose
    input and parameters are all bfloat16 is the bf16 HIP op, and a float32 block under bfloat16 autocast is the same kernel on its
    float32 tensors (feed_forward_residual's bf16 = "fused").
    feedForwardTrain: "torch" (the default: the above) or "fused": where feedForward = "fused" and the module is the feed-forward
    sequence, a call that wants a gradient -- with its dropouts active or not -- is feed_forward_residual's train = "fused" route
    (the HIP op in training mode and its HIP backward) on float32 tensors outside autocast with a supported shape and no extra
    arguments; p comes from module[2] and self.dropout where they are in training mode, else 0.  bfloat16, autocast, extra
    arguments and an unsupported shape take the stock expression.
    feedForwardBf16Train: "torch" (the default: the above) or "fused": where feedForward, feedForwardTrain AND feedForwardBf16 are
    "fused", a gradient-wanting call of a bfloat16 block, or of a float32 block under bfloat16 autocast, is feed_forward_residual's
    bf16_train = "fused" route (the bf16 HIP op in training mode and its HIP backward; float32 parameters keep float32 gradients)."""

    def __init__(self, module, size, prenorm=True, dropoutProb=0.0):
        super().__init__()
        self.module = module
        self.norm = RMSNorm()
        self.scale = nn.Parameter(torch.ones(size) * 1e-2)
        self.dropout = nn.Dropout(dropoutProb)
        self.feedForward = DEFAULT_FEED_FORWARD
        self.feedForwardBf16 = DEFAULT_FEED_FORWARD_BF16
        self.feedForwardTrain = DEFAULT_FEED_FORWARD_TRAIN
        self.feedForwardBf16Train = DEFAULT_FEED_FORWARD_BF16_TRAIN

    def is_feed_forward(self) -> bool:
        """The module is the Linear, GELU (exact), Dropout, Linear sequence of _feed_forward."""
        m = self.module
        return (isinstance(m, nn.Sequential) and len(m) == 4 and isinstance(m[0], nn.Linear) and isinstance(m[1], nn.GELU)
                and getattr(m[1], "approximate", "none") == "none" and isinstance(m[2], nn.Dropout) and isinstance(m[3], nn.Linear)
                and m[0].bias is not None and m[3].bias is not None and type(self.norm) is RMSNorm)

    def _fused_feed_forward(self, x, args):
        """The fused op's answer, or None for the stock expression; counts the call either way."""
        if self.feedForwardBf16 not in FEED_FORWARD_BF16_KINDS:
            raise ValueError(f"feedForwardBf16 must be one of {FEED_FORWARD_BF16_KINDS}, not {self.feedForwardBf16!r}")
        kind = getattr(self, "feedForwardTrain", DEFAULT_FEED_FORWARD_TRAIN)
        if kind not in FEED_FORWARD_TRAIN_KINDS:
            raise ValueError(f"feedForwardTrain must be one of {FEED_FORWARD_TRAIN_KINDS}, not {kind!r}")
        kind16 = getattr(self, "feedForwardBf16Train", DEFAULT_FEED_FORWARD_BF16_TRAIN)
        if kind16 not in FEED_FORWARD_BF16_TRAIN_KINDS:
            raise ValueError(f"feedForwardBf16Train must be one of {FEED_FORWARD_BF16_TRAIN_KINDS}, not {kind16!r}")
        op, is16 = None, False
        if self.feedForward == "fused" and self.is_feed_forward():
            m = self.module
            params = (m[0].weight, m[0].bias, m[3].weight, m[3].bias, self.scale)
            if kind == "fused" and torch.is_grad_enabled() and any(t.requires_grad for t in (x, *params)):
                p1 = float(m[2].p) if m[2].training else 0.0
                p2 = float(self.dropout.p) if self.dropout.training else 0.0
                if not args and _ffn_train_applies(x, *params, p1, p2):
                    FEED_FORWARD_TRAIN_ROUTES["fused"] += 1
                    FEED_FORWARD_ROUTES["fused"] += 1
                    return _ffn_train(x, *params, self.norm.eps, p1, p2, None)
                if kind16 == "fused" and self.feedForwardBf16 == "fused":
                    form, is16t = _ffn_bf16_train_form(x, *params, p1, p2)
                    if form is not None and not args:
                        return _ffn_bf16_train(form, x, *params, self.norm.eps, p1, p2, None)
                    if is16t:
                        FEED_FORWARD_BF16_TRAIN_ROUTES["torch"] += 1
                FEED_FORWARD_TRAIN_ROUTES["torch"] += 1
            op, is16 = _ffn_pick((x, *params), self.feedForwardBf16)
            if args or (self.training and (self.dropout.p > 0 or m[2].p > 0)):
                op = None
        _ffn_count(op, is16)
        return None if op is None else _ffn_fused(x, *params, self.norm.eps, op)

    def forward(self, x, *args):
        if self.feedForward != DEFAULT_FEED_FORWARD:             # a block left at "torch" touches nothing, the counters included
            out = self._fused_feed_forward(x, args)
            if out is not None:
                return out
        return x + self.dropout(self.module(self.norm(x), *args)) * self.scale


class MultiHeadAttentionKernel(nn.Module):
    """Multi-head attention with bias-free q / k / v projections stored [in, hidden] and a Linear output projection.  Only
    kernel = None (exact softmax attention) is implemented, as in the reference: with any other kernel the parameters exist (a
    checkpoint loads) and forward raises NotImplementedError.

    attention: "fused" (axial_attention's HIP op where it applies; the stock route under autograd), "fused-train" (the HIP op and its
    HIP backward under autograd) or "torch" (the stock route).
    attentionBf16: "torch" (bfloat16 tensors take the stock route: the default) or "fused" (axial_attention's bf16 HIP op where it
    applies, forward only).
    attentionBf16Train: "torch" (the default) or "fused": with attention = "fused-train" and attentionBf16 = "fused", bfloat16 calls
    under autograd run the bf16 HIP op and its HIP backward."""

    def __init__(self, embed_dim, num_heads, dropout=0., k_dim=None, v_dim=None, fourierSize=32, kernel="fourier", hiddenFactor=1):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.kernel = kernel
        self.fourierSize = fourierSize
        self.head_dim = int(math.ceil(math.ceil(hiddenFactor * embed_dim) / num_heads))
        hiddenSize = self.head_dim * num_heads
        self.q_proj_weight = nn.Parameter(torch.empty((embed_dim, hiddenSize)))
        self.k_proj_weight = nn.Parameter(torch.empty((embed_dim if k_dim is None else k_dim, hiddenSize)))
        self.v_proj_weight = nn.Parameter(torch.empty((embed_dim if v_dim is None else v_dim, hiddenSize)))
        self.out_proj = nn.Linear(hiddenSize, embed_dim)
        if kernel is not None:
            self.gamma = nn.Parameter(torch.tensor(1.0))
            self.norm = RMSNorm()
        self.attention = DEFAULT_ATTENTION
        self.attentionBf16 = DEFAULT_ATTENTION_BF16
        self.attentionBf16Train = DEFAULT_ATTENTION_BF16_TRAIN
        self._reset_parameters()

    def _reset_parameters(self):
        for w in (self.k_proj_weight, self.q_proj_weight, self.v_proj_weight):
            nn.init.xavier_uniform_(w)

    def forward(self, query, key=None, value=None, seq_dim=-2):
        """query [..., Lq, embed_dim], key / value [..., Lk, .] (key defaults to query, value to key) -> [..., Lq, embed_dim].
        seq_dim = -3: the SEQUENCE is dimension -3 of the inputs and dimension -2 counts independent sequences -- the attention along
        the other axis of the same buffers, without transposing them (the projections are per token)."""
        if key is None:
            key = query
        if value is None:
            value = key
        if self.kernel is not None:
            raise NotImplementedError("MultiHeadAttentionKernel: only kernel = None is implemented")
        if seq_dim not in (-2, -3):
            raise ValueError("seq_dim must be -2 or -3")
        q, k, v = query @ self.q_proj_weight, key @ self.k_proj_weight, value @ self.v_proj_weight
        if seq_dim == -3:
            q, k, v = q.transpose(-3, -2), k.transpose(-3, -2), v.transpose(-3, -2)
        fetched = axial_attention(q, k, v, self.num_heads, route=self.attention, bf16=self.attentionBf16,
                                  bf16_train=self.attentionBf16Train)
        if seq_dim == -3:
            fetched = fetched.transpose(-3, -2)
        return self.out_proj(fetched)


def _feed_forward(inputSize, hiddenSize, dropoutProb):
    return nn.Sequential(nn.Linear(inputSize, hiddenSize), nn.GELU(), nn.Dropout(dropoutProb), nn.Linear(hiddenSize, inputSize))


class BasicBlock(nn.Module):
    """One transformer layer over x [N, T, F, D]: per enabled axis an attention ResBlock and a feed-forward ResBlock.
    "F": along the frequency axis; "T": along the time axis; "All0" / "0All": between the rest and the first frequency track;
    "FT": over all tokens (kernel "positive": not implemented, as in the reference).

    With attention = "fused" or "fused-train" the "F" and "T" halves run on the [N, T, F, D] buffer as it is: everything but the
    attention is per token, and the two halves differ only in which dimension the attention is told is the sequence.  With "torch"
    the block follows the reference's order of operations, `transpose(-3, -2)` around the time-axis half included.
    attentionBf16 = "torch" | "fused" sets the bfloat16 knob of all its attention modules, attentionBf16Train = "torch" | "fused"
    their bfloat16 training knob; feedForward = "torch" | "fused" and feedForwardBf16 = "torch" | "fused" set the two knobs of all
    its feed-forward blocks (ResBlock)."""

    def __init__(self, inputSize, num_heads, fourierSize, hiddenFactor=2, hiddenFactorAttn=1, approxKernels=[None, None, None, None],
                 enabled=["F", "T", "All0", "0All"], dropoutProb=0.0):
        super().__init__()
        fnnHiddenSize = int(math.ceil(inputSize * hiddenFactor))
        self.enabled = enabled

        def attn(kernel, fourier):
            return ResBlock(MultiHeadAttentionKernel(inputSize, num_heads=num_heads, fourierSize=fourier, kernel=kernel,
                                                     hiddenFactor=hiddenFactorAttn), size=inputSize, dropoutProb=dropoutProb)

        def fnn():
            return ResBlock(_feed_forward(inputSize, fnnHiddenSize, dropoutProb), size=inputSize, dropoutProb=dropoutProb)

        if "F" in enabled:
            self.mhaBlockF, self.fnnBlockF = attn(approxKernels[0], fourierSize), fnn()
        if "T" in enabled:
            self.mhaBlockT, self.fnnBlockT = attn(approxKernels[1], fourierSize), fnn()
        if "All0" in enabled or "0All" in enabled:
            self.mhaBlockAll0, self.fnnBlockAll0 = attn(approxKernels[2], fourierSize), fnn()
        if "FT" in enabled:
            self.mhaBlockFT, self.fnnBlockFT = attn("positive", 64), fnn()

    def attention_modules(self):
        return [m for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)]

    @property
    def attention(self):
        routes = {m.attention for m in self.attention_modules()}
        return routes.pop() if len(routes) == 1 else "mixed"

    @attention.setter
    def attention(self, route):
        if route not in ROUTES:
            raise ValueError(f"attention must be one of {ROUTES}, not {route!r}")
        for m in self.attention_modules():
            m.attention = route

    @property
    def attentionBf16(self):
        kinds = {m.attentionBf16 for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @attentionBf16.setter
    def attentionBf16(self, kind):
        if kind not in BF16_KINDS:
            raise ValueError(f"attentionBf16 must be one of {BF16_KINDS}, not {kind!r}")
        for m in self.modules():
            if isinstance(m, MultiHeadAttentionKernel):
                m.attentionBf16 = kind

    @property
    def attentionBf16Train(self):
        kinds = {m.attentionBf16Train for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @attentionBf16Train.setter
    def attentionBf16Train(self, kind):
        if kind not in BF16_TRAIN_KINDS:
            raise ValueError(f"attentionBf16Train must be one of {BF16_TRAIN_KINDS}, not {kind!r}")
        for m in self.modules():
            if isinstance(m, MultiHeadAttentionKernel):
                m.attentionBf16Train = kind

    def feed_forward_blocks(self):
        return [m for m in self.modules() if isinstance(m, ResBlock) and m.is_feed_forward()]

    @property
    def feedForward(self):
        kinds = {m.feedForward for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @feedForward.setter
    def feedForward(self, kind):
        if kind not in FEED_FORWARD_KINDS:
            raise ValueError(f"feedForward must be one of {FEED_FORWARD_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForward = kind

    @property
    def feedForwardBf16(self):
        kinds = {m.feedForwardBf16 for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @feedForwardBf16.setter
    def feedForwardBf16(self, kind):
        if kind not in FEED_FORWARD_BF16_KINDS:
            raise ValueError(f"feedForwardBf16 must be one of {FEED_FORWARD_BF16_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardBf16 = kind

    @property
    def feedForwardTrain(self):
        kinds = {getattr(m, "feedForwardTrain", DEFAULT_FEED_FORWARD_TRAIN) for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else ("mixed" if kinds else DEFAULT_FEED_FORWARD_TRAIN)

    @feedForwardTrain.setter
    def feedForwardTrain(self, kind):
        if kind not in FEED_FORWARD_TRAIN_KINDS:
            raise ValueError(f"feedForwardTrain must be one of {FEED_FORWARD_TRAIN_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardTrain = kind

    @property
    def feedForwardBf16Train(self):
        kinds = {getattr(m, "feedForwardBf16Train", DEFAULT_FEED_FORWARD_BF16_TRAIN) for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else ("mixed" if kinds else DEFAULT_FEED_FORWARD_BF16_TRAIN)

    @feedForwardBf16Train.setter
    def feedForwardBf16Train(self, kind):
        if kind not in FEED_FORWARD_BF16_TRAIN_KINDS:
            raise ValueError(f"feedForwardBf16Train must be one of {FEED_FORWARD_BF16_TRAIN_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardBf16Train = kind

    def forward(self, x, mem=None, crossAttn=False):
        nT, nF = x.shape[-3], x.shape[-2]
        if mem is None:
            mem = x
        h = x
        if "F" in self.enabled:
            h = self.fnnBlockF(self.mhaBlockF(h, mem))
        rest = [e for e in self.enabled if e not in ("F", "T")]
        if self.attention in ("fused", "fused-train"):
            if "T" in self.enabled:                              # the same buffers, the other axis: nothing is transposed
                h = self.fnnBlockT(self.mhaBlockT(h, mem, None, -3))
            if not rest:
                return h
            h, mem = h.transpose(-3, -2), mem.transpose(-3, -2)
        else:
            h, mem = h.transpose(-3, -2), mem.transpose(-3, -2)  # [N, F, T, D]
            if "T" in self.enabled:
                h = self.fnnBlockT(self.mhaBlockT(h, mem))
        if "All0" in self.enabled or "0All" in self.enabled:
            h0, h1 = h.split([1, h.shape[-3] - 1], dim=-3)
            if "All0" in self.enabled:
                h1 = self.mhaBlockAll0(h1, mem[..., 0:1, :, :])
            if "0All" in self.enabled:
                h0 = self.mhaBlockAll0(h0, mem.flatten(-3, -2).unsqueeze(-3))
            h = self.fnnBlockAll0(torch.cat([h0, h1], dim=-3))
        if "FT" in self.enabled:
            h = self.fnnBlockFT(self.mhaBlockFT(h.flatten(-3, -2), mem.flatten(-3, -2))).unflatten(-2, (nF, nT))
        h = h.transpose(-3, -2)
        assert h.shape == x.shape
        return h


def _down_stage(cin, cout, stride, dropoutProb):
    return [nn.Conv2d(cin, cout, 3, padding=1, stride=stride), nn.GroupNorm(4, cout), nn.GELU(), nn.Dropout2d(dropoutProb)]


class Backbone(nn.Module):
    """x [N, T, F, inputSize] (the frontend's features), outputIndices [P] -> ctx [N, P, T, baseSize * expansionFactor].

    A convolution stem (3 x 3 input convolution plus a frequency position embedding, then three strided stages: patches of 8 frames
    x 4 bins with downsampleF, 8 x 1 without) gives tokens of width 4 baseSize on a [T / 8, F / 4] grid; one aggregation track is
    prepended on each axis; P target tokens per frame row (position embeddings of (time, output index)) are appended along the
    frequency axis; nLayers BasicBlocks; the target tokens are upsampled 8x in time by a transposed convolution and cut to T.

    attention: "fused" | "fused-train" | "torch" for all layers (the property reads "mixed" when they differ).
    attentionBf16: "torch" | "fused" for the bfloat16 calls of all layers, likewise.
    attentionBf16Train: "torch" | "fused" for the bfloat16 calls of all layers under autograd, likewise.
    feedForward: "torch" | "fused" for the feed-forward blocks of all layers, likewise.
    feedForwardBf16: "torch" | "fused" for their bfloat16 and bfloat16-autocast calls, likewise."""

    def __init__(self, inputSize, baseSize, posEmbedInitGamma, nHead, fourierSize=16, hiddenFactor=2, hiddenFactorAttn=1,
                 expansionFactor=1, dropoutProb=0.0, nLayers=4, enabledAttn=["F", "T"], useGradientCheckpoint=True, downsampleF=True,
                 upsampleProjOnly=True):
        super().__init__()
        b = baseSize
        self.posEmbedBuilder = LearnableSpatialPositionEmbedding(b, coordDim=1, gamma=posEmbedInitGamma, dropoutProb=dropoutProb)
        self.inputConv = nn.Conv2d(inputSize, b, kernel_size=3, padding=1)
        self.dropoutTied = TiedDropout(dropoutProb, axis=-3)
        fs = 2 if downsampleF else 1                              # the frequency stride of stages 2 and 3
        self.downConv = nn.Sequential(
            nn.ConstantPad2d((2, 1, 4, 3) if downsampleF else (0, 0, 4, 3), value=0.0),
            *_down_stage(b, 2 * b, (2, 1), dropoutProb),
            *_down_stage(2 * b, 4 * b, (2, fs), dropoutProb),
            *_down_stage(4 * b, 4 * b, (2, fs), dropoutProb),
            nn.Conv2d(4 * b, 4 * b, 3, padding=1),
            nn.GroupNorm(4, 4 * b))
        self.upConv1dSkip = nn.ConvTranspose1d(4 * b, b * expansionFactor, 8, stride=8)
        if not upsampleProjOnly:
            self.upConv1d = nn.Sequential(
                nn.ConvTranspose1d(4 * b, 4 * b, 2, stride=2), nn.Conv1d(4 * b, 4 * b, 3, padding=1), nn.GroupNorm(4, 4 * b), nn.GELU(),
                nn.ConvTranspose1d(4 * b, 2 * b, 2, stride=2), nn.Conv1d(2 * b, 2 * b, 3, padding=1), nn.GroupNorm(4, 2 * b), nn.GELU(),
                nn.ConvTranspose1d(2 * b, b, 2, stride=2), nn.Conv1d(b, b, 3, padding=1))
        self.upsampleProjOnly = upsampleProjOnly
        self.posEmbedBuilderAttnTF = LearnableSpatialPositionEmbedding(4 * b, coordDim=2, gamma=posEmbedInitGamma, dropoutProb=dropoutProb)
        self.posEmbedBuilderAttnTE = LearnableSpatialPositionEmbedding(4 * b, coordDim=2, gamma=posEmbedInitGamma, dropoutProb=dropoutProb)
        self.encoderLayers = nn.ModuleList([
            BasicBlock(inputSize=4 * b, num_heads=nHead, fourierSize=fourierSize, dropoutProb=dropoutProb, hiddenFactor=hiddenFactor,
                       hiddenFactorAttn=hiddenFactorAttn, enabled=enabledAttn) for _ in range(nLayers)])
        self.normEncoder = nn.Identity()
        self.useGradientCheckpoint = useGradientCheckpoint
        self.dropout = nn.Dropout(dropoutProb)

    @property
    def attention(self):
        routes = {m.attention for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)}
        return routes.pop() if len(routes) == 1 else "mixed"

    @attention.setter
    def attention(self, route):
        if route not in ROUTES:
            raise ValueError(f"attention must be one of {ROUTES}, not {route!r}")
        for m in self.modules():
            if isinstance(m, MultiHeadAttentionKernel):
                m.attention = route

    @property
    def attentionBf16(self):
        kinds = {m.attentionBf16 for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @attentionBf16.setter
    def attentionBf16(self, kind):
        if kind not in BF16_KINDS:
            raise ValueError(f"attentionBf16 must be one of {BF16_KINDS}, not {kind!r}")
        for m in self.modules():
            if isinstance(m, MultiHeadAttentionKernel):
                m.attentionBf16 = kind

    @property
    def attentionBf16Train(self):
        kinds = {m.attentionBf16Train for m in self.modules() if isinstance(m, MultiHeadAttentionKernel)}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @attentionBf16Train.setter
    def attentionBf16Train(self, kind):
        if kind not in BF16_TRAIN_KINDS:
            raise ValueError(f"attentionBf16Train must be one of {BF16_TRAIN_KINDS}, not {kind!r}")
        for m in self.modules():
            if isinstance(m, MultiHeadAttentionKernel):
                m.attentionBf16Train = kind

    def feed_forward_blocks(self):
        return [m for m in self.modules() if isinstance(m, ResBlock) and m.is_feed_forward()]

    @property
    def feedForward(self):
        kinds = {m.feedForward for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @feedForward.setter
    def feedForward(self, kind):
        if kind not in FEED_FORWARD_KINDS:
            raise ValueError(f"feedForward must be one of {FEED_FORWARD_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForward = kind

    @property
    def feedForwardBf16(self):
        kinds = {m.feedForwardBf16 for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else "mixed"

    @feedForwardBf16.setter
    def feedForwardBf16(self, kind):
        if kind not in FEED_FORWARD_BF16_KINDS:
            raise ValueError(f"feedForwardBf16 must be one of {FEED_FORWARD_BF16_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardBf16 = kind

    @property
    def feedForwardTrain(self):
        kinds = {getattr(m, "feedForwardTrain", DEFAULT_FEED_FORWARD_TRAIN) for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else ("mixed" if kinds else DEFAULT_FEED_FORWARD_TRAIN)

    @feedForwardTrain.setter
    def feedForwardTrain(self, kind):
        if kind not in FEED_FORWARD_TRAIN_KINDS:
            raise ValueError(f"feedForwardTrain must be one of {FEED_FORWARD_TRAIN_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardTrain = kind

    @property
    def feedForwardBf16Train(self):
        kinds = {getattr(m, "feedForwardBf16Train", DEFAULT_FEED_FORWARD_BF16_TRAIN) for m in self.feed_forward_blocks()}
        return kinds.pop() if len(kinds) == 1 else ("mixed" if kinds else DEFAULT_FEED_FORWARD_BF16_TRAIN)

    @feedForwardBf16Train.setter
    def feedForwardBf16Train(self, kind):
        if kind not in FEED_FORWARD_BF16_TRAIN_KINDS:
            raise ValueError(f"feedForwardBf16Train must be one of {FEED_FORWARD_BF16_TRAIN_KINDS}, not {kind!r}")
        for m in self.feed_forward_blocks():
            m.feedForwardBf16Train = kind

    def tokens(self, x, outputIndices):
        """The input of the first layer: [N, T', F' + P, 4 baseSize], the spectrogram tokens followed by the target tokens."""
        x = x.permute(0, 3, 1, 2)                                 # [N, C, T, F]
        dev, dt = x.device, x.dtype
        posF = self.posEmbedBuilder(torch.arange(x.shape[-1], device=dev).to(dt))             # [F, baseSize]
        h = self.downConv(self.inputConv(x) + posF.transpose(-1, -2).unsqueeze(-2))
        h = F.pad(h.permute(0, 2, 3, 1), (0, 0, 1, 0, 1, 0))      # [N, T', F', D]: one aggregation track in front of each axis
        coordT = torch.arange(h.shape[-3], device=dev).to(dt)
        coordF = torch.arange(h.shape[-2], device=dev).to(dt)
        h = h + self.posEmbedBuilderAttnTF(coordT, coordF)
        target = self.posEmbedBuilderAttnTE(coordT, outputIndices.to(dt))
        return torch.cat([h, target.unsqueeze(0).repeat(h.shape[0], 1, 1, 1)], dim=-2), target.shape[-2]

    def forward(self, x, outputIndices):
        nT = x.shape[1]
        hAll, nTarget = self.tokens(x, outputIndices)
        checkpointed = self.useGradientCheckpoint or self.training
        for layer in self.encoderLayers:
            hAll = torch.utils.checkpoint.checkpoint(layer, hAll, use_reentrant=False) if checkpointed else layer(hAll)
        hTarget = hAll[..., hAll.shape[-2] - nTarget:, :]
        hTarget = hTarget[..., 1:, :, :].permute(0, 2, 3, 1).flatten(0, 1)        # [N P, D, T' - 1]: without the time aggregation track
        up = self.upConv1dSkip(hTarget)
        if not self.upsampleProjOnly:
            up = self.upConv1d(hTarget) + up
        return up.unflatten(0, (x.shape[0], nTarget))[..., :nT].permute(0, 1, 3, 2)          # [N, P, T, D]
