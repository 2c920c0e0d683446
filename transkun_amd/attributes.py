"""Interval features for the attribute heads -- host-side mirror of TransKun.fetchIntervalFeaturesBatch
(/root/reference/transkun/ModelTransformer.py:501-532) and of the concatenation that feeds the velocity and
onset/offset predictors (:578-582), on top of the HIP gather kernel.

The reference walks the decoded Python lists per segment, builds index tensors on the host, copies them to the device
and runs two index_selects per segment.  `attribute_input_packed` consumes the packed (begin, end) pairs + offsets
that `semicrf_viterbi` leaves in HBM, so decode -> features needs no host round trip; `fetchIntervalFeaturesBatch`
keeps the reference's signature (Python lists in, four tensors out) for callers that already hold lists.
"""
from __future__ import annotations

import importlib
import weakref
from typing import List, Sequence, Tuple

import torch

from . import _lib

_nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")


class _IntervalFeatures(torch.autograd.Function):
    """out [K, 3D] = [ctx[c,b] | ctx[c,e] | ctx[c,b] * ctx[c,e]]; differentiable w.r.t. ctx (training calls the
    reference method with the ground-truth intervals, ModelTransformer.py:286-290)."""

    @staticmethod
    def forward(ctx_, ctx3, pairs, offsets, K, nSym):
        C, T, D = ctx3.shape
        out = torch.empty(K, 3 * D, dtype=torch.float32, device=ctx3.device)
        sym = torch.empty(K, dtype=torch.int64, device=ctx3.device)
        sc = torch.empty(K, dtype=torch.int64, device=ctx3.device)
        _lib.ops().interval_features_gather(ctx3, C, T, D, ctx3.stride(-2), pairs, int(K), offsets, int(nSym), out, sym, sc)
        ctx_.save_for_backward(ctx3, pairs, offsets)
        ctx_.K = K
        ctx_.mark_non_differentiable(sym, sc)
        return out, sym, sc

    @staticmethod
    def backward(ctx_, gout, gsym, gsc):
        ctx3, pairs, offsets = ctx_.saved_tensors
        C, T, D = ctx3.shape
        dctx = torch.zeros_like(ctx3)
        g = gout.contiguous()
        _lib.ops().interval_features_gather_bwd(g, ctx3, C, T, D, ctx3.stride(-2), pairs, int(ctx_.K), offsets, dctx, dctx.stride(-2))
        return dctx, None, None, None, None


def attribute_input_packed(ctxBatch: torch.Tensor, pairs: torch.Tensor, offsets: torch.Tensor, K: int = None):
    """ctxBatch [N, SYM, T, D] on the GPU; pairs int32 [>=K, 2] and offsets int32 [N*SYM+1] on the same device (chain
    c = n*SYM + sym, the order of NeuralSemiCRFInterval.decode).  Returns (attributeInput [K, 3D], symIdx [K],
    scatterIdx [K]) -- the reference's torch.cat([ctx_a_all, ctx_b_all, ctx_a_all*ctx_b_all], -1), symIdx_all and
    scatterIdx_all (ModelTransformer.py:501-532, :578-582).  K = offsets[-1] if not given (one host sync)."""
    assert ctxBatch.dim() == 4
    N, SYM, T, D = ctxBatch.shape
    _lib.require_gpu(ctxBatch, "ctxBatch")
    if K is None:
        K = int(offsets[-1])
    x = ctxBatch.float()
    if x.stride(-1) != 1 or not x.is_contiguous():
        x = x.contiguous()
    out, sym, sc = _IntervalFeatures.apply(x.view(N * SYM, T, D), pairs, offsets, int(K), SYM)
    return out, sym, sc


def fetchIntervalFeaturesBatch(ctxBatch: torch.Tensor, intervalsBatch: Sequence[Sequence[Sequence[Tuple[int, int]]]]):
    """Same arguments and results as the reference method (ModelTransformer.py:501-532): ctxBatch [N, SYM, T, D],
    intervalsBatch = per segment, per symbol, a list of (begin, end).  Returns (ctx_a_all, ctx_b_all, symIdx_all,
    scatterIdx_all); ctx_a_all / ctx_b_all are views of one [K, 3D] buffer whose last third already holds their product."""
    N, SYM, T, D = ctxBatch.shape
    assert len(intervalsBatch) == N
    flat: List[Sequence[Tuple[int, int]]] = [sym for seg in intervalsBatch for sym in seg]
    assert len(flat) == N * SYM
    pairs, offsets = _nsci.pack_intervals(flat, T, N * SYM, ctxBatch.device)
    K = getattr(pairs, "_semicrf_K", pairs.shape[0])
    if K == 0:
        raise RuntimeError("fetchIntervalFeaturesBatch: no intervals (the reference fails in torch.cat of an empty list)")
    out, sym, sc = attribute_input_packed(ctxBatch, pairs, offsets, K)
    return out[:, :D], out[:, D:2 * D], sym, sc


# ----------------------------------------------------------------------------------------------------------------------
# the attribute-head training loss (TransKun.log_prob, ModelTransformer.py:284-330)
# ----------------------------------------------------------------------------------------------------------------------
def _f32c(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _f32c8(t: torch.Tensor) -> torch.Tensor:
    """_f32c for logitsVelocity: the kernels read a float2 per lane, so the C ABI wants an 8-byte aligned base (include/semicrf_hip.h).
    A contiguous view that starts 4 bytes off (buf[1:1 + K * 128].view(K, 128)) is copied into a fresh tensor; aligned inputs are not."""
    t = _f32c(t)
    return t if t.data_ptr() % 8 == 0 else t.clone(memory_format=torch.contiguous_format)


class _AttributeLogProb(torch.autograd.Function):
    """out [C] = base + the per-chain sums of (lpVel + lpOF) + lpPres over the chain's rows (semicrf_attribute_loss_fwd / _bwd;
    the CPU dispatch key runs the same formulas on the host).  Once differentiable, w.r.t. logitsVelocity, ofLogits and base."""

    @staticmethod
    def forward(ctx, logitsVelocity, ofLogits, base, velocity, ofRefined, ofPresence, offsets):
        K, C = logitsVelocity.shape[0], offsets.shape[0] - 1
        dev = logitsVelocity.device
        lv, of = _f32c8(logitsVelocity), _f32c(ofLogits)
        b = None if base is None else _f32c(base).reshape(C)
        ctx.in_dtypes = (logitsVelocity.dtype, ofLogits.dtype, None if base is None else base.dtype)
        ctx.base_shape = None if base is None else base.shape
        ctx.K, ctx.C = K, C
        if K == 0:                                       # ModelTransformer.py:273: the whole block is skipped
            return b.clone() if b is not None else torch.zeros(C, dtype=torch.float32, device=dev)
        rows = torch.empty(K, dtype=torch.float32, device=dev)
        out = torch.empty(C, dtype=torch.float32, device=dev)
        _lib.ops().attribute_loss_fwd(lv, of, velocity, ofRefined, ofPresence, K, offsets, C, b if b is not None else out, b is not None,
                                      rows, out)
        ctx.save_for_backward(lv, of, velocity, ofRefined, ofPresence, offsets)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        K, C = ctx.K, ctx.C
        dt_lv, dt_of, dt_base = ctx.in_dtypes
        need = ctx.needs_input_grad
        dbase = grad_output.reshape(ctx.base_shape).to(dt_base) if need[2] else None
        if K == 0:
            dev = grad_output.device
            return (torch.zeros(0, 128, dtype=dt_lv, device=dev) if need[0] else None,
                    torch.zeros(0, 4, dtype=dt_of, device=dev) if need[1] else None, dbase, None, None, None, None)
        lv, of, velocity, ofRefined, ofPresence, offsets = ctx.saved_tensors
        g, gstride = _nsci._gout_strided(grad_output, C)
        dlv, dof = torch.empty_like(lv), torch.empty_like(of)
        _lib.ops().attribute_loss_bwd(g, gstride, lv, of, velocity, ofRefined, ofPresence, K, offsets, C, dlv, dof)
        return dlv.to(dt_lv) if need[0] else None, dof.to(dt_of) if need[1] else None, dbase, None, None, None, None


def attribute_log_prob(logitsVelocity: torch.Tensor, ofLogits: torch.Tensor, velocity: torch.Tensor, ofRefined: torch.Tensor,
                       ofPresence: torch.Tensor, offsets: torch.Tensor, base: torch.Tensor = None) -> torch.Tensor:
    """The attribute-head part of TransKun.log_prob (ModelTransformer.py:284-330) on the heads' RAW outputs, as one node: per chain c
    (rows offsets[c] .. offsets[c+1] of the K target intervals, chain order)

        out[c] = base[c] + sum_rows  log_softmax(logitsVelocity)[v]
                                   + ContinuousBernoulli(logits=ofLogits[:, :2]).log_prob(ofRefined * 0.99 + 0.5).sum(-1)
                                   + Bernoulli(logits=ofLogits[:, 2:]).log_prob(ofPresence).sum(-1)

    logitsVelocity [K, 128]; ofLogits [K, 4], the onset/offset head's output before .chunk(2, -1); velocity [K] integers 0..127;
    ofRefined [K, 2] in [-0.5, 0.5] (NOT shifted: the shift of :304 happens inside, in fp32); ofPresence [K, 2] in {0, 1}; offsets int32
    [C+1]; base [C] (any shape with C elements; the CRF's logProb) or None.  Returns fp32 [C].  Gradients flow to logitsVelocity,
    ofLogits and base (once differentiable).  All tensors on one device, a GPU (HIP kernels) or the CPU (host kernels).

    The ContinuousBernoulli normaliser follows torch's fp32 definition, clamp at eps = 2^-23 included, but is evaluated from the
    logit without torch's cancellation.  The sum has a fixed order ((vel + of) + presence per row, rows ascending, base last) and
    uses no atomics: results are bit-identical between runs and a chain's value does not depend on the rest of the batch.
    Nothing here synchronises with the host; velocities outside 0..127 give NaN (pack_attribute_targets checks them on the host).
    A logitsVelocity whose data pointer is off 8 bytes (a view that starts at an odd element) is copied first: the C ABI's rule."""
    K = logitsVelocity.shape[0]
    C = offsets.shape[0] - 1
    assert logitsVelocity.shape == (K, 128) and ofLogits.shape == (K, 4), "logitsVelocity [K, 128] and ofLogits [K, 4] expected"
    assert velocity.shape == (K,) and ofRefined.shape == (K, 2) and ofPresence.shape == (K, 2), "targets: velocity [K], ofRefined [K, 2], ofPresence [K, 2]"
    assert offsets.dtype == torch.int32 and offsets.dim() == 1 and C >= 1, "offsets: int32 [C+1]"
    assert base is None or base.numel() == C, "base must hold one value per chain"
    _lib.require_device(logitsVelocity, "logitsVelocity")
    vel = velocity if velocity.dtype == torch.int32 else velocity.to(torch.int32)
    return _AttributeLogProb.apply(logitsVelocity, ofLogits, base, vel.contiguous(), _f32c(ofRefined), _f32c(ofPresence), offsets.contiguous())


def attribute_log_prob_torch(logitsVelocity, ofLogits, velocity, ofRefined, ofPresence, offsets, base=None) -> torch.Tensor:
    """attribute_log_prob's arguments and result by the reference's OWN formulation (ModelTransformer.py:291-328), torch call for
    torch call: what a caller had to run before the fused op existed.  For comparisons (tools/bench_attr_loss.py, the tests); the
    package itself never takes this route on its own."""
    C = offsets.shape[0] - 1
    logProb = torch.zeros(C, dtype=logitsVelocity.dtype, device=logitsVelocity.device) if base is None else base.reshape(C)
    if logitsVelocity.shape[0] == 0:                                                                     # :273
        return logProb
    counts = (offsets[1:] - offsets[:-1]).long()
    scatterIdx = torch.repeat_interleave(torch.arange(C, device=offsets.device), counts, output_size=logitsVelocity.shape[0])
    logits = torch.nn.functional.log_softmax(logitsVelocity, dim=-1)                                     # :291
    logProbVelocity = torch.gather(logits, dim=-1, index=velocity.long().unsqueeze(-1)).squeeze(-1)      # :295
    refined = ofRefined.to(logitsVelocity.dtype) * 0.99 + 0.5                                            # :304
    ofValue, ofPres = ofLogits.chunk(2, dim=-1)                                                          # :306
    logProbOF = torch.distributions.ContinuousBernoulli(logits=ofValue).log_prob(refined).sum(-1)        # :311-313
    logProbOFPresence = torch.distributions.Bernoulli(logits=ofPres).log_prob(ofPresence.to(logitsVelocity.dtype)).sum(-1)   # :315-317
    return logProb.scatter_add(-1, scatterIdx, logProbVelocity + logProbOF + logProbOFPresence)         # :328


# ----------------------------------------------------------------------------------------------------------------------
# the attribute-head readout of transcription (TransKun.transcribeFrames, ModelTransformer.py:590-651)
# ----------------------------------------------------------------------------------------------------------------------
VELOCITY_CRITERIA = {"hamming": _lib.VEL_HAMMING, "mse": _lib.VEL_MSE, "match": _lib.VEL_MATCH, "mae": _lib.VEL_MAE}


def attribute_decode(logitsVelocity: torch.Tensor, ofLogits: torch.Tensor, criterion: str = "hamming"):
    """What transcribeFrames reads out of the two heads' RAW outputs (ModelTransformer.py:590-651), as one op (one launch on a GPU):
    logitsVelocity [K, 128] and ofLogits [K, 4] (the onset/offset head's output before .chunk(2, -1)) -> (velocity, ofValue, ofPresence).

    velocity [K], with p = softmax(logitsVelocity): "hamming" the mode (int64; the smallest index of the largest logit), "mse" the
    mean sum_w p[w] w (float32), "match" the smallest v with the largest sum of p[w] over |w - v| <= 12 (int64), "mae" the median,
    the smallest v with p[0] + ... + p[v] > 0.5 (int64).  A row whose softmax is not finite gives class 0 / mean NaN.
    ofValue float32 [K, 2] = clamp((ContinuousBernoulli(logits).mean - 0.5) / 0.99, -0.5, 0.5) with torch's fp32 probability clamp,
    evaluated from the logit (below 1e-6 of the definition where the torch calls in fp32 lose 3e-3); ofPresence bool [K, 2] = logit > 0.

    Both tensors on one device, a GPU (csrc/attr_decode.hip) or the CPU (the host kernel: the same formulas in double).  Row-wise,
    without atomics: a row's result depends on that row alone and is bit-identical from run to run; nothing synchronises with the
    host.  An unknown criterion raises with the reference's message.  A logitsVelocity whose data pointer is off 8 bytes is copied
    first (the C ABI's rule)."""
    if criterion not in VELOCITY_CRITERIA:
        raise Exception("Unrecognized criterion: {}".format(criterion))
    K = logitsVelocity.shape[0]
    assert logitsVelocity.shape == (K, 128) and ofLogits.shape == (K, 4), "logitsVelocity [K, 128] and ofLogits [K, 4] expected"
    _lib.require_device(logitsVelocity, "logitsVelocity")
    dev = logitsVelocity.device
    mse = criterion == "mse"
    cls = torch.empty(0 if mse else K, dtype=torch.int64, device=dev)
    mean = torch.empty(K if mse else 0, dtype=torch.float32, device=dev)
    ofValue = torch.empty(K, 2, dtype=torch.float32, device=dev)
    ofPresence = torch.empty(K, 2, dtype=torch.uint8, device=dev)
    if K > 0:
        _lib.ops().attribute_decode(_f32c8(logitsVelocity), _f32c(ofLogits), K, VELOCITY_CRITERIA[criterion], cls, mean, ofValue, ofPresence)
    return (mean if mse else cls), ofValue, ofPresence.view(torch.bool)


def velocity_torch(logitsVelocity: torch.Tensor, criterion: str) -> torch.Tensor:
    """The velocity criteria of ModelTransformer.py:590-632 as the reference's torch calls."""
    pVelocity = torch.nn.functional.softmax(logitsVelocity, dim=-1)                  # :590-637
    dev = pVelocity.device
    if criterion == "hamming":
        return torch.argmax(pVelocity, dim=-1)
    if criterion == "mse":
        return (pVelocity * torch.arange(128, device=dev)).sum(-1)
    if criterion == "match":
        w = torch.arange(128, device=dev)
        utility = ((w.unsqueeze(1) - w.unsqueeze(0)).abs() < 0.1 * 128).float()
        return torch.argmax(pVelocity @ utility, dim=-1)
    if criterion == "mae":
        tmp = (pVelocity.cumsum(-1) - 0.5) > 0
        return torch.argmax(tmp * torch.arange(128, 0., -1, device=dev), dim=-1)
    raise Exception("Unrecognized criterion: {}".format(criterion))


def attribute_decode_torch(logitsVelocity: torch.Tensor, ofLogits: torch.Tensor, criterion: str = "hamming"):
    """attribute_decode's arguments and result by the reference's OWN formulation (ModelTransformer.py:590-651), torch call for torch
    call, in the dtype of its inputs: SegmentTranscriber.decode_step's default route (attributeDecode = "torch"), and the comparison
    route of the tests and tools/bench_attr_decode.py."""
    velocity = velocity_torch(logitsVelocity, criterion)
    ofValue, ofPresence = ofLogits.chunk(2, dim=-1)                                  # :646-655
    ofDist = torch.distributions.ContinuousBernoulli(logits=ofValue, validate_args=False)   # (the argument check is a host sync)
    ofValue = torch.clamp((ofDist.mean - 0.5) / 0.99, -0.5, 0.5).float().contiguous()
    ofPresence = (ofPresence > 0).contiguous()
    return velocity, ofValue, ofPresence


# ----------------------------------------------------------------------------------------------------------------------
# the two attribute heads themselves (TransKun.transcribeFrames, ModelTransformer.py:578-590, :638), inference only
# ----------------------------------------------------------------------------------------------------------------------
HEADS_ROW_TILE = _lib.HEADS_ROW_TILE            # intervals per workgroup of the kernel (SEMICRF_HEADS_ROW_TILE)
_HEADS_PACKED = weakref.WeakKeyDictionary()     # velocityPredictor -> (key, packed weights)


def _head_layers(head: torch.nn.Module, name: str):
    """(first Linear, second Linear, p) of a head built as the reference builds it (ModelTransformer.py:112-128): Linear, GELU (the exact
    erf form), Dropout, Linear.  p: the probability of the head's Dropout if it is in training mode (it must follow the GELU), else 0."""
    mods = list(head.children()) if isinstance(head, torch.nn.Sequential) else []
    if len(mods) < 3 or not isinstance(mods[0], torch.nn.Linear) or not isinstance(mods[-1], torch.nn.Linear):
        raise TypeError(f"{name}: expected nn.Sequential(Linear, GELU, [Dropout,] Linear)")
    ngelu, p = 0, 0.0
    for m in mods[1:-1]:
        if isinstance(m, torch.nn.GELU) and getattr(m, "approximate", "none") == "none":
            ngelu += 1
        elif isinstance(m, torch.nn.Dropout):
            if m.training and m.p > 0:
                if p > 0 or ngelu != 1:
                    raise TypeError(f"{name}: one Dropout, between the GELU and the second Linear, is supported in training mode")
                p = float(m.p)
        else:
            raise TypeError(f"{name}: unsupported layer {type(m).__name__} between the two Linear layers")
    if ngelu != 1 or mods[0].out_features != mods[-1].in_features:
        raise TypeError(f"{name}: expected exactly one exact-erf GELU between two matching Linear layers")
    return mods[0], mods[-1], p


def _head_linears(head: torch.nn.Module, name: str):
    """(first Linear, second Linear) of a head in eval mode.  A training-mode Dropout with p > 0 raises ValueError: attribute_heads
    evaluates the heads in eval mode only (attribute_heads_train takes both modes)."""
    l1, l2, p = _head_layers(head, name)
    if p > 0:
        raise ValueError(f"{name} is in training mode with dropout p = {p}: attribute_heads is the eval-mode forward only "
                         "(call .eval(), or use attribute_heads_train / attribute_heads_torch)")
    return l1, l2


def _packed_heads(velocityPredictor, refinedOFPredictor, train: bool = False):
    """The two heads' parameters in the layout of semicrf_attribute_heads (include/semicrf_hip.h), fp32: W1 [3D, Hv + Ho], b1 [Hv + Ho],
    W2 = W2v^T [Hv, Nv] followed by W2o^T [Ho, No] (flat), b2 [Nv + No].  Packed by torch calls once and kept until a parameter's
    `_version` (an optimizer step, load_state_dict: both write in place) or storage changes.  train: a head may be in training mode
    (attribute_heads_train; the dict is the same)."""
    v1, v2 = (_head_layers if train else _head_linears)(velocityPredictor, "velocityPredictor")[:2]
    o1, o2 = (_head_layers if train else _head_linears)(refinedOFPredictor, "refinedOFPredictor")[:2]
    if v1.in_features != o1.in_features:
        raise ValueError("the two heads must take the same input")
    lins = (v1, v2, o1, o2)
    params = [p for l in lins for p in (l.weight, l.bias) if p is not None]
    key = (id(refinedOFPredictor),) + tuple((p._version, p.data_ptr(), p.dtype, p.device) for p in params)
    hit = _HEADS_PACKED.get(velocityPredictor)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        def bias(l):
            return l.bias.float() if l.bias is not None else torch.zeros(l.out_features, dtype=torch.float32, device=l.weight.device)
        W1 = torch.cat([v1.weight.float().t(), o1.weight.float().t()], dim=1).contiguous()
        b1 = torch.cat([bias(v1), bias(o1)]).contiguous()
        W2 = torch.cat([v2.weight.float().t().reshape(-1), o2.weight.float().t().reshape(-1)]).contiguous()
        b2 = torch.cat([bias(v2), bias(o2)]).contiguous()
    packed = dict(W1=W1, b1=b1, W2=W2, b2=b2, Hv=v1.out_features, Ho=o1.out_features, Nv=v2.out_features, No=o2.out_features,
                  nIn=v1.in_features)
    _HEADS_PACKED[velocityPredictor] = (key, packed)
    return packed


def attribute_heads(ctxBatch: torch.Tensor, pairs: torch.Tensor, offsets: torch.Tensor, velocityPredictor, refinedOFPredictor, K: int = None):
    """The gather and both attribute heads as ONE op (semicrf_attribute_heads; two launches on a GPU): attribute_input_packed's
    arguments plus the two head modules (nn.Sequential(Linear, GELU, Dropout, Linear), as SegmentTranscriber holds them) ->
    (logitsVelocity [K, Nv], ofLogits [K, No], symIdx [K], scatterIdx [K]), what

        x, symIdx, scatterIdx = attribute_input_packed(ctxBatch, pairs, offsets, K)
        velocityPredictor(x), refinedOFPredictor(x)

    gives in eval mode (attribute_heads_torch), without the [K, 3D] input ever reaching memory.  Exact fp32 on the matrix pipe; every
    output element is one fixed chain of operations (include/semicrf_hip.h), so a row's outputs are bit-identical whatever K is,
    wherever the row sits, whatever the other rows hold and from run to run.  Rows past offsets[-1] (the k_cap route of decode_step)
    are legal: any pair of frames inside [0, T-1] is.  ctxBatch [N, SYM, T, D] on a GPU (HIP kernels) or the CPU (the host mirror:
    the same order of operations); any float dtype (converted to fp32 first); a view with a row stride above D is read in place.
    The output sizes Nv, No and the hidden sizes come from the modules.  K = offsets[-1] if not given (one host sync); otherwise
    nothing waits for the host, and the call can be captured in a HIP graph.

    Forward only: RuntimeError if grad mode is on and ctxBatch or a parameter requires grad.  ValueError if a head is in training
    mode with a dropout probability above 0.  The packed weights are cached (see _packed_heads)."""
    assert ctxBatch.dim() == 4
    N, SYM, T, D = ctxBatch.shape
    _lib.require_device(ctxBatch, "ctxBatch")
    w = _packed_heads(velocityPredictor, refinedOFPredictor)
    if torch.is_grad_enabled() and (ctxBatch.requires_grad or any(p.requires_grad for m in (velocityPredictor, refinedOFPredictor)
                                                                  for p in m.parameters())):
        raise RuntimeError("attribute_heads is forward-only: call it under torch.no_grad() (training keeps the torch modules, "
                           "attribute_heads_torch)")
    if w["nIn"] != 3 * D:
        raise ValueError(f"the heads take {w['nIn']} inputs, ctxBatch gives 3 * {D}")
    dev = ctxBatch.device
    if w["W1"].device != dev:
        raise RuntimeError(f"the heads' parameters are on {w['W1'].device}, ctxBatch on {dev}")
    if K is None:
        K = int(offsets[-1])
    K = int(K)
    assert pairs.dtype == torch.int32 and offsets.dtype == torch.int32 and offsets.numel() == N * SYM + 1
    x = ctxBatch.detach()
    if x.dtype != torch.float32:
        x = x.float()
    ldc = x.stride(2)
    if not ((D == 1 or x.stride(3) == 1) and ldc >= D and x.stride(1) == T * ldc and x.stride(0) == SYM * T * ldc):
        x = x.contiguous()
        ldc = D
    C = N * SYM
    x3 = x.as_strided((C, T, D), (T * ldc, ldc, 1), x.storage_offset())
    Hv, Ho, Nv, No = w["Hv"], w["Ho"], w["Nv"], w["No"]
    logitsVelocity = torch.empty(K, Nv, dtype=torch.float32, device=dev)
    ofLogits = torch.empty(K, No, dtype=torch.float32, device=dev)
    sym = torch.empty(K, dtype=torch.int64, device=dev)
    sc = torch.empty(K, dtype=torch.int64, device=dev)
    if K > 0:
        if dev.type == "cpu":
            ws = torch.empty(0, dtype=torch.uint8)
        else:
            ws = torch.empty(int(_lib.load().semicrf_attribute_heads_workspace_bytes(K, Hv, Ho, Nv, No)), dtype=torch.uint8, device=dev)
        _lib.ops().attribute_heads(x3, C, T, D, ldc, pairs.contiguous(), K, offsets.contiguous(), SYM, w["W1"], w["b1"], w["W2"], w["b2"],
                                   Hv, Ho, Nv, No, logitsVelocity, ofLogits, sym, sc, ws)
    return logitsVelocity, ofLogits, sym, sc


# ----------------------------------------------------------------------------------------------------------------------
# the heads in training: dropout in the forward, and the backward (semicrf_attribute_heads_train_fwd / _bwd)
# ----------------------------------------------------------------------------------------------------------------------
HEADS_BWD_ROW_CHUNK = _lib.HEADS_BWD_ROW_CHUNK  # rows per partial plane of the backward's sums over rows (SEMICRF_HEADS_BWD_ROW_CHUNK)


def _seed_arg(seed) -> int:
    """A seed (any int; its low 64 bits count) as the signed 64-bit value the torch ops carry."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed - (1 << 64) if seed >= (1 << 63) else seed


def attribute_heads_dropout_mask(seed: int, K: int, Hv: int, Ho: int, pv: float, po: float, device="cpu") -> torch.Tensor:
    """The dropout mask of attribute_heads_train as a tensor: bool [K, Hv + Ho], True = kept; column j < Hv belongs to the velocity head
    (probability pv), column Hv + j to the onset/offset head (po); a head with p = 0 keeps everything.  A stateless function of
    (seed, row, column) (Philox-4x32-10, include/semicrf_hip.h): the first rows of a larger K are the same rows.  On a GPU by
    semicrf_attribute_heads_dropout_mask, on the CPU by the host mirror: the same bits."""
    dev = torch.device(device)
    mask = torch.empty(int(K), int(Hv) + int(Ho), dtype=torch.uint8, device=dev)
    _lib.ops().attribute_heads_dropout_mask(mask, _seed_arg(seed), int(K), int(Hv), int(Ho), float(pv), float(po))
    return mask.view(torch.bool)


class _AttributeHeadsTrain(torch.autograd.Function):
    """The op behind attribute_heads_train.  Inputs that take a gradient: ctxBatch and the eight parameters (a missing bias is None)."""

    @staticmethod
    def forward(ctx, ctxBatch, pairs, offsets, K, seed, pv, po, w, v1w, v1b, v2w, v2b, o1w, o1b, o2w, o2b):
        N, SYM, T, D = ctxBatch.shape
        dev = ctxBatch.device
        x = ctxBatch.detach()
        if x.dtype != torch.float32:
            x = x.float()
        ldc = x.stride(2)
        if not ((D == 1 or x.stride(3) == 1) and ldc >= D and x.stride(1) == T * ldc and x.stride(0) == SYM * T * ldc):
            x = x.contiguous()
            ldc = D
        C = N * SYM
        x3 = x.as_strided((C, T, D), (T * ldc, ldc, 1), x.storage_offset())
        Hv, Ho, Nv, No = w["Hv"], w["Ho"], w["Nv"], w["No"]
        logitsVelocity = torch.empty(K, Nv, dtype=torch.float32, device=dev)
        ofLogits = torch.empty(K, No, dtype=torch.float32, device=dev)
        z = torch.empty(K, Hv + Ho, dtype=torch.float32, device=dev)
        sym = torch.empty(K, dtype=torch.int64, device=dev)
        sc = torch.empty(K, dtype=torch.int64, device=dev)
        pairs, offsets = pairs.contiguous(), offsets.contiguous()
        if K > 0:
            if dev.type == "cpu":
                ws = torch.empty(0, dtype=torch.uint8)
            else:
                ws = torch.empty(int(_lib.load().semicrf_attribute_heads_train_fwd_workspace_bytes(K, Hv, Ho, Nv, No)), dtype=torch.uint8,
                                 device=dev)
            _lib.ops().attribute_heads_train_fwd(x3, C, T, D, ldc, pairs, K, offsets, SYM, w["W1"], w["b1"], w["W2"], w["b2"], Hv, Ho, Nv, No,
                                                 seed, pv, po, logitsVelocity, ofLogits, z, sym, sc, ws)
        ctx.save_for_backward(x3, pairs, offsets, z, w["W1"], w["W2"])
        ctx.geom = (C, T, D, ldc, K, Hv, Ho, Nv, No, seed, pv, po, tuple(ctxBatch.shape), ctxBatch.dtype)
        ctx.has_bias = tuple(b is not None for b in (v1b, v2b, o1b, o2b))
        ctx.mark_non_differentiable(sym, sc)
        return logitsVelocity, ofLogits, sym, sc

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dLv, dOf, _dsym, _dsc):
        x3, pairs, offsets, z, W1, W2 = ctx.saved_tensors
        C, T, D, ldc, K, Hv, Ho, Nv, No, seed, pv, po, shape, dtype = ctx.geom
        dev = x3.device
        H = Hv + Ho
        dctx = torch.empty(C, T, D, dtype=torch.float32, device=dev)
        # all parameter gradients in one buffer, in the layout of a partial plane: dW1 [3D, H] | db1 [H] | dW2 (as W2) | db2 [Nv + No]
        n1, n2 = 3 * D * H, Hv * Nv + Ho * No
        flat = torch.empty(n1 + H + n2 + Nv + No, dtype=torch.float32, device=dev)
        dW1, db1, dW2, db2 = flat[:n1], flat[n1:n1 + H], flat[n1 + H:n1 + H + n2], flat[n1 + H + n2:]
        if K > 0:
            dLv = torch.zeros(K, Nv, dtype=torch.float32, device=dev) if dLv is None else dLv.float().contiguous()
            dOf = torch.zeros(K, No, dtype=torch.float32, device=dev) if dOf is None else dOf.float().contiguous()
            if dev.type == "cpu":
                ws = torch.empty(0, dtype=torch.uint8)
            else:
                ws = torch.empty(int(_lib.load().semicrf_attribute_heads_bwd_workspace_bytes(K, D, Hv, Ho, Nv, No)), dtype=torch.uint8,
                                 device=dev)
            _lib.ops().attribute_heads_bwd(dLv, dOf, z, x3, C, T, D, ldc, pairs, K, offsets, W1, W2, Hv, Ho, Nv, No, seed, pv, po, dctx, dW1, db1,
                                           dW2, db2, ws)
        else:
            dctx.zero_(); flat.zero_()
        dW1 = dW1.view(3 * D, H)
        gv2, go2 = dW2[:Hv * Nv].view(Hv, Nv), dW2[Hv * Nv:].view(Ho, No)
        # the packed gradients go back to the parameters as transposed slices (nn.Linear keeps [out, in])
        grads = [dW1[:, :Hv].t(), db1[:Hv], gv2.t(), db2[:Nv], dW1[:, Hv:].t(), db1[Hv:], go2.t(), db2[Nv:]]
        for at, has in zip((1, 3, 5, 7), ctx.has_bias):
            if not has:
                grads[at] = None
        need = ctx.needs_input_grad
        gctx = dctx.view(shape).to(dtype) if need[0] else None
        return (gctx, None, None, None, None, None, None, None) + tuple(g if need[8 + i] else None for i, g in enumerate(grads))


def attribute_heads_train(ctxBatch: torch.Tensor, pairs: torch.Tensor, offsets: torch.Tensor, velocityPredictor, refinedOFPredictor,
                          K: int = None, seed: int = None):
    """attribute_heads for TRAINING: the same arguments and the same four results, differentiable (once; a second differentiation
    raises) w.r.t. ctxBatch and the weight and bias of the four Linear layers, with each head's Dropout applied when the head is in
    training mode (its own p; the two may differ).  The forward is attribute_heads' kernel in its training mode
    (semicrf_attribute_heads_train_fwd: it also saves z = W1 x + b1, [K, Hv + Ho] fp32); the backward is semicrf_attribute_heads_bwd
    (csrc/attr_heads_bwd.hip): exact fp32 on the matrix pipe for dW1 and dx, the [K, 3D] input gathered again instead of stored, no
    atomics -- every gradient is bit-identical from run to run.  With both heads in eval mode (or p = 0) the outputs are
    bit-identical to attribute_heads'.

    Dropout: element (row i, packed hidden column j) is kept iff attribute_heads_dropout_mask(seed, ...)[i, j]: a stateless function
    of (seed, i, j), so a row's outputs do not depend on K or on the other rows in training either.  seed = None draws one value per
    call from torch's CPU default generator (torch.manual_seed makes runs reproducible; nothing waits for the device); an explicit
    seed makes the call reproducible.  The seed is a HOST value: a call captured in a HIP graph replays one and the same mask.

    The parameters must be fp32 (TypeError otherwise); ctxBatch may be any float dtype and a view with a row stride above D, its
    gradient comes back in its dtype and shape.  A Linear without a bias gets no bias gradient.  CPU tensors run the host mirror."""
    assert ctxBatch.dim() == 4
    N, SYM, T, D = ctxBatch.shape
    _lib.require_device(ctxBatch, "ctxBatch")
    v1, v2, pv = _head_layers(velocityPredictor, "velocityPredictor")
    o1, o2, po = _head_layers(refinedOFPredictor, "refinedOFPredictor")
    params = (v1.weight, v1.bias, v2.weight, v2.bias, o1.weight, o1.bias, o2.weight, o2.bias)
    for p in params:
        if p is not None and p.dtype != torch.float32:
            raise TypeError(f"attribute_heads_train: the heads' parameters must be float32, not {p.dtype}")
    if not (pv < 1.0 and po < 1.0):
        raise ValueError("attribute_heads_train: a dropout probability of 1 leaves nothing to train")
    w = _packed_heads(velocityPredictor, refinedOFPredictor, train=True)
    if w["nIn"] != 3 * D:
        raise ValueError(f"the heads take {w['nIn']} inputs, ctxBatch gives 3 * {D}")
    if w["W1"].device != ctxBatch.device:
        raise RuntimeError(f"the heads' parameters are on {w['W1'].device}, ctxBatch on {ctxBatch.device}")
    if K is None:
        K = int(offsets[-1])
    K = int(K)
    assert pairs.dtype == torch.int32 and offsets.dtype == torch.int32 and offsets.numel() == N * SYM + 1
    if seed is None:
        if pv > 0 or po > 0:
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()       # the CPU default generator: no device sync
            seed = (hi << 32) | lo
        else:
            seed = 0
    return _AttributeHeadsTrain.apply(ctxBatch, pairs, offsets, K, _seed_arg(seed), float(pv), float(po), w, *params)


def attribute_heads_torch(ctxBatch: torch.Tensor, pairs: torch.Tensor, offsets: torch.Tensor, velocityPredictor, refinedOFPredictor,
                          K: int = None):
    """attribute_heads' arguments and result by the gather kernel and the two torch modules (ModelTransformer.py:578-590, :638): the
    [K, 3D] input in memory, six stock launches and two BLAS calls.  SegmentTranscriber's default route (attributeHeads = "torch"),
    the route of training, and the comparison route of the tests and tools/bench_attr_heads.py."""
    attributeInput, sym, sc = attribute_input_packed(ctxBatch, pairs, offsets, K)
    return velocityPredictor(attributeInput), refinedOFPredictor(attributeInput), sym, sc


def _flatten_target(x):
    """The nested per-segment / per-symbol lists of prepareIntervals (data["velocity"] etc.), a flat sequence or a tensor -> a CPU
    tensor or a flat list (the forms SegmentTranscriber._target_tensor takes)."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    x = list(x)
    if x and isinstance(x[0], (list, tuple)) and (len(x[0]) == 0 or isinstance(x[0][0], (list, tuple))):
        x = [v for seg in x for sym in seg for v in sym]                                 # sum(sum(..., []), []), :251-253, :286-288
    return x


def pack_attribute_targets(velocityBatch, ofRefinedGTBatch, ofPresenceGTBatch, K: int, device):
    """The three targets of the attribute heads as device tensors for attribute_log_prob: (velocity int32 [K], ofRefined fp32 [K, 2],
    ofPresence fp32 [K, 2]).  Each argument: nested per segment and symbol as prepareIntervals yields it, flat in chain order, or a
    tensor.  Checked on the host (ValueError): velocities are integers in 0..127 and every target has K entries.  Everything
    travels in ONE pinned, non-blocking copy (the reference uploads three tensors, :293-298)."""
    K = int(K)
    vel = torch.as_tensor(_flatten_target(velocityBatch))
    if vel.numel() != K:
        raise ValueError(f"velocityBatch: {vel.numel()} values for {K} target intervals")
    velf = vel.to(torch.float64).reshape(K)
    if K and (bool((velf != velf.round()).any()) or float(velf.min()) < 0 or float(velf.max()) > 127):
        raise ValueError("velocityBatch: velocities must be integers in 0..127")
    refined = torch.as_tensor(_flatten_target(ofRefinedGTBatch), dtype=torch.float32)
    presence = torch.as_tensor(_flatten_target(ofPresenceGTBatch), dtype=torch.float32)
    if refined.numel() != 2 * K:
        raise ValueError(f"ofRefinedGTBatch: {refined.numel()} values for {K} target intervals (2 each)")
    if presence.numel() != 2 * K:
        raise ValueError(f"ofPresenceGTBatch: {presence.numel()} values for {K} target intervals (2 each)")
    dev = torch.device(device)
    # one buffer of 5 K 32-bit words: [velocity as int32 bits | refined | presence]
    host = torch.empty(5 * K, dtype=torch.float32, pin_memory=dev.type == "cuda")
    host[:K].view(torch.int32).copy_(velf)
    host[K:3 * K].copy_(refined.reshape(2 * K))
    host[3 * K:].copy_(presence.reshape(2 * K))
    d = host.to(dev, non_blocking=True)
    return d[:K].view(torch.int32), d[K:3 * K].view(K, 2), d[3 * K:].view(K, 2)
