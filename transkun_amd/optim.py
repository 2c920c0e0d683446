"""The optimizer step of the reference's training loop (train.py:239-246) on flat buffers, without a host synchronisation.

    curClipValue = gradNormHist.getQuantile(0.8)                     # train.py:239, a host deque of 10000 norms (TrainUtil.py:12-25)
    totalNorm = clip_grad_norm_(model.parameters(), curClipValue)    # train.py:242
    gradNormHist.step(totalNorm.item())                              # train.py:244, the device waits for the host here
    optimizer.step()                                                 # train.py:246, torch_optimizer.AdaBelief: a Python loop over 182
                                                                     # parameters, about a dozen small launches each

becomes `FusedAdaBelief.step()`: three launches (csrc/optim.hip) -- the squared norm of the flat gradient in double, one workgroup
that takes the clip value from a norm history kept ON THE DEVICE, forms the clip coefficient and appends the norm, and one stream
over the flat parameter, gradient and moment buffers that applies the coefficient and AdaBelief (csrc/optim_math.h).  CPU tensors
take the shim's host kernels, which share that header and give the same bits.

A non-finite gradient norm propagates exactly as in the reference: the clip coefficient becomes NaN and so do the parameters (and
the NaN stays in the history, so every later clip value is NaN too).  Nothing is skipped.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .dist import FlatGradBucket

__all__ = ["FusedAdaBelief", "GradNormHistory", "optimizer_groups", "adabelief_scalars"]


def _f32(x: float) -> float:
    """Round a host float64 to fp32 once (kept in a Python float: exact)."""
    return float(np.float32(x))


def adabelief_scalars(t: int, lr: float, weight_decay: float, betas, eps: float) -> dict:
    """The factors of one parameter group at step t (1 on the first step), computed in float64 and rounded to fp32 once each --
    what the kernels take by value (semicrf_adabelief_group).  With rho_t > 4 the step is rectified (`step` = rt*lr/bc1), otherwise
    it is the SGD-style `p -= lr*m` (`step` = lr): for b2 = 0.999 that is t = 1..4 (rho_4 = 3.99750, rho_5 = 4.99600), for
    b2 = 0.9 t = 1..4 as well (rho_4 = 3.73742, rho_5 = 4.58057)."""
    b1, b2 = float(betas[0]), float(betas[1])
    bc1 = 1.0 - b1 ** t
    bc2 = 1.0 - b2 ** t
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho_t = rho_inf - 2.0 * t * b2 ** t / (1.0 - b2 ** t)
    rect = rho_t > 4.0
    if rect:
        rt = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
        step = rt * lr / bc1
    else:
        step = lr
    return {"decay": _f32(1.0 - lr * weight_decay), "b1": _f32(b1), "omb1": _f32(1.0 - b1), "b2": _f32(b2), "omb2": _f32(1.0 - b2),
            "eps": _f32(eps), "sqrt_bc2": _f32(math.sqrt(bc2)), "step": _f32(step), "rectified": bool(rect), "rho_t": rho_t,
            "rho_inf": rho_inf}


_TABLE_KEYS = ("decay", "b1", "omb1", "b2", "omb2", "eps", "sqrt_bc2", "step")


class GradNormHistory:
    """MovingBuffer(initValue=40, maxLen=10000) of the reference (TrainUtil.py:12-25) as a ring buffer on the device: `ring`
    [capacity] fp32, `state` = (count, head) int32.  quantile / append enqueue one launch each and never wait for the device;
    values() is for tests and logging (it does wait)."""

    def __init__(self, capacity: int = 10000, init: Optional[float] = 40.0, device=None):
        capacity = int(capacity)
        if not 1 <= capacity <= _lib.HISTORY_MAX:
            raise ValueError(f"GradNormHistory: capacity must be in [1, {_lib.HISTORY_MAX}] (the ring is sorted in LDS)")
        self.capacity = capacity
        self.device = torch.device(device if device is not None else "cpu")
        _lib.require_device(torch.empty(0, device=self.device), "history")
        self.ring = torch.zeros(capacity, dtype=torch.float32, device=self.device)
        self.state = torch.zeros(2, dtype=torch.int32, device=self.device)
        if init is not None:
            self.ring[:1].fill_(float(init))
            self.state[:1].fill_(1)
        self._none = torch.empty(0, dtype=torch.float32, device=self.device)
        self._none64 = torch.empty(0, dtype=torch.float64, device=self.device)

    def _launch(self, partials, numel, norm, q, append, stats) -> None:
        _lib.ops().clip_from_history(partials if partials is not None else self._none64, partials is not None, int(numel),
                                     norm if norm is not None else self._none, norm is not None, float(q), self.ring, self.capacity,
                                     self.state, bool(append), stats)

    def quantile(self, q: float) -> torch.Tensor:
        """np.quantile(values, q) (linear interpolation, evaluated in float64) as a 0-dim fp32 device tensor."""
        if not 0.0 <= float(q) <= 1.0:
            raise ValueError("GradNormHistory.quantile: q must lie in [0, 1]")
        stats = torch.empty(3, dtype=torch.float32, device=self.device)
        self._launch(None, 0, None, q, False, stats)
        return stats[1]

    def append(self, value) -> None:
        """Append a norm (a Python number or a one-element tensor); the oldest value leaves once the ring is full."""
        if isinstance(value, torch.Tensor):
            norm = value.detach().to(device=self.device, dtype=torch.float32).reshape(1).contiguous()
        else:
            norm = torch.full((1,), float(value), dtype=torch.float32, device=self.device)
        self._launch(None, 0, norm, -1.0, True, torch.empty(3, dtype=torch.float32, device=self.device))

    def values(self) -> torch.Tensor:
        """The content in insertion order (oldest first), on the host."""
        count, head = (int(x) for x in self.state.cpu())
        ring = self.ring.cpu()
        return ring[(head + torch.arange(count)) % self.capacity]

    def __len__(self) -> int:
        return int(self.state[0])

    def state_dict(self) -> dict:
        return {"capacity": self.capacity, "ring": self.ring.clone(), "state": self.state.clone()}

    def load_state_dict(self, sd: dict) -> None:
        if int(sd["capacity"]) != self.capacity:
            raise ValueError(f"GradNormHistory: the saved history holds {sd['capacity']} values, this one {self.capacity}")
        self.ring.copy_(sd["ring"])
        self.state.copy_(sd["state"])


def optimizer_groups(model: nn.Module, no_decay_types=(nn.GroupNorm, nn.LayerNorm), no_decay_modules: Iterable[nn.Module] = ()):
    """getOptimizerGroup of the reference (TrainUtil.py:82-112): [{"params": everything else}, {"params": no-decay, "weight_decay": 0}].
    The no-decay group holds every parameter of a module of one of `no_decay_types` (the reference adds its position embedding
    class: pass it here) or listed in `no_decay_modules`, and every parameter whose name contains "bias"; both groups keep
    model.parameters() order."""
    types = tuple(no_decay_types)
    listed = {id(m) for m in no_decay_modules}
    no_decay = set()
    for _, module in model.named_modules():
        if isinstance(module, types) or id(module) in listed:
            no_decay.update(id(p) for p in module.parameters())
        else:
            no_decay.update(id(p) for n, p in module.named_parameters() if "bias" in n)
    params = list(model.parameters())
    return [{"params": [p for p in params if id(p) not in no_decay]},
            {"params": [p for p in params if id(p) in no_decay], "weight_decay": 0.0}]


class FusedAdaBelief(torch.optim.Optimizer):
    """torch_optimizer.AdaBelief(weight_decouple=True, rectify=True, amsgrad=False) with clip_grad_norm_ at an adaptive clip value
    in front of it, as three launches on flat buffers (module doc-string; the update rule is csrc/optim_math.h).

    * Parameters live in ONE flat fp32 buffer, group after group (`flat`): every p.data is a view of it, checked by address before
      each step (a parameter found elsewhere is copied back in and rebound; `rebound` counts them).  The moments are flat buffers of
      the same layout; state[p] = {"step", "exp_avg", "exp_avg_var"} are views of them, so state_dict() is the stock one plus the
      norm history, and load_state_dict copies INTO the flat buffers.
    * `bucket`: a FlatGradBucket over the same parameters in the same order -- gradients and parameters share one element layout.
      Its padded tail is neither read by the norm nor written.
    * clip_quantile=q: the clip value of a step is the q-quantile of the norms BEFORE it (`history`, a GradNormHistory, starting
      from the single value 40); None: no norm, no clipping, one launch.
    * step() waits for the bucket's exchange if a step is open, never for the device.  Afterwards last_norm, last_clip and last_coef
      are 0-dim device tensors (None, None and 1 without clipping).  A non-finite norm makes coef and the parameters NaN, as in the
      reference; nothing is skipped.
    * param_groups[i]["lr"] (and weight_decay, betas, eps) are read at every step: torch's schedulers drive it unchanged.
    * step() bumps every parameter's `_version`: the kernel writes through the flat buffer, and caches keyed on `_version`
      (attributes._packed_heads) must see the update."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-3, weight_decay: float = 0,
                 weight_decouple: bool = True, rectify: bool = True, clip_quantile: Optional[float] = None,
                 history: Optional[GradNormHistory] = None, group=None, amsgrad: bool = False):
        if not weight_decouple or not rectify or amsgrad:
            raise NotImplementedError("FusedAdaBelief implements weight_decouple=True, rectify=True, amsgrad=False only")
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("FusedAdaBelief: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)")
        if clip_quantile is not None and not 0.0 <= clip_quantile <= 1.0:
            raise ValueError("FusedAdaBelief: clip_quantile must lie in [0, 1]")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise ValueError(f"FusedAdaBelief: {len(self.param_groups)} parameter groups, at most {_lib.OPTIM_MAX_GROUPS} fit")
        self._params = []
        for g in self.param_groups:
            if not g["params"]:
                raise ValueError("FusedAdaBelief: an empty parameter group")
            self._params.extend(g["params"])
        dev = self._params[0].device
        for p in self._params:
            if p.dtype != torch.float32 or p.device != dev:
                raise ValueError("FusedAdaBelief: parameters must be fp32 on one device")
            if not p.requires_grad:
                raise ValueError("FusedAdaBelief: every parameter must require a gradient (the bucket's layout is the parameters')")
            if p.numel() == 0:
                raise ValueError("FusedAdaBelief: an empty parameter")
        _lib.require_device(self._params[0], "params")
        self.numel = sum(p.numel() for p in self._params)
        self.flat = torch.empty(self.numel, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.exp_avg_var = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self._views, self._ends = [], []
        off = 0
        with torch.no_grad():
            for g in self.param_groups:
                for p in g["params"]:
                    n = p.numel()
                    v = self.flat[off:off + n].view(p.shape)
                    v.copy_(p.data)
                    p.data = v
                    self._views.append(v)
                    self.state[p] = {"step": 0, "exp_avg": self.exp_avg[off:off + n].view(p.shape),
                                     "exp_avg_var": self.exp_avg_var[off:off + n].view(p.shape)}
                    off += n
                self._ends.append(off)
        self.bucket = FlatGradBucket(self._params, group=group)
        self.clip_quantile = clip_quantile
        if history is not None and history.device != dev:
            raise ValueError("FusedAdaBelief: the history lives on another device than the parameters")
        self.history = history if history is not None else (GradNormHistory(device=dev) if clip_quantile is not None else None)
        self._partials = torch.zeros(_lib.SQNORM_MAX_PARTIALS, dtype=torch.float64, device=dev)
        self._one = torch.ones((), dtype=torch.float32, device=dev)
        self._none = torch.empty(0, dtype=torch.float32, device=dev)
        self.rebound = 0                     # parameters found outside the flat buffer and moved back in
        self.last_norm = self.last_clip = None
        self.last_coef = self._one

    # ---- the p.data <-> flat aliasing is checked, not assumed (as FlatGradBucket._rebind does for .grad) ----------------------------
    def _rebind(self) -> int:
        n = 0
        for p, v in zip(self._params, self._views):
            if p.data_ptr() == v.data_ptr() and p.numel() == v.numel():
                continue
            if p.shape != v.shape:
                raise RuntimeError("FusedAdaBelief: a parameter changed its shape")
            with torch.no_grad():
                v.copy_(p.data)
            p.data = v
            n += 1
        self.rebound += n
        return n

    def zero_grad(self, set_to_none: bool = True) -> None:
        """One fill of the flat gradient buffer; the gradients stay views of it (set_to_none is ignored)."""
        self.bucket.zero()

    def _table(self) -> torch.Tensor:
        rows = []
        for g, end in zip(self.param_groups, self._ends):
            t = int(self.state[g["params"][0]]["step"]) + 1
            k = adabelief_scalars(t, float(g["lr"]), float(g["weight_decay"]), g["betas"], float(g["eps"]))
            rows.append([float(end)] + [k[key] for key in _TABLE_KEYS] + [1.0 if k["rectified"] else 0.0])
            for p in g["params"]:
                self.state[p]["step"] = t
        return torch.tensor(rows, dtype=torch.float64)           # a HOST tensor: the shim turns it into the by-value struct

    @torch.no_grad()
    def step(self, closure=None, coef: Optional[torch.Tensor] = None):
        """One update.  coef: a one-element fp32 tensor on the parameters' device that replaces the clip coefficient (the norm, the
        clip value and the history are then left alone)."""
        if coef is not None and (coef.dtype != torch.float32 or coef.numel() != 1 or coef.device != self.flat.device):
            raise ValueError("FusedAdaBelief.step: coef must be one fp32 element on the parameters' device")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        b = self.bucket
        if not b._closed:
            b.wait()                                             # (rebinds the gradients and runs or awaits the exchange)
        else:
            b._rebind(after_backward=True)
        self._rebind()
        ops = _lib.ops()
        table = self._table()
        if coef is not None:
            self.last_norm = self.last_clip = None
            self.last_coef = coef.detach().reshape(())
        elif self.clip_quantile is not None:
            stats = torch.empty(3, dtype=torch.float32, device=self.flat.device)
            ops.grad_sqnorm(b.flat, self.numel, self._partials)
            self.history._launch(self._partials, self.numel, None, self.clip_quantile, True, stats)
            self.last_norm, self.last_clip, self.last_coef = stats[0], stats[1], stats[2]
        else:
            self.last_norm = self.last_clip = None
            self.last_coef = self._one
        has_coef = self.last_coef is not self._one
        ops.adabelief_step(self.flat, b.flat, self.exp_avg, self.exp_avg_var, self.numel,
                           self.last_coef.reshape(1) if has_coef else self._none, has_coef, table)
        torch.autograd.graph.increment_version(self._params)
        return loss

    # ---- checkpoints ---------------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """The stock state_dict (per-parameter step / exp_avg / exp_avg_var, which are views of the flat moments: copy or save it
        before the next step) plus the norm history."""
        sd = super().state_dict()
        if self.history is not None:
            sd["grad_norm_history"] = self.history.state_dict()
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        """Copies the saved moments INTO the flat buffers (the views of state[p] stay views) and takes over the groups' options."""
        groups = state_dict["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("FusedAdaBelief.load_state_dict: the saved parameter groups do not match this optimizer's")
        saved = state_dict["state"]
        for sg, g in zip(groups, self.param_groups):
            for sid, p in zip(sg["params"], g["params"]):
                st = saved.get(sid)
                if st is None:
                    continue
                mine = self.state[p]
                if st["exp_avg"].shape != p.shape or st["exp_avg_var"].shape != p.shape:
                    raise ValueError("FusedAdaBelief.load_state_dict: a saved moment does not have its parameter's shape")
                mine["step"] = int(st["step"])
                mine["exp_avg"].copy_(st["exp_avg"])
                mine["exp_avg_var"].copy_(st["exp_avg_var"])
            for k, v in sg.items():
                if k != "params":
                    g[k] = v
        hist = state_dict.get("grad_norm_history")
        if hist is not None:
            if self.history is None:
                self.history = GradNormHistory(capacity=int(hist["capacity"]), init=None, device=self.flat.device)
            self.history.load_state_dict(hist)
