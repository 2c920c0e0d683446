"""MI355X-native Neural Semi-CRF interval layer -- host-side mirror of the reference class.

Drop-in for /root/reference/transkun/CRF/NeuralSemiCRFInterval.py (class at :553-588): same
constructor, method names, defaults, argument meaning and result types.  All arithmetic runs
in hand-written gfx950 HIP kernels behind the C ABI of include/semicrf_hip.h; this file only
validates shapes, marshals the Python interval lists to/from packed int32 buffers and wires the
kernels into autograd.  CPU tensors are dispatched to the shim's own host kernels (csrc/cpu_ops.cpp; config #1,
crfMinimalExample on the CPU); a GPU tensor is never computed anywhere but in the HIP kernels.

Arithmetic is fp32 (the reference's callers are fp32 throughout); other floating dtypes are computed in fp32 and the
results and gradients are cast back to the input dtype, as the reference preserves it.

What differs from the reference, invisibly at the API:
  * computeLogZ saves alpha (v [T,B]) and logZ instead of the dense marginals [T,T,B]
    (reference :463-464) and recomputes them in backward, fused with the beta sweep.
  * logProb() is ONE autograd node: its backward writes gout*(onehot(path) - marginal) in a single
    pass instead of summing two dense [T,T,B] gradients.
  * decode() backtracks on the device; only the packed (begin,end) pairs cross PCIe.
EXTENSIONS of the reference's surface: decode_packed, sample / sample_packed (exact posterior draws of paths),
  decode_nbest / decode_nbest_packed (the k best paths, ranked), posteriors / interval_marginals /
  interval_marginals_packed (posterior marginals and path entropy without the dense [T,T,B] tensor), and decode_marginal /
  decode_marginal_packed (every interval whose posterior probability reaches a threshold), and expectation / entropy /
  covariance (posterior expectations of additive path functionals, the differentiable entropy, Hessian products of logZ).
  interval_marginals, decode_marginal and decode_mbr (and their _packed forms) take tolerance=(onset, offset) in frames: the
  probability that the path holds an interval within that window of the given one, the currency of note-level metrics.
  compare_paths / compare_paths_packed / decode_stats count in that currency: per chain the matches (exact and within a tolerance)
  and the frame overlaps between a decoded path and a target, on the device, without Python lists.
  posteriors, interval_marginals, decode_marginal and decode_mbr (and their _packed forms) take forcedStartPos= like decode: the
  posterior of the model restricted to the frames from each chain's start on, the one decode(forcedStartPos) maximises.
"""
from __future__ import annotations

import os
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib

Intervals = List[List[Tuple[int, int]]]


# --------------------------------------------------------------------------------------
# marshalling
# --------------------------------------------------------------------------------------

def _check_inputs(score: torch.Tensor, noiseScore: torch.Tensor):
    # same asserts as the reference (:209-215, :377-382, :510-511) -> AssertionError
    assert len(score.shape) == 3
    assert score.shape[0] == score.shape[1]
    assert len(noiseScore.shape) == 2
    T, B = score.shape[0], score.shape[2]
    assert noiseScore.shape[0] == T - 1
    assert noiseScore.shape[1] == B
    _lib.require_device(score, "score")
    _lib.require_device(noiseScore, "noiseScore")
    assert score.device == noiseScore.device
    return T, B


def _prep(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


_SIDE = {}


def _side_stream(device):
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    st = _SIDE.get(key)
    if st is None:
        st = _SIDE[key] = torch.cuda.Stream(device=device)
    return st


def _ready(pairs) -> None:
    """Intervals packed with overlap=True travel on a side stream: make the current stream wait for them (once)."""
    ev = getattr(pairs, "_semicrf_ready", None)
    if ev is not None:
        torch.cuda.current_stream(pairs.device).wait_event(ev)
        pairs._semicrf_ready = None


def pack_intervals(intervals: Sequence[Sequence[Tuple[int, int]]], T: int, B: int, device, overlap: bool = False, ordered: bool = True):
    """List[List[(begin,end)]] (len B) -> (pairs int32 [K,2], offsets int32 [B+1]) on `device`.
    One pass in C (csrc/pymarshal.c) into pinned host buffers, then two asynchronous copies.
    ordered (the default: the paths of evalPath / logProb, whose kernels take begin <= end as a precondition and do not check it
    on the device): ValueError naming the first interval with begin > end, raised here -- before anything is copied or launched.
    ordered=False (interval_marginals, which returns 0 for such a pair) takes any pair inside [0, T).
    overlap=True: the copies go to a side stream (they need nothing from the GPU and would otherwise sit in front of the
    sweep that the caller enqueues next: 20-100 us per call); the caller must pass `pairs` to _ready() before its first use."""
    assert len(intervals) == B, f"expected {B} interval lists, got {len(intervals)}"
    mm = _lib.marshal()
    K = int(mm.count(intervals))
    pin = torch.device(device).type == "cuda"
    pairs_h = torch.empty(max(K, 1), 2, dtype=torch.int32, pin_memory=pin)
    offsets_h = torch.empty(B + 1, dtype=torch.int32, pin_memory=pin)
    if K == 0:
        pairs_h.zero_()
    k = mm.pack_into(intervals, pairs_h.data_ptr(), max(K, 1), offsets_h.data_ptr(), T, bool(ordered))   # IndexError when out of range
    assert k == K
    if overlap and pin:
        main = torch.cuda.current_stream(device)
        side = _side_stream(device)
        with torch.cuda.stream(side):
            pairs_d = pairs_h.to(device, non_blocking=True)
            offsets_d = offsets_h.to(device, non_blocking=True)
            ev = side.record_event()
        pairs_d.record_stream(main); offsets_d.record_stream(main)      # allocated in the side stream's pool, used on `main`
        pairs_d._semicrf_ready = ev
    else:
        pairs_d = pairs_h.to(device, non_blocking=True)
        offsets_d = offsets_h.to(device, non_blocking=True)
    pairs_d._semicrf_K = K          # number of real intervals (the tensor holds one dummy row when K == 0)
    # can logProb's backward take the path as a table (begins ascend strictly, no interval starts inside the previous one)?
    pairs_d._semicrf_simple = bool(ordered) and bool(mm.path_is_simple(pairs_h.data_ptr(), offsets_h.data_ptr(), B))
    return pairs_d, offsets_d


def unpack_intervals(pairs_host: torch.Tensor, offsets_host: torch.Tensor, T: int = 1 << 30) -> Intervals:
    """packed int32 [K,2] + offsets [B+1] (host) -> List[List[Tuple[int,int]]] (the reference's result type), built in C
    with one shared int object per frame index (csrc/pymarshal.c); the cyclic GC is paused meanwhile (hundreds of
    thousands of fresh tuples would otherwise trigger several full collections)."""
    import gc
    pairs_host = pairs_host.contiguous()
    offsets_host = offsets_host.contiguous()
    assert pairs_host.dtype == torch.int32 and offsets_host.dtype == torch.int32
    B = offsets_host.numel() - 1
    total = int(offsets_host[-1]) if B >= 0 else 0
    assert pairs_host.numel() >= 2 * total
    if T >= 1 << 30:
        T = int(pairs_host[:total].max()) + 1 if total else 1
    was = gc.isenabled()
    gc.disable()
    try:
        return _lib.marshal().unpack(pairs_host.data_ptr(), offsets_host.data_ptr(), B, T)
    finally:
        if was:
            gc.enable()


# --------------------------------------------------------------------------------------
# raw kernel calls (no autograd)
# --------------------------------------------------------------------------------------

_DEBUG_WS = []      # test/diagnostic hook: when non-None-appendable and env SEMICRF_DEBUG_KEEP_WS is set, keeps workspaces


def _odd_pad(score) -> bool:
    """The persistent kernels take any NBatch >= 2 (an odd one natively since round 2: 4-byte aligned 16-byte accesses).
    A single chain is run with one all-zero ghost chain appended instead of on the ~100x slower row-sequential kernels;
    the ghost chain's outputs are dropped."""
    return score.is_cuda and score.shape[2] == 1 and score.shape[0] >= 2 and _lib.get_impl() == 0


def _pad1(t):
    return torch.nn.functional.pad(t, (0, 1))


def _logz_fwd_raw(score, noise, want_v: bool):
    if _odd_pad(score):
        logz, v = _logz_fwd_raw(_pad1(score), _pad1(noise), want_v)
        return logz[:-1].contiguous(), (v[:, :-1].contiguous() if v is not None else None)
    T, B = score.shape[0], score.shape[2]
    logz = torch.empty(B, dtype=torch.float32, device=score.device)
    v = torch.empty((T, B) if want_v else (0,), dtype=torch.float32, device=score.device)
    ws = _lib.leased_workspace(_lib.OP_LOGZ_FWD, T, B, score.device)
    _lib.ops().logz_fwd(score, noise, logz, v, want_v, ws)
    if os.environ.get("SEMICRF_DEBUG_KEEP_WS"):
        _DEBUG_WS[:] = [ws]
    return logz, (v if want_v else None)


# --------------------------------------------------------------------------------------
# the dense gradient's buffers
# --------------------------------------------------------------------------------------
# The reference's contract is a DENSE [T,T,B] gradient whose upper triangle (begin > end) is exactly zero
# (NeuralSemiCRFInterval.py:436-440, :469-472).  Those zeros are a third of the bytes the gradient sweep moves (0.74 of
# 2.22 GB at T=1024, NBatch=352) and they never change.  The pool below keeps the MEMORY of gradient tensors this library
# has fully written once (zeros included) and hands it out again -- with SEMICRF_GRAD_UPPER_IS_ZERO, so that the sweep skips
# the zeros -- only while both hold:
#   * nothing else references the storage (every tensor that aliased it -- score.grad, views, what autograd kept -- is gone);
#   * the version counter the handed-out tensor shares with all of its aliases is where the library's last write left it:
#     any in-place operation on the gradient by anybody (grad.add_(..), zero_(), an optimizer, AccumulateGrad adding a second
#     gradient into it) moves the counter, and the buffer is then written in full (zeros included) on its next use.
# The pool keeps `P.detach()` (same storage, same version counter, its own TensorImpl) and not P itself: autograd takes a
# gradient as .grad without a copy only when nobody else holds the tensor object.
GRAD_UPPER_IS_ZERO = _lib.GRAD_UPPER_IS_ZERO


# torch._C._storage_Use_Count is a private binding (present in every torch 2.x this was run on): without it the pool cannot know
# that nobody else holds a buffer, so it stays off -- one warning, every gradient is then written in full like before round 4.
_USE_COUNT = getattr(torch._C, "_storage_Use_Count", None)
_WARNED = set()


def _warn_once(tag: str, msg: str) -> None:
    if tag not in _WARNED:
        _WARNED.add(tag)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _storage_users(t: torch.Tensor) -> int:
    st = t.untyped_storage()
    return _USE_COUNT(st._cdata) - 1           # minus the temporary `st`


def _empty_or_trim(shape, device):
    """torch.empty; on an out-of-memory error the pools (which hold memory outside the caching allocator's reach) are released
    and the allocation is tried once more."""
    try:
        return torch.empty(shape, dtype=torch.float32, device=device)
    except getattr(torch, "OutOfMemoryError", torch.cuda.OutOfMemoryError):      # (older torch 2.x: only torch.cuda.OutOfMemoryError)
        grad_pool_clear()
        if device.type == "cuda":
            torch.cuda.empty_cache()
        return torch.empty(shape, dtype=torch.float32, device=device)


class _GradPool:
    PER_KEY = 2                      # buffers kept per (device, stream, T, B): what one training step can have in flight

    def __init__(self):
        import threading
        self.lock = threading.Lock()
        self.entries = []            # [key, keeper, version] -- most recently used last
        self.enabled = not os.environ.get("SEMICRF_NO_GRAD_POOL")
        if self.enabled and _USE_COUNT is None:
            self.enabled = False
            _warn_once("use_count", "transkun_amd: torch._C._storage_Use_Count is not available in this torch build; the pool of "
                                    "gradient / score buffers is off (every dense gradient is written in full, zeros included)")
        # budget: SEMICRF_GRAD_POOL_BYTES, else 4 GiB (two [1024,1024,352] buffers are 2.75 GiB); never more than PER_KEY per shape
        self.max_bytes = int(os.environ.get("SEMICRF_GRAD_POOL_BYTES", str(4 << 30)))
        self.min_bytes = 16 << 20    # smaller gradients: the zeros cost microseconds
        self.hits = self.misses = 0  # statistics (tests, bench)

    def held_bytes(self) -> int:
        """Bytes of device / host memory the pool keeps alive right now (outside the caching allocator's reach)."""
        with self.lock:
            return sum(e[1].numel() * 4 for e in self.entries)

    def take(self, T: int, B: int, device):
        """(dscore [T,T,B] fp32, flags): a pooled buffer with flags = GRAD_UPPER_IS_ZERO, or a fresh one with flags 0."""
        nbytes = 4 * T * T * B
        # inference tensors have no version counter (and nothing computes gradients under inference_mode): never pooled
        if not self.enabled or nbytes < self.min_bytes or torch.is_inference_mode_enabled():
            return _empty_or_trim((T, T, B), device), 0, None
        if device.type == "cpu":
            # host tensors too: the host kernels write the zeros anyway, but a fresh 1.4 GB allocation is 350 000 first-touch page
            # faults that many threads take at once (T=1024 x 352: the backward took 1.4 s on 8 threads and 8 - 20 s on 22 - 64)
            key = ("cpu", 0, T, B)
        else:
            if device.type != "cuda" or torch.cuda.is_current_stream_capturing():
                return _empty_or_trim((T, T, B), device), 0, None
            key = (device.index if device.index is not None else torch.cuda.current_device(),
                   torch.cuda.current_stream(device).cuda_stream, T, B)
        with self.lock:
            for i in range(len(self.entries) - 1, -1, -1):
                k, keeper, ver = self.entries[i]
                if k == key and _storage_users(keeper) == 1:
                    del self.entries[i]
                    if keeper._version == ver:
                        self.hits += 1
                        return keeper, GRAD_UPPER_IS_ZERO, key           # keeper becomes the handed-out tensor, see give()
                    self.misses += 1
                    return keeper, 0, key                                # written in place since: everything is written again
            self.misses += 1
        return _empty_or_trim((T, T, B), device), 0, key

    def give(self, key, dscore: torch.Tensor) -> None:
        """After the library's last write into `dscore` (its upper triangle holds exact zeros now): remember the memory."""
        if key is None or dscore.is_inference():
            return
        keeper = dscore.detach()
        nbytes = keeper.numel() * 4
        with self.lock:
            self.entries.append([key, keeper, keeper._version])
            same = [i for i, e in enumerate(self.entries) if e[0] == key]
            for i in same[:-self.PER_KEY]:                               # the oldest of this shape beyond PER_KEY
                self.entries[i] = None
            self.entries = [e for e in self.entries if e is not None]
            total = 0
            for i in range(len(self.entries) - 1, -1, -1):               # newest first; drop what exceeds the budget
                total += self.entries[i][1].numel() * 4
                if total > max(self.max_bytes, nbytes):
                    del self.entries[:i + 1]
                    break

    def rerecord(self, dscore: torch.Tensor) -> None:
        """The library itself has written cells with begin <= end into a pooled buffer again (the path cells of evalPath's
        gradient): that write is not an edit of the upper triangle."""
        if dscore is None:
            return
        ptr = dscore.data_ptr()
        with self.lock:
            for e in self.entries:
                if e[1].data_ptr() == ptr:
                    e[2] = e[1]._version

    def clear(self) -> None:
        with self.lock:
            self.entries.clear()


_GRAD_POOL = _GradPool()


def grad_pool_bytes() -> int:
    """Bytes the gradient pool and the scorer's score pool hold right now."""
    from .. import scorer as _sc
    return _GRAD_POOL.held_bytes() + (_sc._SCORE_POOL.held_bytes() if _sc._SCORE_POOL is not None else 0)


def grad_pool_clear() -> None:
    """Release the gradient buffers the pool holds (at most two per (device, stream, T, B) and SEMICRF_GRAD_POOL_BYTES -- 4 GiB by
    default -- in total; SEMICRF_NO_GRAD_POOL=1 disables the pool; an out-of-memory error inside the library releases them by
    itself) -- and the interval scorer's pool of score tensors, which works the same way (transkun_amd/scorer.py)."""
    _GRAD_POOL.clear()
    from .. import scorer as _sc
    if _sc._SCORE_POOL is not None:
        _sc._SCORE_POOL.clear()


def _logz_bwd_raw(score, noise, v, logz, gout, want_q: bool = False):
    if _odd_pad(score):
        ds, dn, q = _logz_bwd_raw(_pad1(score), _pad1(noise), _pad1(v), _pad1(logz), _pad1(gout), want_q)
        return ds[:, :, :-1].contiguous(), dn[:, :-1].contiguous(), (q[:, :-1].contiguous() if q is not None else None)
    T, B = score.shape[0], score.shape[2]
    dscore, flags, pkey = _GRAD_POOL.take(T, B, score.device)
    dnoise = torch.empty_like(noise)
    q = torch.empty((T, B) if want_q else (0,), dtype=torch.float32, device=score.device)
    ws = _lib.leased_workspace(_lib.OP_LOGZ_BWD, T, B, score.device)
    _lib.ops().logz_bwd(score, noise, v, logz, gout, dscore, dnoise, q, want_q, flags, ws)
    _GRAD_POOL.give(pkey, dscore)
    return dscore, dnoise, (q if want_q else None)


# logProb's backward in ONE launch: the forward's path wave leaves the path as a table [T, B] and the gradient sweep's writers add
# the path's own +-gout to what they store (semicrf_logprob_fwd_t / _bwd_t), instead of a scatter kernel behind the sweep.
# PATH_FOLD = False forces the two-launch route (same bits); PATH_ROUTES counts the routes _LogProb.backward has taken.
PATH_FOLD = True
PATH_ROUTES = {"folded": 0, "scatter": 0}


def _path_table_ok(score, pairs) -> bool:
    """Does this call get a path table?  The path must be one the table can hold (pack_intervals checked it on the host), the
    gradient sweep of this shape one whose every cell has a writer that can look its row up (semicrf_logprob_path_table_supported)."""
    if not (PATH_FOLD and score.is_cuda and getattr(pairs, "_semicrf_simple", False)) or _odd_pad(score):
        return False
    return _lib.load().semicrf_logprob_path_table_supported(int(score.shape[0]), int(score.shape[2])) == 1


def _logprob_fwd_raw(score, noise, pairs, offsets, want_v: bool, ptab=None):
    """(logProb [B], logZ [B], alpha [T,B] or None) from ONE launch: spare waves of the forward sweep compute the path scores, the
    ring wave that finalises logZ subtracts (semicrf_logprob_fwd; bit-identical to _eval_path_raw(...) - logZ).  `pairs` must be
    ready on the current stream (_ready).  ptab: an int32 [T, B] tensor the launch fills with the path table, or None."""
    K = getattr(pairs, "_semicrf_K", pairs.shape[0])
    if _odd_pad(score):
        logz, v = _logz_fwd_raw(score, noise, want_v)
        return _eval_path_raw(score, noise, pairs, offsets) - logz, logz, v
    T, B = score.shape[0], score.shape[2]
    dev = score.device
    lp = torch.empty(B, dtype=torch.float32, device=dev)
    logz = torch.empty(B, dtype=torch.float32, device=dev)
    v = torch.empty((T, B) if want_v else (0,), dtype=torch.float32, device=dev)
    ws = _lib.leased_workspace(_lib.OP_LOGZ_FWD, T, B, dev)
    _lib.ops().logprob_fwd(score, noise, pairs, int(K), offsets, lp, logz, v, want_v, ws, ptab if ptab is not None else offsets,
                           ptab is not None)
    return lp, logz, (v if want_v else None)


def _eval_path_raw(score, noise, pairs, offsets):
    T, B = score.shape[0], score.shape[2]
    out = torch.empty(B, dtype=torch.float32, device=score.device)
    ws = _lib.workspace(_lib.OP_EVAL_PATH, T, B, score.device)
    K = getattr(pairs, "_semicrf_K", pairs.shape[0])
    _lib.ops().eval_path(score, noise, pairs, int(K), offsets, out, ws)
    return out


_EMPTY = {}


def _empty(device):
    e = _EMPTY.get(device)
    if e is None:
        e = _EMPTY[device] = torch.empty(0, dtype=torch.float32, device=device)
    return e


def _eval_path_bwd_raw(gout, T, B, pairs, offsets, dscore, dnoise, K: int, pooled: bool = False):
    """pooled: dscore is a gradient buffer this pass got from _logz_bwd_raw and nobody but this library has written to since
    (the scatter touches cells begin <= end only: the pool's record of the buffer stays valid)."""
    e = _empty(gout.device)
    _lib.ops().eval_path_bwd(gout, T, B, pairs, int(K), offsets, dscore if dscore is not None else e, dscore is not None,
                             dnoise if dnoise is not None else e, dnoise is not None)
    if pooled:
        _GRAD_POOL.rerecord(dscore)


def _gout(grad_output: torch.Tensor, B: int) -> torch.Tensor:
    assert grad_output.shape[-1] == B      # reference :471
    g = grad_output.reshape(B)
    if g.dtype != torch.float32:
        g = g.float()
    return g.contiguous()


# --------------------------------------------------------------------------------------
# autograd nodes
# --------------------------------------------------------------------------------------

# The reference's own call pattern is crf.evalPath(...) - crf.computeLogZ() as TWO autograd nodes (ModelTransformer.py:263-265).
# Differentiated naively, the evalPath node returns a dense zero [T,T,B] tensor with a few thousand cells set and autograd
# adds it to the dense gradient of the logZ node: two more passes over 1.48 GB at T=1024, NBatch=352.
#
# The methods of one NeuralSemiCRFInterval object therefore hang their nodes on a private HUB node (_Hub: an identity on
# (score, noiseScore) that only this object knows).  In backward the children do not hand dense gradients to the engine: they
# DEPOSIT them in the hub's accumulator of the running graph task -- the first dense gradient becomes the buffer, later dense
# ones are added in place, an evalPath node scatters its +-gout cells straight into it (or is parked until a dense gradient
# arrives) -- and return None; the hub's own backward, which the engine runs after every child of the pass, hands the
# buffer on.  The accumulator OWNS the tensor (a strong reference, no raw addresses), so any number of consumers of `score`
# in any order is safe: consumers outside this object meet the hub's result one level up, in the engine's own buffers.
# The module-level functions (no object, no hub) differentiate the plain way.


def _graph_task_id() -> int:
    fn = getattr(torch._C, "_current_graph_task_id", None)
    return int(fn()) if fn is not None else -1


class _HubState:
    """Gradient accumulators of one CRF object's hub, one per graph task in flight."""

    def __init__(self):
        self.acc = {}

    def _slot(self, tid):
        a = self.acc.get(tid)
        if a is None:
            a = self.acc[tid] = {"ds": None, "dn": None, "paths": [], "shape": None, "dev": None}
            if len(self.acc) > 8:                       # passes that never reached the hub (an error mid-backward)
                for k in list(self.acc)[:-8]:
                    if self.acc[k]["ds"] is not None or self.acc[k]["paths"]:
                        import warnings
                        warnings.warn("transkun_amd.CRF: more than 8 backward passes through one NeuralSemiCRFInterval object are in "
                                      "flight; the oldest one's deposited gradient is dropped (re-entrant / multi-threaded backward "
                                      "sharing one CRF object?) -- its score gradient will be incomplete")
                    del self.acc[k]
        return a

    @staticmethod
    def _scatter(a, path):
        g, pairs, offsets, K, T, B = path
        _eval_path_bwd_raw(g, T, B, pairs, offsets, a["ds"], a["dn"], K, pooled=a.get("pristine", False))

    def deposit_dense(self, tid, dscore, dnoise):
        a = self._slot(tid)
        if a["ds"] is None:
            a["ds"], a["dn"] = dscore, dnoise
            a["pristine"] = True                    # straight from _logz_bwd_raw: only this library has written to it
            for p in a["paths"]:
                self._scatter(a, p)
            a["paths"] = []
        else:
            a["pristine"] = False
            a["ds"].add_(dscore)
            if dnoise is not None and a["dn"] is not None:
                a["dn"].add_(dnoise)

    def deposit_path(self, tid, g, pairs, offsets, K, T, B):
        a = self._slot(tid)
        a["shape"], a["dev"] = (T, B), g.device
        if a["ds"] is not None:
            self._scatter(a, (g, pairs, offsets, K, T, B))
        else:
            a["paths"].append((g, pairs, offsets, K, T, B))

    def collect(self, tid):
        a = self.acc.pop(tid, None)
        if a is None:
            return None, None
        if a["ds"] is None and a["paths"]:              # only evalPath nodes were reached: the dense zero tensor after all
            T, B = a["shape"]
            a["ds"] = torch.zeros(T, T, B, dtype=torch.float32, device=a["dev"])
            a["dn"] = torch.zeros(max(T - 1, 0), B, dtype=torch.float32, device=a["dev"])
            for p in a["paths"]:
                self._scatter(a, p)
        return a["ds"], a["dn"]


class _Hub(torch.autograd.Function):
    """Identity on (score, noiseScore), private to one NeuralSemiCRFInterval object: collects its children's gradients."""

    @staticmethod
    def forward(ctx, score, noiseScore, state):
        ctx.state = state
        ctx.set_materialize_grads(False)
        ctx.in_dtypes = (score.dtype, noiseScore.dtype)
        ctx.shapes = (score.shape, noiseScore.shape)
        return score.detach(), noiseScore.detach()

    @staticmethod
    def backward(ctx, gs, gn):
        ds, dn = ctx.state.collect(_graph_task_id())
        if gs is not None:                              # a child that returned its gradient the plain way
            ds = gs.float() if ds is None else ds.add_(gs)
        if gn is not None:
            dn = gn.float() if dn is None else dn.add_(gn)
        if ds is not None:
            ds = ds.reshape(ctx.shapes[0]).to(ctx.in_dtypes[0])
        if dn is not None:
            dn = dn.reshape(ctx.shapes[1]).to(ctx.in_dtypes[1])
        return ds, dn, None


def _hub_of(state):
    """The state to deposit in during this backward pass, or None (no hub / no graph task id: return gradients plainly)."""
    if state is None or torch.is_grad_enabled() or _graph_task_id() < 0:
        return None
    return state


class ComputeLogZFasterGrad(torch.autograd.Function):
    """logZ with a hand-written gradient (reference :459-475), recompute-in-backward flavour."""

    @staticmethod
    def forward(ctx, score, noiseScore, hub=None):
        score_c, noise_c = _prep(score), _prep(noiseScore)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        logz, v = _logz_fwd_raw(score_c, noise_c, want_v=need)
        if need:
            ctx.save_for_backward(score_c, noise_c, v, logz)
        ctx.in_dtypes = (score.dtype, noiseScore.dtype)
        ctx.hub = hub
        return logz.to(score.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        score, noise, v, logz = ctx.saved_tensors
        B = score.shape[2]
        dscore, dnoise, _ = _logz_bwd_raw(score, noise, v, logz, _gout(grad_output, B))
        hub = _hub_of(ctx.hub)
        if hub is not None:
            hub.deposit_dense(_graph_task_id(), dscore, dnoise)
            return None, None, None
        return dscore.to(ctx.in_dtypes[0]), dnoise.to(ctx.in_dtypes[1]), None


def computeLogZFasterGrad(score, noiseScore):
    return ComputeLogZFasterGrad.apply(score, noiseScore)


class _EvalPath(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, noiseScore, pairs, offsets, hub=None):
        score_c, noise_c = _prep(score), _prep(noiseScore)
        ctx.save_for_backward(pairs, offsets)
        ctx.shape = (score_c.shape[0], score_c.shape[2])
        ctx.K = getattr(pairs, "_semicrf_K", pairs.shape[0])
        ctx.in_dtypes = (score.dtype, noiseScore.dtype)
        ctx.hub = hub
        return _eval_path_raw(score_c, noise_c, pairs, offsets).to(score.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        pairs, offsets = ctx.saved_tensors
        T, B = ctx.shape
        g = _gout(grad_output, B)
        hub = _hub_of(ctx.hub)
        if hub is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1]:
            # the path cells go straight into the pass's dense gradient (owned by the hub); nothing of its own
            hub.deposit_path(_graph_task_id(), g, pairs, offsets, ctx.K, T, B)
            return None, None, None, None, None
        dscore = torch.zeros(T, T, B, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[0] else None
        dnoise = torch.zeros(max(T - 1, 0), B, dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
        _eval_path_bwd_raw(g, T, B, pairs, offsets, dscore, dnoise, ctx.K)
        return (dscore.to(ctx.in_dtypes[0]) if dscore is not None else None,
                dnoise.to(ctx.in_dtypes[1]) if dnoise is not None else None, None, None, None)


def _gout_strided(grad_output: torch.Tensor, B: int):
    """(fp32 tensor, stride): the cotangent as the kernels take it -- B values (stride 1) or, when autograd hands down an
    expanded scalar (the usual loss, -logProb.sum() / n: train.py:187), that ONE value (stride 0): no [B] copy, no kernel."""
    assert grad_output.shape[-1] == B      # reference :471
    g = grad_output.reshape(B) if grad_output.dim() != 1 else grad_output
    if g.dtype != torch.float32:
        g = g.float()
    if B > 1 and g.stride(0) == 0:
        return g.as_strided((1,), (1,)), 0
    return g.contiguous(), 1


class _LogProb(torch.autograd.Function):
    """evalPath - logZ as one node (semicrf_logprob_fwd / semicrf_logprob_bwd): the forward subtracts inside the path kernel,
    the backward writes gout * (onehot(path) - marginals) in one dense pass."""

    @staticmethod
    def forward(ctx, score, noiseScore, pairs, offsets):
        score_c, noise_c = _prep(score), _prep(noiseScore)
        need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        T, B = score_c.shape[0], score_c.shape[2]
        K = getattr(pairs, "_semicrf_K", pairs.shape[0])
        _ready(pairs)                                   # the intervals' copy ran on a side stream
        # (the table is this call's own tensor, saved for backward -- not workspace: other calls may run in between)
        ptab = torch.empty((T, B), dtype=torch.int32, device=score_c.device) if need and _path_table_ok(score_c, pairs) else None
        lp, logz, v = _logprob_fwd_raw(score_c, noise_c, pairs, offsets, need, ptab)
        if need:
            ctx.save_for_backward(score_c, noise_c, v, logz, pairs, offsets, *([ptab] if ptab is not None else []))
            ctx.K = K
        ctx.in_dtypes = (score.dtype, noiseScore.dtype)
        return lp.to(score.dtype)

    @staticmethod
    def backward(ctx, grad_output):
        score, noise, v, logz, pairs, offsets = ctx.saved_tensors[:6]
        ptab = ctx.saved_tensors[6] if len(ctx.saved_tensors) > 6 else None
        T, B = score.shape[0], score.shape[2]
        # (the library ignores the table where the launch cannot use it -- the implementation switch may have moved since forward)
        folded = ptab is not None and PATH_FOLD and _lib.load().semicrf_logprob_path_table_supported(int(T), int(B)) == 1
        PATH_ROUTES["folded" if folded else "scatter"] += 1
        if _odd_pad(score):
            g = _gout(grad_output, B)
            dscore, dnoise, _ = _logz_bwd_raw(score, noise, v, logz, -g)
            _eval_path_bwd_raw(g, T, B, pairs, offsets, dscore, dnoise, ctx.K)          # (a padded copy: sliced below, never pooled)
        else:
            g, gstride = _gout_strided(grad_output, B)
            dscore, flags, pkey = _GRAD_POOL.take(T, B, score.device)
            dnoise = torch.empty_like(noise)
            ws = _lib.leased_workspace(_lib.OP_LOGZ_BWD, T, B, score.device)
            _lib.ops().logprob_bwd(score, noise, v, logz, g, gstride, pairs, int(ctx.K), offsets, dscore, dnoise, flags, ws,
                                   ptab if folded else offsets, folded)
            _GRAD_POOL.give(pkey, dscore)
        return dscore.to(ctx.in_dtypes[0]), dnoise.to(ctx.in_dtypes[1]), None, None


# --------------------------------------------------------------------------------------
# module-level functions with the reference's names
# --------------------------------------------------------------------------------------

def _viterbi_raw(score_c, noise_c, start, forward: bool):
    """Enqueue the Viterbi sweep + on-device backtrack; returns device tensors (pairs [cap,2], offsets [B+1])."""
    if _odd_pad(score_c):
        st = _pad1(start) if start is not None else None
        pairs, offsets = _viterbi_raw(_pad1(score_c), _pad1(noise_c), st, forward)
        return pairs, offsets[:-1]        # the ghost chain is last: its intervals lie behind offsets[B]
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    cap = B * 2 * T
    pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    ws = _lib.leased_workspace(_lib.OP_VITERBI, T, B, dev)
    has = start is not None
    _lib.ops().viterbi(score_c, noise_c, start if has else offsets, has, bool(forward), pairs, offsets, ws)
    return pairs, offsets


def _start_tensor(forcedStartPos: Optional[Sequence[int]], T: int, B: int, device):
    """forcedStartPos (None or B frames) as the int32 device vector semicrf_viterbi takes; IndexError when out of range."""
    if forcedStartPos is None:
        return None
    assert len(forcedStartPos) == B
    st = np.asarray(forcedStartPos, dtype=np.int64)
    if (st < 0).any() or (st > T - 1).any():
        raise IndexError(f"forcedStartPos out of range for T={T}")
    return torch.from_numpy(st.astype(np.int32)).to(device, non_blocking=True)


def _decode(score, noiseScore, forcedStartPos: Optional[Sequence[int]], forward: bool, packed: bool = False):
    assert len(score.shape) == 3
    assert score.shape[0] == score.shape[1]
    T, B = _check_inputs(score, noiseScore)
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        start = _start_tensor(forcedStartPos, T, B, score_c.device)
        pairs, offsets = _viterbi_raw(score_c, noise_c, start, forward)
        off_h = offsets.cpu()                      # the one host sync of decode
        total = int(off_h[-1])
        if total < 0:
            _lib.async_error()                     # consumed here: the next call must not report this time-out again
            raise RuntimeError("semicrf_viterbi: a bounded hand-off wait timed out on the device (GPU shared with work that "
                               "kept part of the persistent kernel from running?); the decode result is invalid")
        pairs_h = pairs[:total].cpu()
    if packed:
        return pairs_h.numpy(), off_h.numpy()
    return unpack_intervals(pairs_h, off_h, T)


# --------------------------------------------------------------------------------------
# posterior sampling (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

_SAMPLE_CELLS = 1 << 24     # draws * chains * frames per device call: the workspace is ~20 B and the pairs buffer 16 B per cell


def _sample_key(generator) -> int:
    """The 64-bit key of a draw: one value of the (CPU) generator, so torch.manual_seed reproduces a draw."""
    if generator is not None and torch.device(generator.device).type != "cpu":
        raise ValueError(f"sample: the generator is on {generator.device}; pass a CPU torch.Generator (or None for torch's "
                         "default one) -- it only makes the key, the draws themselves run where the scores live")
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator))


def _sample_raw(score_c, noise_c, v, k0: int, n: int, key: int, end):
    """Enqueue draws k0 .. k0+n-1 (code table + on-device walk + packing); returns (pairs [cap,2], offsets [n*B+1]) where the
    scores live."""
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    pairs = torch.empty(n * B * 2 * T, 2, dtype=torch.int32, device=dev)
    offsets = torch.empty(n * B + 1, dtype=torch.int32, device=dev)
    ws = _lib.workspace(_lib.OP_SAMPLE, T, n * B, dev)
    has = end is not None
    _lib.ops().sample(score_c, noise_c, v, int(k0), int(n), int(key), end if has else offsets, has, pairs, offsets, ws)
    return pairs, offsets


def _sample(score, noiseScore, nSample: int, forcedEndPos: Optional[Sequence[int]], generator):
    """(pairs [K,2], offsets [nSample*B+1]) as numpy int32, sample-major: chain c of draw k owns offsets[k*B+c]:offsets[k*B+c+1]."""
    T, B = _check_inputs(score, noiseScore)
    if int(nSample) != nSample or nSample < 1:
        raise ValueError(f"sample: nSample must be a positive integer, got {nSample!r}")
    nSample = int(nSample)
    key = _sample_key(generator)
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        dev = score_c.device
        end = None
        if forcedEndPos is not None:
            if len(forcedEndPos) != B:
                raise IndexError(f"forcedEndPos holds {len(forcedEndPos)} positions for {B} chains")
            e = np.asarray(forcedEndPos, dtype=np.int64)
            if (e < 0).any() or (e > T - 1).any():
                raise IndexError(f"forcedEndPos out of range for T={T}")
            end = torch.from_numpy(e.astype(np.int32)).to(dev, non_blocking=True)
        _, v = _logz_fwd_raw(score_c, noise_c, want_v=True)
        per = max(1, min(nSample, _SAMPLE_CELLS // (B * T)))
        pair_parts, off_parts, base = [], [np.zeros(1, dtype=np.int32)], 0
        for k0 in range(0, nSample, per):
            n = min(per, nSample - k0)
            pairs, offsets = _sample_raw(score_c, noise_c, v, k0, n, key, end)
            off_h = offsets.cpu()                  # the one host sync per call
            total = int(off_h[-1])
            if total < 0:
                _lib.async_error()                 # consumed here: the next call must not report this time-out again
                raise RuntimeError("semicrf_sample: alpha holds NaN in its last row -- the inputs hold NaN (or -inf cells, which the "
                                   "device's forward sweep does not take), or a bounded hand-off wait of the sweep timed out on the "
                                   "device (GPU shared with work that kept part of the persistent kernel from running?); the draws are "
                                   "invalid")
            pair_parts.append(pairs[:total].cpu().numpy())
            off_parts.append(off_h.numpy()[1:] + base)
            base += total
    pairs_np = np.concatenate(pair_parts).reshape(-1, 2).astype(np.int32, copy=False)
    return pairs_np, np.concatenate(off_parts).astype(np.int32, copy=False)


def sample_packed(score, noiseScore, nSample: int = 1, forcedEndPos: Optional[Sequence[int]] = None, generator=None):
    """An EXTENSION of the reference's surface: `nSample` paths per chain drawn exactly from p(path) = exp(evalPath - logZ), as
    two int32 arrays -- pairs [K, 2] of (begin, end) and offsets [nSample * nBatch + 1], sample-major (chain c of draw k owns
    pairs[offsets[k * nBatch + c]:offsets[k * nBatch + c + 1]], ascending within a path, like decode_packed).

    forcedEndPos: None or nBatch frames -- the path's END, as decode(forward=True, forcedStartPos=...): the prefix path on
    [0, e] given a boundary at e.  generator: None (torch's default CPU generator: torch.manual_seed reproduces a draw) or a CPU
    torch.Generator; it makes one 64-bit key, and the draws are a pure function of (inputs, key): the first m of n draws are
    the m draws of nSample=m."""
    return _sample(score, noiseScore, nSample, forcedEndPos, generator)


def sample(score, noiseScore, nSample: int = 1, forcedEndPos: Optional[Sequence[int]] = None, generator=None) -> List[Intervals]:
    """An EXTENSION of the reference's surface: `nSample` exact draws from p(path | score) (forward-filtering backward-sampling);
    a list of nSample Intervals (one interval list per chain, the type decode returns).  Arguments as sample_packed."""
    T, B = _check_inputs(score, noiseScore)
    pairs, offsets = _sample(score, noiseScore, nSample, forcedEndPos, generator)
    flat = unpack_intervals(torch.from_numpy(pairs), torch.from_numpy(offsets), T)
    return [flat[k * B:(k + 1) * B] for k in range(len(flat) // B)]


# --------------------------------------------------------------------------------------
# k-best Viterbi (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

NBEST_MAX = 16


def _nbest_raw(score_c, noise_c, k: int, start, forward: bool):
    """Enqueue semicrf_viterbi_nbest; returns device tensors pairs [cap, 2] and meta = offsets [k*B+1] | npaths [B] | the bits of
    scores [k*B] (one int32 buffer: one copy back)."""
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    nB = k * B
    pairs = torch.empty(nB * 2 * T, 2, dtype=torch.int32, device=dev)
    meta = torch.empty(2 * nB + 1 + B, dtype=torch.int32, device=dev)
    offsets, npaths = meta[:nB + 1], meta[nB + 1:nB + 1 + B]
    scores = meta[nB + 1 + B:].view(torch.float32)
    ws = _lib.workspace(_lib.OP_VITERBI_NBEST, T, nB, dev)
    has = start is not None
    _lib.ops().viterbi_nbest(score_c, noise_c, k, start if has else offsets, has, bool(forward), pairs, offsets, scores, npaths, ws)
    return pairs, meta


def _nbest(score, noiseScore, k, forcedStartPos: Optional[Sequence[int]], forward: bool):
    """(pairs [K,2], offsets [k*B+1], scores [k,B] float32, npaths [B]) as numpy arrays, rank-major: chain c of rank r owns
    pairs[offsets[r*B+c]:offsets[r*B+c+1]]."""
    T, B = _check_inputs(score, noiseScore)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError(f"decode_nbest: k must be an integer in [1, {NBEST_MAX}], got {k!r}")
    k = int(k)
    if not 1 <= k <= NBEST_MAX:
        raise ValueError(f"decode_nbest: k must be in [1, {NBEST_MAX}], got {k}")
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        dev = score_c.device
        start = None
        if forcedStartPos is not None:
            if len(forcedStartPos) != B:
                raise IndexError(f"forcedStartPos holds {len(forcedStartPos)} positions for {B} chains")
            st = np.asarray(forcedStartPos, dtype=np.int64)
            if (st < 0).any() or (st > T - 1).any():
                raise IndexError(f"forcedStartPos out of range for T={T}")
            start = torch.from_numpy(st.astype(np.int32)).to(dev, non_blocking=True)
        nB = k * B
        pairs, meta = _nbest_raw(score_c, noise_c, k, start, forward)
        meta_h = meta.cpu().numpy()                # the one host sync per call
        total = int(meta_h[nB])
        pairs_h = pairs[:total].cpu().numpy()
    return (pairs_h, meta_h[:nB + 1].copy(), meta_h[nB + 1 + B:].view(np.float32).reshape(k, B).copy(),
            meta_h[nB + 1:nB + 1 + B].copy())


def viterbi_nbest_packed(score, noiseScore, k: int, forcedStartPos: Optional[Sequence[int]] = None, forward: bool = False):
    """An EXTENSION of the reference's surface: the k highest-scoring paths of every chain as numpy arrays (pairs [K, 2] int32,
    offsets [k * nBatch + 1] int32, scores [k, nBatch] float32, npaths [nBatch] int32).  Rank-major: chain c of rank r owns
    pairs[offsets[r * nBatch + c]:offsets[r * nBatch + c + 1]], in decode's order.  scores are the Viterbi recursion's fp32
    values; ranks past npaths[c] (fewer than k paths exist at tiny T) are empty with score -inf.  Ties are broken by a fixed
    order (include/semicrf_hip.h: semicrf_viterbi_nbest), so k = 1 is decode bit for bit and the first m ranks of k are m-best.
    forcedStartPos / forward: as decode (the END frame when forward=True).  1 <= k <= 16; no gradient."""
    return _nbest(score, noiseScore, k, forcedStartPos, forward)


def viterbi_nbest(score, noiseScore, k: int, forcedStartPos: Optional[Sequence[int]] = None, forward: bool = False):
    """An EXTENSION of the reference's surface: (paths, scores) -- paths a list of k Intervals (rank r: one interval list per
    chain, the type decode returns, None where chain c has fewer than r + 1 paths), scores a float32 numpy [k, nBatch].
    Arguments as viterbi_nbest_packed; every present path plugs into evalPath / logProb."""
    T, B = _check_inputs(score, noiseScore)
    pairs, offsets, scores, npaths = _nbest(score, noiseScore, k, forcedStartPos, forward)
    flat = unpack_intervals(torch.from_numpy(pairs), torch.from_numpy(offsets), T)
    k = scores.shape[0]
    paths = [[flat[r * B + c] if r < npaths[c] else None for c in range(B)] for r in range(k)]
    return paths, scores


# --------------------------------------------------------------------------------------
# posterior marginals and path entropy (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

Posteriors = namedtuple("Posteriors", "logZ entropy node begin end single noise")
Posteriors.__doc__ = """Posterior summaries of every chain (float32, where the scores live; include/semicrf_hip.h: semicrf_posteriors).
    logZ [B]; entropy [B]: the entropy of p(path) in nats; node [T, B]: P(frame t is not strictly inside an interval);
    begin / end [T, B]: P(an interval of length > 1 begins / ends at t); single [T, B]: P(the singleton (t, t));
    noise [T-1, B]: P(no interval covers the gap between t and t+1)."""


def _beta_raw(score_c, noise_c):
    T, B = score_c.shape[0], score_c.shape[2]
    q = torch.empty(T, B, dtype=torch.float32, device=score_c.device)
    ws = _lib.leased_workspace(_lib.OP_LOGZ_FWD, T, B, score_c.device, "beta")
    _lib.ops().beta(score_c, noise_c, q, ws)
    return q


def _alpha_from_raw(score_c, noise_c, start):
    """(logZ_s [B], alpha_s [T, B]) of semicrf_alpha_from: the alpha sweep of the model restricted to the frames start[c] .. T-1
    (start: int32 [B] where the scores live); alpha_s is -inf before the start.  Enqueued on the current stream, no workspace."""
    T, B = score_c.shape[0], score_c.shape[2]
    logz = torch.empty(B, dtype=torch.float32, device=score_c.device)
    v = torch.empty(T, B, dtype=torch.float32, device=score_c.device)
    _lib.ops().alpha_from(score_c, noise_c, start, v, logz, torch.empty(0, dtype=torch.uint8, device=score_c.device))
    return logz, v


def _marginal_inputs_from(score_c, noise_c, start):
    """(logZ_s, alpha_s, q) of the model that starts chain c at frame start[c]: the forced-start alpha sweep and the ordinary beta
    sweep (q[t] depends on the frames >= t only, so it is the conditional model's beta as it stands).  With these in the place
    of _marginal_inputs' triple every posterior kernel describes the conditional model: alpha_s = -inf before the start makes each
    marginal there an exact 0."""
    logz, v = _alpha_from_raw(score_c, noise_c, start)
    return logz, v, _beta_raw(score_c, noise_c)


def _marginal_inputs(score_c, noise_c, start=None):
    """(logZ, v, q) of the alpha and beta sweeps, enqueued on the current stream.  start (int32 [B] on the device): from a forced
    start, _marginal_inputs_from."""
    if start is not None:
        return _marginal_inputs_from(score_c, noise_c, start)
    logz, v = _logz_fwd_raw(score_c, noise_c, want_v=True)
    return logz, v, _beta_raw(score_c, noise_c)


def _start_arg(forcedStartPos, T: int, B: int, device, name: str):
    """The forcedStartPos keyword of the posterior calls -> None or an int32 vector [B] where the scores live.  A sequence of B
    ints is checked like decode's (IndexError for a wrong length or a frame outside [0, T-1], TypeError for anything but ints); an
    int32 tensor [B] is taken as it is and NOT range-checked (that would synchronise): a start out of range gives NaN for its chain."""
    if forcedStartPos is None:
        return None
    if isinstance(forcedStartPos, torch.Tensor):
        if forcedStartPos.dtype != torch.int32 or tuple(forcedStartPos.shape) != (B,):
            raise TypeError(f"{name}: a forcedStartPos tensor must be int32 of shape [{B}], got {forcedStartPos.dtype} "
                            f"{tuple(forcedStartPos.shape)}")
        return forcedStartPos.detach().to(device).contiguous()
    st = list(forcedStartPos)
    if len(st) != B:
        raise IndexError(f"{name}: forcedStartPos holds {len(st)} entries for {B} chains")
    if not all(isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)) for x in st):
        raise TypeError(f"{name}: forcedStartPos must hold ints (frames), got {forcedStartPos!r}")
    return _start_tensor(st, T, B, device)


def _posteriors_raw(score_c, noise_c, lvq=None, start=None) -> Posteriors:
    """Enqueue the sweeps (unless lvq = (logZ, v, q) is given; from `start` when that is given) and semicrf_posteriors; no host sync."""
    if _odd_pad(score_c) and lvq is None:
        P = _posteriors_raw(_pad1(score_c), _pad1(noise_c), None, _pad1(start) if start is not None else None)
        return Posteriors(*(x[..., :-1].contiguous() for x in P))
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    logz, v, q = _marginal_inputs(score_c, noise_c, start) if lvq is None else lvq
    f = dict(dtype=torch.float32, device=dev)
    node, begin, end, single = (torch.empty(T, B, **f) for _ in range(4))
    noise, entropy = torch.empty(T - 1, B, **f), torch.empty(B, **f)
    ws = _lib.workspace(_lib.OP_POSTERIORS, T, B, dev)
    _lib.ops().posteriors(score_c, noise_c, v, q, logz, node, begin, end, single, noise, entropy, ws)
    return Posteriors(logz, entropy, node, begin, end, single, noise)


def _tolerance(tolerance, name: str) -> Tuple[int, int]:
    """The `tolerance` keyword of the posterior calls -> (onset, offset) in frames: None is (0, 0), an int t is (t, t), a pair of
    ints is taken as it is; each in 0 .. 8 (SEMICRF_TOL_MAX).  Anything else (bool, float, negative, > 8, wrong length): ValueError."""
    if tolerance is None:
        return 0, 0
    is_int = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))
    if is_int(tolerance):
        pair = (int(tolerance), int(tolerance))
    elif isinstance(tolerance, (tuple, list)) and len(tolerance) == 2 and all(is_int(x) for x in tolerance):
        pair = (int(tolerance[0]), int(tolerance[1]))
    else:
        raise ValueError(f"{name}: tolerance must be None, an int or a pair (onset, offset) of ints in 0..{_lib.TOL_MAX} (frames), "
                         f"got {tolerance!r}")
    if not all(0 <= x <= _lib.TOL_MAX for x in pair):
        raise ValueError(f"{name}: tolerance must lie in 0..{_lib.TOL_MAX} frames, got {tolerance!r}")
    return pair


def _interval_marginals_raw(score_c, v, q, logz, pairs, K: int, offsets, tol: Tuple[int, int] = (0, 0), start=None):
    """start (int32 per chain of `offsets`, or None): with a tolerance an interval with begin < start is given an exact 0 here -- its
    box still holds cells at or behind the start, but the model from the start has no such interval (without a tolerance alpha =
    -inf before the start makes the kernel's own value the exact 0)."""
    out = torch.empty(max(K, 1), dtype=torch.float32, device=score_c.device)
    if tol == (0, 0):
        _lib.ops().interval_marginals(score_c, v, q, logz, pairs, int(K), offsets, out)
    else:
        _lib.ops().interval_marginals_tol(score_c, v, q, logz, pairs, int(K), offsets, tol[0], tol[1], out)
        if start is not None and K > 0:
            before = pairs[:K, 0] < start.index_select(0, _chain_of_rows(offsets, K))
            out = torch.where(before, torch.zeros_like(out[:K]), out[:K])
    return out[:K]


def _packed_on(pairs, offsets, T: int, B: int, device):
    """decode_packed's arrays (numpy or tensors) -> (pairs int32 [K,2], offsets int32 [B+1], K) on `device`; host arrays are
    checked with pack_intervals' errors, device tensors by the kernel (an index out of range gives NaN)."""
    on_dev = isinstance(pairs, torch.Tensor) and isinstance(offsets, torch.Tensor) and pairs.device.type != "cpu"
    p = pairs if isinstance(pairs, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pairs))
    o = offsets if isinstance(offsets, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(offsets))
    assert o.dim() == 1 and o.numel() == B + 1, f"expected offsets of {B + 1} entries, got {tuple(o.shape)}"
    p = p.reshape(-1, 2).to(torch.int32)
    o = o.to(torch.int32)
    K = int(p.shape[0])
    if not on_dev:
        pn, on = p.numpy(), o.numpy()
        if on[0] != 0 or on[-1] != K or (np.diff(on) < 0).any():
            raise ValueError("offsets not ascending or not matching the interval count")
        if K and ((pn < 0).any() or (pn >= T).any()):
            raise IndexError(f"interval index out of range for T={T}")
    pin = torch.device(device).type == "cuda" and not on_dev
    if pin:
        p, o = p.pin_memory(), o.pin_memory()
    return p.contiguous().to(device, non_blocking=True), o.contiguous().to(device, non_blocking=True), K


def posteriors(score, noiseScore, forcedStartPos=None) -> Posteriors:
    """An EXTENSION of the reference's surface: posterior marginals and path entropy of every chain, as a Posteriors namedtuple
    (logZ, entropy, node, begin, end, single, noise) of float32 tensors where the scores live -- without the dense [T, T, B]
    marginal tensor of forward_backward and without a host sync.  Runs the alpha and beta sweeps itself; no gradient.

    forcedStartPos: None, or one start frame per chain as decode takes it (a sequence of nBatch ints, IndexError when out of range;
    or an int32 tensor [nBatch] where the scores live, not range-checked).  The result then describes the model restricted to
    the frames start .. T-1 of each chain, the one whose MAP path decode(forcedStartPos) returns: logZ is that model's, entropy
    its path entropy, and node / begin / end / single / noise are exactly 0 before the start."""
    T, B = _check_inputs(score, noiseScore)
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        return _posteriors_raw(score_c, noise_c, None, _start_arg(forcedStartPos, T, B, score_c.device, "posteriors"))


def interval_marginals_packed(score, noiseScore, pairs, offsets, tolerance=None, forcedStartPos=None) -> torch.Tensor:
    """An EXTENSION of the reference's surface: the posterior probability of each given interval, a float32 tensor [K] where the
    scores live.  pairs [K, 2] (begin, end) and offsets [nBatch + 1] as decode_packed returns them (numpy arrays or tensors).

    tolerance: None, an int t (meaning (t, t)) or a pair (onset, offset) of ints in 0..8, in frames.  With a tolerance (db, de) the
    value of (b, e) is M = min(1, the sum of the exact-cell probabilities over the box |b' - b| <= db, |e' - e| <= de): the expected
    number of path intervals that match (b, e) within the tolerance -- for e - b > db + de the probability that one does, the
    quantity a note-level metric with an onset / offset window asks for (include/semicrf_hip.h: semicrf_interval_marginals_tol).
    None and (0, 0) are the exact-cell probabilities.

    forcedStartPos: as posteriors (None, nBatch ints or an int32 tensor [nBatch]): the probabilities under the model that starts
    chain c at that frame; an interval with begin < start has probability exactly 0 (with a tolerance: the cells of its box at or
    behind the start still count)."""
    T, B = _check_inputs(score, noiseScore)
    tol = _tolerance(tolerance, "interval_marginals")
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        start = _start_arg(forcedStartPos, T, B, score_c.device, "interval_marginals")
        p, o, K = _packed_on(pairs, offsets, T, B, score_c.device)
        if _odd_pad(score_c):
            s2, n2 = _pad1(score_c), _pad1(noise_c)
            st2 = _pad1(start) if start is not None else None
            logz, v, q = _marginal_inputs(s2, n2, st2)
            return _interval_marginals_raw(s2, v, q, logz, p, K, torch.cat([o, o[-1:]]), tol, st2)
        logz, v, q = _marginal_inputs(score_c, noise_c, start)
        return _interval_marginals_raw(score_c, v, q, logz, p, K, o, tol, start)


def interval_marginals(score, noiseScore, intervals: Intervals, tolerance=None, forcedStartPos=None) -> List[List[float]]:
    """An EXTENSION of the reference's surface: the posterior probability of each interval of `intervals` (one list per chain,
    e.g. what decode returns), as a list (len nBatch) of lists of floats in the given order.  tolerance: as
    interval_marginals_packed (None, an int or a pair (onset, offset) of frames in 0..8): the probability that the path holds an
    interval within that many frames of the given one.  forcedStartPos: as interval_marginals_packed."""
    T, B = _check_inputs(score, noiseScore)
    _tolerance(tolerance, "interval_marginals")
    pairs, offsets = pack_intervals(intervals, T, B, "cpu", ordered=False)
    K = pairs._semicrf_K
    out = interval_marginals_packed(score, noiseScore, pairs[:K], offsets, tolerance, forcedStartPos).cpu().tolist()
    off = offsets.tolist()
    return [out[off[c]:off[c + 1]] for c in range(B)]


# --------------------------------------------------------------------------------------
# posterior expectations, differentiable entropy, Hessian products of logZ (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

def _expect_workspace(T: int, B: int, device) -> torch.Tensor:
    """The float64 state semicrf_expectation leaves for semicrf_covariance (a fresh buffer: autograd may keep it)."""
    if torch.device(device).type == "cpu":
        return torch.empty((4 * T * B + 2 * B) * 8, dtype=torch.uint8)
    return _lib.workspace(_lib.OP_EXPECTATION, T, B, device)


def _expect_fwd(score_c, noise_c, weight_c, nweight_c):
    """Enqueue the alpha / beta sweeps and semicrf_expectation; no host sync.  weight_c may BE score_c (read once); nweight_c None:
    zeros.  Returns (E [B], H [B] = logZ - E, state); state feeds _expect_cov and _expect_marginals."""
    pad = _odd_pad(score_c)
    if pad:                                         # a single chain runs with a ghost chain, like every sweep
        same = weight_c is score_c
        nsame = nweight_c is noise_c
        score_c, noise_c = _pad1(score_c), _pad1(noise_c)
        weight_c = score_c if same else _pad1(weight_c)
        if nweight_c is not None:
            nweight_c = noise_c if nsame else _pad1(nweight_c)
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    logz, v, q = _marginal_inputs(score_c, noise_c)
    E = torch.empty(B, dtype=torch.float32, device=dev)
    H = torch.empty(B, dtype=torch.float32, device=dev)
    ws = _expect_workspace(T, B, dev)
    has_nw = nweight_c is not None
    _lib.ops().expectation(score_c, noise_c, weight_c, nweight_c if has_nw else _empty(dev), has_nw, v, q, E, H, ws)
    state = (score_c, noise_c, weight_c, nweight_c, ws, v, logz, pad)
    if pad:
        E, H = E[:-1].contiguous(), H[:-1].contiguous()
    return E, H, state


def _expect_cov(state, gout):
    """semicrf_covariance on the state of _expect_fwd: (gout * C [T,T,B], gout * Cn [T-1,B]); the upper triangle is exact zeros."""
    score_c, noise_c, weight_c, nweight_c, ws, _, _, pad = state
    if pad:
        gout = _pad1(gout)
    T, B = score_c.shape[0], score_c.shape[2]
    C = _empty_or_trim((T, T, B), score_c.device)
    Cn = torch.empty_like(noise_c)
    has_nw = nweight_c is not None
    _lib.ops().covariance(score_c, noise_c, weight_c, nweight_c if has_nw else _empty(score_c.device), has_nw, gout, C, Cn, ws)
    if pad:
        C, Cn = C[:, :, :-1].contiguous(), Cn[:, :-1].contiguous()
    return C, Cn


def _expect_marginals(state, gout):
    """gout * the marginals (the gradient of E with respect to weight / noiseWeight), by the existing gradient sweep."""
    score_c, noise_c, _, _, _, v, logz, pad = state
    if pad:
        gout = _pad1(gout)
    ds, dn, _ = _logz_bwd_raw(score_c, noise_c, v, logz, gout)
    if pad:
        ds, dn = ds[:, :, :-1].contiguous(), dn[:, :-1].contiguous()
    return ds, dn


def _check_weights(score, noiseScore, weight, noiseWeight):
    T, B = _check_inputs(score, noiseScore)
    assert tuple(weight.shape) == tuple(score.shape)
    _lib.require_device(weight, "weight")
    assert weight.device == score.device
    if noiseWeight is not None:
        assert tuple(noiseWeight.shape) == tuple(noiseScore.shape)
        _lib.require_device(noiseWeight, "noiseWeight")
        assert noiseWeight.device == score.device
    return T, B


class _Expectation(torch.autograd.Function):
    """E_p[W] (entropy False) or H = logZ - E_p[S] (entropy True; weight / noiseWeight are then ignored) as one node.  The
    backward is the covariance stream on the float64 state the forward left; it is once-differentiable."""

    @staticmethod
    def forward(ctx, score, noiseScore, weight, noiseWeight, entropy: bool):
        score_c, noise_c = _prep(score), _prep(noiseScore)
        if entropy:
            weight_c, nweight_c = score_c, noise_c
        else:
            weight_c = _prep(weight)
            nweight_c = _prep(noiseWeight) if noiseWeight is not None else None
        E, H, state = _expect_fwd(score_c, noise_c, weight_c, nweight_c)
        ctx.entropy = entropy
        ctx.has_nw = noiseWeight is not None
        ctx.in_dtypes = tuple(t.dtype if t is not None else None for t in (score, noiseScore, weight, noiseWeight))
        if any(ctx.needs_input_grad[:4]):
            ctx.state_meta = state[7]
            ctx.save_for_backward(*(t for t in state[:7] if t is not None))
        return H if entropy else E

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_output):
        saved = list(ctx.saved_tensors)
        if ctx.entropy or ctx.has_nw:
            score_c, noise_c, weight_c, nweight_c, ws, v, logz = saved
        else:
            score_c, noise_c, weight_c, ws, v, logz = saved
            nweight_c = None
        if weight_c.data_ptr() == score_c.data_ptr():
            weight_c = score_c                      # (saved tensors are unpacked as distinct objects)
        state = (score_c, noise_c, weight_c, nweight_c, ws, v, logz, ctx.state_meta)
        B = score_c.shape[2] - (1 if ctx.state_meta else 0)
        g = _gout(grad_output, B)
        ds = dn = dw = dnw = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            C, Cn = _expect_cov(state, -g if ctx.entropy else g)            # dH/dscore = -C with the weights = the scores
            ds = C.to(ctx.in_dtypes[0]) if ctx.needs_input_grad[0] else None
            dn = Cn.to(ctx.in_dtypes[1]) if ctx.needs_input_grad[1] else None
        if not ctx.entropy and (ctx.needs_input_grad[2] or (ctx.has_nw and ctx.needs_input_grad[3])):
            mw, mn = _expect_marginals(state, g)
            dw = mw.to(ctx.in_dtypes[2]) if ctx.needs_input_grad[2] else None
            dnw = mn.to(ctx.in_dtypes[3]) if ctx.has_nw and ctx.needs_input_grad[3] else None
        return ds, dn, dw, dnw, None


def expectation(score, noiseScore, weight, noiseWeight=None) -> torch.Tensor:
    """An EXTENSION of the reference's surface: E_p[W] of every chain (float32 [nBatch], where the scores live) for the additive
    path functional W(path) = sum of weight[end, begin] over the path's intervals (singletons included) + sum of noiseWeight[t]
    over the gaps no interval covers.  weight [T, T, nBatch] has the layout of score (only begin <= end is read), noiseWeight
    [T-1, nBatch] defaults to zeros.  Differentiable once: the gradients to score / noiseScore are the covariances
    Cov(1[cell on path], W) (see covariance), those to weight / noiseWeight the marginals of forward_backward; a second
    differentiation raises.  Without a gradient no dense [T, T, nBatch] tensor is allocated.  No host sync."""
    _check_weights(score, noiseScore, weight, noiseWeight)
    return _Expectation.apply(score, noiseScore, weight, noiseWeight, False)


def entropy(score, noiseScore) -> torch.Tensor:
    """An EXTENSION of the reference's surface: the entropy H = logZ - E_p[score of the path] of p(path) in nats, float32 [nBatch],
    differentiable once (dH/dscore = -Cov(1[cell on path], S)): an entropy regulariser, minimum-entropy training, a confidence
    penalty.  posteriors().entropy is the same number without a gradient."""
    _check_inputs(score, noiseScore)
    return _Expectation.apply(score, noiseScore, None, None, True)


def covariance(score, noiseScore, weight, noiseWeight=None):
    """An EXTENSION of the reference's surface: (E [nBatch], C [T, T, nBatch], Cn [T-1, nBatch]) with E = E_p[W] as expectation,
    C[end, begin] = Cov(1[(begin, end) on path], W) (exact zeros for begin > end) and Cn[t] = Cov(1[gap t is noise], W): the
    product of the Hessian of logZ with (weight, noiseWeight), i.e. the explicit second-order route (the reference's computeLogZ
    is plain torch and can be differentiated twice; computeLogZ here cannot).  float32 where the scores live; no gradient."""
    _check_weights(score, noiseScore, weight, noiseWeight)
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        same = weight is score
        weight_c = score_c if same else _prep(weight.detach())
        nweight_c = None if noiseWeight is None else (noise_c if noiseWeight is noiseScore else _prep(noiseWeight.detach()))
        E, _, state = _expect_fwd(score_c, noise_c, weight_c, nweight_c)
        C, Cn = _expect_cov(state, torch.ones(E.shape[0], dtype=torch.float32, device=E.device))
    return E, C, Cn


# --------------------------------------------------------------------------------------
# marginal-threshold (posterior) decoding (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

def _marginal_decode_raw(score_c, noise_c, tau, cap: Optional[int] = None, lvq=None, tol: Tuple[int, int] = (0, 0), start=None):
    """Enqueue the sweeps (unless lvq = (logZ, v, q) is given) and semicrf_marginal_decode (semicrf_marginal_decode_tol for a
    tolerance tol = (onset, offset) other than (0, 0)); no host sync.  tau: a float32 tensor of 1 value or one per chain, where the
    scores live.  Returns device tensors (pairs [cap, 2], offsets [B+1], probs [cap]); offsets is exact even past cap (default 2 T
    per chain: the bound for a threshold > 0.5 without a tolerance).  start (int32 [B] on the device, or None): the sweeps run from
    that forced start (_marginal_inputs_from)."""
    if _odd_pad(score_c) and lvq is None:
        t2 = tau if tau.numel() == 1 else torch.cat([tau, tau.new_full((1,), float("inf"))])     # the ghost chain selects nothing
        st2 = _pad1(start) if start is not None else None
        pairs, offsets, probs = _marginal_decode_raw(_pad1(score_c), _pad1(noise_c), t2, cap, None, tol, st2)
        return pairs, offsets[:-1], probs  # the ghost chain is last: its intervals lie behind offsets[B]
    T, B = score_c.shape[0], score_c.shape[2]
    dev = score_c.device
    logz, v, q = _marginal_inputs(score_c, noise_c, start) if lvq is None else lvq
    cap = max(int(cap), 1) if cap is not None else 2 * T * B
    pairs = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    probs = torch.empty(cap, dtype=torch.float32, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int32, device=dev)
    if tol == (0, 0):
        ws = _lib.workspace(_lib.OP_MARGINAL_DECODE, T, B, dev)
        _lib.ops().marginal_decode(score_c, noise_c, v, q, logz, tau, pairs, probs, offsets, ws)
    else:
        ws = _lib.workspace(_lib.OP_MARGINAL_DECODE_TOL, T, B, dev)
        _lib.ops().marginal_decode_tol(score_c, noise_c, v, q, logz, tau, tol[0], tol[1], pairs, probs, offsets, ws)
        if start is not None:
            return _drop_before_start(pairs, offsets, probs, start)
    return pairs, offsets, probs


def _chain_of_rows(offsets, n: int):
    """The chain of each of the first n rows of a packed list (rows behind offsets[B] get the last chain); no host sync."""
    B = offsets.shape[0] - 1
    rows = torch.arange(n, device=offsets.device)
    return torch.bucketize(rows, offsets[1:].long(), right=True).clamp_(max=B - 1)


def _drop_before_start(pairs, offsets, probs, start):
    """A tolerance-aware lattice from a forced start: the box of a cell with begin < start still holds cells at or behind the
    start, so semicrf_marginal_decode_tol (which knows nothing of the start) can select it; the model has no such interval.  Drops
    those rows and packs the rest in order, on the device and without a host sync (a prefix sum over the rows).
    The kernel's markers in offsets[B] are handed on untouched: -1 (alpha's last row holds NaN: the result is invalid) and a count
    > cap (a truncated lattice: the count is the size to come back with).  In both cases the ORIGINAL offsets are returned next to
    the filtered pairs / probs, which then do not belong together -- that is harmless only because nothing reads such a result:
    every caller raises on the first and retries on the second."""
    cap, B = pairs.shape[0], offsets.shape[0] - 1
    total = offsets[-1]
    rows = torch.arange(cap, device=pairs.device)
    chain = _chain_of_rows(offsets, cap)
    keep = (rows < total) & (pairs[:, 0] >= start.index_select(0, chain))
    dest = torch.where(keep, torch.cumsum(keep, 0) - 1, torch.full_like(rows, cap))      # dropped rows land in a spare last row
    pairs_f = torch.empty(cap + 1, 2, dtype=pairs.dtype, device=pairs.device).index_copy_(0, dest, pairs)[:cap]
    probs_f = torch.empty(cap + 1, dtype=probs.dtype, device=probs.device).index_copy_(0, dest, probs)[:cap]
    counts = torch.zeros(B + 1, dtype=torch.int64, device=pairs.device).index_add_(0, chain + 1, keep.long())
    offsets_f = torch.cumsum(counts, 0).to(offsets.dtype)
    fits = (total >= 0) & (total <= cap)
    return pairs_f, torch.where(fits, offsets_f, offsets), probs_f


def _threshold_tensor(threshold, B: int, device, name: str = "decode_marginal") -> torch.Tensor:
    if isinstance(threshold, torch.Tensor):
        if not threshold.is_floating_point() or tuple(threshold.shape) != (B,):
            raise ValueError(f"{name}: a threshold tensor must be floating point of shape [{B}] (one value per chain), "
                             f"got {threshold.dtype} {tuple(threshold.shape)}")
        return threshold.detach().to(device=device, dtype=torch.float32).contiguous()       # not range-checked: that would synchronise
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating, np.integer)):
        raise ValueError(f"{name}: threshold must be a float in (0, 1] or a float tensor [nBatch], got {threshold!r}")
    t = float(threshold)
    if not (0.0 < t <= 1.0):                   # NaN fails both comparisons
        raise ValueError(f"{name}: threshold must be in (0, 1], got {threshold!r}")
    return torch.full((1,), t, dtype=torch.float32, device=device)


def decode_marginal_packed(score, noiseScore, threshold, tolerance=None, forcedStartPos=None):
    """An EXTENSION of the reference's surface: every interval whose posterior probability P((begin, end) on the path | score) is
    >= threshold, as host arrays like decode_packed plus the probabilities: (pairs int32 [K, 2], offsets int32 [nBatch + 1],
    probs float32 [K]); chain c owns pairs[offsets[c]:offsets[c + 1]], ascending by (begin, end).  probs are the values
    interval_marginals returns for those intervals, bit for bit.

    threshold: a Python float in (0, 1], or a float tensor [nBatch] (one threshold per chain; not range-checked).  There is no
    default: 0.5 is exactly where ties sit and the caller should choose a side.  For threshold > 0.5 the intervals of a chain
    cannot overlap (overlapping intervals never share a path, so their probabilities sum to <= 1): the result is a path that
    plugs into evalPath / logProb, the minimum-Bayes-risk decision for the gain (1 - threshold) per correct and -threshold per
    wrong interval; for threshold <= 0.5 it is a candidate lattice that may overlap.  Runs the alpha and beta sweeps itself,
    never builds the dense [T, T, nBatch] marginal tensor; one host sync; no gradient.

    tolerance: None, an int t (meaning (t, t)) or a pair (onset, offset) of ints in 0..8, in frames; None and (0, 0) are the call
    above, unchanged.  With a tolerance the compared and returned value is interval_marginals(..., tolerance)'s M (bit for bit):
    every interval that the path matches within the tolerance with probability >= threshold.  That set is NO LONGER a path, even
    for threshold > 0.5 -- the neighbours of a confident interval pass together with it (up to (2 onset + 1)(2 offset + 1) cells
    per note): it is a lattice, and decode_mbr(threshold, tolerance) is the call that returns one path.  A single chain runs with a
    ghost chain appended, as without a tolerance; the ghost's cells never show.

    forcedStartPos: as posteriors (None, nBatch ints or an int32 tensor [nBatch]): the probabilities are those of the model that
    starts chain c at that frame; only intervals with begin >= start are returned, and probs stay interval_marginals(...,
    forcedStartPos=...)'s values bit for bit."""
    T, B = _check_inputs(score, noiseScore)
    tol = _tolerance(tolerance, "decode_marginal")
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        tau = _threshold_tensor(threshold, B, score_c.device)
        start = _start_arg(forcedStartPos, T, B, score_c.device, "decode_marginal")
        lvq = None if _odd_pad(score_c) else _marginal_inputs(score_c, noise_c, start)    # (a single chain: the raw call pads and sweeps)
        pairs, offsets, probs = _marginal_decode_raw(score_c, noise_c, tau, None, lvq, tol, start)
        off_h = offsets.cpu()                      # the one host sync
        if int(off_h[-1]) > pairs.shape[0]:
            # more cells than 2 T per chain (a threshold <= 0.5, a tolerance): once more with the exact size -- never a silent truncation
            pairs, offsets, probs = _marginal_decode_raw(score_c, noise_c, tau, int(off_h[-1]), lvq, tol, start)
            off_h = offsets.cpu()
        total = int(off_h[-1])
        if total < 0:
            _lib.async_error()                     # consumed here: the next call must not report this time-out again
            raise RuntimeError("semicrf_marginal_decode: alpha holds NaN in its last row -- the inputs hold NaN (or -inf cells, which "
                               "the device's forward sweep does not take), or a bounded hand-off wait of the sweep timed out on the "
                               "device (GPU shared with work that kept part of the persistent kernel from running?); the result is invalid")
        return pairs[:total].cpu().numpy(), off_h.numpy(), probs[:total].cpu().numpy()


def decode_marginal(score, noiseScore, threshold, tolerance=None, forcedStartPos=None):
    """An EXTENSION of the reference's surface: (paths, probs) -- paths an Intervals (per chain the list of (begin, end) whose
    posterior probability is >= threshold, ascending by (begin, end): the type decode returns), probs per chain the list of those
    probabilities.  Arguments and properties as decode_marginal_packed (with a tolerance the lists are a lattice, not a path)."""
    T, B = _check_inputs(score, noiseScore)
    pairs, offsets, probs = decode_marginal_packed(score, noiseScore, threshold, tolerance, forcedStartPos)
    paths = unpack_intervals(torch.from_numpy(pairs), torch.from_numpy(offsets), T)
    pl, off = probs.tolist(), offsets.tolist()
    return paths, [pl[off[c]:off[c + 1]] for c in range(B)]


# --------------------------------------------------------------------------------------
# MBR path decoding at any threshold (an extension of the reference's surface)
# --------------------------------------------------------------------------------------

def _mbr_select_raw(pairs, probs, offsets, T: int, tau):
    """Enqueue semicrf_mbr_select on a device lattice (_marginal_decode_raw's result); no host sync.  Returns device tensors
    (pairs [2 T B, 2], offsets [B+1], probs [2 T B], gain [B]); offsets[B] = -1 when the lattice is truncated or invalid."""
    B = offsets.shape[0] - 1
    dev = offsets.device
    cap = 2 * T * B                                # a path has at most 2 T - 1 cells
    pairs_out = torch.empty(cap, 2, dtype=torch.int32, device=dev)
    probs_out = torch.empty(cap, dtype=torch.float32, device=dev)
    offsets_out = torch.empty(B + 1, dtype=torch.int32, device=dev)
    gain = torch.empty(B, dtype=torch.float32, device=dev)
    ws = _lib.workspace(_lib.OP_MBR_SELECT, T, B, dev)
    _lib.ops().mbr_select(pairs, probs, offsets, T, tau, pairs_out, probs_out, offsets_out, gain, ws)
    return pairs_out, offsets_out, probs_out, gain


def _mbr_decode_raw(score_c, noise_c, tau, threshold, tol: Tuple[int, int] = (0, 0), start=None, retry: bool = True):
    """The device part of decode_mbr: the sweeps (from `start`, int32 [B] on the device, when given), semicrf_marginal_decode(_tol)
    into a device lattice and semicrf_mbr_select on it.  Returns (pairs [2 T B, 2], offsets [B+1], probs [2 T B], gain [B],
    offsets_host): four device tensors and the host copy of the offsets (None with retry=False); offsets[B] = -1 marks an invalid
    result.
    tau: the float32 threshold tensor (1 value or one per chain); threshold: the caller's scalar (a Python float: it sizes the
    lattice) or anything else (a tensor: 2 T cells per chain).  Without a tolerance and with a scalar threshold the lattice bound
    (floor(1 / threshold) + 1) T cells per chain is exact -- nothing can be truncated -- and retry=False enqueues everything
    without a host sync.  retry=True reads the offsets once (the one host sync; returned as the fifth element) and, where the
    lattice did not fit, runs both kernels once more with the exact size: never a silent truncation."""
    T, B = score_c.shape[0], score_c.shape[2]
    pad = _odd_pad(score_c)
    lvq = None if pad else _marginal_inputs(score_c, noise_c, start)
    nB = B + 1 if pad else B                   # (a single chain: the raw call pads and sweeps; the ghost's cells come last)
    if not isinstance(threshold, (int, float, np.floating, np.integer)):
        cap = 2 * T * nB
    elif tol != (0, 0):
        # a box holds up to 2 (2 db + 1)(2 de + 1) of mass per begin (every column of it <= 1 in intervals + 1 as a singleton,
        # every cell in 2 de + 1 boxes of a begin): at most that / tau cells per begin, or the whole column; start from 2 T per
        # chain when that is smaller (it is, for every tolerance > 0 and T > 4) and let the retry below take the exact count
        per_begin = int(2 * (2 * tol[0] + 1) * (2 * tol[1] + 1) / float(threshold)) + 1
        cap = min(min(per_begin * T, T * (T + 1) // 2), 2 * T) * nB
    else:                                      # sum_{e > b} m(e, b) <= 1: at most floor(1 / tau) + 1 cells per begin
        cap = min((int(1.0 / float(threshold)) + 1) * T, T * (T + 1) // 2) * nB
    lat = _marginal_decode_raw(score_c, noise_c, tau, cap, lvq, tol, start)
    pairs, offsets, probs, gain = _mbr_select_raw(lat[0], lat[2], lat[1], T, tau)
    off_h = None
    if retry:
        off_h = offsets.cpu()                  # the one host sync
        if int(off_h[-1]) < 0:
            lat_total = int(lat[1][-1])
            if lat_total > lat[0].shape[0]:
                # the lattice did not fit (a threshold tensor with small values, a tolerance): once more with the exact size -- never
                # a silent truncation
                lat = _marginal_decode_raw(score_c, noise_c, tau, lat_total + (cap // nB if pad else 0), lvq, tol, start)
                pairs, offsets, probs, gain = _mbr_select_raw(lat[0], lat[2], lat[1], T, tau)
                off_h = offsets.cpu()
    return pairs, offsets, probs, gain, off_h


def decode_mbr_packed(score, noiseScore, threshold, tolerance=None, forcedStartPos=None):
    """An EXTENSION of the reference's surface: the minimum-Bayes-risk PATH for the gain (1 - threshold) per correct and -threshold
    per wrong interval, at ANY threshold: among all paths of a chain the one that maximises the sum over its intervals of
    (P((begin, end) on the path | score) - threshold).  Returns host arrays (pairs int32 [K, 2], offsets int32 [nBatch + 1], probs
    float32 [K], gain float32 [nBatch]): chain c owns pairs[offsets[c]:offsets[c + 1]], ascending by (begin, end) -- always a path
    that plugs into evalPath / logProb -- probs are those intervals' posterior probabilities (interval_marginals' values, bit for
    bit) and gain[c] the maximised sum.  For threshold > 0.5 it is decode_marginal_packed's set without the probabilities equal to
    the threshold; below, where that set is a lattice that may overlap, this is the consistent decision (lower the threshold for
    recall).

    threshold: as decode_marginal_packed (a Python float in (0, 1] or a float tensor [nBatch], not range-checked).  Runs the alpha
    and beta sweeps once, semicrf_marginal_decode into a device lattice and semicrf_mbr_select on it; never builds a dense
    [T, T, nBatch] tensor; one host sync; no gradient.

    tolerance: None, an int t (meaning (t, t)) or a pair (onset, offset) of ints in 0..8, in frames; None and (0, 0) are the call
    above, unchanged.  With a tolerance the lattice is semicrf_marginal_decode_tol's and the recursion is the same: the path
    maximises the sum over its intervals of (M - threshold), M = interval_marginals(..., tolerance)'s value -- the probability that
    the true path holds an interval within the tolerance of the chosen one -- and probs are the M of its intervals, bit for bit.
    This is the call that turns the tolerance-aware set of decode_marginal (a lattice: neighbouring cells pass together) into one
    path: a note whose onset the model spreads over two frames is returned once, with the probability of the pair.  A single chain
    runs with a ghost chain appended, as without a tolerance.

    forcedStartPos: as posteriors (None, nBatch ints or an int32 tensor [nBatch]): the MBR path of the model that starts chain c at
    that frame -- the posterior counterpart of decode(forcedStartPos); every returned interval has begin >= start."""
    T, B = _check_inputs(score, noiseScore)
    tol = _tolerance(tolerance, "decode_mbr")
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        tau = _threshold_tensor(threshold, B, score_c.device, "decode_mbr")
        start = _start_arg(forcedStartPos, T, B, score_c.device, "decode_mbr")
        pairs, offsets, probs, gain, off_h = _mbr_decode_raw(score_c, noise_c, tau, threshold, tol, start)     # (its one host sync)
        total = int(off_h[-1])
        if total < 0:
            _lib.async_error()                     # consumed here: the next call must not report this time-out again
            raise RuntimeError("semicrf_mbr_select: alpha holds NaN in its last row -- the inputs hold NaN (or -inf cells, which "
                               "the device's forward sweep does not take), or a bounded hand-off wait of the sweep timed out on the "
                               "device (GPU shared with work that kept part of the persistent kernel from running?); the result is invalid")
        return pairs[:total].cpu().numpy(), off_h.numpy(), probs[:total].cpu().numpy(), gain.cpu().numpy()


def decode_mbr(score, noiseScore, threshold, tolerance=None, forcedStartPos=None):
    """An EXTENSION of the reference's surface: (paths, probs, gain) -- paths an Intervals (per chain the minimum-Bayes-risk path
    at `threshold`, the type decode returns), probs per chain the list of its intervals' posterior probabilities, gain a float32
    numpy [nBatch].  Arguments and properties as decode_mbr_packed (tolerance: the onset / offset window in frames)."""
    T, B = _check_inputs(score, noiseScore)
    pairs, offsets, probs, gain = decode_mbr_packed(score, noiseScore, threshold, tolerance, forcedStartPos)
    paths = unpack_intervals(torch.from_numpy(pairs), torch.from_numpy(offsets), T)
    pl, off = probs.tolist(), offsets.tolist()
    return paths, [pl[off[c]:off[c + 1]] for c in range(B)], gain


# --------------------------------------------------------------------------------------
# path comparison: decoded paths against target paths (the counts of the reference's computeStats)
# --------------------------------------------------------------------------------------

# column indices of the [nBatch, 7] tensor the comparison returns: stats[:, PathStats.nExact]
PathStats = namedtuple("PathStats", "nRef nEst nExact nRefFrames nEstFrames nBothFrames nMatchTol")(*range(7))


def _compare_paths_raw(est_pairs, est_offsets, ref_pairs, ref_offsets, T: int, tol: Tuple[int, int]):
    """Enqueue semicrf_compare_paths on packed int32 tensors of one device; no host sync.  Returns stats int32 [B, 7]."""
    B = est_offsets.shape[0] - 1
    stats = torch.empty(B, 7, dtype=torch.int32, device=est_offsets.device)
    _lib.ops().compare_paths(est_pairs, est_offsets, ref_pairs, ref_offsets, int(T), tol[0], tol[1], stats)
    return stats


def _packed_list(pairs, offsets, side: str):
    """One packed list of compare_paths_packed as it is: int32, contiguous, pairs [K, 2] 8-byte aligned -- nothing is converted or
    copied (a conversion would hide a wrong buffer, and a copy of a device tensor is a launch)."""
    p = torch.from_numpy(pairs) if isinstance(pairs, np.ndarray) else pairs
    o = torch.from_numpy(offsets) if isinstance(offsets, np.ndarray) else offsets
    for t, name in ((p, f"{side}_pairs"), (o, f"{side}_offsets")):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"compare_paths: {name} must be a tensor or a numpy array, got {type(t).__name__}")
        if t.dtype != torch.int32:
            raise TypeError(f"compare_paths: {name} must be int32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"compare_paths: {name} must be contiguous")
        _lib.require_device(t, name)
    if p.dim() != 2 or p.shape[1] != 2:
        raise ValueError(f"compare_paths: {side}_pairs must be [K, 2], got {tuple(p.shape)}")
    if o.dim() != 1 or o.numel() < 2:
        raise ValueError(f"compare_paths: {side}_offsets must be [nBatch + 1], got {tuple(o.shape)}")
    if p.numel() and p.data_ptr() % 8:
        raise ValueError(f"compare_paths: {side}_pairs must be 8-byte aligned (every pair is one 8-byte load)")
    if p.device != o.device:
        raise ValueError(f"compare_paths: {side}_pairs and {side}_offsets are on different devices")
    if p.is_cuda:
        # the total lives on the device and the kernel reads pairs[: total]: a total beyond the buffer becomes the invalid marker
        o = torch.where(o[-1:] > p.shape[0], torch.full_like(o, -1), o)
    return p, o


def compare_paths_packed(est_pairs, est_offsets, ref_pairs, ref_offsets, T: int, tolerance=None) -> torch.Tensor:
    """An EXTENSION of the reference's surface: per chain the counts that note-level and frame-level precision / recall are made
    of, an int32 tensor [nBatch, 7] on the inputs' device with the columns of PathStats:

      nRef, nEst                            the lengths of the two lists
      nExact                                pairs present in both -- compareBracket's nCorrect (Evaluation.py:10-18)
      nRefFrames, nEstFrames, nBothFrames   compareFramewise(est, ref) (Evaluation.py:67-74), bit for bit
      nMatchTol                             the largest number of estimate / reference pairs that can be matched one to one with
                                            onsets within tolerance[0] and offsets within tolerance[1] frames; nExact at (0, 0)

    est_* and ref_* are packed lists as decode_packed returns them (pairs int32 [K, 2], offsets int32 [nBatch + 1]; tensors or
    numpy arrays, all on one device, contiguous, pairs 8-byte aligned: TypeError / ValueError otherwise, before anything is
    launched).  T: the number of frames.  tolerance: None, an int or a pair (onset, offset) of ints in 0..8, as decode_mbr takes it.

    The lists are checked where they live: a chain with an index outside [0, T), begin > end or a begin or end that decreases
    along the list has all seven entries -1; a negative offsets[-1] (the marker a decode leaves when it gave up) makes every
    entry -1.  Never synchronises: on the GPU one kernel (semicrf_compare_paths), on the CPU the host kernel of the same contract."""
    tol = _tolerance(tolerance, "compare_paths")
    T = int(T)
    if T < 1:
        raise ValueError(f"compare_paths: T must be >= 1, got {T}")
    with torch.no_grad():
        ep, eo = _packed_list(est_pairs, est_offsets, "est")
        rp, ro = _packed_list(ref_pairs, ref_offsets, "ref")
        if eo.shape != ro.shape:
            raise ValueError(f"compare_paths: the two lists hold {eo.numel() - 1} and {ro.numel() - 1} chains")
        if ep.device != rp.device:
            raise ValueError("compare_paths: the two lists are on different devices")
        return _compare_paths_raw(ep, eo, rp, ro, T, tol)


def compare_paths(est: Intervals, ref: Intervals, T: int, tolerance=None) -> torch.Tensor:
    """compare_paths_packed on Python lists (what decode returns and what logProb takes): packs both with
    pack_intervals(..., ordered=True) -- IndexError / ValueError for an index outside [0, T) or begin > end -- and returns the
    int32 [nBatch, 7] tensor on the CPU, where the lists are (the host kernel)."""
    tol = _tolerance(tolerance, "compare_paths")
    assert len(est) == len(ref), f"{len(est)} estimated lists against {len(ref)} reference lists"
    B = len(est)
    ep, eo = pack_intervals(est, int(T), B, "cpu", ordered=True)
    rp, ro = pack_intervals(ref, int(T), B, "cpu", ordered=True)
    with torch.no_grad():
        return _compare_paths_raw(ep, eo, rp, ro, int(T), tol)


def decode_stats(score, noiseScore, intervals: Intervals, forcedStartPos=None, forward: bool = False, tolerance=None) -> torch.Tensor:
    """An EXTENSION of the reference's surface: decode(forcedStartPos, forward) compared with the target `intervals`, as
    compare_paths_packed's int32 [nBatch, 7] tensor where the scores live (columns: PathStats) -- what the reference's
    computeStats gets from decode() + compareBracket + compareFramewise (ModelTransformer.py:403-438), without the Python lists:
    the decoded path stays packed on the device and the comparison kernel reads it there.  Nothing waits for the device: a decode
    that gave up on a bounded wait shows as -1 in every entry.  tolerance: as compare_paths_packed.  No gradient."""
    T, B = _check_inputs(score, noiseScore)
    tol = _tolerance(tolerance, "decode_stats")
    with torch.no_grad():
        score_c, noise_c = _prep(score.detach()), _prep(noiseScore.detach())
        dev = score_c.device
        ref_pairs, ref_offsets = pack_intervals(intervals, T, B, dev, ordered=True)
        start = _start_tensor(forcedStartPos, T, B, dev)
        pairs, offsets = _viterbi_raw(score_c, noise_c, start, bool(forward))
        return _compare_paths_raw(pairs, offsets, ref_pairs, ref_offsets, T, tol)


def viterbiBackward(score, noiseScore, forcedStartPos: Optional[List[int]] = None) -> Intervals:
    """Right-to-left Viterbi, the default decode (reference :13-104)."""
    return _decode(score, noiseScore, forcedStartPos, forward=False)


def viterbi(score, noiseScore, forcedStartPos: Optional[List[int]] = None) -> Intervals:
    """Left-to-right Viterbi (reference :107-202); forcedStartPos is the END position here."""
    return _decode(score, noiseScore, forcedStartPos, forward=True)


def computeLogZ(score, noiseScore):
    """Reference :207-246 (the autograd-traceable variant).  Same kernel as computeLogZFasterGrad."""
    _check_inputs(score, noiseScore)
    return ComputeLogZFasterGrad.apply(score, noiseScore)


def forward_backward(score, noiseScore):
    """Reference :375-456: returns (logZ [B], grad [T,T,B], gradNoise [T-1,B])."""
    T, B = _check_inputs(score, noiseScore)
    with torch.no_grad():
        s, n = _prep(score.detach()), _prep(noiseScore.detach())
        logz, v = _logz_fwd_raw(s, n, want_v=True)
        ones = torch.ones(B, dtype=torch.float32, device=s.device)
        grad, grad_noise, _ = _logz_bwd_raw(s, n, v, logz, ones)
    return logz, grad, grad_noise


def evalPath(intervals: Intervals, score, noiseScore):
    """Unnormalised path score (reference :508-550)."""
    T, B = _check_inputs(score, noiseScore)
    pairs, offsets = pack_intervals(intervals, T, B, score.device)
    return _EvalPath.apply(score, noiseScore, pairs, offsets)


class NeuralSemiCRFInterval:
    def __init__(self, score, noiseScore):
        """The output layer for multiple tracks of non-overlapping intervals (reference :553-564).

        score      -- [T, T, nBatch]: score of every closed interval [begin, end], indexed
                      [end, begin, track]; only end >= begin is read.
        noiseScore -- [T-1, nBatch]: score of "no event" between frames t and t+1.
        """
        self.score = score
        self.noiseScore = noiseScore
        self._hub = None            # (score, noiseScore, score alias, noise alias, _HubState): strong references, compared by identity

    def _hubbed(self):
        """(score, noiseScore, hub state) for the differentiable methods: aliases behind this object's private hub node when a
        gradient can flow, the tensors themselves (hub None) otherwise."""
        s, n = self.score, self.noiseScore
        if not (torch.is_grad_enabled() and (s.requires_grad or n.requires_grad)) :
            return s, n, None
        h = self._hub
        if h is None or h[0] is not s or h[1] is not n:
            state = _HubState()
            hs, hn = _Hub.apply(s, n, state)
            h = self._hub = (s, n, hs, hn, state)
        return h[2], h[3], h[4]

    def decode(self, forcedStartPos=None, forward=False):
        if forward:
            return viterbi(self.score, self.noiseScore, forcedStartPos)
        else:
            return viterbiBackward(self.score, self.noiseScore, forcedStartPos)

    def decode_packed(self, forcedStartPos=None, forward=False):
        """An EXTENSION of the reference's surface: the decoded path of `decode` as two int32 arrays -- pairs [K, 2] of
        (begin, end), chain after chain and ascending within a chain, and offsets [nBatch + 1] (chain c owns
        pairs[offsets[c]:offsets[c + 1]]) -- i.e. what the device produced, before the Python lists are built.  `decode` spends
        ~25 ns of CPython object creation per interval on top of it (657 k intervals at T=2048, nBatch=352: 17 ms against 1 ms
        here); callers that go on with arrays anyway should take this one."""
        return _decode(self.score, self.noiseScore, forcedStartPos, bool(forward), packed=True)

    def decode_stats(self, intervals, forcedStartPos=None, forward=False, tolerance=None):
        """An EXTENSION of the reference's surface: decode_packed(forcedStartPos, forward) followed by the comparison with the
        target `intervals` on the same device: an int32 tensor [nBatch, 7] with the columns of PathStats (list lengths, exact
        matches, the three frame counts of the reference's compareFramewise, matches within `tolerance`) -- see the module-level
        decode_stats and compare_paths_packed.  Builds no Python lists and never waits for the device; no gradient."""
        return decode_stats(self.score, self.noiseScore, intervals, forcedStartPos, bool(forward), tolerance)

    def sample(self, nSample=1, forcedEndPos=None, generator=None):
        """An EXTENSION of the reference's surface: a list of `nSample` Intervals drawn exactly from p(path) =
        exp(evalPath(path) - computeLogZ()); each element plugs into logProb / evalPath.  forcedEndPos (None or nBatch frames) is
        the path's END, as decode(forward=True, forcedStartPos=...); generator: None (torch's default CPU generator) or a CPU
        torch.Generator.  Runs where the scores live (HIP kernels on the GPU, host kernels on the CPU); no gradient."""
        return sample(self.score, self.noiseScore, nSample, forcedEndPos, generator)

    def sample_packed(self, nSample=1, forcedEndPos=None, generator=None):
        """`sample` as two int32 arrays, pairs [K, 2] and offsets [nSample * nBatch + 1] (sample-major), before the Python lists are
        built -- see the module-level sample_packed."""
        return sample_packed(self.score, self.noiseScore, nSample, forcedEndPos, generator)

    def decode_nbest(self, k, forcedStartPos=None, forward=False):
        """An EXTENSION of the reference's surface: the k highest-scoring paths of every chain, ranked -- (paths, scores) with
        paths a list of k Intervals (None where a chain has fewer than k paths) and scores a float32 numpy [k, nBatch].  k = 1
        is decode(forcedStartPos, forward) bit for bit; see the module-level viterbi_nbest.  No gradient."""
        return viterbi_nbest(self.score, self.noiseScore, k, forcedStartPos, bool(forward))

    def decode_nbest_packed(self, k, forcedStartPos=None, forward=False):
        """`decode_nbest` as numpy arrays (pairs, offsets [k * nBatch + 1] rank-major, scores [k, nBatch], npaths [nBatch]) before
        the Python lists are built -- see the module-level viterbi_nbest_packed."""
        return viterbi_nbest_packed(self.score, self.noiseScore, k, forcedStartPos, bool(forward))

    def posteriors(self, forcedStartPos=None):
        """An EXTENSION of the reference's surface: a Posteriors namedtuple (logZ, entropy, node, begin, end, single, noise) of
        float32 tensors where the scores live -- see the module-level posteriors.  No host sync, no gradient.  forcedStartPos (as
        decode's, or an int32 tensor [nBatch] on the device): the posterior of the model restricted to the frames from each chain's
        start on -- the one decode(forcedStartPos) maximises; the same keyword on interval_marginals, decode_marginal, decode_mbr
        and their _packed forms."""
        return posteriors(self.score, self.noiseScore, forcedStartPos)

    def interval_marginals(self, intervals, tolerance=None, forcedStartPos=None):
        """An EXTENSION of the reference's surface: the posterior probability of each interval of `intervals` (e.g. decode()'s
        result), a list (len nBatch) of lists of floats in the given order.  tolerance (None, an int or (onset, offset) in frames,
        0..8): the probability of an interval within that window -- see the module-level interval_marginals_packed."""
        return interval_marginals(self.score, self.noiseScore, intervals, tolerance, forcedStartPos)

    def interval_marginals_packed(self, pairs, offsets, tolerance=None, forcedStartPos=None):
        """`interval_marginals` on decode_packed's arrays (numpy or tensors): a float32 tensor [K] where the scores live."""
        return interval_marginals_packed(self.score, self.noiseScore, pairs, offsets, tolerance, forcedStartPos)

    def expectation(self, weight, noiseWeight=None):
        """An EXTENSION of the reference's surface: E_p[W] [nBatch] of the additive path functional given by weight [T, T, nBatch]
        and noiseWeight [T-1, nBatch] (default zeros), float32, differentiable once -- see the module-level expectation."""
        return expectation(self.score, self.noiseScore, weight, noiseWeight)

    def entropy(self):
        """An EXTENSION of the reference's surface: the path entropy [nBatch] in nats, float32, differentiable once -- see the
        module-level entropy."""
        return entropy(self.score, self.noiseScore)

    def covariance(self, weight, noiseWeight=None):
        """An EXTENSION of the reference's surface: (E, C, Cn), the covariances of every cell with the path functional, i.e. the
        Hessian of logZ times (weight, noiseWeight) -- see the module-level covariance.  No gradient."""
        return covariance(self.score, self.noiseScore, weight, noiseWeight)

    def decode_marginal(self, threshold, tolerance=None, forcedStartPos=None):
        """An EXTENSION of the reference's surface: (paths, probs) -- every interval whose posterior probability is >= threshold
        (a float in (0, 1] or a float tensor [nBatch]; no default), per chain ascending by (begin, end), and those probabilities.
        For threshold > 0.5 each chain's result is a path (plugs into evalPath / logProb) -- see the module-level
        decode_marginal_packed.  With a tolerance (None, an int or (onset, offset) in frames, 0..8) the result is a lattice, not a
        path: decode_mbr is the call that returns one.  No gradient."""
        return decode_marginal(self.score, self.noiseScore, threshold, tolerance, forcedStartPos)

    def decode_marginal_packed(self, threshold, tolerance=None, forcedStartPos=None):
        """`decode_marginal` as host arrays (pairs int32 [K, 2], offsets int32 [nBatch + 1], probs float32 [K]) before the Python
        lists are built; pairs / offsets feed interval_marginals_packed and attributes.attribute_input_packed as they are."""
        return decode_marginal_packed(self.score, self.noiseScore, threshold, tolerance, forcedStartPos)

    def decode_mbr(self, threshold, tolerance=None, forcedStartPos=None):
        """An EXTENSION of the reference's surface: (paths, probs, gain) -- per chain the minimum-Bayes-risk PATH at `threshold` (the
        path maximising the sum over its intervals of (posterior probability - threshold); a float in (0, 1] or a float tensor
        [nBatch]; no default), its intervals' probabilities and the maximised sum.  Always a path (plugs into evalPath / logProb),
        also for threshold <= 0.5 where decode_marginal gives a lattice -- see the module-level decode_mbr_packed.  tolerance (None,
        an int or (onset, offset) in frames, 0..8): the probabilities count an interval within that window.  No gradient."""
        return decode_mbr(self.score, self.noiseScore, threshold, tolerance, forcedStartPos)

    def decode_mbr_packed(self, threshold, tolerance=None, forcedStartPos=None):
        """`decode_mbr` as host arrays (pairs int32 [K, 2], offsets int32 [nBatch + 1], probs float32 [K], gain float32 [nBatch])
        before the Python lists are built."""
        return decode_mbr_packed(self.score, self.noiseScore, threshold, tolerance, forcedStartPos)

    def evalPath(self, intervals):
        """compute the unnormalized score"""
        T, B = _check_inputs(self.score, self.noiseScore)
        pairs, offsets = pack_intervals(intervals, T, B, self.score.device)
        s, n, hub = self._hubbed()
        return _EvalPath.apply(s, n, pairs, offsets, hub)

    def computeLogZ(self, noBackward=False):
        """compute the log normalization factor"""
        _check_inputs(self.score, self.noiseScore)
        s, n, hub = self._hubbed()
        return ComputeLogZFasterGrad.apply(s, n, hub)

    def logProb(self, intervals, noBackward=False):
        T, B = _check_inputs(self.score, self.noiseScore)
        pairs, offsets = pack_intervals(intervals, T, B, self.score.device, overlap=not os.environ.get("SEMICRF_NO_COPY_OVERLAP"))
        return _LogProb.apply(self.score, self.noiseScore, pairs, offsets)
