"""The memory contract of the semi-CRF entry points (include/semicrf_hip.h, "Memory contract"): guard bands, written sets, base
alignment and the workspace.

Every case runs on the CPU path (the shim's host kernels, unmarked) and on the device (@pytest.mark.gpu).  Calls go to
`_lib.ops().<op>` directly: all operands, outputs and the workspace of a case are carved out of ONE guard-band arena
(tests/arena_common.py), so a stray access is a failed assertion and never a fault.

Group A  nothing outside the contract is written (guards, and every output element outside the documented written set keeps the
         pattern), everything inside is (it equals, bit for bit, the same op on ordinary tensors, and it differs from the pattern),
         nothing outside is read into a result (a NaN-pattern arena and a FLT_MAX-pattern arena give identical bits).
Group B  base alignment: operands / outputs at address phases 0, 4, 8, 12 modulo 16, and mixed; bit-identical to phase 0; at
         phase 12 also against float64 (LOGZ_TOL / grad_tol of tests/test_gpu_parity.py, the oracle's Viterbi lists).
Group C  the workspace: the alignment check (through ctypes, nothing is launched), exactly semicrf_workspace_bytes bytes between
         guards (every arena case), results independent of the workspace's earlier contents.

Written sets that the header leaves to the implementation and that are pinned here:
  * SEMICRF_GRAD_UPPER_IS_ZERO is a permission.  The persistent gradient sweep (device, T >= 2, NBatch >= 2, impl 0) leaves the
    cells begin > end untouched; the row-sequential device kernels and the host kernels write +0.0f there.
  * semicrf_eval_path_bwd accumulates: dScore is touched on the path's cells only, dNoise everywhere.
"""
import ctypes

import numpy as np
import pytest
import torch

import arena_common as ac
from conftest import rel_err, unpack_lists
from transkun_amd import _lib, synth

CPU = torch.device("cpu")
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
LOGZ_TOL = 1e-5                                  # tests/test_gpu_parity.py


def grad_tol(logz):                              # tests/test_gpu_parity.py
    return max(1e-4, 2e-6 * float(np.max(np.abs(logz))))


def _dev(request, which):
    return CPU if which == "cpu" else request.getfixturevalue("gpu")


DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]

# T, B, kind: the smallest shape at which each code path of the sweeps exists (PB = 16 rows a block, FAR0 = 4 blocks before the
# first panel, GP = 32 chains a panel task, the in-sweep band copy needs more than 12 row blocks)
SHAPES = [
    pytest.param((1, 3, "randn"), id="T1_B3"),           # no noise, no recurrence: Cn / noiseP / dNoise have no elements
    pytest.param((2, 3, "randn"), id="T2_B3"),           # the smallest shape with a recurrence
    pytest.param((17, 12, "model"), id="T17_B12"),       # two row blocks, no panels
    pytest.param((33, 7, "randn"), id="T33_B7"),         # odd B, T*T*B % 4 == 3
    pytest.param((130, 90, "model"), id="T130_B90"),     # panels, B % 4 == 2
    pytest.param((200, 33, "randn"), id="T200_B33"),     # odd B, in-sweep band copy
]
SMALL = [pytest.param((2, 3, "randn"), id="T2_B3"), pytest.param((17, 12, "model"), id="T17_B12")]
BIG = (1024, 6, "randn")                                 # two far waves per spine plus the band copy; 25 MB


# ---- the shared, read-only context of a shape: inputs and the intermediate results the later ops take ----------------------------
class Context:
    pass


_CTX = {}


def context(shape, dev):
    T, B, kind = shape
    key = (T, B, kind, str(dev))
    if key in _CTX:
        return _CTX[key]
    ops = _lib.ops()
    cx = Context()
    cx.T, cx.B, cx.dev, cx.cuda = T, B, dev, dev.type == "cuda"
    score, noise = synth.crf_inputs(T, B, 4000 + T + B, "cpu", kind)
    weight, nweight = synth.crf_inputs(T, B, 5000 + T + B, "cpu", "randn")
    cx.score, cx.noise = score.contiguous().to(dev), noise.contiguous().to(dev)
    cx.weight, cx.nweight = weight.contiguous().to(dev), nweight.contiguous().to(dev)
    cx.gout = (0.5 + 0.25 * (torch.arange(B) % 3).float()).to(dev)
    cx.gout1 = cx.gout[:1].clone()
    cx.ones = torch.ones(B, dtype=F32, device=dev)
    cx.start = ((torch.arange(B) * 7) % T).to(I32).to(dev)
    cx.end = ((torch.arange(B) * 5 + 1) % T).to(I32).to(dev)

    def wsb(op, nB=None):
        if not cx.cuda:                                       # the host kernels allocate their own scratch; expectation keeps doubles
            return (4 * T * B + 2 * B) * 8 if op == _lib.OP_EXPECTATION else 0
        return int(_lib.load().semicrf_workspace_bytes(op, T, B if nB is None else nB))
    cx.wsb = wsb
    ws = lambda op, nB=None: torch.empty(wsb(op, nB), dtype=U8, device=dev)
    cx.logZ = torch.empty(B, dtype=F32, device=dev)
    cx.v = torch.empty(T, B, dtype=F32, device=dev)
    ops.logz_fwd(cx.score, cx.noise, cx.logZ, cx.v, True, ws(_lib.OP_LOGZ_FWD))
    cx.q = torch.empty(T, B, dtype=F32, device=dev)
    ops.beta(cx.score, cx.noise, cx.q, ws(_lib.OP_LOGZ_FWD))
    # the target path of evalPath / logProb and the query of interval_marginals: the forward Viterbi path (ascending by (begin, end))
    pairs = torch.empty(2 * T * B, 2, dtype=I32, device=dev)
    cx.offsets = torch.empty(B + 1, dtype=I32, device=dev)
    ops.viterbi(cx.score, cx.noise, cx.offsets, False, True, pairs, cx.offsets, ws(_lib.OP_VITERBI))
    cx.K = int(cx.offsets[-1])
    assert 0 < cx.K <= 2 * T * B
    cx.pairs = pairs[:cx.K].clone()
    chain = torch.repeat_interleave(torch.arange(B, device=dev), (cx.offsets[1:] - cx.offsets[:-1]).long())
    cx.path_mask = torch.zeros(T, T, B, dtype=torch.bool, device=dev)
    cx.path_mask[cx.pairs[:, 1].long(), cx.pairs[:, 0].long(), chain] = True
    cx.tril = torch.tril(torch.ones(T, T, dtype=torch.bool, device=dev))[:, :, None].expand(T, T, B)
    cx.tau = torch.tensor([0.3], dtype=F32, device=dev)
    if cx.cuda:
        torch.cuda.synchronize(dev)
        assert _lib.device_status() == 0
    _CTX[key] = cx
    return cx


class Run:
    """One execution of a case: where its tensors come from (an arena, a sizer or torch's allocator) and at which address phases."""

    def __init__(self, A, cx, pin=0, pout=0, wsfill=None):
        self.A, self.cx, self.pin, self.pout, self.wsfill = A, cx, pin, pout, wsfill

    def inp(self, name, t=None):
        return self.A.put(name, getattr(self.cx, name) if t is None else t, self.pin)

    def out(self, name, shape, dtype=F32):
        return self.A.carve(name, shape, dtype, self.pout)

    def ws(self, op, nB=None):
        """Exactly semicrf_workspace_bytes(op, T, B) bytes at the alignment the header demands, between guards."""
        n = self.cx.wsb(op, nB)
        w = self.A.carve("ws", (n,), U8, 0, 256)
        if self.A.real and n and self.wsfill is not None:
            if self.wsfill == "random":
                w.copy_(torch.from_numpy(np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)))
            else:
                w.fill_(self.wsfill)
        return w

    def call(self, fn):
        return self.A.call(fn)


def _head(off):
    """Written rows of a packed list: the first min(total, cap), total = the last offset."""
    def mask(outs, t):
        total = int(outs[off][0][-1])
        assert total >= 0, "the call reported an error through its last offset"
        m = torch.zeros(t.shape, dtype=torch.bool, device=t.device)
        m[:min(total, t.shape[0])] = True
        return m
    return mask


# ---- the cases: each carves its operands, outputs and workspace, calls the op and names the written set ---------------------------
def case_logz_fwd(want_v):
    def case(r):
        T, B = r.cx.T, r.cx.B
        score, noise = r.inp("score"), r.inp("noise")
        logZ, v = r.out("logZ", (B,)), r.out("v", (T, B))
        ws = r.ws(_lib.OP_LOGZ_FWD)
        r.call(lambda: _lib.ops().logz_fwd(score, noise, logZ, v, want_v, ws))
        return {"logZ": (logZ, True), "v": (v, want_v)}
    return case


def case_logz_bwd(want_q, flags):
    def case(r):
        cx, T, B = r.cx, r.cx.T, r.cx.B
        score, noise, v, logZ, gout = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("logZ"), r.inp("gout")
        dS, dN, q = r.out("dScore", (T, T, B)), r.out("dNoise", (T - 1, B)), r.out("q", (T, B))
        ws = r.ws(_lib.OP_LOGZ_BWD)
        r.call(lambda: _lib.ops().logz_bwd(score, noise, v, logZ, gout, dS, dN, q, want_q, flags, ws))
        skips_upper = flags and cx.cuda and _lib.get_impl() == 0 and T >= 2 and B >= 2
        return {"dScore": (dS, (lambda o, t: cx.tril) if skips_upper else True), "dNoise": (dN, True), "q": (q, want_q)}
    return case


def case_beta(r):
    T, B = r.cx.T, r.cx.B
    score, noise = r.inp("score"), r.inp("noise")
    out = r.out("beta", (T, B))
    ws = r.ws(_lib.OP_LOGZ_FWD)
    r.call(lambda: _lib.ops().beta(score, noise, out, ws))
    return {"beta": (out, True)}


def case_alpha_from(r):
    T, B = r.cx.T, r.cx.B
    score, noise, start = r.inp("score"), r.inp("noise"), r.inp("start")
    v, logZ = r.out("v", (T, B)), r.out("logZ", (B,))
    ws = r.A.carve("ws", (0,), U8, 0, 256)
    r.call(lambda: _lib.ops().alpha_from(score, noise, start, v, logZ, ws))
    return {"v": (v, True), "logZ": (logZ, True)}


def case_viterbi(has_start, forward, cap=None):
    def case(r):
        T, B = r.cx.T, r.cx.B
        score, noise, start = r.inp("score"), r.inp("noise"), r.inp("start")
        pairs = r.out("pairs", (2 * T * B + 7 if cap is None else cap, 2), I32)
        offsets = r.out("offsets", (B + 1,), I32)
        ws = r.ws(_lib.OP_VITERBI)
        r.call(lambda: _lib.ops().viterbi(score, noise, start, has_start, forward, pairs, offsets, ws))
        return {"pairs": (pairs, _head("offsets")), "offsets": (offsets, True)}
    return case


def case_sample(n, has_end):
    def case(r):
        T, B = r.cx.T, r.cx.B
        score, noise, v, end = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("end")
        pairs = r.out("pairs", (n * B * 2 * T + 7, 2), I32)
        offsets = r.out("offsets", (n * B + 1,), I32)
        ws = r.ws(_lib.OP_SAMPLE, n * B)
        r.call(lambda: _lib.ops().sample(score, noise, v, 0, n, 0x5EED1234ABCD, end, has_end, pairs, offsets, ws))
        return {"pairs": (pairs, _head("offsets")), "offsets": (offsets, True)}
    return case


def case_nbest(k, has_start, forward):
    def case(r):
        T, B = r.cx.T, r.cx.B
        score, noise, start = r.inp("score"), r.inp("noise"), r.inp("start")
        pairs = r.out("pairs", (k * B * 2 * T + 7, 2), I32)
        offsets, scores, npaths = r.out("offsets", (k * B + 1,), I32), r.out("scores", (k, B)), r.out("npaths", (B,), I32)
        ws = r.ws(_lib.OP_VITERBI_NBEST, k * B)
        r.call(lambda: _lib.ops().viterbi_nbest(score, noise, k, start, has_start, forward, pairs, offsets, scores, npaths, ws))
        return {"pairs": (pairs, _head("offsets")), "offsets": (offsets, True), "scores": (scores, True), "npaths": (npaths, True)}
    return case


def case_posteriors(r):
    T, B = r.cx.T, r.cx.B
    score, noise, v, q, logZ = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("q"), r.inp("logZ")
    names = ["node", "begin", "end", "single"]
    o = {n: r.out(n, (T, B)) for n in names}
    noiseP, entropy = r.out("noiseP", (T - 1, B)), r.out("entropy", (B,))
    ws = r.ws(_lib.OP_POSTERIORS)
    r.call(lambda: _lib.ops().posteriors(score, noise, v, q, logZ, o["node"], o["begin"], o["end"], o["single"], noiseP, entropy, ws))
    res = {n: (o[n], True) for n in names}
    res.update(noiseP=(noiseP, True), entropy=(entropy, True))
    return res


def case_expectation(alias, has_nw):
    """semicrf_expectation and, from the state it leaves in ws, semicrf_covariance.  alias: weight IS score (and noiseWeight IS noise)."""
    def case(r):
        T, B = r.cx.T, r.cx.B
        score, noise, v, q, gout = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("q"), r.inp("gout")
        weight = score if alias else r.inp("weight")
        nweight = (noise if alias else r.inp("nweight")) if has_nw else r.A.carve("none", (0,), F32, r.pin)
        E, H = r.out("E", (B,)), r.out("H", (B,))
        C, Cn = r.out("C", (T, T, B)), r.out("Cn", (T - 1, B))
        ws = r.ws(_lib.OP_EXPECTATION)

        def both():
            _lib.ops().expectation(score, noise, weight, nweight, has_nw, v, q, E, H, ws)
            _lib.ops().covariance(score, noise, weight, nweight, has_nw, gout, C, Cn, ws)
        r.call(both)
        return {"E": (E, True), "H": (H, True), "C": (C, True), "Cn": (Cn, True)}
    return case


def case_interval_marginals(tol):
    def case(r):
        cx, T, B = r.cx, r.cx.T, r.cx.B
        score, v, q, logZ = r.inp("score"), r.inp("v"), r.inp("q"), r.inp("logZ")
        pairs, offsets = r.inp("pairs"), r.inp("offsets")
        out = r.out("out", (cx.K + 5,))

        def go():
            if tol is None:
                _lib.ops().interval_marginals(score, v, q, logZ, pairs, cx.K, offsets, out)
            else:
                _lib.ops().interval_marginals_tol(score, v, q, logZ, pairs, cx.K, offsets, tol[0], tol[1], out)
        r.call(go)
        head = torch.arange(cx.K + 5, device=cx.dev) < cx.K
        return {"out": (out, lambda o, t: head)}
    return case


def case_eval_path(r):
    cx, B = r.cx, r.cx.B
    score, noise, pairs, offsets = r.inp("score"), r.inp("noise"), r.inp("pairs"), r.inp("offsets")
    out = r.out("out", (B,))
    ws = r.ws(_lib.OP_EVAL_PATH)
    r.call(lambda: _lib.ops().eval_path(score, noise, pairs, cx.K, offsets, out, ws))
    return {"out": (out, True)}


def case_eval_path_bwd(r):
    """Accumulates: the cells the header says it adds to start at zero, every other cell at the pattern."""
    cx, T, B = r.cx, r.cx.T, r.cx.B
    gout, pairs, offsets = r.inp("gout"), r.inp("pairs"), r.inp("offsets")
    dS, dN = r.out("dScore", (T, T, B)), r.out("dNoise", (T - 1, B))
    if r.A.real:
        dS[cx.path_mask] = 0.0
        dN.zero_()
    r.call(lambda: _lib.ops().eval_path_bwd(gout, T, B, pairs, cx.K, offsets, dS, True, dN, True))
    return {"dScore": (dS, lambda o, t: cx.path_mask), "dNoise": (dN, True)}


def case_logprob_fwd(want_v):
    def case(r):
        cx, T, B = r.cx, r.cx.T, r.cx.B
        score, noise, pairs, offsets = r.inp("score"), r.inp("noise"), r.inp("pairs"), r.inp("offsets")
        lp, logZ, v = r.out("logProb", (B,)), r.out("logZ", (B,)), r.out("v", (T, B))
        ws = r.ws(_lib.OP_LOGZ_FWD)
        r.call(lambda: _lib.ops().logprob_fwd(score, noise, pairs, cx.K, offsets, lp, logZ, v, want_v, ws, offsets, False))
        return {"logProb": (lp, True), "logZ": (logZ, True), "v": (v, want_v)}
    return case


def case_logprob_bwd(gstride, table):
    """table: the forward call writes the path table and the backward call takes it (device only, where the library supports it)."""
    def case(r):
        cx, T, B = r.cx, r.cx.T, r.cx.B
        score, noise, v, logZ = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("logZ")
        gout = r.inp("gout") if gstride else r.inp("gout1")
        pairs, offsets = r.inp("pairs"), r.inp("offsets")
        dS, dN = r.out("dScore", (T, T, B)), r.out("dNoise", (T - 1, B))
        res = {"dScore": (dS, True), "dNoise": (dN, True)}
        if table:
            ptab, lp, lz = r.out("ptab", (T, B), I32), r.out("logProb", (B,)), r.out("logZ_out", (B,))
            wsf = r.ws(_lib.OP_LOGZ_FWD)
            res.update(ptab=(ptab, True), logProb=(lp, True), logZ_out=(lz, True))
        ws = r.ws(_lib.OP_LOGZ_BWD)

        def go():
            if table:
                _lib.ops().logprob_fwd(score, noise, pairs, cx.K, offsets, lp, lz, v, False, wsf, ptab, True)
            _lib.ops().logprob_bwd(score, noise, v, logZ, gout, gstride, pairs, cx.K, offsets, dS, dN, 0, ws, ptab if table else offsets, table)
        r.call(go)
        return res
    return case


def case_marginal_decode(tol):
    def case(r):
        cx, T, B = r.cx, r.cx.T, r.cx.B
        score, noise, v, q, logZ, tau = r.inp("score"), r.inp("noise"), r.inp("v"), r.inp("q"), r.inp("logZ"), r.inp("tau")
        cap = T * 5 * B + 3
        pairs, probs, offsets = r.out("pairs", (cap, 2), I32), r.out("probs", (cap,)), r.out("offsets", (B + 1,), I32)
        ws = r.ws(_lib.OP_MARGINAL_DECODE if tol is None else _lib.OP_MARGINAL_DECODE_TOL)

        def go():
            if tol is None:
                _lib.ops().marginal_decode(score, noise, v, q, logZ, tau, pairs, probs, offsets, ws)
            else:
                _lib.ops().marginal_decode_tol(score, noise, v, q, logZ, tau, tol[0], tol[1], pairs, probs, offsets, ws)
        r.call(go)
        return {"pairs": (pairs, _head("offsets")), "probs": (probs, _head("offsets")), "offsets": (offsets, True)}
    return case


def case_mbr_select(r):
    """The lattice: the target path with weights that straddle tau.  `pairs` is an 8-byte aligned input (the header's rule)."""
    cx, T, B = r.cx, r.cx.T, r.cx.B
    w = (0.2 + 0.6 * ((torch.arange(cx.K) * 37) % 11).float() / 10.0).to(cx.dev)
    pairs = r.A.put("pairs", cx.pairs, r.pin & 8)
    weight, offsets, tau = r.inp("weight", w), r.inp("offsets"), r.inp("tau")
    cap = 2 * T * B + 3
    po, pr = r.out("pairs_out", (cap, 2), I32), r.out("probs_out", (cap,))
    oo, gain = r.out("offsets_out", (B + 1,), I32), r.out("gain", (B,))
    ws = r.ws(_lib.OP_MBR_SELECT)
    r.call(lambda: _lib.ops().mbr_select(pairs, weight, offsets, T, tau, po, pr, oo, gain, ws))
    return {"pairs_out": (po, _head("offsets_out")), "probs_out": (pr, _head("offsets_out")), "offsets_out": (oo, True), "gain": (gain, True)}


UPPER = 1                                        # SEMICRF_GRAD_UPPER_IS_ZERO
CASES = {
    "logz_fwd-v": case_logz_fwd(True),
    "logz_fwd-nov": case_logz_fwd(False),
    "logz_bwd-q": case_logz_bwd(True, 0),
    "logz_bwd-noq-upper": case_logz_bwd(False, UPPER),
    "beta": case_beta,
    "alpha_from": case_alpha_from,
    "viterbi-bwd": case_viterbi(False, False),
    "viterbi-fwd": case_viterbi(False, True),
    "viterbi-bwd-start": case_viterbi(True, False),
    "viterbi-fwd-start": case_viterbi(True, True),
    "viterbi-bwd-cap3": case_viterbi(False, False, cap=3),
    "sample-1": case_sample(1, False),
    "sample-3-end": case_sample(3, True),
    "nbest-1-bwd": case_nbest(1, False, False),
    "nbest-4-fwd-start": case_nbest(4, True, True),
    "nbest-4-bwd-start": case_nbest(4, True, False),
    "nbest-1-fwd": case_nbest(1, False, True),
    "posteriors": case_posteriors,
    "expectation-alias": case_expectation(True, True),
    "expectation-separate": case_expectation(False, True),
    "expectation-nonw": case_expectation(False, False),
    "interval_marginals": case_interval_marginals(None),
    "interval_marginals_tol": case_interval_marginals((2, 1)),
    "eval_path": case_eval_path,
    "eval_path_bwd": case_eval_path_bwd,
    "logprob_fwd-v": case_logprob_fwd(True),
    "logprob_fwd-nov": case_logprob_fwd(False),
    "logprob_bwd": case_logprob_bwd(1, False),
    "logprob_bwd-g0": case_logprob_bwd(0, False),
    # the workspace's sufficiency for the three ops that have guard tests of their own elsewhere
    "marginal_decode": case_marginal_decode(None),
    "marginal_decode_tol": case_marginal_decode((1, 2)),
    "mbr_select": case_mbr_select,
}
SWEEPS = ["logz_fwd-v", "viterbi-bwd", "viterbi-fwd-start", "logz_bwd-q", "logz_bwd-noq-upper"]          # the three ops of the 25 MB shape
ROWSEQ = ["logz_fwd-v", "logz_fwd-nov", "logz_bwd-q", "logz_bwd-noq-upper", "beta", "viterbi-bwd", "viterbi-fwd-start",
          "logprob_fwd-v", "logprob_bwd", "logprob_bwd-g0"]                                                # what set_impl(1) reroutes
HAS_WS = [n for n in CASES if n.split("-")[0] not in ("alpha_from", "interval_marginals", "interval_marginals_tol", "eval_path_bwd")]


def _guard_bytes(cx):
    return max(4096, cx.T * cx.B * 4)


def _arena(case, cx, pattern, **kw):
    a, outs = ac.run_in_arena(lambda A: case(Run(A, cx, **kw)), _guard_bytes(cx), pattern, cx.dev)
    a.check()
    return outs


def _mask(spec, outs, t):
    if spec is True or spec is False:
        return torch.full(t.shape, bool(spec), dtype=torch.bool, device=t.device)
    return spec(outs, t).expand(t.shape)


def _word(pattern):
    return int(np.array([pattern], dtype=np.uint32).view(np.int32)[0])


def _same_written(outs, ref, pattern, what):
    """Inside the written set: the bits of `ref`, and never the pattern.  Outside: the pattern."""
    for name, (t, spec) in outs.items():
        m = _mask(spec, outs, t)
        assert torch.equal(m, _mask(ref[name][1], ref, ref[name][0])), f"{what}: `{name}`: the written sets differ"
        tb, rb = ac.bits(t).view(t.shape), ac.bits(ref[name][0]).view(t.shape)
        if not torch.equal(tb[m], rb[m]):
            i = int(torch.nonzero(tb[m] != rb[m])[0])
            raise AssertionError(f"{what}: `{name}`: written element {i} of {int(m.sum())} differs from the reference run")
        if bool((tb[m] == _word(pattern)).any()):
            i = int(torch.nonzero((tb == _word(pattern)) & m)[0].tolist()[0])
            raise AssertionError(f"{what}: `{name}`: an element the call must write still holds the pattern (first index {i})")
        if not bool((tb[~m] == _word(pattern)).all()):
            raise AssertionError(f"{what}: `{name}`: {int((tb[~m] != _word(pattern)).sum())} elements outside the written set were written")


def _device_ok(cx):
    if cx.cuda:
        assert _lib.device_status() == 0


def _group_a(name, cx):
    case = CASES[name]
    plain = ac.Plain(ac.NAN_PATTERN, cx.dev)
    ref = case(Run(plain, cx))
    plain.check()
    nan = _arena(case, cx, ac.NAN_PATTERN)
    _same_written(nan, ref, ac.NAN_PATTERN, f"{name}, NaN arena against ordinary tensors")
    # surround independence: the written bits do not depend on what lies around the operands
    # (only the written elements are compared with the other run; the rest is compared with the run's own pattern)
    mx = _arena(case, cx, ac.MAX_PATTERN)
    _same_written(mx, nan, ac.MAX_PATTERN, f"{name}, FLT_MAX arena against NaN arena")
    _device_ok(cx)


# ---- the arena itself ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("pattern", sorted(ac.PATTERNS))
def test_arena_self_test(request, which, pattern):
    """A plain torch write one element before and one element after a carve makes check() fail; a write inside does not."""
    dev = _dev(request, which)
    for dtype, phase in ((F32, 0), (F32, 12), (I32, 4), (U8, 0)):
        def fresh():
            a = ac.Arena(3 * 8192 + 4096, 4096, ac.PATTERNS[pattern], dev)
            a.carve("left", (5,), F32, 8)
            t = a.carve("mid", (33,), dtype, phase, 256 if dtype == U8 else 16)
            a.carve("right", (0,), F32, 4)
            return a, t
        a, t = fresh()
        assert t.data_ptr() % (256 if dtype == U8 else 16) == phase and t.is_contiguous()
        if dtype != U8:
            assert bool((ac.bits(t) == _word(ac.PATTERNS[pattern])).all())
        a.check()
        t.fill_(3)
        a.check()                                                       # inside the carve: fine
        item = 1 if dtype == U8 else 4
        for after, where in ((False, "before the start of `mid`"), (True, "past the end of `mid`")):
            a, t = fresh()
            flat = a.u8 if dtype == U8 else a.words.view(dtype)
            first = (t.data_ptr() - a.base) // item
            flat[first + t.numel() if after else first - 1] = 1
            with pytest.raises(ac.GuardError, match=where):
                a.check()
    # an operand that changes is reported too
    a = ac.Arena(3 * 8192, 4096, ac.PATTERNS[pattern], dev)
    src = torch.arange(6, dtype=F32, device=dev)
    t = a.put("operand", src, 4)
    a.check()
    t[5] = -1.0
    with pytest.raises(ac.GuardError, match="operand"):
        a.check()


# ---- group A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_written_set_guards_and_surround(request, which, shape, name):
    cx = context(shape, _dev(request, which))
    _group_a(name, cx)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("name", ROWSEQ)
def test_written_set_row_sequential(request, which, shape, name):
    """The row-sequential kernels (semicrf_set_impl(1)); on the CPU path the switch changes nothing."""
    dev = _dev(request, which)
    _lib.set_impl(1)
    try:
        _group_a(name, context(shape, dev))
    finally:
        _lib.set_impl(0)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("name", SWEEPS)
def test_written_set_long_sequence(request, which, name):
    _group_a(name, context(BIG, _dev(request, which)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [pytest.param((130, 90, "model"), id="T130_B90"), pytest.param((200, 33, "randn"), id="T200_B33")])
@pytest.mark.parametrize("gstride", [1, 0])
def test_logprob_bwd_with_the_path_table(gpu, shape, gstride):
    """logProb's backward with the forward call's path table: the same contract and the bits of the call without it."""
    import copy
    from transkun_amd.CRF.NeuralSemiCRFInterval import pack_intervals
    cx = copy.copy(context(shape, gpu))
    # the table's precondition (a frame begins at most one interval) holds for target-like paths, not for a Viterbi path, whose
    # singletons share their frame with the interval that begins there
    pairs, cx.offsets = pack_intervals(synth.synthetic_intervals(cx.T, cx.B), cx.T, cx.B, gpu)
    cx.K = pairs._semicrf_K
    assert pairs._semicrf_simple and cx.K > 0
    cx.pairs = pairs[:cx.K].clone()
    # (130, 90): the backward takes the table; (200, 33): an odd batch keeps the scatter and ignores it -- the forward call writes
    # every word of it either way
    assert _lib.load().semicrf_logprob_path_table_supported(cx.T, cx.B) == (1 if cx.B % 2 == 0 else 0)
    without = _arena(case_logprob_bwd(gstride, False), cx, ac.NAN_PATTERN)
    for pattern in (ac.NAN_PATTERN, ac.MAX_PATTERN):
        outs = _arena(case_logprob_bwd(gstride, True), cx, pattern)
        _same_written({k: outs[k] for k in without}, without, pattern, "path table against scatter")
        for k in ("ptab", "logProb", "logZ_out"):
            assert not bool((ac.bits(outs[k][0]) == _word(pattern)).any()), k
    _device_ok(cx)


# ---- group B ------------------------------------------------------------------------------------------------------------------------
PHASES = [(4, 4), (8, 8), (12, 12), (12, 4)]                 # (operands, outputs); compared with (0, 0)


def _group_b(name, cx, phases):
    case = CASES[name]
    ref = _arena(case, cx, ac.NAN_PATTERN)
    for pin, pout in phases:
        outs = _arena(case, cx, ac.NAN_PATTERN, pin=pin, pout=pout)
        for k, (t, _) in outs.items():
            if t.numel() and t.dtype != U8:
                assert t.data_ptr() % 16 == pout, (k, pout)
        _same_written(outs, ref, ac.NAN_PATTERN, f"{name}, operands at phase {pin}, outputs at phase {pout}, against phase 0")
    _device_ok(cx)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_base_alignment(request, which, shape, name):
    """Any 4-byte aligned base gives the bits of a 16-byte aligned one (the documented summation orders name no alignment)."""
    _group_b(name, context(shape, _dev(request, which)), PHASES)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("name", ROWSEQ)
def test_base_alignment_row_sequential(request, which, shape, name):
    dev = _dev(request, which)
    _lib.set_impl(1)
    try:
        _group_b(name, context(shape, dev), PHASES)
    finally:
        _lib.set_impl(0)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("name", SWEEPS)
def test_base_alignment_long_sequence(request, which, name):
    _group_b(name, context(BIG, _dev(request, which)), [(12, 4), (4, 8)])


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("shape", SHAPES)
def test_phase_12_against_float64(request, which, shape, oracle):
    """Wrong-but-consistent cannot pass: at phase 12 logZ, the dense and noise gradients and the four decodes against float64."""
    cx = context(shape, _dev(request, which))
    T, B = cx.T, cx.B
    s64, n64 = cx.score.cpu().numpy(), cx.noise.cpu().numpy()
    lz64, grad64, gn64, _, _ = oracle.forward_backward_f64(s64, n64)
    kw = dict(pin=12, pout=12)
    fwd = _arena(case_logz_fwd(True), cx, ac.NAN_PATTERN, **kw)
    lz = fwd["logZ"][0].cpu().numpy()
    assert rel_err(lz, lz64) < LOGZ_TOL

    def bwd(r):                                               # gout = 1 on the alpha this phase produced
        score, noise = r.inp("score"), r.inp("noise")
        v, logZ, gout = r.inp("v", fwd["v"][0]), r.inp("logZ", fwd["logZ"][0]), r.inp("ones")
        dS, dN, q = r.out("dScore", (T, T, B)), r.out("dNoise", (T - 1, B)), r.out("q", (T, B))
        ws = r.ws(_lib.OP_LOGZ_BWD)
        r.call(lambda: _lib.ops().logz_bwd(score, noise, v, logZ, gout, dS, dN, q, True, 0, ws))
        return {"dScore": (dS, True), "dNoise": (dN, True)}
    g = _arena(bwd, cx, ac.NAN_PATTERN, **kw)
    gt = grad_tol(lz64)
    grad = g["dScore"][0].cpu().numpy()
    assert rel_err(grad, grad64) < gt
    assert rel_err(g["dNoise"][0].cpu().numpy(), gn64) < gt
    assert np.all(np.triu(grad.transpose(2, 0, 1), 1) == 0.0)
    if T > 1:
        start = [int(x) for x in cx.start.cpu()]
        for has_start in (False, True):
            for forward in (False, True):
                o = _arena(case_viterbi(has_start, forward), cx, ac.NAN_PATTERN, **kw)
                got = unpack_lists(o["pairs"][0].cpu().numpy()[:int(o["offsets"][0][-1])], o["offsets"][0].cpu().numpy())
                assert got == oracle.viterbi(s64, n64, start if has_start else None, forward), (has_start, forward)
    _device_ok(cx)


@pytest.mark.parametrize("which", DEVICES)
def test_public_api_takes_a_misaligned_view(request, which):
    """torch.stack([s, s2])[1] with T*T*B % 4 == 3 through the mirror: the bits of an aligned copy."""
    from transkun_amd import CRF
    dev = _dev(request, which)
    T, B = 33, 7
    s, n = synth.crf_inputs(T, B, 77, "cpu", "randn")
    s2, n2 = synth.crf_inputs(T, B, 78, "cpu", "randn")
    score, noise = torch.stack([s, s2]).to(dev)[1], torch.stack([n, n2]).to(dev)[1]
    assert score.is_contiguous() and score.data_ptr() % 16 != 0 and score.data_ptr() % 4 == 0
    aligned_s, aligned_n = score.clone(), noise.clone()
    assert aligned_s.data_ptr() % 16 == 0

    def everything(sc, no):
        crf = CRF.NeuralSemiCRFInterval(sc, no)
        lz, grad, gn = CRF.forward_backward(sc, no)
        post = crf.posteriors()
        res = [lz, grad, gn] + [getattr(post, f) for f in post._fields] if hasattr(post, "_fields") else [lz, grad, gn]
        lists = [crf.decode(), crf.decode(forward=True), crf.sample(3, generator=torch.Generator().manual_seed(5)), crf.decode_nbest(4)]
        return res, lists
    (ra, la), (rm, lm) = everything(aligned_s, aligned_n), everything(score, noise)
    assert len(ra) == len(rm) > 3
    for a, m in zip(ra, rm):
        assert torch.equal(ac.bits(a), ac.bits(m))
    assert repr(la) == repr(lm)
    if dev.type == "cuda":
        assert _lib.device_status() == 0


@pytest.mark.gpu
def test_public_api_single_chain_misaligned(gpu):
    """One chain runs with a ghost chain appended (the mirror pads a copy): T = 64, NBatch = 1 from a view at phase 4."""
    from transkun_amd import CRF
    T = 64
    s, n = synth.crf_inputs(T, 1, 79, "cpu", "randn")
    flat = torch.zeros(T * T + 1, dtype=F32, device=gpu)
    score = flat[1:].view(T, T, 1)
    score.copy_(s)
    noise = n.to(gpu)
    assert score.data_ptr() % 16 == 4
    a, m = CRF.forward_backward(score.clone(), noise), CRF.forward_backward(score, noise)
    for x, y in zip(a, m):
        assert torch.equal(ac.bits(x), ac.bits(y))
    assert CRF.NeuralSemiCRFInterval(score, noise).decode() == CRF.NeuralSemiCRFInterval(score.clone(), noise).decode()
    assert _lib.device_status() == 0


# ---- group C ------------------------------------------------------------------------------------------------------------------------
def _abi_calls(lib, T, B, K, inp, out, ws, n):
    """Every semi-CRF entry point that takes a workspace, with arguments that pass every other check: inputs all point at `inp`,
    outputs at `out`.  Nothing is dereferenced before the argument checks are through."""
    i, o, z = ctypes.c_void_p(inp), ctypes.c_void_p(out), None
    cap = 2 * T * B
    return {
        "semicrf_logz_fwd": lambda: lib.semicrf_logz_fwd(i, i, T, B, o, o, ws, n, z),
        "semicrf_logz_bwd": lambda: lib.semicrf_logz_bwd(i, i, i, i, i, T, B, o, o, o, ws, n, z),
        "semicrf_logz_bwd_f": lambda: lib.semicrf_logz_bwd_f(i, i, i, i, i, T, B, o, o, o, 1, ws, n, z),
        "semicrf_beta": lambda: lib.semicrf_beta(i, i, T, B, o, ws, n, z),
        "semicrf_viterbi": lambda: lib.semicrf_viterbi(i, i, T, B, None, 0, o, cap, o, ws, n, z),
        "semicrf_sample": lambda: lib.semicrf_sample(i, i, i, T, B, 0, 2, 7, None, o, cap, o, ws, n, z),
        "semicrf_viterbi_nbest": lambda: lib.semicrf_viterbi_nbest(i, i, T, B, 2, None, 1, o, cap, o, o, o, ws, n, z),
        "semicrf_posteriors": lambda: lib.semicrf_posteriors(i, i, i, i, i, T, B, o, o, o, o, o, o, ws, n, z),
        "semicrf_expectation": lambda: lib.semicrf_expectation(i, i, i, i, i, i, T, B, o, o, ws, n, z),
        "semicrf_covariance": lambda: lib.semicrf_covariance(i, i, i, i, i, T, B, o, o, ws, n, z),
        "semicrf_alpha_from": lambda: lib.semicrf_alpha_from(i, i, i, T, B, o, o, ws, n, z),
        "semicrf_eval_path": lambda: lib.semicrf_eval_path(i, i, T, B, i, K, i, o, ws, n, z),
        "semicrf_logprob_fwd": lambda: lib.semicrf_logprob_fwd(i, i, T, B, i, K, i, o, o, o, ws, n, z),
        "semicrf_logprob_fwd_t": lambda: lib.semicrf_logprob_fwd_t(i, i, T, B, i, K, i, o, o, o, None, ws, n, z),
        "semicrf_logprob_bwd": lambda: lib.semicrf_logprob_bwd(i, i, i, i, i, 1, T, B, i, K, i, o, o, ws, n, z),
        "semicrf_logprob_bwd_f": lambda: lib.semicrf_logprob_bwd_f(i, i, i, i, i, 0, T, B, i, K, i, o, o, 1, ws, n, z),
        "semicrf_logprob_bwd_t": lambda: lib.semicrf_logprob_bwd_t(i, i, i, i, i, 1, T, B, i, K, i, o, o, 0, None, ws, n, z),
        "semicrf_marginal_decode": lambda: lib.semicrf_marginal_decode(i, i, i, i, i, T, B, i, 0, o, o, cap, o, ws, n, z),
        "semicrf_marginal_decode_tol": lambda: lib.semicrf_marginal_decode_tol(i, i, i, i, i, T, B, i, 1, 1, 2, o, o, cap, o, ws, n, z),
        "semicrf_mbr_select": lambda: lib.semicrf_mbr_select(i, i, i, K, T, B, i, 0, o, o, cap, o, o, ws, n, z),
    }


def test_c_abi_rejects_a_misaligned_workspace():
    """SEMICRF_EINVAL naming the alignment, with the other argument checks: ahead of the sweeps' prologue and of any HIP call, so it
    is the answer on a machine without a GPU too, and nothing is written."""
    lib = _lib.load()
    T, B, K = 4, 2, 3
    inp = np.zeros(T * T * B + 64, dtype=np.float32)
    out = np.full(T * T * B + 64, ac.NAN_PATTERN, dtype=np.uint32)
    host = np.zeros(4096, dtype=np.uint8)
    base = (host.ctypes.data + 255) // 256 * 256
    names = None
    for offset in (1, 4, 16, 128):
        calls = _abi_calls(lib, T, B, K, inp.ctypes.data, out.ctypes.data, ctypes.c_void_p(base + offset), 1 << 30)
        names = sorted(calls)
        for name, fn in calls.items():
            rc = fn()
            msg = lib.semicrf_last_error().decode()
            assert rc == 1, f"{name} with ws at +{offset}: code {rc} ({msg})"
            assert "256-byte aligned" in msg and " ws " in msg, (name, msg)
    assert len(names) == 20
    assert bool((out == ac.NAN_PATTERN).all()) and not inp.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if n in HAS_WS])
def test_ops_reject_a_misaligned_workspace(gpu, name):
    """The same through torch.ops: a uint8 view ws[1:] is a RuntimeError and the outputs keep their bits."""
    cx = context((17, 12, "model"), gpu)

    class Shifted(ac.Plain):
        def carve(self, nm, shape, dtype, phase=0, align=16):
            if nm != "ws":
                return super().carve(nm, shape, dtype, phase, align)
            return super().carve(nm, (shape[0] + 1,), dtype)[1:]
    plain = Shifted(ac.NAN_PATTERN, gpu)
    kept = {}

    class Keep(Run):
        def out(self, nm, shape, dtype=F32):
            kept[nm] = super().out(nm, shape, dtype)
            return kept[nm]
    with pytest.raises(RuntimeError, match="256-byte aligned"):
        CASES[name](Keep(plain, cx))
    torch.cuda.synchronize(gpu)
    assert kept
    for nm, t in kept.items():
        assert bool((ac.bits(t) == _word(ac.NAN_PATTERN)).all()), nm
    assert _lib.device_status() == 0


STALE_GPU = [pytest.param("gpu", n, id=f"gpu-{n}", marks=pytest.mark.gpu) for n in sorted(CASES) if n in HAS_WS]
STALE_CPU = [pytest.param("cpu", n, id=f"cpu-{n}") for n in sorted(CASES) if n.startswith("expectation")]   # the one host workspace


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which,name", STALE_CPU + STALE_GPU)
def test_workspace_stale_contents(request, which, shape, name):
    """An unleased workspace pre-filled with 0x00, 0xff and pseudo-random bytes: identical result bits (leases keep their own test)."""
    cx = context(shape, _dev(request, which))
    ref = _arena(CASES[name], cx, ac.NAN_PATTERN)
    for fill in (0x00, 0xFF, "random"):
        outs = _arena(CASES[name], cx, ac.NAN_PATTERN, wsfill=fill)
        _same_written(outs, ref, ac.NAN_PATTERN, f"{name}, workspace pre-filled with {fill}")
    _device_ok(cx)
