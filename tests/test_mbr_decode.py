"""MBR path decoding at any threshold: NeuralSemiCRFInterval.decode_mbr[_packed], semicrf_mbr_select.

1. bit-exact against a numpy fp32 restatement of the recursion and the trace (include/semicrf_hip.h), run on the library's own
   lattice decode_marginal_packed(tau) -- and, on the same results,
4. structure: a path (in range, ascending, pairwise compatible, accepted by evalPath), gain = sum(probs - tau), gain >= the
   Viterbi path's value of the same objective (an independent kernel as witness),
2. not a no-op below one half, the plain threshold set above it,
3. float64 truth by path enumeration at T <= 7,
5. capacity, invalid lattices, error codes and argument handling,
6. GPU: determinism, graph capture, memory."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs, unpack_lists
from mbr_common import _mbr_reference
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

TAUS = (0.05, 0.3, 0.5, 0.6, 0.9)
EXTRA_GPU = [(256, 90, "model"), (64, 3, "ties"), (70, 1100, "randn")]
LDS_SWITCH = [(4096, 2, "model"), (4097, 2, "model")]      # mbr_decode.hip: MBR_LDS_T = 4096, F in LDS up to there
EPS = float(np.finfo(np.float32).eps)


def _grad_tol(logz):
    return max(1e-4, 2e-6 * float(np.max(np.abs(np.asarray(logz, np.float64)))))


def _per_chain_tau(B):
    return torch.tensor([0.2 + 0.6 * c / B for c in range(B)], dtype=torch.float32)


def _tau_array(thr, B):
    return thr.numpy().astype(np.float32) if isinstance(thr, torch.Tensor) else np.full(B, thr, np.float32)


# ---- the restatement (_mbr_reference: tests/mbr_common.py) -------------------------------------------------------------------

def _check_structure(crf, T, B, tau, got, what):
    pairs, offsets, probs, gain = got
    assert offsets[0] == 0 and np.all(np.diff(offsets) >= 0) and offsets[-1] == len(probs), what
    if len(pairs):
        assert pairs.min() >= 0 and pairs.max() < T and np.all(pairs[:, 0] <= pairs[:, 1]), what
    for c in range(B):
        p = pairs[offsets[c]:offsets[c + 1]].astype(np.int64)
        assert len(p) <= 2 * T - 1, (what, c)
        key = p[:, 0] * T + p[:, 1]
        assert np.all(np.diff(key) > 0), (what, c)                       # ascending by (begin, end), no cell twice
        # pairwise compatible: an entry begins where the previous one ended or later -- no two open intervals intersect, no
        # singleton lies strictly inside an interval
        assert np.all(p[1:, 0] >= p[:-1, 1]), (what, c)
    paths = unpack_lists(pairs, offsets)
    ev = crf.evalPath(paths)
    assert bool(torch.isfinite(ev).all()), what
    # gain against the float64 sum of its own terms: an fp32 sum of n <= 2 T non-negative terms in any order is within
    # (n - 1) u of the exact sum relative to it, u = eps / 2; the other factor 2 covers the rounding of each w - tau
    ch = np.repeat(np.arange(B), np.diff(offsets))
    terms = probs.astype(np.float64) - tau.astype(np.float64)[ch]
    assert np.all(terms > 0), what
    mine = np.bincount(ch, weights=terms, minlength=B)
    tol = 2 * T * EPS * np.maximum(1.0, mine)
    assert np.all(np.abs(gain.astype(np.float64) - mine) <= tol), (what, float(np.max(np.abs(gain - mine))))
    # MBR can only beat Viterbi on its own objective
    dec = crf.decode()
    dm = crf.interval_marginals(dec)
    for c in range(B):
        m = np.asarray(dm[c], np.float64)
        vit = float(np.sum(m - float(tau[c])))
        tv = 2 * T * EPS * max(1.0, float(mine[c]), float(np.sum(np.abs(m - float(tau[c])))))
        assert float(gain[c]) >= vit - tv, (what, c, float(gain[c]), vit)


def _check_case(s, n, thresholds, structure=True):
    T, B = s.shape[0], s.shape[2]
    crf = CRF.NeuralSemiCRFInterval(s, n)
    for thr in thresholds:
        tau = _tau_array(thr, B)
        lp, lo, lw = crf.decode_marginal_packed(thr)
        want = _mbr_reference(lp, lo, lw, T, tau)
        got = crf.decode_mbr_packed(thr)
        what = f"T={T} B={B} thr={thr if not isinstance(thr, torch.Tensor) else 'per-chain'}"
        assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32 and got[3].dtype == np.float32
        assert got[0].shape == (len(got[2]), 2) and got[1].shape == (B + 1,) and got[3].shape == (B,), what
        assert np.array_equal(got[1], want[1]), what
        assert np.array_equal(got[0], want[0]), what
        assert np.array_equal(got[2].view(np.int32), want[2].view(np.int32)), what
        assert np.array_equal(got[3].view(np.int32), want[3].view(np.int32)), what
        if structure:
            _check_structure(crf, T, B, tau, got, what)


# ---- 1. + 4. bit-exact against the restatement; structure ------------------------------------------------------------------

@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_exact_and_structure_cpu(case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    _check_case(s, n, TAUS + (_per_chain_tau(B),))


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_exact_and_structure_edge_gpu(gpu, case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr, gpu)
    _check_case(s, n, TAUS + (_per_chain_tau(B),))
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind", EXTRA_GPU + LDS_SWITCH)
def test_exact_and_structure_gpu(gpu, T, B, kind):
    s, n = synth.crf_inputs(T, B, 7 + T + B, gpu, kind)
    _check_case(s, n, TAUS + (_per_chain_tau(B),))
    assert _lib.device_status() == 0


def test_ties_inputs_hold_ties_cpu():
    """the "ties" inputs hold marginals of exactly 0.5 (the strict compare: not eligible at 0.5) and equal candidates"""
    s, n = synth.crf_inputs(48, 9, 20, "cpu", "ties")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    lat = crf.decode_marginal_packed(0.5)
    assert (lat[2] == 0.5).any()
    got = crf.decode_mbr_packed(0.5)
    assert not (got[2] == 0.5).any() and (got[2] > 0.5).all()


# ---- 2. not a no-op --------------------------------------------------------------------------------------------------------

def _sets(pairs, offsets, keep=None):
    B = len(offsets) - 1
    out = []
    for c in range(B):
        sl = slice(int(offsets[c]), int(offsets[c + 1]))
        p = pairs[sl] if keep is None else pairs[sl][keep[sl]]
        out.append({(int(b), int(e)) for b, e in p})
    return out


@pytest.mark.parametrize("name", ["T24_B63", "T40_B90"])
def test_differs_from_threshold_set_below_one_half_cpu(name):
    case = next(c for c in EDGE_CASES if c[0] == name)
    _, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    differs = {}
    for tau in (0.05, 0.3):
        lp, lo, lw = crf.decode_marginal_packed(tau)
        plain = _sets(lp, lo, lw > np.float32(tau))
        got = crf.decode_mbr_packed(tau)
        mbr = _sets(got[0], got[1])
        assert all(a <= b for a, b in zip(mbr, plain))                   # only cells above the threshold are ever used
        differs[tau] = sum(a != b for a, b in zip(mbr, plain))
    print(f"{name}: differs in {differs[0.05]} / {B} chains at 0.05, {differs[0.3]} / {B} at 0.3")
    assert differs[0.05] == B
    assert 2 * differs[0.3] >= B


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_equals_threshold_set_above_one_half_cpu(case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    for tau in (float(np.nextafter(np.float32(0.5), np.float32(1))), 0.6, 0.9):
        lp, lo, lw = crf.decode_marginal_packed(tau)
        keep = lw > np.float32(tau)                                      # (the entries with probs == tau removed)
        ch = np.repeat(np.arange(B), np.diff(lo))
        want_off = np.concatenate([[0], np.cumsum(np.bincount(ch[keep], minlength=B))]).astype(np.int32)
        got = crf.decode_mbr_packed(tau)
        assert np.array_equal(got[1], want_off), tau
        assert np.array_equal(got[0], lp[keep]), tau
        assert np.array_equal(got[2].view(np.int32), lw[keep].view(np.int32)), tau


# ---- 3. float64 truth by path enumeration ----------------------------------------------------------------------------------

def _enumerate(T):
    """(cells [ncell, 2] ascending by (begin, end), P [npath, ncell] path-cell incidence, G [npath, T-1] the noise gaps)"""
    cells = [(b, e) for b in range(T) for e in range(b, T)]
    index = {c: i for i, c in enumerate(cells)}
    rows, gaps = [], []

    def walk(t, acc, cov):
        for single in (False, True):
            cur = acc + ([index[(t, t)]] if single else [])
            if t == T - 1:
                rows.append(cur); gaps.append(cov)
                continue
            walk(t + 1, cur, cov)
            for e in range(t + 1, T):
                walk(e, cur + [index[(t, e)]], cov + list(range(t, e)))
    walk(0, [], [])
    P = np.zeros((len(rows), len(cells)))
    G = np.ones((len(rows), max(T - 1, 0)))
    for i, (r, cv) in enumerate(zip(rows, gaps)):
        P[i, r] = 1.0
        G[i, cv] = 0.0
    return np.asarray(cells, np.int64).reshape(-1, 2), P, G


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_float64_enumeration_cpu(T):
    B = 4
    s, n = synth.crf_inputs(T, B, 30 + T, "cpu", "randn")
    cells, P, G = _enumerate(T)
    if T == 7:
        assert len(P) == 15564
    s64, n64 = s.double().numpy(), n.double().numpy()
    lut = {(int(b), int(e)): i for i, (b, e) in enumerate(cells)}
    marg, tol = [], []
    for c in range(B):
        sc = P @ s64[cells[:, 1], cells[:, 0], c] + (G @ n64[:, c] if T > 1 else 0.0)
        logz = float(np.logaddexp.reduce(sc))
        marg.append(P.T @ np.exp(sc - logz))                             # float64 marginal of every cell
        tol.append(2 * T * _grad_tol(logz))
    for tau in (0.05, 0.15, 0.3, 0.5):
        pairs, offsets, probs, gain = CRF.decode_mbr_packed(s, n, tau)
        for c in range(B):
            optimum = float(np.max(P @ (marg[c] - tau)))
            assert abs(float(gain[c]) - optimum) <= tol[c], (T, c, tau, float(gain[c]), optimum)
            mine = pairs[offsets[c]:offsets[c + 1]]
            true_gain = sum(marg[c][lut[(int(b), int(e))]] - tau for b, e in mine)
            assert true_gain >= optimum - 2 * tol[c], (T, c, tau, true_gain, optimum)


# ---- 5. capacity and errors ------------------------------------------------------------------------------------------------

def test_abi_argument_checks():
    """argument checks that return before anything touches a device (the buffers are never dereferenced)"""
    lib = _lib.load()
    assert lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, 64, 8) > 0
    T, B = 1024, 352                         # of the order of T * B words, never T * T * B
    assert lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, T, B) <= 8 * 4 * T * B + (1 << 16)
    assert lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, 4097, 2) > lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, 4096, 2) + 4 * 4096 * 2
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    T, B = 4, 2
    good = dict(pairs=p, weight=p, offsets=p, K=8, T=T, B=B, tau=p, tau_stride=0, pairs_out=p, probs_out=p, cap=8, offsets_out=p,
                gain=p, ws=p, ws_bytes=1 << 20, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.semicrf_mbr_select(a["pairs"], a["weight"], a["offsets"], a["K"], a["T"], a["B"], a["tau"], a["tau_stride"],
                                      a["pairs_out"], a["probs_out"], a["cap"], a["offsets_out"], a["gain"], a["ws"], a["ws_bytes"],
                                      a["stream"])

    EINVAL, EWORKSPACE = 1, 2
    for name in ("pairs", "weight", "offsets", "tau", "pairs_out", "probs_out", "offsets_out", "gain", "ws"):
        assert call(**{name: None}) == EINVAL, name
    assert call(T=0) == EINVAL and call(B=0) == EINVAL
    assert call(tau_stride=2) == EINVAL and call(tau_stride=-1) == EINVAL
    assert call(cap=-1) == EINVAL and call(K=-1) == EINVAL
    assert call(T=1 << 20, B=1 << 11) == EINVAL                          # 2 T B would not fit int32 offsets
    need = lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, T, B)
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert b"workspace" in lib.semicrf_last_error()


def _select_op(lat, T, tau, cap, B, device, guard=8):
    """torch.ops.semicrf.mbr_select on a lattice with output buffers of `cap` entries followed by guard words"""
    GUARD = 0x5A5A5A5A
    pb = torch.full((cap + guard, 2), GUARD, dtype=torch.int32, device=device)
    fb = torch.full((cap + guard,), GUARD, dtype=torch.int32, device=device)
    ob = torch.full((B + 1 + guard,), GUARD, dtype=torch.int32, device=device)
    gb = torch.full((B + guard,), GUARD, dtype=torch.int32, device=device)
    ws = _lib.workspace(_lib.OP_MBR_SELECT, T, B, device)
    _lib.ops().mbr_select(lat[0], lat[2], lat[1], T, tau, pb[:cap], fb[:cap].view(torch.float32), ob[:B + 1], gb[:B].view(torch.float32), ws)
    for x, k in ((pb, cap), (fb, cap), (ob, B + 1), (gb, B)):
        assert bool((x[k:] == GUARD).all())                              # nothing written past the buffers
    return pb[:cap], fb[:cap].view(torch.float32), ob[:B + 1], gb[:B].view(torch.float32)


def _capacity(device):
    T, B = 96, 37
    s, n = synth.crf_inputs(T, B, 5, device, "model")
    tau = torch.full((1,), 0.3, device=device)
    with torch.no_grad():
        lat = crf_mod._marginal_decode_raw(s, n, tau, 4 * T * B)
    K = lat[0].shape[0]
    lat_total = int(lat[1][-1])
    assert 0 < lat_total <= K
    full = [x.cpu() for x in _select_op(lat, T, tau, 2 * T * B, B, device)]
    total = int(full[2][-1])
    assert total > 2
    want = _mbr_reference(lat[0][:lat_total].cpu().numpy(), lat[1].cpu().numpy(), lat[2][:lat_total].cpu().numpy(), T, np.full(B, 0.3, np.float32))
    assert np.array_equal(full[2].numpy(), want[1]) and np.array_equal(full[0][:total].numpy(), want[0])
    assert np.array_equal(full[1][:total].numpy().view(np.int32), want[2].view(np.int32))
    assert np.array_equal(full[3].numpy().view(np.int32), want[3].view(np.int32))
    for cap in (1, total - 1):
        pb, fb, ob, gb = [x.cpu() for x in _select_op(lat, T, tau, cap, B, device)]
        assert torch.equal(ob, full[2])                                  # exact although it does not fit
        assert torch.equal(pb, full[0][:cap]) and torch.equal(fb.view(torch.int32), full[1][:cap].view(torch.int32))
        assert torch.equal(gb.view(torch.int32), full[3].view(torch.int32))
    # a negative lattice total (the sweeps' NaN convention) and a truncated lattice (total > K): -1, nothing selected
    neg = lat[1].clone()
    neg[-1] = -1
    for bad in ((lat[0], neg, lat[2]), (lat[0][:lat_total - 1], lat[1], lat[2][:lat_total - 1])):
        pb, fb, ob, gb = [x.cpu() for x in _select_op(bad, T, tau, 2 * T * B, B, device)]
        assert int(ob[-1]) == -1 and bool((ob[:-1] == 0).all()) and bool((gb == 0).all())
    # an empty lattice (K = 0) selects nothing
    empty = (lat[0][:0], torch.zeros(B + 1, dtype=torch.int32, device=device), lat[2][:0])
    pb, fb, ob, gb = [x.cpu() for x in _select_op(empty, T, tau, 4, B, device)]
    assert bool((ob == 0).all()) and bool((gb == 0).all())


def test_capacity_cpu():
    _capacity("cpu")


@pytest.mark.gpu
def test_capacity_gpu(gpu):
    _capacity(gpu)
    # cap = 0 and a short workspace through the C ABI
    T, B = 96, 37
    s, n = synth.crf_inputs(T, B, 5, gpu, "model")
    tau = torch.full((1,), 0.3, device=gpu)
    with torch.no_grad():
        lat = crf_mod._marginal_decode_raw(s, n, tau, 4 * T * B)
        want = crf_mod._mbr_select_raw(lat[0], lat[2], lat[1], T, tau)
    lib = _lib.load()
    need = lib.semicrf_workspace_bytes(_lib.OP_MBR_SELECT, T, B)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    GUARD = 0x5A5A5A5A
    pb = torch.full((8, 2), GUARD, dtype=torch.int32, device=gpu)
    fb = torch.full((8,), GUARD, dtype=torch.int32, device=gpu)
    ob = torch.full((B + 1 + 8,), GUARD, dtype=torch.int32, device=gpu)
    gb = torch.empty(B, dtype=torch.float32, device=gpu)
    args = (vp(lat[0]), vp(lat[2]), vp(lat[1]), lat[0].shape[0], T, B, vp(tau), 0, vp(pb), vp(fb), 0, vp(ob), vp(gb), vp(ws))
    assert lib.semicrf_mbr_select(*args, need, st) == 0, lib.semicrf_last_error()
    torch.cuda.synchronize(gpu)
    assert torch.equal(ob[:B + 1], want[1]) and bool((ob[B + 1:] == GUARD).all())
    assert bool((pb == GUARD).all()) and bool((fb == GUARD).all())
    assert torch.equal(gb.view(torch.int32), want[3].view(torch.int32))
    assert lib.semicrf_mbr_select(*args, need - 1, st) == 2
    assert _lib.device_status() == 0


def _arguments(device):
    T, B = 12, 3
    s, n = synth.crf_inputs(T, B, 41, device, "randn")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    for bad in (0, 0.0, -1, 1.5, float("nan"), None, "0.5", True):
        with pytest.raises(ValueError, match="decode_mbr"):
            crf.decode_mbr_packed(bad)
        with pytest.raises(ValueError, match="decode_mbr"):
            crf.decode_mbr(bad)
    with pytest.raises(ValueError, match="decode_marginal"):            # the other entry point keeps its messages
        crf.decode_marginal_packed(1.5)
    with pytest.raises(ValueError):
        crf.decode_mbr_packed(torch.full((B + 1,), 0.5))
    with pytest.raises(ValueError):
        crf.decode_mbr_packed(torch.full((B,), 1, dtype=torch.int64))
    with pytest.raises(TypeError):
        crf.decode_mbr_packed()                      # no default threshold
    with pytest.raises(AssertionError):
        CRF.decode_mbr_packed(s[:, :-1], n, 0.5)
    want = crf.decode_mbr_packed(0.2)
    same = lambda a, b: all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
    # a threshold tensor on another device is moved; a float64 tensor is taken as float32
    assert same(crf.decode_mbr_packed(torch.full((B,), 0.2, dtype=torch.float64)), want)
    # no gradient flows, whatever the inputs require
    sg, ng = s.clone().requires_grad_(), n.clone().requires_grad_()
    assert same(CRF.decode_mbr_packed(sg, ng, 0.2), want)
    # other float dtypes are computed as .float()
    for dt in (torch.bfloat16, torch.float16):
        sd, nd = s.to(dt), n.to(dt)
        assert same(CRF.decode_mbr_packed(sd, nd, 0.2), CRF.decode_mbr_packed(sd.float(), nd.float(), 0.2))
    # the module-level names, the class and the list form agree
    assert same(CRF.decode_mbr_packed(s, n, 0.2), want)
    paths, probs, gain = crf.decode_mbr(0.2)
    paths2, probs2, gain2 = CRF.decode_mbr(s, n, 0.2)
    assert paths == paths2 and probs == probs2 and np.array_equal(gain, gain2) and np.array_equal(gain, want[3])
    assert paths == unpack_lists(want[0], want[1])
    assert [x for lst in probs for x in lst] == want[2].tolist()
    assert crf.interval_marginals(paths) == probs
    assert bool(torch.isfinite(crf.logProb(paths)).all())
    # T = 1 and T = 2
    for Ts in (1, 2):
        s1, n1 = synth.crf_inputs(Ts, 4, 50 + Ts, device, "randn")
        _check_case(s1, n1, (0.05, 0.3, 0.5, 0.9, _per_chain_tau(4)))
    # a threshold tensor whose lattice exceeds 2 T per chain: rerun with the exact size, never a truncation
    s2, n2 = synth.crf_inputs(24, 6, 61, device, "randn")
    low = torch.full((6,), 0.004)
    lat = CRF.decode_marginal_packed(s2, n2, low)
    assert int(lat[1][-1]) > 2 * 24 * 6
    _check_case(s2, n2, (low,))


def test_arguments_cpu():
    _arguments("cpu")


@pytest.mark.gpu
def test_arguments_gpu(gpu):
    _arguments(gpu)
    assert _lib.device_status() == 0


def test_poisoned_alpha_cpu():
    s, n = synth.crf_inputs(8, 2, 44, "cpu", "randn")
    s[3, 1, 0] = float("nan")
    with pytest.raises(RuntimeError):
        CRF.decode_mbr_packed(s, n, 0.3)


@pytest.mark.gpu
def test_single_chain_gpu(gpu):
    """one chain runs with a ghost chain appended (as decode does): the ghost's cells must not show"""
    s, n = synth.crf_inputs(200, 1, 9, gpu, "model")
    _check_case(s, n, (0.05, 0.5, torch.tensor([0.3])))
    assert _lib.device_status() == 0


# ---- 6. GPU: determinism, graph capture, memory -----------------------------------------------------------------------------

@pytest.mark.gpu
def test_deterministic_and_memory_gpu(gpu):
    T, B = 256, 90
    s, n = synth.crf_inputs(T, B, 12, gpu, "model")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    r1 = crf.decode_mbr_packed(0.3)           # (leased sweep workspaces are set up once)
    torch.cuda.synchronize(gpu)
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    r2 = crf.decode_mbr_packed(0.3)
    torch.cuda.synchronize(gpu)
    peak = torch.cuda.max_memory_allocated(gpu) - base
    assert len(r1[2]) > 0
    for a, b in zip(r1, r2):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))                # bit-identical
    assert peak < 4 * T * T * B, peak / 2 ** 20                                   # below ONE [T, T, B] fp32 tensor
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    T, B = 333, 46
    tau = _per_chain_tau(B).to(gpu)
    lats = []
    with torch.no_grad():
        for i in range(3):
            s, n = synth.crf_inputs(T, B, 600 + i, gpu)
            lats.append(crf_mod._marginal_decode_raw(s, n, tau, 6 * T * B))
    assert all(0 < int(l[1][-1]) <= 6 * T * B for l in lats)
    select = lambda l: list(crf_mod._mbr_select_raw(l[0], l[2], l[1], T, tau))

    def trimmed(out):
        pairs, offsets, probs, gain = out
        k = int(offsets[-1])
        return [pairs[:k].clone(), offsets.clone(), probs[:k].clone(), gain.clone()]

    want = [trimmed(select(l)) for l in lats]
    buf = [x.clone() for x in lats[0]]
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(2):
            select(buf)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = select(buf)
    for i in (1, 2, 0, 1):
        for dst, src in zip(buf, lats[i]):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize(gpu)
        for a, b in zip(trimmed(got), want[i]):
            assert torch.equal(a, b), i
    assert _lib.device_status() == 0
