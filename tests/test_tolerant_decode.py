"""Onset/offset-tolerant interval posteriors and decoding: the `tolerance` keyword of interval_marginals[_packed],
decode_marginal[_packed] and decode_mbr[_packed]; semicrf_interval_marginals_tol, semicrf_marginal_decode_tol.

1. the order of the sums is pinned: the gather equals a numpy float32 restatement of the header's definition, bit for bit,
2. the decode equals the gather exactly (offsets, pairs, probs bit for bit),
3. tolerance None and (0, 0) are the tolerance-free results, bit for bit, for all six functions,
4. the selections are nested in every tolerance component,
5. against float64 truth (the oracle's dense marginals, box-summed in float64; exact enumeration for T <= 7) with a relative band
   whose share of undecided cells is bounded from the reference alone,
6. the case the feature exists for: an onset spread over two frames,
7. MBR over the tolerant lattice: the header's recursion bit for bit, a path, a gain no path of the other decoders beats,
8. capacity, error codes, argument handling, graph capture,
9. full size on the GPU: determinism, order, memory."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs
from mbr_common import _mbr_reference
from test_marginal_decode import F64_CASES, _cells, _enumerate_marginals, _grad_tol, _per_chain_tau
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

TOLS = ((1, 0), (0, 3), (2, 2), (8, 8))
THRS = (0.3, 0.6)
# halos that cross one and two tile edges, chain counts off the quad and off the 32-chain piece, a lone chain
SHAPES = [(63, 5, "model"), (64, 33, "randn"), (65, 37, "ties"), (130, 37, "model"), (200, 1, "model")]
CASES = [(c[0],) + tuple(c[1:]) for c in EDGE_CASES] + [(f"T{T}_B{B}_{kind}", T, B, kind, 300 + T + B, None) for T, B, kind in SHAPES]
CASE_IDS = [c[0] for c in CASES]


def _inputs(case, device="cpu"):
    name, T, B, kind, seed, tr = case
    return edge_inputs(T, B, kind, seed, tr, device)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the library's values of every cell, computed once per (case, device, tolerance) and shared, never modified ----------------

_ALL = {}


def _all_cells(case, device, tol):
    """(crf, pairs [B * n, 2], M float32 [B, n]) for every cell b <= e of every chain, ascending by (begin, end)"""
    key = (case[0], torch.device(device).type, tol)
    if key not in _ALL:
        s, n = _inputs(case, device)
        T, B = s.shape[0], s.shape[2]
        cells = _cells(T)
        pairs = np.tile(cells, (B, 1))
        offsets = (np.arange(B + 1, dtype=np.int64) * len(cells)).astype(np.int32)
        crf = CRF.NeuralSemiCRFInterval(s, n)
        m = crf.interval_marginals_packed(pairs, offsets, tolerance=tol).cpu().numpy()
        assert m.dtype == np.float32
        m = m.reshape(B, len(cells))
        m.setflags(write=False)
        _ALL[key] = (crf, pairs, m)
    return _ALL[key]


# ---- 1. the order is pinned ------------------------------------------------------------------------------------------------------

def _restate(m_cells, T, db, de):
    """The header's definition in numpy float32, on the exact-cell values m_cells [B, n] (cells ascending by (begin, end)): a term
    that does not exist is SKIPPED (np.where keeps the accumulator), every other term is one np.float32 add, in the stated order."""
    B = m_cells.shape[0]
    cells = _cells(T)
    m = np.zeros((T, T, B), np.float32)                           # [e, b, chain]; the cells b > e are never read
    m[cells[:, 1], cells[:, 0]] = m_cells.T
    e = np.arange(T)[:, None]
    b = np.arange(T)[None, :]
    rows = np.zeros((T, T, B), np.float32)                        # rows[e', b] = row(e') of the box around column b
    for j in range(-db, db + 1):                                  # b' = b + j ascending
        bp = b + j
        valid = (bp >= 0) & (bp <= e)
        term = m[e, np.clip(bp, 0, T - 1)]
        acc = rows + term
        assert acc.dtype == np.float32
        rows = np.where(valid[:, :, None], acc, rows)
    M = np.zeros((T, T, B), np.float32)
    for i in range(-de, de + 1):                                  # e' = e + i ascending
        ep = e + i
        valid = (ep >= 0) & (ep <= T - 1) & (ep >= np.maximum(0, b - db))          # a row without a cell contributes nothing
        term = rows[np.clip(ep, 0, T - 1), b]
        acc = M + term
        assert acc.dtype == np.float32
        M = np.where(valid[:, :, None], acc, M)
    with np.errstate(invalid="ignore"):
        M = np.where(M > np.float32(1.0), np.float32(1.0), M)     # clamp1: NaN stays NaN
    return np.ascontiguousarray(M[cells[:, 1], cells[:, 0]].T)    # [B, n]


def _order_pinned(case, device):
    T = case[1]
    _, _, m = _all_cells(case, device, (0, 0))
    for tol in TOLS:
        _, _, M = _all_cells(case, device, tol)
        want = _restate(m, T, *tol)
        bad = _bits(M) != _bits(want)
        assert not bad.any(), (case[0], tol, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_order_pinned_cpu(case):
    _order_pinned(case, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_order_pinned_gpu(gpu, case):
    _order_pinned(case, gpu)
    assert _lib.device_status() == 0


def test_restatement_is_the_literal_definition():
    """the vectorised restatement above against the definition written as plain loops, on a small triangle"""
    rng = np.random.default_rng(5)
    T, B = 9, 2
    cells = _cells(T)
    m_cells = rng.random((B, len(cells)), dtype=np.float32) * np.float32(0.3)
    at = {(int(b), int(e)): i for i, (b, e) in enumerate(cells)}
    for db, de in ((1, 0), (0, 3), (2, 2), (8, 8)):
        got = _restate(m_cells, T, db, de)
        for c in range(B):
            for i, (b, e) in enumerate(cells):
                acc = np.float32(0.0)
                for ep in range(max(0, e - de), min(T - 1, e + de) + 1):
                    row = np.float32(0.0)
                    for bp in range(max(0, b - db), min(b + db, ep) + 1):
                        row = row + m_cells[c, at[(bp, ep)]]
                    acc = acc + row
                acc = np.float32(1.0) if acc > 1 else acc
                assert _bits(acc) == _bits(got[c, i]), (db, de, c, b, e)


# ---- 2. decode equals the gather, exactly ----------------------------------------------------------------------------------------

def _decode_exact(case, device):
    B = case[2]
    for tol in TOLS:
        crf, pairs_all, M = _all_cells(case, device, tol)
        for thr in THRS + (_per_chain_tau(B),):
            tau = thr.numpy() if isinstance(thr, torch.Tensor) else np.full(B, thr, np.float32)
            with np.errstate(invalid="ignore"):
                sel = M >= tau[:, None]                               # fp32 compare; NaN selects nothing
            pairs, offsets, probs = crf.decode_marginal_packed(thr, tolerance=tol)
            assert pairs.dtype == np.int32 and offsets.dtype == np.int32 and probs.dtype == np.float32
            assert pairs.shape == (len(probs), 2) and offsets.shape == (B + 1,)
            want_off = np.concatenate([[0], np.cumsum(sel.sum(1))])
            assert np.array_equal(offsets, want_off), (case[0], tol, thr)
            assert np.array_equal(pairs, pairs_all[sel.ravel()]), (case[0], tol, thr)
            assert np.array_equal(_bits(probs), _bits(M[sel])), (case[0], tol, thr)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decode_equals_gather_cpu(case):
    _decode_exact(case, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_decode_equals_gather_gpu(gpu, case):
    _decode_exact(case, gpu)
    assert _lib.device_status() == 0


# ---- 3. (0, 0) and None are today's results --------------------------------------------------------------------------------------

def _same(a, b):
    """bit for bit: tuples of results member by member, tensors and arrays by their words, lists (paths, probabilities) by =="""
    if isinstance(a, tuple):
        return isinstance(b, tuple) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a == b


def _zero_tolerance(device):
    for T, B, kind in ((70, 20, "model"), (33, 1, "randn")):
        s, n = synth.crf_inputs(T, B, 90 + T, device, kind)
        crf = CRF.NeuralSemiCRFInterval(s, n)
        dec = crf.decode()
        p, o = crf.decode_packed()
        tt = _per_chain_tau(B)
        for zero in (None, 0, (0, 0), [0, 0], np.int64(0)):
            assert _same(crf.interval_marginals(dec, tolerance=zero), crf.interval_marginals(dec))
            assert _same(crf.interval_marginals_packed(p, o, tolerance=zero), crf.interval_marginals_packed(p, o))
            for thr in (0.3, 0.6, tt):
                assert _same(crf.decode_marginal(thr, tolerance=zero), crf.decode_marginal(thr))
                assert _same(crf.decode_marginal_packed(thr, tolerance=zero), crf.decode_marginal_packed(thr))
                assert _same(crf.decode_mbr_packed(thr, tolerance=zero), crf.decode_mbr_packed(thr))
                assert _same(crf.decode_mbr(thr, tolerance=zero), crf.decode_mbr(thr))
        # the module-level names take the keyword too
        assert _same(CRF.interval_marginals(s, n, dec, tolerance=0), crf.interval_marginals(dec))
        assert _same(CRF.interval_marginals_packed(s, n, p, o, tolerance=0), crf.interval_marginals_packed(p, o))
        assert _same(CRF.decode_marginal_packed(s, n, 0.4, tolerance=(0, 0)), crf.decode_marginal_packed(0.4))
        assert _same(CRF.decode_mbr_packed(s, n, 0.4, tolerance=(0, 0)), crf.decode_mbr_packed(0.4))


def test_zero_tolerance_is_todays_result_cpu():
    _zero_tolerance("cpu")


@pytest.mark.gpu
def test_zero_tolerance_is_todays_result_gpu(gpu):
    _zero_tolerance(gpu)
    assert _lib.device_status() == 0


def _abi_zero_forwards(device):
    """the C entry points with (0, 0) against the entry points they extend (through the torch ops, on either device)"""
    T, B = 40, 6
    s, n = synth.crf_inputs(T, B, 17, device, "model")
    lvq = crf_mod._marginal_inputs(s, n)
    tau = torch.full((1,), 0.4, device=s.device)
    a = crf_mod._marginal_decode_raw(s, n, tau, None, lvq)
    pairs, probs = torch.empty_like(a[0]), torch.empty_like(a[2])
    offsets = torch.empty_like(a[1])
    ws = _lib.workspace(_lib.OP_MARGINAL_DECODE_TOL, T, B, s.device)
    _lib.ops().marginal_decode_tol(s, n, lvq[1], lvq[2], lvq[0], tau, 0, 0, pairs, probs, offsets, ws)
    k = int(a[1][-1])
    assert k > 0 and torch.equal(offsets, a[1]) and torch.equal(pairs[:k], a[0][:k])
    assert torch.equal(probs[:k].view(torch.int32), a[2][:k].view(torch.int32))
    out = torch.empty(k, dtype=torch.float32, device=s.device)
    _lib.ops().interval_marginals_tol(s, lvq[1], lvq[2], lvq[0], pairs[:k].contiguous(), k, offsets, 0, 0, out)
    assert torch.equal(out.view(torch.int32), probs[:k].view(torch.int32))


def test_abi_zero_forwards_cpu():
    _abi_zero_forwards("cpu")


@pytest.mark.gpu
def test_abi_zero_forwards_gpu(gpu):
    _abi_zero_forwards(gpu)
    assert _lib.device_status() == 0


# ---- 4. nesting ------------------------------------------------------------------------------------------------------------------

def _nesting(device):
    """fp32 sums of non-negative terms are monotone in the set of terms, so the selection can only grow with a tolerance component"""
    tols = ((0, 0),) + TOLS
    for T, B, kind, seed in ((130, 37, "model", 5), (64, 3, "ties", 71)):
        s, n = synth.crf_inputs(T, B, seed, device, kind)
        crf = CRF.NeuralSemiCRFInterval(s, n)
        for thr in THRS:
            sets = {}
            for tol in tols:
                p, o, _ = crf.decode_marginal_packed(thr, tolerance=tol)
                c = np.repeat(np.arange(B), np.diff(o)).astype(np.int64)
                sets[tol] = set(((c * T + p[:, 0]) * T + p[:, 1]).tolist())
            assert len(sets[(0, 0)]) > 0
            for small in tols:
                for big in tols:
                    if small != big and small[0] <= big[0] and small[1] <= big[1]:
                        assert sets[small] <= sets[big], (T, thr, small, big)
            assert len(sets[(8, 8)]) > len(sets[(0, 0)])


def test_nesting_cpu():
    _nesting("cpu")


@pytest.mark.gpu
def test_nesting_gpu(gpu):
    _nesting(gpu)
    assert _lib.device_status() == 0


# ---- 5. float64 truth ------------------------------------------------------------------------------------------------------------

def _box_f64(marg, db, de):
    """The uncapped float64 box sum U[e, b, c] of a dense marginal tensor marg[e, b, c] (anything above the diagonal is ignored)."""
    T = marg.shape[0]
    low = np.tril(np.ones((T, T), bool))[:, :, None]
    m = np.where(low, marg, 0.0)
    pad = np.zeros((T, T + 2 * db, marg.shape[2]))
    pad[:, db:db + T] = m
    rows = np.zeros((T + 2 * de,) + m.shape[1:])                   # float64: the order of the sums is of no concern here
    for j in range(2 * db + 1):
        rows[de:de + T] += pad[:, j:j + T]
    U = np.zeros_like(m)
    for i in range(2 * de + 1):
        U += rows[i:i + T]
    return np.where(low, U, 0.0)


def _band_is_narrow(U, tau, band):
    """From the float64 reference ALONE: the cells the band leaves undecided are at most 10 % of the selected ones + 2."""
    T = U.shape[0]
    low = np.tril(np.ones((T, T), bool))[:, :, None]
    M = np.minimum(U, 1.0)
    selected = int((low & (M >= tau)).sum())
    undecided = int((low & (M >= tau - band) & (M < tau + band)).sum())
    return undecided, selected, undecided <= 0.1 * selected + 2


def _check_banded(U, tau, band, pairs, offsets, probs, what):
    """Every cell with float64 M >= tau + band is selected, none < tau - band is, probs within the band of the truth"""
    T, B = U.shape[0], U.shape[2]
    M = np.minimum(U, 1.0)
    got = np.zeros((T, T, B), bool)
    c = np.repeat(np.arange(B), np.diff(offsets))
    b, e = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    assert np.all(b <= e), what
    got[e, b, c] = True
    assert got.sum() == len(probs), f"{what}: a cell appears twice"
    low = np.tril(np.ones((T, T), bool))[:, :, None]
    must = low & (M >= tau + band)
    never = low & (M < tau - band)
    assert not (must & ~got).any(), f"{what}: {int((must & ~got).sum())} sure cells missing"
    assert not (never & got).any(), f"{what}: {int((never & got).sum())} cells below the band selected"
    err = np.abs(probs.astype(np.float64) - M[e, b, c])
    assert err.size == 0 or np.all(err <= band[e, b, c]), f"{what}: probs off by {err.max()}"


F64_EXTRA = [(256, 90, 7, "model"), (64, 3, 71, "ties"), (70, 130, 207, "randn"), (130, 37, 5, "model")]
F64_ALL = [("edge",) + tuple(c) for c in F64_CASES] + [("synth", f"T{T}_B{B}_{kind}", T, B, kind, seed, None) for T, B, seed, kind in F64_EXTRA]


def _f64(oracle, entry, device, scale):
    src, name, T, B, kind, seed, tr = entry
    s, n = edge_inputs(T, B, kind, seed, tr) if src == "edge" else synth.crf_inputs(T, B, seed, "cpu", kind)
    lz, grad, _, _, _ = oracle.forward_backward_f64(s.numpy(), n.numpy())
    crf = CRF.NeuralSemiCRFInterval(s.to(device), n.to(device))
    for tol in TOLS:
        U = _box_f64(grad, *tol)
        band = scale * _grad_tol(lz) * np.maximum(1.0, U)          # relative: every m carries a relative error
        for tau in THRS:
            und, sel, ok = _band_is_narrow(U, tau, band)
            print(f"{name} tol={tol} tau={tau}: undecided {und} of {sel} selected")
            assert ok, (name, tol, tau, und, sel)                  # (before the library is called)
            pairs, offsets, probs = crf.decode_marginal_packed(tau, tolerance=tol)
            _check_banded(U, tau, band, pairs, offsets, probs, f"{name} tol={tol} tau={tau}")


@pytest.mark.parametrize("entry", F64_ALL, ids=[e[1] for e in F64_ALL])
def test_f64_truth_cpu(oracle, entry):
    _f64(oracle, entry, "cpu", 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", F64_ALL, ids=[e[1] for e in F64_ALL])
def test_f64_truth_gpu(oracle, gpu, entry):
    _f64(oracle, entry, gpu, 4.0)
    assert _lib.device_status() == 0


def _enumeration(T, device):
    parts = [synth.crf_inputs(T, 1, sd, "cpu", kind) for sd, kind in zip((3, 4, 5), ("randn", "model", "ties"))]
    s = torch.cat([p[0] for p in parts], 2).contiguous()
    n = torch.cat([p[1] for p in parts], 1).contiguous()
    marg = _enumerate_marginals(s, n)
    for tol in TOLS:
        U = _box_f64(marg, *tol)
        band = np.full(U.shape, 1e-5)
        for tau in THRS:
            und, sel, ok = _band_is_narrow(U, tau, band)
            print(f"T={T} tol={tol} tau={tau}: undecided {und} of {sel} selected")
            assert ok, (T, tol, tau, und, sel)
            pairs, offsets, probs = CRF.decode_marginal_packed(s.to(device), n.to(device), tau, tolerance=tol)
            _check_banded(U, tau, band, pairs, offsets, probs, f"T={T} tol={tol} tau={tau}")


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_exact_enumeration_cpu(T):
    _enumeration(T, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_exact_enumeration_gpu(gpu, T):
    _enumeration(T, gpu)
    assert _lib.device_status() == 0


# ---- 6. the case the feature exists for ------------------------------------------------------------------------------------------

def _spread_onset(device):
    """a note whose onset the model places at frame 4 or 5 with about equal weight: certain under a +-1 frame onset window, yet
    neither exact cell reaches 0.6"""
    T = 16
    s = torch.full((T, T, 2), -20.0)
    n = torch.zeros(T - 1, 2)
    s[10, 4] = 10.0
    s[10, 5] = 10.2
    crf = CRF.NeuralSemiCRFInterval(s.to(device), n.to(device))
    paths, probs, _ = crf.decode_mbr(0.6)
    assert all(e == b for path in paths for b, e in path)
    paths, probs, _ = crf.decode_mbr(0.6, tolerance=(1, 0))
    for c in range(2):
        notes = [(iv, p) for iv, p in zip(paths[c], probs[c]) if iv[1] > iv[0]]
        assert len(notes) == 1 and notes[0][0] in ((4, 10), (5, 10)) and notes[0][1] >= 0.99, notes
    tolerant = crf.interval_marginals([[(4, 10)]] * 2, tolerance=(1, 0))
    exact = crf.interval_marginals([[(4, 10)]] * 2)
    assert all(x[0] >= 0.99 for x in tolerant) and all(x[0] < 0.5 for x in exact), (tolerant, exact)


def test_spread_onset_cpu():
    _spread_onset("cpu")


@pytest.mark.gpu
def test_spread_onset_gpu(gpu):
    _spread_onset(gpu)
    assert _lib.device_status() == 0


# ---- 7. MBR ----------------------------------------------------------------------------------------------------------------------

def _path_gain(crf, paths, tau, tol):
    """per chain the sum over the path's intervals of (M - tau), in float64 from interval_marginals' values, and the interval count"""
    M = crf.interval_marginals(paths, tolerance=tol)
    return [sum(float(x) - float(tau[c]) for x in M[c]) for c in range(len(paths))], [len(p) for p in paths]


def _mbr(T, B, kind, seed, device):
    s, n = synth.crf_inputs(T, B, seed, device, kind)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    vit = crf.decode()
    for tol in TOLS:
        for thr in THRS + (_per_chain_tau(B),):
            tau = thr.numpy() if isinstance(thr, torch.Tensor) else np.full(B, thr, np.float32)
            lat_p, lat_o, lat_w = crf.decode_marginal_packed(thr, tolerance=tol)
            pairs, offsets, probs, gain = crf.decode_mbr_packed(thr, tolerance=tol)
            wp, wo, ww, wg = _mbr_reference(lat_p, lat_o, lat_w, T, tau)
            assert np.array_equal(offsets, wo) and np.array_equal(pairs, wp), (tol, thr)
            assert np.array_equal(_bits(probs), _bits(ww)) and np.array_equal(_bits(gain), _bits(wg)), (tol, thr)
            # a path: pairwise compatible, and the path calls take it
            paths, pl, g2 = crf.decode_mbr(thr, tolerance=tol)
            assert np.array_equal(_bits(g2), _bits(gain)) and [x for lst in pl for x in lst] == probs.tolist()
            for c in range(B):
                for (b1, e1), (b2, e2) in zip(paths[c], paths[c][1:]):
                    assert b1 <= e1 and e1 <= b2, (c, (b1, e1), (b2, e2))
            ev, lp = crf.evalPath(paths), crf.logProb(paths)
            assert bool(torch.isfinite(ev).all()) and bool(torch.isfinite(lp).all())
            # probs are the M of its intervals
            assert np.array_equal(_bits(crf.interval_marginals_packed(pairs, offsets, tolerance=tol).cpu().numpy()), _bits(probs))
            # no path of the other decoders has a larger sum of (M - tau): 1e-4 per interval for the other summation order
            for other in (vit, crf.decode_mbr(thr)[0]):
                og, cnt = _path_gain(crf, other, tau, tol)
                for c in range(B):
                    assert float(gain[c]) >= og[c] - 1e-4 * (cnt[c] + len(paths[c])), (tol, thr, c, float(gain[c]), og[c])


@pytest.mark.parametrize("T,B,kind,seed", [(70, 20, "model", 22), (130, 37, "model", 5), (48, 1, "ties", 20)])
def test_mbr_cpu(T, B, kind, seed):
    _mbr(T, B, kind, seed, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind,seed", [(70, 20, "model", 22), (130, 37, "model", 5), (48, 1, "ties", 20)])
def test_mbr_gpu(gpu, T, B, kind, seed):
    _mbr(T, B, kind, seed, gpu)
    assert _lib.device_status() == 0


# ---- 8. boundary behaviour -------------------------------------------------------------------------------------------------------

def test_abi_argument_checks():
    """argument checks that return before anything touches a device (the buffers are never dereferenced)"""
    lib = _lib.load()
    for T, B in ((64, 8), (1024, 352), (691, 360), (3, 1)):
        need = lib.semicrf_workspace_bytes(_lib.OP_MARGINAL_DECODE_TOL, T, B)
        assert 0 < need <= 2 * lib.semicrf_workspace_bytes(_lib.OP_MARGINAL_DECODE, T, B)
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    T, B = 4, 2
    good = dict(score=p, noise=p, v=p, q=p, logZ=p, T=T, B=B, tau=p, tau_stride=0, tb=2, te=2, pairs=p, probs=p, cap=8, offsets=p,
                ws=p, ws_bytes=1 << 20, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.semicrf_marginal_decode_tol(a["score"], a["noise"], a["v"], a["q"], a["logZ"], a["T"], a["B"], a["tau"],
                                               a["tau_stride"], a["tb"], a["te"], a["pairs"], a["probs"], a["cap"], a["offsets"],
                                               a["ws"], a["ws_bytes"], a["stream"])

    EINVAL, EWORKSPACE = 1, 2
    for name in ("score", "noise", "v", "q", "logZ", "tau", "pairs", "probs", "offsets", "ws"):
        assert call(**{name: None}) == EINVAL, name
        assert call(**{name: None, "tb": 0, "te": 0}) == EINVAL, name
    assert call(T=0) == EINVAL and call(B=0) == EINVAL
    assert call(tau_stride=2) == EINVAL and call(tau_stride=-1) == EINVAL
    assert call(cap=-1) == EINVAL
    for bad in (-1, 9):
        assert call(tb=bad) == EINVAL and call(te=bad) == EINVAL and call(tb=bad, te=0) == EINVAL and call(tb=0, te=bad) == EINVAL
        assert b"tolerance" in lib.semicrf_last_error()
    need = lib.semicrf_workspace_bytes(_lib.OP_MARGINAL_DECODE_TOL, T, B)
    assert call(ws_bytes=need - 1) == EWORKSPACE
    assert b"workspace" in lib.semicrf_last_error()
    assert call(ws_bytes=need - 1, tb=8, te=0) == EWORKSPACE

    def gather(**kw):
        a = dict(dict(good, K=1, out=p), **kw)
        return lib.semicrf_interval_marginals_tol(a["score"], a["v"], a["q"], a["logZ"], a["T"], a["B"], a["pairs"], a["K"],
                                                  a["offsets"], a["tb"], a["te"], a["out"], a["stream"])

    for name in ("score", "v", "q", "logZ", "offsets", "pairs", "out"):
        assert gather(**{name: None}) == EINVAL, name
    assert gather(T=0) == EINVAL and gather(B=0) == EINVAL and gather(K=-1) == EINVAL
    for bad in (-1, 9):
        assert gather(tb=bad) == EINVAL and gather(te=bad) == EINVAL


@pytest.mark.gpu
def test_capacity_gpu(gpu):
    T, B = 96, 37
    tol = (2, 2)
    s, n = synth.crf_inputs(T, B, 5, gpu, "model")
    lz, v, q = crf_mod._marginal_inputs(s, n)
    tau = torch.full((1,), 0.3, device=gpu)
    pairs, offsets, probs = crf_mod._marginal_decode_raw(s, n, tau, T * (T + 1) // 2 * B, (lz, v, q), tol)
    off = offsets.cpu().numpy()
    total = int(off[-1])
    assert total > 2
    lib = _lib.load()
    need = lib.semicrf_workspace_bytes(_lib.OP_MARGINAL_DECODE_TOL, T, B)
    ws = torch.empty(need, dtype=torch.uint8, device=gpu)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    GUARD = 0x5A5A5A5A                      # the words behind the buffers must stay as they are
    for cap in (0, total - 1):
        pb = torch.full((cap + 8, 2), GUARD, dtype=torch.int32, device=gpu)
        fb = torch.full((cap + 8,), GUARD, dtype=torch.int32, device=gpu)
        ob = torch.full((B + 1 + 8,), GUARD, dtype=torch.int32, device=gpu)
        rc = lib.semicrf_marginal_decode_tol(vp(s), vp(n), vp(v), vp(q), vp(lz), T, B, vp(tau), 0, tol[0], tol[1], vp(pb), vp(fb), cap,
                                             vp(ob), vp(ws), need, st)
        assert rc == 0, lib.semicrf_last_error()
        torch.cuda.synchronize(gpu)
        assert np.array_equal(ob[:B + 1].cpu().numpy(), off)                      # exact although it does not fit
        assert bool((ob[B + 1:] == GUARD).all())
        assert torch.equal(pb[:cap], pairs[:cap]) and bool((pb[cap:] == GUARD).all())
        assert torch.equal(fb[:cap].view(torch.float32), probs[:cap]) and bool((fb[cap:] == GUARD).all())
    rc = lib.semicrf_marginal_decode_tol(vp(s), vp(n), vp(v), vp(q), vp(lz), T, B, vp(tau), 0, tol[0], tol[1], vp(pb), vp(fb), cap, vp(ob),
                                         vp(ws), need - 1, st)
    assert rc == 2
    # an index outside [0, T) gives NaN, begin > end gives 0
    pr = torch.tensor([[3, 9], [9, 3], [-1, 4], [4, T]], dtype=torch.int32, device=gpu)
    oo = torch.tensor([0, 4] + [4] * (B - 1), dtype=torch.int32, device=gpu)
    out = torch.empty(4, dtype=torch.float32, device=gpu)
    rc = lib.semicrf_interval_marginals_tol(vp(s), vp(v), vp(q), vp(lz), T, B, vp(pr), 4, vp(oo), tol[0], tol[1], vp(out), st)
    assert rc == 0, lib.semicrf_last_error()
    o = out.cpu().numpy()
    assert 0 <= o[0] <= 1 and o[1] == 0 and np.isnan(o[2]) and np.isnan(o[3])
    # the Python calls retry with the exact size instead of truncating: (8, 8) at a small threshold passes 2 T per chain
    wide = CRF.decode_marginal_packed(s, n, 0.01, tolerance=(8, 8))
    assert int(wide[1][-1]) == len(wide[0]) == len(wide[2]) > 2 * T * B
    got = CRF.decode_mbr_packed(s, n, 0.01, tolerance=(8, 8))
    want = _mbr_reference(wide[0], wide[1], wide[2], T, np.full(B, 0.01, np.float32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
    assert _lib.device_status() == 0


def test_retry_with_exact_size_cpu():
    T, B = 40, 3
    s, n = synth.crf_inputs(T, B, 5, "cpu", "model")
    wide = CRF.decode_marginal_packed(s, n, 0.01, tolerance=(8, 8))
    assert int(wide[1][-1]) == len(wide[0]) == len(wide[2]) > 2 * T * B
    got = CRF.decode_mbr_packed(s, n, 0.01, tolerance=(8, 8))
    want = _mbr_reference(wide[0], wide[1], wide[2], T, np.full(B, 0.01, np.float32))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))


def _poisoned_alpha(device):
    """NaN in alpha's last row (a sweep that gave up): the total comes back as -1, the other offsets stay exact"""
    T, B = 20, 5
    s, n = synth.crf_inputs(T, B, 43, device, "randn")
    lz, v, q = crf_mod._marginal_inputs(s, n)
    tau = torch.full((1,), 0.4, device=s.device)
    good = crf_mod._marginal_decode_raw(s, n, tau, None, (lz, v, q), (2, 2))[1].cpu()
    v2 = v.clone()
    v2[T - 1, 3] = float("nan")
    bad = crf_mod._marginal_decode_raw(s, n, tau, None, (lz, v2, q), (2, 2))[1].cpu()
    assert int(good[-1]) > 0 and int(bad[-1]) == -1
    assert torch.equal(bad[:4], good[:4])


def test_poisoned_alpha_cpu():
    _poisoned_alpha("cpu")
    s, n = synth.crf_inputs(8, 2, 44, "cpu", "randn")
    s[3, 1, 0] = float("nan")
    for call in (CRF.decode_marginal_packed, CRF.decode_mbr_packed):
        with pytest.raises(RuntimeError):
            call(s, n, 0.5, tolerance=1)


@pytest.mark.gpu
def test_poisoned_alpha_gpu(gpu):
    _poisoned_alpha(gpu)
    assert _lib.device_status() == 0


def _arguments(device):
    T, B = 12, 3
    s, n = synth.crf_inputs(T, B, 41, device, "randn")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    dec = crf.decode()
    p, o = crf.decode_packed()
    calls = [lambda t: crf.interval_marginals(dec, tolerance=t), lambda t: crf.interval_marginals_packed(p, o, tolerance=t),
             lambda t: crf.decode_marginal(0.4, tolerance=t), lambda t: crf.decode_marginal_packed(0.4, tolerance=t),
             lambda t: crf.decode_mbr(0.4, tolerance=t), lambda t: crf.decode_mbr_packed(0.4, tolerance=t),
             lambda t: CRF.interval_marginals(s, n, dec, tolerance=t), lambda t: CRF.interval_marginals_packed(s, n, p, o, tolerance=t),
             lambda t: CRF.decode_marginal(s, n, 0.4, tolerance=t), lambda t: CRF.decode_marginal_packed(s, n, 0.4, tolerance=t),
             lambda t: CRF.decode_mbr(s, n, 0.4, tolerance=t), lambda t: CRF.decode_mbr_packed(s, n, 0.4, tolerance=t)]
    for bad in (True, False, 1.0, 2.5, -1, 9, (1,), (1, 2, 3), (1.0, 2), (1, True), (-1, 0), (0, 9), "1", [1, None], torch.tensor(1)):
        for f in calls:
            with pytest.raises(ValueError):
                f(bad)
    # an int is (t, t); a list is taken like a tuple; numpy ints are ints
    for a, b in ((2, (2, 2)), ([1, 3], (1, 3)), ((np.int32(1), np.int64(3)), (1, 3)), (8, (8, 8))):
        for f in calls:
            assert _same(f(a), f(b))
    # the threshold's errors stay as they are
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError):
            crf.decode_marginal_packed(bad, tolerance=1)
        with pytest.raises(ValueError):
            crf.decode_mbr_packed(bad, tolerance=1)
    # the list form, the packed form and the gather agree
    want = crf.decode_marginal_packed(0.4, tolerance=(1, 2))
    paths, probs = crf.decode_marginal(0.4, tolerance=(1, 2))
    off = want[1]
    assert paths == [[tuple(int(x) for x in q) for q in want[0][off[c]:off[c + 1]]] for c in range(B)]
    assert [x for lst in probs for x in lst] == want[2].tolist()
    assert crf.interval_marginals(paths, tolerance=(1, 2)) == probs
    # no gradient flows, whatever the inputs require; other float dtypes are computed as .float()
    sg, ng = s.clone().requires_grad_(), n.clone().requires_grad_()
    assert _same(CRF.decode_marginal_packed(sg, ng, 0.4, tolerance=(1, 2)), want)
    assert not CRF.interval_marginals_packed(sg, ng, p, o, tolerance=1).requires_grad
    sd, nd = s.to(torch.bfloat16), n.to(torch.bfloat16)
    assert _same(CRF.decode_mbr_packed(sd, nd, 0.4, tolerance=2), CRF.decode_mbr_packed(sd.float(), nd.float(), 0.4, tolerance=2))
    # T = 1: the only cell is the singleton and its box holds nothing else
    s1, n1 = s[:1, :1].contiguous(), n[:0]
    p1, o1, m1 = CRF.decode_marginal_packed(s1, n1, 1e-6, tolerance=8)
    assert np.array_equal(o1, np.arange(B + 1)) and np.array_equal(p1, np.zeros((B, 2), np.int32))
    assert _same(m1, CRF.decode_marginal_packed(s1, n1, 1e-6)[2])


def test_arguments_cpu():
    _arguments("cpu")


@pytest.mark.gpu
def test_arguments_gpu(gpu):
    _arguments(gpu)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    T, B = 333, 46
    tol = (2, 2)
    data = [synth.crf_inputs(T, B, 600 + i, gpu) for i in range(3)]
    tau = _per_chain_tau(B).to(gpu)
    cap = 8 * T * B

    def chain(s, n):
        lvq = crf_mod._marginal_inputs(s, n)
        lat = crf_mod._marginal_decode_raw(s, n, tau, cap, lvq, tol)
        return list(lat) + list(crf_mod._mbr_select_raw(lat[0], lat[2], lat[1], T, tau))

    def trimmed(out):
        pairs, offsets, probs, mp, mo, mw, gain = out
        k, km = int(offsets[-1]), int(mo[-1])
        assert 0 < k <= cap and km > 0
        return [pairs[:k].clone(), offsets.clone(), probs[:k].clone(), mp[:km].clone(), mo.clone(), mw[:km].clone(), gain.clone()]

    want = [trimmed(chain(s, n)) for s, n in data]
    s_in, n_in = data[0][0].clone(), data[0][1].clone()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(2):
            chain(s_in, n_in)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = chain(s_in, n_in)
    for i in (1, 2, 0, 1):
        s_in.copy_(data[i][0]); n_in.copy_(data[i][1])
        graph.replay()
        torch.cuda.synchronize(gpu)
        for a, b in zip(trimmed(got), want[i]):
            assert torch.equal(a, b), i
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_single_chain_gpu(gpu):
    """one chain runs with a ghost chain appended (as decode does): the ghost's cells must not show (T200_B1 of CASES is the exact
    form; this is the MBR path on top of it)"""
    s, n = synth.crf_inputs(200, 1, 9, gpu, "model")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    for thr in (0.3, torch.tensor([0.6])):
        lat = crf.decode_marginal_packed(thr, tolerance=(2, 1))
        got = crf.decode_mbr_packed(thr, tolerance=(2, 1))
        tau = np.full(1, float(thr), np.float32)
        want = _mbr_reference(lat[0], lat[1], lat[2], 200, tau)
        assert len(lat[0]) > 0 and lat[1].shape == (2,)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(_bits(got[2]), _bits(want[2]))
    assert _lib.device_status() == 0


# ---- 9. full size (GPU) ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(1024, 352), (691, 360)])
def test_full_size_gpu(gpu, T, B):
    tau, tol = 0.5, (2, 2)
    s, n = synth.crf_inputs(T, B, 11, gpu, "model")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    r1 = crf.decode_marginal_packed(tau, tolerance=tol)       # (leased sweep workspaces are set up here)
    torch.cuda.synchronize(gpu)
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    r2 = crf.decode_marginal_packed(tau, tolerance=tol)
    torch.cuda.synchronize(gpu)
    peak = torch.cuda.max_memory_allocated(gpu) - base
    for a, b in zip(r1, r2):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))                # deterministic: bit-identical
    pairs, offsets, probs = r1
    print(f"{T}x{B}: {len(probs)} selected at tolerance {tol}, peak {peak / 2 ** 20:.1f} MiB")
    assert len(probs) > 0 and (probs >= np.float32(tau)).all()
    im = crf.interval_marginals_packed(pairs, offsets, tolerance=tol).cpu().numpy()
    assert np.array_equal(im.view(np.int32), probs.view(np.int32))
    c = np.repeat(np.arange(B), np.diff(offsets)).astype(np.int64)
    key = (c * T + pairs[:, 0]) * T + pairs[:, 1]
    assert np.all(np.diff(key) > 0)                                              # ascending by (begin, end) within every chain
    assert peak <= 128 * 2 ** 20, peak / 2 ** 20                                 # no [T, T, B] tensor anywhere
    assert _lib.device_status() == 0
