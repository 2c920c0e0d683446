"""logProb's backward with the path's own terms applied inside the gradient sweep (semicrf_logprob_fwd_t / _bwd_t).

The yardstick is the two-launch route (gradient sweep, then the scatter kernel): for every case the folded route and the forced
two-launch route run on the same inputs in the same process and dScore / dNoise must agree bit for bit, the upper triangle's
+0.0 included; logProb must equal the stand-alone evalPath - logZ.  The intervals are hand-built per chain, in POSITIONS of the
gradient sweep (position p = T - 1 - frame; a row of the sweep is an interval's begin, a column its end; blocks of 16), so
that every writer of the sweep meets a path cell: the ring (diagonal cell, gaps), the band waves (column block up to 3 blocks
from the row's) and the panels (4 blocks and more)."""
import importlib

import numpy as np
import pytest
import torch

PB, FAR0 = 16, 4                        # positions per block; the first block distance that belongs to the far field
NONE, COVERED = (1 << 30) - 1, 1 << 30  # SEMICRF_PTAB_NONE, SEMICRF_PTAB_COVERED


def _nsci():
    return importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")


def iv(T, pi, pj):
    """The interval whose cell the gradient sweep stores in row position pi, column position pj (pj <= pi)."""
    assert 0 <= pj <= pi < T
    return (T - 1 - pi, T - 1 - pj)


def dense_chain(T, phase):
    """Many short intervals: lengths 0..5 and gaps 0..2 in a fixed cycle, begins strictly ascending."""
    out, b, i = [], phase % 5, phase
    while b < T:
        e = min(b + (i * 7 + 3) % 6, T - 1)
        out.append((b, e))
        b = max(e + (i * 5 + 1) % 3, b + 1)
        i += 1
    return out


def hand_paths(T, B):
    """One list per chain; the pattern repeats every 16 chains, so that every case lands in full and in ragged chain quads."""
    if T < 5 * PB:                                       # no far field (the fallback shapes): the ring's cases only
        cases = [[], [(0, 0), (T // 2, T // 2), (T - 1, T - 1)], [(2, 9), (9, 20)], dense_chain(T, 3), [(0, T - 1)]]
        return [list(cases[c % len(cases)]) for c in range(B)]
    K = (T + PB - 1) // PB
    kl = K - 1                                           # the last row block (it may be ragged)
    far_pi = PB * min(kl, FAR0 + 1)                      # a row whose block has a far field
    cases = [
        [],                                                                       # an empty chain
        [(0, 0), (T // 2, T // 2), (T - 1, T - 1)],                               # singletons: first frame, middle, last frame
        [(2, 9), (9, 20), (20, 20 + 13)],                                         # touching pairs (a, e), (e, e2)
        [iv(T, 3 * PB + 2, 3)],                                                   # begin 3 blocks before the end's block: band
        [iv(T, 4 * PB + 1, 3)],                                                   # ... 4 blocks: the newest far tile
        [iv(T, 3 * PB, PB - 1)],                                                  # 3 blocks apart, nearest corners
        [iv(T, 4 * PB + PB - 1, 0)],                                              # 4 blocks apart, farthest corners
        [(16, 31), (32, 47)],                                                     # both ends of a 16-frame block
        [iv(T, 3 * PB + 5, 2 * PB), iv(T, 2 * PB - 1, PB)],                       # ... and of a 16-position block
        [(0, T - 1)],                                                             # the longest interval
        [(5, T - 1)],                                                             # ends at T-1, begins in the first 16 frames
        [iv(T, far_pi, 2)],                                                       # two far cells of ONE panel task: rows far_pi and
        [iv(T, far_pi + 1, 9)],                                                   # far_pi + 1 (same row quarter), neighbouring chains
        [iv(T, far_pi + 2, 9), (T - 1, T - 1)],                                   # ... a third row, plus the last frame's singleton
        dense_chain(T, 3),
        [(0, 3), (3, 3 + 2 * PB), (T - 2, T - 1)],                                # first gap covered, last gap covered
    ]
    if T >= 20 * PB:
        # a row block whose far field has two column parts (tiles 0..11 and 12..15 of block 19): one cell in each, one row
        cases[5] = [iv(T, 19 * PB + 3, 5 * PB + 6)]
        cases[6] = [iv(T, 19 * PB + 3 - 1, 13 * PB + 1), iv(T, 13 * PB, 13 * PB)]
    return [list(cases[c % len(cases)]) for c in range(B)]


def table_ref(intervals, T):
    """The path table as include/semicrf_hip.h defines it, from the interval lists."""
    B = len(intervals)
    ends = np.full((T, B), NONE, np.int32)
    cov = np.zeros((T, B), np.int32)
    for c, lst in enumerate(intervals):
        for b, e in lst:
            assert ends[b, c] == NONE and not cov[b:e, c].any(), "not a representable path"
            ends[b, c] = e
            cov[b:e, c] = COVERED
    return ends | cov


def weights(B, device, kind):
    """The cotangent of logProb: per chain with zeros and negative values (stride 1), or one expanded scalar (stride 0)."""
    if kind == "scalar":
        return None
    w = torch.tensor([((c * 37) % 11 - 4) / 8.0 for c in range(B)], dtype=torch.float32, device=device)
    assert (w == 0).any() and (w < 0).any()
    return w


def run_logprob(score, noise, intervals, w, fold):
    """One logProb forward + backward through the public API; returns (logProb, dScore, dNoise, route counts taken)."""
    from transkun_amd import CRF
    nsci = _nsci()
    B = score.shape[2]
    before = dict(nsci.PATH_ROUTES)
    was = nsci.PATH_FOLD
    nsci.PATH_FOLD = fold
    try:
        s = score.clone().requires_grad_()
        n = noise.clone().requires_grad_()
        lp = CRF.NeuralSemiCRFInterval(s, n).logProb(intervals)
        loss = -lp.sum() / B if w is None else (lp * w).sum()
        loss.backward()
    finally:
        nsci.PATH_FOLD = was
    took = {k: nsci.PATH_ROUTES[k] - before[k] for k in before}
    return lp.detach(), s.grad, n.grad, took


def assert_same_bits(a, b, what):
    assert a.shape == b.shape, what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} values differ, max |diff| {float((a - b).abs().max())}"
    assert torch.equal(torch.signbit(a), torch.signbit(b)), f"{what}: a zero changed its sign"


def assert_upper_is_plus_zero(g, what):
    T = g.shape[0]
    upper = torch.triu(torch.ones(T, T, dtype=torch.bool, device=g.device), diagonal=1)
    assert float(g[upper].abs().max()) == 0.0 and not torch.signbit(g[upper]).any(), f"{what}: upper triangle not +0.0"


# ---- host side (no GPU) --------------------------------------------------------------------------------------------------------

def test_pack_intervals_knows_which_paths_fit_the_table():
    nsci = _nsci()
    T = 64

    def simple(lists, **kw):
        pairs, _ = nsci.pack_intervals(lists, T, len(lists), "cpu", **kw)
        return pairs._semicrf_simple

    assert simple([[], [(0, 0)], [(0, 3), (3, 3 + 4), (9, 9), (10, 63)]])
    assert simple([[(2, 9), (9, 9)]])                       # two intervals END at frame 9, one begins there: fits
    assert not simple([[(9, 9), (9, 12)]])                  # two intervals BEGIN at frame 9
    assert not simple([[(2, 10), (5, 12)]])                 # overlapping
    assert not simple([[(5, 8), (1, 3)]])                   # not ascending
    assert not simple([[(1, 3)], [(4, 9), (4, 9)]])         # a duplicate
    assert not simple([[(1, 3), (5, 8)]], ordered=False)    # packed without the begin <= end check: never
    for T2, B2 in ((80, 36), (96, 64), (200, 36), (320, 36)):
        lists = hand_paths(T2, B2)
        p2, _ = nsci.pack_intervals(lists, T2, B2, "cpu")
        assert p2._semicrf_simple, (T2, B2)
        table_ref(lists, T2)                                # asserts that every chain is representable


def test_table_reference_on_a_chain_worked_by_hand():
    #            frame:   0        1               2     3        4               5
    # (1, 3), (3, 3), (4, 5): none, begins (end 3), none, begins (end 3), begins (end 5), none;  gaps 1, 2, 4 covered
    want = [NONE, 3 | COVERED, NONE | COVERED, 3, 5 | COVERED, NONE]
    assert table_ref([[(1, 3), (3, 3), (4, 5)]], 6)[:, 0].tolist() == want


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

_INPUTS = {}


def inputs(T, B, gpu):
    from transkun_amd import synth
    key = (T, B)
    if key not in _INPUTS:
        score, noise = synth.crf_inputs(T, B, 900 + T + B, gpu)
        _INPUTS[key] = (score, noise, hand_paths(T, B))
    return _INPUTS[key]


# T = 80, 96: five / six row blocks -- one far tile, band waves.  T = 200: thirteen.  T = 320: the last block's far field has two
# column parts.  B = 36: a ragged 32-chain group and chain quads past the end; 64: two full groups.
SHAPES = [(80, 36), (80, 64), (96, 36), (96, 64), (200, 36), (200, 64), (320, 36)]


@pytest.mark.gpu
@pytest.mark.parametrize("gkind", ["per_chain", "scalar"])
@pytest.mark.parametrize("T,B", SHAPES)
def test_folded_route_matches_two_launch_route_bit_for_bit(gpu, T, B, gkind):
    from transkun_amd import CRF, _lib
    _lib.set_impl(0)
    score, noise, paths = inputs(T, B, gpu)
    w = weights(B, gpu, gkind)
    lp0, ds0, dn0, took0 = run_logprob(score, noise, paths, w, fold=False)
    lp1, ds1, dn1, took1 = run_logprob(score, noise, paths, w, fold=True)
    assert took0 == {"folded": 0, "scatter": 1} and took1 == {"folded": 1, "scatter": 0}, (took0, took1)
    assert_same_bits(ds1, ds0, "dScore")
    assert_same_bits(dn1, dn0, "dNoise")
    assert_upper_is_plus_zero(ds1, "folded route")
    assert_same_bits(lp1, lp0, "logProb")
    with torch.no_grad():
        crf = CRF.NeuralSemiCRFInterval(score, noise)
        assert_same_bits(lp1, crf.evalPath(paths) - crf.computeLogZ(), "logProb vs evalPath - logZ")
    # the path's terms are really there (the yardstick is not an empty gradient): every path cell differs from the marginal alone
    if gkind == "scalar":
        c, (b, e) = next((c, lst[0]) for c, lst in enumerate(paths) if lst)
        assert float(ds1[e, b, c]) < 0.0 and float(ds1[e, b, c]) >= -1.0 / B - 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(80, 36), (200, 64)])
def test_device_table_equals_numpy_reference(gpu, T, B):
    from transkun_amd import _lib
    nsci = _nsci()
    _lib.set_impl(0)
    score, noise, paths = inputs(T, B, gpu)
    pairs, offsets = nsci.pack_intervals(paths, T, B, gpu)
    assert nsci._path_table_ok(score, pairs)
    ptab = torch.full((T, B), -7, dtype=torch.int32, device=gpu)        # every word must be written: no fill is promised
    nsci._logprob_fwd_raw(score, noise, pairs, offsets, True, ptab)
    got = ptab.cpu().numpy()
    want = table_ref(paths, T)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


@pytest.mark.gpu
@pytest.mark.parametrize("T,B", [(96, 36), (320, 36)])
def test_the_table_alone_carries_the_path(gpu, T, B):
    """The route, asserted in the library itself: the backward call gets the forward's table but an EMPTY interval list.  A launch
    that applied the table gives the full gradient of the two-launch route; one that ignored it (and scattered nothing) would
    lack every path term."""
    from transkun_amd import _lib
    nsci = _nsci()
    _lib.set_impl(0)
    score, noise, paths = inputs(T, B, gpu)
    w = weights(B, gpu, "per_chain")
    _, ds0, dn0, _ = run_logprob(score, noise, paths, w, fold=False)
    pairs, offsets = nsci.pack_intervals(paths, T, B, gpu)
    ptab = torch.empty((T, B), dtype=torch.int32, device=gpu)
    _, logz, v = nsci._logprob_fwd_raw(score, noise, pairs, offsets, True, ptab)
    no_pairs, no_offsets = nsci.pack_intervals([[] for _ in range(B)], T, B, gpu)
    ds = torch.empty(T, T, B, dtype=torch.float32, device=gpu)
    dn = torch.empty_like(noise)
    ws = _lib.leased_workspace(_lib.OP_LOGZ_BWD, T, B, gpu)
    _lib.ops().logprob_bwd(score, noise, v, logz, w, 1, no_pairs, 0, no_offsets, ds, dn, 0, ws, ptab, True)
    assert_same_bits(ds, ds0, "dScore")
    assert_same_bits(dn, dn0, "dNoise")
    _lib.ops().logprob_bwd(score, noise, v, logz, w, 1, no_pairs, 0, no_offsets, ds, dn, 0, ws, no_offsets, False)
    assert not torch.equal(ds, ds0) and not torch.equal(dn, dn0)          # without the table the path terms are missing


@pytest.mark.gpu
def test_six_steps_on_a_leased_workspace_with_the_pooled_gradient(gpu):
    """tests/test_gpu_parity.py::test_grad_pool_upper_triangle_stays_exact, folded: the pooled buffer's upper triangle stays +0.0
    (the fix-ups touch lower-triangle cells only), every step equals the first bit for bit, and the first equals the two-launch route."""
    from transkun_amd import CRF, _lib, synth
    nsci = _nsci()
    _lib.set_impl(0)
    T, B = 256, 96                                      # 25 MB: above the pool's threshold
    score, noise = synth.crf_inputs(T, B, 321, gpu)
    paths = hand_paths(T, B)
    _, want_ds, want_dn, _ = run_logprob(score, noise, paths, None, fold=False)
    want_ds, want_dn = want_ds.clone(), want_dn.clone()
    nsci.grad_pool_clear()
    pool = nsci._GRAD_POOL
    h0 = pool.hits
    before = dict(nsci.PATH_ROUTES)
    for step in range(6):
        s = score.clone().requires_grad_()
        n = noise.clone().requires_grad_()
        lp = CRF.NeuralSemiCRFInterval(s, n).logProb(paths)
        (-lp.sum() / B).backward()
        assert_upper_is_plus_zero(s.grad, f"step {step}")
        assert_same_bits(s.grad, want_ds, f"step {step}: dScore")
        assert_same_bits(n.grad, want_dn, f"step {step}: dNoise")
        del s, n, lp
    assert nsci.PATH_ROUTES["folded"] - before["folded"] == 6 and nsci.PATH_ROUTES["scatter"] == before["scatter"]
    assert pool.hits - h0 >= 2                          # the zeros were skipped: the steps ran on pooled buffers


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["odd_B", "T48", "impl1", "overlapping"])
def test_fallbacks_keep_the_scatter_launch_and_its_bits(gpu, case):
    from transkun_amd import _lib
    _lib.set_impl(0)
    T, B = (80, 37) if case == "odd_B" else ((48, 36) if case == "T48" else (80, 36))
    score, noise, paths = inputs(T, B, gpu)
    if case == "overlapping":
        paths = [list(p) for p in paths]
        paths[1] = [(2, 10), (5, 12)]
    w = weights(B, gpu, "per_chain")
    try:
        if case == "impl1":
            _lib.set_impl(1)
        lp0, ds0, dn0, took0 = run_logprob(score, noise, paths, w, fold=False)
        lp1, ds1, dn1, took1 = run_logprob(score, noise, paths, w, fold=True)
    finally:
        _lib.set_impl(0)
    assert took0 == {"folded": 0, "scatter": 1} and took1 == {"folded": 0, "scatter": 1}, (took0, took1)
    assert_same_bits(ds1, ds0, "dScore")
    assert_same_bits(dn1, dn0, "dNoise")
    assert_same_bits(lp1, lp0, "logProb")
    assert_upper_is_plus_zero(ds1, case)


@pytest.mark.gpu
def test_two_node_pattern_still_scatters(gpu):
    """crf.evalPath(...) - crf.computeLogZ() (the reference's own call pattern) goes through the hub and the scatter kernel: no
    _LogProb node, no table.  Same mathematics as the one-node route; the two sum the noise gradient's terms in the same order,
    but nothing promises the last bit, so the bound is two roundings of values of size <= max |gout| = 1: 2 * 2^-23."""
    from transkun_amd import CRF, _lib
    nsci = _nsci()
    _lib.set_impl(0)
    T, B = 80, 36
    score, noise, paths = inputs(T, B, gpu)
    _, ds0, dn0, _ = run_logprob(score, noise, paths, None, fold=False)
    before = dict(nsci.PATH_ROUTES)
    s = score.clone().requires_grad_()
    n = noise.clone().requires_grad_()
    crf = CRF.NeuralSemiCRFInterval(s, n)
    lp = crf.evalPath(paths) - crf.computeLogZ()
    (-lp.sum() / B).backward()
    assert nsci.PATH_ROUTES == before
    tol = 2.0 * 2.0 ** -23
    assert float((s.grad - ds0).abs().max()) <= tol and float((n.grad - dn0).abs().max()) <= tol
    assert_upper_is_plus_zero(s.grad, "two-node")
