"""The sweeps' outputs per element against float64, in the log domain (tests/sweep_accuracy_common.py has the yardstick, the bounds
with their derivation, the floor and the mutants).

Every maximum-norm comparison of the suite (rel_err against max(1e-4, 2e-6 |logZ|), atol 1e-5) sees only the few cells of the dense
gradient that are large: a gradient whose cells below 5e-5 are all zero passes it.  Here every alpha, beta, logZ, every marginal of
end >= begin, every path cell and every dNoise entry has a bound of its own, derived from the kernels' operations.

Ops: logz_fwd (logZ, v), beta, logz_bwd (dScore, dNoise, q_out; cotangent 1 and a per-chain one of mixed sign), logprob_fwd /
logprob_bwd with a cotangent per chain and with gstride 0 -- through the scatter and, where the launch takes it, through the forward
call's path table (logprob_fwd_t / logprob_bwd_t) -- and interval_marginals on a list of band cells, far cells and diagonal cells.
The C ABI fixes gscale: 1 in logz_bwd, -1 in logprob_bwd, which is the gscale != 1 of these cases.

Shapes: the smallest that reach each branch of plan_chunk / band_in_sweep (persist.hip), see SHAPES.  Each numerical case runs on the
host mirror (unmarked) and on the device (gpu); the two 0.5 GB shapes on the device only.  The five-panel-wave plan (T >= 1024 with
256 chains or more) needs 1 GB tensors: it stays with the golden large_* cases of tests/test_gpu_parity.py and is out of scope here.

The module's last test reads the device status word.
"""
import numpy as np
import pytest
import torch

import sweep_accuracy_common as sa
from transkun_amd import _lib

CPU = torch.device("cpu")
F32, I32 = torch.float32, torch.int32
GPU_ONLY = pytest.mark.gpu

# T, B: what the shape reaches (PB = 16, FAR0 = 4, GS = 4, GP = 32, TPT = 12, LEADT = 4)
SHAPES = {
    (17, 2): "ring only (K = 2): no panel tasks, zero_upper_kernel, the spines' spare wave takes the path",
    (33, 7): "ring only (K = 3), odd NBatch",
    (64, 5): "K = 4: the last length without a far tile",
    (65, 5): "K = 5: the first far tile",
    (70, 20): "the floor's reference length for randn and model; five spines",
    (130, 6): "K = 9: the spines' spare waves stream from hybridStart = 8; the path table is taken",
    (200, 33): "K = 13: past GRAD_HSTART = 12 and BANDX_K0 + FAR0; two panel groups, the second with one chain",
    (304, 4): "K = 19: the last length with one column part per block",
    (305, 4): "K = 20: nparts_of(K - 1 - FAR0) == 2 for the first time",
    (306, 4): "... and one past it",
    (340, 4): "K = 22: two column parts in three blocks",
    (70, 520): "two chain chunks on 256 CUs: no path fold, no band copy",
    (1024, 8): "two far waves, the in-sweep band copy of the forward sweeps, gradLazyShort; 32 MB",
    (1024, 128): "the non-temporal cell stream, forward and gradient; 0.5 GB per tensor",
    (1024, 120): "... and the gradient sweep's ordinary loads (NBatch % 32 != 0)",
    (48, 6): "the golden T48_B6 edge case's shape",
    (33, 1): "one chain: the row-sequential kernels whatever the implementation switch says",
}
# (PB, FAR0, TPT, LEADT are read from persist_common.h / persist_tuning.h: if they move, the lengths that bracket the second part move)
assert [sa.nparts_of((T + sa.PB - 1) // sa.PB - 1 - sa.FAR0) for T in (304, 305, 306)] == [1, 2, 2]


def _case(family, T, B, gpu_only=False):
    assert (T, B) in SHAPES
    return pytest.param((family, T, B), id=f"{family}-T{T}_B{B}", marks=[GPU_ONLY] if gpu_only else [])


SMALL_CASES = [_case("balanced", T, B) for T, B in [(17, 2), (33, 7), (64, 5), (65, 5), (130, 6), (200, 33), (304, 4), (305, 4), (306, 4),
                                                    (340, 4), (70, 520), (1024, 8)]] + \
              [_case("randn", T, B) for T, B in [(17, 2), (33, 7), (65, 5), (70, 20), (130, 6), (200, 33), (340, 4)]] + \
              [_case("model", T, B) for T, B in [(70, 20), (130, 6), (200, 33)]] + \
              [_case("huge", 48, 6)]
BIG_CASES = [_case("balanced", 1024, 128, True), _case("balanced", 1024, 120, True)]
ROWSEQ_CASES = [_case("balanced", 17, 2), _case("balanced", 65, 5), _case("balanced", 130, 6), _case("randn", 130, 6), _case("balanced", 33, 1)]
SEED = {"balanced": 31, "randn": 22, "model": 22, "huge": 21}


def _which_cases(cases, impl):
    """(case, which, impl): every case on both devices, the device-only ones on the device."""
    out = []
    for p in cases:
        gpu_only = any(m.name == "gpu" for m in p.marks)
        for w in ("cpu", "gpu"):
            if w == "cpu" and gpu_only:
                continue
            out.append(pytest.param(p.values[0], w, impl, id=f"{p.id}-{w}" + ("-rowseq" if impl else ""),
                                    marks=[GPU_ONLY] if w == "gpu" else []))
    return out


RUNS = _which_cases(SMALL_CASES + BIG_CASES, 0) + _which_cases(ROWSEQ_CASES, 1)


def _note(cx, what, ratio):
    """The worst error / bound of a comparison, printed (pytest -s): the record of DESIGN.md, not a gate."""
    print(f"ACC {cx.family} T={cx.T} B={cx.B} {cx.which} {cx.K['name']} {what}: {ratio:.4f}")


# ---- the shared, read-only context of a case: inputs, truth, and the forward results the later ops take -------------------------------------
class Ctx:
    pass


_LAST = {}


def truth_of(oracle, family, T, B):
    """(score, noise, Truth) of a case; kept for the module's lifetime except for the 0.5 GB shapes (one at a time)."""
    key = ("truth" if T * T * B <= (1 << 24) else "big truth", family, T, B)
    if key not in _LAST:
        for k in [k for k in _LAST if k[0] == "big truth"]:
            del _LAST[k]
        score, noise = sa.make_inputs(family, T, B, SEED[family])
        tr = sa.Truth(oracle, score, noise, sa.chain_subset(B))
        # the caps on what the floor leaves out and on what the persistent sweep's underflow rule exempts, on the float64 truth alone,
        # before any result is looked at
        assert tr.under_floor <= sa.floor_cap(family, T), (family, T, tr.under_floor)
        assert tr.flush_share() <= sa.flush_cap(family, T), (family, T, tr.flush_share())
        _LAST[key] = (score, noise, tr)
    return _LAST[key]


def context(request, oracle, case, which, impl):
    family, T, B = case
    key = ("ctx", family, T, B, which, impl)
    if key in _LAST:
        return _LAST[key]
    for k in [k for k in _LAST if k[0] == "ctx"]:
        del _LAST[k]
    dev = CPU if which == "cpu" else request.getfixturevalue("gpu")
    cx = Ctx()
    cx.family, cx.T, cx.B, cx.which, cx.impl, cx.dev = family, T, B, which, impl, dev
    cx.score, cx.noise, cx.tr = truth_of(oracle, family, T, B)
    cx.K = sa.impl_of(which, T, B, impl)
    cx.persist = cx.K is sa.PERSIST
    cx.ix = torch.tensor(cx.tr.idx)
    cx.sd, cx.nd = cx.score.to(dev), cx.noise.to(dev)
    cx.paths = sa.target_paths(T, B)
    cx.sub_paths = [cx.paths[c] for c in cx.tr.idx]
    # alpha and logZ as the device made them: what the backward ops take in a real step
    cx.logZ = torch.empty(B, dtype=F32, device=dev)
    cx.v = torch.empty(T, B, dtype=F32, device=dev)
    _with_impl(impl, lambda: _lib.ops().logz_fwd(cx.sd, cx.nd, cx.logZ, cx.v, True, _ws(cx, _lib.OP_LOGZ_FWD)))
    _LAST[key] = cx
    return cx


def _ws(cx, op):
    return _lib.workspace(op, cx.T, cx.B, cx.dev)


def _with_impl(impl, fn):
    if not impl:
        return fn()
    _lib.set_impl(1)
    try:
        return fn()
    finally:
        _lib.set_impl(0)


def _sub(cx, t, axis):
    """The truth's chains of a result, on the host."""
    return t.index_select(axis, cx.ix.to(t.device)).cpu().numpy()


def _whole_tensor(cx, dS):
    """Every chain, not only the truth's: finite, and +0.0f above the diagonal."""
    assert bool(torch.isfinite(dS).all())
    up = dS.permute(2, 0, 1).triu(1).contiguous()
    assert bool((up.view(I32) == 0).all()), "the upper triangle is not +0.0f"


def _packed_paths(cx):
    from transkun_amd.CRF.NeuralSemiCRFInterval import pack_intervals
    pairs, offsets = pack_intervals(cx.paths, cx.T, cx.B, cx.dev)
    assert pairs._semicrf_simple
    return pairs, offsets, pairs._semicrf_K


# ---- the numerical cases ------------------------------------------------------------------------------------------------------------------------
def op_forward_sweeps(request, oracle, case, which, impl):
    """logz_fwd's logZ and v, beta, and logprob_fwd's logProb / logZ / v (with the path table where the persistent sweep runs)."""
    cx = context(request, oracle, case, which, impl)
    tr, K, T, B, dev = cx.tr, cx.K, cx.T, cx.B, cx.dev
    _note(cx, "logZ", sa.check_log("logz_fwd logZ", _sub(cx, cx.logZ, 0), tr.lz, tr.logz_bound(K)))
    _note(cx, "alpha", sa.check_log("logz_fwd v", _sub(cx, cx.v, 1), tr.v, tr.alpha_bound(K)))
    q = torch.empty(T, B, dtype=F32, device=dev)
    _with_impl(impl, lambda: _lib.ops().beta(cx.sd, cx.nd, q, _ws(cx, _lib.OP_LOGZ_FWD)))
    _note(cx, "beta", sa.check_log("beta", _sub(cx, q, 1), tr.q, tr.beta_bound(K)))
    pairs, offsets, Kp = _packed_paths(cx)
    want, pb = sa.want_logprob(cx.score, cx.noise, cx.sub_paths, tr)
    for table in ([False, True] if cx.persist else [False]):
        lp, lz, v = torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev), torch.empty(T, B, dtype=F32, device=dev)
        ptab = torch.full((T, B), -7, dtype=I32, device=dev) if table else offsets
        _with_impl(impl, lambda: _lib.ops().logprob_fwd(cx.sd, cx.nd, pairs, Kp, offsets, lp, lz, v, True, _ws(cx, _lib.OP_LOGZ_FWD), ptab, table))
        tag = "logprob_fwd_t" if table else "logprob_fwd"
        _note(cx, tag + " logProb", sa.check_abs(tag + " logProb", _sub(cx, lp, 0), want, pb + tr.logz_bound(K)))
        sa.check_log(tag + " logZ", _sub(cx, lz, 0), tr.lz, tr.logz_bound(K))
        sa.check_log(tag + " v", _sub(cx, v, 1), tr.v, tr.alpha_bound(K))
        if table:
            assert not bool((ptab == -7).any()), "the forward call leaves words of the path table unwritten"


def op_logz_bwd(request, oracle, case, which, impl):
    """dScore, dNoise and q_out with the cotangent 1 and with a per-chain cotangent of mixed sign (one chain exactly 0)."""
    cx = context(request, oracle, case, which, impl)
    tr, K, T, B, dev = cx.tr, cx.K, cx.T, cx.B, cx.dev
    dS, dN, q = torch.empty(T, T, B, dtype=F32, device=dev), torch.empty(max(T - 1, 0), B, dtype=F32, device=dev), torch.empty(T, B, dtype=F32, device=dev)
    for name, g64 in (("gout=1", np.ones(B)), ("gout mixed", sa.mixed_gout(B))):
        gout = torch.from_numpy(g64).to(F32).to(dev)
        dS.fill_(float("nan")); dN.fill_(float("nan")); q.fill_(float("nan"))
        _with_impl(impl, lambda: _lib.ops().logz_bwd(cx.sd, cx.nd, cx.v, cx.logZ, gout, dS, dN, q, True, 0, _ws(cx, _lib.OP_LOGZ_BWD)))
        _whole_tensor(cx, dS)
        res = sa.check_dense("logz_bwd " + name, _sub(cx, dS, 2), _sub(cx, dN, 1), tr, g64[tr.idx], K, flush=cx.persist)
        for k, r in res.items():
            _note(cx, f"logz_bwd {name} {k}", r)
        _note(cx, f"logz_bwd {name} q_out", sa.check_log("logz_bwd q_out", _sub(cx, q, 1), tr.q, tr.beta_bound(K)))


def op_logprob_bwd(request, oracle, case, which, impl):
    """gout (indicator - marginal) and gout (1 - cover - noise marginal) against the float64 restatement, with a cotangent per chain
    and with gstride 0; once through the scatter and, where the persistent sweep runs, once with the forward call's path table
    (the launch folds the path's terms where its plan allows: semicrf_logprob_path_table_supported)."""
    cx = context(request, oracle, case, which, impl)
    tr, K, T, B, dev = cx.tr, cx.K, cx.T, cx.B, cx.dev
    pairs, offsets, Kp = _packed_paths(cx)
    dS, dN = torch.empty(T, T, B, dtype=F32, device=dev), torch.empty(max(T - 1, 0), B, dtype=F32, device=dev)
    ptab = None
    if cx.persist:
        ptab = torch.empty(T, B, dtype=I32, device=dev)
        lp, lz = torch.empty(B, dtype=F32, device=dev), torch.empty(B, dtype=F32, device=dev)
        _lib.ops().logprob_fwd(cx.sd, cx.nd, pairs, Kp, offsets, lp, lz, cx.v, False, _ws(cx, _lib.OP_LOGZ_FWD), ptab, True)
        folds = _lib.load().semicrf_logprob_path_table_supported(T, B) == 1
        assert folds == (B % 2 == 0 and T > sa.PB * sa.FAR0 and (B + sa.GS - 1) // sa.GS <= 128), "the plan this case was chosen for"
    for gname, g64, gstride in (("g per chain", sa.mixed_gout(B, 1), 1), ("gstride 0", np.full(B, -0.625), 0)):
        gout = torch.from_numpy(g64 if gstride else g64[:1]).to(F32).to(dev)
        for table in ([False, True] if cx.persist else [False]):
            dS.fill_(float("nan")); dN.fill_(float("nan"))
            _with_impl(impl, lambda: _lib.ops().logprob_bwd(cx.sd, cx.nd, cx.v, cx.logZ, gout, gstride, pairs, Kp, offsets, dS, dN, 0,
                                                            _ws(cx, _lib.OP_LOGZ_BWD), ptab if table else offsets, table))
            _whole_tensor(cx, dS)
            what = f"logprob_bwd{'_t' if table else ''} {gname}"
            res = sa.check_dense(what, _sub(cx, dS, 2), _sub(cx, dN, 1), tr, g64[tr.idx], K, paths=cx.sub_paths, flush=cx.persist)
            for k, r in res.items():
                _note(cx, f"{what} {k}", r)


def _query(T, chains):
    """(pairs [K, 2], offsets) of band cells, far cells and diagonal cells for every chain."""
    base = [(0, 0), (T - 1, T - 1), (T // 2, T // 2), (0, 1), (T - 2, T - 1), (0, T - 1), (1, T - 2), (3, min(3 + 20, T - 1)),
            (T // 3, min(T // 3 + 63, T - 1)), (T // 3, min(T // 3 + 64, T - 1)), (2, min(2 + 65, T - 1)), (5, T - 1), (0, T // 2)]
    base = [(b, e) for b, e in base if 0 <= b <= e < T]
    pairs, offsets = [], [0]
    for c in range(chains):
        lst = base[c % 3:] + base[:c % 3]
        pairs += lst
        offsets.append(len(pairs))
    return np.asarray(pairs, dtype=np.int32).reshape(-1, 2), np.asarray(offsets, dtype=np.int32)


def op_interval_marginals(request, oracle, case, which, impl):
    """The packed marginals of a list that names band cells, far cells and diagonal cells, from the device's own alpha, beta and logZ."""
    cx = context(request, oracle, case, which, impl)
    tr, K, T, B, dev = cx.tr, cx.K, cx.T, cx.B, cx.dev
    q = torch.empty(T, B, dtype=F32, device=dev)
    _with_impl(impl, lambda: _lib.ops().beta(cx.sd, cx.nd, q, _ws(cx, _lib.OP_LOGZ_FWD)))
    pairs, offsets = _query(T, B)
    out = torch.empty(len(pairs), dtype=F32, device=dev)
    _lib.ops().interval_marginals(cx.sd, cx.v, q, cx.logZ, torch.from_numpy(pairs).to(dev), len(pairs), torch.from_numpy(offsets).to(dev), out)
    out = out.cpu().numpy()
    cb = tr.cell_bound(K, sa.ROWSEQ)
    got, m, bound = [], [], []
    for j, c in enumerate(tr.idx):
        for k in range(offsets[c], offsets[c + 1]):
            b, e = pairs[k]
            got.append(out[k]); m.append(tr.m[e, b, j]); bound.append(cb[e, b, j])
    # (a marginal above 1 by rounding is clamped to 1, which moves it towards the truth)
    _note(cx, "interval_marginals", sa.check_values("interval_marginals", np.asarray(got), np.asarray(m), 1.0, np.asarray(bound)))


OPS = {"forward": op_forward_sweeps, "logz_bwd": op_logz_bwd, "logprob_bwd": op_logprob_bwd, "interval_marginals": op_interval_marginals}


@pytest.mark.parametrize("op", sorted(OPS))                    # (the top decorator varies fastest: a case's four ops share its context)
@pytest.mark.parametrize("case,which,impl", RUNS)
def test_sweep_accuracy(request, oracle, case, which, impl, op):
    OPS[op](request, oracle, case, which, impl)


# ---- what the bounds are worth (no device) --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SMALL_CASES + [_case("balanced", 33, 1)])
def test_fp32_oracle_is_inside_every_bound(oracle, case):
    """oracle.forward_backward (the plain fp32 recurrence) against float64 under the tighter constants (ROWSEQ; PERSIST's are larger in
    every term): every alpha, beta, logZ, marginal and noise marginal.  The worst ratios are printed."""
    family, T, B = case
    score, noise, tr = truth_of(oracle, family, T, B)
    ix = torch.tensor(tr.idx)
    lz, grad, gn, v, q = oracle.forward_backward(score.index_select(2, ix).numpy(), noise.index_select(1, ix).numpy())
    for K in (sa.ROWSEQ, sa.PERSIST):
        r = {"logZ": sa.check_log("logZ", lz, tr.lz, tr.logz_bound(K)), "alpha": sa.check_log("alpha", v, tr.v, tr.alpha_bound(K)),
             "beta": sa.check_log("beta", q, tr.q, tr.beta_bound(K))}
        r.update(sa.check_dense("fp32 oracle", grad, gn, tr, np.ones(len(tr.idx)), K))
        print(f"ACC {family} T={T} B={B} fp32-oracle under {K['name']}: " + ", ".join(f"{k} {x:.4f}" for k, x in r.items()))
        assert max(r.values()) <= 1.0


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


BOTH = [pytest.param(sa.ROWSEQ, id="rowseq"), pytest.param(sa.PERSIST, id="persist")]      # the constants of every implementation the check is used with


def _oracle32(oracle, family, T, B, K):
    """The fp32 oracle's results for the truth's chains (all of them up to 12), which pass the check as they are."""
    score, noise, tr = truth_of(oracle, family, T, B)
    ix = torch.tensor(tr.idx)
    lz, grad, gn, v, q = oracle.forward_backward(score.index_select(2, ix).numpy(), noise.index_select(1, ix).numpy())
    sa.check_dense("unmutated", grad, gn, tr, np.ones(len(tr.idx)), K)
    return score, noise, tr, lz, grad, gn


@pytest.mark.parametrize("K", BOTH)
def test_mutant_small_cells_zeroed(oracle, K):
    """Every cell whose marginal is below 5e-5 set to zero -- more than 80 % of the cells of `randn` at T = 70, 4 % of `balanced` at
    T = 130: today's gate accepts both."""
    for family, T, B in (("randn", 70, 20), ("balanced", 130, 6)):
        score, noise, tr, lz, grad, gn = _oracle32(oracle, family, T, B, K)
        mut = np.where(tr.m < 5e-5, 0.0, grad).astype(np.float32)
        assert np.mean(mut[tr.tril] == 0.0) > (0.8 if family == "randn" else 0.02)
        assert sa.old_gate_accepts(mut, tr.m, tr.lz)
        assert _rejected(lambda: sa.check_dense("mutant 1", mut, gn, tr, np.ones(len(tr.idx)), K))


# the far tile's factor 1 + 2^-j: the smallest power of two each set of constants rejects at T = 97, where ln(1 + 2^-9) = 1.95e-3 stands
# against ROWSEQ's 1.83e-3 on the tile's first column and PERSIST's 4.58e-3 (twice the roundings at |alpha| per step, and the far
# field's exponent arithmetic at magnitude 100): ln(1 + 2^-7) = 7.8e-3 is out, ln(1 + 2^-8) = 3.9e-3 is in
TILE_J = {"rowseq": 9, "persist": 7}


@pytest.mark.parametrize("K", BOTH)
def test_mutant_one_far_tile_scaled(oracle, K):
    """The 16 x 16 far tile (row block 6, column block 1) times 1 + 2^-j at the shortest length that has the row block.  j = 9 is
    rejected under the constants of the row-sequential kernels and the host mirror.  Under the persistent sweep's it is NOT: that
    check's blind spot is pinned here -- it rejects 2^-7 and accepts 2^-8."""
    T, B = 97, 4
    score, noise = sa.balanced(T, B, 31)
    tr = sa.Truth(oracle, score, noise)
    assert tr.under_floor == 0.0
    lz, grad, gn, v, q = oracle.forward_backward(score.numpy(), noise.numpy())
    sa.check_dense("unmutated", grad, gn, tr, np.ones(B), K)

    def scaled(j):
        mut = grad.copy()
        mut[96:112, 16:32] *= np.float32(1.0 + 2.0 ** -j)
        return mut
    j = TILE_J[K["name"]]
    assert sa.old_gate_accepts(scaled(j), tr.m, tr.lz) and sa.old_gate_accepts(scaled(9), tr.m, tr.lz)
    assert _rejected(lambda: sa.check_dense("mutant 2", scaled(j), gn, tr, np.ones(B), K))
    assert not _rejected(lambda: sa.check_dense("mutant 2, half", scaled(j + 1), gn, tr, np.ones(B), K))


@pytest.mark.parametrize("K", BOTH)
def test_mutant_neighbours_logz(oracle, K):
    """One chain's cells normalised with the neighbour's logZ, the two less than 1e-4 apart relative: a hand-off read from the next
    chain.  The pair: chain 1 is chain 0 with every noise score raised by a constant."""
    T = 33
    s1, n1 = sa.balanced(T, 1, 31)
    probe = 1e-3

    def pair(delta):
        score = torch.cat([s1, s1], dim=2).contiguous()
        noise = torch.cat([n1, n1 + np.float32(delta)], dim=1).contiguous()
        return score, noise
    lz = oracle.forward_backward_f64(*[t.numpy() for t in pair(probe)])[0]
    delta = probe * 9e-5 * abs(lz[0]) / abs(lz[1] - lz[0])                  # one secant step: logZ is smooth in the shift
    score, noise = pair(delta)
    tr = sa.Truth(oracle, score, noise)
    gap = abs(tr.lz[1] - tr.lz[0])
    assert 8e-5 * abs(tr.lz[0]) < gap < 1e-4 * abs(tr.lz[0])
    lz32, grad, gn, v, q = oracle.forward_backward(score.numpy(), noise.numpy())
    sa.check_dense("unmutated", grad, gn, tr, np.ones(2), K)
    mut = grad.copy()
    mut[:, :, 0] = (grad[:, :, 0].astype(np.float64) * np.exp(float(lz32[0]) - float(lz32[1]))).astype(np.float32)
    assert sa.old_gate_accepts(mut, tr.m, tr.lz)
    assert _rejected(lambda: sa.check_dense("mutant 3", mut, gn, tr, np.ones(2), K))


@pytest.mark.parametrize("K", BOTH)
def test_mutant_path_term_one_column_left(oracle, K):
    """logProb's backward with the path's term on the neighbouring cell (end, begin - 1)."""
    family, T, B = "balanced", 65, 5
    score, noise, tr, lz, grad, gn = _oracle32(oracle, family, T, B, K)
    g = sa.mixed_gout(B, 1)
    paths = sa.target_paths(T, B)
    good = np.where(tr.tril[:, :, None], -g * grad.astype(np.float64), 0.0)
    cover = np.zeros((T - 1, B))
    for c, lst in enumerate(paths):
        for b, e in lst:
            good[e, b, c] += g[c]
            cover[b:e, c] += 1
    good = good.astype(np.float32)
    dn = (g * (1.0 - cover - gn)).astype(np.float32)
    sa.check_dense("unmutated", good, dn, tr, g, K, paths=paths)
    mut = good.copy()
    b, e = paths[3][1]                                             # an interval of chain 3 that begins after frame 0
    assert b >= 1 and e > b and g[3] != 0.0
    mut[e, b, 3] -= np.float32(g[3])
    mut[e, b - 1, 3] += np.float32(g[3])
    assert _rejected(lambda: sa.check_dense("mutant 4", mut, dn, tr, g, K, paths=paths))


@pytest.mark.parametrize("K", BOTH)
def test_mutant_dnoise_entry_moved(oracle, K):
    """One dNoise entry moved by four times its bound."""
    family, T, B = "balanced", 65, 5
    score, noise, tr, lz, grad, gn = _oracle32(oracle, family, T, B, K)
    bound = tr.mn * np.expm1(tr.gap_bound(K)) + 3 * sa.U
    t, c = 40, 3
    mut = gn.astype(np.float64)
    mut[t, c] = tr.mn[t, c] + 4.0 * bound[t, c]
    assert _rejected(lambda: sa.check_dense("mutant 5", grad, mut, tr, np.ones(B), K))


def test_floor_caps_on_the_truth(oracle):
    """Every cap of FLOOR_CAP and FLUSH_CAP holds on the float64 truth of its case (truth_of asserts them before any op runs); none of
    `balanced` is left out by either."""
    for p in SMALL_CASES:
        family, T, B = p.values[0]
        tr = truth_of(oracle, family, T, B)[2]
        print(f"ACC floor {family} T={T} B={B}: {tr.under_floor:.4f} of the cells are under 2^-100 (cap {sa.floor_cap(family, T)}), "
              f"smallest marginal {tr.min_marginal:.3e}, A = {tr.A.max():.1f}; the underflow rule exempts {tr.flush_share():.5f}")
        assert tr.under_floor <= sa.floor_cap(family, T) and tr.flush_share() <= sa.flush_cap(family, T)
        if family == "balanced":
            assert tr.under_floor == 0.0 and not tr.may_flush().any()


@pytest.mark.gpu
def test_device_status_is_clean(gpu):
    assert _lib.device_status() == 0
