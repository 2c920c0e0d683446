"""Posterior sampling of interval paths (NeuralSemiCRFInterval.sample / sample_packed, semicrf_sample).

The draws are a pure function of (inputs, key), so every test here is deterministic: a fixed generator seed makes the key.
CPU tests check the distribution itself (exact enumeration for tiny T, marginals against forward_backward, a float64
restatement of the contract); GPU tests check the device against the same properties, against the host kernel, and step by step
against the float64 CDF of every visited row (tests/sample_common.py)."""
import importlib
import math
import types

import numpy as np
import pytest
import torch

from conftest import edge_inputs
from sample_common import (StepCase, _alpha64, _check_valid, _restated_sample, _restated_walk, _segments, _steps_to_path, _u, _uniforms,
                           check_steps, flat_inputs, pack_paths)
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")     # the module (the package exports the class by that name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _key(seed):
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=_gen(seed)))


def _mixed_inputs(T, seeds=(3, 4, 5)):
    """Three chains with different constructions (randn, model, ties)."""
    parts = [synth.crf_inputs(T, 1, s, "cpu", kind) for s, kind in zip(seeds, ("randn", "model", "ties"))]
    return (torch.cat([p[0] for p in parts], 2).contiguous(), torch.cat([p[1] for p in parts], 1).contiguous())


# ---- exact distribution --------------------------------------------------------------------------------------------------

def _enumerate_paths(T):
    """Every path on frames 0..T-1 (walked from T-1): a list of sorted interval lists."""
    paths = []

    def walk(t, acc):
        for single in (False, True):
            cur = acc + [(t, t)] if single else acc
            if t == 0:
                paths.append(sorted(cur))
                continue
            walk(t - 1, cur)
            for j in range(t):
                walk(j, cur + [(j, t)])
    walk(T - 1, [])
    return paths


def _path_logscore(path, s, n, c):
    T = s.shape[0]
    cum = np.concatenate([[0.0], np.cumsum(n[:, c].astype(np.float64))]) if T > 1 else np.zeros(1)
    acc = cum[T - 1]
    for b, e in path:
        acc += float(s[e, b, c]) - (cum[e] - cum[b])
    return acc


def _gtest_pvalue(obs, exp_):
    m = obs > 0
    G = 2.0 * float(np.sum(obs[m] * np.log(obs[m] / exp_[m])))
    df = int((exp_ > 0).sum()) - 1
    if df <= 0:
        return 1.0
    z = ((G / df) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * df))) / math.sqrt(2.0 / (9.0 * df))     # Wilson-Hilferty
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def _path_keys(pairs, offsets, T):
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    keys = np.zeros(len(offsets) - 1, np.int64)
    np.add.at(keys, seg, np.left_shift(np.int64(1), pairs[:, 0] * T + pairs[:, 1]))
    return keys


def _key_of(path, T):
    return sum(1 << (b * T + e) for b, e in path)


@pytest.mark.parametrize("T", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("forced", [False, True])
def test_exact_distribution_cpu(T, forced):
    s, n = _mixed_inputs(T)
    B = 3
    N = 200_000
    ends = [T - 1, T // 2, 0] if forced else None
    pairs, offsets = CRF.sample_packed(s, n, N, forcedEndPos=ends, generator=_gen(100 + T))
    _check_valid(pairs, offsets, T, ends, B)
    keys = _path_keys(pairs, offsets, T).reshape(N, B)
    sn, nn = s.numpy(), n.numpy()
    logz = CRF.computeLogZ(s, n).numpy()
    for c in range(B):
        e = T - 1 if ends is None else ends[c]
        paths = _enumerate_paths(e + 1)
        ls = np.array([_path_logscore(p, sn[:e + 1, :e + 1], nn[:e], c) for p in paths])
        lz = np.logaddexp.reduce(ls)
        if e == T - 1:
            assert abs(lz - float(logz[c])) < 1e-4 * max(1.0, abs(lz))        # the enumeration is the whole distribution
        p = np.exp(ls - lz)
        index = {_key_of(path, T): i for i, path in enumerate(paths)}
        assert len(index) == len(paths)
        obs = np.zeros(len(paths))
        uk, cnt = np.unique(keys[:, c], return_counts=True)
        for k_, m_ in zip(uk, cnt):
            assert int(k_) in index, "a drawn path is not a path"
            obs[index[int(k_)]] += m_
        pv = _gtest_pvalue(obs, N * p)
        assert pv > 1e-4, (c, pv)


# ---- marginals -----------------------------------------------------------------------------------------------------------

MARGINAL_CASES = [("ties", 9, "ties", 20, None), ("posdiag", 7, "randn", 18, "posdiag"), ("noise0", 7, "randn", 19, "noise0"),
                  ("model", 6, "model", 22, None)]


def _check_marginals(device, name, B, kind, seed, tr, n=4096):
    T = 48
    s, nz = edge_inputs(T, B, kind, seed, tr, device)
    _, grad, gnoise = CRF.forward_backward(s, nz)
    grad = grad.cpu().double().numpy(); gnoise = gnoise.cpu().double().numpy()
    pairs, offsets = CRF.sample_packed(s, nz, n, generator=_gen(seed))
    _check_valid(pairs, offsets, T)
    pairs = pairs.astype(np.int64)
    seg = np.repeat(np.arange(n * B), np.diff(offsets))
    c = seg % B
    cnt = np.zeros((T, T, B))
    np.add.at(cnt, (pairs[:, 1], pairs[:, 0], c), 1.0)
    cover = np.zeros((T + 1, B))
    ivl = pairs[:, 0] < pairs[:, 1]
    np.add.at(cover, (pairs[ivl, 0], c[ivl]), 1.0)
    np.add.at(cover, (pairs[ivl, 1], c[ivl]), -1.0)
    covered = np.cumsum(cover, 0)[:T - 1]
    tril = np.tril(np.ones((T, T), bool))
    f = cnt / n
    tol = 6.0 * np.sqrt(np.clip(grad * (1 - grad), 0, None) / n) + 2.0 / n
    bad = (np.abs(f - grad) > tol) & tril[:, :, None]
    assert not bad.any(), (name, np.argwhere(bad)[:5], f[bad][:5], grad[bad][:5])
    fg = 1.0 - covered / n
    tolg = 6.0 * np.sqrt(np.clip(gnoise * (1 - gnoise), 0, None) / n) + 2.0 / n
    assert (np.abs(fg - gnoise) <= tolg).all(), name


@pytest.mark.parametrize("case", MARGINAL_CASES, ids=[c[0] for c in MARGINAL_CASES])
def test_marginals_cpu(case):
    _check_marginals("cpu", *case)


# ---- restatement -----------------------------------------------------------------------------------------------------------

def _agreement(paths_a, paths_b):
    return sum(a == b for a, b in zip(paths_a, paths_b)) / len(paths_a)


def test_restatement_agreement_cpu():
    T, B, N = 64, 20, 16
    s, n = synth.crf_inputs(T, B, 31, "cpu")
    key = _key(7)
    v = _alpha64(s.numpy().astype(np.float64), n.numpy().astype(np.float64))
    want = _restated_sample(s.numpy(), n.numpy(), v, N, key)
    pairs, offsets = CRF.sample_packed(s, n, N, generator=_gen(7))
    got = _segments(pairs, offsets)
    assert _agreement(got, want) >= 0.99
    ends = [int(x) for x in np.arange(B) * 3 % T]
    want = _restated_sample(s.numpy(), n.numpy(), v, N, key, ends)
    got = _segments(*CRF.sample_packed(s, n, N, forcedEndPos=ends, generator=_gen(7)))
    assert _agreement(got, want) >= 0.99


# ---- step by step ------------------------------------------------------------------------------------------------------------
# sample_common.StepCase holds the reference side of a case (the float64 restatement's draws, the band delta from the plain-fp32
# restatement's own error, the ambiguous share); a sampler's draws of the same case go through StepCase.check.

def _step_inputs(T, B, seed, kind, device="cpu"):
    """(score, noise, alpha) as fp32 numpy; alpha is the float64 recursion on these inputs, rounded once.  device: where the hash
    of synth.crf_inputs runs (the same bits on either)"""
    if kind == "flat":
        return flat_inputs(T, B, seed)
    s, n = synth.crf_inputs(T, B, seed, device, kind)
    s, n = s.cpu().numpy(), n.cpu().numpy()
    return s, n, _alpha64(s, n).astype(np.float32)


def _mixed_ends(T, B):
    """0, 1 and T - 1 first, then a mixed set"""
    return ([0, 1, T - 1] + [int(x) for x in (np.arange(B) * 7 + 3) % T])[:B]


def _raw_draws(st, nt, vt, k0, N, key, ends):
    """semicrf_sample alone, where the tensors live, on the alpha handed in: (pairs, offsets) as numpy"""
    e = torch.tensor(ends, dtype=torch.int32, device=st.device) if ends is not None else None
    p, o = crf_mod._sample_raw(st, nt, vt, k0, N, key, e)
    o = o.cpu().numpy()
    return p[:int(o[-1])].cpu().numpy(), o


def _run_case(case, tensors):
    """the case's draws from the sampler where `tensors` (score, noise, alpha) live: zero violations"""
    pairs, offsets = _raw_draws(*tensors, case.k0, case.nSample, case.key, case.ends)
    bad, steps, amb = case.check(pairs, offsets)
    assert not bad, (case.name, len(bad), bad[:5])
    assert steps > 0
    return pairs, offsets


def _tensors(arrays, device):
    return tuple(torch.from_numpy(x).to(device) for x in arrays)


def _coins_in_band(case):
    _, u1 = _uniforms(case.T, case.B, case.nSample, case.key, case.k0)
    n = 0
    for i, walk in enumerate(case.walks):
        k, c = divmod(i, case.B)
        for t, _, _ in walk:
            p = 1.0 / (1.0 + math.exp(-float(case.score[t, t, c])))
            n += abs(u1[k, c, t] - p) <= 8 * 2.0 ** -24
    return n


STEP_KINDS = ["randn", "model", "flat"]


@pytest.mark.parametrize("kind", STEP_KINDS)
@pytest.mark.parametrize("forced", [False, True])
def test_steps_restatement_cpu(kind, forced):
    """The restatement's own draws: admissible at every step (StepCase asserts it at its band), and with NO band -- delta = 0 --
    still without a violation and without an ambiguous pick: what is ambiguous there is a coin inside its exception, nothing else."""
    T, B, N = 64, 20, 16
    arrays = _step_inputs(T, B, 31, kind)
    case = StepCase(f"restatement {kind}", *arrays, _key(7), 0, N, _mixed_ends(T, B) if forced else None)
    assert case.paths == _restated_sample(*arrays, N, case.key, case.ends)
    bad, steps, amb = check_steps(*arrays, case.key, 0, N, case.ends, *pack_paths(case.paths), 0.0)
    assert not bad and steps == sum(len(w) for w in case.walks)
    assert amb == _coins_in_band(case)


def test_steps_mutation_cpu():
    """One clear pick moved by one candidate and one clear coin flipped: the checker reports exactly those two steps."""
    T, B, N = 64, 20, 4
    arrays = _step_inputs(T, B, 33, "randn")
    case = StepCase("mutation", *arrays, _key(8), 0, N)
    u0, u1 = _uniforms(T, B, N, case.key)
    moved = flipped = None
    paths = list(case.paths)
    for i, walk in enumerate(case.walks):
        k, c = divmod(i, B)
        for pos, (t, pick, single) in enumerate(walk):
            if moved is None and t >= 8 and pick is not None:
                cs = case.cums[t][c]
                u = u0[k, c, t] * cs[-1]
                d = case.delta * cs[-1]
                alt = pick + 1
                # clear: the pick is the only admissible candidate, with room to spare, and its neighbour exists
                if alt <= t and (pick == 0 or cs[pick - 1] < u - 2 * d) and cs[pick] > u + 2 * d:
                    tail = _restated_walk(*arrays, u0[k, c], u1[k, c], c, t - alt, case.cums)
                    paths[i] = _steps_to_path(walk[:pos] + [(t, alt, single)] + tail)
                    moved = (k, c, t, "pick")
                    break
            if flipped is None and moved is not None and (k, c) != moved[:2]:
                p = 1.0 / (1.0 + math.exp(-float(arrays[0][t, t, c])))
                if abs(u1[k, c, t] - p) > 0.01:
                    paths[i] = _steps_to_path(walk[:pos] + [(t, pick, not single)] + walk[pos + 1:])
                    flipped = (k, c, t, "coin")
                    break
        if moved and flipped:
            break
    assert moved and flipped
    bad, steps, amb = case.check(*pack_paths(paths))
    assert sorted(b[:4] for b in bad) == sorted([moved, flipped])
    # and the unchanged draws stay clean
    assert not case.check(*pack_paths(case.paths))[0]


HOST_STEP_CASES = [(64, 20, 16, kind, forced) for kind in STEP_KINDS for forced in (False, True)] + [(2050, 2, 2, "flat", False)]


@pytest.mark.parametrize("T,B,N,kind,forced", HOST_STEP_CASES, ids=str)
def test_steps_host_kernel_cpu(T, B, N, kind, forced):
    """The host kernel (float64 sums of fp32 log-weights) through the same checker, at the band of the case."""
    arrays = _step_inputs(T, B, 35 + T, kind)
    case = StepCase(f"host {kind} T={T}", *arrays, _key(T + forced), 0, N, _mixed_ends(T, B) if forced else None)
    _run_case(case, _tensors(arrays, "cpu"))
    if T > 2048:
        share, count = case.far_chunk_share()
        assert count > 0 and share > 0.5, (share, count)


# ---- low temperature -----------------------------------------------------------------------------------------------------

def _low_temperature(device):
    T, B = 40, 6
    s, n = synth.crf_inputs(T, B, 41, "cpu")
    d = torch.diagonal(s, dim1=0, dim2=1)
    d.copy_(torch.sign(d) * d.abs().clamp(min=0.25))
    s, n = (s * 1e3).to(device), (n * 1e3).to(device)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    best = crf.decode(forward=True)
    for path in crf.sample(8, generator=_gen(5)):
        assert path == best
    ends = [5, 39, 0, 17, 30, 1]
    best = crf.decode(forcedStartPos=ends, forward=True)
    for path in crf.sample(4, forcedEndPos=ends, generator=_gen(6)):
        assert path == best


def test_low_temperature_is_decode_cpu():
    _low_temperature("cpu")


# ---- edge cases ----------------------------------------------------------------------------------------------------------

def _masked(device):
    T, B = 6, 5
    for mask in ("one_cell", "whole_row"):
        score, noise = synth.crf_inputs(T, B, 11, "cpu")
        if mask == "one_cell":
            score[T - 1, 0, :] = float("-inf")
        else:
            noise[0, :] = float("-inf")
            score[1, 0, :] = float("-inf")
        crf = CRF.NeuralSemiCRFInterval(score.to(device), noise.to(device))
        pairs, offsets = crf.sample_packed(512, generator=_gen(9))
        _check_valid(pairs, offsets, T)
        pl = [tuple(p) for p in pairs.tolist()]
        if mask == "one_cell":
            assert (0, T - 1) not in pl
        else:
            assert (0, 1) not in pl
            # frame 1 is unreachable: never visited, never an endpoint
            assert all(1 not in p for p in pl)
        if mask == "one_cell":              # (a -inf noise makes evalPath's prefix sums NaN whatever the path)
            for path in crf.sample(4, generator=_gen(10)):
                assert torch.isfinite(crf.evalPath(path)).all()


def _dtypes_layouts(device):
    T, B = 20, 4
    s, n = synth.crf_inputs(T, B, 12, "cpu")
    s, n = s.to(device), n.to(device)
    ref = CRF.sample_packed(s, n, 6, generator=_gen(3))
    got = CRF.sample_packed(s.double(), n.double(), 6, generator=_gen(3))
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))
    sb, nb = s.bfloat16(), n.bfloat16()
    got = CRF.sample_packed(sb, nb, 6, generator=_gen(3))
    want = CRF.sample_packed(sb.float(), nb.float(), 6, generator=_gen(3))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    _check_valid(*got, T)
    big = torch.zeros(T, T, 2 * B, device=device); big[:, :, ::2] = s
    bign = torch.zeros(T - 1, 2 * B, device=device); bign[:, ::2] = n
    got = CRF.sample_packed(big[:, :, ::2], bign[:, ::2], 6, generator=_gen(3))
    assert all(np.array_equal(a, b) for a, b in zip(ref, got))
    # B = 1
    s1, n1 = s[:, :, 2:3].contiguous(), n[:, 2:3].contiguous()
    p1, o1 = CRF.sample_packed(s1, n1, 6, generator=_gen(3))
    assert o1.shape == (7,)
    _check_valid(p1, o1, T)


def _argument_errors(device):
    s, n = synth.crf_inputs(8, 3, 13, device)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    with pytest.raises(ValueError):
        crf.sample(0)
    with pytest.raises(ValueError):
        crf.sample_packed(-2)
    with pytest.raises(IndexError):
        crf.sample(2, forcedEndPos=[0, 8, 1])
    with pytest.raises(IndexError):
        crf.sample(2, forcedEndPos=[-1, 0, 1])
    with pytest.raises(IndexError):
        crf.sample(2, forcedEndPos=[1, 2])
    if torch.cuda.is_available():
        cuda_gen = torch.Generator(device="cuda")
    else:                                   # what the check looks at: the generator's device
        cuda_gen = types.SimpleNamespace(device=torch.device("cuda"))
    with pytest.raises(ValueError, match="CPU torch.Generator"):
        crf.sample(1, generator=cuda_gen)


def _determinism(device, monkeypatch):
    T, B = 30, 5
    s, n = synth.crf_inputs(T, B, 14, device)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    a = crf.sample_packed(9, generator=_gen(21))
    b = crf.sample_packed(9, generator=_gen(21))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # prefix stability: the first m of n draws are sample(m)
    m = crf.sample_packed(4, generator=_gen(21))
    assert _segments(*m) == _segments(*a)[:4 * B]
    assert crf.sample(9, generator=_gen(21))[:4] == crf.sample(4, generator=_gen(21))
    # a draw split over several device calls (k0 > 0) is the same draw
    monkeypatch.setattr(crf_mod, "_SAMPLE_CELLS", 2 * B * T)
    c = crf.sample_packed(9, generator=_gen(21))
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    # torch.manual_seed reproduces a draw made with the default generator
    torch.manual_seed(77)
    d = crf.sample_packed(3)
    torch.manual_seed(77)
    e = crf.sample_packed(3)
    assert all(np.array_equal(x, y) for x, y in zip(d, e))
    # every draw is a path, and a finite-score one
    for path in crf.sample(9, generator=_gen(21)):
        assert torch.isfinite(crf.evalPath(path)).all()
        lp = crf.logProb(path)
        assert torch.isfinite(lp).all() and (lp <= 1e-4).all()


def test_masked_cells_cpu():
    _masked("cpu")


def test_dtypes_layouts_cpu():
    _dtypes_layouts("cpu")


def test_argument_errors_cpu():
    _argument_errors("cpu")


def test_determinism_and_prefix_cpu(monkeypatch):
    _determinism("cpu", monkeypatch)


def test_T1_cpu():
    s = torch.tensor([[[3.0, -3.0, 0.0]]])
    out = CRF.sample(s, torch.zeros(0, 3), 2000, generator=_gen(4))
    assert all(p[c] in ([], [(0, 0)]) for p in out for c in range(3))
    freq = [np.mean([p[c] == [(0, 0)] for p in out]) for c in range(3)]
    want = torch.sigmoid(s[0, 0]).tolist()
    assert all(abs(f - w) < 0.05 for f, w in zip(freq, want))


# ---- GPU -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", MARGINAL_CASES, ids=[c[0] for c in MARGINAL_CASES])
def test_marginals_gpu(gpu, case):
    _check_marginals(gpu, *case)


@pytest.mark.gpu
def test_low_temperature_is_decode_gpu(gpu):
    _low_temperature(gpu)


@pytest.mark.gpu
def test_masked_cells_gpu(gpu):
    """The sampler kernel on -inf cells and rows.  Alpha comes from the host kernel here: the device's forward sweep does not take
    -inf cells (its logZ is NaN there, which sample() reports as an error), so this isolates what the sampler itself does."""
    T, B, N = 6, 5, 512
    for mask in ("one_cell", "whole_row"):
        score, noise = synth.crf_inputs(T, B, 11, "cpu")
        if mask == "one_cell":
            score[T - 1, 0, :] = float("-inf")
        else:
            noise[0, :] = float("-inf")
            score[1, 0, :] = float("-inf")
        _, v = crf_mod._logz_fwd_raw(score, noise, True)
        key = _key(9)
        pg, og = crf_mod._sample_raw(score.to(gpu), noise.to(gpu), v.to(gpu), 0, N, key, None)
        og = og.cpu().numpy()
        pg = pg[:int(og[-1])].cpu().numpy()
        _check_valid(pg, og, T)
        pc, oc = crf_mod._sample_raw(score, noise, v, 0, N, key, None)
        oc = oc.numpy(); pc = pc[:int(oc[-1])].numpy()
        assert _agreement(_segments(pg, og), _segments(pc, oc)) >= 0.99
        pl = [tuple(p) for p in pg.tolist()]
        if mask == "one_cell":
            assert (0, T - 1) not in pl
        else:
            assert (0, 1) not in pl and all(1 not in p for p in pl)


@pytest.mark.gpu
def test_dtypes_layouts_gpu(gpu):
    _dtypes_layouts(gpu)


@pytest.mark.gpu
def test_argument_errors_gpu(gpu):
    _argument_errors(gpu)


@pytest.mark.gpu
def test_determinism_and_prefix_gpu(gpu, monkeypatch):
    _determinism(gpu, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 33, 65])
def test_chain_counts_gpu(gpu, B):
    T = 50
    s, n = synth.crf_inputs(T, B, 60 + B, "cpu")
    got = _segments(*CRF.sample_packed(s.to(gpu), n.to(gpu), 8, generator=_gen(B)))
    want = _segments(*CRF.sample_packed(s, n, 8, generator=_gen(B)))
    _check_valid(*CRF.sample_packed(s.to(gpu), n.to(gpu), 8, generator=_gen(B)), T)
    assert _agreement(got, want) >= 0.99


@pytest.mark.gpu
def test_T1_gpu(gpu):
    s = torch.tensor([[[3.0, -3.0, 0.0]]])
    n = torch.zeros(0, 3)
    got = CRF.sample_packed(s.to(gpu), n.to(gpu), 64, generator=_gen(4))
    want = CRF.sample_packed(s, n, 64, generator=_gen(4))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N", [(256, 90, 8), (691, 360, 4)])
def test_gpu_matches_cpu(gpu, T, B, N):
    """Same key, same alpha (the device's, handed to both samplers): the device kernel and the host kernel differ only in the
    sampler's own fp32 / float64 arithmetic, i.e. only where a uniform lands within rounding of a CDF boundary."""
    s, n = synth.crf_inputs(T, B, 70 + T, "cpu")
    sg, ng = s.to(gpu), n.to(gpu)
    _, v = crf_mod._logz_fwd_raw(sg, ng, True)
    ends = [int(x) for x in (np.arange(B) * 7) % T]
    for e in (None, ends):
        key = _key(T if e is None else T + 1)
        eg = torch.tensor(e, dtype=torch.int32, device=gpu) if e is not None else None
        pg, og = crf_mod._sample_raw(sg, ng, v, 0, N, key, eg)
        og = og.cpu().numpy(); pg = pg[:int(og[-1])].cpu().numpy()
        _check_valid(pg, og, T, e, B)
        ec = torch.tensor(e, dtype=torch.int32) if e is not None else None
        pc, oc = crf_mod._sample_raw(s, n, v.cpu(), 0, N, key, ec)
        oc = oc.numpy(); pc = pc[:int(oc[-1])].numpy()
        assert _agreement(_segments(pg, og), _segments(pc, oc)) >= 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N,floor", [(256, 90, 8, 0.99), (691, 360, 4, 0.95)])
def test_gpu_matches_cpu_end_to_end(gpu, T, B, N, floor):
    """Through the public API, each device with its own alpha.  The two forward sweeps agree to a few ulps, and an ulp of alpha is a
    relative weight change of ~1e-4 at T=691 (alpha ~ 1e3): a path of ~650 draws then differs from the host's with a probability
    of a few per cent -- rounding at CDF boundaries, not a different distribution (the marginal tests check that)."""
    s, n = synth.crf_inputs(T, B, 70 + T, "cpu")
    got = CRF.sample_packed(s.to(gpu), n.to(gpu), N, generator=_gen(T))
    _check_valid(*got, T)
    want = CRF.sample_packed(s, n, N, generator=_gen(T))
    assert _agreement(_segments(*got), _segments(*want)) >= floor


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,N", [(1024, 352, 8), (2048, 88, 4)])
def test_full_size_gpu(gpu, T, B, N):
    s, n = synth.crf_inputs(T, B, 80 + B, gpu)
    crf = CRF.NeuralSemiCRFInterval(s, n)
    a = crf.sample_packed(N, generator=_gen(T))
    b = crf.sample_packed(N, generator=_gen(T))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    _check_valid(*a, T)
    assert a[1].shape == (N * B + 1,)
    for path in crf.sample(N, generator=_gen(T)):
        lp = crf.logProb(path)
        assert torch.isfinite(lp).all() and (lp <= 1e-3).all()


# ---- GPU: every step of every draw against the float64 CDF of its row ------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_steps_chain_tiles_gpu(gpu, B):
    """One lane per chain, 64 chains per workgroup: one chain, a full tile, a ragged second tile, a ragged third."""
    T, N = 50, 9
    arrays = _step_inputs(T, B, 90 + B, "randn" if B != 64 else "model")
    tensors = _tensors(arrays, gpu)
    for ends in (None, _mixed_ends(T, B)):
        _run_case(StepCase(f"tiles B={B} ends={ends is not None}", *arrays, _key(B), 0, N, ends), tensors)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 8, 9, 17])
def test_steps_draw_loop_gpu(gpu, N):
    """The draws of a (row, chain) are dealt to 8 waves: fewer draws than waves, one each, one more, two rounds and one."""
    T, B = 50, 5
    arrays = _step_inputs(T, B, 95, "randn")
    tensors = _tensors(arrays, gpu)
    for ends in (None, _mixed_ends(T, B)):
        _run_case(StepCase(f"draws N={N} ends={ends is not None}", *arrays, _key(N), 0, N, ends), tensors)


@pytest.mark.gpu
def test_steps_split_call_gpu(gpu):
    """Nine draws as two calls (k0 = 0 and k0 = 5) are the nine draws of one call, bit for bit, and each call passes on its own."""
    T, B, N = 50, 5, 9
    arrays = _step_inputs(T, B, 96, "randn")
    tensors = _tensors(arrays, gpu)
    key = _key(96)
    for ends in (None, _mixed_ends(T, B)):
        whole = _run_case(StepCase("split 0..8", *arrays, key, 0, N, ends), tensors)
        lo = _run_case(StepCase("split 0..4", *arrays, key, 0, 5, ends), tensors)
        hi = _run_case(StepCase("split 5..8", *arrays, key, 5, 4, ends), tensors)
        assert np.array_equal(np.concatenate([lo[0], hi[0]]), whole[0])
        assert np.array_equal(np.concatenate([lo[1], hi[1][1:] + lo[1][-1]]), whole[1])


def _long_case(gpu, T, B, N, kind, seed, end_sets, first_row):
    arrays = _step_inputs(T, B, seed, kind, gpu)
    tensors = _tensors(arrays, gpu)
    for ends in end_sets:
        case = StepCase(f"{kind} T={T} ends={ends}", *arrays, _key(T + B), 0, N, ends)
        if kind == "flat" and (ends is None or max(ends) >= first_row):
            share, count = case.far_chunk_share(first_row)              # from the reference's picks alone
            print(f"{case.name}: {count} picks on rows >= {first_row}, {100 * share:.3g} % beyond the first chunk, "
                  f"{case.chunks_hit(first_row)} distinct chunks")
            assert count > 0 and share > 0.5, (share, count)
        _run_case(case, tensors)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "randn"])
def test_steps_chunk_switch_gpu(gpu, kind):
    """Rows 2047 (2048 candidates: 128 chunks of one batch, every summary slot used) and 2048, 2049 (chunks of two batches: the
    rescale between the batches of a chunk, the rescan of a two-batch chunk) in one launch.  Forced ends put a walk's first
    step on each of the three rows; the flat rows send the picks into every part of the row."""
    T = 2050
    try:
        end_sets = (None, [T - 1, 2048, 2047, 0, 1, 1033])
        if kind == "flat":                                                  # a flat walk is ~10 steps: eighteen more first steps per row
            end_sets += ([2049] * 6, [2048] * 6, [2047] * 6)
        _long_case(gpu, T, 6, 3, kind, 97, end_sets, 2048)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_steps_three_batches_gpu(gpu):
    """Chunks of three batches (48 candidates) from row 4096 on."""
    T = 4100
    try:
        _long_case(gpu, T, 3, 2, "flat", 98, (None, [T - 1, 4096, 4095], [0, 1, 2048], [4098, 4097, 4096], [4095] * 3), 4096)
    finally:
        torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", ["restated", "device"])
def test_steps_model_shape_gpu(gpu, alpha):
    """The model's row length on three chain tiles: the sampler alone on the restated alpha, and end to end on the alpha of the
    device's own forward sweep, read back and handed to the checker."""
    T, B, N = 691, 130, 2
    st, nt = synth.crf_inputs(T, B, 99, gpu, "model")
    s, n = st.cpu(), nt.cpu()
    if alpha == "device":
        _lib.device_status()
        _, vt = crf_mod._logz_fwd_raw(st, nt, True)
        v = vt.cpu().numpy()
        assert _lib.device_status() == 0
    else:
        v = _alpha64(s.numpy(), n.numpy()).astype(np.float32)
        vt = torch.from_numpy(v).to(gpu)
    _run_case(StepCase(f"model shape, {alpha} alpha", s.numpy(), n.numpy(), v, _key(691), 0, N), (st, nt, vt))
