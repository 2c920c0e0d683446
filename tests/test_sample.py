"""Posterior sampling of interval paths (NeuralSemiCRFInterval.sample / sample_packed, semicrf_sample).

The draws are a pure function of (inputs, key), so every test here is deterministic: a fixed generator seed makes the key.
CPU tests check the distribution itself (exact enumeration for tiny T, marginals against forward_backward, a float64
restatement of the contract); GPU tests check the device against the same properties and against the host kernel."""
import importlib
import math
import types

import numpy as np
import pytest
import torch

from conftest import edge_inputs
from transkun_amd import CRF, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")     # the module (the package exports the class by that name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _key(seed):
    return int(torch.randint(0, 2 ** 63 - 1, (1,), generator=_gen(seed)))


def _segments(pairs, offsets):
    return [[tuple(int(x) for x in p) for p in pairs[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]


def _mixed_inputs(T, seeds=(3, 4, 5)):
    """Three chains with different constructions (randn, model, ties)."""
    parts = [synth.crf_inputs(T, 1, s, "cpu", kind) for s, kind in zip(seeds, ("randn", "model", "ties"))]
    return (torch.cat([p[0] for p in parts], 2).contiguous(), torch.cat([p[1] for p in parts], 1).contiguous())


def _check_valid(pairs, offsets, T, ends=None, B=None):
    """Every segment is a path a walk can produce: 0 <= b <= e < T (e <= forced end), strictly ascending (begin, end), intervals
    that at most touch, and no singleton strictly inside an interval."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int64)
    K = int(offsets[-1])
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and pairs.shape[0] == K
    if K == 0:
        return
    b, e = pairs[:, 0], pairs[:, 1]
    seg = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    assert (b >= 0).all() and (b <= e).all() and (e < T).all()
    if ends is not None:
        lim = np.asarray(ends, np.int64)[seg % B]
        assert (e <= lim).all()
    same = seg[1:] == seg[:-1]
    asc = (b[1:] > b[:-1]) | ((b[1:] == b[:-1]) & (e[1:] > e[:-1]))
    assert asc[same].all(), "not strictly ascending within a path"
    # the last interval (b < e) before each entry, in the same path: its end must not pass the entry's begin
    idx = np.where(b < e, np.arange(K), -1)
    last = np.maximum.accumulate(idx)
    prev = np.concatenate([[-1], last[:-1]])
    ok = prev >= 0
    ok &= seg[np.maximum(prev, 0)] == seg
    assert (e[prev[ok]] <= b[ok]).all(), "overlapping intervals or a singleton inside an interval"


# ---- float64 restatement of the contract ---------------------------------------------------------------------------------

def _u(idx, key):
    return (synth.hash_u64_numpy(np.asarray(idx, np.uint64), key) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def _alpha64(s, n):
    T, B = s.shape[0], s.shape[2]
    v = np.zeros((T, B))
    sp = lambda x: np.logaddexp(0.0, x)
    v[0] = sp(s[0, 0])
    for t in range(1, T):
        cand = np.concatenate([(v[t - 1] + n[t - 1])[None], v[:t] + s[t, :t]], 0)
        v[t] = np.logaddexp.reduce(cand, 0) + sp(s[t, t])
    return v


def _restated_sample(s, n, v, nSample, key, ends=None):
    """List of nSample*B paths (sample-major) from the contract: float64, sequential running sums, first sum > u*Z."""
    T, B = s.shape[0], s.shape[2]
    s = s.astype(np.float64); n = n.astype(np.float64)
    out = []
    cums = {}
    for k in range(nSample):
        for c in range(B):
            t = T - 1 if ends is None else int(ends[c])
            rev = []
            while True:
                base = ((k * B + c) * T + t) * 2
                u = _u([base, base + 1], key)
                if u[1] < 1.0 / (1.0 + math.exp(-s[t, t, c])):
                    rev.append((t, t))
                if t == 0:
                    break
                if (t, c) not in cums:
                    x = np.concatenate([[v[t - 1, c] + n[t - 1, c]], v[t - 1::-1, c] + s[t, t - 1::-1, c]])
                    m = x.max()
                    cums[(t, c)] = np.cumsum(np.exp(x - m)) if m > -np.inf else np.zeros_like(x)
                cs = cums[(t, c)]
                Z = cs[-1]
                pick = 0
                if Z > 0:
                    thr = u[0] * Z
                    pick = int(np.searchsorted(cs, thr, side="right")) if thr < Z else int(np.searchsorted(cs, Z, side="left"))
                if pick == 0:
                    t -= 1
                else:
                    rev.append((t - pick, t))
                    t -= pick
            out.append(sorted(rev))
    return out


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
