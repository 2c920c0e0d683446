"""Posterior marginals and path entropy (NeuralSemiCRFInterval.posteriors / interval_marginals[_packed], semicrf_posteriors,
semicrf_interval_marginals).

CPU tests check the host kernel against exact enumeration, the float64 dense marginals of the C oracle, the structural
identities and the existing ops; GPU tests check the device kernels against the host kernel and a float64 torch restatement,
determinism, memory, sampling and graph capture."""
import importlib
import math

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

FIELDS = ("node", "begin", "end", "single", "noise")


def _mixed_inputs(T, seeds=(3, 4, 5)):
    """Three chains with different constructions (randn, model, ties), as tests/test_sample.py builds them."""
    parts = [synth.crf_inputs(T, 1, s, "cpu", kind) for s, kind in zip(seeds, ("randn", "model", "ties"))]
    return (torch.cat([p[0] for p in parts], 2).contiguous(), torch.cat([p[1] for p in parts], 1).contiguous())


def _grad_tol(logz):
    return max(1e-4, 2e-6 * float(np.max(np.abs(np.asarray(logz, np.float64)))))


def _np(P):
    return {k: getattr(P, k).cpu().double().numpy() for k in ("logZ", "entropy") + FIELDS}


# ---- exact enumeration ---------------------------------------------------------------------------------------------------

def _paths(T):
    """Every path as a list of (b, e) (singletons (t, t) included), walking nodes from frame 0."""
    out = []

    def walk(t, acc):
        for single in (False, True):
            cur = acc + ([(t, t)] if single else [])
            if t == T - 1:
                out.append(cur)
                continue
            walk(t + 1, cur)                                 # the gap t .. t+1 is noise
            for e in range(t + 1, T):
                walk(e, cur + [(t, e)])
    walk(0, [])
    return out


def _enumerate(s, n):
    """float64 truth of every output and of the marginal of every (b, e), by summing over all paths."""
    s = s.double().numpy(); n = n.double().numpy()
    T, B = s.shape[0], s.shape[2]
    paths = _paths(T)
    res = []
    for c in range(B):
        sc = []
        for p in paths:
            covered = np.zeros(max(T - 1, 0), bool)
            x = 0.0
            for b, e in p:
                x += s[e, b, c]
                covered[b:e] = True
            x += n[~covered, c].sum() if T > 1 else 0.0
            sc.append(x)
        sc = np.array(sc)
        lz = np.logaddexp.reduce(sc)
        pr = np.exp(sc - lz)
        r = {k: np.zeros(T) for k in ("node", "begin", "end", "single")}
        r["noise"] = np.zeros(max(T - 1, 0))
        r["marg"] = np.zeros((T, T))
        for p, w in zip(paths, pr):
            inside = np.zeros(T, bool)
            covered = np.zeros(max(T - 1, 0), bool)
            for b, e in p:
                r["marg"][e, b] += w
                if b == e:
                    r["single"][b] += w
                else:
                    r["begin"][b] += w; r["end"][e] += w
                    inside[b + 1:e] = True
                    covered[b:e] = True
            r["node"][~inside] += w
            r["noise"][~covered] += w
        r["entropy"] = float(-(pr * np.log(np.where(pr > 0, pr, 1.0))).sum())
        r["logZ"] = lz
        res.append(r)
    return res


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_exact_enumeration_cpu(T):
    s, n = _mixed_inputs(T)
    B = s.shape[2]
    P = _np(CRF.posteriors(s, n))
    truth = _enumerate(s, n)
    for c in range(B):
        r = truth[c]
        assert abs(P["logZ"][c] - r["logZ"]) < 1e-5 * max(1.0, abs(r["logZ"]))
        assert abs(P["entropy"][c] - r["entropy"]) < 1e-5 * max(1.0, r["entropy"])
        for k in FIELDS:
            np.testing.assert_allclose(P[k][:, c], r[k], rtol=0, atol=1e-5, err_msg=f"{k} chain {c}")
    # the marginal of every possible (b, e), b <= e
    iv = [[(b, e) for e in range(T) for b in range(e + 1)] for _ in range(B)]
    got = CRF.interval_marginals(s, n, iv)
    for c in range(B):
        want = [truth[c]["marg"][e, b] for b, e in iv[c]]
        np.testing.assert_allclose(got[c], want, rtol=0, atol=1e-5)


# ---- edge cases against the oracle's float64 dense marginals ------------------------------------------------------------

def _dense_reference(oracle, s, n):
    """float64 outputs reduced from the oracle's dense marginals; entropy as logZ - E[score]."""
    lz, grad, gn, _, _ = oracle.forward_backward_f64(s.numpy(), n.numpy())
    T = grad.shape[0]
    tril = np.tril(np.ones((T, T), bool), -1)[:, :, None]
    off = np.where(tril, grad, 0.0)
    r = {"logZ": lz, "noise": gn,
         "single": np.stack([grad[t, t] for t in range(T)]),
         "end": off.sum(1), "begin": off.sum(0)}
    node = np.empty_like(r["end"])
    node[0] = 1.0
    if T > 1:
        node[1:] = gn + r["end"][1:]
    r["node"] = node
    sd = s.double().numpy(); nd = n.double().numpy()
    low = np.tril(np.ones((T, T), bool))[:, :, None]
    escore = np.where(low, grad * np.where(low, sd, 0.0), 0.0).sum((0, 1)) + (gn * nd).sum(0)
    r["entropy"] = lz - escore
    return r


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_edge_cases_cpu(oracle, case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    P = _np(CRF.posteriors(s, n))
    r = _dense_reference(oracle, s, n)
    tol = _grad_tol(r["logZ"])
    for k in FIELDS:
        np.testing.assert_allclose(P[k], r[k], rtol=0, atol=tol, err_msg=f"{name}: {k}")
    assert np.all(np.isfinite(P["entropy"])) and np.all(P["entropy"] >= 0.0), name
    if tr == "huge":
        return          # logZ - E[score] cancels ~1e5-sized numbers: the reference itself is noise at this scale
    np.testing.assert_allclose(P["entropy"], r["entropy"], rtol=1e-4, atol=T * tol, err_msg=name)


# ---- identities ------------------------------------------------------------------------------------------------------------

def _check_identities(P, tol):
    node, begin, end, single, noise = (P[k] for k in FIELDS)
    T = node.shape[0]
    for k in FIELDS:
        assert np.all(P[k] >= 0.0) and np.all(P[k] <= 1.0), k
    assert np.all(P["entropy"] >= 0.0)
    assert np.abs(node[0] - 1.0).max() < tol and np.abs(node[T - 1] - 1.0).max() < tol
    if T > 1:
        assert np.abs(node[1:] - (noise + end[1:])).max() < tol
        assert np.abs(node[:-1] - (noise + begin[:-1])).max() < tol
        assert np.abs(np.cumsum(begin - end, 0)[:-1] - (1.0 - noise)).max() < tol * T


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_identities_cpu(case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    P = _np(CRF.posteriors(s, n))
    _check_identities(P, 2 * _grad_tol(P["logZ"]))


# ---- consistency with the existing ops -----------------------------------------------------------------------------------

def _consistency(device):
    T, B = 40, 6
    s, n = synth.crf_inputs(T, B, 31, device, "model")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    dec = crf.decode()
    got = crf.interval_marginals(dec)
    _, grad, _ = CRF.forward_backward(s, n)
    g = grad.cpu().double().numpy()
    tol = _grad_tol(crf.posteriors().logZ.cpu().numpy())
    for c in range(B):
        assert len(got[c]) == len(dec[c])
        for (b, e), m in zip(dec[c], got[c]):
            assert abs(m - g[e, b, c]) <= tol, (c, b, e, m, g[e, b, c])
    pairs, offsets = crf.decode_packed()
    packed = crf.interval_marginals_packed(pairs, offsets)
    assert packed.dtype == torch.float32 and packed.device == s.device
    assert packed.cpu().tolist() == [m for lst in got for m in lst]
    # device tensors are taken as they are
    packed_t = crf.interval_marginals_packed(torch.from_numpy(pairs).to(s.device), torch.from_numpy(offsets).to(s.device))
    assert torch.equal(packed_t, packed)
    # b > e is never on a path
    assert crf.interval_marginals([[(5, 3)]] + [[] for _ in range(B - 1)])[0] == [0.0]


def test_consistency_cpu():
    _consistency("cpu")


# ---- argument handling ---------------------------------------------------------------------------------------------------

def _arguments(device):
    T, B = 12, 3
    s, n = synth.crf_inputs(T, B, 41, device, "randn")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    with pytest.raises(IndexError):
        crf.interval_marginals([[(0, T)], [], []])
    with pytest.raises(IndexError):
        crf.interval_marginals([[(-1, 2)], [], []])
    with pytest.raises(AssertionError):
        crf.interval_marginals([[(0, 1)], []])
    with pytest.raises(IndexError):
        crf.interval_marginals_packed(np.array([[0, T]], np.int32), np.array([0, 1, 1, 1], np.int32))
    with pytest.raises(ValueError):
        crf.interval_marginals_packed(np.array([[0, 1]], np.int32), np.array([0, 2, 1, 1], np.int32))
    with pytest.raises(AssertionError):
        CRF.posteriors(s[:, :-1], n)
    with pytest.raises(AssertionError):
        CRF.posteriors(s, n[:-1])
    # no gradient flows, whatever the inputs require
    sg, ng = s.clone().requires_grad_(), n.clone().requires_grad_()
    P = CRF.posteriors(sg, ng)
    for x in P:
        assert not x.requires_grad and x.dtype == torch.float32 and x.device == s.device
    assert not CRF.interval_marginals_packed(sg, ng, *crf.decode_packed()).requires_grad
    # other float dtypes are computed as .float()
    want = CRF.posteriors(s, n)
    for dt in (torch.bfloat16, torch.float16):
        sd, nd = s.to(dt), n.to(dt)
        got = CRF.posteriors(sd, nd)
        ref = CRF.posteriors(sd.float(), nd.float())
        for a, b in zip(got, ref):
            assert a.dtype == torch.float32
            assert torch.equal(a, b)
    # T = 1
    P1 = CRF.posteriors(s[:1, :1].contiguous(), n[:0])
    assert P1.noise.shape == (0, B) and P1.node.shape == (1, B)
    assert torch.allclose(P1.node, torch.ones_like(P1.node), atol=1e-6)
    # the module-level names and the class agree
    assert all(torch.equal(a, b) for a, b in zip(crf.posteriors(), want))


def test_arguments_cpu():
    _arguments("cpu")


# ---- GPU ---------------------------------------------------------------------------------------------------------------

def _compare(Pd, Ph, what, scale=1.0):
    tol = 4 * _grad_tol(Ph["logZ"]) * scale
    T = Ph["node"].shape[0]
    for k in FIELDS:
        np.testing.assert_allclose(Pd[k], Ph[k], rtol=0, atol=tol, err_msg=f"{what}: {k}")
    np.testing.assert_allclose(Pd["entropy"], Ph["entropy"], rtol=1e-4, atol=T * tol, err_msg=f"{what}: entropy")


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_device_matches_host_edge_gpu(gpu, case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    Ph = _np(CRF.posteriors(s, n))
    Pd = _np(CRF.posteriors(s.to(gpu), n.to(gpu)))
    _compare(Pd, Ph, name)
    _check_identities(Pd, 4 * _grad_tol(Pd["logZ"]))


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind", [(256, 90, "model"), (64, 1, "randn"), (200, 1, "model"), (64, 3, "ties"),
                                      (70, 1100, "randn")])
def test_device_matches_host_gpu(gpu, T, B, kind):
    s, n = synth.crf_inputs(T, B, 7 + T + B, "cpu", kind)
    Ph = _np(CRF.posteriors(s, n))
    Pd = _np(CRF.posteriors(s.to(gpu), n.to(gpu)))
    _compare(Pd, Ph, f"{T}x{B}")
    crf = CRF.NeuralSemiCRFInterval(s.to(gpu), n.to(gpu))
    pairs, offsets = crf.decode_packed()
    md = crf.interval_marginals_packed(pairs, offsets).cpu().double().numpy()
    mh = CRF.interval_marginals_packed(s, n, pairs, offsets).double().numpy()
    np.testing.assert_allclose(md, mh, rtol=0, atol=4 * _grad_tol(Ph["logZ"]))


def _torch_f64(s, n, P, rows=64):
    """float64 restatement from the library's own v / q, chunked over rows (no dense [T, T, B] tensor)."""
    T, B = s.shape[0], s.shape[2]
    lz, v, q = crf_mod._marginal_inputs(s, n)
    v, q, lz = v.double(), q.double(), lz.double()
    sp = torch.nn.functional.softplus
    diag = torch.diagonal(s, dim1=0, dim2=1).t().double()           # [T, B]
    R = v - sp(diag)
    A = q - lz
    end = torch.zeros(T, B, dtype=torch.float64, device=s.device)
    begin = torch.zeros_like(end)
    H = torch.zeros(B, dtype=torch.float64, device=s.device)
    for e0 in range(0, T, rows):
        e1 = min(T, e0 + rows)
        S = s[e0:e1].double()                                          # [r, T, B]
        y = v[None] + S
        mu = torch.exp(y + A[e0:e1, None])
        mask = (torch.arange(T, device=s.device)[None, :] < torch.arange(e0, e1, device=s.device)[:, None])[:, :, None]
        mu = torch.where(mask, mu, torch.zeros((), dtype=torch.float64, device=s.device))
        end[e0:e1] = mu.sum(1)
        begin += mu.sum(0)
        H += torch.where(mu > 0, mu * torch.clamp(R[e0:e1, None] - y, min=0), torch.zeros_like(mu)).sum((0, 1))
    node = torch.exp(R + A)
    a = diag.abs()
    Hb = torch.log1p(torch.exp(-a)) + a * torch.exp(-a) / (1 + torch.exp(-a))
    H += (node * Hb).sum(0)
    if T > 1:
        ys = v[:-1] + n.double()
        mus = torch.exp(ys + A[1:])
        H += (mus * torch.clamp(R[1:] - ys, min=0)).sum(0)
    noise = torch.exp(v[:-1] + n.double() + q[1:] - lz)
    single = torch.exp(v + q - lz + diag - 2 * sp(diag))
    return {"logZ": lz.cpu().numpy(), "entropy": H.cpu().numpy(), "node": node.cpu().numpy(), "begin": begin.cpu().numpy(),
            "end": end.cpu().numpy(), "single": single.cpu().numpy(), "noise": noise.cpu().numpy()}


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind", [(1024, 352, "randn"), (691, 360, "model"), (2048, 88, "randn")])
def test_full_size_gpu(gpu, T, B, kind):
    s, n = synth.crf_inputs(T, B, 11, gpu, kind)
    P1 = CRF.posteriors(s, n)
    P2 = CRF.posteriors(s, n)
    for a, b in zip(P1, P2):
        assert torch.equal(a, b)                                     # deterministic: bit-identical
    P = _np(P1)
    ref = _torch_f64(s, n, P1)
    tol = 4 * _grad_tol(ref["logZ"])
    for k in FIELDS:
        np.testing.assert_allclose(P[k], ref[k], rtol=0, atol=tol, err_msg=k)
    np.testing.assert_allclose(P["entropy"], ref["entropy"], rtol=1e-4, atol=T * tol)
    _check_identities(P, 4 * tol)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_memory_gpu(gpu):
    T, B = 1024, 352
    s, n = synth.crf_inputs(T, B, 12, gpu, "randn")
    CRF.posteriors(s, n)                      # leased sweep workspaces are set up once
    torch.cuda.synchronize(gpu)
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    P = CRF.posteriors(s, n)
    torch.cuda.synchronize(gpu)
    peak = torch.cuda.max_memory_allocated(gpu) - base
    assert peak <= 128 * 2 ** 20, peak / 2 ** 20
    del P


@pytest.mark.gpu
def test_agrees_with_sampling_gpu(gpu):
    T, B, N = 64, 16, 4096
    s, n = synth.crf_inputs(T, B, 13, gpu, "model")
    P = _np(CRF.posteriors(s, n))
    pairs, offsets = CRF.sample_packed(s, n, N, generator=torch.Generator().manual_seed(5))
    pairs = pairs.astype(np.int64)
    c = np.repeat(np.arange(N * B), np.diff(offsets)) % B
    freq = {k: np.zeros((T, B)) for k in ("begin", "end", "single")}
    iv = pairs[:, 0] < pairs[:, 1]
    np.add.at(freq["begin"], (pairs[iv, 0], c[iv]), 1.0)
    np.add.at(freq["end"], (pairs[iv, 1], c[iv]), 1.0)
    np.add.at(freq["single"], (pairs[~iv, 0], c[~iv]), 1.0)
    for k, f in freq.items():
        p = P[k]
        se = np.sqrt(np.clip(p * (1 - p), 0, None) / N)
        assert np.all(np.abs(f / N - p) <= 5 * se + 1.0 / N), k


@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    T, B = 333, 46
    data = [synth.crf_inputs(T, B, 600 + i, gpu) for i in range(3)]
    dec = CRF.NeuralSemiCRFInterval(*data[0]).decode_packed()
    pairs = torch.from_numpy(dec[0]).to(gpu)
    offsets = torch.from_numpy(dec[1]).to(gpu)
    K = int(dec[1][-1])

    def chain(s, n):
        lz, v, q = crf_mod._marginal_inputs(s, n)
        P = crf_mod._posteriors_raw(s, n, (lz, v, q))
        m = crf_mod._interval_marginals_raw(s, v, q, lz, pairs, K, offsets)
        return list(P) + [m]

    want = [[x.clone() for x in chain(s, n)] for s, n in data]
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
        for a, b in zip(got, want[i]):
            assert torch.equal(a, b), i
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_consistency_gpu(gpu):
    _consistency(gpu)


@pytest.mark.gpu
def test_arguments_gpu(gpu):
    _arguments(gpu)
