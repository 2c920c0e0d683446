"""Posterior expectations, the differentiable entropy and Hessian products of logZ (NeuralSemiCRFInterval.expectation / entropy /
covariance, semicrf_expectation / semicrf_covariance).

For W(path) = sum of weight[e,b] over the path's intervals + sum of noiseWeight[t] over its noise gaps:
    E = E_p[W],  C[e,b] = Cov(1[(b,e) on path], W),  Cn[t] = Cov(1[gap t is noise], W),  H = logZ - E_p[S].

The truth is float64: exact enumeration for tiny T, tests/golden/expect_*.npz (tools/make_expectation_golden.py: the reference's own
computeLogZ differentiated twice in float64) and, at full size on the device, a float64 torch restatement of that double backward.

Error metric, per chain c, over C and Cn together, the worst chain counting:
    err = max|X - X64| / max(max|X64[..., c]|, 1e-3 max|w[..., c]|)         bound: err <= 1e-5, host and device kernels alike
(the second term keeps near-deterministic chains, where every covariance is ~0, from dividing by nothing).  The bound is three
orders below what fp32 per-frame state reaches (1e-2 at T = 200, 6e-2 at T = 400; the fixtures' err_ref_fp32 records the reference's
own fp32 double backward), so it also checks that the state is carried in float64.
E and H: |X - X64| <= 1e-5 max(1, |X64|, 1e-2 T max|w|).
"""
import importlib

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs, load_golden
from test_posteriors import _grad_tol, _mixed_inputs, _paths
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

BOUND = 1e-5

# name, T, B, kind, seed   (must match tools/make_expectation_golden.py LARGE_CASES)
LARGE_CASES = [
    ("T256_B90_model", 256, 90, "model", 131),
    ("T256_B90_randn", 256, 90, "randn", 132),
    ("T1024_B88_randn", 1024, 88, "randn", 133),
]


def weights(T, B, seed):
    """The seeded random weighting of a fixture (tools/make_expectation_golden.py: weights)."""
    w, wn = synth.crf_inputs(T, B, seed + 7919, "cpu", "randn")
    return w.contiguous(), wn.contiguous()


def _f64(x):
    return x.detach().cpu().double().numpy()


def _wmax(w, wn):
    """max|w| per chain over the cells that are read (begin <= end) and the gaps."""
    T = w.shape[0]
    low = np.tril(np.ones((T, T), bool))[:, :, None]
    m = np.abs(np.where(low, w, 0.0)).max((0, 1))
    return np.maximum(m, np.abs(wn).max(0)) if wn.size else m


def _metric(C, Cn, C64, Cn64, wmax):
    """The error metric of the module docstring for dense arrays [T, T, B] / [T-1, B]; returns (worst, per chain)."""
    num, den = np.abs(C - C64).max((0, 1)), np.abs(C64).max((0, 1))
    if Cn64.size:
        num, den = np.maximum(num, np.abs(Cn - Cn64).max(0)), np.maximum(den, np.abs(Cn64).max(0))
    err = num / np.maximum(den, 1e-3 * wmax)
    return float(err.max()), err


def _check_scalar(X, X64, T, wmax, what):
    tol = BOUND * np.maximum(np.maximum(1.0, np.abs(X64)), 1e-2 * T * wmax)
    d = np.abs(X - X64)
    print(f"{what}: max |X - X64| / tol = {float((d / tol).max()):.3g}")
    assert np.all(d <= tol), (what, float((d / tol).max()))


def _check_cov(C, Cn, C64, Cn64, wmax, what):
    err, _ = _metric(C, Cn, C64, Cn64, wmax)
    print(f"{what}: err = {err:.3g}")
    assert err <= BOUND, (what, err)
    return err


# ---- exact enumeration ---------------------------------------------------------------------------------------------------

def _enumerate(s, n, w, wn):
    """float64 (E, H, C, Cn) by summing over all paths."""
    s, n, w, wn = (x.double().numpy() for x in (s, n, w, wn))
    T, B = s.shape[0], s.shape[2]
    paths = _paths(T)
    E, H = np.zeros(B), np.zeros(B)
    C, Cn = np.zeros((T, T, B)), np.zeros((max(T - 1, 0), B))
    for c in range(B):
        S, W, gaps = [], [], []
        for p in paths:
            covered = np.zeros(max(T - 1, 0), bool)
            for b, e in p:
                covered[b:e] = True
            S.append(sum(s[e, b, c] for b, e in p) + n[~covered, c].sum())
            W.append(sum(w[e, b, c] for b, e in p) + wn[~covered, c].sum())
            gaps.append(~covered)
        S, W = np.array(S), np.array(W)
        lz = np.logaddexp.reduce(S)
        pr = np.exp(S - lz)
        E[c] = (pr * W).sum()
        H[c] = -(pr * np.log(np.where(pr > 0, pr, 1.0))).sum()
        for p, g, pw, Wp in zip(paths, gaps, pr, W):
            for b, e in p:
                C[e, b, c] += pw * (Wp - E[c])
            Cn[g, c] += pw * (Wp - E[c])
    return E, H, C, Cn


@pytest.mark.parametrize("T", [1, 2, 3, 5, 7])
def test_exact_enumeration_cpu(T):
    s, n = _mixed_inputs(T)
    B = s.shape[2]
    wr, wnr = weights(T, B, 900 + T)
    for tag, w, wn in (("s", s, n), ("r", wr, wnr)):
        E64, H64, C64, Cn64 = _enumerate(s, n, w, wn)
        E, C, Cn = CRF.covariance(s, n, w, wn)
        wmax = _wmax(w.numpy(), wn.numpy())
        _check_cov(_f64(C), _f64(Cn), C64, Cn64, wmax, f"T={T} {tag}")
        _check_scalar(_f64(E), E64, T, wmax, f"T={T} {tag} E")
        _check_scalar(_f64(CRF.expectation(s, n, w, wn)), E64, T, wmax, f"T={T} {tag} expectation")
        if tag == "s":
            _check_scalar(_f64(CRF.entropy(s, n)), H64, T, wmax, f"T={T} H")


# ---- fixtures ------------------------------------------------------------------------------------------------------------

def _edge_fixture(case, device):
    name, T, B, kind, seed, tr = case
    G = load_golden("expect_" + name)
    s, n = edge_inputs(T, B, kind, seed, tr)
    wr, wnr = weights(T, B, seed)
    ee, bb = np.tril_indices(T)
    worst = 0.0
    for tag, w, wn in (("s", s, n), ("r", wr, wnr)):
        C64 = np.zeros((T, T, B))
        C64[ee, bb] = G["Ctril_" + tag]
        sd, nd, wd, wnd = (x.to(device) for x in (s, n, w, wn))
        E, C, Cn = CRF.covariance(sd, nd, wd, wnd)
        wmax = _wmax(w.numpy(), wn.numpy())
        worst = max(worst, _check_cov(_f64(C), _f64(Cn), C64, G["Cn_" + tag], wmax, f"{name} {tag}"))
        assert float(torch.triu(C.permute(2, 0, 1), 1).abs().max()) == 0.0
        _check_scalar(_f64(E), G["E_" + tag], T, wmax, f"{name} {tag} E")
        if tag == "s":
            _check_scalar(_f64(CRF.entropy(sd, nd)), G["H"], T, wmax, f"{name} H")
    return worst


def _large_fixture(case, device, full):
    """full: run every chain and compare the fixture's subset; else run the subset alone (chains are independent)."""
    name, T, B, kind, seed = case
    G = load_golden("expect_" + name)
    ch = G["chains"]
    s, n = synth.crf_inputs(T, B, seed, "cpu", kind)
    wr, wnr = weights(T, B, seed)
    ce, cb, ck = G["cell_e"], G["cell_b"], G["cell_k"]
    worst = 0.0
    for tag, w, wn in (("s", s, n), ("r", wr, wnr)):
        if full:
            sd, nd, wd, wnd = (x.to(device) for x in (s, n, w, wn))
        else:
            sd, nd, wd, wnd = (x[..., ch].contiguous().to(device) for x in (s, n, w, wn))
        E, C, Cn = CRF.covariance(sd, nd, wd, wnd)
        if full:
            sel = torch.from_numpy(ch).to(device)
            E, C, Cn = E[sel], C[:, :, sel], Cn[:, sel]
        C, Cn, E = _f64(C), _f64(Cn), _f64(E)
        wmax = _wmax(w.numpy()[..., ch], wn.numpy()[..., ch])
        cmax = np.maximum(np.maximum(G["cmax_" + tag], np.abs(G["Cn_" + tag]).max(0)), 1e-3 * wmax)       # the metric's denominator
        err = max(float((np.abs(C[ce, cb, ck] - G["cells_" + tag]) / cmax[ck]).max()),
                  float((np.abs(Cn - G["Cn_" + tag]) / cmax).max()))
        print(f"{name} {tag}: err = {err:.3g}")
        assert err <= BOUND, (name, tag, err)
        worst = max(worst, err)
        # every element is within BOUND * cmax, so a sum of k elements is within k * BOUND * cmax: row e has e + 1, column b T - b
        k = np.arange(1, T + 1)[:, None]
        assert np.all(np.abs(C.sum(1) - G["rowsum_" + tag]) <= BOUND * cmax * k), (name, tag, "row sums")
        assert np.all(np.abs(C.sum(0) - G["colsum_" + tag]) <= BOUND * cmax * k[::-1]), (name, tag, "column sums")
        assert float(np.abs(np.triu(C.transpose(2, 0, 1), 1)).max()) == 0.0
        _check_scalar(E, G["E_" + tag], T, wmax, f"{name} {tag} E")
        if tag == "s":
            H = _f64(CRF.entropy(sd, nd))
            _check_scalar(H[ch] if full else H, G["H"], T, wmax, f"{name} H")
    return worst


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_fixture_edge_cpu(case):
    _edge_fixture(case, "cpu")


@pytest.mark.parametrize("case", LARGE_CASES, ids=[c[0] for c in LARGE_CASES])
def test_fixture_large_cpu(case):
    _large_fixture(case, "cpu", full=False)


# ---- invariants ------------------------------------------------------------------------------------------------------------

def _constant_functional(s, n):
    """weight[e,b] = e - b, noiseWeight = 1: W = T - 1 on every path, so E = T - 1 and every covariance is 0."""
    T, B = s.shape[0], s.shape[2]
    t = torch.arange(T, dtype=torch.float32, device=s.device)
    w = (t[:, None] - t[None, :])[:, :, None].expand(T, T, B).contiguous()
    wn = torch.ones(T - 1, B, dtype=torch.float32, device=s.device)
    E, C, Cn = CRF.covariance(s, n, w, wn)
    wmax = float(max(T - 1, 1))
    _check_scalar(_f64(E), np.full(B, T - 1.0), T, wmax, "constant functional E")
    zc, zn = float(C.abs().max()), float(Cn.abs().max())
    print(f"constant functional: max|C| = {zc:.3g}, max|Cn| = {zn:.3g}")
    assert zc <= BOUND * wmax and zn <= BOUND * wmax
    del C


@pytest.mark.parametrize("T,B,kind", [(40, 6, "model"), (200, 4, "randn"), (64, 3, "ties")])
def test_constant_functional_cpu(T, B, kind):
    _constant_functional(*synth.crf_inputs(T, B, 51, "cpu", kind))


def _single_cell_indicator(device):
    T, B = 40, 6
    s, n = synth.crf_inputs(T, B, 31, device, "model")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    tol = _grad_tol(crf.posteriors().logZ.cpu().numpy())
    for b, e in ((3, 17), (9, 9), (0, T - 1), (T - 1, T - 1)):
        w = torch.zeros_like(s)
        w[e, b] = 1.0
        E = crf.expectation(w).cpu().numpy()
        want = np.array([m[0] for m in crf.interval_marginals([[(b, e)]] * B)])
        assert np.abs(E - want).max() <= tol, (b, e)


def test_single_cell_indicator_cpu():
    _single_cell_indicator("cpu")


@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_entropy_value_cpu(case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    P = CRF.posteriors(s, n)
    tol = _grad_tol(P.logZ.numpy())
    np.testing.assert_allclose(_f64(CRF.entropy(s, n)), _f64(P.entropy), rtol=1e-4, atol=T * tol, err_msg=name)


# ---- autograd contract ---------------------------------------------------------------------------------------------------

def _autograd_contract(device):
    T, B = 24, 5
    s, n = synth.crf_inputs(T, B, 61, device, "model")
    w, wn = (x.to(device) for x in weights(T, B, 61))
    g = torch.linspace(-1.5, 2.0, B, device=device)
    E0, C, Cn = CRF.covariance(s, n, w, wn)
    # a per-chain grad_output scales per chain; the gradients to weight / noiseWeight are gout * marginals
    sg, ng, wg, wng = (x.clone().requires_grad_() for x in (s, n, w, wn))
    E = CRF.expectation(sg, ng, wg, wng)
    assert E.dtype == torch.float32 and E.shape == (B,) and E.grad_fn is not None
    assert torch.equal(E.detach(), E0)
    E.backward(g)
    torch.testing.assert_close(sg.grad, C * g, rtol=1e-6, atol=1e-30)
    torch.testing.assert_close(ng.grad, Cn * g, rtol=1e-6, atol=1e-30)
    lz, marg, marg_n = CRF.forward_backward(s, n)
    tol = _grad_tol(lz.cpu().numpy()) * float(g.abs().max())
    assert float((wg.grad - marg * g).abs().max()) <= tol and float((wng.grad - marg_n * g).abs().max()) <= tol
    for d in (sg.grad, wg.grad):                                   # begin > end: exact zeros in every dense gradient
        assert float(torch.triu(d.permute(2, 0, 1), 1).abs().max()) == 0.0
    # noiseWeight defaults to zeros; only the inputs that ask get a gradient
    sg2 = s.clone().requires_grad_()
    E2 = CRF.expectation(sg2, n, w)
    assert torch.equal(E2.detach(), CRF.expectation(s, n, w, torch.zeros_like(n)))
    E2.sum().backward()
    torch.testing.assert_close(sg2.grad, CRF.covariance(s, n, w)[1], rtol=1e-6, atol=1e-30)
    # the entropy's gradient is -C with the weights = the scores
    sg3, ng3 = s.clone().requires_grad_(), n.clone().requires_grad_()
    crf = CRF.NeuralSemiCRFInterval(sg3, ng3)
    H = crf.entropy()
    H.backward(g)
    _, Cs, Cns = crf.covariance(s, n)
    torch.testing.assert_close(sg3.grad, -Cs * g, rtol=1e-6, atol=1e-30)
    torch.testing.assert_close(ng3.grad, -Cns * g, rtol=1e-6, atol=1e-30)
    assert float(torch.triu(sg3.grad.permute(2, 0, 1), 1).abs().max()) == 0.0
    # the no-grad paths return plain tensors
    for x in (CRF.expectation(s, n, w, wn), CRF.entropy(s, n)) + tuple(CRF.covariance(sg, ng, wg, wng)):
        assert x.grad_fn is None and not x.requires_grad and x.dtype == torch.float32 and x.device == s.device
    with torch.no_grad():
        assert CRF.entropy(sg, ng).grad_fn is None
    # a second differentiation raises instead of returning something silently wrong
    sg4 = s.clone().requires_grad_()
    (g1,) = torch.autograd.grad(CRF.entropy(sg4, n).sum(), sg4, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(g1.sum(), sg4)
    # other float dtypes are computed as .float(); gradients come back in the input's dtype
    for dt in (torch.bfloat16, torch.float16):
        sd, nd, wd = s.to(dt), n.to(dt), w.to(dt)
        assert torch.equal(CRF.expectation(sd, nd, wd), CRF.expectation(sd.float(), nd.float(), wd.float()))
        assert torch.equal(CRF.entropy(sd, nd), CRF.entropy(sd.float(), nd.float()))
        for a, b in zip(CRF.covariance(sd, nd, wd), CRF.covariance(sd.float(), nd.float(), wd.float())):
            assert a.dtype == torch.float32 and torch.equal(a, b)
        sdg = sd.clone().requires_grad_()
        CRF.entropy(sdg, nd).sum().backward()
        assert sdg.grad.dtype == dt
    # T = 1: one frame, the singleton alone
    s1, n1 = s[:1, :1].contiguous(), n[:0]
    E1, C1, Cn1 = CRF.covariance(s1, n1, w[:1, :1].contiguous())
    p = torch.sigmoid(s1[0, 0].double())
    w1 = w[0, 0].double()
    assert Cn1.shape == (0, B) and C1.shape == (1, 1, B)
    torch.testing.assert_close(E1.double(), p * w1, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(C1[0, 0].double(), p * (1 - p) * w1, rtol=1e-5, atol=1e-7)
    Hb = -(p * torch.log(p) + (1 - p) * torch.log1p(-p))
    torch.testing.assert_close(CRF.entropy(s1, n1).double(), Hb, rtol=1e-6, atol=1e-7)
    # shape errors as posteriors raises them
    with pytest.raises(AssertionError):
        CRF.entropy(s[:, :-1], n)
    with pytest.raises(AssertionError):
        CRF.entropy(s, n[:-1])
    with pytest.raises(AssertionError):
        CRF.expectation(s, n, w[:-1])
    with pytest.raises(AssertionError):
        CRF.covariance(s, n, w, wn[:-1])
    # the module-level names and the class agree
    assert torch.equal(CRF.NeuralSemiCRFInterval(s, n).expectation(w, wn), E0)


def test_autograd_contract_cpu():
    _autograd_contract("cpu")


# ---- GPU ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_fixture_edge_gpu(gpu, case):
    _edge_fixture(case, gpu)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", LARGE_CASES, ids=[c[0] for c in LARGE_CASES])
def test_fixture_large_gpu(gpu, case):
    _large_fixture(case, gpu, full=True)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind", [(256, 90, "model"), (64, 1, "randn"), (200, 1, "model"), (64, 3, "ties"),
                                      (70, 1100, "randn")])
def test_device_matches_host_gpu(gpu, T, B, kind):
    """Two results each within 1e-5 of the truth: 2e-5 between them."""
    s, n = synth.crf_inputs(T, B, 7 + T + B, "cpu", kind)
    wr, wnr = weights(T, B, 7 + T + B)
    for tag, w, wn in (("s", s, n), ("r", wr, wnr)):
        Eh, Ch, Cnh = CRF.covariance(s, n, w, wn)
        Ed, Cd, Cnd = CRF.covariance(*(x.to(gpu) for x in (s, n, w, wn)))
        wmax = _wmax(w.numpy(), wn.numpy())
        err, _ = _metric(_f64(Cd), _f64(Cnd), _f64(Ch), _f64(Cnh), wmax)
        print(f"{T}x{B} {kind} {tag}: device against host err = {err:.3g}")
        assert err <= 2 * BOUND, (tag, err)
        tol = 2 * BOUND * np.maximum(np.maximum(1.0, np.abs(_f64(Eh))), 1e-2 * T * wmax)
        assert np.all(np.abs(_f64(Ed) - _f64(Eh)) <= tol)
    Hh, Hd = _f64(CRF.entropy(s, n)), _f64(CRF.entropy(s.to(gpu), n.to(gpu)))
    wmax = _wmax(s.numpy(), n.numpy())
    assert np.all(np.abs(Hd - Hh) <= 2 * BOUND * np.maximum(np.maximum(1.0, np.abs(Hh)), 1e-2 * T * wmax))
    assert _lib.device_status() == 0


def _torch_f64(s, n, w, wn):
    """float64 torch restatement of the reference's computeLogZ (rows as separate leaves, so that no slice's gradient is a dense
    tensor), differentiated twice: (logZ, E, C [T,T,B], Cn [T-1,B])."""
    sp = torch.nn.functional.softplus
    T = s.shape[0]
    rows = [s[i, :i + 1].clone().requires_grad_() for i in range(T)]
    nz = n.clone().requires_grad_()
    v = [sp(rows[0][0])]
    for i in range(1, T):
        tmp = torch.cat([(v[i - 1] + nz[i - 1])[None], torch.stack(v) + rows[i][:i]], 0)
        v.append(tmp.logsumexp(0) + sp(rows[i][i]))
    lz = v[-1]
    g = torch.autograd.grad(lz.sum(), rows + [nz], create_graph=True)
    E = sum((g[i] * w[i, :i + 1]).sum(0) for i in range(T)) + (g[T] * wn).sum(0)
    h = torch.autograd.grad(E.sum(), rows + [nz])
    C = torch.zeros_like(s)
    for i in range(T):
        C[i, :i + 1] = h[i]
    return lz.detach(), E.detach(), C, h[T]


def test_torch_restatement_matches_fixture_cpu():
    """The restatement the full-size GPU test relies on reproduces a fixture of the reference."""
    name, T, B, kind, seed, tr = EDGE_CASES[11]
    G = load_golden("expect_" + name)
    s, n = edge_inputs(T, B, kind, seed, tr)
    lz, E, C, Cn = _torch_f64(s.double(), n.double(), s.double(), n.double())
    ee, bb = np.tril_indices(T)
    np.testing.assert_allclose(C.numpy()[ee, bb], G["Ctril_s"], rtol=1e-9, atol=1e-9 * np.abs(G["Ctril_s"]).max())
    np.testing.assert_allclose(E.numpy(), G["E_s"], rtol=1e-11)
    np.testing.assert_allclose((lz - E).numpy(), G["H"], rtol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind", [(1024, 352, "randn"), (691, 360, "model"), (2048, 88, "randn")])
def test_full_size_gpu(gpu, T, B, kind):
    s, n = synth.crf_inputs(T, B, 11, gpu, kind)
    wmax = np.maximum(_f64(s.abs().amax((0, 1))), _f64(n.abs().amax(0)))
    E1, C1, Cn1 = CRF.covariance(s, n, s, n)
    H1 = CRF.entropy(s, n)
    E2, C2, Cn2 = CRF.covariance(s, n, s, n)
    assert torch.equal(E1, E2) and torch.equal(C1, C2) and torch.equal(Cn1, Cn2) and torch.equal(H1, CRF.entropy(s, n))
    del C2, Cn2
    ch = torch.from_numpy(np.sort(np.random.RandomState(T + B).permutation(B)[:8])).to(gpu)
    lz, E64, C64, Cn64 = _torch_f64(s[:, :, ch].double(), n[:, ch].double(), s[:, :, ch].double(), n[:, ch].double())
    chn = ch.cpu().numpy()
    _check_cov(_f64(C1[:, :, ch]), _f64(Cn1[:, ch]), _f64(C64), _f64(Cn64), wmax[chn], f"{T}x{B} {kind}")
    _check_scalar(_f64(E1[ch]), _f64(E64), T, wmax[chn], "E")
    _check_scalar(_f64(H1[ch]), _f64(lz - E64), T, wmax[chn], "H")
    assert float(torch.triu(C1[:, :, ch].permute(2, 0, 1), 1).abs().max()) == 0.0
    del C1, C64
    _constant_functional(s, n)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_memory_gpu(gpu):
    T, B = 1024, 352
    s, n = synth.crf_inputs(T, B, 12, gpu, "randn")
    w = s * 0.5
    MiB = 2 ** 20
    with torch.no_grad():
        CRF.expectation(s, n, w)                  # leased sweep workspaces are set up once
        torch.cuda.synchronize(gpu)
        base = torch.cuda.memory_allocated(gpu)
        torch.cuda.reset_peak_memory_stats(gpu)
        E = CRF.expectation(s, n, w)
        torch.cuda.synchronize(gpu)
        peak = torch.cuda.max_memory_allocated(gpu) - base
        assert peak <= 128 * MiB, peak / MiB
    del w, E
    # entropy with backward: the dense gradient and nothing else of that size
    sg = s.requires_grad_()
    CRF.entropy(sg, n).sum().backward()
    sg.grad = None
    torch.cuda.synchronize(gpu)
    base = torch.cuda.memory_allocated(gpu)
    torch.cuda.reset_peak_memory_stats(gpu)
    CRF.entropy(sg, n).sum().backward()
    torch.cuda.synchronize(gpu)
    peak = torch.cuda.max_memory_allocated(gpu) - base
    dense = 4 * T * T * B
    assert dense <= peak <= dense + 128 * MiB, (peak / MiB, dense / MiB)


@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    T, B = 333, 46
    data = [synth.crf_inputs(T, B, 600 + i, gpu) for i in range(3)]
    ones = torch.ones(B, dtype=torch.float32, device=gpu)

    def chain(s, n):
        E, H, state = crf_mod._expect_fwd(s, n, s, n)
        C, Cn = crf_mod._expect_cov(state, ones)
        return [E, H, C, Cn]

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
def test_constant_functional_gpu(gpu):
    _constant_functional(*synth.crf_inputs(200, 33, 51, gpu, "randn"))


@pytest.mark.gpu
def test_single_cell_indicator_gpu(gpu):
    _single_cell_indicator(gpu)


@pytest.mark.gpu
def test_autograd_contract_gpu(gpu):
    _autograd_contract(gpu)
