"""evalPath / logProb, forward and backward, on hard target paths and cotangents -- the TARGET side of the headline path
(path_score_wave, the sweep's path_role, eval_path_kernel, the gradient sweep's noiseAdd, eval_path_bwd_pairs / _noise_kernel,
the hub's deposit_path, interval_score_path_bwd), which the rest of the suite only sees through synth.synthetic_intervals and
through inputs whose sums are exact in fp32.

Inputs, families, cotangents and float64 expectations: tests/path_targets_common.py.  Every expected value is computed at test
time from numpy float64 (the path side) and the C oracle in float64 (logZ, marginals).

Shapes and the launch configuration each one reaches (persist.hip: launch_persist_sweep_impl; K = ceil(T / 16) row blocks, panel
tasks exist when K > FAR0 = 4, i.e. T > 64; one launch hosts at most #CU / 2 = 128 spines of 4 chains; two far waves forward when
T >= 1024 and the launch has <= 192 chains):
  (1, 3)       T < 2: not a persistent launch at all -- the row-sequential sweep + eval_path_kernel + eval_path_bwd_noise/_pairs
  (2, 3)       persistent, K = 1: no panel workgroups, the path wave is a spare wave of the SPINE workgroups (pathSpine); 1 chunk
  (24, 1)      one chain: the ghost-chain route (sweep on 2 chains, eval_path_kernel and the eval_path_bwd kernels on their own)
  (33, 7)      K = 3, (64, 32) K = 4: still no panel tasks -- path wave on the spine workgroups; 2 and 8 rings; 1 chunk; 1 far wave
  (200, 33)    K = 13: panel workgroups host the path wave; two panel groups, the second with ONE chain; 1 chunk; 1 far wave
  (333, 46)    K = 21: panels, ragged second panel group (14 chains, B % 4 == 2); 1 chunk; 1 far wave
  (691, 90)    the model's segment: panels, band waves in the gradient sweep; 1 chunk; 1 far wave
  (691, 360)   4 x 90 chains: 90 spines, panels; 1 chunk; 1 far wave
  (130, 600)   150 spines > 128: TWO chunks (320 + 280 chains), the path queue (CTRL_PATHQ) runs per chunk; panels; 1 far wave
  (144, 704)   176 spines: TWO chunks of 352 chains; panels; 1 far wave
  (1024, 88)   panels; 1 chunk; TWO far waves in the forward sweep (T >= 1024, 88 <= 192 chains)
  (1100, 190)  panels, T % 16 != 0, B % 4 == 2; 1 chunk; TWO far waves
  (1024, 352)  the headline size: five panel waves per workgroup, 1 chunk, ONE far wave (352 > 192 chains)
With impl 1 every shape runs the row-sequential kernels + eval_path_kernel (small shapes only).  No shape had to be replaced.

Routes (each family x cotangent x shape): (a) crf.logProb; (b) crf.evalPath - crf.computeLogZ through the hub (deposit_path);
(c) the module-level evalPath - computeLogZ (dense zeros + scatter); (d) forward values under no_grad and noBackward=True;
(e) _logprob_fwd_raw against _eval_path_raw - logZ, bit for bit; (f) fused.scorer_crf_logprob on a slot layout with ghost slots.

Bounds (none tuned to the code under test):
  evalPath   |got - path64| <= 2**-23 |path64| + 2**-40 sum|terms|         (double accumulation, one rounding)
  logProb    |got - lp64| <= LOGZ_TOL max(|lz64|, |path64|, 1)
  gradients  per chain |got - want| <= (grad_tol(lz64) + 2**-22) |w_c|;  w_c == 0: every cell finite and == 0
  structure  upper triangle of dScore exactly 0, outputs finite, device status 0, the gap identity within 3 grad_tol.
"""
import importlib
import os

import numpy as np
import pytest
import torch

import path_targets_common as ptc
from conftest import rel_err  # noqa: F401
from test_gpu_parity import LOGZ_TOL, _gap_coverage, grad_tol

# (T, B, kinds, impls on the GPU, on the CPU too)
SHAPES = [
    (1, 3, ("randn", "model", "cancel"), (1, 0), True),
    (2, 3, ("randn", "model", "cancel"), (1, 0), True),
    (24, 1, ("randn", "model", "cancel"), (1, 0), True),
    (33, 7, ("randn", "model", "cancel"), (1, 0), True),
    (64, 32, ("randn", "model", "cancel"), (1, 0), True),
    (200, 33, ("randn", "model", "cancel"), (1, 0), True),
    (257, 12, ("randn", "cancel"), (), True),                     # (CPU twin only: the largest T the twins run)
    (333, 46, ("randn", "model", "cancel"), (1, 0), False),
    (691, 90, ("model", "cancel"), (0,), False),
    (691, 360, ("randn",), (0,), False),
    (130, 600, ("randn", "model"), (0,), False),
    (144, 704, ("model",), (0,), False),
    (1024, 88, ("randn",), (0,), False),
    (1100, 190, ("model",), (0,), False),
    (1024, 352, ("randn",), (0,), False),
]
F64_SHAPES = {(33, 7), (200, 33)}                                   # where the float64 inputs / cotangent run (the _gout conversion)


def _gpu_params():
    out = []
    for T, B, kinds, impls, _ in SHAPES:
        for kind in kinds:
            for im in impls:
                for fam in ptc.FAMILIES:
                    out.append(pytest.param(T, B, kind, im, fam, id=f"T{T}_B{B}-{kind}-impl{im}-{fam}"))
    return out


def _cpu_params():
    out = []
    for T, B, kinds, _, on_cpu in SHAPES:
        if on_cpu:
            for kind in kinds:
                for fam in ptc.FAMILIES:
                    out.append(pytest.param(T, B, kind, fam, id=f"T{T}_B{B}-{kind}-{fam}"))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# one (shape, kind) at a time: inputs, the float64 oracle and the inputs' device copies are made once, not once per family
# ------------------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def _setup(oracle, T, B, kind, dev):
    key = (T, B, kind, str(dev))
    if key not in _CACHE:
        _CACHE.clear()
        nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
        nsci.grad_pool_clear()
        if dev.type == "cuda":
            torch.cuda.empty_cache()
        score, noise = ptc.make_inputs(T, B, 40 + T % 17, kind, base_device=dev)
        _CACHE[key] = dict(score=score, noise=noise, O=ptc.Oracle64(oracle, score, noise, dev), sd=score.to(dev), nd=noise.to(dev))
    return _CACHE[key]


def _status(dev):
    if dev.type == "cuda":
        from transkun_amd import _lib
        return _lib.device_status()
    return 0


def _routes():
    from transkun_amd import CRF
    return {
        "a": lambda s, n, iv: CRF.NeuralSemiCRFInterval(s, n).logProb(iv),
        "b": lambda s, n, iv: (lambda c: c.evalPath(iv) - c.computeLogZ())(CRF.NeuralSemiCRFInterval(s, n)),
        "c": lambda s, n, iv: CRF.evalPath(iv, s, n) - CRF.computeLogZ(s, n),
    }


def _check_forward(tag, got, E, O, what):
    """got [B] tensor; what: "lp" (sampled chains, needs logZ) or "path" (every chain)."""
    g = got.detach().double().cpu().numpy()
    assert np.isfinite(g).all(), tag
    if what == "path":
        err, bound = np.abs(g - E["path64"]), ptc.eval_path_bound(E["path64"], E["terms"])
    else:
        p = E["path64"][O.idx]
        err = np.abs(g[O.idx] - (p - O.lz64))
        bound = LOGZ_TOL * np.maximum(np.maximum(np.abs(O.lz64), np.abs(p)), 1.0)
    r = np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0)          # (an empty path at T == 1: 0 within a bound of 0)
    print(f"{tag} {what}: {float(r.max()):.3f} of the bound")
    assert (err <= bound).all(), (tag, what, float(r.max()), int(np.argmax(r)))


def _check_grads(tag, O, iv, w, dS, dN, gap_identity):
    T, B, dev = O.T, O.B, O.dev
    w = np.asarray(w, np.float64)
    assert dS.shape == (T, T, B) and dN.shape == (max(T - 1, 0), B), tag
    assert bool(torch.isfinite(dS).all()) and bool(torch.isfinite(dN).all()), tag
    if T > 1:
        assert float(torch.triu(dS.permute(2, 0, 1), diagonal=1).abs().max()) == 0.0, f"{tag}: upper triangle of dScore not 0"
    zero = np.nonzero(w == 0.0)[0]
    if len(zero):
        z = torch.from_numpy(zero).to(dev)
        assert bool((dS.index_select(2, z) == 0).all()), f"{tag}: dScore of a chain with weight 0 is not 0"
        assert bool((dN.index_select(1, z) == 0).all()), f"{tag}: dNoise of a chain with weight 0 is not 0"
    wantS, wantN = O.want_grads(iv, w)
    gt = grad_tol(O.lz64)
    tol = torch.from_numpy((gt + 2.0 ** -22) * np.abs(w[O.idx])).to(dev)
    errS = (dS.index_select(2, O.ix).double() - wantS).abs().amax(dim=(0, 1))
    errN = (dN.index_select(1, O.ix).double() - wantN).abs().amax(dim=0) if T > 1 else torch.zeros_like(errS)
    nz = tol > 0
    rS = float((errS[nz] / tol[nz]).max()) if bool(nz.any()) else 0.0
    rN = float((errN[nz] / tol[nz]).max()) if bool(nz.any()) else 0.0
    print(f"{tag}: dScore {rS:.3f}, dNoise {rN:.3f} of the bound (grad_tol {gt:.2e})")
    assert bool((errS <= tol).all()), (tag, "dScore", rS, int((errS / tol.clamp_min(1e-300)).argmax()))
    assert bool((errN <= tol).all()), (tag, "dNoise", rN, int((errN / tol.clamp_min(1e-300)).argmax()))
    if gap_identity and T > 1:
        # dNoise[t] + sum_{b<=t<e} dScore[e,b] == w (1 - cover(t)) - w + w [t covered by a path interval]  (== 0 for a path)
        cov = _gap_coverage(dS, dN)                                             # [sampled gaps, B]
        idx = list(range(0, T - 1, max(1, (T - 1) // 16)))
        cover = ptc.cover_counts(iv, T, B)[idx]
        want = torch.from_numpy(w[None, :] * (1.0 - cover) - w[None, :] + w[None, :] * (cover > 0)).to(dev)
        dev_ = float((cov - want).abs().max())
        print(f"{tag}: gap identity {dev_ / (3 * gt):.3f} of the bound")
        assert dev_ <= 3 * gt, (tag, "gap identity", dev_)


def _targets_case(dev, oracle, T, B, kind, fam):
    """Routes (a) - (d) of one family on one (shape, kind), every cotangent."""
    C = _setup(oracle, T, B, kind, dev)
    O, sd, nd = C["O"], C["sd"], C["nd"]
    iv = ptc.family(fam, T, B, seed=T + B)
    p64, terms = ptc.path_reference(C["score"], C["noise"], iv)
    E = dict(path64=p64, terms=terms)
    from transkun_amd import CRF
    _status(dev)
    wc = ptc.chain_weights(B, seed=T)
    cots = [("scalar", np.full(B, ptc.SCALAR_W)), ("chain", wc)]
    if B == 1:
        cots.append(("chain0", np.zeros(1)))                      # (one chain cannot hold both -1000 and 0)
    if (T, B) in F64_SHAPES:
        cots.append(("f64", wc))
    for rname, route in _routes().items():
        for cname, w in cots:
            tag = f"{fam}/{rname}/{cname}"
            dt = torch.float64 if cname == "f64" else torch.float32
            s = sd.to(dt).clone().requires_grad_()
            n = nd.to(dt).clone().requires_grad_()
            lp = route(s, n, iv)
            assert lp.dtype == dt and lp.shape == (B,), tag
            _check_forward(tag, lp, E, O, "lp")
            if cname == "scalar":
                (lp.sum() * ptc.SCALAR_W).backward()               # autograd hands down an expanded scalar: the stride-0 route
            else:
                (lp * torch.from_numpy(w).to(dev).to(dt)).sum().backward()
            assert s.grad.dtype == dt and n.grad.dtype == dt, tag
            _check_grads(tag, O, iv, w, s.grad, n.grad, gap_identity=(cname == "scalar" and rname == "a" and fam in ptc.IN_CONTRACT))
            assert _status(dev) == 0, tag
            del s, n, lp
    # evalPath's own value, on the object and at module level, and (d): no_grad / noBackward
    crf = CRF.NeuralSemiCRFInterval(sd.clone().requires_grad_(), nd.clone().requires_grad_())
    _check_forward(fam + "/crf.evalPath", crf.evalPath(iv), E, O, "path")
    _check_forward(fam + "/evalPath", CRF.evalPath(iv, sd, nd), E, O, "path")
    with torch.no_grad():
        for tag, val, what in (("no_grad logProb", crf.logProb(iv), "lp"), ("no_grad noBackward", crf.logProb(iv, noBackward=True), "lp"),
                               ("no_grad evalPath", crf.evalPath(iv), "path"),
                               ("no_grad two nodes", crf.evalPath(iv) - crf.computeLogZ(noBackward=True), "lp")):
            assert not val.requires_grad, tag
            _check_forward(f"{fam}/{tag}", val, E, O, what)
    lp_nb = crf.logProb(iv, noBackward=True)                        # (the reference's flag: same value with grad mode on)
    _check_forward(fam + "/noBackward", lp_nb, E, O, "lp")
    assert _status(dev) == 0


@pytest.fixture
def impl_of(gpu):
    """The `impl` fixture pattern of test_gpu_parity.py, with the value taken from the case's parameters."""
    from transkun_amd import _lib

    def use(i):
        _lib.set_impl(i)
    yield use
    _lib.set_impl(0)


# ------------------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("T,B,kind,im,fam", _gpu_params())
def test_targets_gpu(gpu, oracle, impl_of, T, B, kind, im, fam):
    """Routes (a) - (e) on the device.  Host kernels measured 0.30 - 0.45 of the evalPath bound and <= 0.39 of the gradient bound."""
    impl_of(im)
    _targets_case(gpu, oracle, T, B, kind, fam)
    # (e) raw: the one-launch logProb against evalPath - logZ, bit for bit -- also the symptom ADVICE r6 names for a wrong wave
    # budget around path_role / far_role ("logProb is never written")
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    from transkun_amd import _lib
    C = _CACHE[(T, B, kind, str(gpu))]
    iv = ptc.family(fam, T, B, seed=T + B)
    pairs, offsets = nsci.pack_intervals(iv, T, B, gpu)
    ep = nsci._eval_path_raw(C["sd"], C["nd"], pairs, offsets)
    for want_v in (True, False):
        lp, logz, v = nsci._logprob_fwd_raw(C["sd"], C["nd"], pairs, offsets, want_v)
        assert (v is not None) == want_v
        assert bool(torch.isfinite(lp).all()) and torch.equal(lp, ep - logz), f"{fam}: raw logProb != evalPath - logZ (want_v={want_v})"
    assert _lib.device_status() == 0


FUSED_SHAPES = [(2, 90, 130, 64), (1, 90, 200, 128)]               # P = 90 at pitch 96: six ghost slots per segment


@pytest.mark.gpu
@pytest.mark.parametrize("proj", ["merged", "separate"])
@pytest.mark.parametrize("fam", ptc.FAMILIES)
@pytest.mark.parametrize("N,P,T,D", FUSED_SHAPES)
def test_targets_fused_gpu(gpu, N, P, T, D, fam, proj):
    """(f) scorer_crf_logprob on a slot layout WITH ghost slots, the families as targets, against route (a) on the same scorer:
    test_fused_scorer_crf's comparison and tolerances (offsets gathered through the slot map, interval_score_path_bwd)."""
    from transkun_amd import CRF, _lib, synth
    from transkun_amd.fused import scorer_crf_logprob
    from transkun_amd.scorer import ScaledInnerProductIntervalScorer, slot_pitch
    _lib.set_impl(0)
    assert slot_pitch(P, T, D, N) > P
    torch.manual_seed(1234)
    m = ScaledInnerProductIntervalScorer(D, 1, lengthScaling="linear").to(gpu)
    with torch.no_grad():
        m.map[0].weight.mul_(0.3)
    ctx0 = synth.hash_normal(N * P * T * D, 61, gpu).view(N, P, T, D) * 0.5
    iv = ptc.family(fam, T, N * P, seed=T + P)
    gout = synth.hash_normal(N * P, 62, gpu)
    gout[3] = 0.0

    def run(fused):
        m.zero_grad()
        ctx = ctx0.clone().requires_grad_()
        if fused:
            lp = scorer_crf_logprob(m, ctx, iv, projection=proj)
        else:
            S, b = m(ctx)
            lp = CRF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1)).logProb(iv)
        (lp * gout).sum().backward()
        return lp.detach(), ctx.grad.clone(), m.map[0].weight.grad.clone(), m.map[0].bias.grad.clone()

    monkey = os.environ.get("SEMICRF_POISON_UNWRITTEN")
    os.environ["SEMICRF_POISON_UNWRITTEN"] = "1"                    # a read of a cell the scorer does not write would show as NaN
    try:
        a = run(True)
    finally:
        if monkey is None:
            os.environ.pop("SEMICRF_POISON_UNWRITTEN", None)
    b = run(False)
    for x, y, name in zip(a, b, ("logp", "dctx", "dW", "dbias")):
        assert bool(torch.isfinite(x).all()), name
        err = float((x - y).abs().max()) / (float(y.abs().max()) + 1e-30)
        print(f"{fam}/{proj} {name}: {err:.2e}")
        assert err < (1e-3 if (name == "dbias" and proj == "merged") else 2e-4), (name, err)
    assert _lib.device_status() == 0


POOL_FAMILIES = ("all_singletons", "empty_all", "full_span", "long_mixed", "touching_chain", "overlap_dup", "ragged_counts", "boundary")


def _pool_sequence(dev, oracle, T, B):
    """logProb backward again and again at one shape whose gradient is pooled (>= 16 MB): the families cycle, the scalar and the
    per-chain cotangents alternate, one two-node pass (evalPath - computeLogZ through the hub) in between.  Every result is
    checked against its OWN reference: the path cells of the previous family and the previous cotangent must not survive in the
    pooled buffer, whose upper triangle is written once."""
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    C = _setup(oracle, T, B, "randn", dev)
    O, sd, nd = C["O"], C["sd"], C["nd"]
    routes = _routes()
    nsci.grad_pool_clear()
    pool = nsci._GRAD_POOL
    h0 = pool.hits
    wc = ptc.chain_weights(B, seed=5)
    for step, fam in enumerate(POOL_FAMILIES + POOL_FAMILIES[:3]):
        iv = ptc.family(fam, T, B, seed=step)
        w = np.full(B, ptc.SCALAR_W) if step % 2 == 0 else np.roll(wc, step)
        rname = "b" if step in (4, 7) else "a"
        s = sd.clone().requires_grad_(); n = nd.clone().requires_grad_()
        lp = routes[rname](s, n, iv)
        if step % 2 == 0:
            (lp.sum() * ptc.SCALAR_W).backward()
        else:
            (lp * torch.from_numpy(w).to(dev).float()).sum().backward()
        _check_grads(f"step {step} {fam}/{rname}", O, iv, w, s.grad, n.grad, gap_identity=False)
        del s, n, lp
    if pool.enabled:
        assert pool.hits - h0 >= 4, (pool.hits - h0, "the sequence did not run on pooled buffers")
    assert _status(dev) == 0
    nsci.grad_pool_clear()


@pytest.mark.gpu
def test_pooled_buffer_sequence_gpu(gpu, oracle):
    from transkun_amd import _lib
    _lib.set_impl(0)
    _pool_sequence(gpu, oracle, 256, 96)                            # 25 MB, a panel shape (K = 16)


# ------------------------------------------------------------------------------------------------------------------------------
# begin > end: one decision for both devices -- ValueError naming the interval, before anything is launched
# ------------------------------------------------------------------------------------------------------------------------------

def _reversed_interval_case(dev, oracle):
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    from transkun_amd import CRF
    T, B = 256, 96                                                  # pooled gradients
    C = _setup(oracle, T, B, "randn", dev)
    O, sd, nd = C["O"], C["sd"], C["nd"]
    good = ptc.family("long_mixed", T, B, seed=1)
    nsci.grad_pool_clear()

    def backward(iv):
        s = sd.clone().requires_grad_(); n = nd.clone().requires_grad_()
        (CRF.NeuralSemiCRFInterval(s, n).logProb(iv).sum() * ptc.SCALAR_W).backward()
        return s.grad, n.grad

    for _ in range(2):                                              # the second gradient comes from the pool
        ds, dn = backward(good)
        del ds, dn
    bad = [list(x) for x in good]
    bad[B - 2] = bad[B - 2] + [(7, 3)]
    s = sd.clone().requires_grad_(); n = nd.clone().requires_grad_()
    crf = CRF.NeuralSemiCRFInterval(s, n)
    for call in (lambda: crf.logProb(bad), lambda: crf.evalPath(bad), lambda: CRF.evalPath(bad, s, n), lambda: crf.logProb(bad, noBackward=True)):
        with pytest.raises(ValueError, match=rf"\(7, 3\) of chain {B - 2}"):
            call()
    with pytest.raises(ValueError, match=r"\(1, 0\) of chain 0"):
        CRF.NeuralSemiCRFInterval(sd, nd).evalPath([[(1, 0)]] + [[] for _ in range(B - 1)])
    # interval_marginals keeps accepting begin > end and returns 0 for it (include/semicrf_hip.h, tests/test_posteriors.py)
    mu = CRF.NeuralSemiCRFInterval(sd, nd).interval_marginals([[(7, 3), (3, 7)]] + [[] for _ in range(B - 1)])
    assert mu[0][0] == 0.0 and mu[0][1] > 0.0
    # out of range stays an IndexError
    with pytest.raises(IndexError):
        crf.logProb([[(0, T)]] + [[] for _ in range(B - 1)])
    # and the pool is intact: the next gradient is correct and its upper triangle exactly 0
    ds, dn = backward(good)
    _check_grads("after the error", O, good, np.full(B, ptc.SCALAR_W), ds, dn, gap_identity=True)
    assert _status(dev) == 0
    nsci.grad_pool_clear()


@pytest.mark.gpu
def test_reversed_interval_is_an_error_gpu(gpu, oracle):
    from transkun_amd import _lib, synth
    from transkun_amd.fused import scorer_crf_logprob
    from transkun_amd.scorer import ScaledInnerProductIntervalScorer
    _lib.set_impl(0)
    _reversed_interval_case(gpu, oracle)
    m = ScaledInnerProductIntervalScorer(64, 1).to(gpu)
    ctx = synth.hash_normal(2 * 5 * 130 * 64, 3, gpu).view(2, 5, 130, 64)
    with pytest.raises(ValueError, match=r"\(9, 2\) of chain 4"):
        scorer_crf_logprob(m, ctx, [[], [], [], [], [(0, 1), (9, 2)], [], [], [], [], []])
    assert _lib.device_status() == 0


# ------------------------------------------------------------------------------------------------------------------------------
# CPU twins (no GPU needed): the same families, cotangents and routes (a) - (d) on the host kernels -- they validate the
# reference and the bounds
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,B,kind,fam", _cpu_params())
def test_targets_cpu(oracle, T, B, kind, fam):
    _targets_case(torch.device("cpu"), oracle, T, B, kind, fam)


def test_pooled_buffer_sequence_cpu(oracle):
    _pool_sequence(torch.device("cpu"), oracle, 256, 96)


def test_reversed_interval_is_an_error_cpu(oracle):
    _reversed_interval_case(torch.device("cpu"), oracle)
