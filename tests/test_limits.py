"""Long rows and the largest batches: the code paths beyond the sizes the model uses.

A. The trace of the MBR selector on synthetic packed lattices at the row lengths where decode.hip changes its backtrack kernel
   (BT_PAR_MAX = 8192: pointer doubling in LDS up to there; BT_LDS_MAX = 16384: the serial walk on a row staged in LDS up to there;
   the serial walk in global memory beyond), bit for bit against the numpy restatement (tests/mbr_common.py).  No [T, T, B] tensor.
B. Real rows of 4099, 8200 and 16400 frames, two chains each, against the C oracle: the sweeps at 257 .. 1025 row blocks and
   21 .. 85 far parts, and the serial backtrack in both walk directions behind a real Viterbi sweep.
C. The chain-chunk limit: sixteen chunks, a sixteenth chunk of one chain, an uneven ninth chunk, and one chain past the limit
   (the row-sequential kernels).

Rows of T >= 65535 frames (persist_supported's other bound: the row-sequential kernels for LONG rows) need a 34 GB score tensor
per two chains and are left out."""
import importlib

import numpy as np
import pytest
import torch

from conftest import rel_err
from mbr_common import LATTICE_CHAINS, _mbr_reference, lattice
from path_targets_common import cover_counts, path_reference
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

LOGZ_TOL = 1e-5                                               # tests/test_gpu_parity.py


def grad_tol(logz):
    return max(1e-4, 2e-6 * float(np.max(np.abs(logz))))


# ---- A. backtrack switch points on synthetic lattices ----------------------------------------------------------------------

# both sides of MBR_LDS_T (4096: F in LDS up to there), of BT_PAR_MAX and of BT_LDS_MAX, and an odd long row
SWITCH_T = [4095, 4096, 4097, 8191, 8192, 8193, 16384, 16385, 20011]
SWITCH_T_CPU = [4097, 8193, 16385]
TAU_ALL = 0.3
TAU_PER_CHAIN = (0.3, 0.25, 0.35, 0.2)

_LATTICES = {}


def _lattice_case(T):
    """(lattice, {tau name: (tau tensor, restatement's result)}), computed once per length"""
    if T not in _LATTICES:
        lat = lattice(T, T)
        B = len(lat[2]) - 1
        assert B == len(LATTICE_CHAINS) == len(TAU_PER_CHAIN)
        want = {}
        for name, tau in (("all", torch.full((1,), TAU_ALL)), ("per_chain", torch.tensor(TAU_PER_CHAIN))):
            arr = np.full(B, tau.item(), np.float32) if tau.numel() == 1 else tau.numpy()
            want[name] = (tau, _mbr_reference(lat[0], lat[2], lat[1], T, arr))
        _LATTICES[T] = (lat, want)
    return _LATTICES[T]


def _check_lattice(T, pairs, weight, offsets):
    """the generator's contract: ascending by (begin, end) per chain, in range, weights in (0, 1]"""
    assert pairs.dtype == np.int32 and weight.dtype == np.float32 and offsets.dtype == np.int32
    assert pairs.shape == (len(weight), 2) and offsets[0] == 0 and offsets[-1] == len(weight)
    assert weight.min() > 0.0 and weight.max() <= 1.0
    assert pairs.min() >= 0 and pairs.max() < T and np.all(pairs[:, 0] <= pairs[:, 1])
    for c in range(len(offsets) - 1):
        p = pairs[offsets[c]:offsets[c + 1]].astype(np.int64)
        assert np.all(np.diff(p[:, 0] * T + p[:, 1]) > 0), c


def _select_and_compare(T, device):
    (pairs, weight, offsets), want = _lattice_case(T)
    dp, dw, do = (torch.from_numpy(x).to(device) for x in (pairs, weight, offsets))
    for name, (tau, ref) in want.items():
        got_p, got_o, got_w, got_g = crf_mod._mbr_select_raw(dp, dw, do, T, tau.to(device))
        got_o = got_o.cpu().numpy()
        total = int(got_o[-1])
        what = f"T={T} tau={name}"
        assert np.array_equal(got_o, ref[1]), what
        assert np.array_equal(got_p[:total].cpu().numpy(), ref[0]), what
        assert np.array_equal(got_w[:total].cpu().numpy().view(np.int32), ref[2].view(np.int32)), what
        assert np.array_equal(got_g.cpu().numpy().view(np.int32), ref[3].view(np.int32)), what


@pytest.mark.parametrize("T", SWITCH_T_CPU)
def test_backtrack_switch_lattices_cpu(T):
    """The generator emits valid lattices that stress the walk, the restatement handles these lengths, and the host kernels agree
    with it bit for bit."""
    (pairs, weight, offsets), want = _lattice_case(T)
    _check_lattice(T, pairs, weight, offsets)
    ref = want["all"][1]
    count = dict(zip(LATTICE_CHAINS, np.diff(ref[1])))
    assert count["empty"] == 0 and offsets[1] == 0
    assert count["dense"] == 2 * T - 1                                   # the capacity of region and of pairs_out
    assert count["hashed"] >= T // 8 and count["last_frame"] >= T // 8    # a degenerate generator must not pass silently
    for c in (2, 3):
        sel = ref[0][ref[1][c]:ref[1][c + 1]]
        assert int((sel[:, 1] - sel[:, 0]).max()) >= T // 2 - 1           # the long jump is on the path
    last = ref[0][ref[1][3]:ref[1][4]]
    assert tuple(last[-1]) == (T - 1, T - 1) and tuple(last[0]) != (0, 0)
    _select_and_compare(T, "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("T", SWITCH_T)
def test_backtrack_switch_lattices_gpu(gpu, T):
    """semicrf_mbr_select on the device at both sides of BT_PAR_MAX and BT_LDS_MAX: offsets, pairs, probs and gain bit-identical
    to the restatement -- backtrack_par_kernel at its LDS limit (T = 8192: 128 KB dynamic + 1 KB static), the serial walk on a
    row in LDS and on a row in global memory (emission in walk order while walking, 2 T - 1 cells, no cell, a terminal singleton)."""
    _select_and_compare(T, gpu)
    assert _lib.device_status() == 0


# ---- B. real long rows, two chains each ------------------------------------------------------------------------------------

def _starts(T, B, forward):
    """None, the mixed starts of test_persist_vs_oracle, and the extremes of the walk direction"""
    assert B == 2
    return [None, [(c * 7 + 3) % T for c in range(B)], [T - 1, 0] if forward else [0, T - 1]]


def _check_decode(crf, oracle, sc, nc, T, B, variants=((0, 1, 2), (0, 1, 2))):
    """decode against oracle.viterbi; variants: the indices into _starts for the backward and for the forward walk"""
    out = {}
    for forward in (False, True):
        for k in variants[int(forward)]:
            st = _starts(T, B, forward)[k]
            got = crf.decode(forcedStartPos=st, forward=forward)
            assert got == oracle.viterbi(sc, nc, st, forward=forward), (T, forward, st)       # bit-exact lists
            out[(forward, k)] = got
    return out


def _gap_coverage(grad, gn):
    """For sampled gaps t: gradNoise[t] + sum_{b<=t<e} grad[e,b] == 1 (tests/test_gpu_parity.py)."""
    T = grad.shape[0]
    idx = list(range(0, T - 1, max(1, (T - 1) // 16)))
    return torch.stack([grad[t + 1:, :t + 1].double().sum(dim=(0, 1)) + gn[t].double() for t in idx])


def _long_row_dense(dev, oracle, T, kind):
    """forward_backward, computeLogZ and decode of a two-chain row against the oracle, the tolerance taken from the fp32 oracle"""
    B = 2
    score, noise = synth.crf_inputs(T, B, 100 + T, dev, kind)
    sc, nc = score.cpu().numpy(), noise.cpu().numpy()
    lz64, grad64, gn64, _, _ = oracle.forward_backward_f64(sc, nc)
    lz32, grad32, gn32, _, _ = oracle.forward_backward(sc, nc)
    ref_err = max(float(np.abs(grad32 - grad64).max()), 1e-4)
    ref_lz = max(rel_err(lz32, lz64), 1e-6)
    del grad32
    lz, grad, gn = CRF.forward_backward(score, noise)
    g64 = torch.from_numpy(grad64).to(dev)
    err_grad = float((grad.double() - g64).abs().max())
    del g64
    err_gn = float(np.abs(gn.cpu().numpy().astype(np.float64) - gn64).max())
    err_lz = rel_err(lz.cpu().numpy(), lz64)
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    err_lz2 = rel_err(crf.computeLogZ().cpu().numpy(), lz64)
    print(f"T={T} {kind}: logZ rel err {err_lz:.3g} / {err_lz2:.3g} (fp32 oracle {ref_lz:.3g}), marginals {err_grad:.3g}, "
          f"noise gradient {err_gn:.3g} (fp32 oracle {ref_err:.3g}; its noise gradient {float(np.abs(gn32 - gn64).max()):.3g})")
    assert err_lz <= 4 * ref_lz and err_lz2 <= 4 * ref_lz
    assert err_grad <= 1.5 * ref_err
    assert err_gn <= 1.5 * ref_err
    up = torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), diagonal=1)
    assert float(grad[up].abs().max()) == 0.0                             # begin > end: exact zeros
    del up
    cov = _gap_coverage(grad, gn)
    assert float((cov - 1.0).abs().max()) < 3 * grad_tol(lz64)
    del grad, gn
    _check_decode(crf, oracle, sc, nc, T, B)


def _long_row_logz_decode(dev, oracle, T):
    B = 2
    score, noise = synth.crf_inputs(T, B, 100 + T, dev, "randn")
    sc, nc = score.cpu().numpy(), noise.cpu().numpy()
    _, lz64 = oracle.alpha_f64(sc, nc)
    _, lz32 = oracle.alpha(sc, nc)
    ref_lz = max(rel_err(lz32, lz64), 1e-6)
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    err_lz = rel_err(crf.computeLogZ().cpu().numpy(), lz64)
    print(f"T={T} randn: logZ rel err {err_lz:.3g} (fp32 oracle {ref_lz:.3g})")
    assert err_lz <= 4 * ref_lz
    _check_decode(crf, oracle, sc, nc, T, B)


def _long_row_decode(dev, oracle, T):
    B = 2
    score, noise = synth.crf_inputs(T, B, 100 + T, dev, "randn")
    sc, nc = score.cpu().numpy(), noise.cpu().numpy()
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    # backward: the oracle without forced starts; forward: without, mixed and the extremes
    dec = _check_decode(crf, oracle, sc, nc, T, B, ((0,), (0, 1, 2)))
    # the backward extremes [0, T - 1] follow from the definition without another sweep of the oracle: a start at 0 is the default,
    # and from T - 1 the walk is empty -- only the terminal singleton is emitted, if its score is positive
    got = crf.decode(forcedStartPos=_starts(T, B, False)[2])
    assert got[0] == dec[(False, 0)][0]
    assert got[1] == ([(T - 1, T - 1)] if sc[T - 1, T - 1, 1] > 0 else [])
    dec[(False, 2)] = got
    logz = crf.computeLogZ()
    bound = logz + 1e-3 * logz.abs().clamp_min(1.0)
    for path in dec.values():
        assert bool((crf.evalPath(path) <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["randn", "model"])
def test_long_row_T4099_gpu(gpu, oracle, kind):
    """T = 4099 (257 row blocks, 21 far parts, 134 MB): forward_backward, computeLogZ and decode against the oracle.

    The tolerance is the fp32 oracle's own error against float64 on the same inputs (floored at 1e-4 for marginals, 1e-6 for logZ):
    at most 1.5 x for the marginals and the noise gradient, 4 x for relative logZ -- the margin of another, equally long summation
    order; a wrong far part or a dropped tile moves a marginal by 0.1 .. 1.  Measured figures: DESIGN.md section 4."""
    _lib.set_impl(0)
    _lib.device_status()
    _long_row_dense(gpu, oracle, 4099, kind)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_long_row_T8200_gpu(gpu, oracle):
    """T = 8200 (513 row blocks, 537 MB): the Viterbi sweeps end in the serial backtrack on a row staged in LDS, in both walk
    directions, with and without forced starts (its start is not clamped; the forward list is reversed by the pack kernel).
    logZ against the oracle's float64 alpha, by the rule of test_long_row_T4099_gpu.  No dense gradient at this size."""
    _lib.set_impl(0)
    _lib.device_status()
    _long_row_logz_decode(gpu, oracle, 8200)
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_long_row_T16400_gpu(gpu, oracle):
    """T = 16400 (1025 row blocks, 85 far parts, 2.15 GB): decode only -- the serial backtrack walking global memory, in both
    directions, bit-exact against the oracle; evalPath(decode) <= logZ.  The oracle's right-to-left sweep reads the score tensor
    by columns and takes 6 s per call at this length (the left-to-right one 0.6 s), so of the forced starts the mixed set runs in
    the forward direction only here and the backward extremes are checked from the definition; test_long_row_T8200_gpu runs all of
    them against the oracle through the same kernel (the two sizes differ in where the code row is read from, not in the walk).
    T >= 65535 (the row-sequential kernels for long rows) needs 34 GB per two chains and is left out."""
    _lib.set_impl(0)
    _lib.device_status()
    try:
        _long_row_decode(gpu, oracle, 16400)
        assert _lib.device_status() == 0
    finally:
        torch.cuda.empty_cache()                                          # (the helper's tensors are gone with its frame)


# ---- C. the chain-chunk limit ----------------------------------------------------------------------------------------------

MAX_CHUNKS = 16                                               # persist.hip
GS = 4                                                        # chains per ring


def _half_cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count // 2


def _dev_rel_err(a, b64):
    """conftest.rel_err on the device (the dense float64 gradient of 8192 chains is 0.6 GB)"""
    b = torch.from_numpy(b64).to(a.device)
    return float(((a.double() - b).abs() / b.abs().clamp_min(1.0)).max()) if b.numel() else 0.0


def _posterior_reference(lz64, grad64, gn64, sc, nc):
    """float64 posteriors reduced from the oracle's dense marginals (tests/test_posteriors.py: _dense_reference)"""
    T = grad64.shape[0]
    strict = np.tril(np.ones((T, T)), -1)
    r = {"logZ": lz64, "noise": gn64, "single": np.stack([grad64[t, t] for t in range(T)]),
         "end": np.einsum("ebc,eb->ec", grad64, strict), "begin": np.einsum("ebc,eb->bc", grad64, strict)}
    node = np.empty_like(r["end"])
    node[0] = 1.0
    node[1:] = gn64 + r["end"][1:]
    r["node"] = node
    escore = np.einsum("ebc,ebc,eb->c", grad64, sc.astype(np.float64), np.tril(np.ones((T, T)))) + (gn64 * nc).sum(0)
    r["entropy"] = lz64 - escore
    return r


def _chunk_case(dev, oracle, T, B, posteriors=False, logprob=False):
    """The whole batch against the oracle: forward_backward and decode in both directions with the mixed forced starts (the
    tolerances of test_persist_vs_oracle); optionally posteriors() and logProb + backward."""
    score, noise = synth.crf_inputs(T, B, 100 + T, dev, "randn")
    sc, nc = score.cpu().numpy(), noise.cpu().numpy()
    lz64, grad64, gn64, _, _ = oracle.forward_backward_f64(sc, nc)
    gt = grad_tol(lz64)
    lz, grad, gn = CRF.forward_backward(score, noise)
    assert rel_err(lz.cpu().numpy(), lz64) < LOGZ_TOL
    assert _dev_rel_err(grad, grad64) < gt
    assert rel_err(gn.cpu().numpy(), gn64) < gt
    del grad, gn
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    st = [(c * 7 + 3) % T for c in range(B)]
    assert crf.decode(forcedStartPos=st) == oracle.viterbi(sc, nc, st)
    assert crf.decode(forcedStartPos=st, forward=True) == oracle.viterbi(sc, nc, st, forward=True)
    if posteriors:
        P = crf.posteriors()
        ref = _posterior_reference(lz64, grad64, gn64, sc, nc)
        for k in ("node", "begin", "end", "single", "noise"):
            np.testing.assert_allclose(getattr(P, k).cpu().double().numpy(), ref[k], rtol=0, atol=gt, err_msg=k)
        np.testing.assert_allclose(P.logZ.cpu().double().numpy(), lz64, rtol=LOGZ_TOL, atol=LOGZ_TOL)
        ent = P.entropy.cpu().double().numpy()
        assert np.all(np.isfinite(ent)) and np.all(ent >= 0.0)
        np.testing.assert_allclose(ent, ref["entropy"], rtol=1e-4, atol=T * gt)
    if logprob:
        iv = synth.synthetic_intervals(T, B, seed=100 + T)
        s, n = score.clone().requires_grad_(), noise.clone().requires_grad_()
        lp = CRF.NeuralSemiCRFInterval(s, n).logProb(iv)
        path64, _ = path_reference(score.cpu(), noise.cpu(), iv)
        assert rel_err(lp.detach().cpu().numpy(), path64 - lz64) < LOGZ_TOL
        (-lp.sum()).backward()
        want = grad64.copy()                                             # d(-logProb) = marginal - indicator of the path's cells
        for c, lst in enumerate(iv):
            for b, e in lst:
                want[e, b, c] -= 1.0
        assert _dev_rel_err(s.grad, want) < gt
        assert rel_err(n.grad.cpu().numpy(), gn64 - (1.0 - cover_counts(iv, T, B))) < gt
        up = torch.triu(torch.ones(T, T, dtype=torch.bool, device=dev), diagonal=1)
        assert float(s.grad[up].abs().max()) == 0.0


CHUNK_CASES = {
    # name: (T, chains as a function of m = CUs / 2, posteriors, logProb)
    "sixteen_full": (97, lambda m: MAX_CHUNKS * m * GS, False, False),                 # sixteen full chunks with a far field (7 row blocks)
    "ragged_last_quad": (40, lambda m: MAX_CHUNKS * m * GS - 3, False, False),          # odd count, ragged last quad, in the sixteenth chunk
    "one_chain_chunk": (97, lambda m: GS * (MAX_CHUNKS - 1) * m + 1, True, False),      # the sixteenth chunk holds one chain
    "past_the_limit": (40, lambda m: MAX_CHUNKS * m * GS + 1, False, True),             # the row-sequential kernels
    "nine_uneven": (97, lambda m: round(4100 * m / 128), False, False),                 # nine chunks with an uneven last one
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHUNK_CASES))
def test_chain_chunk_limit_gpu(gpu, oracle, name):
    """A call is split into at most MAX_CHUNKS = 16 launches of CUs/2 rings x 4 chains (8192 chains on 256 CUs; one chain more runs
    on the row-sequential kernels): sixteen control-word blocks and error words, a last chunk of a single chain, the boundary."""
    T, chains, posteriors, logprob = CHUNK_CASES[name]
    m = _half_cus(gpu)
    if name == "one_chain_chunk" and m % 8 != 0:
        pytest.skip(f"CUs / 2 = {m} is no multiple of 8: chunks are rounded to whole panel groups and the sixteenth is not one chain")
    B = int(chains(m))
    _lib.set_impl(0)
    _lib.device_status()
    try:
        _chunk_case(gpu, oracle, T, B, posteriors, logprob)
        assert _lib.device_status() == 0
    finally:
        _lib.set_impl(0)
        torch.cuda.empty_cache()
