"""Forced-start posteriors and MBR decoding: semicrf_alpha_from and the forcedStartPos keyword of posteriors / interval_marginals /
decode_marginal / decode_mbr (and their _packed forms), and SegmentTranscriber.decoder = "mbr".

The model: chain c with start s is the semi-CRF on the frames s .. T-1, so every forced-start result equals the unconditional
result on the slice score[s:, s:, c], noise[s:, c], shifted by s.  CPU tests check the host kernels against that identity in
float64 (the C oracle), against exact enumeration and against the existing ops; GPU tests check the device kernel against the host
kernel and the float64 slices at the edges the kernel has (chain quads, the 16-chain group, its 16-row blocks), determinism,
containment, graph capture and the segment loop.

One deviation from what was asked for: decode_step and transcribe_many cannot run on CPU tensors -- the interval scorer, the
attribute gather and the segment kernels are registered for the GPU only -- so the CPU test of the segment loop
(test_transcriber_decode_cpu) covers the decode branch, _decode_packed, behind a stand-in scorer, and decode_step and
transcribe_many (synchronous False and True) are compared on the device (test_transcriber_gpu)."""
import importlib

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs
from forced_start_common import (KINDS, check_against_f64, cycle_starts, inputs, np_fields, peaked_inputs, segment_loop_starts,
                                 slice_reference)
from mbr_common import _mbr_reference
from test_posteriors import FIELDS, _compare, _enumerate, _grad_tol, _mixed_inputs
from test_tolerant_decode import _bits, _box_f64, _check_banded
from transkun_amd import CRF, _lib, synth

crf_mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

SLICE_CASES = [c for c in EDGE_CASES if c[1] in (2, 3, 24, 33, 48, 70)]
ROW_BLOCK = 16          # rows per block of alpha_from.hip (AR)


# ---- 1. the slice identity against float64 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", SLICE_CASES, ids=[c[0] for c in SLICE_CASES])
def test_slice_identity_cpu(oracle, case):
    name, T, B, kind, seed, tr = case
    s, n = edge_inputs(T, B, kind, seed, tr)
    st = cycle_starts(T, B)
    P = np_fields(CRF.posteriors(s, n, forcedStartPos=st))
    r = slice_reference(oracle, s, n, st)
    worst = check_against_f64(P, r, st, name, entropy=tr != "huge")      # (huge: logZ - E[score] cancels ~1e5-sized numbers)
    print(name, "worst field errors", worst)
    for c in range(B):                                                    # a slice of one frame, in closed form
        if st[c] == T - 1:
            d = float(s[T - 1, T - 1, c])
            assert abs(P["logZ"][c] - np.logaddexp(0.0, d)) <= 1e-5 * max(1.0, abs(np.logaddexp(0.0, d)))
            assert abs(P["single"][T - 1, c] - 1.0 / (1.0 + np.exp(-d))) <= 1e-4 and abs(P["node"][T - 1, c] - 1.0) <= 1e-4


# ---- 2. exact enumeration ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [3, 5, 7])
def test_exact_enumeration_cpu(T):
    s, n = _mixed_inputs(T)
    B = s.shape[2]
    iv = [[(b, e) for e in range(T) for b in range(e + 1)] for _ in range(B)]
    for a in range(T):
        got = CRF.interval_marginals(s, n, iv, forcedStartPos=[a] * B)
        truth = _enumerate(s[a:, a:].contiguous(), n[a:].contiguous())
        for c in range(B):
            for (b, e), m in zip(iv[c], got[c]):
                if b < a:
                    assert m == 0.0, (T, a, c, b, e, m)
                else:
                    assert abs(m - truth[c]["marg"][e - a, b - a]) <= 1e-5, (T, a, c, b, e)


# ---- 3. consistency and identities ---------------------------------------------------------------------------------------------------

def _identities(device):
    for name, T, B, kind, seed, tr in SLICE_CASES:
        s, n = edge_inputs(T, B, kind, seed, tr, device)
        P0, Pz = np_fields(CRF.posteriors(s, n)), np_fields(CRF.posteriors(s, n, forcedStartPos=[0] * B))
        tol = _grad_tol(P0["logZ"])
        assert np.all(np.abs(Pz["logZ"] - P0["logZ"]) <= 1e-5 * np.maximum(1.0, np.abs(P0["logZ"]))), name
        for k in FIELDS:
            np.testing.assert_allclose(Pz[k], P0[k], rtol=0, atol=tol, err_msg=f"{name}: {k}")
        if tr != "huge":
            np.testing.assert_allclose(Pz["entropy"], P0["entropy"], rtol=1e-4, atol=T * tol, err_msg=name)
        st = cycle_starts(T, B)
        start = torch.tensor(st, dtype=torch.int32, device=device)
        s2, n2, st2 = (crf_mod._pad1(s), crf_mod._pad1(n), crf_mod._pad1(start)) if B == 1 else (s, n, start)
        lz, v, q = crf_mod._marginal_inputs_from(s2.contiguous(), n2.contiguous(), st2)
        lz, v, q = lz.cpu().double().numpy(), v.cpu().double().numpy(), q.cpu().double().numpy()
        Ps = np_fields(CRF.posteriors(s, n, forcedStartPos=start))
        for c in range(B):
            assert v[T - 1, c] == lz[c]
            assert abs(lz[c] - q[st[c], c]) <= 1e-5 * max(1.0, abs(q[st[c], c])), (name, c, lz[c], q[st[c], c])
            assert np.all(np.isneginf(v[:st[c], c])) and np.all(np.isfinite(v[st[c]:, c])), (name, c)
            assert abs(Ps["node"][st[c], c] - 1.0) <= _grad_tol(lz), (name, c)


def test_identities_cpu():
    _identities("cpu")


@pytest.mark.gpu
def test_identities_gpu(gpu):
    _identities(gpu)
    assert _lib.device_status() == 0


# ---- 4. decode_marginal ------------------------------------------------------------------------------------------------------------------

def _decode_marginal(oracle, device, scale):
    T, B = 70, 20
    s, n = edge_inputs(T, B, "model", 22, None)
    st = cycle_starts(T, B)
    r = slice_reference(oracle, s, n, st)
    crf = CRF.NeuralSemiCRFInterval(s.to(device), n.to(device))
    for tol in (None, (1, 2)):
        U = _box_f64(r["marg"], *(tol or (0, 0)))                     # the box sum on the slice: it has no cell before the start
        for c in range(B):
            U[:, :st[c], c] = 0.0
        band = scale * _grad_tol(r["logZ"]) * np.maximum(1.0, U)
        for tau in (0.3, 0.5, 0.9):
            pairs, offsets, probs = crf.decode_marginal_packed(tau, tolerance=tol, forcedStartPos=st)
            _check_banded(U, tau, band, pairs, offsets, probs, f"tol={tol} tau={tau}")
            chain = np.repeat(np.arange(B), np.diff(offsets))
            assert np.all(pairs[:, 0] >= np.asarray(st)[chain]), "an interval begins before its chain's start"
            m = crf.interval_marginals_packed(pairs, offsets, tolerance=tol, forcedStartPos=st).cpu().numpy()
            assert np.array_equal(_bits(m), _bits(probs)), (tol, tau)
            paths, pl = crf.decode_marginal(tau, tolerance=tol, forcedStartPos=st)
            assert [x for lst in pl for x in lst] == probs.tolist() and sum(len(p) for p in paths) == len(probs)


def test_decode_marginal_cpu(oracle):
    _decode_marginal(oracle, "cpu", 1.0)


# ---- 5. decode_mbr ---------------------------------------------------------------------------------------------------------------------------

def _decode_mbr(T, B, kind, seed, device):
    s, n = synth.crf_inputs(T, B, seed, "cpu", kind)
    st = cycle_starts(T, B)
    crf = CRF.NeuralSemiCRFInterval(s.to(device), n.to(device))
    for tol in (None, (2, 2)):
        for thr in (0.2, 0.5):
            tau = np.full(B, thr, np.float32)
            lat_p, lat_o, lat_w = crf.decode_marginal_packed(thr, tolerance=tol, forcedStartPos=st)
            pairs, offsets, probs, gain = crf.decode_mbr_packed(thr, tolerance=tol, forcedStartPos=st)
            wp, wo, ww, wg = _mbr_reference(lat_p, lat_o, lat_w, T, tau)
            assert np.array_equal(offsets, wo) and np.array_equal(pairs, wp), (tol, thr)
            assert np.array_equal(_bits(probs), _bits(ww)) and np.array_equal(_bits(gain), _bits(wg)), (tol, thr)
            paths, pl, g2 = crf.decode_mbr(thr, tolerance=tol, forcedStartPos=st)
            assert np.array_equal(_bits(g2), _bits(gain)) and [x for lst in pl for x in lst] == probs.tolist()
            for c in range(B):                                        # a valid path of the slice: evalPath takes it there
                a = st[c]
                for (b1, e1), (b2, e2) in zip(paths[c], paths[c][1:]):
                    assert b1 <= e1 and e1 <= b2, (c, (b1, e1), (b2, e2))
                assert all(a <= b <= e < T for b, e in paths[c]), (c, a, paths[c])
                ev = CRF.evalPath([[(b - a, e - a) for b, e in paths[c]]], s[a:, a:, c:c + 1].contiguous(), n[a:, c:c + 1].contiguous())
                assert bool(torch.isfinite(ev).all()), c


@pytest.mark.parametrize("T,B,kind,seed", [(70, 20, "model", 22), (48, 1, "ties", 20)])
def test_decode_mbr_cpu(T, B, kind, seed):
    _decode_mbr(T, B, kind, seed, "cpu")


# ---- 6. MBR equals Viterbi on a peaked posterior --------------------------------------------------------------------------------------

def _peaked(device):
    T, B = 70, 20
    st = segment_loop_starts(T, B, 5)
    st[0], st[1], st[2] = 0, T - 1, T - 2
    s, n, want = peaked_inputs(T, st, 17)
    crf = CRF.NeuralSemiCRFInterval(s.to(device), n.to(device))
    vit = crf.decode(forcedStartPos=st)
    paths, probs, _ = crf.decode_mbr(0.5, forcedStartPos=st)
    assert vit == want, "the construction: Viterbi from the start returns the planted path"
    assert paths == vit
    assert all(p > 0.95 for lst in probs for p in lst)


def test_mbr_equals_viterbi_on_peaked_posterior_cpu():
    _peaked("cpu")


@pytest.mark.gpu
def test_mbr_equals_viterbi_on_peaked_posterior_gpu(gpu):
    _peaked(gpu)
    assert _lib.device_status() == 0


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------

def _errors(device):
    T, B = 24, 5
    s, n = synth.crf_inputs(T, B, 3, device, "randn")
    crf = CRF.NeuralSemiCRFInterval(s, n)
    iv = [[(0, 1)]] * B
    calls = [lambda st: crf.posteriors(forcedStartPos=st), lambda st: crf.interval_marginals(iv, forcedStartPos=st),
             lambda st: crf.decode_marginal(0.5, forcedStartPos=st), lambda st: crf.decode_marginal_packed(0.5, forcedStartPos=st),
             lambda st: crf.decode_mbr(0.5, forcedStartPos=st), lambda st: crf.decode_mbr_packed(0.5, tolerance=1, forcedStartPos=st),
             lambda st: CRF.posteriors(s, n, forcedStartPos=st)]
    for f in calls:
        with pytest.raises(IndexError):
            f([0] * (B - 1))
        with pytest.raises(IndexError):
            f([0] * (B + 1))
        with pytest.raises(IndexError):
            f([0, 0, T, 0, 0])
        with pytest.raises(IndexError):
            f([0, -1, 0, 0, 0])
        with pytest.raises((TypeError, ValueError)):
            f([0.0] * B)
        with pytest.raises((TypeError, ValueError)):
            f(torch.zeros(B, device=device))                          # a float tensor
        f([T - 1] * B)                                                # the last frame is a start


def test_errors_cpu():
    _errors("cpu")
    from transkun_amd.transcribe import SegmentTranscriber
    tr = SegmentTranscriber(32, 48, 48, targetMIDIPitch=list(range(5)))
    tr.decoder = "marginal"
    with pytest.raises(ValueError):
        tr._decode_packed(torch.zeros(1, 5, 8, 32), None)
    with pytest.raises(ValueError):
        tr.transcribe_many([lambda i, T: None], [44100])


@pytest.mark.gpu
def test_errors_gpu(gpu):
    _errors(gpu)


def _invalid_result_raises(device):
    """An invalid result (alpha's last row holds NaN) raises from decode_marginal / decode_mbr, with and without a tolerance: the
    kernels' marker offsets[B] = -1 survives the forced-start path."""
    T, B = 24, 5
    s, n = synth.crf_inputs(T, B, 3, device, "randn")
    st = cycle_starts(T, B)
    s_nan = s.clone()
    s_nan[7, 3, 0] = float("nan")                                     # chain 0 starts at frame 0: the cell is read
    crf = CRF.NeuralSemiCRFInterval(s_nan, n)
    good = CRF.NeuralSemiCRFInterval(s, n)
    for tol in (None, (1, 1)):
        assert len(good.decode_marginal_packed(0.5, tolerance=tol, forcedStartPos=st)[0]) > 0
        assert len(good.decode_mbr_packed(0.5, tolerance=tol, forcedStartPos=st)[0]) > 0
        with pytest.raises(RuntimeError):
            crf.decode_marginal_packed(0.5, tolerance=tol, forcedStartPos=st)
        with pytest.raises(RuntimeError):
            crf.decode_mbr_packed(0.5, tolerance=tol, forcedStartPos=st)
        with pytest.raises(RuntimeError):
            crf.decode_mbr(0.3, tolerance=tol, forcedStartPos=st)
    # the marker itself, through the filter of the tolerance path
    pairs = torch.tensor([[0, 1], [2, 3], [1, 1], [4, 6], [5, 5]], dtype=torch.int32, device=device)
    probs = torch.full((5,), 0.7, device=device)
    start = torch.tensor([1, 0, 0], dtype=torch.int32, device=device)
    for last, want in ((-1, [0, 2, 5, -1]), (9, [0, 2, 5, 9]), (5, [0, 1, 4, 4])):
        off = torch.tensor([0, 2, 5, last], dtype=torch.int32, device=device)
        assert crf_mod._drop_before_start(pairs, off, probs, start)[1].tolist() == want, last
    if torch.device(device).type != "cpu":                            # a start out of range in a device tensor: not checked on the host
        bad = torch.tensor(st, dtype=torch.int32, device=device)
        bad[1] = T
        for tol in (None, (1, 1)):
            with pytest.raises(RuntimeError):
                good.decode_marginal_packed(0.5, tolerance=tol, forcedStartPos=bad)
            with pytest.raises(RuntimeError):
                good.decode_mbr_packed(0.5, tolerance=tol, forcedStartPos=bad)
        _lib.async_error()


def test_invalid_result_raises_cpu():
    _invalid_result_raises("cpu")


@pytest.mark.gpu
def test_invalid_result_raises_gpu(gpu):
    _invalid_result_raises(gpu)


# ---- 8. the segment loop's decode ------------------------------------------------------------------------------------------------------

class _TorchScorer(torch.nn.Module):
    """A stand-in for the interval scorer (whose kernels exist on the GPU only) with its interface: ctx [N, P, T, D] ->
    (S [T, T, N, P], noise [T-1, N, P]).  Any deterministic function of ctx serves: the test is about what follows the scorer."""
    fullSquare, slotPitch, size, expansionFactor = 0, None, 32, 1

    def forward(self, ctx):
        x = ctx.float()
        S = torch.einsum("npeh,npbh->ebnp", x[..., :16], x[..., 16:]) * 4.0
        return S.contiguous(), (x[:, :, 1:, 0] + x[:, :, :-1, 1]).permute(2, 0, 1).contiguous()


def test_transcriber_decode_cpu():
    """decoder = "mbr" on the CPU: _decode_packed hands the scorer's output to the MBR helper with the carried starts and returns
    decode_mbr_packed's path.  (The interval scorer, the attribute gather and the event kernel run on the GPU only, so decode_step
    and transcribe_many are compared on the device: test_transcriber_gpu.)"""
    from segment_common import segment_inputs
    from transkun_amd.transcribe import SegmentTranscriber
    ctx, _, _, _, _, starts = segment_inputs("small")
    N, P, T, D = ctx.shape
    tr = SegmentTranscriber(D, 48, 48, targetMIDIPitch=list(range(P))).eval()
    tr.scorer = _TorchScorer()
    S, b = tr.scorer(ctx)
    score, noise = S.flatten(-2, -1).contiguous(), b.flatten(-2, -1).contiguous()
    start = torch.tensor(starts, dtype=torch.int32)
    assert tr.decoder == "viterbi" and tr.mbrThreshold == 0.5 and tr.mbrTolerance is None
    vp, vo = tr._decode_packed(ctx, start)
    wp, wo = CRF.NeuralSemiCRFInterval(score, noise).decode_packed(forcedStartPos=starts)
    assert np.array_equal(vo.numpy(), wo) and np.array_equal(vp[:int(vo[-1])].numpy(), wp)
    tr.decoder = "mbr"
    for thr, tol, st in ((0.5, None, start), (0.3, None, start), (0.5, (1, 1), start), (0.5, None, None)):
        tr.mbrThreshold, tr.mbrTolerance = thr, tol
        pairs, offsets = tr._decode_packed(ctx, st)
        wp, wo, _, _ = CRF.decode_mbr_packed(score, noise, thr, tolerance=tol, forcedStartPos=starts if st is not None else [0] * (N * P))
        assert offsets.dtype == torch.int32 and pairs.dtype == torch.int32
        assert np.array_equal(offsets.numpy(), wo) and np.array_equal(pairs[:int(offsets[-1])].numpy(), wp), (thr, tol)
        assert int(offsets[-1]) > 0


# ---- 9. device against host and float64 ------------------------------------------------------------------------------------------------

GPU_SHAPES = [(2, 3), (3, 5), (24, 1), (33, 7), (65, 63), (70, 65), (130, 90), (257, 20)]


def start_patterns(T, B):
    clip = lambda x: min(max(int(x), 0), T - 1)
    pats = {"zero": [0] * B, "last": [T - 1] * B, "last2": [clip(T - 2)] * B}
    edges = [ROW_BLOCK - 1, ROW_BLOCK, ROW_BLOCK + 1, 63, 64, 65]
    pats["block_edges"] = [clip(edges[(c // 4) % 6]) if c % 4 == (c // 24) % 4 else 0 for c in range(B)]   # one chain per quad
    pats["quad"] = [clip([0, 1, T // 2, T - 1][c % 4]) for c in range(B)]
    pats["groups"] = [T - 1 if (c // 16) % 2 == 0 else 0 for c in range(B)] if B > 16 else [T - 1 if c < B // 2 else 0 for c in range(B)]
    return pats


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("T,B", GPU_SHAPES)
def test_device_matches_host_and_f64_gpu(oracle, gpu, T, B, kind):
    s, n = inputs(T, B, kind, 31 + T + B)
    sd, nd = s.to(gpu), n.to(gpu)
    for name, st in start_patterns(T, B).items():
        what = f"{T}x{B} {kind} {name}"
        Ph = np_fields(CRF.posteriors(s, n, forcedStartPos=st))
        Pd = np_fields(CRF.posteriors(sd, nd, forcedStartPos=st))
        assert np.all(np.abs(Pd["logZ"] - Ph["logZ"]) <= 1e-5 * np.maximum(1.0, np.abs(Ph["logZ"]))), what
        for k in FIELDS:
            for c in range(B):
                assert np.all(Pd[k][:st[c], c] == 0.0), (what, k, c)
        if kind == "huge":                                            # (entropy: logZ - E[score] cancels ~1e5-sized numbers)
            tol = 4 * _grad_tol(Ph["logZ"])
            for k in FIELDS:
                np.testing.assert_allclose(Pd[k], Ph[k], rtol=0, atol=tol, err_msg=f"{what}: {k}")
        else:
            _compare(Pd, Ph, what)
        if T <= 130:
            r = slice_reference(oracle, s, n, st)
            worst = check_against_f64(Pd, r, st, what, entropy=kind != "huge")
            print(what, "worst against float64", worst)
    assert _lib.device_status() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1100, 2048, 2050])
def test_lds_alpha_limits_gpu(gpu, T):
    """The group's alpha in more than the default 64 KB of LDS (T = 1100: 69 KB; T = 2048: the largest, 128 KB), and T > 2048,
    where it no longer fits and the far field reads the v the workgroup wrote itself."""
    B = 3
    s, n = synth.crf_inputs(T, B, 9, "cpu", "randn")
    st = torch.tensor([0, T // 2 + 6, T - 1], dtype=torch.int32)
    lh, vh = crf_mod._alpha_from_raw(s, n, st)
    ld, vd = crf_mod._alpha_from_raw(s.to(gpu), n.to(gpu), st.to(gpu))
    ld, vd = ld.cpu(), vd.cpu()
    assert torch.equal(torch.isneginf(vd), torch.isneginf(vh))
    fin = torch.isfinite(vh)
    assert float(((vd[fin] - vh[fin]).abs() / vh[fin].abs().clamp(min=1.0)).max()) <= 1e-5
    assert float(((ld - lh).abs() / lh.abs().clamp(min=1.0)).max()) <= 1e-5
    assert _lib.device_status() == 0


# ---- 10. one model-shaped case ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_model_shape_gpu(oracle, gpu):
    T, B = 691, 90
    s, n = synth.crf_inputs(T, B, 41, "cpu", "model")
    st = segment_loop_starts(T, B, 7)
    assert max(st) <= 345 and st.count(0) >= B // 2
    ch, cd = CRF.NeuralSemiCRFInterval(s, n), CRF.NeuralSemiCRFInterval(s.to(gpu), n.to(gpu))
    Ph, Pd = np_fields(ch.posteriors(forcedStartPos=st)), np_fields(cd.posteriors(forcedStartPos=st))
    assert np.all(np.abs(Pd["logZ"] - Ph["logZ"]) <= 1e-5 * np.maximum(1.0, np.abs(Ph["logZ"])))
    _compare(Pd, Ph, "691x90")
    order = np.argsort(st, kind="stable")
    six = [int(order[i]) for i in (0, B // 2, B // 2 + 8, B // 2 + 20, B - 8, B - 1)]       # spread over the start range
    r = slice_reference(oracle, s, n, st, chains=six)
    print("691x90 worst against float64", check_against_f64(Pd, r, st, "691x90", chains=six), "starts", [st[c] for c in six])
    # decode_marginal(0.5): the same cells but for those within the tolerance of the threshold, probs within the tolerance
    tol = 4 * _grad_tol(Ph["logZ"])
    hp, ho, hw = ch.decode_marginal_packed(0.5, forcedStartPos=st)
    dp, do, dw = cd.decode_marginal_packed(0.5, forcedStartPos=st)
    key = lambda p, o: {(int(c), int(b), int(e)): i for i, (c, (b, e)) in enumerate(zip(np.repeat(np.arange(B), np.diff(o)), p))}
    kh, kd = key(hp, ho), key(dp, do)
    for k in set(kh) ^ set(kd):
        w = hw[kh[k]] if k in kh else dw[kd[k]]
        assert abs(float(w) - 0.5) <= tol, (k, float(w))
    both = sorted(set(kh) & set(kd))
    assert len(both) > B and max(abs(float(hw[kh[k]]) - float(dw[kd[k]])) for k in both) <= tol
    # decode_mbr(0.3, tolerance=(2, 2)): each side is the exact recursion on its own lattice; the maximised sums agree
    hp, ho, hw, hg = ch.decode_mbr_packed(0.3, tolerance=(2, 2), forcedStartPos=st)
    dp, do, dw, dg = cd.decode_mbr_packed(0.3, tolerance=(2, 2), forcedStartPos=st)
    lat = cd.decode_marginal_packed(0.3, tolerance=(2, 2), forcedStartPos=st)
    wp, wo, ww, wg = _mbr_reference(lat[0], lat[1], lat[2], T, np.full(B, 0.3, np.float32))
    assert np.array_equal(do, wo) and np.array_equal(dp, wp) and np.array_equal(_bits(dw), _bits(ww)) and np.array_equal(_bits(dg), _bits(wg))
    chain = np.repeat(np.arange(B), np.diff(do))
    assert np.all(dp[:, 0] >= np.asarray(st)[chain])
    counts = np.maximum(np.diff(ho), np.diff(do)) + 1
    # (each interval's M is a box of up to 25 cells, every one within `tol`)
    assert np.all(np.abs(hg.astype(np.float64) - dg.astype(np.float64)) <= 25 * tol * counts), float(np.max(np.abs(hg - dg)))
    assert _lib.device_status() == 0


# ---- 11. determinism and containment ---------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_determinism_and_containment_gpu(gpu):
    for T, B in [(70, 65), (257, 20), (130, 90)]:
        s, n = synth.crf_inputs(T, B, 5 + T, gpu, "randn")
        for name, st in start_patterns(T, B).items():
            start = torch.tensor(st, dtype=torch.int32, device=gpu)
            lz, v = crf_mod._alpha_from_raw(s, n, start)
            lz2, v2 = crf_mod._alpha_from_raw(s, n, start)
            assert torch.equal(v, v2) and torch.equal(lz, lz2), (T, B, name)
            assert torch.equal(lz, v[T - 1])
            before = torch.arange(T, device=gpu)[:, None] < start[None, :]              # [t, c]: t < start[c]
            assert bool(torch.isneginf(v[before]).all()) and bool(torch.isfinite(v[~before]).all()), (T, B, name)
            # cells with begin > end, and the columns (begin) before each chain's start: never read
            col = torch.arange(T, device=gpu)
            dead = (col[None, :, None] > col[:, None, None]) | (col[None, :, None] < start[None, None, :])     # [end, begin, c]
            ndead = col[:-1, None] < start[None, :]                                      # the gap t .. t+1 with t before the start
            for val in (float("nan"), float("inf"), float("-inf"), 1e30):
                s2 = torch.where(dead, torch.full_like(s, val), s)
                n2 = torch.where(ndead, torch.full_like(n, val), n)
                lz3, v3 = crf_mod._alpha_from_raw(s2, n2, start)
                assert torch.equal(v3, v) and torch.equal(lz3, lz), (T, B, name, val)
    # a start out of range (device tensor: not checked on the host) gives NaN for that chain only
    T, B = 70, 21
    s, n = synth.crf_inputs(T, B, 77, gpu, "randn")
    good = torch.tensor(cycle_starts(T, B), dtype=torch.int32, device=gpu)
    bad = good.clone()
    bad[2], bad[9], bad[20] = T, -1, 1 << 30
    lz, v = crf_mod._alpha_from_raw(s, n, good)
    lzb, vb = crf_mod._alpha_from_raw(s, n, bad)
    isbad = torch.zeros(B, dtype=torch.bool, device=gpu)
    isbad[[2, 9, 20]] = True
    assert bool(torch.isnan(lzb[isbad]).all()) and bool(torch.isnan(vb[:, isbad]).all())
    # (the other chains: the same values up to fp32 rounding -- a group's row blocks begin at its smallest valid start, so the
    # order of their sums may move with a neighbour's start)
    a, b = vb[:, ~isbad], v[:, ~isbad]
    assert torch.equal(torch.isneginf(a), torch.isneginf(b)) and not bool(torch.isnan(a).any())
    fin = torch.isfinite(b)
    assert bool(((a[fin] - b[fin]).abs() <= 1e-5 * b[fin].abs().clamp(min=1.0)).all())
    assert bool(((lzb[~isbad] - lz[~isbad]).abs() <= 1e-5 * lz[~isbad].abs().clamp(min=1.0)).all())
    P = CRF.posteriors(s, n, forcedStartPos=bad)
    assert bool(torch.isnan(P.logZ[isbad]).all()) and bool(torch.isfinite(P.logZ[~isbad]).all())
    assert bool(torch.isfinite(P.node[:, ~isbad]).all())
    assert _lib.device_status() == 0


# ---- 12. graph capture ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    T, B = 333, 46
    data = [synth.crf_inputs(T, B, 600 + i, gpu) for i in range(3)]
    starts = [torch.tensor(segment_loop_starts(T, B, 20 + i), dtype=torch.int32, device=gpu) for i in range(3)]

    def chain(s, n, st):
        return list(crf_mod._posteriors_raw(s, n, None, st))

    want = [[x.clone() for x in chain(s, n, st)] for (s, n), st in zip(data, starts)]
    for w, (s, n), st in zip(want, data, starts):
        assert all(torch.equal(a, b) for a, b in zip(w, CRF.posteriors(s, n, forcedStartPos=st)))
    s_in, n_in, st_in = data[0][0].clone(), data[0][1].clone(), starts[0].clone()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(2):
            chain(s_in, n_in, st_in)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = chain(s_in, n_in, st_in)
    for i in (1, 2, 0, 1):
        s_in.copy_(data[i][0]); n_in.copy_(data[i][1]); st_in.copy_(starts[i])
        graph.replay()
        torch.cuda.synchronize(gpu)
        for a, b in zip(got, want[i]):
            assert torch.equal(a, b), i
    assert _lib.device_status() == 0


# ---- 13. the segment loop on the device ------------------------------------------------------------------------------------------------

def _small_transcriber(gpu):
    from segment_common import transcribe_inputs
    from transkun_amd.transcribe import SegmentTranscriber
    I = transcribe_inputs("small", gpu)
    m = SegmentTranscriber(I["D"], I["H"], I["H"], I["hop"], I["win"], I["fs"], I["step_s"], I["seg_s"]).to(gpu).eval()
    with torch.no_grad():
        m.scorer.map[0].weight.copy_(I["W"]); m.scorer.map[0].bias.copy_(I["bias"])
        for mod, w in ((m.velocityPredictor, I["heads"]["velocity"]), (m.refinedOFPredictor, I["heads"]["of"])):
            mod[0].weight.copy_(w[0]); mod[0].bias.copy_(w[1]); mod[3].weight.copy_(w[2]); mod[3].bias.copy_(w[3])
    return m, I


@pytest.mark.gpu
def test_transcriber_gpu(gpu):
    from transkun_amd.scorer import slot_pitch
    from transkun_amd.transcribe import SegmentTranscriber
    # decode_step in the slot layout: 90 symbols of one segment in 96 slots
    N, P, T, D = 1, 90, 128, 64
    assert slot_pitch(P, T, D, N) == 96
    ctx = synth.hash_normal(N * P * T * D, 901, gpu).view(N, P, T, D) * 0.5
    tr = SegmentTranscriber(D, 48, 48).to(gpu).eval()
    with torch.no_grad():
        tr.scorer.map[0].weight.copy_(synth.hash_normal((2 * D + 1) * D, 902, gpu).view(2 * D + 1, D) * (0.3 / D ** 0.5))
        tr.scorer.map[0].bias.copy_(synth.hash_normal(2 * D + 1, 903, gpu) * 0.1)
        S, b = tr.scorer(ctx)                                         # chain layout (no slots): what decode_mbr_packed is given
    score, noise = S.flatten(-2, -1).contiguous(), b.flatten(-2, -1).contiguous()
    starts = [(c * 29 + 3) % (T // 2) if c % 2 else 0 for c in range(N * P)]
    start = torch.tensor(starts, dtype=torch.int32, device=gpu)
    beginTime = torch.zeros(N, dtype=torch.float64, device=gpu)
    vit = tr.decode_step(ctx, start, beginTime, T - 1, T // 2)
    wp, wo = CRF.NeuralSemiCRFInterval(score, noise).decode_packed(forcedStartPos=starts)
    assert np.array_equal(vit["offsets"].cpu().numpy(), wo) and np.array_equal(vit["pairs"].cpu().numpy(), wp)
    tr.decoder = "mbr"
    for thr, tol, st in ((0.5, None, start), (0.3, None, start), (0.5, (1, 1), start), (0.5, None, None)):
        tr.mbrThreshold, tr.mbrTolerance = thr, tol
        step = tr.decode_step(ctx, st, beginTime, T - 1, T // 2)
        wp, wo, _, _ = CRF.decode_mbr_packed(score, noise, thr, tolerance=tol, forcedStartPos=starts if st is not None else [0] * (N * P))
        assert step["K"] == int(wo[-1]) and step["K"] > 0
        assert np.array_equal(step["offsets"].cpu().numpy(), wo) and np.array_equal(step["pairs"].cpu().numpy(), wp), (thr, tol)
    bad = start.clone()
    bad[7] = T                                                        # a start out of range: the step raises, by name
    for tol in (None, (1, 1)):
        tr.mbrTolerance = tol
        with pytest.raises(RuntimeError, match="mbr"):
            tr.decode_step(ctx, bad, beginTime, T - 1, T // 2)
    _lib.async_error()

    # transcribe_many: the capped no-sync route and the synchronous one return the same Notes, and MBR without a tolerance stays
    # on the capped route
    m, I = _small_transcriber(gpu)
    m.decoder = "mbr"
    calls = []
    orig = m.transcribe_many

    def spy(*a, **k):
        calls.append(bool(k.get("synchronous", a[7] if len(a) > 7 else False)))
        return orig(*a, **k)
    m.transcribe_many = spy
    fn = lambda i, T: I["ctxs"][i]
    table = lambda notes: [(e.start, e.end, e.pitch, e.velocity, e.hasOnset, e.hasOffset) for e in notes]
    fast = m.transcribe_many([fn, fn], [I["n_sample_unpadded"]] * 2)
    assert calls == [False], "decoder='mbr' without a tolerance restarted into the synchronous route"
    slow = m.transcribe_many([fn, fn], [I["n_sample_unpadded"]] * 2, synchronous=True)
    assert len(fast[0]) > 0 and table(fast[0]) == table(slow[0]) and table(fast[1]) == table(slow[1]) and table(fast[0]) == table(fast[1])
    m.mbrTolerance = (1, 1)
    tolerant = m.transcribe_many([fn], [I["n_sample_unpadded"]])
    assert len(tolerant[0]) > 0
    m.decoder = "viterbi"
    vit_notes = m.transcribe_many([fn], [I["n_sample_unpadded"]])
    print("notes: mbr", len(fast[0]), "mbr tolerant", len(tolerant[0]), "viterbi", len(vit_notes[0]))
    assert _lib.device_status() == 0


@pytest.mark.gpu
def test_decode_marginal_and_mbr_gpu(oracle, gpu):
    _decode_marginal(oracle, gpu, 4.0)
    _decode_mbr(70, 20, "model", 22, gpu)
    _decode_mbr(48, 1, "ties", 20, gpu)
    assert _lib.device_status() == 0
