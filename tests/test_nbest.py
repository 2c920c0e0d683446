"""k-best Viterbi decoding (NeuralSemiCRFInterval.decode_nbest / decode_nbest_packed, semicrf_viterbi_nbest).

CPU tests check the host kernel against exact enumeration of every path (tiny T), against the reference decode (k = 1) on the
edge goldens, for the prefix property, and against a numpy-fp32 restatement of the recursion and its order; GPU tests check the
device against the host kernel bit for bit (on both sides of the walk's LDS limit too), and k = 1 against the device decode."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs, load_golden, rel_err
from path_targets_common import path_reference
from transkun_amd import CRF, _lib, synth

DIRS = [False, True]


def _segments(pairs, offsets):
    return [[tuple(int(x) for x in p) for p in pairs[offsets[i]:offsets[i + 1]]] for i in range(len(offsets) - 1)]


def _starts(T, B, seed, forward):
    if T == 1:
        return [0] * B
    rng = np.random.default_rng(seed)
    return [int(x) for x in rng.integers(0, T, B)]


# ---- exact enumeration -----------------------------------------------------------------------------------------------------

def _enumerate(s, n, c, T, start, forward):
    """All paths of chain c from `start` (backward) or to `start` (forward) as (sorted pair tuple, float64 score)."""
    s = s.astype(np.float64)
    n = n.astype(np.float64)
    out = []

    def rec(t, acc, path):
        for on in (False, True):
            a2 = acc + (s[t, t, c] if on else 0.0)
            p2 = path + [(t, t)] if on else path
            if t == (0 if forward else T - 1):
                out.append((tuple(sorted(p2)), a2))
                continue
            if forward:
                rec(t - 1, a2 + n[t - 1, c], p2)
                for j in range(t):
                    rec(j, a2 + s[t, j, c], p2 + [(j, t)])
            else:
                rec(t + 1, a2 + n[t, c], p2)
                for e in range(t + 1, T):
                    rec(e, a2 + s[e, t, c], p2 + [(t, e)])
    rec(start, 0.0, [])
    return out


def _eval64(path, s, n, c, T, start, forward):
    """float64 score of a path (decode's walk form) from / to `start`."""
    s = s.astype(np.float64)
    n = n.astype(np.float64)
    tot = 0.0
    covered = set()
    lo, hi = (0, start) if forward else (start, T - 1)
    for b, e in path:
        assert lo <= b <= e <= hi
        tot += s[e, b, c]
        if b < e:
            covered.update(range(b, e))
    for g in range(lo, hi):
        if g not in covered:
            tot += n[g, c]
    return tot


@pytest.mark.parametrize("T", [1, 2, 3, 5, 6])
@pytest.mark.parametrize("kind", ["randn", "ties"])
@pytest.mark.parametrize("forward", DIRS)
@pytest.mark.parametrize("forced", [False, True])
def test_exhaustive_enumeration(T, kind, forward, forced):
    B = 3
    score, noise = synth.crf_inputs(T, B, 100 + T, "cpu", kind)
    s, n = score.numpy(), noise.numpy()
    st = _starts(T, B, T * 7 + forward, forward) if forced else None
    for k in (1, 3, 8, 16):
        pairs, offsets, scores, npaths = CRF.viterbi_nbest_packed(score, noise, k, st, forward)
        assert pairs.dtype == np.int32 and offsets.dtype == np.int32 and scores.dtype == np.float32 and npaths.dtype == np.int32
        assert scores.shape == (k, B) and offsets.shape == (k * B + 1,)
        segs = _segments(pairs, offsets)
        for c in range(B):
            start = st[c] if forced else (T - 1 if forward else 0)
            allp = _enumerate(s, n, c, T, start, forward)
            byp = dict(allp)
            assert len(byp) == len(allp)                                   # derivations and paths correspond one to one
            want = sorted((v for _, v in allp), reverse=True)[:k]
            assert npaths[c] == min(k, len(allp))
            got = []
            for r in range(k):
                seg = segs[r * B + c]
                if r >= npaths[c]:
                    assert seg == [] and scores[r, c] == -np.inf
                    continue
                assert tuple(seg) in byp, (r, c, seg)                      # a valid path, in decode's order
                assert seg == sorted(seg)
                got.append(tuple(seg))
                v64 = _eval64(seg, s, n, c, T, start, forward)
                assert abs(v64 - byp[tuple(seg)]) < 1e-9
                assert abs(float(scores[r, c]) - v64) < 1e-5
            assert len(set(got)) == len(got)                               # distinct
            vals = [byp[p] for p in got]
            assert np.allclose(vals, want, rtol=0, atol=1e-5)
            assert all(vals[i] >= vals[i + 1] - 1e-5 for i in range(len(vals) - 1))


# ---- k = 1 is decode -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_k1_equals_reference_decode(case):
    name, T, B, kind, seed, tr = case
    g = load_golden("edge_" + name)
    score, noise = edge_inputs(T, B, kind, seed, tr)
    for key in ("none", "zero", "Tm2", "Tm1", "mixed"):
        for d in ("bwd", "fwd"):
            st = g.get(f"decode_{key}_{d}_start")
            st = None if st is None else [int(x) for x in st]
            pairs, offsets, scores, npaths = CRF.viterbi_nbest_packed(score, noise, 1, st, d == "fwd")
            assert np.array_equal(offsets, g[f"decode_{key}_{d}_offsets"].astype(np.int32)), (key, d)
            assert np.array_equal(pairs.reshape(-1, 2), g[f"decode_{key}_{d}_pairs"].reshape(-1, 2)), (key, d)
            assert (npaths == 1).all()


# ---- prefix property -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("forward", DIRS)
@pytest.mark.parametrize("inputs", ["T40_B90", "T48_B9_ties", "T70_B20_model"])
def test_prefix_property(forward, inputs):
    case = [c for c in EDGE_CASES if c[0] == inputs][0]
    _, T, B, kind, seed, tr = case
    score, noise = edge_inputs(T, B, kind, seed, tr)
    st = _starts(T, B, 5, forward)
    big = CRF.viterbi_nbest_packed(score, noise, 16, st, forward)
    segs = _segments(big[0], big[1])
    for m in (1, 2, 5):
        p, o, sc, npth = CRF.viterbi_nbest_packed(score, noise, m, st, forward)
        assert _segments(p, o) == segs[:m * B]
        assert np.array_equal(sc.view(np.int32), big[2][:m].view(np.int32))
        assert np.array_equal(npth, np.minimum(big[3], m))


# ---- numpy-fp32 restatement ------------------------------------------------------------------------------------------------

def _restate(s, n, k, start, forward):
    """The recursion and its order, written out in numpy fp32: per (frame, chain) every (candidate, rank, singleton) item is
    built and the list is the first k of a lexsort by (value desc, base desc, candidate, rank, singleton choice)."""
    T, B = s.shape[0], s.shape[2]
    f32 = np.float32
    zero = f32(0.0)
    segs = [[None] * B for _ in range(k)]
    scores = np.full((k, B), -np.inf, np.float32)
    for c in range(B):
        U = [None] * T                       # per frame: (values [m], pointers [m] of (pred frame, pred rank, on, cidx))
        order = range(T) if forward else range(T - 1, -1, -1)
        for t in order:
            d = f32(s[t, t, c])
            flip = 1 if d > 0 else 0
            cands = []                       # (cidx, pred frame, cell)
            if t != (0 if forward else T - 1):
                if forward:
                    cands.append((0, t - 1, f32(n[t - 1, c])))
                    cands += [(j + 1, j, f32(s[t, j, c])) for j in range(t)]
                else:
                    cands.append((0, t + 1, f32(n[t, c])))
                    cands += [(e + 1, e, f32(s[e, t, c])) for e in range(t + 1, T)]
            vals, bases, cid, rk, sg, ptr = [], [], [], [], [], []
            items = ([(zero, -1, 0, 0)] if not cands else
                     [(f32(uv + x), pf, r, ci) for ci, pf, x in cands for r, uv in enumerate(U[pf][0])])
            for base, pf, r, ci in items:
                for on in (0, 1):
                    vals.append(f32(base + d) if on else f32(base + zero))
                    bases.append(base)
                    cid.append(ci)
                    rk.append(r)
                    sg.append(on ^ flip)             # 0: the decode's own choice
                    ptr.append((pf, r, on, ci))
            vals = np.asarray(vals, np.float32)
            bases = np.asarray(bases, np.float32)
            idx = np.lexsort((np.asarray(sg), np.asarray(rk), np.asarray(cid), -bases.astype(np.float64),
                              -vals.astype(np.float64)))[:k]
            U[t] = (vals[idx], [ptr[i] for i in idx])
        st = start[c] if start is not None else (T - 1 if forward else 0)
        vals = U[st][0]
        for r in range(len(vals)):
            scores[r, c] = vals[r]
            path, j, rr = [], st, r
            while True:
                pf, prk, on, ci = U[j][1][rr]
                if on:
                    path.append((j, j))
                if pf < 0:
                    break
                if ci > 0:
                    path.append((pf, j) if forward else (j, pf))
                j, rr = pf, prk
            segs[r][c] = sorted(path)
    return segs, scores


@pytest.mark.parametrize("inputs", ["T24_B63", "T40_B90", "T48_B9_ties", "T70_B20_model"])
@pytest.mark.parametrize("k", [4, 16])
@pytest.mark.parametrize("forward", DIRS)
def test_numpy_restatement(inputs, k, forward):
    case = [c for c in EDGE_CASES if c[0] == inputs][0]
    _, T, B, kind, seed, tr = case
    score, noise = edge_inputs(T, B, kind, seed, tr)
    if B > 24:                                # the restatement is plain Python: a slice of the chains
        score, noise = score[:, :, :24].contiguous(), noise[:, :24].contiguous()
        B = 24
    st = _starts(T, B, 9, forward)
    want_segs, want_scores = _restate(score.numpy(), noise.numpy(), k, st, forward)
    paths, scores = CRF.viterbi_nbest(score, noise, k, st, forward)
    assert np.array_equal(scores.view(np.int32), want_scores.view(np.int32))
    for r in range(k):
        for c in range(B):
            got = paths[r][c]
            assert (got if got is None else list(got)) == want_segs[r][c], (r, c)


# ---- public surface, inputs and errors -------------------------------------------------------------------------------------

def test_list_form_and_evalpath():
    T, B = 24, 5
    score, noise = synth.crf_inputs(T, B, 31, "cpu", "randn")
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    paths, scores = crf.decode_nbest(4)
    assert len(paths) == 4 and all(len(p) == B for p in paths)
    assert paths[0] == crf.decode()
    for r in range(4):
        ev = crf.evalPath(paths[r]).numpy()
        assert np.allclose(ev, scores[r], atol=1e-4)
        lp = crf.logProb(paths[r]).numpy()
        assert (lp <= 1e-4).all()
    assert (scores[:-1] >= scores[1:]).all()
    pk = crf.decode_nbest_packed(4)
    assert np.array_equal(pk[2].view(np.int32), scores.view(np.int32))
    # absent ranks are None
    s1, n1 = synth.crf_inputs(2, 2, 3, "cpu", "randn")
    p1, sc1 = CRF.NeuralSemiCRFInterval(s1, n1).decode_nbest(16)
    assert all(p1[r][c] is None for r in range(8, 16) for c in range(2))
    assert all(p1[r][c] is not None for r in range(8) for c in range(2))
    assert np.isneginf(sc1[8:]).all() and np.isfinite(sc1[:8]).all()


def test_neg_inf_cells_are_present_paths():
    T, B = 5, 2
    score, noise = synth.crf_inputs(T, B, 41, "cpu", "randn")
    score = score.clone()
    score[:, :, 1] = -np.inf                     # chain 1: every path that takes an interval is -inf
    pairs, offsets, scores, npaths = CRF.viterbi_nbest_packed(score, noise, 16, None, False)
    assert (npaths == 16).all()
    dec = CRF.NeuralSemiCRFInterval(score, noise).decode_packed()
    p1, o1, _, _ = CRF.viterbi_nbest_packed(score, noise, 1, None, False)
    assert np.array_equal(p1, dec[0]) and np.array_equal(o1, dec[1])


@pytest.mark.parametrize("bad", [0, 17, -1, 2.0, 2.5, "3", True, None])
def test_bad_k(bad):
    score, noise = synth.crf_inputs(6, 2, 1, "cpu", "randn")
    with pytest.raises(ValueError):
        CRF.viterbi_nbest(score, noise, bad)


def test_bad_forced_start():
    score, noise = synth.crf_inputs(6, 2, 1, "cpu", "randn")
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    for st in ([0, 6], [-1, 0], [0]):
        with pytest.raises(IndexError):
            crf.decode_nbest(2, forcedStartPos=st)


def test_dtypes_and_layouts():
    T, B = 30, 6
    score, noise = synth.crf_inputs(T, B, 51, "cpu", "randn")
    want = CRF.viterbi_nbest_packed(score, noise, 5, None, True)
    for s2, n2 in ((score.double(), noise.double()),
                   (score.permute(2, 0, 1).contiguous().permute(1, 2, 0), noise.t().contiguous().t())):
        got = CRF.viterbi_nbest_packed(s2, n2, 5, None, True)
        for a, b in zip(got, want):
            assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                  b.view(np.int32) if b.dtype == np.float32 else b)


def test_workspace_and_ctypes_rejects_bad_k():
    lib = _lib.load()
    assert lib.semicrf_workspace_bytes(_lib.OP_VITERBI_NBEST, 1024, 4 * 352) > 0
    fake = ctypes.c_void_p(4096)                 # never dereferenced: the argument check comes first
    for k in (0, 17, -3):
        rc = lib.semicrf_viterbi_nbest(fake, fake, 8, 4, k, None, 0, fake, 64, fake, fake, fake, fake, 1 << 20, None)
        assert rc == 1 and b"k=" in lib.semicrf_last_error(), k
    rc = lib.semicrf_viterbi_nbest(fake, fake, 8, 4, 2, None, 0, fake, 64, fake, None, fake, fake, 1 << 20, None)
    assert rc == 1 and b"NULL" in lib.semicrf_last_error()


# ---- GPU: device equals host -----------------------------------------------------------------------------------------------

def _both(score, noise, k, st, forward, dev):
    host = CRF.viterbi_nbest_packed(score, noise, k, st, forward)
    devr = CRF.viterbi_nbest_packed(score.to(dev), noise.to(dev), k, st, forward)
    return host, devr


def _assert_same(host, devr, what):
    for name, a, b in zip(("pairs", "offsets", "scores", "npaths"), host, devr):
        if a.dtype == np.float32:
            a, b = a.view(np.int32), b.view(np.int32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)


@pytest.mark.gpu
@pytest.mark.parametrize("case", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_device_equals_host_edge(gpu, case):
    name, T, B, kind, seed, tr = case
    score, noise = edge_inputs(T, B, kind, seed, tr)
    for k in (1, 4, 16):
        for fwd in DIRS:
            for st in (None, _starts(T, B, k + 3 * fwd, fwd)):
                _assert_same(*_both(score, noise, k, st, fwd, gpu), (name, k, fwd, st is None))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(256, 90, "randn"), (256, 90, "model"), (256, 90, "ties"), (691, 360, "model"),
                                   (40, 1, "randn"), (40, 33, "randn"), (40, 65, "ties"), (24, 704, "randn"),
                                   (1, 5, "randn"), (2, 7, "randn")], ids=str)
def test_device_equals_host(gpu, shape):
    T, B, kind = shape
    score, noise = synth.crf_inputs(T, B, T + B, "cpu", kind)
    for k in (1, 4, 16):
        for fwd in DIRS:
            for st in (None, _starts(T, B, k + 5 * fwd, fwd)):
                _assert_same(*_both(score, noise, k, st, fwd, gpu), (shape, k, fwd, st is None))


@pytest.mark.gpu
def test_device_k1_equals_device_decode(gpu):
    T, B = 1024, 352
    score, noise = synth.crf_inputs(T, B, 61, gpu, "randn")
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    for fwd in DIRS:
        for st in (None, _starts(T, B, 8 + fwd, fwd)):
            dp, do = crf.decode_packed(forcedStartPos=st, forward=fwd)
            p, o, sc, npth = crf.decode_nbest_packed(1, forcedStartPos=st, forward=fwd)
            assert np.array_equal(p, dp) and np.array_equal(o, do) and (npth == 1).all()


@pytest.mark.gpu
def test_device_k1_reproduces_full_size_decode_digests(gpu):
    import hashlib
    g = load_golden("large_T2048_B352_decode")
    T, B, seed = (int(x) for x in g["meta"])
    score, noise = synth.crf_inputs(T, B, seed, gpu, "randn")
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    for name in ("four", "mixed"):
        st = [int(x) for x in g[f"decode_{name}_start"]]
        pairs, off, _, _ = crf.decode_nbest_packed(1, forcedStartPos=st)
        off = off.astype(np.int64)
        assert np.array_equal(off, g[f"decode_{name}_offsets"])
        h = hashlib.sha256(); h.update(off.astype("<i8").tobytes()); h.update(pairs.astype("<i4").tobytes())
        assert h.hexdigest() == str(g[f"decode_{name}_sha256"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1024, 352, 4), (2048, 88, 16)], ids=str)
def test_full_size_device_equals_host(gpu, shape):
    T, B, k = shape
    score, noise = synth.crf_inputs(T, B, 71, "cpu", "randn")
    for fwd in DIRS:
        st = _starts(T, B, 12 + fwd, fwd)
        _assert_same(*_both(score, noise, k, st, fwd, gpu), (shape, fwd))


# ---- both sides of the walk's LDS limit ------------------------------------------------------------------------------------

LOGZ_TOL = 1e-5                                               # tests/test_gpu_parity.py: the suite's tolerance for path scores

# T, B, k: the code table (T * k int32) is the last that fits the walk's 128 KB of LDS (with a ragged last workgroup of the
# sweep's four chains), the first walked in global memory, a long one in global memory, and a long row that is back in LDS
WALK_CASES = [(2048, 5, 16), (2050, 5, 16), (4100, 3, 8), (4100, 3, 4)]


def _path_scores64(score, noise, segs, B, st, forward):
    """float64 score of every path (rank-major list) over its walk's range: path_reference's sum on [lo, hi] = [0, start]
    (forward) or [start, T - 1]"""
    T = score.shape[0]
    out = np.empty(len(segs))
    for c in range(B):
        lo, hi = (0, T - 1) if st is None else ((0, st[c]) if forward else (st[c], T - 1))
        sub_s, sub_n = score[lo:hi + 1, lo:hi + 1, c:c + 1], noise[lo:hi, c:c + 1]
        for r in range(len(segs) // B):
            path = segs[r * B + c]
            assert all(lo <= b <= e <= hi for b, e in path), (r, c)
            out[r * B + c] = path_reference(sub_s, sub_n, [[(b - lo, e - lo) for b, e in path]])[0][0]
    return out


_WALK_INPUTS = {}                                             # the last shape's inputs only (200 MB at T = 4100)


def _walk_inputs(shape, gpu):
    if shape not in _WALK_INPUTS:
        _WALK_INPUTS.clear()
        T, B, k = shape
        sg, ng = synth.crf_inputs(T, B, T + k, gpu, "randn")
        _WALK_INPUTS[shape] = (sg.cpu(), ng.cpu(), sg, ng)
    return _WALK_INPUTS[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("fwd", DIRS)
@pytest.mark.parametrize("shape", WALK_CASES, ids=str)
def test_walk_lds_limit_device_equals_host(gpu, shape, fwd, forced):
    """Device == host bit for bit where the device's walk changes from a code table staged in LDS to one read from global memory
    (the host kernel has no such switch), and on the same results what needs no second kernel: rank 0 is decode, the scores
    do not increase, the paths of a chain are distinct, and every score is the float64 score of its path.  (One device call per
    case: the sweep of k = 16 takes seconds at these lengths whatever the number of chains)"""
    T, B, k = shape
    score, noise, sg, ng = _walk_inputs(shape, gpu)
    st = _starts(T, B, k + 5 * fwd, fwd) if forced else None
    what = (shape, fwd, forced)
    host = CRF.viterbi_nbest_packed(score, noise, k, st, fwd)
    devr = CRF.viterbi_nbest_packed(sg, ng, k, st, fwd)
    _assert_same(host, devr, what)
    pairs, offsets, scores, npaths = devr
    assert (npaths == k).all(), what                                      # (no start is within a few frames of the walk's end)
    dp, do = CRF.NeuralSemiCRFInterval(sg, ng).decode_packed(forcedStartPos=st, forward=fwd)
    assert np.array_equal(offsets[:B + 1], do) and np.array_equal(pairs[:offsets[B]], dp), what
    assert (scores[:-1] >= scores[1:]).all(), what
    segs = _segments(pairs, offsets)
    for c in range(B):
        assert len({tuple(segs[r * B + c]) for r in range(k)}) == k, (what, c)
    want = _path_scores64(score, noise, segs, B, st, fwd)
    assert rel_err(scores.reshape(-1), want) < LOGZ_TOL, what
    if (shape, fwd, forced) == (WALK_CASES[-1], DIRS[-1], True):
        _WALK_INPUTS.clear()
        torch.cuda.empty_cache()


@pytest.mark.gpu
def test_graph_replay(gpu):
    """semicrf_viterbi_nbest captured into a CUDA graph at the ABI level replays on new data."""
    T, B, k = 64, 40, 4
    lib = _lib.load()
    s0, n0 = synth.crf_inputs(T, B, 81, "cpu", "randn")
    s1, n1 = synth.crf_inputs(T, B, 82, "cpu", "model")
    score, noise = s0.to(gpu), n0.to(gpu)
    nB = k * B
    pairs = torch.empty(nB * 2 * T, 2, dtype=torch.int32, device=gpu)
    offsets = torch.empty(nB + 1, dtype=torch.int32, device=gpu)
    scores = torch.empty(k, B, dtype=torch.float32, device=gpu)
    npaths = torch.empty(B, dtype=torch.int32, device=gpu)
    nbytes = int(lib.semicrf_workspace_bytes(_lib.OP_VITERBI_NBEST, T, nB))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=gpu)
    stream = torch.cuda.Stream(gpu)

    def call():
        rc = lib.semicrf_viterbi_nbest(score.data_ptr(), noise.data_ptr(), T, B, k, None, 0, pairs.data_ptr(), pairs.shape[0],
                                       offsets.data_ptr(), scores.data_ptr(), npaths.data_ptr(), ws.data_ptr(), nbytes,
                                       ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
        assert rc == 0, lib.semicrf_last_error()

    with torch.cuda.stream(stream):
        call()                                   # warm-up outside the capture (function attributes)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        call()
    for s, n in ((s1, n1), (s0, n0)):
        score.copy_(s); noise.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        want = CRF.viterbi_nbest_packed(s, n, k)
        total = int(offsets[-1])
        got = (pairs[:total].cpu().numpy(), offsets.cpu().numpy(), scores.cpu().numpy(), npaths.cpu().numpy())
        _assert_same(want, got, "graph")
