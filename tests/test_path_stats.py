"""Path comparison: semicrf_compare_paths, CRF.compare_paths[_packed], NeuralSemiCRFInterval.decode_stats and
SegmentTranscriber.computeStats.

All outputs are integer counts, so every comparison is exact equality.  References: tests/golden/pathstats_small.npz holds what the
reference's own compareBracket / compareFramewise return (tools/make_pathstats_golden.py); the tolerant matching is checked against a
brute-force maximum bipartite matching written in tests/path_stats_common.py; the device kernel is held bit-equal to the host kernel
of the same contract.  CPU tests are unmarked, device tests are marked `gpu`.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from conftest import EDGE_CASES, edge_inputs, load_golden, unpack_lists
from path_stats_common import TOLERANCES, load_groups, max_matching, pack, related_lists, unpack
from transkun_amd.CRF import PathStats, compare_paths, compare_paths_packed      # (fails here without the feature)

nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")

C = PathStats


def _run(dev, lists_or_packed, T, tolerance=None):
    ep, eo, rp, ro = (t.to(dev) for t in lists_or_packed)
    return compare_paths_packed(ep, eo, rp, ro, T, tolerance).cpu().numpy()


def _packed(est, ref):
    return pack(est) + pack(ref)


# ---- the reference's counts ------------------------------------------------------------------------------------------------

def test_fixture_is_not_vacuous():
    names, groups = load_groups()
    counts = np.concatenate([g["counts"] for g in groups])
    n = len(counts)
    assert 4 * int(((counts[:, C.nExact] > 0) & (counts[:, C.nExact] < counts[:, C.nRef])).sum()) >= n
    assert 4 * int(((counts[:, C.nBothFrames] > 0) & (counts[:, C.nBothFrames] < counts[:, C.nRefFrames])).sum()) >= n
    assert 2 in [int(g["T"]) for g in groups]
    e = groups[0]
    est, ref = unpack(e["est_pairs"], e["est_offsets"]), unpack(e["ref_pairs"], e["ref_offsets"])
    at = {nm: (est[i], ref[i]) for i, nm in enumerate(names)}
    assert at["empty_estimate"][0] == [] and at["empty_estimate"][1]
    assert at["empty_reference"][1] == [] and at["empty_reference"][0]
    assert at["both_empty"] == ([], [])
    s = at["singleton_and_interval_share_begin"][0]
    assert any(a[0] == a[1] == b[0] < b[1] for a, b in zip(s, s[1:]))
    t = at["touching_intervals"][0]
    assert any(a[1] == b[0] and a[0] < a[1] and b[0] < b[1] for a, b in zip(t, t[1:]))
    (ib, ie), (ob, oe) = at["estimate_inside_reference"][0][0], at["estimate_inside_reference"][1][0]
    assert ob < ib and ie < oe


def _check_reference_pin(dev):
    _, groups = load_groups()
    for g in groups:
        arrs = [torch.from_numpy(np.ascontiguousarray(g[k])) for k in ("est_pairs", "est_offsets", "ref_pairs", "ref_offsets")]
        if arrs[0].numel() == 0:
            arrs[0] = torch.zeros(1, 2, dtype=torch.int32)
        got = _run(dev, arrs, int(g["T"]))
        assert np.array_equal(got[:, :6], g["counts"]), int(g["T"])
        assert np.array_equal(got[:, C.nMatchTol], got[:, C.nExact])


def test_reference_pin_cpu():
    """Every chain of the fixture reproduces the six counts of the reference's compareBracket / compareFramewise."""
    _check_reference_pin("cpu")


@pytest.mark.gpu
def test_reference_pin_gpu(gpu):
    _check_reference_pin(gpu)


# ---- tolerant matching -----------------------------------------------------------------------------------------------------

# heads (5, 20) / (6, 10) are incompatible at (2, 2).  The reference's head is not too late for the estimate in either coordinate,
# so IT is dropped and (5, 20) meets (7, 20).  A walk that drops the head with the smaller begin (the estimate) ends with one match.
GREEDY_EST = [(5, 20), (8, 21)]
GREEDY_REF = [(6, 10), (7, 20), (8, 23)]
# the mirror image: the reference's head (5, 20) ends too late for (6, 10), so the estimate's head is dropped
GREEDY2_EST = [(6, 10), (7, 20)]
GREEDY2_REF = [(5, 20)]


def _matching_cases():
    cases = []
    for T, seed in ((24, 1), (17, 2), (9, 3), (2, 4)):
        est, ref = related_lists(T, 64, seed)
        cases.append((T, est, ref))
    cases.append((24, [GREEDY_EST, GREEDY2_EST, GREEDY_REF], [GREEDY_REF, GREEDY2_REF, GREEDY_EST]))
    return cases


_BRUTE = {}


def _brute(i, tol, est, ref):
    key = (i, tol)
    if key not in _BRUTE:
        _BRUTE[key] = np.asarray([max_matching(e, r, *tol) for e, r in zip(est, ref)])
    return _BRUTE[key]


def _check_tolerant(dev):
    better, total = 0, 0
    for i, (T, est, ref) in enumerate(_matching_cases()):
        packed = _packed(est, ref)
        exact = None
        for tol in TOLERANCES:
            got = _run(dev, packed, T, tol)
            want = _brute(i, tol, est, ref)
            assert np.array_equal(got[:, C.nMatchTol], want), (T, tol)
            if tol == (0, 0):
                exact = got[:, C.nExact].copy()
            assert np.array_equal(got[:, C.nExact], exact) and np.array_equal(exact, _brute(i, (0, 0), est, ref))
            if tol == (2, 2) and T > 2:
                better += int((got[:, C.nMatchTol] > got[:, C.nExact]).sum())
                total += len(est)
    assert 4 * better >= total, (better, total)


def test_tolerant_matching_is_maximum_cpu():
    """nMatchTol equals a brute-force maximum bipartite matching at every tolerance; (0, 0) equals nExact; a quarter of the chains
    gain matches at (2, 2)."""
    _check_tolerant("cpu")


@pytest.mark.gpu
def test_tolerant_matching_is_maximum_gpu(gpu):
    _check_tolerant(gpu)


def _check_drop_rule(dev):
    got = _run(dev, _packed([GREEDY_EST, GREEDY2_EST], [GREEDY_REF, GREEDY2_REF]), 24, (2, 2))
    assert got[:, C.nMatchTol].tolist() == [2, 1]
    assert max_matching(GREEDY_EST, GREEDY_REF, 2, 2) == 2 and max_matching(GREEDY2_EST, GREEDY2_REF, 2, 2) == 1
    assert got[:, C.nExact].tolist() == [0, 0]


def test_drop_rule_cpu():
    """Hand-built chains where dropping the wrong head of an incompatible pair loses a match."""
    _check_drop_rule("cpu")


@pytest.mark.gpu
def test_drop_rule_gpu(gpu):
    _check_drop_rule(gpu)


# ---- contract edges --------------------------------------------------------------------------------------------------------

T_EDGE = 12
GOOD = [(0, 3), (3, 3), (5, 9)]
BAD = {"begin_after_end": [(0, 3), (6, 5)], "index_equals_T": [(0, 3), (5, T_EDGE)], "decreasing_end": [(0, 6), (2, 5)],
       "decreasing_begin": [(4, 6), (3, 8)], "negative_index": [(-1, 3)]}


def _check_invalid_chains(dev):
    other = [[(0, 2)], [], GOOD, [(1, 1)], [(0, 11)], [(2, 2), (2, 4)], GOOD]
    lists = [GOOD] + list(BAD.values()) + [GOOD[:2]]
    clean = [l if i in (0, len(lists) - 1) else [] for i, l in enumerate(lists)]
    for side in ("est", "ref"):
        if side == "est":
            got, want = _run(dev, _packed(lists, other), T_EDGE, (1, 1)), _run(dev, _packed(clean, other), T_EDGE, (1, 1))
        else:
            got, want = _run(dev, _packed(other, lists), T_EDGE, (1, 1)), _run(dev, _packed(other, clean), T_EDGE, (1, 1))
        for i in range(len(lists)):
            if 0 < i < len(lists) - 1:
                assert (got[i] == -1).all(), (side, list(BAD)[i - 1], got[i])
            else:
                assert (got[i] >= 0).all() and np.array_equal(got[i], want[i]), (side, i)


def test_invalid_chains_cpu():
    """begin > end, an index equal to T, a decreasing end (or begin), a negative index: -1 for that chain only."""
    _check_invalid_chains("cpu")


@pytest.mark.gpu
def test_invalid_chains_gpu(gpu):
    _check_invalid_chains(gpu)


def _check_negative_total(dev):
    est, ref = related_lists(T_EDGE, 5, 9)
    for which in (1, 3):
        packed = list(_packed(est, ref))
        packed[which] = packed[which].clone()
        packed[which][-1] = -1
        assert (_run(dev, packed, T_EDGE) == -1).all()
    # offsets that leave [0, total]: those chains only
    packed = list(_packed(est, ref))
    o = packed[1].clone()
    o[2] = o[-1] + 3
    packed[1] = o
    got, want = _run(dev, packed, T_EDGE), _run(dev, _packed(est, ref), T_EDGE)
    assert (got[1] == -1).all() and (got[2] == -1).all() and np.array_equal(got[[0, 3, 4]], want[[0, 3, 4]])


def test_negative_total_cpu():
    """A negative offsets[B] on either side (the marker of a decode that gave up) gives -1 everywhere."""
    _check_negative_total("cpu")


@pytest.mark.gpu
def test_negative_total_gpu(gpu):
    _check_negative_total(gpu)


@pytest.mark.gpu
def test_total_beyond_the_buffer_is_not_read(gpu):
    """A device-side total larger than the pairs tensor cannot be checked on the host without a synchronisation: the mirror turns
    it into the invalid marker on the device."""
    est, ref = related_lists(T_EDGE, 5, 9)
    ep, eo, rp, ro = (t.to(gpu) for t in _packed(est, ref))
    got = compare_paths_packed(ep[:int(eo[-1]) - 1], eo, rp, ro, T_EDGE)
    assert bool((got == -1).all())


def _check_bad_arguments(dev):
    est, ref = related_lists(T_EDGE, 4, 10)
    ep, eo, rp, ro = (t.to(dev) for t in _packed(est, ref))
    for bad in (9, (0, 9), (9, 0), -1, (1, 2, 3), 1.5, True):
        with pytest.raises(ValueError):
            compare_paths_packed(ep, eo, rp, ro, T_EDGE, bad)
    with pytest.raises(ValueError):
        compare_paths(est, ref, T_EDGE, tolerance=9)
    # unaligned pairs: a view that starts 4 bytes into an aligned buffer
    buf = torch.zeros(2 * ep.shape[0] + 2, dtype=torch.int32, device=dev)
    assert buf.data_ptr() % 8 == 0
    un = buf[1:1 + 2 * ep.shape[0]].view(-1, 2)
    un.copy_(ep)
    assert un.is_contiguous() and un.data_ptr() % 8 == 4
    stats = torch.full((4, 7), 77, dtype=torch.int32, device=dev)
    ops = nsci._lib.ops()
    for args in ((un, eo, rp, ro), (rp, ro, un, eo)):
        with pytest.raises(ValueError, match="8-byte aligned"):
            compare_paths_packed(*args, T_EDGE)
        with pytest.raises(RuntimeError, match="8-byte aligned"):
            ops.compare_paths(*args, T_EDGE, 0, 0, stats)
    # dtypes: nothing is converted
    for k in range(4):
        args = [ep, eo, rp, ro]
        args[k] = args[k].long()
        with pytest.raises(TypeError, match="int32"):
            compare_paths_packed(*args, T_EDGE)
        with pytest.raises(RuntimeError, match="dtype"):
            ops.compare_paths(*args, T_EDGE, 0, 0, stats)
    with pytest.raises(RuntimeError):
        ops.compare_paths(ep, eo, rp, ro, T_EDGE, 9, 0, stats)
    with pytest.raises(RuntimeError):
        ops.compare_paths(ep, eo, rp, ro[:-1], T_EDGE, 0, 0, stats)
    with pytest.raises(RuntimeError):
        ops.compare_paths(ep, eo, rp, ro, T_EDGE, 0, 0, stats[:3])
    with pytest.raises(ValueError):
        compare_paths_packed(ep, eo, rp, ro[:-1], T_EDGE)
    with pytest.raises(ValueError):
        compare_paths_packed(ep.t().contiguous().t(), eo, rp, ro, T_EDGE)
    if dev != "cpu":
        torch.cuda.synchronize(dev)
    assert bool((stats == 77).all()), "a rejected call wrote to its output"


def test_bad_arguments_cpu():
    """A tolerance of 9, unaligned or non-int32 inputs and short buffers raise, before anything runs."""
    _check_bad_arguments("cpu")


@pytest.mark.gpu
def test_bad_arguments_gpu(gpu):
    _check_bad_arguments(gpu)


def test_c_abi_rejects_bad_arguments():
    """semicrf_compare_paths checks its arguments before it launches: no GPU needed to see SEMICRF_EINVAL."""
    lib = nsci._lib.load()
    p = ctypes.c_void_p(4096)               # never dereferenced: the argument checks come first
    ok = (p, p, p, p, 16, 4)
    for tb, te in ((9, 0), (0, 9), (-1, 0), (0, -1)):
        assert lib.semicrf_compare_paths(*ok, tb, te, p, None) == 1 and b"tolerance" in lib.semicrf_last_error()
    assert lib.semicrf_compare_paths(ctypes.c_void_p(4100), p, p, p, 16, 4, 0, 0, p, None) == 1 and b"aligned" in lib.semicrf_last_error()
    assert lib.semicrf_compare_paths(p, p, ctypes.c_void_p(4100), p, 16, 4, 0, 0, p, None) == 1 and b"aligned" in lib.semicrf_last_error()
    assert lib.semicrf_compare_paths(p, None, p, p, 16, 4, 0, 0, p, None) == 1
    assert lib.semicrf_compare_paths(p, p, p, p, 0, 4, 0, 0, p, None) == 1
    assert lib.semicrf_compare_paths(p, p, p, p, 16, 0, 0, 0, p, None) == 1
    assert lib.semicrf_abi_version() == 2


def test_lists_entry_point():
    est = [[(0, 2), (4, 6), (6, 6), (7, 8)], [], [(1, 1)]]
    ref = [[(0, 2), (4, 5), (6, 6), (7, 9)], [(0, 0)], []]
    got = compare_paths(est, ref, 10, tolerance=1)
    assert got.dtype == torch.int32 and got.tolist() == [[4, 4, 2, 9, 8, 8, 4], [1, 0, 0, 1, 0, 0, 0], [0, 1, 0, 0, 1, 0, 0]]
    assert tuple(C) == tuple(range(7)) and C._fields == ("nRef", "nEst", "nExact", "nRefFrames", "nEstFrames", "nBothFrames", "nMatchTol")
    with pytest.raises(ValueError):
        compare_paths([[(3, 2)]], [[]], 10)
    with pytest.raises(IndexError):
        compare_paths([[(3, 10)]], [[]], 10)


# ---- device against the host kernel ----------------------------------------------------------------------------------------

_SHAPE_LISTS = {}


def _shape_lists(T):
    """352 chains per frame count, generated once; smaller batches are prefixes (the first chains differ from case to case in
    length, so a prefix is not a special case)."""
    if T not in _SHAPE_LISTS:
        est, ref = related_lists(T, 352, 100 + T, density=0.6)
        est[3], ref[5] = [], []
        host = {tol: compare_paths_packed(*_packed(est, ref), T, tol).numpy() for tol in ((0, 0), (2, 1))}
        _SHAPE_LISTS[T] = (est, ref, host)
    return _SHAPE_LISTS[T]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [2, 33, 256])
@pytest.mark.parametrize("B", [1, 2, 63, 65, 352])
def test_device_equals_host(gpu, B, T):
    est, ref, host = _shape_lists(T)
    packed = _packed(est[:B], ref[:B])
    for tol in ((0, 0), (2, 1)):
        assert np.array_equal(_run(gpu, packed, T, tol), host[tol][:B]), tol


def _ctypes_call(lib, ep, eo, rp, ro, T, tol, stats):
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(stats.device).cuda_stream)
    return lib.semicrf_compare_paths(vp(ep), vp(eo), vp(rp), vp(ro), T, eo.numel() - 1, tol[0], tol[1], vp(stats), st)


@pytest.mark.gpu
def test_ctypes_and_torch_op_agree(gpu):
    """The same bits through the C ABI (ctypes) and through torch.ops.semicrf, with guard words behind the output."""
    T, B = 33, 65
    est, ref, host = _shape_lists(T)
    ep, eo, rp, ro = (t.to(gpu) for t in _packed(est[:B], ref[:B]))
    lib = nsci._lib.load()
    for tol in ((0, 0), (2, 1)):
        a = torch.full((B + 1, 7), 12345, dtype=torch.int32, device=gpu)
        b = torch.full((B + 1, 7), 12345, dtype=torch.int32, device=gpu)
        assert _ctypes_call(lib, ep, eo, rp, ro, T, tol, a) == 0, lib.semicrf_last_error()
        nsci._lib.ops().compare_paths(ep, eo, rp, ro, T, tol[0], tol[1], b[:B])
        torch.cuda.synchronize(gpu)
        assert torch.equal(a, b) and bool((a[B] == 12345).all())
        assert np.array_equal(a[:B].cpu().numpy(), host[tol][:B])
    # a path compared with itself (the same buffers on both sides; the reference lists are paths, the estimates need not be)
    s = torch.empty(B, 7, dtype=torch.int32, device=gpu)
    assert _ctypes_call(lib, rp, ro, rp, ro, T, (0, 0), s) == 0
    s = s.cpu().numpy()
    assert np.array_equal(s, compare_paths_packed(*_packed(ref[:B], ref[:B]), T).numpy())
    assert np.array_equal(s[:, C.nExact], s[:, C.nRef]) and np.array_equal(s[:, C.nBothFrames], s[:, C.nRefFrames])
    assert nsci._lib.device_status() == 0


@pytest.mark.gpu
def test_compare_paths_graph_capture_replays(gpu):
    """The comparison can be captured into a HIP graph and replayed on new lists: it has no workspace and no host-side state."""
    T, B = 33, 65
    est, ref, host = _shape_lists(T)
    tol = (2, 1)
    sets = [_packed(est[:B], ref[:B]), _packed(ref[:B], est[:B]), _packed(est[B:2 * B], ref[B:2 * B])]
    want = [compare_paths_packed(*s, T, tol) for s in sets]
    cap = max(s[0].shape[0] for s in sets), max(s[2].shape[0] for s in sets)
    ep = torch.zeros(cap[0], 2, dtype=torch.int32, device=gpu); rp = torch.zeros(cap[1], 2, dtype=torch.int32, device=gpu)
    eo = torch.zeros(B + 1, dtype=torch.int32, device=gpu); ro = torch.zeros(B + 1, dtype=torch.int32, device=gpu)

    def load(s):
        ep[:s[0].shape[0]].copy_(s[0]); eo.copy_(s[1]); rp[:s[2].shape[0]].copy_(s[2]); ro.copy_(s[3])
    load(sets[0])
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        for _ in range(2):
            compare_paths_packed(ep, eo, rp, ro, T, tol)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        stats = compare_paths_packed(ep, eo, rp, ro, T, tol)
    for i in (1, 2, 0, 0, 1):
        load(sets[i])
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(stats.cpu(), want[i]), i
    assert torch.equal(compare_paths_packed(ep, eo, rp, ro, T, tol).cpu(), want[1])
    assert nsci._lib.device_status() == 0


# ---- decode_stats ----------------------------------------------------------------------------------------------------------

def _decode_stats_inputs(name, dev):
    from transkun_amd import synth
    if name == "edge_T48_B9_ties":
        case = [c for c in EDGE_CASES if c[0] == "T48_B9_ties"][0]
        score, noise = edge_inputs(*case[1:], dev)
    else:
        g = load_golden(name)
        T, B, seed = (int(x) for x in g["meta"])
        score, noise = synth.crf_inputs(T, B, seed, dev, "model")
    g = load_golden(name)
    return score, noise, unpack_lists(g["intervals_pairs"], g["intervals_offsets"]), [int(x) for x in g["decode_mixed_bwd_start"]]


def _check_decode_stats(name, dev):
    from transkun_amd import CRF
    score, noise, iv, start = _decode_stats_inputs(name, dev)
    T = score.shape[0]
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    nonzero = 0
    for forced in (None, start):
        for forward in (False, True):
            for tol in (None, (2, 2)):
                got = crf.decode_stats(iv, forcedStartPos=forced, forward=forward, tolerance=tol)
                assert got.device == score.device and got.dtype == torch.int32 and tuple(got.shape) == (len(iv), 7)
                want = compare_paths(crf.decode(forced, forward), iv, T, tolerance=tol)
                assert torch.equal(got.cpu(), want), (forced is not None, forward, tol)
                nonzero += int(got[:, C.nExact].sum()) + int(got[:, C.nBothFrames].sum())
    assert nonzero > 0
    if score.is_cuda:
        assert nsci._lib.device_status() == 0


def test_decode_stats_cpu():
    """decode_stats == compare_paths(decode(), intervals), with and without forcedStartPos, on the host kernels."""
    _check_decode_stats("edge_T48_B9_ties", "cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge_T48_B9_ties", "medium_T256_B90_model"])
def test_decode_stats_gpu(gpu, name):
    nsci._lib.set_impl(0)
    _check_decode_stats(name, gpu)


@pytest.mark.gpu
def test_decode_stats_single_chain(gpu):
    """One chain decodes with a ghost chain appended; the comparison sees the real chain only."""
    from transkun_amd import CRF, synth
    nsci._lib.set_impl(0)
    score, noise = synth.crf_inputs(40, 1, 77, gpu)
    crf = CRF.NeuralSemiCRFInterval(score, noise)
    iv = [[(0, 3), (3, 9), (12, 12), (20, 39)]]
    assert torch.equal(crf.decode_stats(iv, tolerance=1).cpu(), compare_paths(crf.decode(), iv, 40, tolerance=1))
    assert nsci._lib.device_status() == 0


# ---- SegmentTranscriber.computeStats ---------------------------------------------------------------------------------------

def _stats_model(gpu, N=2, P=10, T=70, D=64):
    from transkun_amd import synth
    from transkun_amd.transcribe import SegmentTranscriber
    torch.manual_seed(11)
    tr = SegmentTranscriber(D, 48, 48, targetMIDIPitch=list(range(P))).to(gpu).eval()
    ctx = synth.hash_normal(N * P * T * D, 31, gpu).view(N, P, T, D).contiguous()
    return tr, ctx


def _nested(flat, N, P):
    return [[flat[n * P + p] for p in range(P)] for n in range(N)]


@pytest.mark.gpu
def test_compute_stats(gpu):
    """At T=70 x 20 chains with random heads: the six counts are column sums of decode_stats on the scorer's output, and the two
    squared errors equal a float64 restatement of ModelTransformer.py:454-481 within K * 2^-24 relative (the bound of an fp32 sum
    of K non-negative terms, K = the number of target intervals)."""
    from transkun_amd import CRF, attributes
    nsci._lib.set_impl(0)
    N, P, T, D = 2, 10, 70, 64
    tr, ctx = _stats_model(gpu, N, P, T, D)
    g = load_golden("edge_T70_B20_model")
    iv = unpack_lists(g["intervals_pairs"], g["intervals_offsets"])
    K = sum(len(l) for l in iv)
    assert K == 117 and len(iv) == N * P
    rng = np.random.default_rng(3)
    vel = [[int(v) for v in rng.integers(0, 128, len(l))] for l in iv]
    ofs = [[(float(a), float(b)) for a, b in rng.uniform(-0.5, 0.5, (len(l), 2))] for l in iv]
    res = tr.computeStats(ctx, _nested(iv, N, P), _nested(vel, N, P), _nested(ofs, N, P), tolerance=(2, 2))
    assert list(res) == ["nGT", "nEst", "nCorrect", "nGTFramewise", "nEstFramewise", "nCorrectFramewise", "seVelocityForced", "seOFForced",
                         "nCorrectTolerant"]
    with torch.no_grad():
        S, b = tr.scorer(ctx)
        crf = CRF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1))
        sums = crf.decode_stats(iv, tolerance=(2, 2)).sum(0).tolist()
        assert sums == [res[k] for k in ("nGT", "nEst", "nCorrect", "nGTFramewise", "nEstFramewise", "nCorrectFramewise", "nCorrectTolerant")]
        assert res["nGT"] == K and res["nEst"] > 0 and all(isinstance(res[k], int) for k in list(res)[:6])
        # the two heads on the target intervals, in float64
        pairs, offsets = nsci.pack_intervals(iv, T, N * P, gpu)
        x, _, _ = attributes.attribute_input_packed(ctx, pairs, offsets, K)
        x = x.double()
        import copy
        vp, op = copy.deepcopy(tr.velocityPredictor).double(), copy.deepcopy(tr.refinedOFPredictor).double()
        p = torch.softmax(vp(x), dim=-1)
        velocity = (p * torch.arange(128, device=gpu, dtype=torch.float64)).sum(-1)
        ofv, _ = op(x).chunk(2, dim=-1)
        mean = torch.distributions.ContinuousBernoulli(logits=ofv, validate_args=False).mean
        ofv = torch.clamp((mean - 0.5) / 0.99, -0.5, 0.5)
        vel_gt = torch.tensor([v for l in vel for v in l], dtype=torch.float64, device=gpu)
        of_gt = torch.tensor([v for l in ofs for v in l], dtype=torch.float32, device=gpu).double()    # (the targets are fp32 tensors)
        se_v = float((velocity - vel_gt).pow(2).sum())
        se_of = float((ofv - of_gt).pow(2).sum())
    bound = K * 2.0 ** -24
    print(f"seVelocityForced {res['seVelocityForced']!r} vs {se_v!r}: rel {abs(res['seVelocityForced'] - se_v) / se_v:.3e}; "
          f"seOFForced {res['seOFForced']!r} vs {se_of!r}: rel {abs(res['seOFForced'] - se_of) / se_of:.3e}; bound {bound:.3e}")
    assert se_v > 0 and se_of > 0
    assert abs(res["seVelocityForced"] - se_v) <= bound * se_v
    assert abs(res["seOFForced"] - se_of) <= bound * se_of
    # without a tolerance the reference's eight keys, the same numbers; flat targets are taken as well
    res2 = tr.computeStats(ctx, _nested(iv, N, P), [v for l in vel for v in l], torch.tensor([v for l in ofs for v in l]))
    assert list(res2) == list(res)[:8] and all(res2[k] == res[k] for k in res2)
    assert nsci._lib.device_status() == 0


@pytest.mark.gpu
def test_compute_stats_empty_target(gpu):
    """No target interval at all: the counts still come from the decode, both errors are 0 and the heads are not run."""
    nsci._lib.set_impl(0)
    N, P, T, D = 2, 10, 70, 64
    tr, ctx = _stats_model(gpu, N, P, T, D)
    calls = []
    hooks = [m.register_forward_hook(lambda *a: calls.append(1)) for m in (tr.velocityPredictor, tr.refinedOFPredictor)]
    empty = [[[] for _ in range(P)] for _ in range(N)]
    try:
        res = tr.computeStats(ctx, empty, empty, empty)
    finally:
        for h in hooks:
            h.remove()
    assert calls == []
    assert res["seVelocityForced"] == 0.0 and res["seOFForced"] == 0.0
    assert res["nGT"] == res["nCorrect"] == res["nGTFramewise"] == res["nCorrectFramewise"] == 0
    assert res["nEst"] > 0 and res["nEstFramewise"] >= res["nEst"] // 2
    assert nsci._lib.device_status() == 0
