"""The backbone's feed-forward ResBlock on the bf16 matrix instruction (transkun_amd.backbone.feed_forward_residual with bf16 = "fused";
torch.ops.semicrf.ffn_residual_bf16 on bfloat16 tensors -- form A -- and ffn_residual_bf16_mixed on float32 tensors under bfloat16
autocast -- form B; csrc/ffn_bf16.hip on the device, the host mirrors of csrc/cpu_ops.cpp on the CPU).

1. exact answers: closed-form inputs that the chain of csrc/ffn_bf16_math.h reproduces bit for bit, whole op and layer 1 alone; a walk
   that stops one hidden chunk early fails them exactly where there is more than one chunk
2. gates: every width x hidden size x row count x LayerScale x input scale against float64, gated by the stock route's own error
3. every instantiation of the kernel, in both forms, aligned and one element off 16 bytes
4. bits: a row's result whatever the batch; strided views without a copy; non-finite rows stay put; nothing outside `out` is written
5. entry points: the supported set, rejected calls, graph capture
6. routing, read from the counters;  7. the modules against float64
Measured numbers: DESIGN.md section 3, "Backbone feed-forward, bf16", and profiles/feed_forward_bf16_bench.json.
"""
import ctypes

import pytest
import torch

import backbone_bf16_common
import backbone_common
import ffn_bf16_common as c16
import ffn_common

CPU = torch.device("cpu")
BF16 = torch.bfloat16
R, C = c16.tiles()
FORMS = c16.FORMS


# ---- 1. exact answers -------------------------------------------------------------------------------------------------------------------
def _check_exact(dev, form, rows, D, hidden):
    c = c16.exact_case(form, rows, D, hidden)
    got = c16.run(c, dev).cpu()
    assert float(c["want"].double().abs().max()) < 64
    assert c16.bits_equal(got, c["want"]), (form, rows, D, hidden, float((got.double() - c["want"].double()).abs().max()))
    for off in c16.probe_offsets(D, hidden):                 # layer 1 alone, per hidden column
        p = c16.exact_case(form, rows, D, hidden, probe=off)
        assert c16.bits_equal(c16.run(p, dev).cpu(), p["want"]), (form, rows, D, hidden, off)


def test_exact_shapes_reach_the_edges():
    assert c16.EXACT_ROWS_SHORT == R - 1 and (R, C) == (64, 64)


@pytest.mark.parametrize("rows,D,hidden", c16.EXACT_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_exact_answers_cpu(form, rows, D, hidden):
    _check_exact(CPU, form, rows, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,hidden", c16.EXACT_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_exact_answers_gpu(gpu, form, rows, D, hidden):
    _check_exact(gpu, form, rows, D, hidden)


@pytest.mark.parametrize("form", FORMS)
def test_skipping_the_last_chunk_fails_the_exact_answers(monkeypatch, form):
    """A host mirror that leaves out the last hidden chunk misses the exact answer at every shape with hidden > C and at none with
    hidden <= C (there the walk has one chunk and the flag changes nothing)."""
    monkeypatch.setattr(c16, "SKIP_LAST_CHUNK", True)
    for rows, D, hidden in c16.EXACT_SHAPES:
        c = c16.exact_case(form, rows, D, hidden)
        assert c16.bits_equal(c16.run(c, CPU), c["want"]) == (hidden <= C), (form, rows, D, hidden)


# ---- 2. gates ---------------------------------------------------------------------------------------------------------------------------
def _check_gate(dev, form, D, hidden):
    worst = (0.0, 0.0)
    for rows in ffn_common.row_counts():
        for kind in ffn_common.SCALE_KINDS:
            for mult in ffn_common.INPUT_SCALES:
                c = c16.case(form, rows, D, hidden, kind, mult)
                share, ratio = c16.gated(c16.run(c, dev), c, f"rows {rows} D {D} hidden {hidden} scale {kind} x{mult:g}")
                worst = max(worst, (share, ratio))
    print(f"worst share of the gate {worst[0]:.2f} (ratio to the stock route there {worst[1]:.2f})")


@pytest.mark.parametrize("hidden", ffn_common.hidden_sizes())
@pytest.mark.parametrize("D", ffn_common.WIDTHS)
@pytest.mark.parametrize("form", FORMS)
def test_op_gate_cpu(form, D, hidden):
    _check_gate(CPU, form, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", ffn_common.hidden_sizes())
@pytest.mark.parametrize("D", ffn_common.WIDTHS)
@pytest.mark.parametrize("form", FORMS)
def test_op_gate_gpu(gpu, form, D, hidden):
    _check_gate(gpu, form, D, hidden)


# ---- 3. every instantiation -----------------------------------------------------------------------------------------------------------------
def _matrix(dev, form, D, aligned):
    """One instantiation <element type, column blocks of 32>, with 16-byte or element loads: three row tiles, the last of one row; two
    hidden chunks, the second of 8 columns."""
    c = c16.case(form, 2 * R + 1, D, C + 8, "randn", 1.0)
    x = c["x"].to(dev)
    if not aligned:
        x = c16.one_off(x)
    got = c16.run(c, dev, x)
    c16.gated(got, c, f"D {D} {'aligned' if aligned else 'one element off'}")
    assert c16.bits_equal(got.cpu(), c16.run(c, dev).cpu())                # the two load widths give the same bits


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("D", ffn_common.MATRIX_WIDTHS)
@pytest.mark.parametrize("form", FORMS)
def test_op_instantiation_matrix_cpu(form, D, aligned):
    _matrix(CPU, form, D, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("D", ffn_common.MATRIX_WIDTHS)
@pytest.mark.parametrize("form", FORMS)
def test_op_instantiation_matrix_gpu(gpu, form, D, aligned):
    _matrix(gpu, form, D, aligned)


# ---- 4. independence and layout, bit for bit ------------------------------------------------------------------------------------------------
BIT_SHAPES = [(160, 640), (80, C + 8), (256, 1024), (8, 8)]


def _check_row_independence(dev, form):
    """A row's bits are the same alone, in a batch of 3 and in a batch of 2R + 1, wherever it stands."""
    for D, hidden in BIT_SHAPES:
        c = c16.case(form, 2 * R + 1, D, hidden, "randn", 1.0)
        full = c16.run(c, dev).cpu()
        for r in (0, R - 1, R, 2 * R):
            alone = c16.run(c, dev, c["x"][r:r + 1]).cpu()
            assert c16.bits_equal(alone[0], full[r]), (form, D, hidden, r)
            lo = min(r, 2 * R - 2)
            three = c16.run(c, dev, c["x"][lo:lo + 3]).cpu()
            assert c16.bits_equal(three[r - lo], full[r]), (form, D, hidden, r)


@pytest.mark.parametrize("form", FORMS)
def test_row_independence_cpu(form):
    _check_row_independence(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_row_independence_gpu(gpu, form):
    _check_row_independence(gpu, form)


def _check_strided_views(dev, form):
    """The [N, T', F', D] buffer, its transpose(-3, -2) view, a view one element off a 16-byte boundary (an odd row stride) and rows
    with gaps give the contiguous call's bits; the result is laid out like x."""
    for D, hidden in BIT_SHAPES[:2]:
        c = c16.case(form, 0, D, hidden, "randn", 1.0, lead=(2, 5, 7))
        x = c["x"].to(dev)
        want = c16.run(c, dev, x)
        xt = x.transpose(-3, -2)                                         # BasicBlock's attention = "torch" order
        got = c16.run(c, dev, xt)
        assert got.shape == xt.shape and got.stride() == xt.stride()
        assert c16.bits_equal(got.transpose(-3, -2).cpu(), want.cpu())
        assert c16.bits_equal(c16.run(c, dev, xt.contiguous()).transpose(-3, -2).cpu(), want.cpu())
        off = c16.one_off(x)
        assert off.stride(-2) % 2 == 1
        assert c16.bits_equal(c16.run(c, dev, off).cpu(), want.cpu())
        # the raw op on a [n0, n1, D] view with two real row strides, into an `out` with strides of its own
        v = x[0].transpose(0, 1)                                         # [7, 5, D], strides (D, 7 D)
        out = torch.full((7, 5, D + 3), float("nan"), device=dev, dtype=x.dtype)[..., :D]
        c16.raw_op(form, v, tuple(p.to(dev) for p in c["params"]), c["eps"], out)
        assert c16.bits_equal(out.transpose(0, 1).cpu(), want[0].cpu())


@pytest.mark.parametrize("form", FORMS)
def test_strided_views_cpu(form):
    _check_strided_views(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_strided_views_gpu(gpu, form):
    _check_strided_views(gpu, form)


def _check_non_finite_stay_put(dev, form):
    """A NaN or an infinity in one row reaches that row only; every other row keeps the clean run's bits."""
    for D, hidden in BIT_SHAPES[:3]:
        c = c16.case(form, 2 * R + 1, D, hidden, "randn", 1.0)
        clean = c16.run(c, dev).cpu()
        for bad in (float("nan"), float("inf")):
            x = c["x"].clone()
            hit = [1, R, 2 * R]
            for r in hit:
                x[r, (3 * r) % D] = bad
            got = c16.run(c, dev, x).cpu()
            keep = torch.ones(x.shape[0], dtype=torch.bool)
            keep[hit] = False
            assert c16.bits_equal(got[keep], clean[keep]), (form, D, hidden, bad)
            assert not bool(torch.isfinite(got[hit]).all(dim=-1).any())   # the rows that were hit show it


@pytest.mark.parametrize("form", FORMS)
def test_non_finite_stay_put_cpu(form):
    _check_non_finite_stay_put(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_non_finite_stay_put_gpu(gpu, form):
    _check_non_finite_stay_put(gpu, form)


def _check_poison(dev, form):
    """NaN behind the last row of x, behind the last hidden row of W1 and b1, and behind W2, b2 and scale is never read into a result,
    and a sentinel around `out` (in front, behind, and in the gaps between its rows) is never overwritten."""
    dt = c16.dtype_of(form)
    for D, hidden in BIT_SHAPES[:3]:
        for rows in (1, R - 1, R + 1):
            c = c16.case(form, rows, D, hidden, "randn", 1.0)
            want = c16.run(c, dev).cpu()
            buf = torch.full((rows + 2 * R, D), float("nan"), device=dev, dtype=dt)
            buf[:rows] = c["x"].to(dev)
            params = []
            for p in c["params"]:                                         # every parameter in front of a stretch of NaN
                room = torch.full((p.numel() + 4096,), float("nan"), device=dev, dtype=dt)
                room[:p.numel()] = p.to(dev).reshape(-1)
                params.append(room[:p.numel()].view(p.shape))
            pitch = D + 5
            obuf = torch.full((rows + 2, pitch), 7.5, device=dev, dtype=dt)
            out = obuf[1:rows + 1, 2:2 + D]
            c16.raw_op(form, buf[:rows].unsqueeze(0), tuple(params), c["eps"], out.unsqueeze(0))
            assert c16.bits_equal(out.cpu(), want), (form, D, hidden, rows)
            mask = torch.ones_like(obuf, dtype=torch.bool)
            mask[1:rows + 1, 2:2 + D] = False
            assert bool((obuf[mask] == 7.5).all()), (form, D, hidden, rows)


@pytest.mark.parametrize("form", FORMS)
def test_poison_cpu(form):
    _check_poison(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_poison_gpu(gpu, form):
    _check_poison(gpu, form)


def _count_copies(blk, lin):
    from torch.utils._python_dispatch import TorchDispatchMode
    n_hidden = lin.numel()

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.copies = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = func.overloadpacket.__name__
            if name in ("clone", "contiguous", "_to_copy", "copy_") and isinstance(out, torch.Tensor) and out.numel() >= n_hidden:
                self.copies.append((name, tuple(out.shape), tuple(args[0].stride())))
            return out

    with torch.no_grad(), Count() as c:
        blk(lin)
    return c.copies


def test_fused_bf16_feed_forward_adds_no_copy():
    """Counted as test_feed_forward.test_fused_feed_forward_adds_no_copy counts: a bf16 BasicBlock with every fused route on copies
    no hidden-state-sized tensor, in either attention order no more than with feedForwardBf16 = "torch"."""
    from transkun_amd import backbone
    m16, _, fx = backbone_bf16_common.bf16_backbone("backbone_d40", CPU)
    blk = m16.encoderLayers[0]
    lin = fx["layer_in"].bfloat16()
    blk.attentionBf16, blk.feedForward = "fused", "fused"
    counts = {}
    for attention in ("fused", "torch"):
        for kind in ("torch", "fused"):
            blk.attention, blk.feedForwardBf16 = attention, kind
            before = dict(backbone.FEED_FORWARD_BF16_ROUTES)
            counts[attention, kind] = _count_copies(blk, lin)
            assert backbone.FEED_FORWARD_BF16_ROUTES["fused"] == before["fused"] + (2 if kind == "fused" else 0)
    assert counts["fused", "fused"] == []
    assert len(counts["torch", "fused"]) <= len(counts["torch", "torch"])
    assert len(counts["torch", "torch"]) > 0                             # the counter sees the stock route's copies


# ---- 5. entry points ------------------------------------------------------------------------------------------------------------------------
def test_supported_set_and_constants():
    from transkun_amd import _lib, backbone
    assert (R, C) == (_lib.FFN_BF16_ROW_TILE, _lib.FFN_BF16_HIDDEN_CHUNK)
    lib = _lib.load()
    for D, hidden, ok in ((8, 8, True), (256, 4096, True), (160, 640, True), (0, 8, False), (264, 8, False), (12, 8, False), (8, 7, False),
                          (8, 4104, False), (8, 0, False), (-8, 8, False)):
        assert backbone.feed_forward_bf16_supported(D, hidden) == ok, (D, hidden)
        assert backbone.feed_forward_supported(D, hidden) == ok
        assert bool(lib.semicrf_ffn_residual_bf16_supported(D, hidden)) == ok and bool(lib.semicrf_ffn_residual_bf16_mixed_supported(D, hidden)) == ok
    assert _lib.FFN_MAX_D == 256 and _lib.FFN_MAX_HIDDEN == 4096
    assert lib.semicrf_abi_version() == 2


def _entry(lib, form):
    return (lib.semicrf_ffn_residual_bf16, 2) if form == "A" else (lib.semicrf_ffn_residual_bf16_mixed, 4)


def _direct(fn, x, out, n0, n1, st, D, hidden, w=None, stream=None, eps=1e-6):
    w = w or [x] * 5
    return fn(x, out, n0, n1, *st, D, hidden, *w, ctypes.c_float(eps), stream)


@pytest.mark.parametrize("form", FORMS)
def test_bad_direct_calls_are_rejected(form):
    """A call outside the contract returns nonzero with a message before any pointer is used (the pointers here are never valid):
    semicrf_ffn_residual's list, on elements of 2 or 4 bytes."""
    from transkun_amd import _lib
    lib = _lib.load()
    fn, el = _entry(lib, form)
    a, b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    st = [800, 16, 800, 16]
    for D, hidden in ((12, 8), (8, 7), (264, 8), (8, 4104), (0, 8)):
        assert _direct(fn, a, b, 2, 3, st, D, hidden) == 1 and b"supported" in lib.semicrf_last_error()
    assert _direct(fn, a, None, 2, 3, st, 16, 8) == 1 and b"NULL" in lib.semicrf_last_error()
    assert _direct(fn, a, b, 2, 3, st, 16, 8, w=[a, a, None, a, a]) == 1 and b"NULL" in lib.semicrf_last_error()
    for n0, n1 in ((0, 3), (2, 0), (-1, 3)):
        assert _direct(fn, a, b, n0, n1, st, 16, 8) == 1 and b">= 1" in lib.semicrf_last_error()
    assert _direct(fn, a, b, 1 << 20, 1 << 20, st, 16, 8) == 1 and b"2^37" in lib.semicrf_last_error()
    for i in range(4):
        bad = list(st); bad[i] = -16
        assert _direct(fn, a, b, 2, 3, bad, 16, 8) == 1 and b"stride" in lib.semicrf_last_error()
        bad[i] = 1 << 40
        assert _direct(fn, a, b, 2, 3, bad, 16, 8) == 1 and b"stride" in lib.semicrf_last_error()
    assert _direct(fn, a, b, 2, 3, [800, 16, 800, 8], 16, 8) == 1 and b"below D" in lib.semicrf_last_error()
    assert _direct(fn, a, ctypes.c_void_p((1 << 20) + el // 2), 2, 3, st, 16, 8) == 1 and b"aligned" in lib.semicrf_last_error()
    for shift in (0, 64, el * (800 + 2 * 16 + 15), -el * (800 + 2 * 16 + 15)):     # out inside, at either end of, x's span
        assert _direct(fn, a, ctypes.c_void_p((1 << 20) + shift), 2, 3, st, 16, 8) == 1 and b"overlaps" in lib.semicrf_last_error()
    assert _direct(fn, a, ctypes.c_void_p((1 << 20) + el * (800 + 2 * 16 + 16)), 2, 3, st, 16, 0) == 1          # and never a launch
    # the torch op checks the same set, the shapes and the dtype before anything runs
    ops = _lib.ops()
    op = ops.ffn_residual_bf16 if form == "A" else ops.ffn_residual_bf16_mixed
    dt, other = (BF16, torch.float32) if form == "A" else (torch.float32, BF16)
    z = lambda *s: torch.zeros(*s, dtype=dt)
    x = z(1, 2, 16)
    w1, b1, w2, b2, s = z(8, 16), z(8), z(16, 8), z(16), z(16)
    with pytest.raises(RuntimeError, match="support"):
        op(z(1, 2, 12), z(8, 12), b1, z(12, 8), z(12), z(12), 1e-6, z(1, 2, 12))
    with pytest.raises(RuntimeError):
        op(x, w1, b1, w2, b2, s, 1e-6, torch.empty(1, 3, 16, dtype=dt))
    with pytest.raises(RuntimeError, match="must be"):
        op(x.to(other), w1, b1, w2, b2, s, 1e-6, torch.empty_like(x))       # the other form's dtype
    with pytest.raises(RuntimeError, match="dtype"):
        op(x, w1.to(other), b1, w2, b2, s, 1e-6, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="dtype"):
        op(x, w1, b1, w2, b2, s.to(other), 1e-6, torch.empty_like(x))
    with pytest.raises(RuntimeError):
        op(x, w1, b1, w2.T, b2, s, 1e-6, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="overlaps"):
        op(x, w1, b1, w2, b2, s, 1e-6, x)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_rejected_call_leaves_output_untouched_gpu(gpu, form):
    from transkun_amd import _lib
    lib = _lib.load()
    fn, _ = _entry(lib, form)
    dt = c16.dtype_of(form)
    x = torch.randn(2, 3, 12, device=gpu).to(dt)
    out = torch.full_like(x, 3.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _direct(fn, p(x), p(out), 2, 3, [36, 12, 36, 12], 12, 8, stream=_lib.stream_of(x))
    assert rc == 1 and b"supported" in lib.semicrf_last_error()
    y = torch.randn(2, 3, 16, device=gpu).to(dt)
    rc = _direct(fn, p(y), p(y), 2, 3, [48, 16, 48, 16], 16, 8, stream=_lib.stream_of(y))
    torch.cuda.synchronize(gpu)
    assert rc == 1 and b"overlaps" in lib.semicrf_last_error()
    assert bool((out == 3.0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_replays_the_op(gpu, form):
    """One capture-and-replay of the op: the single launch allocates nothing, and the replay on new data matches an eager launch bit
    for bit."""
    cases = [c16.case(form, 2 * R + 1, 160, 640, "randn", m) for m in ffn_common.INPUT_SCALES]
    params = tuple(p.to(gpu) for p in cases[0]["params"])
    data = [c["x"].to(gpu) for c in cases]
    want = [c16.run(cases[0], gpu, x) for x in data]
    xi = data[0].clone()
    out = torch.empty_like(xi)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        c16.raw_op(form, xi.unsqueeze(0), params, cases[0]["eps"], out.unsqueeze(0))
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c16.raw_op(form, xi.unsqueeze(0), params, cases[0]["eps"], out.unsqueeze(0))
    for i in (1, 0, 1):
        xi.copy_(data[i])
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert c16.bits_equal(out, want[i])


# ---- 6. routing -----------------------------------------------------------------------------------------------------------------------------
def _routes():
    from transkun_amd import backbone
    return dict(backbone.FEED_FORWARD_ROUTES), dict(backbone.FEED_FORWARD_BF16_ROUTES)


def _took(before, way, way16):
    """FEED_FORWARD_ROUTES moved by one under `way`, FEED_FORWARD_BF16_ROUTES by one under `way16` (None: not at all)."""
    ff, ff16 = _routes()
    want = dict(before[0]); want[way] += 1
    want16 = dict(before[1])
    if way16 is not None:
        want16[way16] += 1
    return ff == want and ff16 == want16


def _check_routing(dev):
    """Which way a ResBlock goes with feedForwardBf16 = "fused", read from the counters."""
    from transkun_amd import backbone
    kind = torch.device(dev).type
    g = torch.Generator().manual_seed(6)
    blk = ffn_common.stock_modules(32, 64, g).to(dev)
    b16 = ffn_common.stock_modules(32, 64, g).to(BF16).to(dev)
    x = torch.randn(3, 5, 32, generator=g).to(dev)
    x16 = x.bfloat16()
    stock = lambda b, t: t + b.dropout(b.module(b.norm(t))) * b.scale
    assert blk.feedForwardBf16 == "torch" and blk.feedForward == "torch"
    with torch.no_grad():
        before = _routes()                                               # the defaults: nothing is counted, nothing changes
        assert torch.equal(b16(x16), stock(b16, x16))
        with torch.autocast(kind, dtype=BF16):
            assert torch.equal(blk(x), stock(blk, x))
        assert _routes() == before
        blk.feedForwardBf16 = b16.feedForwardBf16 = "fused"               # the knob without feedForward = "fused": the same
        assert torch.equal(b16(x16), stock(b16, x16))
        with torch.autocast(kind, dtype=BF16):
            assert torch.equal(blk(x), stock(blk, x))
        assert _routes() == before
        blk.feedForward = b16.feedForward = "fused"
        b16.feedForwardBf16 = "torch"                                     # feedForward alone: a bf16 block is the stock expression
        before = _routes()
        assert torch.equal(b16(x16), stock(b16, x16))
        assert _took(before, "torch", None)
        b16.feedForwardBf16 = "fused"
        before = _routes()
        got = b16(x16)                                                    # bf16 everywhere: form A
        assert _took(before, "fused", "fused") and got.dtype == BF16
        assert float((got.float() - stock(b16, x16).float()).abs().max()) <= 2.0 ** -6 * float(got.float().abs().max())
        before = _routes()
        with torch.autocast(kind, dtype=BF16):
            got = blk(x)                                                  # fp32 under bf16 autocast: form B
        assert _took(before, "fused", "fused") and got.dtype == torch.float32
        before = _routes()
        want = blk(x)                                                     # the same block outside autocast: the fp32 op
        assert _took(before, "fused", None)
        assert 0 < float((got - want).abs().max()) <= 2.0 ** -6 * float(want.abs().max())
        blk.feedForwardBf16 = "torch"
        before = _routes()
        with torch.autocast(kind, dtype=BF16):
            assert torch.equal(blk(x), want)                              # the knob at "torch" under autocast: as before, the fp32 op
        assert _took(before, "fused", None)
        blk.feedForwardBf16 = "fused"
        before = _routes()
        with torch.autocast(kind, dtype=torch.float16):
            blk(x)                                                        # fp16 autocast
        assert _took(before, "torch", None)
        before = _routes()
        with torch.autocast(kind, dtype=torch.float16):
            b16(x16)
        assert _took(before, "torch", "torch")
        mixed = ffn_common.stock_modules(32, 64, g).to(BF16).to(dev)
        mixed.feedForward = mixed.feedForwardBf16 = "fused"
        mixed.scale.data = mixed.scale.data.float()                       # mixed dtypes: a float32 LayerScale on a bf16 block
        before = _routes()
        mixed(x16)
        assert _took(before, "torch", "torch")
        for D, hidden in ((12, 64), (32, 7)):                             # outside the supported set
            b = ffn_common.stock_modules(D, hidden, g).to(BF16).to(dev)
            b.feedForward = b.feedForwardBf16 = "fused"
            before = _routes()
            xx = torch.randn(4, D, generator=g).to(BF16).to(dev)
            assert torch.equal(b(xx), stock(b, xx))
            assert _took(before, "torch", "torch")
        drop = backbone.ResBlock(backbone._feed_forward(32, 64, 0.5), size=32, dropoutProb=0.5).to(BF16).to(dev)
        drop.feedForward = drop.feedForwardBf16 = "fused"
        drop.train()
        before = _routes()
        drop(x16)                                                         # active dropout
        assert _took(before, "torch", "torch")
        drop.eval()
        before = _routes()
        drop(x16)                                                         # the same block in eval mode
        assert _took(before, "fused", "fused")
        attn = backbone.ResBlock(backbone.MultiHeadAttentionKernel(32, 2, kernel=None), size=32).eval().to(BF16).to(dev)
        attn.feedForward = attn.feedForwardBf16 = "fused"
        before = _routes()
        attn(x16, x16)                                                    # an attention module, and an extra argument
        assert _took(before, "torch", None)
    before = _routes()
    got = b16(x16)                                                        # autograd: the parameters require grad
    assert _took(before, "torch", "torch") and got.requires_grad
    got.float().sum().backward()
    assert all(p.grad is not None for p in b16.parameters())
    params = [p.detach() for p in (b16.module[0].weight, b16.module[0].bias, b16.module[3].weight, b16.module[3].bias, b16.scale)]
    before = _routes()
    backbone.feed_forward_residual(x16, *params, route="fused")          # the function's default: the knob at "torch"
    assert _took(before, "torch", None)
    before = _routes()
    backbone.feed_forward_residual(x16, *params, route="torch", bf16="fused")
    assert _took(before, "torch", None)
    with pytest.raises(ValueError):
        backbone.feed_forward_residual(x16, *params, bf16="hip")
    b16.feedForwardBf16 = "hip"
    with pytest.raises(ValueError):
        b16(x16)


def test_routing_cpu():
    _check_routing(CPU)


@pytest.mark.gpu
def test_routing_gpu(gpu):
    _check_routing(gpu)


def test_properties_and_state_dict():
    """BasicBlock.feedForwardBf16 and Backbone.feedForwardBf16 set every feed-forward block and read "mixed" when they differ;
    parameter names are unchanged: the reference's state dict loads strictly whatever the knobs say."""
    from transkun_amd import backbone
    m, fx = backbone_common.make_backbone("backbone_d40", CPU, "fused")
    assert m.feedForwardBf16 == "torch" and all(b.feedForwardBf16 == "torch" for b in m.encoderLayers)
    m.encoderLayers[0].fnnBlockF.feedForwardBf16 = "fused"
    assert m.encoderLayers[0].feedForwardBf16 == "mixed" and m.feedForwardBf16 == "mixed"
    m.encoderLayers[0].feedForwardBf16 = "fused"
    assert m.encoderLayers[0].feedForwardBf16 == "fused" and m.feedForwardBf16 == ("fused" if len(m.encoderLayers) == 1 else "mixed")
    m.feedForwardBf16 = "fused"
    assert m.feedForwardBf16 == "fused" and all(b.feedForwardBf16 == "fused" for b in m.feed_forward_blocks())
    assert all(b.feedForwardBf16 == "torch" for b in m.modules() if isinstance(b, backbone.ResBlock) and not b.is_feed_forward())
    assert m.feedForward == "torch"                                       # the other knob is its own
    for target in (m, m.encoderLayers[0]):
        with pytest.raises(ValueError):
            target.feedForwardBf16 = "hip"
    m.load_state_dict(fx["sd"], strict=True)
    assert set(m.state_dict()) == set(fx["sd"])


# ---- 7. the modules -------------------------------------------------------------------------------------------------------------------------
def _module_errors(dev, form):
    """A BasicBlock and the small Backbone with attentionBf16, feedForward and feedForwardBf16 at "fused" against the same module in
    float64: the error is at most GATE times that of feedForwardBf16 = "torch", and no feed-forward call took the stock route.  Form A:
    the module cast to bf16 (truth: its bf16 weights upcast).  Form B: the fp32 module under bfloat16 autocast (truth: its own weights)."""
    import copy
    from transkun_amd import backbone
    kind_of = torch.device(dev).type
    if form == "A":
        m, m64, fx = backbone_bf16_common.bf16_backbone("backbone_small", dev)
        x, lin = fx["x"].bfloat16(), fx["layer_in"].bfloat16()
    else:
        m, fx = backbone_common.make_backbone("backbone_small", dev, "fused")
        m64 = copy.deepcopy(m).double().cpu()
        x, lin = fx["x"], fx["layer_in"]
    idx = fx["outputIndices"]
    with torch.no_grad():
        truth = {"backbone": m64(x.double(), idx), "block": m64.encoderLayers[0](lin.double())}
    m.attentionBf16, m.feedForward = "fused", "fused"
    n_ffn = len(m.feed_forward_blocks()) + 2
    f0 = m.encoderLayers[0].fnnBlockF.module[0]
    assert backbone.feed_forward_bf16_supported(f0.in_features, f0.out_features)
    err = {}
    for kind in ("torch", "fused"):
        m.feedForwardBf16 = kind
        before = _routes()
        with torch.no_grad(), torch.autocast(kind_of, dtype=BF16, enabled=form == "B"):
            got = {"backbone": m(x.to(dev), idx.to(dev)), "block": m.encoderLayers[0](lin.to(dev))}
        ff, ff16 = _routes()
        if kind == "fused":                                               # every feed-forward call of both forwards went to the bf16 op
            assert ff16 == {"fused": before[1]["fused"] + n_ffn, "torch": before[1]["torch"]}
            assert ff == {"fused": before[0]["fused"] + n_ffn, "torch": before[0]["torch"]}
        else:
            assert ff16 == before[1]
        for tag, g in got.items():
            assert g.shape == truth[tag].shape and bool(torch.isfinite(g).all())
            err[kind, tag] = float((g.cpu().double() - truth[tag]).abs().max())
    for tag in ("backbone", "block"):
        print(f"form {form} {tag} [{kind_of}]: error fused {err['fused', tag]:.3e}  torch {err['torch', tag]:.3e}  "
              f"ratio {err['fused', tag] / err['torch', tag]:.2f} (gate {c16.GATE:g})")
        assert err["fused", tag] <= c16.GATE * err["torch", tag], tag


@pytest.mark.parametrize("form", FORMS)
def test_modules_cpu(form):
    _module_errors(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_modules_gpu(gpu, form):
    _module_errors(gpu, form)
