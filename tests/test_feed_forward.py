"""The backbone's feed-forward ResBlock as one fused op (transkun_amd.backbone.feed_forward_residual, torch.ops.semicrf.ffn_residual;
csrc/ffn.hip on the device, the host mirror of csrc/cpu_ops.cpp on the CPU).

1. accuracy: every width x hidden size x row count x LayerScale x input scale against float64, gated by the stock fp32 modules' own
   error (ffn_common); every instantiation of the kernel, aligned and one float off 16 bytes
2. bits: a row's result whatever the batch; strided views; non-finite rows stay put; nothing outside `out` is written; the device
   against the host mirror; an emulation of the order of operations that is independent of both
3. mutation: a walk that stops one hidden chunk early fails the gate exactly where there is more than one chunk
4. contract, routing, modules against the reference fixtures, copies, graph capture
"""
import ctypes

import pytest
import torch

import backbone_common
import ffn_common as common

CPU = torch.device("cpu")
R, C = common.tiles()


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------------
def _check_gate(dev, D, hidden, rows_list=None):
    for rows in rows_list or common.row_counts():
        for kind in common.SCALE_KINDS:
            for mult in common.INPUT_SCALES:
                c = common.case(rows, D, hidden, kind, mult)
                got = common.run(c, dev)
                assert got.shape == c["x"].shape and got.dtype == torch.float32
                e = float((got.cpu().double() - c["truth"]).abs().max())
                print(f"[{dev.type}] rows {rows} D {D} hidden {hidden} scale {kind} x{mult:g}: error {e:.3e}  stock fp32 {c['e32']:.3e}  "
                      f"gate {c['gate']:.3e}")
                assert e <= c["gate"], (rows, D, hidden, kind, mult, e, c["gate"])


@pytest.mark.parametrize("hidden", common.hidden_sizes())
@pytest.mark.parametrize("D", common.WIDTHS)
def test_op_gate_cpu(D, hidden):
    _check_gate(CPU, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", common.hidden_sizes())
@pytest.mark.parametrize("D", common.WIDTHS)
def test_op_gate_gpu(gpu, D, hidden):
    _check_gate(gpu, D, hidden)


def _matrix(dev, D, aligned):
    """One instantiation <column blocks of 32, 16-byte or 4-byte loads>: three row tiles, the last of one row; two hidden chunks, the
    second of 8 columns."""
    c = common.case(2 * R + 1, D, C + 8, "randn", 1.0)
    x = c["x"].to(dev)
    if not aligned:
        x = common.one_float_off(x)
    got = common.run(c, dev, x)
    e = float((got.cpu().double() - c["truth"]).abs().max())
    assert e <= c["gate"], (D, aligned, e, c["gate"])
    assert common.bits_equal(got.cpu(), common.run(c, dev).cpu())         # the two load widths give the same numbers


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("D", common.MATRIX_WIDTHS)
def test_op_instantiation_matrix_cpu(D, aligned):
    _matrix(CPU, D, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("D", common.MATRIX_WIDTHS)
def test_op_instantiation_matrix_gpu(gpu, D, aligned):
    _matrix(gpu, D, aligned)


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------
BIT_SHAPES = [(160, 640), (80, C + 8), (256, 1024), (8, 8)]


def _check_row_independence(dev):
    """A row's bits are the same alone, in a batch of 3 and in a batch of 2R + 1, wherever it stands."""
    for D, hidden in BIT_SHAPES:
        c = common.case(2 * R + 1, D, hidden, "randn", 1.0)
        full = common.run(c, dev).cpu()
        for r in (0, R - 1, R, 2 * R):
            alone = common.run(c, dev, c["x"][r:r + 1]).cpu()
            assert common.bits_equal(alone[0], full[r]), (D, hidden, r)
            lo = min(r, 2 * R - 2)
            three = common.run(c, dev, c["x"][lo:lo + 3]).cpu()
            assert common.bits_equal(three[r - lo], full[r]), (D, hidden, r)


def test_row_independence_cpu():
    _check_row_independence(CPU)


@pytest.mark.gpu
def test_row_independence_gpu(gpu):
    _check_row_independence(gpu)


def _check_strided_views(dev):
    """The transposed view, a view one float off a 16-byte boundary and rows with gaps give the contiguous call's bits, without a
    copy where two row strides express the view; the result is laid out like x."""
    from transkun_amd import backbone
    for D, hidden in BIT_SHAPES[:2]:
        c = common.case(0, D, hidden, "randn", 1.0, lead=(2, 5, 7))
        x = c["x"].to(dev)
        want = common.run(c, dev, x)
        xt = x.transpose(-3, -2)                                         # BasicBlock's attention = "torch" order
        got = common.run(c, dev, xt)
        assert got.shape == xt.shape and got.stride() == xt.stride()
        assert common.bits_equal(got.transpose(-3, -2).cpu(), want.cpu())
        off = common.one_float_off(x)
        assert common.bits_equal(common.run(c, dev, off).cpu(), want.cpu())
        # the raw op on a [n0, n1, D] view with two real row strides, into an `out` with strides of its own
        x3 = x[0]                                                        # [5, 7, D]
        v = x3.transpose(0, 1)                                           # [7, 5, D], strides (D, 7 D)
        out = torch.full((7, 5, D + 3), float("nan"), device=dev)[..., :D]
        common.raw_op(v, tuple(p.to(dev) for p in c["params"]), c["eps"], out)
        assert common.bits_equal(out.transpose(0, 1).cpu(), want[0].cpu())
    assert backbone.FEED_FORWARD_ROUTES["fused"] > 0


def test_strided_views_cpu():
    _check_strided_views(CPU)


@pytest.mark.gpu
def test_strided_views_gpu(gpu):
    _check_strided_views(gpu)


def _check_non_finite_stay_put(dev):
    """A NaN or an infinity in one row reaches that row only; every other row keeps the clean run's bits."""
    for D, hidden in BIT_SHAPES[:3]:
        c = common.case(2 * R + 1, D, hidden, "randn", 1.0)
        clean = common.run(c, dev).cpu()
        for bad in (float("nan"), float("inf"), -float("inf")):
            x = c["x"].clone()
            hit = [1, R, 2 * R]
            for r in hit:
                x[r, (3 * r) % D] = bad
            got = common.run(c, dev, x).cpu()
            keep = torch.ones(x.shape[0], dtype=torch.bool)
            keep[hit] = False
            assert common.bits_equal(got[keep], clean[keep]), (D, hidden, bad)
            assert not bool(torch.isfinite(got[hit]).all(dim=-1).any())   # the rows that were hit show it


def test_non_finite_stay_put_cpu():
    _check_non_finite_stay_put(CPU)


@pytest.mark.gpu
def test_non_finite_stay_put_gpu(gpu):
    _check_non_finite_stay_put(gpu)


def _check_poison(dev):
    """NaN behind the last row of x is never read into a result, and a sentinel around `out` (in front, behind, and in the gaps
    between its rows) is never overwritten."""
    for D, hidden in BIT_SHAPES[:3]:
        for rows in (1, R - 1, R + 1):
            c = common.case(rows, D, hidden, "randn", 1.0)
            want = common.run(c, dev).cpu()
            buf = torch.full((rows + 2 * R, D), float("nan"), device=dev)
            buf[:rows] = c["x"].to(dev)
            pitch = D + 5
            obuf = torch.full((rows + 2, pitch), 7.5, device=dev)
            out = obuf[1:rows + 1, 2:2 + D]
            common.raw_op(buf[:rows].unsqueeze(0), tuple(p.to(dev) for p in c["params"]), c["eps"], out.unsqueeze(0))
            assert common.bits_equal(out.cpu(), want), (D, hidden, rows)
            mask = torch.ones_like(obuf, dtype=torch.bool)
            mask[1:rows + 1, 2:2 + D] = False
            assert bool((obuf[mask] == 7.5).all()), (D, hidden, rows)


def test_poison_cpu():
    _check_poison(CPU)


@pytest.mark.gpu
def test_poison_gpu(gpu):
    _check_poison(gpu)


# The CPU math library against float64: at the cases below glibc's erff / erfcf change at most 7 % of the output elements against erf /
# erfc taken in float64 and rounded once (measured: 1 % to 7 %; an output sums `hidden` gelu values, so one last-bit difference in a row
# can show in all of its D outputs).  CAP_CPU is that share with headroom.  Two libraries that both stay near float64 differ from one
# another in at most the sum of their shares; the device library's erf and erfc are allowed twice the host's error, so the share of
# elements in which the device may differ from the host mirror is capped at CAP_CPU + 2 CAP_CPU.
CAP_CPU = 0.10
CAP_DEVICE = 3 * CAP_CPU
LIBM_CASES = [(2 * R + 1, 8, 8), (2 * R + 1, 32, 8), (2 * R + 1, 32, C - 8), (2 * R + 1, 80, C + 8)]


def _exact_case(D, hidden):
    """Every hidden pre-activation above 20: 1 + erf(z) is exactly 2 in any library, gelu is the identity, and the whole op is the
    two fmaf chains, the norm and the epilogue -- no element may differ between two implementations of ffn_math.h."""
    c = dict(common.case(2 * R + 1, D, hidden, "randn", 1.0))
    w1, b1, w2, b2, scale = c["params"]
    c["params"] = (w1, b1 * 0 + 30.0 + b1, w2, b2, scale)
    return c


@pytest.mark.parametrize("rows,D,hidden", LIBM_CASES)
def test_mirror_matches_emulation_cpu(rows, D, hidden):
    """The host mirror against an emulation of ffn_math.h that shares no code with it: the same bits wherever glibc's erff / erfcf
    round like float64's, and the share of the rest below CAP_CPU; with gelu out of the way (every pre-activation large), all bits."""
    for mult in common.INPUT_SCALES:
        c = common.case(rows, D, hidden, "randn", mult)
        differ = float((~common.same_bits_mask(common.run(c, CPU), common.emulate(c))).float().mean())
        print(f"rows {rows} D {D} hidden {hidden} x{mult:g}: host mirror differs from the float64-erf emulation in {differ:.4f} of the elements")
        assert differ <= CAP_CPU
    c = _exact_case(D, hidden)
    assert common.bits_equal(common.run(c, CPU), common.emulate(c))


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,hidden", LIBM_CASES)
def test_device_matches_mirror_gpu(gpu, rows, D, hidden):
    """The device against the host mirror: the same bits wherever the two libraries' erff and erfcf agree; the share of elements that
    differ stays below CAP_DEVICE (and below CAP_DEVICE against the float64-erf emulation as well)."""
    for mult in common.INPUT_SCALES:
        c = common.case(rows, D, hidden, "randn", mult)
        dev_out = common.run(c, gpu).cpu()
        vs_host = float((~common.same_bits_mask(dev_out, common.run(c, CPU))).float().mean())
        vs_f64 = float((~common.same_bits_mask(dev_out, common.emulate(c))).float().mean())
        print(f"rows {rows} D {D} hidden {hidden} x{mult:g}: device differs from the host mirror in {vs_host:.4f}, from the emulation in {vs_f64:.4f}")
        assert vs_host <= CAP_DEVICE and vs_f64 <= CAP_DEVICE


@pytest.mark.gpu
@pytest.mark.parametrize("D,hidden", BIT_SHAPES)
def test_device_equals_mirror_without_gelu_gpu(gpu, D, hidden):
    """With every pre-activation large (gelu the identity in any library) the device and the host mirror agree in every bit: both
    chains, the chunk walk, the norm and the epilogue are the same operations in the same order."""
    c = _exact_case(D, hidden)
    assert common.bits_equal(common.run(c, gpu).cpu(), common.run(c, CPU))


# ---- 3. mutation --------------------------------------------------------------------------------------------------------------------------
def test_skipping_the_last_chunk_fails_the_gate(monkeypatch):
    """A host mirror that leaves out the last hidden chunk fails every case with hidden > C and none with hidden <= C (there the walk
    has one chunk and the flag changes nothing)."""
    monkeypatch.setattr(common, "SKIP_LAST_CHUNK", True)
    for D in common.WIDTHS:
        for hidden in common.hidden_sizes():
            for kind in common.SCALE_KINDS:
                for mult in common.INPUT_SCALES:
                    c = common.case(R + 1, D, hidden, kind, mult)
                    e = float((common.run(c, CPU).double() - c["truth"]).abs().max())
                    assert (e > c["gate"]) == (hidden > C), (D, hidden, kind, mult, e, c["gate"])


# ---- 4. contract, routing, modules --------------------------------------------------------------------------------------------------------
def test_supported_set_and_constants():
    from transkun_amd import _lib, backbone
    assert (R, C) == (_lib.FFN_ROW_TILE, _lib.FFN_HIDDEN_CHUNK)
    for D, hidden, ok in ((8, 8, True), (256, 4096, True), (160, 640, True), (0, 8, False), (264, 8, False), (12, 8, False), (8, 7, False),
                          (8, 4104, False), (8, 0, False), (-8, 8, False)):
        assert backbone.feed_forward_supported(D, hidden) == ok, (D, hidden)


def _direct(lib, x, out, n0, n1, st, D, hidden, w=None, stream=None, eps=1e-6):
    w = w or [x] * 5
    return lib.semicrf_ffn_residual(x, out, n0, n1, *st, D, hidden, *w, ctypes.c_float(eps), stream)


def test_bad_direct_calls_are_rejected():
    """A call outside the contract returns nonzero with a message before any pointer is used (the pointers here are never valid)."""
    from transkun_amd import _lib
    lib = _lib.load()
    a, b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)
    st = [800, 16, 800, 16]
    for D, hidden in ((12, 8), (8, 7), (264, 8), (8, 4104), (0, 8)):
        assert _direct(lib, a, b, 2, 3, st, D, hidden) == 1 and b"supported" in lib.semicrf_last_error()
    assert _direct(lib, a, None, 2, 3, st, 16, 8) == 1 and b"NULL" in lib.semicrf_last_error()
    assert _direct(lib, a, b, 2, 3, st, 16, 8, w=[a, a, None, a, a]) == 1 and b"NULL" in lib.semicrf_last_error()
    for n0, n1 in ((0, 3), (2, 0), (-1, 3)):
        assert _direct(lib, a, b, n0, n1, st, 16, 8) == 1 and b">= 1" in lib.semicrf_last_error()
    assert _direct(lib, a, b, 1 << 20, 1 << 20, st, 16, 8) == 1 and b"2^37" in lib.semicrf_last_error()
    for i in range(4):
        bad = list(st); bad[i] = -16
        assert _direct(lib, a, b, 2, 3, bad, 16, 8) == 1 and b"stride" in lib.semicrf_last_error()
        bad[i] = 1 << 40
        assert _direct(lib, a, b, 2, 3, bad, 16, 8) == 1 and b"stride" in lib.semicrf_last_error()
    assert _direct(lib, a, b, 2, 3, [800, 16, 800, 8], 16, 8) == 1 and b"below D" in lib.semicrf_last_error()
    assert _direct(lib, a, ctypes.c_void_p((1 << 20) + 6), 2, 3, st, 16, 8) == 1 and b"aligned" in lib.semicrf_last_error()
    for shift in (0, 64, 4 * (800 + 2 * 16 + 15), -4 * (800 + 2 * 16 + 15)):       # out inside, at either end of, x's span
        assert _direct(lib, a, ctypes.c_void_p((1 << 20) + shift), 2, 3, st, 16, 8) == 1 and b"overlaps" in lib.semicrf_last_error()
    # the torch op checks the same set and the shapes before anything runs
    ops = _lib.ops()
    x = torch.zeros(1, 2, 16)
    w1, b1, w2, b2, s = torch.zeros(8, 16), torch.zeros(8), torch.zeros(16, 8), torch.zeros(16), torch.zeros(16)
    with pytest.raises(RuntimeError, match="support"):
        ops.ffn_residual(torch.zeros(1, 2, 12), torch.zeros(8, 12), b1, torch.zeros(12, 8), torch.zeros(12), torch.zeros(12), 1e-6, torch.zeros(1, 2, 12))
    with pytest.raises(RuntimeError):
        ops.ffn_residual(x, w1, b1, w2, b2, s, 1e-6, torch.empty(1, 3, 16))
    with pytest.raises(RuntimeError):
        ops.ffn_residual(x.double(), w1, b1, w2, b2, s, 1e-6, torch.empty_like(x))
    with pytest.raises(RuntimeError):
        ops.ffn_residual(x, w1, b1, w2.T, b2, s, 1e-6, torch.empty_like(x))
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.ffn_residual(x, w1, b1, w2, b2, s, 1e-6, x)


@pytest.mark.gpu
def test_rejected_call_leaves_output_untouched_gpu(gpu):
    from transkun_amd import _lib
    lib = _lib.load()
    x = torch.randn(2, 3, 12, device=gpu)
    out = torch.full_like(x, 3.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = _direct(lib, p(x), p(out), 2, 3, [36, 12, 36, 12], 12, 8, stream=_lib.stream_of(x))
    assert rc == 1 and b"supported" in lib.semicrf_last_error()
    y = torch.randn(2, 3, 16, device=gpu)
    rc = _direct(lib, p(y), p(y), 2, 3, [48, 16, 48, 16], 16, 8, stream=_lib.stream_of(y))
    torch.cuda.synchronize(gpu)
    assert rc == 1 and b"overlaps" in lib.semicrf_last_error()
    assert bool((out == 3.0).all())


def _routes():
    from transkun_amd import backbone
    return dict(backbone.FEED_FORWARD_ROUTES)


def _took(before, way):
    after = _routes()
    other = "torch" if way == "fused" else "fused"
    return after[way] == before[way] + 1 and after[other] == before[other]


def _check_routing(dev):
    """Which way a ResBlock set to "fused" goes, read from the counters; the stock route's values are the stock expression's."""
    from transkun_amd import backbone
    g = torch.Generator().manual_seed(5)
    blk = common.stock_modules(32, 64, g).to(dev)
    x = torch.randn(3, 5, 32, generator=g).to(dev)
    stock = lambda b, t: t + b.dropout(b.module(b.norm(t))) * b.scale
    assert blk.feedForward == "torch"                                    # the default: nothing is counted, nothing changes
    before = _routes()
    with torch.no_grad():
        assert torch.equal(blk(x), stock(blk, x))
    assert _routes() == before
    blk.feedForward = "fused"
    before = _routes()
    with torch.no_grad():
        got = blk(x)                                                     # eval, fp32, supported, no gradient: the op
    assert _took(before, "fused")
    with torch.no_grad():
        assert float((got - stock(blk, x)).abs().max()) <= 1e-5 * float(got.abs().max())
    before = _routes()
    got = blk(x)                                                         # autograd: the parameters require grad
    assert _took(before, "torch") and got.requires_grad
    got.sum().backward()
    assert all(p.grad is not None for p in blk.parameters())
    with torch.no_grad():
        before = _routes()
        b64 = common.stock_modules(32, 64, g).double().to(dev)
        b64.feedForward = "fused"
        b64(x.double())                                                  # fp64
        assert _took(before, "torch")
        for D, hidden in ((12, 64), (32, 7)):                            # outside the supported set
            b = common.stock_modules(D, hidden, g).to(dev)
            b.feedForward = "fused"
            before = _routes()
            xx = torch.randn(4, D, generator=g).to(dev)
            assert torch.equal(b(xx), stock(b, xx))
            assert _took(before, "torch")
        drop = backbone.ResBlock(backbone._feed_forward(32, 64, 0.5), size=32, dropoutProb=0.5).to(dev)
        drop.feedForward = "fused"
        drop.train()
        before = _routes()
        drop(x)                                                          # active dropout
        assert _took(before, "torch")
        drop.eval()
        before = _routes()
        drop(x)                                                          # the same block in eval mode
        assert _took(before, "fused")
        zero = backbone.ResBlock(backbone._feed_forward(32, 64, 0.0), size=32, dropoutProb=0.0).to(dev).train()
        zero.feedForward = "fused"
        before = _routes()
        zero(x)                                                          # training mode with p = 0: no dropout is active
        assert _took(before, "fused")
        attn = backbone.ResBlock(backbone.MultiHeadAttentionKernel(32, 2, kernel=None), size=32).eval().to(dev)
        attn.feedForward = "fused"
        before = _routes()
        attn(x, x)                                                       # an attention module, and an extra argument
        assert _took(before, "torch")
        before = _routes()
        attn(x)
        assert _took(before, "torch")
    with pytest.raises(ValueError):
        backbone.feed_forward_residual(x, *[p.detach() for p in (blk.module[0].weight, blk.module[0].bias, blk.module[3].weight,
                                                                   blk.module[3].bias, blk.scale)], route="hip")


def test_routing_cpu():
    _check_routing(CPU)


@pytest.mark.gpu
def test_routing_gpu(gpu):
    _check_routing(gpu)


def test_properties_and_state_dict():
    """BasicBlock.feedForward and Backbone.feedForward set every feed-forward block and read "mixed" when they differ; parameter
    names are unchanged: the reference's state dict loads strictly whatever the route."""
    from transkun_amd import backbone
    m, fx = backbone_common.make_backbone("backbone_d40", CPU, "fused")
    assert m.feedForward == "torch" and all(b.feedForward == "torch" for b in m.encoderLayers)
    n_ffn = len(m.feed_forward_blocks())
    assert n_ffn == 2 * len(m.encoderLayers)
    m.encoderLayers[0].fnnBlockF.feedForward = "fused"
    assert m.encoderLayers[0].feedForward == "mixed" and m.feedForward == "mixed"
    m.encoderLayers[0].feedForward = "fused"
    assert m.encoderLayers[0].feedForward == "fused" and m.feedForward == ("fused" if len(m.encoderLayers) == 1 else "mixed")
    m.feedForward = "fused"
    assert m.feedForward == "fused" and all(b.feedForward == "fused" for b in m.feed_forward_blocks())
    assert all(b.feedForward == "torch" for b in m.modules() if isinstance(b, backbone.ResBlock) and not b.is_feed_forward())
    with pytest.raises(ValueError):
        m.feedForward = "hip"
    m.load_state_dict(fx["sd"], strict=True)
    assert set(m.state_dict()) == set(fx["sd"])


def _check_modules(dev, name, attention):
    """BasicBlock and Backbone with feedForward = "fused" against the reference's float64 outputs, gated by the reference's own fp32
    error from the same fixture."""
    from transkun_amd import backbone
    m, fx = backbone_common.make_backbone(name, dev, attention)
    m.feedForward = "fused"
    x, idx, lin = fx["x"].to(dev), fx["outputIndices"].to(dev), fx["layer_in"].to(dev)
    blk = m.encoderLayers[0]
    before = _routes()
    with torch.no_grad():
        got = {"block_out": blk(lin)}
        mid = _routes()
        got["out"] = m(x, idx)
    D, hidden = blk.fnnBlockF.module[0].in_features, blk.fnnBlockF.module[0].out_features
    way = "fused" if backbone.feed_forward_supported(D, hidden) else "torch"
    assert mid[way] == before[way] + 2 and _routes()[way] == mid[way] + 2 * len(m.encoderLayers)
    for tag, g in got.items():
        want64, ref32 = fx[tag + "64"], fx[tag + "32"]
        assert g.shape == want64.shape and g.dtype == torch.float32
        e32 = float((ref32.double() - want64).abs().max())
        e = float((g.cpu().double() - want64).abs().max())
        print(f"{name} [{dev.type}, attention {attention}, feed-forward {way}] {tag}: error {e:.3e}  reference fp32 {e32:.3e}")
        assert e <= backbone_common.GATE * e32, (tag, e, e32)


@pytest.mark.parametrize("attention", ["fused", "torch"])
@pytest.mark.parametrize("name", backbone_common.FIXTURES)
def test_modules_match_reference_cpu(name, attention):
    _check_modules(CPU, name, attention)


@pytest.mark.gpu
@pytest.mark.parametrize("attention", ["fused", "torch"])
@pytest.mark.parametrize("name", backbone_common.FIXTURES)
def test_modules_match_reference_gpu(gpu, name, attention):
    _check_modules(gpu, name, attention)


def test_fused_feed_forward_adds_no_copy():
    """Counted as test_basic_block_makes_no_transposed_copy counts: with feedForward = "fused" a BasicBlock forward makes no more
    hidden-state-sized copies than with "torch", in either attention order -- none at all beside the fused attention."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m, fx = backbone_common.make_backbone("backbone_d40", CPU, "fused")
    blk = m.encoderLayers[0]
    lin = fx["layer_in"]
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

    counts = {}
    for attention in ("fused", "torch"):
        for ff in ("torch", "fused"):
            blk.attention, blk.feedForward = attention, ff
            before = _routes()
            with torch.no_grad(), Count() as c:
                blk(lin)
            counts[attention, ff] = c.copies
            assert _routes()["fused"] == before["fused"] + (2 if ff == "fused" else 0)
    assert counts["fused", "fused"] == []
    assert len(counts["torch", "fused"]) <= len(counts["torch", "torch"])
    assert len(counts["torch", "torch"]) > 0                             # the counter sees the stock route's copies


@pytest.mark.gpu
def test_graph_capture_replays_the_op(gpu):
    """One capture-and-replay of the op: the single launch allocates nothing, and the replay on new data matches an eager launch bit
    for bit."""
    cases = [common.case(2 * R + 1, 160, 640, "randn", m) for m in common.INPUT_SCALES]
    params = tuple(p.to(gpu) for p in cases[0]["params"])
    data = [c["x"].to(gpu) for c in cases]
    want = [common.run(cases[0], gpu, x) for x in data]
    xi = data[0].clone()
    out = torch.empty_like(xi)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        common.raw_op(xi.unsqueeze(0), params, cases[0]["eps"], out.unsqueeze(0))
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        common.raw_op(xi.unsqueeze(0), params, cases[0]["eps"], out.unsqueeze(0))
    for i in (1, 0, 1):
        xi.copy_(data[i])
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert common.bits_equal(out, want[i])
