"""The fused attribute heads: transkun_amd.attributes.attribute_heads (csrc/attr_heads.hip on the GPU, the host mirror of
csrc/cpu_ops.cpp on CPU tensors) and SegmentTranscriber.attributeHeads = "fused".

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  Yardstick, gate (8 x the error of torch's own
fp32 modules on the CPU) and the per-element running error bound: attr_heads_common.  Measured ratios: DESIGN.md section 3,
"Attribute heads", and profiles/attr_heads_bench.json."""
import copy
import ctypes

import pytest
import torch

import attr_heads_common as common
from conftest import load_golden

CPU = torch.device("cpu")


def _R():
    from transkun_amd import attributes
    return attributes.HEADS_ROW_TILE


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. the gate and the per-element bound, every shape and scale ------------------------------------------------------------------
def _check_gate(dev, D, Hv, Ho, scale):
    c = common.gate_case(D, Hv, Ho, scale)
    vp, op, ctx, pairs, offsets = common.to_device(dev, c["vp"], c["op"], c["ctx"], c["pairs"], c["offsets"])
    K = c["K"]
    lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, K)
    assert lv.shape == (K, 128) and of.shape == (K, 4) and lv.dtype == of.dtype == torch.float32
    assert sym.dtype == sc.dtype == torch.int64 and lv.device == of.device == sym.device == sc.device == ctx.device
    assert torch.equal(sc.cpu(), c["chain"]) and torch.equal(sym.cpu(), c["chain"] % common.N_SYM)
    for tag, got, want, bound, e32, use32 in (("logitsVelocity", lv, c["truth"][0], c["bound"][0], c["e32"][0], c["use32"][0]),
                                              ("ofLogits", of, c["truth"][1], c["bound"][1], c["e32"][1], c["use32"][1])):
        err = (got.cpu().double() - want).abs()
        e, use = float(err.max()), float((err / bound).max())
        print(f"attribute_heads [{dev.type}] D={D} Hv={Hv} Ho={Ho} scale={scale:g} {tag}: error {e:.3e}  torch fp32 {e32:.3e}  "
              f"ratio {e / e32:.2f} (gate {common.GATE:g})  bound used {use:.4f} (torch fp32 {use32:.4f})")
        assert use32 <= 1.0                                   # the bound holds for the yardstick's own fp32 route
        assert bool((err <= bound).all()), (tag, use)
        assert e <= common.GATE * e32, (tag, e, e32)


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("D,Hv,Ho", common.SHAPES)
def test_gate_and_bound_cpu(D, Hv, Ho, scale):
    _check_gate(CPU, D, Hv, Ho, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("D,Hv,Ho", common.SHAPES)
def test_gate_and_bound_gpu(gpu, D, Hv, Ho, scale):
    _check_gate(gpu, D, Hv, Ho, scale)


# ---- 2. row counts around the row tile; bit-identity -------------------------------------------------------------------------------
def _small_case(seed, D=20, Hv=40, Ho=24, scale=1.0):
    vp, op = common.make_heads(D, Hv, Ho, seed)
    return vp, op, common.make_ctx(D, scale, seed + 1)


def _check_row_counts(dev):
    R = _R()
    assert R >= 2
    vp0, op0, ctx0 = _small_case(41)
    for K in (0, 1, R - 1, R, R + 1, 2 * R + 1):
        pairs0, offsets0 = common.pack_rows(common.make_rows(K, 50 + K))
        vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx0, pairs0, offsets0)
        for k_arg in (K, None):                               # K given, and read from offsets[-1]
            lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, k_arg)
            assert lv.shape == (K, 128) and of.shape == (K, 4) and sym.shape == sc.shape == (K,)
        if K == 0:
            continue
        tv, to, bv, bo, chain = common.truth_and_bound(ctx0, pairs0, offsets0, K, vp0, op0)
        assert torch.equal(sc.cpu(), chain) and torch.equal(sym.cpu(), chain % common.N_SYM)
        ev, eo = (lv.cpu().double() - tv).abs(), (of.cpu().double() - to).abs()
        assert bool((ev <= bv).all()) and bool((eo <= bo).all()), K
        if K >= 64:
            fv, fo = common.torch_fp32(ctx0, pairs0, offsets0, K, vp0, op0)
            assert float(ev.max()) <= common.GATE * float((fv.double() - tv).abs().max()), K
            assert float(eo.max()) <= common.GATE * float((fo.double() - to).abs().max()), K


def test_row_counts_cpu():
    _check_row_counts(CPU)


@pytest.mark.gpu
def test_row_counts_gpu(gpu):
    _check_row_counts(gpu)


def _check_bit_identity(dev, D, Hv, Ho):
    """One row (chain 5, frames 2..9) alone, first, last and in the middle of other rows, with the frames it does not read changed
    between the runs: the same bits every time, and between two calls."""
    R = _R()
    vp0, op0, ctx0 = _small_case(61, D, Hv, Ho)
    target = (5, 2, 9)
    g = torch.Generator().manual_seed(62)

    def others(n, chains):
        rows = []
        for _ in range(n):
            b = int(torch.randint(0, common.T_FRAMES, (1,), generator=g)); e = int(torch.randint(b, common.T_FRAMES, (1,), generator=g))
            rows.append((chains[int(torch.randint(0, len(chains), (1,), generator=g))], b, e))
        return sorted(rows, key=lambda r: r[0])

    before, after = others(R + 6, [0, 2, 3, 5]), others(R + 3, [5, 6, 7, 8])
    layouts = {"alone": ([target], 0), "first": ([target] + after, 0), "last": (before + [target], len(before)),
               "middle": (before + [target] + after, len(before))}
    garbage = ctx0 * 37.0 + 11.0                              # NaN-free garbage everywhere ...
    garbage[1, 0, 2] = ctx0[1, 0, 2]; garbage[1, 0, 9] = ctx0[1, 0, 9]        # ... but in the two frames the row reads (chain 5 = [1, 0])
    ref = None
    for tag, (rows, at) in layouts.items():
        for ctx_h in (ctx0, garbage):
            pairs0, offsets0 = common.pack_rows(rows)
            vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx_h, pairs0, offsets0)
            lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, len(rows))
            lv2, of2, _, _ = common.fused(ctx, pairs, offsets, vp, op, len(rows))
            assert _bits_equal(lv, lv2) and _bits_equal(of, of2), tag
            assert int(sc[at]) == 5 and int(sym[at]) == 0
            row = (lv[at].cpu().clone(), of[at].cpu().clone())
            if ref is None:
                ref = row
                assert bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 0
            assert _bits_equal(row[0], ref[0]) and _bits_equal(row[1], ref[1]), tag


@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_bit_identity_cpu(D, Hv, Ho):
    _check_bit_identity(CPU, D, Hv, Ho)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1), (256, 512, 512)])
def test_bit_identity_gpu(gpu, D, Hv, Ho):
    _check_bit_identity(gpu, D, Hv, Ho)


# ---- 3. edge pairs, strided and bf16 ctx, the k_cap form ---------------------------------------------------------------------------
def _check_views(dev, D, Hv, Ho):
    vp0, op0, ctx0 = _small_case(71, D, Hv, Ho)
    K = 70
    rows = common.make_rows(K, 72)
    T = common.T_FRAMES
    assert {(0, 0), (T - 1, T - 1), (0, T - 1)} <= {(b, e) for _, b, e in rows}          # b == e, b = 0, e = T - 1
    pairs0, offsets0 = common.pack_rows(rows)
    vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx0, pairs0, offsets0)
    lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, K)
    tv, to, bv, bo, _ = common.truth_and_bound(ctx0, pairs0, offsets0, K, vp0, op0)
    assert bool(((lv.cpu().double() - tv).abs() <= bv).all()) and bool(((of.cpu().double() - to).abs() <= bo).all())
    # a view with a row stride above D (a multiple of four floats, and not): read in place, the same bits
    for pad in (4, 3):
        big = torch.full((common.N_SEG, common.N_SYM, T, D + pad), 1e30, device=dev)
        big[..., :D] = ctx
        view = big[..., :D]
        assert view.stride(2) == D + pad and not view.is_contiguous()
        lv2, of2, sym2, sc2 = common.fused(view, pairs, offsets, vp, op, K)
        assert _bits_equal(lv, lv2) and _bits_equal(of, of2) and torch.equal(sym, sym2) and torch.equal(sc, sc2), pad
    # bf16: converted to fp32 first, as attribute_input_packed does
    lvb, ofb, _, _ = common.fused(ctx.bfloat16(), pairs, offsets, vp, op, K)
    lvf, off_, _, _ = common.fused(ctx.bfloat16().float(), pairs, offsets, vp, op, K)
    assert _bits_equal(lvb, lvf) and _bits_equal(ofb, off_) and not _bits_equal(lvb, lv)
    # k_cap: rows past offsets[-1] with pairs clamped into the segment give finite outputs, the last chain's indices, and leave the
    # real rows bit-unchanged
    cap = K + _R() + 5
    extra = torch.randint(-3, T + 3, (cap - K, 2), generator=torch.Generator().manual_seed(73), dtype=torch.int32).clamp(0, T - 1)
    pairs_cap = torch.cat([pairs0, extra]).to(dev)
    lv3, of3, sym3, sc3 = common.fused(ctx, pairs_cap, offsets, vp, op, cap)
    assert lv3.shape == (cap, 128) and bool(torch.isfinite(lv3).all()) and bool(torch.isfinite(of3).all())
    assert _bits_equal(lv3[:K], lv) and _bits_equal(of3[:K], of) and torch.equal(sym3[:K], sym) and torch.equal(sc3[:K], sc)
    assert bool((sc3[K:] == common.N_SEG * common.N_SYM - 1).all())


@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_views_cpu(D, Hv, Ho):
    _check_views(CPU, D, Hv, Ho)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_views_gpu(gpu, D, Hv, Ho):
    _check_views(gpu, D, Hv, Ho)


# ---- 4. symIdx / scatterIdx as the gather writes them -----------------------------------------------------------------------------------
def _check_golden_indices(dev, name):
    from test_oracle_golden import _attr_case
    from transkun_amd import _lib
    g, ctx, flat, batch, (N, SYM, T, D) = _attr_case(name)
    pairs = torch.from_numpy(g["pairs"]).to(torch.int32).reshape(-1, 2).to(dev)
    offsets = torch.from_numpy(g["offsets"]).to(torch.int32).to(dev)
    K = pairs.shape[0]
    assert K > 0 and int(offsets[-1]) == K
    vp, op = common.make_heads(D, 8, 4, 81)
    vp, op, ctx = common.to_device(dev, vp, op, ctx)
    lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, K)
    assert torch.equal(sym.cpu(), torch.from_numpy(g["symIdx"]).long()) and torch.equal(sc.cpu(), torch.from_numpy(g["scatterIdx"]).long())
    if dev.type == "cuda":                                    # and the gather kernel's own, on the device
        from transkun_amd import attributes
        _, gsym, gsc = attributes.attribute_input_packed(ctx, pairs, offsets, K)
        assert torch.equal(sym, gsym) and torch.equal(sc, gsc)
    # null index outputs (empty tensors through the torch op): accepted, the same logits
    from transkun_amd.attributes import _packed_heads
    w = _packed_heads(vp, op)
    lv2, of2 = torch.empty_like(lv), torch.empty_like(of)
    none = torch.empty(0, dtype=torch.int64, device=dev)
    ws = torch.empty(0 if dev.type == "cpu" else int(_lib.load().semicrf_attribute_heads_workspace_bytes(K, 8, 4, 128, 4)), dtype=torch.uint8,
                     device=dev)
    _lib.ops().attribute_heads(ctx.view(N * SYM, T, D), N * SYM, T, D, D, pairs, K, offsets, SYM, w["W1"], w["b1"], w["W2"], w["b2"], 8, 4, 128, 4,
                               lv2, of2, none, none, ws)
    assert _bits_equal(lv, lv2) and _bits_equal(of, of2)


@pytest.mark.parametrize("name", ["small", "model"])
def test_indices_equal_the_gathers_cpu(name):
    _check_golden_indices(CPU, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "model"])
def test_indices_equal_the_gathers_gpu(gpu, name):
    _check_golden_indices(gpu, name)


# ---- 5. non-finite values stay in their rows ---------------------------------------------------------------------------------------
def _check_nonfinite(dev, D, Hv, Ho):
    vp0, op0, ctx0 = _small_case(91, D, Hv, Ho)
    K = _R() + 9
    rows = common.make_rows(K, 92)
    pairs0, offsets0 = common.pack_rows(rows)
    vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx0, pairs0, offsets0)
    clean = common.fused(ctx, pairs, offsets, vp, op, K)
    c, f = rows[K // 2][0], rows[K // 2][1]                                        # one (chain, frame) that some row reads
    hit = torch.tensor([rc == c and (b == f or e == f) for rc, b, e in rows])
    assert bool(hit.any()) and not bool(hit.all())
    for bad in (float("nan"), float("inf"), float("-inf")):
        dirty = ctx.clone()
        dirty[c // common.N_SYM, c % common.N_SYM, f, D // 2] = bad
        lv, of, _, _ = common.fused(dirty, pairs, offsets, vp, op, K)
        lv, of = lv.cpu(), of.cpu()
        assert not bool(torch.isfinite(lv[hit]).any()) and not bool(torch.isfinite(of[hit]).any()), bad
        assert _bits_equal(lv[~hit], clean[0].cpu()[~hit]) and _bits_equal(of[~hit], clean[1].cpu()[~hit]), bad


@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_nonfinite_rows_cpu(D, Hv, Ho):
    _check_nonfinite(CPU, D, Hv, Ho)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_nonfinite_rows_gpu(gpu, D, Hv, Ho):
    _check_nonfinite(gpu, D, Hv, Ho)


# ---- 7. the packed weights follow the parameters -----------------------------------------------------------------------------------
def _check_cache(dev):
    vp0, op0, ctx0 = _small_case(101)
    K = 40
    pairs0, offsets0 = common.pack_rows(common.make_rows(K, 102))
    vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx0, pairs0, offsets0)
    first = common.fused(ctx, pairs, offsets, vp, op, K)
    state = copy.deepcopy({"vp": vp.state_dict(), "op": op.state_dict()})
    # an optimizer step writes the parameters in place
    opt = torch.optim.SGD(list(vp.parameters()) + list(op.parameters()), lr=0.5)
    for p in list(vp.parameters()) + list(op.parameters()):
        p.grad = torch.ones_like(p)
    opt.step()
    stepped = common.fused(ctx, pairs, offsets, vp, op, K)
    fresh = common.fused(ctx, pairs, offsets, copy.deepcopy(vp), copy.deepcopy(op), K)       # new modules: packed from scratch
    assert _bits_equal(stepped[0], fresh[0]) and _bits_equal(stepped[1], fresh[1])
    assert not _bits_equal(stepped[0], first[0]) and not _bits_equal(stepped[1], first[1])
    tv, to, bv, bo, _ = common.truth_and_bound(ctx0, pairs0, offsets0, K, copy.deepcopy(vp).cpu(), copy.deepcopy(op).cpu())
    assert bool(((stepped[0].cpu().double() - tv).abs() <= bv).all()) and bool(((stepped[1].cpu().double() - to).abs() <= bo).all())
    # load_state_dict copies in place as well
    vp.load_state_dict(state["vp"]); op.load_state_dict(state["op"])
    back = common.fused(ctx, pairs, offsets, vp, op, K)
    assert _bits_equal(back[0], first[0]) and _bits_equal(back[1], first[1])


def test_weights_cache_cpu():
    _check_cache(CPU)


@pytest.mark.gpu
def test_weights_cache_gpu(gpu):
    _check_cache(gpu)


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------------
def test_training_mode_with_dropout_raises():
    from transkun_amd import attributes
    vp, op, ctx = _small_case(111)
    pairs, offsets = common.pack_rows(common.make_rows(5, 112))
    vp.train()
    with pytest.raises(ValueError, match="training mode with dropout"), torch.no_grad():
        attributes.attribute_heads(ctx, pairs, offsets, vp, op, 5)
    vp.eval(); op.train()
    with pytest.raises(ValueError, match="training mode with dropout"), torch.no_grad():
        attributes.attribute_heads(ctx, pairs, offsets, vp, op, 5)
    # training mode with p = 0 is the identity: allowed
    vp2, op2 = common.make_heads(20, 40, 24, 111, dropout=0.0)
    vp2.train(); op2.train()
    a = common.fused(ctx, pairs, offsets, vp2, op2, 5)
    b = common.fused(ctx, pairs, offsets, vp2.eval(), op2.eval(), 5)
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])


def test_requires_grad_under_grad_mode_raises():
    from transkun_amd import attributes
    vp, op, ctx = _small_case(121)
    pairs, offsets = common.pack_rows(common.make_rows(5, 122))
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="forward-only"):                   # the parameters require grad
            attributes.attribute_heads(ctx, pairs, offsets, vp, op, 5)
        for p in list(vp.parameters()) + list(op.parameters()):
            p.requires_grad_(False)
        attributes.attribute_heads(ctx, pairs, offsets, vp, op, 5)                # nothing requires grad: fine
        with pytest.raises(RuntimeError, match="forward-only"):
            attributes.attribute_heads(ctx.clone().requires_grad_(), pairs, offsets, vp, op, 5)
    with torch.no_grad():
        attributes.attribute_heads(ctx.clone().requires_grad_(), pairs, offsets, vp, op, 5)


def test_attribute_heads_route_is_validated():
    from transkun_amd.transcribe import SegmentTranscriber
    m = SegmentTranscriber(size=8, velocityPredictorHiddenSize=8, refinedOFPredictorHiddenSize=8, targetMIDIPitch=[60])
    assert m.attributeHeads == "torch"
    m.attributeHeads = "hip"
    with pytest.raises(ValueError, match="attributeHeads must be 'torch' or 'fused'"):
        m.decode_step(torch.zeros(1, 1, 4, 8), None, torch.zeros(1, dtype=torch.float64), 3, 0)
    with pytest.raises(ValueError, match="attributeHeads must be 'torch' or 'fused'"):
        m.computeStats(torch.zeros(1, 1, 4, 8), [[[]]], [], [])


def test_c_abi_rejects_bad_arguments_without_gpu():
    """semicrf_attribute_heads: every bad argument is rejected with a message before any pointer is used; K = 0 launches nothing."""
    from transkun_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(4096)                             # never dereferenced: the argument checks come first
    need = lib.semicrf_attribute_heads_workspace_bytes(8, 16, 16, 128, 4)
    assert need >= 8 * (128 + 4) * 4
    assert lib.semicrf_workspace_bytes(_lib.OP_ATTRIBUTE_HEADS, 8, 32) >= need
    assert lib.semicrf_workspace_bytes(_lib.OP_ATTRIBUTE_HEADS, 1400, 1024) >= lib.semicrf_attribute_heads_workspace_bytes(1400, 512, 512, 128, 4)
    assert lib.semicrf_attribute_heads_workspace_bytes(-1, 16, 16, 128, 4) == 0

    def call(ctx=f, C=2, T=4, D=8, ldc=8, pairs=f, K=8, offsets=f, nSym=1, W1=f, b1=f, W2=f, b2=f, Hv=16, Ho=16, Nv=128, No=4, lv=f, of=f,
             sym=f, sc=f, ws=f, ws_bytes=need):
        return lib.semicrf_attribute_heads(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, lv, of, sym, sc, ws,
                                           ws_bytes, None)

    for kw, word in ((dict(ctx=None), b"NULL"), (dict(offsets=None), b"NULL"), (dict(W1=None), b"NULL"), (dict(b1=None), b"NULL"),
                     (dict(W2=None), b"NULL"), (dict(b2=None), b"NULL"), (dict(pairs=None), b"NULL"), (dict(lv=None), b"NULL"),
                     (dict(of=None), b"NULL"), (dict(ws=None), b"NULL"), (dict(K=-1), b"interval count"), (dict(C=0), b"must be >= 1"),
                     (dict(T=0), b"must be >= 1"), (dict(D=0), b"must be >= 1"), (dict(nSym=0), b"must be >= 1"),
                     (dict(Hv=0), b"must be >= 1"), (dict(Ho=-2), b"must be >= 1"), (dict(Nv=0), b"must be >= 1"),
                     (dict(No=0), b"must be >= 1"), (dict(ldc=7), b"row stride")):
        assert call(**kw) == 1, kw
        assert word in lib.semicrf_last_error(), (kw, lib.semicrf_last_error())
    assert call(ws_bytes=need - 1) == 2 and b"workspace too small" in lib.semicrf_last_error()
    assert call(K=0, pairs=None, lv=None, of=None, sym=None, sc=None, ws=None, ws_bytes=0) == 0       # nothing to do, nothing launched
    assert call(K=0, ctx=None) == 1


# ---- 6. the reference's goldens through the transcriber; 9. graph capture, no host wait (device only) ----------------------------
def _transcriber(name, gpu):
    import test_gpu_parity
    return test_gpu_parity._transcriber(name, gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("decode", ["torch", "fused"])
@pytest.mark.parametrize("name", ["small", "real"])
def test_transcribe_end_to_end_fused_heads_vs_reference(gpu, name, decode, monkeypatch):
    """test_transcribe_end_to_end_vs_reference with attributeHeads = "fused" (alone, and with attributeDecode = "fused"), under that
    test's conditions and tolerances -- the final notes, and per segment the reference's own head outputs: head{i}_velocity_argmax
    (mismatches in at most 0.5 % of the rows), the sign of head{i}_of's presence logits (0.05 %), head{i}_ofValue (2e-4 s), and
    head{i}_of itself, torch's fp32 modules on the reference's CPU, under the gate: the fused logits err against float64 by at most
    8 x what the stored ones do."""
    from segment_common import golden_events
    from transkun_amd import attributes
    g = load_golden("transcribe_" + name)
    m, I = _transcriber(name, gpu)
    m.attributeHeads, m.attributeDecode = "fused", decode
    seen = []
    real_op = attributes.attribute_heads

    def recording(ctx, pairs, offsets, vp, op, K=None):
        out = real_op(ctx, pairs, offsets, vp, op, K)
        seen.append((ctx, pairs.clone(), offsets.clone(), K, out[0].clone(), out[1].clone()))
        return out

    monkeypatch.setattr(attributes, "attribute_heads", recording)
    events = m.transcribe(lambda i, T: I["ctxs"][i], I["n_sample_unpadded"])
    want = golden_events(g, "final")
    assert len(events) == len(want)
    by_pitch_got, by_pitch_want = {}, {}
    for e in events:
        by_pitch_got.setdefault(e.pitch, []).append((e.start, e.end, e.velocity, e.hasOnset, e.hasOffset))
    for e in want:
        by_pitch_want.setdefault(e[2], []).append((e[0], e[1], e[3], e[4], e[5]))
    assert sorted(by_pitch_got) == sorted(by_pitch_want)
    n_time, n_vel, n_flag, worst = 0, 0, 0, 0.0
    for pitch, wl in by_pitch_want.items():
        gl = sorted(by_pitch_got[pitch]); wl = sorted(wl)
        assert len(gl) == len(wl), pitch
        for a, b in zip(gl, wl):
            dt = max(abs(a[0] - b[0]), abs(a[1] - b[1]))
            worst = max(worst, dt)
            n_time += dt > 2e-4
            n_vel += a[2] != b[2]
            n_flag += a[3:] != b[3:]
    print(name, decode, "fused heads: events", len(want), "time mismatches", n_time, "velocity mismatches", n_vel, "flag mismatches", n_flag,
          "worst dt", worst)
    assert n_time == 0 and n_flag <= len(want) // 2000 and n_vel <= len(want) // 200, (n_time, n_vel, n_flag)
    # per segment with intervals: the reference's head outputs
    assert len(seen) > 0 and f"head{len(seen) - 1}_of" in g and f"head{len(seen)}_of" not in g
    frame = I["hop"] / I["fs"]
    rows = bad_vel = bad_pres = 0
    vp64, op64 = copy.deepcopy(m.velocityPredictor).cpu(), copy.deepcopy(m.refinedOFPredictor).cpu()
    e_fused = e_stored = 0.0
    for i, (ctx, pairs, offsets, cap, lv, of) in enumerate(seen):
        stored = torch.from_numpy(g[f"head{i}_of"])
        K = int(offsets[-1])                                  # transcribe sizes a step by its cap: the rows behind K are not the reference's
        assert 0 < K <= cap and of.shape == (cap, 4) and stored.shape == (K, 4)
        assert bool(torch.isfinite(lv).all()) and bool(torch.isfinite(of).all())
        lv, of, pairs = lv[:K], of[:K], pairs[:K]
        bad_vel += int((lv.argmax(-1).cpu() != torch.from_numpy(g[f"head{i}_velocity_argmax"]).long()).sum())
        bad_pres += int(((of[:, 2:] > 0).cpu() != (stored[:, 2:] > 0)).sum())
        _, val, _ = attributes.attribute_decode(lv, of, "hamming")
        assert float((val.cpu() - torch.from_numpy(g[f"head{i}_ofValue"])).abs().max()) * frame <= 2e-4, i
        _, to, _, bo, _ = common.truth_and_bound(ctx.cpu(), pairs.cpu(), offsets.cpu(), K, vp64, op64)
        err = (of.cpu().double() - to).abs()
        assert bool((err <= bo).all()), i
        e_fused, e_stored = max(e_fused, float(err.max())), max(e_stored, float((stored.double() - to).abs().max()))
        rows += K
    print(f"{name}: {rows} rows; velocity argmax mismatches {bad_vel}, presence sign mismatches {bad_pres}; ofLogits against float64: "
          f"fused {e_fused:.3e}  the reference's fp32 (stored) {e_stored:.3e}  ratio {e_fused / e_stored:.2f}")
    assert bad_vel <= rows // 200 and bad_pres <= 2 * rows // 2000
    assert e_fused <= common.GATE * e_stored


@pytest.mark.gpu
def test_transcribe_many_fused_heads_one_recording_at_a_time(gpu):
    """transcribe_many (lock step: k_cap rows per step, no host wait for the count) with the fused heads, one recording at a time:
    exactly the events of its synchronous run, which sizes every step by its count -- the op's rows do not depend on K or on the
    rows behind."""
    m, I = _transcriber("small", gpu)
    m.attributeHeads = m.attributeDecode = "fused"
    n_full = I["n_sample_unpadded"]
    fn_a = lambda i, T: I["ctxs"][i]
    fn_b = lambda i, T: I["ctxs"][(i + 2) % len(I["ctxs"])]
    for fn, n in ((fn_a, n_full), (fn_b, int(n_full * 0.55))):
        capped = m.transcribe_many([fn], [n])
        waited = m.transcribe_many([fn], [n], synchronous=True)
        assert len(capped[0]) > 0 and [e.astuple() for e in capped[0]] == [e.astuple() for e in waited[0]]
        assert [e.astuple() for e in m.transcribe(fn, n)] == [e.astuple() for e in capped[0]]


@pytest.mark.gpu
def test_compute_stats_fused_heads(gpu):
    """computeStats with attributeHeads = "fused" against the torch route, on the shape of attr_loss_small: the six counts are
    identical (they do not depend on the heads), the two squared errors agree to fp32 round-off of the logits."""
    import attr_loss_common
    g = load_golden("attr_loss_small")
    model, ctx = attr_loss_common.golden_transcriber(gpu)
    model.eval()
    batch, vel, refined, _ = attr_loss_common.golden_targets(g)
    a = model.computeStats(ctx, batch, vel, refined)
    model.attributeHeads = "fused"
    for route in ("torch", "fused"):
        b = model.computeStats(ctx, batch, vel, refined, attributeRoute=route)
        for k in ("nGT", "nEst", "nCorrect", "nGTFramewise", "nEstFramewise", "nCorrectFramewise"):
            assert a[k] == b[k], (route, k)
        assert a["nGT"] > 0
        for k in ("seOFForced", "seVelocityForced"):
            print(f"computeStats {k} [{route}]: torch heads {a[k]:.9g}  fused heads {b[k]:.9g}")
            assert a[k] > 0 and abs(a[k] - b[k]) <= 1e-3 * a[k], (route, k)      # (logits that agree to ~1e-6: a sanity check, no gate)


@pytest.mark.gpu
def test_graph_capture_and_no_host_wait(gpu):
    """The op captured into a graph and replayed gives the eager call's bits; under torch's sync debug mode ("error": any synchronising
    torch call raises) a warm call runs through; the device status word stays 0."""
    from transkun_amd import _lib
    c = common.gate_case(256, 512, 512, 1.0)
    vp, op, ctx, pairs, offsets = common.to_device(gpu, c["vp"], c["op"], c["ctx"], c["pairs"], c["offsets"])
    K = c["K"]
    eager = common.fused(ctx, pairs, offsets, vp, op, K)
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        for _ in range(2):                                                    # warm-up on the side stream (allocator, lazy loads)
            common.fused(ctx, pairs, offsets, vp, op, K)
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = common.fused(ctx, pairs, offsets, vp, op, K)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = common.fused(ctx, pairs, offsets, vp, op, K)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(again, eager):
        assert torch.equal(a, b)
    assert _lib.device_status() == 0
