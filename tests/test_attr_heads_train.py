"""The attribute heads in training: transkun_amd.attributes.attribute_heads_train (csrc/attr_heads.hip in its training mode and
csrc/attr_heads_bwd.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on CPU tensors), attribute_heads_dropout_mask and
SegmentTranscriber.log_prob(attributeHeads="fused").

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  Yardstick and gate: attr_heads_train_common.
Measured ratios: DESIGN.md section 3, "Attribute heads, training", and profiles/attr_heads_train_bench.json."""
import copy
import ctypes

import pytest
import torch

import attr_heads_common as common
import attr_heads_train_common as tc

CPU = torch.device("cpu")
P_CASES = [(D, Hv, Ho, s, 0.1, 0.1) for (D, Hv, Ho) in common.SHAPES for s in common.SCALES] + \
          [(D, Hv, Ho, 1.0, 0.1, 0.5) for (D, Hv, Ho) in common.SHAPES]


def _attributes():
    from transkun_amd import attributes
    return attributes


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- 1. eval mode (and training mode with p = 0): the bits of attribute_heads -------------------------------------------------------
def _check_eval_bits(dev, D, Hv, Ho):
    A = _attributes()
    c = common.gate_case(D, Hv, Ho, 1.0)
    vp, op, ctx, pairs, offsets = common.to_device(dev, c["vp"], c["op"], c["ctx"], c["pairs"], c["offsets"])
    K = c["K"]
    want = common.fused(ctx, pairs, offsets, vp, op, K)
    got = A.attribute_heads_train(ctx.clone().requires_grad_(), pairs, offsets, vp, op, K)
    assert got[0].requires_grad and got[1].requires_grad and not got[2].requires_grad
    assert _bits_equal(got[0].detach(), want[0]) and _bits_equal(got[1].detach(), want[1])
    assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    vp0, op0 = common.make_heads(D, Hv, Ho, 1000 + 7 * D + Hv + 1, dropout=0.0)       # gate_case's heads (scale 1) with p = 0 ...
    vp0, op0 = copy.deepcopy(vp0).to(dev).train(), copy.deepcopy(op0).to(dev).train()  # ... in training mode
    got0 = A.attribute_heads_train(ctx, pairs, offsets, vp0, op0, K, seed=5)
    assert _bits_equal(got0[0].detach(), want[0]) and _bits_equal(got0[1].detach(), want[1])


@pytest.mark.parametrize("D,Hv,Ho", common.SHAPES)
def test_eval_forward_is_attribute_heads_cpu(D, Hv, Ho):
    _check_eval_bits(CPU, D, Hv, Ho)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho", common.SHAPES)
def test_eval_forward_is_attribute_heads_gpu(gpu, D, Hv, Ho):
    _check_eval_bits(gpu, D, Hv, Ho)


# ---- 2., 3. the gate: training-mode forward and the nine gradients against the float64 modules ---------------------------------------
def _check_gate(dev, D, Hv, Ho, scale, pv, po):
    c = tc.gate_case(D, Hv, Ho, scale, pv, po)
    lv, of, grads = tc.run_op(dev, c)
    assert grads[0].shape == c["ctx"].shape and grads[0].dtype == torch.float32 and grads[0].device == lv.device
    tag = f"attribute_heads_train [{dev.type}] D={D} Hv={Hv} Ho={Ho} scale={scale:g} p={pv:g}/{po:g}"
    tc.check_gate(tag, ("logitsVelocity", "ofLogits") + tc.NAMES, [lv, of] + grads, c["truth"], c["e32"])


@pytest.mark.parametrize("D,Hv,Ho,scale,pv,po", P_CASES)
def test_forward_and_gradient_gate_cpu(D, Hv, Ho, scale, pv, po):
    _check_gate(CPU, D, Hv, Ho, scale, pv, po)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,scale,pv,po", P_CASES)
def test_forward_and_gradient_gate_gpu(gpu, D, Hv, Ho, scale, pv, po):
    _check_gate(gpu, D, Hv, Ho, scale, pv, po)


# ---- 4. sums over rows across the row chunks -----------------------------------------------------------------------------------------
def _check_chunks(dev, D, Hv, Ho):
    R = _attributes().HEADS_BWD_ROW_CHUNK
    assert R >= 2
    c = tc.chunk_case(D, Hv, Ho, 3 * R + 37)
    lv, of, grads = tc.run_op(dev, c)
    tc.check_gate(f"row chunks [{dev.type}] K={c['K']} D={D}", ("logitsVelocity", "ofLogits") + tc.NAMES, [lv, of] + grads, c["truth"], c["e32"])
    lv2, of2, grads2 = tc.run_op(dev, c)
    assert _bits_equal(lv, lv2) and _bits_equal(of, of2)
    for name, a, b in zip(tc.NAMES, grads, grads2):
        assert _bits_equal(a, b), name


def test_row_chunks_cpu():
    _check_chunks(CPU, 20, 40, 24)


@pytest.mark.gpu
def test_row_chunks_gpu(gpu):
    _check_chunks(gpu, 256, 512, 512)


# ---- 5. determinism; a row does not depend on K or on the other rows, in training mode ------------------------------------------------
@pytest.mark.gpu
def test_gradients_are_deterministic_gpu(gpu):
    c = tc.make_case(256, 512, 512, 1.0, 0.1, 0.1, 300, 4100)
    lv, of, grads = tc.run_op(gpu, c)
    lv2, of2, grads2 = tc.run_op(gpu, c)
    assert _bits_equal(lv, lv2) and _bits_equal(of, of2)
    for name, a, b in zip(tc.NAMES, grads, grads2):
        assert _bits_equal(a, b), name
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name


def _check_row_independence(dev, D, Hv, Ho):
    """One row (chain 5, frames 2..9), training mode, one seed.  At global index 0: alone (K = 1) and first among other rows.  At global
    index n: last (K = n + 1) and in the middle of other rows.  Each pair the same bits (the mask reads the global index), also with
    every frame the row does not read replaced by NaN."""
    A = _attributes()
    R = A.HEADS_ROW_TILE
    vp0, op0 = tc.make_train_heads(D, Hv, Ho, 61)
    ctx0 = common.make_ctx(D, 1.0, 62)
    target = (5, 2, 9)
    g = torch.Generator().manual_seed(63)

    def others(n, chains):
        rows = []
        for _ in range(n):
            b = int(torch.randint(0, common.T_FRAMES, (1,), generator=g)); e = int(torch.randint(b, common.T_FRAMES, (1,), generator=g))
            rows.append((chains[int(torch.randint(0, len(chains), (1,), generator=g))], b, e))
        return sorted(rows, key=lambda r: r[0])

    before, after = others(R + 6, [0, 2, 3, 5]), others(R + 3, [5, 6, 7, 8])
    nan = torch.full_like(ctx0, float("nan"))
    nan[1, 0, 2] = ctx0[1, 0, 2]; nan[1, 0, 9] = ctx0[1, 0, 9]               # chain 5 = [1, 0]
    for group in ({"alone": ([target], 0), "first": ([target] + after, 0)},
                  {"last": (before + [target], len(before)), "middle": (before + [target] + after, len(before))}):
        ref = None
        for tag, (rows, at) in group.items():
            for ctx_h in (ctx0, nan):
                pairs0, offsets0 = common.pack_rows(rows)
                vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx_h, pairs0, offsets0)
                vp.train(); op.train()
                with torch.no_grad():
                    lv, of, sym, sc = A.attribute_heads_train(ctx, pairs, offsets, vp, op, len(rows), seed=77)
                assert int(sc[at]) == 5 and int(sym[at]) == 0
                row = (lv[at].cpu().clone(), of[at].cpu().clone())
                if ref is None:
                    ref = row
                    assert bool(torch.isfinite(ref[0]).all()) and float(ref[0].abs().max()) > 0
                assert _bits_equal(row[0], ref[0]) and _bits_equal(row[1], ref[1]), tag


@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (5, 3, 1)])
def test_row_independence_cpu(D, Hv, Ho):
    _check_row_independence(CPU, D, Hv, Ho)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho", [(20, 40, 24), (256, 512, 512)])
def test_row_independence_gpu(gpu, D, Hv, Ho):
    _check_row_independence(gpu, D, Hv, Ho)


# ---- 6. the mask -----------------------------------------------------------------------------------------------------------------------
def _check_mask(dev):
    K, Hv, Ho = 97, 512, 512
    a = tc.mask_of(11, K, Hv, Ho, 0.1, 0.1, dev)
    assert a.shape == (K, Hv + Ho) and a.dtype == torch.bool and a.device.type == dev.type
    assert torch.equal(a, tc.mask_of(11, K, Hv, Ho, 0.1, 0.1, dev))
    assert not torch.equal(a, tc.mask_of(12, K, Hv, Ho, 0.1, 0.1, dev))
    assert not torch.equal(a, tc.mask_of(11 + (1 << 32), K, Hv, Ho, 0.1, 0.1, dev))          # the high word of the seed counts
    assert torch.equal(tc.mask_of(11, 30, Hv, Ho, 0.1, 0.1, dev), a[:30])                    # the first rows do not depend on K
    assert torch.equal(tc.mask_of(11, K + 200, Hv, Ho, 0.1, 0.1, dev)[:K], a)
    assert torch.equal(a.cpu(), tc.mask_of(11, K, Hv, Ho, 0.1, 0.1, "cpu"))                  # device = host mirror
    # keep rate within 5 standard deviations of 1 - p over the 99 328 draws; a head with p = 0 keeps everything
    n = K * (Hv + Ho)
    for seed, p in ((21, 0.1), (22, 0.1), (23, 0.5), (24, 0.5)):
        rate = float(tc.mask_of(seed, K, Hv, Ho, p, p, dev).float().mean())
        print(f"mask [{dev.type}] seed {seed} p {p}: keep rate {rate:.5f}")
        assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5, (seed, p, rate)
    m = tc.mask_of(25, K, Hv, Ho, 0.0, 0.5, dev)
    assert bool(m[:, :Hv].all()) and abs(float(m[:, Hv:].float().mean()) - 0.5) <= 5 * (0.25 / (K * Ho)) ** 0.5


def test_mask_cpu():
    _check_mask(CPU)


@pytest.mark.gpu
def test_mask_gpu(gpu):
    _check_mask(gpu)


def _check_default_seed(dev):
    A = _attributes()
    vp0, op0 = tc.make_train_heads(20, 40, 24, 81)
    ctx0 = common.make_ctx(20, 1.0, 82)
    pairs0, offsets0 = common.pack_rows(common.make_rows(40, 83))
    vp, op, ctx, pairs, offsets = common.to_device(dev, vp0, op0, ctx0, pairs0, offsets0)
    vp.train(); op.train()

    def run(seed=None):
        with torch.no_grad():
            return A.attribute_heads_train(ctx, pairs, offsets, vp, op, 40, seed=seed)[0]

    torch.manual_seed(1234)
    a1, a2 = run(), run()
    torch.manual_seed(1234)
    b1 = run()
    assert _bits_equal(a1, b1) and not _bits_equal(a1, a2)                   # manual_seed reproduces; the generator advances
    assert _bits_equal(run(9), run(9)) and not _bits_equal(run(9), run(10))  # an explicit seed
    state = torch.random.get_rng_state()
    run(9)
    assert torch.equal(state, torch.random.get_rng_state())                  # an explicit seed leaves the generator alone


def test_default_seed_cpu():
    _check_default_seed(CPU)


@pytest.mark.gpu
def test_default_seed_gpu(gpu):
    _check_default_seed(gpu)


# ---- 7. views and dtypes ---------------------------------------------------------------------------------------------------------------
def _check_views(dev):
    A = _attributes()
    c = tc.gate_case(20, 40, 24, 1.0)
    K, D = c["K"], 20
    lv, of, grads = tc.run_op(dev, c)
    vp, op = copy.deepcopy(c["vp"]).to(dev).train(), copy.deepcopy(c["op"]).to(dev).train()
    pairs, offsets, dlv, dof = (c[k].to(dev) for k in ("pairs", "offsets", "dlv", "dof"))
    # a view with a row stride above D (a multiple of four floats, and not): the same bits, dctx in the view's shape
    for pad in (4, 3):
        big = torch.full((common.N_SEG, common.N_SYM, common.T_FRAMES, D + pad), 1e30, device=dev)
        big[..., :D] = c["ctx"].to(dev)
        view = big[..., :D].requires_grad_()
        assert view.stride(2) == D + pad and not view.is_contiguous()
        lv2, of2, _, _ = A.attribute_heads_train(view, pairs, offsets, vp, op, K, seed=c["seed"])
        g2 = torch.autograd.grad([lv2, of2], [view] + tc.params_of(vp, op), [dlv, dof])
        assert _bits_equal(lv2.detach(), lv) and _bits_equal(of2.detach(), of)
        for name, a, b in zip(tc.NAMES, grads, g2):
            assert _bits_equal(a, b), (pad, name)
    # float64 ctx: converted to fp32 first, dctx comes back in float64
    ctx64 = c["ctx"].to(dev).double().requires_grad_()
    lv3, of3, _, _ = A.attribute_heads_train(ctx64, pairs, offsets, vp, op, K, seed=c["seed"])
    (g3,) = torch.autograd.grad([lv3, of3], [ctx64], [dlv, dof])
    assert g3.dtype == torch.float64 and g3.shape == ctx64.shape and torch.equal(g3, grads[0].double())
    # a Linear without a bias gets no gradient; the others' gradients do not change
    vpn = copy.deepcopy(vp)
    vpn[0].bias = None
    ctx = c["ctx"].detach().to(dev).requires_grad_()            # a leaf of its own: the cached case stays as it is
    lv4, of4, _, _ = A.attribute_heads_train(ctx, pairs, offsets, vpn, op, K, seed=c["seed"])
    (lv4 * dlv).sum().add((of4 * dof).sum()).backward()
    assert vpn[0].bias is None and vpn[0].weight.grad is not None and vpn[-1].bias.grad is not None and ctx.grad is not None
    assert _bits_equal(op[0].weight.grad, grads[5]) and _bits_equal(op[-1].bias.grad, grads[8])
    # bf16 parameters
    with pytest.raises(TypeError, match="float32"):
        A.attribute_heads_train(ctx, pairs, offsets, copy.deepcopy(vp).bfloat16(), op, K, seed=1)
    # double backward
    ctx = c["ctx"].detach().to(dev).requires_grad_()            # a leaf of its own: the cached case stays as it is
    lv5, of5, _, _ = A.attribute_heads_train(ctx, pairs, offsets, vp, op, K, seed=c["seed"])
    (g5,) = torch.autograd.grad([lv5, of5], [ctx], [dlv, dof], create_graph=True)
    with pytest.raises(RuntimeError):
        g5.sum().backward()
    # K = 0: empty results, zero gradients
    e_pairs, e_off = common.pack_rows([])
    lv6, of6, sym6, sc6 = A.attribute_heads_train(ctx, e_pairs.to(dev), e_off.to(dev), vp, op, 0)
    assert lv6.shape == (0, 128) and of6.shape == (0, 4) and sym6.shape == sc6.shape == (0,)
    (g6,) = torch.autograd.grad([lv6.sum() + of6.sum()], [ctx])
    assert g6.shape == ctx.shape and float(g6.abs().max()) == 0.0


def test_views_and_dtypes_cpu():
    _check_views(CPU)


@pytest.mark.gpu
def test_views_and_dtypes_gpu(gpu):
    _check_views(gpu)


# ---- 8. the C ABI without a GPU --------------------------------------------------------------------------------------------------------
def test_c_abi_rejects_bad_arguments_without_gpu():
    """The three new entry points: every bad argument is rejected with a message before any pointer is used; K = 0 launches nothing; a
    short workspace is SEMICRF_EWORKSPACE."""
    from transkun_amd import _lib
    lib = _lib.load()
    f = ctypes.c_void_p(4096)                             # never dereferenced: the argument checks come first
    need = lib.semicrf_attribute_heads_train_fwd_workspace_bytes(8, 16, 16, 128, 4)
    assert need == lib.semicrf_attribute_heads_workspace_bytes(8, 16, 16, 128, 4) > 0
    need_b = lib.semicrf_attribute_heads_bwd_workspace_bytes(8, 8, 16, 16, 128, 4)
    # dz, (ga, gb), the frames and one plane of the parameter gradients
    assert need_b >= 4 * (8 * 32 + 8 * 2 * 8 + 2 * 8 + 24 * 32 + 32 + 16 * 132 + 132)
    assert lib.semicrf_attribute_heads_bwd_workspace_bytes(-1, 8, 16, 16, 128, 4) == 0
    assert lib.semicrf_attribute_heads_bwd_workspace_bytes(8, 0, 16, 16, 128, 4) == 0
    assert lib.semicrf_workspace_bytes(_lib.OP_ATTRIBUTE_HEADS_BWD, 8, 32) >= need_b
    assert lib.semicrf_workspace_bytes(_lib.OP_ATTRIBUTE_HEADS_BWD, 7831, 1024) >= lib.semicrf_attribute_heads_bwd_workspace_bytes(7831, 256, 512, 512, 128, 4)
    R = _lib.HEADS_BWD_ROW_CHUNK
    plane = lib.semicrf_attribute_heads_bwd_workspace_bytes(R + 1, 8, 16, 16, 128, 4) - lib.semicrf_attribute_heads_bwd_workspace_bytes(R, 8, 16, 16, 128, 4)
    assert plane >= 4 * (24 * 32 + 32 + 16 * 132 + 132)      # one more row past a chunk: one more plane

    def fwd(ctx=f, C=2, T=4, D=8, ldc=8, pairs=f, K=8, offsets=f, nSym=1, W1=f, b1=f, W2=f, b2=f, Hv=16, Ho=16, Nv=128, No=4, seed=1, pv=0.1,
            po=0.1, lv=f, of=f, z=f, sym=f, sc=f, ws=f, ws_bytes=need):
        return lib.semicrf_attribute_heads_train_fwd(ctx, C, T, D, ldc, pairs, K, offsets, nSym, W1, b1, W2, b2, Hv, Ho, Nv, No, seed, pv, po, lv,
                                                     of, z, sym, sc, ws, ws_bytes, None)

    def bwd(dlv=f, dof=f, z=f, ctx=f, C=2, T=4, D=8, ldc=8, pairs=f, K=8, offsets=f, W1=f, W2=f, Hv=16, Ho=16, Nv=128, No=4, seed=1, pv=0.1,
            po=0.1, dctx=f, dW1=f, db1=f, dW2=f, db2=f, ws=f, ws_bytes=need_b):
        return lib.semicrf_attribute_heads_bwd(dlv, dof, z, ctx, C, T, D, ldc, pairs, K, offsets, W1, W2, Hv, Ho, Nv, No, seed, pv, po, dctx, dW1,
                                               db1, dW2, db2, ws, ws_bytes, None)

    def mask(seed=1, K=8, Hv=16, Ho=16, pv=0.1, po=0.1, m=f):
        return lib.semicrf_attribute_heads_dropout_mask(seed, K, Hv, Ho, pv, po, m, None)

    sizes = ((dict(K=-1), b"interval count"), (dict(C=0), b"must be >= 1"), (dict(T=0), b"must be >= 1"), (dict(D=0), b"must be >= 1"),
             (dict(Hv=0), b"must be >= 1"), (dict(Ho=-2), b"must be >= 1"), (dict(Nv=0), b"must be >= 1"), (dict(No=0), b"must be >= 1"),
             (dict(ldc=7), b"row stride"), (dict(pv=1.0), b"[0, 1)"), (dict(po=-0.1), b"[0, 1)"), (dict(pv=float("nan")), b"[0, 1)"))
    for call, nulls in ((fwd, ("ctx", "offsets", "W1", "b1", "W2", "b2", "pairs", "lv", "of", "z", "ws")),
                        (bwd, ("ctx", "offsets", "W1", "W2", "pairs", "dlv", "dof", "z", "dctx", "dW1", "db1", "dW2", "db2", "ws"))):
        for kw, word in tuple((({n: None}, b"NULL") for n in nulls)) + sizes:
            assert call(**kw) == 1, (call.__name__, kw)
            assert word in lib.semicrf_last_error(), (call.__name__, kw, lib.semicrf_last_error())
    assert fwd(nSym=0) == 1 and b"must be >= 1" in lib.semicrf_last_error()
    assert fwd(ws_bytes=need - 1) == 2 and b"workspace too small" in lib.semicrf_last_error()
    assert bwd(ws_bytes=need_b - 1) == 2 and b"workspace too small" in lib.semicrf_last_error()
    assert bwd(K=65535 * R + 1, ws_bytes=1 << 60) == 1 and b"row chunks" in lib.semicrf_last_error()
    assert fwd(K=0, pairs=None, lv=None, of=None, z=None, sym=None, sc=None, ws=None, ws_bytes=0) == 0     # nothing to do, nothing launched
    assert bwd(K=0, pairs=None, dlv=None, dof=None, z=None, dctx=None, dW1=None, db1=None, dW2=None, db2=None, ws=None, ws_bytes=0) == 0
    assert fwd(K=0, ctx=None) == 1 and bwd(K=0, W2=None) == 1
    for kw, word in ((dict(K=-1), b"interval count"), (dict(Hv=0), b"must be >= 1"), (dict(Ho=0), b"must be >= 1"), (dict(pv=1.5), b"[0, 1)"),
                     (dict(m=None), b"NULL")):
        assert mask(**kw) == 1, kw
        assert word in lib.semicrf_last_error(), (kw, lib.semicrf_last_error())
    assert mask(K=0, m=None) == 0


def test_log_prob_attribute_heads_keyword_is_validated():
    from transkun_amd.transcribe import SegmentTranscriber
    m = SegmentTranscriber(size=8, velocityPredictorHiddenSize=8, refinedOFPredictorHiddenSize=8, targetMIDIPitch=[60])
    with pytest.raises(ValueError, match="attributeHeads must be 'torch' or 'fused'"):
        m.log_prob(torch.zeros(1, 1, 4, 8), [[[]]], [], [], [], attributeHeads="hip")


# ---- 9. through the transcriber (device only) ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_segment_transcriber_log_prob_fused_heads(gpu):
    """SegmentTranscriber.log_prob(attributeHeads="fused") on the attr_loss_small golden, eval mode: the reference's logProb under the
    rule of test_segment_transcriber_log_prob part (2); the gradients against the "torch" heads route -- per tensor at most
    (GATE + 1) x the torch route's error of the heads' contribution against its float64 CPU evaluation, plus 2 eps32 |value| for
    the fp32 addition onto the CRF term's gradient (the CRF term's own gradient is the same bits on both routes: the scorer's
    parameters agree exactly); in training mode a fixed seed reproduces."""
    import numpy as np
    import attr_loss_common
    from test_attr_loss import _crf_logprob_tolerance, _golden_case
    from transkun_amd import attributes, fused
    import importlib
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    g, case = _golden_case(gpu)
    N, P = int(g["meta"][0]), int(g["meta"][1])
    model, ctx0 = attr_loss_common.golden_transcriber(gpu)
    batch, vel, refined, pres = attr_loss_common.golden_targets(g)
    flat = [s for seg in batch for s in seg]
    T = ctx0.shape[2]

    def run(heads, **kw):
        model.zero_grad()
        ctx = ctx0.clone().requires_grad_()
        lp = model.log_prob(ctx, batch, vel, refined, pres, attributeHeads=heads, **kw)
        assert lp.shape == (N, P)
        (-lp.sum(-1).mean()).backward()
        return lp.detach(), ctx.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    lp_f, dctx_f, dpar_f = run("fused")
    lp_t, dctx_t, dpar_t = run("torch")
    # the reference's logProb
    with torch.no_grad():
        pairs, off2 = nsci.pack_intervals(flat, T, N * P, gpu)
        x, _, _ = attributes.attribute_input_packed(ctx0, pairs, off2, pairs._semicrf_K)
        a_t = attributes.attribute_log_prob_torch(model.velocityPredictor(x), model.refinedOFPredictor(x), case[2], case[3], case[4], case[5])
    crf_tol, _ = _crf_logprob_tolerance()
    attr_t = float((a_t.cpu().double() - torch.from_numpy(g["attr"]).double()).abs().max())
    want = g["logProb"].astype(np.float64)
    tol = crf_tol * np.maximum(np.abs(want), 1.0) + 2 * attr_t
    err = np.abs(lp_f.cpu().numpy().astype(np.float64) - want)
    print(f"log_prob fused heads vs reference: {err.max():.3e} (CRF tolerance {crf_tol:g} relative, torch route's attribute part vs golden {attr_t:.3e})")
    assert (err <= tol).all(), (err.max(), tol.min())
    # the CRF term alone, and the heads' contribution in float64 on the CPU
    model.zero_grad()
    ctx = ctx0.clone().requires_grad_()
    p2, o2 = nsci.pack_intervals(flat, T, N * P, gpu)
    (-fused.scorer_crf_logprob(model.scorer, ctx, flat, projection="merged", packed=(p2, o2)).view(N, P).sum(-1).mean()).backward()
    dctx_crf = ctx.grad.clone()
    vp64, op64 = copy.deepcopy(model.velocityPredictor).cpu().double(), copy.deepcopy(model.refinedOFPredictor).cpu().double()
    c64 = ctx0.cpu().double().requires_grad_()
    K = int(case[5][-1])
    a, b, _ = common.gather_ab(c64, pairs.cpu()[:K], case[5].cpu(), K)
    x64 = torch.cat([a, b, a * b], dim=-1)
    rows = attr_loss_common.yardstick_rows(vp64(x64), op64(x64), case[2].cpu(), case[3].cpu(), case[4].cpu())
    (-(rows[0] + rows[1] + rows[2]).sum() / N).backward()
    truth = {"ctx": c64.grad}
    truth.update({"velocityPredictor." + n: p.grad for n, p in vp64.named_parameters()})
    truth.update({"refinedOFPredictor." + n: p.grad for n, p in op64.named_parameters()})
    assert set(truth) - {"ctx"} == {n for n in dpar_t if not n.startswith("scorer.")}
    eps32 = 2.0 ** -23
    bad = []
    for name, t64 in truth.items():
        gf, gt = (dctx_f, dctx_t) if name == "ctx" else (dpar_f[name], dpar_t[name])
        base = dctx_crf.cpu().double() if name == "ctx" else 0.0
        e_t = float(((gt.cpu().double() - base) - t64).abs().max())
        diff = float((gf.double() - gt.double()).abs().max())
        bound = (common.GATE + 1) * e_t + 2 * eps32 * float(gt.abs().max())
        print(f"log_prob gradient {name}: fused vs torch heads {diff:.3e}  torch heads vs float64 {e_t:.3e}  bound {bound:.3e}")
        if not diff <= bound:
            bad.append((name, diff, bound))
    assert not bad, bad
    for n in dpar_t:
        if n.startswith("scorer."):
            assert torch.equal(dpar_f[n], dpar_t[n]), n
    # training mode: a fixed seed reproduces, another seed does not; the modules' own state is what switches dropout on
    model.train()
    try:
        r1, r2, r3 = run("fused", seed=5), run("fused", seed=5), run("fused", seed=6)
    finally:
        model.eval()
    assert torch.equal(r1[0], r2[0]) and torch.equal(r1[1], r2[1]) and all(torch.equal(r1[2][n], r2[2][n]) for n in r1[2])
    assert not torch.equal(r1[0], r3[0]) and not torch.equal(r1[0], lp_f)
    with pytest.raises(ValueError, match="attributeHeads must be 'torch' or 'fused'"):
        model.log_prob(ctx0, batch, vel, refined, pres, attributeHeads="hip")
    from transkun_amd import _lib
    assert _lib.device_status() == 0
