"""The training route of the fused feed-forward ResBlock (feed_forward_residual's train = "fused", ResBlock.feedForwardTrain):
semicrf_ffn_residual_train_fwd, semicrf_ffn_residual_bwd and semicrf_ffn_dropout_mask on the device, their host mirrors on the CPU.
Every device test has a CPU twin that runs anywhere.  Yardstick and gate: tests/ffn_train_common.py."""
import copy
import math

import pytest
import torch

import backbone_common
import ffn_common
import ffn_train_common as common

CPU = torch.device("cpu")


def _bb():
    from transkun_amd import backbone
    return backbone


def _counts():
    bb = _bb()
    return dict(bb.FEED_FORWARD_ROUTES), dict(bb.FEED_FORWARD_TRAIN_ROUTES)


def _delta(before):
    now = _counts()
    return tuple({k: now[i][k] - before[i][k] for k in now[i]} for i in range(2))


# ---- 1. routing ----------------------------------------------------------------------------------------------------------------------------
def _check_routing(dev):
    bb = _bb()
    assert bb.FEED_FORWARD_TRAIN_KINDS == ("torch", "fused") and bb.DEFAULT_FEED_FORWARD_TRAIN == "torch"
    assert set(bb.FEED_FORWARD_TRAIN_ROUTES) == {"fused", "torch", "bwd"}
    assert set(bb.FEED_FORWARD_ROUTES) == {"fused", "torch"} and set(bb.FEED_FORWARD_BF16_ROUTES) == {"fused", "torch"}
    g = torch.Generator().manual_seed(5)
    blk = ffn_common.stock_modules(40, 72, g).to(dev).train()
    blk.module[2].p = 0.1
    blk.dropout.p = 0.1
    x = torch.randn(3, 5, 40, generator=g).to(dev).requires_grad_()
    assert blk.feedForwardTrain == "torch"
    # the knob at its default: the stock expression, no new counter -- with feedForward at "torch" no counter at all
    before = _counts()
    blk(x).sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 0}, {"fused": 0, "torch": 0, "bwd": 0})
    blk.feedForward = "fused"
    before = _counts()
    blk(x).sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 1}, {"fused": 0, "torch": 0, "bwd": 0})
    # "fused": counted fused, in both dicts
    blk.feedForwardTrain = "fused"
    before = _counts()
    out = blk(x)
    assert _delta(before) == ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 0})
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert _delta(before)[1]["bwd"] == 1
    with pytest.raises(RuntimeError):                           # once differentiable
        gx.sum().backward()
    # eval mode, gradient wanted: still the fused training route (p = 0); no gradient wanted: the eval op, not counted as training
    blk.eval()
    before = _counts()
    blk(x).sum().backward()
    assert _delta(before) == ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 1})
    before = _counts()
    with torch.no_grad():
        blk(x)
    assert _delta(before) == ({"fused": 1, "torch": 0}, {"fused": 0, "torch": 0, "bwd": 0})
    blk.train()
    # autocast, bf16, extra arguments, D = 12: the stock expression, counted "torch"
    before = _counts()
    with torch.autocast(dev.type, dtype=torch.bfloat16):
        blk(x).float().sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 1}, {"fused": 0, "torch": 1, "bwd": 0})
    b16 = copy.deepcopy(blk).to(torch.bfloat16)
    before = _counts()
    b16(x.detach().to(torch.bfloat16).requires_grad_()).float().sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 1}, {"fused": 0, "torch": 1, "bwd": 0})

    class TakesExtra(torch.nn.Sequential):
        def forward(self, x, *args):
            return super().forward(x)

    extra = copy.deepcopy(blk)
    extra.module = TakesExtra(*extra.module)
    before = _counts()
    extra(x, 1).sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 1}, {"fused": 0, "torch": 1, "bwd": 0})
    b12 = bb.ResBlock(bb._feed_forward(12, 24, 0.1), size=12).to(dev).train()
    b12.feedForward = "fused"
    b12.feedForwardTrain = "fused"
    before = _counts()
    b12(torch.randn(4, 12, device=dev).requires_grad_()).sum().backward()
    assert _delta(before) == ({"fused": 0, "torch": 1}, {"fused": 0, "torch": 1, "bwd": 0})
    # bad values
    blk.feedForwardTrain = "hip"
    with pytest.raises(ValueError):
        blk(x)
    blk.feedForwardTrain = "fused"
    with pytest.raises(ValueError):
        bb.feed_forward_residual(x, blk.module[0].weight, blk.module[0].bias, blk.module[3].weight, blk.module[3].bias, blk.scale, train="hip")
    m, _ = backbone_common.make_backbone("backbone_small", CPU, "torch")
    assert m.feedForwardTrain == "torch" and m.encoderLayers[0].feedForwardTrain == "torch"
    with pytest.raises(ValueError):
        m.feedForwardTrain = "hip"
    m.encoderLayers[0].feedForwardTrain = "fused"
    assert m.encoderLayers[0].feedForwardTrain == "fused"
    assert m.feedForwardTrain == ("mixed" if len(m.encoderLayers) > 1 else "fused")


def test_routing_cpu():
    _check_routing(CPU)


@pytest.mark.gpu
def test_routing_gpu(gpu):
    _check_routing(gpu)


# ---- 2. the mask -----------------------------------------------------------------------------------------------------------------------------
def _check_mask(dev):
    bb = _bb()
    rows, D, H = 1000, 48, 56                                   # 104 000 draws
    for p in (0.1, 0.5):
        mh, mo = bb.feed_forward_dropout_mask(77, rows, D, H, p, p, dev)
        assert mh.shape == (rows, H) and mo.shape == (rows, D) and mh.dtype == torch.bool
        ch, co = bb.feed_forward_dropout_mask(77, rows, D, H, p, p, "cpu")
        assert torch.equal(mh.cpu(), ch) and torch.equal(mo.cpu(), co)           # device = mirror, bit for bit
        assert not torch.equal(ch[:, :D], co)                                    # the two streams differ
        n = rows * (D + H)
        kept = int(ch.sum()) + int(co.sum())
        assert abs(kept - n * (1 - p)) <= 5 * math.sqrt(n * p * (1 - p)), (p, kept, n)
        sh, so = bb.feed_forward_dropout_mask(77, 37, D, H, p, p, dev)           # a row's mask does not depend on the row count
        assert torch.equal(sh, mh[:37]) and torch.equal(so, mo[:37])
        oh, _ = bb.feed_forward_dropout_mask(78, rows, D, H, p, p, dev)
        assert not torch.equal(oh, mh)
    mh, mo = bb.feed_forward_dropout_mask(77, 9, D, H, 0.0, 0.0, dev)
    assert bool(mh.all()) and bool(mo.all())
    mh, mo = bb.feed_forward_dropout_mask(77, 9, D, H, 0.0, 0.5, dev)
    assert bool(mh.all()) and not bool(mo.all())


def test_mask_cpu():
    _check_mask(CPU)


@pytest.mark.gpu
def test_mask_gpu(gpu):
    _check_mask(gpu)


# ---- 3 + 4. forward and backward against float64 -------------------------------------------------------------------------------------------
def _check_p0_bits(dev):
    bb = _bb()
    for D, hidden in common.SHAPES:
        c = common.case(65, D, hidden, p1=0.0, p2=0.0)
        got = common.run(c, dev)
        with torch.no_grad():
            want = bb.feed_forward_residual(c["x"].to(dev), *(p.to(dev) for p in c["params"]), eps=c["eps"], route="fused")
        assert common.bits_equal(got[0], want.cpu()), (D, hidden)
        ratio, name = common.worst(got, c)
        print(f"p=0 D={D} hidden={hidden}: worst {ratio:.3f} of the gate ({name})")
        assert ratio <= 1.0, (D, hidden, name, ratio)


def test_p0_forward_bits_cpu():
    _check_p0_bits(CPU)


@pytest.mark.gpu
def test_p0_forward_bits_gpu(gpu):
    _check_p0_bits(gpu)


def _check_accuracy(dev, D, hidden):
    for rows in common.ROWS:
        for mult in (1.0, 4.0):
            for kind in ("init", "randn"):
                c = common.case(rows, D, hidden, kind, mult)
                got = common.run(c, dev)
                ratio, name = common.worst(got, c)
                print(f"rows={rows} D={D} hidden={hidden} x{mult} scale={kind}: worst {ratio:.3f} of the gate ({name})")
                assert ratio <= 1.0, (rows, D, hidden, mult, kind, name, ratio)


@pytest.mark.parametrize("D,hidden", common.SHAPES)
def test_accuracy_cpu(D, hidden):
    _check_accuracy(CPU, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("D,hidden", common.SHAPES)
def test_accuracy_gpu(gpu, D, hidden):
    _check_accuracy(gpu, D, hidden)


def _check_three_chunks(dev):
    rows = 2 * _bb().FEED_FORWARD_BWD_ROW_CHUNK + 37            # three planes, a ragged last one
    c = common.case(rows, 8, 8)
    got = common.run(c, dev)
    ratio, name = common.worst(got, c)
    print(f"rows={rows}: worst {ratio:.3f} of the gate ({name})")
    assert ratio <= 1.0, (name, ratio)


def test_three_chunks_cpu():
    _check_three_chunks(CPU)


@pytest.mark.gpu
def test_three_chunks_gpu(gpu):
    _check_three_chunks(gpu)


# ---- 5. exact answers -----------------------------------------------------------------------------------------------------------------------
EXACT = [(5, 8, 8), (70, 64, 72), (130, 256, 136), (2 * 512 + 70, 8, 16)]


def _check_exact(dev):
    used = 0
    for rows, D, hidden in EXACT:
        c = common.exact_case(rows, D, hidden)
        if not c["exact"]:
            continue
        used += 1
        got = common.run(c, dev)
        for a, t, name in zip(got, c["truth"], common.NAMES):
            assert torch.equal(a.double(), t), (rows, D, hidden, name, float((a.double() - t).abs().max()))
    assert used >= 3                                            # a hidden size above 64 and more than one row tile among them
    assert common.exact_case(70, 64, 72)["exact"] and common.exact_case(2 * 512 + 70, 8, 16)["exact"]


def test_exact_cpu():
    _check_exact(CPU)


@pytest.mark.gpu
def test_exact_gpu(gpu):
    _check_exact(gpu)


# ---- 6. determinism and independence --------------------------------------------------------------------------------------------------------
def _check_determinism(dev):
    bb = _bb()
    c = common.case(129, 40, 72)
    a, b = common.run(c, dev), common.run(c, dev)
    assert all(common.bits_equal(u, v) for u, v in zip(a, b))
    # token 2 alone among 3 and among 129: the same index i, the same seed -> the same out and dx bits
    few = common.run(c, dev, x=c["x"][:3], G=c["G"][:3])
    assert common.bits_equal(few[0][2], a[0][2]) and common.bits_equal(few[1][2], a[1][2])
    # [N, T', F', D] and its transpose(-3, -2) view: no copy of x, identical parameter gradients; dout non-contiguous
    g = torch.Generator().manual_seed(31)
    buf = torch.randn(2, 5, 7, 40, generator=g).to(dev)
    G = torch.randn(2, 5, 7, 80, generator=g).to(dev)[..., ::2]             # last stride 2
    Gc = G.contiguous()
    grads = []
    for view, gv in ((buf, Gc), (buf.transpose(-3, -2), G.transpose(-3, -2)), (buf, G)):
        x = view.detach().requires_grad_()
        params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
        out = bb.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", p_hidden=0.1, p_out=0.5, seed=5)
        gs = torch.autograd.grad((out * gv).sum(), [x] + params)
        ptr, shape, strides = bb.FEED_FORWARD_TRAIN_LAST["fwd"]
        assert ptr == buf.data_ptr() and shape == (1, 70, 40) and strides[1:] == (40, 1)     # the buffer itself, tokens by address
        assert bb.FEED_FORWARD_TRAIN_LAST["bwd"][0] == buf.data_ptr()
        assert out.shape == view.shape and gs[0].shape == view.shape
        grads.append([out] + list(gs))
    assert common.bits_equal(grads[0][0], grads[1][0].transpose(-3, -2)) and common.bits_equal(grads[0][1], grads[1][1].transpose(-3, -2))
    for k in range(2, 7):
        assert common.bits_equal(grads[0][k], grads[1][k]) and common.bits_equal(grads[0][k], grads[2][k]), common.NAMES[k]
    # a dout handed over as a view (contiguous last dimension, row stride above D) is read in place
    wide = torch.randn(70, 48, generator=g).to(dev)
    x = buf.view(70, 40).detach().requires_grad_()
    params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
    out = bb.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", p_hidden=0.1, p_out=0.5, seed=5)
    out.backward(wide[:, :40])
    assert bb.FEED_FORWARD_TRAIN_LAST["bwd"][3] == wide.data_ptr() and bb.FEED_FORWARD_TRAIN_LAST["bwd"][4][1] == 48


def test_determinism_cpu():
    _check_determinism(CPU)


@pytest.mark.gpu
def test_determinism_gpu(gpu):
    _check_determinism(gpu)


# ---- 7. the memory contract -----------------------------------------------------------------------------------------------------------------
GUARD = 64
SENT = 12345.5


def _guarded(shape, dev, fill=None, off=0):
    """A contiguous tensor of `shape` inside a buffer with GUARD sentinels on both sides (`off` floats further in): (view, buffer)."""
    n = int(torch.tensor(shape).prod())
    buf = torch.full((n + 2 * GUARD + off,), SENT if fill is None else fill, dtype=torch.float32, device=dev)
    return buf[GUARD + off:GUARD + off + n].view(*shape), buf


def _intact(view, buf, off=0):
    n = view.numel()
    return bool((buf[:GUARD + off] == SENT).all()) and bool((buf[GUARD + off + n:] == SENT).all())


def _check_memory_contract(dev, D, hidden, off):
    from transkun_amd import _lib
    ops = _lib.ops()
    rows = 70
    c = common.case(rows, D, hidden) if (D, hidden) in common.SHAPES else common.case(rows, D, hidden, "randn", 1.0)
    nan = float("nan")
    ins = {}
    for name, t in (("x", c["x"]), ("G", c["G"]), ("W1", c["params"][0]), ("b1", c["params"][1]), ("W2", c["params"][2]),
                    ("b2", c["params"][3]), ("scale", c["params"][4])):
        v, b = _guarded(t.shape, dev, fill=nan, off=off)         # NaN poison around every input
        v.copy_(t)
        ins[name] = v
    x3, g3 = ins["x"].view(1, rows, D), ins["G"].view(1, rows, D)
    outs = {n: _guarded(s, dev, off=off) for n, s in (("out", (1, rows, D)), ("z", (rows, hidden)), ("y", (rows, D)), ("dx", (1, rows, D)),
                                                     ("dW1", (hidden, D)), ("db1", (hidden,)), ("dW2", (D, hidden)), ("db2", (D,)),
                                                     ("dscale", (D,)))}
    ops.ffn_residual_train_fwd(x3, ins["W1"], ins["b1"], ins["W2"], ins["b2"], ins["scale"], c["eps"], 1234, 0.1, 0.5, outs["out"][0],
                               outs["z"][0], outs["y"][0])
    nbytes = int(_lib.load().semicrf_ffn_residual_bwd_workspace_bytes(rows, D, hidden)) if dev.type != "cpu" else 0
    wsbuf = torch.full((nbytes + 256 + 4 * off,), 0x5A, dtype=torch.uint8, device=dev)
    ws = wsbuf[4 * off:4 * off + nbytes]
    ops.ffn_residual_bwd(g3, x3, outs["z"][0], outs["y"][0], ins["W1"], ins["W2"], ins["scale"], c["eps"], 1234, 0.1, 0.5, outs["dx"][0],
                         outs["dW1"][0], outs["db1"][0], outs["dW2"][0], outs["db2"][0], outs["dscale"][0], ws)
    assert bool((wsbuf[4 * off + nbytes:] == 0x5A).all()) and bool((wsbuf[:4 * off] == 0x5A).all())     # nothing past the declared workspace
    for name, (v, b) in outs.items():
        assert _intact(v, b, off), name
        assert bool(torch.isfinite(v).all()), name               # no poison was read, every element was written
    got = [outs[n][0].reshape(t.shape).cpu() for n, t in zip(("out", "dx", "dW1", "db1", "dW2", "db2", "dscale"), c["truth"])]
    ratio, name = common.worst(got, c)
    assert ratio <= 1.0, (name, ratio)
    want = common.run(c, dev)                                    # the aligned and the misaligned instantiation: the same bits
    assert all(common.bits_equal(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D,hidden", [(8, 8), (40, 72), (160, 640), (256, 1032)])
def test_memory_contract_cpu(D, hidden, off):
    _check_memory_contract(CPU, D, hidden, off)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D,hidden", [(8, 8), (40, 72), (96, 200), (160, 640), (256, 1032)])
def test_memory_contract_gpu(gpu, D, hidden, off):
    _check_memory_contract(gpu, D, hidden, off)


def _check_bad_calls(dev):
    from transkun_amd import _lib
    ops = _lib.ops()
    rows, D, H = 6, 8, 16
    c = common.case(rows, D, H)
    w1, b1, w2, b2, scale = (p.to(dev) for p in c["params"])
    x3 = c["x"].to(dev).view(1, rows, D)
    mk = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=dev)
    out, z, y, dx = mk(1, rows, D), mk(rows, H), mk(rows, D), mk(1, rows, D)
    grads = [mk(H, D), mk(H), mk(D, H), mk(D), mk(D)]
    nbytes = int(_lib.load().semicrf_ffn_residual_bwd_workspace_bytes(rows, D, H))
    assert nbytes > 0 and _lib.load().semicrf_workspace_bytes(_lib.OP_FFN_RESIDUAL_BWD, rows, H) >= nbytes
    assert _lib.load().semicrf_ffn_residual_bwd_workspace_bytes(rows, 12, H) == 0
    assert _lib.load().semicrf_ffn_residual_bwd_supported(D, H) == 1 and _lib.load().semicrf_ffn_residual_bwd_supported(12, H) == 0
    ws = torch.zeros(nbytes if dev.type != "cpu" else 0, dtype=torch.uint8, device=dev)
    untouched = lambda: all(bool((t == SENT).all()) for t in [out, z, y, dx] + grads)
    with pytest.raises(RuntimeError):                           # p out of range
        ops.ffn_residual_train_fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 1.0, 0.0, out, z, y)
    with pytest.raises(RuntimeError):                           # z too small
        ops.ffn_residual_train_fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 0.1, 0.0, out, z[:-1], y)
    with pytest.raises(RuntimeError):                           # out overlaps x
        ops.ffn_residual_train_fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 0.1, 0.0, x3, z, y)
    with pytest.raises(RuntimeError):                           # unsupported shape
        ops.ffn_residual_train_fwd(mk(1, rows, 12), mk(H, 12), b1, mk(12, H), mk(12), mk(12), 1e-6, 1, 0.1, 0.0, mk(1, rows, 12), z, mk(rows, 12))
    assert untouched()
    zz, yy = torch.zeros(rows, H, device=dev), torch.zeros(rows, D, device=dev)
    G = c["G"].to(dev).view(1, rows, D)
    with pytest.raises(RuntimeError):                           # dx overlaps x
        ops.ffn_residual_bwd(G, x3, zz, yy, w1, w2, scale, 1e-6, 1, 0.1, 0.1, x3, *grads, ws)
    with pytest.raises(RuntimeError):                           # dx overlaps dout
        ops.ffn_residual_bwd(G, x3, zz, yy, w1, w2, scale, 1e-6, 1, 0.1, 0.1, G, *grads, ws)
    with pytest.raises(RuntimeError):                           # a short gradient
        ops.ffn_residual_bwd(G, x3, zz, yy, w1, w2, scale, 1e-6, 1, 0.1, 0.1, dx, grads[0][:-1], *grads[1:], ws)
    with pytest.raises(RuntimeError):                           # p out of range
        ops.ffn_residual_bwd(G, x3, zz, yy, w1, w2, scale, 1e-6, 1, -0.1, 0.1, dx, *grads, ws)
    if dev.type != "cpu":
        with pytest.raises(RuntimeError, match="workspace too small"):
            ops.ffn_residual_bwd(G, x3, zz, yy, w1, w2, scale, 1e-6, 1, 0.1, 0.1, dx, *grads, ws[:-256])
    assert untouched()


def test_bad_calls_cpu():
    _check_bad_calls(CPU)


@pytest.mark.gpu
def test_bad_calls_gpu(gpu):
    _check_bad_calls(gpu)


# ---- 8. the modules --------------------------------------------------------------------------------------------------------------------------
P_DROP = 0.1


def _model(dev, attention, dtype=torch.float32, fused=True):
    """backbone_small in training mode: the feed-forward dropouts at P_DROP, every other dropout off (their masks are torch's own)."""
    bb = _bb()
    fx = backbone_common.fixture("backbone_small")
    m = bb.Backbone(**dict(fx["cfg"], dropoutProb=0.0, useGradientCheckpoint=False))
    m.load_state_dict(fx["sd"], strict=True)
    m.attention = attention
    m = m.to(dtype).to(dev).train()
    common.set_ffn_dropout(m, P_DROP)
    if fused:
        m.feedForward = "fused"
        m.feedForwardTrain = "fused"
    else:
        common.patch_reference_blocks(m, P_DROP)
    return m, fx


def _within_gate(got, run, seed):
    """Every tensor of `got` against the float64 model with the same masks, gated by the fp32 stock model with the same masks."""
    both = []
    for dtype in (torch.float64, torch.float32):
        ref, _ = _model(CPU, "torch", dtype, fused=False)
        torch.manual_seed(seed)
        both.append(run(ref, dtype, CPU))
    for a, t, s in zip(got, *both):
        gate = common.GATE * max(float((s.double() - t.double()).abs().max()), common.U * float(t.abs().max()))
        assert float((a.double() - t.double()).abs().max()) <= gate


def _check_block(dev, attention):
    m, fx = _model(dev, attention)

    def run(model, dtype, device, checkpoint=False):
        blk = model.encoderLayers[0]
        lin = fx["layer_in"].to(device).to(dtype).clone().requires_grad_()
        if checkpoint:
            from torch.utils.checkpoint import checkpoint as ckpt
            out = ckpt(blk, lin, use_reentrant=False)
        else:
            out = blk(lin)
        out.square().sum().backward()
        return [lin.grad.detach().cpu()] + [p.grad.detach().cpu() for p in blk.parameters()]

    n_ff = len(m.encoderLayers[0].feed_forward_blocks())
    torch.manual_seed(11)
    before = _counts()
    got = run(m, torch.float32, dev)
    d = _delta(before)
    assert d[1] == {"fused": n_ff, "torch": 0, "bwd": n_ff} and d[0] == {"fused": n_ff, "torch": 0}, d
    _within_gate(got, run, 11)
    # recomputation under torch.utils.checkpoint: the preserved RNG state reproduces the seeds, so the same gradient bits
    m.zero_grad()
    torch.manual_seed(11)
    before = _counts()
    again = run(m, torch.float32, dev, checkpoint=True)
    assert _delta(before)[1] == {"fused": 2 * n_ff, "torch": 0, "bwd": n_ff}          # the recomputed forward is fused too
    assert all(common.bits_equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("attention", ["torch", "fused-train"])
def test_basic_block_cpu(attention):
    _check_block(CPU, attention)


@pytest.mark.gpu
@pytest.mark.parametrize("attention", ["torch", "fused-train"])
def test_basic_block_gpu(gpu, attention):
    _check_block(gpu, attention)


def _check_backbone(dev, attention):
    from transkun_amd import optim
    m, fx = _model(dev, attention)
    m.load_state_dict({k: v.to(dev) for k, v in fx["sd"].items()}, strict=True)      # the knob adds no state
    assert set(m.state_dict()) == set(fx["sd"])

    def run(model, dtype, device):
        x = fx["x"].to(device)
        x = x.to(dtype) if x.is_floating_point() else x
        model(x, fx["outputIndices"].to(device)).square().sum().backward()
        return [p.grad.detach().cpu() for p in model.parameters()]

    n_ff = len(m.feed_forward_blocks())
    torch.manual_seed(13)
    before = _counts()
    got = run(m, torch.float32, dev)
    d = _delta(before)
    n_fwd = d[1]["fused"]                                       # a Backbone in training mode may recompute its layers: forward twice
    assert n_fwd in (n_ff, 2 * n_ff) and d[1] == {"fused": n_fwd, "torch": 0, "bwd": n_ff} and d[0] == {"fused": n_fwd, "torch": 0}, d
    _within_gate(got, run, 13)
    opt = optim.FusedAdaBelief(m.parameters(), lr=1e-3)
    opt.step()                                                  # one optimizer step over these gradients runs
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


@pytest.mark.parametrize("attention", ["torch", "fused-train"])
def test_backbone_cpu(attention):
    _check_backbone(CPU, attention)


@pytest.mark.gpu
@pytest.mark.parametrize("attention", ["torch", "fused-train"])
def test_backbone_gpu(gpu, attention):
    _check_backbone(gpu, attention)


# ---- 9. graph capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    """One captured forward + backward replays to the bits of the eager call with the same fixed seed (the seed is a host value:
    a replay repeats one and the same mask)."""
    bb = _bb()
    c = common.case(129, 40, 72)
    want = common.run(c, gpu)
    x = c["x"].to(gpu).requires_grad_()
    G = c["G"].to(gpu)
    params = [p.to(gpu).clone().requires_grad_() for p in c["params"]]

    def step():
        out = bb.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", p_hidden=c["p1"], p_out=c["p2"], seed=c["seed"])
        return [out] + list(torch.autograd.grad((out * G).sum(), [x] + params))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = step()
    for _ in range(2):
        for t in res:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(common.bits_equal(a.cpu(), b) for a, b in zip(res, want))
