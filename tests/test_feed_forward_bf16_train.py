"""The training route of the bf16 feed-forward ResBlock (feed_forward_residual's bf16_train = "fused", ResBlock.feedForwardBf16Train):
semicrf_ffn_residual_bf16_train_fwd / _bwd and their _mixed forms on the device, their host mirrors on the CPU.  Form A: every tensor
bfloat16; form B: every tensor float32 under bfloat16 autocast.  Every device test has a CPU twin that runs anywhere.  Yardstick, gate
and the chain in float64: tests/ffn_bf16_train_common.py."""
import copy

import pytest
import torch

import backbone_common
import ffn_common
import ffn_train_common as tc
import ffn_bf16_train_common as common

CPU = torch.device("cpu")
BF16 = torch.bfloat16
FORMS = common.FORMS


def _bb():
    from transkun_amd import backbone
    return backbone


def _knobs(m, bf16_train="fused"):
    m.feedForward = "fused"
    m.feedForwardTrain = "fused"
    m.feedForwardBf16 = "fused"
    m.feedForwardBf16Train = bf16_train
    return m


Z2, Z3 = {"fused": 0, "torch": 0}, {"fused": 0, "torch": 0, "bwd": 0}
T2, T3 = {"fused": 0, "torch": 1}, {"fused": 0, "torch": 1, "bwd": 0}


# ---- 1. routing ----------------------------------------------------------------------------------------------------------------------------
def _check_routing(dev):
    bb = _bb()
    assert bb.FEED_FORWARD_BF16_TRAIN_KINDS == ("torch", "fused") and bb.DEFAULT_FEED_FORWARD_BF16_TRAIN == "torch"
    assert set(bb.FEED_FORWARD_BF16_TRAIN_ROUTES) == {"fused", "torch", "bwd"}
    assert set(bb.FEED_FORWARD_TRAIN_ROUTES) == {"fused", "torch", "bwd"}
    assert set(bb.FEED_FORWARD_ROUTES) == {"fused", "torch"} and set(bb.FEED_FORWARD_BF16_ROUTES) == {"fused", "torch"}
    g = torch.Generator().manual_seed(5)
    blk = ffn_common.stock_modules(40, 72, g).to(dev).train()
    blk.module[2].p = 0.1
    blk.dropout.p = 0.1
    x = torch.randn(3, 5, 40, generator=g).to(dev).requires_grad_()
    x16 = x.detach().to(BF16).requires_grad_()
    assert blk.feedForwardBf16Train == "torch"
    ac = lambda dt=BF16: torch.autocast(dev.type, dtype=dt)
    # the new knob at its default: what the fp32 route's tests pin, bf16 and autocast calls counted "torch"
    _knobs(blk, "torch")
    b16 = copy.deepcopy(blk).to(BF16)
    before = common.counts()
    with ac():
        blk(x).float().sum().backward()
    assert common.delta(before) == (T2, T3, T2, Z3)
    before = common.counts()
    b16(x16).float().sum().backward()
    assert common.delta(before) == (T2, T3, T2, Z3)
    before = common.counts()
    blk(x).sum().backward()                                    # fp32 outside autocast: the fp32 training route, as before
    assert common.delta(before) == ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 1}, Z2, Z3)
    # "fused": form B (fp32 under bf16 autocast) and form A (bf16, outside autocast and under bf16 autocast) go fused, in all four dicts
    _knobs(blk)
    _knobs(b16)
    before = common.counts()
    with ac():
        out = blk(x)
    assert out.dtype == torch.float32
    assert common.delta(before) == ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 0}, {"fused": 1, "torch": 0},
                                    {"fused": 1, "torch": 0, "bwd": 0})
    (gx,) = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert common.delta(before)[1]["bwd"] == 1 and common.delta(before)[3]["bwd"] == 1
    with pytest.raises(RuntimeError):                           # once differentiable
        gx.sum().backward()
    for ctx in (None, ac()):
        before = common.counts()
        if ctx is None:
            out = b16(x16)
        else:
            with ctx:
                out = b16(x16)
        assert out.dtype == BF16
        out.float().sum().backward()
        assert common.delta(before) == common.FUSED_ONCE
    assert all(p.grad is not None and p.grad.dtype == BF16 for p in b16.parameters())
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in blk.parameters())
    before = common.counts()
    blk(x).sum().backward()                                    # fp32 outside autocast: still the fp32 training route
    assert common.delta(before) == ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 1}, Z2, Z3)
    # eval mode with a gradient wanted: the fused bf16 training route with p = 0; no gradient wanted: the bf16 eval op
    b16.eval()
    before = common.counts()
    b16(x16).float().sum().backward()
    assert common.delta(before) == common.FUSED_ONCE
    before = common.counts()
    with torch.no_grad():
        b16(x16)
    assert common.delta(before) == ({"fused": 1, "torch": 0}, Z3, {"fused": 1, "torch": 0}, Z3)
    b16.train()
    # the stock route: one of the three other knobs missing
    for knob in ("feedForwardTrain", "feedForwardBf16"):
        setattr(b16, knob, "torch")
        before = common.counts()
        b16(x16).float().sum().backward()
        d = common.delta(before)
        assert d[0] == T2 and d[3] == Z3 and d[1]["fused"] == 0 and d[1]["bwd"] == 0, (knob, d)
        setattr(b16, knob, "fused")
    b16.feedForward = "torch"
    before = common.counts()
    b16(x16).float().sum().backward()
    assert common.delta(before) == (Z2, Z3, Z2, Z3)
    b16.feedForward = "fused"
    # D = 12, an extra argument, fp16, autocast to fp16, mixed dtypes
    b12 = _knobs(bb.ResBlock(bb._feed_forward(12, 24, 0.1), size=12).to(dev).to(BF16).train())
    before = common.counts()
    b12(torch.randn(4, 12, device=dev).to(BF16).requires_grad_()).float().sum().backward()
    assert common.delta(before) == (T2, T3, T2, T3)

    class TakesExtra(torch.nn.Sequential):
        def forward(self, x, *args):
            return super().forward(x)

    extra = copy.deepcopy(b16)
    extra.module = TakesExtra(*extra.module)
    before = common.counts()
    extra(x16, 1).float().sum().backward()
    assert common.delta(before) == (T2, T3, T2, T3)
    b_h = copy.deepcopy(blk).to(torch.float16)
    before = common.counts()
    b_h(x.detach().to(torch.float16).requires_grad_()).float().sum().backward()
    assert common.delta(before) == (T2, T3, Z2, Z3)
    before = common.counts()
    with ac(torch.float16):
        blk(x).float().sum().backward()
    assert common.delta(before) == (T2, T3, Z2, Z3)
    before = common.counts()
    with ac():
        blk(x16).float().sum().backward()                      # bf16 x, fp32 parameters (stock torch needs autocast for the mix)
    assert common.delta(before) == (T2, T3, T2, T3)
    # bad values
    blk.feedForwardBf16Train = "hip"
    with pytest.raises(ValueError):
        blk(x)
    blk.feedForwardBf16Train = "fused"
    with pytest.raises(ValueError):
        bb.feed_forward_residual(x, blk.module[0].weight, blk.module[0].bias, blk.module[3].weight, blk.module[3].bias, blk.scale, bf16_train="hip")
    m, _ = backbone_common.make_backbone("backbone_small", CPU, "torch")
    assert m.feedForwardBf16Train == "torch" and m.encoderLayers[0].feedForwardBf16Train == "torch"
    with pytest.raises(ValueError):
        m.feedForwardBf16Train = "hip"
    with pytest.raises(ValueError):
        m.encoderLayers[0].feedForwardBf16Train = "hip"
    m.encoderLayers[0].feedForwardBf16Train = "fused"
    assert m.encoderLayers[0].feedForwardBf16Train == "fused"
    assert m.feedForwardBf16Train == ("mixed" if len(m.encoderLayers) > 1 else "fused")


def test_routing_cpu():
    _check_routing(CPU)


@pytest.mark.gpu
def test_routing_gpu(gpu):
    _check_routing(gpu)


# ---- 2. p = 0: the bits of the eval op ---------------------------------------------------------------------------------------------------
def _check_p0_bits(dev, form):
    bb = _bb()
    for D, hidden in common.SHAPES:
        c = common.case(form, 65, D, hidden, p1=0.0, p2=0.0)
        got = common.run(c, dev)
        with torch.no_grad(), common.autocast(form, dev):
            want = bb.feed_forward_residual(c["x"].to(dev), *(p.to(dev) for p in c["params"]), eps=c["eps"], route="fused", bf16="fused")
        assert common.bits_equal(got[0], want.cpu()), (form, D, hidden)


@pytest.mark.parametrize("form", FORMS)
def test_p0_forward_bits_cpu(form):
    _check_p0_bits(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_p0_forward_bits_gpu(gpu, form):
    _check_p0_bits(gpu, form)


# ---- 3. accuracy of out and all six gradients against float64 -----------------------------------------------------------------------------
def _check_accuracy(dev, form, D, hidden):
    top = (0.0, "")
    for rows in common.ROWS:
        for mult in (1.0, 4.0):
            for kind in ("init", "randn"):
                c = common.case(form, rows, D, hidden, kind, mult)
                got = common.run(c, dev)
                ratio, name = common.worst(got, c)
                print(f"form {form} [{dev.type}] rows={rows} D={D} hidden={hidden} x{mult} scale={kind}: worst {ratio:.3f} of the gate ({name})")
                top = max(top, (ratio, name))
                assert ratio <= 1.0, (form, rows, D, hidden, mult, kind, name, ratio)
    print(f"form {form} [{dev.type}] D={D} hidden={hidden}: worst share of the gate {top[0]:.3f} ({top[1]})")


@pytest.mark.parametrize("D,hidden", common.SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_accuracy_cpu(form, D, hidden):
    _check_accuracy(CPU, form, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("D,hidden", common.SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_accuracy_gpu(gpu, form, D, hidden):
    _check_accuracy(gpu, form, D, hidden)


def _check_three_planes(dev, form):
    rows = 2 * _bb().FEED_FORWARD_BWD_ROW_CHUNK + 37            # three planes, a ragged last one
    c = common.case(form, rows, 8, 8)
    got = common.run(c, dev)
    ratio, name = common.worst(got, c)
    print(f"form {form} [{dev.type}] rows={rows}: worst {ratio:.3f} of the gate ({name})")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("form", FORMS)
def test_three_planes_cpu(form):
    _check_three_planes(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_three_planes_gpu(gpu, form):
    _check_three_planes(gpu, form)


@pytest.mark.parametrize("form", FORMS)
def test_yardstick_rejects_mutants_cpu(form):
    """The gate is not vacuous: it passes the analytic float64 gradient, rejects the one with M1 left out of dz, and rejects
    dW1 * (1 + 2^-4)."""
    c = common.case(form, 65, 40, 72)
    args = (form, c["x"], c["params"], c["eps"], c["f1"], c["f2"], c["G"])
    good, _ = common.chain64(*args, rounded=False, relu=False)
    assert common.worst(good, c)[0] < 1e-3                      # the chain without roundings IS the truth
    bad, _ = common.chain64(*args, rounded=False, relu=False, drop_m1_in_dz=True)
    r = dict((n, v) for v, n in common.ratios(bad, c))
    assert r["dx"] > 1.0 and r["dW1"] > 1.0 and r["db1"] > 1.0, r
    scaled = list(c["truth"])
    scaled[2] = scaled[2] * (1.0 + 2.0 ** -4)
    r = dict((n, v) for v, n in common.ratios(scaled, c))
    assert r["dW1"] > 1.0 and max(v for n, v in r.items() if n != "dW1") == 0.0, r


# ---- 4. exact answers ------------------------------------------------------------------------------------------------------------------------
def _check_exact(dev, form, rows, D, hidden):
    c = common.exact_case(form, rows, D, hidden)
    assert c["exact"], (form, rows, D, hidden)
    got = common.run(c, dev)
    for a, t, name in zip(got, c["truth"], common.NAMES):
        assert torch.equal(a.double(), t), (form, rows, D, hidden, name, float((a.double() - t).abs().max()))


@pytest.mark.parametrize("rows,D,hidden", common.EXACT)
@pytest.mark.parametrize("form", FORMS)
def test_exact_cpu(form, rows, D, hidden):
    _check_exact(CPU, form, rows, D, hidden)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,D,hidden", common.EXACT)
@pytest.mark.parametrize("form", FORMS)
def test_exact_gpu(gpu, form, rows, D, hidden):
    _check_exact(gpu, form, rows, D, hidden)


# ---- 5. determinism and independence --------------------------------------------------------------------------------------------------------
def _call(c, dev, x, params, seed=5):
    with common.autocast(c["form"], dev):
        return _bb().feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", bf16="fused", bf16_train="fused",
                                           p_hidden=0.1, p_out=0.5, seed=seed)


def _check_determinism(dev, form):
    bb = _bb()
    dt = common.dtype_of(form)
    c = common.case(form, 129, 40, 72)
    a, b = common.run(c, dev), common.run(c, dev)
    assert all(common.bits_equal(u, v) for u, v in zip(a, b))
    # token 2 among 3 and among 129: the same index i, the same seed -> the same out and dx bits
    few = common.run(c, dev, x=c["x"][:3], G=c["G"][:3])
    assert common.bits_equal(few[0][2], a[0][2]) and common.bits_equal(few[1][2], a[1][2])
    # 16-byte and element loads (the buffer shifted by one element): the same bits
    off = common.run(c, dev, x=common.one_off(c["x"].to(dev)), G=common.one_off(c["G"].to(dev)))
    assert all(common.bits_equal(u, v) for u, v in zip(a, off))
    # [N, T', F', D] and its transpose(-3, -2) view: no copy of x, identical parameter gradients; dout non-contiguous
    g = torch.Generator().manual_seed(31)
    buf = torch.randn(2, 5, 7, 40, generator=g).to(dt).to(dev)
    G = torch.randn(2, 5, 7, 80, generator=g).to(dt).to(dev)[..., ::2]      # last stride 2
    Gc = G.contiguous()
    grads = []
    for view, gv in ((buf, Gc), (buf.transpose(-3, -2), G.transpose(-3, -2)), (buf, G)):
        x = view.detach().requires_grad_()
        params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
        out = _call(c, dev, x, params)
        gs = torch.autograd.grad((out * gv).sum(), [x] + params)
        ptr, shape, strides = bb.FEED_FORWARD_BF16_TRAIN_LAST["fwd"]
        assert ptr == buf.data_ptr() and shape == (1, 70, 40) and strides[1:] == (40, 1)     # the buffer itself, tokens by address
        assert bb.FEED_FORWARD_BF16_TRAIN_LAST["bwd"][0] == buf.data_ptr()
        assert out.shape == view.shape and gs[0].shape == view.shape
        grads.append([out] + list(gs))
    assert common.bits_equal(grads[0][0], grads[1][0].transpose(-3, -2)) and common.bits_equal(grads[0][1], grads[1][1].transpose(-3, -2))
    for k in range(2, 7):
        assert common.bits_equal(grads[0][k], grads[1][k]) and common.bits_equal(grads[0][k], grads[2][k]), common.NAMES[k]
    # a dout handed over as a view (contiguous last dimension, row stride above D) is read in place
    wide = torch.randn(70, 48, generator=g).to(dt).to(dev)
    x = buf.view(70, 40).detach().requires_grad_()
    params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
    out = _call(c, dev, x, params)
    out.backward(wide[:, :40])
    assert bb.FEED_FORWARD_BF16_TRAIN_LAST["bwd"][3] == wide.data_ptr() and bb.FEED_FORWARD_BF16_TRAIN_LAST["bwd"][4][1] == 48
    # form A: a dout of another dtype is taken over (copied into x's dtype and layout)
    if form == "A":
        x = buf.view(70, 40).detach().requires_grad_()
        out = _call(c, dev, x, params)
        torch.autograd.backward(out, wide[:, :40].float().to(dt))
        assert x.grad.dtype == dt


@pytest.mark.parametrize("form", FORMS)
def test_determinism_cpu(form):
    _check_determinism(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_determinism_gpu(gpu, form):
    _check_determinism(gpu, form)


# ---- 6. the memory contract -----------------------------------------------------------------------------------------------------------------
GUARD = 64
SENT = 12288.0               # exact in bf16
BAND = 256                   # bytes around the saved buffer and the workspace (both need 16-byte alignment)


def _guarded(shape, dev, dt, fill=None, off=0):
    """A contiguous tensor of `shape` inside a buffer with GUARD sentinels on both sides (`off` elements further in): (view, buffer)."""
    n = int(torch.tensor(shape).prod())
    buf = torch.full((n + 2 * GUARD + off,), SENT if fill is None else fill, dtype=dt, device=dev)
    return buf[GUARD + off:GUARD + off + n].view(*shape), buf


def _intact(view, buf, off=0):
    n = view.numel()
    return bool((buf[:GUARD + off] == SENT).all()) and bool((buf[GUARD + off + n:] == SENT).all())


def _banded_bytes(nbytes, dev):
    buf = torch.full((nbytes + 2 * BAND,), 0x5A, dtype=torch.uint8, device=dev)
    view = buf[BAND:BAND + nbytes]
    assert view.data_ptr() % 16 == 0
    return view, buf


def _bands_ok(buf, nbytes):
    return bool((buf[:BAND] == 0x5A).all()) and bool((buf[BAND + nbytes:] == 0x5A).all())


def _ops(form):
    from transkun_amd import _lib
    ops = _lib.ops()
    return (ops.ffn_residual_bf16_train_fwd, ops.ffn_residual_bf16_bwd) if form == "A" else (ops.ffn_residual_bf16_mixed_train_fwd,
                                                                                             ops.ffn_residual_bf16_mixed_bwd)


def _check_memory_contract(dev, form, D, hidden, off):
    from transkun_amd import _lib
    fwd, bwd = _ops(form)
    dt = common.dtype_of(form)
    rows = 70
    c = common.case(form, rows, D, hidden)
    nan = float("nan")
    ins = {}
    for name, t in (("x", c["x"]), ("G", c["G"]), ("W1", c["params"][0]), ("b1", c["params"][1]), ("W2", c["params"][2]),
                    ("b2", c["params"][3]), ("scale", c["params"][4])):
        v, b = _guarded(t.shape, dev, dt, fill=nan, off=off)    # NaN poison around every input
        v.copy_(t)
        ins[name] = v
    x3, g3 = ins["x"].view(1, rows, D), ins["G"].view(1, rows, D)
    outs = {n: _guarded(s, dev, dt, off=off) for n, s in (("out", (1, rows, D)), ("dx", (1, rows, D)), ("dW1", (hidden, D)), ("db1", (hidden,)),
                                                          ("dW2", (D, hidden)), ("db2", (D,)), ("dscale", (D,)))}
    nsaved = int(_lib.load().semicrf_ffn_residual_bf16_train_saved_bytes(rows, D, hidden))
    saved, savedbuf = _banded_bytes(nsaved, dev)
    fwd(x3, ins["W1"], ins["b1"], ins["W2"], ins["b2"], ins["scale"], c["eps"], c["seed"], c["p1"], c["p2"], outs["out"][0], saved)
    assert _bands_ok(savedbuf, nsaved)
    nws = int(_lib.load().semicrf_ffn_residual_bf16_bwd_workspace_bytes(rows, D, hidden)) if dev.type != "cpu" else 0
    ws, wsbuf = _banded_bytes(nws, dev)
    bwd(g3, x3, saved, ins["W1"], ins["W2"], ins["scale"], c["eps"], c["seed"], c["p1"], c["p2"], outs["dx"][0], outs["dW1"][0], outs["db1"][0],
        outs["dW2"][0], outs["db2"][0], outs["dscale"][0], ws)
    assert _bands_ok(wsbuf, nws) and _bands_ok(savedbuf, nsaved)                     # nothing past the declared workspace and saved buffer
    for name, (v, b) in outs.items():
        assert _intact(v, b, off), name
        assert bool(torch.isfinite(v.float()).all()), name       # no poison was read
    got = [outs[n][0].reshape(t.shape).cpu() for n, t in zip(("out", "dx", "dW1", "db1", "dW2", "db2", "dscale"), c["truth"])]
    ratio, name = common.worst(got, c)
    assert ratio <= 1.0, (name, ratio)
    want = common.run(c, dev)                                    # the aligned and the misaligned instantiation: the same bits
    assert all(common.bits_equal(a, b) for a, b in zip(got, want))


MEM_SHAPES = [(8, 8), (40, 72), (96, 200), (160, 640), (256, 1032)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D,hidden", MEM_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_memory_contract_cpu(form, D, hidden, off):
    _check_memory_contract(CPU, form, D, hidden, off)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("D,hidden", MEM_SHAPES)
@pytest.mark.parametrize("form", FORMS)
def test_memory_contract_gpu(gpu, form, D, hidden, off):
    _check_memory_contract(gpu, form, D, hidden, off)


def _check_bad_calls(dev, form):
    from transkun_amd import _lib
    lib = _lib.load()
    fwd, bwd = _ops(form)
    dt = common.dtype_of(form)
    rows, D, H = 6, 8, 16
    c = common.case(form, rows, D, H)
    w1, b1, w2, b2, scale = (p.to(dev) for p in c["params"])
    x3 = c["x"].to(dev).view(1, rows, D)
    mk = lambda *s: torch.full(s, SENT, dtype=dt, device=dev)
    out, dx = mk(1, rows, D), mk(1, rows, D)
    grads = [mk(H, D), mk(H), mk(D, H), mk(D), mk(D)]
    nsaved = int(lib.semicrf_ffn_residual_bf16_train_saved_bytes(rows, D, H))
    nws = int(lib.semicrf_ffn_residual_bf16_bwd_workspace_bytes(rows, D, H))
    assert nsaved >= rows * H * 2 + rows * D * x3.element_size() and nws > 0
    assert lib.semicrf_ffn_residual_bf16_train_saved_bytes(rows, 12, H) == 0 and lib.semicrf_ffn_residual_bf16_bwd_workspace_bytes(rows, 12, H) == 0
    assert lib.semicrf_ffn_residual_bf16_bwd_supported(D, H) == 1 and lib.semicrf_ffn_residual_bf16_bwd_supported(12, H) == 0
    saved = torch.full((nsaved,), 0x5A, dtype=torch.uint8, device=dev)
    ws = torch.full((nws if dev.type != "cpu" else 0,), 0x5A, dtype=torch.uint8, device=dev)
    untouched = lambda: all(bool((t == SENT).all()) for t in [out, dx] + grads) and bool((saved == 0x5A).all()) and bool((ws == 0x5A).all())
    with pytest.raises(RuntimeError):                           # p out of range
        fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 1.0, 0.0, out, saved)
    with pytest.raises(RuntimeError):                           # saved too small
        fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 0.1, 0.0, out, saved[:-16])
    with pytest.raises(RuntimeError):                           # out overlaps x
        fwd(x3, w1, b1, w2, b2, scale, 1e-6, 1, 0.1, 0.0, x3, saved)
    with pytest.raises(RuntimeError):                           # unsupported shape
        fwd(mk(1, rows, 12), mk(H, 12), b1, mk(12, H), mk(12), mk(12), 1e-6, 1, 0.1, 0.0, mk(1, rows, 12), saved)
    with pytest.raises(RuntimeError):                           # another dtype
        fwd(x3.double(), w1, b1, w2, b2, scale, 1e-6, 1, 0.1, 0.0, out, saved)
    assert untouched()
    G = c["G"].to(dev).view(1, rows, D)
    with pytest.raises(RuntimeError):                           # dx overlaps x
        bwd(G, x3, saved, w1, w2, scale, 1e-6, 1, 0.1, 0.1, x3, *grads, ws)
    with pytest.raises(RuntimeError):                           # dx overlaps dout
        bwd(G, x3, saved, w1, w2, scale, 1e-6, 1, 0.1, 0.1, G, *grads, ws)
    with pytest.raises(RuntimeError):                           # a short gradient
        bwd(G, x3, saved, w1, w2, scale, 1e-6, 1, 0.1, 0.1, dx, grads[0][:-1], *grads[1:], ws)
    with pytest.raises(RuntimeError):                           # p out of range
        bwd(G, x3, saved, w1, w2, scale, 1e-6, 1, -0.1, 0.1, dx, *grads, ws)
    with pytest.raises(RuntimeError):                           # saved too small
        bwd(G, x3, saved[:-16], w1, w2, scale, 1e-6, 1, 0.1, 0.1, dx, *grads, ws)
    if dev.type != "cpu":
        with pytest.raises(RuntimeError, match="workspace too small"):
            bwd(G, x3, saved, w1, w2, scale, 1e-6, 1, 0.1, 0.1, dx, *grads, ws[:-256])
    assert untouched()


@pytest.mark.parametrize("form", FORMS)
def test_bad_calls_cpu(form):
    _check_bad_calls(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_bad_calls_gpu(gpu, form):
    _check_bad_calls(gpu, form)


# ---- 7. the modules --------------------------------------------------------------------------------------------------------------------------
P_DROP = 0.1


def _model(dev, form, kind, checkpoint=False):
    """backbone_small in training mode, the feed-forward dropouts at P_DROP and every other dropout off.  kind = "fused": the model under
    test (form A: cast to bf16; form B: fp32, run under autocast) with every fused knob on; "truth": float64 on the CPU from the same
    (in form A: bf16-rounded) weights, its feed-forward blocks the expression with the op's own masks; "stock": the form's stock route
    on the CPU with the same masks."""
    bb = _bb()
    fx = backbone_common.fixture("backbone_small")
    m = bb.Backbone(**dict(fx["cfg"], dropoutProb=0.0, useGradientCheckpoint=checkpoint))
    m.load_state_dict(fx["sd"], strict=True)
    if form == "A":
        m = m.to(BF16)
    if kind == "truth":
        m = m.to(torch.float64)
    m = m.to(dev).train()
    tc.set_ffn_dropout(m, P_DROP)
    if kind == "fused":
        m.attention = "fused-train"
        m.attentionBf16 = "fused"
        m.attentionBf16Train = "fused"
        _knobs(m)
    else:
        m.attention = "torch"
        tc.patch_reference_blocks(m, P_DROP)
    return m, fx


def _within_gate(form, got, run, seed):
    both = []
    for kind in ("truth", "stock"):
        ref, _ = _model(CPU, form, kind)
        torch.manual_seed(seed)
        both.append(run(ref, kind, CPU))
    top = 0.0
    for a, t, s in zip(got, *both):
        t = t.double()
        gate = max(common.GATE * float((s.double() - t).abs().max()), common.floor_of(form, t))
        err = float((a.double() - t).abs().max())
        top = max(top, err / gate if gate > 0 else (0.0 if err == 0 else float("inf")))
    print(f"form {form}: worst share of the gate {top:.3f}")
    assert top <= 1.0


def _dtype_for(form, kind):
    return torch.float64 if kind == "truth" else common.dtype_of(form)


def _ctx(form, kind, device):
    return common.autocast(form, device) if kind != "truth" else common.autocast("A", device)


def _check_block(dev, form):
    m, fx = _model(dev, form, "fused")

    def run(model, kind, device, checkpoint=False):
        blk = model.encoderLayers[0]
        lin = fx["layer_in"].to(_dtype_for(form, kind)).to(device).clone().requires_grad_()
        with _ctx(form, kind, device):
            if checkpoint:
                from torch.utils.checkpoint import checkpoint as ckpt
                out = ckpt(blk, lin, use_reentrant=False)
            else:
                out = blk(lin)
            loss = out.float().square().sum() if kind != "truth" else out.square().sum()
        loss.backward()
        return [lin.grad.detach().cpu()] + [p.grad.detach().cpu() for p in blk.parameters()]

    n_ff = len(m.encoderLayers[0].feed_forward_blocks())
    torch.manual_seed(11)
    before = common.counts()
    got = run(m, "fused", dev)
    d = common.delta(before)
    assert d == ({"fused": n_ff, "torch": 0}, {"fused": n_ff, "torch": 0, "bwd": n_ff}, {"fused": n_ff, "torch": 0},
                 {"fused": n_ff, "torch": 0, "bwd": n_ff}), d
    _within_gate(form, got, run, 11)
    # recomputation under torch.utils.checkpoint: the preserved RNG state reproduces the seeds, so the same gradient bits
    m.zero_grad()
    torch.manual_seed(11)
    before = common.counts()
    again = run(m, "fused", dev, checkpoint=True)
    d = common.delta(before)
    assert d[3] == {"fused": 2 * n_ff, "torch": 0, "bwd": n_ff} and d[0] == {"fused": 2 * n_ff, "torch": 0}, d   # the recomputed forward is fused too
    assert all(common.bits_equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("form", FORMS)
def test_basic_block_cpu(form):
    _check_block(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_basic_block_gpu(gpu, form):
    _check_block(gpu, form)


def _check_backbone(dev, form):
    m, fx = _model(dev, form, "fused", checkpoint=True)
    assert set(m.state_dict()) == set(fx["sd"])                 # the knob adds no state

    def run(model, kind, device):
        x = fx["x"].to(device)
        x = x.to(_dtype_for(form, kind)) if x.is_floating_point() else x
        with _ctx(form, kind, device):
            out = model(x, fx["outputIndices"].to(device))
            loss = out.float().square().sum() if kind != "truth" else out.square().sum()
        loss.backward()
        return [p.grad.detach().cpu() for p in model.parameters()]

    n_ff = len(m.feed_forward_blocks())
    torch.manual_seed(13)
    before = common.counts()
    got = run(m, "fused", dev)
    d = common.delta(before)
    # useGradientCheckpoint: every layer's forward runs twice, the recomputation with the first pass's masks
    assert d == ({"fused": 2 * n_ff, "torch": 0}, {"fused": 2 * n_ff, "torch": 0, "bwd": n_ff}, {"fused": 2 * n_ff, "torch": 0},
                 {"fused": 2 * n_ff, "torch": 0, "bwd": n_ff}), d
    _within_gate(form, got, run, 13)


@pytest.mark.parametrize("form", FORMS)
def test_backbone_cpu(form):
    _check_backbone(CPU, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_backbone_gpu(gpu, form):
    _check_backbone(gpu, form)


# ---- 8. graph capture ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_gpu(gpu, form):
    """One captured forward + backward replays to the bits of the eager call with the same fixed seed (the seed is a host value; the
    saved buffer and the workspace are allocated by the wrapper inside the capture)."""
    bb = _bb()
    c = common.case(form, 129, 40, 72)
    want = common.run(c, gpu)
    x = c["x"].to(gpu).requires_grad_()
    G = c["G"].to(gpu)
    params = [p.to(gpu).clone().requires_grad_() for p in c["params"]]

    def step():
        with common.autocast(form, gpu):
            out = bb.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", bf16="fused", bf16_train="fused",
                                           p_hidden=c["p1"], p_out=c["p2"], seed=c["seed"])
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
        assert all(common.bits_equal(a.detach().cpu(), b) for a, b in zip(res, want))
