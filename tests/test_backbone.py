"""The backbone and its axial attention: transkun_amd.backbone (csrc/attention.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on
CPU tensors) -- the op against float64 at the tile edges and the model's lengths, its strided contract, padding, determinism and
argument checks, the fall-backs of backbone.axial_attention, and the modules against the reference's fixtures.

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  Yardsticks and gates: backbone_common.
Measured numbers: DESIGN.md section 3, "Backbone attention", and profiles/attention_bench.json."""
import ctypes

import pytest
import torch

import backbone_common as common

CPU = torch.device("cpu")


# ---- 1. the op against float64 ------------------------------------------------------------------------------------------------------
def _check_gate(dev, c, tag):
    got = common.fused(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), c["H"])
    assert got.shape == c["truth"].shape and got.dtype == torch.float32 and got.device.type == dev.type
    assert bool(torch.isfinite(got).all()), tag
    e = float((got.cpu().double() - c["truth"]).abs().max())
    print(f"axial_attention [{dev.type}] {tag}: error {e:.3e}  torch fp32 {c['e32']:.3e}  gate {c['gate']:.3e}")
    assert e <= c["gate"], (tag, e, c["e32"], c["gate"])


def _edge(dev, L, scale):
    _check_gate(dev, common.op_case(L, L, 4, 40, (3,), scale), f"L={L} H=4 d=40 scale={scale:g}")


def _heads(dev, L, H, d, scale):
    _check_gate(dev, common.op_case(L, L, H, d, (3,), scale), f"L={L} H={H} d={d} scale={scale:g}")


def _cross(dev, Lq, Lk, scale):
    _check_gate(dev, common.op_case(Lq, Lk, 4, 40, (3,), scale), f"Lq={Lq} Lk={Lk} H=4 d=40 scale={scale:g}")


def _batch(dev, lead, L):
    _check_gate(dev, common.op_case(L, L, 4, 40, lead, 1.0), f"L={L} sequences={lead}")


def _huge(dev):
    c = common.op_case(149, 149, 4, 40, (3,), 1.0, "huge")
    assert c["logit_max"] > 1000.0
    _check_gate(dev, c, "q, k x 30")


def _negative(dev):
    c = common.op_case(33, 33, 4, 40, (3,), 1.0, "negative")
    assert c["logit_max"] <= -50.0                               # a padded zero column would win the maximum
    _check_gate(dev, c, "all scores <= -50")


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_op_tile_edges_cpu(L, scale):
    _edge(CPU, L, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_op_tile_edges_gpu(gpu, L, scale):
    _edge(gpu, L, scale)


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_op_head_sizes_cpu(L, H, d, scale):
    _heads(CPU, L, H, d, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_op_head_sizes_gpu(gpu, L, H, d, scale):
    _heads(gpu, L, H, d, scale)


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_op_cross_lengths_cpu(Lq, Lk, scale):
    _cross(CPU, Lq, Lk, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_op_cross_lengths_gpu(gpu, Lq, Lk, scale):
    _cross(gpu, Lq, Lk, scale)


@pytest.mark.parametrize("lead,L", common.BATCHES)
def test_op_sequence_counts_cpu(lead, L):
    _batch(CPU, lead, L)


@pytest.mark.gpu
@pytest.mark.parametrize("lead,L", common.BATCHES)
def test_op_sequence_counts_gpu(gpu, lead, L):
    _batch(gpu, lead, L)


def test_op_huge_logits_cpu():
    _huge(CPU)


@pytest.mark.gpu
def test_op_huge_logits_gpu(gpu):
    _huge(gpu)


def test_op_all_scores_negative_cpu():
    _negative(CPU)


@pytest.mark.gpu
def test_op_all_scores_negative_gpu(gpu):
    _negative(gpu)


@pytest.mark.gpu
def test_op_model_shape_gpu(gpu):
    """N = 1 of the model: 89 sequences of 149 tokens and 149 sequences of 89 tokens, H = 4, d = 40, from ONE [1, 89, 149, 160] buffer."""
    g = torch.Generator().manual_seed(4242)
    buf = torch.randn(1, 89, 149, 160, generator=g)
    for tag, view in (("frequency axis", buf), ("time axis", buf.transpose(1, 2))):
        c = common.finish_case(view, view, view, 4)
        dv = buf.to(gpu) if tag == "frequency axis" else buf.to(gpu).transpose(1, 2)
        got = common.fused(dv, dv, dv, 4)
        assert got.stride() == dv.stride()                        # laid out like its query: no transposed copy on the way out
        e = float((got.cpu().double() - c["truth"]).abs().max())
        print(f"axial_attention [cuda] model shape, {tag}: error {e:.3e}  torch fp32 {c['e32']:.3e}  gate {c['gate']:.3e}")
        assert e <= c["gate"], (tag, e, c["e32"])


# ---- 2. layout ------------------------------------------------------------------------------------------------------------------------
def _check_strided_views(dev):
    """The same values as a contiguous [S, L, H d] and as the time-axis view of a [N, L, S / N, H d] buffer: the same bits; output into
    a strided view: the same bits."""
    N, J, L, H, d = 2, 3, 37, 2, 24
    g = torch.Generator().manual_seed(91)
    q, k, v = (torch.randn(N * J, L, H * d, generator=g).to(dev) for _ in range(3))
    want = common.fused(q, k, v, H)

    def time_axis(x):                                            # buffer [N, L, J, HD]; its view [N, J, L, HD]
        buf = x.view(N, J, L, H * d).transpose(1, 2).contiguous()
        view = buf.transpose(1, 2)
        assert not view.is_contiguous() and torch.equal(view.reshape(N * J, L, H * d), x)
        return view
    got = common.fused(time_axis(q), time_axis(k), time_axis(v), H)
    assert got.shape == (N, J, L, H * d) and got.transpose(1, 2).is_contiguous()
    assert common.bits_equal(got.reshape(N * J, L, H * d), want)
    # q alone strided (k, v contiguous in another layout), and a 5-d batch
    got = common.fused(time_axis(q), k.view(N, J, L, H * d), v.view(N, J, L, H * d), H)
    assert common.bits_equal(got.reshape(N * J, L, H * d), want)
    got = common.fused(q.view(N, J, 1, L, H * d), k.view(N, J, 1, L, H * d), v.view(N, J, 1, L, H * d), H)
    assert common.bits_equal(got.reshape(N * J, L, H * d), want)
    # the raw op writing into a strided view of a larger buffer
    big = torch.full((N, L + 2, J + 1, H * d + 8), -7.0, device=dev)
    o4 = big[:, 1:L + 1, :J, 8:].transpose(1, 2)
    common.raw_op(q.view(N, J, L, H * d), k.view(N, J, L, H * d), v.view(N, J, L, H * d), o4, H)
    assert common.bits_equal(o4.reshape(N * J, L, H * d), want)
    # misaligned q and k (one float off a 16-byte boundary): the 4-byte loads give the same bits
    qo, ko = (torch.cat([torch.zeros(N * J, L, 1, device=dev), x], dim=-1)[..., 1:] for x in (q, k))
    assert qo.data_ptr() % 16 != 0
    assert common.bits_equal(common.fused(qo, ko, v, H), want)


def test_strided_views_cpu():
    _check_strided_views(CPU)


@pytest.mark.gpu
def test_strided_views_gpu(gpu):
    _check_strided_views(gpu)


def _check_poison(dev):
    """k and v are the first Lk rows of parents whose 7 further rows hold NaN; out is a view into a buffer prefilled with a sentinel.
    Everything stays inside allocations the test owns."""
    S, Lq, Lk, H, d = 5, 35, 33, 4, 40
    c = common.op_case(Lq, Lk, H, d, (S,), 1.0)
    kp = torch.full((S, Lk + 7, H * d), float("nan"))
    vp = torch.full((S, Lk + 7, H * d), float("nan"))
    kp[:, :Lk], vp[:, :Lk] = c["k"], c["v"]
    kp, vp, q = kp.to(dev), vp.to(dev), c["q"].to(dev)
    SENT = -12345.0
    big = torch.full((S + 2, Lq + 5, H * d + 16), SENT, device=dev)
    out = big[1:S + 1, 2:Lq + 2, 8:8 + H * d]
    common.raw_op(q.unsqueeze(0), kp[:, :Lk].unsqueeze(0), vp[:, :Lk].unsqueeze(0), out.unsqueeze(0), H)
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    e = float((got.double() - c["truth"]).abs().max())
    assert e <= c["gate"], (e, c["e32"])
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:S + 1, 2:Lq + 2, 8:8 + H * d] = False
    assert bool((big[mask] == SENT).all())                       # every sentinel outside the view is untouched


def test_poison_cpu():
    _check_poison(CPU)


@pytest.mark.gpu
def test_poison_gpu(gpu):
    _check_poison(gpu)


def _check_independence(dev):
    """Sequence 0 alone, as sequence 0 of 70 and as sequence 69 of 70: the same bits; two runs: the same bits."""
    c = common.op_case(89, 89, 4, 40, (7, 10), 1.0)
    q, k, v = (c[n].to(dev).reshape(70, 89, 160) for n in "qkv")
    full = common.fused(q, k, v, 4)
    assert common.bits_equal(full, common.fused(q, k, v, 4))
    alone = common.fused(q[:1], k[:1], v[:1], 4)
    assert common.bits_equal(alone, full[:1])
    last = torch.cat([q[1:], q[:1]]), torch.cat([k[1:], k[:1]]), torch.cat([v[1:], v[:1]])
    moved = common.fused(*last, 4)
    assert common.bits_equal(moved[69:], alone) and common.bits_equal(moved[:69], full[1:])
    as_grid = common.fused(q.view(7, 10, 89, 160), k.view(7, 10, 89, 160), v.view(7, 10, 89, 160), 4)
    assert common.bits_equal(as_grid.reshape(70, 89, 160), full)


def test_independence_cpu():
    _check_independence(CPU)


@pytest.mark.gpu
def test_independence_gpu(gpu):
    _check_independence(gpu)


@pytest.mark.gpu
def test_graph_capture_replays_attention(gpu):
    """One capture-and-replay of the op: the replay on new data matches an eager launch bit for bit."""
    H = 4
    data = [tuple(common.op_case(65, 33, H, 40, (3,), s)[n].to(gpu) for n in "qkv") for s in common.SCALES]
    want = [common.fused(q, k, v, H) for q, k, v in data]
    qi, ki, vi = (t.clone() for t in data[0])
    out = torch.empty_like(qi)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        common.raw_op(qi.unsqueeze(0), ki.unsqueeze(0), vi.unsqueeze(0), out.unsqueeze(0), H)
    torch.cuda.current_stream(gpu).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        common.raw_op(qi.unsqueeze(0), ki.unsqueeze(0), vi.unsqueeze(0), out.unsqueeze(0), H)
    for i in (1, 0, 1):
        for dst, src in zip((qi, ki, vi), data[i]):
            dst.copy_(src)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert common.bits_equal(out, want[i])


# ---- 3. contract ------------------------------------------------------------------------------------------------------------------------
def test_supported_set_corners():
    from transkun_amd import _lib, backbone
    lib = _lib.load()
    yes = [(1, 1, 1, 8), (256, 256, 1, 64), (256, 1, 1000, 40), (1, 256, 4, 16), (149, 89, 4, 40), (33, 33, 3, 56)]
    no = [(257, 1, 1, 8), (1, 257, 1, 8), (0, 1, 1, 8), (1, 0, 1, 8), (1, 1, 0, 8), (1, 1, 1, 0), (1, 1, 1, 4), (1, 1, 1, 12),
          (1, 1, 1, 72), (1, 1, 1, 65), (-1, 1, 1, 8), (1, 1, -1, 8)]
    for args in yes:
        assert lib.semicrf_axial_attention_supported(*args) == 1, args
        assert backbone.attention_supported(*args)
    for args in no:
        assert lib.semicrf_axial_attention_supported(*args) == 0, args
    assert _lib.ATTENTION_MAX_L == 256 and _lib.ATTENTION_MAX_D == 64


def _direct(lib, q, k, v, out, n0, n1, Lq, Lk, H, d, strides, stream=None):
    return lib.semicrf_axial_attention(q, k, v, out, n0, n1, Lq, Lk, H, d, *strides, stream)


def test_unsupported_direct_call_is_rejected():
    """An unsupported direct call returns nonzero with a message before any pointer is used (the pointers here are never valid)."""
    from transkun_amd import _lib
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)
    st = [1000, 100, 96, 1000, 100, 96, 1000, 100, 96, 1000, 100, 96]
    for Lq, Lk, H, d, word in ((257, 8, 1, 8, b"supported"), (8, 300, 1, 8, b"supported"), (8, 8, 1, 12, b"supported"),
                               (8, 8, 0, 8, b"supported"), (8, 8, 1, 72, b"supported")):
        assert _direct(lib, fake, fake, fake, fake, 1, 1, Lq, Lk, H, d, st) == 1
        assert word in lib.semicrf_last_error()
    assert _direct(lib, fake, fake, fake, None, 1, 1, 8, 8, 1, 8, st) == 1 and b"NULL" in lib.semicrf_last_error()
    assert _direct(lib, fake, fake, fake, fake, -1, 1, 8, 8, 1, 8, st) == 1
    assert _direct(lib, fake, fake, fake, fake, 1 << 20, 1 << 12, 8, 8, 1, 8, st) == 1 and b"2^31" in lib.semicrf_last_error()
    bad = list(st); bad[5] = -96
    assert _direct(lib, fake, fake, fake, fake, 1, 1, 8, 8, 1, 8, bad) == 1 and b"negative" in lib.semicrf_last_error()
    assert _direct(lib, fake, fake, fake, fake, 0, 5, 8, 8, 1, 8, st) == 0           # no sequences: nothing to do, nothing launched
    # the torch op checks the same set (and the shapes) before anything runs
    ops = _lib.ops()
    x = torch.zeros(1, 1, 4, 12)
    with pytest.raises(RuntimeError, match="support"):
        ops.axial_attention(x, x, x, torch.empty_like(x), 1)
    y = torch.zeros(1, 1, 4, 16)
    with pytest.raises(RuntimeError):
        ops.axial_attention(y, y, y, torch.empty(1, 1, 5, 16), 2)
    with pytest.raises(RuntimeError):
        ops.axial_attention(y, y, y.double(), torch.empty_like(y), 2)
    with pytest.raises(RuntimeError):
        ops.axial_attention(y.transpose(-1, -2), y, y, torch.empty_like(y), 2)


@pytest.mark.gpu
def test_unsupported_direct_call_leaves_output_untouched_gpu(gpu):
    from transkun_amd import _lib
    lib = _lib.load()
    x = torch.randn(2, 8, 12, device=gpu)
    out = torch.full_like(x, 3.0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = [0, 96, 12] * 4
    rc = _direct(lib, p(x), p(x), p(x), p(out), 1, 2, 8, 8, 1, 12, st, _lib.stream_of(x))
    torch.cuda.synchronize(gpu)
    assert rc == 1 and b"supported" in lib.semicrf_last_error()
    assert bool((out == 3.0).all())


def _check_fallbacks(dev):
    """Outside the op's reach backbone.axial_attention IS the stock route: the same bits."""
    from transkun_amd import backbone
    g = torch.Generator().manual_seed(5)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=g).to(dtype).to(dev)
    with torch.no_grad():
        for q, k, v, H in ((rnd(2, 257, 32), rnd(2, 257, 32), rnd(2, 257, 32), 2),                      # L = 257
                           (rnd(2, 9, 24), rnd(2, 9, 24), rnd(2, 9, 24), 2),                            # d = 12
                           (rnd(2, 9, 32, dtype=torch.bfloat16),) * 3 + (2,),                           # bf16
                           (rnd(2, 3, 9, 32), rnd(2, 1, 7, 32), rnd(2, 1, 7, 32), 2)):                  # k, v broadcast against q
            got = backbone.axial_attention(q, k, v, H)
            assert torch.equal(got, backbone.attention_torch(q, k, v, H)) and got.dtype == q.dtype
        q, k, v = rnd(3, 9, 32), rnd(3, 7, 32), rnd(3, 7, 32)
        assert torch.equal(backbone.axial_attention(q, k, v, 2, route="torch"), backbone.attention_torch(q, k, v, 2))
    with pytest.raises(ValueError):
        backbone.axial_attention(q, k, v, 2, route="eager")
    # an input that requires grad: the stock route, and its gradients
    grads = []
    for fn in (lambda a, b, c: backbone.axial_attention(a, b, c, 2), lambda a, b, c: backbone.attention_torch(a, b, c, 2)):
        a, b, c = (t.clone().requires_grad_() for t in (q, k, v))
        out = fn(a, b, c)
        assert out.requires_grad
        out.square().sum().backward()
        grads.append((out.detach(), a.grad, b.grad, c.grad))
    for x, y in zip(*grads):
        assert x is not None and torch.equal(x, y)
    with torch.no_grad():                                         # under no_grad the same tensors take the op
        a = q.clone().requires_grad_()
        assert not backbone.axial_attention(a, k, v, 2).requires_grad


def test_fallbacks_cpu():
    _check_fallbacks(CPU)


@pytest.mark.gpu
def test_fallbacks_gpu(gpu):
    _check_fallbacks(gpu)


# ---- 4. the modules against the reference's fixtures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", common.FIXTURES)
def test_state_dict_loads_strict(name):
    from transkun_amd import backbone
    fx = common.fixture(name)
    m = backbone.Backbone(**fx["cfg"])
    assert set(m.state_dict().keys()) == set(fx["sd"].keys())
    m.load_state_dict(fx["sd"], strict=True)
    names = set(fx["sd"])
    for want in ("encoderLayers.0.mhaBlockF.scale", "encoderLayers.0.mhaBlockF.module.q_proj_weight",
                 "encoderLayers.0.mhaBlockT.module.out_proj.bias", "encoderLayers.0.fnnBlockT.module.3.weight", "inputConv.weight",
                 "downConv.13.weight", "upConv1dSkip.weight", "posEmbedBuilderAttnTE.mlp.0.weight", "posEmbedBuilder.proj.bias"):
        assert want in names, want
    assert m.attention == backbone.DEFAULT_ATTENTION
    m.attention = "torch"
    assert all(a.attention == "torch" for a in m.modules() if isinstance(a, backbone.MultiHeadAttentionKernel))
    with pytest.raises(ValueError):
        m.attention = "eager"
    with pytest.raises(NotImplementedError):
        backbone.MultiHeadAttentionKernel(16, 2, kernel="fourier")(torch.zeros(1, 3, 16))
    assert backbone.MultiHeadAttentionKernel(160, 4, kernel=None).head_dim == 40
    assert backbone.MultiHeadAttentionKernel(10, 4, kernel=None, hiddenFactor=0.5).head_dim == 2


def _check_modules(dev, name, route):
    m, fx = common.make_backbone(name, dev, route)
    x, idx = fx["x"].to(dev), fx["outputIndices"].to(dev)
    blk = m.encoderLayers[0]
    mha = blk.mhaBlockF.module
    lin, mem, key = fx["layer_in"].to(dev), fx["layer_mem"].to(dev), fx["mha_key"].to(dev)
    with torch.no_grad():
        got = {"out": m(x, idx), "block_out": blk(lin), "block_mem_out": blk(lin, mem), "mha_out": mha(lin), "mha_mem_out": mha(lin, key)}
    for tag, g in got.items():
        want64, ref32 = fx[tag + "64"], fx[tag + "32"]
        assert g.shape == want64.shape and g.dtype == torch.float32
        e32 = float((ref32.double() - want64).abs().max())
        e = float((g.cpu().double() - want64).abs().max())
        print(f"{name} [{dev.type}, {route}] {tag}: error {e:.3e}  reference fp32 {e32:.3e}  ratio {e / e32:.2f} (gate {common.GATE:g})")
        assert e <= common.GATE * e32, (tag, e, e32)


@pytest.mark.parametrize("route", ["fused", "torch"])
@pytest.mark.parametrize("name", common.FIXTURES)
def test_modules_match_reference_cpu(name, route):
    _check_modules(CPU, name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["fused", "torch"])
@pytest.mark.parametrize("name", common.FIXTURES)
def test_modules_match_reference_gpu(gpu, name, route):
    _check_modules(gpu, name, route)


def test_gradient_checkpoint_switch_and_training_route():
    """useGradientCheckpoint / training mode run the layers under torch.utils.checkpoint as the reference does; under autograd the
    attention takes the stock route, so the fused default trains: gradients reach every parameter and equal the torch route's."""
    from transkun_amd import backbone
    fx = common.fixture("backbone_small")
    grads = {}
    for route in ("fused", "torch"):
        cfg = dict(fx["cfg"], useGradientCheckpoint=True, dropoutProb=0.0)
        m = backbone.Backbone(**cfg)
        m.load_state_dict(fx["sd"], strict=True)
        m.attention = route
        m.train()
        out = m(fx["x"], fx["outputIndices"])
        out.square().sum().backward()
        assert all(p.grad is not None for p in m.parameters())
        grads[route] = torch.cat([p.grad.flatten() for p in m.parameters()])
    scale = float(grads["torch"].abs().max())
    assert float((grads["fused"] - grads["torch"]).abs().max()) <= 1e-5 * scale


def test_basic_block_makes_no_transposed_copy():
    """On the fused route a BasicBlock forward copies no hidden-state-sized tensor: no clone / contiguous / _to_copy / copy_ of one, and
    everything that is not the attention runs on the [N, T, F, D] buffer as it is.  The torch route, counted the same way, does."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m, fx = common.make_backbone("backbone_d40", CPU, "fused")
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
    for route in ("fused", "torch"):
        blk.attention = route
        with torch.no_grad(), Count() as c:
            blk(lin)
        counts[route] = c.copies
    assert counts["fused"] == [], counts["fused"]
    assert len(counts["torch"]) > 0                              # the counter sees the stock route's copies


@pytest.mark.gpu
def test_end_to_end_decode_gpu(gpu):
    """audio -> MelSpectrum -> Backbone (small fixture, fused) -> interval scorer -> NeuralSemiCRFInterval.decode(): the decoded paths
    equal those of attention = "torch"."""
    from transkun_amd import CRF, synth
    from transkun_amd.frontend import MelSpectrum, makeFrame, normalize_gain
    from transkun_amd.scorer import ScaledInnerProductIntervalScorer
    fs, hop, win = 44100, 1024, 4096
    nS = 2 * fs
    audio = synth.hash_normal(2 * nS, 971, gpu).view(1, 2, nS) * 0.1
    frames = makeFrame(audio, hop, win)
    mel = MelSpectrum(win, 30, 8000, 229, fs, nExtraWins=5, log=True, toMono=True).to(gpu)
    feat = mel(normalize_gain(frames))[:, 0]                      # [N, T, 229, 6]
    T = feat.shape[1]
    m, fx = common.make_backbone("backbone_small", gpu, "fused")
    idx = fx["outputIndices"].to(gpu)
    D = fx["cfg"]["baseSize"] * fx["cfg"]["expansionFactor"]
    torch.manual_seed(67280421310721)
    scorer = ScaledInnerProductIntervalScorer(D, 1).to(gpu)
    paths = {}
    with torch.no_grad():
        for route in ("fused", "torch"):
            m.attention = route
            ctx = m(feat, idx)
            assert ctx.shape == (1, idx.numel(), T, D) and bool(torch.isfinite(ctx).all())
            S, b = scorer(ctx)
            paths[route] = CRF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1)).decode()
    assert len(paths["fused"]) == idx.numel() and paths["fused"] == paths["torch"]
