"""The backward of the backbone's axial attention and the training route built on it: torch.ops.semicrf.axial_attention_bwd
(csrc/attention_bwd.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on CPU tensors), backbone.axial_attention(route="fused-train")
and the modules under attention = "fused-train" -- the gradients against float64 autograd at the tile edges and the model's lengths,
in every instantiation <key tiles, output blocks> of the kernel and over the query side, at the limits of its LDS and register budget,
the strided contract (both axes of one buffer, a transposed cotangent, stride 0, misalignment, NULL gradients, poison), determinism,
argument checks, the fall-backs of the route, and that a BasicBlock trains without a transposed copy.

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  Yardsticks and gates: backbone_bwd_common.
Measured numbers: DESIGN.md section 3, "Backbone attention, training", and profiles/attention_bwd_bench.json."""
import ctypes

import pytest
import torch

import backbone_common as common
import backbone_bwd_common as bwd

CPU = torch.device("cpu")


# ---- 1. the gradients against float64 -----------------------------------------------------------------------------------------------
def _edge(dev, L, scale):
    bwd.check_gate(dev, bwd.bwd_case(L, L, 4, 40, (3,), scale), f"L={L} H=4 d=40 scale={scale:g}")


def _cross(dev, Lq, Lk, scale):
    bwd.check_gate(dev, bwd.bwd_case(Lq, Lk, 4, 40, (3,), scale), f"Lq={Lq} Lk={Lk} H=4 d=40 scale={scale:g}")


def _heads(dev, L, H, d):
    bwd.check_gate(dev, bwd.bwd_case(L, L, H, d, (3,), 1.0), f"L={L} H={H} d={d}")


def _huge(dev):
    c = bwd.bwd_case(149, 149, 4, 40, (3,), 1.0, "huge")
    assert c["logit_max"] > 1000.0
    bwd.check_gate(dev, c, "q, k x 30")


def _negative(dev):
    c = bwd.bwd_case(33, 33, 4, 40, (3,), 1.0, "negative")
    assert c["logit_max"] <= -50.0
    bwd.check_gate(dev, c, "all scores <= -50")


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_bwd_tile_edges_cpu(L, scale):
    _edge(CPU, L, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_bwd_tile_edges_gpu(gpu, L, scale):
    _edge(gpu, L, scale)


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bwd_cross_lengths_cpu(Lq, Lk, scale):
    _cross(CPU, Lq, Lk, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bwd_cross_lengths_gpu(gpu, Lq, Lk, scale):
    _cross(gpu, Lq, Lk, scale)


@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_bwd_head_sizes_cpu(L, H, d):
    _heads(CPU, L, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_bwd_head_sizes_gpu(gpu, L, H, d):
    _heads(gpu, L, H, d)


def test_bwd_huge_logits_cpu():
    _huge(CPU)


@pytest.mark.gpu
def test_bwd_huge_logits_gpu(gpu):
    _huge(gpu)


def test_bwd_all_scores_negative_cpu():
    _negative(CPU)


@pytest.mark.gpu
def test_bwd_all_scores_negative_gpu(gpu):
    _negative(gpu)


# ---- 2. every instantiation of the kernel, the query side, the largest shape, co-residency -------------------------------------------
def _instantiation(dev, d, Lk):
    """<NKT = ceil(Lk / 32), DB = 1 | 2> through the raw ops: gated on aligned tensors; with q, k, v, out, dout and the gradients one
    float off 16 bytes, the aligned call's bits."""
    c = bwd.bwd_case(common.MATRIX_LQ, Lk, common.MATRIX_H, d, (3,), 1.0)
    want = bwd.raw_case(dev, c)
    bwd.check_gate(dev, c, f"<NKT={(Lk + 31) // 32}, DB={1 if d <= 32 else 2}> Lq={common.MATRIX_LQ} Lk={Lk} d={d}",
                   [g.reshape(t.shape) for g, t in zip(want, c["truth_g"])])
    got = bwd.raw_case(dev, c, off=True)
    for name, a, b in zip(bwd.NAMES, got, want):
        assert a.data_ptr() % 16 != 0
        assert common.bits_equal(a, b), (name, d, Lk)


@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bwd_every_instantiation_cpu(d, Lk):
    _instantiation(CPU, d, Lk)


@pytest.mark.gpu
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bwd_every_instantiation_gpu(gpu, d, Lk):
    _instantiation(gpu, d, Lk)


def _query_side(dev, Lq, Lk, d):
    bwd.check_gate(dev, bwd.bwd_case(Lq, Lk, 2, d, (3,), 1.0), f"query side Lq={Lq} Lk={Lk} H=2 d={d}")


@pytest.mark.parametrize("Lq,Lk,d", bwd.QUERY_SIDE)
def test_bwd_query_side_cpu(Lq, Lk, d):
    _query_side(CPU, Lq, Lk, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,d", bwd.QUERY_SIDE)
def test_bwd_query_side_gpu(gpu, Lq, Lk, d):
    _query_side(gpu, Lq, Lk, d)


def _largest(dev):
    Lq, Lk, H, d, lead = common.LARGEST
    bwd.check_gate(dev, bwd.bwd_case(Lq, Lk, H, d, lead, 1.0), f"largest Lq={Lq} Lk={Lk} H={H} d={d}")


def test_bwd_largest_configuration_cpu():
    _largest(CPU)


@pytest.mark.gpu
def test_bwd_largest_configuration_gpu(gpu):
    _largest(gpu)


def _coresident(dev):
    """More workgroups than two per CU: 70 sequences x 8 heads at L = 149, d = 64.  Sequence 0 alone gives the bits of its slice."""
    Lq, Lk, H, d, lead = common.CORESIDENT
    c = bwd.bwd_case(Lq, Lk, H, d, lead, 1.0)
    q, k, v, g = (c[n].to(dev) for n in ("q", "k", "v", "dout"))
    full = bwd.route_grads(q, k, v, g, H)
    bwd.check_gate(dev, c, f"co-resident {lead} x H={H} L={Lq} d={d}", full[1:])
    alone = bwd.route_grads(q[:1, :1], k[:1, :1], v[:1, :1], g[:1, :1], H)
    for name, a, b in zip(("out",) + bwd.NAMES, alone, full):
        assert common.bits_equal(a, b[:1, :1]), name


def test_bwd_coresident_workgroups_cpu():
    _coresident(CPU)


@pytest.mark.gpu
def test_bwd_coresident_workgroups_gpu(gpu):
    _coresident(gpu)


# ---- 3. the contract ------------------------------------------------------------------------------------------------------------------
def _contract(dev):
    Lq, Lk, H, d, lead = common.CONTRACT
    c = bwd.bwd_case(Lq, Lk, H, d, lead, 1.0)
    return c, H, tuple(c[n].to(dev) for n in ("q", "k", "v", "dout"))


def _check_axis_views(dev):
    """Frequency- and time-axis views of one [N, T', F', H d] buffer; the cotangent as a transposed view: the bits of the contiguous
    call, gradients laid out like their inputs."""
    N, J, L, H, d = 2, 3, 37, 2, 24
    g = torch.Generator().manual_seed(92)
    q, k, v, go = (torch.randn(N * J, L, H * d, generator=g).to(dev) for _ in range(4))
    want = bwd.route_grads(q, k, v, go, H)

    def time_axis(x):                                            # buffer [N, L, J, HD]; its view [N, J, L, HD]
        return x.view(N, J, L, H * d).transpose(1, 2).contiguous().transpose(1, 2)
    got = bwd.route_grads(time_axis(q), time_axis(k), time_axis(v), time_axis(go), H)
    for name, a, b in zip(("out",) + bwd.NAMES, got, want):
        assert a.shape == (N, J, L, H * d) and a.transpose(1, 2).is_contiguous(), name      # transposes back into a contiguous tensor
        assert common.bits_equal(a.reshape(N * J, L, H * d), b), name
    # the frequency axis of the same buffers ([N, J, L, HD] contiguous), and dout alone transposed
    got = bwd.route_grads(q.view(N, J, L, -1), k.view(N, J, L, -1), v.view(N, J, L, -1), time_axis(go), H)
    for name, a, b in zip(("out",) + bwd.NAMES, got, want):
        assert a.is_contiguous() and common.bits_equal(a.reshape(N * J, L, H * d), b), name
    # the raw op writing the gradients into strided views of larger buffers
    q4, k4, v4, g4 = (x.view(N, J, L, H * d) for x in (q, k, v, go))
    o4 = bwd.raw_fwd(q4, k4, v4, H)
    bigs = [torch.full((N, L + 2, J + 1, H * d + 8), -7.0, device=dev) for _ in range(3)]
    views = [b[:, 1:L + 1, :J, 8:].transpose(1, 2) for b in bigs]
    bwd.raw_bwd(q4, k4, v4, o4, g4, H, *views)
    for name, a, b in zip(bwd.NAMES, views, want[1:]):
        assert common.bits_equal(a.reshape(N * J, L, H * d), b), name


def test_bwd_axis_views_cpu():
    _check_axis_views(CPU)


@pytest.mark.gpu
def test_bwd_axis_views_gpu(gpu):
    _check_axis_views(gpu)


def _check_stride_zero(dev):
    """k and v, then q, expanded over the sequences (stride 0): the bits of their contiguous copies, full-size gradients."""
    c, H, (q, k, v, g) = _contract(dev)
    k0, v0 = k[:1].expand(3, -1, -1), v[:1].expand(3, -1, -1)
    q4, g4 = bwd.as4(q), bwd.as4(g)
    k4, v4 = k0.unsqueeze(1), v0.unsqueeze(1)
    assert k4.stride(0) == 0 and v4.stride(0) == 0
    kc, vc = k4.contiguous(), v4.contiguous()
    o4 = bwd.raw_fwd(q4, kc, vc, H)
    want = bwd.raw_bwd(q4, kc, vc, o4, g4, H)
    got = bwd.raw_bwd(q4, k4, v4, o4, g4, H)
    for name, a, b in zip(bwd.NAMES, got, want):
        assert a.shape == b.shape and common.bits_equal(a, b), name
    q0 = q[:1].expand(3, -1, -1).unsqueeze(1)
    assert q0.stride(0) == 0
    k4, v4 = bwd.as4(k), bwd.as4(v)
    o4 = bwd.raw_fwd(q0.contiguous(), k4, v4, H)
    want = bwd.raw_bwd(q0.contiguous(), k4, v4, o4, g4, H)
    got = bwd.raw_bwd(q0, k4, v4, o4, g4, H, dq=torch.empty_like(want[0]))
    for name, a, b in zip(bwd.NAMES, got, want):
        assert common.bits_equal(a, b), name
    # through the route: autograd sums the expanded input's gradient, as on the stock route
    kk = k[:1].clone().requires_grad_()
    from transkun_amd import backbone
    backbone.axial_attention(q, kk.expand(3, -1, -1), v, H, route="fused-train").backward(g)
    assert kk.grad.shape == (1,) + k.shape[1:] and bool(torch.isfinite(kk.grad).all())


def test_bwd_stride_zero_cpu():
    _check_stride_zero(CPU)


@pytest.mark.gpu
def test_bwd_stride_zero_gpu(gpu):
    _check_stride_zero(gpu)


def _check_independence(dev):
    """Sequence 0 alone, as sequence 0 of 70 and as sequence 69 of 70, and as a 7 x 10 grid: the same bits; two runs: the same bits."""
    c = bwd.bwd_case(89, 89, 4, 40, (7, 10), 1.0)
    q, k, v, g = (c[n].to(dev).reshape(70, 89, 160) for n in ("q", "k", "v", "dout"))
    full = bwd.route_grads(q, k, v, g, 4)
    again = bwd.route_grads(q, k, v, g, 4)
    alone = bwd.route_grads(q[:1], k[:1], v[:1], g[:1], 4)
    moved = bwd.route_grads(*(torch.cat([t[1:], t[:1]]) for t in (q, k, v, g)), 4)
    grid = bwd.route_grads(*(t.view(7, 10, 89, 160) for t in (q, k, v, g)), 4)
    for name, f, a, one, m, gr in zip(("out",) + bwd.NAMES, full, again, alone, moved, grid):
        assert common.bits_equal(f, a), name
        assert common.bits_equal(one, f[:1]), name
        assert common.bits_equal(m[69:], one) and common.bits_equal(m[:69], f[1:]), name
        assert common.bits_equal(gr.reshape(70, 89, 160), f), name


def test_bwd_independence_cpu():
    _check_independence(CPU)


@pytest.mark.gpu
def test_bwd_independence_gpu(gpu):
    _check_independence(gpu)


def _check_null_gradients(dev):
    """dq / dk / dv None one at a time: the other two keep their bits."""
    c, H, (q, k, v, g) = _contract(dev)
    q4, k4, v4, g4 = (bwd.as4(t) for t in (q, k, v, g))
    o4 = bwd.raw_fwd(q4, k4, v4, H)
    want = bwd.raw_bwd(q4, k4, v4, o4, g4, H)
    for skip in range(3):
        flags = [None if i == skip else True for i in range(3)]
        got = bwd.raw_bwd(q4, k4, v4, o4, g4, H, *flags)
        for i, name in enumerate(bwd.NAMES):
            if i == skip:
                assert got[i] is None
            else:
                assert common.bits_equal(got[i], want[i]), (name, "without", bwd.NAMES[skip])
    only_dv = bwd.raw_bwd(q4, k4, v4, o4, g4, H, None, None, True)
    assert common.bits_equal(only_dv[2], want[2])
    bwd.raw_bwd(q4, k4, v4, o4, g4, H, None, None, None)        # nothing wanted: nothing to do


def test_bwd_null_gradients_cpu():
    _check_null_gradients(CPU)


@pytest.mark.gpu
def test_bwd_null_gradients_gpu(gpu):
    _check_null_gradients(gpu)


def _check_poison(dev):
    """q, k, v, out, dout are views into NaN-filled buffers, with NaN behind every row past Lq / Lk and beside every row; the gradients
    are views into sentinel-filled buffers.  The results are finite and gated, every sentinel is untouched."""
    S, Lq, Lk, H, d = 5, 35, 33, 4, 40
    c = bwd.bwd_case(Lq, Lk, H, d, (S,), 1.0)
    HD = H * d

    def inside(x, fill):
        L = x.shape[1]
        big = torch.full((S + 2, L + 7, HD + 16), fill)
        big[1:S + 1, 2:L + 2, 8:8 + HD] = x
        big = big.to(dev)
        return big, big[1:S + 1, 2:L + 2, 8:8 + HD].unsqueeze(0)
    nan = float("nan")
    (_, q4), (_, k4), (_, v4), (_, g4) = (inside(c[n], nan) for n in ("q", "k", "v", "dout"))
    _, o4 = inside(torch.zeros(S, Lq, HD), nan)
    common.raw_op(q4, k4, v4, o4, H)
    SENT = -12345.0
    outs = [inside(torch.full((S, L, HD), SENT), SENT) for L in (Lq, Lk, Lk)]
    bwd.raw_bwd(q4, k4, v4, o4, g4, H, *(view for _, view in outs))
    bwd.check_gate(dev, c, "poison", [view[0] for _, view in outs])
    for (big, _), L in zip(outs, (Lq, Lk, Lk)):
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:S + 1, 2:L + 2, 8:8 + HD] = False
        assert bool((big[mask] == SENT).all())                   # every sentinel outside the view is untouched


def test_bwd_poison_cpu():
    _check_poison(CPU)


@pytest.mark.gpu
def test_bwd_poison_gpu(gpu):
    _check_poison(gpu)


def _direct(lib, ptrs, n0, n1, Lq, Lk, H, d, strides, stream=None):
    return lib.semicrf_axial_attention_bwd(*ptrs, n0, n1, Lq, Lk, H, d, *strides, stream)


def test_bwd_supported_set_and_rejected_direct_calls():
    """The supported set is the forward's; an unsupported direct call returns nonzero with a message before any pointer is used (the
    pointers here are never valid)."""
    from transkun_amd import _lib, backbone
    lib = _lib.load()
    for args in [(1, 1, 1, 8), (256, 256, 1, 64), (256, 1, 1000, 40), (1, 256, 4, 16), (149, 89, 4, 40), (160, 160, 4, 64)]:
        assert lib.semicrf_axial_attention_bwd_supported(*args) == 1 and backbone.attention_bwd_supported(*args), args
    for args in [(257, 1, 1, 8), (1, 257, 1, 8), (0, 1, 1, 8), (1, 0, 1, 8), (1, 1, 0, 8), (1, 1, 1, 4), (1, 1, 1, 12), (1, 1, 1, 72)]:
        assert lib.semicrf_axial_attention_bwd_supported(*args) == 0 and not backbone.attention_bwd_supported(*args), args
    for L in range(1, 161):                                      # every L <= 160 with d <= 64
        assert all(lib.semicrf_axial_attention_bwd_supported(L, L, 4, d) == 1 for d in range(8, 65, 8)), L
    fake = ctypes.c_void_p(4096)
    ptrs = [fake] * 8
    st = [1000, 100, 96] * 8
    for Lq, Lk, H, d in ((257, 8, 1, 8), (8, 300, 1, 8), (8, 8, 1, 12), (8, 8, 0, 8), (8, 8, 1, 72)):
        assert _direct(lib, ptrs, 1, 1, Lq, Lk, H, d, st) == 1 and b"supported" in lib.semicrf_last_error()
    for i in range(5):                                           # q, k, v, out, dout must be there
        bad = list(ptrs); bad[i] = None
        assert _direct(lib, bad, 1, 1, 8, 8, 1, 8, st) == 1 and b"NULL" in lib.semicrf_last_error()
    assert _direct(lib, ptrs, -1, 1, 8, 8, 1, 8, st) == 1
    assert _direct(lib, ptrs, 1 << 20, 1 << 12, 8, 8, 1, 8, st) == 1 and b"2^31" in lib.semicrf_last_error()
    bad = list(st); bad[13] = -96
    assert _direct(lib, ptrs, 1, 1, 8, 8, 1, 8, bad) == 1 and b"negative" in lib.semicrf_last_error()
    for i in range(2, 24, 3):                                    # a token stride of 2^28 elements, one tensor at a time
        bad = list(st); bad[i] = common.TOKEN_STRIDE_LIMIT
        assert _direct(lib, ptrs, 1, 1, 8, 8, 1, 8, bad) == 1 and b"2^28" in lib.semicrf_last_error(), i
    assert _direct(lib, ptrs, 0, 5, 8, 8, 1, 8, st) == 0         # no sequences: nothing to do, nothing launched
    # the torch op checks the same set, the shapes and the layouts before anything runs
    ops = _lib.ops()
    x = torch.zeros(1, 1, 4, 12)
    with pytest.raises(RuntimeError, match="support"):
        ops.axial_attention_bwd(x, x, x, x, x, torch.empty_like(x), None, None, 1)
    y = torch.zeros(1, 1, 4, 16)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bwd(y, y, y, y, y, torch.empty(1, 1, 5, 16), None, None, 2)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bwd(y, y, y, y, y.double(), None, None, torch.empty_like(y), 2)
    with pytest.raises(RuntimeError, match="repeat"):
        ops.axial_attention_bwd(y, y, y, y, y, torch.empty(1, 1, 1, 16).expand(1, 1, 4, 16), None, None, 2)


@pytest.mark.gpu
def test_bwd_rejected_direct_call_leaves_gradients_untouched_gpu(gpu):
    """An unsupported head dimension, and a token stride of 2^28 forged on small tensors: rejected, dq / dk / dv untouched."""
    from transkun_amd import _lib
    lib = _lib.load()
    x = torch.randn(2, 8, 16, device=gpu)
    grads = [torch.full_like(x, 3.0) for _ in range(3)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ptrs = [p(x)] * 5 + [p(g) for g in grads]
    rc = _direct(lib, ptrs, 1, 2, 8, 8, 1, 12, [0, 96, 12] * 8, _lib.stream_of(x))
    assert rc == 1 and b"supported" in lib.semicrf_last_error()
    for i in range(2, 24, 3):
        st = [0, 128, 16] * 8
        st[i] = common.TOKEN_STRIDE_LIMIT
        rc = _direct(lib, ptrs, 1, 2, 8, 8, 1, 16, st, _lib.stream_of(x))
        assert rc == 1 and b"2^28" in lib.semicrf_last_error(), i
    torch.cuda.synchronize(gpu)
    assert all(bool((g == 3.0).all()) for g in grads)


# ---- 4. the Python route --------------------------------------------------------------------------------------------------------------
def _counts():
    from transkun_amd import backbone
    return dict(backbone.ATTENTION_ROUTES)


def _delta(before):
    now = _counts()
    return {k: now[k] - before[k] for k in now}


def _check_route(dev):
    from transkun_amd import backbone
    assert backbone.ROUTES == ("fused", "fused-train", "torch") and backbone.DEFAULT_ATTENTION == "fused"
    c, H, (q, k, v, g) = _contract(dev)
    # no gradient wanted: exactly "fused"
    before = _counts()
    with torch.no_grad():
        a = backbone.axial_attention(q.clone().requires_grad_(), k, v, H, route="fused-train")
        b = backbone.axial_attention(q, k, v, H, route="fused")
    plain = backbone.axial_attention(q, k, v, H, route="fused-train")          # gradients enabled, nothing requires one
    assert _delta(before) == {"fused": 3, "fused-train": 0, "torch": 0, "bwd": 0}
    assert not a.requires_grad and common.bits_equal(a, b) and common.bits_equal(plain, b)
    # under autograd: the Function, once; its gradients pass the gate
    before = _counts()
    got = bwd.route_grads(q, k, v, g, H)
    assert _delta(before) == {"fused": 0, "fused-train": 1, "torch": 0, "bwd": 1}
    assert common.bits_equal(got[0], b)
    bwd.check_gate(dev, c, "route fused-train", got[1:])
    # an input that needs no gradient gets None, the others keep their bits
    for skip in range(3):
        needs = tuple(i != skip for i in range(3))
        part = bwd.route_grads(q, k, v, g, H, needs=needs)
        for i in range(3):
            assert (part[1 + i] is None) if i == skip else common.bits_equal(part[1 + i], got[1 + i])
    # "fused" under autograd is still the stock route
    before = _counts()
    stock = bwd.route_grads(q, k, v, g, H, route="fused")
    assert _delta(before) == {"fused": 0, "fused-train": 0, "torch": 1, "bwd": 0}
    want = bwd.route_grads(q, k, v, g, H, route="torch")
    assert all(torch.equal(x, y) for x, y in zip(stock, want))


def test_route_cpu():
    _check_route(CPU)


@pytest.mark.gpu
def test_route_gpu(gpu):
    _check_route(gpu)


def _check_route_fallbacks(dev):
    """Outside the supported set, for bf16 and for broadcasting keys "fused-train" is the stock route bit for bit, forward and
    gradients."""
    from transkun_amd import backbone
    g = torch.Generator().manual_seed(78)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    cases = {"L > 256": (rnd(2, 300, 32), rnd(2, 300, 32), rnd(2, 300, 32), 2),
             "d = 12": (rnd(2, 9, 24), rnd(2, 9, 24), rnd(2, 9, 24), 2),
             "d = 72": (rnd(2, 9, 144), rnd(2, 9, 144), rnd(2, 9, 144), 2),
             "bf16": (rnd(2, 9, 32).bfloat16(), rnd(2, 9, 32).bfloat16(), rnd(2, 9, 32).bfloat16(), 2),
             "broadcast keys": (rnd(4, 3, 9, 32), rnd(1, 3, 7, 32), rnd(1, 3, 7, 32), 2)}
    for tag, (q, k, v, H) in cases.items():
        go = torch.randn(q.shape, generator=g).to(dev).to(q.dtype)
        before = _counts()
        got = bwd.route_grads(q, k, v, go, H)
        assert _delta(before) == {"fused": 0, "fused-train": 0, "torch": 1, "bwd": 0}, tag
        want = bwd.route_grads(q, k, v, go, H, route="torch")
        for a, b in zip(got, want):
            assert a.dtype == q.dtype and torch.equal(a, b), tag


def test_route_fallbacks_cpu():
    _check_route_fallbacks(CPU)


@pytest.mark.gpu
def test_route_fallbacks_gpu(gpu):
    _check_route_fallbacks(gpu)


def test_route_second_derivative_raises():
    from transkun_amd import backbone
    c, H, (q, k, v, g) = _contract(CPU)
    q, g = q.clone().requires_grad_(), g.clone().requires_grad_()
    out = backbone.axial_attention(q, k, v, H, route="fused-train")
    (dq,) = torch.autograd.grad(out, q, g, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        dq.sum().backward()


def test_route_names_are_checked():
    from transkun_amd import backbone
    x = torch.zeros(1, 4, 16)
    with pytest.raises(ValueError):
        backbone.axial_attention(x, x, x, 2, route="fused-training")
    m, _ = common.make_backbone("backbone_small", CPU, "fused-train")
    assert m.attention == "fused-train" and all(b.attention == "fused-train" for b in m.encoderLayers)
    with pytest.raises(ValueError):
        m.attention = "train"


# ---- 5. the modules -------------------------------------------------------------------------------------------------------------------
def _train_grads(dev, route, checkpoint):
    from transkun_amd import backbone
    fx = common.fixture("backbone_small")
    m = backbone.Backbone(**dict(fx["cfg"], useGradientCheckpoint=checkpoint, dropoutProb=0.0))
    m.load_state_dict(fx["sd"], strict=True)
    m.attention = route
    m.to(dev).train()
    before = _counts()
    out = m(fx["x"].to(dev), fx["outputIndices"].to(dev))
    out.square().sum().backward()
    assert all(p.grad is not None for p in m.parameters())
    n_calls = sum(isinstance(x, backbone.MultiHeadAttentionKernel) for x in m.modules())
    return torch.cat([p.grad.flatten() for p in m.parameters()]).cpu(), _delta(before), n_calls


def _check_backbone_trains(dev, checkpoint):
    """Backbone in training mode under "fused-train": every parameter gets a gradient, the flat gradient is the torch route's within
    1e-5 x its largest entry (the bound of the existing training-route test), and the HIP backward ran once per attention call."""
    want, d_torch, n_calls = _train_grads(dev, "torch", checkpoint)
    got, d_train, _ = _train_grads(dev, "fused-train", checkpoint)
    assert d_torch["bwd"] == 0 and d_torch["fused-train"] == 0
    assert d_train["bwd"] == n_calls and d_train["torch"] == 0 and d_train["fused"] == 0, d_train
    assert d_train["fused-train"] == 2 * n_calls                 # training mode runs every layer under checkpoint: forward twice
    scale = float(want.abs().max())
    e = float((got - want).abs().max())
    print(f"Backbone [{dev.type}] fused-train, checkpoint={checkpoint}: flat gradient differs by {e:.3e} = {e / scale:.2e} x its largest entry")
    assert e <= 1e-5 * scale


@pytest.mark.parametrize("checkpoint", [True, False])
def test_backbone_trains_cpu(checkpoint):
    _check_backbone_trains(CPU, checkpoint)


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint", [True, False])
def test_backbone_trains_gpu(gpu, checkpoint):
    _check_backbone_trains(gpu, checkpoint)


def _block_grads(dev, route):
    m, fx = common.make_backbone("backbone_small", dev, route)
    blk = m.encoderLayers[0]
    lin = fx["layer_in"].to(dev).clone().requires_grad_()
    before = _counts()
    blk(lin).square().sum().backward()
    assert all(p.grad is not None for p in blk.parameters())
    return torch.cat([lin.grad.flatten()] + [p.grad.flatten() for p in blk.parameters()]).cpu(), _delta(before), len(blk.attention_modules())


def _check_block_trains(dev):
    want, _, n_calls = _block_grads(dev, "torch")
    got, delta, _ = _block_grads(dev, "fused-train")
    assert delta == {"fused": 0, "fused-train": n_calls, "torch": 0, "bwd": n_calls}, delta
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_basic_block_trains_cpu():
    _check_block_trains(CPU)


@pytest.mark.gpu
def test_basic_block_trains_gpu(gpu):
    _check_block_trains(gpu)


def test_basic_block_trains_without_a_transposed_copy():
    """A BasicBlock(enabled = ["F", "T"]) forward + backward under "fused-train" copies no hidden-state-sized tensor: no clone /
    contiguous / _to_copy / copy_ of one, in the forward or in the backward.  The torch route, counted the same way, does."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m, fx = common.make_backbone("backbone_d40", CPU, "fused-train")
    blk = m.encoderLayers[0]
    assert sorted(blk.enabled) == ["F", "T"]
    n_hidden = fx["layer_in"].numel()

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
    for route in ("fused-train", "torch"):
        blk.attention = route
        blk.zero_grad()
        lin = fx["layer_in"].clone().requires_grad_()
        before = _counts()
        with Count() as c:
            blk(lin).square().sum().backward()
        counts[route] = c.copies
        assert lin.grad is not None and _delta(before)["bwd"] == (2 if route == "fused-train" else 0)
    assert counts["fused-train"] == [], counts["fused-train"]
    assert len(counts["torch"]) > 0                              # the counter sees the stock route's copies
