"""The backward of the bf16 axial attention and the bf16 training route built on it: torch.ops.semicrf.axial_attention_bf16_bwd
(csrc/attention_bf16_bwd.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on CPU tensors),
backbone.axial_attention(route="fused-train", bf16="fused", bf16_train="fused") and the modules under attentionBf16Train = "fused".

  1. every instantiation of the kernel, aligned and misaligned;  2. the query side;  3. tile edges, cross lengths, head sizes, huge and
  negative logits, the largest shape, co-resident workgroups, head counts;  4. exact answers, bit for bit;  5. the contract (both axes
  of one buffer, stride 0, independence, NULL gradients, poison, rejected calls, the token-stride limit);  6. the route;  7. the modules.

The kernel is instantiated on <NKT = ceil(Lk / 32), KS = ceil(d / 16)> (the output blocks DB = 1 for KS <= 2, else 2); the query count
is a run-time value.  In the matrix of section 1, Lk = 1, 32 launch NKT = 1; 33, 64 NKT = 2; 65, 96 NKT = 3; 97, 128 NKT = 4; 129, 160
NKT = 5; 161, 192 NKT = 6; 193, 224 NKT = 7; 225, 256 NKT = 8; d = 8, 16 launch KS = 1; 24, 32 KS = 2; 40, 48 KS = 3; 56, 64 KS = 4 --
all 32 instantiations, each at both edges of its key tile and at both of its head dimensions.

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  Yardsticks and gates: backbone_bf16_bwd_common.
Measured numbers: DESIGN.md section 3, "Backbone attention, bf16 training", and profiles/attention_bf16_bwd_bench.json."""
import ctypes

import pytest
import torch

import backbone_common as common
import backbone_bf16_common as c16
import backbone_bf16_bwd_common as b16

CPU = torch.device("cpu")
BF16 = torch.bfloat16
QKVG = ("q", "k", "v", "dout")


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------------
def _instantiation(dev, d, Lk):
    """<NKT, KS> through the raw op: gated on aligned tensors; with all seven tensors one bf16 element off 16 bytes (odd token
    strides: 2-byte loads and stores), the aligned call's bits."""
    c = b16.case(common.MATRIX_LQ, Lk, common.MATRIX_H, d, (3,), 1.0)
    want = b16.raw_case(dev, c)
    b16.check_gate(dev, c, f"<NKT={(Lk + 31) // 32}, KS={(d + 15) // 16}> Lq={common.MATRIX_LQ} Lk={Lk} d={d}",
                   [g.reshape(t.shape) for g, t in zip(want, c["truth_g"])])
    got = b16.raw_case(dev, c, off=True)
    for name, a, b in zip(b16.NAMES, got, want):
        assert a.data_ptr() % 16 == 2
        assert c16.bits_equal(a, b), (name, d, Lk)


@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bf16_bwd_every_instantiation_cpu(d, Lk):
    _instantiation(CPU, d, Lk)


@pytest.mark.gpu
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bf16_bwd_every_instantiation_gpu(gpu, d, Lk):
    _instantiation(gpu, d, Lk)


# ---- 2. the query side ------------------------------------------------------------------------------------------------------------------
def _query_side(dev, Lq, Lk, d):
    b16.check_gate(dev, b16.case(Lq, Lk, 2, d, (3,), 1.0), f"query side Lq={Lq} Lk={Lk} H=2 d={d}")


@pytest.mark.parametrize("Lq,Lk,d", b16.QUERY_SIDE)
def test_bf16_bwd_query_side_cpu(Lq, Lk, d):
    _query_side(CPU, Lq, Lk, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,d", b16.QUERY_SIDE)
def test_bf16_bwd_query_side_gpu(gpu, Lq, Lk, d):
    _query_side(gpu, Lq, Lk, d)


# ---- 3. other shapes ---------------------------------------------------------------------------------------------------------------------
def _edge(dev, L, scale):
    b16.check_gate(dev, b16.case(L, L, 4, 40, (3,), scale), f"L={L} H=4 d=40 scale={scale:g}")


@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_bf16_bwd_tile_edges_cpu(L, scale):
    _edge(CPU, L, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
@pytest.mark.parametrize("L", common.EDGE_L)
def test_bf16_bwd_tile_edges_gpu(gpu, L, scale):
    _edge(gpu, L, scale)


def _cross(dev, Lq, Lk):
    b16.check_gate(dev, b16.case(Lq, Lk, 4, 40, (3,), 1.0), f"Lq={Lq} Lk={Lk} H=4 d=40")


@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bf16_bwd_cross_lengths_cpu(Lq, Lk):
    _cross(CPU, Lq, Lk)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bf16_bwd_cross_lengths_gpu(gpu, Lq, Lk):
    _cross(gpu, Lq, Lk)


def _heads(dev, L, H, d):
    b16.check_gate(dev, b16.case(L, L, H, d, (3,), 1.0), f"L={L} H={H} d={d}")


@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_bf16_bwd_head_sizes_cpu(L, H, d):
    _heads(CPU, L, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("L,H,d", common.HEAD_CASES)
def test_bf16_bwd_head_sizes_gpu(gpu, L, H, d):
    _heads(gpu, L, H, d)


def _kinds(dev, Lq, Lk, H, d, kind):
    c = b16.case(Lq, Lk, H, d, (3,), 1.0, kind)
    assert c["logit_max"] > 1000.0 if kind == "huge" else c["logit_max"] <= -50.0
    b16.check_gate(dev, c, f"{kind} Lq={Lq} Lk={Lk} H={H} d={d}")


@pytest.mark.parametrize("Lq,Lk,H,d,kind", c16.KINDS)
def test_bf16_bwd_huge_and_negative_logits_cpu(Lq, Lk, H, d, kind):
    _kinds(CPU, Lq, Lk, H, d, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d,kind", c16.KINDS)
def test_bf16_bwd_huge_and_negative_logits_gpu(gpu, Lq, Lk, H, d, kind):
    _kinds(gpu, Lq, Lk, H, d, kind)


def _largest(dev):
    Lq, Lk, H, d, lead = common.LARGEST
    b16.check_gate(dev, b16.case(Lq, Lk, H, d, lead, 1.0), f"largest Lq={Lq} Lk={Lk} H={H} d={d}")


def test_bf16_bwd_largest_configuration_cpu():
    _largest(CPU)


@pytest.mark.gpu
def test_bf16_bwd_largest_configuration_gpu(gpu):
    _largest(gpu)


def _coresident(dev):
    """More workgroups than fit the device at once: 70 sequences x 8 heads at L = 149, d = 64.  Sequence 0 alone gives the bits of its
    slice."""
    Lq, Lk, H, d, lead = common.CORESIDENT
    c = b16.case(Lq, Lk, H, d, lead, 1.0)
    q, k, v, g = (c[n].to(dev) for n in QKVG)
    full = b16.fused_grads(q, k, v, g, H)
    b16.check_gate(dev, c, f"co-resident {lead} x H={H} L={Lq} d={d}", full[1:])
    alone = b16.fused_grads(q[:1, :1], k[:1, :1], v[:1, :1], g[:1, :1], H)
    for name, a, b in zip(("out",) + b16.NAMES, alone, full):
        assert c16.bits_equal(a, b[:1, :1]), name


def test_bf16_bwd_coresident_workgroups_cpu():
    _coresident(CPU)


@pytest.mark.gpu
def test_bf16_bwd_coresident_workgroups_gpu(gpu):
    _coresident(gpu)


def _head_counts(dev, Lq, Lk, H, d):
    b16.check_gate(dev, b16.case(Lq, Lk, H, d, (3,), 1.0), f"head counts Lq={Lq} Lk={Lk} H={H} d={d}")


@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_bf16_bwd_head_counts_cpu(Lq, Lk, H, d):
    _head_counts(CPU, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_bf16_bwd_head_counts_gpu(gpu, Lq, Lk, H, d):
    _head_counts(gpu, Lq, Lk, H, d)


# ---- 4. exact answers --------------------------------------------------------------------------------------------------------------------
def _raw(dev, c, H):
    return b16.raw_bwd(*(b16.as4(c[n]).to(dev) for n in QKVG), H)


def _one_hot(dev, Lq, Lk, H, d):
    """P exactly one-hot: dq and dk are zeros, dv_j is the exact integer sum of dout over the queries that selected j -- the query and
    key permutation of the register hand-off in the dv product."""
    c = b16.one_hot_bwd_case(Lq, Lk, H, d)
    dq, dk, dv = _raw(dev, c, H)
    assert b16.all_zero(dq) and b16.all_zero(dk)
    assert c16.bits_equal(dv.cpu().reshape(c["dv"].shape), c["dv"])


@pytest.mark.parametrize("Lq,Lk,H,d", b16.EXACT_SHAPES)
def test_bf16_bwd_one_hot_weights_cpu(Lq, Lk, H, d):
    _one_hot(CPU, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", b16.EXACT_SHAPES)
def test_bf16_bwd_one_hot_weights_gpu(gpu, Lq, Lk, H, d):
    _one_hot(gpu, Lq, Lk, H, d)


def _uniform(dev, Lq, Lk, H, d):
    """P = 1 / Lk: dv_j = bf16(bf16(1 / Lk) * sum_i dout_i) for every Lk; with V constant over the keys and Lk a power of two, dq and
    dk are exactly zero."""
    c = b16.uniform_bwd_case(Lq, Lk, H, d)
    dv = _raw(dev, c, H)[2]
    assert c16.bits_equal(dv.cpu().reshape(c["dv"].shape), c["dv"])
    if Lk & (Lk - 1) == 0:
        c = b16.uniform_bwd_case(Lq, Lk, H, d, constant_v=True)
        dq, dk, dv = _raw(dev, c, H)
        assert b16.all_zero(dq) and b16.all_zero(dk)
        assert c16.bits_equal(dv.cpu().reshape(c["dv"].shape), c["dv"])


@pytest.mark.parametrize("Lq,Lk,H,d", b16.EXACT_SHAPES)
def test_bf16_bwd_uniform_weights_cpu(Lq, Lk, H, d):
    _uniform(CPU, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", b16.EXACT_SHAPES)
def test_bf16_bwd_uniform_weights_gpu(gpu, Lq, Lk, H, d):
    _uniform(gpu, Lq, Lk, H, d)


# ---- 5. the contract ---------------------------------------------------------------------------------------------------------------------
def _contract(dev):
    Lq, Lk, H, d, lead = common.CONTRACT
    c = b16.case(Lq, Lk, H, d, lead, 1.0)
    return c, H, tuple(c[n].to(dev) for n in QKVG)


def _axis_views(dev):
    """Frequency- and time-axis views of one [N, T', F', H d] buffer; the cotangent as a transposed view: the bits of the contiguous
    call, gradients laid out like their inputs, no copy asked for."""
    N, J, L, H, d = 2, 3, 37, 2, 24
    g = torch.Generator().manual_seed(92)
    q, k, v, go = (torch.randn(N * J, L, H * d, generator=g).bfloat16().to(dev) for _ in range(4))
    want = b16.fused_grads(q, k, v, go, H)

    def time_axis(x):                                            # buffer [N, L, J, HD]; its view [N, J, L, HD]
        return x.view(N, J, L, H * d).transpose(1, 2).contiguous().transpose(1, 2)
    got = b16.fused_grads(time_axis(q), time_axis(k), time_axis(v), time_axis(go), H)
    for name, a, b in zip(("out",) + b16.NAMES, got, want):
        assert a.shape == (N, J, L, H * d) and a.transpose(1, 2).is_contiguous(), name      # transposes back into a contiguous tensor
        assert c16.bits_equal(a.reshape(N * J, L, H * d), b), name
    got = b16.fused_grads(q.view(N, J, L, -1), k.view(N, J, L, -1), v.view(N, J, L, -1), time_axis(go), H)
    for name, a, b in zip(("out",) + b16.NAMES, got, want):
        assert a.is_contiguous() and c16.bits_equal(a.reshape(N * J, L, H * d), b), name
    # the raw op writing the gradients into strided views of larger buffers
    q4, k4, v4, g4 = (x.view(N, J, L, H * d) for x in (q, k, v, go))
    bigs = [torch.full((N, L + 2, J + 1, H * d + 8), -7.0, dtype=BF16, device=dev) for _ in range(3)]
    views = [b[:, 1:L + 1, :J, 8:].transpose(1, 2) for b in bigs]
    b16.raw_bwd(q4, k4, v4, time_axis(go), H, *views)
    for name, a, b in zip(b16.NAMES, views, want[1:]):
        assert c16.bits_equal(a.reshape(N * J, L, H * d), b), name


def test_bf16_bwd_axis_views_cpu():
    _axis_views(CPU)


@pytest.mark.gpu
def test_bf16_bwd_axis_views_gpu(gpu):
    _axis_views(gpu)


def _stride_zero(dev):
    """k and v, then q, expanded over the sequences (stride 0): the bits of their contiguous copies, full-size gradients."""
    c, H, (q, k, v, g) = _contract(dev)
    q4, g4 = b16.as4(q), b16.as4(g)
    k4, v4 = k[:1].expand(3, -1, -1).unsqueeze(1), v[:1].expand(3, -1, -1).unsqueeze(1)
    assert k4.stride(0) == 0 and v4.stride(0) == 0
    want = b16.raw_bwd(q4, k4.contiguous(), v4.contiguous(), g4, H)
    got = b16.raw_bwd(q4, k4, v4, g4, H)
    for name, a, b in zip(b16.NAMES, got, want):
        assert a.shape == b.shape and c16.bits_equal(a, b), name
    q0 = q[:1].expand(3, -1, -1).unsqueeze(1)
    assert q0.stride(0) == 0
    k4, v4 = b16.as4(k), b16.as4(v)
    want = b16.raw_bwd(q0.contiguous(), k4, v4, g4, H)
    got = b16.raw_bwd(q0, k4, v4, g4, H, dq=torch.empty_like(want[0]))
    for name, a, b in zip(b16.NAMES, got, want):
        assert c16.bits_equal(a, b), name
    # through the route: autograd sums the expanded input's gradient, as on the stock route
    from transkun_amd import backbone
    kk = k[:1].clone().requires_grad_()
    before = b16.train_counts()
    backbone.axial_attention(q, kk.expand(3, -1, -1), v, H, **b16.KNOBS).backward(g)
    assert b16.moved(before)[0] == {"fused": 1, "bwd": 1}
    assert kk.grad.shape == (1,) + k.shape[1:] and kk.grad.dtype == BF16 and bool(torch.isfinite(kk.grad).all())


def test_bf16_bwd_stride_zero_cpu():
    _stride_zero(CPU)


@pytest.mark.gpu
def test_bf16_bwd_stride_zero_gpu(gpu):
    _stride_zero(gpu)


def _independence(dev):
    """Sequence 0 alone, as sequence 0 of 70 and as sequence 69 of 70, and as a 7 x 10 grid: the same bits; two runs: the same bits."""
    c = b16.case(89, 89, 4, 40, (7, 10), 1.0)
    q, k, v, g = (c[n].to(dev).reshape(70, 89, 160) for n in QKVG)
    full = b16.fused_grads(q, k, v, g, 4)
    again = b16.fused_grads(q, k, v, g, 4)
    alone = b16.fused_grads(q[:1], k[:1], v[:1], g[:1], 4)
    moved = b16.fused_grads(*(torch.cat([t[1:], t[:1]]) for t in (q, k, v, g)), 4)
    grid = b16.fused_grads(*(t.view(7, 10, 89, 160) for t in (q, k, v, g)), 4)
    for name, f, a, one, m, gr in zip(("out",) + b16.NAMES, full, again, alone, moved, grid):
        assert c16.bits_equal(f, a), name
        assert c16.bits_equal(one, f[:1]), name
        assert c16.bits_equal(m[69:], one) and c16.bits_equal(m[:69], f[1:]), name
        assert c16.bits_equal(gr.reshape(70, 89, 160), f), name


def test_bf16_bwd_independence_cpu():
    _independence(CPU)


@pytest.mark.gpu
def test_bf16_bwd_independence_gpu(gpu):
    _independence(gpu)


def _null_gradients(dev):
    """dq / dk / dv None one at a time and in pairs: the others keep their bits."""
    c, H, (q, k, v, g) = _contract(dev)
    q4, k4, v4, g4 = (b16.as4(t) for t in (q, k, v, g))
    want = b16.raw_bwd(q4, k4, v4, g4, H)
    for flags in ((None, True, True), (True, None, True), (True, True, None), (True, None, None), (None, True, None), (None, None, True)):
        got = b16.raw_bwd(q4, k4, v4, g4, H, *flags)
        for i, name in enumerate(b16.NAMES):
            if flags[i] is None:
                assert got[i] is None
            else:
                assert c16.bits_equal(got[i], want[i]), (name, flags)
    b16.raw_bwd(q4, k4, v4, g4, H, None, None, None)             # nothing wanted: nothing to do


def test_bf16_bwd_null_gradients_cpu():
    _null_gradients(CPU)


@pytest.mark.gpu
def test_bf16_bwd_null_gradients_gpu(gpu):
    _null_gradients(gpu)


def _poison(dev):
    """q, k, v, dout are views into NaN-filled buffers, with NaN behind every row past Lq / Lk and behind d; the gradients are views into
    sentinel-filled buffers.  The results are finite and gated, every sentinel is untouched."""
    S, Lq, Lk, H, d = 5, 35, 33, 4, 40
    c = b16.case(Lq, Lk, H, d, (S,), 1.0)
    HD = H * d

    def inside(x, fill):
        L = x.shape[1]
        big = torch.full((S + 2, L + 7, HD + 16), fill, dtype=BF16)
        big[1:S + 1, 2:L + 2, 8:8 + HD] = x
        big = big.to(dev)
        return big, big[1:S + 1, 2:L + 2, 8:8 + HD].unsqueeze(0)
    nan = float("nan")
    (_, q4), (_, k4), (_, v4), (_, g4) = (inside(c[n], nan) for n in QKVG)
    SENT = -12288.0                                               # a bf16 value
    outs = [inside(torch.full((S, L, HD), SENT, dtype=BF16), SENT) for L in (Lq, Lk, Lk)]
    b16.raw_bwd(q4, k4, v4, g4, H, *(view for _, view in outs))
    b16.check_gate(dev, c, "poison", [view[0] for _, view in outs])
    for (big, _), L in zip(outs, (Lq, Lk, Lk)):
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[1:S + 1, 2:L + 2, 8:8 + HD] = False
        assert bool((big[mask] == SENT).all())                   # every sentinel outside the view is untouched


def test_bf16_bwd_poison_cpu():
    _poison(CPU)


@pytest.mark.gpu
def test_bf16_bwd_poison_gpu(gpu):
    _poison(gpu)


def _direct(lib, ptrs, n0, n1, Lq, Lk, H, d, strides, stream=None):
    return lib.semicrf_axial_attention_bf16_bwd(*ptrs, n0, n1, Lq, Lk, H, d, *strides, stream)


def _einval_cases(ptrs, st):
    """(pointers, the arguments behind them, word of the message) of every SEMICRF_EINVAL case; ptrs: q, k, v, dout, dq, dk, dv."""
    ptrs = list(ptrs)
    cases = [(ptrs, (1, 1, Lq, Lk, H, d, st), b"supported")
             for Lq, Lk, H, d in ((257, 8, 1, 8), (8, 300, 1, 8), (8, 8, 1, 12), (8, 8, 0, 8), (8, 8, 1, 72), (0, 8, 1, 8))]
    for i in range(4):                                           # q, k, v, dout must be there
        bad = list(ptrs); bad[i] = None
        cases.append((bad, (1, 1, 8, 8, 1, 8, st), b"NULL"))
    for i in range(7):                                           # an odd pointer, one tensor at a time
        bad = list(ptrs); bad[i] = ctypes.c_void_p(bad[i].value + 1)
        cases.append((bad, (1, 1, 8, 8, 1, 8, st), b"aligned"))
    cases.append((ptrs, (-1, 1, 8, 8, 1, 8, st), b">= 0"))
    cases.append((ptrs, (1 << 20, 1 << 12, 8, 8, 1, 8, st), b"2^31"))
    for i in (0, 5, 10, 13, 20):
        bad = list(st); bad[i] = -st[i] - 1
        cases.append((ptrs, (1, 1, 8, 8, 1, 8, bad), b"negative"))
    for i in range(2, 21, 3):                                    # a token stride AT the limit, one tensor at a time
        bad = list(st); bad[i] = common.TOKEN_STRIDE_LIMIT
        cases.append((ptrs, (1, 1, 8, 8, 1, 8, bad), b"2^28"))
    return cases


def test_bf16_bwd_c_entry_point_rejects_cpu():
    """Every EINVAL case returns nonzero with its message before any pointer is used (the pointers here are never valid); the supported
    set is the forward's over a grid; the torch op checks the same set, the shapes, the dtype and the layouts."""
    from transkun_amd import _lib, backbone
    lib = _lib.load()
    assert "semicrf_axial_attention_bf16_bwd" in _lib.EXPORTED and "semicrf_axial_attention_bf16_bwd_supported" in _lib.EXPORTED
    assert lib.semicrf_abi_version() == 2
    fake = [ctypes.c_void_p(4096 + 512 * i) for i in range(7)]
    st = [1000, 100, 96] * 7
    for ptrs, args, word in _einval_cases(fake, st):
        assert _direct(lib, ptrs, *args) == 1, (args[:6], word)
        assert word in lib.semicrf_last_error(), (word, lib.semicrf_last_error())
    assert _direct(lib, fake, 0, 5, 8, 8, 1, 8, st) == 0         # no sequences: nothing to do, nothing launched
    for Lq in (-1, 0, 1, 33, 256, 257):
        for Lk in (0, 1, 149, 256, 257):
            for H in (-1, 0, 1, 4, 1000):
                for d in (0, 4, 8, 12, 40, 64, 65, 72):
                    want = lib.semicrf_axial_attention_bf16_supported(Lq, Lk, H, d)
                    assert lib.semicrf_axial_attention_bf16_bwd_supported(Lq, Lk, H, d) == want, (Lq, Lk, H, d)
                    assert backbone.attention_bf16_bwd_supported(Lq, Lk, H, d) == bool(want)
    ops = _lib.ops()
    x = torch.zeros(1, 1, 4, 12, dtype=BF16)
    with pytest.raises(RuntimeError, match="support"):
        ops.axial_attention_bf16_bwd(x, x, x, x, torch.empty_like(x), None, None, 1)
    y = torch.zeros(1, 1, 4, 16, dtype=BF16)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bf16_bwd(y, y, y, y, torch.empty(1, 1, 5, 16, dtype=BF16), None, None, 2)
    for bad in ((y.float(), y, y, y, y), (y, y.float(), y, y, y), (y, y, y.float(), y, y), (y, y, y, y.float(), y), (y, y, y, y, y.float())):
        with pytest.raises(RuntimeError, match="bfloat16"):
            ops.axial_attention_bf16_bwd(bad[0], bad[1], bad[2], bad[3], None, None, torch.empty_like(bad[4]), 2)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bf16_bwd(y.transpose(-1, -2), y, y, y, torch.empty_like(y), None, None, 2)
    with pytest.raises(RuntimeError, match="repeat"):
        ops.axial_attention_bf16_bwd(y, y, y, y, torch.empty(1, 1, 1, 16, dtype=BF16).expand(1, 1, 4, 16), None, None, 2)
    with pytest.raises(RuntimeError, match="repeat"):
        ops.axial_attention_bf16_bwd(y, y, y, torch.empty(1, 1, 1, 16, dtype=BF16).expand(1, 1, 4, 16), torch.empty_like(y), None, None, 2)


@pytest.mark.gpu
def test_bf16_bwd_c_entry_point_leaves_gradients_untouched_gpu(gpu):
    """The same EINVAL cases on real tensors: sentinel-filled gradients keep every bit, and the valid call of the same arguments runs."""
    from transkun_amd import _lib
    lib = _lib.load()
    x = torch.randn(3, 8, 16, device=gpu).bfloat16()
    go = torch.randn(3, 8, 16, device=gpu).bfloat16()
    grads = [torch.full((3, 8, 16), 3.0, dtype=BF16, device=gpu) for _ in range(3)]
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in (x, x, x, go, *grads)]
    st = [0, 16, 16] * 3 + [0, 128, 16] * 4
    stream = _lib.stream_of(x)
    for bad, args, word in _einval_cases(ptrs, st):
        assert _direct(lib, bad, *args, stream) == 1, (args[:6], word)
        assert word in lib.semicrf_last_error(), word
    torch.cuda.synchronize(gpu)
    assert all(bool((g == 3.0).all()) for g in grads)
    assert _direct(lib, ptrs, 1, 1, 8, 8, 1, 8, st, stream) == 0
    torch.cuda.synchronize(gpu)
    xs = x[:1, :, :8].contiguous()
    want = b16.raw_bwd(*(b16.as4(t) for t in (xs, xs, xs, go[:1, :, :8].contiguous())), 1)
    for g, w in zip(grads, want):
        assert c16.bits_equal(g[:1, :, :8].contiguous(), w[0]) and bool((g[1:] == 3.0).all()) and bool((g[:1, :, 8:] == 3.0).all())


@pytest.mark.gpu
def test_bf16_bwd_token_stride_beyond_the_limit_gpu(gpu):
    """A q whose two tokens lie 2^28 elements apart (512 MiB of bf16, of which two rows are written): the op turns it down, and the
    route, all three knobs set and a gradient wanted, answers by the stock route bit for bit."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    g = torch.Generator().manual_seed(2830)
    q, k, v = (torch.randn(1, L, 48, generator=g).bfloat16().to(gpu) for L in (2, 5, 5))
    buf = torch.empty(lim + 64, dtype=BF16, device=gpu)
    far = buf.as_strided((1, 2, 48), (2 * lim, lim, 1))
    far.copy_(q)
    with pytest.raises(RuntimeError, match=r"2\^28"):
        b16.raw_bwd(far.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), q.unsqueeze(0), 2)
    go = torch.randn(1, 2, 48, generator=g).bfloat16().to(gpu)
    res = []
    for fn in (lambda kk: backbone.axial_attention(far, kk, v, 2, **b16.KNOBS), lambda kk: backbone.attention_torch(far, kk, v, 2)):
        kk = k.clone().requires_grad_()
        before = b16.train_counts()
        out = fn(kk)
        out.backward(go)
        res.append((out.detach(), kk.grad, b16.moved(before)))
    assert res[0][2] == ({"torch": 1}, {"torch": 1}, {"torch": 1}) and res[1][2] == ({}, {}, {})
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    del far, buf
    torch.cuda.empty_cache()


def test_bf16_bwd_token_stride_limit_routes_to_stock():
    """What keeps such views from the device op is read from the views themselves (meta tensors), dout's included."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    buf = torch.empty(2 * lim + 64, dtype=BF16, device="meta")
    ok = torch.empty(1, 5, 48, dtype=BF16, device="meta")
    for stride, L, fits in ((lim, 2, False), (lim - 8, 2, True), (lim, 1, True)):
        view = buf.as_strided((1, L, 48), (0, stride, 1))
        assert backbone._token_strides_fit(view, ok, ok) == fits and backbone._token_strides_fit(view) == fits


# ---- 6. the route -------------------------------------------------------------------------------------------------------------------------
def _route(dev):
    from transkun_amd import backbone
    assert backbone.BF16_TRAIN_KINDS == ("torch", "fused") and backbone.DEFAULT_ATTENTION_BF16_TRAIN == "torch"
    assert set(backbone.ATTENTION_BF16_TRAIN_ROUTES) == {"fused", "torch", "bwd"}
    assert backbone.BF16_KINDS == ("torch", "fused") and set(backbone.ATTENTION_BF16_ROUTES) == {"fused", "torch"}
    assert set(backbone.ATTENTION_ROUTES) == {"fused", "fused-train", "torch", "bwd"}
    c, H, (q, k, v, g) = _contract(dev)
    # guards: without the new keyword, bf16 under autograd is the stock route under both fused routes, output and gradients
    want = b16.route_grads(q, k, v, g, H, route="torch", bf16="torch", bf16_train="torch")
    for route in ("fused", "fused-train"):
        before = b16.train_counts()
        ins = [t.clone().requires_grad_() for t in (q, k, v)]
        out = backbone.axial_attention(*ins, H, route=route, bf16="fused")
        out.backward(g)
        assert b16.moved(before) == ({}, {"torch": 1}, {"torch": 1})
        for a, b in zip((out.detach(), *(t.grad for t in ins)), want):
            assert torch.equal(a, b), route
    # all three knobs and a gradient wanted: the Function answers, once
    with torch.no_grad():
        fwd = backbone.axial_attention(q, k, v, H, bf16="fused")
    got = b16.fused_grads(q, k, v, g, H)                          # (asserts the counters)
    assert c16.bits_equal(got[0], fwd)
    for a, t in zip(got[1:], (q, k, v)):
        assert a.dtype == BF16 and a.shape == t.shape and a.stride() == t.stride() and a.device == t.device
    b16.check_gate(dev, c, "route, all three knobs", got[1:])
    # an input that needs no gradient gets None, the others keep their bits
    for skip in range(3):
        needs = tuple(i != skip for i in range(3))
        part = b16.fused_grads(q, k, v, g, H, needs)
        for i in range(3):
            assert (part[1 + i] is None) if i == skip else c16.bits_equal(part[1 + i], got[1 + i])
    # no gradient wanted: the forward op's bits, the training counters at rest
    before = b16.train_counts()
    with torch.no_grad():
        a = backbone.axial_attention(q.clone().requires_grad_(), k, v, H, **b16.KNOBS)
    plain = backbone.axial_attention(q, k, v, H, **b16.KNOBS)
    assert b16.moved(before) == ({}, {"fused": 2}, {"fused": 2})
    assert not a.requires_grad and c16.bits_equal(a, fwd) and c16.bits_equal(plain, fwd)
    # one knob missing, outside the supported set, broadcasting keys: the stock route's output and gradients
    gen = torch.Generator().manual_seed(79)
    rnd = lambda *s: torch.randn(*s, generator=gen).bfloat16().to(dev)
    cases = {"route torch": ((q, k, v, H), dict(route="torch")),
             "route fused": ((q, k, v, H), dict(route="fused")),
             "bf16 torch": ((q, k, v, H), dict(bf16="torch")),
             "L > 256": ((rnd(2, 300, 32), rnd(2, 300, 32), rnd(2, 300, 32), 2), {}),
             "d = 12": ((rnd(2, 9, 24), rnd(2, 9, 24), rnd(2, 9, 24), 2), {}),
             "broadcast keys": ((rnd(4, 3, 9, 32), rnd(1, 3, 7, 32), rnd(1, 3, 7, 32), 2), {})}
    for tag, ((q_, k_, v_, H_), kw) in cases.items():
        go = torch.randn(q_.shape, generator=gen).bfloat16().to(dev)
        before = b16.train_counts()
        got_ = b16.route_grads(q_, k_, v_, go, H_, **kw)
        m = b16.moved(before)
        assert m[0] == {"torch": 1} and m[1] == {"torch": 1}, (tag, m)
        want_ = b16.route_grads(q_, k_, v_, go, H_, route="torch", bf16="torch", bf16_train="torch")
        for a, b in zip(got_, want_):
            assert a.dtype == BF16 and torch.equal(a, b), tag
    # float32 tensors are what they were, and are not counted
    before = b16.train_counts()
    qf = q.float().requires_grad_()
    backbone.axial_attention(qf, k.float(), v.float(), H, **b16.KNOBS).backward(g.float())
    m = b16.moved(before)
    assert m[0] == {} and m[1] == {"fused-train": 1, "bwd": 1} and m[2] == {} and qf.grad.dtype == torch.float32


def test_bf16_bwd_route_cpu():
    _route(CPU)


@pytest.mark.gpu
def test_bf16_bwd_route_gpu(gpu):
    _route(gpu)


def test_bf16_bwd_route_second_derivative_raises():
    from transkun_amd import backbone
    c, H, (q, k, v, g) = _contract(CPU)
    q, g = q.clone().requires_grad_(), g.clone().requires_grad_()
    out = backbone.axial_attention(q, k, v, H, **b16.KNOBS)
    (dq,) = torch.autograd.grad(out, q, g, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        dq.float().sum().backward()


def test_bf16_bwd_names_are_checked():
    from transkun_amd import backbone
    x = torch.zeros(1, 4, 16, dtype=BF16)
    with pytest.raises(ValueError):
        backbone.axial_attention(x, x, x, 2, bf16_train="eager")
    with pytest.raises(ValueError):
        backbone.axial_attention(x.float(), x.float(), x.float(), 2, bf16_train="train")
    m, _ = common.make_backbone("backbone_small", CPU, "fused-train")
    assert m.attentionBf16Train == "torch" and all(layer.attentionBf16Train == "torch" for layer in m.encoderLayers)
    m.attentionBf16Train = "fused"
    assert m.attentionBf16Train == "fused" and all(layer.attentionBf16Train == "fused" for layer in m.encoderLayers)
    assert all(a.attentionBf16Train == "fused" for a in m.modules() if isinstance(a, backbone.MultiHeadAttentionKernel))
    m.encoderLayers[0].attentionBf16Train = "torch"
    assert m.attentionBf16Train == "mixed" and m.encoderLayers[0].attentionBf16Train == "torch"
    with pytest.raises(ValueError):
        m.attentionBf16Train = "eager"
    with pytest.raises(ValueError):
        m.encoderLayers[0].attentionBf16Train = "eager"


# ---- 7. the modules ------------------------------------------------------------------------------------------------------------------------
def _module_grads(m, dev, x, idx, fused, autocast):
    """The flat gradient of sum(out^2) under the new route (fused) or the stock bf16 route, and the training counters' movement."""
    import contextlib
    b16.set_knobs(m, fused)
    m.zero_grad(set_to_none=True)
    before = b16.train_counts()
    ctx = torch.autocast(device_type=dev.type, dtype=BF16) if autocast else contextlib.nullcontext()
    with ctx:
        out = m(x, idx)
    out.float().square().sum().backward()
    return b16.flat_grad(m), b16.moved(before)


def _backbone_trains(dev, checkpoint, autocast):
    """backbone_small in training mode, bf16 weights (or fp32 weights under bf16 autocast): every parameter gets a gradient under the new
    route, every attention call's backward launches the op once, and the flat gradient's error against the float64 module's is at
    most GATE x that of the stock bf16 route against the same truth."""
    import copy
    from transkun_amd import backbone
    m, fx = b16.training_backbone("backbone_small", checkpoint)
    if not autocast:
        m = m.to(BF16)
    m64 = copy.deepcopy(m).double()
    m64.attention = "torch"
    x, idx = fx["x"], fx["outputIndices"]
    x = x if autocast else x.bfloat16()
    m64(x.double(), idx).square().sum().backward()
    truth = b16.flat_grad(m64)
    m = m.to(dev)
    n_calls = sum(isinstance(a, backbone.MultiHeadAttentionKernel) for a in m.modules())
    stock, d_stock = _module_grads(m, dev, x.to(dev), idx.to(dev), False, autocast)
    got, d_fused = _module_grads(m, dev, x.to(dev), idx.to(dev), True, autocast)
    assert d_stock[0] == {}, d_stock
    # training mode runs every layer under checkpoint: each forward twice, each backward once
    assert d_fused[0] == {"fused": 2 * n_calls, "bwd": n_calls}, d_fused
    assert d_fused[1] == {"fused-train": 2 * n_calls} and d_fused[2] == {"fused": 2 * n_calls}, d_fused
    e, e16 = float((got - truth).abs().max()), float((stock - truth).abs().max())
    print(f"Backbone [{dev.type}] bf16 training, checkpoint={checkpoint}, autocast={autocast}: flat gradient error {e:.3e}  "
          f"stock bf16 route {e16:.3e}  ratio {e / e16:.2f} (gate {b16.GATE:g})")
    assert bool(torch.isfinite(got).all()) and e <= b16.GATE * e16


@pytest.mark.parametrize("autocast", [False, True], ids=["bf16-weights", "autocast"])
@pytest.mark.parametrize("checkpoint", [True, False])
def test_bf16_backbone_trains_cpu(checkpoint, autocast):
    _backbone_trains(CPU, checkpoint, autocast)


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [False, True], ids=["bf16-weights", "autocast"])
@pytest.mark.parametrize("checkpoint", [True, False])
def test_bf16_backbone_trains_gpu(gpu, checkpoint, autocast):
    _backbone_trains(gpu, checkpoint, autocast)


def test_bf16_basic_block_trains_without_a_transposed_copy():
    """A bf16 BasicBlock(enabled = ["F", "T"]) forward + backward under the new route copies no hidden-state-sized tensor: no clone /
    contiguous / _to_copy / copy_ of one, in the forward or in the backward.  The stock route, counted the same way, does."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m16, _, fx = c16.bf16_backbone("backbone_d40", CPU)
    blk = m16.encoderLayers[0]
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
    for fused in (True, False):
        b16.set_knobs(blk, fused)
        blk.zero_grad()
        lin = fx["layer_in"].bfloat16().requires_grad_()
        before = b16.train_counts()
        with Count() as c:
            blk(lin).square().sum().backward()
        counts[fused] = c.copies
        assert lin.grad is not None and b16.moved(before)[0] == ({"fused": 2, "bwd": 2} if fused else {})
    assert counts[True] == [], counts[True]
    assert len(counts[False]) > 0                                # the counter sees the stock route's copies
