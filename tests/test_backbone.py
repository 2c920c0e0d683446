"""The backbone and its axial attention: transkun_amd.backbone (csrc/attention.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on
CPU tensors) -- the op against float64 at the tile edges and the model's lengths, in every instantiation <key tiles, output blocks,
16- or 4-byte loads> of the kernel and at the limits of its LDS and register budget, its strided contract (stride 0, misalignment,
non-finite values, the token-stride limit), padding, determinism and argument checks, the fall-backs of backbone.axial_attention,
and the modules against the reference's fixtures.

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


# ---- 1b. every instantiation <NKT, DB, VEC> of the kernel, and the limits of its budget -----------------------------------------------
def _gated(got, c, tag):
    """got against the case's float64 truth under the case's own gate; returns error / gate."""
    assert got.shape == c["truth"].shape and got.dtype == torch.float32, tag
    assert bool(torch.isfinite(got).all()), tag
    e = float((got.cpu().double() - c["truth"]).abs().max())
    print(f"axial_attention [{got.device.type}] {tag}: error {e:.3e}  torch fp32 {c['e32']:.3e}  gate {c['gate']:.3e}  "
          f"error/gate {e / c['gate']:.3f}")
    assert e <= c["gate"], (tag, e, c["e32"], c["gate"])
    return e / c["gate"]


def _matrix(dev, d, Lk, aligned):
    """NKT = ceil(Lk / 32), DB = 1 (d <= 32) or 2, VEC = aligned.  The misaligned form (q and k one float off a 16-byte boundary: the
    4-byte loads) is gated like the aligned one and must give its bits."""
    Lq, H = common.MATRIX_LQ, common.MATRIX_H
    for scale in common.SCALES:
        c = common.op_case(Lq, Lk, H, d, (3,), scale)
        q, k, v = (c[n].to(dev) for n in "qkv")
        assert q.data_ptr() % 16 == 0 and k.data_ptr() % 16 == 0 and q.stride(-2) % 4 == 0 and k.stride(-2) % 4 == 0
        tag = f"Lq={Lq} Lk={Lk} H={H} d={d} scale={scale:g} "
        want = common.fused(q, k, v, H)
        if aligned:
            _gated(want, c, tag + "aligned")
        else:
            got = common.fused(common.one_float_off(q), common.one_float_off(k), v, H)
            _gated(got, c, tag + "q, k one float off 16 bytes")
            assert common.bits_equal(got, want), tag + "q, k one float off 16 bytes: not the bits of the aligned call"


def _passes(dev, Lq, Lk, d):
    c = common.op_case(Lq, Lk, 2, d, (3,), 1.0)
    _gated(common.fused(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), 2), c, f"Lq={Lq} Lk={Lk} H=2 d={d} scale=1")


def _largest(dev, scale):
    Lq, Lk, H, d, lead = common.LARGEST
    c = common.op_case(Lq, Lk, H, d, lead, scale)
    _gated(common.fused(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), H), c, f"Lq={Lq} Lk={Lk} H={H} d={d} scale={scale:g}")


def _coresident(dev):
    """70 sequences x 8 heads = 560 workgroups, each with 75 KB of LDS (NKT = 5, d = 64, two per CU): against float64, and sequence 0
    computed alone gives the bits of its slice of the full result."""
    Lq, Lk, H, d, lead = common.CORESIDENT
    c = common.op_case(Lq, Lk, H, d, lead, 1.0)
    q, k, v = (c[n].to(dev) for n in "qkv")
    full = common.fused(q, k, v, H)
    _gated(full, c, f"Lq={Lq} Lk={Lk} H={H} d={d} sequences={lead}")
    alone = common.fused(q[0, :1], k[0, :1], v[0, :1], H)
    assert common.bits_equal(alone, full[0, :1])


def _head_counts(dev, Lq, Lk, H, d):
    c = common.op_case(Lq, Lk, H, d, (3,), 1.0)
    _gated(common.fused(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), H), c, f"Lq={Lq} Lk={Lk} H={H} d={d} scale=1")


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_op_instantiation_matrix_cpu(d, Lk, aligned):
    _matrix(CPU, d, Lk, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_op_instantiation_matrix_gpu(gpu, d, Lk, aligned):
    _matrix(gpu, d, Lk, aligned)


@pytest.mark.parametrize("Lq,Lk,d", common.PASSES)
def test_op_query_passes_cpu(Lq, Lk, d):
    _passes(CPU, Lq, Lk, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,d", common.PASSES)
def test_op_query_passes_gpu(gpu, Lq, Lk, d):
    _passes(gpu, Lq, Lk, d)


@pytest.mark.parametrize("scale", common.SCALES)
def test_op_largest_configuration_cpu(scale):
    _largest(CPU, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
def test_op_largest_configuration_gpu(gpu, scale):
    _largest(gpu, scale)


def test_op_coresident_workgroups_cpu():
    _coresident(CPU)


@pytest.mark.gpu
def test_op_coresident_workgroups_gpu(gpu):
    _coresident(gpu)


@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_op_head_counts_cpu(Lq, Lk, H, d):
    _head_counts(CPU, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_op_head_counts_gpu(gpu, Lq, Lk, H, d):
    _head_counts(gpu, Lq, Lk, H, d)


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


def _contract_case(dev):
    Lq, Lk, H, d, lead = common.CONTRACT
    c = common.op_case(Lq, Lk, H, d, lead, 1.0)
    return c, H, d, tuple(c[n].to(dev) for n in "qkv")


def _check_stride_zero(dev):
    """k and v, then q, expanded over the sequence dimension (stride 0): the bits of their contiguous copies, which pass the gate."""
    c, H, d, (q, k, v) = _contract_case(dev)
    k0, v0 = k[:1].expand(3, -1, -1), v[:1].expand(3, -1, -1)
    assert k0.stride(0) == 0 and v0.stride(0) == 0
    want = common.fused(q, k0.contiguous(), v0.contiguous(), H)
    _gated(want, common.finish_case(c["q"], c["k"][:1].expand(3, -1, -1).contiguous(), c["v"][:1].expand(3, -1, -1).contiguous(), H),
           "k, v of sequence 0 for all sequences")
    assert common.bits_equal(common.fused(q, k0, v0, H), want)
    q0 = q[:1].expand(3, -1, -1)
    assert q0.stride(0) == 0
    got = common.fused(q0, k, v, H)
    assert got.shape == q.shape and got.is_contiguous() and got.device == q.device      # a dense tensor, not a repeated view
    assert common.bits_equal(got, common.fused(q0.contiguous(), k, v, H))
    assert common.bits_equal(got[0], common.fused(q, k, v, H)[0])


def test_stride_zero_cpu():
    _check_stride_zero(CPU)


@pytest.mark.gpu
def test_stride_zero_gpu(gpu):
    _check_stride_zero(gpu)


def _check_alignment_conditions(dev):
    """Each tensor one float off a 16-byte boundary, and an odd token stride from an aligned base, one condition at a time: the bits
    of the aligned call."""
    c, H, d, (q, k, v) = _contract_case(dev)
    S, Lq, Lk, HD = q.shape[0], q.shape[1], k.shape[1], H * d
    want = common.fused(q, k, v, H)
    _gated(want, c, "aligned")
    assert common.bits_equal(common.fused(q, k, common.one_float_off(v), H), want), "v one float off 16 bytes"
    assert common.bits_equal(common.fused(common.one_float_off(q), k, v, H), want), "q one float off 16 bytes"
    assert common.bits_equal(common.fused(q, common.one_float_off(k), v, H), want), "k one float off 16 bytes"
    # the raw op writing into a view one float off 16 bytes
    big = torch.full((S, Lq, HD + 1), -7.0, device=dev)
    o = big[..., 1:]
    assert o.data_ptr() % 16 != 0
    common.raw_op(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), o.unsqueeze(0), H)
    assert common.bits_equal(o, want), "out one float off 16 bytes"
    assert bool((big[..., 0] == -7.0).all())
    # an odd token stride (a parent of width H d + 1) from an aligned base
    for name in "kq":
        x = {"q": q, "k": k}[name]
        parent = torch.zeros(*x.shape[:-1], HD + 1, device=dev)
        parent[..., :HD] = x
        view = parent[..., :HD]
        assert view.data_ptr() % 16 == 0 and view.stride(-2) == HD + 1
        got = common.fused(view, k, v, H) if name == "q" else common.fused(q, view, v, H)
        assert common.bits_equal(got, want), f"{name} with token stride H d + 1"


def test_alignment_conditions_cpu():
    _check_alignment_conditions(CPU)


@pytest.mark.gpu
def test_alignment_conditions_gpu(gpu):
    _check_alignment_conditions(gpu)


def _check_non_finite_stay_put(dev):
    """A NaN in k, a NaN in q and a +inf in v reach the outputs they belong to and no other: everything else keeps the clean run's bits."""
    from transkun_amd import backbone
    c, H, d, (q, k, v) = _contract_case(dev)
    clean = common.fused(q, k, v, H)
    assert bool(torch.isfinite(clean).all())
    head1 = slice(d, 2 * d)
    # k at (sequence 1, key 5, head 1): every query of that sequence and head
    kn = k.clone()
    kn[1, 5, head1] = float("nan")
    got = common.fused(q, kn, v, H)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[1, :, head1] = True
    assert torch.equal(torch.isnan(got), hit), "NaN in k"
    assert bool(common.same_bits_mask(got, clean)[~hit].all()), "NaN in k"
    # q at (sequence 2, query 7, one column of head 0): that row of that head
    qn = q.clone()
    qn[2, 7, 3] = float("nan")
    got = common.fused(qn, k, v, H)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[2, 7, :d] = True
    assert torch.equal(torch.isnan(got), hit), "NaN in q"
    assert bool(common.same_bits_mask(got, clean)[~hit].all()), "NaN in q"
    # one +inf in v: the inf / NaN pattern of the stock fp32 route on identical inputs
    vi = v.clone()
    vi[0, 11, d + 2] = float("inf")
    got = common.fused(q, k, vi, H)
    with torch.no_grad():
        stock = backbone.attention_torch(q, k, vi, H)
    assert not bool(torch.isfinite(stock).all())
    assert torch.equal(torch.isnan(got), torch.isnan(stock)), "+inf in v"
    assert torch.equal(torch.isposinf(got), torch.isposinf(stock)) and torch.equal(torch.isneginf(got), torch.isneginf(stock)), "+inf in v"
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[0, :, d + 2] = True                                       # an output column reads its own column of v only
    assert bool(common.same_bits_mask(got, clean)[~hit].all()), "+inf in v"


def test_non_finite_stay_put_cpu():
    _check_non_finite_stay_put(CPU)


@pytest.mark.gpu
def test_non_finite_stay_put_gpu(gpu):
    _check_non_finite_stay_put(gpu)


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
    for i, name in ((2, "q"), (5, "k"), (8, "v"), (11, "out")):                      # a token stride of 2^28 elements, one tensor at a time
        bad = list(st); bad[i] = common.TOKEN_STRIDE_LIMIT
        assert _direct(lib, fake, fake, fake, fake, 1, 1, 8, 8, 1, 8, bad) == 1, name
        assert b"2^28" in lib.semicrf_last_error(), name
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


def test_token_stride_limit_is_read_from_the_views():
    """Which views backbone.axial_attention keeps from the device op: a token stride of 2^28 elements or more at a length above one
    (meta tensors: no memory behind them)."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    assert backbone.ATTENTION_TOKEN_STRIDE_LIMIT == lim
    buf = torch.empty(2 * lim + 64, device="meta")
    ok = torch.empty(1, 5, 48, device="meta")
    for stride, L, fits in ((lim, 2, False), (lim + 4, 2, False), (lim - 4, 2, True), (lim, 1, True), (2 * lim, 1, True)):
        view = buf.as_strided((1, L, 48), (0, stride, 1))
        for args in ((view, ok, ok), (ok, view, ok), (ok, ok, view)):
            assert backbone._token_strides_fit(*args) == fits, (stride, L)


def _check_token_stride(gpu, which):
    """A view whose two tokens lie 2^28 elements apart (1 GiB, of which only the two rows are ever written): outside the device
    op's reach, so backbone.axial_attention answers by the stock route instead of raising."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    g = torch.Generator().manual_seed(2828)
    Lq, Lk = (2, 5) if which == "q" else (5, 2)
    host = dict(q=torch.randn(1, Lq, 48, generator=g), k=torch.randn(1, Lk, 48, generator=g), v=torch.randn(1, Lk, 48, generator=g))
    c = common.finish_case(host["q"], host["k"], host["v"], 2)
    dev = {n: t.to(gpu) for n, t in host.items()}
    buf = torch.empty(lim + 64, device=gpu)                       # 1 GiB + 256 B, uninitialised
    far = buf.as_strided((1, 2, 48), (2 * lim, lim, 1))
    far.copy_(dev[which])
    assert far.stride(-2) == lim and torch.equal(far, dev[which])
    dev[which] = far
    with pytest.raises(RuntimeError, match=r"2\^28"):             # the op itself turns the view down before it launches anything
        common.raw_op(dev["q"].unsqueeze(0), dev["k"].unsqueeze(0), dev["v"].unsqueeze(0), torch.empty(1, 1, Lq, 48, device=gpu), 2)
    with torch.no_grad():
        got = backbone.axial_attention(dev["q"], dev["k"], dev["v"], 2)
        assert torch.equal(got, backbone.attention_torch(dev["q"], dev["k"], dev["v"], 2))
    _gated(got, c, f"token stride 2^28 of {which}")
    del far, buf, dev
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["q", "v"])
def test_token_stride_beyond_the_limit_gpu(gpu, which):
    _check_token_stride(gpu, which)


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
