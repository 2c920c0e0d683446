"""The bf16 axial attention: torch.ops.semicrf.axial_attention_bf16 (csrc/attention_bf16.hip on the GPU, the host mirror of
csrc/cpu_ops.cpp on CPU tensors) behind backbone.axial_attention(bf16="fused") and the attentionBf16 knob of the modules.

a. accuracy against float64 in every instantiation of the kernel, aligned and misaligned;  b. exact answers, bit for bit against a
closed form (one-hot weights, uniform weights);  c. independence of batch, position, strides and alignment;  d. the memory contract;
e. non-finite values;  f. the C entry point;  g. the route;  h. the modules in bf16 weights and under bf16 autocast.

Every check runs on the CPU path (unmarked) and on the device (marked gpu).  Yardsticks and bounds: backbone_bf16_common.
Measured numbers: DESIGN.md section 3, "Backbone attention, bf16", and profiles/attention_bf16_bench.json."""
import ctypes

import pytest
import torch

import backbone_bf16_common as c16
import backbone_common as common

CPU = torch.device("cpu")
BF16 = torch.bfloat16


def _run(dev, c):
    return c16.fused16(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), c["H"])


# ---- a. the accuracy gate --------------------------------------------------------------------------------------------------------------
def _matrix(dev, d, Lk, aligned):
    """NKT = ceil(Lk / 32), KS = ceil(d / 16).  Misaligned: q, k and v one element off a 16-byte boundary with an odd token stride (the
    2-byte loads), gated like the aligned call and giving its bits."""
    Lq, H = common.MATRIX_LQ, common.MATRIX_H
    for scale in common.SCALES:
        c = c16.case(Lq, Lk, H, d, (3,), scale)
        q, k, v = (c[n].to(dev) for n in "qkv")
        assert all(t.data_ptr() % 16 == 0 and t.stride(-2) % 8 == 0 for t in (q, k, v))
        tag = f"Lq={Lq} Lk={Lk} H={H} d={d} scale={scale:g} "
        want = c16.fused16(q, k, v, H)
        if aligned:
            c16.gated(want, c, tag + "aligned")
        else:
            got = c16.fused16(c16.one_off(q), c16.one_off(k), c16.one_off(v), H)
            c16.gated(got, c, tag + "q, k, v one element off 16 bytes")
            assert c16.bits_equal(got, want), tag + "misaligned: not the bits of the aligned call"


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bf16_instantiation_matrix_cpu(d, Lk, aligned):
    _matrix(CPU, d, Lk, aligned)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
@pytest.mark.parametrize("Lk", common.MATRIX_LK)
@pytest.mark.parametrize("d", common.MATRIX_D)
def test_bf16_instantiation_matrix_gpu(gpu, d, Lk, aligned):
    _matrix(gpu, d, Lk, aligned)


def _edge(dev, L):
    for scale in common.SCALES:
        c = c16.case(L, L, 4, 40, (3,), scale)
        c16.gated(_run(dev, c), c, f"L={L} H=4 d=40 scale={scale:g}")


@pytest.mark.parametrize("L", common.EDGE_L)
def test_bf16_edge_lengths_cpu(L):
    _edge(CPU, L)


@pytest.mark.gpu
@pytest.mark.parametrize("L", common.EDGE_L)
def test_bf16_edge_lengths_gpu(gpu, L):
    _edge(gpu, L)


def _cross(dev, Lq, Lk):
    c = c16.case(Lq, Lk, 4, 40, (3,), 1.0)
    c16.gated(_run(dev, c), c, f"Lq={Lq} Lk={Lk} H=4 d=40")


@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bf16_cross_attention_cpu(Lq, Lk):
    _cross(CPU, Lq, Lk)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk", common.CROSS)
def test_bf16_cross_attention_gpu(gpu, Lq, Lk):
    _cross(gpu, Lq, Lk)


def _passes(dev, Lq, Lk, d):
    c = c16.case(Lq, Lk, 2, d, (3,), 1.0)
    c16.gated(_run(dev, c), c, f"Lq={Lq} Lk={Lk} H=2 d={d}")


@pytest.mark.parametrize("Lq,Lk,d", common.PASSES)
def test_bf16_query_passes_cpu(Lq, Lk, d):
    _passes(CPU, Lq, Lk, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,d", common.PASSES)
def test_bf16_query_passes_gpu(gpu, Lq, Lk, d):
    _passes(gpu, Lq, Lk, d)


def _largest(dev, scale):
    Lq, Lk, H, d, lead = common.LARGEST
    c = c16.case(Lq, Lk, H, d, lead, scale)
    c16.gated(_run(dev, c), c, f"Lq={Lq} Lk={Lk} H={H} d={d} scale={scale:g}")


@pytest.mark.parametrize("scale", common.SCALES)
def test_bf16_largest_configuration_cpu(scale):
    _largest(CPU, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", common.SCALES)
def test_bf16_largest_configuration_gpu(gpu, scale):
    _largest(gpu, scale)


def _coresident(dev):
    """70 sequences x 8 heads = 560 workgroups that share CUs: against float64, and sequence 0 alone gives the bits of its slice."""
    Lq, Lk, H, d, lead = common.CORESIDENT
    c = c16.case(Lq, Lk, H, d, lead, 1.0)
    q, k, v = (c[n].to(dev) for n in "qkv")
    full = c16.fused16(q, k, v, H)
    c16.gated(full, c, f"Lq={Lq} Lk={Lk} H={H} d={d} sequences={lead}")
    assert c16.bits_equal(c16.fused16(q[0, :1], k[0, :1], v[0, :1], H), full[0, :1])


def test_bf16_coresident_workgroups_cpu():
    _coresident(CPU)


@pytest.mark.gpu
def test_bf16_coresident_workgroups_gpu(gpu):
    _coresident(gpu)


def _head_counts(dev, Lq, Lk, H, d):
    c = c16.case(Lq, Lk, H, d, (3,), 1.0)
    c16.gated(_run(dev, c), c, f"Lq={Lq} Lk={Lk} H={H} d={d}")


@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_bf16_head_counts_cpu(Lq, Lk, H, d):
    _head_counts(CPU, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", common.HEAD_COUNTS)
def test_bf16_head_counts_gpu(gpu, Lq, Lk, H, d):
    _head_counts(gpu, Lq, Lk, H, d)


def _kinds(dev, Lq, Lk, H, d, kind):
    """"huge": logits in the thousands; "negative": every true score far below 0 (a padded zero score would win the maximum)."""
    c = c16.case(Lq, Lk, H, d, (3,), 1.0, kind)
    c16.gated(_run(dev, c), c, f"Lq={Lq} Lk={Lk} H={H} d={d} {kind}")


@pytest.mark.parametrize("Lq,Lk,H,d,kind", c16.KINDS)
def test_bf16_huge_and_negative_logits_cpu(Lq, Lk, H, d, kind):
    _kinds(CPU, Lq, Lk, H, d, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d,kind", c16.KINDS)
def test_bf16_huge_and_negative_logits_gpu(gpu, Lq, Lk, H, d, kind):
    _kinds(gpu, Lq, Lk, H, d, kind)


# ---- b. exact answers ------------------------------------------------------------------------------------------------------------------
def _exact(dev, make, Lq, Lk, H, d):
    c = make(Lq, Lk, H, d)
    got = c16.fused16(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), H).cpu()
    same = c16.same_bits_mask(got, c["want"])
    bad = int((~same).sum())
    print(f"{make.__wrapped__.__name__} [{dev.type}] Lq={Lq} Lk={Lk} H={H} d={d}: {bad} of {same.numel()} elements differ")
    if bad:
        s, i, col = (int(x) for x in torch.nonzero(~same)[0])
        raise AssertionError(f"{bad} elements differ; the first at sequence {s}, query {i}, column {col}: got {float(got[s, i, col])}, "
                             f"want {float(c['want'][s, i, col])}")


@pytest.mark.parametrize("Lq,Lk,H,d", c16.EXACT_SHAPES)
def test_bf16_one_hot_weights_return_the_selected_row_cpu(Lq, Lk, H, d):
    _exact(CPU, c16.one_hot_case, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", c16.EXACT_SHAPES)
def test_bf16_one_hot_weights_return_the_selected_row_gpu(gpu, Lq, Lk, H, d):
    _exact(gpu, c16.one_hot_case, Lq, Lk, H, d)


@pytest.mark.parametrize("Lq,Lk,H,d", c16.EXACT_SHAPES)
def test_bf16_uniform_weights_return_the_exact_mean_cpu(Lq, Lk, H, d):
    _exact(CPU, c16.uniform_case, Lq, Lk, H, d)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk,H,d", c16.EXACT_SHAPES)
def test_bf16_uniform_weights_return_the_exact_mean_gpu(gpu, Lq, Lk, H, d):
    _exact(gpu, c16.uniform_case, Lq, Lk, H, d)


# ---- c. independence and strides ---------------------------------------------------------------------------------------------------------
def _independence(dev):
    """Sequence 0 alone, as sequence 0 of 70 and as sequence 69 of 70: the same bits; a second run: the same bits."""
    c = c16.case(89, 89, 4, 40, (7, 10), 1.0)
    q, k, v = (c[n].to(dev).reshape(70, 89, 160) for n in "qkv")
    full = c16.fused16(q, k, v, 4)
    assert c16.bits_equal(full, c16.fused16(q, k, v, 4))
    alone = c16.fused16(q[:1], k[:1], v[:1], 4)
    assert c16.bits_equal(alone, full[:1])
    moved = c16.fused16(torch.cat([q[1:], q[:1]]), torch.cat([k[1:], k[:1]]), torch.cat([v[1:], v[:1]]), 4)
    assert c16.bits_equal(moved[69:], alone) and c16.bits_equal(moved[:69], full[1:])
    grid = c16.fused16(q.view(7, 10, 89, 160), k.view(7, 10, 89, 160), v.view(7, 10, 89, 160), 4)
    assert c16.bits_equal(grid.reshape(70, 89, 160), full)


def test_bf16_independence_cpu():
    _independence(CPU)


@pytest.mark.gpu
def test_bf16_independence_gpu(gpu):
    _independence(gpu)


def _axes(dev):
    """Both axes of one [N, T', F', H d] buffer (q, k, v slices of one projection-like buffer) against contiguous copies."""
    N, T, Fq, H, d = 2, 5, 37, 2, 24
    g = torch.Generator().manual_seed(92)
    buf = torch.randn(N, T, Fq, 3 * H * d, generator=g).bfloat16().to(dev)
    q, k, v = buf[..., :H * d], buf[..., H * d:2 * H * d], buf[..., 2 * H * d:]
    want_f = c16.fused16(q.contiguous(), k.contiguous(), v.contiguous(), H)
    got_f = c16.fused16(q, k, v, H)                               # the frequency axis: sequences (N, T'), tokens F'
    assert c16.bits_equal(got_f, want_f)
    qt, kt, vt = (x.transpose(1, 2) for x in (q, k, v))           # the time axis: sequences (N, F'), tokens T'
    want_t = c16.fused16(qt.contiguous(), kt.contiguous(), vt.contiguous(), H)
    got_t = c16.fused16(qt, kt, vt, H)
    assert got_t.shape == (N, Fq, T, H * d) and got_t.transpose(1, 2).is_contiguous()      # laid out like q
    assert c16.bits_equal(got_t, want_t)
    c16.gated(want_t, c16.finish(qt.cpu().contiguous(), kt.cpu().contiguous(), vt.cpu().contiguous(), H), "time axis of a shared buffer")


def test_bf16_both_axes_of_one_buffer_cpu():
    _axes(CPU)


@pytest.mark.gpu
def test_bf16_both_axes_of_one_buffer_gpu(gpu):
    _axes(gpu)


def _contract_case(dev):
    Lq, Lk, H, d, lead = common.CONTRACT
    c = c16.case(Lq, Lk, H, d, lead, 1.0)
    return c, H, d, tuple(c[n].to(dev) for n in "qkv")


def _strides(dev):
    """Stride-0 q, k, v; an odd token stride from an aligned base; each tensor one element off 16 bytes; out one element off."""
    c, H, d, (q, k, v) = _contract_case(dev)
    S, Lq, HD = q.shape[0], q.shape[1], H * d
    want = c16.fused16(q, k, v, H)
    c16.gated(want, c, "contract shape, aligned")
    k0, v0 = k[:1].expand(S, -1, -1), v[:1].expand(S, -1, -1)
    assert k0.stride(0) == 0 and v0.stride(0) == 0
    assert c16.bits_equal(c16.fused16(q, k0, v0, H), c16.fused16(q, k0.contiguous(), v0.contiguous(), H))
    q0 = q[:1].expand(S, -1, -1)
    got = c16.fused16(q0, k, v, H)
    assert got.is_contiguous() and c16.bits_equal(got, c16.fused16(q0.contiguous(), k, v, H)) and c16.bits_equal(got[0], want[0])
    for name in "qkv":
        args = {"q": q, "k": k, "v": v}
        x = args[name]
        args[name] = c16.one_off(x)
        assert c16.bits_equal(c16.fused16(args["q"], args["k"], args["v"], H), want), f"{name} one element off 16 bytes"
        parent = torch.zeros(*x.shape[:-1], HD + 1, dtype=BF16, device=dev)
        parent[..., :HD] = x
        args[name] = parent[..., :HD]
        assert args[name].data_ptr() % 16 == 0 and args[name].stride(-2) == HD + 1
        assert c16.bits_equal(c16.fused16(args["q"], args["k"], args["v"], H), want), f"{name} with token stride H d + 1"
    big = torch.full((S, Lq, HD + 1), -7.0, dtype=BF16, device=dev)
    o = big[..., 1:]
    assert o.data_ptr() % 8 == 2
    c16.raw_op16(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), o.unsqueeze(0), H)
    assert c16.bits_equal(o.contiguous(), want), "out one element off alignment"
    assert bool((big[..., 0] == -7.0).all())


def test_bf16_strides_and_alignment_cpu():
    _strides(CPU)


@pytest.mark.gpu
def test_bf16_strides_and_alignment_gpu(gpu):
    _strides(gpu)


# ---- d. the memory contract ----------------------------------------------------------------------------------------------------------------
def _poison(dev):
    """q, k, v are views into parents that hold NaN behind Lq, behind Lk and in the gaps between their strided rows; out is a strided
    view into a sentinel-filled buffer.  Nothing outside the Lq x H d rows changes, no NaN leaks in, the inputs keep their bits."""
    S, Lq, Lk, H, d = 5, 35, 33, 4, 40
    HD = H * d
    c = c16.case(Lq, Lk, H, d, (S,), 1.0)
    parents = {}
    for name, L in (("q", Lq), ("k", Lk), ("v", Lk)):
        p = torch.full((S, L + 7, HD + 8), float("nan"), dtype=BF16)
        p[:, :L, :HD] = c[name]
        parents[name] = p.to(dev)
    kept = {n: c16.bits(p).clone() for n, p in parents.items()}
    q, k, v = (parents[n][:, :L, :HD] for n, L in (("q", Lq), ("k", Lk), ("v", Lk)))
    SENT = -12345.0                                               # -12352 in bf16: a value no output takes
    big = torch.full((S + 2, Lq + 5, HD + 16), SENT, dtype=BF16, device=dev)
    out = big[1:S + 1, 2:Lq + 2, 8:8 + HD]
    c16.raw_op16(q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), out.unsqueeze(0), H)
    assert bool(torch.isfinite(out).all())
    c16.gated(out.contiguous(), c, "poisoned parents")
    assert c16.bits_equal(out.contiguous(), c16.fused16(c["q"].to(dev), c["k"].to(dev), c["v"].to(dev), H))
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[1:S + 1, 2:Lq + 2, 8:8 + HD] = False
    assert bool((big[mask] == torch.tensor(SENT, dtype=BF16)).all())                  # every sentinel outside the view is untouched
    for n, p in parents.items():
        assert torch.equal(c16.bits(p), kept[n]), n


def test_bf16_poison_cpu():
    _poison(CPU)


@pytest.mark.gpu
def test_bf16_poison_gpu(gpu):
    _poison(gpu)


# ---- e. non-finite values ----------------------------------------------------------------------------------------------------------------
def _non_finite(dev):
    """A NaN in one k row, a NaN in one q row and a +inf in one v element reach exactly the outputs they belong to."""
    c, H, d, (q, k, v) = _contract_case(dev)
    clean = c16.fused16(q, k, v, H)
    assert bool(torch.isfinite(clean).all())
    head1 = slice(d, 2 * d)
    kn = k.clone()
    kn[1, 5, head1] = float("nan")                                # every query of that sequence and head
    got = c16.fused16(q, kn, v, H)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[1, :, head1] = True
    assert torch.equal(torch.isnan(got), hit) and bool(c16.same_bits_mask(got, clean)[~hit].all()), "NaN in k"
    qn = q.clone()
    qn[2, 7, 3] = float("nan")                                    # that query, head 0
    got = c16.fused16(qn, k, v, H)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[2, 7, :d] = True
    assert torch.equal(torch.isnan(got), hit) and bool(c16.same_bits_mask(got, clean)[~hit].all()), "NaN in q"
    vi = v.clone()
    vi[0, 11, d + 2] = float("inf")                               # its column of that sequence: every weight of key 11 is positive here
    got = c16.fused16(q, k, vi, H)
    hit = torch.zeros_like(clean, dtype=torch.bool)
    hit[0, :, d + 2] = True
    assert torch.equal(torch.isposinf(got), hit) and not bool(torch.isnan(got).any()), "+inf in v"
    assert bool(c16.same_bits_mask(got, clean)[~hit].all()), "+inf in v"


def test_bf16_non_finite_stay_put_cpu():
    _non_finite(CPU)


@pytest.mark.gpu
def test_bf16_non_finite_stay_put_gpu(gpu):
    _non_finite(gpu)


# ---- f. the C entry point -----------------------------------------------------------------------------------------------------------------
def _direct(lib, q, k, v, out, n0, n1, Lq, Lk, H, d, strides, stream=None):
    return lib.semicrf_axial_attention_bf16(q, k, v, out, n0, n1, Lq, Lk, H, d, *strides, stream)


def _einval_cases(ptr, st):
    """(arguments after the four pointers with those, word of the message) of every SEMICRF_EINVAL case; `ptr`: the four pointers."""
    q, k, v, o = ptr
    cases = [((q, k, v, o, 1, 1, Lq, Lk, H, d, st), b"supported")
             for Lq, Lk, H, d in ((257, 8, 1, 8), (8, 300, 1, 8), (8, 8, 1, 12), (8, 8, 0, 8), (8, 8, 1, 72), (0, 8, 1, 8))]
    cases += [((q, k, v, None, 1, 1, 8, 8, 1, 8, st), b"NULL"), ((None, k, v, o, 1, 1, 8, 8, 1, 8, st), b"NULL"),
              ((q, k, v, o, -1, 1, 8, 8, 1, 8, st), b">= 0"), ((q, k, v, o, 1 << 20, 1 << 12, 8, 8, 1, 8, st), b"2^31")]
    for i in range(4):
        odd = [q, k, v, o]
        odd[i] = ctypes.c_void_p(odd[i].value + 1)
        cases.append(((*odd, 1, 1, 8, 8, 1, 8, st), b"aligned"))
    for i in (0, 5, 10):
        bad = list(st); bad[i] = -st[i] - 1
        cases.append(((q, k, v, o, 1, 1, 8, 8, 1, 8, bad), b"negative"))
    for i in (2, 5, 8, 11):                                      # a token stride AT the limit, one tensor at a time
        bad = list(st); bad[i] = common.TOKEN_STRIDE_LIMIT
        cases.append(((q, k, v, o, 1, 1, 8, 8, 1, 8, bad), b"2^28"))
    return cases


def test_bf16_c_entry_point_rejects_cpu():
    """Every EINVAL case returns nonzero with its message before any pointer is used (the pointers here are never valid); the supported
    predicate is the fp32 op's over a grid; the torch op checks the same set, the shapes and the dtype."""
    from transkun_amd import _lib, backbone
    lib = _lib.load()
    assert "semicrf_axial_attention_bf16" in _lib.EXPORTED and "semicrf_axial_attention_bf16_supported" in _lib.EXPORTED
    assert lib.semicrf_abi_version() == 2
    fake = tuple(ctypes.c_void_p(4096 + 512 * i) for i in range(4))
    st = [1000, 100, 96] * 4
    for args, word in _einval_cases(fake, st):
        assert _direct(lib, *args[:10], args[10]) == 1, (args[4:10], word)
        assert word in lib.semicrf_last_error(), (word, lib.semicrf_last_error())
    assert _direct(lib, *fake, 0, 5, 8, 8, 1, 8, st) == 0        # no sequences: nothing to do, nothing launched
    for Lq in (-1, 0, 1, 33, 256, 257):
        for Lk in (0, 1, 149, 256, 257):
            for H in (-1, 0, 1, 4, 1000):
                for d in (0, 4, 8, 12, 40, 64, 65, 72):
                    want = lib.semicrf_axial_attention_supported(Lq, Lk, H, d)
                    assert lib.semicrf_axial_attention_bf16_supported(Lq, Lk, H, d) == want, (Lq, Lk, H, d)
                    assert backbone.attention_bf16_supported(Lq, Lk, H, d) == bool(want)
    ops = _lib.ops()
    x = torch.zeros(1, 1, 4, 12, dtype=BF16)
    with pytest.raises(RuntimeError, match="support"):
        ops.axial_attention_bf16(x, x, x, torch.empty_like(x), 1)
    y = torch.zeros(1, 1, 4, 16, dtype=BF16)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bf16(y, y, y, torch.empty(1, 1, 5, 16, dtype=BF16), 2)
    for bad in ((y.float(), y, y, y), (y, y.float(), y, y), (y, y, y.float(), y), (y, y, y, y.float()), (y.half(),) * 4):
        with pytest.raises(RuntimeError, match="bfloat16"):
            ops.axial_attention_bf16(bad[0], bad[1], bad[2], torch.empty_like(bad[3]), 2)
    with pytest.raises(RuntimeError):
        ops.axial_attention_bf16(y.transpose(-1, -2), y, y, torch.empty_like(y), 2)
    with pytest.raises(RuntimeError, match="repeat"):
        ops.axial_attention_bf16(y, y, y, torch.empty(1, 1, 1, 16, dtype=BF16).expand(1, 1, 4, 16), 2)


@pytest.mark.gpu
def test_bf16_c_entry_point_leaves_output_untouched_gpu(gpu):
    """The same EINVAL cases on real tensors: a sentinel-filled `out` keeps every bit, and the error text is set."""
    from transkun_amd import _lib
    lib = _lib.load()
    x = torch.randn(3, 8, 16, device=gpu).bfloat16()
    out = torch.full((3, 8, 16), 3.0, dtype=BF16, device=gpu)
    ptrs = tuple(ctypes.c_void_p(t.data_ptr()) for t in (x, x, x, out))
    st = [0, 16, 16] * 3 + [0, 128, 16]
    stream = _lib.stream_of(x)
    for args, word in _einval_cases(ptrs, st):
        assert _direct(lib, *args[:10], args[10], stream) == 1, (args[4:10], word)
        assert word in lib.semicrf_last_error(), word
    torch.cuda.synchronize(gpu)
    assert bool((out == 3.0).all())
    assert _direct(lib, *ptrs, 1, 1, 8, 8, 1, 8, st, stream) == 0                      # and the valid call of the same arguments runs
    torch.cuda.synchronize(gpu)
    want = c16.fused16(x[:1, :, :8], x[:1, :, :8], x[:1, :, :8], 1)
    assert c16.bits_equal(out[:1, :, :8].contiguous(), want.contiguous()) and bool((out[1:] == 3.0).all()) and bool((out[:1, :, 8:] == 3.0).all())


def test_bf16_token_stride_limit_routes_to_stock():
    """The views backbone.axial_attention keeps from the device op, bf16 included: the limit is read from the views (meta tensors)."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    assert backbone.ATTENTION_TOKEN_STRIDE_LIMIT == lim
    buf = torch.empty(2 * lim + 64, dtype=BF16, device="meta")
    ok = torch.empty(1, 5, 48, dtype=BF16, device="meta")
    for stride, L, fits in ((lim, 2, False), (lim - 8, 2, True), (lim, 1, True)):
        view = buf.as_strided((1, L, 48), (0, stride, 1))
        assert backbone._token_strides_fit(view, ok, ok) == fits and backbone._token_strides_fit(ok, ok, view) == fits


@pytest.mark.gpu
def test_bf16_token_stride_beyond_the_limit_gpu(gpu):
    """A q whose two tokens lie 2^28 elements apart (512 MiB of bf16, of which two rows are written): the op turns it down, and
    backbone.axial_attention(bf16="fused") answers by the stock route bit for bit."""
    from transkun_amd import backbone
    lim = common.TOKEN_STRIDE_LIMIT
    g = torch.Generator().manual_seed(2829)
    q, k, v = (torch.randn(1, L, 48, generator=g).bfloat16().to(gpu) for L in (2, 5, 5))
    buf = torch.empty(lim + 64, dtype=BF16, device=gpu)
    far = buf.as_strided((1, 2, 48), (2 * lim, lim, 1))
    far.copy_(q)
    with pytest.raises(RuntimeError, match=r"2\^28"):
        c16.raw_op16(far.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0), torch.empty(1, 1, 2, 48, dtype=BF16, device=gpu), 2)
    before = dict(backbone.ATTENTION_BF16_ROUTES)
    with torch.no_grad():
        got = backbone.axial_attention(far, k, v, 2, bf16="fused")
        assert torch.equal(got, backbone.attention_torch(far, k, v, 2))
    assert backbone.ATTENTION_BF16_ROUTES == {"fused": before["fused"], "torch": before["torch"] + 1}
    del far, buf
    torch.cuda.empty_cache()


# ---- g. the route ------------------------------------------------------------------------------------------------------------------------
def _routes(dev):
    from transkun_amd import backbone
    assert backbone.ROUTES == ("fused", "fused-train", "torch") and set(backbone.ATTENTION_ROUTES) == {"fused", "fused-train", "torch", "bwd"}
    assert backbone.BF16_KINDS == ("torch", "fused") and backbone.DEFAULT_ATTENTION_BF16 == "torch"
    assert set(backbone.ATTENTION_BF16_ROUTES) == {"fused", "torch"}
    g = torch.Generator().manual_seed(6)

    def rnd(*shape, dtype=BF16):
        return torch.randn(*shape, generator=g).to(dtype).to(dev)

    def moved(fn):
        a, b = dict(backbone.ATTENTION_ROUTES), dict(backbone.ATTENTION_BF16_ROUTES)
        out = fn()
        return out, {n: backbone.ATTENTION_ROUTES[n] - a[n] for n in a if backbone.ATTENTION_ROUTES[n] != a[n]}, \
            {n: backbone.ATTENTION_BF16_ROUTES[n] - b[n] for n in b if backbone.ATTENTION_BF16_ROUTES[n] != b[n]}
    q, k, v = rnd(3, 9, 32), rnd(3, 7, 32), rnd(3, 7, 32)
    with torch.no_grad():
        stock = backbone.attention_torch(q, k, v, 2)
        # the defaults are unchanged: without the keyword a bf16 call is the stock route and moves its counter alone
        got, a, b = moved(lambda: backbone.axial_attention(q, k, v, 2))
        assert torch.equal(got, stock) and got.dtype == BF16 and a == {"torch": 1} and b == {}
        got, a, b = moved(lambda: backbone.axial_attention(q, k, v, 2, bf16="torch"))
        assert torch.equal(got, stock) and a == {"torch": 1} and b == {}
        # the keyword: the op answers
        got, a, b = moved(lambda: backbone.axial_attention(q, k, v, 2, bf16="fused"))
        assert got.dtype == BF16 and got.shape == q.shape and a == {"fused": 1} and b == {"fused": 1}
        c16.gated(got, c16.finish(q.cpu(), k.cpu(), v.cpu(), 2), "the keyword's call")
        got2, a, b = moved(lambda: backbone.axial_attention(q, k, v, 2, route="fused-train", bf16="fused"))
        assert c16.bits_equal(got2, got) and a == {"fused": 1} and b == {"fused": 1}
        # float32 calls are what they were, and are not counted
        qf, kf, vf = q.float(), k.float(), v.float()
        got, a, b = moved(lambda: backbone.axial_attention(qf, kf, vf, 2, bf16="fused"))
        assert common.bits_equal(got, backbone.axial_attention(qf, kf, vf, 2)) and a == {"fused": 1} and b == {}
        # with the keyword, the stock route bit for bit: route = "torch", outside the supported set, broadcasting keys
        for args, kw in (((q, k, v, 2), dict(route="torch")),
                         ((rnd(2, 257, 32), rnd(2, 257, 32), rnd(2, 257, 32), 2), {}),
                         ((rnd(2, 9, 24), rnd(2, 9, 24), rnd(2, 9, 24), 2), {}),
                         ((rnd(2, 3, 9, 32), rnd(2, 1, 7, 32), rnd(2, 1, 7, 32), 2), {})):
            got, a, b = moved(lambda: backbone.axial_attention(*args, bf16="fused", **kw))
            assert torch.equal(got, backbone.attention_torch(*args)) and a == {"torch": 1} and b == {"torch": 1}, (kw, a, b)
    # mixed dtypes: what the call is without the keyword (the stock call's own answer or its own error), uncounted
    for mixed in ((q, k.float(), v.float()), (q.float(), k, v)):
        outcome = []
        for kw in ({}, dict(bf16="fused")):
            try:
                with torch.no_grad():
                    outcome.append(backbone.axial_attention(*mixed, 2, **kw))
            except RuntimeError as ex:
                outcome.append(type(ex))
        assert (outcome[0] is outcome[1]) if isinstance(outcome[0], type) else torch.equal(outcome[0], outcome[1])
    assert moved(lambda: None)[2] == {}
    # under autograd both fused routes answer by the stock route for bf16: output and gradients
    for route in ("fused", "fused-train"):
        grads = []
        for fn in (lambda x, y, z: backbone.axial_attention(x, y, z, 2, route=route, bf16="fused"),
                   lambda x, y, z: backbone.attention_torch(x, y, z, 2)):
            x, y, z = (t.clone().requires_grad_() for t in (q, k, v))
            (out, a, b) = moved(lambda: fn(x, y, z))
            assert out.requires_grad
            out.float().square().sum().backward()
            grads.append((out.detach(), x.grad, y.grad, z.grad))
        assert a == {} and b == {}                                # (the second call is attention_torch itself)
        for x, y in zip(*grads):
            assert x is not None and torch.equal(x, y)
    x, y, z = (t.clone().requires_grad_() for t in (q, k, v))
    _, a, b = moved(lambda: backbone.axial_attention(x, y, z, 2, bf16="fused"))
    assert a == {"torch": 1} and b == {"torch": 1}
    with torch.no_grad():                                         # under no_grad the same tensors take the op
        _, a, b = moved(lambda: backbone.axial_attention(x, y, z, 2, bf16="fused"))
    assert a == {"fused": 1} and b == {"fused": 1}
    with pytest.raises(ValueError):
        backbone.axial_attention(q, k, v, 2, bf16="eager")
    with pytest.raises(ValueError):
        backbone.axial_attention(q, k, v, 2, route="eager", bf16="fused")


def test_bf16_routes_cpu():
    _routes(CPU)


@pytest.mark.gpu
def test_bf16_routes_gpu(gpu):
    _routes(gpu)


# ---- h. the modules ------------------------------------------------------------------------------------------------------------------------
def _module_errors(dev):
    """A BasicBlock and the small Backbone in bf16 weights: the error of attentionBf16 = "fused" against the same module in float64
    (weights upcast from the bf16 ones) is at most GATE times the error of "torch" against the same truth."""
    from transkun_amd import backbone
    m16, m64, fx = c16.bf16_backbone("backbone_small", dev)
    assert m16.attentionBf16 == "torch" and m16.encoderLayers[0].attentionBf16 == "torch"
    x, idx, lin = fx["x"].bfloat16(), fx["outputIndices"], fx["layer_in"].bfloat16()
    with torch.no_grad():
        truth = {"backbone": m64(x.double(), idx), "block": m64.encoderLayers[0](lin.double())}
    calls = []
    hooks = [a.register_forward_hook(lambda *_: calls.append(1)) for a in m16.modules() if isinstance(a, backbone.MultiHeadAttentionKernel)]
    err = {}
    for kind in ("torch", "fused"):
        m16.attentionBf16 = kind
        assert m16.attentionBf16 == kind and all(layer.attentionBf16 == kind for layer in m16.encoderLayers)
        del calls[:]
        before = dict(backbone.ATTENTION_BF16_ROUTES), backbone.ATTENTION_ROUTES["torch"]
        with torch.no_grad():
            got = {"backbone": m16(x.to(dev), idx.to(dev)), "block": m16.encoderLayers[0](lin.to(dev))}
        if kind == "fused":                                       # every attention call of both forwards went to the bf16 op
            assert len(calls) > 0 and backbone.ATTENTION_BF16_ROUTES["fused"] - before[0]["fused"] == len(calls)
            assert backbone.ATTENTION_BF16_ROUTES["torch"] == before[0]["torch"] and backbone.ATTENTION_ROUTES["torch"] == before[1]
        else:
            assert backbone.ATTENTION_BF16_ROUTES == before[0]
        for tag, g in got.items():
            assert g.dtype == BF16 and g.shape == truth[tag].shape and bool(torch.isfinite(g).all())
            err[kind, tag] = float((g.cpu().double() - truth[tag]).abs().max())
    for tag in ("backbone", "block"):
        print(f"bf16 {tag} [{dev.type}]: error fused {err['fused', tag]:.3e}  torch {err['torch', tag]:.3e}  "
              f"ratio {err['fused', tag] / err['torch', tag]:.2f} (gate {c16.GATE:g})")
        assert err["fused", tag] <= c16.GATE * err["torch", tag], tag
    for h in hooks:
        h.remove()
    m16.encoderLayers[0].attentionBf16 = "torch"
    assert m16.attentionBf16 == "mixed"
    with pytest.raises(ValueError):
        m16.attentionBf16 = "eager"
    with pytest.raises(ValueError):
        m16.encoderLayers[0].attentionBf16 = "eager"


def test_bf16_modules_cpu():
    _module_errors(CPU)


@pytest.mark.gpu
def test_bf16_modules_gpu(gpu):
    _module_errors(gpu)


def test_bf16_basic_block_makes_no_transposed_copy():
    """With attentionBf16 = "fused" a bf16 BasicBlock forward copies no hidden-state-sized tensor (the idiom of
    test_backbone.test_basic_block_makes_no_transposed_copy); with "torch", counted the same way, it does."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m16, _, fx = c16.bf16_backbone("backbone_d40", CPU)
    blk = m16.encoderLayers[0]
    lin = fx["layer_in"].bfloat16()
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
    for kind in ("fused", "torch"):
        blk.attentionBf16 = kind
        with torch.no_grad(), Count() as c:
            blk(lin)
        counts[kind] = c.copies
    assert counts["fused"] == [], counts["fused"]
    assert len(counts["torch"]) > 0


def _autocast(dev):
    """The fp32-weight Backbone under torch.autocast(bfloat16): its attention calls are bf16 calls, and with attentionBf16 = "fused"
    ATTENTION_BF16_ROUTES["fused"] counts every one of them."""
    from transkun_amd import backbone
    m, fx = common.make_backbone("backbone_small", dev, "fused")
    x, idx = fx["x"].to(dev), fx["outputIndices"].to(dev)
    calls = []
    hooks = [a.register_forward_hook(lambda *_: calls.append(1)) for a in m.modules() if isinstance(a, backbone.MultiHeadAttentionKernel)]
    outs = {}
    for kind in ("torch", "fused"):
        m.attentionBf16 = kind
        del calls[:]
        before = dict(backbone.ATTENTION_BF16_ROUTES), backbone.ATTENTION_ROUTES["torch"]
        with torch.no_grad(), torch.autocast(device_type=dev.type, dtype=BF16):
            outs[kind] = m(x, idx)
        assert len(calls) > 0 and bool(torch.isfinite(outs[kind]).all())
        if kind == "fused":
            assert backbone.ATTENTION_BF16_ROUTES["fused"] - before[0]["fused"] == len(calls)
            assert backbone.ATTENTION_BF16_ROUTES["torch"] == before[0]["torch"] and backbone.ATTENTION_ROUTES["torch"] == before[1]
        else:
            assert backbone.ATTENTION_BF16_ROUTES == before[0] and backbone.ATTENTION_ROUTES["torch"] - before[1] == len(calls)
    for h in hooks:
        h.remove()
    want = fx["out64"]
    e = {kind: float((o.cpu().double() - want).abs().max()) for kind, o in outs.items()}
    print(f"autocast backbone [{dev.type}]: error fused {e['fused']:.3e}  torch {e['torch']:.3e}")
    assert e["fused"] <= c16.GATE * e["torch"]


def test_bf16_autocast_backbone_cpu():
    _autocast(CPU)


@pytest.mark.gpu
def test_bf16_autocast_backbone_gpu(gpu):
    _autocast(gpu)


@pytest.mark.gpu
def test_bf16_end_to_end_decode_gpu(gpu):
    """audio -> log-mel -> bf16 Backbone (small fixture) -> fp32 interval scorer -> decode() completes with both settings and returns
    one path per output index (the shapes of test_backbone.test_end_to_end_decode_gpu)."""
    from transkun_amd import CRF, backbone, synth
    from transkun_amd.frontend import MelSpectrum, makeFrame, normalize_gain
    from transkun_amd.scorer import ScaledInnerProductIntervalScorer
    fs, hop, win = 44100, 1024, 4096
    nS = 2 * fs
    audio = synth.hash_normal(2 * nS, 971, gpu).view(1, 2, nS) * 0.1
    frames = makeFrame(audio, hop, win)
    mel = MelSpectrum(win, 30, 8000, 229, fs, nExtraWins=5, log=True, toMono=True).to(gpu)
    feat = mel(normalize_gain(frames))[:, 0]                      # [N, T, 229, 6]
    T = feat.shape[1]
    m16, _, fx = c16.bf16_backbone("backbone_small", gpu)
    idx = fx["outputIndices"].to(gpu)
    D = fx["cfg"]["baseSize"] * fx["cfg"]["expansionFactor"]
    torch.manual_seed(67280421310721)
    scorer = ScaledInnerProductIntervalScorer(D, 1).to(gpu)
    with torch.no_grad():
        for kind in ("fused", "torch"):
            m16.attentionBf16 = kind
            before = backbone.ATTENTION_ROUTES["torch"]
            ctx = m16(feat.bfloat16(), idx)
            assert ctx.dtype == BF16 and ctx.shape == (1, idx.numel(), T, D) and bool(torch.isfinite(ctx).all())
            assert (backbone.ATTENTION_ROUTES["torch"] == before) == (kind == "fused")
            S, b = scorer(ctx.float())
            paths = CRF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1)).decode()
            assert len(paths) == idx.numel()
