"""The fused attribute heads, forward and backward, at their edges: transkun_amd.attributes.attribute_heads / attribute_heads_train
(csrc/attr_heads.hip, csrc/attr_heads_bwd.hip on the GPU, the host mirror of csrc/cpu_ops.cpp on CPU tensors).

Head sizes other than 128 / 4, shapes that take the scalar loaders over several tiles or the forward and the backward down different
paths, D > 256, the row edges of the backward (K = 1 .. 513), rows past offsets[-1], pairs outside [0, T - 1], one chain, one frame,
per-element bounds of the nine gradients, device against host mirror bit for bit where no transcendental is involved, poisoned
workspaces and outputs, and ctx views whose data pointer is not 16-byte aligned.

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu); cases, yardstick, gate and bounds:
attr_heads_edges_common.  Measured figures: DESIGN.md section 3, "Attribute heads" and "Attribute heads, training"."""
import copy

import pytest
import torch

import attr_heads_common as common
import attr_heads_train_common as tc
import attr_heads_edges_common as ec

CPU = torch.device("cpu")
T, C = ec.T, ec.C


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _run(dev, c, pairs=None):
    if pairs is None:
        return tc.run_op(dev, c)
    c2 = dict(c)
    c2["pairs"] = pairs
    return tc.run_op(dev, c2)


def _check_train(tag, dev, c, gate=True, pairs=None):
    """The op on a case: the per-element bounds of the two outputs and the nine gradients, and (gate) the max-abs gate."""
    lv, of, grads = _run(dev, c, pairs)
    got = [lv, of] + grads
    assert grads[0].shape == c["ctx"].shape
    for g in got:
        assert bool(torch.isfinite(g).all())
    worst = ec.check_bound(tag, got, c)
    if gate:
        tc.check_gate(tag, ec.OUT_NAMES, got, c["truth"], c["e32"])
    print(f"{tag}: worst fraction of the per-element bound {worst:.4f}")
    return got


# ---- 1. the shape grid ---------------------------------------------------------------------------------------------------------------
def _check_eval_grid(dev, D, Hv, Ho, Nv, No):
    c = ec.eval_case(D, Hv, Ho, Nv, No)
    vp, op, ctx, pairs, offsets = common.to_device(dev, c["vp"], c["op"], c["ctx"], c["pairs"], c["offsets"])
    K = c["K"]
    lv, of, sym, sc = common.fused(ctx, pairs, offsets, vp, op, K)
    assert lv.shape == (K, Nv) and of.shape == (K, No) and lv.dtype == of.dtype == torch.float32
    assert torch.equal(sc.cpu(), c["chain"]) and torch.equal(sym.cpu(), c["chain"] % common.N_SYM)
    for tag, got, want, bound, e32, use32 in (("logitsVelocity", lv, c["truth"][0], c["bound"][0], c["e32"][0], c["use32"][0]),
                                              ("ofLogits", of, c["truth"][1], c["bound"][1], c["e32"][1], c["use32"][1])):
        err = (got.cpu().double() - want).abs()
        e, use = float(err.max()), float((err / bound).max())
        print(f"attribute_heads [{dev.type}] D={D} Hv={Hv} Ho={Ho} Nv={Nv} No={No} {tag}: error {e:.3e}  torch fp32 {e32:.3e}  "
              f"ratio {e / e32:.2f} (gate {common.GATE:g})  bound used {use:.4f} (torch fp32 {use32:.4f})")
        assert use32 <= 1.0
        assert bool((err <= bound).all()), (tag, use)
        assert e <= common.GATE * e32, (tag, e, e32)


@pytest.mark.parametrize("D,Hv,Ho,Nv,No", ec.GRID)
def test_grid_eval_forward_cpu(D, Hv, Ho, Nv, No):
    _check_eval_grid(CPU, D, Hv, Ho, Nv, No)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No", ec.GRID)
def test_grid_eval_forward_gpu(gpu, D, Hv, Ho, Nv, No):
    _check_eval_grid(gpu, D, Hv, Ho, Nv, No)


P_GRID = [s + ec.P_MAIN for s in ec.GRID] + [ec.GRID[0] + p for p in ec.P_EXTRA]


def _check_train_grid(dev, D, Hv, Ho, Nv, No, pv, po):
    c = ec.train_case(D, Hv, Ho, Nv, No, pv, po)
    _check_train(f"grid [{dev.type}] D={D} Hv={Hv} Ho={Ho} Nv={Nv} No={No} p={pv:g}/{po:g}", dev, c)


@pytest.mark.parametrize("D,Hv,Ho,Nv,No,pv,po", P_GRID)
def test_grid_training_cpu(D, Hv, Ho, Nv, No, pv, po):
    _check_train_grid(CPU, D, Hv, Ho, Nv, No, pv, po)


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No,pv,po", P_GRID)
def test_grid_training_gpu(gpu, D, Hv, Ho, Nv, No, pv, po):
    _check_train_grid(gpu, D, Hv, Ho, Nv, No, pv, po)


# ---- 2. the row edges of the backward ------------------------------------------------------------------------------------------------
def _check_rows(dev, K):
    c = ec.train_case(*ec.ROW_SHAPE, K=K)
    _check_train(f"rows [{dev.type}] K={K}", dev, c, gate=K >= 64)       # below 64 rows the maximum is no stable statistic


@pytest.mark.parametrize("K", ec.ROW_KS)
def test_row_edges_cpu(K):
    _check_rows(CPU, K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", ec.ROW_KS)
def test_row_edges_gpu(gpu, K):
    _check_rows(gpu, K)


def _check_last_row_plane(dev):
    """K = HEADS_BWD_ROW_CHUNK + 1: the second chunk holds one row.  The parameter gradients are fp32(plane 0 + plane 1); plane 0 is
    the result on the first chunk's rows alone (the same seed: the mask reads the global row), plane 1 the result of the whole call
    with the cotangents of the first chunk's rows zero (a zero cotangent row contributes an exact zero to every chain).  Bit for bit."""
    R = ec._R()
    c = ec.train_case(*ec.ROW_SHAPE, K=R + 1)
    whole = tc.run_op(dev, c)[2]
    first = dict(c)
    first.update(K=R, pairs=c["pairs"][:R].contiguous(), dlv=c["dlv"][:R].contiguous(), dof=c["dof"][:R].contiguous())
    # the R + 1 rows are sorted by chain and the last chain is empty: the first R rows keep their chains under the same offsets
    assert torch.equal(common.chains_of(c["offsets"], R + 1)[:R], common.chains_of(c["offsets"], R))
    plane0 = tc.run_op(dev, first)[2]
    last = dict(c)
    last.update(dlv=c["dlv"].clone(), dof=c["dof"].clone())
    last["dlv"][:R] = 0; last["dof"][:R] = 0
    plane1 = tc.run_op(dev, last)[2]
    for name, a, p0, p1 in list(zip(tc.NAMES, whole, plane0, plane1))[1:]:
        assert float(p1.abs().max()) > 0, name
        assert _bits_equal(a, p0 + p1), name
        assert not _bits_equal(a, p0), name


def test_last_row_is_its_own_plane_cpu():
    _check_last_row_plane(CPU)


@pytest.mark.gpu
def test_last_row_is_its_own_plane_gpu(gpu):
    _check_last_row_plane(gpu)


# ---- 3. the layout edges of the backward ---------------------------------------------------------------------------------------------
def _check_layout(dev, kind):
    c = ec.layout_case(kind)
    got = _check_train(f"layout {kind} [{dev.type}] K={c['K']}", dev, c)
    dctx = got[2].detach().cpu()
    unread = c["hits"] == 0
    assert bool(unread.any()) and bool((dctx[unread] == 0).all())         # exactly 0.0 at every frame that no row reads
    assert bool((dctx[~unread].abs().amax(-1) > 0).all())
    if kind == "past":
        assert int(c["hits"].view(C, T)[C - 1].sum()) == 2 * 30 and float(dctx.view(C, T, -1)[C - 1].abs().max()) > 0
    elif kind == "outside":
        raw = _run(dev, c, c["raw_pairs"])                                # the op clamps: the bits of the run on clamped pairs
        for name, a, b in zip(ec.OUT_NAMES, got, [raw[0], raw[1]] + raw[2]):
            assert _bits_equal(a.detach(), b.detach()), name
    elif kind in ("chain0", "chainlast"):
        only = 0 if kind == "chain0" else C - 1
        assert bool(((c["hits"].view(C, T).sum(1) > 0) == (torch.arange(C) == only)).all())
    else:
        assert int((~unread).sum()) == 1 and int(c["hits"].view(C, T)[2, 3]) == 2 * c["K"] == 400


LAYOUTS = ["past", "outside", "chain0", "chainlast", "frame"]


@pytest.mark.parametrize("kind", LAYOUTS)
def test_layout_edges_cpu(kind):
    _check_layout(CPU, kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", LAYOUTS)
def test_layout_edges_gpu(gpu, kind):
    _check_layout(gpu, kind)


# ---- 5. device = host mirror, bit for bit, where no transcendental is involved (device only) -------------------------------------------
BIT_CASES = [s + (common.K_GATE,) for s in ec.GRID] + [ec.ROW_SHAPE + (513,)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No", ec.GRID)
def test_training_forward_z_bits_gpu(gpu, D, Hv, Ho, Nv, No):
    """z = (W1 x) + b1 of the training forward is a k-ordered fmaf chain from +0 and one addition on both sides: the same bits."""
    c = ec.train_case(D, Hv, Ho, Nv, No)
    out = {}
    for dev in (CPU, gpu):
        w = ec.packed(dev, c["vp"], c["op"])
        out[dev.type] = ec.direct_forward(dev, w, c["ctx"].to(dev), c["pairs"].to(dev), c["offsets"].to(dev), c["K"], True,
                                          ec.seed_arg(c["seed"]), c["pv"], c["po"])
    z_h, z_d = out["cpu"][2], out["cuda"][2].cpu()
    diff = float((z_h.double() - z_d.double()).abs().max())
    print(f"z bits D={D} Hv={Hv} Ho={Ho}: elements that differ {int((z_h.view(torch.int32) != z_d.view(torch.int32)).sum())} of "
          f"{z_h.numel()}, largest difference {diff:.3e}")
    assert _bits_equal(z_h, z_d)
    assert torch.equal(out["cpu"][3], out["cuda"][3].cpu()) and torch.equal(out["cpu"][4], out["cuda"][4].cpu())


def _premise_probe(dev):
    """K = 1: db1 is dz[0].  dOut one-hot and W2 powers of two make dA exact, so dz must have the bits of 0, 0.5 M dA and M dA for
    z = -(16 + |n|), 0 and +(16 + |n|): gelu' is 0, 0.5 and 1 there on any correct fp32 libm.  Returns the mismatching columns."""
    D, Hv, Ho, Nv, No = ec.ROW_SHAPE
    pv, po = ec.P_MAIN
    H = Hv + Ho
    vp, op = tc.make_train_heads(D, Hv, Ho, 901, pv, po, Nv, No)
    with torch.no_grad():
        for head in (vp, op):
            rows = torch.arange(head[-1].in_features)
            head[-1].weight.copy_((2.0 ** ((rows % 7) - 3).double()).float()[None, :].expand_as(head[-1].weight))
    w = ec.packed(dev, vp, op)
    cls = torch.arange(H) % 3
    mag = 16.0 + torch.randn(H, generator=torch.Generator().manual_seed(902)).abs()
    z = torch.where(cls == 0, torch.zeros(H), torch.where(cls == 1, mag, -mag))[None, :].contiguous()
    dlv, dof = torch.zeros(1, Nv), torch.zeros(1, No)
    dlv[0, 5], dof[0, No - 1] = 1.0, 1.0
    pairs, offsets = common.pack_rows([(0, 2, 7)])
    seed = ec.seed_arg(903)
    ctx = common.make_ctx(D, 1.0, 904)
    outs = ec.direct_backward(dev, w, dlv.to(dev), dof.to(dev), z.to(dev), ctx.to(dev), pairs.to(dev), offsets.to(dev), 1, seed, pv, po)
    keep = tc.mask_of(903, 1, Hv, Ho, pv, po)[0]
    dA = torch.cat([vp[-1].weight[5], op[-1].weight[No - 1]]).detach()
    scale = torch.cat([torch.full((Hv,), 1.0 / (1.0 - pv), dtype=torch.float64), torch.full((Ho,), 1.0 / (1.0 - po), dtype=torch.float64)]).float()
    gp = torch.tensor([0.5, 1.0, 0.0])[cls]
    want = torch.where(keep, (dA * scale) * gp, torch.zeros(H))            # fp32 multiplications, no transcendental
    assert float(want.abs().max()) > 0 and int((want == 0).sum()) > 0
    got = outs[2].cpu()
    return (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten().tolist(), got, want


def test_libm_free_premise_cpu():
    bad, got, want = _premise_probe(CPU)
    assert not bad, (bad, got[bad], want[bad])


@pytest.fixture(scope="module")
def premise(gpu):
    """The premise of the libm-free comparisons on the device; a failure is the finding (the device libm breaks it)."""
    bad_h, _, _ = _premise_probe(CPU)
    bad_d, got, want = _premise_probe(gpu)
    return None if not (bad_h or bad_d) else f"gelu' of |z| >= 16 or 0 is not exact: host columns {bad_h}, device columns {bad_d}"


@pytest.mark.gpu
def test_libm_free_premise_gpu(gpu):
    bad, got, want = _premise_probe(gpu)
    assert not bad, (bad, got[bad], want[bad])


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No,K", BIT_CASES)
def test_backward_bits_with_libm_free_z_gpu(gpu, premise, D, Hv, Ho, Nv, No, K):
    """semicrf_attribute_heads_bwd on the device and its host mirror on a z that needs no libm accuracy: dctx, dW1, db1, dW2, db2 the
    same bits -- the order of operations of include/semicrf_hip.h, chain for chain."""
    if premise:
        pytest.skip(premise)
    pv, po = ec.P_MAIN
    c = ec.train_case(D, Hv, Ho, Nv, No, K=K)
    z = ec.libm_free_z(K, Hv + Ho, 950 + D)
    seed = ec.seed_arg(c["seed"])
    out = {}
    for dev in (CPU, gpu):
        w = ec.packed(dev, c["vp"], c["op"])
        out[dev.type] = ec.direct_backward(dev, w, c["dlv"].to(dev), c["dof"].to(dev), z.to(dev), c["ctx"].to(dev), c["pairs"].to(dev),
                                           c["offsets"].to(dev), K, seed, pv, po)
    bad = []
    for name, h, d in zip(("dctx", "dW1", "db1", "dW2", "db2"), out["cpu"], out["cuda"]):
        d = d.cpu()
        assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0, name
        n = int((h.view(torch.int32) != d.view(torch.int32)).sum())
        print(f"backward bits D={D} Hv={Hv} Ho={Ho} Nv={Nv} No={No} K={K} {name}: elements that differ {n} of {h.numel()}, largest "
              f"difference {float((h.double() - d.double()).abs().max()):.3e}")
        if n:
            bad.append(name)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No", ec.GRID)
def test_layer2_bits_with_libm_free_z_gpu(gpu, premise, D, Hv, Ho, Nv, No):
    """Heads whose b1 is +20 on even and -20 on odd columns: every |z| >= 16, gelu(z) is z or -0 without any libm accuracy, and the
    eval-mode outputs on the device have the bits of the host mirror's (layer 2: slice chains, slices ascending, b2 last)."""
    if premise:
        pytest.skip(premise)
    c = ec.eval_case(D, Hv, Ho, Nv, No)
    vp, op = copy.deepcopy(c["vp"]), copy.deepcopy(c["op"])
    with torch.no_grad():
        for head in (vp, op):
            n = head[0].out_features
            head[0].bias.copy_(torch.where(torch.arange(n) % 2 == 0, torch.full((n,), 20.0), torch.full((n,), -20.0)))
    out = {}
    for dev in (CPU, gpu):
        w = ec.packed(dev, vp, op)
        args = (c["ctx"].to(dev), c["pairs"].to(dev), c["offsets"].to(dev), c["K"])
        z = ec.direct_forward(dev, w, *args, True)[2]
        assert float(z.abs().min()) >= 16.0
        out[dev.type] = ec.direct_forward(dev, w, *args, False)[:2]
    for name, h, d in zip(("logitsVelocity", "ofLogits"), out["cpu"], out["cuda"]):
        d = d.cpu()
        assert bool(torch.isfinite(h).all()) and float(h.abs().max()) > 0
        n = int((h.view(torch.int32) != d.view(torch.int32)).sum())
        print(f"layer 2 bits D={D} Hv={Hv} Ho={Ho} Nv={Nv} No={No} {name}: elements that differ {n} of {h.numel()}, largest difference "
              f"{float((h.double() - d.double()).abs().max()):.3e}")
        assert n == 0, name


# ---- 6. nothing unwritten is read, nothing due is left unwritten (device only) ---------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("D,Hv,Ho,Nv,No,K", [ec.GRID[0] + (common.K_GATE,), ec.ROW_SHAPE + (513,)])
def test_poisoned_workspace_and_outputs_gpu(gpu, D, Hv, Ho, Nv, No, K):
    """The eval forward, the training forward and the backward, once as attributes calls them and once with the workspace 4 KiB larger
    and full of NaN and every output pre-filled with NaN (-1 for the index outputs): all finite, the same bits."""
    c = ec.train_case(D, Hv, Ho, Nv, No, K=K)
    w = ec.packed(gpu, c["vp"], c["op"])
    ctx, pairs, offsets, dlv, dof = (c[k].to(gpu) for k in ("ctx", "pairs", "offsets", "dlv", "dof"))
    seed, pv, po = ec.seed_arg(c["seed"]), c["pv"], c["po"]
    runs = []
    for poison in (False, True):
        ev = ec.direct_forward(gpu, w, ctx, pairs, offsets, K, False, poison=poison)
        tr = ec.direct_forward(gpu, w, ctx, pairs, offsets, K, True, seed, pv, po, poison=poison)
        bw = ec.direct_backward(gpu, w, dlv, dof, tr[2], ctx, pairs, offsets, K, seed, pv, po, poison=poison)
        runs.append(list(ev) + list(tr) + list(bw))
    names = ("eval lv", "eval of", "eval sym", "eval sc", "lv", "of", "z", "sym", "sc", "dctx", "dW1", "db1", "dW2", "db2")
    for name, a, b in zip(names, *runs):
        if a.dtype == torch.int64:
            assert bool((b >= 0).all()) and torch.equal(a, b), name
        else:
            assert bool(torch.isfinite(b).all()), name
            assert _bits_equal(a, b), name


# ---- 7. ctx views whose data pointer is not 16-byte aligned -----------------------------------------------------------------------------
def _check_misaligned(dev):
    """ctx as a view with a row stride of D + 4 floats (a multiple of four) and a storage offset of 1, 2 and 3 floats: read in place
    (no copy in Python: attributes keeps the view's strides and offset), the 16-byte loads refused by the pointer test of the
    launchers, and the bits of the contiguous run; dctx in the view's shape."""
    from transkun_amd import attributes
    D, Hv, Ho, Nv, No = ec.ROW_SHAPE
    c = ec.train_case(D, Hv, Ho, Nv, No)
    K = c["K"]
    lv, of, grads = tc.run_op(dev, c)
    vp, op = copy.deepcopy(c["vp"]).to(dev).train(), copy.deepcopy(c["op"]).to(dev).train()
    vpe, ope = copy.deepcopy(vp).eval(), copy.deepcopy(op).eval()
    pairs, offsets, dlv, dof = (c[k].to(dev) for k in ("pairs", "offsets", "dlv", "dof"))
    ev = common.fused(c["ctx"].to(dev), pairs, offsets, vpe, ope, K)
    for off in (1, 2, 3):
        big = torch.full((common.N_SEG, common.N_SYM, T, D + 4), 1e30, device=dev)
        big[..., off:off + D] = c["ctx"].to(dev)
        view = big[..., off:off + D]
        assert view.stride(2) == D + 4 and view.storage_offset() == off and view.data_ptr() % 16 == 4 * off
        ev2 = common.fused(view, pairs, offsets, vpe, ope, K)
        assert _bits_equal(ev2[0], ev[0]) and _bits_equal(ev2[1], ev[1]) and torch.equal(ev2[2], ev[2]) and torch.equal(ev2[3], ev[3]), off
        view = view.requires_grad_()
        lv2, of2, _, _ = attributes.attribute_heads_train(view, pairs, offsets, vp, op, K, seed=c["seed"])
        g2 = torch.autograd.grad([lv2, of2], [view] + tc.params_of(vp, op), [dlv, dof])
        assert g2[0].shape == view.shape
        assert _bits_equal(lv2.detach(), lv) and _bits_equal(of2.detach(), of), off
        for name, a, b in zip(tc.NAMES, grads, g2):
            assert _bits_equal(a, b), (off, name)


def test_misaligned_views_cpu():
    _check_misaligned(CPU)


@pytest.mark.gpu
def test_misaligned_views_gpu(gpu):
    _check_misaligned(gpu)
