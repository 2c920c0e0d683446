"""The attribute-head training loss: transkun_amd.attributes.attribute_log_prob (csrc/attr_loss.hip on the GPU, the host kernels of
csrc/cpu_ops.cpp on CPU tensors), pack_attribute_targets and SegmentTranscriber.log_prob.

Every numerical case runs on the CPU path (unmarked) and on the device (marked gpu).  The tolerance rule (attr_loss_common.check_bound):
against the float64 yardstick the op may err by the larger of (a) what the torch-fp32 route -- the reference's own torch calls --
errs on the same family of inputs and (b) a floor of 8 eps32 max(1, |value|) per row term, rows adding linearly per chain.

Measured (worst |error| against the yardstick; op on the MI355X / op on the CPU path / torch-fp32 route on the CPU): see DESIGN.md
section 3, "Attribute-head loss"."""
import inspect
import re

import numpy as np
import pytest
import torch

import attr_loss_common as common
from attr_loss_common import (test_yardstick_matches_continuous_bernoulli_float64,  # noqa: F401  (collected here: the yardstick's own tests)
                              test_yardstick_matches_golden_float64)  # noqa: F401
from conftest import load_golden


def _op(*a, **kw):
    from transkun_amd import attributes
    return attributes.attribute_log_prob(*a, **kw)


def _run(case, gout, base=None):
    """(out, dLogitsVelocity, dOfLogits, dbase) of the op for (out * gout).sum()"""
    lv, of, vel, refined, pres, offsets = case
    lv = lv.clone().requires_grad_(); of = of.clone().requires_grad_()
    b = None if base is None else base.clone().requires_grad_()
    out = _op(lv, of, vel, refined, pres, offsets, base=b)
    (out * gout).sum().backward()
    return out.detach(), lv.grad, of.grad, None if b is None else b.grad


# ---- families of rows ----------------------------------------------------------------------------------------------------
def _check_family(name, dev):
    case = common.family(name, dev)
    lv, of, vel, refined, pres, offsets = case
    C = offsets.numel() - 1
    gout = torch.ones(C, device=dev)
    y = common.yardstick(*case, gout=gout)
    t_out, t_dlv, t_dof = common.torch_route_grads(*case, gout)
    out, dlv, dof, _ = _run(case, gout)
    assert out.dtype == torch.float32 and out.shape == (C,)
    common.check_bound(f"{name} [{dev.type}] value", out, y["out"], t_out, common.value_floor(y, offsets))
    common.check_bound(f"{name} [{dev.type}] dLogitsVelocity", dlv, y["dLogitsVelocity"], t_dlv, common.grad_floor(y["dLogitsVelocity"]))
    common.check_bound(f"{name} [{dev.type}] dOfLogits", dof, y["dOfLogits"], t_dof, common.grad_floor(y["dOfLogits"]))
    if name == "clamp":
        # the clamped definition, not the closed form: beyond l* the value logit's derivative is x - sigmoid(l) alone
        x = refined.double() * 0.99 + 0.5
        l = of[:, :2].double()
        far = l.abs() > common.LSTAR
        assert bool(far.any())
        assert float((dof[:, :2].double() - (x - torch.sigmoid(l)))[far].abs().max()) <= common.FLOOR


@pytest.mark.parametrize("name", common.FAMILIES)
def test_family_cpu(name):
    _check_family(name, torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", common.FAMILIES)
def test_family_gpu(gpu, name):
    _check_family(name, gpu)


# ---- shapes, determinism, cotangents ---------------------------------------------------------------------------------------
def _check_shape(name, dev):
    lv, of, vel, refined, pres, offsets, base, gout = common.shape_case(name, dev)
    case = (lv, of, vel, refined, pres, offsets)
    C, K = offsets.numel() - 1, lv.shape[0]
    if K == 0:
        out = _op(*case, base=base)
        assert torch.equal(out, base) and out.data_ptr() != base.data_ptr()
        assert torch.equal(_op(*case), torch.zeros(C, device=dev))
        b = base.clone().requires_grad_()
        lvg = lv.clone().requires_grad_()
        (_op(lvg, of, vel, refined, pres, offsets, base=b) * gout).sum().backward()
        assert torch.equal(b.grad, gout) and lvg.grad.shape == (0, 128)
        return
    for g, tag in ((torch.ones(C, device=dev), "ones"), (gout, "random"), (gout * (torch.arange(C, device=dev) % 3 != 1), "zeros on some chains")):
        y = common.yardstick(*case, base=base, gout=g)
        t_out, t_dlv, t_dof = common.torch_route_grads(*case, g, base=base)
        out, dlv, dof, dbase = _run(case, g, base)
        rows = common.scatter_index(offsets)
        # base is added last, in fp32: one more rounding of the result
        floor = common.value_floor(y, offsets) + common.EPS32 * y["out"].abs()
        common.check_bound(f"{name} [{dev.type}] g={tag} value", out, y["out"], t_out, floor)
        common.check_bound(f"{name} [{dev.type}] g={tag} dLogitsVelocity", dlv, y["dLogitsVelocity"], t_dlv, common.grad_floor(y["dLogitsVelocity"], g[rows]))
        common.check_bound(f"{name} [{dev.type}] g={tag} dOfLogits", dof, y["dOfLogits"], t_dof, common.grad_floor(y["dOfLogits"], g[rows]))
        assert torch.equal(dbase, g)                                          # dbase == g, bit for bit
        if tag != "ones":
            dead = (g == 0)[rows]
            assert float(dlv[dead].abs().max() if dead.any() else 0.0) == 0.0 and float(dof[dead].abs().max() if dead.any() else 0.0) == 0.0
    # an expanded scalar, as -logp.sum(-1).mean() hands down (stride 0)
    lv1 = lv.clone().requires_grad_(); of1 = of.clone().requires_grad_()
    (-_op(lv1, of1, vel, refined, pres, offsets, base=base).sum() / 4).backward()
    _, dlv2, dof2, _ = _run(case, torch.full((C,), -0.25, device=dev), base)
    assert torch.equal(lv1.grad, dlv2) and torch.equal(of1.grad, dof2)
    # two runs: the same bits
    out1, dlv1, dof1, _ = _run(case, gout, base)
    out2, dlv2, dof2, _ = _run(case, gout, base)
    assert torch.equal(out1, out2) and torch.equal(dlv1, dlv2) and torch.equal(dof1, dof2)
    # without base: the bare sums; empty chains give exactly 0
    bare = _op(*case)
    counts = offsets[1:] - offsets[:-1]
    assert float(bare[counts == 0].abs().max() if (counts == 0).any() else 0.0) == 0.0
    assert torch.equal(out1[counts == 0], base[counts == 0])
    # every chain alone: the same bits as in the batch (value and gradients)
    off = offsets.tolist()
    step = max(1, C // 40)                                                    # (all chains of the small cases, every 9th of C = 360)
    for c in sorted(set(range(0, C, step)) | {C - 1}):
        b, e = off[c], off[c + 1]
        one = (lv[b:e], of[b:e], vel[b:e], refined[b:e], pres[b:e], torch.tensor([0, e - b], dtype=torch.int32, device=dev))
        o, dl, do, _ = _run(one, gout[c:c + 1], base[c:c + 1])
        assert torch.equal(o, out1[c:c + 1]) and torch.equal(dl, dlv1[b:e]) and torch.equal(do, dof1[b:e]), c


@pytest.mark.parametrize("name", list(common.SHAPES))
def test_shape_cpu(name):
    _check_shape(name, torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(common.SHAPES))
def test_shape_gpu(gpu, name):
    _check_shape(name, gpu)


def _check_second_backward_raises(dev):
    lv, of, vel, refined, pres, offsets, base, gout = common.shape_case("C5", dev)
    lv = lv.clone().requires_grad_()
    out = _op(lv, of, vel, refined, pres, offsets, base=base)
    (g,) = torch.autograd.grad((out * gout).sum(), lv, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    out = _op(lv, of, vel, refined, pres, offsets, base=base)
    out.sum().backward()
    with pytest.raises(RuntimeError):
        out.sum().backward()                                                  # the graph's buffers are gone


def test_second_backward_raises_cpu():
    _check_second_backward_raises(torch.device("cpu"))


@pytest.mark.gpu
def test_second_backward_raises_gpu(gpu):
    _check_second_backward_raises(gpu)


def test_out_of_range_velocity_is_nan_not_a_fault():
    lv, of, vel, refined, pres, offsets, base, gout = common.shape_case("C5", "cpu")
    vel = vel.clone(); vel[1] = 128
    out = _op(lv, of, vel, refined, pres, offsets)
    assert bool(torch.isnan(out[1])) and bool(torch.isfinite(out[3]))


# ---- targets ---------------------------------------------------------------------------------------------------------------
def test_pack_attribute_targets():
    from transkun_amd.attributes import pack_attribute_targets
    vel = [[[3, 127], []], [[0], [64]]]                                           # per segment, per symbol
    refined = [[[(0.25, -0.5), (0.0, 0.5)], []], [[(-0.125, 0.125)], [(0.5, 0.5)]]]
    presence = [[[(True, False), (True, True)], []], [[(False, False)], [(True, True)]]]
    v, r, p = pack_attribute_targets(vel, refined, presence, 4, "cpu")
    assert v.dtype == torch.int32 and v.tolist() == [3, 127, 0, 64]
    assert r.dtype == torch.float32 and r.tolist() == [[0.25, -0.5], [0.0, 0.5], [-0.125, 0.125], [0.5, 0.5]]
    assert p.dtype == torch.float32 and p.tolist() == [[1.0, 0.0], [1.0, 1.0], [0.0, 0.0], [1.0, 1.0]]
    # flat sequences and tensors
    v2, r2, p2 = pack_attribute_targets([3, 127, 0, 64], torch.tensor(r.tolist()), [(1, 0), (1, 1), (0, 0), (1, 1)], 4, "cpu")
    assert torch.equal(v, v2) and torch.equal(r, r2) and torch.equal(p, p2)
    v3, _, _ = pack_attribute_targets(torch.tensor([3.0, 127.0, 0.0, 64.0]), r, p, 4, "cpu")
    assert torch.equal(v, v3)
    for bad in ([3, 128, 0, 64], [3, -1, 0, 64], [3, 1.5, 0, 64]):
        with pytest.raises(ValueError, match="0..127"):
            pack_attribute_targets(bad, r, p, 4, "cpu")
    with pytest.raises(ValueError, match="target intervals"):
        pack_attribute_targets([3, 127, 0], r, p, 4, "cpu")
    with pytest.raises(ValueError, match="target intervals"):
        pack_attribute_targets([3, 127, 0, 64], r[:3], p, 4, "cpu")
    with pytest.raises(ValueError, match="target intervals"):
        pack_attribute_targets([3, 127, 0, 64], r, p, 5, "cpu")
    e = pack_attribute_targets([], [], [], 0, "cpu")
    assert e[0].shape == (0,) and e[1].shape == (0, 2) and e[2].shape == (0, 2)


@pytest.mark.gpu
def test_pack_attribute_targets_gpu(gpu):
    from transkun_amd.attributes import pack_attribute_targets
    v, r, p = pack_attribute_targets([3, 127, 0, 64], [(0.25, -0.5), (0.0, 0.5), (-0.125, 0.125), (0.5, 0.5)], [(1, 0), (1, 1), (0, 0), (1, 1)], 4, gpu)
    assert v.is_cuda and v.tolist() == [3, 127, 0, 64] and r[3].tolist() == [0.5, 0.5] and p[0].tolist() == [1.0, 0.0]
    with pytest.raises(ValueError, match="0..127"):
        pack_attribute_targets([3, 128, 0, 64], r.cpu(), p.cpu(), 4, gpu)


# ---- the reference's numbers -------------------------------------------------------------------------------------------------
def _golden_case(dev):
    g = load_golden("attr_loss_small")
    t = [torch.from_numpy(g[k]).to(dev) for k in ("logitsVelocity", "ofLogits", "velocity", "ofRefined", "ofPresence")]
    return g, tuple(t) + (torch.from_numpy(g["offsets"].astype(np.int32)).to(dev),)


def _check_golden(dev):
    """The stored head outputs and targets give the reference's per-chain attribute sums and both gradients of
    -logProb.sum(-1).mean().  Bound: the golden's own fp32-vs-float64 error, or the floor, whichever is larger."""
    g, case = _golden_case(dev)
    N, P = int(g["meta"][0]), int(g["meta"][1])
    offsets = case[-1]
    y = common.yardstick(*case)
    gout = torch.full((N * P,), -1.0 / N, device=dev)
    out, dlv, dof, _ = _run(case, gout)
    # the torch-fp32 route's numbers here ARE the golden's fp32 arrays: the rule, against the golden's float64 arrays
    for name, got, k32, k64, floor in (("attr", out, "attr", "attr64", common.value_floor(y, offsets).cpu()),
                                       ("dLogitsVelocity", dlv, "dLogitsVelocity", "dLogitsVelocity64", None),
                                       ("dOfLogits", dof, "dOfLogits", "dOfLogits64", None)):
        want = torch.from_numpy(g[k64]).reshape(got.shape)
        common.check_bound(f"golden [{dev.type}] {name}", got.cpu(), want, torch.from_numpy(g[k32]).reshape(got.shape),
                           floor if floor is not None else common.grad_floor(want))
    # and with the reference's CRF term as base: its logProb [N, P]
    full = _op(*case, base=torch.from_numpy(g["crf"]).to(dev)).view(N, P).cpu()
    want = torch.from_numpy(g["crf"]).double() + torch.from_numpy(g["attr64"]).view(N, P)
    bound = (common.value_floor(y, offsets).cpu().view(N, P) + common.EPS32 * want.abs()).clamp(min=float(np.abs(g["attr"] - g["attr64"]).max()))
    assert bool(((full.double() - want).abs() <= bound).all())
    assert float((full - torch.from_numpy(g["logProb"])).abs().max()) <= 2 * float(bound.max())


def test_golden_cpu():
    _check_golden(torch.device("cpu"))


@pytest.mark.gpu
def test_golden_gpu(gpu):
    _check_golden(gpu)


# ---- end to end: SegmentTranscriber.log_prob -----------------------------------------------------------------------------------
def _crf_logprob_tolerance():
    """The relative tolerance test_segment_logprob_vs_reference holds the CRF's logProb to (read from that test, not copied)."""
    import test_gpu_parity
    src = inspect.getsource(test_gpu_parity.test_segment_logprob_vs_reference)
    m = re.search(r'rel_err\(lp\.detach\(\)\.cpu\(\)\.numpy\(\), g\["logProb"\]\) < ([0-9.eE+-]+)', src)
    assert m, "test_segment_logprob_vs_reference no longer states its logProb tolerance in the expected form"
    return float(m.group(1)), test_gpu_parity.rel_err


@pytest.mark.gpu
def test_segment_transcriber_log_prob(gpu):
    """SegmentTranscriber.log_prob at the golden's shape, eval mode: against the same method on the torch-call route (identical head
    outputs: only the op differs), against the reference's logProb [N, P], and the gradients of both routes."""
    g, case = _golden_case(gpu)
    N, P = int(g["meta"][0]), int(g["meta"][1])
    model, ctx0 = common.golden_transcriber(gpu)
    batch, vel, refined, pres = common.golden_targets(g)
    offsets = case[-1]

    def run(route):
        model.zero_grad()
        ctx = ctx0.clone().requires_grad_()
        lp = model.log_prob(ctx, batch, vel, refined, pres, attributeRoute=route)
        assert lp.shape == (N, P)
        (-lp.sum(-1).mean()).backward()
        return lp.detach(), ctx.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    lp_f, dctx_f, dpar_f = run("fused")
    lp_t, dctx_t, dpar_t = run("torch")
    # the CRF term alone (no target interval anywhere)
    empty = [[[] for _ in range(P)] for _ in range(N)]
    crf_only = model.log_prob(ctx0, empty, [], [], [])
    assert crf_only.shape == (N, P) and bool(torch.isfinite(crf_only).all())
    # (1) the two routes: the head outputs are the same bits, so the difference is the op's against the torch calls' -- each within
    # the rule of the yardstick, which needs the head outputs: recomputed here exactly as log_prob does
    from transkun_amd import attributes
    import importlib
    nsci = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    with torch.no_grad():
        flat = [s for seg in batch for s in seg]
        pairs, off2 = nsci.pack_intervals(flat, ctx0.shape[2], N * P, gpu)
        x, _, _ = attributes.attribute_input_packed(ctx0, pairs, off2, pairs._semicrf_K)
        lv, ofl = model.velocityPredictor(x), model.refinedOFPredictor(x)
    assert torch.equal(off2, offsets)
    targets = (case[2], case[3], case[4], offsets)
    crf = lp_f.view(-1) - attributes.attribute_log_prob(lv, ofl, *targets)          # not exact; only sizes the floor's last term
    y = common.yardstick(lv, ofl, *targets)
    a_f = attributes.attribute_log_prob(lv, ofl, *targets)
    a_t = attributes.attribute_log_prob_torch(lv, ofl, *targets)
    e_f, e_t = common.check_bound("log_prob attr part", a_f, y["out"], a_t, common.value_floor(y, offsets))
    bound = torch.maximum(common.value_floor(y, offsets), torch.full_like(y["out"], e_t)) + e_t + 2 * common.EPS32 * (crf.abs().double() + y["out"].abs())
    diff = (lp_f.view(-1).double() - lp_t.view(-1).double()).abs()
    print(f"log_prob fused vs torch route: {float(diff.max()):.3e}")
    assert bool((diff <= bound).all())
    # (2) the reference's logProb: the CRF term's tolerance + twice what the torch-call route's attribute part differs from the golden's
    # (the device's GEMMs of the heads are not the CPU's)
    crf_tol, rel_err = _crf_logprob_tolerance()
    attr_t = float((a_t.cpu().double() - torch.from_numpy(g["attr"]).double()).abs().max())
    want = g["logProb"].astype(np.float64)
    tol = crf_tol * np.maximum(np.abs(want), 1.0) + 2 * attr_t
    err = np.abs(lp_f.cpu().numpy().astype(np.float64) - want)
    print(f"log_prob vs reference: {err.max():.3e} (CRF tolerance {crf_tol:g} relative, torch route's attribute part vs golden {attr_t:.3e})")
    assert (err <= tol).all(), (err.max(), tol.min())
    # without a target interval: the CRF term of the empty paths itself -- the fused node's bits, and the reference's numbers on the
    # chains whose target is empty in the golden too
    from transkun_amd import fused as fused_mod
    assert torch.equal(crf_only.detach().view(-1), fused_mod.scorer_crf_logprob(model.scorer, ctx0, [[] for _ in range(N * P)]).detach())
    none = (offsets[1:] == offsets[:-1]).cpu().numpy()
    assert none.any() and rel_err(crf_only.detach().cpu().numpy().reshape(-1)[none], g["crf"].reshape(-1)[none]) < crf_tol
    # (3) gradients w.r.t. ctx and every parameter.  The two routes differ in the cotangents they hand to the heads (dLogitsVelocity,
    # dOfLogits: each within the rule, the torch calls being off by 2e-4 at these inputs) pushed through the same backward.  The rule
    # once more, per tensor and relative to its largest entry, against a third run whose attribute part is the float64 yardstick
    # differentiated by autograd: the op's route may be off by what the torch route is off, or by the floor -- the cotangents' own
    # floor of 8 eps32, grown by the square root of the K * max(H, 3 D) products a gradient entry accumulates in fp32.
    from transkun_amd import fused

    def run_yardstick():
        model.zero_grad()
        ctx = ctx0.clone().requires_grad_()
        p2, o2 = nsci.pack_intervals(flat, ctx0.shape[2], N * P, gpu)
        base = fused.scorer_crf_logprob(model.scorer, ctx, flat, packed=(p2, o2))
        xx, _, _ = attributes.attribute_input_packed(ctx, p2, o2, p2._semicrf_K)
        t = common.yardstick_rows(model.velocityPredictor(xx).double(), model.refinedOFPredictor(xx).double(), case[2], case[3], case[4])
        lp = base.double().index_add(0, common.scatter_index(offsets), t[0] + t[1] + t[2]).view(N, P)
        (-lp.sum(-1).mean()).backward()
        return ctx.grad.clone(), {n: p.grad.clone() for n, p in model.named_parameters()}

    dctx_y, dpar_y = run_yardstick()
    c = common.GOLDEN_CASE
    floor_rel = common.FLOOR * (lv.shape[0] * max(c["H"], 3 * c["D"])) ** 0.5

    def close(a, b, want, what):
        scale = float(want.abs().max()) + 1e-30
        e_f, e_t = float((a - want).abs().max()) / scale, float((b - want).abs().max()) / scale
        print(f"log_prob gradient {what}: op route {e_f:.3e}  torch route {e_t:.3e}  floor {floor_rel:.3e} (relative to the largest entry)")
        assert e_f <= max(e_t, floor_rel), (what, e_f, e_t)
    close(dctx_f, dctx_t, dctx_y, "ctx")
    for n in dpar_y:
        close(dpar_f[n], dpar_t[n], dpar_y[n], n)


@pytest.mark.gpu
def test_graph_capture_replay_matches_eager(gpu):
    """Forward + backward of the op captured into a graph on one stream and replayed: the same bits as the eager call."""
    lv, of, vel, refined, pres, offsets, base, gout = common.shape_case("C360", gpu)
    case = (lv, of, vel, refined, pres, offsets)
    out_e, dlv_e, dof_e, db_e = _run(case, gout, base)
    lvg = lv.clone().requires_grad_(); ofg = of.clone().requires_grad_(); bg = base.clone().requires_grad_()
    s = torch.cuda.Stream(device=gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        for _ in range(2):                                                    # warm-up on the side stream (allocator, lazy loads)
            o = _op(lvg, ofg, vel, refined, pres, offsets, base=bg)
            grads = torch.autograd.grad((o * gout).sum(), (lvg, ofg, bg))
    torch.cuda.current_stream(gpu).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o = _op(lvg, ofg, vel, refined, pres, offsets, base=bg)
        grads = torch.autograd.grad((o * gout).sum(), (lvg, ofg, bg))
    o.zero_()
    for t in grads:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o.detach(), out_e) and torch.equal(grads[0], dlv_e) and torch.equal(grads[1], dof_e) and torch.equal(grads[2], db_e)
