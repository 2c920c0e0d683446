"""The memory contract of the training step's and the readout's ops (include/semicrf_hip.h): semicrf_adabelief_step,
semicrf_grad_sqnorm, semicrf_clip_from_history, semicrf_attribute_loss_fwd / _bwd and semicrf_attribute_decode -- the companion of
tests/test_memory_contract.py, which does the same for the semi-CRF layer.

Every case runs on the CPU path (the shim's host kernels, unmarked) and on the device (@pytest.mark.gpu).  Calls go to
`_lib.ops().<op>` directly.  All operands, outputs and scalars of a case are carved out of ONE guard-band arena
(tests/arena_common.py), at chosen address phases modulo 16 and with guards of at least 4 KiB between them, so a stray access is a
failed assertion and never a fault.  Every case asserts
  * guards intact, read-only operands unchanged (Arena.check);
  * every element the header says is written holds the bits of the same call on ordinary tensors (Plain) and not the pattern;
  * every other element of an output still holds the pattern: output carves are a few elements longer than the call needs;
  * a NaN-pattern arena and a FLT_MAX-pattern arena give the same bits (nothing outside the operands reaches a result).

A  semicrf_adabelief_step: the 4-byte kernel (any buffer off 16 bytes) against the 16-byte one, 1 to 8 groups with boundaries at every
   position inside a 4-element access, both grid-stride trips; the bits of the host kernel, and every element against the float64
   yardstick of tests/optimizer_common.py under its own bound.
B  semicrf_grad_sqnorm: every head / tail length of the float4 body, one and many workgroups, the strided trip beyond 256 partials; an
   integer-valued family whose sum of squares is exact in any order, and two float families against math.fsum.
C  semicrf_clip_from_history: the sort at every count where its shape changes, full rings with a head, the written set of each mode.
D  the attribute loss and readout: written sets at K % 4 != 0 and K == 0, the unused output, and the 8-byte rule of logitsVelocity.

No tolerance is new here: every bound is one of optimizer_common, attr_loss_common or attr_decode_common, or exact equality.
Measured figures: DESIGN.md section 4, "The memory contract of the step's ops".
"""
import ctypes
import math
from unittest import mock

import numpy as np
import pytest
import torch

import arena_common as ac
import attr_decode_common as adc
import attr_loss_common as alc
import optimizer_common as oc
from transkun_amd import _lib, synth
from transkun_amd.optim import adabelief_scalars

CPU = torch.device("cpu")
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
GUARD = 4096
EXTRA = 5                                        # elements an output carve is longer than the call needs


def _dev(request, which):
    return CPU if which == "cpu" else request.getfixturevalue("gpu")


DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


# ---- one execution of a case ------------------------------------------------------------------------------------------------------------
class Run:
    """Where a case's tensors come from (an arena, its sizer or torch's allocator).  inp: a read-only operand (Arena.check finds it
    unchanged); out: an output of n elements holding the pattern, optionally with the first elements set (an in/out buffer)."""

    def __init__(self, A):
        self.A, self.outs = A, {}

    def inp(self, name, src, phase=0):
        return self.A.put(name, src, phase)

    def out(self, name, n, dtype=F32, phase=0, init=None):
        t = self.A.carve(name, (n,), dtype, phase)
        if self.A.real:
            snap = t.clone()
            if init is not None:
                t[:init.numel()].copy_(init.reshape(-1))
            self.outs[name] = (t, snap)
        return t

    def call(self, fn):
        return self.A.call(fn)


def _words(t):
    """[numel, words per element] int32 on the host (bytes: one column)."""
    t = t.detach().cpu().contiguous()
    if t.dtype == U8:
        return t.reshape(-1, 1).to(I32)
    return t.view(I32).reshape(t.numel(), -1)


class Result:
    """An output after the call: its words, the pattern words it held when it was carved, the written set, the tensor on the host."""

    def __init__(self, t, snap, mask):
        self.t = t.detach().cpu().clone()
        self.words, self.pattern, self.mask = _words(t), _words(snap), mask
        assert mask.dtype == torch.bool and mask.numel() == t.numel()


def _head(n, k):
    return torch.arange(n) < k


def _execute(case, dev, pattern, plain=False):
    """case(Run) carves, calls and returns {output name: written set}.  Returns {name: Result}."""
    if plain:
        A = ac.Plain(pattern, dev)
        r = Run(A)
        masks = case(r)
    else:
        last = {}

        def go(arena):
            last["r"] = Run(arena)
            last["m"] = case(last["r"])
        A, _ = ac.run_in_arena(go, GUARD, pattern, dev)
        r, masks = last["r"], last["m"]
    A.check()
    if dev.type == "cuda":
        assert _lib.device_status() == 0
    assert set(masks) == set(r.outs)
    return {n: Result(t, snap, masks[n]) for n, (t, snap) in r.outs.items()}


def _check_written(res, ref, what):
    """Outside the written set: the pattern.  Inside: not the pattern, and (ref given) the bits of the reference run."""
    for name, o in res.items():
        changed = (o.words != o.pattern).any(-1)
        m = o.mask
        if bool(changed[~m].any()):
            i = int(torch.nonzero(changed & ~m)[0])
            raise AssertionError(f"{what}: `{name}`: {int(changed[~m].sum())} elements outside the written set were written (first: {i})")
        if not bool(changed[m].all()):
            i = int(torch.nonzero(~changed & m)[0])
            raise AssertionError(f"{what}: `{name}`: element {i}, which the call must write, still holds the pattern")
        if ref is not None:
            assert torch.equal(m, ref[name].mask), f"{what}: `{name}`: the written sets differ"
            a, b = o.words[m], ref[name].words[m]
            if not torch.equal(a, b):
                i = int(torch.nonzero((a != b).any(-1))[0])
                raise AssertionError(f"{what}: `{name}`: written element {i} of {int(m.sum())} differs from the reference run")


def _contract(case, dev, what, plain=None, compare_plain=True):
    """The four assertions of the module docstring for one case.  plain: the reference run if the caller has it already.
    Returns (the plain run, the NaN-arena run)."""
    if plain is None:
        plain = _execute(case, dev, ac.NAN_PATTERN, plain=True)
        _check_written(plain, None, what + ", ordinary tensors")
    nan = _execute(case, dev, ac.NAN_PATTERN)
    _check_written(nan, plain if compare_plain else None, what + ", NaN arena against ordinary tensors")
    mx = _execute(case, dev, ac.MAX_PATTERN)
    _check_written(mx, nan, what + ", FLT_MAX arena against NaN arena")
    return plain, nan


# ---- the arena's 8-byte carves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("pattern", sorted(ac.PATTERNS))
def test_arena_carves_eight_byte_items(request, which, pattern):
    """float64 / int64 carves at phases 0 and 8: aligned as asked, two pattern words an element, guarded on either side."""
    dev = _dev(request, which)
    word = int(np.array([ac.PATTERNS[pattern]], dtype=np.uint32).view(np.int32)[0])
    for dtype, phase in ((F64, 0), (F64, 8), (I64, 8), (I64, 0)):
        def fresh():
            a = ac.Arena(3 * 8192 + 4096, 4096, ac.PATTERNS[pattern], dev)
            a.carve("left", (5,), F32, 4)
            t = a.carve("mid", (33,), dtype, phase)
            a.carve("right", (0,), F32, 12)
            return a, t
        a, t = fresh()
        assert t.dtype == dtype and t.shape == (33,) and t.is_contiguous() and t.data_ptr() % 16 == phase
        assert ac.bits(t).shape == (66,) and bool((ac.bits(t) == word).all())
        a.check()
        t.fill_(3)
        a.check()
        for where, match in ((-1, "before the start of `mid`"), (66, "past the end of `mid`")):
            a, t = fresh()
            a.words[(t.data_ptr() - a.base) // 4 + where] = 1
            with pytest.raises(ac.GuardError, match=match):
                a.check()
        with pytest.raises(AssertionError):
            fresh()[0].carve("odd", (2,), dtype, 4)                          # an 8-byte item at phase 4
    s = ac.Sizer(4096)
    assert s.carve("x", (3,), F64, 8).dtype == F64 and s.bytes >= 4096 + 24 + 4096
    p = ac.Plain(ac.PATTERNS[pattern], dev)
    assert bool((ac.bits(p.carve("x", (3,), I64)) == word).all())
    src = torch.arange(4, dtype=F64)
    a = ac.Arena(3 * 8192, 4096, ac.PATTERNS[pattern], dev)
    t = a.put("operand", src, 8)
    a.check()
    t[3] = -1.0
    with pytest.raises(ac.GuardError, match="operand"):
        a.check()


# ======== A. semicrf_adabelief_step =========================================================================================================
COEF = float(np.float32(0.37))
STEP_CONFIGS = [(n, [n]) for n in (1, 2, 3, 4, 5, 7, 8, 9)] + [
    (259, [3, 67, 259]), (1027, [3, 67, 1027]),
    (8, [1, 2, 3, 4, 5, 6, 7, 8]),
    (259, [int(x) for x in np.cumsum([3, 1, 4, 1, 5, 9, 2])] + [259]),
]
TRIP = 2048 * 256                                # work items of one grid-stride trip (csrc/optim.hip: at most 2048 workgroups of 256)
STRIDE_CONFIGS = [
    # the 4-byte kernel: one element a work item, the second trip holds 259 elements and the group boundary
    pytest.param((TRIP + 259, [TRIP + 1, TRIP + 259], (4, 4, 4, 4), 12), id="scalar-2trips"),
    # the 16-byte kernel: four elements a work item, the second trip holds the 7 last elements (one full access and a tail of 3)
    pytest.param((4 * TRIP + 7, [3, 67, 4 * TRIP + 7], (0, 0, 0, 0), None), id="vector-2trips"),
]
STEP_PHASES = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (0, 0, 4, 0), (0, 0, 0, 4), (12, 12, 12, 12), (4, 8, 12, 0)]    # p, g, m, s
COEF_PHASES = [None, 0, 12]                      # absent (has_coef = False), a one-element carve at phase 0 / 12


def test_group_boundaries_cover_a_four_element_access():
    inner = {e % 4 for _, ends in STEP_CONFIGS for e in ends[:-1]}
    assert inner == {0, 1, 2, 3}
    assert max(len(ends) for _, ends in STEP_CONFIGS) == _lib.OPTIM_MAX_GROUPS == 8


def _group_hyper(gi):
    """Every group its own lr, wd, betas and eps; t = 3 (the SGD-style branch) for even groups, t = 7 (rectified) for odd ones."""
    return dict(t=3 if gi % 2 == 0 else 7, lr=1e-2 * (gi + 1), wd=0.05 * (gi + 1), betas=(0.9 - 0.03 * gi, 0.999 - 0.012 * gi),
                eps=1e-3 * (gi + 1))


def _group_table(ends):
    """The raw host table of the op, float64 [n][10] = {end, decay, b1, 1-b1, b2, 1-b2, eps, sqrt_bc2, step, rectified}."""
    rows = []
    for gi, end in enumerate(ends):
        h = _group_hyper(gi)
        k = adabelief_scalars(h["t"], h["lr"], h["wd"], h["betas"], h["eps"])
        assert k["rectified"] == (gi % 2 == 1)
        rows.append([float(end)] + [k[key] for key in ("decay", "b1", "omb1", "b2", "omb2", "eps", "sqrt_bc2", "step")] +
                    [1.0 if k["rectified"] else 0.0])
    return torch.tensor(rows, dtype=F64)


_STEP_INPUTS = {}


def _step_inputs(numel, family):
    """p, m ~ N(0, 1), s = squares plus eps, g from optimizer_common.gradient: full-mantissa fp32 values."""
    key = (numel, family)
    if key not in _STEP_INPUTS:
        g = torch.Generator().manual_seed(77 + numel)
        p, m = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
        s = torch.randn(numel, generator=g) ** 2 + 1e-8
        _STEP_INPUTS[key] = (p, oc.gradient(family, numel, 3), m, s)
    return _STEP_INPUTS[key]


def case_step(inputs, ends, phases, coef_phase):
    p0, g0, m0, s0 = inputs
    numel, table = ends[-1], _group_table(ends)
    coef0 = torch.tensor([COEF], dtype=F32)

    def case(r):
        pp, pg, pm, ps = phases
        p = r.out("p", numel + EXTRA, F32, pp, init=p0)
        g = r.inp("g", g0, pg)
        m = r.out("m", numel + EXTRA, F32, pm, init=m0)
        s = r.out("s", numel + EXTRA, F32, ps, init=s0)
        coef = r.inp("coef", coef0, coef_phase) if coef_phase is not None else None
        if r.A.real and isinstance(r.A, ac.Arena):
            assert [t.data_ptr() % 16 for t in (p, g, m, s)] == list(phases)
            assert coef is None or coef.data_ptr() % 16 == coef_phase
        r.call(lambda: _lib.ops().adabelief_step(p, g, m, s, numel, coef if coef is not None else p.new_empty(0), coef is not None, table))
        return {k: _head(numel + EXTRA, numel) for k in ("p", "m", "s")}
    return case


def _yardstick_arrays(res, inputs, ends, has_coef, yard_ends=None):
    """{quantity: (the op's fp32 result, yardstick_update in float64, the torch-fp32 route)} over the whole call.  yard_ends: the group
    ranges the yardstick and the torch route use (a wrong table on purpose)."""
    p0, g0, m0, s0 = inputs
    numel, coef = ends[-1], COEF if has_coef else 1.0
    yard, route, lo = {"p": [], "m": [], "s": []}, {"p": [], "m": [], "s": []}, 0
    for gi, hi in enumerate(yard_ends or ends):
        h = _group_hyper(gi)
        k = adabelief_scalars(h["t"], h["lr"], h["wd"], h["betas"], h["eps"])
        sl = slice(lo, hi)
        ys = oc.yardstick_update(p0[sl].numpy(), g0[sl].numpy(), m0[sl].numpy(), s0[sl].numpy(), coef, k)
        ts = oc.torch_route_flat(p0[sl], g0[sl], m0[sl], s0[sl], coef, h["t"], h["lr"], h["wd"], h["betas"], h["eps"])
        for name, y, tr in zip(("p", "m", "s"), ys, ts):
            yard[name].append(y)
            route[name].append(tr.numpy())
        lo = hi
    return {name: (res[name].t[:numel].numpy(), np.concatenate(yard[name]), np.concatenate(route[name])) for name in ("m", "s", "p")}


def _against_yardstick(arrays, tag):
    """Every element of p, m, s under check_against_yardstick's bound.  arrays: _yardstick_arrays of one call or of several.  The
    bound's first half, the torch-fp32 route's worst error "on the same inputs", is a statistic of the sample it is taken over:
    a group of one element, or a call of eight, is no sample, so the small configurations are checked together (one family, one
    coef: about 1600 elements), the large ones alone.  Returns the worst ratio."""
    worst = 0.0
    for name in ("m", "s", "p"):
        got, yard, route = (np.concatenate([a[name][i] for a in arrays]) for i in range(3))
        worst = max(worst, oc.check_against_yardstick(got, yard, route, f"{tag}/{name}"))
    return worst


_HOST_STEP = {}


def _host_step(ends, family, has_coef):
    """The host kernel on ordinary tensors (once per configuration): the bit reference of every other run of the configuration,
    on either device; test_adabelief_step_against_float64 holds it against the yardstick."""
    key = (tuple(ends), family, has_coef)
    if key not in _HOST_STEP:
        inputs = _step_inputs(ends[-1], family)
        res = _execute(case_step(inputs, ends, (0, 0, 0, 0), 0 if has_coef else None), CPU, ac.NAN_PATTERN, plain=True)
        _check_written(res, None, f"step n={ends[-1]} groups={len(ends)} {family} coef={'yes' if has_coef else 'no'}")
        _HOST_STEP[key] = res
    return _HOST_STEP[key]


@pytest.mark.parametrize("has_coef", [False, True], ids=["nocoef", "coef"])
@pytest.mark.parametrize("family", ["randn", "zeros"])
def test_adabelief_step_against_float64(family, has_coef):
    """The host kernel's results of every small configuration, per element, against float64.  The device cases require the host's
    bits, so this holds for them as it stands."""
    arrays = [_yardstick_arrays(_host_step(ends, family, has_coef), _step_inputs(numel, family), ends, has_coef) for numel, ends in STEP_CONFIGS]
    worst = _against_yardstick(arrays, f"step, {len(STEP_CONFIGS)} configurations, {family}, coef={'yes' if has_coef else 'no'}")
    print(f"worst |op - yardstick| / bound = {worst:.3f}")


def _step_contract(dev, ends, family, phases, coef_phase):
    has_coef = coef_phase is not None
    host = _host_step(ends, family, has_coef)
    tag = f"step n={ends[-1]} groups={len(ends)} {family} phases={phases} coef={coef_phase} on {dev.type}"
    case = case_step(_step_inputs(ends[-1], family), ends, phases, coef_phase)
    if dev.type == "cpu":
        plain = host
    else:                                        # optim_math.h: device and host give the same bits
        plain = _execute(case, dev, ac.NAN_PATTERN, plain=True)
        _check_written(plain, host, tag + ", device against host")
    _contract(case, dev, tag, plain=plain)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("phases", STEP_PHASES, ids=lambda ph: "p%d_g%d_m%d_s%d" % ph)
def test_adabelief_step_phases_sizes_and_groups(request, which, phases):
    """Any buffer off 16 bytes selects the 4-byte kernel: the bits of the 16-byte one and of the host kernel at every size, group
    table and coef form."""
    dev = _dev(request, which)
    for i, (numel, ends) in enumerate(STEP_CONFIGS):
        for j, coef_phase in enumerate(COEF_PHASES):
            _step_contract(dev, ends, ("randn", "zeros")[(i + j) % 2], phases, coef_phase)
            if len(ends) > 1:
                _step_contract(dev, ends, ("zeros", "randn")[(i + j) % 2], phases, coef_phase)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("cfg", STRIDE_CONFIGS)
def test_adabelief_step_grid_stride(request, which, cfg):
    """The second trip of the grid-stride loop, in either kernel; whole buffers are compared."""
    numel, ends, phases, coef_phase = cfg
    assert numel == ends[-1] and (numel if any(phases) else (numel + 3) // 4) > TRIP
    _step_contract(_dev(request, which), ends, "randn", phases, coef_phase)
    if which == "cpu":                           # (the device run has just been found to hold the host's bits)
        has_coef = coef_phase is not None
        arrays = _yardstick_arrays(_host_step(ends, "randn", has_coef), _step_inputs(numel, "randn"), ends, has_coef)
        print(f"worst |op - yardstick| / bound = {_against_yardstick([arrays], f'step n={numel}'):.3f}")


def test_yardstick_sees_a_group_table_shifted_by_one():
    """What the comparison is worth: the yardstick run with every inner boundary one element later fails the very check that the
    op passes -- a factor taken from the neighbouring group moves p, m and s by far more than the bound."""
    for numel, ends in STEP_CONFIGS:
        if len(ends) < 2 or ends[-2] + 1 >= numel:
            continue
        for family in ("randn", "zeros"):
            res = _host_step(ends, family, True)
            shifted = [e + 1 for e in ends[:-1]] + [numel]
            with pytest.raises(AssertionError, match="bound"):
                _against_yardstick([_yardstick_arrays(res, _step_inputs(numel, family), ends, True, yard_ends=shifted)], "shifted")
            _against_yardstick([_yardstick_arrays(res, _step_inputs(numel, family), ends, True)], "as it is")


# ======== B. semicrf_grad_sqnorm and the norm ================================================================================================
SQNORM_PER_BLOCK, SQNORM_MAX = 32768, _lib.SQNORM_MAX_PARTIALS
SQNORM_NUMELS = [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 32767, 32768, 32769, 65541, 98309]
SQNORM_BIG = 257 * 32768 + 5                     # beyond the cap of 256 partials: the workgroups stride (34 MB)


def sqnorm_partials(numel):                      # csrc/optim_math.h
    return min(max((numel + SQNORM_PER_BLOCK - 1) // SQNORM_PER_BLOCK, 1), SQNORM_MAX)


_GRADS = {}


def _gradient(numel, family):
    """(fp32 gradient, what the family pins): "exact" -- integers in [-510, 510] \\ {0} from a hash of the index, the int sum of
    squares; "randn" / "huge" -- the norm by math.fsum in float64."""
    key = (numel, family)
    if key not in _GRADS:
        if family == "exact":
            h = synth.hash_u64_numpy(np.arange(numel, dtype=np.uint64), 991)
            v = ((h % np.uint64(510)).astype(np.int64) + 1) * np.where((h >> np.uint64(40)) & np.uint64(1), 1, -1)
            assert v.min() >= -510 and v.max() <= 510 and not (v == 0).any()
            _GRADS[key] = (torch.from_numpy(v.astype(np.float32)), int((v * v).sum()))
        else:
            g = oc.gradient(family, numel, 3)
            g64 = g.numpy().astype(np.float64)
            _GRADS[key] = (g, math.sqrt(math.fsum(g64 * g64)))
    return _GRADS[key]


def case_sqnorm(g0, numel, pflat, ppart, to_stats):
    """flat holds three NaNs behind flat[numel]; partials are SEMICRF_SQNORM_MAX_PARTIALS + EXTRA doubles.  to_stats: the norm
    through semicrf_clip_from_history (no quantile, no append) into stats[0]."""
    flat0 = torch.cat([g0, torch.full((3,), float("nan"))])
    nparts = sqnorm_partials(numel)

    def case(r):
        flat = r.inp("flat", flat0, pflat)
        partials = r.out("partials", SQNORM_MAX + EXTRA, F64, ppart)
        masks = {"partials": _head(SQNORM_MAX + EXTRA, nparts)}
        if to_stats:
            ring, state = r.inp("ring", torch.tensor([40.0]), pflat), r.inp("state", torch.tensor([1, 0], dtype=I32), pflat)
            stats = r.out("stats", 3 + EXTRA, F32, pflat)
            masks["stats"] = _head(3 + EXTRA, 1)

        def go():
            _lib.ops().grad_sqnorm(flat, numel, partials)
            if to_stats:
                _lib.ops().clip_from_history(partials, True, numel, flat.new_empty(0), False, -1.0, ring, 1, state, False, stats)
        r.call(go)
        return masks
    return case


def _sqnorm_phases(numel):
    return [(0, 0), (4, 8)] if numel == SQNORM_BIG else [(0, 0), (4, 8), (8, 0), (12, 8)]


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("numel", SQNORM_NUMELS + [SQNORM_BIG])
def test_grad_sqnorm_exact_family(request, which, numel):
    """Squares and partial sums of integers below 2^53 are exact doubles in any order: the written partials add up to the integer
    sum of squares EXACTLY -- one dropped or doubled element, or one read behind flat[numel], changes it."""
    dev = _dev(request, which)
    g0, want = _gradient(numel, "exact")
    assert want < 2 ** 53
    n = sqnorm_partials(numel)
    plain = None
    for pflat, ppart in _sqnorm_phases(numel):
        tag = f"grad_sqnorm exact n={numel} flat at {pflat}, partials at {ppart} on {dev.type}"
        # (which elements a workgroup sums depends on the phase of flat: the partials are compared with the ordinary-tensor run
        # at phase 0 only, their sum at every phase)
        plain, nan = _contract(case_sqnorm(g0, numel, pflat, ppart, False), dev, tag, plain=plain, compare_plain=pflat == 0)
        for run in (plain, nan):
            parts = run["partials"].t[:n].tolist()
            assert all(x == int(x) and x >= 0 for x in parts), tag
            assert sum(int(x) for x in parts) == want, (tag, sum(int(x) for x in parts) - want)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("family", ["randn", "huge"])
@pytest.mark.parametrize("numel", SQNORM_NUMELS + [SQNORM_BIG])
def test_norm_float_families(request, which, numel, family):
    """The norm through semicrf_clip_from_history: within 2 eps32 of math.fsum (test_optimizer.test_norm's bound) at every phase,
    the same bits from two runs at one phase; from phase to phase the order of addition may differ (the header says so)."""
    dev = _dev(request, which)
    g0, norm64 = _gradient(numel, family)
    seen, worst, plain = {}, 0.0, None
    for pflat, ppart in _sqnorm_phases(numel):
        tag = f"norm {family} n={numel} flat at {pflat}, partials at {ppart} on {dev.type}"
        # (two arena runs, NaN and FLT_MAX pattern, at this phase: _contract requires the same bits of them)
        plain, nan = _contract(case_sqnorm(g0, numel, pflat, ppart, True), dev, tag, plain=plain, compare_plain=pflat == 0)
        for run in (plain, nan):
            norm = float(run["stats"].t[0])
            assert np.isfinite(norm) and abs(norm - norm64) <= 2 * oc.EPS32 * norm64, (tag, norm, norm64)
            worst = max(worst, abs(norm - norm64) / (2 * oc.EPS32 * norm64))
        total = 0.0
        for x in nan["partials"].t[:sqnorm_partials(numel)].tolist():        # (the second stage's order)
            total += x
        seen[pflat] = (np.float32(float(nan["stats"].t[0])), total)
    ulps = max(abs(float(v) - float(seen[0][0])) / float(np.spacing(np.abs(seen[0][0]))) for v, _ in seen.values())
    rel = max(abs(t - seen[0][1]) / seen[0][1] for _, t in seen.values())
    print(f"norm {family} n={numel} on {dev.type}: worst |norm - fsum| / (2 eps32 norm) = {worst:.3f}; largest difference between "
          f"phases: {ulps:.0f} ulp of the fp32 norm, {rel:.2e} relative in the double sum of squares")


# ======== C. semicrf_clip_from_history ======================================================================================================
CAP_MAX = _lib.HISTORY_MAX
RINGS = [(CAP_MAX, c, 0) for c in (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 2049, 8192, 8193, 16383, 16384)] + [
    (1025, 1025, 1000), (CAP_MAX, CAP_MAX, CAP_MAX - 1)]                     # capacity, count, head
CLIP_QS = [0.0, 0.5, 0.8, 1.0, 0.3337]
NORM_IN = 17.5
FULL_PARTIALS, FULL_NUMEL = [1.0e4, 2.5e3, 7.25], 65541                      # three partials (sqnorm_partials(65541) == 3)


def _ring(capacity, count, head):
    """(ring content fp32 [capacity], the HostHistory of it): lognormal values with every seventh a tie, oldest at `head`;
    slots that hold no value are -1 (a value that would change every quantile if it were read)."""
    rng = np.random.default_rng(6 + count)
    vals = rng.lognormal(3.0, 1.0, count).astype(np.float32)
    vals[::7] = vals[min(3, count - 1)]
    ring = np.full(capacity, -1.0, dtype=np.float32)
    ring[(head + np.arange(count)) % capacity] = vals
    ref = oc.HostHistory(capacity, init=None)
    for v in vals:
        ref.append(v)
    return torch.from_numpy(ring), ref


def case_clip(ring0, capacity, count, head, phase, ppart):
    state0 = torch.tensor([count, head], dtype=I32)
    part0 = torch.full((SQNORM_MAX,), float("nan"), dtype=F64)
    part0[:len(FULL_PARTIALS)] = torch.tensor(FULL_PARTIALS, dtype=F64)
    assert sqnorm_partials(FULL_NUMEL) == len(FULL_PARTIALS)

    def case(r):
        masks = {}
        # quantile only: the ring and the state are operands
        ring, state = r.inp("ring", ring0, phase), r.inp("state", state0, phase)
        stats_q = [r.out(f"stats_q{i}", 3 + EXTRA, F32, phase) for i in range(len(CLIP_QS))]
        masks.update({f"stats_q{i}": torch.arange(3 + EXTRA) == 1 for i in range(len(CLIP_QS))})
        # append only, and the full step: a ring and a state of their own each
        norm_in = r.inp("norm_in", torch.tensor([NORM_IN]), phase)
        partials = r.inp("partials", part0, ppart)
        rings = {}
        for k, written in (("a", [0]), ("f", [0, 1, 2])):
            rings[k] = (r.out("ring_" + k, capacity + EXTRA, F32, phase, init=ring0), r.out("state_" + k, 2 + EXTRA, I32, phase, init=state0),
                        r.out("stats_" + k, 3 + EXTRA, F32, phase))
            masks.update({"ring_" + k: _head(capacity + EXTRA, capacity), "state_" + k: _head(2 + EXTRA, 2),
                          "stats_" + k: torch.isin(torch.arange(3 + EXTRA), torch.tensor(written))})

        def go():
            ops, none, none64 = _lib.ops(), ring.new_empty(0), ring.new_empty(0, dtype=F64)
            for q, st in zip(CLIP_QS, stats_q):
                ops.clip_from_history(none64, False, 0, none, False, q, ring, capacity, state, False, st)
            ops.clip_from_history(none64, False, 0, norm_in, True, -1.0, rings["a"][0], capacity, rings["a"][1], True, rings["a"][2])
            ops.clip_from_history(partials, True, FULL_NUMEL, none, False, 0.8, rings["f"][0], capacity, rings["f"][1], True, rings["f"][2])
        r.call(go)
        return masks
    return case


def _bits32(t):
    return t.contiguous().view(I32)


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("ring", RINGS, ids=lambda x: "cap%d_count%d_head%d" % x)
def test_clip_from_history_sizes_and_written_sets(request, which, ring):
    dev = _dev(request, which)
    capacity, count, head = ring
    ring0, ref = _ring(capacity, count, head)
    norm_full = math.sqrt(sum(FULL_PARTIALS))
    slot = (head + count) % capacity if count < capacity else head           # where an append goes
    plain = None
    for phase, ppart in ((0, 0), (12, 8)):
        tag = f"clip_from_history capacity={capacity} count={count} head={head} at phase {phase} on {dev.type}"
        plain, nan = _contract(case_clip(ring0, capacity, count, head, phase, ppart), dev, tag, plain=plain)
        for run in (plain, nan):
            # quantile only: stats[1], within one fp32 ulp of np.quantile (the ring and the state: operands, found unchanged)
            for i, q in enumerate(CLIP_QS):
                got, want = float(run[f"stats_q{i}"].t[1]), ref.quantile(q)
                assert oc.ulp_close(got, want), (tag, q, got, want)
            # append only: stats[0] is the norm handed in; exactly one ring word and one state word change
            assert float(run["stats_a"].t[0]) == NORM_IN
            for k, norm in (("a", NORM_IN), ("f", norm_full)):
                rg, st = run["ring_" + k].t[:capacity], run["state_" + k].t[:2]
                diff = torch.nonzero(_bits32(rg) != _bits32(ring0)).reshape(-1).tolist()
                assert diff == [slot], (tag, k, diff, slot)
                assert abs(float(rg[slot]) - norm) <= 2 * oc.EPS32 * norm
                assert st.tolist() == ([count + 1, head] if count < capacity else [count, (head + 1) % capacity]), (tag, k)
            # the full step: the norm of the partials, the clip value BEFORE the append, their coefficient
            norm, clip, coef = (float(x) for x in run["stats_f"].t[:3])
            assert abs(norm - norm_full) <= 2 * oc.EPS32 * norm_full
            assert oc.ulp_close(clip, ref.quantile(0.8)), (tag, clip)
            want = oc.yardstick_coef(clip, norm)
            assert abs(coef - want) <= 2 * oc.EPS32 * want, (tag, coef, want)
    after = oc.HostHistory(capacity, init=None)
    for v in list(ref.values) + [NORM_IN]:
        after.append(v)
    rg = plain["ring_a"].t[:capacity]
    n, h = plain["state_a"].t[:2].tolist()
    assert rg[(h + torch.arange(n)) % capacity].tolist() == list(after.values)


# ======== D. the attribute loss and readout ==================================================================================================
ATTR_KS, ATTR_CS = [1, 5, 259], [1, 7]


def _counts(K, C):
    """Rows per chain; C = 7: empty chains first, in the middle and last."""
    if C == 1:
        return [K]
    a = K // 3 + (K % 3 > 0)
    b = (K - a) // 2
    c = (K - a - b) // 2
    counts = [0, a, b, 0, c, K - a - b - c, 0]
    assert sum(counts) == K and len(counts) == C == 7
    return counts


def _loss_inputs(K, C):
    """attr_loss_common.shape_case for the chain counts of _counts (the generator takes its counts from a table by name)."""
    with mock.patch.dict(alc.SHAPES, {"_step_contract": _counts(K, C) if K else [0] * C}):
        return alc.shape_case("_step_contract")


def _phase_of(j):
    """Phase assignment j of 4: tensor number i of a case sits at phase 4 ((i + j) % 4); the float2 / int64 buffers at 8 (j % 2)."""
    return (lambda i: 4 * ((i + j) % 4)), 8 * (j % 2)


def case_loss_fwd(inputs, K, C, j):
    lv0, of0, vel0, ref0, pres0, off0, base0, _ = inputs
    ph, ph8 = _phase_of(j)

    def case(r):
        lv = r.inp("logitsVelocity", lv0, ph8)
        of, vel, refined, pres = r.inp("ofLogits", of0, ph(0)), r.inp("velocity", vel0, ph(1)), r.inp("ofRefined", ref0, ph(2)), r.inp("ofPresence", pres0, ph(3))
        offsets, base = r.inp("offsets", off0, ph(4)), r.inp("base", base0, ph(5))
        rows, out = r.out("rowLogProb", K + EXTRA, F32, ph(6)), r.out("out", C + EXTRA, F32, ph(7))
        r.call(lambda: _lib.ops().attribute_loss_fwd(lv, of, vel, refined, pres, K, offsets, C, base, True, rows, out))
        # K == 0: nothing is launched, out keeps the pattern (the result is base itself)
        return {"rowLogProb": _head(K + EXTRA, K), "out": _head(C + EXTRA, C if K else 0)}
    return case


def case_loss_bwd(inputs, K, C, j, gstride):
    lv0, of0, vel0, ref0, pres0, off0, _, gout0 = inputs
    ph, ph8 = _phase_of(j)

    def case(r):
        lv = r.inp("logitsVelocity", lv0, ph8)
        of, vel, refined, pres = r.inp("ofLogits", of0, ph(1)), r.inp("velocity", vel0, ph(2)), r.inp("ofRefined", ref0, ph(3)), r.inp("ofPresence", pres0, ph(0))
        offsets, gout = r.inp("offsets", off0, ph(5)), r.inp("gout", gout0 if gstride else gout0[:1], ph(6))
        dlv, dof = r.out("dLogitsVelocity", K * 128 + 2 * EXTRA, F32, 8 - ph8), r.out("dOfLogits", K * 4 + EXTRA, F32, ph(7))
        r.call(lambda: _lib.ops().attribute_loss_bwd(gout, gstride, lv, of, vel, refined, pres, K, offsets, C, dlv, dof))
        return {"dLogitsVelocity": _head(K * 128 + 2 * EXTRA, K * 128), "dOfLogits": _head(K * 4 + EXTRA, K * 4)}
    return case


def case_decode(lv0, of0, K, j, criterion):
    ph, ph8 = _phase_of(j)
    mse = criterion == "mse"

    def case(r):
        lv, of = r.inp("logitsVelocity", lv0, ph8), r.inp("ofLogits", of0, ph(0))
        # both velocity outputs are passed at full size: the one the criterion does not use keeps the pattern
        cls, mean = r.out("velocityClass", K + EXTRA, I64, 8 - ph8), r.out("velocityMean", K + EXTRA, F32, ph(1))
        val, pres = r.out("ofValue", 2 * K + EXTRA, F32, ph(2)), r.out("ofPresence", 2 * K + EXTRA, U8, ph(3))
        r.call(lambda: _lib.ops().attribute_decode(lv, of, K, _lib.VEL_HAMMING + adc.CRITERIA.index(criterion), cls, mean, val, pres))
        return {"velocityClass": _head(K + EXTRA, 0 if mse else K), "velocityMean": _head(K + EXTRA, K if mse else 0),
                "ofValue": _head(2 * K + EXTRA, 2 * K), "ofPresence": _head(2 * K + EXTRA, 2 * K)}
    return case


def test_criteria_are_numbered_in_order():
    assert [_lib.VEL_HAMMING, _lib.VEL_MSE, _lib.VEL_MATCH, _lib.VEL_MAE] == [0, 1, 2, 3] and adc.CRITERIA == ("hamming", "mse", "match", "mae")


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("K", ATTR_KS + [0])
def test_attribute_loss_written_sets(request, which, K):
    dev = _dev(request, which)
    for C in ATTR_CS if K else [7]:
        inputs = _loss_inputs(K, C)
        for j in range(4):
            tag = f"attribute_loss K={K} C={C} phases {j} on {dev.type}"
            plain, _ = _contract(case_loss_fwd(inputs, K, C, j), dev, tag + " fwd")
            bwd = {gs: _contract(case_loss_bwd(inputs, K, C, j, gs), dev, tag + f" bwd gstride={gs}")[0] for gs in (0, 1)}
            if j == 3 and K:                     # an off-phase configuration against float64, under the helpers' own bounds
                lv, of, vel, refined, pres, offsets, base, gout = inputs
                y = alc.yardstick(lv, of, vel, refined, pres, offsets, base=base, gout=gout)
                t_out, t_dlv, t_dof = alc.torch_route_grads(lv, of, vel, refined, pres, offsets, gout, base=base)
                rows = alc.scatter_index(offsets)
                floor = alc.value_floor(y, offsets) + alc.EPS32 * y["out"].abs()            # base is added last: one more rounding
                alc.check_bound(tag + " value", plain["out"].t[:C], y["out"], t_out, floor)
                alc.check_bound(tag + " dLogitsVelocity", bwd[1]["dLogitsVelocity"].t[:K * 128].view(K, 128), y["dLogitsVelocity"], t_dlv,
                                alc.grad_floor(y["dLogitsVelocity"], gout[rows]))
                alc.check_bound(tag + " dOfLogits", bwd[1]["dOfLogits"].t[:K * 4].view(K, 4), y["dOfLogits"], t_dof,
                                alc.grad_floor(y["dOfLogits"], gout[rows]))


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("criterion", adc.CRITERIA)
@pytest.mark.parametrize("K", ATTR_KS)
def test_attribute_decode_written_sets(request, which, K, criterion):
    dev = _dev(request, which)
    lv, of = adc.mixed_rows(K)
    for j in range(4):
        tag = f"attribute_decode K={K} {criterion} phases {j} on {dev.type}"
        plain, _ = _contract(case_decode(lv, of, K, j, criterion), dev, tag)
    assert set(plain["ofPresence"].t[:2 * K].tolist()) <= {0, 1}
    # (the last, off-phase, configuration) against float64
    from transkun_amd import attributes
    t_vel, t_val, t_pres = attributes.attribute_decode_torch(lv, of, criterion)
    adc.check_values(tag + " ofValue", plain["ofValue"].t[:2 * K].view(K, 2), adc.of_value64(of[:, :2]), t_val)
    assert torch.equal(plain["ofPresence"].t[:2 * K].view(K, 2).bool(), of[:, 2:] > 0)
    y = adc.velocity64(lv)
    if criterion == "mse":
        adc.check_values(tag + " mean", plain["velocityMean"].t[:K], y["mean"], t_vel)
    elif criterion == "hamming":
        assert torch.equal(plain["velocityClass"].t[:K], y["hamming"])
    else:
        s = adc.slack(y, criterion, plain["velocityClass"].t[:K])
        assert bool((s <= adc.SLACK_MAX).all()), (tag, float(s.max()) / adc.EPS32)


def test_c_abi_rejects_a_logits_velocity_off_eight_bytes():
    """SEMICRF_EINVAL with the other argument checks, ahead of any HIP call: the answer on a machine without a GPU too (the
    pointers are never dereferenced)."""
    lib = _lib.load()
    ok = ctypes.c_void_p(4096)
    for off in (4, 12):
        bad = ctypes.c_void_p(4096 + off)
        calls = {
            "loss_fwd": lambda: lib.semicrf_attribute_loss_fwd(bad, ok, ok, ok, ok, 5, ok, 2, None, ok, ok, None),
            "loss_bwd, logitsVelocity": lambda: lib.semicrf_attribute_loss_bwd(ok, 1, bad, ok, ok, ok, ok, 5, ok, 2, ok, ok, None),
            "loss_bwd, dLogitsVelocity": lambda: lib.semicrf_attribute_loss_bwd(ok, 0, ok, ok, ok, ok, ok, 5, ok, 2, bad, ok, None),
            "decode": lambda: lib.semicrf_attribute_decode(bad, ok, 5, 0, ok, None, ok, ok, None),
            "decode, mse": lambda: lib.semicrf_attribute_decode(bad, ok, 5, 1, None, ok, ok, ok, None),
        }
        for name, fn in calls.items():
            rc = fn()
            msg = lib.semicrf_last_error().decode()
            assert rc == 1 and "8-byte aligned" in msg and "ogitsVelocity" in msg, (name, off, rc, msg)


def _off_view(src, off_bytes):
    """A contiguous view with src's values whose data_ptr() % 16 == off_bytes."""
    buf = torch.zeros(src.numel() + 8, dtype=src.dtype, device=src.device)
    skip = ((off_bytes - buf.data_ptr()) % 16) // 4
    v = buf[skip:skip + src.numel()].view(src.shape)
    v.copy_(src)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("off", [4, 12])
def test_ops_reject_a_logits_velocity_off_eight_bytes(gpu, off):
    """The same through torch.ops on the device: a RuntimeError, and the outputs keep the pattern."""
    K, C = 5, 7
    lv, of, vel, refined, pres, offsets, base, gout = (t.to(gpu) for t in _loss_inputs(K, C))
    P = ac.Plain(ac.NAN_PATTERN, gpu)
    word = int(np.array([ac.NAN_PATTERN], dtype=np.uint32).view(np.int32)[0])
    outs = {n: P.carve(n, (k,), dt) for n, k, dt in (("rowLogProb", K, F32), ("out", C, F32), ("dLogitsVelocity", K * 128 + 4, F32), ("dOfLogits", K * 4, F32),
                                                     ("velocityClass", K, I64), ("velocityMean", K, F32), ("ofValue", 2 * K, F32))}
    presence = P.carve("ofPresence", (2 * K,), U8)
    presence0 = presence.clone()
    bad = _off_view(lv, off)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        _lib.ops().attribute_loss_fwd(bad, of, vel, refined, pres, K, offsets, C, base, True, outs["rowLogProb"], outs["out"])
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        _lib.ops().attribute_loss_bwd(gout, 1, bad, of, vel, refined, pres, K, offsets, C, outs["dLogitsVelocity"], outs["dOfLogits"])
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        _lib.ops().attribute_loss_bwd(gout, 1, lv, of, vel, refined, pres, K, offsets, C, _off_view(outs["dLogitsVelocity"][:K * 128], off),
                                      outs["dOfLogits"])
    for crit in range(4):
        with pytest.raises(RuntimeError, match="8-byte aligned"):
            _lib.ops().attribute_decode(bad, of, K, crit, outs["velocityClass"], outs["velocityMean"], outs["ofValue"], presence)
    torch.cuda.synchronize(gpu)
    for n, t in outs.items():
        assert bool((ac.bits(t) == word).all()), n
    assert torch.equal(presence, presence0)
    assert _lib.device_status() == 0


@pytest.mark.parametrize("which", DEVICES)
@pytest.mark.parametrize("K", [5, 259])
def test_public_wrappers_take_a_view_four_bytes_off(request, which, K):
    """buf[1:1 + K * 128].view(K, 128): attribute_log_prob (forward and backward) and attribute_decode copy it into an aligned tensor
    and give the aligned call's bits; an aligned input is not copied."""
    from transkun_amd import attributes
    dev = _dev(request, which)
    C = 7
    lv, of, vel, refined, pres, offsets, base, gout = (t.to(dev) for t in _loss_inputs(K, C))
    buf = torch.zeros(K * 128 + 1, dtype=F32, device=dev)
    view = buf[1:1 + K * 128].view(K, 128)
    view.copy_(lv)
    assert view.is_contiguous() and view.data_ptr() % 8 == 4 and lv.data_ptr() % 8 == 0
    assert attributes._f32c8(lv).data_ptr() == lv.data_ptr() and attributes._f32c8(view).data_ptr() % 8 == 0
    res = []
    for x in (lv, view):
        x = x.detach().requires_grad_()
        o = of.clone().requires_grad_()
        out = attributes.attribute_log_prob(x, o, vel, refined, pres, offsets, base=base)
        (out * gout).sum().backward()
        res.append([out.detach(), x.grad, o.grad] + [r for c in adc.CRITERIA for r in attributes.attribute_decode(x.detach(), of, c)])
    assert res[1][1].shape == (K, 128)
    for a, b in zip(*res):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else ac.bits(a),
                                                  b.view(torch.uint8) if b.dtype == torch.bool else ac.bits(b))
    assert torch.equal(view, lv)                                             # the caller's tensor is not written
    if dev.type == "cuda":
        assert _lib.device_status() == 0
