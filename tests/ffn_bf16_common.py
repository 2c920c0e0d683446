"""Shared by the CPU and GPU tests of the bf16 feed-forward ResBlock (tests/test_feed_forward_bf16.py): the two forms' cases on
ffn_common's generator, the float64 yardstick, the stock routes on identical inputs, the gates and the closed-form inputs of the
exact-answer tests.

Form A (torch.ops.semicrf.ffn_residual_bf16): x and the parameters of ffn_common.case rounded to bf16.  Truth: ffn_common.formula64 on
float64 copies of the ROUNDED tensors.  Gate: max(GATE x e16, 2^-8 max|truth|), e16 the error of the case's ResBlock cast to bf16 on the
CPU on identical inputs; the floor is half a bf16 ulp of the largest output, the final rounding.
Form B (ffn_residual_bf16_mixed): the fp32 tensors of ffn_common.case as they are.  Truth: the case's own, on the UNROUNDED parameters
(weight rounding counts as error).  Gate: max(GATE x e_ac, 4 x 2^-24 max|truth|), e_ac the error of the stock block under
torch.autocast("cpu", dtype=torch.bfloat16).

Cases are built once on the CPU (lru_cache) and never modified; the GPU tests move copies.
"""
import copy
import functools

import torch

import ffn_common

GATE = ffn_common.GATE
FORMS = ("A", "B")
BF16 = torch.bfloat16
# set by a test to run the op WITHOUT the last hidden chunk (when there is more than one): the mutation the exact-answer test must catch
SKIP_LAST_CHUNK = False


def tiles():
    """(R, C): the bf16 op's row tile and hidden chunk, read from the constants exported next to it."""
    from transkun_amd import backbone
    return backbone.FEED_FORWARD_BF16_ROW_TILE, backbone.FEED_FORWARD_BF16_HIDDEN_CHUNK


def dtype_of(form):
    return BF16 if form == "A" else torch.float32


@functools.lru_cache(maxsize=None)
def case(form, rows, D, hidden, scale_kind="randn", mult=1.0, lead=None):
    """One case of the gate: x, the parameters, the float64 truth, the stock route's error and the gate."""
    c = ffn_common.case(rows, D, hidden, scale_kind, mult, lead)
    if form == "A":
        x = c["x"].bfloat16()
        params = tuple(p.bfloat16() for p in c["params"])
        blk = copy.deepcopy(c["block"]).bfloat16()
        with torch.no_grad():
            truth = ffn_common.formula64(x, *params, c["eps"])
            stock = blk(x)
        floor = 2.0 ** -8 * float(truth.abs().max())
    else:
        x, params, truth = c["x"], c["params"], c["truth"]
        with torch.no_grad(), torch.autocast("cpu", dtype=BF16):
            stock = c["block"](x)
        floor = 4 * ffn_common.U * float(truth.abs().max())
    e_stock = float((stock.double() - truth).abs().max())
    return dict(form=form, x=x, params=params, eps=c["eps"], truth=truth, e_stock=e_stock, gate=max(GATE * e_stock, floor), D=D, hidden=hidden)


def _autocast(form, dev):
    return torch.autocast(torch.device(dev).type, dtype=BF16, enabled=form == "B")


def run(c, dev, x=None):
    """backbone.feed_forward_residual with bf16 = "fused" (form B under bfloat16 autocast), and the counters say that the bf16 op
    answered.  x defaults to the case's own."""
    from transkun_amd import backbone
    x = c["x"] if x is None else x
    w1, b1, w2, b2, scale = c["params"]
    _, C = tiles()
    if SKIP_LAST_CHUNK and c["hidden"] > C:                 # the mutation: the walk stops one chunk early
        keep = (c["hidden"] + C - 1) // C * C - C
        w1, b1, w2 = w1[:keep], b1[:keep], w2[:, :keep].contiguous()
    before = dict(backbone.FEED_FORWARD_BF16_ROUTES), dict(backbone.FEED_FORWARD_ROUTES)
    with torch.no_grad(), _autocast(c["form"], dev):
        out = backbone.feed_forward_residual(x.to(dev), *(p.to(dev) for p in (w1, b1, w2, b2, scale)), eps=c["eps"], route="fused",
                                             bf16="fused")
    assert backbone.FEED_FORWARD_BF16_ROUTES == {"fused": before[0]["fused"] + 1, "torch": before[0]["torch"]}
    assert backbone.FEED_FORWARD_ROUTES == {"fused": before[1]["fused"] + 1, "torch": before[1]["torch"]}
    assert out.dtype == dtype_of(c["form"]) and out.shape == x.shape
    return out


def raw_op(form, x3, params, eps, out3):
    """The torch op itself on [n0, n1, D] views."""
    from transkun_amd import _lib
    ops = _lib.ops()
    (ops.ffn_residual_bf16 if form == "A" else ops.ffn_residual_bf16_mixed)(x3, *params, float(eps), out3)
    return out3


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def one_off(x):
    """The values of x in a view one element off a 16-byte boundary (rows one element longer than x's: an odd row stride too)."""
    view = torch.cat([torch.zeros(*x.shape[:-1], 1, dtype=x.dtype, device=x.device), x], dim=-1)[..., 1:]
    assert view.data_ptr() % 16 == x.element_size()
    return view


def gated(got, c, tag):
    """The gate, the figures printed before it is asserted."""
    assert got.dtype == dtype_of(c["form"]) and got.shape == c["truth"].shape, tag
    e = float((got.cpu().double() - c["truth"]).abs().max())
    ratio = e / c["e_stock"] if c["e_stock"] > 0 else float("nan")
    print(f"ffn_residual_bf16 form {c['form']} [{got.device.type}] {tag}: error {e:.3e}  stock {c['e_stock']:.3e}  ratio {ratio:.2f}  "
          f"{e / c['gate']:.2f} of the gate")
    assert e <= c["gate"], (tag, e, c["gate"])
    return e / c["gate"], ratio


# ---- the exact-answer inputs -------------------------------------------------------------------------------------------------------
EXACT_ROWS_SHORT = 63        # one short of the row tile (asserted against tiles() by the tests)
# (rows, D, hidden): the smallest of everything; a ragged last k-step of layer 1 (D = 8 mod 16) and a second chunk of 8 columns; the
# model's shape with one row in the second tile; the largest width, a third tile of one row and a 17th chunk of 8 columns; a row count
# one short of the tile on three column blocks
EXACT_SHAPES = [(3, 8, 8), (64, 40, 72), (65, 160, 640), (129, 256, 1032), (EXACT_ROWS_SHORT, 96, 136)]


@functools.lru_cache(maxsize=None)
def exact_case(form, rows, D, hidden, probe=None):
    """Inputs whose float64 answer is exactly representable and which the chain reproduces in any summation order: eps = 0 and x = +-1
    (rs = 1, xh = x); W1 in {-1, 0, 1} with at most 8 non-zeros per row and b1 = +-32, so every pre-activation is an integer with
    24 <= |h| <= 40 (gelu is h above, +-0 below, exact in bf16); W2 in {-1, 0, 1}, b2 integers in [-4, 4], scale = 2^-6.  Every partial
    sum is an integer below 2^24.  want = the float64 formula rounded once to the output type.
    probe = an offset: W2 is one-hot, output column n takes hidden column (n + probe) mod hidden, scale = 1, b2 = 0: out = x + gelu(h_j),
    an integer of at most 41 -- layer 1 alone, per hidden column."""
    g = torch.Generator().manual_seed(4242 + 7 * rows + 131 * D + 17 * hidden + (0 if probe is None else 1 + probe))
    x = torch.randint(0, 2, (rows, D), generator=g).float() * 2 - 1
    w1 = torch.zeros(hidden, D)
    nz = min(8, D)
    for j in range(hidden):
        cols = torch.randperm(D, generator=g)[:nz]
        w1[j, cols] = torch.randint(0, 2, (nz,), generator=g).float() * 2 - 1
    b1 = (torch.randint(0, 2, (hidden,), generator=g).float() * 2 - 1) * 32
    if probe is None:
        w2 = torch.randint(-1, 2, (D, hidden), generator=g).float()
        b2 = torch.randint(-4, 5, (D,), generator=g).float()
        scale = torch.full((D,), 2.0 ** -6)
    else:
        w2 = torch.zeros(D, hidden)
        w2[torch.arange(D), (torch.arange(D) + probe) % hidden] = 1.0
        b2 = torch.zeros(D)
        scale = torch.ones(D)
    h = x.double() @ w1.double().T + b1.double()
    assert float(h.abs().min()) >= 24 and float(h.abs().max()) <= 40
    want64 = x.double() + (torch.where(h > 0, h, torch.zeros_like(h)) @ w2.double().T + b2.double()) * scale.double()
    dt = dtype_of(form)
    want = want64.to(dt)
    assert torch.equal(want64.float().double(), want64)                     # exact in fp32: the one rounding (form A) is the last step
    return dict(form=form, x=x.to(dt), params=tuple(p.to(dt) for p in (w1, b1, w2, b2, scale)), eps=0.0, want=want, D=D, hidden=hidden)


def probe_offsets(D, hidden):
    """Offsets with which the one-hot probes read every hidden column once."""
    return list(range(0, hidden, D))
