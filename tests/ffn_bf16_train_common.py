"""Shared by the CPU and GPU tests of the bf16 feed-forward ResBlock's training route (tests/test_feed_forward_bf16_train.py): the two
forms' cases on ffn_train_common's generator, the float64 yardstick with the op's own masks as explicit factors, the stock routes on
identical inputs and masks, the gates, and the chain of csrc/ffn_bf16_train_math.h in float64 for the exact-answer tests.

Form A (bfloat16 tensors): x, dout and the parameters of ffn_train_common.case rounded to bf16.  Truth: float64 autograd on the ROUNDED
tensors.  Stock: the same expression in bf16 on the CPU under autograd.  Floor of the gate: 2^-8 max|truth| (half a bf16 ulp of the
largest element, the final rounding).
Form B (float32 tensors under bfloat16 autocast): the fp32 tensors as they are.  Truth: float64 autograd on them (weight rounding counts
as error).  Stock: the expression under torch.autocast("cpu", dtype=bfloat16).  Floor: 4 x 2^-24 max|truth|.
Gate per tensor: error <= max(GATE x e_stock, floor), the GATE = 8 idiom of ffn_common and ffn_bf16_common.

Cases are built once on the CPU (lru_cache) and never modified; the GPU tests move copies.
"""
import contextlib
import functools

import torch

import ffn_train_common as tc

GATE = tc.GATE
NAMES = tc.NAMES
FORMS = ("A", "B")
BF16 = torch.bfloat16
ROWS = tc.ROWS
SHAPES = tc.SHAPES
EXACT = [(5, 8, 8), (70, 64, 72), (130, 256, 136), (1094, 8, 16), (65, 128, 640)]


def dtype_of(form):
    return BF16 if form == "A" else torch.float32


def autocast(form, dev):
    return torch.autocast(torch.device(dev).type, dtype=BF16) if form == "B" else contextlib.nullcontext()


def floor_of(form, truth):
    return (2.0 ** -8 if form == "A" else 4 * tc.U) * float(truth.abs().max())


def _stock(form, x, params, eps, f1, f2, G):
    """The stock route on the CPU under autograd: in bf16 (form A), under CPU bf16 autocast on the fp32 tensors (form B)."""
    leaves = [t.detach().clone().requires_grad_() for t in (x, *params)]
    with autocast(form, "cpu"):
        out = tc.expression(*leaves, eps, f1, f2)
    grads = torch.autograd.grad((out.to(G.dtype) * G).sum(), leaves)
    return [out.detach().double()] + [g.double() for g in grads]


@functools.lru_cache(maxsize=None)
def case(form, rows, D, hidden, scale_kind="randn", mult=1.0, p1=0.1, p2=0.5, seed=1234):
    if (p1, p2, seed) == (0.1, 0.5, 1234):
        base = tc.case(rows, D, hidden, scale_kind, mult)       # the call of the fp32 route's tests: one cache entry for both
    else:
        base = tc.case(rows, D, hidden, scale_kind, mult, p1=p1, p2=p2, seed=seed)
    dt = dtype_of(form)
    x, G = base["x"].to(dt), base["G"].to(dt)
    params = tuple(p.to(dt) for p in base["params"])
    f1, f2 = tc.masks_for(seed, base["x"], hidden, p1, p2)
    truth = tc.reference(x, params, base["eps"], f1, f2, G.double(), torch.float64)
    stock = _stock(form, x, params, base["eps"], f1, f2, G)
    e_stock = [float((a - b).abs().max()) for a, b in zip(stock, truth)]
    gates = [max(GATE * e, floor_of(form, t)) for e, t in zip(e_stock, truth)]
    return dict(form=form, x=x, G=G, params=params, eps=base["eps"], truth=truth, e_stock=e_stock, gates=gates, D=D, hidden=hidden, p1=p1, p2=p2,
                seed=seed, f1=f1, f2=f2)


def counts():
    from transkun_amd import backbone as bb
    return (dict(bb.FEED_FORWARD_ROUTES), dict(bb.FEED_FORWARD_TRAIN_ROUTES), dict(bb.FEED_FORWARD_BF16_ROUTES),
            dict(bb.FEED_FORWARD_BF16_TRAIN_ROUTES))


def delta(before):
    now = counts()
    return tuple({k: now[i][k] - before[i][k] for k in now[i]} for i in range(4))


FUSED_ONCE = ({"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 1}, {"fused": 1, "torch": 0}, {"fused": 1, "torch": 0, "bwd": 1})


def run(c, dev, x=None, G=None, seed=None):
    """The fused bf16 training route on the case (the host mirrors for the CPU): [out, dx, dW1, db1, dW2, db2, dscale] on the CPU, in the
    form's dtype; the counters say that the bf16 training op and its backward answered."""
    from transkun_amd import backbone
    x = (c["x"] if x is None else x).to(dev).detach().clone().requires_grad_()
    G = (c["G"] if G is None else G).to(dev)
    params = [p.to(dev).clone().requires_grad_() for p in c["params"]]
    before = counts()
    with autocast(c["form"], dev):
        out = backbone.feed_forward_residual(x, *params, eps=c["eps"], route="fused", train="fused", bf16="fused", bf16_train="fused",
                                             p_hidden=c["p1"], p_out=c["p2"], seed=c["seed"] if seed is None else seed)
    grads = torch.autograd.grad((out * G).sum(), [x] + params)
    assert delta(before) == FUSED_ONCE
    dt = dtype_of(c["form"])
    assert out.dtype == dt and all(g.dtype == dt for g in grads)
    return [out.detach().cpu()] + [g.cpu() for g in grads]


def ratios(got, c):
    return [(float((a.double() - t).abs().max()) / gate, n) for a, t, gate, n in zip(got, c["truth"], c["gates"], NAMES)]


def worst(got, c):
    """(ratio, name): the largest error / gate over the seven tensors."""
    return max(ratios(got, c))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def one_off(x):
    """The values of x in a view one element off a 16-byte boundary (rows one element longer than x's: an odd row stride too)."""
    view = torch.cat([torch.zeros(*x.shape[:-1], 1, dtype=x.dtype, device=x.device), x], dim=-1)[..., 1:]
    assert view.data_ptr() % 16 == x.element_size()
    return view


# ---- the chain of csrc/ffn_bf16_train_math.h in float64 ------------------------------------------------------------------------------
def _r16(t):
    """bf16_rne of float64 values that are exact in fp32."""
    f = t.float()
    assert torch.equal(f.double(), t)
    return f.bfloat16().double()


def chain64(form, x, params, eps, f1, f2, G, rounded=True, relu=True, drop_m1_in_dz=False):
    """[out, dx, dW1, db1, dW2, db2, dscale] in float64 by the chain of the header: with its bf16_rne roundings at the named points and
    max(z, 0) for gelu (the exact-answer truth), or with neither (rounded = relu = False: the analytic gradient, for the yardstick's
    self-test).  drop_m1_in_dz: the mutation that leaves M1 out of dz."""
    r16 = _r16 if rounded else (lambda t: t)
    rT = r16 if (rounded and form == "A") else (lambda t: t)
    x, G = x.double(), G.double()
    w1, b1, w2, b2, scale = (p.double() for p in params)
    f1, f2 = f1.reshape(-1, f1.shape[-1]), f2.reshape(-1, f2.shape[-1])
    D = x.shape[-1]
    if relu:
        act, dact = torch.relu, (lambda z: (z > 0).double())
    else:
        act = lambda z: 0.5 * z * torch.special.erfc(-z / 2.0 ** 0.5)
        dact = lambda z: 0.5 * torch.special.erfc(-z / 2.0 ** 0.5) + z * torch.exp(-0.5 * z * z) / (2.0 * torch.pi) ** 0.5
    rs = torch.rsqrt(x.pow(2).mean(dim=-1, keepdim=True) + eps)
    xn = x * rs
    xh, wh1, wh2 = r16(xn), r16(w1), r16(w2)
    h = xh @ wh1.T + b1
    zs = r16(h)
    a = r16(act(h) * f1)
    y = a @ wh2.T + b2
    ys = rT(y)
    out = rT(x + (y * f2) * scale)
    dyf = (G * scale) * f2
    dyh = r16(dyf)
    dscale = (G * (ys * f2)).sum(0)
    db2 = dyf.sum(0)
    da = dyh @ wh2
    dzf = (da if drop_m1_in_dz else da * f1) * dact(zs)
    dzh = r16(dzf)
    ah = r16(act(zs) * f1)
    db1 = dzh.sum(0)
    dW2 = dyh.T @ ah
    dW1 = dzh.T @ xh
    dxn = dzh @ wh1
    t = (dxn * xn).sum(-1, keepdim=True)
    dx = rT(G + rs * (dxn - xn * (t / D)))
    parts = dict(x=x, xh=xh, wh1=wh1, wh2=wh2, b1=b1, b2=b2, h=h, a=a, ah=ah, y=y, f2=f2, scale=scale, G=G, dyf=dyf, dyh=dyh, ys=ys, dzh=dzh,
                 dxn=dxn, xn=xn, t=t, zs=zs)
    return [out, dx, rT(dW1), rT(db1), rT(dW2), rT(db2), rT(dscale)], parts


def _grid_ok(t):
    """Every value is an integer over one power of two (2^0 .. 2^14), below 2^23 on that grid: sums of such terms are exact in fp32
    whatever their order."""
    for k in range(15):
        q = t * 2.0 ** k
        if bool((q == q.round()).all()):
            return float(q.abs().max()) < 2.0 ** 23
    return False


@functools.lru_cache(maxsize=None)
def exact_case(form, rows, D, hidden, seed=99):
    """ffn_train_common.exact_case's inputs (all of them exact in bf16) in the form's dtype, the chain's float64 answer with its roundings
    as the truth, and `exact`: every sum of ABSOLUTE terms of the chain lies on a grid as _grid_ok says (so every partial sum is exact in
    fp32 in any order), gelu is max(z, 0) (|z| >= 24, an integer), the recomputed ah equals the forward's a, and t / D is exact."""
    base = tc.exact_case(rows, D, hidden, seed)
    dt = dtype_of(form)
    x, G = base["x"].to(dt), base["G"].to(dt)
    params = tuple(p.to(dt) for p in base["params"])
    assert all(torch.equal(a.float(), b) for a, b in zip((x, G, *params), (base["x"], base["G"], *base["params"])))
    f1, f2 = tc.masks_for(seed, base["x"], hidden, 0.5, 0.5)
    truth, p = chain64(form, x, params, 0.0, f1, f2, G)
    ab = torch.abs
    sums = [ab(p["xh"]) @ ab(p["wh1"]).T + ab(p["b1"]),                            # h
            ab(p["a"]) @ ab(p["wh2"]).T + ab(p["b2"]),                             # y
            ab(p["x"]) + ab(p["y"] * p["f2"] * p["scale"]),                        # out before its rounding
            ab(p["dyf"]).sum(0), (ab(p["G"]) * ab(p["ys"] * p["f2"])).sum(0),      # db2, dscale
            ab(p["dyh"]) @ ab(p["wh2"]),                                           # da
            ab(p["dzh"]).sum(0), ab(p["dyh"]).T @ ab(p["ah"]), ab(p["dzh"]).T @ ab(p["xh"]),       # db1, dW2, dW1
            ab(p["dzh"]) @ ab(p["wh1"]),                                           # dxn
            (ab(p["dxn"]) * ab(p["xn"])).sum(-1), p["t"] / D,                      # t and t / D
            ab(p["G"]) + ab(p["dxn"]) + ab(p["xn"]) * ab(p["t"] / D)]              # dx before its rounding
    exact = all(_grid_ok(s) for s in sums)
    exact = exact and bool((p["h"].abs() >= 24).all()) and bool((p["h"] == p["h"].round()).all()) and torch.equal(p["zs"], p["h"])
    exact = exact and torch.equal(p["a"], p["ah"]) and bool((p["xn"] == p["x"]).all()) and (D & (D - 1)) == 0
    exact = exact and bool((torch.nn.functional.gelu(p["h"].float()) == torch.relu(p["h"].float())).all())
    return dict(form=form, x=x, G=G, params=params, eps=0.0, truth=truth, exact=exact, D=D, hidden=hidden, p1=0.5, p2=0.5, seed=seed,
                gates=[0.0] * 7, e_stock=[0.0] * 7)
