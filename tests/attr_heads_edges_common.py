"""Shared by the CPU and GPU tests of the attribute heads at their edges (tests/test_attr_heads_edges.py): the shape grid with head
sizes other than 128 / 4, the row and layout edges of the backward, direct calls of the torch ops with a workspace of the test's own,
and the per-element running error bounds of the training forward and of the nine gradients.

Yardstick and gate: attr_heads_common / attr_heads_train_common, unchanged.  The bounds follow attr_heads_common.truth_and_bound:
float64, u = 2^-24, gamma_n = n u / (1 - n u), first order in u.  Per head, with x = [a | b | a b] in float64 from the fp32 ctx,
z = W1 x + b1, Phi and phi the normal distribution and density, g = gelu(z) = z Phi, g' = Phi + z phi, M = keep / (1 - p) (1 where
p = 0), A = g M, dA = dOut W2, dz = dA M g', R = HEADS_BWD_ROW_CHUNK, nch = ceil(K / R), H = Hv + Ho:

    z      E1   = gamma_{3D+1} (|x| |W1| + |b1|) + u |a b| |W1 third|          the chain of 3D fma and the bias; the product's rounding
    g      dg   = 1.13 E1 + 4 u (|z| + |g|)                                    |gelu'| < 1.13 carries E1; the evaluation of gelu
    A      EA   = (dg + 2 u |g|) M                                             the rounded scale and the multiplication (p > 0 only)
    out    E2   = gamma_{Hh+1} ((|A| + EA) |W2| + |b2|) + EA |W2|              the chains of the slices, their sum, the bias
    g'     Egp  = 0.8 E1 + 8 u (|Phi| + |z phi|)                               |gelu''| <= 2 phi(0) = 0.798 carries E1; the evaluation
    dA     EdA  = gamma_N |dOut| |W2|                                          the chain over the head's N outputs
    dz     Edz  = EdA M |g'| + |dA| M Egp + 3 u |dz|                           propagation; scale and two multiplications (1 u at p = 0)
    dW1    (gamma_{R+1} + gamma_{nch-1}) sum_i |x| |dz| + sum_i |x| Edz + u sum_i |a b| |dz|
                                                                               a chunk's chain, the chunks' sum; the product's rounding
    dW2    (gamma_{R+1} + gamma_{nch-1}) sum_i |A| |dOut| + sum_i EA |dOut|    likewise, with the error of A
    db1    sum_i Edz + (u + gamma_{nch-1}) sum_chunks |chunk sum| + K 2^-53 sum_i |dz|
                                                                               a chunk's sum is formed in double and rounded once
    db2    (u + gamma_{nch-1}) sum_chunks |chunk sum| + K 2^-53 sum_i |dOut|   (dOut is exact: nothing is propagated)
    dx     Edx  = gamma_H sum_j |dz| |W1| + sum_j Edz |W1|                     one chain over the packed columns of both heads
    ga     Ega  = Edx_a + Edx_ab |ctx_e| + u (|ga| + |dx_ab ctx_e|)            the fma; a route that rounds the product first (torch)
    dctx   per frame: the sum of its rows' Ega / Egb + gamma_{hits-1} sum |g|  hits ordered additions onto an exact zero

db2 is where the op and torch's fp32 route differ by construction: the op forms a chunk's sum in double and rounds once, torch sums
dOut in fp32, and nothing is propagated into db2 that would cover a running sum (torch's db2 exceeds u |sum| a thousandfold where
the column cancels).  The term of that route, gamma_K sum_i |dOut|, is added to the bound when torch's fp32 results are checked
against it (the validation of the derivation) and is NOT part of the bound the op is held to.  db1 needs no such term: the
propagated Edz covers torch's running sum.
"""
import copy
import functools
import math

import torch

import attr_heads_common as common
import attr_heads_train_common as tc

U = common.U
gamma = common.gamma
T, C = common.T_FRAMES, common.N_SEG * common.N_SYM
GRID = [(100, 70, 66, 128, 4), (68, 64, 65, 128, 4), (12, 20, 12, 200, 70), (260, 8, 8, 128, 4), (8, 6, 6, 3, 1)]   # (D, Hv, Ho, Nv, No)
P_MAIN = (0.1, 0.5)
P_EXTRA = [(0.0, 0.5), (0.5, 0.0), (0.9, 0.9)]              # at GRID[0] only
ROW_SHAPE = (20, 40, 24, 128, 4)
ROW_KS = [1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 511, 512, 513]
OUT_NAMES = ("logitsVelocity", "ofLogits") + tc.NAMES


def _R():
    from transkun_amd import attributes
    return attributes.HEADS_BWD_ROW_CHUNK


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def bounds(c):
    """(bound, torch's own term for db2, hits per frame) of a case of attr_heads_train_common.make_case: the two lists in the order of
    OUT_NAMES (module docstring)."""
    ctx, pairs, offsets, K = c["ctx"], c["pairs"], c["offsets"], c["K"]
    a, b, chain = common.gather_ab(ctx.float().double(), pairs, offsets, K)
    D = a.shape[1]
    x, ab = torch.cat([a, b, a * b], dim=-1), (a * b).abs()
    R = _R()
    nch = (K + R - 1) // R
    g_rows = gamma(R + 1) + gamma(nch - 1)
    Hv, Ho = c["vp"][0].out_features, c["op"][0].out_features
    chunks = [slice(s, min(s + R, K)) for s in range(0, K, R)]

    def chunk_sums(t):                                      # sum over the chunks of |a chunk's column sum|
        return sum(t[s].sum(0).abs() for s in chunks)

    out = {}
    dx, Edx = 0.0, 0.0
    with torch.no_grad():
        for tag, head, m, p, dOut in (("v", c["vp"], c["mask"][:, :Hv], c["pv"], c["dlv"]), ("o", c["op"], c["mask"][:, Hv:], c["po"], c["dof"])):
            W1, b1, W2, b2 = (t.detach().double() for t in (head[0].weight, head[0].bias, head[-1].weight, head[-1].bias))
            dOut = dOut.double()
            Hh, N = W1.shape[0], W2.shape[0]
            z = x @ W1.t() + b1
            E1 = gamma(3 * D + 1) * (x.abs() @ W1.abs().t() + b1.abs()) + U * (ab @ W1[:, 2 * D:].abs().t())
            Phi, phi = 0.5 * torch.erfc(-z / math.sqrt(2.0)), torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
            g, gp = z * Phi, Phi + z * phi
            dg = 1.13 * E1 + 4 * U * (z.abs() + g.abs())
            M = m.double() / (1.0 - p) if p > 0 else torch.ones_like(z)
            A = g * M
            EA = (dg + 2 * U * g.abs()) * M if p > 0 else dg
            out[tag + "out"] = gamma(Hh + 1) * ((A.abs() + EA) @ W2.abs().t() + b2.abs()) + EA @ W2.abs().t()
            Egp = 0.8 * E1 + 8 * U * (Phi.abs() + (z * phi).abs())
            dA, EdA = dOut @ W2, gamma(N) * (dOut.abs() @ W2.abs())
            dz = dA * M * gp
            Edz = EdA * M * gp.abs() + dA.abs() * M * Egp + (3 if p > 0 else 1) * U * dz.abs()
            bw1 = g_rows * (dz.abs().t() @ x.abs()) + Edz.t() @ x.abs()
            bw1[:, 2 * D:] += U * (dz.abs().t() @ ab)
            out[tag + "1.weight"] = bw1
            out[tag + "2.weight"] = g_rows * (dOut.abs().t() @ A.abs()) + dOut.abs().t() @ EA
            dbl = K * 2.0 ** -53
            out[tag + "1.bias"] = Edz.sum(0) + (U + gamma(nch - 1)) * chunk_sums(dz) + dbl * dz.abs().sum(0)
            out[tag + "2.bias"] = (U + gamma(nch - 1)) * chunk_sums(dOut) + dbl * dOut.abs().sum(0)
            out[tag + "2.bias32"] = gamma(K) * dOut.abs().sum(0)        # a route that sums dOut in fp32 (torch): module docstring
            dx = dx + dz @ W1
            Edx = Edx + dz.abs() @ W1.abs() * gamma(Hv + Ho) + Edz @ W1.abs()
        ga, gb = dx[:, :D] + dx[:, 2 * D:] * b, dx[:, D:2 * D] + dx[:, 2 * D:] * a
        Ega = Edx[:, :D] + Edx[:, 2 * D:] * b.abs() + U * (ga.abs() + (dx[:, 2 * D:] * b).abs())
        Egb = Edx[:, D:2 * D] + Edx[:, 2 * D:] * a.abs() + U * (gb.abs() + (dx[:, 2 * D:] * a).abs())
        fa, fb = chain * T + pairs[:K, 0].long(), chain * T + pairs[:K, 1].long()
        idx = torch.cat([fa, fb])
        hits = torch.zeros(C * T, dtype=torch.float64).index_add_(0, idx, torch.ones(2 * K, dtype=torch.float64))
        prop = torch.zeros(C * T, D, dtype=torch.float64).index_add_(0, idx, torch.cat([Ega, Egb]))
        mass = torch.zeros(C * T, D, dtype=torch.float64).index_add_(0, idx, torch.cat([ga.abs(), gb.abs()]))
        gh = (hits - 1).clamp(min=0) * U
        bdctx = prop + (gh / (1.0 - gh))[:, None] * mass
    bound = [out["vout"], out["oout"], bdctx.view(common.N_SEG, common.N_SYM, T, D)] + \
            [out[h + k] for h in "vo" for k in ("1.weight", "1.bias", "2.weight", "2.bias")]
    extra = [torch.zeros_like(t) for t in bound]
    for at, key in ((6, "v2.bias32"), (10, "o2.bias32")):
        extra[at] = out[key]
    return bound, extra, hits.view(common.N_SEG, common.N_SYM, T)


def finish(c):
    """Adds the bounds and what torch's fp32 route uses of them (db2 with that route's own summation term) to a case."""
    c["bound"], extra, c["hits"] = bounds(c)
    use = []
    for f, t, bd, ex in zip(c["f32"], c["truth"], c["bound"], extra):
        err, lim = (f.double() - t).abs(), bd + ex
        assert bool((err[lim == 0] == 0).all())
        use.append(float((err[lim > 0] / lim[lim > 0]).max()) if bool((lim > 0).any()) else 0.0)
    c["use32"] = use
    return c


def check_bound(tag, got, c, names=OUT_NAMES):
    """Prints the fraction of the bound every tensor uses (and torch's fp32 route's), then asserts: the derivation holds for torch's
    fp32 route (use32 <= 1), every element is within its bound, and an element whose bound is exactly zero is exactly zero.
    Returns the worst fraction."""
    bad, worst = [], 0.0
    at = {n: i for i, n in enumerate(OUT_NAMES)}
    for name, g in zip(names, got):
        i = at[name]
        t, bd = c["truth"][i], c["bound"][i]
        g = g.detach().cpu().double()
        assert g.shape == t.shape, (name, g.shape, t.shape)
        err = (g - t).abs()
        live = bd > 0
        use = float((err[live] / bd[live]).max()) if bool(live.any()) else 0.0
        worst = max(worst, use)
        print(f"{tag} {name}: bound used {use:.4f} (torch fp32 {c['use32'][i]:.4f})  elements with a zero bound {int((~live).sum())}")
        assert c["use32"][i] <= 1.0, (name, c["use32"][i])
        if not (bool((err <= bd).all()) and bool((g[~live] == 0).all())):
            bad.append((name, use))
    assert not bad, bad
    return worst


# ---- cases, computed once ------------------------------------------------------------------------------------------------------------
def _seed(D, Hv, Ho, Nv, No, pv, po, K):
    return 5000 + 7 * D + Hv + 3 * Ho + Nv + 11 * No + int(100 * pv) + int(1000 * po) + 13 * K


@functools.lru_cache(maxsize=None)
def train_case(D, Hv, Ho, Nv, No, pv=P_MAIN[0], po=P_MAIN[1], K=common.K_GATE):
    return finish(tc.make_case(D, Hv, Ho, 1.0, pv, po, K, _seed(D, Hv, Ho, Nv, No, pv, po, K), Nv, No))


@functools.lru_cache(maxsize=None)
def eval_case(D, Hv, Ho, Nv, No):
    return common.make_gate_case(D, Hv, Ho, 1.0, 6000 + 7 * D + Hv + 3 * Ho + Nv + 11 * No, Nv, No)


def _draw_pairs(n, g):
    b = torch.randint(0, T, (n,), generator=g)
    e = torch.stack([torch.randint(int(x), T, (1,), generator=g)[0] for x in b]) if n else b
    return torch.stack([b, e], dim=1).to(torch.int32)


@functools.lru_cache(maxsize=None)
def layout_case(kind):
    """The layout edges of the backward on ROW_SHAPE.  "past": 30 rows behind offsets[-1] (the last chain, otherwise empty); "outside":
    a dozen rows with pairs outside [0, T - 1] (c["raw_pairs"]; c["pairs"] holds them clamped, as the yardstick reads them); "chain0" /
    "chainlast": every row in one chain; "frame": 200 rows with b == e == 3 in chain 2."""
    D, Hv, Ho, Nv, No = ROW_SHAPE
    K = common.K_GATE
    g = torch.Generator().manual_seed({"past": 71, "outside": 72, "chain0": 73, "chainlast": 74, "frame": 75}[kind])
    raw = None
    if kind == "past":
        pairs, offsets = common.pack_rows(common.make_rows(K, 7100))
        assert int(offsets[-1]) == K and int(offsets[-2]) == K            # chain 9 is empty
        pairs = torch.cat([pairs, _draw_pairs(30, g)])
        K += 30
    elif kind == "outside":
        pairs, offsets = common.pack_rows(common.make_rows(K, 7200))
        raw = pairs.clone()
        vals = torch.tensor([-3, -1, T, T + 5], dtype=torch.int32)
        for i in torch.randperm(K, generator=g)[:12].tolist():
            side = int(torch.randint(0, 3, (1,), generator=g))            # begin, end or both
            for s in ((0,), (1,), (0, 1))[side]:
                raw[i, s] = vals[int(torch.randint(0, 4, (1,), generator=g))]
        assert int(((raw < 0) | (raw > T - 1)).any(dim=1).sum()) == 12
        pairs = raw.clamp(0, T - 1)
    elif kind in ("chain0", "chainlast"):
        pairs = _draw_pairs(K, g)
        offsets = torch.zeros(C + 1, dtype=torch.int32)
        if kind == "chain0":
            offsets[1:] = K
        else:
            offsets[C] = K
    else:
        K = 200
        pairs = torch.full((K, 2), 3, dtype=torch.int32)
        offsets = torch.zeros(C + 1, dtype=torch.int32)
        offsets[3:] = K                                                   # chain 2
    c = finish(tc.make_case(D, Hv, Ho, 1.0, P_MAIN[0], P_MAIN[1], K, 7000 + len(kind) + K, Nv, No, layout=(pairs, offsets)))
    c["raw_pairs"] = raw
    return c


# ---- direct calls of the torch ops ----------------------------------------------------------------------------------------------------
def packed(dev, vp, op):
    """The packed weights of two heads on `dev` (copies: the cached cases stay unchanged)."""
    from transkun_amd import attributes
    vp2, op2 = copy.deepcopy(vp).to(dev), copy.deepcopy(op).to(dev)
    return dict(attributes._packed_heads(vp2, op2, train=True))


def _ws(dev, nbytes, fill, extra):
    if dev.type == "cpu":
        return torch.empty(0, dtype=torch.uint8)
    if not fill:
        return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return torch.full((int(nbytes) + extra,), 0xFF, dtype=torch.uint8, device=dev)       # every float a NaN, every int -1


def geometry(ctx4):
    """(x3, C, T, D, ldc) of a [N, SYM, T, D] fp32 tensor whose rows may be ldc >= D floats apart, as attributes forms them: no copy."""
    N, SYM, T_, D = ctx4.shape
    ldc = ctx4.stride(2)
    assert ctx4.stride(3) == 1 and ldc >= D and ctx4.stride(1) == T_ * ldc and ctx4.stride(0) == SYM * T_ * ldc
    return ctx4.as_strided((N * SYM, T_, D), (T_ * ldc, ldc, 1), ctx4.storage_offset()), N * SYM, T_, D, ldc


def direct_forward(dev, w, ctx4, pairs, offsets, K, train, seed=0, pv=0.0, po=0.0, poison=False):
    """semicrf_attribute_heads (train = False) or _train_fwd through the torch op, as attributes calls it.  poison: the workspace
    4 KiB larger than its size and full of NaN, every output buffer pre-filled with NaN (-1 for the index outputs)."""
    from transkun_amd import _lib
    x3, C_, T_, D, ldc = geometry(ctx4)
    Hv, Ho, Nv, No = w["Hv"], w["Ho"], w["Nv"], w["No"]

    def buf(shape, dtype=torch.float32):
        if not poison:
            return torch.empty(shape, dtype=dtype, device=dev)
        return torch.full(shape, float("nan") if dtype == torch.float32 else -1, dtype=dtype, device=dev)

    lv, of, z = buf((K, Nv)), buf((K, No)), buf((K, Hv + Ho))
    sym, sc = buf((K,), torch.int64), buf((K,), torch.int64)
    lib = _lib.load()
    if train:
        ws = _ws(dev, lib.semicrf_attribute_heads_train_fwd_workspace_bytes(K, Hv, Ho, Nv, No), poison, 4096)
        _lib.ops().attribute_heads_train_fwd(x3, C_, T_, D, ldc, pairs, K, offsets, common.N_SYM, w["W1"], w["b1"], w["W2"], w["b2"], Hv, Ho, Nv,
                                             No, seed, pv, po, lv, of, z, sym, sc, ws)
        return lv, of, z, sym, sc
    ws = _ws(dev, lib.semicrf_attribute_heads_workspace_bytes(K, Hv, Ho, Nv, No), poison, 4096)
    _lib.ops().attribute_heads(x3, C_, T_, D, ldc, pairs, K, offsets, common.N_SYM, w["W1"], w["b1"], w["W2"], w["b2"], Hv, Ho, Nv, No, lv, of,
                               sym, sc, ws)
    return lv, of, sym, sc


def direct_backward(dev, w, dlv, dof, z, ctx4, pairs, offsets, K, seed, pv, po, poison=False):
    """semicrf_attribute_heads_bwd through the torch op -> (dctx, dW1, db1, dW2, db2), packed as the ABI states."""
    from transkun_amd import _lib
    x3, C_, T_, D, ldc = geometry(ctx4)
    Hv, Ho, Nv, No = w["Hv"], w["Ho"], w["Nv"], w["No"]
    H = Hv + Ho
    fill = float("nan") if poison else 0.0
    outs = [torch.full((n,), fill, dtype=torch.float32, device=dev) if poison else torch.empty(n, dtype=torch.float32, device=dev)
            for n in (C_ * T_ * D, 3 * D * H, H, Hv * Nv + Ho * No, Nv + No)]
    ws = _ws(dev, _lib.load().semicrf_attribute_heads_bwd_workspace_bytes(K, D, Hv, Ho, Nv, No), poison, 4096)
    _lib.ops().attribute_heads_bwd(dlv, dof, z, x3, C_, T_, D, ldc, pairs, K, offsets, w["W1"], w["W2"], Hv, Ho, Nv, No, seed, pv, po,
                                   outs[0].view(C_, T_, D), outs[1], outs[2], outs[3], outs[4], ws)
    return outs


def seed_arg(seed):
    from transkun_amd import attributes
    return attributes._seed_arg(seed)


def libm_free_z(K, H, seed):
    """z [K, H] whose entries are exact 0.0, +(16 + |n|) or -(16 + |n|), a third each: gelu and gelu' of such a z need no libm
    accuracy (erf(11.3) rounds to 1, erfc(11.3) and exp(-128) underflow to 0)."""
    g = torch.Generator().manual_seed(seed)
    cls = torch.randint(0, 3, (K, H), generator=g)
    mag = 16.0 + torch.randn(K, H, generator=g).abs()
    return torch.where(cls == 0, torch.zeros(K, H), torch.where(cls == 1, mag, -mag))
