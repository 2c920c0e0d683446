"""Shared by the CPU and GPU tests of the fused attribute heads (tests/test_attr_heads.py): seeded heads and inputs, the float64
yardstick, torch's own fp32 modules on identical inputs, and the per-element running error bound.

Yardstick: the same modules evaluated in float64 on the CPU, on x = [a | b | a * b] formed in float64 from the fp32 ctx (the product
exact).  The gate on the maximum absolute error over an output matrix is GATE x the error of torch's fp32 modules (CPU) against it on
identical inputs: one in-order chain of n additions has an expected rounding error about sqrt(b) times that of a b-way blocked sum,
b is unknown for the BLAS behind torch, and 8 = sqrt(64).

Per-element condition (float64, u = 2^-24, gamma_n = n u / (1 - n u)):
    layer 1   E1 = gamma_{3D+1} (|x| |W1| + |b1|) + u |a b| |W1 third|                    (the last term: the product's rounding)
    GELU      dg = 1.13 E1 + 4 u (|h| + |gelu h|)                                         (1.13 > max |gelu'|)
    layer 2   E2 = gamma_{H+1} ((|g| + dg) |W2| + |b2|) + dg |W2|
"""
import copy
import functools

import torch

U = 2.0 ** -24
GATE = 8.0
T_FRAMES, N_SEG, N_SYM = 12, 2, 5                       # C = 10 chains
EMPTY_CHAINS = (1, 4, 9)
SHAPES = [(8, 16, 16), (20, 40, 24), (5, 3, 1), (256, 512, 512)]       # (D, Hv, Ho)
SCALES = [1.0, 8.0]
K_GATE = 97                                             # >= 64 rows: the maximum over the matrix is a stable statistic


def gamma(n):
    return n * U / (1.0 - n * U)


def make_heads(D, Hv, Ho, seed, Nv=128, No=4, dropout=0.1):
    """The two heads as the transcriber builds them (Linear, GELU, Dropout, Linear), default initialisation from a seeded generator,
    eval mode."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        vp = torch.nn.Sequential(torch.nn.Linear(3 * D, Hv), torch.nn.GELU(), torch.nn.Dropout(dropout), torch.nn.Linear(Hv, Nv))
        op = torch.nn.Sequential(torch.nn.Linear(3 * D, Ho), torch.nn.GELU(), torch.nn.Dropout(dropout), torch.nn.Linear(Ho, No))
    return vp.eval(), op.eval()


def pack_rows(rows, C=N_SEG * N_SYM):
    """rows: (chain, begin, end), ascending in chain -> pairs int32 [K, 2], offsets int32 [C + 1]."""
    assert all(rows[i][0] <= rows[i + 1][0] for i in range(len(rows) - 1))
    pairs = torch.tensor([[b, e] for _, b, e in rows], dtype=torch.int32).reshape(-1, 2)
    counts = torch.zeros(C, dtype=torch.int64)
    for c, _, _ in rows:
        counts[c] += 1
    offsets = torch.zeros(C + 1, dtype=torch.int32)
    offsets[1:] = counts.cumsum(0)
    return pairs, offsets


def make_rows(K, seed, T=T_FRAMES, C=N_SEG * N_SYM, empty=EMPTY_CHAINS):
    """K rows over the non-empty chains, seeded; the first rows are the edge pairs b == e, b = 0, e = T - 1 (as far as K allows)."""
    g = torch.Generator().manual_seed(seed)
    live = [c for c in range(C) if c not in empty]
    edge = [(0, 0), (T - 1, T - 1), (0, T - 1), (3, 3), (0, 1), (T - 2, T - 1)]
    rows = []
    for i in range(K):
        c = live[int(torch.randint(0, len(live), (1,), generator=g))]
        if i < len(edge):
            b, e = edge[i]
        else:
            b = int(torch.randint(0, T, (1,), generator=g)); e = int(torch.randint(b, T, (1,), generator=g))
        rows.append((c, b, e))
    rows.sort(key=lambda r: r[0])
    return rows


def make_ctx(D, scale, seed, T=T_FRAMES):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N_SEG, N_SYM, T, D, generator=g) * scale


def chains_of(offsets, K):
    """chain_of_interval for every row: the largest c with offsets[c] <= i (rows past offsets[-1] get the last chain)."""
    C = offsets.numel() - 1
    c = torch.searchsorted(offsets[1:].long().contiguous(), torch.arange(K), right=True)
    return torch.clamp(c, max=C - 1)


def gather_ab(ctx, pairs, offsets, K):
    N, SYM, T, D = ctx.shape
    chain = chains_of(offsets, K)
    c3 = ctx.reshape(N * SYM, T, D)
    return c3[chain, pairs[:K, 0].long()], c3[chain, pairs[:K, 1].long()], chain


def torch_fp32(ctx, pairs, offsets, K, vp, op):
    """torch's own fp32 modules (CPU) on the identical inputs."""
    a, b, _ = gather_ab(ctx.float(), pairs, offsets, K)
    x = torch.cat([a, b, a * b], dim=-1)
    with torch.no_grad():
        return vp(x), op(x)


def truth_and_bound(ctx, pairs, offsets, K, vp, op):
    """The float64 yardstick (logitsVelocity, ofLogits) and the per-element running error bounds (module docstring)."""
    a, b, chain = gather_ab(ctx.float().double(), pairs, offsets, K)
    x = torch.cat([a, b, a * b], dim=-1)
    D = a.shape[1]
    out, bound = [], []
    with torch.no_grad():
        for head in (vp, op):
            h64 = copy.deepcopy(head).double()
            l1, l2 = h64[0], h64[-1]
            W1, b1, W2, b2 = l1.weight, l1.bias, l2.weight, l2.bias
            h = x @ W1.t() + b1
            g = torch.nn.functional.gelu(h)
            y = g @ W2.t() + b2
            E1 = gamma(3 * D + 1) * (x.abs() @ W1.abs().t() + b1.abs()) + U * ((a * b).abs() @ W1[:, 2 * D:].abs().t())
            dg = 1.13 * E1 + 4 * U * (h.abs() + g.abs())
            H = W1.shape[0]
            E2 = gamma(H + 1) * ((g.abs() + dg) @ W2.abs().t() + b2.abs()) + dg @ W2.abs().t()
            out.append(y); bound.append(E2)
    return out[0], out[1], bound[0], bound[1], chain


def make_gate_case(D, Hv, Ho, scale, seed, Nv=128, No=4):
    """One case of the gate at K_GATE rows: inputs, yardstick, bounds, torch's fp32 error."""
    vp, op = make_heads(D, Hv, Ho, seed, Nv, No)
    ctx = make_ctx(D, scale, seed + 1)
    pairs, offsets = pack_rows(make_rows(K_GATE, seed + 2))
    tv, to, bv, bo, chain = truth_and_bound(ctx, pairs, offsets, K_GATE, vp, op)
    fv, fo = torch_fp32(ctx, pairs, offsets, K_GATE, vp, op)
    e32 = (float((fv.double() - tv).abs().max()), float((fo.double() - to).abs().max()))
    use32 = (float(((fv.double() - tv).abs() / bv).max()), float(((fo.double() - to).abs() / bo).max()))
    return dict(vp=vp, op=op, ctx=ctx, pairs=pairs, offsets=offsets, K=K_GATE, truth=(tv, to), bound=(bv, bo), e32=e32, use32=use32,
                chain=chain)


@functools.lru_cache(maxsize=None)
def gate_case(D, Hv, Ho, scale):
    """make_gate_case with the head sizes of the model, computed once and shared by the CPU and GPU forms."""
    return make_gate_case(D, Hv, Ho, scale, 1000 + 7 * D + Hv + int(scale))


def to_device(dev, vp, op, *tensors):
    """Copies of the heads and the tensors on `dev` (the cached cases stay unchanged on the CPU)."""
    vp2, op2 = copy.deepcopy(vp).to(dev).eval(), copy.deepcopy(op).to(dev).eval()
    return (vp2, op2) + tuple(t.to(dev) for t in tensors)


def fused(ctx, pairs, offsets, vp, op, K=None):
    from transkun_amd import attributes
    with torch.no_grad():
        return attributes.attribute_heads(ctx, pairs, offsets, vp, op, K)
