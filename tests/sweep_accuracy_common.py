"""What tests/test_sweep_accuracy.py is made of: the float64 yardstick of the sweeps' outputs, the input families, the PER-ELEMENT error
bounds of alpha / beta / logZ (log domain), of the marginals (log domain), of logProb's path cells and of dNoise (absolute), the check
that applies them, and the gate of today's suite that the mutants of tests/test_sweep_accuracy.py are also held against.

Yardstick.  oracle.forward_backward_f64 on the same fp32 inputs, for a subset of chains where the batch is large (`chain_subset`);
logProb's backward and a cotangent other than 1 are restated here in float64 numpy (`check_dense` with `paths`, `want_logprob`).

Bounds.  u = 2^-24, natural-log units.  log-sum-exp is a convex combination of its inputs: the error of alpha[t] is at most a convex
combination of the errors of the alpha[j] it was formed from, plus the roundings of its own step.  Walking back along the worst chain
of steps, an element with n recurrence steps behind it (alpha[t]: t + 1, beta[t]: T - t, logZ: T) satisfies

    |got - truth| <= u ( (a n + b) A_c  +  s n P_c  +  c0 n  +  c1 n^2 / 2 )                                         (LOG)

(the persistent sweep has two c0: one for the steps at positions below PB FAR0 = 64, which have no far field, one for the others)

  A_c  the chain's largest magnitude among alpha, beta, logZ, the scores of the lower triangle and the noise (from the float64 truth);
       a counts the roundings of one step whose operand has that size (an addition at |alpha|, a product cell * log2e), b those made
       once per output;
  P_c  the chain's largest softplus(diagonal score); s counts the roundings inside softplus, which scale with its value;
  c0   the roundings of one step at magnitude one, in units of u: the exp2 / log2 (v_exp_f32, v_log_f32: 1 ulp = 2u relative, the
       figure of the CDNA ISA guide; libm / OCML expf, logf 1 ulp, log1pf 2 ulp), the additions of the linear-domain sums, and the
       roundings of differences that are small whenever their term has weight (|x| 2^x <= 0.54);
  c1   per term of a sum that grows with the row: a serial fp32 sum of k positive terms is off by at most (k - 1) u relative, and
       summing that over the steps gives n^2 / 2.

The constants are counted per implementation, below at `ROWSEQ` and `PERSIST`, operation by operation with the line of the kernel.
They are worst-case counts: nothing here was fitted to a result of the device, the host mirror or the oracle.  The fp32 oracle
(oracle.forward_backward, the plain recurrence with one rounding more per step than rowseq.hip) sits 38 to 3000 times inside them
(test_fp32_oracle_is_inside_every_bound prints the figures).

Marginals (dScore for end >= begin, interval_marginals' out) are compared as ln|got| against ln|truth| with equal signs; the bound is
LOG(alpha, begin side) + LOG(beta, end side) + LOG(logZ) + the roundings of the marginal's own expression (`E_CELL`).  A path cell of
logProb's backward holds gout (1 - m): absolute, |gout| (m (e^bound - 1) + 2u).  dNoise[t] is ONE term in both implementations --
gout gscale exp(alpha[t] + noise[t] + beta[t+1] - logZ), the marginal of the skip over gap t (persist_spine.h, the two `nv =` lines;
marginals.hip: noise_grad_kernel; cpu_ops.cpp: logz_bwd) -- so "the cells the kernel adds for that gap" is that single term and the
summation term is the two roundings of logProb's `+ gout` and `- gout`: |g| (m (e^bound - 1) + 3u).  The upper triangle is +0.0f.

Floor.  A cell whose true |value| is below 2^-100 |gout gscale| is not compared in the log domain (fp32 exp2 flushes near 2^-126): it
must be finite, of the right sign or zero, and below 2^-99 |gout gscale|.  `FLOOR_CAP` bounds the share of such cells per input family
and length; the test asserts it on the float64 truth before it looks at a result.

One operation of the persistent gradient sweep has a term of its own (`may_flush`).  The panels form a far-field marginal as
(gz 2^(M + arow)) * 2^(t - M) with the reference M of the accumulator of (row, chain, lane) (persist_panel.h, `mg[0][j] = gF * p0`),
and v_exp_f32 returns 0 for an argument below -126, so either factor can come back as 0 for a marginal far above the floor.  M is only
ever set by acc_lift, to floor(t*) + RESC_LIFT (96) for the larger term t* of a pair of cells the lane has just read; accumulators
start empty with every task (row block, column part of TPT tiles, 32 chains, row quarter) and a task walks its tiles in ascending
order.  Within one row and chain a marginal is 2^(t + arow) with one arow, so terms and marginals order alike, and:
  * 2^(M + arow) is 2^96 times the marginal m* of the cell that set M (within one binade): it is 0 only if m* < 2^-221.  So a cell
    can be lost this way only if an EARLIER cell of its row, chain and column part (a tile up to its own) has a marginal below 2^-220;
  * 2^(t - M) is 0 only if the cell's term lies 30 below t*: only if its marginal is below 2^-28 of the LARGEST marginal among those
    earlier cells.
(One binade of slack in each for the distance of the device's alpha, beta, logZ from the truth: a cell's whole bound is 0.7 binades at
T = 1024.)  A far-field cell of implementation 0 on the device for which either holds on the float64 truth may be exactly zero; where
it is not zero it must be inside the log bound, and no other cell may be zero.  `FLUSH_CAP` bounds the share of the compared cells that
the rule exempts, per family and length, and is asserted on the truth alone: none in `balanced` at any length.  (Measured on the
MI355X: `balanced` and `randn` return every cell accurately; `model` at 130 x 6 and 200 x 33 returns 34 and 96 far-field cells with
marginals between 2^-100 and 2^-75 as 0, all by the first route.)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -100                      # of |gout gscale|
FLOOR_TOP = 2.0 ** -99
FLUSH_SET = 2.0 ** -220                  # a cell that set the accumulator's reference had a marginal below this: the common factor is 0
FLUSH_REL = 2.0 ** -28                   # ... or the cell is this far below the largest marginal the accumulator has seen: its own factor is 0
GS, GP = 4, 32                           # chains per spine workgroup and per panel task (persist_common.h)


def _kernel_constants():
    """PB, FAR0 (= RING), TPT, LEADT as the kernel's own headers define them."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "transkun_amd", "csrc")
    tuning = open(os.path.join(csrc, "persist_tuning.h")).read()
    common = open(os.path.join(csrc, "persist_common.h")).read()
    macro = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)", tuning).group(1))
    assert re.search(r"constexpr int FAR0 = RING;", common) and re.search(r"constexpr int RING = SEMICRF_RING;", common)
    assert re.search(r"nfull_of\(int q\) \{ return q \+ 1 - LEADT >= 0 \? \(q \+ 1 - LEADT\) / TPT : 0; \}", common)
    assert re.search(r"RESC_LIFT = 96\.0f, RESC_HI = 108\.0f", common)
    return int(re.search(r"constexpr int PB = (\d+);", common).group(1)), macro("SEMICRF_RING"), macro("SEMICRF_TPT"), macro("SEMICRF_LEADT")


PB, FAR0, TPT, LEADT = _kernel_constants()


def nfull_of(q):                         # persist_common.h
    return (q + 1 - LEADT) // TPT if q + 1 - LEADT >= 0 else 0


def nparts_of(q):
    return nfull_of(q) + 1

# ---- the constants of LOG and of the marginal's own expression, per implementation ------------------------------------------------------
# ROWSEQ: rowseq.hip + marginals.hip (semicrf_set_impl(1), one chain, T = 1) and the host mirror (cpu_ops.cpp: logz_fwd / logz_bwd).
#   one step of rowseq_sweep_kernel, along the worst chain of operations:
#     t = u[rr] + score[cell]                     1 rounding at |alpha|                                    a += 1
#     lse_push: expf(t - nm)                      t - nm is small where the term has weight (0.4 u); expf 2u: once, the sum is convex
#     S = S * expf(M - nm) + expf(t - nm)         per push: product, sum, expf -> 4.4 u; ceil(k / 16) + 1 pushes of a slot and the skip
#                                                 (k terms, 16 slots)                                       c0 += 8.8, c1 += 4.4 / 16
#     lse_merge x 16                              two expf, two products, one sum each -> 5.4 u             c0 += 86.4
#     res = M + logf(S) + softplus_f(d)           logf: 2u |ln S| <= 2u ln(1025) = 13.9 u; two additions at |alpha|
#                                                                                                           a += 2, c0 += 13.9
#     softplus_f = log1pf(expf(d))                expf: 2u sigmoid(d) <= 2u; log1pf: 2 ulp = 4u of its value   s = 4, c0 += 2
#   the host mirror (logz_fwd) makes the same three roundings at |alpha| (vj + cell, mm + log, + softplus) and keeps its sums in double.
#   a = 3, b = 0, s = 4, c0 = 2.4 + 8.8 + 86.4 + 13.9 + 2 = 113.5 -> 114, c1 = 0.275.
#   the marginal: marginals_kernel  v + ((q - logZ) + s): |q - logZ| <= 2 A_c, the next sum <= A_c + |ln m|, the last one is ln m;
#     expf 2u, two products 2u.  logz_bwd of the host mirror: expf(vt + qe + cell - logZ): 2 A_c, 3 A_c, ln m.  The diagonal takes
#     2 softplus more (8 P_c + 4) and one rounding more at |ln m|.
#   E_CELL = 5 A_c + 8 P_c + 3 |ln m| + 8.
# PERSIST: persist_spine.h / persist_panel.h / persist_grad.h (log2 units inside; a rounding of size u |x| log2 units is u |x| ln 2
#   natural units and the magnitudes scale the other way, so the counts carry over).
#   one step (one row of a block), own operations of spine_role's diagonal phase:
#     mine = e + flog2(acc) + sp                  two additions at |alpha|                                  a += 2
#     flog2(acc), acc in [1, 17^16]               2u * 65.4 * ln 2                                          c0 += 90.7
#     softplus2: x * LOG2E, fexp2, flog2          u |x2| sigmoid + 0.22 u |x2| (the constant LOG2E is off by 0.22 u) + 2u + 2u of its value
#                                                                                                           s = 3.25, c0 += 2.3
#     acc = S fexp2(mx - e); 15 fmaf(Y[j], fexp2((e[j] - e) + d[j]), acc)
#                                                 3.4 u; per coefficient fexp2 2u + fmaf 1u; (e[j] - e) + d[j] <= 0 is rounded at its own
#                                                 size, its term weighs at most min(1, 2^(65 + x)): 50 u once   c0 += 3.4 + 45 + 50
#   the term it came in by (the largest of the three routes counts, the sum is convex):
#     the block's own triangle, first sub-diagonal:  a0 = s1 * LOG2E (1.22), wl = fmaxf + flog2(..) (1), d[j] = cj + sp (1),
#                                                 (e[j] - e) + d[j] with e[j] - e ~ -d (1)                  a += 4.22, c0 += 5.4
#     the band (shadow):  p = fmaf(X, LOG2E, u) (1.22); per batch of 16: the old sum's rescale 3.4 u, the terms 2.4 u, 16 additions;
#                                                 three batches                                             (a += 1.22) c0 += 65.4
#     the far field (panel_role, far_role):  u - M at |alpha| (1), fmaf at |e| <= 126 (87.3 u each for u - M's own part and the fmaf),
#                                                 LOG2E (0.22), fexp2 2u, 2 TPT additions per lane, flushed terms (each below 2^-30 of the
#                                                 largest: n / 64 u <= 32 u at T = 2048), the 8 slots 11.4 u, flog2(sum) 2u * 126 ln 2 = 174.7 u,
#                                                 mx + flog2(sum) (1); far_role: <= 11 parts * 3.4 u + 4 u, aM + flog2(aS) (1); the spine's
#                                                 acc_push1 3.4 u                                            (a += 3.22) c0 += 463.6
#   once per output: mine * LN2 (1.05).
#   The routes are alternatives for a term, so the largest counts, for c0 as for a -- but a partial sum also passes through what the
#   step does to it afterwards: the band's sum takes the spine's acc_push1 of the far value (3.4 u) on top, and every route the
#   diagonal phase.  Rows of the first FAR0 blocks have no far field.
#   a = 2 + 4.22 = 6.22 -> 6.25, b = 1.05 -> 1.1, s = 3.25, c1 = 0 (T <= 2048),
#   c0 = 90.7 + 2.3 + 98.4 + max(5.4, 65.4 + 3.4, 463.6) = 655 for a step at position >= PB FAR0, 191.4 + 65.4 = 256.8 -> 257 below.
#   the marginal: arow = (vfl - lzc) * LOG2E: a difference and a product of size <= 2 A_c (4.44);
#     band_role / the ring: fmaf(x, LOG2E, u) <= 2 A_c (2.22), + arow is log2 m, fexp2 2u, gz 2u                   6.66 A_c + |ln m| + 4
#     panel_role: fa = M + arow (|fa| <= 100 + |log2 m|: 69.3 u + |ln m|), fexp2 2u, three products, and p0's exponent: u - M (1 at
#       |alpha|, 87.3 u), fmaf 87.3 u, fexp2 2u                                                                 5.66 A_c + |ln m| + 251
#     the diagonal (spine_role): arow + mine (2), draw = d * LOG2E (1.22), + draw (3), - 2 sp (ln m; 6.5 P_c + 4.6)
#                                                                                                            10.66 A_c + 6.5 P_c + |ln m| + 9
#     dNoise: nz * LOG2E (1.22), um1 + .. (2), + arow (ln m)                                                    7.66 A_c + |ln m| + 4
#   E_CELL = 11 A_c + 6.5 P_c + |ln m| + 256 (the largest of each).
# interval_marginals (posterior_cell.h, on v / q / logZ of either implementation): (vb + s) + (q - logZ): 2 A_c, 2 A_c, ln m;
#   __expf = exp2(x log2e): 1.22 |ln m| + 2u; single_marg: five roundings of at most 2 A_c + |ln m| and two softplus.  It takes ROWSEQ's
#   E_CELL on top of the LOG bounds of the implementation that produced its inputs; the host mirror evaluates in double.
ROWSEQ = dict(name="rowseq", a=3.0, b=0.0, s=4.0, c0=114.0, c0_near=114.0, c1=0.275, ea=5.0, ep=8.0, el=3.0, e1=8.0)
PERSIST = dict(name="persist", a=6.25, b=1.1, s=3.25, c0=655.0, c0_near=257.0, c1=0.0, ea=11.0, ep=6.5, el=1.0, e1=256.0)
T_MAX = 2048                             # PERSIST's c0 counts at most 11 column parts and 32 u of flushed terms


def impl_of(which, T, B, impl):
    """The constants of the kernels a call reaches (api.hip: use_persist)."""
    return PERSIST if (which == "gpu" and impl == 0 and B >= 2 and T >= 2) else ROWSEQ


# ---- input families ----------------------------------------------------------------------------------------------------------------------
def balanced(T, B, seed):
    """score[e][b][c] = 0.5 (e - b) - 5 + 0.3 N(0,1), noise = 0.3 N(0,1): every cell of the lower triangle carries weight (the smallest
    marginal is 4.7e-5 at T = 70 and 9.5e-9 at T = 520), so a dropped tile or column part moves every alpha behind it.  The cells above
    the diagonal, which nothing reads, hold the same expression."""
    rng = np.random.default_rng(seed)
    score = torch.empty(T, T, B, dtype=torch.float32)
    b = torch.arange(T, dtype=torch.float32)[None, :, None]
    rows = max(1, (1 << 23) // (T * B))
    for r in range(0, T, rows):
        n = min(rows, T - r)
        z = torch.from_numpy(rng.standard_normal((n, T, B), dtype=np.float32))
        e = torch.arange(r, r + n, dtype=torch.float32)[:, None, None]
        score[r:r + n] = z.mul_(0.3).add_(0.5 * (e - b) - 5.0)
    noise = torch.from_numpy((0.3 * rng.standard_normal((max(T - 1, 0), B), dtype=np.float32)))
    return score.contiguous(), noise.contiguous()


def make_inputs(family, T, B, seed):
    from transkun_amd import synth
    if family == "balanced":
        return balanced(T, B, seed)
    if family == "huge":
        from conftest import edge_inputs
        return edge_inputs(T, B, "model", seed, "huge")
    s, n = synth.crf_inputs(T, B, seed, "cpu", family)
    return s.contiguous(), n.contiguous()


# share of the cells end >= begin whose true marginal is below FLOOR, at most: (family, T) -> cap.  balanced: none; randn and model at
# T = 70: 25 % (23.3 % and 15.8 % measured on the float64 truth of the test's inputs).  The other lengths, measured the same
# way and rounded up: randn 0 / 0 / 20.2 / 52.3 / 67.6 / 80.2 % at T = 17 / 33 / 65 / 130 / 200 / 340, model 45.0 / 61.7 % at 130 / 200;
# `huge` (scores times 4000: A_c = 1.4e5) keeps 1 % of its cells above the floor -- it is there for alpha, beta and logZ
FLOOR_CAP = {("randn", 17): 0.0, ("randn", 33): 0.0, ("randn", 65): 0.25, ("randn", 70): 0.25, ("model", 70): 0.25,
             ("randn", 130): 0.55, ("model", 130): 0.50, ("randn", 200): 0.70, ("model", 200): 0.65, ("randn", 340): 0.82,
             ("huge", 48): 0.99}


# share of the compared cells that `may_flush` exempts, at most, on the float64 truth: (family, T) -> cap; `balanced`: none
# (measured: model 0.01 / 0.68 / 0.90 % at T = 70 / 130 / 200 -- 4 / 81 / 88 % of the few far-field cells it has above the floor; randn none)
FLUSH_CAP = {("model", 70): 0.001, ("model", 130): 0.01, ("model", 200): 0.012}


def flush_cap(family, T):
    return 0.0 if family == "balanced" else FLUSH_CAP.get((family, T), 0.0)


def floor_cap(family, T):
    return 0.0 if family == "balanced" else FLOOR_CAP[(family, T)]


def chain_subset(B):
    """All chains up to 12; beyond: the first four, four in the middle that straddle a 32-chain panel group, the last four."""
    if B <= 12:
        return list(range(B))
    mid = max(6, min(B - 6, (B // 2) // GP * GP))            # a group boundary near the middle (or the middle itself)
    return sorted(set(list(range(4)) + [mid - 2, mid - 1, mid, mid + 1] + list(range(B - 4, B))))


# ---- target paths and cotangents -----------------------------------------------------------------------------------------------------------
def target_paths(T, B):
    """Per chain, by c % 4: the full-length interval; every frame a singleton; a mix of singletons and longer intervals from the first
    frame to the last with gaps between them; the two boundary singletons with a long interval in between.  Begins ascend strictly
    and no interval begins inside the previous one (the path table's precondition)."""
    out = []
    for c in range(B):
        k = c % 4
        if k == 0 or T < 6:
            out.append([(0, T - 1)])
        elif k == 1:
            out.append([(t, t) for t in range(T)])
        elif k == 2:
            lens, lst, t, i = (0, 4, 0, 21, 1, 40), [], 0, c
            while t < T:
                e = min(t + lens[i % len(lens)], T - 1)
                if T - 1 - e <= 2:
                    e = T - 1                                   # the last interval ends on the last frame
                lst.append((t, e))
                t, i = e + 2, i + 1
            out.append(lst)
        else:
            out.append([(0, 0), (2, T - 3), (T - 1, T - 1)])
    return out


def mixed_gout(B, seed=0):
    """Per-chain cotangent of mixed sign, one exact zero, fp32 values (float64 numpy)."""
    rs = np.random.RandomState(977 + seed)
    w = rs.uniform(0.25, 2.0, B) * np.where(np.arange(B) % 3 == 1, -1.0, 1.0)
    w[B // 2] = 0.0 if B > 2 else w[B // 2]
    if B > 1:
        w[B - 1] = -37.5
    return w.astype(np.float32).astype(np.float64)


# ---- the float64 truth of a case --------------------------------------------------------------------------------------------------------------
class Truth:
    """The yardstick of one (family, T, B): float64 logZ, alpha, beta, marginals and noise marginals of the chains `idx`, the magnitudes
    A_c and P_c, and the share of cells under the floor."""

    def __init__(self, oracle, score, noise, idx=None):
        T, B = score.shape[0], score.shape[2]
        self.T, self.B = T, B
        self.idx = list(range(B)) if idx is None else list(idx)
        ix = torch.tensor(self.idx)
        s = score.index_select(2, ix).numpy()
        n = noise.index_select(1, ix).numpy()
        self.lz, self.m, self.mn, self.v, self.q = oracle.forward_backward_f64(s, n)
        self.tril = np.tril(np.ones((T, T), dtype=bool))
        tri3 = self.tril[:, :, None]
        diag = np.diagonal(s, axis1=0, axis2=1).T.astype(np.float64)                        # [T, n]
        self.P = np.max(np.maximum(diag, 0.0) + np.log1p(np.exp(-np.abs(diag))), axis=0)     # softplus, [n]
        smax = np.max(np.abs(np.where(tri3, s, 0.0)), axis=(0, 1))
        nmax = np.max(np.abs(n), axis=0) if T > 1 else np.zeros(len(self.idx))
        self.A = np.maximum.reduce([np.max(np.abs(self.v), axis=0), np.max(np.abs(self.q), axis=0), np.abs(self.lz), smax, nmax])
        cells = self.m[self.tril]                                                            # [cells, n]
        self.under_floor = float(np.mean(cells < FLOOR))
        self.min_marginal = float(cells.min())

    # LOG of the module docstring for n steps (an array broadcast against the chains)
    def log_bound(self, n, K):
        n = np.asarray(n, dtype=np.float64)
        assert self.T <= T_MAX
        near = np.minimum(n, float(PB * FAR0))               # the steps at positions below PB FAR0 (c0_near), the others (c0)
        return U * ((K["a"] * n + K["b"]) * self.A + K["s"] * n * self.P + K["c0_near"] * near + K["c0"] * (n - near) + K["c1"] * n * n / 2.0)

    def alpha_bound(self, K):                                    # [T, n]
        return self.log_bound(np.arange(1, self.T + 1)[:, None], K)

    def beta_bound(self, K):
        return self.log_bound(np.arange(self.T, 0, -1)[:, None], K)

    def logz_bound(self, K):                                     # [n]
        return self.log_bound(float(self.T), K)

    def cell_bound(self, K, KE=None):
        """[T, T, n] log-domain bound of the marginal of (end e, begin b), e >= b: alpha at the begin side, beta at the end side, logZ,
        and the marginal's own expression (KE: the constants of the kernel that evaluates it, K: of those that made alpha / beta / logZ)."""
        KE = K if KE is None else KE
        lnm = np.abs(np.log(np.maximum(self.m, 1e-300)))
        own = U * (KE["ea"] * self.A + KE["ep"] * self.P + KE["el"] * lnm + KE["e1"])
        return self.alpha_bound(K)[None, :, :] + self.beta_bound(K)[:, None, :] + self.logz_bound(K) + own

    def gap_bound(self, K):
        """[T-1, n]: the skip over gap t = alpha[t] + noise[t] + beta[t+1] - logZ."""
        lnm = np.abs(np.log(np.maximum(self.mn, 1e-300)))
        own = U * (K["ea"] * self.A + K["ep"] * self.P + K["el"] * lnm + K["e1"])
        return self.alpha_bound(K)[:-1] + self.beta_bound(K)[1:] + self.logz_bound(K) + own

    def far_mask(self):
        """[T, T] cells (e, b) the panels of the persistent gradient sweep write: position pi = T-1-b in row block k >= FAR0, position
        pj = T-1-e in a tile m <= k - FAR0."""
        T = self.T
        pi = (T - 1 - np.arange(T))[None, :]
        pj = (T - 1 - np.arange(T))[:, None]
        return pj < PB * (pi // PB - (FAR0 - 1))

    def may_flush(self):
        """[T, T, n] far-field cells that the persistent gradient sweep may store as exactly 0 (module docstring): by the float64
        marginals of the cells its accumulator has read before -- same begin frame and chain, the tiles of its column part up to its own."""
        T = self.T
        far = self.far_mask()
        out = np.zeros(self.m.shape, dtype=bool)
        pos = T - 1 - np.arange(T)                               # position of a frame in the descending sweep
        for b in range(T):
            k = pos[b] // PB
            if k < FAR0:
                continue
            q = k - FAR0
            for part in range(nparts_of(q)):
                m0 = part * TPT
                m1 = m0 + TPT if part < nfull_of(q) else q + 1
                # end frames of the part, in the order the task reads them: tiles ascending = positions ascending = frames descending
                e_hi, e_lo = T - 1 - m0 * PB, T - 1 - (m1 * PB - 1)
                ends = np.arange(e_hi, e_lo - 1, -1)
                assert far[ends, b].all()
                col = self.m[ends, b, :]                          # [cells, n]
                tile_last = ((np.arange(len(ends)) // PB) + 1) * PB - 1          # the last cell of a cell's own tile
                lo = np.minimum.accumulate(col, axis=0)[tile_last]
                hi = np.maximum.accumulate(col, axis=0)[tile_last]
                out[ends, b, :] = (lo < FLUSH_SET) | (col < FLUSH_REL * hi)
        return out

    def flush_share(self):
        """Share of the compared cells (end >= begin, above the floor) that may_flush exempts."""
        cmp_ = self.tril[:, :, None] & (self.m >= FLOOR)
        return float(np.sum(self.may_flush() & cmp_)) / max(int(np.sum(cmp_)), 1)


# ---- the checks: every one returns the worst error / bound of what it compared ------------------------------------------------------------
def check_log(what, got, truth, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    assert np.all(np.isfinite(got)), f"{what}: {int(np.sum(~np.isfinite(got)))} values are not finite"
    ratio = np.abs(got - truth) / np.broadcast_to(bound, truth.shape)
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: element {i}: got {got[i]!r}, float64 {truth[i]!r}, error {abs(got[i] - truth[i]):.3e} is "
                             f"{worst:.2f} times its bound {np.broadcast_to(bound, truth.shape)[i]:.3e}")
    return worst


def check_values(what, got, m, g, bound, flush=None):
    """Values g * m (g [n] per chain, m the true marginal, any leading shape) in the log domain with equal signs; under the floor:
    finite, the right sign or zero, below FLOOR_TOP |g|.  flush: cells that may be exactly zero instead."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == m.shape, (what, got.shape, m.shape)
    assert np.all(np.isfinite(got)), f"{what}: {int(np.sum(~np.isfinite(got)))} values are not finite"
    g = np.broadcast_to(np.asarray(g, dtype=np.float64), m.shape)
    want = g * m
    ag = np.abs(g)
    zero_g = ag == 0.0
    assert np.all(got[zero_g] == 0.0), f"{what}: a chain with a zero cotangent holds nonzero values"
    sign_ok = (got == 0.0) | (np.sign(got) == np.sign(want))
    assert np.all(sign_ok), f"{what}: {int(np.sum(~sign_ok))} values have the wrong sign"
    small = (np.abs(want) < FLOOR * ag) & ~zero_g
    assert np.all(np.abs(got[small]) < FLOOR_TOP * ag[small]), f"{what}: a cell under the floor holds a value above 2^-99 |g|"
    big = ~small & ~zero_g
    if flush is not None:
        big = big & ~(np.broadcast_to(flush, m.shape) & (got == 0.0))
    if not big.any():
        return 0.0
    gb, wb = got[big], want[big]
    if np.any(gb == 0.0):
        k = int(np.sum(gb == 0.0))
        raise AssertionError(f"{what}: {k} cells are zero whose float64 value is above the floor (the largest: {np.abs(wb[gb == 0.0]).max():.3e})")
    ratio = np.abs(np.log(np.abs(gb)) - np.log(np.abs(wb))) / np.broadcast_to(bound, m.shape)[big]
    worst = float(ratio.max())
    if worst > 1.0:
        j = int(np.argmax(ratio))
        i = tuple(int(x[j]) for x in np.nonzero(big))
        raise AssertionError(f"{what}: element {i}: got {gb[j]!r}, float64 {wb[j]!r}: |ln got - ln truth| = "
                             f"{abs(math.log(abs(gb[j])) - math.log(abs(wb[j]))):.3e} is {worst:.2f} times its bound")
    return worst


def check_abs(what, got, want, bound):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), f"{what}: values that are not finite"
    if not got.size:
        return 0.0
    err = np.abs(got - want)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(int(np.argmax(err - bound)), err.shape)
        raise AssertionError(f"{what}: element {i}: got {got[i]!r}, float64 {want[i]!r}: error {err[i]:.3e} against {np.broadcast_to(bound, err.shape)[i]:.3e}")
    return float(np.max(err / np.maximum(bound, 1e-300)))


def check_dense(what, dS, dN, tr, g, K, paths=None, flush=False):
    """The dense gradient dS [T, T, n] and dN [T-1, n] of the chains tr.idx against g[c] * marginal (paths None: logZ's backward, g =
    gout gscale) or against logProb's g[c] (indicator - marginal) and g[c] (1 - cover - noise marginal) (paths: per chain of tr.idx).
    Returns {"cells", "dNoise"[, "path"]} -> worst ratio."""
    T = tr.T
    dS = np.asarray(dS, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    upper = ~tr.tril
    up = np.asarray(dS)[upper]
    assert np.all(up == 0.0) and not np.any(np.signbit(up)), f"{what}: the upper triangle is not +0.0"
    cb = tr.cell_bound(K)
    fl = tr.may_flush() if flush else None
    res = {}
    if paths is None:
        res["cells"] = check_values(what + " dScore", dS[tr.tril], tr.m[tr.tril], g, cb[tr.tril], None if fl is None else fl[tr.tril])
        want_n = g * tr.mn
        res["dNoise"] = check_abs(what + " dNoise", dN, want_n, np.abs(g) * (tr.mn * np.expm1(tr.gap_bound(K)) + 3 * U)) if T > 1 else 0.0
        return res
    on = np.zeros((T, T, len(tr.idx)), dtype=bool)
    cover = np.zeros((T + 1, len(tr.idx)))
    for j, lst in enumerate(paths):
        for b, e in lst:
            on[e, b, j] = True
            cover[b, j] += 1
            cover[e, j] -= 1
    cover = np.cumsum(cover, axis=0)[:max(T - 1, 0)]
    off = tr.tril[:, :, None] & ~on
    gg = np.broadcast_to(g, on.shape)
    res["cells"] = check_values(what + " dScore", dS[off], tr.m[off], -gg[off], cb[off], None if fl is None else fl[off])
    res["path"] = check_abs(what + " dScore on the path", dS[on], gg[on] * (1.0 - tr.m[on]),
                            np.abs(gg[on]) * (tr.m[on] * np.expm1(cb[on]) + 2 * U))
    if T > 1:
        res["dNoise"] = check_abs(what + " dNoise", dN, g * (1.0 - cover - tr.mn), np.abs(g) * (tr.mn * np.expm1(tr.gap_bound(K)) + 3 * U))
    return res


def want_logprob(score, noise, paths, tr):
    """(logProb64 [n], its bound without logZ's part [n]) of the chains tr.idx: the path side of tests/path_targets_common.py."""
    import path_targets_common as ptc
    ix = torch.tensor(tr.idx)
    p64, terms = ptc.path_reference(score.index_select(2, ix), noise.index_select(1, ix), paths)
    return p64 - tr.lz, ptc.eval_path_bound(p64, terms) + U * np.abs(p64 - tr.lz)


# ---- the gate of today's suite (tests/test_gpu_parity.py), for the mutants ------------------------------------------------------------------
def old_gate_accepts(grad, grad64, lz64):
    from conftest import rel_err
    return rel_err(grad, grad64) < max(1e-4, 2e-6 * float(np.max(np.abs(lz64))))
