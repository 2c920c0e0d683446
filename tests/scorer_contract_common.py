"""What tests/test_scorer_contract.py is made of: the guard-band execution of a case, the float64 references of the interval scorer, its
backward, the projection GEMMs and the weight-staging ops, the plain float32 evaluations and the PER-ELEMENT error bounds.

Execution.  A case is a function case(R) of a Run: it carves every operand, output and workspace, calls the library through ctypes
(include/semicrf_hip.h: the C ABI itself, so that NULL pointers, exact workspace sizes and pointers at any phase can be passed) and
returns {output name: the set of elements the header says the call writes}.  `contract` runs it three times -- in a NaN-pattern arena,
in a FLT_MAX-pattern arena and on ordinary tensors (tests/arena_common.py) -- and asserts
  1. Arena.check(): guards intact, operands unchanged;
  2. every output element outside the written set keeps the bits it had (the pattern, or the values an accumulating output held);
  3. every element inside the written set differs from the pattern;
  4. the three runs agree bit for bit, i.e. nothing outside the read set reaches a result.
Strided operands are carved at their FULL pitch, the pattern stays in the pad columns.

Bounds.  u = 2^-24.  Every exact kernel is an fp32 fmaf chain per output in SOME fixed order (v_mfma_f32_32x32x2_f32, fmaf loops, partial
sums combined in a fixed tree), so for a contraction of n terms t_i the computed sum s satisfies |s - sum t_i| <= gamma_n sum |t_i| with
gamma_n = n u / (1 - n u) whatever the order (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a product that is
rounded before it is added costs one more factor (1 + delta), an fmaf none).  Each bound below is (n + a few) u sum |t_i|: the "few"
are the roundings outside the chain, listed in the helper's docstring.  (n + 8) u < 2^-15 at n <= 512, so gamma_n and n u differ by
less than one part in 2^15 of the bound: the slack of the "+ 8" (at most 6 are used) covers it.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import arena_common as ac
from transkun_amd import _lib, synth

F32, I32, U8 = torch.float32, torch.int32, torch.uint8
U = 2.0 ** -24
OK, EINVAL, EWORKSPACE = 0, 1, 2


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def normal(shape, seed, scale=1.0):
    """synth.hash_normal values of the shape, on the host."""
    n = 1
    for s in shape:
        n *= int(s)
    t = synth.hash_normal(n, seed).view(*shape)
    return t * scale if scale != 1.0 else t


def qscale_of(D):
    return float(np.float32(1.0 / math.sqrt(D)))


def len64(mode, d):
    """len(|e - b|) of include/semicrf_hip.h in float64: 0 linear, 1 sqrt, 2 none."""
    d = np.abs(np.asarray(d, dtype=np.float64))
    return d if mode == 0 else (np.sqrt(d) if mode == 1 else np.ones_like(d))


def len32(mode, d):
    d = np.abs(np.asarray(d)).astype(np.float32)
    return d if mode == 0 else (np.sqrt(d) if mode == 1 else np.ones_like(d))


def slot_index(C, group, pitch):
    """(slot of every chain [C], ghost slots) of the slot layout (include/semicrf_hip.h, SLOT LAYOUT); group == 0: contiguous."""
    if not group or group == pitch:
        return np.arange(C), np.zeros(0, dtype=np.int64)
    c = np.arange(C)
    real = (c // group) * pitch + c % group
    ghosts = np.setdiff1d(np.arange(C // group * pitch), real)
    return real, ghosts


# ---- one execution of a case ------------------------------------------------------------------------------------------------------------------
class Run:
    """Where a case's tensors come from: an arena, its sizer or torch's allocator."""

    def __init__(self, A, dev):
        self.A, self.dev, self.outs = A, dev, {}
        self.real = A.real
        self.pattern = getattr(A, "pattern", ac.NAN_PATTERN)

    def _carve(self, name, shape, dtype, phase):
        """A.carve; on ordinary tensors a phase is real too (a view `phase` bytes into a 16-byte aligned allocation), so that the three
        runs of a case take the same route."""
        if isinstance(self.A, ac.Plain) and phase:
            n = (1 if dtype == U8 else 4)
            for s in shape:
                n *= int(s)
            raw = self.A.carve(name, (n + 16,), U8)
            assert raw.data_ptr() % 16 == 0 and phase % 4 == 0
            t = raw[phase:phase + n]
            return (t if dtype == U8 else t.view(dtype)).view(tuple(shape))
        return self.A.carve(name, tuple(shape), dtype, phase)

    def _operand(self, t):
        if isinstance(self.A, ac.Arena):
            self.A.carves[-1][4] = ac.bits(t).clone()          # Arena.check() finds it unchanged

    def inp(self, name, src, phase=0):
        """A contiguous read-only operand."""
        if isinstance(self.A, ac.Plain) and phase:
            t = self._carve(name, tuple(src.shape), src.dtype, phase)
            t.copy_(src)
            return t
        return self.A.put(name, src.contiguous(), phase)

    def inp_strided(self, name, data, ld, phase=0):
        """data [..., n] as rows of pitch ld >= n: the carve is [..., ld], the pattern stays in the columns n .. ld-1."""
        n = data.shape[-1]
        assert ld >= n
        t = self._carve(name, tuple(data.shape[:-1]) + (ld,), data.dtype, phase)
        if self.real:
            t[..., :n].copy_(data)
            self._operand(t)
        return t

    def out(self, name, shape, phase=0, init=None, dtype=F32):
        """An output carve holding the pattern (init: values an accumulating output holds before the call, the whole carve)."""
        t = self._carve(name, tuple(shape), dtype, phase)
        if self.real:
            if init is not None:
                t.copy_(init)
            self.outs[name] = (t, t.clone())
        return t

    def ws(self, name, nbytes, fill=None, phase=0):
        """A workspace of exactly nbytes between guards, 16-byte aligned (+ phase); fill: None = the pattern, else a byte value."""
        t = self._carve(name, (int(nbytes),), U8, phase)
        if self.real and fill is not None:
            t.fill_(fill)
        return t

    def call(self, fn):
        """fn() -> the library's return code (not run by the sizer)."""
        return self.A.call(fn)


def P(t, offset_elems=0):
    """A tensor's address for the C ABI (None: NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * offset_elems)


def stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if torch.device(dev).type == "cuda" else None


class Outcome:
    """A finished run: the return code, and per output its values, the bits it held before the call and the written set (numpy)."""

    def __init__(self, rc, outs, masks):
        self.rc = rc
        self.val, self.before, self.mask = {}, {}, {}
        for name, (t, snap) in outs.items():
            self.val[name] = t.detach().cpu().numpy().copy()
            self.before[name] = snap.detach().cpu().numpy().view(np.uint32)
            m = masks[name]
            m = np.broadcast_to(np.asarray(m, dtype=bool), self.val[name].shape)
            self.mask[name] = m

    def words(self, name):
        return self.val[name].view(np.uint32)


def guard_bytes(T=1, Cs=1, widest_row_floats=1):
    """The guard of every case: the largest of 4 KiB, 128 rows of the widest operand row, one [T][Cs] plane of S."""
    return max(4096, 128 * int(widest_row_floats) * 4, int(T) * int(Cs) * 4)


def execute(case, dev, pattern, guard, plain=False):
    """case(R) -> (rc, {output: written set}).  Returns the Outcome; Arena.check() has passed."""
    box = {}

    def go(A):
        R = Run(A, dev)
        box["R"], box["ret"] = R, case(R)

    if plain:
        A = ac.Plain(pattern, dev)
        go(A)
    else:
        A, _ = ac.run_in_arena(go, guard, pattern, dev)
    try:
        A.check()
        status = _lib.device_status() if torch.device(dev).type == "cuda" else 0
    except RuntimeError as ex:                   # (a GuardError is an AssertionError; this is the runtime reporting a device error)
        pytest.exit(f"device error, nothing more is launched: {ex}", returncode=3)
    if status < 0:
        pytest.exit("semicrf_debug_device_status reports a HIP error, nothing more is launched", returncode=3)
    assert status == 0
    rc, masks = box["ret"]
    assert set(masks) == set(box["R"].outs), (sorted(masks), sorted(box["R"].outs))
    return Outcome(rc, box["R"].outs, masks)


def _where(name, arr_shape, flat):
    return f"`{name}` element {tuple(int(i) for i in np.unravel_index(flat, arr_shape))} (offset {int(flat)} of the carve)"


def check_written(o, pattern, what):
    """Assertions 2 and 3 of the module docstring."""
    pat = np.uint32(pattern)
    for name in o.val:
        w, before, m = o.words(name), o.before[name], o.mask[name]
        touched = (w != before) & ~m
        if touched.any():
            i = int(np.flatnonzero(touched)[0])
            raise AssertionError(f"{what}: {_where(name, w.shape, i)} lies outside the written set and was written "
                                 f"({int(touched.sum())} such elements; {int(before.reshape(-1)[i]):#010x} -> {int(w.reshape(-1)[i]):#010x})")
        still = (w == pat) & m
        if still.any():
            i = int(np.flatnonzero(still)[0])
            raise AssertionError(f"{what}: {_where(name, w.shape, i)} must be written and still holds the pattern ({int(still.sum())} such elements)")


def check_same_bits(a, b, what):
    """Assertion 4: two runs agree bit for bit inside the written sets (outside them both hold what they held)."""
    assert a.rc == b.rc, f"{what}: return codes {a.rc} and {b.rc}"
    for name in a.val:
        m = a.mask[name]
        assert np.array_equal(m, b.mask[name])
        x, y = a.words(name), b.words(name)
        diff = (x != y) & m
        if diff.any():
            i = int(np.flatnonzero(diff)[0])
            raise AssertionError(f"{what}: {_where(name, x.shape, i)} differs between the two runs ({int(diff.sum())} elements: "
                                 f"{a.val[name].reshape(-1)[i]!r} against {b.val[name].reshape(-1)[i]!r})")


def contract(case, dev, guard, what, rc=OK):
    """Assertions 1 - 4 for one case; returns the run on ordinary tensors."""
    plain = execute(case, dev, ac.NAN_PATTERN, guard, plain=True)
    assert plain.rc == rc, f"{what}: return code {plain.rc}, expected {rc}: {_lib.load().semicrf_last_error().decode()}"
    check_written(plain, ac.NAN_PATTERN, what + " (ordinary tensors)")
    nan = execute(case, dev, ac.NAN_PATTERN, guard)
    check_written(nan, ac.NAN_PATTERN, what + " (NaN arena)")
    check_same_bits(nan, plain, what + ": NaN arena against ordinary tensors")
    mx = execute(case, dev, ac.MAX_PATTERN, guard)
    check_written(mx, ac.MAX_PATTERN, what + " (FLT_MAX arena)")
    check_same_bits(mx, nan, what + ": FLT_MAX arena against NaN arena")
    return plain


def assert_within(name, got, ref64, bound, what, mask=None, quiet=False):
    """|got - ref64| <= bound in EVERY element (of the mask).  Prints the worst error in units of its bound first."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref64)
    bad = ~(err <= bound)
    if mask is not None:
        bad &= np.broadcast_to(mask, bad.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    if mask is not None:
        ratio = np.where(np.broadcast_to(mask, ratio.shape), ratio, 0.0)
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    if not quiet:
        print(f"{what}: `{name}` worst |error| / bound = {worst:.4f}")
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {_where(name, bad.shape, i)} is outside its bound: got {got.reshape(-1)[i]!r}, float64 "
                             f"{np.asarray(ref64).reshape(-1)[i]!r}, |error| {err.reshape(-1)[i]:.3e} > bound "
                             f"{np.broadcast_to(bound, bad.shape).reshape(-1)[i]:.3e} ({int(bad.sum())} elements; worst {worst:.2f} bounds)")
    return worst


# ---- three bf16 limbs (csrc/bf16x3.h) on the host --------------------------------------------------------------------------------------------
def bf16_round(x):
    """float32 -> the nearest bf16 (ties to even), as float32."""
    w = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    w = (w + 0x7FFF + ((w >> 16) & 1)) & 0xFFFF0000
    return w.astype(np.uint32).view(np.float32)


def limbs(x, n=3):
    """The exact split x = l1 + l2 + l3 of a float32 into bf16 limbs (24 = 3 x 8 significand bits); n < 3 drops the last ones."""
    x = np.asarray(x, dtype=np.float32)
    out, r = [], x.copy()
    for _ in range(n):
        l = bf16_round(r)
        out.append(l)
        r = r - l
    return out


LIMB_PRODUCTS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))          # six of the nine: the ones down to 2^-16 of the leading one


# ---- the forward: S[e,b,c] = qscale (<q_e, k_b> + rowc_e) len(|e-b|) (+ diag_e on e == b) ---------------------------------------------------
def fwd_ref(q, k, diag, rowc, qs, mode, prec=0):
    """(S64 [T][T][C], bound [T][T][C]) of the full square.

    Bound, forward S[e,b,c]: (D + 8) u (qscale len (sum_d |q_d k_d| + |rowc|) + |diag|).  The chain has D terms (gamma_D); outside it
    at most: q * qscale rounded per term in the plain kernel (1), the row constant's add (1), qscale * len (1), the length function
    (sqrtf: 1, the header allows 2), the product with it (1), the diagonal's add (1): 6 <= 8.
    prec = 1 (SEMICRF_SCORE_BF16X3): the header's 2^-21 qscale len sum_d |q_d k_d| on top (the dropped limb products), the fp32
    accumulation term stays."""
    q64, k64 = q.astype(np.float64), k.astype(np.float64)
    C, T, D = q.shape
    dot = np.matmul(q64, k64.transpose(0, 2, 1))                          # [C][e][b]
    absdot = np.matmul(np.abs(q64), np.abs(k64).transpose(0, 2, 1))
    e, b = np.arange(T)[:, None], np.arange(T)[None, :]
    ln = len64(mode, e - b)[None]
    rc = np.zeros((C, T, 1)) if rowc is None else rowc.astype(np.float64)[:, :, None]
    S = float(qs) * (dot + rc) * ln
    eye = (e == b)[None]
    dg = diag.astype(np.float64)[:, :, None]
    S = S + np.where(eye, dg, 0.0)
    bound = (D + 8) * U * (float(qs) * ln * (absdot + np.abs(rc)) + np.where(eye, np.abs(dg), 0.0))
    if prec:
        bound = bound + 2.0 ** -21 * float(qs) * ln * absdot
    return S.transpose(1, 2, 0).copy(), bound.transpose(1, 2, 0).copy()


def fwd_f32(q, k, diag, rowc, qs, mode, nlimbs=0, drop_last=False):
    """The formula in plain float32 numpy, the contraction accumulated sequentially over d (nlimbs: through that many bf16 limbs of
    every operand, the six limb products of the kernel that exist; drop_last: without the last term -- a yardstick).  [T][T][C]."""
    C, T, D = q.shape
    acc = np.zeros((C, T, T), dtype=np.float32)
    if nlimbs:
        ql, kl = limbs(q, nlimbs), limbs(k, nlimbs)
    for d in range(D - 1 if drop_last else D):
        if nlimbs:
            for i, j in LIMB_PRODUCTS:
                if i < nlimbs and j < nlimbs:
                    acc = acc + ql[i][:, :, None, d] * kl[j][:, None, :, d]
        else:
            acc = acc + q[:, :, None, d] * k[:, None, :, d]
    e, b = np.arange(T)[:, None], np.arange(T)[None, :]
    if rowc is not None:
        acc = acc + rowc[:, :, None]
    S = acc * (np.float32(qs) * len32(mode, e - b))[None]
    S = S + np.where((e == b)[None], diag[:, :, None], np.float32(0))
    return S.astype(np.float32).transpose(1, 2, 0).copy()


# ---- the backward -----------------------------------------------------------------------------------------------------------------------------
def bwd_ref(G_or_dS, q, k, qs, mode, prec=0, scaled=False):
    """float64 gradients and bounds from the cotangent [T][T][C] (chain-indexed, only e >= b is used).

    G[e,b,c] = dS[e,b,c] qscale len(e-b);  dq[c,e,:] = sum_{b<=e} G k[c,b,:];  dk[c,b,:] = sum_{e>=b} G q[c,e,:];
    drowc[c,e] = sum_{b<=e} G;  ddiag[c,t] = dS[t,t,c] (a copy: bit-equal).
    Bounds: dq (n + 8) u sum_b |G k|, n = e + 1 terms; dk the same over e, n = T - b; drowc (n + 8) u sum_b |G|.  Outside the chain:
    qscale * len (1), the length function (1 - 2), dS times it (1): 4 <= 8 (drowc multiplies by qscale after the sum: 1 more).
    prec = 1 (SEMICRF_LEN_BF16X3): + 2^-21 sum |G k| for dq and dk (the header's statement), drowc and ddiag stay exact fp32."""
    T = G_or_dS.shape[0]
    e, b = np.arange(T)[:, None], np.arange(T)[None, :]
    G = G_or_dS.astype(np.float64).transpose(2, 0, 1)                     # [C][e][b]
    if not scaled:
        G = G * (float(qs) * len64(mode, e - b))[None]
    G = np.where((e >= b)[None], G, 0.0)
    q64, k64 = q.astype(np.float64), k.astype(np.float64)
    aG = np.abs(G)
    ne = (np.arange(T) + 1 + 8)[None, :, None] * U                        # dq / drowc row e: e + 1 terms
    nb = (T - np.arange(T) + 8)[None, :, None] * U                        # dk row b: T - b terms
    sdq, sdk = np.matmul(aG, np.abs(k64)), np.matmul(aG.transpose(0, 2, 1), np.abs(q64))
    extra = 2.0 ** -21 if prec else 0.0
    ref = {"dq": np.matmul(G, k64), "dk": np.matmul(G.transpose(0, 2, 1), q64), "drowc": G.sum(2)}
    bound = {"dq": ne * sdq + extra * sdq, "dk": nb * sdk + extra * sdk, "drowc": ne[:, :, 0] * aG.sum(2)}
    return ref, bound


def bwd_f32(dS, q, k, qs, mode, skip_dq_term=None, skip_dk_last=False):
    """The backward in plain float32 numpy, the contractions accumulated sequentially (b ascending for dq and drowc, e ascending for
    dk).  skip_dq_term: the term b = e - skip is left out of dq (a yardstick); skip_dk_last: dk without its last term e = T - 1."""
    T = dS.shape[0]
    C, _, D = q.shape
    e, b = np.arange(T)[:, None], np.arange(T)[None, :]
    G = (dS.transpose(2, 0, 1) * (np.float32(qs) * len32(mode, e - b))[None]).astype(np.float32)
    G = np.where((e >= b)[None], G, np.float32(0))
    dq = np.zeros((C, T, D), dtype=np.float32)
    dk = np.zeros((C, T, D), dtype=np.float32)
    dr = np.zeros((C, T), dtype=np.float32)
    rows = np.arange(T)
    for j in range(T):
        g = G[:, :, j]
        if skip_dq_term is not None:
            g = np.where((rows - j == skip_dq_term)[None], np.float32(0), g)
        dq = dq + g[:, :, None] * k[:, None, j, :]
        dr = dr + G[:, :, j]
        if not (skip_dk_last and j == T - 1):
            dk = dk + G[:, j, :, None] * q[:, None, j, :]
    return {"dq": dq, "dk": dk, "drowc": dr}


# ---- the semi-CRF's marginals in float64 (NeuralSemiCRFInterval.py:207-246, :386-447; the recurrences of oracle/semicrf_oracle_fp.inc) ---------
def _softplus64(x):
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def marginals64(S, noise=None):
    """S [T][T][C] float64 (e >= b used), noise [T-1][C] or None (zeros).  Returns (marginal [T][T][C], zero for e < b; alpha [T][C];
    beta [T][C]; logZ [C]):
        alpha[0] = sp(S00);  alpha[i] = logaddexp(alpha[i-1] + n[i-1], lse_{j<i}(alpha[j] + S[i,j])) + sp(S[i,i])
        beta[T-1] = sp(S[T-1,T-1]);  beta[i] = logaddexp(beta[i+1] + n[i], lse_{e>i}(beta[e] + S[e,i])) + sp(S[i,i])
        marginal[e,b] = exp(alpha[b] + beta[e] + S[e,b] - logZ)  (e > b),  [t,t]: exp(alpha[t] + beta[t] + S[t,t] - 2 sp(S[t,t]) - logZ)."""
    T, _, C = S.shape
    n = np.zeros((max(T - 1, 0), C)) if noise is None else noise.astype(np.float64)
    sp = _softplus64(np.stack([S[t, t] for t in range(T)]))               # [T][C]
    al, be = np.zeros((T, C)), np.zeros((T, C))
    al[0] = sp[0]
    for i in range(1, T):
        x = al[:i] + S[i, :i]
        m = x.max(0)
        al[i] = np.logaddexp(al[i - 1] + n[i - 1], m + np.log(np.exp(x - m).sum(0))) + sp[i]
    be[T - 1] = sp[T - 1]
    for i in range(T - 2, -1, -1):
        x = be[i + 1:] + S[i + 1:, i]
        m = x.max(0)
        be[i] = np.logaddexp(be[i + 1] + n[i], m + np.log(np.exp(x - m).sum(0))) + sp[i]
    logZ = al[T - 1]
    e, b = np.arange(T)[:, None, None], np.arange(T)[None, :, None]
    x = al[None, :, :] + be[:, None, :] + S - logZ[None, None, :]
    x = x - np.where(e == b, 2.0 * sp[:, None, :], 0.0)
    marg = np.where(e >= b, np.exp(np.where(e >= b, x, 0.0)), 0.0)
    return marg, al, be, logZ


# ---- the projection GEMMs ------------------------------------------------------------------------------------------------------------------------
def nn_ref(A, B, bias, w2, b2, old=None):
    """scorer_proj_nn in float64: (main [M][N], extra [M][2] or None) and their bounds.

    Bound: (K + 4) u (sum_k |a b| + |bias|), + u |old| when accumulating (bias is not added then: include/semicrf_hip.h).  Outside the
    chain of K terms: the bias or the old value's add (1), the two half-waves' partial sums of the extra columns (1): 2 <= 4; the
    rounding of old + product is u |result| <= u (|old| + the product's magnitude), which the "+ u |old|" and the + 4 hold.
    prec (scorer_proj_nn3): the caller adds 2^-21 sum_k |a b|."""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    K = A.shape[1]
    main, amain = A64 @ B64, np.abs(A64) @ np.abs(B64)
    bound = amain.copy()
    if old is not None:
        main = main + old.astype(np.float64)
    elif bias is not None:
        main = main + bias.astype(np.float64)[None]
        bound = bound + np.abs(bias.astype(np.float64))[None]
    bound = (K + 4) * U * bound
    if old is not None:
        bound = bound + U * np.abs(old.astype(np.float64))
    ex = exb = None
    if w2 is not None:
        w64 = w2.astype(np.float64)
        ex = A64 @ w64.T + b2.astype(np.float64)[None]
        exb = (K + 4) * U * (np.abs(A64) @ np.abs(w64).T + np.abs(b2.astype(np.float64))[None])
    return main, bound, amain, ex, exb


def nn_f32(A, B, bias, old=None, nlimbs=0, drop_last=False):
    """A B (+ bias | + old) in plain float32 numpy, accumulated sequentially over k."""
    M, K = A.shape
    acc = np.zeros((M, B.shape[1]), dtype=np.float32)
    if nlimbs:
        al, bl = limbs(A, nlimbs), limbs(B, nlimbs)
    for kk in range(K - 1 if drop_last else K):
        if nlimbs:
            for i, j in LIMB_PRODUCTS:
                if i < nlimbs and j < nlimbs:
                    acc = acc + al[i][:, kk, None] * bl[j][None, kk, :]
        else:
            acc = acc + A[:, kk, None] * B[None, kk, :]
    if old is not None:
        acc = acc + old
    elif bias is not None:
        acc = acc + bias[None]
    return acc


def tn_ref(dy, x):
    """dW = dy^T x, db = column sums of dy in float64 with the bounds (M + 8) u sum_m |dy x| and (M + 8) u sum_m |dy|: a chain of M
    terms in the kernel's fixed order (slices, partial sums, a fixed tree); nothing outside it but the tree's own adds, which are part
    of the M - 1 additions of any order."""
    dy64, x64 = dy.astype(np.float64), x.astype(np.float64)
    M = dy.shape[0]
    a = np.abs(dy64).T @ np.abs(x64)
    return dy64.T @ x64, (M + 8) * U * a, a, dy64.sum(0), (M + 8) * U * np.abs(dy64).sum(0)


def tn_f32(dy, x, drop_last=False):
    M = dy.shape[0]
    acc = np.zeros((dy.shape[1], x.shape[1]), dtype=np.float32)
    db = np.zeros(dy.shape[1], dtype=np.float32)
    for m in range(M - 1 if drop_last else M):
        acc = acc + dy[m, :, None] * x[m, None, :]
        db = db + dy[m]
    return acc, db


# ---- the merged projection's weights (csrc/merge_weights.hip) ---------------------------------------------------------------------------------
def merge_fwd_ref(W, bias, D, size):
    """(Wm [size+2][size], bm [size+2]) in float64 with the bounds (D + 4) u sum_r |.|: chains of D terms (four partial chains combined
    in a fixed order for Wm, a block tree for bm: orders of the same D - 1 additions); the rows size + 1 (the diagonal row) are copies."""
    W64, b64 = W.astype(np.float64), bias.astype(np.float64)
    Wq, Wk, bq, bk = W64[:D], W64[D:2 * D], b64[:D], b64[D:2 * D]
    Wk1 = np.concatenate([Wk, bk[:, None]], axis=1)                       # [D][size + 1]
    Wm = np.concatenate([Wk1.T @ Wq, W64[2 * D:2 * D + 1]])
    bm = np.concatenate([Wk1.T @ bq, b64[2 * D:2 * D + 1]])
    bW = np.concatenate([(D + 4) * U * (np.abs(Wk1).T @ np.abs(Wq)), np.zeros((1, size))])
    bb = np.concatenate([(D + 4) * U * (np.abs(Wk1).T @ np.abs(bq)), np.zeros(1)])
    return Wm, bW, bm, bb


def merge_bwd_ref(W, bias, dWm, dbm, D, size):
    """(dW [2D+1][size], dbias [2D+1]) in float64, the autograd of merge_fwd_ref, with (n + 4) u sum |.| for chains of n = size + 1
    (dWq, dbq) and n = size + 1 (dWk, dbk: size terms and the bias term joined by one fmaf) terms; the last row and entry are copies."""
    W64, b64 = W.astype(np.float64), bias.astype(np.float64)
    dWm64, dbm64 = dWm.astype(np.float64), dbm.astype(np.float64)
    Wq, Wk, bq, bk = W64[:D], W64[D:2 * D], b64[:D], b64[D:2 * D]
    Wk1 = np.concatenate([Wk, bk[:, None]], axis=1)
    g, gb = dWm64[:size + 1], dbm64[:size + 1]
    n = (size + 1 + 4) * U
    dWq, bWq = Wk1 @ g, n * (np.abs(Wk1) @ np.abs(g))
    dbq, bbq = Wk1 @ gb, n * (np.abs(Wk1) @ np.abs(gb))
    dWk1 = Wq @ g.T + bq[:, None] * gb[None]                              # [D][size + 1]
    bWk1 = n * (np.abs(Wq) @ np.abs(g).T + np.abs(bq)[:, None] * np.abs(gb)[None])
    dW = np.concatenate([dWq, dWk1[:, :size], dWm64[size + 1:size + 2]])
    bW = np.concatenate([bWq, bWk1[:, :size], np.zeros((1, size))])
    db = np.concatenate([dbq, dWk1[:, size], dbm64[size + 1:size + 2]])
    bb = np.concatenate([bbq, bWk1[:, size], np.zeros(1)])
    return dW, bW, db, bb
