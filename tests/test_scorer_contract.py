"""The memory contract of the scorer and projection entry points (include/semicrf_hip.h, "Memory contract of the scorer entry points"):
interval_score_fwd[_p|_pc], interval_score_bwd[_ws[_p|_pc]], interval_score_bwd_fused[_ws[_p|_pc]], interval_score_path_bwd[_p|_pc],
scorer_proj_nn / _nn3 / _tn, scorer_stage_linear, scorer_merge_weights_fwd / _bwd -- the companion of tests/test_memory_contract.py
(the semi-CRF layer) and tests/test_step_contract.py (the step's ops).  The header's paragraph is lettered S1 .. S12; every test
names the sentences it pins.

Device cases (@pytest.mark.gpu: these ops have no host mirror) carve everything out of ONE guard-band arena and make the five
assertions of tests/scorer_contract_common.py: guards and operands intact, nothing outside the written set touched, everything inside
it written, NaN arena == FLT_MAX arena == ordinary tensors bit for bit, and every element inside a bound against float64 that is
DERIVED there (never fitted).  The unmarked tests need no device: the forward's route table, the argument checks that return before
any HIP call, and what the bounds are worth -- a plain float32 evaluation stays inside them in every element, four subtly wrong
results do not.
"""
import functools

import numpy as np
import pytest
import torch

import arena_common as ac
import scorer_contract_common as sc
from scorer_contract_common import F32, I32, U, OK, EINVAL, EWORKSPACE, P
from transkun_amd import _lib

L = _lib.load()
BF16X3_FWD, BF16X3_BWD, BF16X3_TN = _lib.SCORE_BF16X3, _lib.LEN_BF16X3, _lib.PROJ_TN_BF16X3


@pytest.fixture(scope="module", autouse=True)
def _device_status_at_the_end():
    yield
    if torch.cuda.is_available():
        assert _lib.device_status() == 0


def _err():
    return L.semicrf_last_error().decode()


# =================================================================================================================================================
# A.  interval_score_fwd[_p|_pc]
# =================================================================================================================================================
class Fwd:
    """One row of the forward table: the shape, how the operands lie in memory and the kernel plan_score_route picks for it."""

    def __init__(self, name, C, T, D, layout, route, group=0, pitch=0, rowc=0, prec=0, forced=-1):
        self.name, self.C, self.T, self.D, self.layout, self.route = name, C, T, D, layout, route
        self.group, self.pitch, self.rowc, self.prec, self.forced = group or C, pitch or C, rowc, prec, forced
        self.Cs = C // self.group * self.pitch
        self.ld = 2 * D + 1 if layout == "packed" else D + 4                # row pitch of q and k
        self.ldd = 2 * D + 1 if layout == "packed" else 3

    def __repr__(self):
        return self.name


REGLOAD, PLAIN, TILED, TILE3, STREAM, REFUSED = 0, 1, 2, 3, 32, -1
FWD = [
    # the plain kernel: every D that is no multiple of 64
    Fwd("plain_3x1x8", 3, 1, 8, "pad", PLAIN), Fwd("plain_3x2x8", 3, 2, 8, "pad", PLAIN), Fwd("plain_5x33x48", 5, 33, 48, "pad", PLAIN),
    # register loads, rows only 4-byte aligned (slices of one packed [C][T][2D+1] carve): nch = 1, 2, 3, 4 and the run-time loop (0)
    Fwd("regload_u_D64", 5, 70, 64, "packed", REGLOAD), Fwd("regload_u_D128", 6, 40, 128, "packed", REGLOAD),
    Fwd("regload_u_D192", 4, 65, 192, "packed", REGLOAD), Fwd("regload_u_D256", 4, 65, 256, "packed", REGLOAD),
    Fwd("regload_u_D320", 3, 40, 320, "packed", REGLOAD),
    # register loads, 16-byte loads (forced through semicrf_debug_score_variant(0))
    Fwd("regload_a_D64", 5, 70, 64, "pad", REGLOAD, forced=0), Fwd("regload_a_D256", 4, 65, 256, "pad", REGLOAD, forced=0),
    # streaming
    Fwd("stream_5x70x64", 5, 70, 64, "pad", STREAM), Fwd("stream_9x255x128", 9, 255, 128, "pad", STREAM),
    Fwd("stream_3x31x256", 3, 31, 256, "pad", STREAM),
    # the 64 x 128 tiles
    Fwd("tiled_5x256x64", 5, 256, 64, "pad", TILED), Fwd("tiled_33x257x256", 33, 257, 256, "pad", TILED),
    Fwd("tiled_4x320x128", 4, 320, 128, "pad", TILED),
    Fwd("tiled_slots_T128", 10, 128, 64, "pad", TILED, group=5, pitch=8), Fwd("tiled_slots_T130", 18, 130, 192, "pad", TILED, group=6, pitch=8),
    Fwd("tiled_rowc", 5, 128, 64, "pad", TILED, rowc=3), Fwd("tiled_rowc_slots", 10, 130, 128, "pad", TILED, group=5, pitch=8, rowc=2),
    # the three-limb tiles
    Fwd("tile3_5x128x64", 5, 128, 64, "pad", TILE3, prec=1), Fwd("tile3_6x257x256", 6, 257, 256, "pad", TILE3, prec=1),
    Fwd("tile3_slots_rowc_T128", 5, 128, 64, "pad", TILE3, prec=1, group=5, pitch=8, rowc=2),
    Fwd("tile3_slots_rowc_T257", 6, 257, 256, "pad", TILE3, prec=1, group=3, pitch=4, rowc=3),
]
FWD_IDS = [f.name for f in FWD]
# refused calls: (what, table row to start from, changes, the route's answer or None where an argument check refuses first)
FWD_REFUSED = [
    ("padded_pitch_T127", Fwd("r", 10, 127, 64, "pad", REFUSED, group=5, pitch=8), {}),
    ("padded_pitch_D96", Fwd("r", 10, 128, 96, "pad", REFUSED, group=5, pitch=8), {}),
    ("padded_pitch_q_phase4", Fwd("r", 10, 128, 64, "pad", REFUSED, group=5, pitch=8), {"qphase": 4}),
    ("padded_pitch_S_phase4", Fwd("r", 10, 128, 64, "pad", REFUSED, group=5, pitch=8), {"Sphase": 4}),
    ("rowc_T70", Fwd("r", 5, 70, 64, "pad", REFUSED, rowc=2), {}),
    ("pitch_6", Fwd("r", 10, 128, 64, "pad", None, group=5, pitch=6), {}),
    ("ldq_below_D", Fwd("r", 5, 70, 64, "pad", None), {"ldq": 60}),
]


@functools.lru_cache(maxsize=None)
def _fwd_data(C, T, D, scale=1.0):
    seed = 1000 + 7 * C + 13 * T + D
    return (sc.normal((C, T, D), seed, scale).contiguous(), sc.normal((C, T, D), seed + 1, scale).contiguous(), sc.normal((C, T), seed + 2),
            sc.normal((C, T), seed + 3))


_FWD_REF = {}


def _fwd_ref(f, mode):
    """The float64 scores and their bounds of a table row, once per (shape, mode)."""
    key = (f.C, f.T, f.D, bool(f.rowc), f.prec, mode)
    if key not in _FWD_REF:
        if len(_FWD_REF) > 4:
            _FWD_REF.clear()                    # tens of MB each at T = 257
        q, k, dg, rc = (x.numpy() for x in _fwd_data(f.C, f.T, f.D))
        _FWD_REF[key] = sc.fwd_ref(q, k, dg, rc if f.rowc else None, sc.qscale_of(f.D), mode, f.prec)
    return _FWD_REF[key]


def _fwd_case(f, mode, full, noise, dev, qphase=0, Sphase=0, ldq=None):
    """interval_score_fwd (no slot layout, no row constant), _p (slots) or _pc for a table row.  Written (S2): S in the cells e >= b
    (full_square 2) or everywhere; noise_out everywhere, or nothing when it is NULL."""
    C, T, D = f.C, f.T, f.D
    q, k, dg, rc = _fwd_data(C, T, D)
    qs = sc.qscale_of(D)
    e, b = np.arange(T)[:, None, None], np.arange(T)[None, :, None]
    smask = (e >= b) if full == 2 else np.ones((1, 1, 1), dtype=bool)

    def case(R):
        if f.layout == "packed":
            pk = R.inp("q|k|diag", torch.cat([q, k, dg[..., None]], -1))
            qa, ka, da = (pk, 0), (pk, D), (pk, 2 * D)
        else:
            qa, ka = (R.inp_strided("q", q, f.ld, qphase), 0), (R.inp_strided("k", k, f.ld), 0)
            da = (R.inp_strided("diag", dg[..., None], f.ldd), 0)
        ra = R.inp_strided("rowc", rc[..., None], f.rowc) if f.rowc else None
        S = R.out("S", (T, T, f.Cs), Sphase)
        N = R.out("noise", (max(T - 1, 0), f.Cs))
        st = sc.stream(dev)
        lq = f.ld if ldq is None else ldq
        fs = full | (BF16X3_FWD if f.prec else 0)

        def go():
            L.semicrf_debug_score_variant(f.forced)
            try:
                if f.rowc:
                    return L.interval_score_fwd_pc(P(*qa), P(*ka), P(*da), P(ra), C, T, D, lq, f.ld, f.ldd, f.rowc, qs, mode, fs, f.group,
                                                   f.pitch, P(S), P(N) if noise else None, st)
                if f.group != C:
                    return L.interval_score_fwd_p(P(*qa), P(*ka), P(*da), C, T, D, lq, f.ld, f.ldd, qs, mode, fs, f.group, f.pitch, P(S),
                                                  P(N) if noise else None, st)
                return L.interval_score_fwd(P(*qa), P(*ka), P(*da), C, T, D, lq, f.ld, f.ldd, qs, mode, fs, P(S), P(N) if noise else None, st)
            finally:
                L.semicrf_debug_score_variant(-1)
        refused = f.route is None or f.route == REFUSED
        return R.call(go), {"S": smask & (not refused), "noise": bool(noise) and not refused}
    return case


def _fwd_guard(f):
    return sc.guard_bytes(f.T, f.Cs, f.ld)


def _check_scores(f, mode, full, o, what):
    """Assertion 5 for S and the exact values: real slots inside the forward bound, +0.0f above the diagonal under full_square 0,
    +0.0f in every ghost slot that is written, noise_out all zeros."""
    T = f.T
    S = o.val["S"]
    ref, bound = _fwd_ref(f, mode)
    real, ghosts = sc.slot_index(f.C, f.group, f.pitch)
    e, b = np.arange(T)[:, None, None], np.arange(T)[None, :, None]
    lower = e >= b
    sc.assert_within("S", S[:, :, real], ref, bound, what, mask=lower if full != 1 else None)
    bits = S.view(np.uint32)
    if full == 0:
        assert not bits[np.broadcast_to(~lower, bits.shape)].any(), f"{what}: `S` above the diagonal is not exactly +0.0f"
    if ghosts.size:
        g = bits[:, :, ghosts]
        written = np.broadcast_to(lower if full == 2 else np.ones_like(lower), g.shape)
        assert not g[written].any(), f"{what}: a ghost slot of `S` is not exactly +0.0f"
    if "noise" in o.val and o.mask["noise"].any():
        assert not o.val["noise"].view(np.uint32).any(), f"{what}: `noise` is not all zeros"


def _fwd_combos(f):
    """(length scaling, full_square, noise_out present): the nine pairs where S is at most 1 MB, else a Latin square of three that
    shows every scaling and every full_square once per row and, over the rows of the table, every pair."""
    if f.T * f.T * f.Cs * 4 <= (1 << 20):
        return [(m, fs, (m + fs) % 2 == 0) for m in (0, 1, 2) for fs in (0, 1, 2)]
    r = FWD.index(f) if f in FWD else 0
    return [(m, (m + r) % 3, (m + r) % 2 == 0) for m in (0, 1, 2)]


def test_forward_route_table():
    """S3 (which kernel a call runs, by alignment and shape): semicrf_debug_score_route names the intended kernel for every row of the
    forward table with the row's own strides and alignment, and refuses the calls the header says are refused."""
    for f in FWD:
        aligned = 1                                 # every carve of the table is 16-byte aligned; a packed row pitch is odd
        got = L.semicrf_debug_score_route(f.C, f.T, f.D, f.ld, f.ld, aligned, f.prec, f.group, f.pitch, 1 if f.rowc else 0, f.forced, 0)
        assert got == f.route, f"{f.name}: route {got}, the table says {f.route}"
    for name, f, chg in FWD_REFUSED:
        if f.route is None:
            continue
        aligned = 0 if ("qphase" in chg or "Sphase" in chg) else 1
        got = L.semicrf_debug_score_route(f.C, f.T, f.D, f.ld, f.ld, aligned, f.prec, f.group, f.pitch, 1 if f.rowc else 0, -1, 0)
        assert got == REFUSED, f"{name}: route {got}"
    # an S (or q, k) off 16 bytes without slots: the register-load kernel, which stores dword by dword
    assert L.semicrf_debug_score_route(8, 70, 64, 68, 68, 0, 0, 8, 8, 0, -1, 0) == REGLOAD
    assert L.semicrf_debug_score_route(8, 256, 64, 68, 68, 0, 0, 8, 8, 0, -1, 0) == REGLOAD
    assert L.semicrf_debug_score_route(8, 256, 64, 68, 68, 0, 1, 8, 8, 0, -1, 0) == REGLOAD          # three-limb asked for: exact fp32 instead


@pytest.mark.gpu
@pytest.mark.parametrize("f", FWD, ids=FWD_IDS)
def test_forward(gpu, f):
    """S1 (read set: the D used columns of the C T rows of q and k, diag and rowc at their strides -- no pad column, no row past T),
    S2 (written set: S e >= b / everything, noise_out [T-1][Cs] or nothing; ghost slots exact zeros), S3 (the route) and the forward
    bound, for one row of the table at every length scaling and full_square."""
    assert L.semicrf_debug_score_route(f.C, f.T, f.D, f.ld, f.ld, 1, f.prec, f.group, f.pitch, 1 if f.rowc else 0, f.forced, 0) == f.route
    for mode, full, noise in _fwd_combos(f):
        what = f"{f.name} scaling {mode} full_square {full} noise {'yes' if noise else 'NULL'}"
        o = sc.contract(_fwd_case(f, mode, full, noise, gpu), gpu, _fwd_guard(f), what)
        _check_scores(f, mode, full, o, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name,f,chg", FWD_REFUSED, ids=[r[0] for r in FWD_REFUSED])
def test_forward_refused(gpu, name, f, chg):
    """S3: a padded pitch or a row constant outside the tiled kernels' shapes and alignments, a pitch that is no multiple of 4 and
    ldq < D are SEMICRF_EINVAL, and S and noise_out keep their bits."""
    for full in (0, 2):
        o = sc.contract(_fwd_case(f, 0, full, True, gpu, **chg), gpu, _fwd_guard(f), f"{name} full_square {full}", rc=EINVAL)
        assert o.rc == EINVAL and _err()


@pytest.mark.gpu
def test_forward_S_off_16_bytes_takes_the_register_load_kernel(gpu):
    """S3: the LDS-staged kernels store 16-byte pieces of S's chain axis, so an S that is only 4-byte aligned runs the register-load
    kernel (dword stores): the bits of that kernel on an aligned S (forced through the test hook), inside the forward bound -- not
    the bits of the streaming kernel, which sums two accumulators.  C % 4 == 0 is where the 16-byte stores happen."""
    for f, g in ((Fwd("S4_stream", 8, 70, 64, "pad", STREAM), Fwd("S4_stream_forced", 8, 70, 64, "pad", REGLOAD, forced=0)),
                 (Fwd("S4_tiled", 4, 256, 64, "pad", TILED), Fwd("S4_tiled_forced", 4, 256, 64, "pad", REGLOAD, forced=0))):
        ref = sc.contract(_fwd_case(g, 0, 0, True, gpu), gpu, _fwd_guard(g), g.name + " aligned")
        _check_scores(g, 0, 0, ref, g.name)
        for ph in (4, 8, 12):
            o = sc.contract(_fwd_case(f, 0, 0, True, gpu, Sphase=ph), gpu, _fwd_guard(f), f"{f.name} S at phase {ph}")
            _check_scores(f, 0, 0, o, f"{f.name} S at phase {ph}")
            sc.check_same_bits(o, ref, f"{f.name}: S at phase {ph} against the register-load kernel on an aligned S")


# =================================================================================================================================================
# B.  interval_score_bwd, interval_score_bwd_ws[_p|_pc]
# =================================================================================================================================================
ALL_OUTS = ("dq", "dk", "ddiag", "drowc")
LDDD, LDDRC = 3, 2


@functools.lru_cache(maxsize=None)
def _cotangent(T, Cs):
    return sc.normal((T, T, Cs), 5000 + 3 * T + Cs)


def _ignored_cells(T, C, group, pitch):
    """The cells of dS (or S) the backward must not look at: e < b, and every ghost slot of a padded pitch.  [T][T][Cs] bool."""
    real, ghosts = sc.slot_index(C, group, pitch)
    Cs = C // (group or C) * (pitch or C)
    m = torch.zeros(T, T, Cs, dtype=torch.bool)
    m |= (torch.arange(T)[:, None] < torch.arange(T)[None, :])[:, :, None]
    if ghosts.size:
        m[:, :, torch.from_numpy(ghosts)] = True
    return m


def _with_ignored(t, mask, R, upper):
    """A copy of t whose ignored cells hold zeros or the run's pattern, bit for bit."""
    t = t.clone()
    word = int(np.array([R.pattern if upper == "pattern" else 0], dtype=np.uint32).view(np.int32)[0])
    t.view(I32)[mask] = word
    return t


def _packed_applies(C, T, D, outs, ws, layout, dev):
    return (D in (64, 128, 256) and T >= 64 and ws == "exact" and layout == "pad" and ("dq" in outs or "dk" in outs)
            and not ("drowc" in outs and "dq" not in outs))


def _bwd_case(C, T, D, mode, dev, group=0, pitch=0, outs=ALL_OUTS, ws="exact", ws_fill=None, upper="zero", entry="pc", prec=0,
              layout="pad", refused=False, dSphase=0):
    """One call of the backward.  Read (S5): the cells e >= b of the real slots of dS, the D used columns of q and k.  Written (S6):
    the D used columns of dq / dk, ddiag and drowc at their strides, each only when its pointer is not NULL."""
    group, pitch = group or C, pitch or C
    Cs = C // group * pitch
    q, k, _, _ = _fwd_data(C, T, D)
    dS, ign = _cotangent(T, Cs), _ignored_cells(T, C, group, pitch)
    qs = sc.qscale_of(D)
    ld = 2 * D + 1 if layout == "packed" else D + 4
    lddq, lddk = D + 4, D
    nws = int(L.interval_score_bwd_workspace_bytes(C, T, D))

    def case(R):
        g = R.inp("dS", _with_ignored(dS, ign, R, upper), dSphase)
        if layout == "packed":
            pk = R.inp("q|k|diag", torch.cat([q, k, q[..., :1]], -1))
            qa, ka = (pk, 0), (pk, D)
        else:
            qa, ka = (R.inp_strided("q", q, ld), 0), (R.inp_strided("k", k, ld), 0)
        o = {"dq": R.out("dq", (C, T, lddq)), "dk": R.out("dk", (C, T, lddk)), "ddiag": R.out("ddiag", (C, T, LDDD)),
             "drowc": R.out("drowc", (C, T, LDDRC))}
        w = R.ws("ws", nws, ws_fill, 4 if ws == "phase4" else 0) if ws else None
        wp = P(w) if (w is not None and nws) else None
        wb = 0 if wp is None else (nws - 1 if ws == "short" else nws)
        st = sc.stream(dev)
        a = {n: (P(o[n]) if n in outs else None) for n in ALL_OUTS}
        ls = mode | (BF16X3_BWD if prec else 0)

        def go():
            if entry == "plain":
                return L.interval_score_bwd(P(g), P(*qa), P(*ka), C, T, D, ld, ld, qs, mode, a["dq"], a["dk"], a["ddiag"], lddq, lddk, LDDD, st)
            if entry == "ws":
                return L.interval_score_bwd_ws(P(g), P(*qa), P(*ka), C, T, D, ld, ld, qs, ls, a["dq"], a["dk"], a["ddiag"], lddq, lddk, LDDD, wp, wb, st)
            if entry == "p":
                return L.interval_score_bwd_ws_p(P(g), P(*qa), P(*ka), C, T, D, ld, ld, qs, ls, group, pitch, a["dq"], a["dk"], a["ddiag"], lddq,
                                                 lddk, LDDD, wp, wb, st)
            return L.interval_score_bwd_ws_pc(P(g), P(*qa), P(*ka), C, T, D, ld, ld, qs, ls, group, pitch, a["dq"], a["dk"], a["ddiag"], a["drowc"],
                                              lddq, lddk, LDDD, LDDRC, wp, wb, st)
        col = np.arange(lddq)[None, None, :]
        wr = lambda n: (n in outs) and not refused and not (n == "drowc" and entry != "pc")
        return R.call(go), {"dq": (col < D) & wr("dq"), "dk": wr("dk"), "ddiag": (np.arange(LDDD) == 0)[None, None, :] & wr("ddiag"),
                            "drowc": (np.arange(LDDRC) == 0)[None, None, :] & wr("drowc")}
    return case


def _bwd_guard(C, T, D, group=0, pitch=0):
    return sc.guard_bytes(T, C // (group or C) * (pitch or C), 2 * D + 1)


def _check_bwd(o, C, T, D, mode, what, group=0, pitch=0, prec=0):
    """Assertion 5 for whatever outputs the run has: dq, dk and drowc inside their bounds against float64, ddiag bit-equal to dS[t,t,c]."""
    group, pitch = group or C, pitch or C
    real, _ = sc.slot_index(C, group, pitch)
    dS = _cotangent(T, C // group * pitch).numpy()[:, :, real]
    q, k, _, _ = (x.numpy() for x in _fwd_data(C, T, D))
    ref, bound = sc.bwd_ref(dS, q, k, sc.qscale_of(D), mode, prec)
    if o.mask["dq"].any():
        sc.assert_within("dq", o.val["dq"][:, :, :D], ref["dq"], bound["dq"], what)
    if o.mask["dk"].any():
        sc.assert_within("dk", o.val["dk"][:, :, :D], ref["dk"], bound["dk"], what)
    if o.mask["drowc"].any():
        sc.assert_within("drowc", o.val["drowc"][:, :, 0], ref["drowc"], bound["drowc"], what)
    if o.mask["ddiag"].any():
        want = np.ascontiguousarray(np.stack([dS[t, t] for t in range(T)]).T)                      # [C][T]
        got = np.ascontiguousarray(o.val["ddiag"][:, :, 0])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: `ddiag` is not bit-equal to dS[t,t,c]"


def _bwd_contract(C, T, D, mode, dev, what, **kw):
    """The five assertions, and the cells the backward must ignore (S5): the pattern in e < b and in the ghost slots gives the bits
    that zeros give.  Returns the run on ordinary tensors."""
    guard = _bwd_guard(C, T, D, kw.get("group", 0), kw.get("pitch", 0))
    o = sc.contract(_bwd_case(C, T, D, mode, dev, **kw), dev, guard, what)
    for pat in (ac.NAN_PATTERN, ac.MAX_PATTERN):
        p = sc.execute(_bwd_case(C, T, D, mode, dev, upper="pattern", **kw), dev, pat, guard)
        sc.check_same_bits(p, o, f"{what}: pattern {pat:#x} in the ignored cells of dS against zeros")
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("D", [32, 96, 160, 256])
def test_backward_direct_kernels(gpu, D):
    """S5, S6 and the backward bounds on the direct kernels (no workspace): every D / 32 instantiation the list names at T = 1, 2, one
    tile and a part, two tiles less one, two tiles and a part; C = 5 takes the dword loads of dS, C = 8 the 16-byte ones."""
    for i, T in enumerate((1, 2, 33, 63, 70)):
        for C in ((5, 8) if T == 33 else (5,)):
            mode = (i + D // 32) % 3
            what = f"direct C={C} T={T} D={D} scaling {mode}"
            o = _bwd_contract(C, T, D, mode, gpu, what, ws=None)
            _check_bwd(o, C, T, D, mode, what)
            if C % 4 == 0:                       # dS off 16 bytes: dword loads, the same bits
                p = sc.contract(_bwd_case(C, T, D, mode, gpu, ws=None, dSphase=4), gpu, _bwd_guard(C, T, D), what + ", dS at phase 4")
                sc.check_same_bits(p, o, what + ": dS at phase 4 against phase 0")


@pytest.mark.gpu
def test_backward_falls_back_to_the_direct_kernels(gpu):
    """S7: with ws == NULL, a ws one byte short of interval_score_bwd_workspace_bytes, a ws off 16 bytes, q / k rows that are only
    4-byte aligned, or drowc wanted without dq, interval_score_bwd_ws_pc runs exactly interval_score_bwd (+ the row-sum kernel): the
    same bits.  At the same shape the packed path gives other bits somewhere, so the comparison can tell the two apart."""
    C, T, D, mode = 5, 70, 64, 0
    base = _bwd_contract(C, T, D, mode, gpu, "interval_score_bwd", entry="plain", outs=("dq", "dk", "ddiag"))
    _check_bwd(base, C, T, D, mode, "interval_score_bwd")
    rows = None
    for what, kw in (("ws NULL", dict(ws=None)), ("ws one byte short", dict(ws="short")), ("ws at phase 4", dict(ws="phase4")),
                     ("packed-slice rows", dict(layout="packed")), ("drowc without dq", dict(outs=("dk", "ddiag", "drowc")))):
        o = _bwd_contract(C, T, D, mode, gpu, what, **kw)
        _check_bwd(o, C, T, D, mode, what)
        for n in ("dq", "dk", "ddiag"):
            if o.mask[n].any():
                assert np.array_equal(o.words(n)[o.mask[n]], base.words(n)[base.mask[n]]), f"{what}: `{n}` differs from interval_score_bwd's"
        if rows is None:
            rows = o.val["drowc"].copy()
        else:
            assert np.array_equal(o.val["drowc"][:, :, 0].view(np.uint32), rows[:, :, 0].view(np.uint32)), f"{what}: `drowc` differs"
    packed = _bwd_contract(C, T, D, mode, gpu, "packed")
    _check_bwd(packed, C, T, D, mode, "packed")
    assert (packed.words("dq")[packed.mask["dq"]] != base.words("dq")[base.mask["dq"]]).any(), "the packed path gave the direct kernels' bits"


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16x3"])
@pytest.mark.parametrize("D,T", [(D, T) for D in (64, 128, 256) for T in (64, 65, 129, 257)])
def test_backward_packed_gemms(gpu, D, T, prec):
    """S5 - S8 on the packed path (exactly interval_score_bwd_workspace_bytes bytes of pattern between guards), exact and three-limb
    (SEMICRF_LEN_BF16X3: the header's 2^-21 term on top; ddiag stays a copy, drowc an exact fp32 sum): one tile, a tile and a row, two
    128-row blocks and a row, three; one chain, a part of a pack block, more than eight."""
    for C in (1, 5, 9):
        mode = (T + C) % 3
        what = f"packed C={C} T={T} D={D} scaling {mode} prec {prec}"
        assert _packed_applies(C, T, D, ALL_OUTS, "exact", "pad", gpu)
        o = _bwd_contract(C, T, D, mode, gpu, what, prec=prec)
        _check_bwd(o, C, T, D, mode, what, prec=prec)


@pytest.mark.gpu
@pytest.mark.parametrize("C,T,D", [(5, 65, 64), (5, 33, 96)], ids=["packed", "direct"])
def test_backward_output_subsets(gpu, C, T, D):
    """S6: any output may be NULL; a NULL output touches nothing, the others get the bits of the call that asks for everything."""
    full = _bwd_contract(C, T, D, 1, gpu, "all outputs")
    _check_bwd(full, C, T, D, 1, "all outputs")
    for outs in (("dq",), ("dk",), ("dq", "dk", "ddiag"), ("dq", "drowc")):
        what = "outputs " + "+".join(outs)
        o = _bwd_contract(C, T, D, 1, gpu, what, outs=outs)
        _check_bwd(o, C, T, D, 1, what)
        for n in outs:
            assert np.array_equal(o.words(n)[o.mask[n]], full.words(n)[full.mask[n]]), f"{what}: `{n}` differs from the call with every output"


@pytest.mark.gpu
@pytest.mark.parametrize("group,pitch", [(5, 8), (6, 8)])
def test_backward_slot_layout(gpu, group, pitch):
    """S5 with a padded pitch: dS is slot-indexed, the ghost slots' cells are ignored (the CRF's gradient there is not zero), the
    outputs are chain-indexed.  Without the packed path a padded pitch is SEMICRF_EINVAL and nothing is written."""
    C, T, D = 2 * group, 129, 64
    for prec in (0, 1):
        what = f"slots {group}->{pitch} prec {prec}"
        o = _bwd_contract(C, T, D, 0, gpu, what, group=group, pitch=pitch, prec=prec)
        _check_bwd(o, C, T, D, 0, what, group=group, pitch=pitch, prec=prec)
        p = sc.contract(_bwd_case(C, T, D, 0, gpu, group=group, pitch=pitch, prec=prec, dSphase=12), gpu, _bwd_guard(C, T, D, group, pitch),
                        what + ", dS at phase 12")
        sc.check_same_bits(p, o, what + ": dS at phase 12 (the pack kernel's dword loads) against phase 0")
    o = sc.contract(_bwd_case(C, T, D, 0, gpu, group=group, pitch=pitch, ws=None, refused=True), gpu, _bwd_guard(C, T, D, group, pitch),
                    "slots without a workspace", rc=EINVAL)
    assert "packed path" in _err()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1], ids=["fp32", "bf16x3"])
def test_backward_workspace_contents_do_not_matter(gpu, prec):
    """S8: the workspace is exactly interval_score_bwd_workspace_bytes(C, T, D) bytes (the 4096 bytes of slack for the transposed walk
    are part of that figure), and what it held before -- 0x00, 0xFF, the arena's pattern -- reaches no result."""
    C, T, D = 5, 129, 128
    guard = _bwd_guard(C, T, D)
    runs = [sc.execute(_bwd_case(C, T, D, 0, gpu, ws_fill=fill, prec=prec), gpu, ac.NAN_PATTERN, guard) for fill in (0x00, 0xFF, None)]
    runs.append(sc.execute(_bwd_case(C, T, D, 0, gpu, ws_fill=None, prec=prec), gpu, ac.MAX_PATTERN, guard))
    for r, name in zip(runs[1:], ("0xFF", "the NaN pattern", "the FLT_MAX pattern")):
        sc.check_same_bits(r, runs[0], f"workspace filled with {name} against 0x00")
    _check_bwd(runs[0], C, T, D, 0, "workspace 0x00", prec=prec)


@pytest.mark.gpu
def test_backward_entry_point_forms(gpu):
    """S4: interval_score_bwd_ws and _ws_p are _ws_pc without a row constant (and without slots): the same bits, packed and direct;
    interval_score_bwd is the direct kernels."""
    for C, T, D in ((5, 65, 64), (5, 33, 96)):
        outs = ("dq", "dk", "ddiag")
        pc = _bwd_contract(C, T, D, 2, gpu, "_ws_pc", outs=outs)
        for entry in ("p", "ws") + (("plain",) if D == 96 else ()):
            o = _bwd_contract(C, T, D, 2, gpu, entry, outs=outs, entry=entry)
            sc.check_same_bits(o, pc, f"C={C} T={T} D={D}: entry form {entry} against _ws_pc")


# =================================================================================================================================================
# C.  interval_score_bwd_fused[_ws[_p|_pc]] and interval_score_path_bwd[_p|_pc]
# =================================================================================================================================================
FUSED_SCALE = 0.25          # q and k of the fused cases: scores of a few units, so that the marginals are spread over many cells
# The fused bound.  The derivable part: the kernel evaluates exp(x), x = alpha[b] + beta[e] + S[e,b] - logZ (- 2 softplus(S) on the
# diagonal), in fp32: |delta G| <= G u (|alpha| + |S| + |beta| + |logZ| + 4) for the operands it is GIVEN.  Those operands are the
# library's own fp32 sweeps of its own fp32 scores, whose distance from the float64 marginals of the float64 scores (the reference
# of this test) is the error of a whole path's sum -- not a per-cell rounding, and not derivable from the cell's own terms.  That excess
# is therefore MEASURED: against the non-fused op fed the float64 marginals rounded to fp32, in units of
# sum_b |G k| (dq, dk), sum_b |G| (drowc) and G[t,t] (ddiag); the constant is twice the worst value seen.  Measured on the MI355X:
# (T, C, D) = (70, 6, 64), direct kernels: dq 2.85e-5, dk 2.92e-5, drowc 2.61e-5, ddiag 3.06e-5; (129, 6, 128), packed path: dq 6.20e-5,
# dk 6.08e-5, drowc 6.09e-5, ddiag 6.81e-5 (the worst).  With the derived term alone the worst element is at 2.69 times its bound (ddiag,
# T = 129; dq 2.39), i.e. the per-cell rounding is a third of what is seen and the sweeps' own error the rest.  Figures: DESIGN.md section 4.
FUSED_EXCESS = 2 * 6.82e-5


def _fused_inputs(dev, C, T, D, mode):
    """S (the library's forward of q, k, diag), alpha / logZ (semicrf_logz_fwd), beta (semicrf_beta), gout -- host tensors."""
    q, k, dg, _ = _fwd_data(C, T, D, FUSED_SCALE)
    qs = sc.qscale_of(D)
    qd, kd, dd = q.to(dev), k.to(dev), dg.to(dev)
    S = torch.empty(T, T, C, dtype=F32, device=dev)
    noise = torch.empty(T - 1, C, dtype=F32, device=dev)
    st = sc.stream(dev)
    assert L.interval_score_fwd(P(qd), P(kd), P(dd), C, T, D, D, D, 1, qs, mode, 0, P(S), P(noise), st) == OK, _err()
    alpha, beta = torch.empty(T, C, dtype=F32, device=dev), torch.empty(T, C, dtype=F32, device=dev)
    logZ = torch.empty(C, dtype=F32, device=dev)
    ws = _lib.workspace(_lib.OP_LOGZ_FWD, T, C, dev)
    assert L.semicrf_logz_fwd(P(S), P(noise), T, C, P(logZ), P(alpha), P(ws), ws.numel(), st) == OK, _err()
    assert L.semicrf_beta(P(S), P(noise), T, C, P(beta), P(ws), ws.numel(), st) == OK, _err()
    torch.cuda.synchronize(dev)
    gout = sc.normal((C,), 77) + 2.0
    return q, k, dg, S.cpu(), alpha.cpu(), beta.cpu(), logZ.cpu(), gout


def _fused_case(inp, C, T, D, mode, dev, entry, upper="zero", ws="exact", phases=(0, 0, 0)):
    """Read (S9): S in the cells e >= b, alpha, beta [T][C], logZ, gout [C], q, k.  Written: as the plain backward."""
    q, k, _, S, alpha, beta, logZ, gout = inp
    qs = sc.qscale_of(D)
    ign = _ignored_cells(T, C, 0, 0)
    ld, lddq, lddk = D + 4, D + 4, D
    nws = int(L.interval_score_bwd_workspace_bytes(C, T, D))

    def case(R):
        s = R.inp("S", _with_ignored(S, ign, R, upper), phases[0])
        al, be, lz, go_ = R.inp("alpha", alpha, phases[1]), R.inp("beta", beta, phases[2]), R.inp("logZ", logZ, 4), R.inp("gout", gout, 8)
        qa, ka = R.inp_strided("q", q, ld), R.inp_strided("k", k, ld)
        o = {"dq": R.out("dq", (C, T, lddq)), "dk": R.out("dk", (C, T, lddk)), "ddiag": R.out("ddiag", (C, T, LDDD)),
             "drowc": R.out("drowc", (C, T, LDDRC))}
        w = R.ws("ws", nws) if ws else None
        wp = P(w) if (w is not None and nws) else None
        st = sc.stream(dev)

        def go():
            if entry == "plain":
                return L.interval_score_bwd_fused(P(s), P(al), P(be), P(lz), P(go_), P(qa), P(ka), C, T, D, ld, ld, qs, mode, P(o["dq"]),
                                                  P(o["dk"]), P(o["ddiag"]), lddq, lddk, LDDD, st)
            if entry == "ws":
                return L.interval_score_bwd_fused_ws(P(s), P(al), P(be), P(lz), P(go_), P(qa), P(ka), C, T, D, ld, ld, qs, mode, P(o["dq"]),
                                                     P(o["dk"]), P(o["ddiag"]), lddq, lddk, LDDD, wp, nws if wp else 0, st)
            return L.interval_score_bwd_fused_ws_pc(P(s), P(al), P(be), P(lz), P(go_), P(qa), P(ka), C, T, D, ld, ld, qs, mode, C, C,
                                                    P(o["dq"]), P(o["dk"]), P(o["ddiag"]), P(o["drowc"]), lddq, lddk, LDDD, LDDRC, wp,
                                                    nws if wp else 0, st)
        col = np.arange(lddq)[None, None, :]
        return R.call(go), {"dq": col < D, "dk": True, "ddiag": (np.arange(LDDD) == 0)[None, None, :],
                            "drowc": (np.arange(LDDRC) == 0)[None, None, :] & (entry == "pc")}
    return case


def _fused_reference(inp, C, T, D, mode):
    """float64 marginals of the float64 scores -> the cotangent G = gout * marginal, the gradients and the derived bounds; and the
    per-cell rounding term E = G u (|alpha| + |S| + |beta| + |logZ| + 4 (+ 2 softplus(S) on the diagonal))."""
    q, k, dg, _, _, _, _, gout = inp
    qn, kn = q.numpy(), k.numpy()
    qs = sc.qscale_of(D)
    S64, _ = sc.fwd_ref(qn, kn, dg.numpy(), None, qs, mode)
    marg, al, be, lz = sc.marginals64(S64)
    G = marg * gout.numpy().astype(np.float64)[None, None, :]
    e, b = np.arange(T)[:, None, None], np.arange(T)[None, :, None]
    E = np.abs(G) * U * (np.abs(al)[None, :, :] + np.abs(S64) + np.abs(be)[:, None, :] + np.abs(lz)[None, None, :] + 4.0
                         + np.where(e == b, 2.0 * np.log1p(np.exp(np.minimum(np.abs(S64), 50.0))), 0.0))
    ref, bound = sc.bwd_ref(G, qn, kn, qs, mode)
    w = (float(qs) * sc.len64(mode, e - b))
    Ew = np.where(e >= b, E * w, 0.0).transpose(2, 0, 1)
    Gw = np.where(e >= b, np.abs(G) * w, 0.0).transpose(2, 0, 1)
    term = {"dq": np.matmul(Ew, np.abs(kn.astype(np.float64))), "dk": np.matmul(Ew.transpose(0, 2, 1), np.abs(qn.astype(np.float64))),
            "drowc": Ew.sum(2)}
    unit = {"dq": np.matmul(Gw, np.abs(kn.astype(np.float64))), "dk": np.matmul(Gw.transpose(0, 2, 1), np.abs(qn.astype(np.float64))),
            "drowc": Gw.sum(2)}
    diag = np.stack([G[t, t] for t in range(T)]).T
    ediag = np.stack([E[t, t] for t in range(T)]).T
    return G, ref, bound, {n: bound[n] + term[n] for n in term}, unit, diag, ediag


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,D", [(70, 6, 64), (129, 6, 128)], ids=["direct", "packed"])
def test_backward_fused(gpu, T, C, D):
    """S9: interval_score_bwd_fused[_ws[_pc]] with alpha, beta and logZ from the library's own sweeps of the forward's S: the arena
    assertions, the cells e < b of S ignored, the entry forms' bits, and every element against float64 marginals of float64 scores."""
    mode = 0
    inp = _fused_inputs(gpu, C, T, D, mode)
    guard = sc.guard_bytes(T, C, D + 4)
    what = f"fused T={T} C={C} D={D}"
    ws = "exact" if T >= 128 else None          # (70, 6, 64): the direct kernels (no workspace); (129, 6, 128): the packed path
    o = sc.contract(_fused_case(inp, C, T, D, mode, gpu, "pc", ws=ws), gpu, guard, what)
    for pat in (ac.NAN_PATTERN, ac.MAX_PATTERN):
        p = sc.execute(_fused_case(inp, C, T, D, mode, gpu, "pc", upper="pattern", ws=ws), gpu, pat, guard)
        sc.check_same_bits(p, o, f"{what}: pattern {pat:#x} above the diagonal of S against zeros")
    w = sc.contract(_fused_case(inp, C, T, D, mode, gpu, "ws", ws=ws), gpu, guard, what + " _ws")
    for n in ("dq", "dk", "ddiag"):
        assert np.array_equal(w.words(n), o.words(n)), f"{what}: `{n}` of _fused_ws differs from _fused_ws_pc's"
    d = sc.contract(_fused_case(inp, C, T, D, mode, gpu, "plain"), gpu, guard, what + " direct")
    if ws is None:
        for n in ("dq", "dk", "ddiag"):
            assert np.array_equal(d.words(n), o.words(n)), f"{what}: `{n}`: _fused_ws did not fall back to interval_score_bwd_fused"
    # against float64, and the measured part of the bound: the non-fused op on the float64 marginals rounded to fp32
    G, ref, bound, derived, unit, diag, ediag = _fused_reference(inp, C, T, D, mode)
    G32 = torch.from_numpy(G.astype(np.float32))
    q, k = inp[0], inp[1]
    Gd, qd, kd = G32.to(gpu), q.to(gpu), k.to(gpu)
    outs = {"dq": torch.zeros(C, T, D, device=gpu), "dk": torch.zeros(C, T, D, device=gpu), "ddiag": torch.zeros(C, T, device=gpu),
            "drowc": torch.zeros(C, T, device=gpu)}
    nws = int(L.interval_score_bwd_workspace_bytes(C, T, D)) if ws else 0          # (the same path as the fused call)
    wsd = torch.empty(max(nws, 16), dtype=torch.uint8, device=gpu)
    assert L.interval_score_bwd_ws_pc(P(Gd), P(qd), P(kd), C, T, D, D, D, sc.qscale_of(D), mode, C, C, P(outs["dq"]), P(outs["dk"]),
                                      P(outs["ddiag"]), P(outs["drowc"]), D, D, 1, 1, P(wsd) if nws else None, nws, sc.stream(gpu)) == OK, _err()
    torch.cuda.synchronize(gpu)
    got = {"dq": o.val["dq"][:, :, :D], "dk": o.val["dk"], "drowc": o.val["drowc"][:, :, 0], "ddiag": o.val["ddiag"][:, :, 0]}
    unit["ddiag"] = np.abs(diag)
    excess = {}
    for n in got:
        nf = outs[n].cpu().numpy().astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(unit[n] > 0, np.abs(got[n].astype(np.float64) - nf) / unit[n], 0.0)
        excess[n] = float(r.max())
        print(f"{what}: `{n}` fused against non-fused on float64 marginals: worst excess {excess[n]:.3e} of its unit")
    ref["ddiag"], bound["ddiag"], derived["ddiag"] = diag, U * np.abs(diag), ediag + U * np.abs(diag)
    for n in got:
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(derived[n] > 0, np.abs(got[n].astype(np.float64) - ref[n]) / derived[n], 0.0)
        print(f"{what}: `{n}` worst |error| in units of the derived (per-cell rounding) bound alone: {float(r.max()):.3f}")
        sc.assert_within(n, got[n], ref[n], bound[n] + FUSED_EXCESS * unit[n], what)


@pytest.mark.gpu
@pytest.mark.parametrize("T,C,D,ws", [(33, 8, 32, None), (65, 8, 64, "exact")], ids=["direct", "packed"])
def test_backward_fused_operands_off_16_bytes(gpu, T, C, D, ws):
    """S9: with C % 4 == 0 the fused kernels load four chains of S, alpha and beta at once -- only when all three are 16-byte aligned;
    any one of them at another phase gives the aligned call's bits."""
    inp = _fused_inputs(gpu, C, T, D, 1)
    guard = sc.guard_bytes(T, C, D + 4)
    ref = sc.contract(_fused_case(inp, C, T, D, 1, gpu, "pc", ws=ws), gpu, guard, "aligned")
    for phases in ((4, 0, 0), (0, 4, 0), (0, 0, 12), (8, 4, 12)):
        o = sc.contract(_fused_case(inp, C, T, D, 1, gpu, "pc", ws=ws, phases=phases), gpu, guard, f"S / alpha / beta at phases {phases}")
        sc.check_same_bits(o, ref, f"fused T={T} C={C} D={D}: S / alpha / beta at phases {phases} against the aligned call")


def _paths(T):
    """Sorted intervals [begin, end] per chain: none; a zero-length one and an ordinary one; one from frame 0 and one that ends at
    T - 1; two that touch."""
    return [[], [(3, 3), (5, 9)], [(0, 4), (10, T - 1)], [(2, 7), (7, 12)]]


def _path_case(C, T, D, mode, dev, group, pitch, paths, outs=ALL_OUTS):
    """interval_score_path_bwd_pc ADDS (S10): outputs hold hash_normal values before the call, rows and entries off every path keep
    their bits."""
    real, _ = sc.slot_index(C, group, pitch)
    Cs = C // group * pitch
    q, k, _, _ = _fwd_data(C, T, D)
    qs = sc.qscale_of(D)
    pairs = torch.tensor([p for ch in paths for p in ch], dtype=I32).reshape(-1, 2)
    counts = np.zeros(Cs, dtype=np.int64)
    counts[real] = [len(ch) for ch in paths]
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    gout = sc.normal((Cs,), 91) + 1.5
    K = int(pairs.shape[0])
    ld, lddq, lddk = D + 4, D + 4, D
    old = {"dq": sc.normal((C, T, lddq), 301), "dk": sc.normal((C, T, lddk), 302), "ddiag": sc.normal((C, T, LDDD), 303),
           "drowc": sc.normal((C, T, LDDRC), 304)}
    masks = {n: np.zeros(tuple(old[n].shape), dtype=bool) for n in old}
    for c, ch in enumerate(paths):
        for b, e in ch:
            masks["dq"][c, e, :D] = "dq" in outs
            masks["dk"][c, b, :D] = "dk" in outs
            masks["drowc"][c, e, 0] = "drowc" in outs
            if b == e:
                masks["ddiag"][c, e, 0] = "ddiag" in outs

    def case(R):
        g, pr, of = R.inp("gout", gout), R.inp("pairs", pairs if K else torch.zeros(1, 2, dtype=I32)), R.inp("offsets", offsets)
        qa, ka = R.inp_strided("q", q, ld), R.inp_strided("k", k, ld)
        o = {n: R.out(n, tuple(old[n].shape), init=old[n]) for n in ALL_OUTS}
        a = {n: (P(o[n]) if n in outs else None) for n in ALL_OUTS}
        st = sc.stream(dev)
        return R.call(lambda: L.interval_score_path_bwd_pc(P(g), P(pr) if K else None, K, P(of), P(qa), P(ka), C, T, D, ld, ld, qs, mode, group,
                                                           pitch, a["dq"], a["dk"], a["ddiag"], a["drowc"], lddq, lddk, LDDD, LDDRC, st)), masks
    return case, old, gout, real


@pytest.mark.gpu
@pytest.mark.parametrize("group,pitch", [(4, 4), (2, 4)], ids=["contiguous", "slots"])
def test_path_backward(gpu, group, pitch):
    """S10: one wave per interval adds w k_b to dq[e], w q_e to dk[b], w to drowc[e] and gout to ddiag[e] when b == e; everything else
    keeps its bits; K == 0 launches nothing.  Bound per touched element: (terms + 2) u sum |terms| + u |old|: the weight, its product with the
    row and the add to the old value."""
    C, T, D = 4, 40, 64
    for mode in (0, 1, 2):
        for paths in (_paths(T), [[], [], [], []]):
            case, old, gout, real = _path_case(C, T, D, mode, gpu, group, pitch, paths)
            what = f"path backward scaling {mode} group {group} pitch {pitch} K={sum(len(p) for p in paths)}"
            o = sc.contract(case, gpu, sc.guard_bytes(T, C, D + 4), what)
            q, k, _, _ = (x.numpy().astype(np.float64) for x in _fwd_data(C, T, D))
            qs = float(sc.qscale_of(D))
            ref = {n: old[n].numpy().astype(np.float64) for n in old}
            mag = {n: np.zeros_like(ref[n]) for n in old}
            for c, ch in enumerate(paths):
                g = float(gout[real[c]])
                for b, e in ch:
                    w = g * qs * float(sc.len64(mode, e - b))
                    ref["dq"][c, e, :D] += w * k[c, b]; mag["dq"][c, e, :D] += np.abs(w * k[c, b])
                    ref["dk"][c, b, :D] += w * q[c, e]; mag["dk"][c, b, :D] += np.abs(w * q[c, e])
                    ref["drowc"][c, e, 0] += w; mag["drowc"][c, e, 0] += abs(w)
                    if b == e:
                        ref["ddiag"][c, e, 0] += g; mag["ddiag"][c, e, 0] += abs(g)
            for n in old:
                bound = (1 + 2) * U * mag[n] + U * np.abs(old[n].numpy().astype(np.float64))          # (one term per touched element)
                sc.assert_within(n, o.val[n], ref[n], bound, what, mask=o.mask[n])
    case, *_ = _path_case(C, T, D, 0, gpu, group, pitch, _paths(T), outs=("dk", "ddiag"))
    sc.contract(case, gpu, sc.guard_bytes(T, C, D + 4), "path backward, dq and drowc NULL")


# =================================================================================================================================================
# D.  scorer_proj_nn, scorer_proj_nn3, scorer_proj_tn
# =================================================================================================================================================
# options of a scorer_proj_nn call: (name, bias, w2 / b2, zero_cols, accumulate, padded leading dimensions)
NN_OPTS = [
    ("forward_packed", True, True, 2, 0, True),          # [q | diag | 0 0] = x W^T + b
    ("input_grad_tight", False, False, 0, 1, False),     # dx += dy W: lda == K, so the bytes behind A's last row are the guard
    ("input_grad", False, False, 0, 1, True),
    ("bias_only", True, False, 0, 0, True),
    ("extras_no_bias", False, True, 0, 0, True),
    ("accumulate_with_bias_and_extras", True, True, 1, 1, True),      # the bias is NOT added to an accumulating call, the extras are written
]
NN_OPT = {o[0]: o for o in NN_OPTS}
NN_M = [1, 31, 33, 127, 128, 129, 257]


@functools.lru_cache(maxsize=None)
def _nn_data(M, K, N):
    seed = 7000 + M + 3 * K + 5 * N
    Kpad = (K + 31) // 32 * 32
    B = torch.zeros(Kpad, N)
    B[:K] = sc.normal((K, N), seed + 1, 1.0 / 16)
    return (sc.normal((M, K), seed), B, sc.normal((N,), seed + 2), sc.normal((2, K), seed + 3, 1.0 / 16), sc.normal((2,), seed + 4),
            sc.normal((M, N + 16), seed + 5))


def _nn_case(M, K, N, dev, opt, entry="nn", ws="exact", ws_fill=None, refused=False, Aphase=0, lda=None, ldout=None, Kcall=None, Ncall=None):
    """scorer_proj_nn / _nn3.  Read (S11): the K used columns of A's M rows, B's Kpad rows (zero beyond K: the caller's promise), bias
    [N] unless accumulating, w2 [2][K], b2 [2].  Written: the N main columns, with w2 the two extra columns and zero_cols zeros."""
    _, use_bias, use_w2, zc, acc, pad = NN_OPT[opt]
    A, B, bias, w2, b2, old = _nn_data(M, K, N)
    la, lb = (K + 4, N + 4) if pad else (K, N)
    width = N + (2 + zc if use_w2 else 0)
    lo = width + (4 if pad else 0)
    nws = int(L.scorer_proj_nn3_workspace_bytes(K, N)) if entry == "nn3" else 0

    def case(R):
        a = R.inp_strided("A", A, la, Aphase)
        b = R.inp_strided("B", B, lb)
        bi, w, bb = R.inp("bias", bias, 4), R.inp("w2", w2, 8), R.inp("b2", b2, 12)          # any 4-byte aligned address
        out = R.out("out", (M, lo), init=old[:, :lo] if acc else None)
        wsp = R.ws("ws", nws, ws_fill, 4 if ws == "phase4" else 0) if (entry == "nn3" and ws) else None
        st = sc.stream(dev)
        wide = 0 if Ncall is None else Ncall - N                       # (a refused width: leading dimensions that would hold it)
        args = (P(a), la if lda is None else lda, M, K if Kcall is None else Kcall, P(b), lb + wide, N + wide, P(out),
                lo + wide if ldout is None else ldout, P(bi) if use_bias else None, P(w) if use_w2 else None, P(bb) if use_w2 else None, zc, acc)
        if entry == "nn3":
            fn = lambda: L.scorer_proj_nn3(*args, P(wsp) if wsp is not None else None, 0 if wsp is None else (nws - 1 if ws == "short" else nws), st)
        else:
            fn = lambda: L.scorer_proj_nn(*args, st)
        return R.call(fn), {"out": (np.arange(lo) < width)[None, :] & (not refused)}
    return case


def _nn_guard(K, N):
    return sc.guard_bytes(widest_row_floats=max(K, N) + 8)


def _check_nn(o, M, K, N, opt, what, prec=0):
    _, use_bias, use_w2, zc, acc, _ = NN_OPT[opt]
    A, B, bias, w2, b2, old = (x.numpy() for x in _nn_data(M, K, N))
    main, bound, amain, ex, exb = sc.nn_ref(A, B[:K], bias if use_bias else None, w2 if use_w2 else None, b2 if use_w2 else None,
                                            old[:, :N] if acc else None)
    got = o.val["out"]
    sc.assert_within("out", got[:, :N], main, bound + (2.0 ** -21 * amain if prec else 0.0), what)
    if use_w2:
        sc.assert_within("out (extra columns)", got[:, N:N + 2], ex, exb, what)
        assert not got[:, N + 2:N + 2 + zc].view(np.uint32).any(), f"{what}: the zero columns are not exactly +0.0f"


NN_PAIRS = [(K, N) for K in (64, 128, 256) for N in (64, 128, 256)] + [(68, 64), (132, 128), (260, 256), (260, 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", NN_PAIRS)
def test_proj_nn_every_width(gpu, K, N):
    """S11 for scorer_proj_nn: all nine (K, N) and the input-gradient forms whose K is no multiple of 32 (Kpad 96, 160, 288: the last
    chunk's clamp at K; without w2 the 4-wide tail runs as ONE group of matrix instructions), at M = 129 (a whole tile and a row: the
    clamp at M), every combination of bias, the two extra columns, zero columns and accumulation."""
    M = 129
    for opt in NN_OPT:
        what = f"proj_nn M={M} K={K} N={N} {opt}"
        o = sc.contract(_nn_case(M, K, N, gpu, opt), gpu, _nn_guard(K, N), what)
        _check_nn(o, M, K, N, opt, what)
    a, b = (sc.contract(_nn_case(M, K, N, gpu, opt), gpu, _nn_guard(K, N), opt) for opt in ("accumulate_with_bias_and_extras", "input_grad"))
    assert np.array_equal(a.words("out")[:, :N], b.words("out")[:, :N]), "the bias reached an accumulating call's result"


@pytest.mark.gpu
@pytest.mark.parametrize("M", NN_M)
def test_proj_nn_every_row_count(gpu, M):
    """S11: one row, a tile less one, a tile, a tile and one, two tiles and one ... for the forward's and the input gradient's forms."""
    for K, N in ((256, 256), (260, 64)):
        for opt in ("forward_packed", "input_grad_tight", "input_grad"):
            what = f"proj_nn M={M} K={K} N={N} {opt}"
            o = sc.contract(_nn_case(M, K, N, gpu, opt), gpu, _nn_guard(K, N), what)
            _check_nn(o, M, K, N, opt, what)


@pytest.mark.gpu
@pytest.mark.parametrize("M", NN_M)
def test_proj_nn3(gpu, M):
    """S11 for scorer_proj_nn3 (N == 256): exactly scorer_proj_nn3_workspace_bytes bytes whose earlier contents do not matter; the
    header's 2^-21 sum |a b| on top of the fp32 accumulation term; with ws == NULL, one byte short or off 16 bytes the exact kernel's
    bits -- and with the workspace other bits somewhere, i.e. the three-limb kernel ran."""
    N = 256
    for K in (256, 260):
        for opt in ("forward_packed", "input_grad"):
            what = f"proj_nn3 M={M} K={K} {opt}"
            guard = _nn_guard(K, N)
            o = sc.contract(_nn_case(M, K, N, gpu, opt, entry="nn3"), gpu, guard, what)
            _check_nn(o, M, K, N, opt, what, prec=1)
            for fill in (0x00, 0xFF):
                s = sc.execute(_nn_case(M, K, N, gpu, opt, entry="nn3", ws_fill=fill), gpu, ac.NAN_PATTERN, guard)
                sc.check_same_bits(s, o, f"{what}: workspace filled with {fill:#04x} against the pattern")
            exact = sc.contract(_nn_case(M, K, N, gpu, opt), gpu, guard, what + " (exact)")
            for ws in (None, "short", "phase4"):
                f = sc.contract(_nn_case(M, K, N, gpu, opt, entry="nn3", ws=ws), gpu, guard, f"{what} ws {ws}")
                sc.check_same_bits(f, exact, f"{what}: ws {ws} against scorer_proj_nn")
            assert (o.words("out")[:, :N] != exact.words("out")[:, :N]).any(), f"{what}: the three-limb kernel gave the exact kernel's bits"
            if "forward" in opt:
                assert np.array_equal(o.val["out"][:, N + 2:].view(np.uint32), exact.val["out"][:, N + 2:].view(np.uint32))


TN_M = [1, 2, 33, 257, 700]
TN_PAIRS = [(64, 64), (128, 256), (256, 64), (256, 256)]


@functools.lru_cache(maxsize=None)
def _tn_data(M, R, N):
    seed = 9000 + M + 3 * R + 5 * N
    return sc.normal((M, R + 2), seed), sc.normal((M, N), seed + 1)


def _tn_case(M, R, N, dev, extra, ws="exact", ws_fill=None, prec=0, refused=False, dyphase=0, lddy=None, extra_col0=None, Ncall=None):
    """scorer_proj_tn.  Read (S11): the R main columns of dy's M rows and, with extra columns, the two at extra_col0; the N used columns
    of x.  Written: dW [total_rows][lddw] in its N used columns, db [total_rows]; rows / entries R + 2 .. total_rows - 1 are zeros."""
    dy, x = _tn_data(M, R, N)
    ldy, ldx, ldw = R + 4, N + 4, N + 4
    total = R + 4 if extra else R
    nws = int(L.scorer_proj_tn_workspace_bytes(M, R, N))

    def case(R_):
        a = R_.inp_strided("dy", dy, ldy, dyphase)
        b = R_.inp_strided("x", x, ldx)
        dW, db = R_.out("dW", (total + 3, ldw)), R_.out("db", (total + 3,))
        w = R_.ws("ws", nws, ws_fill, 4 if ws == "phase4" else 0) if ws else None
        st = sc.stream(dev)
        ec = (R if extra else -1) if extra_col0 is None else extra_col0
        wide = 0 if Ncall is None else Ncall - N                       # (a refused width: leading dimensions that would hold it)
        fn = lambda: L.scorer_proj_tn(P(a), ldy if lddy is None else lddy, M, R, ec, total | (BF16X3_TN if prec else 0), P(b), ldx + wide,
                                      N + wide, P(dW), ldw + wide, P(db), P(w) if w is not None else None,
                                      0 if w is None else (nws - 1 if ws == "short" else nws), st)
        rows = (np.arange(total + 3) < total) & (not refused)
        return R_.call(fn), {"dW": rows[:, None] & (np.arange(ldw) < N)[None, :], "db": rows}
    return case


def _check_tn(o, M, R, N, extra, what, prec=0):
    dy, x = (t.numpy() for t in _tn_data(M, R, N))
    used = R + 2 if extra else R
    dW, bW, aW, db, bb = sc.tn_ref(dy[:, :used], x)
    if prec:
        bW[:R] += 2.0 ** -21 * aW[:R]
    sc.assert_within("dW", o.val["dW"][:used, :N], dW, bW, what)
    sc.assert_within("db", o.val["db"][:used], db, bb, what)
    if extra:
        assert not o.val["dW"][used:R + 4, :N].view(np.uint32).any() and not o.val["db"][used:R + 4].view(np.uint32).any(), \
            f"{what}: the rows behind the two extra ones are not exactly +0.0f"


@pytest.mark.gpu
@pytest.mark.parametrize("R,N", TN_PAIRS)
def test_proj_tn(gpu, R, N):
    """S11 for scorer_proj_tn: one and two rows (a slice of one chunk), a chunk and a row, many chunks, more slices than one; with the
    two extra columns (extra_col0 = R, total_rows = R + 4, lddy = R + 4) and without; exactly scorer_proj_tn_workspace_bytes bytes whose
    earlier contents do not matter; the three-limb form (N == 256) leaves the two extra rows and the bias gradient the exact call's bits."""
    guard = sc.guard_bytes(widest_row_floats=max(R, N) + 8)
    for M in TN_M:
        for extra in (True, False):
            what = f"proj_tn M={M} R={R} N={N} extra {extra}"
            o = sc.contract(_tn_case(M, R, N, gpu, extra), gpu, guard, what)
            _check_tn(o, M, R, N, extra, what)
            for fill in (0x00, 0xFF):
                s = sc.execute(_tn_case(M, R, N, gpu, extra, ws_fill=fill), gpu, ac.NAN_PATTERN, guard)
                sc.check_same_bits(s, o, f"{what}: workspace filled with {fill:#04x} against the pattern")
            if N == 256:
                t = sc.contract(_tn_case(M, R, N, gpu, extra, prec=1), gpu, guard, what + " bf16x3")
                _check_tn(t, M, R, N, extra, what + " bf16x3", prec=1)
                assert np.array_equal(t.words("db"), o.words("db")), f"{what}: the three-limb call's bias gradient differs"
                if extra:
                    assert np.array_equal(t.words("dW")[R:R + 4], o.words("dW")[R:R + 4]), f"{what}: the three-limb call's extra rows differ"
        for ws in (None, "short", "phase4"):
            o = sc.contract(_tn_case(33, R, N, gpu, True, ws=ws, refused=True), gpu, guard, f"proj_tn ws {ws}", rc=EWORKSPACE)
            assert "workspace" in _err()


# =================================================================================================================================================
# E.  scorer_stage_linear, scorer_merge_weights_fwd, scorer_merge_weights_bwd
# =================================================================================================================================================
MERGE_SHAPES = [(64, 64), (100, 100), (128, 256), (256, 256)]          # (size, D)


@functools.lru_cache(maxsize=None)
def _linear(size, D):
    seed = 11000 + size + 3 * D
    return sc.normal((2 * D + 1, size), seed, 1.0 / 16), sc.normal((2 * D + 1,), seed + 1, 0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("size,D", MERGE_SHAPES)
def test_stage_linear(gpu, size, D):
    """S12 for scorer_stage_linear: BT [size][2 D], Wqd [rows_pad][size], w2 [2][size], b2 [2] are pure rearrangements of W and bias
    (bit-equal), the rows of Wqd behind the diagonal row and the second row of w2 / entry of b2 exactly zero; nothing else is written."""
    W, bias = _linear(size, D)
    rows_pad = D + 1 + 5

    def case(R):
        w, b = R.inp("W", W, 4), R.inp("bias", bias, 8)
        BT, Wqd, w2, b2 = R.out("BT", (size * 2 * D + 3,)), R.out("Wqd", (rows_pad * size + 3,)), R.out("w2", (2 * size + 3,)), R.out("b2", (5,))
        rc = R.call(lambda: L.scorer_stage_linear(P(w), P(b), D, size, rows_pad, P(BT), P(Wqd), P(w2), P(b2), sc.stream(gpu)))
        return rc, {"BT": np.arange(size * 2 * D + 3) < size * 2 * D, "Wqd": np.arange(rows_pad * size + 3) < rows_pad * size,
                    "w2": np.arange(2 * size + 3) < 2 * size, "b2": np.arange(5) < 2}
    o = sc.contract(case, gpu, sc.guard_bytes(widest_row_floats=2 * D), f"stage_linear size={size} D={D}")
    Wn, bn = W.numpy(), bias.numpy()
    eq = lambda got, want: np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).view(np.uint32))
    assert eq(o.val["BT"][:size * 2 * D].reshape(size, 2 * D), Wn[:2 * D].T)
    Wqd = np.zeros((rows_pad, size), dtype=np.float32)
    Wqd[:D], Wqd[D] = Wn[:D], Wn[2 * D]
    assert eq(o.val["Wqd"][:rows_pad * size].reshape(rows_pad, size), Wqd)
    assert eq(o.val["w2"][:2 * size].reshape(2, size), np.stack([Wn[2 * D], np.zeros(size, dtype=np.float32)]))
    assert eq(o.val["b2"][:2], np.array([bn[2 * D], 0.0], dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("size,D", MERGE_SHAPES)
def test_merge_weights(gpu, size, D):
    """S12 for scorer_merge_weights_fwd / _bwd: rows more than the minimum (the zero rows exactly zero), WmT present and NULL (the same
    Wm bits), every element inside (n + 4) u sum |.|; the backward's workspace is exactly scorer_merge_weights_bwd_workspace_bytes(size)
    bytes, its earlier contents do not matter, and a short or missing one is SEMICRF_EWORKSPACE with nothing written."""
    W, bias = _linear(size, D)
    rows = size + 2 + 3
    guard = sc.guard_bytes(widest_row_floats=size)

    def fwd(with_T):
        def case(R):
            w, b = R.inp("W", W, 4), R.inp("bias", bias, 8)
            Wm, bm, WmT = R.out("Wm", (rows * size + 3,), 4), R.out("bm", (rows + 3,), 8), R.out("WmT", (size * size + 3,), 12)
            rc = R.call(lambda: L.scorer_merge_weights_fwd(P(w), P(b), D, size, rows, P(Wm), P(bm), P(WmT) if with_T else None, sc.stream(gpu)))
            return rc, {"Wm": np.arange(rows * size + 3) < rows * size, "bm": np.arange(rows + 3) < rows,
                        "WmT": (np.arange(size * size + 3) < size * size) & with_T}
        return case
    o = sc.contract(fwd(True), gpu, guard, f"merge_weights_fwd size={size} D={D}")
    n = sc.contract(fwd(False), gpu, guard, f"merge_weights_fwd size={size} D={D}, WmT NULL")
    assert np.array_equal(o.words("Wm"), n.words("Wm")) and np.array_equal(o.words("bm"), n.words("bm"))
    Wm64, bW, bm64, bb = sc.merge_fwd_ref(W.numpy(), bias.numpy(), D, size)
    Wm = o.val["Wm"][:rows * size].reshape(rows, size)
    sc.assert_within("Wm", Wm[:size + 2], Wm64, bW, f"merge_weights_fwd size={size} D={D}")
    sc.assert_within("bm", o.val["bm"][:size + 2], bm64, bb, f"merge_weights_fwd size={size} D={D}")
    assert not Wm[size + 2:].view(np.uint32).any() and not o.val["bm"][size + 2:rows].view(np.uint32).any(), "the zero rows are not exactly +0.0f"
    assert np.array_equal(o.val["WmT"][:size * size].reshape(size, size).view(np.uint32), np.ascontiguousarray(Wm[:size].T).view(np.uint32))

    dWm, dbm = sc.normal((rows, size), 12001 + size), sc.normal((rows,), 12002 + size)
    nws = int(L.scorer_merge_weights_bwd_workspace_bytes(size))
    assert nws == size * (size + 1) * 4

    def bwd(ws, fill=None):
        def case(R):
            w, b, g, gb = R.inp("W", W, 4), R.inp("bias", bias, 8), R.inp("dWm", dWm, 12), R.inp("dbm", dbm, 4)
            dW, db = R.out("dW", ((2 * D + 1) * size + 3,), 8), R.out("dbias", (2 * D + 1 + 3,), 12)
            wsp = R.ws("ws", nws, fill, 4) if ws else None
            rc = R.call(lambda: L.scorer_merge_weights_bwd(P(w), P(b), P(g), P(gb), D, size, rows, P(dW), P(db), P(wsp) if ws else None,
                                                           0 if not ws else (nws - 1 if ws == "short" else nws), sc.stream(gpu)))
            ok = ws == "exact"
            return rc, {"dW": (np.arange((2 * D + 1) * size + 3) < (2 * D + 1) * size) & ok, "dbias": (np.arange(2 * D + 4) < 2 * D + 1) & ok}
        return case
    what = f"merge_weights_bwd size={size} D={D}"
    o = sc.contract(bwd("exact"), gpu, guard, what)
    for fill in (0x00, 0xFF):
        sc.check_same_bits(sc.execute(bwd("exact", fill), gpu, ac.NAN_PATTERN, guard), o, f"{what}: workspace filled with {fill:#04x}")
    dW64, bW, db64, bb = sc.merge_bwd_ref(W.numpy(), bias.numpy(), dWm.numpy(), dbm.numpy(), D, size)
    sc.assert_within("dW", o.val["dW"][:(2 * D + 1) * size].reshape(2 * D + 1, size), dW64, bW, what)
    sc.assert_within("dbias", o.val["dbias"][:2 * D + 1], db64, bb, what)
    for ws in (None, "short"):
        sc.contract(bwd(ws), gpu, guard, f"{what} ws {ws}", rc=EWORKSPACE)
        assert "workspace" in _err()


# =================================================================================================================================================
# F.  Argument checks of the projection entry points
# =================================================================================================================================================
# (name, entry point, overrides of the ordinary call, what the message names).  Every one of these returns from the entry point's own
# checks (csrc/api.hip) or from the launcher's first lines (launch_proj_nn: proj_gemm_supported; launch_proj_tn: the width and
# rows_addressable, ahead of the workspace's geometry) -- before any HIP call, so the answer is the same on a machine without a GPU.
PROJ_REJECTED = [
    ("nn_A_off_16", "nn", dict(Aphase=4), "16-byte aligned"),
    ("nn_lda_not_times_4", "nn", dict(lda=69), "16-byte aligned"),
    ("nn_N_96", "nn", dict(Ncall=96), "N must be 64, 128 or 256"),
    ("nn_K_66", "nn", dict(Kcall=66), "K % 4 == 0"),
    ("nn_ldout_too_small", "nn", dict(ldout=64 + 3), "ldout too small"),
    ("nn3_A_off_16", "nn3", dict(Aphase=4), "16-byte aligned"),          # not the three-limb kernel's call: the exact kernel's answer
    ("nn3_N_96", "nn3", dict(Ncall=96), "N must be 64, 128 or 256"),
    ("tn_dy_off_16", "tn", dict(dyphase=4), "16-byte aligned"),
    ("tn_lddy_not_times_4", "tn", dict(lddy=64 + 5), "16-byte aligned"),
    ("tn_N_96", "tn", dict(Ncall=96), "N must be 64, 128 or 256"),
    ("tn_extra_columns_inside_R", "tn", dict(extra_col0=63), "bad extra columns"),
]
REJ_M, REJ_K, REJ_N = 33, 64, 64


@pytest.mark.parametrize("name,entry,chg,msg", PROJ_REJECTED, ids=[r[0] for r in PROJ_REJECTED])
def test_projection_rejections_host(name, entry, chg, msg):
    """S11: a pointer off 16 bytes, a leading dimension that is no multiple of 4, a width outside {64, 128, 256}, K % 4 != 0, an ldout
    that does not hold the packed output and extra columns inside the R main ones are SEMICRF_EINVAL, with the message that names the
    rule.  Nothing is launched: the pointers here are host addresses that are never dereferenced."""
    buf = np.zeros(1 << 16, dtype=np.uint8)
    base = (buf.ctypes.data + 255) // 256 * 256
    a, b, o, w = base + chg.get("Aphase", chg.get("dyphase", 0)), base + 4096, base + 8192, base + 16384
    M, K, N = REJ_M, chg.get("Kcall", REJ_K), chg.get("Ncall", REJ_N)
    if entry == "tn":
        rc = L.scorer_proj_tn(a, chg.get("lddy", REJ_K + 4), M, REJ_K, chg.get("extra_col0", REJ_K), REJ_K + 4, b, N + 4, N, o, N + 4, w,
                              None, 0, None)
    else:
        args = (a, chg.get("lda", REJ_K + 4), M, K, b, N + 4, N, o, chg.get("ldout", N + 8), w, w + 1024, w + 2048, 2, 0)
        rc = L.scorer_proj_nn(*args, None) if entry == "nn" else L.scorer_proj_nn3(*args, base + 32768, 1 << 14, None)
    assert rc == EINVAL and msg in _err(), (rc, _err())
    assert not buf.any()


@pytest.mark.gpu
@pytest.mark.parametrize("name,entry,chg,msg", PROJ_REJECTED, ids=[r[0] for r in PROJ_REJECTED])
def test_projection_rejections_device(gpu, name, entry, chg, msg):
    """The same calls on device memory: SEMICRF_EINVAL, and every output keeps the pattern."""
    guard = sc.guard_bytes(widest_row_floats=REJ_K + 8)
    if entry == "tn":
        case = _tn_case(REJ_M, REJ_K, REJ_N, gpu, True, refused=True, **chg)
    else:
        case = _nn_case(REJ_M, REJ_K, REJ_N, gpu, "forward_packed", entry=entry, refused=True, **chg)
    sc.contract(case, gpu, guard, name, rc=EINVAL)
    assert msg in _err()


# =================================================================================================================================================
# G.  What the bounds are worth (no device)
# =================================================================================================================================================
def _distinct(rows):
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


FWD_SHAPES = _distinct([(f.C, f.T, f.D, bool(f.rowc), f.prec) for f in FWD])


@pytest.mark.parametrize("C,T,D,rowc,prec", FWD_SHAPES, ids=[f"{c}x{t}x{d}{'_rowc' if r else ''}{'_bf16x3' if p else ''}" for c, t, d, r, p in FWD_SHAPES])
def test_forward_bound_admits_plain_float32(C, T, D, rowc, prec):
    """The forward bound admits a plain float32 numpy evaluation of the formula, accumulated sequentially over d (through the six limb
    products of three bf16 limbs for the three-limb rows), at every shape of the table: no element is exempt.  All three scalings
    where the square is small, one (rotating with the shape) above 2^20 cells."""
    q, k, dg, rc = (x.numpy() for x in _fwd_data(C, T, D))
    modes = (0, 1, 2) if C * T * T <= (1 << 20) and not prec else ((C + T) % 3,)
    for mode in modes:
        ref, bound = sc.fwd_ref(q, k, dg, rc if rowc else None, sc.qscale_of(D), mode, prec)
        got = sc.fwd_f32(q, k, dg, rc if rowc else None, sc.qscale_of(D), mode, nlimbs=3 if prec else 0)
        sc.assert_within("S", got, ref, bound, f"float32 forward {C}x{T}x{D} scaling {mode}")


BWD_SHAPES = [(5, 1, 32), (5, 2, 96), (8, 33, 160), (5, 63, 256), (5, 70, 64), (1, 64, 64), (5, 65, 128), (9, 129, 64), (9, 257, 256), (10, 129, 64)]


@pytest.mark.parametrize("C,T,D", BWD_SHAPES)
def test_backward_bound_admits_plain_float32(C, T, D):
    """The backward bounds admit plain float32 numpy sums in index order, in every element of dq, dk and drowc."""
    q, k, _, _ = (x.numpy() for x in _fwd_data(C, T, D))
    dS = _cotangent(T, C).numpy()
    for mode in ((0, 1, 2) if T <= 70 else ((C + T) % 3,)):
        ref, bound = sc.bwd_ref(dS, q, k, sc.qscale_of(D), mode)
        got = sc.bwd_f32(dS, q, k, sc.qscale_of(D), mode)
        got["drowc"] = got["drowc"]
        for n in ("dq", "dk", "drowc"):
            sc.assert_within(n, got[n], ref[n], bound[n], f"float32 backward {C}x{T}x{D} scaling {mode}")


@pytest.mark.parametrize("K,N", NN_PAIRS)
def test_proj_nn_bound_admits_plain_float32(K, N):
    A, B, bias, w2, b2, old = (x.numpy() for x in _nn_data(129, K, N))
    for use_bias, acc in ((True, False), (False, True), (False, False)):
        main, bound, _, ex, exb = sc.nn_ref(A, B[:K], bias if use_bias else None, w2, b2, old[:, :N] if acc else None)
        sc.assert_within("out", sc.nn_f32(A, B[:K], bias if use_bias else None, old[:, :N] if acc else None), main, bound, f"float32 proj_nn K={K} N={N}")
        sc.assert_within("extras", sc.nn_f32(A, np.ascontiguousarray(w2.T), b2), ex, exb, f"float32 proj_nn extras K={K}")
    if N == 256:
        main, bound, amain, _, _ = sc.nn_ref(A, B[:K], bias, None, None)
        sc.assert_within("out", sc.nn_f32(A, B[:K], bias, nlimbs=3), main, bound + 2.0 ** -21 * amain, f"float32 three-limb proj_nn K={K}")


@pytest.mark.parametrize("R,N", TN_PAIRS)
def test_proj_tn_bound_admits_plain_float32(R, N):
    for M in TN_M:
        dy, x = (t.numpy() for t in _tn_data(M, R, N))
        dW, bW, _, db, bb = sc.tn_ref(dy, x)
        gW, gb = sc.tn_f32(dy, x)
        sc.assert_within("dW", gW, dW, bW, f"float32 proj_tn M={M} R={R} N={N}")
        sc.assert_within("db", gb, db, bb, f"float32 proj_tn M={M} R={R} N={N}")


@pytest.mark.parametrize("size,D", MERGE_SHAPES)
def test_merge_bound_admits_plain_float32(size, D):
    W, bias = (x.numpy() for x in _linear(size, D))
    Wm64, bW, bm64, bb = sc.merge_fwd_ref(W, bias, D, size)
    Wk1 = np.concatenate([W[D:2 * D], bias[D:2 * D, None]], axis=1)
    Wm = np.concatenate([sc.nn_f32(np.ascontiguousarray(Wk1.T), W[:D], None), W[2 * D:]])
    bm = np.concatenate([sc.nn_f32(np.ascontiguousarray(Wk1.T), bias[:D, None], None)[:, 0], bias[2 * D:]])
    sc.assert_within("Wm", Wm, Wm64, bW, f"float32 merged weights size={size} D={D}")
    sc.assert_within("bm", bm, bm64, bb, f"float32 merged weights size={size} D={D}")


def _violates(name, got, ref, bound, what, mask=None):
    with pytest.raises(AssertionError, match="outside its bound"):
        sc.assert_within(name, got, ref, bound, what, mask=mask, quiet=True)


@pytest.mark.parametrize("C,T,D,mode", [(5, 70, 64, 0), (6, 40, 128, 1), (5, 33, 48, 0)])
def test_yardstick_forward(C, T, D, mode):
    """What the forward bound is worth: a correct float32 result passes; the same result without the last contraction term, with the
    cells e == b + 1 scaled by len(2) / len(1), or with the last row taken from the row before, does not."""
    q, k, dg, _ = (x.numpy() for x in _fwd_data(C, T, D))
    qs = sc.qscale_of(D)
    ref, bound = sc.fwd_ref(q, k, dg, None, qs, mode)
    good = sc.fwd_f32(q, k, dg, None, qs, mode)
    sc.assert_within("S", good, ref, bound, "as it is")
    _violates("S", sc.fwd_f32(q, k, dg, None, qs, mode, drop_last=True), ref, bound, "last term dropped")
    wrong = good.copy()
    i = np.arange(T - 1)
    wrong[i + 1, i] *= np.float32(sc.len64(mode, 2) / sc.len64(mode, 1))
    _violates("S", wrong, ref, bound, "e == b + 1 scaled as length 2")
    wrong = good.copy()
    wrong[T - 1] = good[T - 2]
    _violates("S", wrong, ref, bound, "tail row from the row before")
    # the violations are not confined to a few cells: without the last term most of the lower triangle is outside
    err = np.abs(sc.fwd_f32(q, k, dg, None, qs, mode, drop_last=True).astype(np.float64) - ref)
    lower = np.tril(np.ones((T, T), dtype=bool), -1)[:, :, None]
    assert (err > bound)[np.broadcast_to(lower, err.shape)].mean() > 0.9


def test_yardstick_three_limbs():
    """What the three-limb bound is worth.  Two limbs an operand miss the third by up to 2^-17 of the value: 2^-16 sum |q k| when every
    product errs the same way.  The three-limb bound at D = 64 is (2^-21 + 72 u) sum |q k| = 2^-17.7 sum |q k|, so operands whose third
    limb is as large as it gets (x = 0x1.00f28p+0: limbs 1, 2^-8 - ..., 2^-17) show the dropped limb; at D = 256 the fp32 accumulation
    term alone is 2^-15.9 sum |q k| and the bound cannot see it -- nor can it on hash_normal operands, whose limb errors cancel."""
    C, T, D = 2, 8, 64
    x = np.float32(float.fromhex("0x1.00f28p+0"))
    l = sc.limbs(np.array([x]))
    assert float(l[2][0]) / float(x) > 2.0 ** -17.01
    q = np.full((C, T, D), x, dtype=np.float32)
    dg = np.zeros((C, T), dtype=np.float32)
    qs = sc.qscale_of(D)
    ref, bound = sc.fwd_ref(q, q, dg, None, qs, 2, prec=1)
    sc.assert_within("S", sc.fwd_f32(q, q, dg, None, qs, 2, nlimbs=3), ref, bound, "three limbs")
    _violates("S", sc.fwd_f32(q, q, dg, None, qs, 2, nlimbs=2), ref, bound, "third limb dropped")
    A, B = np.full((4, D), x, dtype=np.float32), np.full((D, 256), x, dtype=np.float32)
    main, nb, amain, _, _ = sc.nn_ref(A, B, None, None, None)
    sc.assert_within("out", sc.nn_f32(A, B, None, nlimbs=3), main, nb + 2.0 ** -21 * amain, "three limbs, proj_nn3")
    _violates("out", sc.nn_f32(A, B, None, nlimbs=2), main, nb + 2.0 ** -21 * amain, "third limb dropped, proj_nn3")


def test_yardstick_backward_and_projection():
    """The same for the backward and the GEMMs: a term left out of the contraction, or a tail row taken from the row before, is outside
    the bound that the correct float32 result meets."""
    C, T, D, mode = 5, 70, 64, 0
    q, k, _, _ = (x.numpy() for x in _fwd_data(C, T, D))
    dS = _cotangent(T, C).numpy()
    qs = sc.qscale_of(D)
    ref, bound = sc.bwd_ref(dS, q, k, qs, mode)
    good = sc.bwd_f32(dS, q, k, qs, mode)
    for n in ("dq", "dk", "drowc"):
        sc.assert_within(n, good[n], ref[n], bound[n], "as it is")
    bad = sc.bwd_f32(dS, q, k, qs, mode, skip_dq_term=1, skip_dk_last=True)          # (linear scaling: the term b == e is zero anyway)
    _violates("dq", bad["dq"], ref["dq"], bound["dq"], "dq without the term b = e - 1")
    _violates("dk", bad["dk"], ref["dk"], bound["dk"], "dk without the term e = T - 1")
    for n in ("dq", "dk"):
        wrong = good[n].copy()
        wrong[:, T - 1] = good[n][:, T - 2]
        _violates(n, wrong, ref[n], bound[n], "tail row from the row before")
    M, K, N = 129, 260, 64
    A, B, bias, _, _, _ = (x.numpy() for x in _nn_data(M, K, N))
    main, nb, _, _, _ = sc.nn_ref(A, B[:K], bias, None, None)
    good = sc.nn_f32(A, B[:K], bias)
    sc.assert_within("out", good, main, nb, "as it is")
    _violates("out", sc.nn_f32(A, B[:K], bias, drop_last=True), main, nb, "proj_nn without the term k = K - 1")
    wrong = good.copy()
    wrong[M - 1] = good[M - 2]
    _violates("out", wrong, main, nb, "proj_nn tail row from the row before")
    M, R, N = 257, 64, 64
    dy, x = (t.numpy() for t in _tn_data(M, R, N))
    dW, bW, _, db, bb = sc.tn_ref(dy, x)
    gW, gb = sc.tn_f32(dy, x)
    sc.assert_within("dW", gW, dW, bW, "as it is")
    wW, wb = sc.tn_f32(dy, x, drop_last=True)
    _violates("dW", wW, dW, bW, "proj_tn without the row m = M - 1")
    _violates("db", wb, db, bb, "proj_tn bias gradient without the row m = M - 1")
    wrong = gW.copy()
    wrong[R + 1] = gW[R]
    _violates("dW", wrong, dW, bW, "proj_tn second extra row from the first")
