"""Shared by tests/test_mbr_decode.py and tests/test_limits.py: the numpy-float32 restatement of semicrf_mbr_select and a
deterministic generator of packed lattices for rows far longer than a [T, T, B] tensor allows.

Everything here is a function of its arguments; nothing is read from a fixture or from a global random generator."""
import numpy as np

from transkun_amd import synth


def _mbr_reference(pairs, offsets, weight, T, tau):
    """semicrf_mbr_select as the header states it, in numpy float32 (np.float32 + np.float32 is one fp32 add)."""
    B = len(offsets) - 1
    zero = np.float32(0.0)
    sel, off, gain = [], [0], np.zeros(B, np.float32)
    for c in range(B):
        lo, hi = int(offsets[c]), int(offsets[c + 1])
        th = np.float32(tau[c])
        w, b, e = weight[lo:hi], pairs[lo:hi, 0], pairs[lo:hi, 1]
        with np.errstate(invalid="ignore"):
            elig = w > th                                     # strict; NaN is never eligible
        g = w - th
        assert g.dtype == np.float32
        single, begins = {}, {}
        for i in np.nonzero(elig)[0]:
            if b[i] == e[i]:
                single.setdefault(int(b[i]), int(i))
            else:
                begins.setdefault(int(b[i]), []).append(int(i))          # the lattice is ascending by (begin, end)
        gS = lambda t: g[single[t]] if t in single else zero
        F = np.zeros(T, np.float32)
        choice = [-1] * T
        F[T - 1] = gS(T - 1)
        for t in range(T - 2, -1, -1):
            best, ch = F[t + 1], -1
            for i in begins.get(t, ()):
                cv = g[i] + F[e[i]]
                if cv > best:
                    best, ch = cv, i
            F[t] = best + gS(t)
            choice[t] = ch
        assert F.dtype == np.float32
        t = 0
        while True:
            if t in single:
                sel.append(lo + single[t])
            if t == T - 1:
                break
            if choice[t] < 0:
                t += 1
            else:
                sel.append(lo + choice[t])
                t = int(e[choice[t]])
        off.append(len(sel))
        gain[c] = F[0]
    sel = np.asarray(sel, np.int64)
    return pairs[sel].reshape(-1, 2), np.asarray(off, np.int32), weight[sel], gain


# ---- synthetic lattices ----------------------------------------------------------------------------------------------------

LATTICE_CHAINS = ("empty", "dense", "hashed", "last_frame")
_LONG_EVERY = 512                                             # one long interval per ~512 frames of a hashed chain


def _unit(h, shift):
    """24 bits of the hash as a float32 in (0, 1]: k / 2**24, k = 1 .. 2**24 (exact in fp32)."""
    return (((h >> np.uint64(shift)) & np.uint64(0xFFFFFF)).astype(np.int64) + 1).astype(np.float32) * np.float32(2.0 ** -24)


def _hashed_chain(T, seed, last_frame):
    """Per frame t a singleton with probability 1/2 and 0..2 intervals of length 1..64 (ends clipped to T - 1, equal ends kept
    once), weights uniform in (0, 1].  In addition a long interval of length 65 .. T/2 and weight in (0.5, 1] begins at about one
    frame in 512.  A long interval loses against the ~0.1 of gain per frame that skipping collects at tau = 0.3 unless the frames
    under it are empty, so some of them get a HOLE -- no entry begins strictly inside -- and are then certain to be selected:
    those of length <= T/16 whose hash says so, and one of length T/2 that begins at T/3 with weight 1.  The walk then jumps over
    thousands of frames: across many 64-entry pieces of the recursion and many per-thread runs of the parallel trace.
    last_frame: an eligible singleton (weight 0.95) is forced at T - 1 and none is left at frame 0."""
    t = np.arange(T, dtype=np.uint64)
    h0 = synth.hash_u64_numpy(t, seed)                        # singleton yes / no, its weight, the number of short intervals
    h1 = synth.hash_u64_numpy(t, seed + 1)                    # the short intervals' lengths and weights
    h2 = synth.hash_u64_numpy(t, seed + 2)                    # the long intervals
    one = np.uint64(1)
    has_single = (h0 & one) == one
    w_single = _unit(h0, 8)
    n_short = ((h0 >> np.uint64(1)) % np.uint64(3)).astype(np.int64)
    len_a = ((h1 & np.uint64(63)).astype(np.int64)) + 1
    len_b = (((h1 >> np.uint64(6)) & np.uint64(63)).astype(np.int64)) + 1
    w_a, w_b = _unit(h1, 12), _unit(h1, 36)
    is_long = (h2 % np.uint64(_LONG_EVERY)) == np.uint64(7)
    half = max(T // 2, 66)
    len_long = 65 + ((h2 >> np.uint64(12)) % np.uint64(half - 64)).astype(np.int64)
    w_long = np.float32(0.5) + np.float32(0.5) * _unit(h2, 36)
    wants_hole = ((h2 >> np.uint64(9)) & one) == one
    big = T // 3                                              # the one jump of T/2 frames
    hole = np.zeros(T, bool)                                  # frames at which nothing may begin
    longs = {}
    for f in np.nonzero(is_long)[0]:
        f = int(f)
        e = min(f + int(len_long[f]), T - 1)
        if e > f:
            longs[f] = (e, w_long[f])
            if wants_hole[f] and e - f <= T // 16:
                hole[f + 1:e] = True
    if big + T // 2 <= T - 1 and T // 2 > 64:
        longs[big] = (big + T // 2, np.float32(1.0))
        hole[big + 1:big + T // 2] = True
    rows, ws = [], []
    for f in range(T):
        if hole[f]:
            continue
        if has_single[f] and not (last_frame and f == 0):
            if not (last_frame and f == T - 1):
                rows.append((f, f)); ws.append(w_single[f])
        if last_frame and f == T - 1:
            rows.append((f, f)); ws.append(np.float32(0.95))
        cand = {}
        for k, (ln, w) in enumerate(((len_a[f], w_a[f]), (len_b[f], w_b[f]))):
            if k < n_short[f]:
                cand.setdefault(min(f + int(ln), T - 1), w)
        if f in longs:
            cand[longs[f][0]] = longs[f][1]                    # (replaces a short interval with the same end)
        for e in sorted(cand):
            if e > f:
                rows.append((f, e)); ws.append(cand[e])
    return rows, ws


def lattice(T, seed):
    """(pairs int32 [K, 2], weight float32 [K], offsets int32 [B + 1]) for B = 4 chains (LATTICE_CHAINS), ascending by (begin, end)
    per chain, weights in (0, 1]:
      empty       no entries: the walk is T - 1 skips, the longest dependent chain, and nothing is emitted;
      dense       every frame holds (t, t) with weight 0.9 and (t, t + 1) with 0.8: the selected path has 2 T - 1 cells, the
                  capacity of the trace's region and of pairs_out;
      hashed      _hashed_chain: jumps of every length up to T/2;
      last_frame  the same from another seed, with an eligible singleton at T - 1 (the terminal frame emits it without having
                  been marked) and none at frame 0."""
    chains = [([], [])]
    rows, ws = [], []
    for t in range(T):
        rows.append((t, t)); ws.append(np.float32(0.9))
        if t < T - 1:
            rows.append((t, t + 1)); ws.append(np.float32(0.8))
    chains.append((rows, ws))
    chains.append(_hashed_chain(T, 1000 * seed + 11, False))
    chains.append(_hashed_chain(T, 1000 * seed + 57, True))
    pairs = np.asarray([p for r, _ in chains for p in r], np.int32).reshape(-1, 2)
    weight = np.asarray([w for _, wl in chains for w in wl], np.float32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r, _ in chains])]).astype(np.int32)
    return pairs, weight, offsets
