"""Guard-band arena for the memory-contract tests (tests/test_memory_contract.py, tests/test_step_contract.py).

One int32 tensor per case, filled with a 32-bit word pattern; every operand, output and workspace of the case is a contiguous view
("carve") into it, at a chosen address phase modulo 16, with guards of at least max(4 KiB, one [T][B] row plane) on either side.
A stray access therefore stays inside ONE mapped allocation: an overrun is a failed assertion, never a fault.

    NAN_PATTERN  0x7FC5A5A5   a quiet NaN as float32, an out-of-range index (2143659429) as int32
    MAX_PATTERN  0x7F7FFFFF   FLT_MAX as float32: finite, so a stray read changes a result without poisoning it

Three allocators share one interface -- carve(name, shape, dtype, phase, align), put(name, tensor, phase), call(fn):
    Sizer   adds up what a case needs (carves are meta tensors, call() does nothing): a case is written once and sized by a dry run
    Arena   the real thing
    Plain   ordinary tensors from torch's allocator, outputs pre-filled with the same pattern: the reference run of a case
"""
import numpy as np
import torch

NAN_PATTERN = 0x7FC5A5A5
MAX_PATTERN = 0x7F7FFFFF
PATTERNS = {"nan": NAN_PATTERN, "max": MAX_PATTERN}

# float64 / int64 carves (tests/test_step_contract.py) are 8-byte items: their phases modulo 16 are 0 and 8, each element holds the
# word pattern twice
_ITEM = {torch.float32: 4, torch.int32: 4, torch.uint8: 1, torch.float64: 8, torch.int64: 8}


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def pattern_bytes(pattern: int) -> np.ndarray:
    return np.frombuffer(np.array([pattern], dtype="<u4").tobytes(), dtype=np.uint8)


def fill_pattern_(t: torch.Tensor, pattern: int) -> torch.Tensor:
    """Fill a float32 / int32 (or float64 / int64: two words an element) tensor with the word pattern, bit for bit."""
    t.view(torch.int32).fill_(int(np.array([pattern], dtype=np.uint32).view(np.int32)[0]))
    return t


def bits(t: torch.Tensor) -> torch.Tensor:
    """A tensor's bits as int32 (uint8 stays; an 8-byte element gives two words, so the last dimension doubles), for comparisons
    that must not treat NaN != NaN or -0 == +0."""
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


class GuardError(AssertionError):
    pass


class Sizer:
    """Dry run: the bytes an Arena needs for the same sequence of carves."""
    real = False

    def __init__(self, guard_bytes: int):
        self.guard = _guard(guard_bytes)
        self.bytes = self.guard

    def carve(self, name, shape, dtype, phase=0, align=16):
        n = _numel(shape) * _ITEM[dtype]
        self.bytes += align + phase + (n + 3) // 4 * 4 + self.guard      # the worst padding, the carve, the guard behind it
        return torch.empty(shape, dtype=dtype, device="meta")

    def put(self, name, src, phase=0, align=16):
        return self.carve(name, tuple(src.shape), src.dtype, phase, align)

    def call(self, fn):
        return None


def _guard(guard_bytes: int) -> int:
    return (max(4096, int(guard_bytes)) + 255) // 256 * 256


class Arena:
    real = True

    def __init__(self, nbytes: int, guard_bytes: int, pattern: int, device):
        self.pattern = pattern
        self.guard = _guard(guard_bytes)
        self.device = torch.device(device)
        self.words = torch.empty((int(nbytes) + 3) // 4 + 64, dtype=torch.int32, device=self.device)
        fill_pattern_(self.words, pattern)
        self.u8 = self.words.view(torch.uint8)
        self.base = self.words.data_ptr()
        self.cursor = self.guard                 # byte offset of the first byte that may be handed out
        self.carves = []                         # (name, byte offset, bytes, tensor, source bits or None)
        self._pat = torch.from_numpy(pattern_bytes(pattern).copy()).to(self.device)

    def carve(self, name, shape, dtype, phase=0, align=16):
        """A contiguous view whose data_ptr() % align == phase, a guard away from the previous carve; it holds the pattern."""
        assert 0 <= phase < align and phase % _ITEM[dtype] == 0
        n = _numel(shape) * _ITEM[dtype]
        off = self.cursor
        off += (phase - (self.base + off)) % align
        assert off + n + self.guard <= self.u8.numel(), "arena too small (the Sizer run and the real run must carve alike)"
        t = self.u8[off:off + n]
        t = (t if dtype == torch.uint8 else t.view(dtype)).view(shape)
        assert t.is_contiguous() and (n == 0 or t.data_ptr() == self.base + off) and (self.base + off) % align == phase
        self.carves.append([name, off, n, t, None])
        self.cursor = off + n + self.guard
        return t

    def put(self, name, src, phase=0, align=16):
        """An operand: a carve holding a copy of `src`; check() also finds it unchanged afterwards."""
        t = self.carve(name, tuple(src.shape), src.dtype, phase, align)
        t.copy_(src)
        self.carves[-1][4] = bits(t).clone()
        return t

    def call(self, fn):
        return fn()

    def _expected(self, a, b):
        """The pattern bytes of the byte range [a, b)."""
        return self._pat.repeat((b - a) // 4 + 2)[a % 4:a % 4 + (b - a)]

    def check(self):
        """Every guard byte holds the pattern and every operand its bits.  Raises GuardError naming the first offset and the
        carve(s) the damaged guard borders."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        edges = [(None, 0, 0)] + [(c[0], c[1], c[2]) for c in self.carves] + [(None, self.u8.numel(), 0)]
        for (ln, lo, ls), (rn, ro, _) in zip(edges[:-1], edges[1:]):
            a, b = lo + ls, ro
            got = self.u8[a:b]
            bad = got != self._expected(a, b)
            if bool(bad.any()):
                i = int(torch.nonzero(bad)[0])
                raise GuardError(f"guard damaged at arena byte {a + i}: {i} bytes past the end of `{ln}`, {b - a - i} bytes before "
                                 f"the start of `{rn}` (byte {int(got[i]):#04x}, pattern {self.pattern:#010x})")
        for name, off, n, t, src in self.carves:
            if src is not None and not torch.equal(bits(t), src):
                i = int(torch.nonzero(bits(t).reshape(-1) != src.reshape(-1))[0])
                raise GuardError(f"operand `{name}` was written: element {i} changed")


class Plain:
    """The same interface on ordinary tensors: outputs come pre-filled with the pattern, operands are fresh copies."""
    real = True

    def __init__(self, pattern: int, device):
        self.pattern = pattern
        self.device = torch.device(device)

    def carve(self, name, shape, dtype, phase=0, align=16):
        t = torch.empty(shape, dtype=dtype, device=self.device)
        if dtype == torch.uint8:
            n = t.numel()
            if n:
                t.copy_(torch.from_numpy(np.resize(pattern_bytes(self.pattern), n).copy()).to(self.device).view(shape))
            return t
        return fill_pattern_(t, self.pattern)

    def put(self, name, src, phase=0, align=16):
        return src.to(self.device).clone()

    def call(self, fn):
        return fn()

    def check(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)


def run_in_arena(case, guard_bytes: int, pattern: int, device):
    """case(A) carves, calls and returns its outputs.  Sized by a dry run, then run in an arena of exactly that size (+ slack)."""
    s = Sizer(guard_bytes)
    case(s)
    a = Arena(s.bytes, guard_bytes, pattern, device)
    out = case(a)
    return a, out
