"""Audio front-end of the reference model: framing, the six-window spectrum and the log-mel features that feed
the backbone (/root/reference/transkun/Util.py:21-170, ModelTransformer.py:159-164).

Two routes.  "torch", the default, is the reference's own sequence of stock ops: the frames times the windows, rFFT, |.|^2, the channel
mean, a [2049 x 229] matmul, log.  "fused" (`MelSpectrum.route = "fused"`, `log_mel(..., route="fused")`, `segment_features`) is ONE
op, `torch.ops.semicrf.log_mel` (csrc/logmel.hip on a GPU, its host mirror on the CPU): gain, windows, a real transform per window in
LDS, power, channel mean, the mel bands from the filterbank's non-zero ranges (`compact_filterbank`) and the log compression; the
overlapping frame view is read in place and neither the windowed frames nor a spectrum are ever written.  The fused route is forward
only and fp32: with gradients wanted (the Gaussian windows are Parameters, so whenever grad mode is on), another dtype, a shape outside
the op's supported set or a sample stride other than 1 the call runs the stock expression.  `FRONTEND_ROUTES` counts which way the calls
went.  The module keeps the reference's parameter names (`spectrogramExtractor.win`, `spectrogramExtractor.winGen.sigma|center`,
`freq2mels`), so a caller who replaces the reference end to end finds the same pieces.

Parity: framing, the Gaussian windows and the spectrum are pinned against the reference's own classes (importable in the
build container; tests/golden/frontend.npz).  The mel filterbank is PARITY UNPINNED: the reference takes it from
torchaudio.functional.melscale_fbanks (Util.py:134-141), which is not installed here; `melscale_fbanks` below restates
torchaudio's documented definition (HTK mel scale, triangular filters, no area normalisation) and is checked for its
structural properties only.
"""
from __future__ import annotations

import math
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

FRONTEND_ROUTE_KINDS = ("fused", "torch")
DEFAULT_FRONTEND_ROUTE = "torch"
# calls of log_mel (and so of the MelSpectrum modules set to "fused") by the way they went; tests read it
FRONTEND_ROUTES = {"fused": 0, "torch": 0}


def makeFrame(x: torch.Tensor, hopSize: int, windowSize: int, leftPaddingHalfFrame: bool = True) -> torch.Tensor:
    """[..., nSample] -> [..., nFrame, windowSize] with nFrame = ceil(nSample / hop) + 1 (Util.py:21-43): frame t is centred
    on sample t * hop when the signal is padded by half a window on the left."""
    assert hopSize < windowSize
    n = x.shape[-1]
    nFrame = math.ceil(n / hopSize) + 1
    left = windowSize // 2 if leftPaddingHalfFrame else 0
    covered = (nFrame - 1) * hopSize + windowSize            # samples the nFrame windows span
    right = covered - left - n
    frames = F.pad(x, (left, right)).unfold(-1, windowSize, hopSize)
    assert frames.shape[-2] == nFrame, (frames.shape[-2], nFrame)
    return frames


class GaussianWindows(nn.Module):
    """n learnable Gaussian analysis windows of length nWin (Util.py:47-71): centre and width are sigmoids of free parameters,
    initialised to evenly spaced centres and a common width."""

    def __init__(self, n: int, nWin: int):
        super().__init__()
        self.n, self.nWin = n, nWin
        self.sigma = nn.Parameter(torch.full((n,), -1.0))
        self.center = nn.Parameter(torch.logit(torch.arange(1, n + 1) / (n + 1)))

    def get(self) -> torch.Tensor:
        width = torch.sigmoid(self.sigma) * self.nWin / 2
        mid = torch.sigmoid(self.center) * self.nWin
        t = torch.arange(self.nWin, device=self.sigma.device).unsqueeze(1)
        return torch.exp(-0.5 * ((t - mid) / width) ** 2)               # [nWin, n]


class Spectrum(nn.Module):
    """Orthonormal rFFT of every frame under a Hann window and nExtraWins Gaussian windows (Util.py:78-124):
    [..., nFrame, windowSize] -> complex [..., nFrame, windowSize//2+1, 1+nExtraWins]."""

    def __init__(self, windowSize: int, nExtraWins: int = 0, log: bool = False):
        super().__init__()
        self.outputDim = windowSize // 2 + 1
        self.nChannel = nExtraWins + 1
        self.log = log
        self.nExtraWins = nExtraWins
        self.register_buffer("win", torch.hann_window(windowSize))
        if nExtraWins > 0:
            self.winGen = GaussianWindows(nExtraWins, windowSize)

    def windows(self) -> torch.Tensor:
        wins = self.win.unsqueeze(0)
        if self.nExtraWins > 0:
            wins = torch.cat([wins, self.winGen.get().t()], dim=0)
        return wins                                                          # [1+nExtraWins, windowSize]

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        spec = torch.fft.rfft(frames.unsqueeze(-2) * self.windows(), norm="ortho")
        if self.log:
            spec = torch.complex(spec.abs(), spec.angle())
        return spec.transpose(-1, -2)


def _hz_to_mel_htk(f):
    return 2595.0 * math.log10(1.0 + f / 700.0)


def melscale_fbanks(n_freqs: int, f_min: float, f_max: float, n_mels: int, sample_rate: int) -> torch.Tensor:
    """[n_freqs, n_mels] triangular filterbank: n_mels + 2 points equally spaced on the HTK mel scale between f_min and
    f_max; filter m rises from point m to point m+1 and falls to point m+2; linear frequency bins 0 .. sample_rate/2; no
    area normalisation (torchaudio.functional.melscale_fbanks with its defaults -- restated, parity unpinned)."""
    freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_mel_htk(f_min), _hz_to_mel_htk(f_max), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]                                          # [n_mels + 1]
    slopes = f_pts.unsqueeze(0) - freqs.unsqueeze(1)                         # [n_freqs, n_mels + 2]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return torch.clamp(torch.minimum(down, up), min=0.0)


class MelSpectrum(nn.Module):
    """Power spectrum of every window -> mel bands -> optional log compression mapped to [0, 1] (Util.py:126-170):
    [..., nFrame, windowSize] -> [..., nFrame, n_mels, 1+nExtraWins].

    route: "torch" (the default: the stock ops below as they stand) or "fused": `log_mel`'s one op wherever it applies (float32, a
    supported shape, sample stride 1, no gradient wanted), the stock expression in every other case."""

    def __init__(self, windowSize, f_min, f_max, n_mels, fs, nExtraWins=0, log=False, eps=1e-5, toMono=False):
        super().__init__()
        self.outputDim = n_mels
        self.nChannel = nExtraWins + 1
        self.register_buffer("freq2mels", melscale_fbanks(windowSize // 2 + 1, f_min, f_max, n_mels, fs))
        self.log, self.eps, self.toMono = log, eps, toMono
        self.spectrogramExtractor = Spectrum(windowSize, nExtraWins)
        self.route = DEFAULT_FRONTEND_ROUTE

    def forward(self, frames: torch.Tensor) -> torch.Tensor:
        if self.route != DEFAULT_FRONTEND_ROUTE:                             # left at "torch" it touches nothing, the counters included
            return log_mel(frames, self.spectrogramExtractor.windows(), self.freq2mels, log=self.log, eps=self.eps, toMono=self.toMono,
                           route=self.route)
        power = self.spectrogramExtractor(frames).abs().pow(2)              # [..., nFrame, nFreq, nWin]
        if self.toMono and power.dim() >= 4:
            power = power.mean(dim=-4, keepdim=True)                         # over the audio channels
        mel = (power.transpose(-1, -2) @ self.freq2mels).transpose(-1, -2)
        if self.log:
            mel = ((mel + self.eps).log() - math.log(self.eps)) / (-math.log(self.eps))
        return mel


def normalize_gain(framesBatch: torch.Tensor) -> torch.Tensor:
    """Per-recording gain normalisation in front of the feature extractor (ModelTransformer.py:159-161)."""
    mean = torch.mean(framesBatch, dim=[1, 2, 3], keepdim=True)
    std = torch.std(framesBatch, dim=[1, 2, 3], keepdim=True)
    return (framesBatch - mean) / (std + 1e-8)


# ---- the fused route ------------------------------------------------------------------------------------------------------------------
_FILTERBANKS = {}                # (device, data_ptr) -> ((_version, shape, dtype), compact form, weak reference to the tensor)
_TWIDDLES = {}                   # (W, device) -> [W / 2, 2] float32
_CACHE_LIMIT = 16


def log_mel_torch(frames, windows, freq2mels, log=True, eps=1e-5, toMono=False):
    """The stock route: MelSpectrum.forward's expression on windows [nWin, W] and a filterbank [W / 2 + 1, nMel], op for op."""
    spec = torch.fft.rfft(frames.unsqueeze(-2) * windows, norm="ortho").transpose(-1, -2)
    power = spec.abs().pow(2)                                               # [..., nFrame, nFreq, nWin]
    if toMono and power.dim() >= 4:
        power = power.mean(dim=-4, keepdim=True)                             # over the audio channels
    mel = (power.transpose(-1, -2) @ freq2mels).transpose(-1, -2)
    if log:
        mel = ((mel + eps).log() - math.log(eps)) / (-math.log(eps))
    return mel


def _capturing(device) -> bool:
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


def _compact(fb: torch.Tensor):
    """The compact form of a dense [nFreq, nMel] matrix, built on the host: per column the first and the last non-zero row and the
    values between them (zeros inside the range included)."""
    dense = fb.detach().to("cpu")
    nz = dense != 0                                                         # a NaN weight counts as non-zero
    rows = torch.arange(dense.shape[0]).unsqueeze(1)
    has = nz.any(dim=0)
    first = torch.where(nz, rows, dense.shape[0]).amin(dim=0)
    last = torch.where(nz, rows, -1).amax(dim=0)
    start = torch.where(has, first, 0).to(torch.int32)
    length = torch.where(has, last - first + 1, 0).to(torch.int32)
    offset = (torch.cumsum(length, 0) - length).to(torch.int32)
    pieces = [dense[int(s):int(s) + int(n), m] for m, (s, n) in enumerate(zip(start.tolist(), length.tolist()))]
    values = torch.cat(pieces) if pieces else dense.new_zeros(0)
    max_len = int(length.max()) if length.numel() else 0
    total = int(values.numel())
    if total == 0:
        values = dense.new_zeros(1)                                         # never read: a pointer the op may check
    dev = fb.device
    return start.to(dev), length.to(dev), offset.to(dev), values.contiguous().to(dev), max_len, total


def compact_filterbank(freq2mels: torch.Tensor):
    """(start, length, offset, values, max_len, total) of a [W / 2 + 1, nMel] filterbank: band m weighs the `length[m]` rows from
    `start[m]` with `values[offset[m] : offset[m] + length[m]]` (its first to its last non-zero row; a column of zeros has length 0);
    max_len is the longest range, total the sum of all.  start / length / offset are int32 tensors and values has the matrix' dtype,
    all on its device.  Computed once per buffer -- one host synchronisation at first use -- and cached by (device, data_ptr,
    _version) for as long as that tensor lives: load_state_dict and in-place writes bump the version, .to() makes a new buffer, and a
    temporary is never taken for the one whose address it inherits.  Inside a graph capture a matrix that is
    not cached yet is an error, never a silent synchronisation."""
    assert freq2mels.dim() == 2
    key = (str(freq2mels.device), freq2mels.data_ptr())
    tag = (freq2mels._version, tuple(freq2mels.shape), freq2mels.dtype)
    hit = _FILTERBANKS.get(key)
    if hit is not None and hit[0] == tag and hit[2]() is freq2mels:       # the tensor itself: a freed one's address is handed out again
        return hit[1]
    if _capturing(freq2mels.device):
        raise RuntimeError("compact_filterbank: this filterbank has not been seen yet, and building its compact form synchronises with "
                           "the host, which a graph capture forbids: run the fused front end once eagerly before capturing")
    if len(_FILTERBANKS) >= _CACHE_LIMIT:
        _FILTERBANKS.pop(next(iter(_FILTERBANKS)))
    form = _compact(freq2mels)
    _FILTERBANKS[key] = (tag, form, weakref.ref(freq2mels))
    return form


def _twiddles(W: int, device) -> torch.Tensor:
    """exp(-2 pi i k / W), k < W / 2, as [W / 2, 2] (cos, -sin): float64 rounded to fp32, once per (W, device)."""
    key = (int(W), str(device))
    tw = _TWIDDLES.get(key)
    if tw is None:
        if _capturing(device):
            raise RuntimeError("log_mel: the twiddle table of this window size is not on the device yet, and a graph capture cannot "
                               "copy it there: run the fused front end once eagerly before capturing")
        ang = torch.arange(W // 2, dtype=torch.float64) * (-2.0 * math.pi / W)
        tw = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).to(torch.float32).contiguous().to(device)
        _TWIDDLES[key] = tw
    return tw


def log_mel_supported(W: int, nWin: int, C: int, nMel: int, max_len: int, total: int) -> bool:
    """semicrf_log_mel_supported: W a power of two in [256, 4096], 1..8 windows, 1..16 channels, 1..512 bands, a longest column
    support of at most W / 2 + 1 and at most 65536 rows of support in all."""
    return bool(_lib.load().semicrf_log_mel_supported(int(W), int(nWin), int(C), int(nMel), int(max_len), int(total)))


def _as_batch(frames: torch.Tensor):
    """frames [..., nFrame, W] as the op's [N, C, nFrame, W] view, or None: the channel axis is the one in front of the frames."""
    if frames.dim() == 2:
        return frames.unsqueeze(0).unsqueeze(0)
    if frames.dim() == 3:
        return frames.unsqueeze(0)
    if frames.dim() == 4:
        return frames
    return None


def _log_mel_plan(frames, windows, freq2mels, shift, denom):
    """The op's arguments when the fused route applies, None otherwise."""
    ts = [frames, windows, freq2mels] + ([shift, denom] if shift is not None else [])
    if any(t.dtype != torch.float32 for t in ts) or any(t.device != frames.device for t in ts):
        return None
    if frames.device.type not in ("cuda", "cpu") or windows.dim() != 2 or freq2mels.dim() != 2 or frames.numel() == 0:
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return None                                                         # forward only
    x = _as_batch(frames)
    if x is None or x.stride(-1) != 1 or any(s < 0 for s in x.stride()):
        return None
    N, C, nFrame, W = x.shape
    nWin, nMel = windows.shape[0], freq2mels.shape[1]
    if windows.shape[1] != W or freq2mels.shape[0] != W // 2 + 1 or N * nFrame >= 2 ** 31:
        return None
    if not log_mel_supported(W, nWin, C, nMel, 0, 0):
        return None                                                         # before the filterbank is looked at
    start, length, offset, values, max_len, total = compact_filterbank(freq2mels)
    if not log_mel_supported(W, nWin, C, nMel, max_len, total):
        return None
    if shift is not None and (shift.numel() != N or denom.numel() != N):
        return None
    return x, (start, length, offset, values, max_len)


def log_mel(frames, windows, freq2mels, *, shift=None, denom=None, log=True, eps=1e-5, toMono=False, route="fused"):
    """The features of MelSpectrum from frames [..., nFrame, W] (the channel axis in front of the frames), windows [nWin, W] and a
    filterbank [W / 2 + 1, nMel]: [..., nFrame, nMel, nWin], one channel when toMono.  shift / denom, one value per recording
    (frames [N, C, nFrame, W]; any shape with N elements), apply (x - shift) / denom to every sample first: the gain normalisation
    without a normalised copy of the frames.

    route = "fused": the HIP op (the host kernel for CPU tensors) whenever it applies; the stock route (log_mel_torch) when a dtype
    is not float32, the shape is outside the supported set (log_mel_supported), the sample stride is not 1, or gradients are enabled
    and an input requires grad.  route = "torch": always the stock route.  Always usable, always differentiable."""
    if route not in FRONTEND_ROUTE_KINDS:
        raise ValueError(f"route must be one of {FRONTEND_ROUTE_KINDS}, not {route!r}")
    if (shift is None) != (denom is None):
        raise ValueError("shift and denom come together")
    usable = route == "fused" and not (log and not eps > 0)                 # the op refuses a log compression without a positive eps
    plan = _log_mel_plan(frames, windows, freq2mels, shift, denom) if usable else None
    if plan is None:
        FRONTEND_ROUTES["torch"] += 1
        if shift is not None:
            lead = (-1,) + (1,) * (frames.dim() - 1)
            frames = (frames - shift.reshape(lead)) / denom.reshape(lead)
        return log_mel_torch(frames, windows, freq2mels, log=log, eps=eps, toMono=toMono)
    FRONTEND_ROUTES["fused"] += 1
    x, (start, length, offset, values, max_len) = plan
    N, C, nFrame, W = x.shape
    mono = bool(toMono) and frames.dim() >= 3
    tw = _twiddles(W, x.device)
    out = torch.empty((N, 1 if mono else C, nFrame, freq2mels.shape[1], windows.shape[0]), dtype=torch.float32, device=x.device)
    gain = shift is not None
    none = tw                                                               # a defined tensor for the two unused arguments
    _lib.ops().log_mel(x, windows.contiguous(), tw, start, length, offset, values, int(max_len),
                       shift.reshape(-1).contiguous() if gain else none, denom.reshape(-1).contiguous() if gain else none, gain,
                       bool(log), float(eps), mono, out)
    return out.reshape(tuple(frames.shape[:-3]) + tuple(out.shape[-4:])) if frames.dim() >= 3 else out.reshape(out.shape[-3:])


def segment_features(mel: MelSpectrum, audio: torch.Tensor, hopSize: int, normalize: bool = True, route=None) -> torch.Tensor:
    """processFramesBatch (ModelTransformer.py:159-164) from audio [N, C, nSample]: frames, the per-recording gain normalisation and
    the features [N, C or 1, nFrame, nMel, nWin].  route: "torch", "fused" or None for the module's own.

    "torch": mel(normalize_gain(makeFrame(audio))) as the reference runs it.  "fused": the frames stay a view of the padded audio; the
    gain's mean and standard deviation are the reference's own two reductions over that view (stock ops), and they enter `log_mel` as
    shift and denom, so neither the normalised nor the windowed frames ever exist."""
    route = mel.route if route is None else route
    if route not in FRONTEND_ROUTE_KINDS:
        raise ValueError(f"route must be one of {FRONTEND_ROUTE_KINDS}, not {route!r}")
    ext = mel.spectrogramExtractor
    frames = makeFrame(audio, hopSize, ext.win.shape[0])
    if route == "torch":
        if normalize:
            frames = normalize_gain(frames)
        return log_mel_torch(frames, ext.windows(), mel.freq2mels, log=mel.log, eps=mel.eps, toMono=mel.toMono)
    shift = denom = None
    if normalize:
        shift = torch.mean(frames, dim=[1, 2, 3], keepdim=True)
        denom = torch.std(frames, dim=[1, 2, 3], keepdim=True) + 1e-8
    return log_mel(frames, ext.windows(), mel.freq2mels, shift=shift, denom=denom, log=mel.log, eps=mel.eps, toMono=mel.toMono, route="fused")
