"""Shared by the CPU and GPU tests of the fused audio front end (tests/test_logmel.py): seeded cases, the float64 yardstick, the stock
fp32 route on identical inputs and the gate.

Yardstick: the MelSpectrum module in float64 on the CPU (its stock expression; tests/test_frontend.py pins it to the reference).  Gate
(GATE = 8, as in backbone_common and ffn_common): per (recording, channel, window) slice of the output, the op's maximum absolute error
is at most GATE x the error of the stock fp32 route on the CPU in the same slice -- a quiet channel or a narrow window is not hidden
behind a loud one.

Shapes: N = 2 recordings, C = 2 channels, 7 frames from makeFrame of 6 hop + 17 samples, hop = W / 4, 24 bands unless stated
otherwise.  Audio: noise plus a 440 Hz sine, channel 1 scaled by 1e-3.  Cases are built once on the CPU (lru_cache) and never modified;
the GPU tests move copies, so that the device and the host mirror see the same bits (windows and gain are computed once, on the CPU).
"""
import functools
import math

import torch

GATE = 8.0
FS = 44100
WINDOW_SIZES = [256, 512, 1024, 2048, 4096]
WINDOW_COUNTS = [1, 2, 6, 8]
N_BANDS = 24


def make_audio(W, N=2, C=2, seed=0, dc=0.0):
    hop = W // 4
    n = 6 * hop + 17
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.randn(N, C, n, generator=g) * 0.1 + torch.sin(torch.arange(n) * (2 * math.pi * 440 / FS)) + dc
    if C > 1:
        a[:, 1] *= 1e-3
    return a


def make_module(W, nWin, log, mono, n_mels=N_BANDS, f_min=30.0, f_max=FS / 2, seed=0):
    """MelSpectrum with sigma and center moved off their initial values."""
    from transkun_amd import frontend as fe
    mel = fe.MelSpectrum(W, f_min, f_max, n_mels, FS, nExtraWins=nWin - 1, log=log, toMono=mono).eval()
    if nWin > 1:
        g = torch.Generator().manual_seed(2000 + seed)
        with torch.no_grad():
            mel.spectrogramExtractor.winGen.sigma.add_(torch.randn(nWin - 1, generator=g) * 0.3)
            mel.spectrogramExtractor.winGen.center.add_(torch.randn(nWin - 1, generator=g) * 0.3)
    return mel


def banded_matrix(W, n_mels=N_BANDS, seed=0):
    """A random banded [W / 2 + 1, n_mels] matrix whose supports reach row 0 (column 0) and row W / 2 (the last column), with an
    all-zero column (3) and a zero inside a support (column 5)."""
    nF = W // 2 + 1
    g = torch.Generator().manual_seed(3000 + seed)
    fb = torch.zeros(nF, n_mels)
    width = max(4, nF // n_mels + 3)
    for m in range(n_mels):
        lo = min(nF - width, (m * (nF - width)) // (n_mels - 1))
        fb[lo:lo + width, m] = torch.rand(width, generator=g) + 0.1
    fb[:, 3] = 0.0
    lo5 = int((fb[:, 5] != 0).nonzero()[0])
    fb[lo5 + 2, 5] = 0.0
    assert fb[0, 0] != 0 and fb[nF - 1, n_mels - 1] != 0
    return fb


def slice_error(got, truth):
    """max |got - truth| per (recording, channel, window): [N, C, nWin] from [N, C, nFrame, nMel, nWin]."""
    return (got.detach().cpu().double() - truth).abs().amax(dim=(2, 3))


def stock64(mel, frames):
    import copy
    with torch.no_grad():
        return copy.deepcopy(mel).double()(frames.double())


def build_case(mel, audio, gain=False):
    """Everything a test needs, all on the CPU: the frame view, the windows, truth, the stock fp32 result and its error per slice."""
    from transkun_amd import frontend as fe
    W = mel.spectrogramExtractor.win.shape[0]
    frames = fe.makeFrame(audio, W // 4, W)
    with torch.no_grad():
        windows = mel.spectrogramExtractor.windows().contiguous()
        truth = stock64(mel, fe.normalize_gain(frames.double()) if gain else frames)
        stock = mel(fe.normalize_gain(frames) if gain else frames)
        shift = denom = None
        if gain:
            shift = torch.mean(frames, dim=[1, 2, 3], keepdim=True)
            denom = torch.std(frames, dim=[1, 2, 3], keepdim=True) + 1e-8
    assert mel.route == "torch"
    return {"mel": mel, "audio": audio, "W": W, "frames": frames, "windows": windows, "fb": mel.freq2mels, "truth": truth, "stock": stock,
            "e32": slice_error(stock, truth), "shift": shift, "denom": denom, "log": mel.log, "mono": mel.toMono, "eps": mel.eps}


@functools.lru_cache(maxsize=None)
def case(W, nWin, log, mono, C=2, n_mels=N_BANDS, f_min=30.0, f_max=FS / 2, bank="mel", gain=False, dc=0.0):
    mel = make_module(W, nWin, log, mono, n_mels, f_min, f_max)
    if bank == "banded":
        mel.freq2mels = banded_matrix(W, n_mels)
    return build_case(mel, make_audio(W, C=C, dc=dc), gain)


def run(c, dev, frames=None):
    """The fused route on a copy of the case on `dev`; asserts that the fused route was taken."""
    from transkun_amd import frontend as fe
    dev = torch.device(dev)
    if frames is None:
        frames = fe.makeFrame(c["audio"].to(dev), c["W"] // 4, c["W"])
    before = dict(fe.FRONTEND_ROUTES)
    with torch.no_grad():
        out = fe.log_mel(frames, c["windows"].to(dev), c["fb"].to(dev), shift=None if c["shift"] is None else c["shift"].to(dev),
                         denom=None if c["denom"] is None else c["denom"].to(dev), log=c["log"], eps=c["eps"], toMono=c["mono"])
    assert fe.FRONTEND_ROUTES["fused"] == before["fused"] + 1 and fe.FRONTEND_ROUTES["torch"] == before["torch"], "the stock route ran"
    return out


def check_gate(c, got, what):
    assert got.shape == c["truth"].shape and got.dtype == torch.float32, (got.shape, c["truth"].shape)
    e = slice_error(got, c["truth"])
    ratio = e / c["e32"]
    worst = float(ratio.max())
    print(f"{what}: worst slice ratio {worst:.2f} (error {float(e.max()):.3e}, stock fp32 {float(c['e32'].max()):.3e})")
    assert bool((e <= GATE * c["e32"]).all()), (what, worst, e.tolist(), c["e32"].tolist())
    return worst


def raw_op(frames, windows, fb, shift, denom, log, eps, mono, out):
    """torch.ops.semicrf.log_mel as the Python layer calls it, into a caller's `out`."""
    from transkun_amd import _lib, frontend as fe
    start, length, offset, values, max_len, total = fe.compact_filterbank(fb)
    tw = fe._twiddles(frames.shape[-1], frames.device)
    gain = shift is not None
    _lib.ops().log_mel(frames, windows, tw, start, length, offset, values, max_len, shift.reshape(-1) if gain else tw,
                       denom.reshape(-1) if gain else tw, gain, log, eps, mono, out)
    return out
