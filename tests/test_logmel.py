"""The audio front end as one fused op (transkun_amd.frontend.log_mel / segment_features / MelSpectrum.route = "fused",
torch.ops.semicrf.log_mel; csrc/logmel.hip on the device, the host mirror of csrc/cpu_ops.cpp on the CPU).

1. accuracy: every window size x window count x log x mono against float64, gated per (recording, channel, window) slice by the stock
   fp32 route's own error (logmel_common); the model's own shape
2. band edges: supports that reach DC and Nyquist, an all-zero column, a zero inside a support; compact_filterbank round-trips; a
   matrix outside the caps takes the stock route
3. bits: the unfold view, a contiguous copy, a batch slice and swapped strides; a recording alone; one frame; one and three channels
4. gain folding: segment_features against float64 normalize_gain + module, on audio with an offset (the zero padding reads -mean / denom)
5. a NaN sample poisons exactly the frames that hold it; nothing behind the last sample is read, nothing around `out` is written
6. the device against the host mirror: the two run the same chain (logarithm included), so the bits must be EQUAL
7. routing; 8. graph capture; 9. audio -> decoded paths with the fused front end
The CPU tests run the host mirror; the same cases marked gpu run the kernel.
"""
import ctypes
import math

import pytest
import torch

import backbone_common
import logmel_common as common

CPU = torch.device("cpu")


def _fe():
    from transkun_amd import frontend
    return frontend


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------------
def _check_matrix(dev, W, nWin):
    for log in (True, False):
        for mono in (True, False):
            c = common.case(W, nWin, log, mono)
            common.check_gate(c, common.run(c, dev), f"[{torch.device(dev).type}] W {W} nWin {nWin} log {log} mono {mono}")


@pytest.mark.parametrize("nWin", common.WINDOW_COUNTS)
@pytest.mark.parametrize("W", common.WINDOW_SIZES)
def test_accuracy_matrix_cpu(W, nWin):
    _check_matrix(CPU, W, nWin)


@pytest.mark.gpu
@pytest.mark.parametrize("nWin", common.WINDOW_COUNTS)
@pytest.mark.parametrize("W", common.WINDOW_SIZES)
def test_accuracy_matrix_gpu(gpu, W, nWin):
    _check_matrix(gpu, W, nWin)


def _model_case():
    return common.case(4096, 6, True, True, n_mels=229, f_max=8000.0)


def test_model_shape_cpu():
    c = _model_case()
    common.check_gate(c, common.run(c, CPU), "[cpu] the model's front end")


@pytest.mark.gpu
def test_model_shape_gpu(gpu):
    c = _model_case()
    common.check_gate(c, common.run(c, gpu), "[cuda] the model's front end")


# ---- 2. band edges ----------------------------------------------------------------------------------------------------------------------
def _dense_from_compact(form, shape, dtype):
    start, length, offset, values, max_len, total = form
    dense = torch.zeros(shape, dtype=dtype)
    for m, (s, n, o) in enumerate(zip(start.tolist(), length.tolist(), offset.tolist())):
        dense[s:s + n, m] = values.cpu()[o:o + n]
    return dense


@pytest.mark.parametrize("W", [256, 1024, 4096])
def test_compact_filterbank_round_trip(W):
    fe = _fe()
    nF = W // 2 + 1
    banded = common.banded_matrix(W)
    start, length, offset, values, max_len, total = form = fe.compact_filterbank(banded)
    assert torch.equal(_dense_from_compact(form, banded.shape, banded.dtype), banded)
    assert start.dtype == torch.int32 and length.dtype == torch.int32 and offset.dtype == torch.int32
    assert int(start[0]) == 0 and int(start[-1] + length[-1]) == nF              # DC and Nyquist lie inside a support
    assert int(length[3]) == 0                                                   # the all-zero column
    s5, n5 = int(start[5]), int(length[5])
    assert n5 > 3 and float(banded[s5 + 2, 5]) == 0.0                            # a zero inside a support is kept
    assert max_len == int(length.max()) and total == int(length.sum()) == int((values != 0).sum()) + 1
    assert offset.tolist() == (torch.cumsum(length, 0) - length).tolist()
    full = fe.melscale_fbanks(nF, 0.0, common.FS / 2, common.N_BANDS, common.FS)
    form = fe.compact_filterbank(full)
    assert torch.equal(_dense_from_compact(form, full.shape, full.dtype), full)
    model = fe.melscale_fbanks(2049, 30.0, 8000.0, 229, common.FS)
    form = fe.compact_filterbank(model)
    assert torch.equal(_dense_from_compact(form, model.shape, model.dtype), model)
    assert form[5] == int((model != 0).sum()) == 1472 and form[4] == int(form[1].max())
    assert fe.compact_filterbank(model) is form                                  # cached


def test_compact_filterbank_does_not_mistake_a_new_tensor_for_a_freed_one():
    """A temporary's storage is handed out again once it is freed, with the same address, shape and version: the cache must not
    answer for the tensor that lived there before."""
    fe = _fe()
    seen = set()
    for seed in range(8):
        fb = common.banded_matrix(512, seed=seed)
        seen.add(fb.data_ptr())
        assert torch.equal(_dense_from_compact(fe.compact_filterbank(fb), fb.shape, fb.dtype), fb), seed
        del fb
    print("distinct addresses among 8 temporaries:", len(seen))


def _check_band_edges(dev, W):
    for bank, f_min in (("banded", 30.0), ("mel", 0.0)):
        for log in (True, False):
            c = common.case(W, 2, log, False, f_min=f_min, bank=bank)
            common.check_gate(c, common.run(c, dev), f"[{torch.device(dev).type}] W {W} bank {bank} log {log}")


@pytest.mark.parametrize("W", [256, 2048])
def test_band_edges_cpu(W):
    _check_band_edges(CPU, W)
    c = common.case(W, 2, False, False, bank="banded")
    got = common.run(c, CPU)
    assert float(got[:, :, :, 3].abs().max()) == 0.0                             # the all-zero column gives 0
    assert float(got[:, :, :, 0].min()) > 0.0 and float(got[:, :, :, -1].min()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("W", [256, 2048])
def test_band_edges_gpu(gpu, W):
    _check_band_edges(gpu, W)


def test_matrix_outside_the_caps_takes_the_stock_route():
    from transkun_amd import _lib
    fe = _fe()
    c = common.case(1024, 2, True, False)
    g = torch.Generator().manual_seed(5)
    dense = torch.rand(513, common.N_BANDS, generator=g)                          # total = 513 x 24 <= the cap: fused
    wide = torch.rand(513, _lib.LOGMEL_MAX_BANDS + 1, generator=g) * (torch.rand(513, 1, generator=g) < 0.05)
    heavy = torch.rand(513, 200, generator=g)                                    # 102 600 rows of support > 65 536
    assert fe.log_mel_supported(1024, 2, 2, 24, 513, 513 * 24) and not fe.log_mel_supported(1024, 2, 2, 200, 513, 513 * 200)
    assert not fe.log_mel_supported(1024, 2, 2, 24, 514, 600) and not fe.log_mel_supported(1000, 2, 2, 24, 10, 100)
    assert not fe.log_mel_supported(1024, 9, 2, 24, 10, 100) and not fe.log_mel_supported(1024, 2, _lib.LOGMEL_MAX_CHANNELS + 1, 24, 10, 100)
    assert not fe.log_mel_supported(128, 1, 1, 24, 10, 100) and not fe.log_mel_supported(8192, 1, 1, 24, 10, 100)
    for fb, want in ((dense, "fused"), (wide, "torch"), (heavy, "torch")):
        before = dict(fe.FRONTEND_ROUTES)
        with torch.no_grad():
            got = fe.log_mel(c["frames"], c["windows"], fb)
            ref = fe.log_mel_torch(c["frames"], c["windows"], fb)
        assert fe.FRONTEND_ROUTES[want] == before[want] + 1, (want, fb.shape)
        assert got.shape == ref.shape
        if want == "torch":
            assert torch.equal(got, ref)
        else:
            assert torch.allclose(got, ref, atol=1e-5)


# ---- 3. strides and independence ----------------------------------------------------------------------------------------------------------
def _check_strides(dev):
    fe = _fe()
    dev = torch.device(dev)
    for mono in (False, True):
        c = common.case(1024, 6, True, mono)
        W, hop = 1024, 256
        audio = c["audio"].to(dev)
        view = fe.makeFrame(audio, hop, W)
        assert view.stride(-2) == hop and not view.is_contiguous()
        ref = common.run(c, dev, view)
        copy = view.contiguous()
        assert copy.stride(-2) == W
        assert torch.equal(common.run(c, dev, copy), ref), "contiguous copy"
        big = torch.cat([torch.full_like(copy[:1], 3.0), copy, torch.full_like(copy[:1], -2.0)], dim=0)
        assert torch.equal(common.run(c, dev, big[1:3]), ref), "batch slice"
        swapped = copy.transpose(0, 1).contiguous().transpose(0, 1)
        assert swapped.stride(0) < swapped.stride(1)
        assert torch.equal(common.run(c, dev, swapped), ref), "swapped recording and channel strides"
        odd = torch.zeros(copy.numel() + 3, device=dev)[3:].view(copy.shape).copy_(copy)          # 12 bytes off the allocation
        assert torch.equal(common.run(c, dev, odd), ref), "off 16 bytes"
        alone = common.run(c, dev, view[:1])
        assert torch.equal(alone, ref[:1]), "recording 0 alone"
        one = common.run(c, dev, view[:, :, 3:4])
        assert one.shape[2] == 1 and torch.equal(one, ref[:, :, 3:4]), "one frame"
        assert torch.equal(common.run(c, dev, view[1:, :, 5:]), ref[1:, :, 5:]), "another position in the launch"


def test_strides_and_independence_cpu():
    _check_strides(CPU)


@pytest.mark.gpu
def test_strides_and_independence_gpu(gpu):
    _check_strides(gpu)


def _check_channels(dev):
    for C in (1, 3):
        for mono in (False, True):
            c = common.case(512, 2, True, mono, C=C)
            got = common.run(c, dev)
            assert got.shape[1] == (1 if mono else C)
            common.check_gate(c, got, f"[{torch.device(dev).type}] C {C} mono {mono}")


def test_one_and_three_channels_cpu():
    _check_channels(CPU)


@pytest.mark.gpu
def test_one_and_three_channels_gpu(gpu):
    _check_channels(gpu)


def test_fewer_dimensions_cpu():
    """[C, nFrame, W] and [nFrame, W] inputs give the shapes of the stock route (no channel mean without a channel axis)."""
    fe = _fe()
    c = common.case(512, 2, True, True)
    ref = common.run(c, CPU)
    with torch.no_grad():
        got3 = fe.log_mel(c["frames"][0], c["windows"], c["fb"], toMono=True)
        got2 = fe.log_mel(c["frames"][0, 0], c["windows"], c["fb"], toMono=True)
        ref2 = fe.log_mel_torch(c["frames"][0, 0], c["windows"], c["fb"], toMono=True)
    assert torch.equal(got3, ref[0]) and got2.shape == ref2.shape and torch.allclose(got2, ref2, atol=1e-5)


# ---- 4. gain folding ----------------------------------------------------------------------------------------------------------------------
def _check_gain(dev):
    fe = _fe()
    dev = torch.device(dev)
    for W, nWin, log, mono in ((1024, 2, True, True), (4096, 6, True, False), (256, 1, False, False)):
        c = common.case(W, nWin, log, mono, gain=True, dc=0.5)
        common.check_gate(c, common.run(c, dev), f"[{dev.type}] gain folded, W {W}")
        # the padding of the first frame reads -mean / denom: without the gain there the first frame would be far off
        mel = c["mel"]
        with torch.no_grad():
            wrong = mel(torch.where(c["frames"] == 0, c["frames"], fe.normalize_gain(c["frames"])))
        assert float((wrong.double() - c["truth"]).abs()[:, :, 0].max()) > 1e3 * float(c["e32"].max())
    # segment_features itself: its own reductions on `dev`, so gated against the stock route's error with a margin-free gate as well
    c = common.case(1024, 2, True, True, gain=True, dc=0.5)
    import copy
    mel = copy.deepcopy(c["mel"]).to(dev)
    before = dict(fe.FRONTEND_ROUTES)
    with torch.no_grad():
        got = fe.segment_features(mel, c["audio"].to(dev), 256, normalize=True, route="fused")
        stock = fe.segment_features(mel, c["audio"].to(dev), 256, normalize=True, route="torch")
        plain = fe.segment_features(mel, c["audio"].to(dev), 256, normalize=False, route="fused")
    assert fe.FRONTEND_ROUTES["fused"] == before["fused"] + 2
    common.check_gate(c, got, f"[{dev.type}] segment_features")
    if dev.type == "cpu":
        assert torch.equal(stock, c["stock"])                                     # the "torch" route is the reference's expression
    assert not torch.allclose(plain, got)


def test_gain_folding_cpu():
    _check_gain(CPU)


@pytest.mark.gpu
def test_gain_folding_gpu(gpu):
    _check_gain(gpu)


# ---- 5. non-finite and poison -------------------------------------------------------------------------------------------------------------
def _check_nan(dev):
    fe = _fe()
    dev = torch.device(dev)
    W, hop = 1024, 256
    for mono in (False, True):
        c = common.case(W, 6, True, mono)
        assert int(fe.compact_filterbank(c["fb"])[1].min()) > 0                   # every band has a support
        clean = common.run(c, dev)
        audio = c["audio"].clone()
        pos = 2 * hop + 100                                                      # padded position W / 2 + pos
        audio[1, 0, pos] = float("nan")
        got = common.run(c, dev, fe.makeFrame(audio.to(dev), hop, W))
        padded = W // 2 + pos
        hit = [t for t in range(clean.shape[2]) if t * hop <= padded < t * hop + W]
        assert len(hit) == 4
        bad = torch.zeros(clean.shape, dtype=torch.bool)
        bad[1, 0, hit] = True                                                    # channel 0 of recording 1 (its mixdown when mono)
        assert bool(torch.isnan(got.cpu()[bad]).all()), "a frame that holds the NaN is not NaN in every window and band"
        assert torch.equal(got.cpu()[~bad], clean.cpu()[~bad]), "an element outside those frames changed"


def test_nan_sample_cpu():
    _check_nan(CPU)


@pytest.mark.gpu
def test_nan_sample_gpu(gpu):
    _check_nan(gpu)


def _check_poison(dev):
    fe = _fe()
    dev = torch.device(dev)
    W, hop = 512, 128
    for mono in (False, True):
        c = common.case(W, 2, True, mono)
        ref = common.run(c, dev)
        padded = fe.makeFrame(c["audio"], hop, W)
        L = (padded.shape[2] - 1) * hop + W                                      # the samples the frames span
        N, C = c["audio"].shape[:2]
        buf = torch.full((N, C, L + 5), float("nan"))
        buf[:, :, :L] = torch.nn.functional.pad(c["audio"], (W // 2, L - W // 2 - c["audio"].shape[-1]))
        buf = buf.to(dev)
        frames = buf[:, :, :L].unfold(-1, W, hop)                                 # NaN behind the last sample of every row
        assert torch.equal(frames.cpu(), padded)
        guard = 64
        flat = torch.full((ref.numel() + 2 * guard,), 777.0, device=dev)
        out = flat[guard:guard + ref.numel()].view(ref.shape)
        common.raw_op(frames, c["windows"].to(dev), c["fb"].to(dev), None, None, True, c["eps"], mono, out)
        assert torch.equal(out, ref)
        assert bool((flat[:guard] == 777.0).all()) and bool((flat[guard + ref.numel():] == 777.0).all())


def test_poison_cpu():
    _check_poison(CPU)


@pytest.mark.gpu
def test_poison_gpu(gpu):
    _check_poison(gpu)


# ---- 6. the device against the host mirror ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W", common.WINDOW_SIZES)
def test_device_equals_mirror_gpu(gpu, W):
    """Both sides run logmel_math.h's chain on the same inputs, and the chain has no library call in it (the logarithm is evaluated in
    float64 arithmetic and rounded once): measured on the device, the difference is 0 with and without the log, so equality is required
    (the issue's fallback of 2 ulp for the log output is not needed)."""
    for nWin, log, mono, gain in ((6, False, False, False), (6, True, True, True), (1, True, False, False), (8, False, True, True)):
        c = common.case(W, nWin, log, mono, gain=gain, dc=0.5 if gain else 0.0)
        host, device = common.run(c, CPU), common.run(c, gpu).cpu()
        assert torch.equal(host, device), (W, nWin, log, mono, gain, float((host - device).abs().max()))
    c = _model_case() if W == 4096 else common.case(W, 2, True, False, bank="banded")
    assert torch.equal(common.run(c, CPU), common.run(c, gpu).cpu())


# ---- 7. routing -------------------------------------------------------------------------------------------------------------------------
def _forward_as_before(self, frames):
    """MelSpectrum.forward as it stood before the fused route existed."""
    power = self.spectrogramExtractor(frames).abs().pow(2)
    if self.toMono and power.dim() >= 4:
        power = power.mean(dim=-4, keepdim=True)
    mel = (power.transpose(-1, -2) @ self.freq2mels).transpose(-1, -2)
    if self.log:
        mel = ((mel + self.eps).log() - math.log(self.eps)) / (-math.log(self.eps))
    return mel


def test_routing_cpu():
    fe = _fe()
    assert fe.DEFAULT_FRONTEND_ROUTE == "torch" and set(fe.FRONTEND_ROUTES) == {"fused", "torch"}
    c = common.case(1024, 6, True, True)
    mel = common.make_module(1024, 6, True, True)
    assert mel.route == "torch"
    frames = c["frames"]

    def routes(fn):
        before = dict(fe.FRONTEND_ROUTES)
        out = fn()
        return out, {k: fe.FRONTEND_ROUTES[k] - before[k] for k in before}

    with torch.no_grad():
        ref = _forward_as_before(mel, frames)
        out, d = routes(lambda: mel(frames))
        assert d == {"fused": 0, "torch": 0} and torch.equal(out, ref)             # the default touches nothing
        out, d = routes(lambda: fe.log_mel(frames, mel.spectrogramExtractor.windows(), mel.freq2mels, log=True, toMono=True, route="torch"))
        assert d == {"fused": 0, "torch": 1} and torch.equal(out, ref)
        mel.route = "fused"
        out, d = routes(lambda: mel(frames))
        assert d == {"fused": 1, "torch": 0} and not torch.equal(out, ref) and torch.allclose(out, ref, atol=1e-5)
        out, d = routes(lambda: mel.double()(frames.double()))                     # float64: the stock route
        mel.float()
        assert d == {"fused": 0, "torch": 1} and out.dtype == torch.float64
        strided = torch.zeros(frames.shape + (2,))[..., 0].copy_(frames)            # sample stride 2
        assert strided.stride(-1) == 2
        out, d = routes(lambda: mel(strided))
        assert d == {"fused": 0, "torch": 1} and torch.equal(out, ref)
    out, d = routes(lambda: mel(frames))                                           # grad mode on: sigma and center are Parameters
    assert d == {"fused": 0, "torch": 1} and out.requires_grad and torch.equal(out.detach(), ref)
    out.sum().backward()
    assert mel.spectrogramExtractor.winGen.sigma.grad is not None
    with pytest.raises(ValueError):
        fe.log_mel(frames, c["windows"], c["fb"], route="triton")
    with pytest.raises(ValueError):
        fe.log_mel(frames, c["windows"], c["fb"], shift=torch.zeros(2))


def test_c_entry_rejects_bad_arguments_without_a_gpu():
    """semicrf_log_mel checks its arguments before anything is launched: SEMICRF_EINVAL and a message."""
    from transkun_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)                                                    # never dereferenced
    good = dict(W=1024, nWin=2, C=2, nMel=24, total=100, N=1, nFrame=3, shift=None, denom=None, eps=1e-5, out=ctypes.c_void_p(1 << 30))

    def call(**kw):
        a = dict(good, **kw)
        return lib.semicrf_log_mel(p, 5000, 2000, 256, a["N"], a["C"], a["nFrame"], a["W"], p, a["nWin"], p, p, p, p, p, a["nMel"], a["total"],
                                   a["shift"], a["denom"], 1, a["eps"], 0, a["out"], None)

    for kw, msg in ((dict(W=1000), b"supported set"), (dict(W=8192), b"supported set"), (dict(nWin=9), b"supported set"),
                    (dict(C=17), b"supported set"), (dict(nMel=513), b"supported set"), (dict(total=65537), b"supported set"),
                    (dict(nFrame=0), b">= 1"), (dict(shift=p), b"together"), (dict(eps=0.0), b"positive"), (dict(out=None), b"non-NULL"),
                    (dict(out=ctypes.c_void_p(4098)), b"aligned"), (dict(out=ctypes.c_void_p(4096 + 1024)), b"overlaps")):
        assert call(**kw) == 1 and msg in lib.semicrf_last_error(), (kw, lib.semicrf_last_error())
    assert lib.semicrf_log_mel_supported(4096, 6, 2, 229, 2049, 1472) == 1


def test_load_state_dict_refreshes_the_compact_form():
    fe = _fe()
    c = common.case(1024, 6, True, True)
    mel = common.make_module(1024, 6, True, True)
    mel.route = "fused"
    with torch.no_grad():
        a = mel(c["frames"])
        form = fe.compact_filterbank(mel.freq2mels)
        assert fe.compact_filterbank(mel.freq2mels) is form
        sd = {k: v.clone() for k, v in mel.state_dict().items()}
        sd["freq2mels"] = torch.roll(sd["freq2mels"], 7, dims=0) * 2.0
        mel.load_state_dict(sd, strict=True)
        assert fe.compact_filterbank(mel.freq2mels) is not form
        b = mel(c["frames"])
        mel.route = "torch"
        ref = mel(c["frames"])
    assert not torch.allclose(a, b, atol=1e-3) and torch.allclose(b, ref, atol=1e-5)


# ---- 8. graph capture ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_graph_capture_gpu(gpu):
    fe = _fe()
    c = common.case(1024, 6, True, True, gain=True, dc=0.5)
    import copy
    mel = copy.deepcopy(c["mel"]).to(gpu)
    mel.route = "fused"
    static = c["audio"].to(gpu).clone()
    other = common.make_audio(1024, seed=9, dc=-0.25).to(gpu)
    with torch.no_grad():
        warm = fe.segment_features(mel, static, 256)                              # fills the caches
        eager_other = fe.segment_features(mel, other, 256)
        torch.cuda.synchronize()
        before = dict(fe.FRONTEND_ROUTES)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = fe.segment_features(mel, static, 256)
        assert fe.FRONTEND_ROUTES["fused"] == before["fused"] + 1 and fe.FRONTEND_ROUTES["torch"] == before["torch"]
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, warm)
        static.copy_(other)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager_other) and not torch.equal(out, warm)


def test_cold_call_inside_a_capture_is_an_error(monkeypatch):
    """A filterbank or a twiddle table that is not cached yet cannot be built during a capture: a clear error, no synchronisation."""
    fe = _fe()
    monkeypatch.setattr(fe, "_capturing", lambda device: True)
    fresh = common.banded_matrix(512, seed=77)
    with pytest.raises(RuntimeError, match="eagerly before capturing"):
        fe.compact_filterbank(fresh)
    monkeypatch.setattr(fe, "_TWIDDLES", {})
    with pytest.raises(RuntimeError, match="eagerly before capturing"):
        fe._twiddles(512, CPU)
    monkeypatch.undo()
    assert fe.compact_filterbank(fresh)[5] > 0


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_decode_gpu(gpu):
    """audio -> segment_features -> Backbone (small fixture) -> interval scorer -> NeuralSemiCRFInterval.decode(), the chain of
    tests/test_backbone.py::test_end_to_end_decode_gpu: with the fused front end the decoded paths EQUAL those of the stock one (the
    paths are compared, not ctx)."""
    from transkun_amd import CRF, synth
    from transkun_amd.frontend import MelSpectrum, segment_features
    from transkun_amd.scorer import ScaledInnerProductIntervalScorer
    fs, hop, win = 44100, 1024, 4096
    nS = 2 * fs
    audio = synth.hash_normal(2 * nS, 971, gpu).view(1, 2, nS) * 0.1
    mel = MelSpectrum(win, 30, 8000, 229, fs, nExtraWins=5, log=True, toMono=True).to(gpu).eval()
    m, fx = backbone_common.make_backbone("backbone_small", gpu, "fused")
    idx = fx["outputIndices"].to(gpu)
    D = fx["cfg"]["baseSize"] * fx["cfg"]["expansionFactor"]
    torch.manual_seed(67280421310721)
    scorer = ScaledInnerProductIntervalScorer(D, 1).to(gpu)
    paths, ctxs = {}, {}
    fe = _fe()
    with torch.no_grad():
        for route in ("fused", "torch"):
            before = dict(fe.FRONTEND_ROUTES)
            feat = segment_features(mel, audio, hop, normalize=True, route=route)[:, 0]
            assert fe.FRONTEND_ROUTES["fused"] == before["fused"] + (route == "fused")
            T = feat.shape[1]
            ctx = m(feat, idx)
            assert ctx.shape == (1, idx.numel(), T, D) and bool(torch.isfinite(ctx).all())
            S, b = scorer(ctx)
            ctxs[route] = ctx
            paths[route] = CRF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1)).decode()
    print("max |ctx(fused) - ctx(torch)|", float((ctxs["fused"] - ctxs["torch"]).abs().max()))
    assert len(paths["fused"]) == idx.numel() and paths["fused"] == paths["torch"]
