"""CPU-side checks of the drop-in boundary: the C-ABI library builds, loads and exports every
symbol include/semicrf_hip.h declares; the Python mirror keeps the reference's surface and
refuses to run without a GPU (no CPU fallback)."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    src = open(os.path.join(ROOT, "include", "semicrf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = re.findall(r"\b([a-z_0-9]+)\s*\([^;{]*\)\s*;", src)
    return sorted(set(n for n in names if n.startswith(("semicrf_", "interval_score", "interval_features", "segment_", "scorer_proj", "scorer_merge", "scorer_stage"))))


def test_library_builds_and_exports_header_symbols():
    from transkun_amd import _build, _lib
    path = _build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    declared = _declared_functions()
    assert len(declared) >= 10
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in semicrf_hip.h but not exported"
    assert set(_lib.EXPORTED) == set(declared)
    loaded = _lib.load()
    assert loaded.semicrf_abi_version() == 2
    assert loaded.semicrf_workspace_bytes(_lib.OP_VITERBI, 1024, 352) > 0


def test_ctypes_prototypes_come_from_the_header():
    """_lib._SIGS is parsed from include/semicrf_hip.h (transkun_amd/_abi.py).  Six prototypes are written out here by hand, so that
    the parser is held against something that is not itself; the count is held against this module's own regex."""
    from transkun_amd import _lib
    vp, i, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_size_t
    pinned = {
        "semicrf_last_error": (ctypes.c_char_p, []),
        "semicrf_workspace_bytes": (sz, [i, i, i]),
        "semicrf_logz_fwd": (i, [vp, vp, i, i, vp, vp, vp, sz, vp]),
        "semicrf_sample": (i, [vp, vp, vp, i, i, i64, i, ctypes.c_uint64, vp, vp, i64, vp, vp, sz, vp]),
        "semicrf_adabelief_step": (i, [vp, vp, vp, vp, i64, vp, _lib.AdaBeliefGroups, vp]),
        "semicrf_axial_attention_bwd": (i, [vp] * 8 + [i64] * 2 + [i] * 4 + [i64] * 24 + [vp]),
    }
    for name, sig in pinned.items():
        assert _lib._SIGS[name] == sig, name
    assert _lib._SIGS["semicrf_sample"][1][7] is ctypes.c_uint64
    assert _lib._SIGS["semicrf_adabelief_step"][1][6] is _lib.AdaBeliefGroups
    declared = _declared_functions()
    assert len(_lib._SIGS) == len(declared) == len(_lib.EXPORTED)
    assert _lib.EXPORTED == tuple(_lib._SIGS)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "semicrf_hip.h")).read(), flags=re.S)
    order = [n for n in re.findall(r"\b([a-z_0-9]+)\s*\([^;{]*\)\s*;", src) if n in set(declared)]
    assert list(_lib.EXPORTED) == order                       # the header's order


def test_header_parser_never_guesses():
    from transkun_amd import _abi
    with pytest.raises(_abi.SemiCRFLibraryError, match=r"f.*long double"):
        _abi.prototypes("int f(long double x);", {})
    with pytest.raises(_abi.SemiCRFLibraryError):
        _abi.prototypes("int g(struct_by_value s);", {})
    assert _abi.prototypes("const char* h(void); void k(const unsigned char* p, size_t n);", {}) == {
        "h": (ctypes.c_char_p, []), "k": (None, [ctypes.c_void_p, ctypes.c_size_t])}
    got = _abi.constants("#define SEMICRF_X foo(1)\n#define SEMICRF_Y ((1 << 4) - 1) /* c */\n#define SEMICRF_Z 0x10\n"
                         "#define SEMICRF_W 1.5\n#define SEMICRF_V 010\n#define OTHER 3\n#define SEMICRF_GUARD\n")
    assert got == {"Y": 15, "Z": 16}


def test_constants_come_from_the_header():
    from transkun_amd import _lib, attributes, scorer
    import importlib
    mod = importlib.import_module("transkun_amd.CRF.NeuralSemiCRFInterval")
    assert _lib.OP_LOGZ_FWD == 0 and _lib.OP_VITERBI == 2 and _lib.OP_ATTRIBUTE_HEADS_BWD == 13
    assert _lib.TOL_MAX == 8 and _lib.HEADS_ROW_TILE == 64 and _lib.OPTIM_MAX_GROUPS == 8 and _lib.ABI_VERSION == 2
    assert _lib.LEN_MODES == {"linear": 0, "sqrt": 1, "none": 2}
    assert scorer.BF16X3 == 4 and scorer.LEN_BF16X3 == 16 and scorer.PROJ_TN_BF16X3 == 0x40000000
    assert attributes.VELOCITY_CRITERIA == {"hamming": 0, "mse": 1, "match": 2, "mae": 3}
    assert mod.GRAD_UPPER_IS_ZERO == 1
    assert _lib.PTAB_COVERED == 1 << 30 and _lib.PTAB_NONE == (1 << 30) - 1


def test_structures_match_the_header():
    """The two ctypes.Structure classes stay hand-written: their fields are held against the header's typedef struct text, in
    name, order and C type, and their sizes against the layout the header spells out (it pads explicitly with pad_)."""
    from transkun_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "semicrf_hip.h")).read(), flags=re.S)
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "float": ctypes.c_float}
    size = {"int64_t": 8, "int32_t": 4, "float": 4}

    def members(name):
        body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), src, flags=re.S).group(1)
        out = []
        for decl in body.split(";"):
            if decl.strip():
                kind, names = decl.split(None, 1)
                out += [(kind, n.strip()) for n in names.split(",")]
        return out

    group = members("semicrf_adabelief_group")
    assert [(n, ctype[k]) for k, n in group] == list(_lib.AdaBeliefGroup._fields_)
    group_bytes = sum(size[k] for k, _ in group)
    assert ctypes.sizeof(_lib.AdaBeliefGroup) == group_bytes == 48

    groups = members("semicrf_adabelief_groups")
    assert groups == [("int32_t", "n"), ("int32_t", "pad_"), ("semicrf_adabelief_group", "g[SEMICRF_OPTIM_MAX_GROUPS]")]
    fields = list(_lib.AdaBeliefGroups._fields_)
    assert [f[0] for f in fields] == ["n", "pad_", "g"]
    assert fields[0][1] is ctypes.c_int32 and fields[1][1] is ctypes.c_int32
    assert fields[2][1]._type_ is _lib.AdaBeliefGroup and fields[2][1]._length_ == _lib.OPTIM_MAX_GROUPS
    assert ctypes.sizeof(_lib.AdaBeliefGroups) == 4 + 4 + _lib.OPTIM_MAX_GROUPS * group_bytes


def test_invalid_arguments_are_rejected_without_gpu():
    from transkun_amd import _lib
    lib = _lib.load()
    rc = lib.semicrf_logz_fwd(None, None, 0, 4, None, None, None, 0, None)
    assert rc == 1
    assert b"must be >= 1" in lib.semicrf_last_error()
    rc = lib.semicrf_logz_fwd(None, None, 8, 4, None, None, None, 0, None)
    assert rc == 1 and b"NULL" in lib.semicrf_last_error()
    # full_square: triangle mode 0..2 in bits 0-1, SEMICRF_SCORE_BF16X3 (4) in bit 2, nothing else
    import ctypes
    fake = ctypes.c_void_p(4096)            # never dereferenced: the argument check comes first
    for bad in (3, 7, 8, -1):
        rc = lib.interval_score_fwd(fake, fake, fake, 2, 8, 64, 64, 64, 1, 0.125, 0, bad, fake, None, None)
        assert rc == 1 and b"full_square" in lib.semicrf_last_error(), bad


def test_python_surface_matches_reference():
    from transkun_amd import CRF
    cls = CRF.NeuralSemiCRFInterval
    assert list(inspect.signature(cls.__init__).parameters) == ["self", "score", "noiseScore"]
    sig = inspect.signature(cls.decode)
    assert list(sig.parameters) == ["self", "forcedStartPos", "forward"]
    assert sig.parameters["forcedStartPos"].default is None and sig.parameters["forward"].default is False
    assert list(inspect.signature(cls.evalPath).parameters) == ["self", "intervals"]
    assert inspect.signature(cls.computeLogZ).parameters["noBackward"].default is False
    assert list(inspect.signature(cls.logProb).parameters) == ["self", "intervals", "noBackward"]
    for fn in ("viterbi", "viterbiBackward", "computeLogZ", "forward_backward", "evalPath", "computeLogZFasterGrad"):
        assert hasattr(CRF, fn)
    crf = cls(torch.zeros(3, 3, 2), torch.zeros(2, 2))
    assert crf.score.shape == (3, 3, 2) and crf.noiseScore.shape == (2, 2)


def test_gpu_only_entry_points_refuse_cpu_tensors():
    """CPU tensors are dispatched to the shim's host kernels for the CRF ops (tests/test_cpu_dispatch.py); the GPU-only entry
    points say so instead of computing anything elsewhere, and no op has a fallback from one device to another."""
    from transkun_amd import _lib
    with pytest.raises(RuntimeError, match="only runs on an AMD GPU"):
        _lib.require_gpu(torch.zeros(1), "ctx")
    ops = _lib.ops()
    with pytest.raises((NotImplementedError, RuntimeError)):        # no CPU kernel registered for the segment loop
        ops.segment_onset_filter(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), 1, 4,
                                 torch.zeros(1, 2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


def test_shape_asserts_like_reference():
    from transkun_amd import CRF
    with pytest.raises(AssertionError):
        CRF.NeuralSemiCRFInterval(torch.zeros(4, 5, 2), torch.zeros(3, 2)).computeLogZ()
    with pytest.raises(AssertionError):
        CRF.NeuralSemiCRFInterval(torch.zeros(4, 4, 2), torch.zeros(4, 2)).computeLogZ()
    with pytest.raises(AssertionError):
        CRF.NeuralSemiCRFInterval(torch.zeros(4, 4), torch.zeros(3, 2)).decode()


def test_product_never_imports_oracle():
    """The product package must not reference oracle/ (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "transkun_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "import oracle" not in txt and "from oracle" not in txt and "oracle/" not in txt, f


def test_pack_unpack_roundtrip():
    from transkun_amd.CRF.NeuralSemiCRFInterval import pack_intervals, unpack_intervals
    iv = [[(0, 2), (4, 6), (6, 6), (7, 8)], [(1, 2), (3, 5), (19, 19)], [(0, 0), (4, 7)], []]
    pairs, offsets = pack_intervals(iv, 200, 4, "cpu")
    assert offsets.tolist() == [0, 4, 7, 9, 9]
    assert unpack_intervals(pairs, offsets) == iv
    with pytest.raises(IndexError):
        pack_intervals([[(0, 200)], [], [], []], 200, 4, "cpu")
    p2, o2 = pack_intervals([[], []], 5, 2, "cpu")
    assert o2.tolist() == [0, 0, 0]
    assert unpack_intervals(p2[:0], o2) == [[], []]


def test_synth_numpy_torch_identical():
    import numpy as np
    from transkun_amd import synth
    a = synth.hash_normal(10007, 99, "cpu").numpy()
    b = synth.hash_normal_numpy(10007, 99)
    assert np.array_equal(a, b)
    assert abs(float(a.mean())) < 0.05 and 1.0 < float(a.std()) < 1.3
    iv = synth.synthetic_intervals(256, 12, seed=3)
    for lst in iv:
        last = -1
        for (b0, e0) in lst:
            assert 0 <= b0 <= e0 < 256 and b0 >= last
            last = e0


def test_scorer_regrouped_linear_rows():
    """The mirror runs the reference's Linear ([q | k | diag] rows, LayersTransformer.py:392-397) as [q | diag | pad] and k:
    same numbers as slicing the packed output, gradients reach the original parameter rows, pad rows stay zero."""
    import torch
    import torch.nn.functional as F
    from transkun_amd.scorer import QPAD, ScaledInnerProductIntervalScorer, qd_weights
    D = 8
    m = ScaledInnerProductIntervalScorer(D, 1)
    assert list(m.state_dict().keys()) == ["map.0.weight", "map.0.bias"]          # checkpoints of the reference load
    W, b = m.map[0].weight, m.map[0].bias
    assert W.shape == (2 * D + 1, D)
    x = torch.randn(3, 5, D)
    packed = F.linear(x, W, b)
    Wqd, bqd = qd_weights(W, b, D)
    qd = F.linear(x, Wqd, bqd)
    assert qd.shape[-1] == D + QPAD and (D + QPAD) % 4 == 0
    assert torch.allclose(qd[..., :D], packed[..., :D], atol=1e-6)
    assert torch.allclose(qd[..., D], packed[..., 2 * D], atol=1e-6)
    assert float(qd[..., D + 1:].abs().max()) == 0.0
    qd.sum().backward()
    g = W.grad
    assert float(g[D:2 * D].abs().max()) == 0.0 and float(g[:D].abs().max()) > 0 and float(g[2 * D].abs().max()) > 0


def test_torch_ops_shim_registers_every_op():
    """libsemicrf_torch.so (LibTorch stable ABI, csrc/torch_ops.cpp) registers the compute entry points of the C ABI as
    torch.ops.semicrf.*: the CRF ops for the dispatch keys CUDA (HIP kernels) and CPU (the shim's own host kernels), the
    scorer / gather / segment ops for CUDA only (a CPU tensor fails in the dispatcher; nothing falls back across devices)."""
    import torch
    from transkun_amd import _lib
    ops = _lib.ops()
    for name in ("logz_fwd", "logz_bwd", "beta", "viterbi", "eval_path", "eval_path_bwd", "interval_score_fwd",
                 "interval_score_bwd_ws", "interval_score_bwd_fused_ws", "interval_score_path_bwd",
                 "interval_features_gather", "interval_features_gather_bwd"):
        assert hasattr(ops, name), name
    s = torch.zeros(4, 4, 2); n = torch.zeros(3, 2)
    lz = torch.full((2,), float("nan"))
    ops.logz_fwd(s, n, lz, torch.zeros(4, 2), True, torch.zeros(0, dtype=torch.uint8))
    # all-zero scores: logZ = log(number of segmentations weighted by 2 per frame) -- finite, equal for both chains
    assert bool(torch.isfinite(lz).all()) and float(lz[0]) == float(lz[1])
    with pytest.raises(NotImplementedError):
        ops.interval_score_fwd(torch.zeros(2, 4, 8), torch.zeros(2, 4, 8), torch.zeros(2, 4), torch.zeros(2, 4), 2, 4, 8, 8, 8, 1, 0, 1.0, 0, 0, 2, 2,
                               torch.zeros(4, 4, 2), torch.zeros(3, 2))


def test_workgroup_role_map_is_a_permutation():
    """The sweeps deal roles by workgroup index (rings of one 32-chain panel group on one XCD): for every launch shape the map
    must hit every ticket exactly once, and the rings of a panel group must share their index modulo 8 when they fit."""
    from transkun_amd import _lib
    lib = _lib.load()
    for n_spine, grid in [(88, 256), (90, 256), (22, 256), (12, 40), (5, 256), (128, 256), (1, 9), (3, 7), (64, 100), (88, 88), (2, 2),
                          (23, 256), (75, 256), (128, 304)]:
        t = [lib.semicrf_debug_wg_ticket(n_spine, grid, b) for b in range(grid)]
        assert sorted(t) == list(range(grid)), (n_spine, grid)
        where = {tk: b for b, tk in enumerate(t)}
        if t != list(range(grid)):                           # the XCD-aware map is in force
            for g in range((n_spine + 7) // 8):
                xs = {where[sg] % 8 for sg in range(8 * g, min(8 * g + 8, n_spine))}
                assert len(xs) == 1, (n_spine, grid, g, xs)


@pytest.mark.parametrize("src", ["proj_gemm.hip", "scorer_bwd_gemm.hip"])
def test_no_register_copies_ahead_of_the_lds_waits(src):
    """The matrix-core kernels issue their LDS reads through inline asm and wait for them in a later asm statement; a compiler copy
    of a destination register between the two reads stale data (tools/check_asm_waits.py: the failure, seen on proj_gemm.hip in round
    4, depends on timing and passes small tests).  The generated gfx950 assembly must show none, nor a select on a stale SCC."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("check_asm_waits", os.path.join(root, "tools", "check_asm_waits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    text = mod.compile_to_asm(os.path.join(root, "transkun_amd", "csrc", src), [])
    assert mod.check(text, src) == 0


def test_documented_persist_variants_compile():
    """tools/README.md tells people which variants of persist.hip to build (`python tools/mkvar.py NAME DEFINE ...`); a recipe
    that no longer compiles is a rotten document (one did: a later static_assert ruled its geometry out and nobody noticed).  Every
    recipe listed there goes through the compiler's front end -- host and device pass, static_asserts included -- with the release
    flags; all of them at once.  The list is read from the README: it exists nowhere else."""
    import subprocess
    from transkun_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "tools", "README.md")) as f:
        recipes = re.findall(r"^\* `python tools/mkvar\.py (\w+)((?: \w+=\w+)+)`", f.read(), re.M)
    variants = {name: defs.split() for name, defs in recipes}
    assert len(variants) == len(recipes) >= 5, recipes
    for must in (["SEMICRF_DEBUG_BUILD=1"], ["SEMICRF_PANEL_PROBES=1", "SEMICRF_CT_DBG=16"], ["SEMICRF_PANEL_PROBES=1", "SEMICRF_PROBE_TASKS=1"],
                 ["SEMICRF_PANEL_PROBES=1", "SEMICRF_PROBE_HIST=1"], ["SEMICRF_BANDX=0"]):
        assert must in variants.values(), must
    src = os.path.join(_build.CSRC, "persist.hip")
    flags = ["--offload-arch=" + _build.ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-Wall",
             "-Wno-unused-function"] + _build.EXTRA_FLAGS["persist.hip"]
    procs = {name: subprocess.Popen([_build._hipcc()] + flags + ["-D" + d for d in defs] + ["-fsyntax-only", src],
                                    stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for name, defs in variants.items()}
    status = {name: (p.communicate(), p.returncode)[1] for name, p in procs.items()}
    assert all(rc == 0 for rc in status.values()), status


def test_documented_scorer_variants_compile():
    """The sibling of test_documented_persist_variants_compile for the scorer, projection and limb-split code: every recipe that
    tools/README.md lists as `python tools/mkvar.py NAME --files a.hip[,b.hip] DEFINE=V ...` goes through the compiler's front
    end (host and device pass, release flags), every named file of every recipe at once.  The probe builds that the scripts in
    tools/ drive have to be among them."""
    import subprocess
    from transkun_amd import _build
    with open(os.path.join(ROOT, "tools", "README.md")) as f:
        recipes = re.findall(r"^\* `python tools/mkvar\.py (\w+) --files ([\w.,]+)((?: \w+=\w+)+)`", f.read(), re.M)
    variants = {name: (files.split(","), defs.split()) for name, files, defs in recipes}
    assert len(variants) == len(recipes) >= 5, recipes
    for must in ((["scorer_mfma.hip"], ["SEMICRF_SCORE_PROBE=1"]), (["scorer_tiled.hip"], ["SEMICRF_TILED_PROBE=1"]),
                 (["scorer_bwd_gemm.hip"], ["SEMICRF_G3_PROBE=1"]), (["proj_gemm3.hip"], ["SEMICRF_P3_PROBE=1"])):
        assert must in variants.values(), must
    assert any(files == ["scorer_bwd_gemm.hip"] and any(d.startswith("SEMICRF_G3_ABL=") for d in defs) for files, defs in variants.values())
    flags = ["--offload-arch=" + _build.ARCH, "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", "-ffp-contract=off", "-Wall",
             "-Wno-unused-function"]
    procs = {}
    for name, (files, defs) in variants.items():
        for base in files:
            src = os.path.join(_build.CSRC, base)
            assert os.path.exists(src), (name, base)
            procs[name, base] = subprocess.Popen([_build._hipcc()] + flags + _build.EXTRA_FLAGS.get(base, []) + ["-D" + d for d in defs]
                                                 + ["-fsyntax-only", src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    status = {key: (p.communicate(), p.returncode)[1] for key, p in procs.items()}
    assert all(rc == 0 for rc in status.values()), status


# interval_score_fwd's kernel choice, recorded from the commit before the route became one function (b09adaa): its launcher
# compiled with the kernel launches stubbed to name the kernel, release and debug flags.  Key: (C, T, D, ldq = ldk, bases 16-byte
# aligned, prec, group, pitch, row constant, forced variant, impl); value: (release library, debug library) in
# semicrf_debug_score_route's numbering -- 0 register loads, 1 plain, 2 tiled, 3 three-limb, 32 streaming, 64 / 128 the reference
# tiles, -1 refused.  ld = 2097160 at T = 256: T * ld * 4 >= 2^31 with ld % 4 == 0.
_SCORE_ROUTES = {
    (4, 256, 32, 32, 1, 0, 4, 4, 0, -1, 0): (1, 1),
    (4, 256, 64, 64, 1, 0, 4, 4, 0, -1, 1): (1, 1),
    (4, 256, 64, 129, 1, 0, 4, 4, 0, -1, 0): (0, 0),
    (4, 256, 64, 2097160, 1, 0, 4, 4, 0, -1, 0): (0, 0),
    (4, 256, 64, 64, 0, 0, 4, 4, 0, -1, 0): (0, 0),
    (4, 100, 64, 64, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 100, 64, 64, 1, 1, 4, 4, 0, -1, 0): (32, 32),
    (4, 128, 64, 64, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 128, 64, 64, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 128, 256, 256, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 128, 320, 320, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 128, 320, 320, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 255, 64, 64, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 255, 64, 64, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 255, 320, 320, 1, 0, 4, 4, 0, -1, 0): (32, 32),
    (4, 255, 320, 320, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 256, 64, 64, 1, 0, 4, 4, 0, -1, 0): (2, 2),
    (4, 256, 64, 64, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 256, 256, 256, 1, 0, 4, 4, 0, -1, 0): (2, 2),
    (4, 256, 320, 320, 1, 0, 4, 4, 0, -1, 0): (0, 128),
    (4, 256, 320, 320, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 691, 64, 64, 1, 0, 4, 4, 0, -1, 0): (2, 2),
    (4, 691, 64, 64, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 691, 320, 320, 1, 0, 4, 4, 0, -1, 0): (0, 64),
    (4, 691, 320, 320, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 1024, 64, 64, 1, 0, 4, 4, 0, -1, 0): (2, 2),
    (4, 1024, 64, 64, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (4, 1024, 256, 256, 1, 0, 4, 4, 0, -1, 0): (2, 2),
    (4, 1024, 320, 320, 1, 0, 4, 4, 0, -1, 0): (0, 128),
    (4, 1024, 320, 320, 1, 1, 4, 4, 0, -1, 0): (3, 3),
    (16384, 1024, 64, 64, 1, 0, 16384, 16384, 0, -1, 0): (0, 128),
    (4, 256, 32, 32, 1, 0, 2, 4, 0, -1, 0): (-1, -1),
    (4, 256, 64, 64, 1, 0, 2, 4, 0, -1, 1): (-1, -1),
    (4, 256, 64, 129, 1, 0, 2, 4, 0, -1, 0): (-1, -1),
    (4, 256, 64, 2097160, 1, 0, 2, 4, 0, -1, 0): (-1, -1),
    (4, 256, 64, 64, 0, 0, 2, 4, 0, -1, 0): (-1, -1),
    (4, 100, 64, 64, 1, 0, 2, 4, 0, -1, 0): (-1, -1),
    (4, 100, 64, 64, 1, 1, 2, 4, 0, -1, 0): (-1, -1),
    (4, 128, 64, 64, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 128, 64, 64, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 128, 256, 256, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 128, 320, 320, 1, 0, 2, 4, 0, -1, 0): (-1, 128),
    (4, 128, 320, 320, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 255, 64, 64, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 255, 64, 64, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 255, 320, 320, 1, 0, 2, 4, 0, -1, 0): (-1, 128),
    (4, 255, 320, 320, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 256, 64, 64, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 256, 64, 64, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 256, 256, 256, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 256, 320, 320, 1, 0, 2, 4, 0, -1, 0): (-1, 128),
    (4, 256, 320, 320, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 691, 64, 64, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 691, 64, 64, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 691, 320, 320, 1, 0, 2, 4, 0, -1, 0): (-1, 64),
    (4, 691, 320, 320, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 1024, 64, 64, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 1024, 64, 64, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 1024, 256, 256, 1, 0, 2, 4, 0, -1, 0): (2, 2),
    (4, 1024, 320, 320, 1, 0, 2, 4, 0, -1, 0): (-1, 128),
    (4, 1024, 320, 320, 1, 1, 2, 4, 0, -1, 0): (3, 3),
    (4, 100, 64, 64, 1, 0, 4, 4, 1, -1, 0): (-1, -1),
    (4, 128, 64, 64, 1, 0, 4, 4, 1, -1, 0): (2, 2),
    (4, 256, 64, 64, 1, 0, 4, 4, 1, -1, 0): (2, 2),
    (4, 691, 320, 320, 1, 0, 4, 4, 1, -1, 0): (-1, 64),
    (4, 100, 64, 64, 1, 0, 4, 4, 0, 0, 0): (0, 0),
    (4, 128, 64, 64, 1, 0, 4, 4, 0, 0, 0): (0, 0),
    (4, 256, 64, 64, 1, 0, 4, 4, 0, 0, 0): (0, 0),
    (4, 1024, 64, 64, 1, 0, 4, 4, 0, 0, 0): (0, 0),
    (4, 256, 64, 64, 1, 1, 4, 4, 0, 0, 0): (3, 3),
    (4, 256, 64, 64, 1, 0, 2, 4, 0, 0, 0): (-1, 128),
    (4, 1024, 320, 320, 1, 0, 4, 4, 0, 0, 0): (0, 0),
    (4, 100, 64, 64, 1, 0, 4, 4, 0, 2, 0): (0, 128),
    (4, 128, 64, 64, 1, 0, 4, 4, 0, 2, 0): (2, 2),
    (4, 256, 64, 64, 1, 0, 4, 4, 0, 2, 0): (2, 2),
    (4, 1024, 64, 64, 1, 0, 4, 4, 0, 2, 0): (2, 2),
    (4, 256, 64, 64, 1, 1, 4, 4, 0, 2, 0): (3, 3),
    (4, 256, 64, 64, 1, 0, 2, 4, 0, 2, 0): (2, 2),
    (4, 1024, 320, 320, 1, 0, 4, 4, 0, 2, 0): (0, 128),
    (4, 100, 64, 64, 1, 0, 4, 4, 0, 32, 0): (32, 32),
    (4, 128, 64, 64, 1, 0, 4, 4, 0, 32, 0): (32, 32),
    (4, 256, 64, 64, 1, 0, 4, 4, 0, 32, 0): (32, 32),
    (4, 1024, 64, 64, 1, 0, 4, 4, 0, 32, 0): (32, 32),
    (4, 256, 64, 64, 1, 1, 4, 4, 0, 32, 0): (3, 3),
    (4, 256, 64, 64, 1, 0, 2, 4, 0, 32, 0): (-1, 128),
    (4, 1024, 320, 320, 1, 0, 4, 4, 0, 32, 0): (32, 32),
}


def test_scorer_forward_routes_without_gpu():
    """plan_score_route through semicrf_debug_score_route: one row per line of the route table (naive for D % 64 != 0 and impl != 0,
    register loads for rows that are not addressable, streaming below 128 / 256 frames, the tiled kernel, the three-limb kernel,
    what the release library refuses with a slot layout or a row constant and the debug library gives to its reference tiles, the
    32 T Cs limit at C = 16384, every forced variant)."""
    from transkun_amd import _lib
    libs = (_lib.load(), _lib.load_debug())
    assert set(v for pair in _SCORE_ROUTES.values() for v in pair) == {-1, 0, 1, 2, 3, 32, 64, 128}
    for key, want in _SCORE_ROUTES.items():
        C, T, D, ld, aligned, prec, group, pitch, rowc, forced, impl = key
        got = tuple(lib.semicrf_debug_score_route(C, T, D, ld, ld, aligned, prec, group, pitch, rowc, forced, impl) for lib in libs)
        assert got == want, (key, got, want)
    # a shape the entry points would refuse before they ask: no crash, "refused"
    assert libs[0].semicrf_debug_score_route(4, 256, 64, 64, 64, 1, 0, 3, 4, 0, -1, 0) == -1
    # the forced variant is an argument: the query neither reads nor changes the process-wide hook
    assert libs[0].semicrf_debug_score_route(4, 1024, 64, 64, 64, 1, 0, 4, 4, 0, -1, 0) == 2
