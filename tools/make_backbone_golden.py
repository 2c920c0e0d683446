#!/usr/bin/env python3
"""Generate tests/golden/backbone_*.npz by running the REFERENCE's Backbone itself (torch, CPU), in fp32 and in float64.

Run where the reference checkout is available:
    PYTHONDONTWRITEBYTECODE=1 python tools/make_backbone_golden.py --reference <path to the reference checkout>
(or TRANSKUN_REFERENCE=<path>).  The reference is imported at run time; the fixtures hold data only: the seeded state_dict, the
inputs, and the reference's outputs.

Per fixture (all arrays; `sd/<name>` are the state_dict entries; a fixture that would exceed PART_BYTES is cut into
NAME.npz, NAME.part1.npz, ... -- tests/backbone_common.py reads them back as one):
    cfg_*                       the constructor arguments
    qk_factor                   what the q and k projection weights were multiplied by (below)
    x, outputIndices            Backbone input [N, T, F, nWin], the P output indices
    out32, out64                Backbone output of the fp32 module and of its float64 copy
    layer_in                    the input of encoderLayers[0] as the fp32 run saw it [N, T', F' + P, D]; layer_mem: a seeded memory
    block_out32/64              encoderLayers[0](layer_in);  block_mem_out32/64: encoderLayers[0](layer_in, layer_mem)
    mha_key                     a seeded key of another length [N, T', Lk, D]
    mha_out32/64                encoderLayers[0].mhaBlockF.module(layer_in);  mha_mem_out32/64: (layer_in, mha_key)

Default initialisation would make the fixtures blind to the attention (LayerScale 1e-2, logits near zero), so before evaluating every
`scale` is overwritten with seeded values in [0.5, 1.5] and the q and k projection weights are multiplied by QK_FACTOR, which brings
the softmax off uniform.

The float64 run is a `.double()` copy of the reference module; the reference hard-codes `.float()` on the position coordinates, so
a forward pre-hook on the three position embeddings' `proj` casts their input (integers: exact in both types).
"""
from __future__ import annotations

import argparse
import copy
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
PART_BYTES = 900 * 1024                       # a committed file stays below 1 MiB
QK_FACTOR = 2.0

# the model's own ratios (ModelConfig): hiddenFactor 4, hiddenFactorAttn 1, scoringExpansionFactor 4, posEmbedInitGamma 1
COMMON = dict(inputSize=6, posEmbedInitGamma=1, fourierSize=64, hiddenFactor=4, hiddenFactorAttn=1, expansionFactor=4, dropoutProb=0.1,
              enabledAttn=["F", "T"], useGradientCheckpoint=False, downsampleF=True)
CASES = {
    "backbone_small": dict(cfg=dict(COMMON, baseSize=8, nHead=2, nLayers=2), x=(2, 21, 37, 6), P=5, seed=101),
    "backbone_d40": dict(cfg=dict(COMMON, baseSize=20, nHead=2, nLayers=1), x=(2, 19, 30, 6), P=7, seed=202),
}


def import_reference(path):
    sys.dont_write_bytecode = True
    sys.path.insert(0, path)
    from transkun import LayersTransformer            # noqa: E402
    return LayersTransformer


def to_double(module):
    m = copy.deepcopy(module).double()
    for name in ("posEmbedBuilder", "posEmbedBuilderAttnTF", "posEmbedBuilderAttnTE"):
        getattr(m, name).proj.register_forward_pre_hook(lambda mod, args: (args[0].double(),))
    return m


def run_case(LT, name, spec):
    g = torch.Generator().manual_seed(spec["seed"])
    torch.manual_seed(spec["seed"])
    ref = LT.Backbone(**spec["cfg"]).eval()
    with torch.no_grad():
        for pname, p in ref.named_parameters():
            if pname.endswith(".scale"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            if pname.endswith(("q_proj_weight", "k_proj_weight")):
                p.mul_(QK_FACTOR)
    ref64 = to_double(ref)
    x = torch.randn(*spec["x"], generator=g)
    idx = torch.arange(spec["P"])
    seen = {}
    hook = ref.encoderLayers[0].register_forward_pre_hook(lambda mod, args: seen.setdefault("layer_in", args[0].detach().clone()))
    with torch.no_grad():
        out32 = ref(x, idx)
        hook.remove()
        out64 = ref64(x.double(), idx)
        lin = seen["layer_in"]
        mem = torch.randn(lin.shape, generator=g)
        key = torch.randn(*lin.shape[:2], 11, lin.shape[-1], generator=g)
        blk, blk64 = ref.encoderLayers[0], ref64.encoderLayers[0]
        mha, mha64 = blk.mhaBlockF.module, blk64.mhaBlockF.module
        arrays = {
            "x": x, "outputIndices": idx, "out32": out32, "out64": out64, "layer_in": lin, "layer_mem": mem, "mha_key": key,
            "block_out32": blk(lin), "block_out64": blk64(lin.double()),
            "block_mem_out32": blk(lin, mem), "block_mem_out64": blk64(lin.double(), mem.double()),
            "mha_out32": mha(lin), "mha_out64": mha64(lin.double()),
            "mha_mem_out32": mha(lin, key), "mha_mem_out64": mha64(lin.double(), key.double()),
        }
    arrays = {k: v.numpy() for k, v in arrays.items()}
    arrays["qk_factor"] = np.float64(QK_FACTOR)
    for k, v in spec["cfg"].items():
        arrays["cfg_" + k] = np.array(v)
    weights = {"sd/" + k: v.numpy() for k, v in ref.state_dict().items()}
    e32 = float(np.abs(out32.double().numpy() - arrays["out64"]).max())
    print(f"{name}: out {tuple(out32.shape)} |out| max {float(out32.abs().max()):.3f}  reference fp32 error {e32:.3e}  "
          f"state_dict {sum(v.nbytes for v in weights.values()) / 1e6:.2f} MB")
    # cut into parts below PART_BYTES (the data is incompressible): the inputs and outputs first, then the weights by name
    entries = list(arrays.items()) + sorted(weights.items())
    parts, cur, size = [], {}, 0
    for k, v in entries:
        if size + v.nbytes > PART_BYTES and cur:
            parts.append(cur); cur, size = {}, 0
        cur[k] = v; size += v.nbytes
    parts.append(cur)
    for stale in glob.glob(os.path.join(OUT, name + ".part*.npz")):
        os.remove(stale)
    for i, part in enumerate(parts):
        path = os.path.join(OUT, name + (".npz" if i == 0 else f".part{i}.npz"))
        np.savez_compressed(path, **part)
        print(f"  {os.path.relpath(path, ROOT)}: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("TRANSKUN_REFERENCE"), help="path to the reference checkout")
    ap.add_argument("cases", nargs="*", default=list(CASES))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or TRANSKUN_REFERENCE) is required")
    LT = import_reference(args.reference)
    for name in args.cases:
        run_case(LT, name, CASES[name])


if __name__ == "__main__":
    main()
