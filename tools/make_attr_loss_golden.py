#!/usr/bin/env python3
"""Generate tests/golden/attr_loss_small.npz by running the REFERENCE's training loss itself (torch CPU).

Run where the reference checkout is available (as tools/make_golden.py): `PYTHONDONTWRITEBYTECODE=1 python tools/make_attr_loss_golden.py`.

TransKun.log_prob (ModelTransformer.py:228-332), .fetchIntervalFeaturesBatch (:501-532) and Data.prepareIntervals are lifted out
of the reference's source files with ast at run time (the module cannot be imported: pretty_midi / torchaudio / moduleconf are
absent) and run unchanged; makeFrame and processFramesBatch are stubbed to hand over a hash-generated ctx and the reference's own
CRF on the reference's own scorer.  Nothing of the reference's text is stored: the fixture holds numbers only.

Inputs (ctx, the scorer's and the heads' weights) come from transkun_amd.synth's integer hash through
tests/attr_loss_common.py:golden_inputs and are NOT stored; the notes are derived from synth.synthetic_intervals.  Stored:
  pairs, offsets, velocity, ofRefined, ofPresence       the targets as prepareIntervals produced them (chain order)
  logitsVelocity [K,128], ofLogits [K,4]                the heads' raw outputs (fp32)
  lpVel, lpOF, lpPres [K]; attr [C]; crf [N,P]; logProb [N,P]        the reference's fp32 results (attr = logProb - crf, per chain)
  dLogitsVelocity, dOfLogits                            autograd's gradients of -logProb.sum(-1).mean() w.r.t. the raw outputs
  *64                                                   the same expressions evaluated in float64 on the stored raw outputs
"""
from __future__ import annotations

import ast
import os
import sys
import types
from collections import defaultdict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REFERENCE = os.environ.get("TRANSKUN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REFERENCE, "transkun"))
sys.path.insert(0, REFERENCE)
sys.dont_write_bytecode = True

import CRF as REF  # noqa: E402  (the reference package)
from transkun_amd import synth  # noqa: E402
import attr_loss_common as common  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "attr_loss_small.npz")


def lift(ns, path, names, kinds=(ast.FunctionDef, ast.ClassDef)):
    tree = ast.parse(open(path).read())
    found = {}
    for node in ast.walk(tree):
        if isinstance(node, kinds) and node.name in names and node.name not in found:
            found[node.name] = node
    assert set(found) == set(names), (names, list(found))
    exec(compile(ast.Module(body=[found[n] for n in names], type_ignores=[]), path, "exec"), ns)


def make_notes(ns, c):
    """Per segment a list of the reference's Note objects whose quantisation gives synth.synthetic_intervals' frames: the
    refinements (|r| <= 0.45 frames) and the presence flags come from the hash as well."""
    N, P, T, hop, fs = c["N"], c["P"], c["T"], c["hop"], c["fs"]
    iv = synth.synthetic_intervals(T, N * P, seed=c["seed"], every=6, active_every=2)
    h = synth.hash_u64_numpy(np.arange(N * P * T * 4, dtype=np.uint64), c["seed"] + 1).reshape(N * P, T, 4)
    sec = hop / fs
    batch = []
    for n in range(N):
        notes = []
        for p in range(P):
            prev = None                                                             # (end frame, its refinement) of the pitch's last note
            for k, (b, e) in enumerate(iv[n * P + p]):
                r0 = (int(h[n * P + p, k, 0] % np.uint64(901)) - 450) / 1000.0
                r1 = (int(h[n * P + p, k, 1] % np.uint64(901)) - 450) / 1000.0
                if b == 0:
                    r0 = abs(r0)
                if prev is not None and prev[0] == b:
                    r0 = max(r0, prev[1])                                           # touching notes: no overlap in time
                if e == b:
                    r1 = max(r1, r0)
                prev = (e, r1)
                note = ns["Note"](start=(b + r0) * sec, end=(e + r1) * sec, pitch=c["pitches"][p], velocity=int(h[n * P + p, k, 2] % np.uint64(128)))
                note.hasOnset = bool(h[n * P + p, k, 3] % np.uint64(4))          # 3 in 4 present
                note.hasOffset = bool((h[n * P + p, k, 3] >> np.uint64(8)) % np.uint64(4))
                notes.append(note)
        batch.append(notes)
    return batch


def main():
    from transkun.LayersTransformer import ScaledInnerProductIntervalScorer
    torch.set_num_threads(4)
    c = common.GOLDEN_CASE
    N, P, T, D, H = c["N"], c["P"], c["T"], c["D"], c["H"]
    ns = {"torch": torch, "F": torch.nn.functional, "nn": torch.nn, "defaultdict": defaultdict, "np": np}
    lift(ns, os.path.join(REFERENCE, "transkun", "Data.py"), ["Note", "validateNotes", "prepareIntervals"])
    lift(ns, os.path.join(REFERENCE, "transkun", "Util.py"), ["listToIdx"])
    lift(ns, os.path.join(REFERENCE, "transkun", "ModelTransformer.py"), ["fetchIntervalFeaturesBatch", "log_prob"])
    ns["makeFrame"] = lambda x, hop, win: x                                        # the stub below ignores the frames

    ctx, W, bias, heads = common.golden_inputs("cpu")
    scorer = ScaledInnerProductIntervalScorer(D, 1)
    with torch.no_grad():
        scorer.map[0].weight.copy_(W); scorer.map[0].bias.copy_(bias)

    def head(nout, w):
        m = torch.nn.Sequential(torch.nn.Linear(3 * D, H), torch.nn.GELU(), torch.nn.Dropout(0.1), torch.nn.Linear(H, nout))
        with torch.no_grad():
            m[0].weight.copy_(w[0]); m[0].bias.copy_(w[1]); m[3].weight.copy_(w[2]); m[3].bias.copy_(w[3])
        return m.eval()

    vel, of = head(128, heads["velocity"]), head(4, heads["of"])
    rec = {}

    def keep(key):
        def hook(m, i, o):
            o.retain_grad()
            rec[key] = o
        return hook

    vel.register_forward_hook(keep("logitsVelocity"))
    of.register_forward_hook(keep("ofLogits"))

    class CrfRec:
        """The reference's CRF; remembers the two numbers log_prob derives its CRF term from (:263-265)."""
        def __init__(self, crf): self.crf = crf
        def evalPath(self, intervals):
            rec["intervals"] = intervals
            rec["path"] = self.crf.evalPath(intervals)
            return rec["path"]
        def computeLogZ(self):
            rec["logZ"] = self.crf.computeLogZ()
            return rec["logZ"]

    def processFramesBatch(framesBatch):
        S, b = scorer(ctx)
        return CrfRec(REF.NeuralSemiCRFInterval(S.flatten(-2, -1), b.flatten(-2, -1))), ctx

    prep = ns["prepareIntervals"]
    targets = []
    ns["prepareIntervals"] = lambda notes, hopSec, pitches: targets.append(prep(notes, hopSec, pitches)) or targets[-1]
    me = types.SimpleNamespace(hopSize=c["hop"], windowSize=4096, fs=c["fs"], targetMIDIPitch=c["pitches"], velocityPredictor=vel,
                               refinedOFPredictor=of, processFramesBatch=processFramesBatch)
    me.fetchIntervalFeaturesBatch = types.MethodType(ns["fetchIntervalFeaturesBatch"], me)
    x = torch.zeros(N, 16, 1)                                                        # [nBatch, nSample, nChannel]: only its batch size matters
    logProb = ns["log_prob"](me, x, make_notes(ns, c))                                  # [N, P]
    (-logProb.sum(-1).mean()).backward()

    flat = rec["intervals"]
    counts = [len(l) for l in flat]
    offsets = np.zeros(N * P + 1, np.int64); np.cumsum(counts, out=offsets[1:])
    K = int(offsets[-1])
    pairs = np.asarray([p for l in flat for p in l], np.int32).reshape(-1, 2)
    velocity = np.asarray([v for d in targets for sym in d["velocity"] for v in sym], np.int32)
    refined = np.asarray([v for d in targets for sym in d["endPointRefine"] for v in sym], np.float32).reshape(-1, 2)
    presence = np.asarray([v for d in targets for sym in d["endPointPresence"] for v in sym], np.float32).reshape(-1, 2)
    assert len(velocity) == K and refined.shape == (K, 2) and presence.shape == (K, 2)
    assert np.abs(refined).max() <= 0.5 and sum(1 for n in counts if n == 0) >= 2

    lv, ofl = rec["logitsVelocity"].detach(), rec["ofLogits"].detach()
    crf = (rec["path"] - rec["logZ"]).detach().view(N, P)
    tv, tr, tp, toff = torch.from_numpy(velocity), torch.from_numpy(refined), torch.from_numpy(presence), torch.from_numpy(offsets.astype(np.int32))

    def rows(lv_, of_, dt):
        """:290-317 in dtype dt, by the same torch calls"""
        logits = torch.nn.functional.log_softmax(lv_, dim=-1)
        a = torch.gather(logits, dim=-1, index=tv.long().unsqueeze(-1)).squeeze(-1)
        r = tr.to(dt) * 0.99 + 0.5
        ofValue, ofPres = of_.chunk(2, dim=-1)
        b = torch.distributions.ContinuousBernoulli(logits=ofValue).log_prob(r).sum(-1)
        cc = torch.distributions.Bernoulli(logits=ofPres).log_prob(tp.to(dt)).sum(-1)
        return a, b, cc

    a32, b32, c32 = rows(lv, ofl, torch.float32)
    sc = common.scatter_index(toff)
    again = crf.reshape(-1).scatter_add(-1, sc, a32 + b32 + c32).view(N, P)
    assert torch.equal(again, logProb.detach()), "the row terms recomputed outside log_prob must reproduce it bit for bit"
    attr = torch.zeros(N * P).scatter_add(-1, sc, a32 + b32 + c32)

    lv64, of64 = lv.double().requires_grad_(), ofl.double().requires_grad_()
    a64, b64, c64 = rows(lv64, of64, torch.float64)
    attr64 = torch.zeros(N * P, dtype=torch.float64).scatter_add(-1, sc, a64 + b64 + c64)
    (-(attr64.view(N, P)).sum(-1).mean()).backward()

    d = dict(meta=np.asarray([N, P, T, D, H, K]), pairs=pairs, offsets=offsets, velocity=velocity, ofRefined=refined, ofPresence=presence,
             logitsVelocity=lv.numpy(), ofLogits=ofl.numpy(), lpVel=a32.numpy(), lpOF=b32.numpy(), lpPres=c32.numpy(), attr=attr.numpy(),
             crf=crf.numpy(), logProb=logProb.detach().numpy(), dLogitsVelocity=rec["logitsVelocity"].grad.numpy(),
             dOfLogits=rec["ofLogits"].grad.numpy(), lpVel64=a64.detach().numpy(), lpOF64=b64.detach().numpy(), lpPres64=c64.detach().numpy(),
             attr64=attr64.detach().numpy(), dLogitsVelocity64=lv64.grad.numpy(), dOfLogits64=of64.grad.numpy())
    np.savez_compressed(OUT, **d)
    print(f"attr_loss_small: N={N} P={P} T={T} D={D}, K={K} intervals over {N * P} chains ({counts}), max |value logit| "
          f"{float(ofl[:, :2].abs().max()):.2f}, max |velocity logit| {float(lv.abs().max()):.2f}, {os.path.getsize(OUT)} bytes")
    print("  fp32 vs float64: rows %.2e, attr %.2e, dLogitsVelocity %.2e, dOfLogits %.2e" % (
        float(((a32 + b32 + c32).double() - (a64 + b64 + c64).detach()).abs().max()), float((attr.double() - attr64.detach()).abs().max()),
        float((rec["logitsVelocity"].grad.double() - lv64.grad).abs().max()), float((rec["ofLogits"].grad.double() - of64.grad).abs().max())))


if __name__ == "__main__":
    main()
