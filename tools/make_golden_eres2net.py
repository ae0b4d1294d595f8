#!/usr/bin/env python
"""Generate tests/golden/eres2net_ref.npz by running the REFERENCE's own ERes2Net34_Base / _Large / _aug modules
(wespeaker/models/eres2net.py, imported through oracle.ref_shim) on the synthetic weights of fixtures/synth.py.
Needs the reference checkout (WESPEAKER_REFERENCE); writes embeddings only -- weights and inputs are regenerated from
their seeds by the tests (golden_cases below is what they import).

The module is run in float64 (`.double()`): the file pins what the reference's code computes, not the rounding noise
of one fp32 summation order.

    python tools/make_golden_eres2net.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fixtures import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "eres2net_ref.npz")
BASE, LARGE, AUG = "ERes2Net34_Base", "ERes2Net34_Large", "ERes2Net34_aug"


def narrow_feats():
    """The narrow case's input: (2, 37, 24) random features."""
    return np.random.RandomState(37).randn(2, 37, 24).astype(np.float32)


def golden_cases():
    """key -> (model name, constructor arguments of the reference, features (B, T, F))."""
    from oracle.fbank import speaker_features
    feats = np.stack([speaker_features(synth.synth_wav(i)) for i in range(2)])
    wide = dict(feat_dim=80, embed_dim=192)
    return {
        BASE + "/emb": (BASE, wide, feats),
        BASE + "/emb_T57": (BASE, wide, feats[:, :57].copy()),
        BASE + "_f24/emb_T37": (BASE, dict(feat_dim=24, embed_dim=32), narrow_feats()),
        BASE + "_two/emb_T57": (BASE, dict(wide, two_emb_layer=True), feats[:, :57].copy()),
        LARGE + "/emb_T57": (LARGE, wide, feats[:1, :57].copy()),
        AUG + "/emb_T33": (AUG, wide, feats[:1, :33].copy()),
    }


def case_state_dict(name, args):
    return synth.synth_eres2net_state_dict(name, args["feat_dim"], args["embed_dim"],
                                           two_emb_layer=args.get("two_emb_layer", False), seed=42)


def ref_model(name, args, sd, dtype=torch.float64):
    from oracle import ref_shim
    mod = ref_shim.ref_module("wespeaker.models.eres2net")
    model = getattr(mod, name)(**args)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()
    if dtype == torch.float64:
        model.double()
    return model


def ref_forward(name, args, sd, feats, dtype=torch.float64):
    with torch.no_grad():
        return ref_model(name, args, sd, dtype)(torch.from_numpy(np.asarray(feats)).to(dtype)).numpy()


def main():
    out = {}
    for key, (name, args, feats) in golden_cases().items():
        out[key] = ref_forward(name, args, case_state_dict(name, args), feats)
        print(key, out[key].shape, float(np.abs(out[key]).mean()))
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")


if __name__ == "__main__":
    main()
