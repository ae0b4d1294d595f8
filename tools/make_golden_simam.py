#!/usr/bin/env python
"""Generate tests/golden/samresnet_ref.npz by running the REFERENCE's own SimAM_ResNet34_ASP / SimAM_ResNet100_ASP
modules (wespeaker/models/samresnet.py, imported through oracle.ref_shim) on the synthetic weights of
fixtures/synth.py.  Needs the reference checkout (WESPEAKER_REFERENCE); writes embeddings only -- weights and
inputs are regenerated from their seeds by the tests (golden_cases below is what they import).

The module is run in float64 (`.double()`): the file pins what the reference's code computes, not the rounding noise
of one fp32 summation order -- which reaches 5e-5 of the embedding through SimAM_ResNet100's 49 gated blocks (fp32
module against float64 module, T = 57; 3e-6 for SimAM_ResNet34 at 198 frames).

    python tools/make_golden_simam.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fixtures import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "samresnet_ref.npz")


def narrow_feats():
    """The narrow case's input: (2, 37, 24) random features."""
    return np.random.RandomState(37).randn(2, 37, 24).astype(np.float32)


def golden_cases():
    """key -> (model name, constructor arguments of the reference, features (B, T, F))."""
    from oracle.fbank import speaker_features
    feats = np.stack([speaker_features(synth.synth_wav(i)) for i in range(2)])
    wide = dict(in_planes=64, embed_dim=256, acoustic_dim=80)
    return {
        "SimAM_ResNet34_ASP/emb": ("SimAM_ResNet34_ASP", wide, feats),
        "SimAM_ResNet34_ASP/emb_T57": ("SimAM_ResNet34_ASP", wide, feats[:, :57].copy()),
        "SimAM_ResNet34_ASP_p16/emb_T37": ("SimAM_ResNet34_ASP", dict(in_planes=16, embed_dim=32, acoustic_dim=24),
                                           narrow_feats()),
        "SimAM_ResNet100_ASP/emb_T57": ("SimAM_ResNet100_ASP", wide, feats[:, :57].copy()),
    }


def case_state_dict(name, args):
    return synth.synth_simam_resnet_state_dict(name, args["acoustic_dim"], args["embed_dim"],
                                               in_planes=args["in_planes"], seed=42)


def ref_forward(name, args, sd, feats, dtype=torch.float64):
    from oracle import ref_shim
    mod = ref_shim.ref_module("wespeaker.models.samresnet")
    model = getattr(mod, name)(**args)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()
    if dtype == torch.float64:
        model.double()
    with torch.no_grad():
        return model(torch.from_numpy(np.asarray(feats)).to(dtype)).numpy()


def main():
    out = {}
    for key, (name, args, feats) in golden_cases().items():
        out[key] = ref_forward(name, args, case_state_dict(name, args), feats)
        print(key, out[key].shape, float(np.abs(out[key]).mean()))
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")


if __name__ == "__main__":
    main()
