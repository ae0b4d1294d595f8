#!/usr/bin/env python
"""Generate tests/golden/gemini_ref.npz by running the REFERENCE's own Gemini_DF_ResNet60 / 114 / 237 modules
(wespeaker/models/gemini_dfresnet.py, imported through oracle.ref_shim) on the synthetic weights of fixtures/synth.py.
Needs the reference checkout (WESPEAKER_REFERENCE); writes embeddings only -- weights and inputs are regenerated from
their seeds by the tests (golden_cases below is what they import).

The module is run in float64 (`.double()`): the file pins what the reference's code computes, not the rounding noise
of one fp32 summation order.

    python tools/make_golden_gemini.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fixtures import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "gemini_ref.npz")
G60, G114, G183, G237 = ("Gemini_DF_ResNet%d" % n for n in (60, 114, 183, 237))


def narrow_feats(T, F):
    """The narrow cases' input: (2, T, F) random features."""
    return np.random.RandomState(T).randn(2, T, F).astype(np.float32)


def golden_cases():
    """key -> (model name, constructor arguments of the reference, features (B, T, F))."""
    from oracle.fbank import speaker_features
    feats = np.stack([speaker_features(synth.synth_wav(i)) for i in range(2)])
    wide = dict(feat_dim=80, embed_dim=256)
    return {
        G60 + "/emb": (G60, wide, feats),
        G60 + "/emb_T57": (G60, wide, feats[:, :57].copy()),
        G60 + "_f32/emb_T33": (G60, dict(feat_dim=32, embed_dim=32), narrow_feats(33, 32)),     # F: 32, 16, 8, 4, 2
        G60 + "_f16/emb_T9": (G60, dict(feat_dim=16, embed_dim=256), narrow_feats(9, 16)),      # the final F is 1
        G60 + "_two/emb_T57": (G60, dict(wide, two_emb_layer=True), feats[:, :57].copy()),
        G114 + "/emb_T57": (G114, wide, feats[:1, :57].copy()),
        G237 + "/emb_T57": (G237, wide, feats[:1, :57].copy()),
    }


def case_state_dict(name, args):
    return synth.synth_gemini_state_dict(name, args["feat_dim"], args["embed_dim"],
                                         two_emb_layer=args.get("two_emb_layer", False), seed=42)


def ref_model(name, args, sd, dtype=torch.float64):
    from oracle import ref_shim
    mod = ref_shim.ref_module("wespeaker.models.gemini_dfresnet")
    model = getattr(mod, name)(**args)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()
    if dtype == torch.float64:
        model.double()
    return model


def ref_forward(name, args, sd, feats, dtype=torch.float64):
    """The last element of the module's tuple: (tensor(0.), embed_a) or (embed_a, embed_b)."""
    with torch.no_grad():
        return ref_model(name, args, sd, dtype)(torch.from_numpy(np.array(feats)).to(dtype))[-1].numpy()


def main():
    out = {}
    for key, (name, args, feats) in golden_cases().items():
        out[key] = ref_forward(name, args, case_state_dict(name, args), feats)
        print(key, out[key].shape, float(np.abs(out[key]).mean()))
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")


if __name__ == "__main__":
    main()
