#!/usr/bin/env python
"""Generate tests/golden/tdnn_ref.npz by running the REFERENCE's own XVEC / XI_VEC_XVEC / XI_VEC_ECAPA_TDNN_c512 / _c1024
modules (wespeaker/models/tdnn.py, xi_vector.py, ecapa_tdnn.py, imported through oracle.ref_shim) on the seeded
synthetic weights below.  Needs the reference checkout (WESPEAKER_REFERENCE); writes embeddings only -- weights and
inputs are regenerated from their seeds by the tests (golden_cases below is what they import).

The module is run in float64 (`.double()`): the file pins what the reference's code computes, not the rounding noise
of one fp32 summation order.

    python tools/make_golden_tdnn.py
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fixtures import synth  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "tdnn_ref.npz")
XVEC, XI_XVEC, XI_C512, XI_C1024 = "XVEC", "XI_VEC_XVEC", "XI_VEC_ECAPA_TDNN_c512", "XI_VEC_ECAPA_TDNN_c1024"
XI_HIDDEN = 256                     # pooling_layers.py:345
TAPS = (5, 3, 3, 1, 1)              # tdnn.py:74-81
DILATIONS = (1, 2, 3, 1, 1)


class _Gen:
    """Seeded weights: every running_var positive, every running_mean non-zero (an identity BN would hide a dropped one)."""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.sd = OrderedDict()

    def conv(self, name, cout, cin, k=None, gain=2.0, bias_std=0.1):
        shape = (cout, cin) if k is None else (cout, cin, k)
        std = np.sqrt(gain / (cin * (k or 1)))
        self.sd[name + ".weight"] = (std * self.rng.standard_normal(shape)).astype(np.float32)
        self.sd[name + ".bias"] = (bias_std * self.rng.standard_normal(cout)).astype(np.float32)

    def bn(self, name, c, affine=True):
        if affine:
            self.sd[name + ".weight"] = self.rng.uniform(0.8, 1.2, c).astype(np.float32)
            self.sd[name + ".bias"] = (0.1 * self.rng.standard_normal(c)).astype(np.float32)
        sign = self.rng.choice([-1.0, 1.0], c)
        self.sd[name + ".running_mean"] = (sign * self.rng.uniform(0.05, 0.3, c)).astype(np.float32)
        self.sd[name + ".running_var"] = self.rng.uniform(0.5, 1.5, c).astype(np.float32)
        self.sd[name + ".num_batches_tracked"] = np.array(1000, dtype=np.int64)

    def xi(self, prefix, dim):
        """XI's parameters in the module's order (pooling_layers.py:354-367).  lin2 is wide (z ~ N(0, 40^2)), so that z
        reaches all three regimes of softplus -> log -> clamp: below -7.5 (clamped to -15; below -104 the float32
        softplus underflows to 0), between -7.5 and 20, above 20 (softplus' threshold branch).  prior_logprec is drawn
        around the log of the frame weights' sum, so that the prior pseudo-frame is neither negligible nor dominant."""
        self.sd[prefix + ".prior_mean"] = (0.5 * self.rng.standard_normal((1, dim))).astype(np.float32)
        self.sd[prefix + ".prior_logprec"] = self.rng.uniform(8.0, 12.5, (1, dim)).astype(np.float32)
        self.conv(prefix + ".lin1_relu_bn.0", XI_HIDDEN, dim, 1)
        self.bn(prefix + ".lin1_relu_bn.2", XI_HIDDEN)
        self.conv(prefix + ".lin2", dim, XI_HIDDEN, 1, gain=1600.0, bias_std=10.0)


def synth_xvec_state_dict(name=XVEC, feat_dim=80, embed_dim=512, hid_dim=512, stats_dim=1500, seed=42):
    g = _Gen(seed)
    for k in range(5):
        p = "frame_%d" % (k + 1)
        cout, cin = (stats_dim if k == 4 else hid_dim), (feat_dim if k == 0 else hid_dim)
        g.conv(p + ".conv_1d", cout, cin, TAPS[k])
        g.bn(p + ".bn", cout, affine=False)
    if name == XI_XVEC:
        g.xi("pool", stats_dim)
    g.conv("seg_1", embed_dim, stats_dim * (1 if name == XI_XVEC else 2), gain=1.0)
    g.bn("seg_bn_1", embed_dim, affine=False)
    g.conv("seg_2", embed_dim, embed_dim, gain=1.0)
    return g.sd


def synth_xi_ecapa_state_dict(name=XI_C512, feat_dim=80, embed_dim=192, emb_bn=False, seed=42):
    """The ECAPA trunk of fixtures/synth.py (its pooling, bn and linear left out) + XI + bn (1536) + linear [+ bn2]."""
    trunk = synth.synth_ecapa_state_dict(name[len("XI_VEC_"):], feat_dim, embed_dim, seed=seed)
    g = _Gen(seed + 1)
    for k, v in trunk.items():
        if not k.startswith(("pool.", "bn.", "linear.", "bn2.")):
            g.sd[k] = v
    g.xi("pool", 1536)
    g.bn("bn", 1536)
    g.conv("linear", embed_dim, 1536, gain=1.0)
    if emb_bn:
        g.bn("bn2", embed_dim)
    return g.sd


def feats_for(T, F, B=2):
    return np.random.RandomState(1000 + T).randn(B, T, F).astype(np.float32)


def golden_cases():
    """key -> (model name, constructor arguments of the reference, engine extras (hid_dim, stats_dim), features)."""
    wide, narrow = dict(feat_dim=80, embed_dim=512), dict(feat_dim=40, embed_dim=64)
    eca = dict(feat_dim=80, embed_dim=192)
    cases = OrderedDict()
    for name in (XVEC, XI_XVEC):
        for T in (200, 33):
            cases["%s/emb_T%d" % (name, T)] = (name, wide, dict(hid_dim=512, stats_dim=1500), feats_for(T, 80))
        for T in (15, 16, 57):
            cases["%s_h64_s100/emb_T%d" % (name, T)] = (name, narrow, dict(hid_dim=64, stats_dim=100), feats_for(T, 40))
    for T in (9, 57, 200):
        cases["%s/emb_T%d" % (XI_C512, T)] = (XI_C512, eca, {}, feats_for(T, 80))
    cases["%s_embbn/emb_T57" % XI_C512] = (XI_C512, dict(eca, emb_bn=True), {}, feats_for(57, 80))
    cases["%s/emb_T57" % XI_C1024] = (XI_C1024, eca, {}, feats_for(57, 80, B=1))
    return cases


def case_state_dict(name, args, extra):
    if name in (XVEC, XI_XVEC):
        return synth_xvec_state_dict(name, args["feat_dim"], args["embed_dim"], seed=42, **extra)
    return synth_xi_ecapa_state_dict(name, args["feat_dim"], args["embed_dim"], emb_bn=args.get("emb_bn", False), seed=42)


def ref_model(name, args, extra, sd, dtype=torch.float64):
    """The named constructor where it builds the case (xi_vector.py:31-49, tdnn.py:57); the narrow cases go through the
    class the constructors call, with the same pooling_func."""
    from oracle import ref_shim
    if name in (XVEC, XI_XVEC):
        mod = ref_shim.ref_module("wespeaker.models.tdnn")
        pooling = "XI" if name == XI_XVEC else "TSTP"
        if extra.get("hid_dim", 512) == 512 and extra.get("stats_dim", 1500) == 1500 and name == XI_XVEC:
            model = ref_shim.ref_module("wespeaker.models.xi_vector").XI_VEC_XVEC(**args)
        else:
            model = mod.XVEC(pooling_func=pooling, **dict(args, **extra))
    else:
        model = getattr(ref_shim.ref_module("wespeaker.models.xi_vector"), name)(**args)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()
    if dtype == torch.float64:
        model.double()
    return model


def ref_forward(name, args, extra, sd, feats, dtype=torch.float64):
    """The last element of the module's tuple: (embed_a, embed_b) for XVEC, (out, embed) for ECAPA."""
    with torch.no_grad():
        return ref_model(name, args, extra, sd, dtype)(torch.from_numpy(np.array(feats)).to(dtype))[-1].numpy()


def main():
    out = {}
    for key, (name, args, extra, feats) in golden_cases().items():
        out[key] = ref_forward(name, args, extra, case_state_dict(name, args, extra), feats)
        print(key, out[key].shape, float(np.abs(out[key]).mean()))
    np.savez_compressed(GOLD, **out)
    print("wrote", GOLD, os.path.getsize(GOLD), "bytes")


if __name__ == "__main__":
    main()
