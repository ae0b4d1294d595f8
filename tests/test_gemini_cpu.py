"""Gemini DF-ResNet on the CPU: the float64 oracle (tests/gemini_oracle.py) against the reference's own module (where the
reference checkout is present) and against the committed golden (tests/golden/gemini_ref.npz); the synthetic weight
generator's key set; the model directory round trip; the fixtures with teeth of tests/test_gpu_gemini.py.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gemini_oracle as go  # noqa: E402
import make_golden_gemini as mg  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import ref_shim  # noqa: E402

ORACLE_TOL = 1e-5          # oracle (float64) against the reference module (float64) / the golden: relative L2 per utterance
REL_TOL = 2e-4             # the GPU embedding bar (tests/test_gpu_gemini.py)
GOLD = mg.GOLD
G60 = mg.G60

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason="reference checkout not present")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def test_oracle_matches_the_committed_golden():
    gold = dict(np.load(GOLD))
    cases = mg.golden_cases()
    assert set(gold) == set(cases)
    for key, (name, args, feats) in cases.items():
        emb = go.gemini_forward(mg.case_state_dict(name, args), feats, name).numpy()
        assert emb.shape == gold[key].shape
        err = _rel(emb, gold[key])
        print(key, "%.2e" % err)
        assert err < ORACLE_TOL, (key, err)


@needs_reference
@pytest.mark.parametrize("key", [G60 + "/emb_T57", G60 + "_f16/emb_T9", G60 + "_two/emb_T57", mg.G114 + "/emb_T57"])
def test_oracle_matches_the_live_reference_module(key):
    name, args, feats = mg.golden_cases()[key]
    sd = mg.case_state_dict(name, args)
    err = _rel(go.gemini_forward(sd, feats, name).numpy(), mg.ref_forward(name, args, sd, feats))
    assert err < ORACLE_TOL, err


@needs_reference
def test_reference_in_float32_stays_well_inside_the_gpu_bar():
    """The condition under which REL_TOL says something about an fp32 engine: on every golden case the reference module
    itself, run in float32, is within REL_TOL / 4 of the golden (measured: 2e-7 .. 4e-7)."""
    gold = dict(np.load(GOLD))
    for key, (name, args, feats) in mg.golden_cases().items():
        err = _rel(mg.ref_forward(name, args, mg.case_state_dict(name, args), feats, dtype=torch.float32), gold[key])
        print(key, "%.2e" % err)
        assert err < REL_TOL / 4, (key, err)


def _expected_keys(name, two=False):
    """The module's state_dict keys, written out (gemini_dfresnet.py:66-103)."""
    bn = lambda p: [p + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]  # noqa: E731
    keys = []
    for i in range(5):
        keys += ["downsample_layers.%d.0.weight" % i] + bn("downsample_layers.%d.1" % i)
    for s, nb in enumerate(synth.GEMINI_LAYOUTS[name]):
        for b in range(nb):
            p = "stages.%d.%d" % (s, b)
            for k in (1, 2, 3):
                keys += [p + ".conv%d.weight" % k] + bn(p + ".bn%d" % k)
    keys += ["seg_1.weight", "seg_1.bias"]
    if two:
        keys += ["seg_bn_1.running_mean", "seg_bn_1.running_var", "seg_bn_1.num_batches_tracked", "seg_2.weight", "seg_2.bias"]
    return keys


@pytest.mark.parametrize("name,two,count", [(G60, False, 30 + 18 * 18 + 2), (G60, True, 30 + 18 * 18 + 7),
                                            (mg.G114, False, 30 + 36 * 18 + 2), (mg.G183, False, 30 + 59 * 18 + 2),
                                            (mg.G237, False, 30 + 77 * 18 + 2)])
def test_synthetic_key_set(name, two, count):
    sd = synth.synth_gemini_state_dict(name, 80, 256, two_emb_layer=two)
    assert list(sd) == _expected_keys(name, two)
    assert len(sd) == count
    dim = {0: 32, 1: 64, 2: 128, 3: 256}
    for s in range(4):
        assert sd["stages.%d.0.conv1.weight" % s].shape == (4 * dim[s], dim[s], 1, 1)
        assert sd["stages.%d.0.conv2.weight" % s].shape == (4 * dim[s], 1, 3, 3)           # groups = 4 dim
        assert sd["stages.%d.0.conv3.weight" % s].shape == (dim[s], 4 * dim[s], 1, 1)
    assert sd["seg_1.weight"].shape == (256, 2 * 5 * 256)
    if ref_shim.available():
        model = mg.ref_model(name, dict(feat_dim=80, embed_dim=256, two_emb_layer=two), sd, dtype=torch.float32)
        ref = model.state_dict()
        assert list(ref) == list(sd)
        assert all(tuple(ref[k].shape) == tuple(np.asarray(sd[k]).shape) for k in sd)


def test_existing_generators_are_unchanged():
    """The new generator is additive: the older families' default weight sets, by digest (recorded before it existed)."""
    import hashlib

    def digest(sd):
        m = hashlib.sha256()
        for k, v in sd.items():
            m.update(k.encode())
            m.update(np.ascontiguousarray(v).tobytes())
        return m.hexdigest()[:16]

    assert digest(synth.synth_resnet_state_dict("ResNet34")) == "c37221e9021b18a6"
    assert digest(synth.synth_ecapa_state_dict()) == "f718739c695b0fd2"
    assert digest(synth.synth_eres2net_state_dict()) == "9f4d60c9771f2d00"
    assert digest(synth.synth_campplus_state_dict()) == "19c2e5b47f16f79e"
    assert synth.synth_state_dict("Gemini_DF_ResNet60", 80, 256).keys() == synth.synth_gemini_state_dict().keys()


def test_synthetic_activations_stay_in_range():
    """O(1) through the 77 blocks of the deepest model: neither collapsed to zero nor exploding."""
    name, args, feats = mg.golden_cases()[mg.G237 + "/emb_T57"]
    _, mid = go.gemini_forward(mg.case_state_dict(name, args), feats, name, return_intermediates=True)
    pts = go.stop_points(name)
    assert len(pts) == 4 + 77
    for n, pt in enumerate(pts, 1):
        if pt[0] == "block":
            b = mid["u%d.block" % n]
            assert 0.1 < float(b.mean()) < 5.0 and float((b == 0).double().mean()) < 0.8, (n, pt)


def test_write_model_dir_round_trip(tmp_path):
    import yaml
    d = str(tmp_path / "m")
    sd = synth.write_model_dir(d, G60, feat_dim=32, embed_dim=32, seed=42, two_emb_layer=True)
    with open(os.path.join(d, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["model"] == G60
    assert cfg["model_args"] == dict(feat_dim=32, embed_dim=32, pooling_func="TSTP", two_emb_layer=True)
    back = torch.load(os.path.join(d, "avg_model.pt"))
    assert list(back) == list(sd) and all(np.array_equal(back[k].numpy(), sd[k]) for k in sd)
    assert synth.synth_state_dict(G60, 32, 32, two_emb_layer=True).keys() == sd.keys()


def test_native_model_file_round_trip(tmp_path):
    """save_native_model writes every tensor the engine asks for under the reference's names (the file ws_engine_load reads)."""
    import struct
    from wespeaker_amd import engine
    sd = synth.synth_gemini_state_dict(G60, 32, 32)
    path = engine.save_native_model(str(tmp_path / "g.wsamd"), G60, sd, feat_dim=32)
    with open(path, "rb") as f:
        assert f.read(8) == b"WSAMDW01"
        n, = struct.unpack("<i", f.read(4))
        assert f.read(n).decode() == G60
        feat_dim, embed_dim, count = struct.unpack("<iii", f.read(12))
    assert (feat_dim, embed_dim) == (32, 256)                      # DEFAULT_EMBED_DIM["Gemin"]
    assert count == sum(1 for v in sd.values() if np.asarray(v).dtype.kind == "f")


def test_model_args_mapping():
    from wespeaker_amd import engine
    assert all(n in engine.SUPPORTED_MODELS for n in synth.GEMINI_LAYOUTS)
    assert engine.DEFAULT_EMBED_DIM["Gemin"] == 256
    assert engine.NativeSpeakerModel.GEMINI_TAP_NAMES == ("stem", "ds", "exp", "dw", "block", "pooled", "emb_a")


def test_pooling_other_than_tstp_is_refused_by_name(tmp_path):
    import yaml
    from wespeaker_amd import extract, speaker
    d = str(tmp_path / "m")
    synth.write_model_dir(d, G60, feat_dim=32, embed_dim=32, seed=42)
    with open(os.path.join(d, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model_args"]["pooling_func"] = "ASTP"
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(NotImplementedError, match="Gemini_DF_ResNet60 with pooling_func='ASTP'"):
        speaker.load_model_pt(d)
    with pytest.raises(NotImplementedError, match="Gemini_DF_ResNet60 with pooling_func='ASTP'"):
        extract.build_gpu_extractor(cfg, os.path.join(d, "avg_model.pt"))


@pytest.mark.parametrize("variant,what", [(dict(transpose_dw=True), "depthwise filter with F and T taps transposed"),
                                          (dict(ds_relu=True), "a ReLU after every downsample layer"),
                                          (dict(ds1_stride_t=2), "stride (2,2) on downsample layer 1")])
def test_fixture_has_teeth(variant, what):
    """Each mistake, made in the oracle, misses the GPU embedding bar against the true oracle: the GPU tests see it."""
    name, args, feats = mg.golden_cases()[G60 + "/emb_T57"]
    sd = mg.case_state_dict(name, args)
    gap = _rel(go.gemini_forward(sd, feats, name, **variant).numpy(), go.gemini_forward(sd, feats, name).numpy())
    print("%s: %.3e (bar %.1e)" % (what, gap, REL_TOL))
    assert gap > REL_TOL, (what, gap)
