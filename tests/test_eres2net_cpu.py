"""ERes2Net34 on the CPU: the float64 oracle (tests/eres2net_oracle.py) against the reference's own module (where the
reference checkout is present) and against the committed golden (tests/golden/eres2net_ref.npz); the synthetic weight
generator's key set; the model directory round trip; the fixtures with teeth of tests/test_gpu_eres2net.py.
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

import eres2net_oracle as eo  # noqa: E402
import make_golden_eres2net as mg  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import ref_shim  # noqa: E402

ORACLE_TOL = 1e-5          # oracle (float64) against the reference module (float64) / the golden: relative L2 per utterance
REL_TOL = 2e-4             # the GPU embedding bar (tests/test_gpu_eres2net.py)
GOLD = os.path.join(ROOT, "tests", "golden", "eres2net_ref.npz")
BASE = mg.BASE
CLAMP_OFFSET = 25.0
CLAMP_CHANNELS = (3, 17, 40, 63)

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason="reference checkout not present")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def test_oracle_matches_the_committed_golden():
    gold = dict(np.load(GOLD))
    cases = mg.golden_cases()
    assert set(gold) == set(cases)
    for key, (name, args, feats) in cases.items():
        emb = eo.eres2net_forward(mg.case_state_dict(name, args), feats, name).numpy()
        assert emb.shape == gold[key].shape
        err = _rel(emb, gold[key])
        print(key, "%.2e" % err)
        assert err < ORACLE_TOL, (key, err)


@needs_reference
@pytest.mark.parametrize("key", [BASE + "/emb_T57", BASE + "_two/emb_T57", mg.AUG + "/emb_T33"])
def test_oracle_matches_the_live_reference_module(key):
    name, args, feats = mg.golden_cases()[key]
    sd = mg.case_state_dict(name, args)
    err = _rel(eo.eres2net_forward(sd, feats, name).numpy(), mg.ref_forward(name, args, sd, feats))
    assert err < ORACLE_TOL, err


def _expected_keys(name, two=False):
    """The module's state_dict keys, written out (eres2net.py:243-335)."""
    m, bw, scale, exp = synth.ERES2NET_LAYOUTS[name]
    bn = lambda p: [p + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]  # noqa: E731
    aff = lambda p: ([p + ".local_att.0.weight", p + ".local_att.0.bias"] + bn(p + ".local_att.1") +  # noqa: E731
                     [p + ".local_att.3.weight", p + ".local_att.3.bias"] + bn(p + ".local_att.4"))
    keys = ["conv1.weight"] + bn("bn1")
    cin = m
    for s, nb in enumerate((3, 4, 6, 3)):
        planes = m << s
        for b in range(nb):
            p = "layer%d.%d" % (s + 1, b)
            keys += [p + ".conv1.weight"] + bn(p + ".bn1")
            n = scale
            if s >= 2:
                keys += [p + ".conv2_1.weight"] + bn(p + ".bn2_1")
                n = scale - 1
            keys += [p + ".convs.%d.weight" % i for i in range(n)]
            for i in range(n):
                keys += bn(p + ".bns.%d" % i)
            if s >= 2:
                for i in range(n):
                    keys += aff(p + ".fuse_models.%d" % i)
            keys += [p + ".conv3.weight"] + bn(p + ".bn3")
            if b == 0 and (s > 0 or cin != planes * exp):
                keys += [p + ".shortcut.0.weight"] + bn(p + ".shortcut.1")
            cin = planes * exp
    keys += ["layer%d_downsample.weight" % k for k in (1, 2, 3)]
    for fn in ("fuse_mode12", "fuse_mode123", "fuse_mode1234"):
        keys += aff(fn)
    keys += ["seg_1.weight", "seg_1.bias"]
    if two:
        keys += ["seg_bn_1.running_mean", "seg_bn_1.running_var", "seg_bn_1.num_batches_tracked", "seg_2.weight", "seg_2.bias"]
    return keys


@pytest.mark.parametrize("name,two,count", [(BASE, False, 587), (BASE, True, 592), (mg.LARGE, False, 587), (mg.AUG, False, None)])
def test_synthetic_key_set(name, two, count):
    sd = synth.synth_eres2net_state_dict(name, 80, 192, two_emb_layer=two)
    assert list(sd) == _expected_keys(name, two)
    if count:
        assert len(sd) == count
    if ref_shim.available():
        model = mg.ref_model(name, dict(feat_dim=80, embed_dim=192, two_emb_layer=two), sd, dtype=torch.float32)
        ref = model.state_dict()
        assert list(ref) == list(sd)
        assert all(tuple(ref[k].shape) == tuple(np.asarray(sd[k]).shape) for k in sd)


def test_synthetic_activations_stay_in_range():
    """O(1) through the 16 blocks: neither collapsed to zero nor sitting on the clamp."""
    name, args, feats = mg.golden_cases()[BASE + "/emb_T57"]
    _, mid = eo.eres2net_forward(mg.case_state_dict(name, args), feats, name, return_intermediates=True)
    for i in range(1, 17):
        b = mid["b%d.block" % i]
        assert 0.1 < float(b.mean()) < 5.0 and float((b == 0).double().mean()) < 0.8 and float((b >= 20).double().mean()) < 0.01, i


def test_write_model_dir_round_trip(tmp_path):
    import yaml
    d = str(tmp_path / "m")
    sd = synth.write_model_dir(d, BASE, feat_dim=24, embed_dim=32, seed=42, two_emb_layer=True)
    with open(os.path.join(d, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    assert cfg["model"] == BASE
    assert cfg["model_args"] == dict(feat_dim=24, embed_dim=32, pooling_func="TSTP", two_emb_layer=True)
    back = torch.load(os.path.join(d, "avg_model.pt"))
    assert list(back) == list(sd) and all(np.array_equal(back[k].numpy(), sd[k]) for k in sd)
    assert synth.synth_state_dict(BASE, 24, 32, two_emb_layer=True).keys() == sd.keys()


def test_model_args_mapping():
    from wespeaker_amd import engine
    assert all(n in engine.SUPPORTED_MODELS for n in synth.ERES2NET_LAYOUTS)
    assert engine.DEFAULT_EMBED_DIM["ERes2"] == 512
    assert "cat" in engine.NativeSpeakerModel.ERES2NET_TAP_NAMES and "fuse1234" in engine.NativeSpeakerModel.ERES2NET_TAP_NAMES


def test_pooling_other_than_tstp_is_refused_by_name(tmp_path):
    import yaml
    from wespeaker_amd import speaker
    d = str(tmp_path / "m")
    synth.write_model_dir(d, BASE, feat_dim=24, embed_dim=32, seed=42)
    with open(os.path.join(d, "config.yaml")) as f:
        cfg = yaml.safe_load(f)
    cfg["model_args"]["pooling_func"] = "ASTP"
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    with pytest.raises(NotImplementedError, match="ERes2Net34_Base with pooling_func='ASTP'"):
        speaker.load_model_pt(d)


def _clamp_sd():
    sd = {k: np.array(v, copy=True) for k, v in synth.synth_eres2net_state_dict(BASE, 80, 192).items()}
    sd["layer1.0.bn3.bias"][list(CLAMP_CHANNELS)] += CLAMP_OFFSET
    sd["layer3.0.bns.0.bias"][list(CLAMP_CHANNELS)] += CLAMP_OFFSET
    return sd


def test_clamp_fixture_has_teeth():
    """+25 on four channels of layer1.0.bn3.bias and layer3.0.bns.0.bias: an oracle with max(x, 0) in place of
    Hardtanh(0, 20) misses the GPU embedding bar against the true oracle (measured gap: see the printed figure)."""
    feats = mg.golden_cases()[BASE + "/emb_T57"][2]
    sd = _clamp_sd()
    true, mid = eo.eres2net_forward(sd, feats, BASE, return_intermediates=True)
    assert float((mid["b1.block"][:, list(CLAMP_CHANNELS)] == 20.0).double().mean()) > 0.5
    plain = eo.eres2net_forward(sd, feats, BASE, clamp=False)
    gap = _rel(plain.numpy(), true.numpy())
    print("relu for the clamp: %.3e (bar %.1e)" % (gap, REL_TOL))
    assert gap > REL_TOL, gap
    # ... and on the plain weights the ceiling is never reached: the fixture is what gives the clamp teeth
    sd0 = synth.synth_eres2net_state_dict(BASE, 80, 192)
    assert _rel(eo.eres2net_forward(sd0, feats, BASE, clamp=False).numpy(), eo.eres2net_forward(sd0, feats, BASE).numpy()) == 0.0


def test_swapped_aff_arguments_miss_the_bar():
    feats = mg.golden_cases()[BASE + "/emb_T57"][2]
    sd = synth.synth_eres2net_state_dict(BASE, 80, 192)
    gap = _rel(eo.eres2net_forward(sd, feats, BASE, swap_aff=True).numpy(), eo.eres2net_forward(sd, feats, BASE).numpy())
    print("AFF(y, x) for AFF(x, y): %.3e (bar %.1e)" % (gap, REL_TOL))
    assert gap > REL_TOL, gap
