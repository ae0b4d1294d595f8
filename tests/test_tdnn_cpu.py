"""The TDNN x-vector and the xi-vector models on the CPU: the float64 oracle (tests/tdnn_oracle.py) against the
reference's own modules (where the reference checkout is present) and against the committed golden
(tests/golden/tdnn_ref.npz); the synthetic generators' key sets; the regimes the XI fixtures must reach; the
`pooling_func` acceptances and refusals.
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

import make_golden_tdnn as mg  # noqa: E402
import tdnn_oracle as to  # noqa: E402
from oracle import ref_shim  # noqa: E402

ORACLE_TOL = 1e-5          # oracle (float64) against the reference module (float64) / the golden: relative L2 per utterance
REL_TOL = 2e-4             # the GPU embedding bar (tests/test_gpu_tdnn.py)
NAN_CASE = mg.XVEC + "_h64_s100/emb_T15"

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason="reference checkout not present")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)).max())


def _same(key, got, ref, tol):
    """Within tol -- or, where the reference itself is NaN (TSTP's unbiased variance of ONE frame, XVEC at T = 15:
    pooling_layers.py:81), NaN in the same places."""
    if key == NAN_CASE:
        assert np.isnan(ref).all() and np.isnan(got).all(), key
        return 0.0
    assert np.isfinite(ref).all() and np.isfinite(got).all(), key
    err = _rel(got, ref)
    print(key, "%.2e" % err)
    assert err < tol, (key, err)
    return err


def test_oracle_matches_the_committed_golden():
    gold = dict(np.load(mg.GOLD))
    cases = mg.golden_cases()
    assert set(gold) == set(cases)
    assert os.path.getsize(mg.GOLD) < 64 * 1024
    for key, (name, args, extra, feats) in cases.items():
        emb = to.forward(name, mg.case_state_dict(name, args, extra), feats).numpy()
        assert emb.shape == gold[key].shape == (feats.shape[0], args["embed_dim"])
        _same(key, emb, gold[key], ORACLE_TOL)


@needs_reference
@pytest.mark.parametrize("key", [mg.XVEC + "/emb_T33", mg.XI_XVEC + "/emb_T33", mg.XVEC + "_h64_s100/emb_T16",
                                 mg.XI_XVEC + "_h64_s100/emb_T15", mg.XI_C512 + "/emb_T9", mg.XI_C512 + "_embbn/emb_T57",
                                 mg.XI_C1024 + "/emb_T57"])
def test_oracle_matches_the_live_reference_module(key):
    name, args, extra, feats = mg.golden_cases()[key]
    sd = mg.case_state_dict(name, args, extra)
    _same(key, to.forward(name, sd, feats).numpy(), mg.ref_forward(name, args, extra, sd, feats), ORACLE_TOL)


@needs_reference
def test_reference_in_float32_stays_well_inside_the_gpu_bar():
    """The condition under which REL_TOL says something about an fp32 engine: on every golden case the reference module
    itself, run in float32, is within REL_TOL / 4 of the golden."""
    gold = dict(np.load(mg.GOLD))
    for key, (name, args, extra, feats) in mg.golden_cases().items():
        got = mg.ref_forward(name, args, extra, mg.case_state_dict(name, args, extra), feats, dtype=torch.float32)
        _same(key, got, gold[key], REL_TOL / 4)


XI_DEBUG_WINDOWS = [((0, 1), (7, 2), (7, 63)), ((0, 64), (3, 65), (7, 186))]      # (t0, n) per utterance, B = 3


def xi_debug_fixture(D, T, seed=0):
    """The inputs of the ws_debug_xi_pool tests (tests/test_gpu_tdnn.py): x, z (3, T, D) and the priors (D,), with z in
    all three regimes and the prior neither negligible nor dominant for windows of 1 .. 186 frames."""
    rng = np.random.RandomState(seed + D)
    x = rng.randn(3, T, D).astype(np.float32)
    z = (40.0 * rng.randn(3, T, D)).astype(np.float32)
    return x, z, (0.5 * rng.randn(D)).astype(np.float32), rng.uniform(6.0, 11.0, D).astype(np.float32)


def _regimes(z):
    z = np.asarray(z, dtype=np.float64)
    return dict(low=float((z < -7.5).mean()), underflow=float((z < -104).mean()),
                mid=float(((z >= -7.5) & (z <= 20)).mean()), high=float((z > 20).mean()))


def _assert_regimes(what, z, weight):
    r = _regimes(z)
    inside = float(((weight >= 0.01) & (weight <= 0.9)).mean())
    print(what, r, "prior weight in [0.01, 0.9]: %.2f of the channels" % inside)
    assert r["low"] >= 0.01 and r["mid"] >= 0.01 and r["high"] >= 0.01 and r["underflow"] > 0, (what, r)
    assert inside >= 0.5, (what, inside)


@pytest.mark.parametrize("key", [mg.XI_XVEC + "/emb_T200", mg.XI_XVEC + "_h64_s100/emb_T57", mg.XI_C512 + "/emb_T57",
                                 mg.XI_C1024 + "/emb_T57"])
def test_xi_fixture_reaches_every_regime(key):
    name, args, extra, feats = mg.golden_cases()[key]
    sd = mg.case_state_dict(name, args, extra)
    _, mid = to.forward(name, sd, feats, return_intermediates=True)
    w = to.prior_weight(mid["xi_z"], torch.as_tensor(sd["pool.prior_logprec"]).double()).numpy()
    _assert_regimes(key, mid["xi_z"].numpy(), w)


@pytest.mark.parametrize("D", [100, 1500, 1536])
@pytest.mark.parametrize("windows", XI_DEBUG_WINDOWS)
def test_xi_debug_fixture_reaches_every_regime(D, windows):
    """Over the three windows of a set together (a window of one frame has one z per channel)."""
    x, z, pm, pl = xi_debug_fixture(D, 200)
    zz = np.concatenate([z[b, t0:t0 + n] for b, (t0, n) in enumerate(windows)])
    w = np.concatenate([to.prior_weight(torch.from_numpy(z[b:b + 1, t0:t0 + n]).double().permute(0, 2, 1),
                                        torch.from_numpy(pl[None]).double()).numpy().reshape(-1)
                        for b, (t0, n) in enumerate(windows)])
    _assert_regimes("D=%d %s" % (D, windows), zz, w)


def test_numpy_xi_formula_is_the_torch_one():
    x, z, pm, pl = xi_debug_fixture(100, 80)
    win = [(0, 1), (7, 2), (7, 63)]
    got = to.xi_pool_windows(x, z, pm, pl, win)
    for b, (t0, n) in enumerate(win):
        ref = to.xi_posterior_mean(torch.from_numpy(x[b:b + 1, t0:t0 + n]).double().permute(0, 2, 1),
                                   torch.from_numpy(z[b:b + 1, t0:t0 + n]).double().permute(0, 2, 1),
                                   torch.from_numpy(pm[None]).double(), torch.from_numpy(pl[None]).double()).numpy()
        assert _rel(got[b:b + 1], ref) < 1e-12
    assert to.xi_pool_windows(x, z, pm, pl, win, dtype=np.float32).dtype == np.float32


def _bn_keys(p, affine=True):
    return [p + s for s in ((".weight", ".bias") if affine else ())] + [p + s for s in (".running_mean", ".running_var",
                                                                                        ".num_batches_tracked")]


def _xi_keys(p="pool"):
    return ([p + ".prior_mean", p + ".prior_logprec", p + ".lin1_relu_bn.0.weight", p + ".lin1_relu_bn.0.bias"] +
            _bn_keys(p + ".lin1_relu_bn.2") + [p + ".lin2.weight", p + ".lin2.bias"])


@pytest.mark.parametrize("name", [mg.XVEC, mg.XI_XVEC])
def test_xvec_generator_key_set(name):
    sd = mg.synth_xvec_state_dict(name, 80, 512)
    keys = []
    for k in range(1, 6):
        keys += ["frame_%d.conv_1d.weight" % k, "frame_%d.conv_1d.bias" % k] + _bn_keys("frame_%d.bn" % k, affine=False)
    if name == mg.XI_XVEC:
        keys += _xi_keys()
    keys += ["seg_1.weight", "seg_1.bias"] + _bn_keys("seg_bn_1", affine=False) + ["seg_2.weight", "seg_2.bias"]
    assert set(sd) == set(keys) and len(sd) == len(keys)
    assert sd["frame_1.conv_1d.weight"].shape == (512, 80, 5) and sd["frame_5.conv_1d.weight"].shape == (1500, 512, 1)
    assert sd["seg_1.weight"].shape == (512, 1500 if name == mg.XI_XVEC else 3000)
    for k, v in sd.items():
        if k.endswith("running_var"):
            assert (v > 0).all(), k
        if k.endswith("running_mean"):
            assert (v != 0).all(), k
    if ref_shim.available():
        ref = mg.ref_model(name, dict(feat_dim=80, embed_dim=512), {}, sd, dtype=torch.float32).state_dict()
        assert set(ref) == set(sd)
        assert all(tuple(ref[k].shape) == tuple(np.asarray(sd[k]).shape) for k in sd)


@pytest.mark.parametrize("name,emb_bn", [(mg.XI_C512, False), (mg.XI_C512, True), (mg.XI_C1024, False)])
def test_xi_ecapa_generator_key_set(name, emb_bn):
    sd = mg.synth_xi_ecapa_state_dict(name, 80, 192, emb_bn=emb_bn)
    assert set(_xi_keys()) <= set(sd) and not any(k.startswith("pool.linear") for k in sd)
    assert sd["bn.running_mean"].shape == (1536,) and sd["linear.weight"].shape == (192, 1536)
    assert ("bn2.running_mean" in sd) == emb_bn
    if ref_shim.available():
        ref = mg.ref_model(name, dict(feat_dim=80, embed_dim=192, emb_bn=emb_bn), {}, sd, dtype=torch.float32).state_dict()
        assert set(ref) == set(sd)
        assert all(tuple(ref[k].shape) == tuple(np.asarray(sd[k]).shape) for k in sd)


def test_model_names_and_tap_names():
    from wespeaker_amd import engine
    for n in (mg.XVEC, mg.XI_XVEC, mg.XI_C512, mg.XI_C1024):
        assert n in engine.SUPPORTED_MODELS
    assert engine.NativeSpeakerModel.TDNN_TAP_NAMES == ("frame", "pooled", "emb_a", "xi_hid", "xi_z")


def write_model_dir(d, name, sd, **model_args):
    """config.yaml + avg_model.pt, the layout wespeaker_amd.load_model reads (cli/speaker.py:306-335)."""
    import yaml
    os.makedirs(d, exist_ok=True)
    cfg = {"model": name, "model_args": dict(model_args),
           "dataset_args": {"resample_rate": 16000, "frontend": "fbank",
                            "fbank_args": {"num_mel_bins": model_args["feat_dim"], "frame_shift": 10, "frame_length": 25,
                                           "dither": 0.0}}}
    with open(os.path.join(d, "config.yaml"), "w") as f:
        yaml.safe_dump(cfg, f)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, os.path.join(d, "avg_model.pt"))
    return cfg


@pytest.mark.parametrize("name,good,bad", [(mg.XVEC, "TSTP", "XI"), (mg.XI_XVEC, "XI", "TSTP"), (mg.XI_C512, "XI", "ASTP"),
                                           (mg.XI_C1024, "XI", "TSTP")])
def test_pooling_func_acceptances_and_refusals(tmp_path, name, good, bad):
    from wespeaker_amd import engine, extract, speaker
    for ok in (None, good):
        engine.check_pooling_func(name, ok)
    with pytest.raises(NotImplementedError, match=r"%s with pooling_func='%s' \(only %s\)" % (name, bad, good)):
        engine.check_pooling_func(name, bad)
    engine.check_pooling_func("ResNet34", "XI")            # other families: not this function's business
    d = str(tmp_path / "m")
    sd = {"frame_1.conv_1d.weight": np.zeros((4, 40, 5), np.float32)}
    cfg = write_model_dir(d, name, sd, feat_dim=40, embed_dim=64, pooling_func=bad)
    with pytest.raises(NotImplementedError, match="%s with pooling_func='%s'" % (name, bad)):
        speaker.load_model_pt(d)
    with pytest.raises(NotImplementedError, match="%s with pooling_func='%s'" % (name, bad)):
        extract.build_gpu_extractor(cfg, os.path.join(d, "avg_model.pt"))
