"""SimAM_ResNet34_ASP / SimAM_ResNet100_ASP on the GPU: the engine against the float64 oracle (tests/simam_oracle.py)
and the reference-made golden (tests/golden/samresnet_ref.npz).

Bars: COS_TOL = 1e-4 and REL_TOL = 2e-4 on embeddings (those of tests/test_gpu_parity.py); 1e-5 between a row of a
ragged batch and its own batch-1 result (the bar of the ragged ResNet test there); per-test bars in the docstrings.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_simam as mg  # noqa: E402
import simam_oracle as so  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import fbank as ofbank  # noqa: E402

pytestmark = pytest.mark.gpu

COS_TOL = 1e-4
REL_TOL = 2e-4
RAGGED_VS_SINGLE_TOL = 1e-5
S34, S100 = "SimAM_ResNet34_ASP", "SimAM_ResNet100_ASP"


def _rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _scaled_errors(got, ref):
    """(max |got - ref| / max |ref|, relative L2), in float64."""
    d = np.asarray(got, dtype=np.float64) - ref
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.sqrt((d * d).sum() / (ref * ref).sum()))


@functools.lru_cache(maxsize=None)
def _sd(name=S34, in_planes=64, feat_dim=80, embed_dim=256):
    return synth.synth_simam_resnet_state_dict(name, feat_dim, embed_dim, in_planes=in_planes, seed=42)


_ENGINES = {}


def _engine(name=S34, in_planes=64, feat_dim=80, embed_dim=256, sd=None, key=None, max_batch=8, max_frames=200):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = key or (name, in_planes, feat_dim, embed_dim, max_batch, max_frames)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, sd if sd is not None else _sd(name, in_planes, feat_dim, embed_dim),
                                           feat_dim=feat_dim, embed_dim=embed_dim, max_batch=max_batch,
                                           max_frames=max_frames)
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def _fixture_feats():
    f = np.stack([ofbank.speaker_features(synth.synth_wav(i)) for i in range(3)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "samresnet_ref.npz")))


def _oracle(sd, feats, name=S34, **kw):
    out = so.simam_resnet_forward(sd, np.array(feats), name, **kw)
    return (out[0].numpy(), {k: v.numpy() for k, v in out[1].items()}) if isinstance(out, tuple) else out.numpy()


def _check(got, ref, what):
    assert np.isfinite(got).all(), what
    cos, rel = _cos_err(got, ref).max(), _rel_err(got, ref).max()
    print(what, "cos %.2e rel %.2e" % (cos, rel))
    assert cos < COS_TOL and rel < REL_TOL, (what, cos, rel)


def test_forward_parity_with_oracle_and_golden():
    model = _engine()
    assert model.ignored_keys == []
    f = _fixture_feats()
    out = model(torch.from_numpy(np.array(f)))
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (3, 256)          # a bare tensor (samresnet.py:142-149)
    got = out.cpu().numpy()
    _check(got, _oracle(_sd(), f), "fp32 vs oracle")
    _check(got[:2], _golden()[S34 + "/emb"], "fp32 vs golden")
    _check(model(torch.from_numpy(np.array(f[:2, :57]))).cpu().numpy(), _golden()[S34 + "/emb_T57"], "T57 vs golden")
    model.check_range()


@pytest.mark.parametrize("T", [9, 57, 64, 131])
def test_odd_lengths_through_the_stride_two_stages(T):
    f = np.random.RandomState(T).randn(2, T, 80).astype(np.float32)
    got = _engine()(torch.from_numpy(f)).cpu().numpy()
    _check(got, _oracle(_sd(), f), "T = %d" % T)


def test_narrow_width():
    """in_planes 16, 24 mel bins, embed 32, T = 37: stage widths 16 / 32 / 64 / 128 (N below every GEMM tile width)."""
    name, args, feats = mg.golden_cases()[S34 + "_p16/emb_T37"]
    model = _engine(S34, 16, 24, 32)
    assert model.ignored_keys == []
    got = model(torch.from_numpy(feats)).cpu().numpy()
    _check(got, _golden()[S34 + "_p16/emb_T37"], "in_planes 16 vs golden")
    model.set_precision("f16x3")                          # the split-binary16 GEMM back-end: same bar
    try:
        got3 = model(torch.from_numpy(feats)).cpu().numpy()
    finally:
        model.set_precision("fp32")
    _check(got3, _golden()[S34 + "_p16/emb_T37"], "in_planes 16, f16x3 vs golden")


def test_deep_layout():
    feats = mg.golden_cases()[S100 + "/emb_T57"][2][:1]
    model = _engine(S100, max_batch=2, max_frames=64)
    assert model.ignored_keys == []
    got = model(torch.from_numpy(feats)).cpu().numpy()
    _check(got, _golden()[S100 + "/emb_T57"][:1], "SimAM_ResNet100 vs golden")


def test_ragged_batch_rows_equal_their_own_batch_of_one():
    """Plane statistics that include padding columns, or a wrong n, show up here: every length of the batch but the
    first has padding at every stride level."""
    lens = [200, 199, 131, 57, 9]
    feats = [np.random.RandomState(100 + i).randn(L, 80).astype(np.float32) for i, L in enumerate(lens)]
    pad = np.full((len(lens), max(lens), 80), np.nan, dtype=np.float32)
    for i, f in enumerate(feats):
        pad[i, :lens[i]] = f
    model = _engine()
    got = model.embed_ragged(torch.from_numpy(pad), lens).cpu().numpy()
    assert np.isfinite(got).all()
    for i, f in enumerate(feats):
        one = model(torch.from_numpy(f[None])).cpu().numpy()
        err = _rel_err(got[i:i + 1], one).max()
        print("row %d (%d frames) vs batch of one: %.2e" % (i, lens[i], err))
        assert err < RAGGED_VS_SINGLE_TOL, (i, lens[i], err)
        _check(got[i:i + 1], _oracle(_sd(), f[None]), "ragged row %d vs oracle" % i)
    model.check_range()                                    # (fp32: a no-op; kept for the call path)


OFFSET_CHANNELS = (3, 17, 40, 63)
# measured on the CPU, this fixture, the first block's output against the float64 oracle:
OFFSET_REF_FP32_ERR = (1.61e-6, 4.55e-7)       # the reference's own float32 module: (scaled max error, relative L2)
OFFSET_BAR = tuple(8 * e for e in OFFSET_REF_FP32_ERR)


def test_offset_channels_need_centred_plane_statistics():
    """bn2.bias = 30 on four channels of front.layer1.0: conv2's output sits at 30 with a spread of 0.4 .. 0.7 there
    (|mean| / std = 44 .. 72).  The first block's output (tap 'block1') against the float64 oracle, two metrics:
    scaled max error max|got - ref| / max|ref| and relative L2.

    Bar = 8 x the error of the reference's own float32 module on this fixture (the GPU's summation order differs from
    torch's), measured on the CPU: reference fp32 module 1.61e-6 / 4.55e-7  ->  bar 1.29e-5 / 3.64e-6.
    The cancelling form v = (sum x^2 - N mu^2) / (N - 1), evaluated below in numpy float32 on the oracle's own conv2
    output, gives 4.9e-5 / 1.5e-5 (its v is off by 3.6e-4): it misses the bar, so the fixture has teeth.
    """
    sd = {k: np.array(v, copy=True) for k, v in _sd().items()}
    sd["front.layer1.0.bn2.bias"][list(OFFSET_CHANNELS)] = 30.0
    f = _fixture_feats()[:2]
    _, mid = _oracle(sd, f, return_intermediates=True)
    ref = mid["block1"]                                                   # (B, C, F, T)
    # the cancelling form, float32 (CPU): must miss the bar
    y, r = mid["block1_y"].astype(np.float32), mid["block1_res"].astype(np.float32)
    n = np.float32(y.shape[2] * y.shape[3])
    mu = y.sum(axis=(2, 3), keepdims=True, dtype=np.float32) / n
    v = ((y * y).sum(axis=(2, 3), keepdims=True, dtype=np.float32) - n * mu * mu) / (n - 1)
    e = (y - mu) ** 2 / (np.float32(4) * (v + np.float32(1e-4))) + np.float32(0.5)
    naive = np.maximum(y / (1 + np.exp(-e)) + r, 0)
    e_naive = _scaled_errors(naive, ref)
    print("cancelling form %.2e %.2e | bar %.2e %.2e" % (e_naive + OFFSET_BAR))
    assert e_naive[0] > OFFSET_BAR[0] and e_naive[1] > OFFSET_BAR[1]
    model = _engine(sd=sd, key="offset", max_batch=2, max_frames=200)
    emb = model(torch.from_numpy(np.array(f))).cpu().numpy()
    assert np.isfinite(emb).all()
    got = model.tap("block1").cpu().numpy().reshape(2, 80, f.shape[1], 64).transpose(0, 3, 1, 2)
    e_dev = _scaled_errors(got, ref)
    print("device %.2e %.2e" % e_dev)
    assert np.isfinite(got).all()
    assert e_dev[0] <= OFFSET_BAR[0] and e_dev[1] <= OFFSET_BAR[1], (e_dev, OFFSET_BAR)
    worst = max(_scaled_errors(got[:, c], ref[:, c])[0] for c in OFFSET_CHANNELS)
    print("offset channels alone %.2e" % worst)
    assert worst <= OFFSET_BAR[0], worst


@pytest.mark.parametrize("T", [9, 198])
def test_asp_head_alone(T):
    """The pooled (B, 2D) vector (tap 'pooled') against the oracle, T' = 2 (T = 9) and T' = 25 (T = 198), relative L2
    per utterance below REL_TOL."""
    f = _fixture_feats()[:2, :T]
    model = _engine()
    model(torch.from_numpy(np.array(f)))
    got = model.tap("pooled").cpu().numpy()
    _, mid = _oracle(_sd(), f, return_intermediates=True)
    assert got.shape == mid["pooled"].shape == (2, 2 * 5120)
    assert mid["logits"].shape[2] == (2 if T == 9 else 25)
    err = _rel_err(got, mid["pooled"]).max()
    print("pooled, T = %d: %.2e" % (T, err))
    assert np.isfinite(got).all() and err < REL_TOL, err


def test_asp_softmax_survives_shifted_logits():
    """pooling.attention.3.bias + 80 on every third channel.  The bias is per channel, so every frame of those channels
    is shifted (a softmax over time does not change); exp() of the shifted logits themselves overflows float32, which
    a softmax without max subtraction would turn into inf / inf."""
    sd = {k: np.array(v, copy=True) for k, v in _sd().items()}
    sd["pooling.attention.3.bias"][::3] += 80.0
    f = _fixture_feats()[:1]
    emb_ref, mid = _oracle(sd, f, return_intermediates=True)
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(mid["logits"].astype(np.float32))).any()          # the fixture does overflow
    model = _engine(sd=sd, key="shifted", max_batch=2, max_frames=200)
    emb = model(torch.from_numpy(np.array(f))).cpu().numpy()
    got = model.tap("pooled").cpu().numpy()
    err = _rel_err(got, mid["pooled"]).max()
    print("pooled with shifted logits: %.2e" % err)
    assert np.isfinite(got).all() and err < REL_TOL, err
    _check(emb, emb_ref, "embedding with shifted logits")


def test_public_surface(tmp_path):
    import wespeaker_amd
    from wespeaker_amd._lib import NativeError
    d = str(tmp_path / "m")
    synth.write_model_dir(d, S34, feat_dim=24, embed_dim=32, seed=42, in_planes=16)
    spk = wespeaker_amd.load_model(d, max_batch=4, max_frames=200)
    assert spk.model.model_name == S34 and spk.model.feat_dim == 24 and spk.model.embed_dim == 32
    assert spk.model.ignored_keys == []
    pcm = torch.from_numpy(synth.synth_wav(5))
    e1 = spk.extract_embedding_from_pcm(pcm.unsqueeze(0), 16000)
    feats = spk.compute_features(pcm.unsqueeze(0).to(torch.float32), 16000)
    out = spk.model(feats)
    assert isinstance(out, torch.Tensor)
    assert torch.equal(e1, out[0].cpu())
    ref = _oracle(_sd(S34, 16, 24, 32), feats.cpu().numpy())
    _check(e1.numpy()[None], ref, "load_model -> extract_embedding_from_pcm vs oracle")
    # mode 2 (binary16 tensors) is refused, with a message that names the model; nothing beyond the error return
    with pytest.raises(NativeError, match="SimAM_ResNet34_ASP has no binary16-tensor back-end"):
        spk.set_precision("f16")
    assert spk.model.precision == "fp32"
    assert torch.equal(spk.extract_embedding_from_pcm(pcm.unsqueeze(0), 16000), e1)
    # a config whose in_planes disagrees with the checkpoint
    import yaml
    with open(os.path.join(d, "config.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    cfg["model_args"]["in_planes"] = 64
    with open(os.path.join(d, "config.yaml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    with pytest.raises(ValueError, match="in_planes"):
        wespeaker_amd.load_model(d, max_batch=4, max_frames=200)


def test_row_permutation_and_lanes_give_the_same_bits():
    from wespeaker_amd.engine import SpeakerModelLanes
    f = np.random.RandomState(8).randn(8, 100, 80).astype(np.float32)
    model = _engine()
    base = model(torch.from_numpy(f))
    perm = np.random.RandomState(9).permutation(8)
    assert torch.equal(model(torch.from_numpy(f[perm])), base[torch.from_numpy(perm).to(base.device)])
    lanes = SpeakerModelLanes(S34, _sd(), lanes=2, feat_dim=80, embed_dim=256, max_batch=8, max_frames=200)
    x = torch.from_numpy(f).to(model.device)
    r = [lanes.embed(x), lanes.embed(x)]                   # one batch on each lane, in flight together
    for res in r:
        assert torch.equal(res.synchronize(), base)
    assert {res.lane for res in r} == {0, 1}
