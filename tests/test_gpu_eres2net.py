"""ERes2Net34_Base / _Large / _aug on the GPU: the engine against the float64 oracle (tests/eres2net_oracle.py) and the
reference-made golden (tests/golden/eres2net_ref.npz).

Bars: COS_TOL = 1e-4 and REL_TOL = 2e-4 on embeddings (those of tests/test_gpu_parity.py); 1e-5 between a row of a
ragged batch and its own batch-1 result; per-tap parity by the rule of tests/test_gpu_resnet_layers.py: a tap's error
against the float64 oracle (scaled max and relative L2) at most k = 8 x the error of the float32 oracle, floored at
2^-24 (tests/test_gpu_layers.py: tap_check).

Measured worst ratios (test_every_tap, Base, T = 57, MI355X): fp32 2.35 (b16.cat; stem 0.94, block outputs 0.87 .. 1.72,
fuse12 / fuse123 / fuse1234 1.20 / 1.82 / 2.14, pooled 2.01); f16x3 3.58 (fuse1234; block outputs 1.39 .. 3.01, pooled 3.37).
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

import eres2net_oracle as eo  # noqa: E402
import make_golden_eres2net as mg  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import fbank as ofbank  # noqa: E402
from test_gpu_layers import _assert_all, tap_check  # noqa: E402

pytestmark = pytest.mark.gpu

COS_TOL = 1e-4
REL_TOL = 2e-4
RAGGED_VS_SINGLE_TOL = 1e-5
K_TAP = 8.0
BASE, LARGE, AUG = mg.BASE, mg.LARGE, mg.AUG
CLAMP_OFFSET = 25.0
CLAMP_CHANNELS = (3, 17, 40, 63)


def _rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@functools.lru_cache(maxsize=None)
def _sd(name=BASE, feat_dim=80, embed_dim=192, two=False):
    return synth.synth_eres2net_state_dict(name, feat_dim, embed_dim, two_emb_layer=two, seed=42)


def clamp_fixture_sd():
    """+25 on four channels of layer1.0.bn3.bias and of layer3.0.bns.0.bias: those maps pass Hardtanh's ceiling."""
    sd = {k: np.array(v, copy=True) for k, v in _sd().items()}
    sd["layer1.0.bn3.bias"][list(CLAMP_CHANNELS)] += CLAMP_OFFSET
    sd["layer3.0.bns.0.bias"][list(CLAMP_CHANNELS)] += CLAMP_OFFSET
    return sd


_ENGINES = {}


def _engine(name=BASE, feat_dim=80, embed_dim=192, two=False, sd=None, key=None, max_batch=8, max_frames=200):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = key or (name, feat_dim, embed_dim, two, max_batch, max_frames)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, sd if sd is not None else _sd(name, feat_dim, embed_dim, two),
                                           feat_dim=feat_dim, embed_dim=embed_dim, max_batch=max_batch,
                                           max_frames=max_frames)
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def _fixture_feats():
    f = np.stack([ofbank.speaker_features(synth.synth_wav(i)) for i in range(2)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "eres2net_ref.npz")))


def _oracle(sd, feats, name=BASE, **kw):
    out = eo.eres2net_forward(sd, np.array(feats), name, **kw)
    return out.numpy() if not isinstance(out, tuple) else (out[0].numpy(), out[1])


def _check(got, ref, what):
    assert np.isfinite(got).all(), what
    cos, rel = _cos_err(got, ref).max(), _rel_err(got, ref).max()
    print(what, "cos %.2e rel %.2e" % (cos, rel))
    assert cos < COS_TOL and rel < REL_TOL, (what, cos, rel)


def _cl(t):
    """(B, C, F, T) oracle map -> the engine's rows (B*F*T, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


def test_forward_parity_with_oracle_and_golden():
    model = _engine()
    assert model.ignored_keys == []
    f = _fixture_feats()
    out = model(torch.from_numpy(np.array(f)))
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (2, 192)          # a bare tensor (eres2net.py:380-391)
    got = out.cpu().numpy()
    _check(got, _oracle(_sd(), f), "fp32 vs oracle")
    _check(got, _golden()[BASE + "/emb"], "fp32 vs golden")
    _check(model(torch.from_numpy(np.array(f[:, :57]))).cpu().numpy(), _golden()[BASE + "/emb_T57"], "T57 vs golden")
    model.check_range()


@pytest.mark.parametrize("T", [9, 57, 64, 131])
def test_odd_lengths_through_the_stride_two_stages(T):
    """The block path (1x1 stride 2) and the downsample path (3x3 stride 2, pad 1) both give (T - 1) // 2 + 1."""
    f = np.random.RandomState(T).randn(2, T, 80).astype(np.float32)
    model = _engine()
    got = model(torch.from_numpy(f)).cpu().numpy()
    _check(got, _oracle(_sd(), f), "T = %d" % T)
    L = T
    for k, n in enumerate(("fuse12", "fuse123", "fuse1234")):
        L = (L - 1) // 2 + 1
        assert model.tap_shape(n) == (2 * (80 >> (k + 1)) * L, 128 << k)


def test_narrow_features_both_backends():
    name, args, feats = mg.golden_cases()[BASE + "_f24/emb_T37"]
    model = _engine(BASE, 24, 32)
    assert model.ignored_keys == []
    _check(model(torch.from_numpy(feats)).cpu().numpy(), _golden()[BASE + "_f24/emb_T37"], "24 mel vs golden")
    model.set_precision("f16x3")
    try:
        got3 = model(torch.from_numpy(feats)).cpu().numpy()
        model.check_range()
    finally:
        model.set_precision("fp32")
    _check(got3, _golden()[BASE + "_f24/emb_T37"], "24 mel, f16x3 vs golden")


def test_two_embedding_layers():
    name, args, feats = mg.golden_cases()[BASE + "_two/emb_T57"]
    model = _engine(BASE, two=True)
    assert model.ignored_keys == []
    out = model(torch.from_numpy(feats))
    assert isinstance(out, torch.Tensor)
    _check(out.cpu().numpy(), _golden()[BASE + "_two/emb_T57"], "two_emb_layer vs golden")
    _, mid = _oracle(_sd(two=True), feats, return_intermediates=True)
    err = _rel_err(model.tap("emb_a").cpu().numpy(), mid["emb_a"].numpy()).max()
    assert err < REL_TOL, err


@pytest.mark.parametrize("name,key", [(LARGE, LARGE + "/emb_T57"), (AUG, AUG + "/emb_T33")])
def test_large_and_aug(name, key):
    feats = mg.golden_cases()[key][2]
    model = _engine(name, max_batch=2, max_frames=64)
    assert model.ignored_keys == []
    _check(model(torch.from_numpy(feats)).cpu().numpy(), _golden()[key], name + " vs golden")


def test_ragged_batch_rows_equal_their_own_batch_of_one():
    lens = [200, 199, 131, 57, 9]
    feats = [np.random.RandomState(100 + i).randn(L, 80).astype(np.float32) for i, L in enumerate(lens)]
    pad = np.full((len(lens), max(lens), 80), np.nan, dtype=np.float32)
    for i, f in enumerate(feats):
        pad[i, :lens[i]] = f
    model = _engine()
    got = model.embed_ragged(torch.from_numpy(pad), lens).cpu().numpy()
    assert np.isfinite(got).all()
    f12 = model.tap("fuse12").cpu().numpy().reshape(len(lens), 40, 100, 128)
    for i, L in enumerate(lens):
        L1 = (L - 1) // 2 + 1
        assert (f12[i, :, L1:] == 0.0).all(), i               # exact-zero padding columns
        assert np.abs(f12[i, :, :L1]).max() > 0
    for i, f in enumerate(feats):
        one = model(torch.from_numpy(f[None])).cpu().numpy()
        err = _rel_err(got[i:i + 1], one).max()
        print("row %d (%d frames) vs batch of one: %.2e" % (i, lens[i], err))
        assert err < RAGGED_VS_SINGLE_TOL, (i, lens[i], err)
        _check(got[i:i + 1], _oracle(_sd(), f[None]), "ragged row %d vs oracle" % i)


def test_clamp_fixture_on_the_device():
    """The fixture of tests/test_eres2net_cpu.py (an oracle with max(x, 0) for the clamp misses REL_TOL on it): the
    embedding, and layer1.0's output, whose four offset channels sit on the ceiling."""
    sd = clamp_fixture_sd()
    f = _fixture_feats()[:, :57]
    ref, mid = _oracle(sd, f, return_intermediates=True)
    assert float((mid["b1.block"][:, list(CLAMP_CHANNELS)] == 20.0).double().mean()) > 0.5
    model = _engine(sd=sd, key="clamp", max_batch=2, max_frames=64)
    _check(model(torch.from_numpy(np.array(f))).cpu().numpy(), ref, "clamp fixture, embedding")
    r32 = _oracle(sd, f, return_intermediates=True, dtype=torch.float32)[1]
    with model.stopped_after(1):
        model(torch.from_numpy(np.array(f)))
        got = model.tap("block").cpu().numpy()
    assert got.max() == 20.0
    ok, ratio = tap_check("b1.block", got, _cl(mid["b1.block"]), _cl(r32["b1.block"]), K_TAP)
    assert ok, ratio


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_every_tap(prec):
    """Stem, every block's block / mid / cat / sc through stopped_after(n), the three global fusions and pooled, T = 57.
    Measured worst ratios (device error / float32-oracle error): see DESIGN.md."""
    f = _fixture_feats()[:, :57]
    r64 = _oracle(_sd(), f, return_intermediates=True)[1]
    r32 = _oracle(_sd(), f, return_intermediates=True, dtype=torch.float32)[1]
    model = _engine().set_precision(prec)
    x = torch.from_numpy(np.array(f))
    rows, checks = [], []

    def one(tag, tap, key, flat=False):
        got = model.tap(tap).cpu().numpy()
        a, b = (r64[key].numpy(), r32[key].numpy()) if flat else (_cl(r64[key]), _cl(r32[key]))
        checks.append((tag, tap_check(tag, got, a, b, K_TAP, rows)[0]))

    try:
        with model.stopped_after(0):
            model(x)
            one("stem", "stem", "stem")
        for n in range(1, 17):
            with model.stopped_after(n):
                model(x)
                for t in ("mid", "cat", "sc", "block"):
                    if "b%d.%s" % (n, t) in r64:
                        one("b%d.%s" % (n, t), t, "b%d.%s" % (n, t))
        model(x)
        for t in ("fuse12", "fuse123", "fuse1234"):
            one(t, t, t)
        one("pooled", "pooled", "pooled", flat=True)
    finally:
        model.set_precision("fp32")
    _assert_all("ERes2Net34_Base %s T=57" % prec, checks, rows)


def test_dispatch_no_layer_falls_to_a_kernel_without_the_clamp():
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    f = np.random.RandomState(3).randn(8, 200, 80).astype(np.float32)
    model = _engine()
    x = torch.from_numpy(f)
    model(x)
    dispatch_log(True, clear=True)
    try:
        model(x)
        torch.cuda.synchronize()
        lines = dispatch_report()
    finally:
        dispatch_log(False, clear=True)
    print("\n".join(lines))
    # every clamped layer ran on a kernel whose epilogue has ACT_RELU20 (the tile kernels); the persistent fp32 GEMM and
    # the direct 3x3 kernels have none and must have declined
    clamped = [ln for ln in lines if "+relu20" in ln]
    assert sum(int(ln.rsplit("x", 1)[1]) for ln in clamped) >= 16 * 4           # conv1, two branches, conv3 per block
    for ln in clamped:
        assert "conv_gemm_kernel" in ln or "conv_gemm_dual_kernel" in ln, ln
    aff = [ln for ln in lines if "aff_fuse_kernel" in ln]
    assert sum(int(ln.rsplit("x", 1)[1]) for ln in aff) == 12, aff


def test_public_surface(tmp_path):
    import wespeaker_amd
    from wespeaker_amd._lib import NativeError
    from wespeaker_amd.engine import NativeSpeakerModel
    d = str(tmp_path / "m")
    synth.write_model_dir(d, BASE, feat_dim=24, embed_dim=32, seed=42)
    spk = wespeaker_amd.load_model(d, max_batch=4, max_frames=200)
    assert spk.model.model_name == BASE and spk.model.feat_dim == 24 and spk.model.embed_dim == 32
    assert spk.model.ignored_keys == []
    pcm = torch.from_numpy(synth.synth_wav(5))
    e1 = spk.extract_embedding_from_pcm(pcm.unsqueeze(0), 16000)
    feats = spk.compute_features(pcm.unsqueeze(0).to(torch.float32), 16000)
    out = spk.model(feats)
    assert isinstance(out, torch.Tensor)
    assert torch.equal(e1, out[0].cpu())
    _check(e1.numpy()[None], _oracle(_sd(BASE, 24, 32), feats.cpu().numpy()), "load_model -> extract_embedding_from_pcm")
    with pytest.raises(NativeError, match="ERes2Net34_Base has no binary16-tensor back-end"):
        spk.set_precision("f16")
    assert spk.model.precision == "fp32"
    # a checkpoint of another width under this name
    with pytest.raises(NativeError, match="m_channels = 64"):
        NativeSpeakerModel(LARGE, _sd(BASE, 24, 32), feat_dim=24, embed_dim=32, max_batch=2, max_frames=64)


def test_row_permutation_and_lanes_give_the_same_bits():
    from wespeaker_amd.engine import SpeakerModelLanes
    f = np.random.RandomState(8).randn(8, 100, 80).astype(np.float32)
    model = _engine()
    base = model(torch.from_numpy(f))
    perm = np.random.RandomState(9).permutation(8)
    assert torch.equal(model(torch.from_numpy(f[perm])), base[torch.from_numpy(perm).to(base.device)])
    lanes = SpeakerModelLanes(BASE, _sd(), lanes=2, feat_dim=80, embed_dim=192, max_batch=8, max_frames=200)
    x = torch.from_numpy(f).to(model.device)
    r = [lanes.embed(x), lanes.embed(x)]                   # one batch on each lane, in flight together
    for res in r:
        assert torch.equal(res.synchronize(), base)
    assert {res.lane for res in r} == {0, 1}
