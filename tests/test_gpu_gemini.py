"""Gemini_DF_ResNet60 / 114 / 183 / 237 on the GPU: the engine against the float64 oracle (tests/gemini_oracle.py) and
the reference-made golden (tests/golden/gemini_ref.npz).

Bars (those of tests/test_gpu_eres2net.py): COS_TOL = 1e-4 and REL_TOL = 2e-4 on embeddings; 1e-5 between a row of a
ragged batch and its own batch-1 result; per-tap parity: a tap's error against the float64 oracle (scaled max and
relative L2) at most k = 8 x the error of the float32 oracle, floored at 2^-24 (tests/test_gpu_layers.py: tap_check).
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

import gemini_oracle as go  # noqa: E402
import make_golden_gemini as mg  # noqa: E402
from fixtures import synth  # noqa: E402
from test_gpu_layers import _assert_all, tap_check  # noqa: E402

pytestmark = pytest.mark.gpu

COS_TOL = 1e-4
REL_TOL = 2e-4
RAGGED_VS_SINGLE_TOL = 1e-5
K_TAP = 8.0
G60, G114, G183, G237 = mg.G60, mg.G114, mg.G183, mg.G237


def _rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


@functools.lru_cache(maxsize=None)
def _sd(name=G60, feat_dim=80, embed_dim=256, two=False):
    return synth.synth_gemini_state_dict(name, feat_dim, embed_dim, two_emb_layer=two, seed=42)


_ENGINES = {}


def _engine(name=G60, feat_dim=80, embed_dim=256, two=False, max_batch=8, max_frames=200):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = (name, feat_dim, embed_dim, two, max_batch, max_frames)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, _sd(name, feat_dim, embed_dim, two), feat_dim=feat_dim,
                                           embed_dim=embed_dim, max_batch=max_batch, max_frames=max_frames)
    return _ENGINES[key]


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(mg.GOLD))


@functools.lru_cache(maxsize=None)
def _cases():
    return mg.golden_cases()


def _oracle(sd, feats, name=G60, **kw):
    out = go.gemini_forward(sd, np.array(feats), name, **kw)
    return out.numpy() if not isinstance(out, tuple) else (out[0].numpy(), out[1])


def _check(got, ref, what):
    assert np.isfinite(got).all(), what
    cos, rel = _cos_err(got, ref).max(), _rel_err(got, ref).max()
    print(what, "cos %.2e rel %.2e" % (cos, rel))
    assert cos < COS_TOL and rel < REL_TOL, (what, cos, rel)


def _cl(t):
    """(B, C, F, T) oracle map -> the engine's rows (B*F*T, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).numpy()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("key", [G60 + "/emb", G60 + "/emb_T57", G60 + "_f32/emb_T33", G60 + "_f16/emb_T9",
                                 G60 + "_two/emb_T57", G114 + "/emb_T57", G237 + "/emb_T57"])
def test_forward_parity_with_oracle_and_golden(key, prec):
    name, args, feats = _cases()[key]
    two = args.get("two_emb_layer", False)
    small = name != G60
    model = _engine(name, args["feat_dim"], args["embed_dim"], two, max_batch=2 if small else 8,
                    max_frames=64 if small else 200)
    assert model.ignored_keys == []
    model.set_precision(prec)
    try:
        out = model(torch.from_numpy(np.array(feats)))
        model.check_range()
    finally:
        model.set_precision("fp32")
    # the reference's tuple shape (gemini_dfresnet.py:129-141); its callers use the last element
    assert isinstance(out, tuple) and len(out) == 2 and tuple(out[-1].shape) == (feats.shape[0], args["embed_dim"])
    got = out[-1].cpu().numpy()
    _check(got, _golden()[key], "%s %s vs golden" % (key, prec))
    _check(got, _oracle(_sd(name, args["feat_dim"], args["embed_dim"], two), feats, name), "%s %s vs oracle" % (key, prec))


def _stride_chain(F, T):
    """(F, T) after each downsample layer: (n - 1) // 2 + 1 on every strided axis."""
    out = []
    for st in go.STRIDE_T:
        F = (F - 1) // 2 + 1
        if st == 2:
            T = (T - 1) // 2 + 1
        out.append((F, T))
    return out


@pytest.mark.parametrize("T", [1, 9, 57, 64, 131])
def test_odd_lengths_through_the_strided_layers(T):
    f = np.random.RandomState(T).randn(2, T, 80).astype(np.float32)
    model = _engine()
    got = model(torch.from_numpy(f))[-1].cpu().numpy()
    ref, mid = _oracle(_sd(), f, return_intermediates=True)
    pts = go.stop_points(G60)
    chain = _stride_chain(80, T)
    Fl, Tl = chain[-1]
    assert model.tap_shape("block") == (2 * Fl * Tl, 256) and model.tap_shape("pooled") == (2, 2 * 256 * Fl)
    if Tl >= 2:
        _check(got, ref, "T = %d" % T)
    else:
        # one frame left: TSTP's unbiased variance is 0 / 0 in the reference too (pooling_layers.py:83) -- the std half
        # of the statistics and with it the embedding are NaN there and here; the maps and the mean half are checked
        assert np.isnan(ref).all() and np.isnan(got).all()
        r32 = _oracle(_sd(), f, return_intermediates=True, dtype=torch.float32)[1]
        ok, ratio = tap_check("block", model.tap("block").cpu().numpy(), _cl(mid["u%d.block" % len(pts)]),
                              _cl(r32["u%d.block" % len(pts)]), K_TAP)
        assert ok, ratio
        D = 256 * Fl
        ok, ratio = tap_check("mean", model.tap("pooled").cpu().numpy()[:, :D], mid["pooled"].numpy()[:, :D],
                              r32["pooled"].numpy()[:, :D], K_TAP)
        assert ok, ratio
    for n, pt in enumerate(pts, 1):                       # every downsample layer's output shape
        if pt[0] == "ds":
            with model.stopped_after(n):
                model(torch.from_numpy(f))
                Fk, Tk = chain[pt[1] - 1]
                assert model.tap_shape("ds") == (2 * Fk * Tk, synth.GEMINI_DIMS[pt[1]])


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_every_tap(prec):
    """Stem, every downsample layer's ds and every block's exp / dw / block through stopped_after(n), and pooled, T = 57.

    Measured on MI355X (worst ratio = device error / float32-oracle error over the 60 taps): fp32 2.56 (u20.block;
    pooled 1.43), f16x3 1.93 (u3.block; last block 1.65, pooled 1.46).  The f16x3 figures depend on the binary16 planes of
    conv3 and of the downsample layers being cut from 2^k W (gemini_model.hip, "f16x3 and small weights"): cut from W
    itself, their subnormal lo halves put the last block at 4.3 and `pooled` at 8.89, beyond the bound."""
    name, args, feats = _cases()[G60 + "/emb_T57"]
    r64 = _oracle(_sd(), feats, return_intermediates=True)[1]
    r32 = _oracle(_sd(), feats, return_intermediates=True, dtype=torch.float32)[1]
    model = _engine().set_precision(prec)
    x = torch.from_numpy(np.array(feats))
    rows, checks = [], []

    def one(tag, tap, key, flat=False):
        got = model.tap(tap).cpu().numpy()
        a, b = (r64[key].numpy(), r32[key].numpy()) if flat else (_cl(r64[key]), _cl(r32[key]))
        checks.append((tag, tap_check(tag, got, a, b, K_TAP, rows)[0]))

    try:
        with model.stopped_after(0):
            model(x)
            one("stem", "stem", "stem")
        for n, pt in enumerate(go.stop_points(G60), 1):
            with model.stopped_after(n):
                model(x)
                for t in (("ds",) if pt[0] == "ds" else ("exp", "dw", "block")):
                    one("u%d.%s" % (n, t), t, "u%d.%s" % (n, t))
        model(x)
        one("pooled", "pooled", "pooled", flat=True)
    finally:
        model.set_precision("fp32")
    _assert_all("%s %s T=57" % (G60, prec), checks, rows)


def test_deepest_model_last_block_of_each_stage_and_pooled():
    name, args, feats = _cases()[G237 + "/emb_T57"]
    r64 = _oracle(_sd(G237), feats, G237, return_intermediates=True)[1]
    r32 = _oracle(_sd(G237), feats, G237, return_intermediates=True, dtype=torch.float32)[1]
    model = _engine(G237, max_batch=2, max_frames=64)
    x = torch.from_numpy(np.array(feats))
    pts = go.stop_points(G237)
    assert len(pts) == 81
    rows, checks = [], []
    for n, pt in enumerate(pts, 1):
        if pt[0] == "block" and (n == len(pts) or pts[n][0] == "ds"):         # the last block of its stage
            with model.stopped_after(n):
                model(x)
                key = "u%d.block" % n
                checks.append((key, tap_check(key, model.tap("block").cpu().numpy(), _cl(r64[key]), _cl(r32[key]), K_TAP, rows)[0]))
    assert len(checks) == 4
    model(x)
    checks.append(("pooled", tap_check("pooled", model.tap("pooled").cpu().numpy(), r64["pooled"].numpy(),
                                       r32["pooled"].numpy(), K_TAP, rows)[0]))
    _assert_all(G237 + " fp32 T=57", checks, rows)


def test_two_embedding_layers_tap():
    name, args, feats = _cases()[G60 + "_two/emb_T57"]
    model = _engine(G60, two=True)
    model(torch.from_numpy(feats))
    _, mid = _oracle(_sd(two=True), feats, return_intermediates=True)
    err = _rel_err(model.tap("emb_a").cpu().numpy(), mid["emb_a"].numpy()).max()
    assert err < REL_TOL, err


def test_ragged_batch_rows_equal_their_own_batch_of_one():
    lens = [200, 199, 131, 57, 9, 3]
    feats = [np.random.RandomState(100 + i).randn(L, 80).astype(np.float32) for i, L in enumerate(lens)]
    pad = np.full((len(lens), max(lens), 80), np.nan, dtype=np.float32)
    for i, f in enumerate(feats):
        pad[i, :lens[i]] = f
    model = _engine()
    got = model.embed_ragged(torch.from_numpy(pad), lens).cpu().numpy()
    assert np.isfinite(got).all()
    blk = model.tap("block").cpu().numpy().reshape(len(lens), 5, 100, 256)
    dw = model.tap("dw").cpu().numpy().reshape(len(lens), 5, 100, 1024)
    for i, L in enumerate(lens):
        L1 = (L - 1) // 2 + 1
        assert (blk[i, :, L1:] == 0.0).all() and (dw[i, :, L1:] == 0.0).all(), i      # exact-zero padding columns
        assert np.abs(blk[i, :, :L1]).max() > 0
    for i, f in enumerate(feats):
        one = model(torch.from_numpy(f[None]))[-1].cpu().numpy()
        err = _rel_err(got[i:i + 1], one).max()
        print("row %d (%d frames) vs batch of one: %.2e" % (i, lens[i], err))
        assert err < RAGGED_VS_SINGLE_TOL, (i, lens[i], err)
        _check(got[i:i + 1], _oracle(_sd(), f[None]), "ragged row %d vs oracle" % i)


def test_row_permutation_and_lanes_give_the_same_bits():
    from wespeaker_amd.engine import SpeakerModelLanes
    f = np.random.RandomState(8).randn(8, 100, 80).astype(np.float32)
    model = _engine()
    base = model(torch.from_numpy(f))[-1]
    perm = np.random.RandomState(9).permutation(8)
    assert torch.equal(model(torch.from_numpy(f[perm]))[-1], base[torch.from_numpy(perm).to(base.device)])
    lanes = SpeakerModelLanes(G60, _sd(), lanes=2, feat_dim=80, embed_dim=256, max_batch=8, max_frames=200)
    x = torch.from_numpy(f).to(model.device)
    r = [lanes.embed(x), lanes.embed(x)]                   # one batch on each lane, in flight together
    for res in r:
        assert torch.equal(res.synchronize(), base)
    assert {res.lane for res in r} == {0, 1}


def test_dispatch_no_block_layer_on_an_unexpected_kernel():
    """A 256 x 200 batch: every block's conv1 and conv3 (1x1, N = 4 dim / dim) runs on the persistent fp32 GEMM where that
    kernel takes the problem -- N a multiple of 128 and K >= 128, its documented floor of four K-tiles
    (gemm_f32_stream_rows) -- and otherwise (stage 1 / 2: K = 32, 64 or N = 32, 64; rows behind the last whole round) on
    the MFMA tile kernels; the depthwise kernel runs once per block."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    model = _engine(G60, max_batch=256, max_frames=200)
    x = torch.from_numpy(np.random.RandomState(3).randn(256, 200, 80).astype(np.float32))
    model(x)
    dispatch_log(True, clear=True)
    try:
        model(x)
        torch.cuda.synchronize()
        lines = dispatch_report()
    finally:
        dispatch_log(False, clear=True)
    print("\n".join(lines))
    count = lambda ln: int(ln.rsplit("x", 1)[1])  # noqa: E731
    dw = [ln for ln in lines if "dwconv3x3_kernel" in ln]
    assert sum(count(ln) for ln in dw) == 18, dw
    assert sorted(int(ln.split("C=")[1].split()[0]) for ln in dw) == [128, 256, 512, 1024]
    one_by_one = [ln for ln in lines if " k=1x1 " in ln and "rows=256 " not in ln]
    for ln in one_by_one:
        assert ("gemm_f32_stream_kernel" in ln or "conv_gemm_kernel" in ln or "conv_gemm_dual_kernel" in ln), ln
    # conv3 carries the residual, conv1 does not: 18 of each, whatever the split between main tiles and remaining rows
    res = [ln for ln in one_by_one if "+res" in ln]
    assert sum(count(ln) for ln in res) >= 18 and sum(count(ln) for ln in one_by_one if "+res" not in ln) >= 18
    # the wide layers (N >= 128) with K >= 128 of a batch this size belong on the persistent kernel
    for ln in one_by_one:
        n, k = int(ln.split(" N=")[1].split()[0]), int(ln.split(" K=")[1].split()[0])
        if n >= 128 and k >= 128 and "gemm_f32_stream_kernel" not in ln:
            rows_ = int(ln.split("rows=")[1].split()[0])
            assert rows_ < 256 * 5 * 100, "a wide 1x1 layer fell off the persistent GEMM: " + ln
    strided = [ln for ln in lines if " k=3x3 " in ln]
    assert sum(count(ln) for ln in strided) == 4 and all("s=2x1" in ln or "s=2x2" in ln for ln in strided), strided


def test_public_surface(tmp_path):
    import wespeaker_amd
    from wespeaker_amd._lib import NativeError
    from wespeaker_amd.engine import NativeSpeakerModel
    d = str(tmp_path / "m")
    synth.write_model_dir(d, G60, feat_dim=32, embed_dim=32, seed=42)
    spk = wespeaker_amd.load_model(d, max_batch=4, max_frames=200)
    assert spk.model.model_name == G60 and spk.model.feat_dim == 32 and spk.model.embed_dim == 32
    assert spk.model.ignored_keys == []
    pcm = torch.from_numpy(synth.synth_wav(5))
    e1 = spk.extract_embedding_from_pcm(pcm.unsqueeze(0), 16000)
    feats = spk.compute_features(pcm.unsqueeze(0).to(torch.float32), 16000)
    out = spk.model(feats)
    assert isinstance(out, tuple) and float(out[0]) == 0.0
    assert torch.equal(e1, out[-1][0].cpu())
    _check(e1.numpy()[None], _oracle(_sd(G60, 32, 32), feats.cpu().numpy()), "load_model -> extract_embedding_from_pcm")
    with pytest.raises(NativeError, match="Gemini_DF_ResNet60 has no binary16-tensor back-end"):
        spk.set_precision("f16")
    assert spk.model.precision == "fp32"
    with pytest.raises(NativeError, match="feat_dim % 16 == 0, got 40"):
        NativeSpeakerModel(G60, synth.synth_gemini_state_dict(G60, 40, 32), feat_dim=40, embed_dim=32, max_batch=2, max_frames=64)
    # the flat weight file of the native runtime: same bits as the state_dict engine
    from wespeaker_amd.engine import save_native_model
    path = save_native_model(str(tmp_path / "g.wsamd"), G60, _sd(G60, 32, 32), feat_dim=32, embed_dim=32)
    native = NativeSpeakerModel.from_file(path, max_batch=4, max_frames=200)
    assert native.model_name == G60 and torch.equal(native(feats)[-1], out[-1])
    with pytest.raises(NativeError, match="unknown model 'Gemini_DF_ResNet61'"):
        NativeSpeakerModel("Gemini_DF_ResNet61", _sd(G60, 32, 32), feat_dim=32, embed_dim=32, max_batch=2, max_frames=64)


def test_extract_windows_matches_window_by_window():
    """Diarization sub-segment embeddings (ws_extract_windows) equal the per-window forward, as for ResNet."""
    from wespeaker_amd.engine import Frontend
    model = _engine()
    fe = Frontend(16000, 80, device=model.device)
    pcm = torch.from_numpy(synth.synth_wav(3, 16000 * 3))
    emb = model.extract_windows(fe, pcm, window_frames=150, period_frames=75)
    assert emb.shape[1] == 256 and emb.shape[0] >= 2 and torch.isfinite(emb).all()
    feats = fe.fbank(pcm.unsqueeze(0), cmn=False)[0]
    w0 = feats[:150]
    w0 = (w0 - w0.mean(0, keepdim=True)).unsqueeze(0)
    one = model(w0)[-1]
    assert _rel_err(emb[:1].cpu().numpy(), one.cpu().numpy()).max() < RAGGED_VS_SINGLE_TOL
