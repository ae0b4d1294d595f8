"""XVEC, XI_VEC_XVEC and XI_VEC_ECAPA_TDNN_c512 / _c1024 on the GPU: the engines against the float64 oracle
(tests/tdnn_oracle.py) and the reference-made golden (tests/golden/tdnn_ref.npz); the XI pooling kernel alone through
ws_debug_xi_pool against float64 numpy.

Bars: COS_TOL = 1e-4 and REL_TOL = 2e-4 on embeddings; 1e-5 between a row of a ragged batch and its own batch-1 result;
per-tap parity and the XI kernel: the error against the float64 oracle (scaled max and relative L2) at most k = 8 x the
error of the same formula evaluated in float32, floored at 2^-24 (tests/test_gpu_layers.py: tap_check).

XVEC at T = 15 pools ONE frame with TSTP: the unbiased variance is 0 / 0 in the reference (pooling_layers.py:81), the
golden holds NaN there, and so must the engine (as tests/test_gpu_gemini.py treats its one-frame case).
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

import make_golden_tdnn as mg  # noqa: E402
import tdnn_oracle as to  # noqa: E402
from test_gpu_layers import _assert_all, tap_check  # noqa: E402
from test_tdnn_cpu import NAN_CASE, XI_DEBUG_WINDOWS, write_model_dir, xi_debug_fixture  # noqa: E402

pytestmark = pytest.mark.gpu

COS_TOL = 1e-4
REL_TOL = 2e-4
RAGGED_VS_SINGLE_TOL = 1e-5
K_TAP = 8.0
NARROW = dict(hid_dim=64, stats_dim=100)
ALL_NAMES = (mg.XVEC, mg.XI_XVEC, mg.XI_C512, mg.XI_C1024)


def _rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _check(got, ref, what):
    assert np.isfinite(got).all(), what
    cos, rel = _cos_err(got, ref).max(), _rel_err(got, ref).max()
    print(what, "cos %.2e rel %.2e" % (cos, rel))
    assert cos < COS_TOL and rel < REL_TOL, (what, cos, rel)


def _freeze(d):
    return tuple(sorted(d.items()))


@functools.lru_cache(maxsize=None)
def _sd(name, args, extra):
    return mg.case_state_dict(name, dict(args), dict(extra))


_ENGINES = {}


def _engine(name, args, extra=(), max_batch=4, max_frames=200):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = (name, args, extra, max_batch, max_frames)
    if key not in _ENGINES:
        a = dict(args)
        _ENGINES[key] = NativeSpeakerModel(name, _sd(name, args, extra), feat_dim=a["feat_dim"], embed_dim=a["embed_dim"],
                                           max_batch=max_batch, max_frames=max_frames)
    return _ENGINES[key]


def _narrow(name):
    return _engine(name, _freeze(dict(feat_dim=40, embed_dim=64)), _freeze(NARROW))


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(mg.GOLD))


@functools.lru_cache(maxsize=None)
def _cases():
    return mg.golden_cases()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("key", list(mg.golden_cases()))
def test_forward_parity_with_oracle_and_golden(key, prec):
    name, args, extra, feats = _cases()[key]
    model = _engine(name, _freeze(args), _freeze(extra))
    assert model.ignored_keys == []
    model.set_precision(prec)
    try:
        out = model(torch.from_numpy(np.array(feats)))
        got = out[-1].cpu().numpy()
        if key == NAN_CASE:
            # the reference's own answer: a non-finite embedding, which the range guard of the f16x3 back-end reports
            assert np.isnan(_golden()[key]).all() and np.isnan(got).all()
            if prec != "fp32":
                from wespeaker_amd._lib import NativeError
                with pytest.raises(NativeError):
                    model.check_range()
            return
        model.check_range()
    finally:
        model.set_precision("fp32")
    assert isinstance(out, tuple) and len(out) == 2 and tuple(out[-1].shape) == (feats.shape[0], args["embed_dim"])
    _check(got, _golden()[key], "%s %s vs golden" % (key, prec))
    _check(got, to.forward(name, _sd(name, _freeze(args), _freeze(extra)), feats).numpy(), "%s %s vs oracle" % (key, prec))


def _xi_pool_device(x, z, pm, pl, windows, ldx=None, ldz=None):
    from wespeaker_amd import _lib
    dev = torch.device("cuda", 0)
    B, T, D = x.shape
    ldx, ldz = ldx or D, ldz or D
    xd = torch.full((B * T, ldx), float("nan"), device=dev)
    zd = torch.full((B * T, ldz), float("nan"), device=dev)
    xd[:, :D] = torch.from_numpy(x.reshape(B * T, D)).to(dev)
    zd[:, :D] = torch.from_numpy(z.reshape(B * T, D)).to(dev)
    pmd, pld = torch.from_numpy(pm).to(dev), torch.from_numpy(pl).to(dev)
    out = torch.full((B, D), float("nan"), device=dev)
    win = None if windows is None else np.ascontiguousarray(np.asarray(windows, dtype=np.int32).reshape(-1))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ws_debug_xi_pool(_lib.ptr(xd), ldx, _lib.ptr(zd), ldz, _lib.ptr(pmd), _lib.ptr(pld),
                                               _lib.ptr(out), B, T, D, None if win is None else _lib.ptr(win),
                                               _lib.current_stream_ptr(dev)), "ws_debug_xi_pool")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("windows", XI_DEBUG_WINDOWS)
@pytest.mark.parametrize("D", [100, 1500, 1536])
def test_xi_pool_kernel_against_float64_numpy(D, windows):
    T = 200
    x, z, pm, pl = xi_debug_fixture(D, T)
    r64 = to.xi_pool_windows(x, z, pm, pl, windows)
    r32 = to.xi_pool_windows(x, z, pm, pl, windows, dtype=np.float32)
    rows, checks = [], []
    got = _xi_pool_device(x, z, pm, pl, windows)
    checks.append(("packed", tap_check("packed", got, r64, r32, K_TAP, rows)[0]))
    # rows wider than D (the engines' padded frame tensor), NaN in the padding columns: never read
    wide = _xi_pool_device(x, z, pm, pl, windows, ldx=D + 36, ldz=D + 28)
    assert np.array_equal(wide, got)
    # a row's result does not depend on its batch: utterance 2 alone, bit for bit
    alone = _xi_pool_device(x[2:], z[2:], pm, pl, windows[2:])
    assert np.array_equal(alone[0], got[2])
    _assert_all("xi_pool D=%d %s" % (D, windows), checks, rows)


def test_xi_pool_kernel_scalar_path_and_refusals():
    from wespeaker_amd._lib import NativeError
    x, z, pm, pl = xi_debug_fixture(100, 40)
    x, z, pm, pl = x[:, :, :98], z[:, :, :98], pm[:98], pl[:98]      # D = 98: no 16-byte loads
    win = ((0, 40), (3, 9), (39, 1))
    r64, r32 = to.xi_pool_windows(x, z, pm, pl, win), to.xi_pool_windows(x, z, pm, pl, win, dtype=np.float32)
    ok, ratio = tap_check("D=98", _xi_pool_device(np.ascontiguousarray(x), np.ascontiguousarray(z), pm, pl, win), r64, r32, K_TAP)
    assert ok, ratio
    whole = _xi_pool_device(np.ascontiguousarray(x), np.ascontiguousarray(z), pm, pl, None)
    ok, ratio = tap_check("whole", whole, to.xi_pool_windows(x, z, pm, pl, [(0, 40)] * 3),
                          to.xi_pool_windows(x, z, pm, pl, [(0, 40)] * 3, dtype=np.float32), K_TAP)
    assert ok, ratio
    for bad in (((0, 41), (0, 1), (0, 1)), ((0, 0), (0, 1), (0, 1)), ((-1, 2), (0, 1), (0, 1))):
        with pytest.raises(NativeError, match="ws_debug_xi_pool: window 0"):
            _xi_pool_device(np.ascontiguousarray(x), np.ascontiguousarray(z), pm, pl, bad)


def _rows(t, trim=0):
    """(B, C, Tk) oracle tensor -> (B, Tk, C) numpy."""
    return t.permute(0, 2, 1).contiguous().numpy()


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", [mg.XVEC, mg.XI_XVEC])
def test_xvec_taps_at_each_stop_point(name, prec):
    key = "%s_h64_s100/emb_T57" % name
    _, args, extra, feats = _cases()[key]
    sd = _sd(name, _freeze(args), _freeze(extra))
    r64 = to.xvec_forward(sd, feats, return_intermediates=True)[1]
    r32 = to.xvec_forward(sd, feats, dtype=torch.float32, return_intermediates=True)[1]
    model = _narrow(name).set_precision(prec)
    x = torch.from_numpy(np.array(feats))
    B, T = feats.shape[:2]
    rows, checks = [], []

    def one(tag, tap, okey, trim=None):
        got = model.tap(tap).cpu().numpy()
        a, b = r64[okey], r32[okey]
        if trim is not None:          # frame-level: the engine's rows are T long, the reference's valid ones lie inside
            got = got.reshape(B, T, -1)[:, trim:T - trim]
            a, b = _rows(a), _rows(b)
            assert got.shape == a.shape, (tag, got.shape, a.shape)
        else:
            a, b = a.numpy(), b.numpy()
        checks.append((tag, tap_check(tag, got, a, b, K_TAP, rows)[0]))

    try:
        for n in range(1, 6):
            with model.stopped_after(n):
                emb = model(x)[-1]
                assert float(emb.abs().max()) == 0.0
                assert model.tap_shape("frame") == (B * T, 100 if n == 5 else 64)
                one("frame%d" % n, "frame", "frame%d" % n, to.TRIM[n - 1])
        model(x)
        one("frame5", "frame", "frame5", 7)
        if name == mg.XI_XVEC:
            one("xi_hid", "xi_hid", "xi_hid", 7)
            one("xi_z", "xi_z", "xi_z", 7)
        one("pooled", "pooled", "pooled")
        one("emb_a", "emb_a", "emb_a")
        assert model.tap_shape("pooled") == (B, 100 if name == mg.XI_XVEC else 200)
    finally:
        model.set_precision("fp32")
    _assert_all("%s %s T=57" % (name, prec), checks, rows)


@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_xi_ecapa_taps(prec):
    key = mg.XI_C512 + "/emb_T57"
    name, args, extra, feats = _cases()[key]
    sd = _sd(name, _freeze(args), _freeze(extra))
    r64 = to.xi_ecapa_forward(sd, feats, return_intermediates=True)[1]
    r32 = to.xi_ecapa_forward(sd, feats, dtype=torch.float32, return_intermediates=True)[1]
    model = _engine(name, _freeze(args), _freeze(extra)).set_precision(prec)
    x = torch.from_numpy(np.array(feats))
    B, T = feats.shape[:2]
    rows, checks = [], []
    try:
        for n in (1, 2, 3):          # the stop points of the trunk keep working: cat holds out2 .. out(n + 1)
            with model.stopped_after(n):
                assert float(model(x)[-1].abs().max()) == 0.0
                got = model.tap("cat").cpu().numpy().reshape(B, T, 3, 512)[:, :, n - 1]
                tag = "out%d" % (n + 1)
                checks.append((tag, tap_check(tag, got, _rows(r64[tag]), _rows(r32[tag]), K_TAP, rows)[0]))
        model(x)
        for tap, cols in (("h", 1536), ("xi_hid", 256), ("xi_z", 1536)):
            got = model.tap(tap).cpu().numpy().reshape(B, T, cols)
            checks.append((tap, tap_check(tap, got, _rows(r64[tap]), _rows(r32[tap]), K_TAP, rows)[0]))
        assert model.tap_shape("pooled") == (B, 1536)
        checks.append(("pooled", tap_check("pooled", model.tap("pooled").cpu().numpy(), r64["pooled"].numpy(),
                                           r32["pooled"].numpy(), K_TAP, rows)[0]))
    finally:
        model.set_precision("fp32")
    _assert_all("%s %s T=57" % (name, prec), checks, rows)


def _ragged_case(F):
    lens = [15, 16, 64, 200]
    feats = [np.random.RandomState(300 + i).randn(L, F).astype(np.float32) for i, L in enumerate(lens)]
    pad = np.full((len(lens), max(lens), F), np.nan, dtype=np.float32)
    for i, f in enumerate(feats):
        pad[i, :lens[i]] = f
    return lens, feats, pad


@pytest.mark.parametrize("name", [mg.XI_XVEC, mg.XVEC, mg.XI_C512])
def test_ragged_batch_rows_equal_their_own_batch_of_one(name):
    if name == mg.XI_C512:
        args, extra = _freeze(dict(feat_dim=80, embed_dim=192)), ()
        model = _engine(name, args, extra)
    else:
        args, extra = _freeze(dict(feat_dim=40, embed_dim=64)), _freeze(NARROW)
        model = _narrow(name)
    lens, feats, pad = _ragged_case(dict(args)["feat_dim"])
    got = model.embed_ragged(torch.from_numpy(pad), lens).cpu().numpy()
    for i, f in enumerate(feats):
        one = model(torch.from_numpy(f[None]))[-1].cpu().numpy()
        if name == mg.XVEC and lens[i] == 15:            # TSTP over one frame: NaN in the reference, here, and in the batch
            assert np.isnan(one).all() and np.isnan(got[i]).all()
            continue
        err = _rel_err(got[i:i + 1], one).max()
        print("row %d (%d frames) vs batch of one: %.2e" % (i, lens[i], err))
        assert err < RAGGED_VS_SINGLE_TOL, (i, lens[i], err)
        _check(got[i:i + 1], to.forward(name, _sd(name, args, extra), f[None]).numpy(), "ragged row %d vs oracle" % i)


@pytest.mark.parametrize("name", [mg.XVEC, mg.XI_XVEC])
def test_fourteen_frames_are_refused(name):
    from wespeaker_amd._lib import NativeError
    model = _narrow(name)
    # WS_ERR_INVALID_ARG = -1 (include/wespeaker_amd.h), and the message names 15
    with pytest.raises(NativeError, match=r"\(code -1\): .*at least 15 frames"):
        model(torch.zeros(2, 14, 40))
    pad = torch.zeros(3, 64, 40)
    with pytest.raises(NativeError, match=r"\(code -1\): .*utterance 1 has 14 frames, valid range is \[15, 64\]"):
        model.embed_ragged(pad, [64, 14, 20])
    # the engine is still usable
    assert torch.isfinite(model(torch.randn(1, 20, 40))[-1]).all()


@pytest.mark.parametrize("name,T", [(mg.XVEC, 100), (mg.XI_XVEC, 100), (mg.XI_C512, 57), (mg.XI_C512, 128)])
def test_row_permutation_gives_the_same_bits(name, T):
    """The x-vector engines at any T.  The ECAPA trunk under XI is the existing one: for T >= 64 its SE means come from
    the GEMM epilogue's 64-row tile sums, whose split -- and with it the fp32 summation order, ~1e-7 -- follows the
    utterance's row offset unless T is a multiple of 64 (tests/test_gpu_parity.py:842 pins 1e-5 there); so the bits
    are pinned where the trunk is position independent: below 64 frames and at a multiple of 64.  The XI tail itself
    (xi_pool_kernel) is pinned for any window in test_xi_pool_kernel_against_float64_numpy."""
    if name == mg.XI_C512:
        model, F = _engine(name, _freeze(dict(feat_dim=80, embed_dim=192)), ()), 80
    else:
        model, F = _narrow(name), 40
    f = np.random.RandomState(8).randn(4, T, F).astype(np.float32)
    base = model(torch.from_numpy(f))[-1]
    perm = np.array([2, 0, 3, 1])
    assert torch.equal(model(torch.from_numpy(f[perm]))[-1], base[torch.from_numpy(perm).to(base.device)])


@pytest.mark.parametrize("name", ALL_NAMES)
def test_binary16_tensor_backend_is_refused(name):
    from wespeaker_amd._lib import NativeError
    if name in (mg.XVEC, mg.XI_XVEC):
        model = _narrow(name)
    else:
        model = _engine(name, _freeze(dict(feat_dim=80, embed_dim=192)), ())
    with pytest.raises(NativeError, match="%s has no binary16-tensor back-end" % name):
        model.set_precision("f16")
    assert model.precision == "fp32"


@pytest.mark.parametrize("name", [mg.XVEC, mg.XI_C512])
def test_speaker_end_to_end_from_a_model_directory(tmp_path, name):
    import wespeaker_amd
    from fixtures import synth
    if name == mg.XVEC:
        args, extra = dict(feat_dim=40, embed_dim=64), NARROW
    else:
        args, extra = dict(feat_dim=80, embed_dim=192), {}
    sd = _sd(name, _freeze(args), _freeze(extra))
    d = str(tmp_path / "m")
    write_model_dir(d, name, sd, pooling_func="TSTP" if name == mg.XVEC else "XI", **args)
    spk = wespeaker_amd.load_model(d, max_batch=4, max_frames=200)
    assert spk.model.model_name == name and spk.model.embed_dim == args["embed_dim"] and spk.model.ignored_keys == []
    pcm = torch.from_numpy(synth.synth_wav(5))
    e1 = spk.extract_embedding_from_pcm(pcm.unsqueeze(0), 16000)
    feats = spk.compute_features(pcm.unsqueeze(0).to(torch.float32), 16000)
    out = spk.model(feats)
    assert isinstance(out, tuple) and torch.equal(e1, out[-1][0].cpu())
    # embed_b (XVEC) / the embedding (ECAPA): the last element of the reference's tuple
    _check(e1.numpy()[None], to.forward(name, sd, feats.cpu().numpy()).numpy(), "load_model -> extract_embedding_from_pcm")
    spk.model.set_precision("f16x3")
    try:
        spk.model(feats)
        spk.model.check_range()
    finally:
        spk.model.set_precision("fp32")
    assert spk.model.flops(1, 200) > 0
