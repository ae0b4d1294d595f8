"""Per-block ResNet / SimAM-ResNet parity: the tensors each residual block leaves in the engine's rotating buffers
(ws_debug_engine_stop_after + ws_debug_engine_tap) against the float64 oracle, block by block.

tests/test_gpu_parity.py and tests/test_gpu_samresnet.py judge the 2-D families by the embedding alone, at
REL_TOL = 2e-4 -- 400 .. 1000x what a faithful fp32 forward needs (fp32 oracle vs float64 oracle: <= 5.2e-7 at the stem
and at every block output), behind up to 73 blocks, a pooling over all frames and a K = 5120 .. 20480 linear.  Both
models rotate four activation buffers, so after a forward only the last block's tensors survive: the engine is told to
return after the stem / after block n, and the taps read what those launches left.

    reference   oracle.resnet.resnet_forward / tests/simam_oracle.py, dtype=torch.float64, return_intermediates=True
    metric      tests/test_gpu_layers.py: scaled max error and relative L2 (tap_errors)
    bound       k x the same metric of the fp32 CPU oracle against the float64 oracle, same inputs, same tap, oracle
                error floored at 2^-24 (tap_check)
    k           8 for every tap, fp32 and f16x3: the rationale of tests/test_gpu_layers.py (two fp32 summation orders,
                each about as far from the truth as the other; f16x3's 2^-21 product errors average out under the fp32
                accumulation).  test_the_per_block_bound_has_teeth (CPU) keeps it from drifting up.

Tap names: stem (stopped at 0), block / mid / sc / next_y1 of the last executed block, pooled / emb_a after a full
forward (include/wespeaker_amd.h).  Every test prints its table (run with -s).

Measured on MI355X -- worst ratio = device error / fp32-oracle error (worst of the two metrics) over EVERY case of this
file, per tap kind, with the case that gave it (oracle32 / device: error against the float64 oracle in that case):

    family, back-end   tap       worst   case                               oracle32   device
    ResNet fp32        stem      0.95    ResNet18 T=64                      1.3e-07    1.3e-07
                       block     3.11    ResNet50 T=9, block 15             2.4e-07    7.5e-07
                       mid       4.57    ragged ResNet18, block 8, utt 0    3.4e-07    1.5e-06
                       sc        2.88    ResNet50 T=9, block 14             2.5e-07    7.1e-07
                       next_y1   2.14    ragged ResNet50, block 2, utt 2    2.9e-07    6.2e-07
                       pooled    1.79    ResNet34 head                      1.8e-07    2.8e-07
                       emb_a     0.58    ResNet34 two_emb head              1.0e-06    5.1e-07
                       emb       0.78    ResNet34 two_emb head              9.0e-07    7.1e-07
    ResNet f16x3       stem      0.95    ResNet18 T=64                      1.3e-07    1.3e-07
                       block     4.92    ResNet34 T=57, block 16            3.6e-07    1.7e-06
                       mid       5.32    ResNet34 T=131, block 14           5.2e-07    2.8e-06
                       sc        4.21    ResNet34 T=57, block 14            3.4e-07    1.5e-06
    SimAM fp32         stem      0.86    ragged, utt 2                      1.4e-07    1.2e-07
                       block     3.99    ragged, block 10, utt 0            3.6e-07    1.4e-06
                       mid       5.64    ragged, block 16, utt 0            5.0e-07    2.8e-06
                       sc        2.88    T=57, block 14                     4.2e-07    1.2e-06
                       hid       5.10    T=9                                5.8e-07    3.0e-06
                       logits    3.35    T=57                               6.8e-07    2.1e-06
                       pooled    2.66    T=57                               1.1e-06    2.2e-06
                       emb       1.17    T=57                               1.7e-06    1.8e-06
No tap needs more than k = 8; the largest ratio anywhere is 5.64.  The large-batch kernels (direct 3x3, the persistent
kernel's convolution forms on 256 x 64 / 256 x 128 tiles and its masked twins, the plain 1x1 + residual form, the dual
tile kernel) stay below 3.9.  No kernel had to be changed.  DESIGN.md carries the same table.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import simam_oracle as so  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import fbank as ofbank  # noqa: E402
from oracle import resnet as oresnet  # noqa: E402
from test_gpu_layers import ERR_FLOOR, REL_TOL, _assert_all, tap_check, tap_errors  # noqa: E402,F401

MAP_TAPS = ("stem", "block", "mid", "sc", "next_y1")
HEAD_TAPS = ("pooled", "emb_a", "emb")
SIMAM_TAPS = ("stem", "block", "mid", "sc", "hid", "logits", "pooled", "emb")
K = {p: {t: 8.0 for t in set(MAP_TAPS + HEAD_TAPS + SIMAM_TAPS)} for p in ("fp32", "f16x3")}
S34 = "SimAM_ResNet34_ASP"


def _kind(key):
    return key.split(".")[-1]


# ---------------------------------------------------------------------------------------------- the oracle side (CPU)
@functools.lru_cache(maxsize=None)
def _sd(name, two_emb=False):
    kw = {"two_emb_layer": True} if two_emb else {}
    return synth.synth_state_dict(name, 80, 256, seed=42, **kw)


@functools.lru_cache(maxsize=None)
def _fixture_feats():
    f = np.stack([ofbank.speaker_features(synth.synth_wav(i)) for i in range(3)])
    f.setflags(write=False)
    return f


def _cl(t):
    """(B, C, F, T) -> the engine's [b][f][t][c]."""
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def n_blocks(name):
    return sum(so.LAYOUTS[name]) if name in so.LAYOUTS else sum(oresnet.LAYOUTS[name][1])


def fused_next(name, i, prec):
    """Does block i (1-based) of `name` run bneck_c3c1_kernel -- conv3 of this block with conv1 of the next -- in the
    `prec` back-end?  fp32 Bottleneck nets, 32 -> 32 / 32 -> 64 / 64 -> 64 planes (resnet_model.hip)."""
    if name not in oresnet.LAYOUTS or not oresnet.LAYOUTS[name][0] or prec != "fp32" or i >= n_blocks(name):
        return False
    planes = [32 << s for s, nb in enumerate(oresnet.LAYOUTS[name][1]) for _ in range(nb)]
    p, pn = planes[i - 1], planes[i]
    return (p == 32 and pn in (32, 64)) or (p == 64 and pn == 64)


def oracle_taps(name, feats, dtype, two_emb=False):
    """key -> numpy array in the engine's layout.  Keys: 'stem', 'b<i>.block' / '.mid' / '.sc' / '.next_y1' (i 1-based;
    next_y1 of block i = the oracle's conv1 + bn1 + relu of block i + 1), 'pooled', 'emb_a', 'emb'."""
    sd = _sd(name, two_emb)
    if name in so.LAYOUTS:
        emb, mid = so.simam_resnet_forward(sd, np.array(feats), name, return_intermediates=True, dtype=dtype)
        out = {"stem": _cl(mid["stem"]), "pooled": mid["pooled"].numpy(), "emb": emb.numpy(),
               "hid": mid["hid"].permute(0, 2, 1).contiguous().numpy()}
        last = mid["b%d.block" % n_blocks(name)]
        B, C, Fl, Tl = last.shape
        out["logits"] = mid["logits"].reshape(B, C, Fl, Tl).permute(0, 3, 2, 1).reshape(B, Tl, Fl * C).contiguous().numpy()
        for k, v in mid.items():
            if k[0] == "b" and "." in k:
                out[k] = _cl(v)
        return out
    emb, mid = oresnet.resnet_forward(sd, np.array(feats), name, dtype=dtype, return_intermediates=True)
    out = {"stem": _cl(mid["stem"]), "pooled": mid["pooled"].numpy(), "emb_a": mid["emb_a"].numpy(), "emb": emb.numpy()}
    for i, t in enumerate(mid["blocks"], 1):
        for k in ("block", "mid", "sc"):
            if k in t:
                out["b%d.%s" % (i, k)] = _cl(t[k])
        if i < len(mid["blocks"]) and "y1" in mid["blocks"][i]:
            out["b%d.next_y1" % i] = _cl(mid["blocks"][i]["y1"])
    return out


@functools.lru_cache(maxsize=2)
def _fixture_refs(name, T):
    """(float64 taps, fp32 taps) of the fixture features cut to T frames; shared by the two precisions of a case."""
    f = _fixture_feats()[:, :T]
    return oracle_taps(name, f, torch.float64), oracle_taps(name, f, torch.float32)


def _keys_at(name, n, prec, r64):
    """The taps that exist when `name` is stopped after block n, as oracle keys."""
    if n == 0:
        return ["stem"]
    keys = ["b%d.block" % n, "b%d.mid" % n]
    if "b%d.sc" % n in r64:
        keys.append("b%d.sc" % n)
    if fused_next(name, n, prec):
        keys.append("b%d.next_y1" % n)
    return keys


def test_the_per_block_bound_has_teeth():
    """Why this file exists (CPU): errors that the embedding bar lets through must fail the per-tap bound.  ResNet34,
    two 57-frame fixture utterances, fed to the very comparison the GPU tests use:
      * one 32-pixel x 32-channel tile of a stage-2 block output (block 5) scaled by 1 + 1e-4 -- a wrong BN scale in
        one column tile, a dropped K-tile;
      * the t = 0 border column of one channel of a stage-3 mid (block 9's conv1 output; the channel of median range)
        shifted by 1e-4 of that channel's range -- a wrong border tap.
    Both leave the embedding inside REL_TOL (oracle.resnet.resnet_resume runs the forward's own tail) and both are
    refused at the k in force.  Both oracles themselves pass every tap."""
    name = "ResNet34"
    sd, f = _sd(name), _fixture_feats()[:2, :57]
    r64, r32 = oracle_taps(name, f, torch.float64), oracle_taps(name, f, torch.float32)
    k = K["fp32"]
    rows = []
    for t in r64:
        assert tap_check(t, r64[t], r64[t], r32[t], k[_kind(t)])[0]
        assert tap_check(t, r32[t], r64[t], r32[t], k[_kind(t)], rows)[0], rows[-1]
    # the slack the issue measured: the fp32 oracle is below 1e-6 of the float64 one at the stem and every block output
    assert max(max(tap_errors(r32[t], r64[t])) for t in r64 if _kind(t) in ("stem", "block")) < 1e-6, rows
    emb64 = r64["emb"]
    rel = lambda e: float((np.linalg.norm(e - emb64, axis=1) / np.linalg.norm(emb64, axis=1)).max())
    cf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)          # back to channels first
    eps = 1e-4

    blk = r64["b5.block"]                                          # (B, 40, 29, 64)
    B, H, W, C = blk.shape
    bad = blk.reshape(B, H * W, C).copy()
    bad[0, 320:352, 16:48] *= 1.0 + eps
    bad = bad.reshape(blk.shape)
    ok, ratio = tap_check("b5.block", bad, blk, r32["b5.block"], k["block"], rows)
    assert not ok and ratio > k["block"], rows
    e_bad = oresnet.resnet_resume(sd, name, torch.float64, after_block=5, x=cf(bad)).numpy()
    assert 0.0 < rel(e_bad) < REL_TOL, rel(e_bad)

    mid = r64["b9.mid"]                                            # (B, 20, 15, 128)
    rng = mid.max(axis=(0, 1, 2)) - mid.min(axis=(0, 1, 2))
    c = int(np.argsort(rng)[mid.shape[3] // 2])
    bad = mid.copy()
    bad[:, :, 0, c] += eps * rng[c]
    ok, ratio = tap_check("b9.mid", bad, mid, r32["b9.mid"], k["mid"], rows)
    assert not ok and ratio > k["mid"], rows
    e_bad = oresnet.resnet_resume(sd, name, torch.float64, after_block=9, x=cf(r64["b8.block"]), mid=cf(bad)).numpy()
    assert 0.0 < rel(e_bad) < REL_TOL, rel(e_bad)
    # resnet_resume is the forward's own tail: unperturbed it returns the embedding, from a block and from a mid
    assert rel(oresnet.resnet_resume(sd, name, torch.float64, after_block=5, x=cf(blk)).numpy()) < 1e-12
    assert rel(oresnet.resnet_resume(sd, name, torch.float64, after_block=9, x=cf(r64["b8.block"]), mid=cf(mid)).numpy()) < 1e-12
    print("\n".join(rows))


# ------------------------------------------------------------------------------------------------------- GPU side
_ENGINES = {}


def _engine(name, max_batch=8, max_frames=208, two_emb=False):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = (name, max_batch, max_frames, two_emb)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, _sd(name, two_emb), feat_dim=80, embed_dim=256, max_batch=max_batch,
                                           max_frames=max_frames)
    return _ENGINES[key]


def _read(model, tap, like, spots=None):
    """The device's `tap` in the shape of the oracle array `like` ((B, H, W, C) or (B, cols)); `spots`: those utterances
    only, sliced on the device before the host copy."""
    v = model.tap(tap)
    if spots is not None:
        v = v.reshape((-1,) + tuple(like.shape[1:]))[torch.as_tensor(spots, device=v.device)]
    got = v.cpu().numpy()
    assert got.size == like.size, (tap, tuple(v.shape), like.shape)
    return got.reshape(like.shape)


def _run(model, feats, n, lens=None):
    """One forward stopped after block n (-1: the full forward) -> embeddings (numpy)."""
    x = torch.from_numpy(np.ascontiguousarray(feats))
    with model.stopped_after(n):
        out = model.embed_ragged(x, lens) if lens is not None else model.embed(x)
    emb = out.cpu().numpy()
    if n >= 0:
        assert not emb.any(), "a stopped forward must return zeros"
    return emb


def _check_stops(tag, name, prec, feats, stops, r64, r32, rows, checks, spots=None, model=None):
    model = model or _engine(name)
    for n in stops:
        _run(model, feats, n)
        for key in _keys_at(name, n, prec, r64):
            got = _read(model, _kind(key), r64[key], spots)
            checks.append((key, tap_check(key, got, r64[key], r32[key], K[prec][_kind(key)], rows)[0]))
        if n >= 1:       # what does not exist is refused, with the reason
            from wespeaker_amd._lib import NativeError
            if "b%d.sc" % n not in r64:
                with pytest.raises(NativeError, match="no (shortcut|downsample) convolution"):
                    model.tap_shape("sc")
            if name in oresnet.LAYOUTS and not fused_next(name, n, prec):
                with pytest.raises(NativeError, match="did not run the fused"):
                    model.tap_shape("next_y1")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("T", [57, 9, 64, 131])
@pytest.mark.parametrize("name", ["ResNet18", "ResNet34", "ResNet50"])
def test_every_block_small_uniform_batch(name, T, prec):
    """B = 3 fixture utterances cut to T frames, stopped at 0 .. n_blocks: every tap that exists at that stop.  Odd T:
    (L - 1) / 2 + 1 at all three strides.  ResNet50 at T = 57: 13 680 stage-1 pixels, not a multiple of 32 --
    bneck_c3c1_kernel's partial pixel block, through block and next_y1."""
    model = _engine(name).set_precision(prec)
    r64, r32 = _fixture_refs(name, T)
    rows, checks = [], []
    try:
        _check_stops("", name, prec, _fixture_feats()[:, :T], range(n_blocks(name) + 1), r64, r32, rows, checks)
    finally:
        model.set_precision("fp32")
    _assert_all("%s %s T=%d" % (name, prec, T), checks, rows)


def _stage_stops(name):
    """0, then the first, second and last block of each stage."""
    stops, first = [0], 1
    for nb in oresnet.LAYOUTS[name][1]:
        stops += sorted({first, min(first + 1, first + nb - 1), first + nb - 1})
        first += nb
    return stops


@pytest.mark.gpu
def test_deep_layout_first_second_and_last_block_of_each_stage():
    """ResNet221, B = 2, T = 57, fp32: block / mid / sc / next_y1 at 13 stops.  Both fusion transitions (32 -> 64 at the
    end of stage 1, 64 -> 64 inside stage 2) and the unfused 64 -> 128 fallback at the end of stage 2."""
    name = "ResNet221"
    f = _fixture_feats()[:2, :57]
    r64, r32 = oracle_taps(name, f, torch.float64), oracle_taps(name, f, torch.float32)
    stops = _stage_stops(name)
    assert len(stops) <= 13 and 6 in stops and 22 in stops
    assert fused_next(name, 6, "fp32") and fused_next(name, 7, "fp32") and not fused_next(name, 22, "fp32")
    rows, checks = [], []
    _check_stops("", name, "fp32", f, stops, r64, r32, rows, checks, model=_engine(name, 2, 64))
    _assert_all("ResNet221 fp32 T=57", checks, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("name,two_emb", [("ResNet34", False), ("ResNet34", True)])
def test_head_after_a_full_forward(name, two_emb):
    """pooled (TSTP), emb_a (seg_1, split-K over K = 5120) and the embedding of a full forward; the maps of the last
    block are there too, the stem is not."""
    from wespeaker_amd._lib import NativeError
    f = _fixture_feats()
    model = _engine(name, two_emb=two_emb)
    r64, r32 = oracle_taps(name, f, torch.float64, two_emb), oracle_taps(name, f, torch.float32, two_emb)
    emb = _run(model, f, -1)
    rows, checks = [], []
    nb = n_blocks(name)
    for key, tap in (("pooled", "pooled"), ("b%d.block" % nb, "block"), ("b%d.mid" % nb, "mid")):
        checks.append((key, tap_check(key, _read(model, tap, r64[key]), r64[key], r32[key], K["fp32"][tap], rows)[0]))
    if two_emb:
        # the tap holds seg_1's output AFTER its epilogue (relu, seg_bn_1): what seg_2 reads
        sd = _sd(name, True)
        post = lambda e: np.maximum(e, 0) / np.sqrt(np.asarray(sd["seg_bn_1.running_var"], dtype=e.dtype) + e.dtype.type(1e-5)) \
            - np.asarray(sd["seg_bn_1.running_mean"], dtype=e.dtype) / np.sqrt(np.asarray(sd["seg_bn_1.running_var"], dtype=e.dtype) + e.dtype.type(1e-5))
        a64, a32 = post(r64["emb_a"]), post(r32["emb_a"])
        checks.append(("emb_a", tap_check("emb_a", _read(model, "emb_a", a64), a64, a32, K["fp32"]["emb_a"], rows)[0]))
    else:
        with pytest.raises(NativeError, match="one embedding layer"):
            model.tap_shape("emb_a")
    checks.append(("emb", tap_check("emb", emb, r64["emb"], r32["emb"], K["fp32"]["emb"], rows)[0]))
    with pytest.raises(NativeError, match="stop it at 0"):
        model.tap_shape("stem")
    _assert_all("%s head two_emb=%s" % (name, two_emb), checks, rows)


# ---- large-batch kernels (fp32): reached only above a row count; three spot utterances against the oracle
LARGE_T = 208


@functools.lru_cache(maxsize=None)
def _large_base():
    f = np.random.RandomState(LARGE_T).randn(3, LARGE_T, 80).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=2)
def _large_refs(name):
    return oracle_taps(name, _large_base(), torch.float64), oracle_taps(name, _large_base(), torch.float32)


def _large_case(name, B, stops, want, lens=None):
    """Utterance b of the batch is base[b % 3]; spots = first, middle, last, chosen so that they are base[0], [1], [2].
    `want`: [(substrings that one dispatch-log line must all contain)]."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    idx = np.arange(B) % 3
    spots = [0, (B // 2) // 3 * 3 + 1, max(b for b in range(B) if b % 3 == 2)]
    assert [int(idx[s]) for s in spots] == [0, 1, 2]
    feats = _large_base()[idx]
    model = _engine(name, max_batch=B, max_frames=LARGE_T)
    r64, r32 = _large_refs(name)
    rows, checks = [], []
    lines = []
    for n in stops:
        dispatch_log(True, clear=True)
        try:
            _run(model, feats, n)
            lines = dispatch_report()
        finally:
            dispatch_log(False, clear=True)
        for key in _keys_at(name, n, "fp32", r64):
            got = _read(model, _kind(key), r64[key], spots)
            checks.append((key, tap_check(key, got, r64[key], r32[key], K["fp32"][_kind(key)], rows)[0]))
    print("\n".join(lines))
    for subs in want:
        assert any(all(s in l for s in subs) for l in lines), (subs, lines)
    _assert_all("%s B=%d T=%d" % (name, B, LARGE_T), checks, rows)
    del _ENGINES[(name, B, LARGE_T, False)]


@pytest.mark.gpu
def test_large_batch_direct_conv3x3_stage1():
    """ResNet18, B = 8: M = 8 * 80 * 208 = 133 120 rows x 32 channels >= 2^22 elements -- conv3x3_direct_f32_kernel
    takes stage 1, without the residual (conv1 -> mid) and with it (conv2 -> block), blocks 1 - 2."""
    _large_case("ResNet18", 8, [1, 2], [("N=32 K=288", "+res", "conv3x3_direct_f32_kernel"),
                                        ("N=32 K=288", "out=f32 ->", "conv3x3_direct_f32_kernel")])


@pytest.mark.gpu
def test_large_batch_conv_form_256x64_stage2():
    """ResNet18, B = 32: stage 2 is 32 * 40 * 104 = 133 120 rows, N = 64 -- the persistent kernel's convolution form on
    256 x 64 tiles, with and without the residual (blocks 3 - 4)."""
    _large_case("ResNet18", 32, [3, 4], [("N=64 K=576", "+res", "gemm_f32_stream_kernel<256x64 tile", "conv>"),
                                         ("N=64 K=576", "out=f32 ->", "gemm_f32_stream_kernel<256x64 tile", "conv>")])


@pytest.mark.gpu
def test_large_batch_plain_1x1_with_residual_stage3():
    """ResNet50, B = 32: stage 3's conv3 (K = 128 -> N = 512, + residual) on the persistent kernel's plain form with
    64 x 64 units behind the last whole tile (blocks 8 - 9).  The same batch shows two more kernels: block 8's shortcut
    (1x1, stride 2, N = 512) is served by conv_gemm_dual_kernel -- judged through the sc tap --, and block 1's conv1
    (1x1, 32 -> 32) by conv_gemm_kernel<128,32>, whose output is not a tap of its own: block 1's mid is the 3x3
    convolution that reads it, held to the same bound."""
    _large_case("ResNet50", 32, [1, 8, 9], [("N=512 K=128 k=1x1", "+res", "gemm_f32_stream_kernel"),
                                            ("N=512 K=256 k=1x1 s=2x2", "conv_gemm_dual_kernel"),
                                            ("N=32 K=32 k=1x1", "conv_gemm_kernel<128,32")])


@pytest.mark.gpu
def test_large_batch_conv_form_256x128_stage3():
    """ResNet18, B = 128: stage 3 is 128 * 20 * 52 rows, N = 128 -- the convolution form on 256 x 128 tiles (blocks 5 - 6);
    block 5's stride-2 conv1 (its mid) goes to conv_gemm_dual_kernel."""
    _large_case("ResNet18", 128, [5, 6], [("N=128 K=576 k=3x3 s=2x2", "conv_gemm_dual_kernel"),
                                          ("N=128 K=1152", "+res", "gemm_f32_stream_kernel<256x128 tile", "conv>"),
                                          ("N=128 K=1152", "out=f32 ->", "gemm_f32_stream_kernel<256x128 tile", "conv>")])


@pytest.mark.gpu
def test_large_batch_conv_form_256x128_stage4():
    """ResNet18, B = 256: stage 4 is 256 * 10 * 26 rows, N = 256 -- the same form, two column tiles (blocks 7 - 8)."""
    _large_case("ResNet18", 256, [7, 8], [("N=256 K=2304", "+res", "gemm_f32_stream_kernel<256x128 tile", "conv>"),
                                          ("N=256 K=2304", "out=f32 ->", "gemm_f32_stream_kernel<256x128 tile", "conv>")])


# ---- ragged batches
RAGGED_LENS = [131, 113, 64, 57, 9, 2]


def _level_len(L, level):
    for _ in range(level):
        L = (L - 1) // 2 + 1
    return L


def _block_levels(name):
    """Stride level of the output of block i (index i; 0 = the stem)."""
    lay = so.LAYOUTS[name] if name in so.LAYOUTS else oresnet.LAYOUTS[name][1]
    lv = [0]
    for s, nb in enumerate(lay):
        lv += [s] * nb
    return lv


def _ragged_case(name, prec, lens, TS, seed):
    B = len(lens)
    rng = np.random.RandomState(seed)
    utts = [rng.randn(L, 80).astype(np.float32) for L in lens]
    pad = np.full((B, TS, 80), np.nan, dtype=np.float32)
    for b, u in enumerate(utts):
        pad[b, :len(u)] = u
    refs = [(oracle_taps(name, u[None], torch.float64), oracle_taps(name, u[None], torch.float32)) for u in utts]
    model = _engine(name).set_precision(prec)
    levels = _block_levels(name)
    rows, checks = [], []
    try:
        for n in range(n_blocks(name) + 1):
            _run(model, pad, n, lens)
            for key in _keys_at(name, n, prec, refs[0][0]):
                slot = model.tap(_kind(key)).cpu().numpy()
                Hn, C = refs[0][0][key].shape[1], refs[0][0][key].shape[3]
                slot = slot.reshape(B, Hn, _level_len(TS, levels[n]), C)
                for b, L in enumerate(lens):
                    Wv = _level_len(L, levels[n])
                    r64, r32 = refs[b]
                    assert r64[key].shape[2] == Wv
                    tag = "%s[%d]" % (key, b)
                    checks.append((tag, tap_check(tag, slot[b:b + 1, :, :Wv], r64[key], r32[key], K[prec][_kind(key)], rows)[0]))
                    if key != "stem":
                        tail = slot[b, :, Wv:]
                        assert not tail.any(), "%s: %d non-zero values in the padding columns of utterance %d (len %d)" % (
                            key, int(np.count_nonzero(tail)), b, L)
    finally:
        model.set_precision("fp32")
    _assert_all("ragged %s %s" % (name, prec), checks, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", ["ResNet18", "ResNet50"])
def test_every_block_ragged_batch_and_its_zero_padding_columns(name, prec):
    """Six utterances in 131-frame slots, NaN in the feature padding.  Columns of an utterance: every tap equals the
    batch-1 oracle of that utterance.  Columns beyond its length at that stride level: block, mid, sc and next_y1 are
    EXACTLY zero -- resnet_model.hip promises it (row_len) and the pooling and every later border tap rest on it."""
    _ragged_case(name, prec, RAGGED_LENS, 131, 131)


@pytest.mark.gpu
def test_ragged_large_batch_on_the_masked_persistent_forms():
    """ResNet18, B = 32, T = 208, lens in [150, 208]: stage 2 on the masked twins of the persistent kernel's convolution
    form (blocks 3 - 4).  The three spot utterances keep their full length; the others are cut."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    name, B = "ResNet18", 32
    idx = np.arange(B) % 3
    spots = [0, 16, 29]
    assert [int(idx[s]) for s in spots] == [0, 1, 2]
    lens = [int(x) for x in np.random.RandomState(B).randint(150, LARGE_T + 1, size=B)]
    for s in spots:
        lens[s] = LARGE_T
    feats = _large_base()[idx].copy()
    for b, L in enumerate(lens):
        feats[b, L:] = np.nan
    model = _engine(name, max_batch=B, max_frames=LARGE_T)
    r64, r32 = _large_refs(name)
    rows, checks, lines = [], [], []
    for n in (3, 4):
        dispatch_log(True, clear=True)
        try:
            _run(model, feats, n, lens)
            lines = dispatch_report()
        finally:
            dispatch_log(False, clear=True)
        for key in _keys_at(name, n, "fp32", r64):
            slot = model.tap(_kind(key)).reshape((B,) + r64[key].shape[1:])
            got = slot[torch.as_tensor(spots, device=slot.device)].cpu().numpy()
            checks.append((key, tap_check(key, got, r64[key], r32[key], K["fp32"][_kind(key)], rows)[0]))
            cut = min(b for b in range(B) if lens[b] < LARGE_T - 8)
            tail = slot[cut, :, _level_len(lens[cut], 1):].cpu().numpy()
            assert tail.size and not tail.any(), (key, cut, lens[cut])
    print("\n".join(lines))
    for subs in (("N=64 K=576", "+res", "+mask", "gemm_f32_stream_kernel<256x64 tile", "conv>"),
                 ("N=64 K=576", "out=f32 +mask", "gemm_f32_stream_kernel<256x64 tile", "conv>")):
        assert any(all(s in l for s in subs) for l in lines), (subs, lines)
    _assert_all("ragged ResNet18 B=32", checks, rows)
    del _ENGINES[(name, B, LARGE_T, False)]


# ---- SimAM-ResNet
@pytest.mark.gpu
@pytest.mark.parametrize("T", [57, 9])
def test_simam_every_block_and_the_asp_head(T):
    """SimAM_ResNet34_ASP, B = 3, fp32: block (the gated result), mid, sc at every stop; hid / logits / pooled and the
    embedding on a full forward."""
    f = _fixture_feats()[:, :T]
    r64, r32 = oracle_taps(S34, f, torch.float64), oracle_taps(S34, f, torch.float32)
    model = _engine(S34)
    rows, checks = [], []
    _check_stops("", S34, "fp32", f, range(n_blocks(S34) + 1), r64, r32, rows, checks, model=model)
    emb = _run(model, f, -1)
    for t in ("hid", "logits", "pooled"):
        checks.append((t, tap_check(t, _read(model, t, r64[t]), r64[t], r32[t], K["fp32"][t], rows)[0]))
    checks.append(("emb", tap_check("emb", emb, r64["emb"], r32["emb"], K["fp32"]["emb"], rows)[0]))
    _assert_all("SimAM T=%d" % T, checks, rows)


@pytest.mark.gpu
def test_simam_ragged_batch_and_its_zero_padding_columns():
    """lens [57, 40, 9] in 57-frame slots, NaN padding: the plane statistics of the SimAM gate must not see the padding,
    and the gated result, mid and sc are exactly zero beyond each utterance."""
    _ragged_case(S34, "fp32", [57, 40, 9], 57, 57)


# ---- API edges
@pytest.mark.gpu
def test_stop_and_tap_api_edges():
    from wespeaker_amd._lib import NativeError
    from wespeaker_amd.engine import NativeSpeakerModel
    name = "ResNet50"
    model = NativeSpeakerModel(name, _sd(name), feat_dim=80, embed_dim=256, max_batch=2, max_frames=64)
    with pytest.raises(NativeError, match="no forward"):                       # before any forward
        model.tap("block")
    f = np.random.RandomState(5).randn(5, 57, 80).astype(np.float32)
    x = torch.from_numpy(f)
    first = model(x)[-1].clone()
    assert first.abs().max() > 0
    with pytest.raises(NativeError, match="unknown tensor 'h'"):
        model.tap("h")
    # stop beyond the block count / below -1; the stop point stays where it was
    with pytest.raises(NativeError, match="has 16 residual blocks"):
        model.stop_after(17)
    with pytest.raises(NativeError, match="n_blocks = -2"):
        model.stop_after(-2)
    assert torch.equal(model(x)[-1], first)
    # 5 utterances on max_batch = 2: the tap holds the LAST chunk (utterance 4); a stopped forward returns all zeros
    with model.stopped_after(2):
        z = model(x)[-1]
        assert tuple(z.shape) == (5, 256) and not z.any()
        assert model.tap_shape("block") == (1 * 80 * 57, 128) and model.tap_shape("next_y1") == (80 * 57, 32)
        last = model.tap("block")
        with pytest.raises(NativeError, match="block 2 has no shortcut"):      # sc on a block without a shortcut
            model.tap("sc")
        with pytest.raises(NativeError, match="pooling and the head did not run"):
            model.tap("pooled")
        z1 = model(torch.from_numpy(f[4:5].copy()))[-1]
        assert not z1.any() and torch.equal(model.tap("block"), last)
    with model.stopped_after(7):                 # the last block of stage 2: 64 -> 128 planes is not fused
        model(x)
        with pytest.raises(NativeError, match="did not run the fused"):
            model.tap("next_y1")
        assert model.tap_shape("mid") == (40 * 29, 64)
    # the context manager restored the full forward: same bits as before the stopped ones
    assert torch.equal(model(x)[-1], first)
    assert model.tap_shape("pooled") == (1, 2 * 10 * 256 * 4)
    # f16 back-end: every map is binary16 only; the head's fp32 tensors still tap
    model.set_precision("f16")
    try:
        with model.stopped_after(0):
            model(x)
            with pytest.raises(NativeError, match="binary16"):
                model.tap("stem")
        with model.stopped_after(3):
            model(x)
            for t in ("block", "mid"):
                with pytest.raises(NativeError, match="binary16"):
                    model.tap(t)
        model(x)
        assert model.tap_shape("pooled") == (1, 20480)
    finally:
        model.set_precision("fp32")
    model.reserve(2, 100)                         # re-sizing the workspace forgets the last chunk
    with pytest.raises(NativeError, match="no forward"):
        model.tap("block")
    # ECAPA-TDNN stops after its SE-Res2 blocks 1 .. 3 only (tests/test_gpu_f16_layers.py reads them)
    from test_gpu_layers import _engine as ecapa_engine
    for n in (0, 4):
        with pytest.raises(NativeError, match="1, 2 or 3"):
            ecapa_engine("ECAPA_TDNN_c512").stop_after(n)
    ecapa_engine("ECAPA_TDNN_c512").stop_after(2).stop_after(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ResNet34", S34, "ERes2Net34_Base"])
def test_a_refused_reserve_leaves_the_engine_usable(name):
    """ws_engine_reserve beyond 2^31 elements per activation map is refused before anything is re-laid-out: the
    workspace, the activation buffers and their zero pads stay what they were, the next forward gives the same bits
    and ws_engine_check_range still reads the pads."""
    from wespeaker_amd._lib import NativeError
    from wespeaker_amd.engine import NativeSpeakerModel
    from test_gpu_eres2net_layers import _check_invariants    # (ws_engine_check_range in fp32 too: the zero pads)
    model = NativeSpeakerModel(name, synth.synth_state_dict(name, 80, None, seed=42), feat_dim=80, max_batch=2,
                               max_frames=64)
    x = torch.from_numpy(np.ascontiguousarray(_fixture_feats()[:2, :57])).cuda()
    before = model.embed(x).cpu().numpy()
    with pytest.raises(NativeError, match="limit 2\\^31"):
        model.reserve(1 << 20, 200)
    assert (model.max_batch, model.max_frames) == (2, 64)
    after = model.embed(x).cpu().numpy()
    _check_invariants(model)
    assert np.isfinite(before).all() and np.array_equal(before, after)
    model.reserve(2, 64)                          # and an accepted one after it works as ever
    assert np.array_equal(before, model.embed(x).cpu().numpy())
    _check_invariants(model)
