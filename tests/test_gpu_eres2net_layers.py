"""Per-block ERes2Net34 parity beyond tests/test_gpu_eres2net.py::test_every_tap (Base, B = 2, T = 57, the 64x64 tile
only): the 128-row tile forms of launch_prec (conv_gemm.hip) at the batch sizes that reach them, the clamp's ceiling on
those tiles, every tap of Large and aug, and ragged batches with every padding column.

    reference   tests/eres2net_oracle.py, dtype=torch.float64, return_intermediates=True
    metric      tests/test_gpu_layers.py: scaled max error and relative L2 (tap_errors)
    bound       k = 8 x the same metric of the float32 CPU oracle, floored at 2^-24 (tap_check); fp32 and f16x3 alike
    ragged      a row's embedding within 1e-5 of its own batch of one; padding columns EXACTLY zero

Taps: stem (stopped at 0); mid / cat / sc / block of the last executed block (stopped_after(n)); fuse12 / fuse123 /
fuse1234 / pooled after a full forward.  Large batches follow tests/test_gpu_resnet_layers.py::_large_case: utterance b
is base[b % 3] and only the spot utterances are read back, sliced on the device.  Every large case asserts on the
dispatch log that the forms it is there for ran (slots = 2 x 256 CUs on MI355X), and that the rows a peeled launch
gives to the 64x64 half of conv_gemm_dual_kernel lie in the last utterance, which is always a spot; every test prints
its dispatch lines (the B = 2 and ragged cases: those of the full forward; ragged: `+mask` on every map launch) and its table of ratios (run with -s).

Cases and the forms they reach (T = 208 unless said; see DESIGN.md 4.2.17 for the log lines and the measured ratios):
    Base B = 2, blocks 1 - 3      <128,32> conv and A2 (N = 16, K = 144), <128,32> 1x1 (conv1), <128,64> 1x1 (+res, shortcut)
    Base B = 16, blocks 4 - 7     <128,32> conv and A2 (N = 32, K = 288), <128,64> conv1 (also s = 2x2), dual kernel (conv3
                                  + res, the stride-2 shortcut); fp32 and f16x3
    Base B = 32, blocks 8 - 13    <128,64> conv (N = 64, K = 576), 128x128 class for conv1 / conv3, aff_fuse C = 64
    Base B = 126, blocks 14 - 16  <128,128> conv (N = 128, K = 1152); full forward: the three downsample convolutions,
                                  the global AFFs, pooled, the zero pads of all fourteen buffers; fp32 and f16x3
    clamp fixture                 20.0 out of <128,64> 1x1 + res (B = 2), the dual kernel (B = 16), <128,64> conv (B = 32)
    Large / aug, B = 2            every tap, fp32 and f16x3 (aug also T = 9 and 64)
    aug B = 8, T = 57             N = 24, K = 216 on <128,32>, plain and A2; Large B = 30, T = 57: N = 64, K = 576 + A2
    ragged                        Base (fp32, f16x3) and aug, every tap and every padding column; Base B = 16 masked

Measured on MI355X -- worst ratio = device error / float32-oracle error (worst of the two metrics) per tap kind over
the cases of each group, with the case that gave it:

    group                                mid    cat    sc     block  fuse12 fuse123 fuse1234 pooled  emb
    large batches, fp32 (128-row tiles)  1.53   2.39   1.59   1.50   1.19   1.75    2.08     2.15    0.63
    large batches, f16x3                 1.97   2.37   1.80   2.18   1.62   2.37    2.47     5.38    1.23
    Large / aug B = 2, fp32              2.44   2.52   2.40   2.34   2.72   3.15    2.92     3.36    1.42
    Large / aug B = 2, f16x3             3.17   3.34   3.46   4.76   3.30   3.39    3.83     5.86    1.44
    ragged, fp32 (Base, aug, B = 16)     2.83   3.16   2.57   2.45   2.77   3.29    3.03     3.03    1.58
    ragged Base, f16x3                   2.34   2.57   1.98   2.48   1.84   2.44    2.63     4.55    1.42
The stem stays at 0.81 .. 1.02.  The largest ratio anywhere is 5.86 (pooled, Large f16x3 T = 57: oracle32 7.5e-7, device
4.4e-6; f16x3's pooled is the worst tap of every group, as in tests/test_gpu_eres2net.py).  The 128-row tile forms
themselves stay below 2.4 in fp32.  Every padding column is exactly zero, every ragged row equals its batch of one bit
for bit, the clamp reads 20.0 out of all three kernels, and no kernel had to be changed.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(os.path.dirname(TESTS), "tools"), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import eres2net_oracle as eo  # noqa: E402
from fixtures import synth  # noqa: E402
from oracle import fbank as ofbank  # noqa: E402
from test_gpu_layers import REL_TOL, _assert_all, tap_check  # noqa: E402
from test_gpu_resnet_layers import _level_len, _read, _run  # noqa: E402

BASE, LARGE, AUG = "ERes2Net34_Base", "ERes2Net34_Large", "ERes2Net34_aug"
K_TAP = 8.0
RAGGED_VS_SINGLE_TOL = 1e-5
LARGE_T = 208
CLAMP_OFFSET = 25.0
CLAMP_OFFSET_B4 = 28.0        # layer2.0.bn3.bias: the smallest whole offset that saturates b4.block (25: 0.26, 27: 0.45, 28: 0.64)
CLAMP_CHANNELS = (3, 17, 40, 63)
BLOCK_TAPS = ("mid", "cat", "sc", "block")
FUSIONS = ("fuse12", "fuse123", "fuse1234")
STAGE_OF = [0] + [s for s, nb in enumerate(eo.BLOCKS) for _ in range(nb)]      # stride level of block i's output


# ---------------------------------------------------------------------------------------------- the oracle side (CPU)
@functools.lru_cache(maxsize=None)
def _sd(name=BASE):
    return synth.synth_eres2net_state_dict(name, 80, 192, seed=42)


@functools.lru_cache(maxsize=None)
def clamp_fixture_sd():
    """tests/test_gpu_eres2net.py's fixture (+25 on four channels of layer1.0.bn3.bias and layer3.0.bns.0.bias), and +28
    on the same channels of layer2.0.bn3.bias: conv3 of block 4, N = 128 + residual -- the dual kernel at B = 16.  (+25
    there leaves 26 % of those values on the ceiling in the float64 oracle, T = 208: block 4's pre-activations lie lower
    than block 1's.  28 is the smallest whole offset that puts more than half there.)
    layer3.0.bns.0 is the batch norm of block 8's SECOND branch (the first is conv2_1 / bn2_1 in the AFF blocks): the
    offset channels of b8.cat are 64 + CLAMP_CHANNELS, in slice 1 -- the convolution that reads the AFF scratch."""
    sd = {k: np.array(v, copy=True) for k, v in _sd().items()}
    for key, off in (("layer1.0.bn3.bias", CLAMP_OFFSET), ("layer2.0.bn3.bias", CLAMP_OFFSET_B4),
                     ("layer3.0.bns.0.bias", CLAMP_OFFSET)):
        sd[key][list(CLAMP_CHANNELS)] += off
    return sd


def _cl(t):
    """(B, C, F, T) -> the engine's [b][f][t][c]."""
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def oracle_taps(sd, name, feats, dtype, keep=None, **kw):
    """key -> numpy array in the engine's layout: 'stem', 'b<i>.mid' / '.cat' / '.sc' / '.block' and the fusions as
    (B, F, T, C); 'pooled' (B, 2D), 'emb' (B, E).  keep: a predicate on keys (the big maps are many)."""
    emb, mid = eo.eres2net_forward(sd, np.array(feats), name, dtype=dtype, return_intermediates=True, **kw)
    out = {"pooled": mid["pooled"].numpy(), "emb": emb.numpy()}
    for k, v in mid.items():
        if k not in ("aff", "pooled", "emb_a") and (keep is None or keep(k)):
            out[k] = _cl(v)
    return out


@functools.lru_cache(maxsize=None)
def _fixture_feats():
    f = np.stack([ofbank.speaker_features(synth.synth_wav(i)) for i in range(2)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _fixture_refs(name, T):
    """(float64 taps, float32 taps) of the two fixture utterances cut to T frames; one per (layout, T)."""
    f = _fixture_feats()[:, :T]
    return oracle_taps(_sd(name), name, f, torch.float64), oracle_taps(_sd(name), name, f, torch.float32)


@functools.lru_cache(maxsize=None)
def _large_base(T=LARGE_T):
    f = np.random.RandomState(T).randn(3, T, 80).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _large_refs(name, T=LARGE_T):
    """(float64 taps, float32 taps) of the three base utterances; shared by every large case of the layout."""
    f = _large_base(T)
    return oracle_taps(_sd(name), name, f, torch.float64), oracle_taps(_sd(name), name, f, torch.float32)


_CLAMP_KEYS = ("b1.block", "b4.block", "b8.cat")


def _clamp_channels(key):
    return [c + (64 if key == "b8.cat" else 0) for c in CLAMP_CHANNELS]


@functools.lru_cache(maxsize=None)
def _clamp_ref(dtype):
    return oracle_taps(clamp_fixture_sd(), BASE, _large_base(LARGE_T), dtype, keep=lambda k: k in _CLAMP_KEYS)


def _keys_at(n, r64):
    """The oracle keys of the taps that exist when the engine is stopped after block n (-1: the full forward)."""
    if n == 0:
        return ["stem"]
    if n < 0:
        return list(FUSIONS) + ["pooled"]
    return [k for k in ("b%d.%s" % (n, t) for t in BLOCK_TAPS) if k in r64]


def _kind(key):
    return key.split(".")[-1]


def test_clamp_fixture_saturates_the_three_layers():
    """The pre-condition of the device test below, on the float64 oracle of its own inputs (T = 208): more than half of
    the offset channels' values of b1.block, b4.block and of b8.cat (slice 1) sit on the ceiling, EXACTLY 20.0.
    Measured: 1.000 / 0.636 / 0.963."""
    r64 = _clamp_ref(torch.float64)
    for key in _CLAMP_KEYS:
        share = float((r64[key][..., _clamp_channels(key)] == 20.0).mean())
        print("%s: %.3f of the offset channels' values equal 20.0" % (key, share))
        assert share > 0.5, (key, share)
        assert r64[key].max() == 20.0
    # on the plain weights the ceiling is never reached: nothing but this fixture produces a 20.0
    assert max(float(v.max()) for k, v in _fixture_refs(BASE, 57)[0].items() if k.startswith("b")) < 20.0


def test_the_per_block_bound_has_teeth():
    """Why this file exists (CPU).  Base, the two 57-frame fixture utterances, fed to the very comparison the GPU tests
    use.  Two errors that the embedding bar (REL_TOL = 2e-4) lets through and k = 8 refuses:
      * slice 1 (channels 32 .. 63) of b5.cat over 32 consecutive pixels of utterance 0, scaled by 1 + 1e-4 -- a branch
        convolution that read the wrong a2_off, a dropped K-tile;
      * the t = 0 border column of the channel of median range of b9.block, shifted by 1e-4 of that channel's range --
        a wrong border tap.
    The embeddings come from the oracle's own tail (eres2net_forward(override=...)); unperturbed, the override
    reproduces the embedding to 1e-12.  Both oracles pass every tap."""
    sd, f = _sd(), _fixture_feats()[:, :57]
    r64, r32 = _fixture_refs(BASE, 57)
    rows = []
    for t in r64:
        assert tap_check(t, r64[t], r64[t], r32[t], K_TAP)[0]
        assert tap_check(t, r32[t], r64[t], r32[t], K_TAP, rows)[0], rows[-1]
    emb64 = r64["emb"]
    rel = lambda e: float((np.linalg.norm(e - emb64, axis=1) / np.linalg.norm(emb64, axis=1)).max())  # noqa: E731
    cf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2)                       # noqa: E731
    tail = lambda key, a: eo.eres2net_forward(sd, np.array(f), BASE, override={key: cf(a)}).numpy()     # noqa: E731
    eps = 1e-4

    cat = r64["b5.cat"]                                            # (B, 40, 29, 64)
    B, H, W, C = cat.shape
    assert (H, W, C) == (40, 29, 64)
    bad = cat.reshape(B, H * W, C).copy()
    bad[0, 320:352, 32:64] *= 1.0 + eps
    bad = bad.reshape(cat.shape)
    ok, ratio = tap_check("b5.cat", bad, cat, r32["b5.cat"], K_TAP, rows)
    assert not ok and ratio > K_TAP, rows
    e = rel(tail("b5.cat", bad))
    print("b5.cat slice 1, 32 pixels x (1 + %g): embedding moves by %.2e, tap ratio %.1f" % (eps, e, ratio))
    assert 0.0 < e < REL_TOL, e

    blk = r64["b9.block"]                                          # (B, 20, 15, 256)
    assert blk.shape[1:] == (20, 15, 256)
    rng = blk.max(axis=(0, 1, 2)) - blk.min(axis=(0, 1, 2))
    c = int(np.argsort(rng)[blk.shape[3] // 2])
    bad = blk.copy()
    bad[:, :, 0, c] += eps * rng[c]
    ok, ratio = tap_check("b9.block", bad, blk, r32["b9.block"], K_TAP, rows)
    assert not ok and ratio > K_TAP, rows
    e = rel(tail("b9.block", bad))
    print("b9.block channel %d, t = 0 column + %g of its range: embedding moves by %.2e, tap ratio %.1f" % (c, eps, e, ratio))
    assert 0.0 < e < REL_TOL, e

    assert rel(tail("b5.cat", cat)) < 1e-12 and rel(tail("b9.block", blk)) < 1e-12
    print("\n".join(rows))


# ------------------------------------------------------------------------------------------------------- GPU side
_ENGINES = {}


def _engine(name, max_batch, max_frames, sd=None, tag=""):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = (name, max_batch, max_frames, tag)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, sd if sd is not None else _sd(name), feat_dim=80, embed_dim=192,
                                           max_batch=max_batch, max_frames=max_frames)
    return _ENGINES[key]


def _check_invariants(model):
    """ws_engine_check_range in either back-end: the non-finite count and the zero pads behind all fourteen activation
    buffers (NativeSpeakerModel.check_range skips the call in fp32).  A private coupling: this reaches past the public
    surface to the engine handle (`model._h`) and the ctypes wrapper (`wespeaker_amd._lib`); if either changes, this
    helper is the place to repair -- or to drop, once check_range() reads the pads back in fp32 too."""
    from wespeaker_amd import _lib
    with torch.cuda.device(model.device):
        _lib.check(_lib.lib().ws_engine_check_range(model._h, _lib.current_stream_ptr(model.device)), "ws_engine_check_range")


def _logged_run(model, feats, n, lens, lines):
    """_run with the dispatch log on; the distinct lines are added to `lines`."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    dispatch_log(True, clear=True)
    try:
        emb = _run(model, feats, n, lens)
        for ln in dispatch_report():
            if ln not in lines:
                lines.append(ln)
    finally:
        dispatch_log(False, clear=True)
    return emb


def _assert_forms(lines, want):
    """want: [(substrings one dispatch-log line must all contain; a leading '!' = must not contain)]."""
    print("\n".join(lines))
    for subs in want:
        hit = [ln for ln in lines if all((s[1:] not in ln) if s[0] == "!" else (s in ln) for s in subs)]
        assert hit, "no dispatch line with %s:\n%s" % (subs, "\n".join(lines))


def _check_taps(model, n, r64, r32, rows, checks, spots=None, ref_rows=None, tag=""):
    """Every tap that exists after a forward stopped at n, against the oracle rows `ref_rows` (default: all)."""
    sel = (lambda a: a) if ref_rows is None else (lambda a: a[ref_rows])
    for key in _keys_at(n, r64):
        a, b = sel(r64[key]), sel(r32[key])
        got = _read(model, _kind(key), a, spots)
        checks.append((tag + key, tap_check(tag + key, got, a, b, K_TAP, rows)[0]))


def _small_case(name, T, prec):
    """B = 2 fixture utterances cut to T frames: stem, every block's taps, the fusions, pooled and the embedding."""
    model = _engine(name, 2, 64).set_precision(prec)
    assert model.ignored_keys == []
    f = _fixture_feats()[:, :T]
    r64, r32 = _fixture_refs(name, T)
    rows, checks, lines = [], [], []
    try:
        for n in range(17):
            _run(model, f, n)
            _check_taps(model, n, r64, r32, rows, checks)
        emb = _logged_run(model, f, -1, None, lines)
        print("\n".join(lines))
        _check_taps(model, -1, r64, r32, rows, checks)
        checks.append(("emb", tap_check("emb", emb, r64["emb"], r32["emb"], K_TAP, rows)[0]))
        _check_invariants(model)
    finally:
        model.set_precision("fp32")
    _assert_all("%s %s B=2 T=%d" % (name, prec, T), checks, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name,T", [(LARGE, 57), (AUG, 33)])
def test_large_and_aug_every_tap(name, T, prec):
    """Large (m = 64, widths 32 / 64 / 128 / 256) and aug (baseWidth 24, scale 3, expansion 4: widths 24 / 48 / 96 / 192,
    three branches, K = 216 stage-1 branch convolutions whose K-tiles straddle filter taps, a2_off = w on the third)."""
    _small_case(name, T, prec)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [9, 64])
def test_aug_every_tap_at_the_minimum_length_and_at_64(T):
    """T = 9 -> 5 -> 3 -> 2 (the minimum: TSTP's unbiased variance needs two frames) and T = 64, fp32."""
    _small_case(AUG, T, "fp32")


def _spots(B, last=1):
    """Utterance b of a large batch is base[b % 3]: first, middle, last, chosen so that they are base[0], [1], [2] (B = 2:
    both utterances) -- and ALWAYS the `last` final utterances: conv_gemm_dual_kernel gives rows [tail_begin, M) to its
    64x64 tiles, and a peeled tail must lie inside them (_assert_tails_are_read; one utterance but for Large B = 30)."""
    if B < 3:
        return list(range(B))
    spots = [0, (B // 2) // 3 * 3 + 1, max(b for b in range(B) if b % 3 == 2)]
    assert [s % 3 for s in spots] == [0, 1, 2]
    return spots + [b for b in range(B - last, B) if b not in spots]


def _assert_tails_are_read(lines, B, rows, last=1):
    """Every conv_gemm_dual_kernel launch over `rows` rows (the maps the last stop read back): its 64x64 half, rows
    [tail_begin, rows), lies inside the `last` final utterances, which are spots.  -> the number of such lines"""
    import re
    n = 0
    for ln in lines:
        m = re.match(r"rows=(\d+) N=(\d+) .*conv_gemm_dual_kernel.* big=(\d+) small=(\d+)", ln)
        if m and int(m.group(1)) == rows:
            N, big, small = int(m.group(2)), int(m.group(3)), int(m.group(4))
            tail_begin = big // ((N + 127) // 128) * 128
            assert small > 0 and rows // B * (B - last) <= tail_begin < rows, (ln, tail_begin, rows // B * (B - last))
            n += 1
    return n


def _large_case(name, B, stops, want, prec="fp32", T=LARGE_T, full=False, sd=None, refs=None, tag="", after=None, last=1):
    """Stopped forwards of a B-utterance batch (+ the full one), the spots against the oracle, `want` against the
    dispatch log.  The engine is deleted when the case ends.  -> (rows, lines)"""
    spots = _spots(B, last)
    feats = _large_base(T)[np.arange(B) % 3]
    r64, r32 = refs or _large_refs(name, T)
    ref_rows = [s % 3 for s in spots]
    model = _engine(name, B, T, sd=sd, tag=tag).set_precision(prec)
    rows, checks, lines = [], [], []
    try:
        for n in stops:
            _logged_run(model, feats, n, None, lines)
            _check_taps(model, n, r64, r32, rows, checks, spots, ref_rows)
            if after:
                after(model, n, spots)
        if full:
            emb = _logged_run(model, feats, -1, None, lines)
            _check_taps(model, -1, r64, r32, rows, checks, spots, ref_rows)
            checks.append(("emb", tap_check("emb", emb[spots], r64["emb"][ref_rows], r32["emb"][ref_rows], K_TAP, rows)[0]))
            _check_invariants(model)
        else:
            duals = _assert_tails_are_read(lines, B, model.tap_shape("block")[0], last)
            assert duals or not any("conv_gemm_dual_kernel" in s for subs in want for s in subs), lines
    finally:
        model.set_precision("fp32")
        del _ENGINES[(name, B, T, tag)], model
    _assert_forms(lines, want)
    _assert_all("%s %s B=%d T=%d" % (name, prec, B, T), checks, rows)
    return rows, lines


def _p(prec):
    return "prec=%d" % {"fp32": 0, "f16x3": 1}[prec]


@pytest.mark.gpu
def test_large_batch_stage1_128x32_and_128x64_tiles():
    """Base, B = 2: stage 1 is 2 * 80 * 208 = 33 280 rows = 260 row tiles, 520 >= 512 slots -- the 16-wide branches on
    conv_gemm_kernel<128,32> without A2 (branch 0) and with it (branch 1: a_off = d_off = 16, a2_off = 0), conv1
    (N = 32, 1x1) on the same tile, conv3 + residual and block 1's shortcut on <128,64> (blocks 1 - 3)."""
    _large_case(BASE, 2, [1, 2, 3], [
        ("rows=33280 N=16 K=144 k=3x3", "!+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=33280 N=16 K=144 k=3x3", "+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=33280 N=32 K=32 k=1x1", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=33280 N=32 K=64 k=1x1", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=33280 N=64 K=32 k=1x1", "+res", "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=33280 N=64 K=32 k=1x1", "!+res", "!+relu20", "conv_gemm_kernel<128,64")])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_large_batch_stage2_and_the_dual_kernel(prec):
    """Base, B = 16: stage 2 is 16 * 40 * 104 = 66 560 rows = 520 row tiles -- the 32-wide branches (K = 288) on <128,32>
    with and without A2, conv1 on <128,64> (block 4's with stride 2), conv3 (N = 128, + residual) and block 4's stride-2
    shortcut in the 128x128 class, where 520 tiles over 512 slots peel a tail: conv_gemm_dual_kernel (blocks 4 - 7)."""
    pr = _p(prec)
    _, lines = _large_case(BASE, 16, [4, 5, 6, 7], [
        ("rows=66560 N=32 K=288 k=3x3", pr, "!+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=66560 N=32 K=288 k=3x3", pr, "+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=66560 N=64 K=64 k=1x1 s=2x2", pr, "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=66560 N=64 K=128 k=1x1 s=1x1", pr, "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=66560 N=128 K=64 k=1x1 s=1x1", pr, "+res", "+relu20", "128,128"),
        ("rows=66560 N=128 K=64 k=1x1 s=2x2", pr, "!+relu20", "128,128"),
        (pr, "+relu20", "conv_gemm_dual_kernel")], prec=prec)


@pytest.mark.gpu
def test_large_batch_stage3_aff_blocks():
    """Base, B = 32: stage 3 is 32 * 20 * 52 = 33 280 rows -- the 64-wide branches (K = 576, no A2: the second reads the
    AFF scratch) on <128,64>, conv1 (N = 128) and conv3 (N = 256) in the 128x128 class, aff_fuse_kernel with C = 64 on
    33 280 pixels inside a block: cat's slice 1 is the convolution of its output (blocks 8 - 13)."""
    _large_case(BASE, 32, [8, 9, 10, 11, 12, 13], [
        ("rows=33280 N=64 K=576 k=3x3", "!+A2", "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=33280 N=128 K=128 k=1x1 s=2x2", "+relu20", "128,128"),
        ("rows=33280 N=128 K=256 k=1x1 s=1x1", "+relu20", "128,128"),
        ("rows=33280 N=256 K=128 k=1x1", "+res", "+relu20", "128,128"),
        ("rows=33280 N=256 K=128 k=1x1 s=2x2", "!+res", "128,128"),
        ("rows=33280 C=64", "aff_fuse_kernel")])


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_large_batch_stage4_and_the_full_forward(prec):
    """Base, B = 126: stage 4 is 126 * 10 * 26 = 32 760 rows = 256 row tiles, 512 = the slots -- the 128-wide branches
    (K = 1152) on conv_gemm_kernel<128,128> (blocks 14 - 16).  The full forward: the three stride-2 downsample
    convolutions (N = 128 / 256 / 512, no clamp) on 128-row tiles, the global AFFs at C = 128 / 256 / 512 on 524 160 /
    131 040 / 32 760 pixels, pooled; then the zero pads behind all fourteen buffers are read back."""
    pr = _p(prec)
    _large_case(BASE, 126, [14, 15, 16], [
        ("rows=32760 N=128 K=1152 k=3x3", pr, "!+A2", "+relu20", "conv_gemm_kernel<128,128"),
        ("rows=32760 N=256 K=256 k=1x1 s=2x2", pr, "+relu20", "128,128"),
        ("rows=32760 N=512 K=256 k=1x1 s=1x1", pr, "+res", "+relu20", "128,128"),
        ("rows=524160 N=128 K=576 k=3x3 s=2x2", pr, "!+relu20", "<128,"),
        ("rows=131040 N=256 K=1152 k=3x3 s=2x2", pr, "!+relu20", "<128,"),
        ("rows=32760 N=512 K=2304 k=3x3 s=2x2", pr, "!+relu20", "<128,"),
        ("rows=524160 C=128", "aff_fuse_kernel"), ("rows=131040 C=256", "aff_fuse_kernel"),
        ("rows=32760 C=512", "aff_fuse_kernel")], prec=prec, full=True)


@pytest.mark.gpu
@pytest.mark.parametrize("B,stop,key,form", [
    (2, 1, "b1.block", ("rows=33280 N=64 K=32 k=1x1", "+res", "+relu20", "conv_gemm_kernel<128,64")),
    (16, 4, "b4.block", ("rows=66560 N=128 K=64 k=1x1 s=1x1", "+res", "+relu20", "128,128")),
    (32, 8, "b8.cat", ("rows=33280 N=64 K=576 k=3x3", "+relu20", "conv_gemm_kernel<128,64"))])
def test_clamp_ceiling_on_the_128_row_tiles(B, stop, key, form):
    """The clamp fixture at the large batches: the layer that passes Hardtanh's ceiling runs on a 128-row kernel with
    the clamp in its epilogue, and the tap's maximum is EXACTLY 20.0 (conv3 + residual of block 1 on <128,64>, of block
    4 in the 128x128 class / the dual kernel, branch 1 of block 8 -- the one behind aff_fuse -- on <128,64>)."""
    r64, r32 = _clamp_ref(torch.float64), _clamp_ref(torch.float32)
    seen = {}

    def after(model, n, spots):
        v = model.tap(_kind(key))
        seen["max"] = float(v.max())
        seen["share"] = float((v[:, _clamp_channels(key)] == 20.0).float().mean())
        last = v.reshape(B, -1, v.shape[1])[B - 1]              # the utterance that holds a peeled tail
        tail = last[-512:]                                      # (the dual kernel's tail at B = 16: the last 1024 rows)
        seen["last"] = (float(last.max()), float((last[:, _clamp_channels(key)] == 20.0).float().mean()),
                        float(tail.max()), float((tail[:, _clamp_channels(key)] == 20.0).float().mean()))

    # (the oracle keeps three maps of this fixture: the other taps of the stop are judged on the plain weights above)
    only = ({key: r64[key]}, {key: r32[key]})
    _large_case(BASE, B, [stop], [form], sd=clamp_fixture_sd(), refs=only, tag="clamp", after=after)
    print("%s: max %.9g, %.3f of the offset channels' values on the ceiling" % (key, seen["max"], seen["share"]))
    print("utterance %d: max %.9g, share %.3f; its last 512 rows: max %.9g, share %.3f" % ((B - 1,) + seen["last"]))
    assert seen["max"] == 20.0 and seen["share"] > 0.5, seen
    o = r64[key][(B - 1) % 3].reshape(-1, r64[key].shape[-1])[-512:, _clamp_channels(key)]
    o_share = float((o == 20.0).mean())
    assert o_share > 0.25, o_share                              # (the oracle's own share in those rows)
    assert seen["last"][0] == 20.0 and seen["last"][2] == 20.0 and abs(seen["last"][3] - o_share) < 0.01, (seen, o_share)


@pytest.mark.gpu
def test_aug_odd_widths_on_the_128_row_tiles():
    """aug, B = 8, T = 57: stage 1 is 8 * 80 * 57 = 36 480 rows = 285 row tiles -- N = 24 (a partial column tile),
    K = 216 (K-tiles straddle filter taps) on conv_gemm_kernel<128,32>, plain (a_off = 0) and with A2 (a_off = 24 / 48,
    a2_off = 0 / 24): the three 24-wide slices of cat.  conv1 has N = 72, conv3 N = 256 (blocks 1 - 3)."""
    _large_case(AUG, 8, [1, 2, 3], [
        ("rows=36480 N=24 K=216 k=3x3", "!+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=36480 N=24 K=216 k=3x3", "+A2", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=36480 N=72 K=64 k=1x1", "+relu20", "128,128"),
        ("rows=36480 N=72 K=256 k=1x1", "+relu20", "128,128"),
        ("rows=36480 N=256 K=72 k=1x1", "+res", "+relu20", "128,128")], T=57)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_large_layout_64_wide_branches_with_the_second_addend(prec):
    """Large, B = 30, T = 57: stage 2 is 30 * 40 * 29 = 34 800 rows = 272 row tiles -- N = 64, K = 576 with A2 on
    conv_gemm_kernel<128,64>, a form no Base layer reaches (its 64-wide branches are AFF blocks) (blocks 4 - 5).  conv3
    (N = 256, + residual) and block 4's shortcut peel a tail: the dual kernel, its 64x64 half (rows 32 768 .. 34 800) in
    utterances 28 and 29, both spots."""
    pr = _p(prec)
    _large_case(LARGE, 30, [4, 5], [
        ("rows=34800 N=64 K=576 k=3x3", pr, "+A2", "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=34800 N=64 K=576 k=3x3", pr, "!+A2", "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=34800 N=256 K=128 k=1x1 s=1x1", pr, "+res", "+relu20", "conv_gemm_dual_kernel")], T=57, prec=prec, last=2)


# ---- ragged batches
@functools.lru_cache(maxsize=None)
def _ragged_refs(name, lens, seed):
    """Per utterance: (features, float64 taps, float32 taps) of its own batch of one."""
    rng = np.random.RandomState(seed)
    utts = [rng.randn(L, 80).astype(np.float32) for L in lens]
    return [(u, oracle_taps(_sd(name), name, u[None], torch.float64), oracle_taps(_sd(name), name, u[None], torch.float32))
            for u in utts]


def _ragged_case(name, prec, lens, TS, seed):
    """tests/test_gpu_resnet_layers.py::_ragged_case for this family: stops 0 .. 16 and the full forward."""
    B = len(lens)
    refs = _ragged_refs(name, tuple(lens), seed)
    pad = np.full((B, TS, 80), np.nan, dtype=np.float32)
    for b, (u, _, _) in enumerate(refs):
        pad[b, :len(u)] = u
    model = _engine(name, 8, TS).set_precision(prec)
    rows, checks, lines = [], [], []
    try:
        for n in list(range(17)) + [-1]:
            emb = _run(model, pad, n, list(lens)) if n >= 0 else _logged_run(model, pad, n, list(lens), lines)
            lvl = STAGE_OF[n] if n >= 0 else None
            for key in _keys_at(n, refs[0][1]):
                kind = _kind(key)
                slot = model.tap(kind).cpu().numpy()
                assert not np.isnan(slot).any(), key
                if kind == "pooled":
                    for b in range(B):
                        tag = "pooled[%d]" % b
                        checks.append((tag, tap_check(tag, slot[b:b + 1], refs[b][1][key], refs[b][2][key], K_TAP, rows)[0]))
                    continue
                level = FUSIONS.index(kind) + 1 if kind in FUSIONS else lvl
                Hn, C = refs[0][1][key].shape[1], refs[0][1][key].shape[3]
                slot = slot.reshape(B, Hn, _level_len(TS, level), C)
                for b, L in enumerate(lens):
                    Wv = _level_len(L, level)
                    r64, r32 = refs[b][1], refs[b][2]
                    assert r64[key].shape[2] == Wv
                    tag = "%s[%d]" % (key, b)
                    checks.append((tag, tap_check(tag, slot[b:b + 1, :, :Wv], r64[key], r32[key], K_TAP, rows)[0]))
                    if kind != "stem":
                        tail = slot[b, :, Wv:]
                        assert not tail.any(), "%s: %d non-zero values in the padding columns of utterance %d (len %d)" % (
                            key, int(np.count_nonzero(tail)), b, L)
        print("\n".join(lines))
        head = "rows=%d N=192 " % B                             # (seg_1 over the pooled rows: one row per utterance)
        assert lines and all("+mask" in ln for ln in lines if not ln.startswith(head)), lines
        assert sum(ln.startswith(head) for ln in lines) == 1, lines
        assert np.isfinite(emb).all()
        for b, (u, r64, r32) in enumerate(refs):
            tag = "emb[%d]" % b
            checks.append((tag, tap_check(tag, emb[b:b + 1], r64["emb"], r32["emb"], K_TAP, rows)[0]))
            one = model(torch.from_numpy(u[None])).cpu().numpy().astype(np.float64)
            err = float(np.linalg.norm(emb[b] - one[0]) / np.linalg.norm(one[0]))
            print("row %d (%d frames) vs its batch of one: %.2e" % (b, lens[b], err))
            assert err < RAGGED_VS_SINGLE_TOL, (b, lens[b], err)
        _check_invariants(model)
    finally:
        model.set_precision("fp32")
    _assert_all("ragged %s %s" % (name, prec), checks, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_every_tap_ragged_batch_and_its_zero_padding_columns(prec):
    """Base, five utterances of 131 / 113 / 64 / 57 / 9 frames in 131-frame slots, NaN in the feature padding.  Columns
    of an utterance: every tap equals the batch-1 oracle of that utterance.  Columns beyond its length at that stride
    level: mid, cat, sc, block and the three fusions are EXACTLY zero -- eres2net_model.hip passes cur_lens[level] to
    every launch, and every later 3x3 border tap and the pooling rest on it."""
    _ragged_case(BASE, prec, (131, 113, 64, 57, 9), 131, 131)


@pytest.mark.gpu
def test_aug_ragged_batch_partial_column_tiles_under_the_row_mask():
    """aug, 57 / 33 / 9 frames in 57-frame slots, fp32: N = 24 column tiles and three branches with the row mask."""
    _ragged_case(AUG, "fp32", (57, 33, 9), 57, 57)


@pytest.mark.gpu
def test_ragged_large_batch_on_the_masked_128_row_tiles():
    """Base, B = 16, T = 208, lens in [150, 208] (seed 16), blocks 4 - 5: the 128-row kernels with the row mask.  The
    three spot utterances keep their full length and meet the tap bound; the padding columns of the first utterance
    shorter than 200 frames are exactly zero in mid, cat, sc and block.  Utterance 15 holds the rows of the dual
    kernel's 64x64 half (rows 65 536 .. 66 560: its frequency rows 31 .. 39 and a part of row 30): it is cut to 171
    frames and judged against its own batch-1 oracle, columns and padding, so that the small tile's residual / clamp /
    mask epilogue at a non-zero row origin is value-checked."""
    B, L_LAST = 16, 171
    spots = _spots(B)[:3]
    lens = [int(x) for x in np.random.RandomState(B).randint(150, LARGE_T + 1, size=B)]
    for s in spots:
        lens[s] = LARGE_T
    lens[B - 1] = L_LAST
    keep = lambda k: k.startswith(("b4.", "b5."))  # noqa: E731
    u_last = _large_base(LARGE_T)[(B - 1) % 3][None, :L_LAST]
    l64, l32 = (oracle_taps(_sd(BASE), BASE, u_last, dt, keep=keep) for dt in (torch.float64, torch.float32))
    cut = min(b for b in range(B) if lens[b] < 200)
    feats = _large_base(LARGE_T)[np.arange(B) % 3].copy()
    for b, L in enumerate(lens):
        feats[b, L:] = np.nan
    r64, r32 = _large_refs(BASE, LARGE_T)
    model = _engine(BASE, B, LARGE_T, tag="ragged")
    rows, checks, lines = [], [], []
    try:
        for n in (4, 5):
            _logged_run(model, feats, n, lens, lines)
            _check_taps(model, n, r64, r32, rows, checks, spots, [s % 3 for s in spots])
            for key in _keys_at(n, r64):
                slot = model.tap(_kind(key)).reshape((B,) + r64[key].shape[1:])
                tail = slot[cut, :, _level_len(lens[cut], 1):].cpu().numpy()
                assert tail.size and not tail.any(), (key, cut, lens[cut], int(np.count_nonzero(tail)))
                assert not torch.isnan(slot).any(), key
                last, Wv = slot[B - 1].cpu().numpy(), _level_len(L_LAST, 1)
                assert l64[key].shape[2] == Wv and not last[:, Wv:].any(), (key, int(np.count_nonzero(last[:, Wv:])))
                tag = "%s[15]" % key
                checks.append((tag, tap_check(tag, last[None, :, :Wv], l64[key], l32[key], K_TAP, rows)[0]))
                # ... and the rows of the dual kernel's 64x64 half alone (frequency rows 31 .. 39 lie wholly in it)
                tag = "%s[15,f>=31]" % key
                checks.append((tag, tap_check(tag, last[None, 31:, :Wv], l64[key][:, 31:], l32[key][:, 31:], K_TAP, rows)[0]))
        assert _assert_tails_are_read(lines, B, 66560) >= 2
    finally:
        del _ENGINES[(BASE, B, LARGE_T, "ragged")], model
    _assert_forms(lines, [
        ("rows=66560 N=32 K=288 k=3x3", "!+A2", "+mask", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=66560 N=32 K=288 k=3x3", "+A2", "+mask", "+relu20", "conv_gemm_kernel<128,32"),
        ("rows=66560 N=64 K=64 k=1x1 s=2x2", "+mask", "+relu20", "conv_gemm_kernel<128,64"),
        ("rows=66560 N=128 K=64 k=1x1 s=1x1", "+res", "+mask", "+relu20", "128,128"),
        ("+mask", "+relu20", "conv_gemm_dual_kernel")])
    _assert_all("ragged Base B=16 T=208", checks, rows)
