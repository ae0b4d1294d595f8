"""Per-layer ECAPA parity: the activations a forward leaves in the engine's workspace (NativeSpeakerModel.tap,
ws_debug_engine_tap) against the float64 oracle, tap by tap.

tests/test_gpu_parity.py judges the ECAPA path by the embedding alone, at REL_TOL = 2e-4 -- about 400x what a faithful
fp32 forward needs (fp32 oracle vs float64 oracle: 4.5e-7), behind a chain of 18 launches that dilutes a local error
further.  Here every tap is compared where it is produced, and the bound is not a constant:

    reference   ecapa_forward(..., dtype=torch.float64, return_intermediates=True)
    metrics     scaled max error  max|got - ref| / max|ref|   and   relative L2  |got - ref| / |ref|
    bound       k x the same metric of the fp32 CPU oracle against the float64 oracle, same inputs, same tap
                (oracle error floored at 2^-24: the scaled error of ONE correctly rounded fp32 store; an fp32 result
                cannot be asked to be closer than that, however lucky the CPU's summation order was)

k (K_FP32 / K_F16X3 below, per tap):
  fp32   8 for every tap: the device and the CPU oracle are two different fp32 summation orders, each about as far
         from the truth as the other (2x), the device has its own tanh / exp / sigmoid (a few ulps), and the context
         std in its sums-of-squares form costs a few more.
  f16x3  8 as well, per tap.  The split-binary16 back-end forms a product as hi*hi + hi*lo + lo*hi of operands cut to
         22 significant bits -- a relative product error of ~2^-21 (include/wespeaker_amd.h) where fp32 rounds at
         2^-24 -- so the number format alone would allow 8 x 8 = 64.  Measured, no tap needs it: the product errors are
         independent and average out under the same fp32 accumulation (worst ratio 3.8), so the back-end is held to
         the fp32 allowance, with a factor of two in hand at the worst tap.

Every test prints its table (tap, fp32-oracle error, device error, ratio = device / fp32-oracle; run with -s).
Measured on MI355X, standard fixture (B = 3, T = 198, seed 42), worst of the two metrics, worst of the four constructors:

                 fp32 back-end                          f16x3 back-end
    tap        oracle32   device    ratio   worst*      oracle32   device    ratio   worst*
    out1       2.3e-07    6.0e-07   2.64    3.83        2.3e-07    6.2e-07   2.76    2.76
    y1         7.5e-07    1.5e-06   2.02    2.35        7.5e-07    1.4e-06   1.91    2.12
    y2         4.4e-07    9.4e-07   2.14    2.43        8.2e-07    1.3e-06   1.94    2.28
    y3         1.0e-06    1.4e-06   1.81    1.89        1.0e-06    1.7e-06   2.09    2.22
    se_s       1.5e-06    1.0e-06   0.75    1.42        1.5e-06    3.3e-06   2.18    2.67
    cat        1.6e-06    1.6e-06   1.52    2.16        1.6e-06    2.2e-06   1.98    2.44
    h          7.8e-07    1.9e-06   2.37    3.99        7.8e-07    1.9e-06   2.40    3.44
    stats      4.6e-07    6.6e-07   1.45    3.39        2.9e-07    9.7e-07   3.33    3.78
    bias_img   7.9e-07    4.9e-07   0.67    1.23        7.9e-07    1.4e-06   1.94    2.01
    pooled     5.9e-07    9.9e-07   1.68    2.16        6.4e-07    2.4e-06   3.78    3.78
    emb        7.8e-07    7.9e-07   1.00    1.33        7.8e-07    1.4e-06   1.99    2.18
    (oracle32 / device: error against the float64 oracle in the case with the worst ratio.  * worst ratio over every
    case of this file: T = 198 / 64 / 57 / 5, the ragged batch, the persistent-kernel batch, the segmented pooling.)
No tap needs more than k = 8 in either back-end; the largest ratio anywhere is 3.99 (h, fp32, T = 5).  Other cases:
persistent-kernel path 0.7 .. 3.0 (h beyond column 416: 2.07), ragged 0.8 .. 2.1 (fp32) / 1.2 .. 3.1 (f16x3), segmented
pooling with empty segments 0.6 .. 1.0, the cancelling channel's context std 0.10 (fp32 oracle 1.8e-3 of the channel's
own std, device 1.8e-4: the two-pass recomputation is closer to the truth than torch's fp32 var).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ecapa as oecapa
from oracle import fbank as ofbank
from fixtures import synth

REL_TOL = 2e-4           # the embedding bar of tests/test_gpu_parity.py (what the taps are so much tighter than)
ERR_FLOOR = 2.0 ** -24   # see the module docstring

FRAME_TAPS = ("out1", "cat", "h", "y1", "y2", "y3")
UTT_TAPS = ("se_s", "stats", "bias_img", "pooled")
GLOB_ONLY = ("stats", "bias_img")
K_FP32 = {t: 8.0 for t in FRAME_TAPS + UTT_TAPS + ("emb",)}
K_F16X3 = {t: 8.0 for t in FRAME_TAPS + UTT_TAPS + ("emb",)}
K = {"fp32": K_FP32, "f16x3": K_F16X3}

NAMES = ["ECAPA_TDNN_GLOB_c512", "ECAPA_TDNN_c512", "ECAPA_TDNN_GLOB_c1024", "ECAPA_TDNN_c1024"]


# ------------------------------------------------------------------------------------------- the comparison (CPU)
def tap_errors(got, ref):
    """(scaled max error, relative L2) of got against ref, in float64."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    d = got - ref
    return float(np.abs(d).max() / np.abs(ref).max()), float(np.sqrt((d * d).sum() / (ref * ref).sum()))


def tap_check(name, got, ref64, ref32, k, rows=None, floor=ERR_FLOOR):
    """Is `got` within k x (fp32 oracle's error) of the float64 oracle, on both metrics?  -> (ok, ratio) with
    ratio = worst of device error / fp32-oracle error; appends a line to `rows` for the printed table.
    floor: the oracle error's floor -- one correctly rounded store of the tap's format (tests/f16_layer_oracle.py passes
    2^-11 for a binary16 tensor)."""
    e_dev, e_ref = tap_errors(got, ref64), tap_errors(ref32, ref64)
    base = [max(e, floor) for e in e_ref]
    ratio = max(d / b for d, b in zip(e_dev, base))
    if rows is not None:
        rows.append("%-9s oracle32 max %.2e l2 %.2e | device max %.2e l2 %.2e | ratio %6.2f (k = %g)"
                    % (name, e_ref[0], e_ref[1], e_dev[0], e_dev[1], ratio, k))
    return bool(np.isfinite(np.asarray(got)).all()) and ratio <= k, ratio


def oracle_taps(sd, feats, dtype):
    """name -> numpy array in the engine's layout: frame-level taps (B, T, cols), utterance-level (B, cols); + emb."""
    emb, mid = oecapa.ecapa_forward(sd, np.array(feats), return_intermediates=True, dtype=dtype)
    cl = lambda t: t.permute(0, 2, 1).contiguous().numpy()                  # channels last
    out = {"out1": cl(mid["out1"]), "cat": cl(torch.cat([mid["out2"], mid["out3"], mid["out4"]], dim=1)),
           "h": cl(mid["h"]), "y1": cl(mid["y1"]), "y2": cl(mid["y2"]), "y3": cl(mid["y3"]),
           "se_s": mid["se_s"].numpy(), "pooled": mid["pooled"].numpy(), "emb": emb.numpy()}
    for t in GLOB_ONLY:
        if t in mid:
            out[t] = mid[t].numpy()
    return out


@functools.lru_cache(maxsize=None)
def _fixture_feats():
    f = np.stack([ofbank.speaker_features(synth.synth_wav(i)) for i in range(3)])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _sd(name):
    return synth.synth_ecapa_state_dict(name, 80, 192, seed=42)


@functools.lru_cache(maxsize=None)
def _fixture_refs(name, T):
    """(float64 taps, fp32 taps) of the fixture features cut to T frames: computed once, shared by the precisions."""
    f = _fixture_feats()[:, :T]
    return oracle_taps(_sd(name), f, torch.float64), oracle_taps(_sd(name), f, torch.float32)


def test_the_per_tap_bound_has_teeth():
    """Why this file exists (CPU): errors that the embedding bar lets through must fail the per-tap bound.  On the
    standard fixture (GLOB_c512, seed 42, two 198-frame utterances), fed to the very comparison the GPU tests use:
    one 64-frame x 64-channel tile of h scaled by 1 + 1e-4 (a wrong BN scale in one column tile, a dropped K-tile, an
    epilogue storing a neighbour's column sums), and one channel of out3 shifted by 1e-4 of its range (a BN shift read
    from the neighbouring channel).  Both leave the embedding inside REL_TOL and both are refused here -- which also
    keeps the k's from drifting up to uselessness."""
    name = "ECAPA_TDNN_GLOB_c512"
    sd, f = _sd(name), _fixture_feats()[:2]
    r64, r32 = oracle_taps(sd, f, torch.float64), oracle_taps(sd, f, torch.float32)
    k = K_FP32
    rows = []
    for t in FRAME_TAPS + UTT_TAPS + ("emb",):       # the float64 oracle itself passes, so does the fp32 oracle (k >= 1)
        assert tap_check(t, r64[t], r64[t], r32[t], k[t])[0] and tap_check(t, r32[t], r64[t], r32[t], k[t], rows)[0]
    # the slack the issue measured: fp32 oracle vs float64 oracle is below 1e-6 at every tap, 400x inside REL_TOL
    assert max(max(tap_errors(r32[t], r64[t])) for t in FRAME_TAPS + UTT_TAPS + ("emb",)) < 2e-6, rows
    emb64 = r64["emb"]
    rel = lambda e: float((np.linalg.norm(e - emb64, axis=1) / np.linalg.norm(emb64, axis=1)).max())

    h_bad = r64["h"].copy()                                        # (B, T, 1536)
    h_bad[0, 64:128, 640:704] *= 1.0 + 1e-4
    ok, ratio = tap_check("h", h_bad, r64["h"], r32["h"], k["h"], rows)
    assert not ok and ratio > k["h"], rows
    e_bad = oecapa.ecapa_resume(sd, torch.float64, h=torch.from_numpy(h_bad).permute(0, 2, 1)).numpy()
    assert 0.0 < rel(e_bad) < REL_TOL, rel(e_bad)

    # the channel of median range: a typical one (over all 512 the ratio runs from 4.7 to 61 with a median of 14 --
    # the narrowest sixth of the channels would still slip through k = 8, a shift of 1e-4 of THEIR range being that small)
    C = 512
    cat_bad = r64["cat"].copy()                                    # (B, T, 3C) = out2 | out3 | out4
    out3 = cat_bad[:, :, C:2 * C]
    c = int(np.argsort(out3.max(axis=(0, 1)) - out3.min(axis=(0, 1)))[C // 2])
    ch = cat_bad[:, :, C + c]
    cat_bad[:, :, C + c] += 1e-4 * (ch.max() - ch.min())
    ok, ratio = tap_check("cat", cat_bad, r64["cat"], r32["cat"], k["cat"], rows)
    assert not ok and ratio > k["cat"], rows
    cf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 2, 1)
    e_bad = oecapa.ecapa_resume(sd, torch.float64, out2=cf(cat_bad[:, :, :C]), out3=cf(cat_bad[:, :, C:2 * C])).numpy()
    assert 0.0 < rel(e_bad) < REL_TOL, rel(e_bad)
    # ecapa_resume is the forward's own tail: unperturbed it returns the embedding
    e_same = oecapa.ecapa_resume(sd, torch.float64, out2=cf(r64["cat"][:, :, :C]), out3=cf(r64["cat"][:, :, C:2 * C]))
    assert rel(e_same.numpy()) < 1e-12
    print("\n".join(rows))


# ------------------------------------------------------------------------------------------------------- GPU side
_ENGINES = {}


def _engine(name, max_batch=8, max_frames=400, sd=None, key=None):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = key or (name, max_batch, max_frames)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel(name, sd if sd is not None else _sd(name), feat_dim=80, embed_dim=192,
                                           max_batch=max_batch, max_frames=max_frames)
    return _ENGINES[key]


def _device_taps(model, B, T, names):
    return {t: model.tap(t).cpu().numpy().reshape((B, T, -1) if t in FRAME_TAPS else (B, -1)) for t in names}


def _tap_names(name):
    return [t for t in FRAME_TAPS + UTT_TAPS if "GLOB" in name or t not in GLOB_ONLY]


def _assert_all(tag, checks, rows):
    print("\n%s\n%s" % (tag, "\n".join(rows)))
    bad = [t for t, ok in checks if not ok]
    assert not bad, "%s: taps beyond their bound (the FIRST one names the launch): %s\n%s" % (tag, bad, "\n".join(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [198, 57, 5, 64])
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
@pytest.mark.parametrize("name", NAMES)
def test_every_tap_small_uniform_batch(name, prec, T):
    """B = 3 fixture utterances cut to T frames, all four constructors.  T = 198: the tile kernels, SE from the conv3
    epilogue's column sums, the pooling branch the dispatcher picks; T = 57 and 5: the T < 64 fallbacks
    (launch_se_pool_fc, launch_astp_stats, launch_astp_pool); T = 64: the threshold itself."""
    model = _engine(name).set_precision(prec)
    try:
        emb = model(torch.from_numpy(_fixture_feats()[:, :T].copy()))[-1].cpu().numpy()
        got = _device_taps(model, 3, T, _tap_names(name))
    finally:
        model.set_precision("fp32")
    got["emb"] = emb
    r64, r32 = _fixture_refs(name, T)
    rows, checks = [], []
    for t in _tap_names(name) + ["emb"]:
        checks.append((t, tap_check(t, got[t], r64[t], r32[t], K[prec][t], rows)[0]))
    _assert_all("%s %s T=%d" % (name, prec, T), checks, rows)


@pytest.mark.gpu
def test_every_tap_on_the_persistent_kernel_path():
    """GLOB_c512, fp32, B = 128 x T = 130 = 16 640 rows: above the 16 384-row threshold at which layer 1 becomes an fp32
    im2col image in the (not yet used) h buffer + a plain GEMM, and the 1x1 GEMMs go to gemm_f32_stream_kernel with the
    context statistics from the epilogue's sums and sums of squares.  Utterances 0, 64, 127 against the oracle on every
    tap; h in particular was im2col scratch first (416 columns per row) and must be the catconv output on all 1536."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    name, B, T = "ECAPA_TDNN_GLOB_c512", 128, 130
    spots = [0, 64, 127]
    f = np.random.RandomState(130).randn(B, T, 80).astype(np.float32)
    model = _engine(name, max_batch=B, max_frames=T)
    dispatch_log(True, clear=True)
    try:
        emb = model(torch.from_numpy(f))[-1].cpu().numpy()
        lines = dispatch_report()
    finally:
        dispatch_log(False, clear=True)
    got = {t: v[spots] for t, v in _device_taps(model, B, T, _tap_names(name)).items()}
    got["emb"] = emb[spots]
    # layer 1 as a 1x1 GEMM over the im2col image (K = 5 * 80 rounded up to 32 = 416) on the persistent kernel ...
    assert any("N=512 K=416 k=1x1" in l and "gemm_f32_stream_kernel" in l for l in lines), lines
    # ... and catconv there too, with column sums and no mask: the one condition under which ecapa_model.hip attaches
    # the sums of squares and calls launch_astp_std_from_sums (fp32, GLOB, T >= 64, not ragged)
    cat_lines = [l for l in lines if "N=1536 K=1536 " in l and "+colsum" in l]
    assert cat_lines and all("gemm_f32_stream_kernel" in l and "+mask" not in l and "prec=0" in l for l in cat_lines), lines
    r64, r32 = oracle_taps(_sd(name), f[spots], torch.float64), oracle_taps(_sd(name), f[spots], torch.float32)
    rows, checks = [], []
    for t in _tap_names(name) + ["emb"]:
        checks.append((t, tap_check(t, got[t], r64[t], r32[t], K_FP32[t], rows)[0]))
    checks.append(("h[:, 416:]", tap_check("h[416:]", got["h"][:, :, 416:], r64["h"][:, :, 416:], r32["h"][:, :, 416:],
                                           K_FP32["h"], rows)[0]))
    _assert_all("persistent path", checks, rows)


RAGGED_LENS = [160, 113, 129, 75, 64, 5]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_every_tap_ragged_batch_and_its_zero_padding_rows(prec):
    """GLOB_c512, six utterances in 160-row slots, NaN in the feature padding.  Rows of an utterance: every frame-level
    tap equals the batch-1 oracle of that utterance.  Rows beyond it: out1, cat, h and y3 are EXACTLY zero -- the
    column sums behind the SE means and the context statistics are taken over whole slots and only divided by lens[b],
    so they rest on these zeros.  se_s / stats / bias_img / pooled equal the batch-1 oracle (divisors lens[b])."""
    name, TS = "ECAPA_TDNN_GLOB_c512", 160
    B = len(RAGGED_LENS)
    rng = np.random.RandomState(160)
    utts = [rng.randn(L, 80).astype(np.float32) for L in RAGGED_LENS]
    pad = np.full((B, TS, 80), np.nan, dtype=np.float32)
    for b, u in enumerate(utts):
        pad[b, :len(u)] = u
    model = _engine(name).set_precision(prec)
    try:
        emb = model.embed_ragged(torch.from_numpy(pad), RAGGED_LENS).cpu().numpy()
        got = _device_taps(model, B, TS, _tap_names(name))
    finally:
        model.set_precision("fp32")
    assert np.isfinite(emb).all()
    rows, checks = [], []
    for b, u in enumerate(utts):
        L = len(u)
        r64, r32 = oracle_taps(_sd(name), u[None], torch.float64), oracle_taps(_sd(name), u[None], torch.float32)
        for t in _tap_names(name):
            g = got[t][b:b + 1, :L] if t in FRAME_TAPS else got[t][b:b + 1]
            checks.append(("%s[%d]" % (t, b), tap_check("%s[%d]" % (t, b), g, r64[t], r32[t], K[prec][t], rows)[0]))
        checks.append(("emb[%d]" % b, tap_check("emb[%d]" % b, emb[b:b + 1], r64["emb"], r32["emb"], K[prec]["emb"], rows)[0]))
        for t in ("out1", "cat", "h", "y3"):
            tail = got[t][b, L:]
            assert tail.size == (TS - L) * got[t].shape[2]
            assert not tail.any(), "%s: %d non-zero values in the padding rows of utterance %d (len %d)" % (
                t, int(np.count_nonzero(tail)), b, L)
    _assert_all("ragged %s" % prec, checks, rows)


@pytest.mark.gpu
def test_segmented_pooling_with_empty_trailing_segments():
    """astp_fused_kernel on segments (T = 798: 4 x 200 frames) of a ragged batch in which utterances END inside the
    first segment: lens 150 and 64 leave segments 1..3 without a single live frame (their tuples must merge as weight
    0), the rest keep lens >= T - 150.  pooled and the embedding of those utterances and of a full one: finite and
    equal to the batch-1 oracle within the per-tap bound; the dispatch log names the kernel."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    name, B, T = "ECAPA_TDNN_GLOB_c512", 64, 798
    f = np.random.RandomState(T).randn(B, T, 80).astype(np.float32)
    lens = np.random.RandomState(B).randint(T - 150, T + 1, size=B)
    spots = {0: 798, 31: 150, 63: 64}
    for b, L in spots.items():
        lens[b] = L
    pad = np.full((B, T, 80), np.nan, dtype=np.float32)
    for b in range(B):
        pad[b, :lens[b]] = f[b, :lens[b]]
    model = _engine(name, max_batch=B, max_frames=T)
    dispatch_log(True, clear=True)
    try:
        emb = model.embed_ragged(torch.from_numpy(pad), [int(x) for x in lens]).cpu().numpy()
        lines = dispatch_report()
    finally:
        dispatch_log(False, clear=True)
    pooled = model.tap("pooled").cpu().numpy()
    assert pooled.shape == (B, 3072)
    assert any("astp_fused_kernel" in l for l in lines), lines
    assert np.isfinite(pooled).all() and np.isfinite(emb).all()
    rows, checks = [], []
    for b, L in spots.items():
        u = f[b:b + 1, :L]
        r64, r32 = oracle_taps(_sd(name), u, torch.float64), oracle_taps(_sd(name), u, torch.float32)
        checks.append(("pooled[%d]" % b, tap_check("pooled[%d]" % b, pooled[b:b + 1], r64["pooled"], r32["pooled"],
                                                   K_FP32["pooled"], rows)[0]))
        checks.append(("emb[%d]" % b, tap_check("emb[%d]" % b, emb[b:b + 1], r64["emb"], r32["emb"], K_FP32["emb"], rows)[0]))
    _assert_all("segments with empty tails", checks, rows)


@pytest.mark.gpu
def test_context_std_of_the_cancelling_channel():
    """The weight set of test_ecapa_glob_context_std_two_pass_fallback (channel 5 of h at ~200 with a spread of a few
    1e-2: the single-pass sums-of-squares form loses its variance and the kernel recomputes it in two passes), judged
    where it is produced: the `stats` tap's std of that channel against the float64 oracle, relative to the channel's
    OWN value, within k x what the fp32 oracle gets on the same channel.  Until now only seen through the attention."""
    c = 5
    sd = synth.cancelling_channel_state_dict(c=c)
    feats = np.stack([ofbank.speaker_features(synth.synth_wav(50 + i)) for i in range(4)])
    model = _engine("ECAPA_TDNN_GLOB_c512", sd=sd, key="cancelling")
    model(torch.from_numpy(feats))
    got = model.tap("stats").cpu().numpy()
    r64, r32 = oracle_taps(sd, feats, torch.float64), oracle_taps(sd, feats, torch.float32)
    assert (r64["stats"][:, 1536 + c] / r64["stats"][:, c] < 0.03).all()       # the kernel's `cancelled` condition
    rows, checks = [], []
    for what, col in (("mean", c), ("std", 1536 + c)):
        e_dev = float((np.abs(got[:, col] - r64["stats"][:, col]) / np.abs(r64["stats"][:, col])).max())
        e_ref = float((np.abs(r32["stats"][:, col] - r64["stats"][:, col]) / np.abs(r64["stats"][:, col])).max())
        ratio = e_dev / max(e_ref, ERR_FLOOR)
        rows.append("stats %-4s of channel %d: oracle32 %.2e | device %.2e | ratio %.2f (k = %g)"
                    % (what, c, e_ref, e_dev, ratio, K_FP32["stats"]))
        checks.append((what, ratio <= K_FP32["stats"]))
    checks.append(("stats", tap_check("stats", got, r64["stats"], r32["stats"], K_FP32["stats"], rows)[0]))
    _assert_all("cancelling channel", checks, rows)


@pytest.mark.gpu
def test_tap_api_edges():
    from wespeaker_amd import _lib
    from wespeaker_amd.engine import NativeSpeakerModel
    import ctypes
    name = "ECAPA_TDNN_c512"
    model = NativeSpeakerModel(name, _sd(name), feat_dim=80, embed_dim=192, max_batch=8, max_frames=200)

    def raw(m, tap, dst=None, cap=0):
        r, c = ctypes.c_int32(-7), ctypes.c_int32(-7)
        rc = _lib.lib().ws_debug_engine_tap(m._h, tap.encode(), dst, cap, ctypes.byref(r), ctypes.byref(c),
                                            _lib.current_stream_ptr(m.device))
        return rc, r.value, c.value, _lib.lib().ws_last_error().decode()

    # before any forward
    rc, _, _, msg = raw(model, "pooled")
    assert rc == -1 and "no forward" in msg
    with pytest.raises(_lib.NativeError, match="no forward"):
        model.tap("pooled")
    f = np.random.RandomState(11).randn(11, 70, 80).astype(np.float32)
    first = model(torch.from_numpy(f))[-1].clone()
    # unknown name; a GLOB-only tensor on a model without global context
    rc, _, _, msg = raw(model, "out5")
    assert rc == -1 and "unknown tensor 'out5'" in msg
    rc, _, _, msg = raw(model, "stats")
    assert rc == -1 and "GLOB" in msg
    # NULL destination: the shape alone.  11 utterances on max_batch = 8: the tap holds the LAST chunk, utterances 8..10
    assert raw(model, "h")[:3] == (0, 3 * 70, 1536)
    assert raw(model, "pooled")[:3] == (0, 3, 3072) and raw(model, "cat")[:3] == (0, 3 * 70, 3 * 512)
    assert model.tap_shape("se_s") == (3, 512)
    small = torch.empty(16, device=model.device)
    rc, _, _, msg = raw(model, "h", _lib.ptr(small), 16)
    assert rc == -7 and "210 x 1536" in msg and "holds 16" in msg          # WS_ERR_CAPACITY, nothing copied
    chunk = {t: model.tap(t) for t in ("out1", "h", "pooled")}
    # after the taps a second forward has the first one's bits
    assert torch.equal(model(torch.from_numpy(f))[-1], first)
    model(torch.from_numpy(f[8:11].copy()))
    for t, v in chunk.items():
        assert torch.equal(model.tap(t), v), t
    model(torch.from_numpy(f[0:3].copy()))
    assert not torch.equal(model.tap("pooled"), chunk["pooled"])
    # f16 back-end, T >= 64: the block chain and h live in binary16 only; the fp32 tensors of the same forward still tap
    model.set_precision("f16")
    model(torch.from_numpy(f[:2].copy()))
    for t in ("h", "out1", "cat", "y3"):
        rc, _, _, msg = raw(model, t)
        assert rc == -1 and "binary16" in msg, (t, msg)
    assert raw(model, "pooled")[:3] == (0, 2, 3072) and raw(model, "y1")[:3] == (0, 2 * 70, 512)
    model(torch.from_numpy(f[:2, :40].copy()))               # T < 64: fp32 tensors again
    assert raw(model, "h")[:3] == (0, 2 * 40, 1536)
    model.set_precision("fp32")
    # re-sizing the workspace forgets the last chunk
    model.reserve(4, 100)
    rc, _, _, msg = raw(model, "pooled")
    assert rc == -1 and "no forward" in msg
    # another family's names: CAM++ has its own table (tests/test_gpu_campplus_layers.py) and refuses, with the reason,
    # the tensors that its fused dense-block kernel keeps in LDS
    csd = synth.synth_state_dict("CAMPPlus", 80, 512, seed=42)
    cam = NativeSpeakerModel("CAMPPlus", csd, feat_dim=80, embed_dim=512, max_batch=2, max_frames=100)
    cam(torch.from_numpy(f[:2, :64].copy()))
    rc, _, _, msg = raw(cam, "out1")
    assert rc == -1 and "unknown tensor 'out1'" in msg and "CAMPPlus" in msg
    rc, _, _, msg = raw(cam, "h")
    assert rc == -1 and "stay in LDS" in msg
    assert raw(cam, "dense")[:3] == (0, 2 * 32, 1024)
