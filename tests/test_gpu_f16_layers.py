"""Per-launch parity of ECAPA-TDNN's binary16 back-end (WS_PREC_F16): every tensor a forward leaves in the workspace
(NativeSpeakerModel.tap, the *16 names and the stop points 1 .. 3) against the launch-local oracle of
tests/f16_layer_oracle.py, fed with the DEVICE's own inputs of that launch.  The embedding tests of
tests/test_gpu_parity.py sit behind 18 launches and a bar of 1.5e-3; here a launch is judged alone:

  A  one binary16 store of an fp32-accumulated value (out1_16, y3_16, cat16, h16, att16, y2_16): every element is the
     oracle's rounding, its binary16 neighbour, or within eps = 8 x the float32 baseline's error; the share of elements
     that differ from the oracle's rounding is at most 8 x the baseline's share (floored at 16 / numel), per tap and
     per channel.
  B  fp32 outputs (y1, se_s, stats, bias_img, att, pooled, emb) and the Res2 chain's y2_16: tap_check with k = 8
     against the launch oracle, floor 2^-24 (2^-11 for y2_16).
  T < 64 keeps the fp32 tensors: they pass B, and every binary16 copy is the rounding of its fp32 tensor bit for bit.

Measured on MI355X, worst over the cases of this file (the full table: DESIGN.md, section 4.2.18).  A: share of elements
!= R(oracle) 3e-4 .. 1.6e-3 on the device against 4e-4 .. 1.7e-3 for the float32 baseline, worst share ratio 1.41
(y2_16, att16) of 8, no element outside the ulp / eps clause; B: worst ratio 2.19 (att), 1.95 (stats), the rest below
1.6, of 8; every binary16 copy at T < 64 equals R(fp32 tensor).  Every test prints its table (run with -s).
"""
import functools
import re

import numpy as np
import pytest
import torch

import f16_layer_oracle as fo
from f16_layer_oracle import rnd16
from oracle import ecapa as oecapa
from test_gpu_layers import RAGGED_LENS, _assert_all, _engine, _fixture_feats, _sd, oracle_taps

COS_TOL = 1e-4            # the embedding bars of tests/test_gpu_parity.py that the per-launch checks are so much tighter than
F16_REL_TOL = 1.5e-3
F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------- one utterance, every launch
def verify(sd, name, taps, feats, rows, checks, tag, L=2, full=True, half=True, summed16=None):
    """taps: name -> (B, T, cols) / (B, cols) arrays of the utterances in `feats` (B, T, F), own rows only.
    L: the block whose y1 / y2_16 / y3 / se_s the taps hold; full: pooling and head ran (taps['emb'] = the embedding).
    half: the all-binary16 chain (T >= 64); else the fp32 tensors exist beside their binary16 copies.
    summed16: {'conv3': mask, 'catconv': mask} boolean (B, T) -- rows whose column sums were taken from the STORED
    binary16 values (the 256 x 256 kernel's binary16 epilogue); None: from the fp32 values everywhere."""
    glob = "GLOB" in name
    C = taps["out1_16"].shape[-1]
    w = C // 8
    both = lambda f, *a: (f(*a, F64), f(*a, F32))

    def A(t, Y, y):
        checks.append((tag + t, fo.check_a(tag + t, Y, y[0], y[1], rows)[0]))

    def Bc(t, got, y, floor=None):
        checks.append((tag + t, fo.check_b(tag + t, got, y[0], y[1], rows, floor)[0]))

    def same_bits(t16, t32):
        ok = np.array_equal(taps[t16], rnd16(taps[t32]))
        rows.append("%-12s == R(%s) bit for bit: %s" % (tag + t16, t32, ok))
        checks.append((tag + t16 + "==R(%s)" % t32, ok))

    def summed(key, y):                    # what the epilogue's column sums added up, per evaluation
        m = None if summed16 is None else summed16.get(key)
        return tuple(v if m is None else np.where(m[:, :, None], rnd16(v), v) for v in y)

    if "col16" in taps:
        ok = np.array_equal(taps["col16"], fo.im2col(feats, taps["col16"].shape[-1]))
        rows.append("%-12s == R(features) in im2col order, zero padded, bit for bit: %s" % (tag + "col16", ok))
        checks.append((tag + "col16", ok))
    y = both(fo.layer1, sd, feats)
    if half:
        A("out1_16", taps["out1_16"], y)
    else:
        Bc("out1", taps["out1"], y)
        same_bits("out1_16", "out1")
    # block L
    x16 = taps["out1_16"] if L == 0 else taps["cat16"][:, :, (L - 1) * C:L * C]
    y = both(fo.conv1, sd, L, x16)
    Bc("y1", taps["y1"], y)
    A("y2_16[7w:]", taps["y2_16"][:, :, 7 * w:], tuple(v[:, :, 7 * w:] for v in y))
    y = both(fo.res2, sd, L, taps["y1"])
    Bc("y2_16[:7w]", taps["y2_16"][:, :, :7 * w], tuple(rnd16(v) for v in y), floor=fo.ULP16_FLOOR)
    # (stricter than asked: the chain never rounds its running activation to binary16 -- res2_fused.hip -- so its output
    # is one binary16 store of an fp32-grade value as well)
    A("y2_16[:7w]", taps["y2_16"][:, :, :7 * w], y)
    y = both(fo.conv3, sd, L, taps["y2_16"])
    if half:
        A("y3_16", taps["y3_16"], y)
        s = summed("conv3", y)
        Bc("se_s", taps["se_s"], (fo.se_gate(sd, L, s[0], F64), fo.se_gate(sd, L, s[1], F32)))
        y = both(fo.se_residual, x16, taps["y3_16"], taps["se_s"])
        A("cat16[%d]" % L, taps["cat16"][:, :, L * C:(L + 1) * C], y)
    else:
        Bc("y3", taps["y3"], y)
        Bc("se_s", taps["se_s"], both(fo.se_gate, sd, L, taps["y3"]))
        x = taps["out1"] if L == 0 else taps["cat"][:, :, (L - 1) * C:L * C]
        y = both(fo.se_residual, x, taps["y3"], taps["se_s"])
        Bc("cat[%d]" % L, taps["cat"][:, :, L * C:(L + 1) * C], y)
        same_bits("cat16", "cat")
    if not full:
        return
    y = both(fo.catconv, sd, taps["cat16"])
    if half:
        A("h16", taps["h16"], y)
    else:
        Bc("h", taps["h"], y)
        same_bits("h16", "h")
    if glob:
        if half:
            s = summed("catconv", y)
            st = (fo.context_stats(s[0], taps["h16"], F64), fo.context_stats(s[1], taps["h16"], F32))
        else:
            st = (fo.context_stats(taps["h"], taps["h"], F64), fo.context_stats(taps["h"], taps["h"], F32))
        Bc("stats", taps["stats"], st)
        Bc("bias_img", taps["bias_img"], both(fo.bias_img, sd, taps["stats"]))
    y = both(fo.linear1, sd, taps["h16"], taps["bias_img"] if glob else None)
    Bc("att", taps["att"], y)
    A("att16", taps["att16"], y)
    same_bits("att16", "att")
    Bc("pooled", taps["pooled"], both(fo.pooling, sd, taps["att16"], taps["h16"] if half else taps["h"]))
    Bc("emb", taps["emb"], both(fo.head, sd, taps["pooled"]))


# ------------------------------------------------------------------- a CPU stand-in for the device (float32 launches)
def simulate(sd, name, feats, dt=F32, half=True):
    """The launches chained as ecapa_model.hip chains them, each evaluated by the oracle in `dt` and stored with the
    device's rounding: name -> tap, for a full forward (block internals: layer4's)."""
    glob = "GLOB" in name
    f = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)          # an fp32 store
    t = {"col16": fo.im2col(feats, (5 * feats.shape[-1] + 63) // 64 * 64)}
    t["out1"] = f(fo.layer1(sd, feats, dt))
    t["out1_16"] = rnd16(t["out1"])
    C = t["out1"].shape[-1]
    w = C // 8
    t["cat"] = np.zeros(t["out1"].shape[:2] + (3 * C,))
    t["cat16"] = np.zeros_like(t["cat"])
    for L in range(3):
        x16 = t["out1_16"] if L == 0 else t["cat16"][:, :, (L - 1) * C:L * C]
        x = t["out1"] if L == 0 else t["cat"][:, :, (L - 1) * C:L * C]
        t["y1"] = f(fo.conv1(sd, L, x16, dt))
        t["y2_16"] = rnd16(np.concatenate([fo.res2(sd, L, t["y1"], dt), t["y1"][:, :, 7 * w:]], axis=2))
        t["y3"] = f(fo.conv3(sd, L, t["y2_16"], dt))
        t["y3_16"] = rnd16(t["y3"])
        t["se_s"] = f(fo.se_gate(sd, L, t["y3"], dt))
        if half:
            t["cat16"][:, :, L * C:(L + 1) * C] = rnd16(f(fo.se_residual(x16, t["y3_16"], t["se_s"], dt)))
        else:
            t["cat"][:, :, L * C:(L + 1) * C] = f(fo.se_residual(x, t["y3"], t["se_s"], dt))
            t["cat16"][:, :, L * C:(L + 1) * C] = rnd16(t["cat"][:, :, L * C:(L + 1) * C])
    t["h"] = f(fo.catconv(sd, t["cat16"], dt))
    t["h16"] = rnd16(t["h"])
    if glob:
        t["stats"] = f(fo.context_stats(t["h"], t["h16"] if half else t["h"], dt))
        t["bias_img"] = f(fo.bias_img(sd, t["stats"], dt))
    t["att"] = f(fo.linear1(sd, t["h16"], t["bias_img"] if glob else None, dt))
    t["att16"] = rnd16(t["att"])
    t["pooled"] = f(fo.pooling(sd, t["att16"], t["h16"] if half else t["h"], dt))
    t["emb"] = f(fo.head(sd, t["pooled"], dt))
    return t


@functools.lru_cache(maxsize=None)
def _cpu_case():
    name = "ECAPA_TDNN_GLOB_c512"
    feats = _fixture_feats()[:2]
    return name, feats, simulate(_sd(name), name, feats)


def test_the_float32_evaluation_passes_every_check():
    """The harness on the CPU: the launches evaluated in float32 and stored as the device stores them pass A and B at
    every tap, in the all-binary16 form (T = 198) and in the T < 64 form (fp32 tensors beside their copies)."""
    name, feats, taps = _cpu_case()
    rows, checks = [], []
    verify(_sd(name), name, taps, feats, rows, checks, "")
    short = feats[:, :57]
    verify(_sd(name), name, simulate(_sd(name), name, short, half=False), short, rows, checks, "T57 ", half=False)
    _assert_all("float32 evaluation", checks, rows)
    # and the whole simulated network meets the embedding bars the GPU back-end is held to
    ref = oracle_taps(_sd(name), feats, F64)["emb"]
    assert _emb_errors(taps["emb"], ref)[0] < COS_TOL and _emb_errors(taps["emb"], ref)[1] < F16_REL_TOL


def _emb_errors(e, ref):
    cos = np.sum(e * ref, 1) / (np.linalg.norm(e, axis=1) * np.linalg.norm(ref, axis=1))
    return float((1.0 - cos).max()), float((np.linalg.norm(e - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())


def test_check_a_has_teeth_where_the_embedding_bars_have_none():
    """CPU.  h16 as the float64 launch oracle gives it (from a binary16 cat16), corrupted three ways that each leave the
    embedding inside COS_TOL and F16_REL_TOL and must each fail check A:
      one 64 x 64 tile off by two binary16 ulps (a dropped K-tile's worth of error, a stale tile);
      one channel rounded by truncation instead of to nearest even;
      one channel finished with the neighbouring channel's additive constant.  catconv has no BN: its per-channel
      constant is the bias, so that is what is swapped here; the BN-shift form of the same bug is applied to out1_16
      (layer 1: conv -> ReLU -> BN), which must fail A as well."""
    name, feats, taps = _cpu_case()
    sd = _sd(name)
    emb64 = oracle_taps(sd, feats, F64)["emb"]
    y64, y32 = fo.catconv(sd, taps["cat16"], F64), fo.catconv(sd, taps["cat16"], F32)
    good = rnd16(y64)
    rows = []
    assert fo.check_a("h16 oracle", good, y64, y32, rows)[0] and fo.check_a("h16 float32", rnd16(y32), y64, y32, rows)[0]
    resume = lambda h: oecapa.ecapa_resume(sd, F64, h=torch.from_numpy(h).permute(0, 2, 1)).numpy()
    e_good = _emb_errors(resume(good), emb64)
    assert e_good[0] < COS_TOL and e_good[1] < F16_REL_TOL, e_good

    def refused(tag, bad):
        ok, ratio = fo.check_a(tag, bad, y64, y32, rows)
        e = _emb_errors(resume(bad), emb64)
        rows.append("%-12s embedding: 1 - cos %.2e  rel %.2e (bars %g / %g)" % (tag, e[0], e[1], COS_TOL, F16_REL_TOL))
        assert not ok, "\n".join(rows)
        assert e[0] < COS_TOL and e[1] < F16_REL_TOL and e != e_good, "\n".join(rows)

    h16 = good.astype(np.float16)
    two_ulps = np.nextafter(np.nextafter(h16, np.float16(np.inf)), np.float16(np.inf)).astype(np.float64)
    bad = good.copy()
    bad[0, 64:128, 640:704] = two_ulps[0, 64:128, 640:704]
    refused("tile +2ulp", bad)

    # the busiest channel (h is a ReLU output: a channel that is mostly zero has little to round)
    c = int(np.argmax((good > 0).sum(axis=(0, 1))))
    trunc = np.where(np.abs(good) > np.abs(y64), np.nextafter(h16, np.float16(0)).astype(np.float64), good)
    bad = good.copy()
    bad[:, :, c] = trunc[:, :, c]
    refused("truncated ch", bad)

    bias = fo._np(sd, "conv.bias")
    bad = good.copy()
    bad[:, :, c] = rnd16(np.maximum(y64[:, :, c] - bias[c] + bias[c + 1], 0.0))
    refused("neighbour b", bad)

    o64, o32 = fo.layer1(sd, feats, F64), fo.layer1(sd, feats, F32)
    sh = fo._post(sd, "layer1.bn")[1]
    bad = rnd16(o64)
    bad[:, :, 7] = rnd16(o64[:, :, 7] - sh[7] + sh[8])
    assert fo.check_a("out1_16 oracle", rnd16(o64), o64, o32, rows)[0]
    assert not fo.check_a("out1 BN shift", bad, o64, o32, rows)[0], "\n".join(rows)
    print("\n".join(rows))


# ------------------------------------------------------------------------------------------------------- GPU side
F16_TAPS = ("col16", "out1_16", "cat16", "y2_16", "y1", "se_s")
TAIL_TAPS = ("h16", "att", "att16", "pooled")
FP32_TAPS = ("out1", "cat", "y3", "h")            # T < 64 only


def _device_taps(model, B, T, name, full=True, half=True, sel=None):
    """name -> float64 array, (B, T, cols) for the frame-level taps; sel: only these utterances (picked on the device)."""
    names = list(F16_TAPS) + (["y3_16"] if half else list(FP32_TAPS[:3]))
    if full:
        names += list(TAIL_TAPS) + ([] if half else ["h"]) + (["stats", "bias_img"] if "GLOB" in name else [])
    out = {}
    for t in names:
        v = model.tap(t)
        v = v.reshape(B, T, -1) if v.shape[0] == B * T else v
        out[t] = (v if sel is None else v[sel]).cpu().numpy().astype(np.float64)
    return out


def _cut(taps, sel, T=None):
    """The utterances `sel` (a list), frame-level taps cut to T own rows."""
    return {k: (v[sel][:, :T] if v.ndim == 3 else v[sel]) for k, v in taps.items()}


def _run(model, feats, lens=None):
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    dispatch_log(True, clear=True)
    try:
        x = torch.from_numpy(np.ascontiguousarray(feats))
        emb = (model.embed_ragged(x, lens) if lens is not None else model(x)[-1]).cpu().numpy().astype(np.float64)
        return emb, dispatch_report()
    finally:
        dispatch_log(False, clear=True)


def _has(lines, *parts):
    return [l for l in lines if all(p in l for p in parts)]


@pytest.mark.gpu
@pytest.mark.parametrize("T", [198, 64, 57, 5])
@pytest.mark.parametrize("name", ["ECAPA_TDNN_GLOB_c512", "ECAPA_TDNN_c512", "ECAPA_TDNN_GLOB_c1024"])
def test_every_launch_small_uniform_batch(name, T):
    """B = 3 fixture utterances.  T = 198 and 64: the all-binary16 chain (gemm_f16_dma_kernel<64,64,64>, SE + residual
    in se_fc_scale_residual_f16, context std from h16, the pool_h16 epilogue); T = 57 and 5: the fp32 tensors beside
    their copies.  T = 198 also reads blocks 1 and 2 through the stop points."""
    sd, C = _sd(name), 1024 if "c1024" in name else 512
    half = T >= 64
    feats = _fixture_feats()[:, :T].copy()
    model = _engine(name).set_precision("f16")
    rows, checks = [], []
    try:
        emb, lines = _run(model, feats)
        taps = _device_taps(model, 3, T, name, half=half)
        taps["emb"] = emb
        # the kernel forms: binary16 operands on every 1x1 layer, the im2col'd layer 1, fp32 small-M GEMMs for the M = B layers
        assert _has(lines, "N=%d K=448 k=1x1" % C, "A=f16", "out=f16" if half else "out=f32f16", "gemm_f16_dma_kernel<64,64,64,2>"), lines
        assert _has(lines, "N=1536 K=%d " % (3 * C), "A=f16", "out=f16" if half else "out=f32f16", "gemm_f16_dma_kernel"), lines
        assert _has(lines, "N=192 K=3072", "small_m_gemm_f32_kernel"), lines
        if half:
            assert _has(lines, "N=%d K=%d " % (C, C), "out=f16 +colsum", "gemm_f16_dma_kernel") and _has(lines, "+pool"), lines
        verify(sd, name, taps, feats, rows, checks, "", half=half)
        if T == 198:
            for n in (1, 2, 3):
                with model.stopped_after(n):
                    z = model(torch.from_numpy(feats))[-1]
                    assert not z.any()
                    st = _device_taps(model, 3, T, name, full=False)
                    with pytest.raises(Exception, match="stopped"):
                        model.tap("h16")
                verify(sd, name, st, feats, rows, checks, "stop%d " % n, L=n - 1, full=False)
            # the stop point is gone: the same bits as before it
            assert np.array_equal(model(torch.from_numpy(feats))[-1].cpu().numpy(), emb.astype(np.float32))
    finally:
        model.stop_after(-1)
        model.set_precision("fp32")
    _assert_all("%s f16 T=%d" % (name, T), checks, rows)


def _p8_rows(lines, *parts):
    """Rows the 256 x 256 kernel took of the layer whose dispatch line has `parts` (0: it did not run)."""
    got = [int(re.match(r"rows=(\d+) ", l).group(1)) for l in _has(lines, "gemm_f16_p8_kernel<256,256>", *parts)]
    return max(got) if got else 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,wide_only", [(64, True), (168, False)])
def test_every_launch_on_the_256x256_tile_forms(B, wide_only):
    """GLOB_c512, T = 198.  B = 64 (12 672 rows): catconv (N = 1536: 50 x 6 tiles >= 256 CUs) runs on gemm_f16_p8_kernel
    with the binary16 epilogue and its remainder re-enters the 128 / 64 forms; B = 168 (33 264 rows): the N = 512 layers
    as well (130 x 2 tiles).  There the column sums behind se_s / stats come from the STORED binary16 values.  Spot
    utterances: first, last, one straddling a 256-row tile boundary, one straddling the main / remainder boundary, one
    inside the remainder / the last partial tile."""
    name, T = "ECAPA_TDNN_GLOB_c512", 198
    sd = _sd(name)
    feats = np.random.RandomState(B).randn(B, T, 80).astype(np.float32)
    model = _engine(name, max_batch=168, max_frames=T).set_precision("f16")
    try:
        emb, lines = _run(model, feats)
    except BaseException:
        model.set_precision("fp32")
        raise
    M = B * T
    main_cat = _p8_rows(lines, "N=1536 K=1536", "+colsum", "epi16")
    main_c3 = _p8_rows(lines, "N=512 K=512", "out=f16 +colsum", "epi16")
    print("\n".join(lines))
    assert main_cat > 0 and main_cat % 256 == 0, lines
    if main_cat < M:           # the remainder re-enters the 128 / 64-row forms
        assert _has(lines, "rows=%d N=1536 K=1536" % (M - main_cat), "gemm_f16_dma_kernel"), lines
    assert (main_c3 == 0) == wide_only, lines
    if not wide_only:
        assert _p8_rows(lines, "N=512 K=448", "epi16") > 0 and _p8_rows(lines, "N=512 K=512", "out=f32") > 0, lines
    spots = {0, B - 1, 256 // T, (M - 1) // 256 * 256 // T}      # first, last, across the first tile boundary, the last partial tile
    for main in (main_cat, main_c3):
        if 0 < main < M:
            spots |= {main // T, min(B - 1, main // T + 1)}       # across the main / remainder boundary, inside the remainder
    spots = sorted(spots)
    try:
        taps = _device_taps(model, B, T, name, sel=spots)
    finally:
        model.set_precision("fp32")
    taps["emb"] = emb[spots]
    m = np.arange(M).reshape(B, T)
    summed16 = {"catconv": (m < main_cat)[spots], "conv3": (m < main_c3)[spots]}
    rows, checks = [], []
    verify(sd, name, taps, feats[spots], rows, checks, "", summed16=summed16)
    _assert_all("256x256 forms B=%d, utterances %s" % (B, spots), checks, rows)


@pytest.mark.gpu
def test_every_launch_ragged_batch_and_its_zero_padding_rows():
    """GLOB_c512, six utterances in 160-row slots, NaN in the feature padding: the rows of each utterance pass A and B
    against its own inputs (utterance-level taps divided by lens[b]); every padding row of out1_16, cat16, h16 and y3_16
    is exactly zero (the column sums rest on those zeros)."""
    name, TS = "ECAPA_TDNN_GLOB_c512", 160
    sd, B = _sd(name), len(RAGGED_LENS)
    rng = np.random.RandomState(160)
    utts = [rng.randn(L, 80).astype(np.float32) for L in RAGGED_LENS]
    pad = np.full((B, TS, 80), np.nan, dtype=np.float32)
    for b, u in enumerate(utts):
        pad[b, :len(u)] = u
    model = _engine(name).set_precision("f16")
    try:
        emb, lines = _run(model, pad, RAGGED_LENS)
        taps = _device_taps(model, B, TS, name)
    finally:
        model.set_precision("fp32")
    taps["emb"] = emb
    assert np.isfinite(emb).all()
    assert _has(lines, "N=1536 K=1536", "+colsum", "+mask"), lines
    rows, checks = [], []
    for b, u in enumerate(utts):
        L = len(u)
        verify(sd, name, _cut(taps, [b], L), u[None], rows, checks, "[%d] " % b)
        for t in ("out1_16", "cat16", "h16", "y3_16"):
            tail = taps[t][b, L:]
            assert tail.size == (TS - L) * taps[t].shape[2]
            assert not tail.any(), "%s: %d non-zero values in the padding rows of utterance %d (len %d)" % (
                t, int(np.count_nonzero(tail)), b, L)
    _assert_all("ragged f16", checks, rows)
