"""Per-layer CAM++ parity: what every stage of the forward leaves in the engine's workspace (ws_debug_engine_stop_after,
stages 0 .. 9, + ws_debug_engine_tap) against the float64 oracle, tensor by tensor and dense layer by dense layer.

tests/test_gpu_parity.py judges CAM++ by the embedding alone, at REL_TOL = 2e-4 -- 100x or more what a faithful fp32
forward needs (fp32 oracle vs float64 oracle: <= 1.6e-6 at every tensor of the model) -- behind up to 52 dense layers,
three transits, a TSTP over every frame and a K = 1024 linear.  A second context segment of 28 frames divided by 29 in
ONE dense layer moves the embedding by ~1e-4 and passes that bar (test_the_per_layer_bound_has_teeth).  The FCM head
rotates three buffers and the trunk ping-pongs two, so the engine is told to return after a stage and the taps read what
its launches left:

    stop   0 stem | 1 .. 4 FCM residual blocks | 5 head.conv2 | 6 TDNN | 7 / 8 / 9 dense block 1 / 2 / 3 + its transit
    taps   stem, block / mid / sc (the last executed FCM block), fcm, tdnn, dense (the block's whole buffer, judged PER
           LAYER: the input columns, then each 32-column slice), transit, h / mask (the LAST layer's bottleneck output
           and context mask, only where the three-launch path ran), pooled; the embedding
    reference   oracle.campplus.campplus_forward(dtype=torch.float64, return_intermediates=True)
    metric      tests/test_gpu_layers.py: scaled max error and relative L2 (tap_errors)
    bound       k x the same metric of the fp32 CPU oracle against the float64 oracle, same inputs, same tensor, oracle
                error floored at 2^-24 (tap_check)
    k           8 for every tap kind, fp32 and f16x3: the rationale of tests/test_gpu_layers.py (two fp32 summation
                orders, each about as far from the truth as the other; the device's own expf in the sigmoid; f16x3's
                2^-21 product errors average out under the fp32 accumulation) -- but 64 for the f16x3 mask, where
                that averaging does not happen (the reason stands at K below).  The CPU teeth test keeps the k's from
                drifting up: its divisor fault is at 2 774 x the oracle's error in the layer and 13 367 x in the mask.

Paths (campplus_model.hip): fp32 with T' = (T - 1) / 2 + 1 <= 128 runs a whole dense block in one launch of
cam_dense_block_kernel, seven template variants by T' (NB = 1 .. 4 row blocks, with or without the 4-row tail); f16x3 at
every length and fp32 above T' = 128 run three launches per layer (1x1 GEMM with BN-ReLU on A, cam_context_kernel or --
one segment, T' >= 64 -- cam_context_from_colsum_kernel, dilated k3 GEMM with the per-segment mask in its epilogue).
cam_dense_layer_kernel, the ONE-layer launch, is out of scope: it is unreachable from the shipped model (the block
launch takes every case it would) and no switch is added to force it.

Every test prints its table (run with -s).

Measured on MI355X -- worst ratio = device error / fp32-oracle error (worst of the two metrics) per tap kind and back-end
over every case of this file, with the case that gave it (oracle32 / device: error against the float64 oracle there):

    back-end  tap       worst   case                                               oracle32   device
    fp32      stem      0.95    T=63                                               1.3e-07    1.3e-07
              block     2.11    ragged 603-frame slots, FCM block 2, utt 5         2.1e-07    4.4e-07
              mid       3.15    T=200, FCM block 1                                 3.0e-07    9.4e-07
              sc        1.53    T=130, FCM block 3                                 3.2e-07    5.0e-07
              fcm       1.62    T=5                                                3.9e-07    6.3e-07
              tdnn      3.37    T=5                                                3.7e-07    1.3e-06
              dense     3.37    T=5, block 1's input columns (= tdnn)              3.7e-07    1.3e-06
              transit   2.60    T=63, transit 3                                    8.6e-07    2.3e-06
              h         1.91    T=603, block 3 layer 16                            8.3e-07    1.6e-06
              mask      1.93    ragged 603-frame slots, block 1 layer 12, utt 5    8.0e-07    1.5e-06
              pooled    2.06    T=5                                                5.4e-07    1.1e-06
              emb       1.89    T=5                                                6.6e-07    1.2e-06
    f16x3     stem      0.84    T=57                                               1.5e-07    1.2e-07
              block     2.37    ragged, FCM block 3, utt 3                         2.4e-07    5.7e-07
              mid       2.33    T=202, FCM block 4                                 3.1e-07    7.2e-07
              sc        2.52    ragged, FCM block 3, utt 3                         2.5e-07    6.3e-07
              fcm       1.97    ragged, utt 5                                      3.3e-07    6.5e-07
              tdnn      2.92    ragged, utt 2                                      5.7e-07    1.7e-06
              dense     4.29    T=128, block 1 layer 11                            7.1e-07    3.1e-06
              transit   2.72    T=198, transit 2                                   6.7e-07    1.8e-06
              h         3.06    T=57, block 2 layer 24                             6.5e-07    2.0e-06
              mask      8.06    ragged, block 1 layer 12, utt 4 (57 frames)        3.5e-07    2.8e-06
              pooled    3.95    ragged, utt 3                                      2.3e-07    8.9e-07
              emb       2.75    T=198                                              4.5e-07    1.2e-06
Every dense layer of every case stays below 4.3 (the fused block kernel, all seven variants: below 3.4), and so do the
large-batch kernels (B = 327: below 2.1).  One tap kind needed more than k = 8: the f16x3 mask, 8.06 in one case and
3.3 .. 4.0 elsewhere -- arithmetic, not a fault (the device's error is the same 2.5 .. 3.2e-6 in every case; the reason
and the new k stand at K below).  No kernel had to be changed.  DESIGN.md 4.2.16 carries the same table.
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

from fixtures import synth  # noqa: E402
from oracle import campplus as ocam  # noqa: E402
from test_gpu_layers import ERR_FLOOR, REL_TOL, _assert_all, _fixture_feats, tap_check, tap_errors  # noqa: E402,F401

KINDS = ("stem", "block", "mid", "sc", "fcm", "tdnn", "dense", "transit", "h", "mask", "pooled", "emb")
K = {p: {t: 8.0 for t in KINDS} for p in ("fp32", "f16x3")}
# f16x3, mask: 64 = 8 x 8, the allowance of the number format itself (products of operands cut to 22 significant bits,
# ~2^-21, where fp32 rounds at 2^-24; tests/test_gpu_layers.py).  Everywhere else the back-end is held to 8 because its
# product errors are independent and average out under the fp32 accumulation.  The mask is the one tensor where that
# argument fails: it is a function of TIME MEANS of the bottleneck output.  The fp32 oracle's rounding errors are
# independent from frame to frame and shrink like 1 / sqrt(T') in the mean; the error of a weight cut to 22 bits is the
# same in every frame and does not.  Measured, the device's f16x3 mask error is the same everywhere -- 2.5 .. 3.2e-6
# scaled max, 0.8 .. 1.1e-6 L2, uniform or ragged, T' = 29 .. 302, both context kernels (fp32 back-end: <= 1.5e-6) --
# while the yardstick, the fp32 oracle's max error over the 32 values of a batch-1 mask, swings from 3.5e-7 to 1.1e-6:
# ratios 3.3 .. 4.0, and 8.06 where the oracle was luckiest (ragged, the 57-frame utterance, block 1).  A fault in the
# context path is not an error of that size: the divisor fault of the teeth test moves the mask by > 1000 x the oracle's
# error and is refused at 64 as well (asserted there).
K["f16x3"]["mask"] = 64.0
N_LAYERS = tuple(n for n, _ in ocam.BLOCKS)        # (12, 24, 16)
CIN = (128, 256, 512)                             # a dense block's input columns (the TDNN / previous transit output)
LDX = (512, 1024, 1024)                           # its buffer's columns
FULL = -1
STOPS = tuple(range(10)) + (FULL,)


def _kind(key):
    """Oracle key -> the tap kind whose k applies."""
    if key.startswith("res"):
        return key.split(".")[1] if "." in key else "block"
    if key.startswith("b"):
        return key.split(".")[2] if key.count(".") == 2 else "dense"
    return re.sub(r"\d+$", "", key)


def _tp(T):
    return (T - 1) // 2 + 1


def _segs(Tp):
    return (Tp + 99) // 100


# ---------------------------------------------------------------------------------------------- the oracle side (CPU)
@functools.lru_cache(maxsize=None)
def _sd():
    return synth.synth_campplus_state_dict(80, 512, seed=42)


def oracle_taps(feats, dtype):
    """key -> numpy array in the engine's layout.  FCM maps (B, F, T, 32): stem, res<i>, res<i>.mid, res<i>.sc, fcm.
    Trunk (B, T', cols): tdnn, b<k>.in (the block's input columns), b<k>.l<j>, b<k>.l<j>.h, transit<k>.  b<k>.l<j>.mask
    (B, segments, 32), pooled (B, 1024), emb."""
    emb, mid = ocam.campplus_forward(_sd(), np.array(feats), dtype=dtype, return_intermediates=True)
    out = {"emb": emb.numpy(), "pooled": mid["pooled"].numpy()}
    for key, v in mid.items():
        if v.dim() == 4:
            out[key] = v.permute(0, 2, 3, 1).contiguous().numpy()
        elif v.dim() == 3:
            out[key] = v.permute(0, 2, 1).contiguous().numpy()
    for k in range(3):
        out["b%d.in" % (k + 1)] = out["tdnn" if k == 0 else "transit%d" % k]
    return out


def _feats(T, B=3):
    """The fixture utterances cut to T frames; random features beyond their 198 frames."""
    if T <= _fixture_feats().shape[1]:
        return _fixture_feats()[:B, :T]
    f = np.random.RandomState(T).randn(B, T, 80).astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=2)
def _refs(T, B=3):
    """(float64 taps, fp32 taps) at T frames; computed once, shared by the precisions of a case."""
    return oracle_taps(_feats(T, B), torch.float64), oracle_taps(_feats(T, B), torch.float32)


def _block_keys(k):
    """Oracle keys of dense block k's (1-based) buffer, in column order."""
    return ["b%d.in" % k] + ["b%d.l%d" % (k, j + 1) for j in range(N_LAYERS[k - 1])]


def keys_at(n, generic):
    """The oracle keys that the taps hold when the forward is stopped at n (FULL: not stopped)."""
    if n == 0:
        return ["stem"]
    if 1 <= n <= 4:
        return ["res%d" % n, "res%d.mid" % n] + (["res%d.sc" % n] if n in (1, 3) else [])
    if n == 5:
        return ["fcm", "res4"]
    if n == 6:
        return ["tdnn", "fcm"]
    k = 3 if n == FULL else n - 6
    keys = _block_keys(k) + ["transit%d" % k]
    if generic:
        keys += ["b%d.l%d.h" % (k, N_LAYERS[k - 1]), "b%d.l%d.mask" % (k, N_LAYERS[k - 1])]
    if n == 7:
        keys.append("tdnn")
    if n == FULL:
        keys += ["pooled", "fcm", "res4"]
    return keys


def test_the_per_layer_bound_has_teeth():
    """Why this file exists (CPU): faults that the embedding bar lets through must fail the per-layer bound.  Fed to the
    very comparison the GPU tests use:
      1. T = 256 (T' = 128: a second context segment of 28 frames): that segment's mean divided by 29 instead of 28 in
         block2.tdnnd5 only -- an off-by-one in a partial segment's divisor;
      2. T = 198 (T' = 99): rows 96 .. 98, the 4-row tail of the NB = 3 + tail variant, of one layer's 32 channels
         (block1.tdnnd7) scaled by 1 + 1e-4.
    Both leave the embedding inside REL_TOL (oracle.campplus.campplus_resume, the forward's own tail, in float64) and
    both are refused at the k in force.  Both oracles themselves pass every tensor, and the fp32 oracle is below 2e-6
    of the float64 one at every tensor, so the k's cannot drift."""
    sd64 = ocam._cast(_sd(), torch.float64)
    k = K["fp32"]
    rows = []
    cf = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 2, 1)          # back to channels first

    def both_oracles_pass(r64, r32):
        for t in r64:
            assert tap_check(t, r64[t], r64[t], r32[t], k[_kind(t)])[0]
            assert tap_check(t, r32[t], r64[t], r32[t], k[_kind(t)], rows)[0], rows[-1]
            assert max(tap_errors(r32[t], r64[t])) < 2e-6, rows[-1]

    rel = lambda e, ref: float((np.linalg.norm(e - ref, axis=1) / np.linalg.norm(ref, axis=1)).max())

    # 1. the divisor fault
    r64, r32 = _refs(256, 2)
    both_oracles_pass(r64, r32)
    buf = torch.cat([cf(r64[key]) for key in _block_keys(2)[:5]], dim=1)             # transit1 | layers 1 .. 4
    assert buf.shape[1:] == (256 + 4 * 32, 128)

    def seg_mean_29(x):
        seg = ocam._seg_pooling(x).clone()
        seg[..., 100:] *= 28.0 / 29.0
        return seg

    with torch.no_grad():
        good = ocam._dense_layer(sd64, 1, 4, buf)
        bad = ocam._dense_layer(sd64, 1, 4, buf, seg_pooling=seg_mean_29)
    cl = lambda t: t.permute(0, 2, 1).contiguous().numpy()
    assert np.allclose(cl(good), r64["b2.l5"], rtol=1e-12, atol=0)
    ok, ratio = tap_check("b2.l5 /29", cl(bad), r64["b2.l5"], r32["b2.l5"], k["dense"], rows)
    assert not ok and ratio > k["dense"], rows
    # ... and the layer's mask itself, at the k of either back-end
    taps = {}
    with torch.no_grad():
        ocam._dense_layer(sd64, 1, 4, buf, taps, seg_pooling=seg_mean_29)
    ok, ratio = tap_check("b2.l5.mask /29", cl(taps["mask"]), r64["b2.l5.mask"], r32["b2.l5.mask"], k["mask"], rows)
    assert not ok and ratio > max(K["fp32"]["mask"], K["f16x3"]["mask"]), rows
    e_bad = ocam.campplus_resume(_sd(), torch.cat([buf, bad], dim=1), 2, 5, torch.float64).numpy()
    assert 0.0 < rel(e_bad, r64["emb"]) < REL_TOL, rel(e_bad, r64["emb"])
    # campplus_resume is the forward's own tail: unperturbed it returns the embedding
    e_same = ocam.campplus_resume(_sd(), torch.cat([buf, good], dim=1), 2, 5, torch.float64).numpy()
    assert rel(e_same, r64["emb"]) < 1e-12
    assert rel(ocam.campplus_resume(_sd(), cf(r64["tdnn"]), 1, 0, torch.float64).numpy(), r64["emb"]) < 1e-12

    # 2. the tail rows
    r64, r32 = _refs(198, 2)
    both_oracles_pass(r64, r32)
    assert r64["b1.l7"].shape == (2, 99, 32)
    bad = r64["b1.l7"].copy()
    bad[:, 96:99] *= 1.0 + 1e-4
    ok, ratio = tap_check("b1.l7 tail", bad, r64["b1.l7"], r32["b1.l7"], k["dense"], rows)
    assert not ok and ratio > k["dense"], rows
    buf = torch.cat([cf(r64[key]) for key in _block_keys(1)[:7]] + [cf(bad)], dim=1)
    e_bad = ocam.campplus_resume(_sd(), buf, 1, 7, torch.float64).numpy()
    assert 0.0 < rel(e_bad, r64["emb"]) < REL_TOL, rel(e_bad, r64["emb"])
    print("\n".join(rows))


# ------------------------------------------------------------------------------------------------------- GPU side
_ENGINES = {}


def _engine(max_batch=8, max_frames=608):
    from wespeaker_amd.engine import NativeSpeakerModel
    key = (max_batch, max_frames)
    if key not in _ENGINES:
        _ENGINES[key] = NativeSpeakerModel("CAMPPlus", _sd(), feat_dim=80, embed_dim=512, max_batch=max_batch,
                                           max_frames=max_frames)
    return _ENGINES[key]


def _run(model, feats, n, lens=None):
    """One forward stopped at n (FULL: the full forward) -> embeddings (numpy) and the dispatch log's lines."""
    from wespeaker_amd.engine import dispatch_log, dispatch_report
    x = torch.from_numpy(np.array(feats))
    dispatch_log(True, clear=True)
    try:
        with model.stopped_after(n):
            out = model.embed_ragged(x, lens) if lens is not None else model.embed(x)
        lines = dispatch_report()
    finally:
        dispatch_log(False, clear=True)
    if n >= 0:
        assert not out.any(), "a stopped forward must return zeros"
    return out, lines


def device_taps(model, n, B, T, generic, spots=None):
    """oracle key -> the device's tensor (numpy, slot layout (B, ...)) for every key of keys_at(n); `spots`: those
    utterances only, sliced on the device before the host copy."""
    Tp = _tp(T)
    cache = {}

    def rd(tap, shape):
        if tap not in cache:
            v = model.tap(tap)
            assert v.numel() == B * int(np.prod(shape)), (tap, tuple(v.shape), B, shape)
            v = v.reshape((B,) + tuple(shape))
            cache[tap] = (v[torch.as_tensor(spots, device=v.device)] if spots is not None else v).cpu().numpy()
        return cache[tap]

    out = {}
    for key in keys_at(n, generic):
        kind = _kind(key)
        if key.startswith("res"):
            out[key] = rd(kind, (40 if key[3] in "12" else 20, T, 32))
        elif key == "stem":
            out[key] = rd("stem", (80, T, 32))
        elif key == "fcm":
            out[key] = rd("fcm", (10, T, 32))
        elif key == "tdnn":
            out[key] = rd("tdnn", (Tp, 128))
        elif key.startswith("transit"):
            out[key] = rd("transit", (Tp, CIN[int(key[-1]) - 1] // 2 + 16 * N_LAYERS[int(key[-1]) - 1]))
        elif key == "pooled":
            out[key] = rd("pooled", (1024,))
        elif kind == "h":
            out[key] = rd("h", (Tp, 128))
        elif kind == "mask":
            out[key] = rd("mask", (_segs(Tp), 32))
        else:                                          # a column slice of the dense block's buffer
            k = int(key[1])
            buf = rd("dense", (Tp, LDX[k - 1]))
            if key.endswith(".in"):
                out[key] = buf[:, :, :CIN[k - 1]]
            else:
                c0 = CIN[k - 1] + 32 * (int(key.split(".l")[1]) - 1)
                out[key] = buf[:, :, c0:c0 + 32]
    return out


def _refusals(model, n, generic):
    """What does not exist at stop n is refused, with the reason."""
    from wespeaker_amd._lib import NativeError
    want = []
    if n != 0:
        want.append(("stem", "stop it at 0"))
    if n == 0:
        want += [("block", "no FCM block ran"), ("fcm", "before head.conv2")]
    if n in (2, 4):
        want.append(("sc", "FCM block %d has no shortcut" % n))
    if n >= 5 or n == FULL:
        want.append(("mid", "head.conv2 wrote over"))
    if 0 <= n <= 6:
        want += [("dense", "no dense block ran"), ("transit", "no dense block ran"), ("h", "no dense block ran")]
    if n >= 8 or n == FULL:
        want.append(("tdnn", "transit 2 wrote over"))
    if (n >= 7 or n == FULL) and not generic:
        want += [("h", "stay in LDS"), ("mask", "stay in LDS")]
    if n != FULL:
        want.append(("pooled", "pooling and the head did not run"))
    for tap, why in want:
        with pytest.raises(NativeError, match=why):
            model.tap_shape(tap)


def _uniform_case(prec, T, generic):
    """B = 3 utterances of T frames, stops 0 .. 9 and the full forward: every tensor that exists at that stop."""
    model = _engine().set_precision(prec)
    r64, r32 = _refs(T)
    feats = _feats(T)
    rows, checks = [], []
    try:
        for n in STOPS:
            emb, lines = _run(model, feats, n)
            got = device_taps(model, n, 3, T, generic)
            for key in keys_at(n, generic):
                tag = key if n != FULL else key + " (full)"
                checks.append((tag, tap_check(tag, got[key], r64[key], r32[key], K[prec][_kind(key)], rows)[0]))
            _refusals(model, n, generic)
            if n == FULL or n >= 7:
                fused = [l for l in lines if "cam_dense_block_kernel" in l]
                assert (len(fused) == (3 if n == FULL else n - 6)) if not generic else not fused, lines
                assert not any("cam_dense_layer_kernel" in l for l in lines), lines
        checks.append(("emb", tap_check("emb", emb.cpu().numpy(), r64["emb"], r32["emb"], K[prec]["emb"], rows)[0]))
    finally:
        model.set_precision("fp32")
    _assert_all("CAM++ %s T=%d (T'=%d)" % (prec, T, _tp(T)), checks, rows)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [5, 63, 66, 72, 74, 130, 198, 200, 202, 256])
def test_every_stage_fp32_fused_block_kernel(T):
    """cam_dense_block_kernel's seven variants and their edges, by T' = (T - 1) / 2 + 1: 3 the smallest length, 32 NB = 1,
    33 NB = 1 + tail, 36 a tail of 4, 37 NB = 2, 65 NB = 2 + tail, 99 NB = 3 + tail (the 2-s utterance), 100 the last
    frame of segment 0 in the tail, 101 NB = 4 with a one-frame second segment, 128 the kernel's largest.  The dispatch
    log names the kernel once per executed block; h and mask are refused (they stay in LDS)."""
    _uniform_case("fp32", T, generic=False)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [258, 603])
def test_every_stage_fp32_generic_path(T):
    """T' = 129: the first length the fused kernel refuses, cam_context_kernel in its 1024-thread form, two segments;
    T' = 302: four segments, the last of 2 frames.  h and mask of the last layer at stops 7, 8, 9."""
    _uniform_case("fp32", T, generic=True)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [57, 128, 198, 202])
def test_every_stage_f16x3(T):
    """f16x3 runs the three-launch path at every length.  T' = 29 < 64: cam_context_kernel with 256 threads; 64: the
    threshold of cam_context_from_colsum_kernel; 99: the colsum form; 101: two segments."""
    _uniform_case("f16x3", T, generic=True)


# ---- ragged batches
def _ragged_case(prec, lens, TS, generic):
    """Utterances of lens[b] frames in TS-frame slots, NaN in the feature padding.  Frames of an utterance: every
    tensor equals the batch-1 oracle of that utterance.  Beyond: the FCM maps past L0 = lens[b], the trunk rows past
    L1 = (L0 - 1) / 2 + 1 in EVERY column of the dense buffer, tdnn and transit, and the mask rows of segments the
    utterance does not have are EXACTLY zero -- the kernels promise it (row_len / lens) and every later border tap, the
    context sums and the pooling rest on it."""
    B = len(lens)
    rng = np.random.RandomState(TS)
    utts = [rng.randn(L, 80).astype(np.float32) for L in lens]
    pad = np.full((B, TS, 80), np.nan, dtype=np.float32)
    for b, u in enumerate(utts):
        pad[b, :len(u)] = u
    refs = [(oracle_taps(u[None], torch.float64), oracle_taps(u[None], torch.float32)) for u in utts]
    model = _engine().set_precision(prec)
    rows, checks = [], []
    try:
        for n in STOPS:
            emb, lines = _run(model, pad, n, lens)
            got = device_taps(model, n, B, TS, generic)
            for key in keys_at(n, generic):
                slot, kind = got[key], _kind(key)
                for b, L0 in enumerate(lens):
                    r64, r32 = refs[b]
                    if slot.ndim == 4:                                   # an FCM map (B, F, TS, 32)
                        mine, tail = slot[b:b + 1, :, :L0], slot[b, :, L0:]
                    elif kind == "mask":
                        s = _segs(_tp(L0))
                        mine, tail = slot[b:b + 1, :s], slot[b, s:]
                    elif kind == "pooled":
                        mine, tail = slot[b:b + 1], slot[b, :0]
                    else:                                                # trunk rows (B, T', cols)
                        mine, tail = slot[b:b + 1, :_tp(L0)], slot[b, _tp(L0):]
                    assert mine.shape == r64[key].shape, (key, b, mine.shape, r64[key].shape)
                    tag = "%s[%d]" % (key, b)
                    checks.append((tag, tap_check(tag, mine, r64[key], r32[key], K[prec][kind], rows)[0]))
                    if key != "stem":
                        assert not tail.any(), "%s at stop %d: %d non-zero values beyond utterance %d (len %d)" % (
                            key, n, int(np.count_nonzero(tail)), b, L0)
            if not generic and (n == FULL or n >= 7):
                assert sum("cam_dense_block_kernel" in l and "+mask" in l for l in lines) == (3 if n == FULL else n - 6), lines
        emb = emb.cpu().numpy()
        for b in range(B):
            r64, r32 = refs[b]
            checks.append(("emb[%d]" % b, tap_check("emb[%d]" % b, emb[b:b + 1], r64["emb"], r32["emb"], K[prec]["emb"], rows)[0]))
    finally:
        model.set_precision("fp32")
    _assert_all("ragged CAM++ %s %s" % (prec, lens), checks, rows)


@pytest.mark.gpu
def test_every_stage_ragged_batch_fused_block_kernel():
    """fp32, lens [256, 203, 199, 131, 64, 7] in 256-frame slots: cam_dense_block_kernel runs with `lens` (NB = 4 for the
    slot), T' = 128, 102, 100, 66, 32, 4 -- utterances with two segments, with exactly one, ending inside every row
    block."""
    _ragged_case("fp32", [256, 203, 199, 131, 64, 7], 256, generic=False)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["fp32", "f16x3"])
def test_every_stage_ragged_batch_generic_path(prec):
    """lens [603, 328, 201, 99, 57, 7] in 603-frame slots: the three-launch path, 4 / 2 / 2 / 1 / 1 / 1 segments per
    utterance, the mask rows of the missing ones zeroed."""
    _ragged_case(prec, [603, 328, 201, 99, 57, 7], 603, generic=True)


# ---- large-batch kernels (fp32): reached only above a row count; three spot utterances against the oracle
LARGE_T, LARGE_B = 200, 327


@pytest.mark.gpu
def test_large_batch_direct_conv_transit_tiles_and_tdnn_form():
    """The kernels that tests/golden/dispatch_CAMPPlus_fp32.txt names and a batch of 3 never reaches, at T = 200
    (T' = 100).  Thresholds read from the dispatcher, 2 x 256 = 512 workgroup slots on MI355X:
      * conv3x3_direct_f32_kernel (conv3x3_direct.hip: rows x 32 >= 2^22): the 40-row FCM maps from B = 17 on
        (17 x 40 x 200 = 136 000 rows) -- block 1's conv1 at stride 2x1, its conv2 with +res, block 2's conv1 without;
      * conv_gemm_kernel<128,128,pre 1x1> on a transit (conv_gemm.hip launch_prec: 128-row tiles x column tiles x 2 >=
        the slots): transit 2 / 3 (N = 512) from B = 81 on, transit 1 (N = 256) from B = 163 on;
      * the TDNN layer's k = 10x5 convolution over the never-materialised (B, C*F', T) reshape on 128 x 128 tiles:
        N = 128 is one column tile, so more than 255 x 128 = 32 640 rows: B = 327 (32 700 rows).
    B = 327 is the smallest batch that shows all of them; utterance b is base[b % 3], spots 0, 163, 326 are base[0],
    [1], [2], sliced on the device.  Stops 1, 2 (the direct kernel through block / mid / sc), 6 (tdnn), 7, 8 (dense per
    layer -- the fused block kernel at a grid of 327 -- and both transit tile shapes)."""
    B, T = LARGE_B, LARGE_T
    base = np.random.RandomState(T).randn(3, T, 80).astype(np.float32)
    idx = np.arange(B) % 3
    spots = [0, 163, 326]
    assert [int(idx[s]) for s in spots] == [0, 1, 2]
    r64, r32 = oracle_taps(base, torch.float64), oracle_taps(base, torch.float32)
    feats = base[idx]
    model = _engine(B, T)
    want = {1: [("N=32 K=288 k=3x3 s=2x1", "out=f32 ->", "conv3x3_direct_f32_kernel<2,1>"),
                ("N=32 K=288 k=3x3 s=1x1", "+res", "conv3x3_direct_f32_kernel<1,1>")],
            2: [("N=32 K=288 k=3x3 s=1x1", "out=f32 ->", "conv3x3_direct_f32_kernel<1,1>")],
            6: [("rows=32700 N=128 K=1600 k=10x5 s=1x2", "conv_gemm_kernel<128,128,conv>")],
            7: [("rows=32700 N=256 K=512 k=1x1", "+pre", "conv_gemm_kernel<128,128,pre 1x1>")],
            8: [("rows=32700 N=512 K=1024 k=1x1", "+pre", "conv_gemm_kernel<128,128,pre 1x1>")]}
    rows, checks = [], []
    try:
        for n in sorted(want):
            _, lines = _run(model, feats, n)
            print("\n".join(lines))
            for subs in want[n]:
                assert any(all(s in l for s in subs) for l in lines), (subs, lines)
            got = device_taps(model, n, B, T, False, spots)
            for key in keys_at(n, False):
                checks.append((key, tap_check(key, got[key], r64[key], r32[key], K["fp32"][_kind(key)], rows)[0]))
    finally:
        del _ENGINES[(B, T)]
    _assert_all("CAM++ B=%d T=%d" % (B, T), checks, rows)


# ---- API edges
@pytest.mark.gpu
def test_stop_and_tap_api_edges():
    from wespeaker_amd._lib import NativeError
    from wespeaker_amd.engine import NativeSpeakerModel
    model = NativeSpeakerModel("CAMPPlus", _sd(), feat_dim=80, embed_dim=512, max_batch=2, max_frames=300)
    with pytest.raises(NativeError, match="no forward"):                       # before any forward
        model.tap("dense")
    f = np.random.RandomState(5).randn(5, 66, 80).astype(np.float32)
    x = torch.from_numpy(f)
    first = model(x).clone()
    assert first.abs().max() > 0
    with pytest.raises(NativeError, match="unknown tensor 'out1'"):
        model.tap("out1")
    # stop beyond 9 / below -1, the message names the stage count; the stop point stays where it was
    with pytest.raises(NativeError, match="has 10 stop points 0 .. 9"):
        model.stop_after(10)
    with pytest.raises(NativeError, match="n = -2"):
        model.stop_after(-2)
    assert torch.equal(model(x), first)
    # 5 utterances on max_batch = 2: the tap holds the LAST chunk (utterance 4); a stopped forward returns all zeros
    with model.stopped_after(8):
        z = model(x)
        assert tuple(z.shape) == (5, 512) and not z.any()
        assert model.tap_shape("dense") == (33, 1024) and model.tap_shape("transit") == (33, 512)
        assert model.tap_shape("fcm") == (10 * 66, 32) and model.tap_shape("block") == (20 * 66, 32)
        last = model.tap("transit")
        with pytest.raises(NativeError, match="stay in LDS"):                  # the fused block kernel ran
            model.tap("h")
        with pytest.raises(NativeError, match="pooling and the head did not run"):
            model.tap("pooled")
        z1 = model(torch.from_numpy(f[4:5].copy()))
        assert not z1.any() and torch.equal(model.tap("transit"), last)
    with model.stopped_after(9):                  # transit 2, gathered above from block 3's row stride, IS its input
        model(torch.from_numpy(f[4:5].copy()))
        assert torch.equal(model.tap("dense")[:, :512], last)
    with model.stopped_after(2):
        model(x)
        with pytest.raises(NativeError, match="FCM block 2 has no shortcut"):
            model.tap("sc")
        assert model.tap_shape("mid") == (40 * 66, 32)
    # the context manager restored the full forward: same bits as before the stopped ones
    assert torch.equal(model(x), first)
    assert model.tap_shape("pooled") == (1, 1024)
    # above T' = 128 the three-launch path leaves h and mask
    g = torch.from_numpy(np.random.RandomState(6).randn(2, 258, 80).astype(np.float32))
    model(g)
    assert model.tap_shape("h") == (2 * 129, 128) and model.tap_shape("mask") == (2 * 2, 32)
    # f16 back-end: the FCM maps are binary16 only; one segment and T' >= 64 keeps h in binary16 too, the mask taps
    model.set_precision("f16")
    try:
        with model.stopped_after(0):
            model(x)
            with pytest.raises(NativeError, match="binary16"):
                model.tap("stem")
        with model.stopped_after(7):
            model(torch.from_numpy(f[:2, :57].copy()))                          # T' = 29: cam_context_kernel, fp32 h
            for t in ("block", "fcm"):
                with pytest.raises(NativeError, match="binary16"):
                    model.tap(t)
            assert model.tap_shape("h") == (2 * 29, 128) and model.tap_shape("dense") == (2 * 29, 512)
            model(torch.from_numpy(np.concatenate([f[:2], f[:2]], axis=1)))     # T = 132, T' = 66: the colsum form
            with pytest.raises(NativeError, match="binary16"):
                model.tap("h")
            assert model.tap_shape("mask") == (2, 32) and model.tap_shape("transit") == (2 * 66, 256)
        model(x)
        assert model.tap_shape("pooled") == (1, 1024)
    finally:
        model.set_precision("fp32")
    model.reserve(2, 100)                         # re-sizing the workspace forgets the last chunk
    with pytest.raises(NativeError, match="no forward"):
        model.tap("dense")
