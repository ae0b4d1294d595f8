"""The depthwise 3x3 kernel (wespeaker_amd/csrc/dwconv3x3.hip) through ws_debug_dwconv3x3, against a float64 numpy
statement of its formula

    out[b,f,t,c] = relu(sum_{df,dt in -1..1} x[b,f+df,t+dt,c] * w[c][3 (df+1) + (dt+1)] + bias[c])      (zero padding)

Bound: K_TAP = 8 x the error of the same formula evaluated in float32 (tests/test_gpu_layers.py: tap_check, oracle error
floored at 2^-24) -- the device and numpy are two fp32 evaluation orders of a 9-term sum, each about as far from the
truth as the other.  Ragged batches: bit-exact against the batch of one, exact zeros beyond row_len.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_layers import tap_check  # noqa: E402

pytestmark = pytest.mark.gpu

K_TAP = 8.0
TIME_TILE = 4             # DW_TT of dwconv3x3.hip: time steps per thread


def reference(x, w, bias, dtype, row_len=None):
    """x (B, F, T, C), w (C, 9), bias (C) -> (B, F, T, C) in `dtype`, taps accumulated in the formula's order."""
    B, F, T, C = x.shape
    x = x.astype(dtype)
    if row_len is not None:
        x = x.copy()
        for b, L in enumerate(row_len):
            x[b, :, L:] = 0
    xp = np.zeros((B, F + 2, T + 2, C), dtype=dtype)
    xp[:, 1:F + 1, 1:T + 1] = x
    w = w.astype(dtype)
    acc = np.zeros((B, F, T, C), dtype=dtype)
    for df in range(3):
        for dt in range(3):
            acc += xp[:, df:df + F, dt:dt + T] * w[:, 3 * df + dt]
    out = np.maximum(acc + bias.astype(dtype), 0)
    if row_len is not None:
        for b, L in enumerate(row_len):
            out[b, :, L:] = 0
    return out


def run(x, w, bias, row_len=None, out=None):
    from wespeaker_amd import _lib
    dev = torch.device("cuda", 0)
    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    wd, bd = torch.from_numpy(np.ascontiguousarray(w)).to(dev), torch.from_numpy(np.ascontiguousarray(bias)).to(dev)
    B, F, T, C = xd.shape
    od = torch.full((B, F, T, C), float("nan"), dtype=torch.float32, device=dev) if out is None else out
    ld = torch.tensor(list(row_len), dtype=torch.int32, device=dev) if row_len is not None else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ws_debug_dwconv3x3(_lib.ptr(xd), _lib.ptr(od), _lib.ptr(wd), _lib.ptr(bd), B, F, T, C,
                                                 _lib.ptr(ld) if ld is not None else None,
                                                 _lib.current_stream_ptr(dev)), "ws_debug_dwconv3x3")
    torch.cuda.synchronize()
    return od.cpu().numpy()


def _inputs(B, F, T, C, seed):
    rng = np.random.RandomState(seed)
    x = rng.randn(B, F, T, C).astype(np.float32)
    w = (rng.randn(C, 9) / 3.0).astype(np.float32)
    bias = (0.3 * rng.randn(C)).astype(np.float32)
    return x, w, bias


@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 1, 17, 128), (2, 2, 1, 128), (3, 5, 100, 1024), (2, 40, 57, 128),
                                   (2, 3, TIME_TILE + 1, 256), (2, 3, TIME_TILE - 1, 256), (1, 13, 2 * TIME_TILE + 1, 12)])
def test_against_the_formula(shape):
    """F = 1 / T = 1 leave one filter row / column alive; T one beyond and one short of the time tile; 13 lines = four
    whole turns of the three-line rotation and one more; (3, 5, 100, 1024) and (2, 40, 57, 128) are model shapes, the second
    cut into walks of 8 lines."""
    x, w, bias = _inputs(*shape, seed=sum(shape))
    got = run(x, w, bias)
    ok, ratio = tap_check("dw %s" % (shape,), got, reference(x, w, bias, np.float64), reference(x, w, bias, np.float32), K_TAP)
    print(shape, "ratio %.2f" % ratio)
    assert ok, (shape, ratio)
    assert (got >= 0).all()


def test_ragged_rows_equal_their_batch_of_one_bit_for_bit():
    B, F, T, C = 3, 5, 22, 128
    x, w, bias = _inputs(B, F, T, C, seed=5)
    lens = (T, 1, T // 2)
    clean = x.copy()
    for b, L in enumerate(lens):
        clean[b, :, L:] = 0
    got = run(clean, w, bias, row_len=lens)
    ok, ratio = tap_check("ragged", got, reference(x, w, bias, np.float64, lens), reference(x, w, bias, np.float32, lens), K_TAP)
    assert ok, ratio
    for b, L in enumerate(lens):
        assert (got[b, :, L:] == 0.0).all(), b                       # exact zeros beyond row_len
        assert np.abs(got[b, :, :L]).max() > 0
        one = run(np.ascontiguousarray(x[b:b + 1, :, :L]), w, bias)     # the utterance alone, at its own width
        assert np.array_equal(got[b, :, :L].view(np.uint32), one[0].view(np.uint32)), b
    # garbage (NaN, inf, large values) left in the padded columns changes nothing
    dirty = x.copy()
    for b, L in enumerate(lens):
        dirty[b, :, L:] = np.array([np.nan, np.inf, -1e30, 7.0], dtype=np.float32)[np.arange(C) % 4]
    assert np.array_equal(run(dirty, w, bias, row_len=lens).view(np.uint32), got.view(np.uint32))


def test_refusals_come_back_by_name():
    from wespeaker_amd._lib import NativeError
    x, w, bias = _inputs(1, 2, 3, 8, seed=1)
    with pytest.raises(NativeError, match="ws_debug_dwconv3x3: C must be a positive multiple of 4"):
        run(x[..., :6], w[:6], bias[:6])
    xd = torch.from_numpy(x).to("cuda:0")
    with pytest.raises(NativeError, match="ws_debug_dwconv3x3: out aliases x"):
        run(xd, w, bias, out=xd)
    both = torch.zeros(2 * xd.numel() - 8, dtype=torch.float32, device="cuda:0")        # a partial overlap
    with pytest.raises(NativeError, match="ws_debug_dwconv3x3: out aliases x"):
        run(both[:xd.numel()].view(1, 2, 3, 8), w, bias, out=both[xd.numel() - 8:].view(1, 2, 3, 8))
    with pytest.raises(NativeError, match="B, F and T must be at least 1"):
        from wespeaker_amd import _lib
        _lib.check(_lib.lib().ws_debug_dwconv3x3(_lib.ptr(xd), _lib.ptr(both), _lib.ptr(xd), _lib.ptr(xd), 1, 0, 3, 8, None,
                                                 ctypes.c_void_p(0)), "ws_debug_dwconv3x3")
