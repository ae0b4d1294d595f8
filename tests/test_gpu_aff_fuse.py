"""aff_fuse_kernel (wespeaker_amd/csrc/aff_fuse.hip) through ws_debug_aff_fuse against a float64 numpy AFF
(wespeaker/models/eres2net.py:97-103 with the 1x1 convolutions' biases and BatchNorms folded).

Bound: max |got - ref| / max |ref| <= K * the same figure of the same AFF evaluated in numpy float32 on the same data
(the yardstick is measured here, per case).  K = 8 everywhere: the kernel adds its products in another order than
numpy's float32 matmul (k permuted inside a 32-deep tile, exact-fp32 MFMA), nothing else differs.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_BOUND = 8.0


def _silu(v):
    return v / (1.0 + np.exp(-v))


def _aff_numpy(x, y, w1, b1, w2, b2, dtype):
    x, y, w1, b1, w2, b2 = (a.astype(dtype) for a in (x, y, w1, b1, w2, b2))
    h = _silu(np.concatenate([x, y], axis=1) @ w1.T + b1)
    a = dtype(1.0) + np.tanh(h @ w2.T + b2)
    return x * a + y * (dtype(2.0) - a)


@functools.lru_cache(maxsize=None)
def _weights(C, shift=0.0):
    rng = np.random.RandomState(C)
    H = C // 4
    w1 = (rng.randn(H, 2 * C) / np.sqrt(2 * C)).astype(np.float32)
    b1 = (0.1 * rng.randn(H)).astype(np.float32)
    w2 = (rng.randn(C, H) * np.sqrt(2.0 / H)).astype(np.float32)
    b2 = (0.1 * rng.randn(C)).astype(np.float32)
    if shift:
        b2 = b2 + np.where(np.arange(C) % 2 == 0, shift, -shift).astype(np.float32)
    return w1, b1, w2, b2


def _run(x, y, C, M, w, x_slice=False, y_slice=False, o_slice=False, row_len=None, HW=0, W=0):
    """x / y: (M, C) host arrays.  *_slice: the operand is columns [C, 2C) (x, out) or [0, C) (y) of a 2C-wide row whose
    other half holds a sentinel.  Returns the (M, C) output and the untouched half of out's rows (or None)."""
    from wespeaker_amd import _lib
    dev = torch.device("cuda", 0)

    def place(a, sliced, off):
        if not sliced:
            return torch.from_numpy(a).to(dev).contiguous(), C, 0
        wide = np.full((M, 2 * C), 777.0, dtype=np.float32)
        wide[:, off:off + C] = a
        return torch.from_numpy(wide).to(dev).contiguous(), 2 * C, off

    xd, ldx, xo = place(x, x_slice, C)
    yd, ldy, yo = place(y, y_slice, 0)
    od, ldo, oo = place(np.full((M, C), -555.0, dtype=np.float32), o_slice, C)
    wd = [torch.from_numpy(a).to(dev).contiguous() for a in w]
    rl = torch.from_numpy(np.asarray(row_len, dtype=np.int32)).to(dev) if row_len is not None else None
    rc = _lib.lib().ws_debug_aff_fuse(_lib.ptr(xd), ldx, xo, _lib.ptr(yd), ldy, yo, _lib.ptr(od), ldo, oo,
                                      _lib.ptr(wd[0]), _lib.ptr(wd[1]), _lib.ptr(wd[2]), _lib.ptr(wd[3]), M, C,
                                      _lib.ptr(rl) if rl is not None else None, HW, W,
                                      _lib.current_stream_ptr(dev))
    _lib.check(rc, "ws_debug_aff_fuse")
    torch.cuda.synchronize()
    o = od.cpu().numpy()
    return (o[:, oo:oo + C], o[:, :C]) if o_slice else (o, None)


def _data(C, M, seed=0):
    rng = np.random.RandomState(1000 * C + M + seed)
    return rng.randn(M, C).astype(np.float32), rng.randn(M, C).astype(np.float32)


def _check(got, x, y, w, what):
    ref = _aff_numpy(x, y, *w, dtype=np.float64)
    f32 = _aff_numpy(x, y, *w, dtype=np.float32)
    scale = np.abs(ref).max()
    err = np.abs(got.astype(np.float64) - ref).max() / scale
    yard = np.abs(f32.astype(np.float64) - ref).max() / scale
    print("%s: err %.3e yardstick %.3e ratio %.2f" % (what, err, yard, err / yard if yard else float("inf") if err else 0.0))
    assert np.isfinite(got).all(), what
    assert err <= K_BOUND * yard, (what, err, yard)


@pytest.mark.parametrize("C", [64, 96, 128, 512, 2048])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 250, 1000])
def test_full_tensors(C, M):
    x, y = _data(C, M)
    got, _ = _run(x, y, C, M, _weights(C))
    _check(got, x, y, _weights(C), "C %d M %d" % (C, M))


@pytest.mark.parametrize("C", [64, 96, 128, 512, 2048])
@pytest.mark.parametrize("M", [1, 65, 250])
def test_channel_slices_of_wider_rows(C, M):
    """x = columns [C, 2C), y = columns [0, C), out = columns [C, 2C) of 2C-wide rows; the other half of out's rows
    keeps its sentinel."""
    x, y = _data(C, M, seed=7)
    got, rest = _run(x, y, C, M, _weights(C), x_slice=True, y_slice=True, o_slice=True)
    _check(got, x, y, _weights(C), "slices C %d M %d" % (C, M))
    assert (rest == 777.0).all()


@pytest.mark.parametrize("C", [64, 512])
def test_ragged_rows_are_exact_zeros_whatever_the_inputs_hold(C):
    """3 images of 5 x 11 pixels, valid widths (11, 4, 7); NaN in the padding columns of both inputs."""
    B, Hh, Ww = 3, 5, 11
    lens = [11, 4, 7]
    M = B * Hh * Ww
    x, y = _data(C, M, seed=3)
    col = np.tile(np.arange(Ww), B * Hh)
    img = np.repeat(np.arange(B), Hh * Ww)
    pad = col >= np.asarray(lens)[img]
    x[pad], y[pad] = np.nan, np.nan
    got, _ = _run(x, y, C, M, _weights(C), row_len=lens, HW=Hh * Ww, W=Ww)
    assert (got[pad] == 0.0).all() and not np.signbit(got[pad]).any()
    assert np.isfinite(got).all()
    _check(got[~pad], x[~pad], y[~pad], _weights(C), "ragged C %d" % C)


@pytest.mark.parametrize("C", [64, 512])
def test_saturated_gate(C):
    """Logits shifted by +30 (even channels) / -30 (odd): tanh is +-1 to the last bit, so out = 2 x or 2 y exactly."""
    M = 100
    x, y = _data(C, M, seed=5)
    w = _weights(C, shift=30.0)
    got, _ = _run(x, y, C, M, w)
    assert np.array_equal(got[:, 0::2], 2.0 * x[:, 0::2])
    assert np.array_equal(got[:, 1::2], 2.0 * y[:, 1::2])
    _check(got, x, y, w, "saturated C %d" % C)


def test_arguments_outside_the_contract_are_refused_without_a_launch():
    from wespeaker_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    buf = torch.full((64, 4096), 3.0, dtype=torch.float32, device=dev)
    other = torch.zeros((64, 4096), dtype=torch.float32, device=dev)
    w = torch.zeros(4 * 1024 * 1024, dtype=torch.float32, device=dev)
    st = _lib.current_stream_ptr(dev)

    def call(C, out, ldo=4096, oo=0):
        return L.ws_debug_aff_fuse(_lib.ptr(buf), 4096, 0, _lib.ptr(other), 4096, 0, _lib.ptr(out), ldo, oo, _lib.ptr(w),
                                   _lib.ptr(w), _lib.ptr(w), _lib.ptr(w), 64, C, None, 0, 0, st)

    for C, out, word in ((48, other, "multiple of 32"), (4096, other, "multiple of 32"), (64, buf, "aliases x")):
        rc = call(C, out)
        assert rc == -1, (C, rc)                                   # WS_ERR_INVALID_ARG
        assert word in L.ws_last_error().decode(), L.ws_last_error()
    # a disjoint channel window of x's own rows is not an alias
    assert call(64, buf, 4096, 64) == 0
    torch.cuda.synchronize()
    assert (buf[:, :64] == 3.0).all() and (buf[:, 128:] == 3.0).all() and (other == 0).all()
