"""Launch-local oracle of ECAPA-TDNN's binary16 back-end (WS_PREC_F16), and the two comparisons built on it.

A chained binary16 oracle cannot judge this back-end: a perturbation below one binary16 ulp u turns into ~sqrt(delta * u)
at the next rounding point, so two honest evaluations of the same rounded network drift 6e-4 apart within three
blocks.  Every function here therefore restates ONE launch of ecapa_model.hip: it takes that launch's inputs as the
device left them (the taps, NativeSpeakerModel.tap) and returns the launch's output BEFORE the store's rounding, in
`dtype` arithmetic -- torch.float64 is the oracle, torch.float32 the baseline that sizes every bound.

Rounding model, launch by launch (R = round-to-nearest-even to binary16, the kernels' `(_Float16)` cast; W16 = R(weight),
the Wh plane of pack_conv; bias and the BN scale / shift are the fp32 constants of the device; sums are fp32 on the device):
  im2col     col16[b, t, tap * F + f] = R(feats[b, t + tap - 2, f]), 0 outside the utterance and in the K padding (fbank.hip)
  layer1     out1_16 = R(relu(col16 . W16 + b) * sc + sh)
  conv1      y1 = relu(x16 . W16 + b) * sc + sh in fp32; y2_16[:, 7w:] = R(y1[:, 7w:])   (the pass-through split)
  Res2       the f16 mode runs the split-binary16 chain (res2_fused.hip): an operand x is hi + lo, hi = R(x),
             lo = R(x - hi) (22 bits), weights alike, a product is hi*hi + hi*lo + lo*hi (lo*lo dropped), the running
             activation v_i + split_(i+1) is formed in fp32 and split again -- it is NEVER rounded to binary16;
             only the store is: y2_16[:, i*w:(i+1)*w] = R(v_i), v_i = relu(conv + b) * sc + sh.  Rounded AFTER the split is added.
  conv3      y3_16 = R(v), v = relu(y2_16 . W16 + b) * sc + sh; the SE mean is the column sum of the UNROUNDED fp32 v in
             the 64 / 128-row tile kernels and of the STORED binary16 values in the 256 x 256 kernel's binary16 epilogue
             (conv_gemm.hip); T < 64: the mean of the fp32 y3 (se_pool_fc).  se_s = sigmoid(W2 relu(W1 mean + b1) + b2),
             fp32 weights.
  SE         cat16[:, L*C:(L+1)*C] = R(x + y3 * s): one rounding; x, y3 binary16 rows (T >= 64) or the fp32 tensors.
  catconv    h16 = R(relu(cat16 . W16 + b)); column sums for the context mean as in conv3.
  stats      mean from those column sums, std = sqrt(sum((h16 - mean)^2) / (T - 1) + 1e-7) over the STORED h16 rows
             (astp_std_from_colsum_kernel); T < 64: both from the fp32 h (astp_stats_kernel).
  bias_img   stats . W1[:, 1536:]^T + b1 on fp32 operands (small_m_gemm_f32_kernel; nothing is rounded to binary16)
  linear1    att = tanh(h16 . W16[:, :1536] + bias_img | b1) in fp32, att16 = R(att)
  pooling    logits = att16 . W16 (the column bias cancels in the softmax over time), a = softmax_t, mean = sum a h16,
             std = sqrt(max(sum a h16^2 - mean^2, 1e-7)); T < 64 reads the fp32 h
  head       pooled . Wf^T + Bf, the BN + Linear (+ bn2) fold of ecapa_model.hip in float64, stored as fp32 operands

Check A (check_a) is for outputs that are ONE binary16 store of an fp32-accumulated value, check B is
tests/test_gpu_layers.py's tap_check against these launch oracles.  No tolerance here is a bare constant: each is 8 x
the float32 baseline of the same launch (the per-tap allowance reasoned in tests/test_gpu_layers.py), or one binary16 ulp.
"""
import numpy as np
import torch
import torch.nn.functional as F

K_TAP = 8.0                  # the project's per-tap allowance (tests/test_gpu_layers.py, module docstring)
ULP16_FLOOR = 2.0 ** -11     # scaled error of ONE correctly rounded binary16 store (check B on a binary16 output)
BN_EPS = 1e-5


def rnd16(x):
    """Round-to-nearest-even to binary16, returned in float64 (numpy converts float64 / float32 -> float16 directly)."""
    return np.asarray(x).astype(np.float16).astype(np.float64)


def _t(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dt)


def _np(sd, key):
    v = sd[key]
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)


def _post(sd, prefix):
    """The device's fp32 BN constants: computed in float64, stored as fp32 (ModelBase::bn_affine / pack_conv)."""
    s = _np(sd, prefix + ".weight") / np.sqrt(_np(sd, prefix + ".running_var") + BN_EPS)
    sh = _np(sd, prefix + ".bias") - _np(sd, prefix + ".running_mean") * s
    return s.astype(np.float32).astype(np.float64), sh.astype(np.float32).astype(np.float64)


def _split(x):
    """hi + lo binary16 planes of x (a tensor): hi = R(x), lo = R(x - hi)."""
    hi = x.to(torch.float16).to(x.dtype)
    lo = (x - hi).to(torch.float16).to(x.dtype)
    return hi, lo


def _conv_relu_bn(sd, prefix, x, w, dt, padding=0, dilation=1, bn=True):
    """x (B, T, K) channels last, w (N, K, k) -> relu(conv + b) [* sc + sh], (B, T, N) numpy float64."""
    y = F.conv1d(_t(x, dt).permute(0, 2, 1), _t(w, dt), _t(_np(sd, prefix + ".conv.bias" if bn else prefix + ".bias"), dt),
                 padding=padding, dilation=dilation)
    y = torch.relu(y)
    if bn:
        sc, sh = _post(sd, prefix + ".bn")
        y = y * _t(sc, dt)[None, :, None] + _t(sh, dt)[None, :, None]
    return y.permute(0, 2, 1).double().numpy()


# ------------------------------------------------------------------------------------------------- the launches
def im2col(feats, ldw):
    """(B, T, F) fp32 features -> the binary16 im2col image (B, T, ldw) of the k5 / p2 layer 1, exactly."""
    f = rnd16(feats)
    B, T, Fd = f.shape
    out = np.zeros((B, T, ldw))
    for tap in range(5):
        lo, hi = max(0, 2 - tap), min(T, T + 2 - tap)
        out[:, lo:hi, tap * Fd:(tap + 1) * Fd] = f[:, lo + tap - 2:hi + tap - 2]
    return out


def layer1(sd, feats, dt):
    return _conv_relu_bn(sd, "layer1", rnd16(feats), rnd16(_np(sd, "layer1.conv.weight")), dt, padding=2)


def _blk(L):
    return "layer%d.se_res2block" % (L + 2)


def conv1(sd, L, x16, dt):
    """Block L (0 .. 2), first 1x1 conv from the binary16 block input -> y1 before any store."""
    p = _blk(L) + ".0"
    return _conv_relu_bn(sd, p, x16, rnd16(_np(sd, p + ".conv.weight")), dt)


def res2(sd, L, y1, dt):
    """The fused chain from the fp32 y1 -> the 7 step outputs (B, T, 7w) before the binary16 store."""
    p = _blk(L) + ".1"
    dil = L + 2
    y1 = _t(y1, dt).permute(0, 2, 1)                              # (B, C, T)
    w = y1.shape[1] // 8
    out = []
    x = y1[:, :w]
    for i in range(7):
        wt = _t(_np(sd, "%s.convs.%d.weight" % (p, i)), dt)
        wh, wl = _split(wt)
        xh, xl = _split(x)
        conv = lambda a, k: F.conv1d(a, k, None, padding=dil, dilation=dil)
        acc = conv(xl, wh) + conv(xh, wl) + conv(xh, wh)          # the kernel's order: cross terms first, hi*hi last
        sc, sh = _post(sd, "%s.bns.%d" % (p, i))
        v = torch.relu(acc + _t(_np(sd, "%s.convs.%d.bias" % (p, i)), dt)[None, :, None])
        v = v * _t(sc, dt)[None, :, None] + _t(sh, dt)[None, :, None]
        out.append(v)
        if i < 6:
            x = v + y1[:, (i + 1) * w:(i + 2) * w]
    return torch.cat(out, dim=1).permute(0, 2, 1).double().numpy()


def conv3(sd, L, y2_16, dt):
    p = _blk(L) + ".2"
    return _conv_relu_bn(sd, p, y2_16, rnd16(_np(sd, p + ".conv.weight")), dt)


def se_gate(sd, L, y3_summed, dt):
    """y3_summed (B, T, C): the values the device summed for the SE mean (see the module docstring) -> se_s (B, C)."""
    p = _blk(L) + ".3"
    s = _t(y3_summed, dt).mean(dim=1)
    s = torch.relu(F.linear(s, _t(_np(sd, p + ".linear1.weight"), dt), _t(_np(sd, p + ".linear1.bias"), dt)))
    s = torch.sigmoid(F.linear(s, _t(_np(sd, p + ".linear2.weight"), dt), _t(_np(sd, p + ".linear2.bias"), dt)))
    return s.double().numpy()


def se_residual(x, y3, s, dt):
    """x + y3 * s from the rows the device read (binary16 or fp32) and its fp32 gate, before the store."""
    return (_t(x, dt) + _t(y3, dt) * _t(s, dt)[:, None, :]).double().numpy()


def catconv(sd, cat16, dt):
    return _conv_relu_bn(sd, "conv", cat16, rnd16(_np(sd, "conv.weight")), dt, bn=False)


def context_stats(h_summed, h_rows, dt):
    """[mean; std] (B, 3072): the mean of h_summed (what the column sums added up), the centred squares over h_rows."""
    m = _t(h_summed, dt).mean(dim=1)
    d = _t(h_rows, dt) - m[:, None, :]
    var = (d * d).sum(dim=1) / (h_rows.shape[1] - 1)
    return torch.cat([m, torch.sqrt(var + 1e-7)], dim=1).double().numpy()


def bias_img(sd, stats, dt):
    w1 = _np(sd, "pool.linear1.weight")[:, :, 0]
    return F.linear(_t(stats, dt), _t(w1[:, 1536:], dt), _t(_np(sd, "pool.linear1.bias"), dt)).double().numpy()


def linear1(sd, h16, bimg, dt):
    """tanh(h16 . W16[:, :1536] + bias): bimg (B, 128) for the GLOB models, None -> the layer's own bias."""
    w1 = rnd16(_np(sd, "pool.linear1.weight")[:, :1536, 0])
    y = torch.matmul(_t(h16, dt), _t(w1, dt).T)
    y = y + (_t(bimg, dt)[:, None, :] if bimg is not None else _t(_np(sd, "pool.linear1.bias"), dt))
    return torch.tanh(y).double().numpy()


def pooling(sd, att16, h_rows, dt):
    w2 = rnd16(_np(sd, "pool.linear2.weight")[:, :, 0])
    e = torch.matmul(_t(att16, dt), _t(w2, dt).T)
    a = torch.softmax(e, dim=1)
    h = _t(h_rows, dt)
    mean = (a * h).sum(dim=1)
    var = (a * h * h).sum(dim=1) - mean * mean
    return torch.cat([mean, torch.sqrt(var.clamp(min=1e-7))], dim=1).double().numpy()


def head(sd, pooled, dt):
    """bn -> linear (-> bn2) folded in float64 and stored as fp32 operands, as EcapaModel::finalize does."""
    s = 1.0 / np.sqrt(_np(sd, "bn.running_var") + BN_EPS) * _np(sd, "bn.weight")
    sh = _np(sd, "bn.bias") - _np(sd, "bn.running_mean") * s
    lw, lb = _np(sd, "linear.weight"), _np(sd, "linear.bias")
    s2, t2 = np.ones(lw.shape[0]), np.zeros(lw.shape[0])
    if "bn2.running_mean" in sd:
        s2 = _np(sd, "bn2.weight") / np.sqrt(_np(sd, "bn2.running_var") + BN_EPS)
        t2 = _np(sd, "bn2.bias") - _np(sd, "bn2.running_mean") * s2
    W = (lw * s[None, :] * s2[:, None]).astype(np.float32).astype(np.float64)
    Bv = ((lb + lw @ sh) * s2 + t2).astype(np.float32).astype(np.float64)
    return F.linear(_t(pooled, dt), _t(W, dt), _t(Bv, dt)).double().numpy()


# ------------------------------------------------------------------------------------------------ the comparisons
def _mismatch_share(y, r):
    return float(np.count_nonzero(y != r)) / y.size


def check_a(name, Y, y64, y32, rows=None):
    """Check A: Y (the device's binary16 tensor, widened) against the float64 launch value y64, with the float32
    evaluation y32 of the same launch as the baseline.  Every element: Y == R(y64), or its binary16 neighbour, or
    |Y - y64| <= eps = 8 x max|y32 - y64| (near zero one binary16 ulp is smaller than the fp32 accumulation error).
    Share of Y != R(y64): at most 8 x the baseline's share, the baseline floored at 16 / numel -- over the whole tap AND
    over every column (channel) on its own (numel = the column's rows), so that one channel rounded the wrong way is
    seen among a thousand honest ones.  -> (ok, worst ratio = share / (baseline share, floored))."""
    Y, y64, y32 = (np.asarray(a, dtype=np.float64) for a in (Y, y64, y32))
    assert Y.shape == y64.shape == y32.shape, (Y.shape, y64.shape, y32.shape)
    Y, y64, y32 = (a.reshape(-1, a.shape[-1]) for a in (Y, y64, y32))
    r64h = y64.astype(np.float16)
    r64, r32 = r64h.astype(np.float64), rnd16(y32)
    up = np.nextafter(r64h, np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(r64h, np.float16(-np.inf)).astype(np.float64)
    eps = K_TAP * float(np.abs(y32 - y64).max())

    def judge(Z):
        elem = (Z == r64) | (Z == up) | (Z == dn) | (np.abs(Z - y64) <= eps)
        share, base = _mismatch_share(Z, r64), max(_mismatch_share(r32, r64), 16.0 / Z.size)
        col_share = np.count_nonzero(Z != r64, axis=0) / Z.shape[0]
        col_base = np.maximum(np.count_nonzero(r32 != r64, axis=0) / Z.shape[0], 16.0 / Z.shape[0])
        ratio = max(share / base, float((col_share / col_base).max()))
        return int(np.count_nonzero(~elem)), share, ratio, bool(np.isfinite(Z).all())

    # the CPU baseline must stay under its own cap before it is relied on
    b_bad, b_share, b_ratio, _ = judge(r32)
    assert b_bad == 0 and b_ratio <= K_TAP, "%s: the float32 baseline fails its own check (%d, %.2f)" % (name, b_bad, b_ratio)
    bad, share, ratio, finite = judge(Y)
    if rows is not None:
        rows.append("%-12s A  mismatch share: baseline %.2e device %.2e | worst share ratio %6.2f (cap %g) | elements "
                    "outside ulp / eps: %d (eps %.1e)" % (name, b_share, share, ratio, K_TAP, bad, eps))
    return finite and bad == 0 and ratio <= K_TAP, ratio


def check_b(name, got, y64, y32, rows=None, floor=None):
    """Check B: tests/test_gpu_layers.py's tap_check against the launch oracle, k = 8; floor = ULP16_FLOOR for a
    binary16 output (y64 / y32 are then the ROUNDED launch values)."""
    from test_gpu_layers import ERR_FLOOR, tap_check
    return tap_check(name, got, y64, y32, K_TAP, rows, floor=ERR_FLOOR if floor is None else floor)
