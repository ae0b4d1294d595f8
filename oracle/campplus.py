"""ORACLE (test infrastructure, never shipped): CPU fp32 restatement of the reference's CAM++
forward as one straight-line function over a state_dict.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.

Follows (file:line in /root/reference):
  wespeaker/models/campplus.py:409-413  CAMPPlus.forward ((B,T,F) -> (B,F,T) -> head -> xvector)
  wespeaker/models/campplus.py:282-330  FCM (conv1+bn+relu, 2x2 BasicResBlocks stride (2,1), conv2 stride (2,1), reshape (B, C*F', T))
  wespeaker/models/campplus.py:245-279  BasicResBlock
  wespeaker/models/campplus.py:55-83    TDNNLayer (conv1d k5 stride 2 pad 2 -> BN -> ReLU)
  wespeaker/models/campplus.py:138-170  CAMDenseTDNNLayer (BN-ReLU -> 1x1 -> BN-ReLU -> CAMLayer)
  wespeaker/models/campplus.py:86-135   CAMLayer (local conv * sigmoid(W2 relu(W1 (mean + segmean_100))))
  wespeaker/models/campplus.py:173-201  dense block: x = cat([x, layer(x)])
  wespeaker/models/campplus.py:204-238  TransitLayer, DenseLayer
PINNED by tests/golden/campplus_ref.npz (outputs of the reference's own nn.Module).
"""
import torch
import torch.nn.functional as F

from .ecapa import _bn, _t, tstp

BLOCKS = ((12, 1), (24, 2), (16, 2))     # (layers, dilation); kernel 3, growth 32, bn_channels 128


def _bn_relu(sd, prefix, x):
    return F.relu(_bn(sd, prefix + ".batchnorm", x))


def _res_block(sd, p, x, stride, taps=None):
    """taps (a dict, optional) receives mid = conv1 + bn1 + relu, sc = the shortcut convolution's output (blocks that
    have one) and block = the result."""
    mid = F.relu(_bn(sd, p + ".bn1", F.conv2d(x, _t(sd, p + ".conv1.weight"), None,
                                              stride=(stride, 1), padding=1)))
    out = _bn(sd, p + ".bn2", F.conv2d(mid, _t(sd, p + ".conv2.weight"), None, padding=1))
    sc = x
    if p + ".shortcut.0.weight" in sd:
        sc = _bn(sd, p + ".shortcut.1", F.conv2d(x, _t(sd, p + ".shortcut.0.weight"), None,
                                                 stride=(stride, 1)))
        if taps is not None:
            taps["sc"] = sc
    out = F.relu(out + sc)
    if taps is not None:
        taps["mid"], taps["block"] = mid, out
    return out


def _seg_pooling(x, seg_len=100):
    seg = F.avg_pool1d(x, kernel_size=seg_len, stride=seg_len, ceil_mode=True)
    shape = seg.shape
    seg = seg.unsqueeze(-1).expand(shape[0], shape[1], shape[2], seg_len).reshape(shape[0], shape[1], -1)
    return seg[..., :x.shape[-1]]


def _cam_layer(sd, p, x, dilation, taps=None, seg_pooling=_seg_pooling):
    """taps (a dict, optional) receives mask = the sigmoid gate of every 100-frame segment, (B, 32, segments).
    seg_pooling: the segment-mean function (tests replace it to state a fault)."""
    y = F.conv1d(x, _t(sd, p + ".linear_local.weight"), None, padding=dilation, dilation=dilation)
    ctx = x.mean(-1, keepdim=True) + seg_pooling(x)
    ctx = F.relu(F.conv1d(ctx, _t(sd, p + ".linear1.weight"), _t(sd, p + ".linear1.bias")))
    m = torch.sigmoid(F.conv1d(ctx, _t(sd, p + ".linear2.weight"), _t(sd, p + ".linear2.bias")))
    if taps is not None:
        taps["mask"] = m[..., ::100]
    return y * m


def _dense_layer(sd, k, j, x, taps=None, seg_pooling=_seg_pooling):
    """Layer j (0-based) of dense block k (0-based) on the block buffer x (B, C, T'): the 32 gated channels.
    taps receives h = the bottleneck after BN-ReLU (what the CAM layer reads) and mask."""
    p = "xvector.block%d.tdnnd%d" % (k + 1, j + 1)
    h = F.conv1d(_bn_relu(sd, p + ".nonlinear1", x), _t(sd, p + ".linear1.weight"), None)
    h = _bn_relu(sd, p + ".nonlinear2", h)
    if taps is not None:
        taps["h"] = h
    return _cam_layer(sd, p + ".cam_layer", h, BLOCKS[k][1], taps, seg_pooling)


def _trunk(sd, x, k0=0, j0=0, mid=None):
    """Dense blocks from layer j0 of block k0 on (x = that block's buffer so far), transits, pooling, embedding."""
    for k in range(k0, len(BLOCKS)):
        for j in range(j0 if k == k0 else 0, BLOCKS[k][0]):
            taps = {} if mid is not None else None
            h = _dense_layer(sd, k, j, x, taps)
            if mid is not None:
                key = "b%d.l%d" % (k + 1, j + 1)
                mid[key], mid[key + ".h"], mid[key + ".mask"] = h, taps["h"], taps["mask"]
            x = torch.cat([x, h], dim=1)
        p = "xvector.transit%d" % (k + 1)
        x = F.conv1d(_bn_relu(sd, p + ".nonlinear", x), _t(sd, p + ".linear.weight"), None)
        if mid is not None:
            mid["transit%d" % (k + 1)] = x
    x = _bn_relu(sd, "xvector.out_nonlinear", x)
    stats = tstp(x)
    if mid is not None:
        mid["pooled"] = stats
    emb = F.conv1d(stats.unsqueeze(-1), _t(sd, "xvector.dense.linear.weight"), None).squeeze(-1)
    return _bn(sd, "xvector.dense.nonlinear.batchnorm", emb)


def _cast(sd, dtype):
    if dtype == torch.float32:               # (the fp32 path as it always was: tensors taken as they are)
        return sd
    return {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v))
            for k, v in sd.items()}


@torch.no_grad()
def campplus_forward(sd, feats, dtype=torch.float32, return_intermediates=False):
    """feats (B, T, F) float32 -> (B, E).
    dtype=torch.float64 evaluates the same network in double precision (the ground truth of the per-layer parity tests).
    return_intermediates: also a dict, channels first: `stem`, `res1` .. `res4` (the FCM residual blocks; `res<i>.mid`
    and, for blocks 1 and 3, `res<i>.sc` beside them) and `fcm` (head.conv2's output), all (B, 32, F', T); `tdnn`
    (B, 128, T'); per dense layer `b<k>.l<j>` (its 32 gated channels), `b<k>.l<j>.h` (the bottleneck after BN-ReLU,
    (B, 128, T')) and `b<k>.l<j>.mask` (B, 32, segments); `transit1` .. `transit3`; `pooled` (B, 1024)."""
    sd = _cast(sd, dtype)
    mid = {} if return_intermediates else None
    x = torch.as_tensor(feats, dtype=dtype).permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_bn(sd, "head.bn1", F.conv2d(x, _t(sd, "head.conv1.weight"), None, padding=1)))
    if mid is not None:
        mid["stem"] = out
    i = 0
    for layer in ("head.layer1", "head.layer2"):
        for blk, stride in ((".0", 2), (".1", 1)):
            i += 1
            taps = {} if mid is not None else None
            out = _res_block(sd, layer + blk, out, stride, taps)
            if mid is not None:
                mid["res%d" % i] = out
                for t in ("mid", "sc"):
                    if t in taps:
                        mid["res%d.%s" % (i, t)] = taps[t]
    out = F.relu(_bn(sd, "head.bn2", F.conv2d(out, _t(sd, "head.conv2.weight"), None, stride=(2, 1),
                                              padding=1)))
    if mid is not None:
        mid["fcm"] = out
    x = out.reshape(out.shape[0], out.shape[1] * out.shape[2], out.shape[3])
    x = F.conv1d(x, _t(sd, "xvector.tdnn.linear.weight"), None, stride=2, padding=2)
    x = _bn_relu(sd, "xvector.tdnn.nonlinear", x)
    if mid is not None:
        mid["tdnn"] = x
    emb = _trunk(sd, x, 0, 0, mid)
    return (emb, mid) if return_intermediates else emb


@torch.no_grad()
def campplus_resume(sd, x, block, layer, dtype=torch.float32):
    """The rest of campplus_forward from a dense-block buffer: `x` (B, C, T'), channels first, is the buffer of dense
    block `block` (1-based) with its first `layer` layers appended (C = the block's input channels + 32 * layer; layer
    = 0: the TDNN / previous transit output alone).  Layers layer + 1 .. of that block, its transit, the later blocks,
    pooling and the embedding layer follow.  For tests that perturb a layer's output and ask how far the embedding
    moves."""
    sd = _cast(sd, dtype)
    return _trunk(sd, torch.as_tensor(x).to(dtype), block - 1, layer)
