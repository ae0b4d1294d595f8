"""ORACLE (test infrastructure, never shipped): CPU fp32 restatement of the reference's ResNet
speaker-embedding forward as one straight-line function over a state_dict.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.

Follows (file:line in /root/reference):
  wespeaker/models/resnet.py:171-182  _get_frame_level_feat  ((B,T,F) -> (B,1,F,T), conv1+bn1+relu, layer1-4)
  wespeaker/models/resnet.py:63-69    BasicBlock.forward   (conv-bn-relu, conv-bn, += shortcut, relu)
  wespeaker/models/resnet.py:101-107  Bottleneck.forward   (1x1, 3x3 (stride here), 1x1 x4, += shortcut, relu)
  wespeaker/models/resnet.py:163-169  _make_layer (first block of a stage carries the stride)
  wespeaker/models/resnet.py:192-204  forward: TSTP -> seg_1 [-> relu -> seg_bn_1 -> seg_2]
  wespeaker/models/pooling_layers.py:78-85 TSTP
PINNED by tests/golden/resnet_ref.npz (outputs of the reference's own nn.Modules).
"""
import torch
import torch.nn.functional as F

from .ecapa import _bn, _t, tstp

LAYOUTS = {            # name -> (bottleneck?, blocks per stage)   resnet.py:207-260
    "ResNet18": (False, [2, 2, 2, 2]), "ResNet34": (False, [3, 4, 6, 3]),
    "ResNet50": (True, [3, 4, 6, 3]), "ResNet101": (True, [3, 4, 23, 3]),
    "ResNet152": (True, [3, 8, 36, 3]), "ResNet221": (True, [6, 16, 48, 3]),
    "ResNet293": (True, [10, 20, 64, 3]),
}


def _conv_bn(sd, conv, bn, x, stride=1, padding=0):
    return _bn(sd, bn, F.conv2d(x, _t(sd, conv + ".weight"), None, stride=stride, padding=padding))


def _block(sd, p, x, stride, bottleneck, taps=None, mid=None):
    """taps (a dict, optional) receives the block's tensors: mid = the BasicBlock conv1 / Bottleneck conv2 output (after
    bn + relu), y1 = the Bottleneck conv1 output, sc = the shortcut convolution's output (blocks that have one), block = the result.  mid (optional): take
    that tensor as given and run the block's rest (resnet_resume)."""
    if bottleneck:
        if mid is None:
            out = F.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", x))
            if taps is not None:
                taps["y1"] = out
            mid = F.relu(_conv_bn(sd, p + ".conv2", p + ".bn2", out, stride=stride, padding=1))
        out = _conv_bn(sd, p + ".conv3", p + ".bn3", mid)
    else:
        if mid is None:
            mid = F.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", x, stride=stride, padding=1))
        out = _conv_bn(sd, p + ".conv2", p + ".bn2", mid, padding=1)
    sc = x
    if p + ".shortcut.0.weight" in sd:
        sc = _conv_bn(sd, p + ".shortcut.0", p + ".shortcut.1", x, stride=stride)
        if taps is not None:
            taps["sc"] = sc
    out = F.relu(out + sc)
    if taps is not None:
        taps["mid"], taps["block"] = mid, out
    return out


def block_list(model_name):
    """[(state_dict prefix, stride)] of the residual blocks in forward order."""
    return [("layer%d.%d" % (s + 1, b), (1 if s == 0 else 2) if b == 0 else 1)
            for s, nb in enumerate(LAYOUTS[model_name][1]) for b in range(nb)]


def _cast(sd, dtype):
    if dtype == torch.float32:               # (the fp32 path as it always was: tensors taken as they are)
        return sd
    return {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v))
            for k, v in sd.items()}


def _head(sd, out, mid=None):
    stats = tstp(out)
    emb = F.linear(stats, _t(sd, "seg_1.weight"), _t(sd, "seg_1.bias"))
    if mid is not None:
        mid["pooled"], mid["emb_a"] = stats, emb
    if "seg_2.weight" in sd:
        o = F.relu(emb)
        o = F.batch_norm(o, _t(sd, "seg_bn_1.running_mean"), _t(sd, "seg_bn_1.running_var"), None,
                         None, False, 0.0, 1e-5)
        emb = F.linear(o, _t(sd, "seg_2.weight"), _t(sd, "seg_2.bias"))
    return emb


@torch.no_grad()
def resnet_forward(sd, feats, model_name="ResNet34", dtype=torch.float32, return_intermediates=False):
    """feats (B, T, F) float32 -> embedding (B, E): embed_a, or embed_b when the state_dict has
    seg_2.* (two_emb_layer=True; callers take outputs[-1]).
    dtype=torch.float64 evaluates the same network in double precision (the ground truth of the per-block parity tests).
    return_intermediates: also a dict with `stem` (B, 32, F, T), `blocks` = one dict per residual block (`mid`, `block`,
    `sc` where the block has a shortcut convolution, `y1` = a Bottleneck's conv1 output; channels first), `pooled` (B, 2 * stats_dim) and `emb_a` (seg_1's
    output before relu / seg_bn_1 / seg_2)."""
    bottleneck, _ = LAYOUTS[model_name]
    sd = _cast(sd, dtype)
    x = torch.as_tensor(feats, dtype=dtype).permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_conv_bn(sd, "conv1", "bn1", x, padding=1))
    mid = {"stem": out, "blocks": []} if return_intermediates else None
    for p, stride in block_list(model_name):
        taps = {} if return_intermediates else None
        out = _block(sd, p, out, stride, bottleneck, taps)
        if return_intermediates:
            mid["blocks"].append(taps)
    emb = _head(sd, out, mid)
    return (emb, mid) if return_intermediates else emb


@torch.no_grad()
def resnet_resume(sd, model_name, dtype=torch.float32, after_block=0, x=None, mid=None):
    """The rest of resnet_forward from an intermediate of return_intermediates (channels first): from `x`, the output
    of block `after_block` (1-based; 0 = the stem), or -- with `mid` -- from the `mid` tensor of block `after_block`,
    `x` then being that block's INPUT (its shortcut reads it).  For tests that perturb an activation and ask how far
    the embedding moves."""
    bottleneck, _ = LAYOUTS[model_name]
    sd = _cast(sd, dtype)
    blocks = block_list(model_name)
    out = torch.as_tensor(x).to(dtype)
    if mid is not None:
        p, stride = blocks[after_block - 1]
        out = _block(sd, p, out, stride, bottleneck, mid=torch.as_tensor(mid).to(dtype))
    for p, stride in blocks[after_block:]:
        out = _block(sd, p, out, stride, bottleneck)
    return _head(sd, out)
