"""ORACLE (test infrastructure, never shipped): float64 restatement of the reference's ERes2Net34_Base / _Large / _aug
forward as one straight-line function over a state_dict.

Follows (file:line in the reference, wenet-e2e/wespeaker):
  wespeaker/models/eres2net.py:44-52     ReLU = Hardtanh(0, 20)
  wespeaker/models/eres2net.py:97-103    AFF.forward: cat, local_att (conv-bn-silu-conv-bn), 1 + tanh, x a + y (2 - a)
  wespeaker/models/eres2net.py:145-168   BasicBlockERes2Net.forward (layers 1 - 2: sp = sp + spx[i])
  wespeaker/models/eres2net.py:216-240   BasicBlockERes2Net_diff_AFF.forward (layers 3 - 4: sp = AFF(sp, spx[i]))
  wespeaker/models/eres2net.py:354-391   _get_frame_level_feat + forward (downsample convs, global AFFs, TSTP, seg_1 [seg_2])
  wespeaker/models/pooling_layers.py:78-85 TSTP
PINNED by tests/golden/eres2net_ref.npz (outputs of the reference's own nn.Module, tools/make_golden_eres2net.py) and,
where the reference is present, by a live comparison (tests/test_eres2net_cpu.py).

`clamp` and `swap_aff` exist for the fixtures with teeth of the tests: clamp=False replaces Hardtanh(0, 20) by max(x, 0),
swap_aff=True exchanges AFF's two arguments -- what an implementation with either mistake would compute.
"""
import re

import torch
import torch.nn.functional as F

from oracle.ecapa import _bn, _t
from oracle.resnet import _conv_bn

LAYOUTS = {      # eres2net.py:394-430: m_channels, baseWidth, scale, expansion
    "ERes2Net34_Base": (32, 32, 2, 2), "ERes2Net34_Large": (64, 32, 2, 2), "ERes2Net34_aug": (64, 24, 3, 4),
}
BLOCKS = (3, 4, 6, 3)


def _cast(sd, dtype):
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def aff(sd, p, x, y):
    """AFF.forward (eres2net.py:97-103) with the module at prefix p."""
    xa = torch.cat((x, y), dim=1)
    h = F.conv2d(xa, _t(sd, p + ".local_att.0.weight"), _t(sd, p + ".local_att.0.bias"))
    h = F.silu(_bn(sd, p + ".local_att.1", h))
    a = F.conv2d(h, _t(sd, p + ".local_att.3.weight"), _t(sd, p + ".local_att.3.bias"))
    a = 1.0 + torch.tanh(_bn(sd, p + ".local_att.4", a))
    return x * a + y * (2.0 - a)


@torch.no_grad()
def eres2net_forward(sd, feats, name="ERes2Net34_Base", dtype=torch.float64, return_intermediates=False, clamp=True,
                     swap_aff=False, override=None):
    """feats (B, T, F) -> embedding (B, E) in `dtype`.  return_intermediates: also a dict of (B, C, F, T) maps -- `stem`;
    for the i-th block (1-based) `b<i>.block`, `b<i>.mid` (conv1 + bn1 + relu), `b<i>.cat` (what conv3 reads), `b<i>.sc`
    where the block has a shortcut convolution; `fuse12`, `fuse123`, `fuse1234`; `pooled` (B, 2D); `emb_a` (two-layer
    models: relu + seg_bn_1 of seg_1's output, what seg_2 reads); and `aff` = a list of (prefix, x, y, out) per AFF in
    execution order.  override = {`b<i>.cat` / `b<i>.block`: (B, C, F, T) tensor}: that intermediate is replaced where it
    is recorded and the forward's own tail runs on it (the fixtures with teeth of tests/test_gpu_eres2net_layers.py)."""
    m, base_width, scale, exp = LAYOUTS[name]
    sd = _cast(sd, dtype)
    act = (lambda t: t.clamp(0.0, 20.0)) if clamp else (lambda t: t.clamp(min=0.0))
    mid = {"aff": []}
    override = {k: torch.as_tensor(v).to(dtype) for k, v in (override or {}).items()}
    unknown = [k for k in override if not re.fullmatch(r"b([1-9]|1[0-6])\.(cat|block)", k)]
    assert not unknown, unknown

    def replaced(key, own):
        if key not in override:
            return own
        assert override[key].shape == own.shape, (key, tuple(override[key].shape), tuple(own.shape))
        return override[key]

    def fuse(p, x, y):
        out = aff(sd, p, y, x) if swap_aff else aff(sd, p, x, y)
        mid["aff"].append((p, x, y, out))
        return out

    x = torch.as_tensor(feats).to(dtype).permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_conv_bn(sd, "conv1", "bn1", x, padding=1))
    mid["stem"] = out
    i = 0
    stage_out = []
    for s, nb in enumerate(BLOCKS):
        width = int(m * 2 ** s * (base_width / 64.0))
        for b in range(nb):
            stride = (1 if s == 0 else 2) if b == 0 else 1
            p = "layer%d.%d" % (s + 1, b)
            i += 1
            y1 = act(_conv_bn(sd, p + ".conv1", p + ".bn1", out, stride=stride))
            spx = torch.split(y1, width, 1)
            if s < 2:
                sp, cat = spx[0], []
                for j in range(scale):
                    if j >= 1:
                        sp = sp + spx[j]
                    sp = act(_conv_bn(sd, p + ".convs.%d" % j, p + ".bns.%d" % j, sp, padding=1))
                    cat.append(sp)
            else:
                sp = act(_conv_bn(sd, p + ".conv2_1", p + ".bn2_1", spx[0], padding=1))
                cat = [sp]
                for j in range(1, scale):
                    sp = fuse(p + ".fuse_models.%d" % (j - 1), sp, spx[j])
                    sp = act(_conv_bn(sd, p + ".convs.%d" % (j - 1), p + ".bns.%d" % (j - 1), sp, padding=1))
                    cat.append(sp)
            cat = replaced("b%d.cat" % i, torch.cat(cat, 1))
            y3 = _conv_bn(sd, p + ".conv3", p + ".bn3", cat)
            res = out
            if p + ".shortcut.0.weight" in sd:
                res = _conv_bn(sd, p + ".shortcut.0", p + ".shortcut.1", out, stride=stride)
                mid["b%d.sc" % i] = res
            out = replaced("b%d.block" % i, act(y3 + res))
            mid["b%d.mid" % i], mid["b%d.cat" % i], mid["b%d.block" % i] = y1, cat, out
        stage_out.append(out)
    prev = stage_out[0]
    for k, fn in enumerate(("fuse_mode12", "fuse_mode123", "fuse_mode1234")):
        ds = F.conv2d(prev, _t(sd, "layer%d_downsample.weight" % (k + 1)), None, stride=2, padding=1)
        prev = fuse(fn, stage_out[k + 1], ds)
        mid[fn.replace("_mode", "")] = prev
    xs = prev.reshape(prev.shape[0], -1, prev.shape[-1])
    pooled = torch.cat([xs.mean(dim=-1), torch.sqrt(xs.var(dim=-1) + 1e-7)], dim=-1)   # pooling_layers.py:78-85
    mid["pooled"] = pooled
    emb = F.linear(pooled, _t(sd, "seg_1.weight"), _t(sd, "seg_1.bias"))
    if "seg_2.weight" in sd:
        h = _bn(sd, "seg_bn_1", F.relu(emb))                # BatchNorm1d(affine=False), eres2net.py:331
        mid["emb_a"] = h
        emb = F.linear(h, _t(sd, "seg_2.weight"), _t(sd, "seg_2.bias"))
    return (emb, mid) if return_intermediates else emb

