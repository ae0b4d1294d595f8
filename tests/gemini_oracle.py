"""ORACLE (test infrastructure, never shipped): float64 restatement of the reference's Gemini_DF_ResNet60 / 114 / 183 /
237 forward as one straight-line function over a state_dict.

Follows (file:line in the reference, wenet-e2e/wespeaker):
  wespeaker/models/gemini_dfresnet.py:30-48     Inverted_Bottleneck.forward (1x1, depthwise 3x3, 1x1, += x, relu)
  wespeaker/models/gemini_dfresnet.py:66-85     the stem and the four downsample layers: strides (2,1) (2,2) (2,1) (2,1)
                                                 on (frequency, time), BatchNorm, NO activation
  wespeaker/models/gemini_dfresnet.py:105-141   _get_frame_level_feat + forward (TSTP, seg_1 [, relu, seg_bn_1, seg_2])
  wespeaker/models/pooling_layers.py:78-85      TSTP
PINNED by tests/golden/gemini_ref.npz (outputs of the reference's own nn.Module, tools/make_golden_gemini.py) and, where
the reference is present, by a live comparison (tests/test_gemini_cpu.py).

`transpose_dw`, `ds_relu` and `ds1_stride_t` exist for the fixtures with teeth of the tests: what an implementation that
swapped the depthwise filter's frequency and time taps, rectified a downsample layer's output, or strode the first
downsample layer over time as well would compute.
"""
import torch
import torch.nn.functional as F

from oracle.ecapa import _bn, _t

LAYOUTS = {      # gemini_dfresnet.py:145-178
    "Gemini_DF_ResNet60": (3, 3, 9, 3), "Gemini_DF_ResNet114": (3, 3, 27, 3),
    "Gemini_DF_ResNet183": (3, 8, 45, 3), "Gemini_DF_ResNet237": (3, 8, 63, 3),
}
STRIDE_T = (1, 2, 1, 1)


def _cast(sd, dtype):
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def stop_points(name):
    """The engine's stop points after the stem, in forward order: ("ds", layer 1..4) or ("block", stage, index)."""
    out = []
    for s, nb in enumerate(LAYOUTS[name]):
        out.append(("ds", s + 1))
        out += [("block", s, b) for b in range(nb)]
    return out


@torch.no_grad()
def gemini_forward(sd, feats, name="Gemini_DF_ResNet60", dtype=torch.float64, return_intermediates=False,
                   transpose_dw=False, ds_relu=False, ds1_stride_t=1):
    """feats (B, T, F) -> embedding (B, E) in `dtype` (the LAST element of the reference's tuple).
    return_intermediates: also a dict of (B, C, F, T) maps keyed like the engine's stop points -- `stem`; `u<n>.ds` for
    stop point n when it is a downsample layer, else `u<n>.exp` (conv1 + bn1 + relu), `u<n>.dw` (conv2 + bn2 + relu) and
    `u<n>.block`; `pooled` (B, 2D); `emb_a` (two-layer models: relu + seg_bn_1 of seg_1's output, what seg_2 reads)."""
    sd = _cast(sd, dtype)
    mid = {}
    x = torch.as_tensor(feats).to(dtype).permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_bn(sd, "downsample_layers.0.1", F.conv2d(x, _t(sd, "downsample_layers.0.0.weight"), None, padding=1)))
    mid["stem"] = out
    n = 0
    for s, nb in enumerate(LAYOUTS[name]):
        n += 1
        p = "downsample_layers.%d" % (s + 1)
        st = ds1_stride_t if s == 0 else STRIDE_T[s]
        out = _bn(sd, p + ".1", F.conv2d(out, _t(sd, p + ".0.weight"), None, stride=(2, st), padding=1))
        if ds_relu:
            out = F.relu(out)
        mid["u%d.ds" % n] = out
        for b in range(nb):
            n += 1
            p = "stages.%d.%d" % (s, b)
            c = out.shape[1] * 4
            e = F.relu(_bn(sd, p + ".bn1", F.conv2d(out, _t(sd, p + ".conv1.weight"))))
            w2 = _t(sd, p + ".conv2.weight")
            if transpose_dw:
                w2 = w2.transpose(2, 3)
            d = F.relu(_bn(sd, p + ".bn2", F.conv2d(e, w2, None, padding=1, groups=c)))
            out = F.relu(_bn(sd, p + ".bn3", F.conv2d(d, _t(sd, p + ".conv3.weight"))) + out)
            mid["u%d.exp" % n], mid["u%d.dw" % n], mid["u%d.block" % n] = e, d, out
    xs = out.reshape(out.shape[0], -1, out.shape[-1])
    pooled = torch.cat([xs.mean(dim=-1), torch.sqrt(xs.var(dim=-1) + 1e-7)], dim=-1)   # pooling_layers.py:78-85
    mid["pooled"] = pooled
    emb = F.linear(pooled, _t(sd, "seg_1.weight"), _t(sd, "seg_1.bias"))
    if "seg_2.weight" in sd:
        h = _bn(sd, "seg_bn_1", F.relu(emb))                # BatchNorm1d(affine=False), gemini_dfresnet.py:99
        mid["emb_a"] = h
        emb = F.linear(h, _t(sd, "seg_2.weight"), _t(sd, "seg_2.bias"))
    return (emb, mid) if return_intermediates else emb
