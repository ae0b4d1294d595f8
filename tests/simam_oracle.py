"""ORACLE (test infrastructure, never shipped): float64 restatement of the reference's SimAM_ResNet34_ASP /
SimAM_ResNet100_ASP forward as one straight-line function over a state_dict.

Follows (file:line in the reference, wenet-e2e/wespeaker):
  wespeaker/models/samresnet.py:142-149   forward: (B,T,F) -> permute -> unsqueeze -> front -> pooling -> bottleneck
  wespeaker/models/samresnet.py:117-123   ResNet.forward (conv1 + bn1 + relu, layer1..4)
  wespeaker/models/samresnet.py:100-115   _make_layer (the first block of a stage carries the stride)
  wespeaker/models/samresnet.py:57-63     SimAMBasicBlock.forward (conv-bn-relu, conv-bn, SimAM, += downsample, relu)
  wespeaker/models/samresnet.py:65-70     SimAM: n = H*W - 1, d = (X - mean)^2, v = sum d / n, X * sigmoid(d / (4 (v + 1e-4)) + 0.5)
  wespeaker/models/pooling_layers.py:180-186 ASP attention: Conv1d, ReLU, BatchNorm1d, Conv1d, Softmax(dim=2)
  wespeaker/models/pooling_layers.py:188-204 ASP.forward: reshape (B, C*F, T), mu = sum x w, sg = sqrt(clamp(sum x^2 w - mu^2, 1e-5))
PINNED by tests/golden/samresnet_ref.npz (outputs of the reference's own nn.Module, tools/make_golden_simam.py) and,
where the reference is present, by a live comparison (tests/test_samresnet_cpu.py).
"""
import torch
import torch.nn.functional as F

from oracle.ecapa import _bn, _t
from oracle.resnet import _conv_bn

LAYOUTS = {"SimAM_ResNet34_ASP": [3, 4, 6, 3], "SimAM_ResNet100_ASP": [6, 16, 24, 3]}     # samresnet.py:126-131
LAMBDA = 1e-4                                                                               # samresnet.py:65


def _cast(sd, dtype):
    out = {}
    for k, v in sd.items():
        t = torch.as_tensor(v)
        out[k] = t.to(dtype) if t.is_floating_point() else t
    return out


def simam(x, lambda_p=LAMBDA):
    n = x.shape[2] * x.shape[3] - 1
    d = (x - x.mean(dim=[2, 3], keepdim=True)).pow(2)
    v = d.sum(dim=[2, 3], keepdim=True) / n
    return x * torch.sigmoid(d / (4 * (v + lambda_p)) + 0.5)


def _block(sd, p, x, stride, mid=None, taps=None):
    out = F.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", x, stride=stride, padding=1))
    y = _conv_bn(sd, p + ".conv2", p + ".bn2", out, padding=1)
    sc = x
    if p + ".downsample.0.weight" in sd:
        sc = _conv_bn(sd, p + ".downsample.0", p + ".downsample.1", x, stride=stride)
        if taps is not None:
            taps["sc"] = sc
    if mid is not None:
        mid["block1_y"], mid["block1_res"] = y, sc
    res = F.relu(simam(y) + sc)
    if taps is not None:
        taps["mid"], taps["block"] = out, res
    return res


def asp(sd, x, mid=None):
    """x (B, C, F, T) -> (B, 2 C F)."""
    x = x.reshape(x.size(0), -1, x.size(-1))
    h = F.relu(F.conv1d(x, _t(sd, "pooling.attention.0.weight"), _t(sd, "pooling.attention.0.bias")))
    if mid is not None:
        mid["hid"] = h
    h = _bn(sd, "pooling.attention.2", h)
    e = F.conv1d(h, _t(sd, "pooling.attention.3.weight"), _t(sd, "pooling.attention.3.bias"))
    w = torch.softmax(e, dim=2)
    mu = torch.sum(x * w, dim=2)
    sg = torch.sqrt((torch.sum((x ** 2) * w, dim=2) - mu ** 2).clamp(min=1e-5))
    if mid is not None:
        mid["logits"] = e
    return torch.cat([mu, sg], dim=1)


@torch.no_grad()
def simam_resnet_forward(sd, feats, model_name="SimAM_ResNet34_ASP", return_intermediates=False, dtype=torch.float64):
    """feats (B, T, F) -> embedding (B, E) in `dtype` (float64: the ground truth; float32: what a faithful fp32
    implementation computes).  return_intermediates: also a dict with `block1` (the first block's output, (B, C, F, T)),
    `block1_y` / `block1_res` (what its SimAM gate and residual add read: conv2 + bn2, and the block input), `pooled`
    (the ASP vector, (B, 2D)), `logits` (the attention logits, (B, D, T')), `hid` (the first attention layer after its
    ReLU, before the BatchNorm1d, (B, 128, T')), `stem` (B, C, F, T) and, for the i-th residual block (1-based), `b<i>.mid`
    (conv1 + bn1 + relu), `b<i>.block` (the gated result), `b<i>.sc` where the block has a downsample convolution."""
    blocks = LAYOUTS[model_name]
    sd = _cast(sd, dtype)
    x = torch.as_tensor(feats).to(dtype).permute(0, 2, 1).unsqueeze(1)
    out = F.relu(_conv_bn(sd, "front.conv1", "front.bn1", x, padding=1))
    mid = {"stem": out}
    i = 0
    for s, nb in enumerate(blocks):
        for b in range(nb):
            stride = (1 if s == 0 else 2) if b == 0 else 1
            first = s == 0 and b == 0
            taps = {}
            out = _block(sd, "front.layer%d.%d" % (s + 1, b), out, stride, mid if first else None, taps)
            i += 1
            mid.update({"b%d.%s" % (i, k): v for k, v in taps.items()})
            if first:
                mid["block1"] = out
    pooled = asp(sd, out, mid)
    mid["pooled"] = pooled
    emb = F.linear(pooled, _t(sd, "bottleneck.weight"), _t(sd, "bottleneck.bias"))
    return (emb, mid) if return_intermediates else emb
