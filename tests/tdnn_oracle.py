"""Test oracle (never shipped): a float64 restatement, over a state dict, of the reference's TDNN x-vector
(wespeaker/models/tdnn.py:23-115), of XI pooling (pooling_layers.py:344-416, stddev=False) and of the xi-vector ECAPA
models (xi_vector.py:31-44: the ECAPA-TDNN trunk of oracle/ecapa.py up to `h`, then XI, bn, linear [, bn2]).

dtype=torch.float32 evaluates the same functions in single precision: the yardstick of the per-tap bars
(tests/test_gpu_layers.py: tap_check).  tests/test_tdnn_cpu.py pins these functions to the reference's own modules and
to tests/golden/tdnn_ref.npz.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ecapa as eo

TAPS = (5, 3, 3, 1, 1)
DILATIONS = (1, 2, 3, 1, 1)
TRIM = (2, 4, 7, 7, 7)             # frames a "same"-padded layer k has on each side beyond the reference's valid ones


def _cast(sd, dtype):
    return {k: (torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v))
            for k, v in sd.items()}


def xi_logprec(z):
    """pooling_layers.py:380-386 behind lin2: softplus (beta 1, threshold 20) -> 2 log -> clamp to [-15, 15]."""
    return (2.0 * torch.log(F.softplus(z, beta=1, threshold=20))).clamp(min=-15.0, max=15.0)


def xi_posterior_mean(x, z, prior_mean, prior_logprec):
    """pooling_layers.py:389-401 with stddev=False.  x, z: (B, D, T); the priors (1, D) -> phi (B, D)."""
    lp = torch.cat((xi_logprec(z), prior_logprec.repeat(z.shape[0], 1).unsqueeze(2)), 2)
    w = torch.softmax(lp, dim=2)
    return torch.sum(torch.cat((x, prior_mean.repeat(x.shape[0], 1).unsqueeze(2)), 2) * w, dim=2)


def xi_pool(sd, prefix, x, taps=None):
    """XI.forward.  taps: xi_hid = lin1 + ReLU (before its BatchNorm, which the engines fold into lin2), xi_z = lin2."""
    h = F.relu(F.conv1d(x, eo._t(sd, prefix + ".lin1_relu_bn.0.weight"), eo._t(sd, prefix + ".lin1_relu_bn.0.bias")))
    z = F.conv1d(eo._bn(sd, prefix + ".lin1_relu_bn.2", h), eo._t(sd, prefix + ".lin2.weight"), eo._t(sd, prefix + ".lin2.bias"))
    if taps is not None:
        taps["xi_hid"], taps["xi_z"] = h, z
    return xi_posterior_mean(x, z, eo._t(sd, prefix + ".prior_mean"), eo._t(sd, prefix + ".prior_logprec"))


def prior_weight(z, prior_logprec):
    """The softmax weight of the prior pseudo-frame per (utterance, channel): z (B, D, T), prior_logprec (1, D)."""
    lp = torch.cat((xi_logprec(z), prior_logprec.repeat(z.shape[0], 1).unsqueeze(2)), 2)
    return torch.softmax(lp, dim=2)[:, :, -1]


@torch.no_grad()
def xvec_forward(sd, feats, dtype=torch.float64, return_intermediates=False):
    """(B, T, F) -> embed_b (B, E) [, dict]: frame1 .. frame5 (B, C, T_k: the VALID convolutions' outputs after ReLU and
    BN), pooled, emb_a and -- XI -- xi_hid, xi_z (B, ., T - 14).  XI is recognised by pool.prior_mean."""
    sd = _cast(sd, dtype)
    x = torch.as_tensor(feats).to(dtype).permute(0, 2, 1)
    mid = {}
    for k in range(5):
        p = "frame_%d" % (k + 1)
        x = F.conv1d(x, eo._t(sd, p + ".conv_1d.weight"), eo._t(sd, p + ".conv_1d.bias"), dilation=DILATIONS[k])
        x = eo._bn(sd, p + ".bn", F.relu(x))
        mid["frame%d" % (k + 1)] = x
    pooled = xi_pool(sd, "pool", x, mid) if "pool.prior_mean" in sd else eo.tstp(x)
    emb_a = F.linear(pooled, eo._t(sd, "seg_1.weight"), eo._t(sd, "seg_1.bias"))
    emb_b = F.linear(eo._bn(sd, "seg_bn_1", F.relu(emb_a)), eo._t(sd, "seg_2.weight"), eo._t(sd, "seg_2.bias"))
    mid["pooled"] = pooled
    # the engine's emb_a tap is what seg_2 reads: seg_1 -> ReLU -> seg_bn_1 (one GEMM epilogue)
    mid["emb_a"] = eo._bn(sd, "seg_bn_1", F.relu(emb_a))
    return (emb_b, mid) if return_intermediates else emb_b


@torch.no_grad()
def xi_ecapa_forward(sd, feats, dtype=torch.float64, return_intermediates=False):
    """XI_VEC_ECAPA_TDNN_*: oracle/ecapa.py's trunk functions as they are (layer1 .. layer4, cat, conv, ReLU), then XI over
    the whole utterance, bn (1536), linear [, bn2]."""
    sd = _cast(sd, dtype)
    x = torch.as_tensor(feats).to(dtype).permute(0, 2, 1)
    out1 = eo._conv_relu_bn(sd, "layer1", x, padding=2)
    out2 = eo._se_res2block(sd, "layer2", out1, 2)
    out3 = eo._se_res2block(sd, "layer3", out2, 3)
    out4 = eo._se_res2block(sd, "layer4", out3, 4)
    h = F.relu(F.conv1d(torch.cat([out2, out3, out4], dim=1), eo._t(sd, "conv.weight"), eo._t(sd, "conv.bias")))
    mid = {"out1": out1, "out2": out2, "out3": out3, "out4": out4, "h": h}
    pooled = xi_pool(sd, "pool", h, mid)
    emb = F.linear(eo._bn(sd, "bn", pooled), eo._t(sd, "linear.weight"), eo._t(sd, "linear.bias"))
    if "bn2.running_mean" in sd:
        emb = eo._bn(sd, "bn2", emb)
    mid["pooled"] = pooled
    return (emb, mid) if return_intermediates else emb


def forward(name, sd, feats, **kw):
    return (xvec_forward if name in ("XVEC", "XI_VEC_XVEC") else xi_ecapa_forward)(sd, feats, **kw)


def xi_pool_windows(x, z, prior_mean, prior_logprec, windows, dtype=np.float64):
    """The formula of csrc/xi_pool.hip in plain numpy, evaluated in `dtype`: x, z (B, T, D) rows, windows [(t0, n)] per
    utterance -> (B, D).  float32: np.log1p / np.exp / np.log on float32 arrays stay float32."""
    x, z = np.asarray(x, dtype=dtype), np.asarray(z, dtype=dtype)
    pm, pl = np.asarray(prior_mean, dtype=dtype).reshape(-1), np.asarray(prior_logprec, dtype=dtype).reshape(-1)
    out = np.empty((x.shape[0], x.shape[2]), dtype=dtype)
    with np.errstate(divide="ignore", over="ignore"):
        for b, (t0, n) in enumerate(windows):
            zz, xx = z[b, t0:t0 + n], x[b, t0:t0 + n]
            sp = np.where(zz > 20, zz, np.log1p(np.exp(np.minimum(zz, dtype(30)))))
            lp = np.clip(dtype(2) * np.log(sp), dtype(-15), dtype(15))
            m = np.maximum(lp.max(axis=0), pl)
            w, wp = np.exp(lp - m), np.exp(pl - m)
            out[b] = ((w * xx).sum(axis=0) + wp * pm) / (w.sum(axis=0) + wp)
    return out
