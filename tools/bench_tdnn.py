#!/usr/bin/env python
"""Forward throughput of the x-vector / xi-vector engines at the flagship batch (256 utterances x 2 s = 200 frames,
fp32), with plain ECAPA_TDNN_c512 measured in the same process for comparison: one JSON line per model, appended to
profiles/tdnn_bench.jsonl.  Weights are the seeded synthetic ones of tools/make_golden_tdnn.py / fixtures/synth.py.

    python tools/bench_tdnn.py [--steps 20] [--warmup 5] [--models XVEC XI_VEC_ECAPA_TDNN_c512 ECAPA_TDNN_c512]

Each figure is the median of `steps` forwards timed one by one with stream events (no host time inside), behind
`warmup` untimed ones; the per-class split is the engine's own event profile of ONE further forward
(NativeSpeakerModel.profile: gemm_main / gemm_narrow / reduce_elementwise / gemm_splitk -- xi_pool_kernel and TSTP are
the reduce_elementwise launches of these models' tails)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_tdnn as mg  # noqa: E402
from fixtures import synth  # noqa: E402


def state_dict(name, embed_dim):
    if name in (mg.XVEC, mg.XI_XVEC):
        return mg.synth_xvec_state_dict(name, 80, embed_dim)
    if name.startswith("XI_VEC_"):
        return mg.synth_xi_ecapa_state_dict(name, 80, embed_dim)
    return synth.synth_state_dict(name, 80, embed_dim, seed=42)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=[mg.XVEC, mg.XI_C512, "ECAPA_TDNN_c512"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tdnn_bench.jsonl"))
    args = ap.parse_args()
    from wespeaker_amd.engine import NativeSpeakerModel
    feats = torch.from_numpy(np.random.RandomState(0).randn(args.batch, args.frames, 80).astype(np.float32)).cuda()
    lines = []
    for name in args.models:
        E = 512 if name in (mg.XVEC, mg.XI_XVEC) else 192
        model = NativeSpeakerModel(name, state_dict(name, E), feat_dim=80, embed_dim=E, max_batch=args.batch,
                                   max_frames=args.frames)
        for _ in range(args.warmup):
            model.embed(feats)
        ms = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            emb = model.embed(feats)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        assert bool(torch.isfinite(emb).all())
        model.profile(True)
        model.embed(feats)
        classes = model.profile_read()
        model.profile(False)
        med = float(np.median(ms))
        rec = {"model": name, "precision": "fp32", "batch": args.batch, "frames": args.frames, "steps": args.steps,
               "step_ms_median": med, "step_ms_min": float(min(ms)), "utt_per_s": args.batch / med * 1e3,
               "tflops": model.flops(args.batch, args.frames) / med / 1e9, "classes": classes}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del model
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
