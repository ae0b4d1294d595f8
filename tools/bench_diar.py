"""Times wespeaker_amd.diar.cluster on the GPU, stage by stage, beside the reference clusterer on the host.

    python tools/bench_diar.py [--sizes 1030 2000 4800] [--out profiles/diar_cluster.jsonl]
                               [--reference | --merge-reference profiles/diar_cluster_reference_host.jsonl]

One JSON line per size (the output file is rewritten, not appended to): n, keep, nnz, sweeps, kernel launches of
the solve, wall times of the graph stage, the eigen-solve and the k-means (device stages bracketed by events on the
stream, host stages by perf_counter), the total, and the reference's `cluster()` on one host thread -- timed here
with --reference where the reference checkout, scipy and sklearn exist, or taken with --merge-reference from the rows
an earlier `--no-gpu --reference --out FILE` run wrote on a machine that has them (the machine with the GPU has no
reference checkout; merged rows say so in `reference_host_from`).  Embeddings: five speakers of unit-variance noise
around random centres in 256 dimensions.  No speed-up is asserted anywhere: this writes what it measures."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def embeddings(n, seed=7):
    rng = np.random.default_rng(seed)
    sizes = np.array([0.29, 0.24, 0.2, 0.15, 0.12]) * n
    sizes = sizes.astype(int)
    sizes[0] += n - sizes.sum()
    centres = rng.standard_normal((5, 256))
    truth = np.repeat(np.arange(5), sizes)
    emb = centres[truth] + rng.standard_normal((n, 256))
    order = rng.permutation(n)
    return emb[order].astype(np.float32), truth[order]


def time_gpu(emb, repeats):
    import torch
    from wespeaker_amd import diar
    best = None
    for _ in range(repeats + 1):                       # the first pass warms the allocator and the code objects
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        graph = diar.Graph(emb)
        ev[1].record()
        stats = {}
        lam, vec = diar._solve(graph, graph.n, min(diar.BLOCK, graph.n), graph.max_deg, min(21, graph.n), stats=stats)
        ev[2].record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        k = diar.choose_num_spks(lam)
        labels = diar.kmeans(vec[:, :k], k, 0)
        t2 = time.perf_counter()
        row = dict(n=graph.n, keep=graph.keep, nnz=graph.nnz, max_deg=graph.max_deg, num_spks=int(k),
                   sweeps=stats["sweeps"], launches=stats["launches"], worst_residual=stats["worst_residual"],
                   residual_bound=float(stats["bound"]), graph_ms=ev[0].elapsed_time(ev[1]),
                   solve_ms=ev[1].elapsed_time(ev[2]), kmeans_ms=(t2 - t1) * 1e3, total_ms=(t2 - t0) * 1e3)
        if best is None or row["total_ms"] < best[0]["total_ms"]:
            best = (row, labels)
    return best


def time_reference(emb):
    from oracle import ref_shim
    import types
    ref_shim._seed_packages()
    if "wespeaker.diar" not in sys.modules:
        pkg = types.ModuleType("wespeaker.diar")
        pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "wespeaker", "diar")]
        sys.modules["wespeaker.diar"] = pkg
    mod = ref_shim.ref_module("wespeaker.diar.spectral_clusterer")
    t0 = time.perf_counter()
    labels = mod.cluster(emb.copy())
    return (time.perf_counter() - t0) * 1e3, np.asarray(labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1030, 2000, 4800])
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--reference", action="store_true", help="also time the reference's cluster() on the host")
    ap.add_argument("--no-gpu", action="store_true", help="reference timings only (a machine without a GPU)")
    ap.add_argument("--merge-reference", default=None, metavar="FILE",
                    help="take reference_host_ms per n from the rows of an earlier --no-gpu --reference run")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diar_cluster.jsonl"))
    args = ap.parse_args()
    import diar_oracle as do
    merged = {}
    if args.merge_reference:
        with open(args.merge_reference) as f:
            merged = {r["n"]: r for r in map(json.loads, filter(str.strip, f))}
    with open(args.out, "w") as f:
        for n in args.sizes:
            emb, truth = embeddings(n)
            row = {"n": n}
            if not args.no_gpu:
                row, labels = time_gpu(emb, args.repeats)
                row["recovers_truth"] = bool(do.same_partition(labels, truth))
            if args.reference:
                ms, ref_labels = time_reference(emb)
                row["reference_host_ms"] = ms
                row["reference_recovers_truth"] = bool(do.same_partition(ref_labels, truth))
            if n in merged:
                row["reference_host_ms"] = merged[n]["reference_host_ms"]
                row["reference_recovers_truth"] = merged[n]["reference_recovers_truth"]
                row["reference_host_from"] = os.path.basename(args.merge_reference)
            line = json.dumps(row)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
