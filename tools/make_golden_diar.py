"""Writes tests/golden/diar_ref.npz: what the reference's spectral clusterer and segment merger answer on the
seeded fixtures of tests/diar_oracle.py, next to the float64 quantities the tests bound their errors with.

    python tools/make_golden_diar.py

Needs the reference checkout (oracle/ref_shim.py) with scipy and sklearn; the reference's `cluster` and
`merge_segments` are imported and called, nothing of them is restated here.  The embeddings themselves are not
stored: tests regenerate them from the fixture's seed, and the golden holds a checksum to catch a generator that
drifted.

Per fixture <f>: <f>_labels (the reference's labels; five calls must agree up to a permutation), <f>_num_spks,
<f>_lam / <f>_vec (float64 eigenvalues / eigenvectors [:K] of the float64 graph, K = min(21, n)),
<f>_gaps (largest and second largest entry of diff(lam[:K]), and lam[k] - lam[k-1] at the cut),
<f>_eig_err32 (the reference-float32 eigenvalues' largest distance from float64), <f>_aff_err32 (same for its
affinity), <f>_min_gap (smallest float64 distance between a row's last kept and first dropped affinity) and
<f>_checksum.  The tool refuses a fixture whose float32 graph differs from the float64 one in a row the
8 x aff_err32 rule does not excuse, or in more than 2 % of the rows, and -- stronger, so that the golden
eigenvalues are those of the one graph every correct float32 pipeline builds -- one whose <f>_min_gap is not
above 8 x aff_err32: change the fixture's seed then."""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diar_oracle as do  # noqa: E402
from oracle import ref_shim  # noqa: E402

MERGE_CASES = [
    [["a", [[0.0, 1.5, "0"]]]],                                                     # one window: the `e` quirk
    [["a", [[0.0, 1.5, "0"], [0.75, 2.25, "0"], [1.5, 3.0, "1"], [2.25, 3.75, "1"]]]],   # pivot between speakers
    [["a", [[0.0, 1.5, "0"], [0.75, 2.25, "1"], [1.5, 3.0, "0"]]]],                 # two pivots in a row
    [["a", [[0.0, 1.5, "0"], [4.0, 5.5, "0"], [4.75, 6.25, "1"]]], ["b", [[1.0, 2.0, "2"], [2.0, 3.0, "2"]]]],
    [["a", [[0.0, 1.0, "1"], [1.0, 2.0, "0"], [3.0, 3.2, "0"]]], ["empty", []]],    # touching windows, a gap, no windows
    [["a", [[0.0, 1.5, "0"], [0.75, 2.25, "1"], [5.0, 6.0, "1"]]]],                 # the last turn ends at the last window
]


def ref_diar(module):
    ref_shim._seed_packages()
    if "wespeaker.diar" not in sys.modules:
        pkg = types.ModuleType("wespeaker.diar")
        pkg.__path__ = [os.path.join(ref_shim.REF_ROOT, "wespeaker", "diar")]
        sys.modules["wespeaker.diar"] = pkg
    return ref_shim.ref_module("wespeaker.diar." + module)


def main():
    import scipy.linalg
    clusterer = ref_diar("spectral_clusterer")
    rttm = ref_diar("make_rttm")
    out = {}
    for name in do.FIXTURES:
        emb, truth = do.make_fixture(name)
        n = len(emb)
        K = min(21, n)
        runs = [np.asarray(clusterer.cluster(emb.copy())) for _ in range(5)]
        for r in runs[1:]:
            assert do.same_partition(runs[0], r), "%s: the reference's own labels are not stable" % name
        if not name.startswith("n15"):                  # (n15, n15m are chosen for their near-tie of gaps, not for truth)
            assert do.same_partition(runs[0], truth), "%s: the reference does not recover the truth" % name
        o64 = do.oracle(emb)
        o32 = do.oracle(emb, dtype=np.float32)
        aff_err = float(np.abs(o32["S"].astype(np.float64) - o64["S"]).max())
        lam32 = scipy.linalg.eigh(o32["L"].astype(np.float32), eigvals_only=True)
        eig_err = float(np.abs(lam32.astype(np.float64) - o64["lam"]).max())
        hi, lo = do.boundary_gaps(o64["S"], o64["keep"])
        min_gap = float((hi - lo).min())
        rows, bad = do.excused_rows(o32["P"], o64["P"], o64["S"], o64["keep"], 8 * aff_err)
        assert not bad and len(rows) <= 0.02 * n, "%s: float32 graph outside the rule (%s); change the seed" % (name, bad)
        assert min_gap > 8 * aff_err, "%s: min boundary gap %.3e <= 8 x %.3e; change the seed" % (name, min_gap, aff_err)
        lam = o64["lam"][:K]
        k = do.choose(lam)
        assert k == len(set(runs[0].tolist())), (name, k)
        d = np.sort(np.diff(lam))[::-1]
        out[name + "_labels"] = runs[0].astype(np.int64)
        out[name + "_num_spks"] = np.int64(k)
        out[name + "_lam"] = lam
        out[name + "_vec"] = o64["V"][:, :K]
        out[name + "_gaps"] = np.array([d[0] if d.size else 0.0, d[1] if d.size > 1 else 0.0,
                                        o64["lam"][k] - o64["lam"][k - 1]])
        out[name + "_eig_err32"] = np.float64(eig_err)
        out[name + "_aff_err32"] = np.float64(aff_err)
        out[name + "_min_gap"] = np.float64(min_gap)
        out[name + "_checksum"] = np.array([emb.astype(np.float64).sum(), np.abs(emb.astype(np.float64)).sum()])
        print("%-6s n=%4d k=%d zero-eigenvalues=%d aff_err32=%.2e eig_err32=%.2e min_gap=%.2e excused=%d"
              % (name, n, k, int((lam < 1e-9).sum()), aff_err, eig_err, min_gap, len(rows)))
    cases = []
    for case in MERGE_CASES:
        inp = {utt: [tuple(s) for s in subsegs] for utt, subsegs in case}
        merged = rttm.merge_segments(inp)
        # the label file that read_labels turns into `inp`-like input, and the RTTM text the reference prints for it
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "labels")
            lines = []
            for utt, subsegs in case:
                for (b, e, la) in subsegs:
                    lines.append("%s-%08d-%08d-%08d-%08d %s" % (utt, int(b * 1000), int(e * 1000), 0,
                                                                 int(round((e - b) * 100)), la))
            with open(path, "w") as f:
                f.write("\n".join(lines) + "\n")
            read = rttm.read_labels(path)
            argv, sys.argv = sys.argv, ["make_rttm.py", "--labels", path, "--channel", "2"]
            buf = io.StringIO()
            try:
                with contextlib.redirect_stdout(buf):
                    rttm.main()
            finally:
                sys.argv = argv
        cases.append({"input": case, "merged": [list(m) for m in merged], "label_lines": lines,
                      "read": [[utt, [list(s) for s in v]] for utt, v in read.items()],
                      "rttm_channel2": buf.getvalue()})
    out["merge_cases_json"] = np.array(json.dumps(cases))
    path = os.path.join(ROOT, "tests", "golden", "diar_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
