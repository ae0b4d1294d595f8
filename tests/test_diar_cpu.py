"""CPU: the host half of the diarization back end (wespeaker_amd/diar.py) against tests/golden/diar_ref.npz, which
tools/make_golden_diar.py recorded from the reference's own `cluster` / `merge_segments` / make_rttm.py.

No GPU here: segment merging, label files and RTTM text byte for byte; the pruning count; the host k-means on the
golden's float64 eigenvectors (and on a rotated basis of the same subspace); the float64 oracle of
tests/diar_oracle.py against the golden eigenvalues; the solver's host logic on dense numpy panels; and the
teeth -- four wrong clusterers that the golden must be able to tell from the right one."""
import functools
import json
import os

import numpy as np
import pytest

import diar_oracle as do
from wespeaker_amd import diar

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diar_ref.npz")
NAMES = list(do.FIXTURES)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def fixture(name):
    emb, truth = do.make_fixture(name)
    emb.setflags(write=False)
    return emb, truth


@functools.lru_cache(maxsize=None)
def oracle(name):
    return do.oracle(fixture(name)[0])


def merge_cases():
    return json.loads(str(golden()["merge_cases_json"]))


def test_fixture_generator_has_not_drifted():
    g = golden()
    for name in NAMES:
        emb = fixture(name)[0].astype(np.float64)
        np.testing.assert_allclose([emb.sum(), np.abs(emb).sum()], g[name + "_checksum"], rtol=1e-12)


def test_merge_segments_matches_the_reference():
    for case in merge_cases():
        inp = {utt: [tuple(s) for s in subsegs] for utt, subsegs in case["input"]}
        got = diar.merge_segments(inp)
        assert [list(m) for m in got] == case["merged"]


def test_read_labels_and_rttm_lines_byte_for_byte(tmp_path, capsys):
    for i, case in enumerate(merge_cases()):
        path = tmp_path / ("labels%d" % i)
        path.write_text("\n".join(case["label_lines"]) + "\n")
        read = diar.read_labels(str(path))
        assert [[utt, [list(s) for s in v]] for utt, v in read.items()] == case["read"]
        # the command line of diar/make_rttm.py
        assert diar.main(["rttm", "--labels", str(path), "--channel", "2"]) == 0
        assert capsys.readouterr().out == case["rttm_channel2"]
        # Speaker.make_rttm's file form (channel 1, cli/speaker.py:283-289)
        out = tmp_path / ("rttm%d" % i)
        diar.make_rttm(diar.merge_segments(read), str(out))
        want = case["rttm_channel2"].splitlines()
        got = out.read_text().splitlines()
        assert len(got) == len(want)
        for a, b in zip(got, want):
            fa, fb = a.split(" "), b.split(" ")
            assert fa[2] == "1" and fb[2] == "2" and fa[:2] + fa[3:] == fb[:2] + fb[3:]


def test_single_subsegment_keeps_the_reference_quirk():
    assert diar.merge_segments({"u": [(1.0, 2.5, 3)]}) == [("u", 1.0, 2.5, 3)]
    assert diar.merge_segments({"u": []}) == []


def test_window_times_with_and_without_an_utterance_prefix():
    assert diar.window_times("rec-00001230-00004000-00000075-00000225") == ("rec", 1.98, 3.48)
    assert diar.window_times("00001230-00004000-00000000-00000150", frame_shift=20) == ("", 1.23, 4.23)
    with pytest.raises(ValueError):
        diar.window_times("rec-12")


@pytest.mark.parametrize("m", [3, 11, 12, 999, 1000, 1001, 8192])
def test_spectral_keep_rule(built_lib, m):
    low = max(m - 10, 2) if m < 1000 else int((1.0 - .01) * m)      # spectral_clusterer.py:40-44
    assert built_lib.ws_spectral_keep(m, .01) == m - low == do.keep_rule(m)
    assert diar.spectral_keep(m) == m - low
    if m >= 1000:
        assert built_lib.ws_spectral_keep(m, .05) == m - int((1.0 - .05) * m)
        assert built_lib.ws_spectral_keep(m, 2.0) == m and built_lib.ws_spectral_keep(m, -1.0) == 0


def test_spectral_entry_points_refuse_bad_sizes_on_the_host(built_lib):
    assert built_lib.ws_spectral_scratch(8193, 256) == 0 and built_lib.ws_spectral_scratch(2, 256) == 0
    assert built_lib.ws_spectral_scratch(8192, 256) >= 8192 * 8192 * 4
    assert built_lib.ws_spectral_apply(None, None, None, None, 100, 8, 1.0, 0.0, 0.0, None, None, None, None) == -1


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_golden_eigenvalues_and_count(name):
    g = golden()
    o = oracle(name)
    K = min(21, len(fixture(name)[0]))
    np.testing.assert_allclose(o["lam"][:K], g[name + "_lam"], rtol=0, atol=1e-10)
    assert do.choose(o["lam"][:K]) == int(g[name + "_num_spks"])
    if name == "n120":
        assert int((g[name + "_lam"] < 1e-9).sum()) == 3            # three components: a triple zero eigenvalue
    if name == "n3":
        assert not o["L"].any()                                     # keep = 1: the diagonal only, an empty graph


@pytest.mark.parametrize("name", NAMES)
def test_kmeans_recovers_the_golden_partition(name):
    g = golden()
    k = int(g[name + "_num_spks"])
    vec = g[name + "_vec"][:, :k]
    for seed in (0, 1):
        assert do.same_partition(diar.kmeans(vec, k, seed), g[name + "_labels"])
    # any orthonormal basis of the same subspace must do: the eigen-solver owes the subspace, not the vectors
    q, _ = np.linalg.qr(np.random.default_rng(5).standard_normal((k, k)))
    assert do.same_partition(diar.kmeans(vec @ q, k, 0), g[name + "_labels"])


@pytest.mark.parametrize("name", NAMES)
def test_solver_logic_on_dense_panels(name):
    """diar._solve with numpy panels in place of the device's: eigenvalues to rounding, residuals under TOL,
    orthonormal vectors, and the golden partition through the same k-means."""
    g = golden()
    o = oracle(name)
    n = o["L"].shape[0]
    K = min(21, n)
    stats = {}
    lam, vec = diar._solve(do.DenseOps(o["L"]), n, min(diar.BLOCK, n), float(np.diag(o["L"]).max()), K, stats=stats)
    scale = 2.0 * float(np.diag(o["L"]).max())
    res = np.linalg.norm(o["L"] @ vec - vec * lam, axis=0)
    assert res.max() <= diar.TOL * scale
    assert np.abs(vec.T @ vec - np.eye(K)).max() <= 64 * 2.0 ** -52 * n
    assert np.abs(lam - g[name + "_lam"]).max() <= res.max() + 64 * 2.0 ** -52 * n
    k = diar.choose_num_spks(lam)
    assert k == int(g[name + "_num_spks"])
    assert do.same_partition(diar.kmeans(vec[:, :k], k, 0), g[name + "_labels"])


def test_solver_refuses_to_return_unconverged_vectors():
    o = oracle("n430")
    n = o["L"].shape[0]
    with pytest.raises(diar._lib.NativeError, match="residual"):
        diar._solve(do.DenseOps(o["L"]), n, 64, float(np.diag(o["L"]).max()), 21, max_sweeps=1)


# ---------------------------------------------------------------------------------------------- teeth
def _outcome(name, **corruption):
    o = do.oracle(fixture(name)[0], **corruption)
    K = min(21, o["L"].shape[0])
    k = do.choose(o["lam"][:K])
    return k, diar.kmeans(o["V"][:, :k], k, 0)


def _bites(name, k, labels):
    g = golden()
    return k != int(g[name + "_num_spks"]) or not do.same_partition(labels, g[name + "_labels"])


SMALL = ["n3", "n12", "n15", "n15m", "n65", "n120", "n430"]


@pytest.mark.parametrize("corruption", [dict(keep_delta=-1), dict(sym="max")], ids=["keep-1", "max-symmetrisation"])
def test_teeth_graph_corruptions_change_the_answer(corruption):
    assert not any(_bites(n, *_outcome(n)) for n in SMALL)          # the uncorrupted chain passes
    assert any(_bites(n, *_outcome(n, **corruption)) for n in SMALL), corruption


def test_teeth_diagonal_left_in_the_degree():
    """Every row keeps its own diagonal entry (the row maximum), so leaving it in the degree adds exactly 1 to every
    eigenvalue: no gap moves, and neither the speaker count nor the partition CAN change on any input.  What does
    change is what the GPU tests pin: the eigenvalues themselves (Weyl bound against the golden) and the number of
    them below 1e-9 on the disconnected fixture."""
    g = golden()
    for name in ("n65", "n120"):
        o = do.oracle(fixture(name)[0], diag_in_degree=True)
        K = g[name + "_lam"].size
        np.testing.assert_allclose(o["lam"][:K], g[name + "_lam"] + 1.0, rtol=0, atol=1e-10)
        assert not _bites(name, *_outcome(name, diag_in_degree=True))
    assert int((do.oracle(fixture("n120")[0], diag_in_degree=True)["lam"] < 1e-9).sum()) == 0
    assert int((g["n120_lam"] < 1e-9).sum()) == 3


def test_teeth_single_vector_iteration_misses_the_multiple_zero():
    o = oracle("n120")
    lam, vec = do.single_vector_krylov(o["L"], 21)
    k = do.choose(lam)
    assert int((lam < 1e-9).sum()) == 1
    assert _bites("n120", k, diar.kmeans(vec[:, :k], k, 0))
