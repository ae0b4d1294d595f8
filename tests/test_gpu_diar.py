"""GPU: the device half of the diarization back end (csrc/spectral.hip behind the ws_spectral_* entries) against the
float64 oracle of tests/diar_oracle.py and the golden tools/make_golden_diar.py recorded from the reference.

Bounds, all derived, none fitted:
  graph     an edge of the pruning mask may differ from float64 only in a row whose float64 affinity lies within
            tau = 8 x (the reference-float32 affinity error, golden) of that row's boundary values, in at most 2 % of
            the rows.  The fixtures' seeds put every boundary farther than tau apart, so here the graph must be EQUAL.
  operator  nnz_row_max * 2^-52 * sum|terms| per element: a sum of nnz + 7 roundings of 2^-53 each, nnz >= 9.
  gram      (n + 1) * 2^-53 * sum|x_p x_q| <= n * 2^-52 * sum|...|; rotate: b * 2^-52 * sum|x_p W_pq| likewise.
            References are numpy longdouble, so their own rounding is out of the picture.
  solve     residuals <= diar.TOL * 2 max(deg) (computed here from the returned vectors); |V^T V - I| <=
            64 * 2^-52 * n =: rounding; Weyl: |lam_i - golden_i| <= r_i + rounding; Davis-Kahan: sin(largest angle to
            the golden k-dimensional subspace) <= 2 max r_i / gap + rounding, gap = golden lam[k] - lam[k-1].  The
            "+ rounding" of the last bound is this file's addition to the theorem's 2 r / gap: on the n <= 64 fixtures
            r is ~1e-14 and the returned and the golden vectors each carry their own float64 rounding."""
import functools
import os

import numpy as np
import pytest
import torch

import diar_oracle as do
from fixtures import synth
from wespeaker_amd import _lib, diar

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diar_ref.npz")
NAMES = list(do.FIXTURES)
EPS = 2.0 ** -52


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


@functools.lru_cache(maxsize=None)
def graph(name):
    return diar.Graph(fixture(name)[0], keep_mask=True)


@functools.lru_cache(maxsize=None)
def dense(name):
    L = graph(name).dense_laplacian()
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def solved(name):
    n = len(fixture(name)[0])
    stats = {}
    lam, vec = diar.spectral_embedding(fixture(name)[0], min(21, n), stats=stats)
    return lam, vec, stats


def unpack(mask, n):
    bits = np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")
    assert not bits[:, n:].any(), "mask bits beyond column n"
    return bits[:, :n].astype(bool)


# ---------------------------------------------------------------------------------------------- graph
@pytest.mark.parametrize("name", NAMES)
def test_graph_structure_and_float64_parity(name):
    g, o, gr = golden(), oracle(name), graph(name)
    n, keep = gr.n, gr.keep
    assert keep == o["keep"]
    P = unpack(gr.mask(), n)
    assert (P.sum(1) == keep).all()
    L = dense(name)
    assert np.array_equal(L, L.T)
    assert (L.sum(1) == 0.0).all()
    off = L[~np.eye(n, dtype=bool)]
    assert np.isin(off, [0.0, -0.5, -1.0]).all()
    assert np.array_equal(L, do.laplacian(P))                       # the CSR is the symmetrised mask, nothing else
    tau = 8.0 * float(g[name + "_aff_err32"])
    rows, bad = do.excused_rows(P, o["P"], o["S"], keep, tau)
    print("%s: %d of %d rows differ from float64 (cap %.1f), %d unexcused; min boundary gap %.2e, tau %.2e"
          % (name, len(rows), n, 0.02 * n, len(bad), float(g[name + "_min_gap"]), tau))
    assert not bad
    assert len(rows) <= 0.02 * n
    if float(g[name + "_min_gap"]) > tau:
        assert len(rows) == 0 and np.array_equal(L, o["L"])
    # CSR invariants
    rowptr = gr.rowptr.cpu().numpy()
    col = gr.colidx.cpu().numpy()[:gr.nnz]
    val = gr.vals.cpu().numpy()[:gr.nnz]
    deg = gr.deg.cpu().numpy()
    assert rowptr[0] == 0 and rowptr[n] == gr.nnz == int((L != 0).sum() - (np.diag(L) != 0).sum())
    for i in range(n):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert (np.diff(c) > 0).all() and (c != i).all() and ((c >= 0) & (c < n)).all()
        assert deg[i] == val[rowptr[i]:rowptr[i + 1]].sum() == L[i, i]


def test_ties_go_to_the_higher_column():
    """Three copies of eight embeddings: the copies' affinities are exactly equal on the device (equal operands, equal
    order of summation), so every value of a row comes three times and the boundary falls inside a triple.  Exactly
    `keep` entries stay, and of the tied triple the later columns -- what the stable ascending argsort of
    spectral_clusterer.py:47-48 keeps."""
    base = np.random.default_rng(3).standard_normal((8, 32)).astype(np.float32)
    emb = np.concatenate([base, base, base])                        # n = 24, keep = 10 = 3 + 3 + 3 + 1
    gr = diar.Graph(emb, keep_mask=True)
    assert gr.keep == 10
    P = unpack(gr.mask(), 24)
    assert (P.sum(1) == 10).all()
    S8 = do.affinity(base)                                          # class values in float64 (gaps ~0.1: no near ties)
    want = np.zeros_like(P)
    for i in range(24):
        key = np.array([S8[i % 8, j % 8] for j in range(24)])
        order = np.lexsort((np.arange(24), key))                    # ascending by value, then by column
        want[i, order[24 - 10:]] = True
    assert np.array_equal(P, want)
    for i in range(24):                                             # the lone survivor of the fourth class is its LAST copy
        fourth = [j for j in range(24) if P[i, j] and not (P[i, j % 8] and P[i, j % 8 + 8] and P[i, j % 8 + 16])]
        assert len(fourth) == 1 and fourth[0] >= 16


# ---------------------------------------------------------------------------------------------- operator, gram, rotate
def _panels(n, b, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, b)), rng.standard_normal((n, b))


@pytest.mark.parametrize("name", ["n65", "n1030"])
@pytest.mark.parametrize("b", [1, 21, 64])
def test_operator_gram_rotate_against_numpy(name, b):
    gr, L = graph(name), dense(name)
    n = gr.n
    X, Z = _panels(n, b, 100 + b)
    W = np.random.default_rng(7).standard_normal((b, b))
    gr.alloc(4, b)
    gr.load(0, X)
    gr.load(1, Z)
    alpha, beta, gamma = 0.37, -1.25, 0.6
    gr.apply(alpha, beta, gamma, 0, 1, 2)
    Y = gr.fetch(2, b)
    ld = np.longdouble
    Ll, Xl, Zl = L.astype(ld), X.astype(ld), Z.astype(ld)
    ref = alpha * (Ll @ Xl) + beta * Xl + gamma * Zl
    mag = abs(alpha) * (np.abs(L) @ np.abs(X)) + abs(beta) * np.abs(X) + abs(gamma) * np.abs(Z)
    nnz_row_max = int(np.diff(gr.rowptr.cpu().numpy()).max())
    err = np.abs(Y.astype(ld) - ref).astype(np.float64)
    print("%s b=%d: operator error / bound = %.3f (nnz_row_max %d)" % (name, b, (err / (nnz_row_max * EPS * mag)).max(),
                                                                     nnz_row_max))
    assert (err <= nnz_row_max * EPS * mag).all()
    # plain product (beta = gamma = 0, Z absent), then Y aliasing Z
    gr.apply(1.0, 0.0, 0.0, 0, None, 2)
    LX = gr.fetch(2, b)
    assert (np.abs(LX.astype(ld) - Ll @ Xl).astype(np.float64) <= nnz_row_max * EPS * (np.abs(L) @ np.abs(X))).all()
    gr.apply(alpha, beta, gamma, 0, 1, 1)
    assert np.array_equal(gr.fetch(1, b), Y)
    # gram pair: accuracy, and the same bits from a second pair of launches
    G1, H1 = gr.gram(0, 2)
    G2, H2 = gr.gram(0, 2)
    assert np.array_equal(G1, G2) and np.array_equal(H1, H2)
    LXl = LX.astype(ld)
    assert (np.abs(G1.astype(ld) - Xl.T @ Xl).astype(np.float64) <= n * EPS * (np.abs(X).T @ np.abs(X))).all()
    assert (np.abs(H1.astype(ld) - Xl.T @ LXl).astype(np.float64) <= n * EPS * (np.abs(X).T @ np.abs(LX))).all()
    # rotate: out of place with an additive panel, then in place
    gr.load(1, Z)
    gr.rotate(0, W, gamma, 1, 3)
    R = gr.fetch(3, b)
    bound = b * EPS * (np.abs(X) @ np.abs(W) + abs(gamma) * np.abs(Z))
    assert (np.abs(R.astype(ld) - (Xl @ W.astype(ld) + gamma * Zl)).astype(np.float64) <= bound).all()
    gr.rotate(0, W, 0.0, None, 0)
    assert (np.abs(gr.fetch(0, b).astype(ld) - Xl @ W.astype(ld)).astype(np.float64)
            <= b * EPS * (np.abs(X) @ np.abs(W))).all()


# ---------------------------------------------------------------------------------------------- solve
@pytest.mark.parametrize("name", NAMES)
def test_solver_residuals_orthogonality_weyl_davis_kahan(name):
    g = golden()
    lam, vec, stats = solved(name)
    L = dense(name)
    n = L.shape[0]
    K = lam.size
    scale = 2.0 * float(np.diag(L).max())
    res = np.linalg.norm(L @ vec - vec * lam, axis=0)
    rounding = 64 * EPS * n
    ortho = np.abs(vec.T @ vec - np.eye(K)).max()
    weyl = np.abs(lam - g[name + "_lam"])
    k = int(g[name + "_num_spks"])
    gap = float(g[name + "_gaps"][2])
    gv = g[name + "_vec"][:, :k]
    sin = np.linalg.norm(vec[:, :k] - gv @ (gv.T @ vec[:, :k]), 2)
    print("%s: sweeps %s launches %s worst residual %.3e (bound %.3e) ortho %.3e (bound %.3e) max |dlam| %.3e "
          "sin %.3e (bound %.3e)" % (name, stats.get("sweeps"), stats.get("launches"), res.max(), diar.TOL * scale,
                                     ortho, rounding, weyl.max(), sin,
                                     2 * res.max() / gap + rounding if gap > 0 else float("nan")))
    assert (res <= diar.TOL * scale).all()
    assert ortho <= rounding
    assert (weyl <= res + rounding).all()
    if gap > 0:
        assert sin <= 2 * res[:k].max() / gap + rounding
    assert int((lam < 1e-9).sum()) == int((g[name + "_lam"] < 1e-9).sum())
    if name == "n120":
        assert int((lam < 1e-9).sum()) == 3


def test_solver_is_repeatable():
    lam, vec, _ = solved("n65")
    lam2, vec2 = diar.spectral_embedding(fixture("n65")[0], 21)
    assert np.array_equal(lam, lam2) and np.array_equal(vec, vec2)


# ---------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("name", NAMES)
def test_cluster_equals_the_reference_partition(name):
    g = golden()
    for seed in (0, 1):
        labels = diar.cluster(fixture(name)[0], seed=seed)
        assert labels.shape == g[name + "_labels"].shape
        assert do.same_partition(labels, g[name + "_labels"]), (name, seed)


def test_cluster_edge_cases_and_forced_counts():
    g = golden()
    emb = fixture("n12")[0]
    assert diar.cluster(emb[:0]).tolist() == [] and diar.cluster(emb[:1]).tolist() == [0]
    assert diar.cluster(emb[:2]).tolist() == [0, 0]
    assert diar.cluster(fixture("n3")[0]).tolist() == [0, 0, 0]     # an empty graph: one speaker
    # min_num_spks above the gap's choice: three components, four asked -- the first four eigenvectors span a
    # well-defined subspace (lam[3] is simple), so the oracle's vectors give the same partition through the k-means
    labels = diar.cluster(fixture("n120")[0], min_num_spks=4)
    assert len(set(labels.tolist())) == 4
    assert do.same_partition(labels, diar.kmeans(g["n120_vec"][:, :4], 4, 0))
    # num_spks forced to 2 on five components: ANY two vectors of the five-fold null space are "the first two
    # eigenvectors" (the reference's own answer depends on LAPACK's choice of basis), so the partition cannot be
    # pinned to the oracle's; what every basis gives is a two-way grouping of the five golden speakers
    labels = diar.cluster(fixture("n1030")[0], num_spks=2)
    assert len(set(labels.tolist())) == 2
    ref = g["n1030_labels"]
    for spk in set(ref.tolist()):
        assert len(set(labels[ref == spk].tolist())) == 1
    ov = diar.kmeans(g["n1030_vec"][:, :2], 2, 0)
    for spk in set(ref.tolist()):
        assert len(set(ov[ref == spk].tolist())) == 1


# ---------------------------------------------------------------------------------------------- end to end
SEG_SECONDS = 4.5
# six given segments over a recording that changes speaker every 4.5 s: abutting, apart, and one that starts
# 0.2 s inside its predecessor (a pivot that is not a segment boundary)
SEGMENTS = [(0.0, 4.5), (4.5, 9.0), (9.25, 13.5), (13.3, 18.0), (18.0, 22.25), (22.5, 27.0)]


def recording():
    seg = int(SEG_SECONDS * 16000)
    return np.concatenate([synth.synth_speaker_wav(k % 2, seg, k * seg) for k in range(6)])


def test_diarize_segments_end_to_end(tmp_path):
    import wespeaker_amd as wespeaker
    mdir = str(tmp_path / "model")
    synth.write_model_dir(mdir, "ECAPA_TDNN_GLOB_c512", 80, 192, seed=42)
    spk = wespeaker.load_model(mdir)
    rec = recording()
    segments = [{"start": b, "end": e} for b, e in SEGMENTS] + [{"start": 27.0, "end": 27.2}]   # too short: dropped
    turns = spk.diarize_segments(torch.from_numpy(rec)[None], segments, utt="rec", sample_rate=16000)
    # the reference formula on one speaker per segment: a turn per segment, cut at (b + end) / 2 where they touch
    want = []
    for k, (b, e) in enumerate(SEGMENTS):
        begin = b if k == 0 or b > SEGMENTS[k - 1][1] else (b + SEGMENTS[k - 1][1]) / 2.0
        end = e if k == 5 or SEGMENTS[k + 1][0] > e else (SEGMENTS[k + 1][0] + e) / 2.0
        want.append((begin, end))
    assert len(turns) == 6 and all(t[0] == "rec" for t in turns)
    for (utt, b, e, la), (wb, we) in zip(turns, want):
        assert abs(b - wb) < 1e-9 and abs(e - we) < 1e-9
    labels = [t[3] for t in turns]
    assert len(set(labels)) == 2 and labels == [labels[0], labels[1]] * 3 and labels[0] != labels[1]
    for a, b in zip(turns[:-1], turns[1:]):
        assert a[2] <= b[1]                                         # no overlap
    assert turns[0][1] == 0.0 and turns[-1][2] == 27.0
    # from a file, and through make_rttm
    wav = str(tmp_path / "rec.wav")
    synth.write_wav(wav, rec)
    assert spk.diarize_segments(wav, segments, utt="rec") == turns
    out = str(tmp_path / "rec.rttm")
    spk.make_rttm(turns, out)
    lines = open(out).read().splitlines()
    assert lines == ["SPEAKER rec 1 %.3f %.3f <NA> <NA> %s <NA> <NA>" % (b, e - b, la) for (_, b, e, la) in turns]
    assert spk.diarize_segments(wav, [{"start": 0.0, "end": 0.1}]) == []
    with pytest.raises(NotImplementedError):
        spk.diarize(wav)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_name_the_limit_and_launch_nothing():
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    buf = torch.zeros((1 << 16,), dtype=torch.float64, device=dev)
    i32 = torch.zeros((1 << 12,), dtype=torch.int32, device=dev)
    st = _lib.current_stream_ptr(dev)
    p, q = _lib.ptr(buf), _lib.ptr(i32)
    assert L.ws_spectral_graph(p, 8193, 4, 82, p, 1 << 19, q, q, p, 1 << 12, p, st) == -7
    assert b"8192" in L.ws_last_error()
    assert L.ws_spectral_graph(p, 2, 4, 1, p, 1 << 19, q, q, p, 1 << 12, p, st) == -1
    assert L.ws_spectral_graph(p, 100, 4, 10, p, 16, q, q, p, 1 << 12, p, st) == -7
    assert b"scratch" in L.ws_last_error()
    y = _lib.c_void_p(buf.data_ptr() + 8 * 8192)
    assert L.ws_spectral_apply(q, q, p, p, 100, 65, 1.0, 0.0, 0.0, p, None, y, st) == -1
    assert b"b = 65" in L.ws_last_error()
    assert L.ws_spectral_rotate(p, p, 0.0, None, y, 100, 65, st) == -1
    assert L.ws_spectral_gram(p, p, 100, 65, y, y, p, 1 << 19, st) == -1
    assert L.ws_spectral_gram(p, p, 100, 8, y, y, p, 64, st) == -7
    assert L.ws_spectral_apply(q, q, p, p, 100, 8, 1.0, 0.0, 0.0, p, None, p, st) == -1     # Y aliases X
    with pytest.raises(_lib.NativeError, match="8192"):
        diar.Graph(np.zeros((8193, 4), np.float32))
    with pytest.raises(ValueError):
        diar.cluster(fixture("n120")[0], max_num_spks=64)
    torch.cuda.synchronize()
    assert not buf.any() and not i32.any()                          # nothing ran
