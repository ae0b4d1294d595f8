"""Diarization back half behind the reference's interface: spectral clustering of sub-segment embeddings
on the GPU, segment merging and RTTM output.

Mirrors
    wespeaker/diar/spectral_clusterer.py:33-87   cluster()                         -> cluster (GPU + host)
    wespeaker/diar/spectral_clusterer.py:90-126  read_emb / main                   -> read_emb, `cluster` command
    wespeaker/diar/make_rttm.py:33-70            read_labels / merge_segments      -> same names (host)
    wespeaker/diar/make_rttm.py:73-82, cli/speaker.py:283-289                      -> `rttm` command, make_rttm

Division of labour.  Everything whose size is the number n of sub-segments runs in the HIP library
(include/wespeaker_amd.h, "spectral clustering"): the cosine affinity, the pruning, the symmetrised graph as
CSR, and the three products of the eigen-solver (operator, Gram pair, basis update).  The reference's dense
`scipy.linalg.eigh` of the n x n Laplacian (:59, O(n^3)) is replaced by Chebyshev-filtered subspace iteration
on a block of b = min(64, n) vectors, driven from here like the PLDA EM of plda_train.py: per sweep the host
sees two b x b float64 matrices and answers with one (Cholesky + eigh in numpy).  The k-means of :65-69 runs
here too, in numpy float64 on the n x k spectral embedding (k <= 21 by default): O(n k^2) on at most
8192 x 64 numbers.  numpy only: no scipy, no sklearn.

Solver parameters (DESIGN.md "Spectral clustering" has the measured sweep counts):
    TOL         1e-10   a Ritz pair (theta, v) counts as converged when |L v - theta v|_2 <= TOL * 2 max(deg);
                        the reference's own float32 eigh is about 1e-7 of the same scale off its float64 values
    MAX_DEGREE  24      longest Chebyshev filter of one sweep; a sweep's degree is the largest that keeps the
                        filter's gain at 0 over its gain at the damped edge below MAX_GAIN, so that the
                        filtered block stays well inside what a float64 Cholesky of its Gram matrix resolves
    MAX_GAIN    1e5
    MAX_SWEEPS  80      past it `spectral_embedding` raises NativeError naming the worst residual
    START_SEED  2022    the start block is np.random.default_rng(START_SEED).standard_normal((n, b))
"""
import argparse
import collections
import math
import sys

import numpy as np

from . import _lib

TOL = 1e-10
MAX_DEGREE = 24
MAX_GAIN = 1e5
MAX_SWEEPS = 80
START_SEED = 2022
BLOCK = 64
MAX_N = 8192
# kernels of one Rayleigh-Ritz pass with its residual check: the plain product, two Gram pairs of two kernels each
# (partials + fold), three basis updates (X, LX, residual panel); `stats["launches"]` counts kernels, filter steps included
RITZ_KERNELS = 8


# ------------------------------------------------------------------------------------- device stages
def spectral_keep(n, p=.01):
    """spectral_clusterer.py:40-44 -- how many entries of a row survive the pruning (ws_spectral_keep)."""
    return int(_lib.lib().ws_spectral_keep(int(n), float(p)))


class Graph:
    """The pruned, symmetrised affinity of spectral_clusterer.py:76-80 on the device: CSR of M, deg, and the
    panels of the solver.  L = diag(deg) - M is applied, never stored.  keep_mask=True keeps the graph stage's
    scratch alive so that `mask()` can read the pruning mask back (tests)."""

    def __init__(self, embeddings, p=.01, device=None, keep_mask=False):
        import torch
        _lib.require_gpu()
        self.torch = torch
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.lib = _lib.lib()
        emb = np.array(embeddings, dtype=np.float32, order="C")     # (a copy: torch wants a writable array)
        if emb.ndim != 2:
            raise ValueError("expected (n, dim) embeddings, got shape %s" % (emb.shape,))
        self.n, self.dim = int(emb.shape[0]), int(emb.shape[1])
        n = self.n
        self.keep = spectral_keep(n, p)
        self.cap = max(1, min(n * (n - 1), 2 * n * self.keep))
        self.scratch_bytes = int(self.lib.ws_spectral_scratch(n, self.dim))
        with torch.cuda.device(self.dev):
            self.emb = torch.from_numpy(emb).to(self.dev)
            # (a refused n leaves scratch_bytes at 0: the call below then names the reason)
            self.scratch = torch.empty((max(self.scratch_bytes, 256),), dtype=torch.uint8, device=self.dev)
            self.gram_bytes = int(self.lib.ws_spectral_gram_scratch(n))
            self.gram_scratch = torch.empty((max(self.gram_bytes, 256),), dtype=torch.uint8, device=self.dev)
            self.rowptr = torch.zeros((n + 1,), dtype=torch.int32, device=self.dev)
            self.colidx = torch.zeros((self.cap,), dtype=torch.int32, device=self.dev)
            self.vals = torch.zeros((self.cap,), dtype=torch.float64, device=self.dev)
            self.deg = torch.zeros((n,), dtype=torch.float64, device=self.dev)
            _lib.check(self.lib.ws_spectral_graph(
                _lib.ptr(self.emb), n, self.dim, self.keep, _lib.ptr(self.scratch), self.scratch_bytes,
                _lib.ptr(self.rowptr), _lib.ptr(self.colidx), _lib.ptr(self.vals), self.cap, _lib.ptr(self.deg),
                self._stream()), "ws_spectral_graph")
            self.nnz = int(self.rowptr[n].item())
            self.max_deg = float(self.deg.max().item())
            # the graph scratch holds the n x n fp32 affinity (256 MB at n = 8192): the solve does not need it, so
            # it goes back now (the two .item() reads above have waited for the stream) unless a test wants the mask
            if not keep_mask:
                self.scratch = None
        assert self.nnz <= self.cap
        self.b = min(BLOCK, n)
        self._panels = None

    def _stream(self):
        return _lib.current_stream_ptr(self.dev)

    # -- debug stages (tests)
    def dense_laplacian(self):
        torch = self.torch
        with torch.cuda.device(self.dev):
            out = torch.empty((self.n, self.n), dtype=torch.float64, device=self.dev)
            _lib.check(self.lib.ws_debug_spectral_dense(
                _lib.ptr(self.rowptr), _lib.ptr(self.colidx), _lib.ptr(self.vals), _lib.ptr(self.deg), self.n,
                _lib.ptr(out), self._stream()), "ws_debug_spectral_dense")
            return out.cpu().numpy()

    def mask(self):
        if self.scratch is None:
            raise ValueError("the pruning mask is gone with the graph scratch: build the Graph with keep_mask=True")
        torch = self.torch
        words = (self.n + 31) // 32
        with torch.cuda.device(self.dev):
            out = torch.empty((self.n, words), dtype=torch.int32, device=self.dev)
            _lib.check(self.lib.ws_debug_spectral_mask(_lib.ptr(self.scratch), self.n, self.dim, _lib.ptr(out),
                                                     self._stream()), "ws_debug_spectral_mask")
            return out.cpu().numpy().view(np.uint32)

    # -- the solver's operations on numbered n x b panels (see _solve)
    def alloc(self, count, b):
        self.b = b
        self._panels = [self.torch.zeros((self.n, b), dtype=self.torch.float64, device=self.dev)
                        for _ in range(count)]
        self._small = [self.torch.zeros((b, b), dtype=self.torch.float64, device=self.dev) for _ in range(3)]

    def load(self, i, host):
        self._panels[i].copy_(self.torch.from_numpy(np.ascontiguousarray(host, dtype=np.float64)))

    def fetch(self, i, k):
        return self._panels[i][:, :k].cpu().numpy()

    def apply(self, alpha, beta, gamma, x, z, y):
        with self.torch.cuda.device(self.dev):
            _lib.check(self.lib.ws_spectral_apply(
                _lib.ptr(self.rowptr), _lib.ptr(self.colidx), _lib.ptr(self.vals), _lib.ptr(self.deg), self.n,
                self.b, float(alpha), float(beta), float(gamma), _lib.ptr(self._panels[x]),
                _lib.ptr(self._panels[z]) if z is not None else None, _lib.ptr(self._panels[y]),
                self._stream()), "ws_spectral_apply")

    def gram(self, x, lx):
        with self.torch.cuda.device(self.dev):
            g, h = self._small[0], self._small[1]
            _lib.check(self.lib.ws_spectral_gram(
                _lib.ptr(self._panels[x]), _lib.ptr(self._panels[lx]), self.n, self.b, _lib.ptr(g), _lib.ptr(h),
                _lib.ptr(self.gram_scratch), self.gram_bytes, self._stream()), "ws_spectral_gram")
            return g.cpu().numpy(), h.cpu().numpy()

    def rotate(self, x, w, gamma, z, out):
        with self.torch.cuda.device(self.dev):
            wd = self._small[2]
            wd.copy_(self.torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64)))
            _lib.check(self.lib.ws_spectral_rotate(
                _lib.ptr(self._panels[x]), _lib.ptr(wd), float(gamma),
                _lib.ptr(self._panels[z]) if z is not None else None, _lib.ptr(self._panels[out]), self.n,
                self.b, self._stream()), "ws_spectral_rotate")


def _filter_degree(a, ub):
    """Largest degree <= MAX_DEGREE whose Chebyshev polynomial, damping [a, ub], grows by at most MAX_GAIN from
    a to 0: T_m(x0) = cosh(m acosh(x0)), x0 = (ub + a) / (ub - a)."""
    x0 = (ub + a) / (ub - a)
    return max(1, min(MAX_DEGREE, int(math.acosh(MAX_GAIN) / math.acosh(x0))))


def _solve(ops, n, b, max_deg, want, tol=TOL, max_sweeps=MAX_SWEEPS, stats=None):
    """Chebyshev-filtered subspace iteration for the `want` smallest eigenpairs of L = diag(deg) - M.
    `ops` owns four n x b panels and offers load / fetch / apply / gram / rotate on them (Graph above).
    Returns (theta[:want], V (n, want)); raises NativeError when max_sweeps filters were not enough."""
    ops.alloc(4, b)
    ub = 2.0 * max_deg                                  # Gershgorin: every eigenvalue lies in [0, 2 max(deg)]
    if n <= b:
        ops.load(0, np.eye(n))                          # the block spans everything: one exact Rayleigh-Ritz step
    else:
        ops.load(0, np.random.default_rng(START_SEED).standard_normal((n, b)))
    x, spare, lx, rbuf = 0, 1, 2, 3
    edge, launches, worst, theta = None, 0, float("inf"), None

    def rayleigh_ritz():
        ops.apply(1.0, 0.0, 0.0, x, None, lx)
        g, h = ops.gram(x, lx)
        d = np.sqrt(np.diag(g))
        if not np.all(np.isfinite(d)) or np.any(d <= 0.0):
            raise _lib.NativeError("spectral solver: the block lost a column (Gram diagonal %r)" % (d.min(),))
        try:
            c = np.linalg.cholesky(0.5 * (g + g.T) / np.outer(d, d))
        except np.linalg.LinAlgError:
            raise _lib.NativeError("spectral solver: the filtered block lost rank (Cholesky of its Gram matrix failed)")
        ci = np.linalg.inv(c)
        th, q = np.linalg.eigh(ci @ (0.5 * (h + h.T) / np.outer(d, d)) @ ci.T)
        w = (ci.T @ q) / d[:, None]
        ops.rotate(x, w, 0.0, None, x)
        ops.rotate(lx, w, 0.0, None, lx)
        return th

    def residuals(th):
        ops.rotate(x, -np.diag(th), 1.0, lx, rbuf)      # L V - V diag(theta)
        rr, _ = ops.gram(rbuf, rbuf)
        return np.sqrt(np.maximum(np.diag(rr), 0.0))

    for sweep in range(max_sweeps + 1):
        if sweep > 0:
            # three-term recurrence scaled to 1 at 0 (no overflow): damps [edge, ub]
            m = _filter_degree(edge, ub)
            e, c = 0.5 * (ub - edge), 0.5 * (ub + edge)
            sigma1 = -e / c
            sigma = sigma1
            ops.apply(sigma1 / e, -sigma1 * c / e, 0.0, x, None, spare)
            cur, prev = spare, x
            for _ in range(2, m + 1):
                sigma2 = 1.0 / (2.0 / sigma1 - sigma)
                ops.apply(2.0 * sigma2 / e, -2.0 * sigma2 * c / e, -sigma * sigma2, cur, prev, prev)
                cur, prev = prev, cur
                sigma = sigma2
            x, spare = cur, prev
            launches += m
        theta = rayleigh_ritz()
        res = residuals(theta)
        launches += RITZ_KERNELS
        worst = float(res[:want].max())
        if worst <= tol * ub:
            # one more orthonormalisation without a filter: V^T V = I to rounding whatever the sweeps left
            theta = rayleigh_ritz()
            res = residuals(theta)
            launches += RITZ_KERNELS
            worst = float(res[:want].max())
            if worst <= tol * ub:
                if stats is not None:
                    stats.update(sweeps=sweep, launches=launches, worst_residual=worst, bound=tol * ub)
                return theta[:want].copy(), ops.fetch(x, want)
        if n <= b:
            break
        # the largest Ritz value is the lower edge of the next filter; it must stay inside (0, ub)
        edge = float(min(max(theta[-1], 1e-3 * ub), 0.95 * ub))
    raise _lib.NativeError("spectral solver: %d sweeps left a residual of %.3e (bound %.3e = %g * 2 max(deg)) among "
                           "the first %d Ritz pairs" % (max_sweeps, worst, tol * ub, tol, want))


def spectral_embedding(embeddings, want, p=.01, device=None, stats=None):
    """The `want` smallest eigenvalues (ascending) and eigenvectors of the Laplacian of
    spectral_clusterer.py:76-80, as (float64[want], float64 (n, want)).  3 <= n <= 8192."""
    graph = Graph(embeddings, p, device)
    n = graph.n
    b = min(BLOCK, n)
    if want > b:
        raise ValueError("%d eigenvectors asked of a block of %d (max_num_spks + 1, num_spks and min_num_spks "
                         "may not exceed %d)" % (want, b, BLOCK))
    if stats is not None:
        stats.update(n=n, keep=graph.keep, nnz=graph.nnz, max_deg=graph.max_deg)
    return _solve(graph, n, b, graph.max_deg, want, stats=stats)


# ------------------------------------------------------------------------------------- host k-means
def kmeans(data, k, seed=0, n_init=10, max_iter=300):
    """k-means on the rows of `data` (n, d) in numpy float64: k-means++ seeding from
    np.random.default_rng(seed), n_init initialisations, Lloyd to a fixed point, the lowest inertia wins
    (the role of sklearn's k_means(data, k, n_init=10) at spectral_clusterer.py:65-69, with a seed where the
    reference has none).  Host code on purpose: n <= 8192 rows of k <= 64 numbers."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    n = x.shape[0]
    k = int(k)
    if k <= 1 or n == 0:
        return np.zeros((n,), dtype=np.int64)
    rng = np.random.default_rng(seed)
    xx = np.einsum("ij,ij->i", x, x)

    def sqdist(centres):
        d = xx[:, None] - 2.0 * (x @ centres.T) + np.einsum("ij,ij->i", centres, centres)[None, :]
        return np.maximum(d, 0.0)

    best, best_inertia = None, None
    for _ in range(n_init):
        centres = np.empty((k, x.shape[1]))
        centres[0] = x[rng.integers(n)]
        closest = sqdist(centres[:1])[:, 0]
        for j in range(1, k):
            tot = closest.sum()
            idx = rng.integers(n) if tot <= 0.0 else min(n - 1, int(np.searchsorted(np.cumsum(closest), rng.random() * tot)))
            centres[j] = x[idx]
            closest = np.minimum(closest, sqdist(centres[j:j + 1])[:, 0])
        labels = None
        for _ in range(max_iter):
            d = sqdist(centres)
            new = d.argmin(1)
            if labels is not None and np.array_equal(new, labels):
                break
            labels = new
            for j in range(k):
                sel = labels == j
                if sel.any():
                    centres[j] = x[sel].mean(0)
                else:                                   # an empty cluster takes the point farthest from its centre
                    far = int(d[np.arange(n), labels].argmax())
                    centres[j] = x[far]
        inertia = float(sqdist(centres)[np.arange(n), labels].sum())
        if best_inertia is None or inertia < best_inertia:
            best, best_inertia = labels, inertia
    return best.astype(np.int64)


def choose_num_spks(eig_values, num_spks=None, min_num_spks=1, max_num_spks=20):
    """spectral_clusterer.py:60-62: the largest gap among the first max_num_spks + 1 eigenvalues."""
    if num_spks is None:
        num_spks = int(np.argmax(np.diff(eig_values[:max_num_spks + 1]))) + 1
    return max(int(num_spks), int(min_num_spks))


def cluster(embeddings, p=.01, num_spks=None, min_num_spks=1, max_num_spks=20, seed=0, device=None):
    """spectral_clusterer.py:33-87 with the same arguments and edge cases (<= 2 embeddings: all zeros; 3: an
    empty graph and one speaker).  Affinity, pruning, Laplacian and the eigen-solve run on the GPU; the k-means
    on the (n, num_spks) spectral embedding runs here in numpy float64 with `seed` (see `kmeans`).
    Returns an int64 label per embedding."""
    n = len(embeddings)
    if n <= 2:
        return np.zeros((n,), dtype=np.int64)
    emb = np.asarray(embeddings, dtype=np.float32)
    k_gap = min(max_num_spks + 1, n)
    want = min(n, max(k_gap, num_spks or 0, min_num_spks))
    eig_values, eig_vectors = spectral_embedding(emb, want, p, device)
    k = min(choose_num_spks(eig_values[:k_gap], num_spks, min_num_spks, max_num_spks), n)
    return kmeans(eig_vectors[:, :k], k, seed)


# ------------------------------------------------------------------------------------- labels -> RTTM
def window_times(name, frame_shift=10):
    """A sub-segment name "[<utt>-]<segment begin ms>-<segment end ms>-<first frame>-<last frame>" (the names
    diar/extract_emb.py:55-83 gives its windows) -> (utt, begin s, end s).  A window's times count frames of
    `frame_shift` ms from the segment's begin (make_rttm.py:33-44, cli/speaker.py:259-264); the segment's end is
    not used.  `utt` is everything in front of the four numeric fields ('' when there is nothing)."""
    fields = name.split("-")
    if len(fields) < 4:
        raise ValueError("not a sub-segment name: %r" % (name,))
    origin_ms = int(fields[-4])
    first_ms, last_ms = (origin_ms + int(frames) * frame_shift for frames in fields[-2:])
    return "-".join(fields[:-4]), first_ms / 1000.0, last_ms / 1000.0


def read_labels(labels_file, frame_shift=10):
    """The label file of the `cluster` command (`<sub-segment name> <label>` per line) -> OrderedDict
    utt -> [(begin s, end s, label)] in file order, labels kept as text: what make_rttm.py:33-44 returns.
    Like there, a name must have exactly five '-' separated fields."""
    per_utt = collections.OrderedDict()
    with open(labels_file, "r") as f:
        for line in f:
            name, label = line.split()
            if name.count("-") != 4:
                raise ValueError("expected <utt>-<begin ms>-<end ms>-<first frame>-<last frame>, got %r" % (name,))
            utt, begin, end = window_times(name, frame_shift)
            per_utt.setdefault(utt, []).append((begin, end, label))
    return per_utt


def merge_segments(utt_to_subseg_labels):
    """Windows (begin, end, label) per utterance, in time order -> speaker turns [(utt, begin, end, label)] with
    the behaviour of make_rttm.py:47-70.  One turn is open at a time.  A window that starts after the open turn's
    reach closes it there; one that starts inside it either extends it (same label: the reach becomes this
    window's end) or takes over at the middle between its own begin and the reach (other label).  The last turn
    of an utterance is closed at the end of the last window read, whichever turn that window belonged to."""
    turns = []
    for utt, windows in utt_to_subseg_labels.items():
        start = reach = who = tail = None
        for (w_begin, w_end, w_label) in windows:
            if tail is None:
                start, reach, who = w_begin, w_end, w_label
            elif w_begin > reach:
                turns.append((utt, start, reach, who))
                start, reach, who = w_begin, w_end, w_label
            elif w_label == who:
                reach = w_end
            else:
                cut = (w_begin + reach) / 2.0
                turns.append((utt, start, cut, who))
                start, reach, who = cut, w_end, w_label
            tail = w_end
        if tail is not None:
            turns.append((utt, start, tail, who))
    return turns


RTTM_LINE = "SPEAKER {} {} {:.3f} {:.3f} <NA> <NA> {} <NA> <NA>"


def rttm_lines(merged_segment_to_labels, channel=1):
    return [RTTM_LINE.format(utt, channel, float(begin), float(end) - float(begin), label)
            for (utt, begin, end, label) in merged_segment_to_labels]


def make_rttm(merged_segment_to_labels, outfile, channel=1):
    """cli/speaker.py:283-289 (channel 1 there; make_rttm.py:80-82 takes it from --channel)."""
    with open(outfile, "w", encoding="utf-8") as fout:
        for line in rttm_lines(merged_segment_to_labels, channel):
            fout.write(line + "\n")


# ------------------------------------------------------------------------------------- command lines
def read_emb(scp):
    """An embedding scp of sub-segments -> (list of name lists, list of (n, dim) arrays), one entry per utterance:
    the utterance of a sub-segment is the text before its first '-', utterances come in order of first appearance
    (what spectral_clusterer.py:90-105 returns)."""
    from .kaldi_io import read_vec_scp
    names, rows = collections.OrderedDict(), {}
    for key, vec in read_vec_scp(scp).items():
        utt = key.partition("-")[0]
        names.setdefault(utt, []).append(key)
        rows.setdefault(utt, []).append(vec)
    return list(names.values()), [np.stack(rows[utt]) for utt in names]


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m wespeaker_amd.diar", description=__doc__.split("\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)
    pc = sub.add_parser("cluster", help="diar/spectral_clusterer.py: embedding scp -> `<sub-segment> <label>` lines")
    pc.add_argument("--scp", required=True, help="Kaldi scp of the sub-segment embeddings, named <utt>-<...>")
    pc.add_argument("--output", required=True, help="file that receives one `<sub-segment> <label>` line per row")
    pr = sub.add_parser("rttm", help="diar/make_rttm.py: label file -> RTTM on standard output")
    pr.add_argument("--labels", required=True, help="the `cluster` command's output file")
    pr.add_argument("--channel", type=int, default=1, help="value of the RTTM channel field (default 1)")
    args = parser.parse_args(argv)
    if args.command == "cluster":
        import os
        subsegs_list, embeddings_list = read_emb(args.scp)
        out_dir = os.path.dirname(args.output)
        if out_dir:
            os.makedirs(out_dir, exist_ok=True)
        with open(args.output, "w") as f:
            for subsegs, embeddings in zip(subsegs_list, embeddings_list):
                for subseg, label in zip(subsegs, cluster(embeddings)):
                    print(subseg, label, file=f)
    else:
        for line in rttm_lines(merge_segments(read_labels(args.labels)), args.channel):
            print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
