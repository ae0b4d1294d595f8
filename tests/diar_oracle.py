"""Float64 oracle of the spectral clusterer (steps 2-5 of wespeaker/diar/spectral_clusterer.py:33-63, restated in
numpy), the seeded fixtures of tests/golden/diar_ref.npz, a dense numpy stand-in for the device panels of
wespeaker_amd.diar._solve, and the deliberately wrong variants the tests must be able to tell apart.

Test infrastructure only: nothing under wespeaker_amd/ imports it."""
import numpy as np

# name -> (cluster sizes, noise, seed): unit-variance Gaussian noise * `noise` around N(0, I) centres in 256 dims.
# The seeds are the first ones at which no row's last kept and first dropped affinity lie closer than 8 x the
# float32 affinity error (tools/make_golden_diar.py asserts it): every correct float32 pipeline then builds the
# SAME graph as float64, so the golden eigenvalues bound the device's and no row needs the tie excuse.
FIXTURES = {
    "n3": ((3,), 1.0, 3),
    "n12": ((12,), 1.0, 13),
    # three tight groups that the near-complete graph (keep = 10 of 15) still joins into ONE speaker, with the
    # second eigen-gap close behind: the fixture on which pruning to keep - 1 changes the speaker count
    "n15": ((6, 5, 4), 0.6, 12),
    # the same shape at a seed where the reference hears TWO speakers and symmetrising with max hears one
    "n15m": ((6, 5, 4), 0.6, 29),
    "n65": ((35, 30), 0.6, 65),
    "n120": ((40, 30, 50), 0.6, 122),
    "n430": ((400, 30), 1.0, 495),
    "n1030": ((300, 250, 200, 150, 130), 1.0, 1999),
}
DIM = 256


def make_fixture(name):
    """(float32 (n, 256) embeddings, int truth labels); rows are shuffled so that speakers interleave."""
    sizes, noise, seed = FIXTURES[name]
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((len(sizes), DIM))
    truth = np.repeat(np.arange(len(sizes)), sizes)
    emb = centres[truth] + noise * rng.standard_normal((truth.size, DIM))
    order = rng.permutation(truth.size)
    return emb[order].astype(np.float32), truth[order]


def keep_rule(m, p=.01):
    low = max(m - 10, 2) if m < 1000 else int((1.0 - p) * m)
    return min(max(m - low, 0), m)


def affinity(emb, dtype=np.float64):
    x = np.asarray(emb).astype(dtype)
    u = x / np.linalg.norm(x, axis=1, keepdims=True)
    return (dtype(0.5) * (dtype(1.0) + u @ u.T)).astype(dtype)


def prune_mask(S, keep):
    """Boolean P: the `keep` largest entries of each row, ties to the higher column (stable ascending argsort)."""
    n = S.shape[0]
    order = np.argsort(S, axis=1, kind="stable")
    P = np.zeros((n, n), dtype=bool)
    if keep > 0:
        np.put_along_axis(P, order[:, n - keep:], True, axis=1)
    return P


def laplacian(P, sym="mean", diag_in_degree=False):
    Pf = P.astype(np.float64)
    M = np.maximum(Pf, Pf.T) if sym == "max" else 0.5 * (Pf + Pf.T)
    if diag_in_degree:
        deg = np.abs(M).sum(1)
        M = M.copy()
        np.fill_diagonal(M, 0.0)
    else:
        M = M.copy()
        np.fill_diagonal(M, 0.0)
        deg = np.abs(M).sum(1)
    return np.diag(deg) - M


def choose(eig_values, num_spks=None, min_num_spks=1, max_num_spks=20):
    if num_spks is None:
        num_spks = int(np.argmax(np.diff(eig_values[:max_num_spks + 1]))) + 1
    return max(num_spks, min_num_spks)


def oracle(emb, p=.01, keep_delta=0, sym="mean", diag_in_degree=False, dtype=np.float64):
    """-> dict(S, P, L, lam, V): the float64 (or `dtype`) chain with optional corruptions."""
    S = affinity(emb, dtype)
    keep = keep_rule(S.shape[0], p) + keep_delta
    P = prune_mask(S, keep)
    L = laplacian(P, sym, diag_in_degree)
    lam, V = np.linalg.eigh(L)
    return dict(S=S, P=P, L=L, lam=lam, V=V, keep=keep)


def boundary_gaps(S64, keep):
    """Per row the two values either side of the pruning boundary: (keep-th largest, (keep+1)-th largest)."""
    srt = np.sort(S64, axis=1)
    n = S64.shape[0]
    hi = srt[:, n - keep]
    lo = srt[:, n - keep - 1] if keep < n else np.full(n, -np.inf)
    return hi, lo


def excused_rows(P_test, P64, S64, keep, tau):
    """Rows of P_test that differ from P64.  Returns (rows that differ, rows that differ in an entry farther
    than tau from the row's float64 boundary values -- these are errors)."""
    hi, lo = boundary_gaps(S64, keep)
    diff = P_test != P64
    rows = np.flatnonzero(diff.any(1))
    bad = []
    for i in rows:
        cols = np.flatnonzero(diff[i])
        gap = np.minimum(np.abs(S64[i, cols] - hi[i]), np.abs(S64[i, cols] - lo[i]))
        if (gap > tau).any():
            bad.append(int(i))
    return rows, bad


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    fwd, bwd = {}, {}
    for x, y in zip(a.tolist(), b.tolist()):
        if fwd.setdefault(x, y) != y or bwd.setdefault(y, x) != x:
            return False
    return True


def single_vector_krylov(L, k, seed=0):
    """The WRONG solver: what one Krylov sequence from one start vector converges to in exact arithmetic -- every
    DISTINCT eigenvalue once, with the start vector's projection on its eigenspace.  A multiple zero eigenvalue
    (a disconnected graph) is counted a single time.  (A floating-point Lanczos run is no stable stand-in: its
    rounding errors let the copies in after enough steps.)"""
    lam, V = np.linalg.eigh(L)
    q = np.random.default_rng(seed).standard_normal(L.shape[0])
    out_l, out_v, i = [], [], 0
    while i < lam.size and len(out_l) < k:
        j = i
        while j + 1 < lam.size and lam[j + 1] - lam[i] < 1e-9:
            j += 1
        v = V[:, i:j + 1] @ (V[:, i:j + 1].T @ q)
        out_l.append(lam[i:j + 1].mean())
        out_v.append(v / np.linalg.norm(v))
        i = j + 1
    return np.array(out_l), np.stack(out_v, axis=1)


class DenseOps:
    """The panel operations of wespeaker_amd.diar._solve on a dense float64 L in numpy: checks the solver's
    host logic without a GPU (the device kernels are checked against the same formulas in test_gpu_diar.py)."""

    def __init__(self, L):
        self.Lm = np.asarray(L, dtype=np.float64)
        self.n = self.Lm.shape[0]
        self.applies = 0

    def alloc(self, count, b):
        self.b = b
        self.p = [np.zeros((self.n, b)) for _ in range(count)]

    def load(self, i, host):
        self.p[i] = np.array(host, dtype=np.float64)

    def fetch(self, i, k):
        return self.p[i][:, :k].copy()

    def apply(self, alpha, beta, gamma, x, z, y):
        out = alpha * (self.Lm @ self.p[x]) + beta * self.p[x]
        if gamma != 0.0:
            out = out + gamma * self.p[z]
        self.p[y] = out
        self.applies += 1

    def gram(self, x, lx):
        return self.p[x].T @ self.p[x], self.p[x].T @ self.p[lx]

    def rotate(self, x, w, gamma, z, out):
        r = self.p[x] @ w
        if gamma != 0.0:
            r = r + gamma * self.p[z]
        self.p[out] = r
