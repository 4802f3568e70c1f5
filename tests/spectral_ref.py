"""CPU reference for the spectral kernels (csrc/eigpe.hip, k_lanczos_lmax of
csrc/hodge.hip), numpy only, no hlhgat import: the dense L0 = B1 B1^T of an
edge list, the acceptance rules of an eigenvector positional encoding
(check_pe), and deterministic graph families that reach the kernels' size
classes.  tests/test_eig_pe.py and tests/test_hodge_lmax.py hold the HIP path
to it; the CPU tests of test_eig_pe.py hold check_pe itself to planted errors.

A graph is a Graph(ei, n): ei int64 [2, E] with i < j per edge, no duplicate
edges, n nodes.  Its dense L0 and fp64 eigh are computed once and kept.
"""
from __future__ import annotations

import functools

import numpy as np

# check_pe's bounds (the output is float32 of an fp64 computation)
GAP = 1e-3        # an eigenvalue further than this from both neighbours is separated
VEC_TOL = 2e-6    # separated column vs the reference vector, up to sign
RES_TOL = 1e-5    # |L p - lambda p|_max <= RES_TOL * max(1, lambda_max)
ORTH_TOL = 1e-5   # |P^T P - I|_max


def dense_l0(ei, n):
    L = np.zeros((n, n))
    np.add.at(L, (ei[0], ei[1]), -1.0)
    np.add.at(L, (ei[1], ei[0]), -1.0)
    L[np.diag_indices(n)] = -L.sum(1)
    return L


class Graph:
    def __init__(self, ei, n):
        self.ei = np.asarray(ei, np.int64).reshape(2, -1)
        self.n = int(n)
        assert self.ei.size == 0 or (self.ei[0] < self.ei[1]).all() and self.ei.max() < n

    @functools.cached_property
    def L(self):
        return dense_l0(self.ei, self.n)

    @functools.cached_property
    def eigh(self):
        """(w ascending, V) of the dense L0 in fp64."""
        if self.n == 0:
            return np.zeros(0), np.zeros((0, 0))
        return np.linalg.eigh(self.L)

    @property
    def lmax(self):
        return float(self.eigh[0][-1]) if self.n else 0.0

    @property
    def nnz(self):
        """Entries of the incidence CSR (2 E)."""
        return 2 * self.ei.shape[1]


def separated(w, K):
    """The PE columns c (eigenpair c + 1) of a graph with eigenvalues w that
    check_pe compares vector for vector."""
    n = len(w)
    out = []
    for c in range(min(K, n) - 1):
        j = c + 1
        gap = min(w[j] - w[j - 1], (w[j + 1] - w[j]) if j + 1 < n else np.inf)
        if gap > GAP:
            out.append(c)
    return out


def check_pe(L, P, K, eigh=None):
    """Acceptance of P [n, K - 1] as the eigenvector PE of the dense L0 = L
    (eigenvectors 1 .. K-1, ascending; eigh = a precomputed np.linalg.eigh(L)):
    columns past the graph's size are zero; every column is an eigenvector of
    its eigenvalue (residual <= 1e-5 max(1, lambda_max)); the columns are
    orthonormal within 1e-5; every column whose eigenvalue is further than
    1e-3 from its neighbours equals the reference vector up to sign within
    2e-6.  Returns how many columns were compared vector for vector."""
    P = np.asarray(P, np.float64)
    n = L.shape[0]
    assert P.shape == (n, K - 1), (P.shape, n, K)
    if n == 0:
        return 0
    w, V = np.linalg.eigh(L) if eigh is None else eigh
    m = min(K, n)
    assert np.all(P[:, m - 1:] == 0.0), "nonzero column past the graph's size"
    if m <= 1:
        return 0
    P = P[:, :m - 1]
    lam = w[1:m]
    res = np.abs(L @ P - P * lam[None, :]).max()
    assert res <= RES_TOL * max(1.0, w[-1]), ("residual", res)
    orth = np.abs(P.T @ P - np.eye(m - 1)).max()
    assert orth <= ORTH_TOL, ("orthonormality", orth)
    cols = separated(w, K)
    for c in cols:
        j = c + 1
        s = np.sign(P[:, c] @ V[:, j]) or 1.0
        err = np.abs(P[:, c] * s - V[:, j]).max()
        assert err <= VEC_TOL, ("vector", c, err)
    return len(cols)


# ---- graph families -----------------------------------------------------------

def _graph(pairs, n):
    e = sorted({(min(a, b), max(a, b)) for a, b in pairs if a != b})
    return Graph(np.array(e, np.int64).reshape(-1, 2).T, n)


def path(n):
    return _graph([(j, j + 1) for j in range(n - 1)], n)


def ring(n):
    return _graph([(j, (j + 1) % n) for j in range(n)], n)


def star(n):
    return _graph([(0, j) for j in range(1, n)], n)


def complete(n):
    return _graph([(i, j) for i in range(n) for j in range(i + 1, n)], n)


def grid(s, t=None):
    t = s if t is None else t
    e = [(i * t + j, i * t + j + 1) for i in range(s) for j in range(t - 1)]
    e += [(i * t + j, (i + 1) * t + j) for i in range(s - 1) for j in range(t)]
    return _graph(e, s * t)


def ring_chords(n, seed):
    """A ring of n >= 5 nodes plus n random chords (simple graph, 2 n edges):
    no symmetry, so its low eigenvalues are separated."""
    rng = np.random.default_rng(seed)
    e = {(j, j + 1) for j in range(n - 1)} | {(0, n - 1)}
    while len(e) < 2 * n:
        a, b = (int(x) for x in rng.integers(0, n, 2))
        if a != b:
            e.add((min(a, b), max(a, b)))
    return _graph(e, n)


def chain_tree(n, seed):
    """Chain-like tree (molecule backbones): node v hangs off a random earlier
    node within 6 places whose degree is below 4 (v - 1 always qualifies)."""
    rng = np.random.default_rng(seed)
    deg = np.zeros(n, np.int64)
    e = []
    for v in range(1, n):
        cand = [u for u in range(max(0, v - 6), v) if deg[u] < 4]
        u = cand[int(rng.integers(len(cand)))]
        e.append((u, v))
        deg[u] += 1
        deg[v] += 1
    return _graph(e, n)


def knn(n, k, seed, drop=0.0):
    """Symmetrised k-nearest-neighbour graph of n uniform points in the unit
    square (the superpixel graphs' family); drop = the fraction of edges
    removed at random afterwards (isolated nodes may appear)."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 2))
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nb = np.argsort(d, axis=1, kind="stable")[:, :min(k, n - 1)]
    e = sorted({(min(i, int(j)), max(i, int(j))) for i in range(n) for j in nb[i]})
    if drop:
        e = [p for p in e if rng.random() >= drop]
    return _graph(e, n)


def copies(g, c, isolated=0):
    """c disjoint copies of g followed by `isolated` nodes without edges
    (every eigenvalue c-fold, eigenvalue 0 a further `isolated` times)."""
    ei = np.concatenate([g.ei + i * g.n for i in range(c)], axis=1)
    return Graph(ei, c * g.n + isolated)


def batch(graphs):
    """(ei int64 [2, E] with node offsets, node counts, offsets [B + 1])."""
    ns = [g.n for g in graphs]
    offs = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    ei = np.concatenate([np.zeros((2, 0), np.int64)] + [g.ei + o for g, o in zip(graphs, offs[:-1])],
                        axis=1)
    return np.ascontiguousarray(ei), ns, offs
