"""CPU reference for the edge-side spectral kernel (hlhgat_eig_pe_edges of
csrc/eigpe.hip), numpy only, no hlhgat import: the dense edge Laplacian
L1 = B1^T B1 of a spectral_ref.Graph (B1[i, e] = -1, B1[j, e] = +1 for the
edge e = (i, j), i < j) and its fp64 eigh.  Acceptance is
spectral_ref.check_pe(L1, P, K), whose rules take any symmetric L.

L1's kernel is the cycle space (dimension beta1 = E - n + c); its nonzero
spectrum is L0's, with eigenvectors B1^T v / sqrt(lambda).
"""
from __future__ import annotations

import functools

import numpy as np

import spectral_ref as S


def incidence(ei, n):
    """B1 [n, E] of the edge list ei (i < j)."""
    E = ei.shape[1]
    B = np.zeros((n, E))
    B[ei[0], np.arange(E)] = -1.0
    B[ei[1], np.arange(E)] = 1.0
    return B


def dense_l1(ei, n):
    B = incidence(ei, n)
    return B.T @ B


class EdgeSide:
    """The edge side of a spectral_ref.Graph with check_pe's attributes: n is
    the dimension (the graph's edges), L the dense L1, eigh its fp64 eigh."""

    def __init__(self, g):
        self.g = g
        self.n = g.ei.shape[1]

    @functools.cached_property
    def L(self):
        return dense_l1(self.g.ei, self.g.n)

    @functools.cached_property
    def eigh(self):
        if self.n == 0:
            return np.zeros(0), np.zeros((0, 0))
        return np.linalg.eigh(self.L)

    @property
    def beta1(self):
        """Dimension of the cycle space, from the rank of L0."""
        if self.g.n == 0:
            return 0
        c = int((self.g.eigh[0] < 1e-9).sum())
        return self.n - self.g.n + c


def chain_rings(n, r, seed):
    """spectral_ref.chain_tree(n, seed) plus r ring closures between nodes 4
    or 5 places apart (a chain molecule: E = n - 1 + r, beta1 = r)."""
    rng = np.random.default_rng(seed + 7919)
    e = {(int(a), int(b)) for a, b in S.chain_tree(n, seed).ei.T}
    want = len(e) + r
    while len(e) < want:
        a = int(rng.integers(0, n - 5))
        b = a + 4 + int(rng.integers(0, 2))
        e.add((a, b))
    return S._graph(e, n)


def batch(graphs):
    """(ei int64 [2, E] with node offsets, node counts, edge counts, edge
    offsets [B + 1]): the batch's edges grouped by graph."""
    ei, ns, _ = S.batch(graphs)
    es = [g.ei.shape[1] for g in graphs]
    eoffs = np.concatenate([[0], np.cumsum(es)]).astype(np.int64)
    return ei, ns, es, eoffs
