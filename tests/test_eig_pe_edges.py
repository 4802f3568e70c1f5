"""hlhgat_eig_pe_edges (ops.eig_pe_edges): the edge-side eigenvector PE of
every graph of a batch in one launch -- the molecular datasets' eig_pe(L1)
(lib/Hodge_Dataset.py:458, :587: eigenvectors 1 .. k-1 of a dense eigh of the
E x E edge Laplacian) -- against numpy's fp64 eigh of the dense L1 = B1^T B1
by spectral_ref.check_pe:

* columns past a graph's edge count are zero;
* every column is an eigenvector of its eigenvalue (residual <= 1e-5
  max(1, lambda_max)) and the columns are orthonormal within 1e-5 -- this is
  all that can be asked inside L1's kernel, the cycle space, whose basis is
  arbitrary (the reference's own is LAPACK noise);
* every column whose eigenvalue is further than 1e-3 from its neighbours
  equals the fp64 vector up to sign within 2e-6.

The harmonic-only case (ring_chords(12) at k = 10: beta1 = 13 >= k) compares
no column vector for vector; the molecule case (k = 16 on the fixture's
molecules) must compare at least half of its (graph, column) pairs.
"""
import functools

import numpy as np
import pytest
import torch

import spectral_edge_ref as E1
import spectral_ref as S

MI355X_CUS = 256  # the CPU tests build the turns case for this many workgroups
LDS_BYTES = 158 * 1024

# zinc (seed, n) of tests/golden/make_golden_molecule.py, and its two peptides
MOLECULES = ((1, 9), (2, 12), (3, 17), (4, 23), (5, 30), (6, 38), (10, 14), (11, 14), (7, 60),
             (8, 150))


def _small_bytes_edges(e, nv, k):
    """small_bytes_edges() of csrc/eigpe.hip (kEpSplit = 8, kEpSolvers = 3):
    the bytes a graph of e edges and nv nodes needs to run from the LDS."""
    return 8 * (e * (e + 1) + (3 + 8) * e + (e + 1) + (k - 1) * e + 3 * 5 * e) + 4 * (nv + 1 + 4 * e)


def _lds_limit(k):
    """The largest edge count of a chain molecule with two rings (nv = E - 1)
    that fits kEpLdsBytes."""
    e = 8
    while _small_bytes_edges(e + 1, e, k) <= LDS_BYTES:
        e += 1
    return e


def _molecule(seed, n):
    from hlhgat.synthetic import molecule_edges
    return S.Graph(molecule_edges(np.random.default_rng(seed), n), n)


def _tiny(i):
    """Graph i of the turns batch: 1 .. 12 nodes, mixed shapes, trees and
    graphs with cycles."""
    n = 1 + (i * 7) % 12
    shape = i % 8
    if shape in (0, 3):
        return S.path(n)
    if shape in (1, 4):
        return S.chain_tree(n, i)
    if shape == 2:
        return S.knn(n, 3, i) if n > 1 else S.path(n)
    if shape in (5, 6):
        return S.ring_chords(n, i) if n >= 7 else S.ring(max(n, 3))
    return (S.star, S.complete)[(i // 8) % 2](min(n, 7))


def _turn_graphs(cus):
    """2 cus + 3 small graphs: workgroup i takes graphs i, i + cus, i + 2 cus.
    For i = 0, 1, 2 those are a workspace-path graph (E = 150), an LDS graph
    and a workspace-path graph again; graphs without edges sit in the middle."""
    gs = [_tiny(i) for i in range(2 * cus + 3)]
    for i in range(3):
        gs[i] = E1.chain_rings(148, 3, 150 + i)
        gs[i + cus] = E1.chain_rings(60 + 7 * i, 2, 100 + i)
        gs[i + 2 * cus] = E1.chain_rings(140 - i, 3, 160 + i)
    for i in (cus // 2, cus // 2 + 1, cus + 5, 2 * cus - 1):
        gs[i] = S.Graph(np.zeros((2, 0), np.int64), 1 + i % 2)
    return gs


SWEEP_K = (2, 3, 4, 5, 10, 64)


@functools.lru_cache(maxsize=None)
def _case(name, cus=MI355X_CUS):
    """(graphs, k) of a GPU case below."""
    if name == "tiny":  # E = 0 (one atom), E = 1, a 3-node path (E < k)
        return [S.path(1), S.path(2), S.path(3)], 10
    if name == "tree":  # beta1 = 0: L1 nonsingular
        return [S.chain_tree(20, 20)], 10
    if name == "ring":  # beta1 = 1, doubly degenerate pairs
        return [S.ring(12)], 10
    if name == "harmonic":  # beta1 = 13 >= k: every column harmonic, 12 restarts
        return [S.ring_chords(12, 12)], 10
    if name == "copies":
        return [S.copies(S.ring(7), 3, isolated=2)], 10
    if name == "molecules":
        return [_molecule(s, n) for s, n in MOLECULES], 16
    if name.startswith("k="):
        k = int(name[2:])
        gs = [_molecule(5, 30)]
        if k in (2, 10, 64):
            lim = _lds_limit(k)
            gs += [E1.chain_rings(e - 1, 2, e) for e in (lim - 1, lim, lim + 1)]
        return gs, k
    if name == "workspace":  # E = 257 at k = 64
        return [E1.chain_rings(250, 8, 257)], 64
    if name == "chain450":
        return [E1.chain_rings(440, 11, 450)], 10
    if name == "turns":
        return _turn_graphs(cus), 10
    if name == "undersized":
        return [_molecule(4, 23), E1.chain_rings(148, 3, 150), S.path(10), _molecule(7, 60)], 10
    raise KeyError(name)


CASES = (("tiny", "tree", "ring", "harmonic", "copies", "molecules") + tuple(f"k={k}" for k in SWEEP_K)
         + ("workspace", "chain450", "turns", "undersized"))


def _sides(graphs):
    return [_side(g) for g in graphs]


_SIDES = {}


def _side(g):
    # one EdgeSide (dense L1 + eigh) per Graph object, shared among the tests
    s = _SIDES.get(id(g))
    if s is None or s.g is not g:
        s = _SIDES[id(g)] = E1.EdgeSide(g)
    return s


def _pairs_compared(graphs, k):
    """(pairs, compared) by the fp64 reference alone."""
    sides = _sides(graphs)
    pairs = sum(max(min(k, s.n) - 1, 0) for s in sides)
    compared = sum(len(S.separated(s.eigh[0], k)) for s in sides if s.n)
    return pairs, compared


def _ideal_pe(s, k):
    """float32 of the fp64 eigh vectors 1 .. k-1 of L1, zero past its size."""
    P = np.zeros((s.n, k - 1))
    m = min(k, s.n)
    if m > 1:
        P[:, :m - 1] = s.eigh[1][:, 1:m]
    return P.astype(np.float32)


def _check_case(graphs, k, pe, eoffs):
    compared = 0
    for i, g in enumerate(graphs):
        s = _side(g)
        try:
            compared += S.check_pe(s.L, pe[eoffs[i]:eoffs[i + 1], :k - 1], k, s.eigh)
        except AssertionError as e:
            raise AssertionError(f"graph {i} (E = {s.n}, n = {g.n}): {e}") from None
    return compared


# ---- CPU: the cases and the rule itself ---------------------------------------------

def test_lds_limit_moves_with_k():
    """The restated small_bytes_edges() puts the LDS limit near the node
    side's (E ~ 120 at k = 10) and below it at k = 64."""
    lims = [_lds_limit(k) for k in (2, 10, 64)]
    assert lims == [127, 123, 102], lims
    for k, lim in zip((2, 10, 64), lims):
        gs, _ = _case(f"k={k}")
        assert [g.ei.shape[1] for g in gs[1:]] == [lim - 1, lim, lim + 1]
        assert [g.n for g in gs[1:]] == [lim - 2, lim - 1, lim]


def test_cases_reach_their_branches():
    assert [g.ei.shape[1] for g in _case("tiny")[0]] == [0, 1, 2]
    assert _side(_case("tree")[0][0]).beta1 == 0 and _case("tree")[0][0].ei.shape[1] == 19
    assert _side(_case("ring")[0][0]).beta1 == 1
    g, k = _case("harmonic")
    assert _side(g[0]).beta1 == 13 >= k and _pairs_compared(g, k) == (9, 0)  # stated, not hidden
    assert _side(_case("copies")[0][0]).beta1 == 3
    assert _case("workspace")[0][0].ei.shape[1] == 257
    assert _case("chain450")[0][0].ei.shape[1] == 450
    assert len(_case("turns")[0]) == 2 * MI355X_CUS + 3
    # the k sweep's molecule: every (m - 1) mod 3 of the solver batches
    e30 = _case("k=2")[0][0].ei.shape[1]
    assert e30 >= 29 and {(min(k, e30) - 1) % 3 for k in SWEEP_K} == {0, 1, 2}


def test_molecule_case_compares_half():
    """k = 16 on the fixture's molecules: at least half of the (graph,
    column) pairs are compared vector for vector, on both sides."""
    graphs, k = _case("molecules")
    pairs, compared = _pairs_compared(graphs, k)
    print("edge side:", compared, "of", pairs)
    assert 2 * compared >= pairs > 0, (compared, pairs)
    npairs = sum(min(k, g.n) - 1 for g in graphs)
    ncomp = sum(len(S.separated(g.eigh[0], k)) for g in graphs)
    print("node side:", ncomp, "of", npairs)
    assert 2 * ncomp >= npairs, (ncomp, npairs)


@pytest.mark.parametrize("name", CASES)
def test_check_pe_accepts_rounded_eigh(name):
    """check_pe accepts float32(eigh(L1) vectors) for every GPU case."""
    graphs, k = _case(name)
    pairs, compared = _pairs_compared(graphs, k)
    got = 0
    for g in graphs:
        s = _side(g)
        got += S.check_pe(s.L, _ideal_pe(s, k).astype(np.float64), k, s.eigh)
    assert got == compared and pairs > 0


def test_check_pe_rejects_planted_errors():
    g, k = _molecule(5, 30), 10
    s = _side(g)
    assert s.beta1 >= 1
    P = _ideal_pe(s, k).astype(np.float64)
    assert S.check_pe(s.L, P, k, s.eigh) > 0
    w, V = s.eigh
    # the columns starting at eigenvector 0 instead of 1
    bad = V[:, 0:k - 1].astype(np.float32).astype(np.float64)
    with pytest.raises(AssertionError):
        S.check_pe(s.L, bad, k, s.eigh)
    # L0's vectors mapped through B1^T without the harmonic block in front
    w0, V0 = g.eigh
    B = E1.incidence(g.ei, g.n)
    bad = (B.T @ V0[:, 1:k]) / np.sqrt(w0[1:k])[None, :]
    assert np.abs(bad.T @ bad - np.eye(k - 1)).max() < 1e-9  # orthonormal eigenvectors of L1 ...
    with pytest.raises(AssertionError, match="residual"):  # ... of the wrong eigenvalues
        S.check_pe(s.L, bad.astype(np.float32).astype(np.float64), k, s.eigh)
    # on a tree the same map IS the answer (no harmonic block)
    t = _case("tree")[0][0]
    ts = _side(t)
    w0, V0 = t.eigh
    ok = (E1.incidence(t.ei, t.n).T @ V0[:, 1:k + 1]) / np.sqrt(w0[1:k + 1])[None, :]
    S.check_pe(ts.L, ok[:, 1:].astype(np.float32).astype(np.float64), k, ts.eigh)
    # an unnormalised column
    bad = P.copy()
    bad[:, 5] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="orthonormality"):
        S.check_pe(s.L, bad, k, s.eigh)
    # a nonzero column past E - 1
    small = _side(S.path(4))
    P = _ideal_pe(small, k).astype(np.float64)
    assert S.check_pe(small.L, P, k, small.eigh) == 2
    P[1, 2] = 1e-30
    with pytest.raises(AssertionError, match="past the graph's size"):
        S.check_pe(small.L, P, k, small.eigh)


# ---- GPU --------------------------------------------------------------------------------

def _eig_pe_edges_c(graphs, k, dev, max_edges, ws_edges=None, pad=0):
    """hlhgat_eig_pe_edges through the C entry with device pointers:
    max_edges as given, the workspace sized for ws_edges (default max_edges),
    pe rows of k - 1 + pad floats that start as NaN, so what the kernel did
    not write shows.  Returns (pe [E, k - 1 + pad], edge offsets)."""
    from hlhgat import ops
    from hlhgat._lib import LIB, check
    ei, ns, es, eoffs = E1.batch(graphs)
    N, B, E = int(sum(ns)), len(ns), ei.shape[1]
    ei = torch.from_numpy(ei).to(dev)
    node_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)).to(dev)
    edge_ptr = torch.from_numpy(eoffs).to(dev)
    inc = ops.incidence(ei, N)
    ld = k - 1 + pad
    pe = torch.full((E, ld), float("nan"), dtype=torch.float32, device=dev)
    wsb = int(LIB.hlhgat_eig_pe_edges_workspace_bytes(B, max_edges if ws_edges is None else ws_edges, k))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_eig_pe_edges(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr(), ei.data_ptr(), E, N,
                                  node_ptr.data_ptr(), edge_ptr.data_ptr(), B, max_edges, k,
                                  pe.data_ptr(), ld, ws.data_ptr(), wsb, ops._stream(ei)),
          "eig_pe_edges")
    torch.cuda.synchronize()
    return pe, eoffs


def _run_case(name, dev):
    from hlhgat import ops
    graphs, k = _case(name)
    ei, ns, es, eoffs = E1.batch(graphs)
    ops.check_device_errors()
    pe = ops.eig_pe_edges(torch.from_numpy(ei).to(dev), ns, es, k)
    torch.cuda.synchronize()
    ops.check_device_errors()
    assert pe.shape == (eoffs[-1], k - 1)
    compared = _check_case(graphs, k, pe.cpu().numpy().astype(np.float64), eoffs)
    assert compared == _pairs_compared(graphs, k)[1]
    return compared


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "tree", "ring", "harmonic", "copies", "workspace", "chain450"])
def test_eig_pe_edges_case(cuda, name):
    _run_case(name, cuda)


@pytest.mark.gpu
def test_eig_pe_edges_molecules_k16(cuda):
    graphs, k = _case("molecules")
    compared = _run_case("molecules", cuda)
    pairs = _pairs_compared(graphs, k)[0]
    assert 2 * compared >= pairs, (compared, pairs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", SWEEP_K)
def test_eig_pe_edges_k_sweep(cuda, k):
    """k = 2 .. 64 on one 30-atom molecule; for k = 2, 10, 64 also the three
    edge counts around that k's LDS limit."""
    _run_case(f"k={k}", cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 65])
def test_eig_pe_edges_k_out_of_range_raises(cuda, k):
    from hlhgat import ops
    ei, ns, es, _ = E1.batch([S.path(5)])
    with pytest.raises(RuntimeError, match="eig_pe_edges"):
        ops.eig_pe_edges(torch.from_numpy(ei).to(cuda), ns, es, k)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.gpu
def test_eig_pe_edges_workgroups_take_graphs_in_turn(cuda):
    """2 CUs + 3 graphs: every workgroup runs its loop two or three times,
    the first three alternate between the workspace and the LDS, graphs
    without edges sit between the others.  Row padding stays untouched and a
    second launch gives the same bits; device counts through ops give them
    too."""
    from hlhgat import ops
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    graphs, k = _case("turns", cus)
    assert len(graphs) == 2 * cus + 3
    mx = max(g.ei.shape[1] for g in graphs)
    ops.check_device_errors()
    pe, eoffs = _eig_pe_edges_c(graphs, k, cuda, mx, pad=3)
    pe2, _ = _eig_pe_edges_c(graphs, k, cuda, mx, pad=3)
    ei, ns, es, _ = E1.batch(graphs)
    pe3 = ops.eig_pe_edges(torch.from_numpy(ei).to(cuda), torch.tensor(ns, device=cuda),
                           torch.tensor(es, device=cuda), k, max_edges=mx, n_nodes=sum(ns))
    ops.check_device_errors()
    assert torch.equal(_bits(pe), _bits(pe2))
    assert torch.equal(_bits(pe[:, :k - 1].contiguous()), _bits(pe3))
    pe = pe.cpu().numpy()
    assert np.isnan(pe[:, k - 1:]).all()  # the row padding
    assert not np.isnan(pe[:, :k - 1]).any()
    _check_case(graphs, k, pe.astype(np.float64), eoffs)


@pytest.mark.gpu
def test_eig_pe_edges_undersized_max_edges_raises(cuda):
    """Device counts with max_edges = 140 below the 150-edge graph (the
    workspace itself sized for 150, so nothing can land out of bounds): that
    graph gets zero rows, HLHGAT_DEVERR_EIGPE_SIZE is raised, the other
    graphs are computed."""
    from hlhgat import _lib, ops
    graphs, k = _case("undersized")
    assert graphs[1].ei.shape[1] == 150 and _lib.LIB.hlhgat_version() >= 111
    ops.check_device_errors()
    try:
        pe, eoffs = _eig_pe_edges_c(graphs, k, cuda, 140, ws_edges=150)
        assert ops.device_errors() == _lib.DEVERR_EIGPE_SIZE
        with pytest.raises(RuntimeError, match="eig_pe"):
            ops.check_device_errors()
    finally:
        ops.clear_device_errors()
    pe = pe.cpu().numpy().astype(np.float64)
    assert np.all(pe[eoffs[1]:eoffs[2]] == 0.0)
    keep = [0, 2, 3]
    sub_offs = np.concatenate([[0], np.cumsum([graphs[i].ei.shape[1] for i in keep])])
    sub_pe = np.concatenate([pe[eoffs[i]:eoffs[i + 1]] for i in keep])
    _check_case([graphs[i] for i in keep], k, sub_pe, sub_offs)
    # the true bound: clean, and every graph computed
    pe, eoffs = _eig_pe_edges_c(graphs, k, cuda, 150)
    ops.check_device_errors()
    _check_case(graphs, k, pe.cpu().numpy().astype(np.float64), eoffs)
