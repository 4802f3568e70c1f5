"""hlhgat_eig_pe (ops.eig_pe): the eigenvector PE and lambda_max of every
graph of a batch in one launch -- the reference's per-sample eig_pe(L0)
(lib/Hodge_Dataset.py:97-112: eigenvectors 1 .. k-1 of a dense eigh) and
torch.linalg.eigh(L0).max() (lib/Hodge_Dataset.py:782) -- against numpy's
fp64 eigh of the same dense L0 = B1 B1^T:

* lambda_max within 1e-12 relative;
* every PE column whose eigenvalue is separated from its neighbours by more
  than 1e-3 equals the reference eigenvector up to sign within 2e-6 (the
  output is float32 of an fp64 computation);
* every column (clusters included: disconnected graphs, isolated nodes, equal
  eigenvalues) is an eigenvector of its eigenvalue (residual <= 1e-5) and the
  columns of a graph are orthonormal within 1e-5;
* a graph with fewer than k nodes has zero columns past its own size;
* graphs too large for the LDS (the workspace path) agree as well.
"""
import functools

import numpy as np
import pytest
import torch

import spectral_ref as S
from spectral_ref import dense_l0 as _dense_l0

K = 10


def _graphs(seed):
    """Superpixel kNN graphs with dropout (isolated nodes appear), sizes on
    both sides of the LDS limit, a disconnected graph, a path, a star, tiny
    graphs."""
    from hlhgat.pipeline import superpixel_raw, to_undirected_min
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate([118, 40, 150, 97, 200, 64, 123, 130]):
        r = superpixel_raw(300 + i + 17 * seed, n=n)
        ei, _ = to_undirected_min(r.edge_index, r.edge_attr, n)
        ei = ei[:, ei[0] < ei[1]]
        if i % 2 == 0:
            ei = ei[:, rng.random(ei.shape[1]) >= 0.5]
        out.append((ei, n))
    # two disjoint 5-cycles + 3 isolated nodes; a path; a star; n < k; one node
    cyc = [(j, (j + 1) % 5) for j in range(5)]
    e = [(min(a, b), max(a, b)) for a, b in cyc] + [(min(a, b) + 5, max(a, b) + 5) for a, b in cyc]
    out.append((np.array(e, np.int64).T, 13))
    out.append((np.array([[j, j + 1] for j in range(29)], np.int64).T, 30))
    out.append((np.array([[0, j] for j in range(1, 25)], np.int64).T, 25))
    out.append((np.array([[0, 1], [1, 2], [2, 3], [0, 3], [1, 4]], np.int64).T, 6))
    out.append((np.zeros((2, 0), np.int64), 1))
    return out


def _batch(graphs, dev):
    offs = np.concatenate([[0], np.cumsum([n for _, n in graphs])])
    ei = np.concatenate([e + o for (e, _), o in zip(graphs, offs[:-1])], axis=1)
    return torch.from_numpy(np.ascontiguousarray(ei)).to(dev), [n for _, n in graphs], offs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_eig_pe_matches_fp64_eigh(cuda, seed):
    from hlhgat import ops
    graphs = _graphs(seed)
    ei, ns, offs = _batch(graphs, cuda)
    pe, lmax = ops.eig_pe(ei, ns, K)
    torch.cuda.synchronize()
    pe, lmax = pe.cpu().numpy().astype(np.float64), lmax.cpu().numpy()
    assert pe.shape == (offs[-1], K - 1)
    for g, (e, n) in enumerate(graphs):
        L = _dense_l0(e, n)
        w, V = np.linalg.eigh(L)
        assert abs(lmax[g] - w[-1]) <= 1e-12 * max(w[-1], 1.0), (g, lmax[g], w[-1])
        P = pe[offs[g]:offs[g + 1]]
        m = min(K, n)
        assert np.all(P[:, m - 1:] == 0.0), g  # columns past the graph's size
        if m <= 1:
            continue
        P = P[:, :m - 1]
        lam = w[1:m]
        # eigenvectors of their eigenvalues, orthonormal
        res = np.abs(L @ P - P * lam[None, :]).max()
        assert res <= 1e-5 * max(1.0, w[-1]), (g, res)
        orth = np.abs(P.T @ P - np.eye(m - 1)).max()
        assert orth <= 1e-5, (g, orth)
        # separated eigenvalues: the reference vector up to sign
        for c in range(m - 1):
            j = c + 1
            gap = min(w[j] - w[j - 1], (w[j + 1] - w[j]) if j + 1 < n else np.inf)
            if gap > 1e-3:
                s = np.sign(P[:, c] @ V[:, j]) or 1.0
                err = np.abs(P[:, c] * s - V[:, j]).max()
                assert err <= 2e-6, (g, c, gap, err)


@pytest.mark.gpu
def test_eig_pe_device_counts_and_repeatability(cuda):
    """Device node counts (max_nodes given) give the same bits as host
    counts, and a second launch the same bits as the first."""
    from hlhgat import ops
    graphs = _graphs(2)
    ei, ns, _ = _batch(graphs, cuda)
    a, la = ops.eig_pe(ei, ns, K)
    b, lb = ops.eig_pe(ei, torch.tensor(ns, device=cuda), K, max_nodes=max(ns))
    c, lc = ops.eig_pe(ei, ns, K)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert torch.equal(a, c) and torch.equal(la, lc)


# ---- beyond the CIFAR sizes ----------------------------------------------------
# The cases below reach what k = 10 on 13 graphs of <= 200 nodes does not: a
# workgroup's second and third graph (more graphs than CUs), the n <= 0 path,
# every `split` width of orthogonalise() (8, 4, 2, 1) and its second trips
# (n > 1024), k from 2 to 64 (the solver batches of 3, lam[64], the LDS limit
# that moves with k), and a max_nodes smaller than a graph with device counts.
# Each case is a list of spectral_ref.Graph and a k; the CPU tests hold
# spectral_ref.check_pe to them before any device does.

MI355X_CUS = 256  # the CPU tests build the turns case for this many workgroups


def _small_bytes(n, nnz, k):
    """small_bytes() of csrc/eigpe.hip (kEpSplit = 8, kEpSolvers = 3): the
    bytes a graph needs to run from the LDS."""
    return 8 * (n * (n + 1) + (3 + 8) * n + (n + 1) + (k - 1) * n + 3 * 5 * n) + 4 * (n + 1 + nnz)


def _lds_limit(k):
    """The largest ring-with-chords size (nnz = 4 n) that fits kEpLdsBytes."""
    n = 5
    while _small_bytes(n + 1, 4 * (n + 1), k) <= 158 * 1024:
        n += 1
    return n


def _tiny(i):
    """Graph i of the turns batch: n = 1 .. 12, mixed shapes."""
    n = 1 + (i * 7) % 12
    shape = i % 8
    if shape in (0, 3):
        return S.path(n)
    if shape in (1, 4, 6):
        return S.chain_tree(n, i)
    if shape == 2:
        return S.knn(n, 3, i) if n > 1 else S.path(n)
    if shape == 5:
        return S.ring_chords(n, i) if n >= 7 else S.ring(max(n, 3))
    return (S.star, S.complete)[(i // 8) % 2](n)


def _turn_graphs(cus):
    """2 cus + 3 graphs: workgroup i takes graphs i, i + cus, i + 2 cus.  For
    i = 0, 1, 2 those are a workspace-path graph (n = 150), an LDS graph and a
    workspace-path graph again; empty graphs sit in the middle."""
    gs = [_tiny(i) for i in range(2 * cus + 3)]
    for i in range(3):
        gs[i] = S.ring_chords(150, 150 + i)
        gs[i + cus] = S.ring_chords(100 + 7 * i, 100 + i)
        gs[i + 2 * cus] = S.ring_chords(150 - i, 160 + i)
    for i in (cus // 2, cus // 2 + 1, cus + 5, 2 * cus - 1):
        gs[i] = S.Graph(np.zeros((2, 0), np.int64), 0)
    return gs


@functools.lru_cache(maxsize=None)
def _sweep_base():
    return (S.ring_chords(130, 130), S.ring_chords(97, 97), S.knn(50, 8, 1), S.chain_tree(70, 2),
            S.path(30), S.path(3), S.path(2), S.path(1))


def _sweep_graphs(k):
    gs = list(_sweep_base())
    if k in (2, 10, 64):
        ns = _lds_limit(k)
        gs += [S.ring_chords(n, n) for n in (ns - 1, ns, ns + 1)]
    return gs


SWEEP_K = (2, 3, 4, 5, 10, 64)
SIZE_CLASSES = (128, 129, 256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def _case(name, cus=MI355X_CUS):
    """(graphs, k) of a GPU case below."""
    if name == "turns":
        return _turn_graphs(cus), 10
    if name.startswith("k="):
        return _sweep_graphs(int(name[2:])), int(name[2:])
    if name == "sizes":
        return ([S.ring_chords(n, n) for n in SIZE_CLASSES]
                + [S.copies(S.ring_chords(70, 1), 4, isolated=5)]), 10
    if name == "n257-k64":
        return [S.ring_chords(257, 257)], 64
    if name == "n1030":
        return [S.ring_chords(1030, 1030)], 10
    if name == "undersized":
        return [S.ring_chords(40, 40), S.ring_chords(150, 150), S.path(10), S.ring_chords(130, 130)], 10
    raise KeyError(name)


CASES = ("turns",) + tuple(f"k={k}" for k in SWEEP_K) + ("sizes", "n257-k64", "n1030", "undersized")


def _half_compared(graphs, k):
    """At least half of the (graph, column) pairs of a case are compared
    vector for vector (numpy alone); returns (compared, pairs)."""
    pairs = sum(max(min(k, g.n) - 1, 0) for g in graphs)
    compared = sum(len(S.separated(g.eigh[0], k)) for g in graphs if g.n)
    assert 2 * compared >= pairs, (compared, pairs)
    return compared, pairs


def _ideal_pe(g, k):
    """float32 of the fp64 eigh vectors 1 .. k-1, zero past the graph's size."""
    P = np.zeros((g.n, k - 1))
    m = min(k, g.n)
    if m > 1:
        P[:, :m - 1] = g.eigh[1][:, 1:m]
    return P.astype(np.float32)


def _check_case(graphs, k, pe, lmax, offs):
    """Every graph of a case against spectral_ref: check_pe and lambda_max
    within 1e-12 relative (exactly 0 for an empty graph)."""
    compared = 0
    for i, g in enumerate(graphs):
        if g.n == 0:
            assert lmax[i] == 0.0, (i, lmax[i])
            continue
        assert abs(lmax[i] - g.lmax) <= 1e-12 * max(g.lmax, 1.0), (i, g.n, lmax[i], g.lmax)
        try:
            compared += S.check_pe(g.L, pe[offs[i]:offs[i + 1], :k - 1], k, g.eigh)
        except AssertionError as e:
            raise AssertionError(f"graph {i} (n = {g.n}): {e}") from None
    return compared


def test_lds_limit_moves_with_k():
    """The restated small_bytes() puts the LDS limit where eigpe.hip's header
    says (n ~ 120 at k = 10) and below it at k = 64."""
    assert [_lds_limit(k) for k in (2, 10, 64)] == [127, 123, 102]


@pytest.mark.parametrize("name", CASES)
def test_check_pe_accepts_rounded_eigh(name):
    """check_pe accepts float32(eigh vectors) for every GPU case -- float32
    rounding alone leaves the residual and the orthonormality two orders
    inside its bounds -- and compares at least half of the columns vector
    for vector."""
    graphs, k = _case(name)
    compared, pairs = _half_compared(graphs, k)
    got = 0
    for g in graphs:
        P = _ideal_pe(g, k).astype(np.float64)
        got += S.check_pe(g.L, P, k, g.eigh)
        m = min(k, g.n)
        if m > 1:
            w = g.eigh[0]
            Q = P[:, :m - 1]
            assert np.abs(g.L @ Q - Q * w[None, 1:m]).max() <= S.RES_TOL / 100 * max(1.0, w[-1])
            assert np.abs(Q.T @ Q - np.eye(m - 1)).max() <= S.ORTH_TOL / 100
    assert got == compared and pairs > 0


def test_check_pe_rejects_planted_errors():
    g, k = S.ring_chords(129, 129), 10
    P = _ideal_pe(g, k).astype(np.float64)
    assert S.check_pe(g.L, P, k, g.eigh) == k - 1
    assert S.check_pe(g.L, P, k) == k - 1  # its own eigh
    bad = P.copy()
    bad[:, [3, 4]] = bad[:, [4, 3]]  # two adjacent columns swapped
    with pytest.raises(AssertionError):
        S.check_pe(g.L, bad, k, g.eigh)
    bad = P.copy()
    bad[:, 5] *= 1.0 + 1e-4  # one column scaled
    with pytest.raises(AssertionError, match="orthonormality"):
        S.check_pe(g.L, bad, k, g.eigh)
    bad = P.copy()
    bad[17, 2] += 1e-4  # one entry moved
    with pytest.raises(AssertionError):
        S.check_pe(g.L, bad, k, g.eigh)
    small = S.path(6)
    P = _ideal_pe(small, k).astype(np.float64)
    assert S.check_pe(small.L, P, k, small.eigh) == 5
    P[2, 7] = 1e-30  # a value in a column past the graph's size
    with pytest.raises(AssertionError, match="past the graph's size"):
        S.check_pe(small.L, P, k, small.eigh)


def _eig_pe_c(graphs, k, dev, max_nodes, ws_nodes=None, pad=0):
    """hlhgat_eig_pe through the C entry with DEVICE node counts: max_nodes as
    given, the workspace sized for ws_nodes (default max_nodes), pe rows of
    k - 1 + pad floats.  pe and lmax start as NaN, so what the kernel did not
    write shows.  Returns (pe [N, k - 1 + pad], lmax [B], offs)."""
    from hlhgat import ops
    from hlhgat._lib import LIB, check
    ei, ns, offs = S.batch(graphs)
    N, B, E = int(offs[-1]), len(ns), ei.shape[1]
    ei = torch.from_numpy(ei).to(dev)
    node_ptr = torch.from_numpy(offs).to(dev)
    inc = ops.incidence(ei, N)
    ld = k - 1 + pad
    pe = torch.full((N, ld), float("nan"), dtype=torch.float32, device=dev)
    lmax = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    wsb = int(LIB.hlhgat_eig_pe_workspace_bytes(B, max_nodes if ws_nodes is None else ws_nodes, k))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_eig_pe(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr(), ei.data_ptr(), E, N,
                            node_ptr.data_ptr(), B, max_nodes, k, pe.data_ptr(), ld,
                            lmax.data_ptr(), ws.data_ptr(), wsb, ops._stream(ei)), "eig_pe")
    torch.cuda.synchronize()
    return pe, lmax, offs


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.gpu
def test_eig_pe_workgroups_take_graphs_in_turn(cuda):
    """2 CUs + 3 graphs: every workgroup runs its loop two or three times,
    the first three alternate between the workspace and the LDS, empty graphs
    (lmax 0, no row) sit between the others.  Row padding stays untouched and
    a second launch gives the same bits."""
    from hlhgat import ops
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    graphs, k = _case("turns", cus)
    assert len(graphs) == 2 * cus + 3
    _half_compared(graphs, k)
    mx = max(g.n for g in graphs)
    ops.check_device_errors()
    pe, lmax, offs = _eig_pe_c(graphs, k, cuda, mx, pad=3)
    pe2, lmax2, _ = _eig_pe_c(graphs, k, cuda, mx, pad=3)
    ops.check_device_errors()
    assert torch.equal(_bits(pe), _bits(pe2)) and torch.equal(_bits(lmax), _bits(lmax2))
    pe, lmax = pe.cpu().numpy(), lmax.cpu().numpy()
    assert np.isnan(pe[:, k - 1:]).all()  # the row padding
    assert not np.isnan(pe[:, :k - 1]).any() and not np.isnan(lmax).any()
    _check_case(graphs, k, pe.astype(np.float64), lmax, offs)


def _run_case(name, dev):
    from hlhgat import ops
    graphs, k = _case(name)
    _half_compared(graphs, k)
    ei, ns, offs = S.batch(graphs)
    pe, lmax = ops.eig_pe(torch.from_numpy(ei).to(dev), ns, k)
    torch.cuda.synchronize()
    assert pe.shape == (offs[-1], k - 1)
    _check_case(graphs, k, pe.cpu().numpy().astype(np.float64), lmax.cpu().numpy(), offs)


@pytest.mark.gpu
@pytest.mark.parametrize("k", SWEEP_K)
def test_eig_pe_k_sweep(cuda, k):
    """k = 2 .. 64 on graphs of 1 .. 130 nodes (n < k, n = 1, 2, 3 among
    them): every (m - 1) mod 3 of the solver batches, lam[64]; for k = 2, 10,
    64 also the three ring-with-chords sizes around that k's LDS limit."""
    _run_case(f"k={k}", cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 65])
def test_eig_pe_k_out_of_range_raises(cuda, k):
    from hlhgat import ops
    ei, ns, _ = S.batch([S.path(5)])
    with pytest.raises(RuntimeError, match="eig_pe"):
        ops.eig_pe(torch.from_numpy(ei).to(cuda), ns, k)


@pytest.mark.gpu
def test_eig_pe_size_classes(cuda):
    """n on both sides of 128, 256 and 512 (orthogonalise()'s split = 8, 4,
    2, 1) in one launch, with four disjoint copies of a 70-node graph plus 5
    isolated nodes (4-fold eigenvalues, a 9-fold zero: the restart branch on
    the workspace path)."""
    _run_case("sizes", cuda)


@pytest.mark.gpu
def test_eig_pe_k64_on_workspace_path(cuda):
    _run_case("n257-k64", cuda)


@pytest.mark.gpu
def test_eig_pe_above_1024_nodes(cuda):
    """n = 1030 > kEpThreads: every per-node loop and the coefficient loop
    of orthogonalise() take a second trip."""
    _run_case("n1030", cuda)


@pytest.mark.gpu
def test_eig_pe_undersized_max_nodes_raises(cuda):
    """Device counts with max_nodes = 140 below the 150-node graph (the
    workspace itself sized for 150, so nothing can land out of bounds): that
    graph gets zero rows and lmax 0, HLHGAT_DEVERR_EIGPE_SIZE is raised, the
    other graphs are computed."""
    from hlhgat import _lib, ops
    graphs, k = _case("undersized")
    assert _lib.DEVERR_EIGPE_SIZE == 32 and _lib.LIB.hlhgat_version() >= 107
    ops.check_device_errors()
    try:
        pe, lmax, offs = _eig_pe_c(graphs, k, cuda, 140, ws_nodes=150)
        assert ops.device_errors() == _lib.DEVERR_EIGPE_SIZE
        with pytest.raises(RuntimeError, match="eig_pe"):
            ops.check_device_errors()
    finally:
        ops.clear_device_errors()
    pe, lmax = pe.cpu().numpy().astype(np.float64), lmax.cpu().numpy()
    assert lmax[1] == 0.0 and np.all(pe[offs[1]:offs[2]] == 0.0)
    keep = [0, 2, 3]
    sub_offs = np.concatenate([[0], np.cumsum([graphs[i].n for i in keep])])
    sub_pe = np.concatenate([pe[offs[i]:offs[i + 1]] for i in keep])
    _check_case([graphs[i] for i in keep], k, sub_pe, lmax[keep], sub_offs)
    # the true bound: clean, and every graph computed
    pe, lmax, offs = _eig_pe_c(graphs, k, cuda, 150)
    ops.check_device_errors()
    _check_case(graphs, k, pe.cpu().numpy().astype(np.float64), lmax.cpu().numpy(), offs)
