"""MLGC_Weight on the host (hlhgat_mlgc_prune, hodge_dataset.mlgc_weight /
brain_levels) against the reference-generated fixture
(tests/golden/make_golden_mlgc_weight.py), hand cases for the two pruning
passes, and the argument errors of the three new C entries.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden

INF = np.float32(np.inf)


@pytest.fixture(scope="module")
def gold():
    return load_golden("mlgc_weight_small")


def _graph(gold, gi):
    from hlhgat.hodge_dataset import PairData
    p = f"g{gi}/"
    n = int(gold[p + "num_node1"])
    d = PairData(x_s=torch.from_numpy(gold[p + "x_s"]), x_t=torch.ones(n, 1))
    d.edge_index = torch.from_numpy(gold[p + "edge_index"])
    d.num_node1, d.num_edge1, d.num_nodes = n, int(gold[p + "edge_index"].shape[1]), n
    return d


@pytest.mark.parametrize("gi", [0, 1, 2, 3])
def test_mlgc_weight_matches_reference_golden(gold, gi):
    """The reference's MLGC_Weight output on the brain skeleton and three
    signed-weight kNN graphs: every stored array, inf positions included."""
    from hlhgat.hodge_dataset import graclus, mlgc_weight
    p = f"g{gi}/"
    d = _graph(gold, gi)
    lab = graclus(gold[p + "edge_index"], int(d.num_node1), weight=gold[p + "x_s"].reshape(-1),
                  perm=gold[p + "perm"])
    assert np.array_equal(lab, gold[p + "graclus"])
    coarse, c_node, c_edge = mlgc_weight(d, perm=gold[p + "perm"])
    assert c_node.dtype == torch.float32 and c_edge.dtype == torch.float32
    assert torch.equal(c_node, torch.from_numpy(gold[p + "c_node"]))
    assert torch.equal(c_edge, torch.from_numpy(gold[p + "c_edge"]))
    assert torch.equal(coarse.edge_index, torch.from_numpy(gold[p + "coarse/edge_index"]))
    assert torch.equal(coarse.x_s, torch.from_numpy(gold[p + "coarse/x_s"]))
    assert int(coarse.num_node1) == int(gold[p + "coarse/num_node1"])
    assert torch.equal(coarse.x_t, torch.ones(int(coarse.num_node1), 1))


def test_fixture_exercises_both_passes(gold):
    dropped = sum(int(np.isinf(gold[f"g{gi}/c_node"]).sum()) for gi in (1, 2, 3))
    assert dropped >= 1
    for gi in (1, 2, 3):
        p = f"g{gi}/"
        lab, ei = gold[p + "graclus"], gold[p + "edge_index"]
        cut = int((lab[ei[0]] != lab[ei[1]]).sum())
        assert int(np.isinf(gold[p + "c_edge"]).sum()) > ei.shape[1] - cut  # pruned edges exist


def test_brain_levels_on_the_skeleton(gold):
    """brain_levels(pool_num=2): level 0's pos_* are the fixture's; level 1 is
    consistent with level 2 (finite ids below the next level's counts, which
    equal its sizes)."""
    from hlhgat.hodge_dataset import brain_levels
    fine = _graph(gold, 0)
    levels = brain_levels(fine, pool_num=2, perms=[gold["g0/perm"], None], seed=3)
    assert len(levels) == 3 and levels[0] is fine
    assert torch.equal(levels[0].pos_t, torch.from_numpy(gold["g0/c_node"]))
    assert torch.equal(levels[0].pos_s, torch.from_numpy(gold["g0/c_edge"]))
    assert torch.equal(levels[1].edge_index, torch.from_numpy(gold["g0/coarse/edge_index"]))
    assert getattr(levels[2], "pos_t", None) is None
    for p in (0, 1):
        cur, nxt = levels[p], levels[p + 1]
        assert tuple(cur.pos_t.shape) == (int(cur.num_node1), 1)
        assert tuple(cur.pos_s.shape) == (cur.edge_index.shape[1], 1)
        n1, e1 = int(nxt.num_node1), int(nxt.edge_index.shape[1])
        assert nxt.x_t.shape[0] == n1 and nxt.x_s.shape[0] == e1 and int(nxt.num_edge1) == e1
        ft = cur.pos_t[~torch.isinf(cur.pos_t)]
        fs = cur.pos_s[~torch.isinf(cur.pos_s)]
        assert ft.numel() and float(ft.max()) == n1 - 1 and float(ft.min()) == 0
        assert fs.numel() and float(fs.max()) == e1 - 1 and float(fs.min()) == 0
        assert torch.unique(ft).numel() == n1 and torch.unique(fs).numel() == e1
        assert bool((nxt.edge_index[0] < nxt.edge_index[1]).all())


def _map(n, edges, lab):
    from hlhgat.hodge_dataset import mlgc_map
    ei = np.asarray(edges, np.int64).T.reshape(2, -1)
    return ei, mlgc_map(np.asarray(lab, np.int64), ei)


def test_prune_without_flags_is_identity():
    from hlhgat.hodge_dataset import mlgc_prune
    from hlhgat.synthetic import knn_edges
    rng = np.random.default_rng(5)
    n = 40
    ei = np.asarray(knn_edges(rng.random((n, 2)), 6), np.int64)
    lab = np.arange(n) // 2 * 2
    _, (cn, ce, e1, n1) = _map(n, ei.T, lab)
    cn2, ce2, e12, n12 = mlgc_prune(cn, ce, e1, n1, prune_single=False, drop_isolated=False)
    assert cn2.dtype == np.float32 and np.array_equal(cn2, cn.astype(np.float32))
    assert np.array_equal(ce2, ce) and np.array_equal(e12, e1) and n12 == n1


def test_prune_triangle_with_pendant():
    """Triangle 0-1-2 plus pendant 2-3, clusters {0,1} {2} {3}: coarse edges
    (0,1) with support 2 and (1,2) with support 1.  Pruning removes (1,2);
    coarse node 2 (fine node 3) is then isolated and dropped."""
    from hlhgat.hodge_dataset import mlgc_prune
    _, (cn, ce, e1, n1) = _map(4, [(0, 1), (0, 2), (1, 2), (2, 3)], [0, 0, 2, 3])
    assert np.array_equal(ce, [INF, 0, 0, 1]) and n1 == 3
    a = mlgc_prune(cn, ce, e1, n1, prune_single=True, drop_isolated=False)
    assert np.array_equal(a[0], [0, 0, 1, 2]) and np.array_equal(a[1], [INF, 0, 0, INF])
    assert np.array_equal(a[2], [[0], [1]]) and a[3] == 3
    b = mlgc_prune(cn, ce, e1, n1)
    assert np.array_equal(b[0], [0, 0, 1, INF]) and np.array_equal(b[1], [INF, 0, 0, INF])
    assert np.array_equal(b[2], [[0], [1]]) and b[3] == 2
    # isolated nodes alone: nothing is isolated before the pruning
    c = mlgc_prune(cn, ce, e1, n1, prune_single=False, drop_isolated=True)
    assert np.array_equal(c[0], [0, 0, 1, 2]) and np.array_equal(c[1], ce) and c[3] == 3


def _two_cliques(bridges):
    """Two 4-cliques {0..3} and {4..7}, clusters {0,1} {2,3} {4,5} {6,7}."""
    edges = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    edges += [(i, j) for i in range(4, 8) for j in range(i + 1, 8)]
    edges += bridges
    return _map(8, edges, [0, 0, 2, 2, 4, 4, 6, 6])


def test_prune_bridge_between_cliques():
    """One bridge 3-4: coarse (1,2) has support 1 and is pruned; every coarse
    node keeps its clique edge (support 4), so nothing is isolated and the
    ids of the later coarse edge close up."""
    from hlhgat.hodge_dataset import mlgc_prune
    ei, (cn, ce, e1, n1) = _two_cliques([(3, 4)])
    assert np.array_equal(e1, [[0, 2, 1], [1, 3, 2]])
    cn2, ce2, e12, n12 = mlgc_prune(cn, ce, e1, n1)
    assert n12 == 4 and np.array_equal(cn2, cn.astype(np.float32))
    assert np.array_equal(e12, [[0, 2], [1, 3]])
    assert ce2[-1] == INF and ce[-1] == 2
    assert np.array_equal(ce2[:-1], ce[:-1])


def test_prune_two_bridges_keep_everything():
    """Bridges 2-4 and 3-5 map onto the same coarse pair (1,2): support 2."""
    from hlhgat.hodge_dataset import mlgc_prune
    ei, (cn, ce, e1, n1) = _two_cliques([(2, 4), (3, 5)])
    cn2, ce2, e12, n12 = mlgc_prune(cn, ce, e1, n1)
    assert n12 == n1 == 4 and np.array_equal(ce2, ce) and np.array_equal(e12, e1)
    assert np.array_equal(cn2, cn.astype(np.float32))


def test_new_entries_report_argument_errors_without_gpu():
    """Argument validation of hlhgat_mlgc_prune, hlhgat_mlgc_device and its
    workspace query runs before any HIP call."""
    from hlhgat import _lib
    L = _lib.LIB
    assert L.hlhgat_version() >= 108 and _lib.DEVERR_MLGC_RANGE == 64
    n1, ne = C.c_int64(0), C.c_int64(0)
    assert L.hlhgat_mlgc_prune(-1, 0, 0, None, None, None, None, C.byref(n1), C.byref(ne)) == 1
    assert b"sizes" in L.hlhgat_last_error()
    assert L.hlhgat_mlgc_prune(1 << 24, 0, 0, None, None, None, None, C.byref(n1), C.byref(ne)) == 1
    assert L.hlhgat_mlgc_prune(0, 0, 8, None, None, None, None, C.byref(n1), C.byref(ne)) == 1
    assert b"flag" in L.hlhgat_last_error()
    assert L.hlhgat_mlgc_prune(2, 0, 0, None, None, None, None, C.byref(n1), C.byref(ne)) == 1
    assert b"NULL" in L.hlhgat_last_error()
    cn = np.array([0, 5], np.int64)
    out = np.zeros(2, np.float32)
    n1.value = 2
    assert L.hlhgat_mlgc_prune(2, 0, 0, cn.ctypes.data, out.ctypes.data, None, None,
                               C.byref(n1), C.byref(ne)) == 1
    assert b"out of range" in L.hlhgat_last_error()
    assert L.hlhgat_mlgc_device_workspace_bytes(-1, 0, 0) == 0
    assert L.hlhgat_mlgc_device_workspace_bytes(118, 560, 1) >= 118 * 16 + 560 * 24
    args = [None] * 5 + [0, 0, None, None, 0] + [None] * 6 + [0, None]
    assert L.hlhgat_mlgc_device(-1, *args) == 1
    assert b"sizes" in L.hlhgat_last_error()
    bad = list(args)
    bad[9] = 8
    assert L.hlhgat_mlgc_device(1, *bad) == 1
    assert b"flag" in L.hlhgat_last_error()
    assert L.hlhgat_mlgc_device(1, *args) == 1
    assert b"NULL" in L.hlhgat_last_error()
    # short workspace: host buffers stand in for device pointers (never dereferenced)
    buf = np.zeros(64, np.int64)
    p = buf.ctypes.data
    short = [p, p, p, p, p, 4, 4, None, p, 0, p, p, p, p, p, p, 16, None]
    assert L.hlhgat_mlgc_device(1, *short) == 1
    assert b"workspace" in L.hlhgat_last_error()
    assert L.hlhgat_mlgc_device(0, *args) == 0


def test_device_route_has_no_cpu_fallback():
    from hlhgat import ops
    z = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.mlgc_device(torch.zeros(2, 1, dtype=torch.int64), z, z, z)
