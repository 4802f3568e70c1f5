"""MLGC on the device (hlhgat_mlgc_device, ops.mlgc_device): every result is
compared with torch.equal against the host builders (hlhgat_graclus,
hlhgat_mlgc_map, hlhgat_mlgc_prune) on the same edges, node orders and
weights -- host weights are uploaded, nothing is recomputed on the device."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------
# graphs
# ----------------------------------------------------------------------------
def _star(deg, hub_last=False):
    n = deg + 1
    if hub_last:
        return n, np.stack([np.arange(deg), np.full(deg, deg)]).astype(np.int64)
    return n, np.stack([np.zeros(deg, np.int64), np.arange(1, n)]).astype(np.int64)


def _complete(n):
    iu = np.triu_indices(n, 1)
    return n, np.stack(iu).astype(np.int64)


def _bipartite(a, b):
    i, j = np.meshgrid(np.arange(a), a + np.arange(b), indexing="ij")
    return a + b, np.stack([i.reshape(-1), j.reshape(-1)]).astype(np.int64)


def _knn(seed, n, k):
    from hlhgat.synthetic import knn_edges
    ei = np.asarray(knn_edges(np.random.default_rng(seed).random((n, 2)), k), np.int64)
    assert (ei[0] < ei[1]).all()
    return n, ei


def mixed_graphs():
    """The shapes of the issue: degenerate graphs, stars across the wave
    width, dense graphs onto few coarse pairs, workload graphs, the brain
    skeleton and one graph too large for the LDS route."""
    from hlhgat.synthetic import peptides_like_graphs
    gs = [(1, np.zeros((2, 0), np.int64)), (3, np.zeros((2, 0), np.int64)),
          (2, np.array([[0], [1]], np.int64)),
          (7, np.stack([np.arange(6), np.arange(1, 7)]).astype(np.int64)),
          _star(63), _star(64, hub_last=True), _star(65), _complete(9), _bipartite(20, 20)]
    cif = _knn(11, 118, 8)
    gs += [cif] * 5  # the same graph, five node orders
    pep = peptides_like_graphs(23)[0]
    gs.append((int(pep.num_node1), np.asarray(pep.edge_index, np.int64)))
    sk = load_golden("brain_skeleton")
    gs.append((int(sk["n_nodes"]), sk["edge_index"].astype(np.int64)))
    gs.append(_knn(12, 3000, 9))
    return gs


class HostBatch:
    """Flat arrays of a batch of (n, local i<j edges) graphs."""

    def __init__(self, graphs, seed, quantised=False):
        rng = np.random.default_rng(seed)
        self.graphs = graphs
        self.ns = np.array([g[0] for g in graphs], np.int64)
        self.ms = np.array([g[1].shape[1] for g in graphs], np.int64)
        self.node_ptr = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        self.edge_ptr = np.concatenate([[0], np.cumsum(self.ms)]).astype(np.int64)
        self.perms = [rng.permutation(n).astype(np.int64) for n in self.ns]
        E = int(self.edge_ptr[-1])
        # ties, zeros, negatives and NaN
        self.w = (rng.choice(np.array([-1.0, 0.0, 0.25, 0.5, np.nan]), E) if quantised
                  else None)

    def upload(self, dev):
        ei = np.concatenate([g[1] + o for g, o in zip(self.graphs, self.node_ptr[:-1])], axis=1)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        return (t(ei), t(self.node_ptr), t(self.edge_ptr), t(np.concatenate(self.perms)),
                None if self.w is None else t(self.w))

    def host(self, one_way, prune):
        """[(c_node float32, c_edge, coarse edge_index, n1)] per graph by the
        host builders."""
        from hlhgat.hodge_dataset import graclus, mlgc_map, mlgc_prune
        out = []
        for g, (n, ei) in enumerate(self.graphs):
            w = None if self.w is None else self.w[self.edge_ptr[g]:self.edge_ptr[g + 1]]
            if one_way:
                lab = graclus(ei, n, weight=w, perm=self.perms[g])
            else:
                both = np.concatenate([ei, ei[::-1]], axis=1)
                lab = graclus(both, n, weight=None if w is None else np.concatenate([w, w]),
                              perm=self.perms[g])
            cn, ce, e1, n1 = mlgc_map(lab, ei)
            if prune:
                cn, ce, e1, n1 = mlgc_prune(cn, ce, e1, n1)
            out.append((cn.astype(np.float32), ce, e1, n1))
        return out


def run_device(hb, dev, one_way, prune):
    from hlhgat import ops
    ei, nptr, eptr, perm, w = hb.upload(dev)
    r = ops.mlgc_device(ei, nptr, eptr, perm, weight=w, one_way=one_way, prune_single=prune,
                        drop_isolated=prune)
    ops.check_device_errors()
    return r


def assert_equal_host(hb, r, ref, graphs=None):
    cn, cm = r.cn.cpu(), r.cm.cpu()
    c_node, c_edge, ce = r.c_node.cpu(), r.c_edge.cpu(), r.ce.cpu()
    assert c_node.dtype == torch.float32 and c_edge.dtype == torch.float32
    for g in (range(len(hb.graphs)) if graphs is None else graphs):
        hn, he, h1, n1 = ref[g]
        n0, n_end, e0, e_end = hb.node_ptr[g], hb.node_ptr[g + 1], hb.edge_ptr[g], hb.edge_ptr[g + 1]
        assert int(cn[g]) == n1 and int(cm[g]) == h1.shape[1], (g, int(cn[g]), int(cm[g]))
        assert torch.equal(c_node[n0:n_end], torch.from_numpy(hn)), g
        assert torch.equal(c_edge[e0:e_end], torch.from_numpy(he)), g
        assert torch.equal(ce[:, e0:e0 + h1.shape[1]], torch.from_numpy(h1)), g


# ----------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graphs():
    return mixed_graphs()


@pytest.mark.parametrize("quantised", [False, True], ids=["unit", "quantised"])
@pytest.mark.parametrize("one_way,prune", [(False, False), (True, False), (True, True)],
                         ids=["both_ways", "one_way", "one_way_pruned"])
def test_mixed_batch_equals_host(cuda, graphs, one_way, prune, quantised):
    """One launch over graphs of 1 node, no edges, one edge, a path, stars of
    hub degree 63 / 64 / 65, K9, K20,20, five orders of a superpixel graph, a
    peptide, the brain skeleton and a 3000-node kNN graph (the last two take
    the workspace route, the others the LDS route)."""
    from hlhgat import _lib
    assert _lib.LIB.hlhgat_mlgc_device_workspace_bytes(118, 600, 1) > 0
    hb = HostBatch(graphs, seed=31, quantised=quantised)
    r = run_device(hb, cuda, one_way, prune)
    assert_equal_host(hb, r, hb.host(one_way, prune))


def test_same_launch_twice_is_deterministic(cuda, graphs):
    hb = HostBatch(graphs, seed=32, quantised=True)
    a = run_device(hb, cuda, False, False)
    b = run_device(hb, cuda, False, False)
    ref = hb.host(False, False)
    assert torch.equal(a.c_node, b.c_node) and torch.equal(a.c_edge, b.c_edge)
    assert torch.equal(a.cn, b.cn) and torch.equal(a.cm, b.cm)
    cm = a.cm.cpu()
    for g in range(len(hb.graphs)):
        e0 = hb.edge_ptr[g]
        assert torch.equal(a.ce[:, e0:e0 + int(cm[g])], b.ce[:, e0:e0 + int(cm[g])]), g
    assert_equal_host(hb, a, ref)


def test_two_chained_levels_equal_host(cuda):
    """Level 2 coarsens level 1's coarse graphs: the device chain (each
    level's coarse edges cut from the head of its edge slots) equals the host
    chain."""
    sk = load_golden("brain_skeleton")
    gs = [_knn(40 + s, 118, 8) for s in range(3)] + [
        (int(sk["n_nodes"]), sk["edge_index"].astype(np.int64)), _complete(9)]
    hb = HostBatch(gs, seed=7)
    for level in range(2):
        r = run_device(hb, cuda, False, False)
        ref = hb.host(False, False)
        assert_equal_host(hb, r, ref)
        cn, cm, ce = r.cn.cpu().numpy(), r.cm.cpu().numpy(), r.ce.cpu().numpy()
        nxt = [(int(cn[g]), np.ascontiguousarray(ce[:, hb.edge_ptr[g]:hb.edge_ptr[g] + cm[g]]))
               for g in range(len(gs))]
        for (n1, e1), h in zip(nxt, ref):
            assert n1 == h[3] and np.array_equal(e1, h[2])
        hb = HostBatch(nxt, seed=8 + level)
    assert all(n < g[0] for (n, _), g in zip(nxt, gs))


def _tensors(lv):
    return {k: v for k, v in vars(lv).items() if torch.is_tensor(v)}


def test_pipeline_device_mlgc_equals_host_mlgc(cuda):
    """SuperpixelPipeline(mlgc="device") builds the same two level batches as
    mlgc="host" for 16 augmented 118-node graphs: every tensor of both
    levels."""
    from hlhgat.pipeline import SuperpixelPipeline, superpixel_raw
    raws = [superpixel_raw(3100 + i) for i in range(16)]
    idx = list(range(15, -1, -1))
    host = SuperpixelPipeline(raws, keig=11, aug=True).batch(idx, seed=4, device=cuda)
    devb = SuperpixelPipeline(raws, keig=11, aug=True, mlgc="device").batch(idx, seed=4,
                                                                            device=cuda)
    assert host[0].edge_index.shape[1] < 16 * 600
    for lv, (h, d) in enumerate(zip(host, devb)):
        th, td = _tensors(h), _tensors(d)
        assert set(th) == set(td), (lv, set(th) ^ set(td))
        assert {"x_t", "x_s", "edge_index", "edge_index_t", "edge_weight_t", "edge_index_s",
                "edge_weight_s", "num_node1", "num_edge1"} <= set(th)
        for k in th:
            assert th[k].dtype == td[k].dtype and torch.equal(th[k], td[k]), (lv, k)
        assert h.num_nodes == d.num_nodes and h.num_graphs == d.num_graphs


def test_brain_levels_device_equals_host(cuda):
    """brain_levels(device="cuda") on the skeleton: pos_* and the coarse
    edge_index of every level exactly the host's; the pooled x_s within
    count * 2^-24 * max|x_s| per coarse edge (an fp32 sum of count terms in
    another order)."""
    from hlhgat.hodge_dataset import PairData, brain_levels
    sk = load_golden("brain_skeleton")
    n = int(sk["n_nodes"])

    def fine():
        d = PairData(x_s=torch.from_numpy(sk["values"]).view(-1, 1), x_t=torch.ones(n, 1))
        d.edge_index = torch.from_numpy(sk["edge_index"].astype(np.int64))
        d.num_node1, d.num_edge1, d.num_nodes = n, int(sk["edge_index"].shape[1]), n
        return d
    host = brain_levels(fine(), pool_num=2, seed=5)
    devl = brain_levels(fine(), pool_num=2, seed=5, device=cuda)
    assert len(host) == len(devl) == 3
    for p in range(2):
        assert torch.equal(host[p].pos_t, devl[p].pos_t), p
        assert torch.equal(host[p].pos_s, devl[p].pos_s), p
        assert torch.equal(host[p + 1].edge_index, devl[p + 1].edge_index), p
        assert int(host[p + 1].num_node1) == int(devl[p + 1].num_node1)
        pos = host[p].pos_s.view(-1)
        keep = ~torch.isinf(pos)
        count = torch.bincount(pos[keep].long(), minlength=host[p + 1].x_s.shape[0]).double()
        bound = count * 2.0 ** -24 * float(host[p].x_s.abs().max())
        err = (host[p + 1].x_s.double() - devl[p + 1].x_s.double()).abs().view(-1)
        print(f"level {p + 1}: max |x_s host - device| {float(err.max()):.3e}, "
              f"smallest bound {float(bound.min()):.3e}, worst err/bound "
              f"{float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), p


def test_edge_across_graphs_raises_range_error(cuda):
    """One extra edge from the last node of graph 0 to the first node of graph
    1 (both real rows of the batch) in graph 0's slot: it is treated as
    absent, HLHGAT_DEVERR_MLGC_RANGE is raised, and every graph's outputs are
    those of the clean batch."""
    from hlhgat import _lib, ops
    gs = [_knn(60 + s, 20 + s, 4) for s in range(3)]
    hb = HostBatch(gs, seed=9)
    ref = hb.host(False, False)
    ei, nptr, eptr, perm, _ = hb.upload(cuda)
    m0, n0 = int(hb.ms[0]), int(hb.ns[0])
    extra = torch.tensor([[n0 - 1], [n0]], dtype=torch.int64, device=cuda)
    ei_bad = torch.cat([ei[:, :m0], extra, ei[:, m0:]], dim=1).contiguous()
    eptr_bad = eptr.clone()
    eptr_bad[1:] += 1
    ops.check_device_errors()
    try:
        r = ops.mlgc_device(ei_bad, nptr, eptr_bad, perm)
        torch.cuda.synchronize()
        assert ops.device_errors() & _lib.DEVERR_MLGC_RANGE
        with pytest.raises(RuntimeError, match="mlgc_device"):
            ops.check_device_errors()
    finally:
        ops.clear_device_errors()
    cn, cm = r.cn.cpu(), r.cm.cpu()
    c_node, c_edge, ce = r.c_node.cpu(), r.c_edge.cpu(), r.ce.cpu()
    assert bool(torch.isinf(c_edge[m0]))  # the bad edge is absent
    for g in range(3):
        hn, he, h1, n1 = ref[g]
        e0 = int(hb.edge_ptr[g]) + (1 if g > 0 else 0)
        assert int(cn[g]) == n1 and int(cm[g]) == h1.shape[1], g
        assert torch.equal(c_node[hb.node_ptr[g]:hb.node_ptr[g + 1]], torch.from_numpy(hn)), g
        assert torch.equal(c_edge[e0:e0 + he.size], torch.from_numpy(he)), g
        assert torch.equal(ce[:, e0:e0 + h1.shape[1]], torch.from_numpy(h1)), g
