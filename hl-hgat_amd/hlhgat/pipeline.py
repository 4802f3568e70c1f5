"""Per-sample data path of BASELINE config 3 (CIFAR10 superpixels, attpool
head), batched and fed to the device.

The reference rebuilds every sample in its Dataset.get() EVERY epoch
(main_cifar10SP_HL_HGCNN_dense_int3_attpool.py:67-125): PyG
to_undirected(reduce='min') and the i<j half of the kNN edges, dropout_edge
augmentation (a quarter of the samples, p = 0.5), the dense B1 and L0 = B1
B1^T, a dense eigh for lambda_max, L0 = 2 B1 B1^T / lmax, L1 = 2 B1^T B1 /
lmax, eig_pe(L0) (lib/Hodge_Dataset.py:97-112: eigenvectors 1..k-1 of an
eigh), edge PE |pe[i] + pe[j]|, the feature concatenations, one MLGC level
(lib/Hodge_Dataset.py:241-295: graclus, the fine -> coarse map, the coarse
graph's own dense eigh and Laplacians), and random sign flips of the PE
columns; then the DataLoader collates the level lists.

SuperpixelPipeline does the same for a whole batch of graphs at once:

  host (numpy, vectorised over the batch): the undirected edge lists (once,
    at construction: they do not change between epochs), the dropout masks,
    graclus + the MLGC map (native, hlhgat_graclus / hlhgat_mlgc_map), the
    offsets of the block-diagonal batch;
  device: the eigenvector PE and lambda_max of every level-0 graph in ONE
    launch (hlhgat_eig_pe: per graph, fp64 Lanczos with full
    re-orthogonalisation, Sturm multisection, inverse iteration; it replaced
    a batched rocSOLVER eigh of the block-padded L0 stack, 3.9 ms and a host
    sync per 256 graphs), the coarse level's lambda_max (hlhgat_hodge_lmax),
    both levels' Hodge Laplacians (hlhgat_hodge_build: the L0 / L1 rows in
    the reference's dense_to_sparse order, sizes known on the host), the
    feature concatenations, the sign flips;

and returns the two level batches on the device, collated, marked sorted /
symmetric and with the factored L1 declared (every L1 the builder emits is
alpha B1^T B1 exactly, alpha = fl(2 / lmax) per graph), ready for the head.
device="cpu" runs the same steps on the host with the reference's own
arithmetic (dense eigh lambda_max, hodge_laplacians) -- the restatement the
golden test pins (tests/golden/make_golden_pipeline.py).

Parity: structure, features, cluster maps and coarse graphs are exact;
lambda_max (fp64 Lanczos vs float32 eigh) within 1e-6 relative, so the
Laplacian entries are; PE columns equal the reference's up to sign (the reference flips them at
random, and an eigenvector's sign is arbitrary), checked where the
eigenvalue is separated from its neighbours.

BrainPipeline (below) is the DEMO brain model's input in the same spirit:
Brain_MLGC_ALL.get's z-score and skeleton correlations for a whole batch on
the device (csrc/fc.hip), the level list collated once per batch size.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .hodge_dataset import (Batch, PairData, _h2d, collate, dense_to_sparse, graclus,
                            hodge_laplacians, mlgc_batch, mlgc_batch_flat, mlgc_map,
                            pool_tables)

__all__ = ["SuperpixelPipeline", "to_undirected_min", "superpixel_raw", "BrainPipeline",
           "brain_target", "MoleculePipeline", "to_undirected_min_nd", "molecule_raw"]


def to_undirected_min(edge_index, attr, n: int):
    """PyG to_undirected(edge_index, edge_attr, reduce='min') (called at
    main_cifar10SP...:71): both directions, coalesced in (row, col) order,
    duplicates reduced by min.  Returns (int64 [2, E'], float32 [E'])."""
    ei = np.asarray(edge_index, dtype=np.int64)
    a = np.asarray(attr, dtype=np.float32).reshape(-1)
    r = np.concatenate([ei[0], ei[1]])
    c = np.concatenate([ei[1], ei[0]])
    aa = np.concatenate([a, a])
    o = np.lexsort((c, r))
    r, c, aa = r[o], c[o], aa[o]
    first = np.ones(r.size, dtype=bool)
    first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(first)
    return np.stack([r[starts], c[starts]]), np.minimum.reduceat(aa, starts)


def superpixel_raw(seed: int, n: int = 118, k: int = 8):
    """A CIFAR10-superpixel-like raw sample in the layout of PyG's
    GNNBenchmarkDataset('CIFAR10') items: x [n, 3] (mean RGB), pos [n, 2],
    a DIRECTED kNN edge_index [2, n k] with edge_attr [n k] (a distance
    weight), y [1]."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(seed)
    pos = rng.random((n, 2)).astype(np.float32)
    dist, nbr = cKDTree(pos).query(pos, k=min(k + 1, n))
    src = np.repeat(np.arange(n), nbr.shape[1] - 1)
    dst = nbr[:, 1:].reshape(-1)
    w = np.exp(-(dist[:, 1:].reshape(-1) / 0.1) ** 2).astype(np.float32)
    d = PairData()
    d.x = torch.from_numpy(rng.random((n, 3)).astype(np.float32))
    d.pos = torch.from_numpy(pos)
    d.edge_index = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    d.edge_attr = torch.from_numpy(w)
    d.y = torch.tensor([int(rng.integers(10))])
    return d


class SuperpixelPipeline:
    """Config-3 per-sample work for batches of raw superpixel graphs.

    graphs: raw samples (x, pos, edge_index, edge_attr, y; superpixel_raw).
    keig: the dataset's keig (the reference's trainset uses keig + 1 = 11,
      main_cifar10SP...:206; eig_pe is called with k=10 -> 9 PE columns).
    aug: dropout_edge augmentation as the reference's training set.
    mlgc: "host" (default) runs graclus and the fine -> coarse map on host
      threads before the upload (hlhgat_mlgc_batch); "device" runs them after
      the upload in one launch (ops.mlgc_device: the node orders travel in the
      int64 upload, the coarse counts come back in ONE device -> host read to
      size the coarse level, the coarse edges are compacted on the device) --
      the same batches bit for bit.  device="cpu" always takes the host path."""

    NODE_DIM, EDGE_DIM = 5, 4

    def __init__(self, graphs: Sequence, keig: int = 11, aug: bool = True, pe_k: int = 10,
                 mlgc: str = "host"):
        if mlgc not in ("host", "device"):
            raise ValueError(f"SuperpixelPipeline: mlgc must be 'host' or 'device' (got {mlgc!r})")
        self.mlgc = mlgc
        self.keig = keig
        self.aug = aug
        self.pe_k = pe_k
        self.n = np.array([int(g.x.shape[0]) for g in graphs], dtype=np.int64)
        self.x = [np.asarray(g.x, dtype=np.float32) for g in graphs]
        self.pos = [np.asarray(g.pos, dtype=np.float32) for g in graphs]
        self.y = [torch.as_tensor(g.y) for g in graphs]
        # to_undirected(reduce='min') + the i<j half (main_cifar10SP...:71-73):
        # fixed per sample, so done once here instead of in every get()
        self.ei, self.attr = [], []
        for g, n in zip(graphs, self.n):
            ei, a = to_undirected_min(g.edge_index, g.edge_attr, int(n))
            keep = ei[0] < ei[1]
            self.ei.append(ei[:, keep])
            self.attr.append(a[keep])
        # the same, concatenated (local node ids), for the vectorised batch gather
        self.m = np.array([e.shape[1] for e in self.ei], dtype=np.int64)
        self.e_off = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.ei_all = (np.concatenate(self.ei, axis=1) if len(self.ei)
                       else np.zeros((2, 0), np.int64))
        self.attr_all = (np.concatenate(self.attr) if len(self.attr)
                         else np.zeros(0, np.float32))
        self.x_all = np.concatenate(self.x) if len(self.x) else np.zeros((0, 3), np.float32)
        self.pos_all = np.concatenate(self.pos) if len(self.pos) else np.zeros((0, 2), np.float32)
        self.n_off = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.y_all = (torch.cat([y.reshape(-1) for y in self.y]) if len(self.y)
                      else torch.zeros(0, dtype=torch.int64))

    def __len__(self) -> int:
        return len(self.n)

    # -- host steps ------------------------------------------------------------
    @staticmethod
    def _segments(starts, lengths):
        """Concatenated index ranges [starts[b], starts[b] + lengths[b])."""
        tot = int(lengths.sum())
        if tot == 0:
            return np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        return np.repeat(starts - off, lengths) + np.arange(tot, dtype=np.int64)

    def _select(self, idx, rng):
        """The batch's graphs, vectorised over the batch: dropout_edge(p = 0.5)
        on the samples drawn for augmentation (torch.rand(1) > 0.75,
        main_cifar10SP...:74-77), then the kept i<j edges (local node ids),
        their attributes and per-graph edge counts, and graclus's random node
        order per graph (keys drawn once, sorted within each graph)."""
        B = len(idx)
        ns = self.n[idx]
        m = self.m[idx]
        eidx = self._segments(self.e_off[idx], m)
        gid_e = np.repeat(np.arange(B), m)
        if self.aug:
            drop = rng.random(B) > 0.75
            keep = ~drop[gid_e] | (rng.random(eidx.size) >= 0.5)
        else:
            keep = np.ones(eidx.size, dtype=bool)
        eidx, gid_e = eidx[keep], gid_e[keep]
        ei = self.ei_all[:, eidx]
        attr = self.attr_all[eidx]
        E_g = np.bincount(gid_e, minlength=B).astype(np.int64)
        # a random permutation of each graph's nodes: argsort of random keys
        # per row of a [B, nmax] table whose padding keys sort last
        nmax = int(ns.max()) if B else 0
        pad = np.arange(nmax)[None, :] >= ns[:, None]
        keys = rng.random((B, nmax))
        keys[pad] = 2.0
        perm = np.argsort(keys, axis=1)[~pad]
        return ns, ei, attr, E_g, gid_e, perm

    def _pe_signs(self, rng, B, width):
        """The reference's random PE sign flips for B graphs: ones on the first
        columns, +-1 on the last keig - 1 (main_cifar10SP...:113-124)."""
        s = np.ones((B, width), np.float32)
        s[:, width - (self.keig - 1):] = -1 + 2 * rng.integers(0, 2, (B, self.keig - 1))
        return s

    # -- the batch -------------------------------------------------------------
    def batch(self, idx, seed: int = 0, device="cuda", perms=None) -> List[Batch]:
        """[level-0 batch, level-1 batch] of graphs idx.  seed drives the
        augmentation, graclus's node order and the sign flips (perms: an
        explicit graclus node order per graph, e.g. to replay a fixture)."""
        rng = np.random.default_rng(seed)
        idx = np.asarray([int(i) for i in idx], dtype=np.int64)
        self._tick(None)
        ns, ei, attr, E_g, gid_e, perm = self._select(idx, rng)
        if perms is not None:
            perm = np.concatenate([np.asarray(p, np.int64) for p in perms])
        self._tick("dropout + edge lists")
        # MLGC on the host: graclus on L0's pattern (= the edges, both ways; its
        # self-loops are dropped by graclus) with unit weights, the fine -> coarse map
        # (all graphs in one native call on host threads: hlhgat_mlgc_batch)
        on_host = self.mlgc == "host" or str(device) == "cpu"
        mg = mlgc_batch_flat(ei, E_g, ns, perm) if on_host else None
        self._tick("MLGC (native batch)")
        if str(device) == "cpu":
            e_off = np.concatenate([[0], np.cumsum(E_g)])
            eis = [ei[:, e_off[b]:e_off[b + 1]] for b in range(len(idx))]
            attrs = [attr[e_off[b]:e_off[b + 1]] for b in range(len(idx))]
            lv0, lv1 = self._levels_host(idx, eis, attrs, [int(n) for n in ns], mg.per_graph())
        else:
            lv0, lv1 = self._levels_device(idx, ei, attr, ns, E_g, gid_e, mg, torch.device(device),
                                           perm)
        # sign flips of the PE columns (after the cluster column is prepended),
        # one row of signs per graph broadcast over its nodes / edges
        B = len(idx)
        sg = np.concatenate([self._pe_signs(rng, B, lv0.x_t.shape[1]),
                             self._pe_signs(rng, B, lv0.x_s.shape[1])], 1)
        sg = _h2d(sg, lv0.x_t.device)
        wt = lv0.x_t.shape[1]
        lv0.x_t.mul_(sg[:, :wt].index_select(0, lv0._gid_t))
        lv0.x_s.mul_(sg[:, wt:].index_select(0, lv0._gid_s))
        del lv0._gid_t, lv0._gid_s
        self._tick("PE sign flips")
        return [lv0, lv1]

    # stage timing (tools/probes/pipeline_stages.py): PROFILE = True makes
    # every stage boundary synchronise the device and accumulate its ms
    PROFILE = False

    def _tick(self, name):
        if not self.PROFILE:
            return
        import time
        if torch.cuda.is_available() and torch.cuda.is_initialized():
            torch.cuda.synchronize()
        now = time.perf_counter()
        if name is not None:
            st = self.__dict__.setdefault("stage_ms", {})
            st[name] = st.get(name, 0.0) + (now - self._t0) * 1e3
        self._t0 = now

    def _features(self, i, ei, attr, pe):
        """x_t = [x, pos, pe], x_s = [attr, |x_i - x_j|, |pe_i + pe_j|], each
        zero-padded to the reference's widths (main_cifar10SP...:86-91,
        :113-124; the cluster column is prepended later)."""
        x, pos = self.x[i], self.pos[i]
        node = np.concatenate([x, pos, pe], axis=1)
        edge = np.concatenate([attr.reshape(-1, 1), np.abs(x[ei[0]] - x[ei[1]]),
                               np.abs(pe[ei[0]] + pe[ei[1]])], axis=1)
        return node, edge

    def _pad_width(self, a, width):
        if a.shape[1] < width:
            a = np.concatenate([a, np.zeros((a.shape[0], width - a.shape[1]), a.dtype)], 1)
        return a[:, :width]

    def _levels_host(self, idx, eis, attrs, ns, cmaps):
        """device='cpu': the reference's arithmetic, graph by graph (dense eigh
        for lambda_max and the PE, hodge_laplacians, dense_to_sparse)."""
        from scipy.linalg import eigh
        f0, f1 = [], []
        wt = self.NODE_DIM + self.keig
        ws = self.EDGE_DIM + self.keig
        for i, ei, attr, n, (c_node, c_edge, ei1, n1) in zip(idx, eis, attrs, ns, cmaps):
            L0, L1, _, _ = hodge_laplacians(ei, n)
            vals, vecs = eigh(L0.numpy())
            pe = np.real(vecs[:, vals.argsort()])[:, 1:self.pe_k].astype(np.float32)
            node, edge = self._features(i, ei, attr, pe)
            x_t = self._pad_width(np.concatenate([c_node.reshape(-1, 1).astype(np.float32),
                                                  node], 1), wt)
            x_s = self._pad_width(np.concatenate([c_edge.reshape(-1, 1), edge], 1), ws)
            eit, ewt = dense_to_sparse(L0)
            eis_, ews = dense_to_sparse(L1)
            g = PairData(x_s=torch.from_numpy(x_s), edge_index_s=eis_, edge_weight_s=ews,
                         x_t=torch.from_numpy(x_t), edge_index_t=eit, edge_weight_t=ewt,
                         y=self.y[i])
            g.edge_index = torch.from_numpy(ei)
            g.num_node1, g.num_edge1, g.num_nodes = n, int(ei.shape[1]), n
            g._hodge_sorted = True
            f0.append(g)
            C0, C1, _, _ = hodge_laplacians(ei1, n1)
            eit, ewt = dense_to_sparse(C0)
            eis_, ews = dense_to_sparse(C1)
            c = PairData(x_s=torch.ones(ei1.shape[1], 1), edge_index_s=eis_, edge_weight_s=ews,
                         x_t=torch.ones(n1, 1), edge_index_t=eit, edge_weight_t=ewt)
            c.edge_index = torch.from_numpy(ei1)
            c.num_node1, c.num_edge1, c.num_nodes = n1, int(ei1.shape[1]), n1
            c._hodge_sorted = True
            f1.append(c)
        lv0 = collate(f0, check_hodge=False)
        lv0._gid_t = torch.repeat_interleave(torch.arange(len(f0)), torch.as_tensor(ns))
        lv0._gid_s = torch.repeat_interleave(torch.arange(len(f0)),
                                             torch.as_tensor([e.shape[1] for e in eis]))
        return lv0, collate(f1, check_hodge=False)

    def _levels_device(self, idx, ei, attr, ns, E_g, gid_e, mg, dev, perm=None):
        """Both levels on the device.  The host arrays travel in two
        asynchronous uploads from pinned memory (one int64, one float32; the
        device tensors are views of them); the Hodge builder gets its sizes from the host (the nnz of L0
        and L1 follow from the degrees), so nothing here waits on the device
        but the eigh's own error check.  mg None (mlgc="device"): MLGC runs
        here after the upload (ops.mlgc_device), its coarse counts are read
        back once and the coarse Hodge builder sizes itself on the device."""
        from . import ops
        B = len(idx)
        N, E = int(ns.sum()), int(ei.shape[1])
        n_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        gid_n = np.repeat(np.arange(B), ns)
        ei_b = ei + n_off[gid_e]  # block-diagonal batch (PairData offsets)
        e_off = np.concatenate([[0], np.cumsum(E_g)]).astype(np.int64)
        nodes = self._segments(self.n_off[idx], ns)
        if mg is None:
            return self._levels_device_mlgc(idx, ei_b, attr, ns, E_g, gid_n, gid_e, n_off, e_off,
                                            nodes, perm, dev)
        # coarse level: each graph's coarse edges at the head of its edge slot
        n1 = mg.cn
        m1 = mg.cm
        o1 = np.concatenate([[0], np.cumsum(n1)]).astype(np.int64)
        cidx = self._segments(e_off[:-1], m1)
        gid_c = np.repeat(np.arange(B), m1)
        ei1 = mg.ce[:, cidx] + o1[gid_c]
        N1, E1 = int(o1[-1]), int(ei1.shape[1])
        ints = [ei_b.reshape(-1), ei1.reshape(-1), ns, E_g, n1, m1,
                self.y_all.numpy()[idx].astype(np.int64), gid_n, gid_e]
        flts = [self.x_all[nodes].reshape(-1), self.pos_all[nodes].reshape(-1), attr,
                mg.c_node.astype(np.float32), mg.c_edge]
        idev = _h2d(np.concatenate(ints), dev)
        fdev = _h2d(np.concatenate(flts), dev)

        def cut(t, sizes):
            out, o = [], 0
            for z in sizes:
                out.append(t[o:o + z])
                o += z
            return out
        ei_d, ei1_d, ns_d, Eg_d, n1_d, m1_d, y_d, gid_d, gide_d = cut(
            idev, [a.size for a in ints])
        ei_d, ei1_d = ei_d.view(2, E), ei1_d.view(2, E1)
        x, pos, attr_d, c_node, c_edge = cut(fdev, [a.size for a in flts])
        x, pos = x.view(N, 3), pos.view(N, 2)
        self._tick("device levels: edge upload")
        return self._levels_finish(ns, ei_b, ei_d, ns_d, Eg_d, y_d, gid_d, gide_d, x, pos, attr_d,
                                   c_node, c_edge, ei1_d, n1_d, m1_d, N1, E1,
                                   (N1,) + self._nnz(ei1, N1), dev)

    @staticmethod
    def _nnz(e, n):
        """(nnz(L0), nnz(L1)) from the degrees.  The formulas (and the
        Laplacians themselves) assume a simple graph: unique edges with i < j."""
        if e.shape[1] and ((e[0] >= e[1]).any() or
                           np.unique(e[0] * n + e[1]).size != e.shape[1]):
            raise ValueError("hlhgat: coarse edges are not unique i < j pairs")
        deg = np.bincount(e.reshape(-1), minlength=n)
        return int((deg > 0).sum()) + 2 * e.shape[1], int((deg * deg).sum()) - e.shape[1]

    def _levels_device_mlgc(self, idx, ei_b, attr, ns, E_g, gid_n, gid_e, n_off, e_off, nodes,
                            perm, dev):
        """mlgc="device": the upload carries the node orders and the graph
        offsets instead of the host's coarse maps; MLGC runs on the device."""
        from . import ops
        B = len(idx)
        N, E = int(ns.sum()), int(ei_b.shape[1])
        ints = [ei_b.reshape(-1), ns, E_g, self.y_all.numpy()[idx].astype(np.int64), gid_n, gid_e,
                np.asarray(perm, np.int64), n_off, e_off]
        flts = [self.x_all[nodes].reshape(-1), self.pos_all[nodes].reshape(-1), attr]
        idev = _h2d(np.concatenate(ints), dev)
        fdev = _h2d(np.concatenate(flts), dev)
        o, cuts = 0, []
        for a in ints:
            cuts.append(idev[o:o + a.size])
            o += a.size
        ei_d, ns_d, Eg_d, y_d, gid_d, gide_d, perm_d, nptr_d, eptr_d = cuts
        ei_d = ei_d.view(2, E)
        x, pos, attr_d = fdev[:3 * N].view(N, 3), fdev[3 * N:5 * N].view(N, 2), fdev[5 * N:]
        self._tick("device levels: edge upload")
        r = ops.mlgc_device(ei_d, nptr_d, eptr_d, perm_d)
        n1_d, m1_d = r.cn, r.cm
        # the one read-back: the coarse level's sizes
        N1, E1 = (int(v) for v in torch.stack([n1_d.sum(), m1_d.sum()]).cpu())
        # compact each graph's coarse edges (the head of its edge slot) to
        # [2, E1] and add the coarse PairData offsets
        gid_c = torch.repeat_interleave(torch.arange(B, device=dev), m1_d, output_size=E1)
        c_off = torch.cumsum(m1_d, 0) - m1_d
        o1 = torch.cumsum(n1_d, 0) - n1_d
        src = torch.arange(E1, device=dev) - c_off[gid_c] + eptr_d[:-1][gid_c]
        ei1_d = r.ce[:, src] + o1[gid_c]
        self._tick("device levels: MLGC (device)")
        return self._levels_finish(ns, ei_b, ei_d, ns_d, Eg_d, y_d, gid_d, gide_d, x, pos, attr_d,
                                   r.c_node, r.c_edge, ei1_d, n1_d, m1_d, N1, E1, None, dev)

    def _levels_finish(self, ns, ei_b, ei_d, ns_d, Eg_d, y_d, gid_d, gide_d, x, pos, attr_d, c_node,
                       c_edge, ei1_d, n1_d, m1_d, N1, E1, sizes1, dev):
        """The device stages after the upload (and MLGC): eig_pe, both Hodge
        builds, the features.  sizes1: the coarse builder's host sizes, or
        None (it then reads its own row sizes)."""
        from . import ops
        nnz = self._nnz
        B = len(ns)
        N, E = int(ns.sum()), int(ei_b.shape[1])
        # eig_pe and lambda_max of every graph in one launch (hlhgat_eig_pe:
        # fp64 Lanczos with full re-orthogonalisation per graph), then the
        # Hodge Laplacians with that lambda_max
        pe, lam64 = ops.eig_pe(ei_d, ns_d, self.pe_k, max_nodes=int(ns.max()), n_nodes=N)
        self._tick("device levels: eig_pe + lambda_max")
        ei_t, w_t, ei_s, w_s, lam = ops.hodge_build(ei_d, ns_d, lmax=lam64.to(torch.float32),
                                                    sizes=(N,) + nnz(ei_b, N))
        self._tick("device levels: Hodge build (fine)")
        src, dst = ei_d[0], ei_d[1]
        wt, ws = self.NODE_DIM + self.keig, self.EDGE_DIM + self.keig
        k1 = pe.shape[1]
        lv0 = Batch()
        lv0.num_graphs = B
        # x_t = [cluster, x, pos, pe, 0...], x_s = [cluster, attr, |x_i - x_j|,
        # |pe_i + pe_j|, 0...] written straight into their padded widths
        xt = torch.zeros(N, wt, device=dev)
        xt[:, 0] = c_node
        xt[:, 1:4] = x
        xt[:, 4:6] = pos
        xt[:, 6:6 + k1] = pe[:, :wt - 6]
        xs = torch.zeros(E, ws, device=dev)
        xs[:, 0] = c_edge
        xs[:, 1] = attr_d
        xs[:, 2:5] = (x[src] - x[dst]).abs()
        xs[:, 5:5 + k1] = (pe[src] + pe[dst]).abs()[:, :ws - 5]
        lv0.x_t, lv0.x_s = xt, xs
        lv0.edge_index_t, lv0.edge_weight_t = ei_t, w_t
        lv0.edge_index_s, lv0.edge_weight_s = ei_s, w_s
        lv0.edge_index = ei_d
        lv0.y = y_d
        # per-graph counts on the device, as Batch.to leaves them (the step's
        # forward reads them inside a capture)
        lv0.num_node1, lv0.num_edge1 = ns_d, Eg_d
        lv0.num_nodes = N
        lv0._gid_t, lv0._gid_s = gid_d, gide_d
        self._tick("device levels: features")
        c_t, c_wt, c_s, c_ws, _ = ops.hodge_build(ei1_d, n1_d, sizes=sizes1)
        self._tick("device levels: Hodge build (coarse)")
        lv1 = Batch()
        lv1.num_graphs = B
        lv1.x_t = torch.ones(N1, 1, device=dev)
        lv1.x_s = torch.ones(E1, 1, device=dev)
        lv1.edge_index_t, lv1.edge_weight_t = c_t, c_wt
        lv1.edge_index_s, lv1.edge_weight_s = c_s, c_ws
        lv1.edge_index = ei1_d
        lv1.num_node1, lv1.num_edge1 = n1_d, m1_d
        lv1.num_nodes = N1
        for lv in (lv0, lv1):
            lv.hodge_sorted = {"edge_index_s": True, "edge_index_t": True}
            lv.l1_factor = False
            lv._mark()
        # every L1 of the builder is fl(2 / lmax) B1^T B1 exactly (entries
        # fl(fl(2 v) / lmax), v in {2, +-1}): the factored L1 holds by
        # construction -- declared where it pays (hodge_dataset.FACTOR_MIN_ROW)
        from .hodge_dataset import FACTOR_MIN_ROW
        if ei_s.shape[1] >= FACTOR_MIN_ROW * max(E, 1):
            ops.set_hodge_factor(lv0.edge_index_s, lv0.edge_index, lv0.num_nodes)
            lv0.l1_factor = True
        return lv0, lv1


def brain_target(scores, y_mean: float = 95.1377, y_std: float = 7.3) -> torch.Tensor:
    """The regression target of Brain_MLGC_ALL.get (HL-HGAT-DEMO/lib/
    Hodge_Dataset.py:140): (mean of the subject's first five scores, as
    float32, - y_mean) / y_std, a 0-d float32 tensor."""
    m = torch.tensor(np.asarray(scores)[:5].mean()).to(torch.float)
    return (m - y_mean) / y_std


class BrainPipeline:
    """The DEMO brain model's input (HL-HGAT-DEMO/lib/Hodge_Dataset.py:130-145,
    Brain_MLGC_ALL.get, and the DataLoader collation of OHBM_DEMO.ipynb) for
    whole batches, on the device.

    The reference z-scores each subject's [N, T] fMRI block by its global mean
    and std (x_t), takes torch.corrcoef of it at the skeleton's edges (x_s),
    deep-copies the whole level list per sample and lets the DataLoader
    concatenate the copies.  The skeleton and its Laplacians are the same for
    every subject, so here the level list is collated ONCE per batch size
    (hodge_dataset.collate: CSR, incidence and factor tables included), moved
    to the device and cached; batch() returns it with only x_t, x_s and y of
    level 0 replaced -- two library calls (ops.fc_prepare, ops.fc_edges) and
    one gather, no host synchronisation, no copy of graph structure and no
    allocation but the three outputs and the batch's index upload.

    series: S arrays [N, T_s] (equal N).  resident=True uploads them once as
      one [S, N, Tmax] block; resident=False keeps that block pinned on the
      host and uploads only a batch's rows.
    targets: [S] floats (brain_target).
    levels: the per-subject level list [fine, coarse, ...] of PairData, level
      p carrying pos_t / pos_s, as the notebook builds it once; the fine
      level's edge_index ([2, E], i < j) is the skeleton.

    Two stated differences from the reference:
      * window="random" draws t_begin in [0, 75) and a length in [250, 300)
        ONCE PER BATCH from `seed`; the reference draws them per sample
        (:131-133), which its own collation cannot batch when the lengths
        differ (x_t rows of different widths).  window="per_sample" is the
        reference's draw, one (t_begin, length) per subject: x_t is then
        padded to [B N, t_max] (zeros past a subject's own length), level 0
        carries t_len (int32 [B N], each time course's length) and
        Inception1D runs its ragged path on it.  t_max = min(299, the
        shortest series of the pipeline) whatever was drawn, so every batch
        of one size has one shape -- one captured graph under TrainStep;
      * a region whose series is constant over the window gets NaN on its
        edges (the exact 0 / 0); the reference's float result there is
        rounding noise.
    device="cpu" restates the reference's arithmetic in torch, sample by
    sample ((f - f.mean()) / f.std(), torch.corrcoef, the indexing): the
    restatement the golden test pins (tests/golden/make_golden_brainfc.py).
    The device path works on the current stream and reuses one workspace per
    batch size: use a batch's tensors (or order later work after them on that
    stream) before asking for the next batch from another stream."""

    def __init__(self, series: Sequence, targets, levels: Sequence[PairData],
                 resident: bool = True):
        if len(series) == 0:
            raise ValueError("BrainPipeline: no series")
        # as the reference reads a sample: torch.tensor(arr).to(torch.float)
        self.series = [torch.as_tensor(np.asarray(s)).to(torch.float) for s in series]
        self.N = int(self.series[0].shape[0])
        if any(s.dim() != 2 or s.shape[0] != self.N for s in self.series):
            raise ValueError("BrainPipeline: every series must be [N, T] with the same N")
        self.lens = np.array([int(s.shape[1]) for s in self.series], dtype=np.int64)
        self.targets = torch.as_tensor(np.asarray(targets, dtype=np.float32)).reshape(-1)
        if self.targets.numel() != len(self.series):
            raise ValueError("BrainPipeline: one target per series")
        self.levels = list(levels)
        fine = self.levels[0]
        self.edge_index = torch.as_tensor(np.asarray(fine.edge_index)).to(torch.int64)
        self.E = int(self.edge_index.shape[1])
        nf = fine.x_t.shape[0] if torch.is_tensor(getattr(fine, "x_t", None)) else self.N
        if int(nf) != self.N:
            raise ValueError(f"BrainPipeline: the fine level has {nf} nodes, the series {self.N}")
        from . import ops
        self._pair2edge, self._tiles = ops.fc_pair_table(self.edge_index, self.N)
        self.resident = bool(resident)
        self._block = None   # [S, N, Tmax] host block (pinned when it feeds a device)
        self._dev = {}       # device -> per-device state
        self._levels = {}    # (device, B) -> collated level list

    def __len__(self) -> int:
        return len(self.series)

    # -- cached state ----------------------------------------------------------
    def _host_block(self, pin: bool) -> torch.Tensor:
        if self._block is None:
            blk = torch.zeros((len(self.series), self.N, int(self.lens.max())),
                              dtype=torch.float32)
            for i, s in enumerate(self.series):
                blk[i, :, :s.shape[1]] = s
            self._block = blk.pin_memory() if pin else blk
        return self._block

    def _device_state(self, dev: torch.device) -> dict:
        st = self._dev.get(dev)
        if st is None:
            blk = self._host_block(pin=True)
            st = {"pair2edge": self._pair2edge.to(dev), "tiles": self._tiles.to(dev),
                  "targets": self.targets.to(dev), "ws": {}, "stage": {}}
            if self.resident:
                st["block"] = blk.to(dev).view(-1, blk.shape[2])
            self._dev[dev] = st
        return st

    def levels_for(self, B: int, device="cuda") -> List[Batch]:
        """B copies of every level, collated once and cached per (device, B)."""
        dev = torch.device(device)
        key = (dev, int(B))
        out = self._levels.get(key)
        if out is None:
            out = []
            for p, lv in enumerate(self.levels):
                g = lv
                if p == 0:  # the placeholders that batch() replaces
                    g = PairData(**{k: getattr(lv, k) for k in lv.keys()})
                    g.x_t = torch.zeros(self.N, 1)
                    g.x_s = torch.zeros(self.E, 1)
                    g.y = None
                out.append(collate([g] * int(B), check_hodge=True))
            # the cluster CSR of every pooled level next to the CSR, incidence
            # and degree tables of collate: the head then sorts no cluster
            # assignment in its forward (HL_HGAT_attpool, hodge_st_model._pool)
            if len(out) > 1 and all(torch.is_tensor(getattr(b, k, None))
                                    for b in out[:-1] for k in ("pos_t", "pos_s")):
                pool_tables(out, pos=True)
            if dev.type == "cuda":
                out = [b.to(dev) for b in out]
            self._levels[key] = out
        return out

    T_MAX = 299  # the longest window Brain_MLGC_ALL.get draws (:132)

    @property
    def t_max(self) -> int:
        """The padded width of x_t under per-sample windows."""
        return min(self.T_MAX, int(self.lens.min()))

    def _windows(self, idx, window, seed) -> np.ndarray:
        """Per-subject (t0, len) as int64 [B, 2]: drawn from `seed` as
        Brain_MLGC_ALL.get draws them (:131-133), or the caller's array."""
        lens = self.lens[idx]
        if isinstance(window, str):
            rng = np.random.default_rng(seed)
            w = np.stack([rng.integers(0, 75, size=idx.size),
                          rng.integers(250, 300, size=idx.size)], 1).astype(np.int64)
            # a slice past the series end is cut, as in the reference; the
            # padded width bounds it when the series differ in length
            w[:, 1] = np.minimum(np.minimum(w[:, 1], lens - w[:, 0]), self.t_max)
        else:
            w = np.asarray(window)
            if w.shape != (idx.size, 2) or not np.issubdtype(w.dtype, np.integer):
                raise ValueError(f"BrainPipeline: per-sample windows must be an int array "
                                 f"[{idx.size}, 2] of (t0, len), got {w.dtype} {w.shape}")
            w = w.astype(np.int64)
        if (w[:, 0] < 0).any() or (w[:, 1] < 2).any() or (w.sum(1) > lens).any() or \
                (w[:, 1] > self.t_max).any():
            raise ValueError(f"BrainPipeline: windows {w.tolist()} do not fit series of lengths "
                             f"{lens.tolist()} with 2 <= len <= t_max = {self.t_max}")
        return w

    def _batch_per_sample(self, idx, w, dev, levels, lv0):
        B, N, t_max = idx.size, self.N, self.t_max
        if dev.type == "cpu":
            xs_t, xs_s = [], []
            ei = self.edge_index
            for i, (t0, n) in zip(idx, w.tolist()):
                f = self.series[i][:, t0:t0 + n]
                f = (f - f.mean()) / f.std()
                xs_t.append(torch.nn.functional.pad(f, (0, t_max - n)))
                xs_s.append(torch.corrcoef(f)[ei[0], ei[1]].view(-1, 1))
            lv0.x_t, lv0.x_s = torch.cat(xs_t), torch.cat(xs_s)
            lv0.t_len = torch.from_numpy(np.repeat(w[:, 1], N).astype(np.int32))
            lv0.y = self.targets[torch.from_numpy(idx)]
            return [lv0] + list(levels[1:])
        from . import ops
        st = self._device_state(dev)
        ids = _h2d(np.concatenate([idx, idx * N, w[:, 0], w[:, 1]]), dev)
        win = ids[2 * B:].to(torch.int32)
        x, rows = self._batch_rows(st, idx, ids, dev)
        prep = ops.fc_prepare(x, B, n_nodes=N, graph_rows=rows, workspace=self._batch_ws(st, B, dev),
                              windows=(win[:B], win[B:]), t_max=t_max)
        lv0.x_t = prep.z
        lv0.t_len = win[B:].repeat_interleave(N)
        lv0.x_s = ops.fc_edges(prep, st["pair2edge"], self.E, tiles=st["tiles"])
        lv0.y = st["targets"].index_select(0, ids[:B])
        return [lv0] + list(levels[1:])

    def _batch_rows(self, st, idx, ids, dev):
        """(x, graph_rows) of a batch: the resident block and the subjects'
        first rows, or the batch's rows staged from the pinned block."""
        B = idx.size
        if self.resident:
            return st["block"], ids[B:2 * B]
        blk = self._host_block(pin=True)
        x = st["stage"].get(B)
        if x is None:
            x = st["stage"][B] = torch.empty((B * self.N, blk.shape[2]), device=dev)
        for b, i in enumerate(idx):
            x[b * self.N:(b + 1) * self.N].copy_(blk[i], non_blocking=True)
        return x, None

    def _batch_ws(self, st, B, dev):
        from . import _lib
        ws = st["ws"].get(B)
        if ws is None:
            need = int(_lib.LIB.hlhgat_fc_workspace_bytes(B, self.N, int(self.lens.max())))
            ws = st["ws"][B] = torch.empty(need, dtype=torch.uint8, device=dev)
        return ws

    def _window(self, idx, window, seed):
        lens = self.lens[idx]
        if window is None:
            if (lens != lens[0]).any():
                raise ValueError("BrainPipeline: window=None needs series of one length in a "
                                 f"batch, got {sorted(set(lens.tolist()))}")
            return 0, int(lens[0])
        if isinstance(window, str):
            if window != "random":
                raise ValueError(f"BrainPipeline: window={window!r}")
            rng = np.random.default_rng(seed)
            t0 = int(rng.integers(0, 75))
            T = int(rng.integers(250, 300))
            T = min(T, int(lens.min()) - t0)  # a slice past the end is cut, as in the reference
        else:
            t0, T = int(window[0]), int(window[1])
        if t0 < 0 or T < 2 or t0 + T > int(lens.min()):
            raise ValueError(f"BrainPipeline: window [{t0}, {t0 + T}) does not fit series of "
                             f"length {int(lens.min())} with at least two samples")
        return t0, T

    # -- the batch -------------------------------------------------------------
    def batch(self, idx, window=None, seed: int = 0, device="cuda") -> List[Batch]:
        """The level list of subjects idx: the cached collation of len(idx)
        copies with x_t [B N, T], x_s [B E, 1] and y [B] of level 0 set.
        window: None (the whole series), (t0, T), "random" (one draw per
        batch), "per_sample" (one draw per subject, as the reference) or an
        int array [B, 2] of per-subject (t0, len); the last two give x_t
        [B N, t_max] with t_len (see the class docstring)."""
        import copy
        idx = np.asarray([int(i) for i in idx], dtype=np.int64)
        B = idx.size
        if B == 0 or idx.min() < 0 or idx.max() >= len(self.series):
            raise ValueError(f"BrainPipeline: subjects {idx.tolist()} outside [0, {len(self)})")
        dev = torch.device(device)
        levels = self.levels_for(B, dev)
        lv0 = copy.copy(levels[0])  # the same structure tensors, three fields of its own
        if (isinstance(window, str) and window == "per_sample") or np.ndim(window) == 2:
            return self._batch_per_sample(idx, self._windows(idx, window, seed), dev, levels, lv0)
        t0, T = self._window(idx, window, seed)
        if dev.type == "cpu":
            xs_t, xs_s = [], []
            ei = self.edge_index
            for i in idx:
                f = self.series[i][:, t0:t0 + T]
                f = (f - f.mean()) / f.std()
                xs_t.append(f)
                xs_s.append(torch.corrcoef(f)[ei[0], ei[1]].view(-1, 1))
            lv0.x_t, lv0.x_s = torch.cat(xs_t), torch.cat(xs_s)
            lv0.y = self.targets[torch.from_numpy(idx)]
            return [lv0] + list(levels[1:])
        from . import _lib, ops
        st = self._device_state(dev)
        ids = _h2d(np.concatenate([idx, idx * self.N]), dev)
        x, rows = self._batch_rows(st, idx, ids, dev)
        prep = ops.fc_prepare(x, B, window=(t0, T), n_nodes=self.N, graph_rows=rows,
                              workspace=self._batch_ws(st, B, dev))
        lv0.x_t = prep.z
        lv0.x_s = ops.fc_edges(prep, st["pair2edge"], self.E, tiles=st["tiles"])
        lv0.y = st["targets"].index_select(0, ids[:B])
        return [lv0] + list(levels[1:])


# ----------------------------------------------------------------------------
# molecules (ZINC, Peptides-func): process() for whole batches
# ----------------------------------------------------------------------------
def to_undirected_min_nd(edge_index, attr, n: int):
    """to_undirected_min for attributes of any dtype with one or more columns
    (Peptides' edge_attr is [E, 3]; lib/Hodge_Dataset.py:447, :576): both
    directions, coalesced in (row, col) order, duplicates reduced by an
    element-wise min.  Returns (int64 [2, E'], attr's dtype [E', ...])."""
    ei = np.asarray(edge_index, dtype=np.int64)
    a = np.asarray(attr)
    r = np.concatenate([ei[0], ei[1]])
    c = np.concatenate([ei[1], ei[0]])
    aa = np.concatenate([a, a])
    o = np.lexsort((c, r))
    r, c, aa = r[o], c[o], aa[o]
    first = np.ones(r.size, dtype=bool)
    first[1:] = (r[1:] != r[:-1]) | (c[1:] != c[:-1])
    starts = np.flatnonzero(first)
    if starts.size == 0:
        return np.zeros((2, 0), np.int64), aa[:0]
    return np.stack([r[starts], c[starts]]), np.minimum.reduceat(aa, starts, axis=0)


def molecule_raw(seed: int, n: int, kind: str = "zinc", edges=None):
    """A raw molecule in the layout of PyG's ZINC / LRGB Peptides-func items:
    x (zinc: atom class [n, 1] in 0..20; peptides: [n, 9] ints), edge_index
    [2, 2 E] with BOTH directions in shuffled order, edge_attr (zinc: bond
    class [2 E] in 1..3; peptides: [2 E, 3] ints), y (zinc [1]; peptides
    [1, 10]).  The bonds are synthetic.molecule_edges(default_rng(seed), n),
    or the given i < j edge list."""
    from .synthetic import molecule_edges
    rng = np.random.default_rng(seed)
    ei = molecule_edges(rng, n) if edges is None else np.asarray(edges, np.int64).reshape(2, -1)
    E = ei.shape[1]
    d = PairData()
    if kind == "zinc":
        d.x = torch.from_numpy(rng.integers(0, 21, (n, 1)))
        attr = rng.integers(1, 4, E)
        d.y = torch.tensor([float(rng.normal())])
    elif kind == "peptides":
        d.x = torch.from_numpy(rng.integers(0, 10, (n, 9)))
        attr = rng.integers(0, 4, (E, 3))
        d.y = torch.from_numpy(rng.integers(0, 2, (1, 10)).astype(np.float32))
    else:
        raise ValueError(f"molecule_raw: kind must be 'zinc' or 'peptides' (got {kind!r})")
    o = rng.permutation(2 * E)
    d.edge_index = torch.from_numpy(np.concatenate([ei, ei[::-1]], axis=1)[:, o].copy())
    d.edge_attr = torch.from_numpy(np.concatenate([attr, attr])[o])
    return d


def _coarse_level(ei1_d, n1_d, m1_d, N1, E1, sizes1, dev) -> Batch:
    """The collated coarse level of one MLGC step on the device: ones
    features and its own Hodge Laplacians (lib/Hodge_Dataset.py:275-294), as
    SuperpixelPipeline._levels_finish builds it."""
    from . import ops
    c_t, c_wt, c_s, c_ws, _ = ops.hodge_build(ei1_d, n1_d, sizes=sizes1)
    lv1 = Batch()
    lv1.num_graphs = int(n1_d.numel())
    lv1.x_t = torch.ones(N1, 1, device=dev)
    lv1.x_s = torch.ones(E1, 1, device=dev)
    lv1.edge_index_t, lv1.edge_weight_t = c_t, c_wt
    lv1.edge_index_s, lv1.edge_weight_s = c_s, c_ws
    lv1.edge_index = ei1_d
    lv1.num_node1, lv1.num_edge1 = n1_d, m1_d
    lv1.num_nodes = N1
    lv1.hodge_sorted = {"edge_index_s": True, "edge_index_t": True}
    lv1.l1_factor = False
    lv1._mark()
    return lv1


class MoleculePipeline:
    """The molecular datasets' process() (ZINC_HG_BM_par1_EigPE.process,
    lib/Hodge_Dataset.py:442-477; Peptides_Func_EigPE.process, :571-605) for
    whole batches on the device, and Peptides_Func_EigPE_MLGC.get's per-access
    MLGC (:628-650).

    raw: samples with x, edge_index, edge_attr, y as PyG's ZINC / LRGB
      datasets give them (molecule_raw).
    kind: "zinc" (x_t = [one_hot(x, 21), pe], x_s = [one_hot(attr - 1, 3), pe],
      y = (y - 0.0153) / 2.0109) or "peptides" (the 9 / 3 raw columns cast to
      float, then the PE).
    keig: the dataset's keig: each side is fixed + keig - 1 wide, the widths
      get() cuts or pads to (:425-440, :554-569); columns past a small
      graph's size are zero.  No sign flip is applied: ops / nn.PESignFlip
      does that per replay.

    The reference runs three dense LAPACK eighs per graph at batch size 1;
    batch() runs one hlhgat_eig_pe launch (node PE and lambda_max), one
    hlhgat_eig_pe_edges launch (edge PE: eigenvectors of L1 = B1^T B1) and one
    hlhgat_hodge_build with that lambda_max for the whole batch.  The sizes of
    the Laplacians come from the host degrees, so nothing waits on the device.
    device="cpu" runs the reference's arithmetic graph by graph (dense float32
    eigh) -- the restatement the golden test pins
    (tests/golden/make_golden_molecule.py)."""

    FIXED = {"zinc": (21, 3), "peptides": (9, 3)}
    PROFILE = False
    _tick = SuperpixelPipeline._tick
    _segments = staticmethod(SuperpixelPipeline._segments)

    def __init__(self, raw: Sequence, kind: str = "zinc", keig: int = 16):
        if kind not in self.FIXED:
            raise ValueError(f"MoleculePipeline: kind must be 'zinc' or 'peptides' (got {kind!r})")
        if not 2 <= int(keig) <= 64:
            raise ValueError("MoleculePipeline: keig must be 2..64")
        self.kind, self.keig = kind, int(keig)
        self.ft, self.fs = self.FIXED[kind]
        self.n = np.array([int(g.x.shape[0]) for g in raw], dtype=np.int64)
        eis, xts, xss, ys = [], [], [], []
        for g, n in zip(raw, self.n):
            # to_undirected(reduce='min') and the i < j half (:447-450)
            ei, a = to_undirected_min_nd(g.edge_index, g.edge_attr, int(n))
            keep = ei[0] < ei[1]
            ei, a = ei[:, keep], torch.from_numpy(np.ascontiguousarray(a[keep]))
            x = torch.as_tensor(np.asarray(g.x))
            if kind == "zinc":
                xs = torch.nn.functional.one_hot(a.long() - 1, num_classes=3).to(torch.float)
                xt = torch.nn.functional.one_hot(x.long().reshape(-1), num_classes=21).to(torch.float)
                y = (torch.as_tensor(g.y).to(torch.float) - 0.0153) / 2.0109
            else:
                xs, xt = a.to(torch.float).reshape(-1, 3), x.to(torch.float).reshape(-1, 9)
                y = torch.as_tensor(g.y).to(torch.float)
            eis.append(ei)
            xts.append(xt.numpy())
            xss.append(xs.numpy())
            ys.append(y)
        self.ei, self.y = eis, ys
        self.m = np.array([e.shape[1] for e in eis], dtype=np.int64)
        self.n_off = np.concatenate([[0], np.cumsum(self.n)]).astype(np.int64)
        self.e_off = np.concatenate([[0], np.cumsum(self.m)]).astype(np.int64)
        self.ei_all = np.concatenate(eis, axis=1) if eis else np.zeros((2, 0), np.int64)
        self.xt_all = np.concatenate(xts) if xts else np.zeros((0, self.ft), np.float32)
        self.xs_all = np.concatenate(xss) if xss else np.zeros((0, self.fs), np.float32)
        self.y_dim = int(ys[0].numel()) if ys else 1
        self.y_all = (torch.stack([y.reshape(-1) for y in ys]).numpy() if ys
                      else np.zeros((0, 1), np.float32))

    def __len__(self) -> int:
        return len(self.n)

    @property
    def widths(self):
        """(x_t width, x_s width) = fixed + keig - 1."""
        return self.ft + self.keig - 1, self.fs + self.keig - 1

    # -- device="cpu": the reference's arithmetic ----------------------------------
    def _graph_host(self, i: int) -> PairData:
        from scipy.linalg import eigh
        ei, n = self.ei[i], int(self.n[i])
        L0, L1, _, _ = hodge_laplacians(ei, n)

        def pe(L, rows):
            out = np.zeros((rows, self.keig - 1), np.float32)
            if rows:
                vals, vecs = eigh(L.numpy())
                v = np.real(vecs[:, vals.argsort()])[:, 1:self.keig]
                out[:, :v.shape[1]] = v
            return out

        n0, e0 = self.n_off[i], self.e_off[i]
        x_t = np.concatenate([self.xt_all[n0:n0 + n], pe(L0, n)], axis=1)
        x_s = np.concatenate([self.xs_all[e0:e0 + ei.shape[1]], pe(L1, ei.shape[1])], axis=1)
        eit, ewt = dense_to_sparse(L0)
        eis, ews = dense_to_sparse(L1)
        g = PairData(x_s=torch.from_numpy(x_s), edge_index_s=eis, edge_weight_s=ews,
                     x_t=torch.from_numpy(x_t), edge_index_t=eit, edge_weight_t=ewt, y=self.y[i])
        g.edge_index = torch.from_numpy(ei)
        g.num_node1, g.num_edge1, g.num_nodes = n, int(ei.shape[1]), n
        g._hodge_sorted = True
        return g

    # -- the batch -------------------------------------------------------------------
    def batch(self, idx, device="cuda") -> Batch:
        """process() of the molecules idx as one collated Batch."""
        idx = np.asarray([int(i) for i in idx], dtype=np.int64)
        B = idx.size
        if B == 0 or idx.min() < 0 or idx.max() >= len(self):
            raise ValueError(f"MoleculePipeline: molecules {idx.tolist()} outside [0, {len(self)})")
        self._tick(None)
        ns, E_g = self.n[idx], self.m[idx]
        eidx = self._segments(self.e_off[idx], E_g)
        ei = self.ei_all[:, eidx]
        if str(device) == "cpu":
            b = collate([self._graph_host(int(i)) for i in idx], check_hodge=False)
            b._mol_host = (ns, E_g, ei)
            self._tick("host: reference arithmetic")
            return b
        from . import ops
        dev = torch.device(device)
        N, E = int(ns.sum()), int(E_g.sum())
        n_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        gid_e = np.repeat(np.arange(B), E_g)
        ei_b = ei + n_off[gid_e]  # block-diagonal batch (PairData offsets)
        nodes = self._segments(self.n_off[idx], ns)
        ints = [ei_b.reshape(-1), ns, E_g]
        flts = [self.xt_all[nodes].reshape(-1), self.xs_all[eidx].reshape(-1),
                self.y_all[idx].reshape(-1)]
        idev = _h2d(np.concatenate(ints), dev)
        fdev = _h2d(np.concatenate(flts), dev)
        ei_d, ns_d, Eg_d = idev[:2 * E].view(2, E), idev[2 * E:2 * E + B], idev[2 * E + B:]
        xt_f = fdev[:N * self.ft].view(N, self.ft)
        xs_f = fdev[N * self.ft:N * self.ft + E * self.fs].view(E, self.fs)
        y_d = fdev[N * self.ft + E * self.fs:]
        self._tick("upload")
        k = self.keig
        pe_t, lam64 = ops.eig_pe(ei_d, ns_d, k, max_nodes=int(ns.max()), n_nodes=N)
        self._tick("eig_pe + lambda_max")
        pe_s = ops.eig_pe_edges(ei_d, ns_d, Eg_d, k, max_edges=int(E_g.max()), n_nodes=N)
        self._tick("eig_pe_edges")
        ei_t, w_t, ei_s, w_s, _ = ops.hodge_build(ei_d, ns_d, lmax=lam64.to(torch.float32),
                                                  sizes=(N,) + SuperpixelPipeline._nnz(ei_b, N))
        self._tick("Hodge build")
        wt, ws = self.widths
        b = Batch()
        b.num_graphs = B
        b.x_t = torch.empty(N, wt, device=dev)
        b.x_t[:, :self.ft] = xt_f
        b.x_t[:, self.ft:] = pe_t
        b.x_s = torch.empty(E, ws, device=dev)
        b.x_s[:, :self.fs] = xs_f
        b.x_s[:, self.fs:] = pe_s
        b.edge_index_t, b.edge_weight_t = ei_t, w_t
        b.edge_index_s, b.edge_weight_s = ei_s, w_s
        b.edge_index = ei_d
        b.y = y_d.clone() if self.y_dim == 1 else y_d.view(B, self.y_dim).clone()
        b.num_node1, b.num_edge1 = ns_d, Eg_d
        b.num_nodes = N
        b.hodge_sorted = {"edge_index_s": True, "edge_index_t": True}
        b.l1_factor = False
        b._mark()
        b._mol_host = (ns, E_g, ei)
        self._tick("features")
        return b

    # -- the stored dataset --------------------------------------------------------
    def graphs(self, device="cuda", chunk: int = 1024) -> List[PairData]:
        """The stored dataset process() writes, as per-graph host PairData
        (ready for PackedGraphs / GraphLoader / shard_graphs): device batches
        of `chunk` molecules cut back into graphs.  An eigenvector's sign, and
        the basis inside a cluster of equal eigenvalues, follow the graph's
        place in its launch (the solver's start vectors are seeded by it), so
        another chunk size gives other, equally valid signs; everything else
        is the same bits."""
        if str(device) == "cpu":
            return [self._graph_host(i) for i in range(len(self))]
        out = []
        for c0 in range(0, len(self), int(chunk)):
            idx = np.arange(c0, min(c0 + int(chunk), len(self)))
            b = self.batch(idx, device)
            ns, E_g, ei = b._mol_host
            x_t, x_s, y = b.x_t.cpu(), b.x_s.cpu(), b.y.cpu()
            eit, wt, eis, ws = (t.cpu() for t in (b.edge_index_t, b.edge_weight_t,
                                                  b.edge_index_s, b.edge_weight_s))
            n_off = np.concatenate([[0], np.cumsum(ns)])
            e_off = np.concatenate([[0], np.cumsum(E_g)])
            # entries of L0 / L1 per graph, from the degrees (SuperpixelPipeline._nnz)
            gid_e = np.repeat(np.arange(idx.size), E_g)
            deg = np.bincount((ei + n_off[gid_e]).reshape(-1), minlength=int(n_off[-1]))
            gid_n = np.repeat(np.arange(idx.size), ns)
            z_t = np.bincount(gid_n, weights=(deg > 0), minlength=idx.size).astype(np.int64) + 2 * E_g
            z_s = np.bincount(gid_n, weights=deg * deg, minlength=idx.size).astype(np.int64) - E_g
            t_off = np.concatenate([[0], np.cumsum(z_t)])
            s_off = np.concatenate([[0], np.cumsum(z_s)])
            for g in range(idx.size):
                n0, n1, e0, e1 = n_off[g], n_off[g + 1], e_off[g], e_off[g + 1]
                p = PairData(x_s=x_s[e0:e1].clone(),
                             edge_index_s=(eis[:, s_off[g]:s_off[g + 1]] - e0).contiguous(),
                             edge_weight_s=ws[s_off[g]:s_off[g + 1]].clone(),
                             x_t=x_t[n0:n1].clone(),
                             edge_index_t=(eit[:, t_off[g]:t_off[g + 1]] - n0).contiguous(),
                             edge_weight_t=wt[t_off[g]:t_off[g + 1]].clone(),
                             y=y[g:g + 1].clone())
                p.edge_index = torch.from_numpy(np.ascontiguousarray(ei[:, e0:e1]))
                p.num_node1, p.num_edge1, p.num_nodes = int(ns[g]), int(E_g[g]), int(ns[g])
                p._hodge_sorted = True
                out.append(p)
        return out

    # -- per-access MLGC -------------------------------------------------------------
    def coarsen(self, batch: Batch, seed: int = 0, perms=None, mlgc: str = "device") -> List[Batch]:
        """Peptides_Func_EigPE_MLGC.get's MLGC (:633-637) for a collated
        level-0 batch (batch()): graclus node orders per graph drawn from
        `seed` (perms: explicit orders), the fine -> coarse maps by
        ops.mlgc_device (mlgc="device": one device -> host read, the coarse
        sizes) or hodge_dataset.mlgc_batch_flat (mlgc="host"); returns [lv0,
        lv1]: lv0 = the batch with c_node / c_edge as a new column 0 of x_t /
        x_s, lv1 the coarse level (ones features, its own Laplacians).  The
        two routes agree bit for bit given the same orders.  A batch on the
        host takes the reference's arithmetic graph by graph."""
        import copy
        if mlgc not in ("host", "device"):
            raise ValueError(f"MoleculePipeline: mlgc must be 'host' or 'device' (got {mlgc!r})")
        host = getattr(batch, "_mol_host", None)
        if host is None:  # a batch collated elsewhere: its counts and edges are read back
            ns = np.asarray(batch.num_node1.cpu(), np.int64)
            E_g = np.asarray(batch.num_edge1.cpu(), np.int64)
            ei = np.asarray(batch.edge_index.cpu(), np.int64)[:, :int(E_g.sum())]
            ei = ei - np.repeat(np.concatenate([[0], np.cumsum(ns)[:-1]]), E_g)
        else:
            ns, E_g, ei = host
        B = ns.size
        if perms is None:
            rng = np.random.default_rng(seed)
            perms = [rng.permutation(int(n)) for n in ns]
        perm = np.concatenate([np.asarray(p, np.int64) for p in perms])
        dev = batch.x_t.device
        lv0 = copy.copy(batch)
        n_off = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
        e_off = np.concatenate([[0], np.cumsum(E_g)]).astype(np.int64)
        if dev.type == "cpu" or mlgc == "host":
            mg = mlgc_batch_flat(ei, E_g, ns, perm)
            c_node = torch.from_numpy(mg.c_node.astype(np.float32))
            c_edge = torch.from_numpy(mg.c_edge)
            if dev.type == "cpu":
                from .hodge_dataset import _mlgc_level
                lv1 = collate([_mlgc_level(e1, n1) for _, _, e1, n1 in mg.per_graph()],
                              check_hodge=False)
            else:
                n1, m1 = mg.cn, mg.cm
                o1 = np.concatenate([[0], np.cumsum(n1)]).astype(np.int64)
                cidx = self._segments(e_off[:-1], m1)
                ei1 = mg.ce[:, cidx] + o1[np.repeat(np.arange(B), m1)]
                N1, E1 = int(o1[-1]), int(ei1.shape[1])
                idev = _h2d(np.concatenate([ei1.reshape(-1), n1, m1]), dev)
                fdev = _h2d(np.concatenate([mg.c_node.astype(np.float32), mg.c_edge]), dev)
                c_node, c_edge = fdev[:n_off[-1]], fdev[n_off[-1]:]
                lv1 = _coarse_level(idev[:2 * E1].view(2, E1), idev[2 * E1:2 * E1 + B],
                                    idev[2 * E1 + B:], N1, E1,
                                    (N1,) + SuperpixelPipeline._nnz(ei1, N1), dev)
        else:
            from . import ops
            ptrs = _h2d(np.concatenate([perm, n_off, e_off]), dev)
            N = int(n_off[-1])
            perm_d, nptr_d, eptr_d = ptrs[:N], ptrs[N:N + B + 1], ptrs[N + B + 1:]
            r = ops.mlgc_device(batch.edge_index, nptr_d, eptr_d, perm_d)
            n1_d, m1_d = r.cn, r.cm
            # the one read-back: the coarse level's sizes
            N1, E1 = (int(v) for v in torch.stack([n1_d.sum(), m1_d.sum()]).cpu())
            gid_c = torch.repeat_interleave(torch.arange(B, device=dev), m1_d, output_size=E1)
            c_off = torch.cumsum(m1_d, 0) - m1_d
            o1 = torch.cumsum(n1_d, 0) - n1_d
            src = torch.arange(E1, device=dev) - c_off[gid_c] + eptr_d[:-1][gid_c]
            ei1_d = r.ce[:, src] + o1[gid_c]
            c_node, c_edge = r.c_node, r.c_edge
            lv1 = _coarse_level(ei1_d, n1_d, m1_d, N1, E1, None, dev)
        lv0.x_t = torch.cat([c_node.view(-1, 1), batch.x_t], dim=1)
        lv0.x_s = torch.cat([c_edge.view(-1, 1), batch.x_s], dim=1)
        return [lv0, lv1]
