"""Golden fixture for simplex dropout (tests/golden/tsp_aug_small.npz) from the
REFERENCE itself.

Run where a checkout of the reference is at hand (like make_golden.py):

    python tests/golden/make_golden_tsp_aug.py REFERENCE_ROOT

It imports the reference's lib/Hodge_Dataset.py and lib/Hodge_ST_Model.py
behind pyg_standin.py, calls the reference's own dropout_node
(lib/Hodge_Dataset.py:142-166, the function TSP_EigPE.get applies at :690-708)
with p = 0.2 and training=True on each of the two TSP-like graphs of
tsp_model_small, with seeded torch and numpy generators and a fixed protected
subset y, then runs the reference's HL_HGCNN_TSP_dense_int3_pyr forward and
backward on the FILTERED edge_index_s / edge_weight_s with the keep mask as the
second column of x_s -- what the training loop would see with the augmentation
on.  Stored: the UNFILTERED batch, y, the mask, out, R, the state dict and
every parameter gradient, as plain .npz arrays.  Nothing from the reference
source is copied.

dropout_node calls torch_geometric.utils.subgraph, which the stand-in leaves a
placeholder; this script gives the reference module its own restatement of the
documented mask form (below).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "hl-hgat_amd"))

from make_golden import _RefData, _np, _save  # noqa: E402


def subgraph(subset, edge_index, edge_attr=None, relabel_nodes=False, num_nodes=None,
             return_edge_mask=False):
    """torch_geometric.utils.subgraph for a boolean node mask (documented
    semantics): keep the edges whose two ends are both in ``subset``, in
    order, without relabelling; returns (edge_index, edge_attr[, edge_mask])."""
    assert subset.dtype == torch.bool and not relabel_nodes
    edge_mask = subset[edge_index[0]] & subset[edge_index[1]]
    ei = edge_index[:, edge_mask]
    ea = edge_attr[edge_mask] if edge_attr is not None else None
    return (ei, ea, edge_mask) if return_edge_mask else (ei, ea)


def protected(E: int) -> torch.Tensor:
    """The fixed protected subset (the reference's y_loc: the tour's edges)."""
    return (torch.arange(E) % 5 == 0).to(torch.float32)


def tsp_aug_case(ref_ds, ref_model):
    from hlhgat.hodge_dataset import collate
    from hlhgat.synthetic import tsp_like_graph
    graphs = [tsp_like_graph(40 + s, n=48, k=4, row_order=False) for s in range(2)]
    b = collate(graphs, check_hodge=True)
    torch.manual_seed(21)
    np.random.seed(21)
    masks, ys, ei_f, w_f, off = [], [], [], [], 0
    for g in graphs:
        E = g.x_s.shape[0]
        y = protected(E)
        ei, w, edge_mask, node_mask = ref_ds.dropout_node(
            edge_index=g.edge_index_s, edge_attr=g.edge_weight_s, y_loc=y, p=0.2, training=True)
        assert node_mask.shape == (E,) and bool(node_mask[y.bool()].all())
        masks.append(node_mask.to(torch.float32))
        ys.append(y)
        ei_f.append(ei + off)
        w_f.append(w)
        off += E
    mask, y = torch.cat(masks), torch.cat(ys)
    assert 0 < int(mask.sum()) < mask.numel()
    # x_s = [length, node_mask] (lib/Hodge_Dataset.py:707)
    x_s = torch.cat([b.x_s[:, :1], mask.view(-1, 1)], dim=-1)
    torch.manual_seed(4)
    m = ref_model.HL_HGCNN_TSP_dense_int3_pyr(channels=[1, 1], filters=[16, 16],
                                              mlp_channels=[32], K=3)
    m.train()
    d = _RefData()
    for k in ("x_t", "edge_index_t", "edge_weight_t", "edge_index"):
        setattr(d, k, getattr(b, k))
    d.x_s = x_s
    d.edge_index_s, d.edge_weight_s = torch.cat(ei_f, dim=1), torch.cat(w_f)
    d.num_node1 = [int(v) for v in b.num_node1]
    d.num_edge1 = [int(v) for v in b.num_edge1]
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    out, s_batch = m(d, device="cpu")
    R = torch.randn(out.shape, generator=torch.Generator().manual_seed(8))
    (out * R).sum().backward()
    arrays = dict(x_t=_np(b.x_t), x_s=_np(x_s), edge_index_t=_np(b.edge_index_t),
                  edge_weight_t=_np(b.edge_weight_t), edge_index_s=_np(b.edge_index_s),
                  edge_weight_s=_np(b.edge_weight_s), edge_index=_np(b.edge_index),
                  num_node1=_np(b.num_node1), num_edge1=_np(b.num_edge1), y=_np(y),
                  mask=_np(mask), nnz_filtered=np.int64(d.edge_index_s.shape[1]), out=_np(out),
                  s_batch=_np(s_batch), R=_np(R))
    for k, v in sd0.items():
        arrays["sd/" + k] = _np(v)
    for k, p in m.named_parameters():
        arrays["grad/" + k] = _np(p.grad)
    _save("tsp_aug_small", **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_tsp_aug.py REFERENCE_ROOT")
    ref_root = sys.argv[1]
    import pyg_standin
    pyg_standin.install()
    sys.path.insert(0, ref_root)
    import lib.Hodge_Dataset as ref_ds          # noqa: E402  (reference code)
    import lib.Hodge_ST_Model as ref_model      # noqa: E402
    ref_ds.subgraph = subgraph
    torch.set_num_threads(1)  # deterministic CPU reduction order
    tsp_aug_case(ref_ds, ref_model)
