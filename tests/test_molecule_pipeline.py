"""The molecular data path (hlhgat.pipeline.MoleculePipeline) against the
reference's own ZINC_HG_BM_par1_EigPE.process, Peptides_Func_EigPE.process and
Peptides_Func_EigPE_MLGC.get (lib/Hodge_Dataset.py:442-477, :571-605,
:628-650; fixture tests/golden/make_golden_molecule.py: keig = 16, the PE cut
to its first 15 columns, graclus node orders stored).

Columns: zinc x_t = [one_hot(x, 21), PE(15)], x_s = [one_hot(attr - 1, 3),
PE(15)]; peptides x_t = [x(9), PE(15)], x_s = [attr(3), PE(15)]; a graph with
fewer PE columns than 15 is zero-padded, as get() pads it.  An eigenvector is
defined up to sign (get() flips the signs at random anyway), so PE columns
are compared in absolute value.

* CPU (device="cpu", the reference's arithmetic): edge_index, both
  Laplacians' COO and weights, the non-PE columns, y and the widths exact; PE
  columns |.| exact; coarsen(mlgc="host") with the stored orders reproduces
  both stored MLGC levels.  The *_structure_* tests hold what no LAPACK call
  touches; the weights' and the PE's bits are float32 LAPACK's and equal the
  fixture's only on a host like the one that generated it (see
  test_molecule_host_matches_reference_process).
* GPU (hlhgat_eig_pe, hlhgat_eig_pe_edges, hlhgat_hodge_build): indices
  exact, weights within 1e-6 relative, PE |.| within 1e-4 at the columns whose
  eigenvalue in the fixture's scaled Laplacian is > 1e-3 from its neighbours
  (at least half of the fixture's PE columns per side are so compared);
  coarsen device == host bitwise; graphs() -> PackedGraphs.collate -> a head's
  eager forward bitwise the forward on batch().
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import close, load_golden

G = "molecule_process"
KEYS_IDX = ("edge_index", "edge_index_t", "edge_index_s")
KEYS_W = ("edge_weight_t", "edge_weight_s")
FIXED = {"zinc": (21, 3), "peptides": (9, 3)}


@functools.lru_cache(maxsize=None)
def _golden():
    return load_golden(G)


def _raw(tag):
    from hlhgat.hodge_dataset import PairData
    g = _golden()
    d = PairData()
    for key in ("x", "edge_index", "edge_attr", "y"):
        setattr(d, key, torch.from_numpy(g[f"{tag}/raw/{key}"]))
    return d


@functools.lru_cache(maxsize=None)
def _pipe(kind):
    from hlhgat.pipeline import MoleculePipeline
    g = _golden()
    t, n = ("z", int(g["n_zinc"])) if kind == "zinc" else ("p", int(g["n_peptides"]))
    return MoleculePipeline([_raw(f"{t}{i}") for i in range(n)], kind=kind, keig=int(g["keig"]))


def _samples():
    return [("zinc", i) for i in range(10)] + [("peptides", i) for i in range(2)]


def _tag(kind, i):
    return f"{'z' if kind == 'zinc' else 'p'}{i}"


def _padded(ref, width):
    """The stored feature block in get()'s width (zero-padded when the graph
    has fewer PE columns)."""
    out = np.zeros((ref.shape[0], width), ref.dtype)
    out[:, :ref.shape[1]] = ref[:, :width]
    return out


def test_fixture_is_the_issue_s():
    g = _golden()
    assert int(g["keig"]) == 16 and int(g["n_zinc"]) == 10 and int(g["n_peptides"]) == 2
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", G + ".npz")) < 300 * 1024
    n = [g[f"z{i}/x_t"].shape[0] for i in range(10)]
    assert n == [9, 12, 17, 23, 30, 38, 14, 14, 20, 12]
    assert g["z8/x_s"].shape[0] == 19 and g["z9/x_s"].shape[0] == 12  # the tree, the ring
    assert [g[f"p{i}/x_t"].shape[0] for i in range(2)] == [60, 150]
    assert g["p0/raw/edge_attr"].shape[1] == 3
    # both directions, shuffled: to_undirected has work to do
    ei = g["z3/raw/edge_index"]
    assert ei.shape[1] == 2 * g["z3/x_s"].shape[0] and (ei[0] > ei[1]).any() and (ei[0] < ei[1]).any()
    assert (np.diff(ei[0]) < 0).any()


def test_to_undirected_min_nd_matches_standin():
    """The 2-D (and integer) to_undirected(reduce='min') against the stand-in
    of tests/golden, with attributes that differ between the two directions."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden_molecule import standin_to_undirected
    from hlhgat.pipeline import to_undirected_min, to_undirected_min_nd
    g = _golden()
    rng = np.random.default_rng(0)
    for tag, shape in (("p0", (3,)), ("p1", (3,)), ("z4", ())):
        ei = g[f"{tag}/raw/edge_index"]
        n = g[f"{tag}/x_t"].shape[0]
        attr = rng.integers(0, 9, (ei.shape[1],) + shape)
        got_ei, got_a = to_undirected_min_nd(ei, attr, n)
        ref_ei, ref_a = standin_to_undirected(torch.from_numpy(ei), torch.from_numpy(attr), n, "min")
        assert np.array_equal(got_ei, ref_ei.numpy()) and got_a.dtype == attr.dtype
        assert np.array_equal(got_a, ref_a.numpy())
        if not shape:  # the 1-D float function it stands beside
            e1, a1 = to_undirected_min(ei, attr.astype(np.float32), n)
            assert np.array_equal(e1, got_ei) and np.array_equal(a1, got_a.astype(np.float32))


def _ulps(a, b):
    """Largest distance of two float32 arrays in units of the last place."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    if a.size == 0:
        return 0
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("kind,i", _samples())
def test_molecule_host_structure_matches_reference_process(kind, i):
    """What no LAPACK touches: edge_index, both Laplacians' COO, the non-PE
    columns, y and the widths are exact, and every weight is exactly
    fl(fl(2 v) / lambda_max) of this host's float32 lambda_max (v the integer
    entry of B1 B1^T / B1^T B1)."""
    from hlhgat.hodge_dataset import hodge_laplacians
    g, p = _golden(), _pipe(kind)
    b = p.batch([i], device="cpu")
    t = _tag(kind, i) + "/"
    for key in KEYS_IDX:
        assert np.array_equal(getattr(b, key).numpy(), g[t + key]), key
    assert np.array_equal(b.y.numpy().reshape(-1), g[t + "y"].reshape(-1))
    ft, fs = FIXED[kind]
    assert (b.x_t.shape[1], b.x_s.shape[1]) == (ft + 15, fs + 15) == p.widths
    for key, nf in (("x_t", ft), ("x_s", fs)):
        got, ref = getattr(b, key).numpy(), _padded(g[t + key], nf + 15)
        assert got.shape == ref.shape, key
        assert np.array_equal(got[:, :nf], ref[:, :nf]), key
        assert np.all(got[:, nf + min(15, got.shape[0] - 1):] == 0.0), key  # past the graph's size
    _, _, m, par1 = hodge_laplacians(p.ei[i], int(p.n[i]))
    for key, wkey, U in (("edge_index_t", "edge_weight_t", par1 @ par1.T),
                         ("edge_index_s", "edge_weight_s", par1.T @ par1)):
        coo = getattr(b, key)
        assert torch.equal(getattr(b, wkey), (2 * U / m)[coo[0], coo[1]]), wkey


@pytest.mark.parametrize("kind,i", _samples())
def test_molecule_host_matches_reference_process(kind, i):
    """device="cpu" against the stored graph, bit for bit: lambda_max, both
    Laplacians' weights, and the PE columns in absolute value.  These bits are
    LAPACK's (torch.linalg.eigh and scipy.linalg.eigh in float32), which are
    the fixture's only on a host whose LAPACK takes the same code path as the
    one that generated it (MKL 2024.2 on an AVX-512 Intel Xeon: all 12 cases
    pass there).  Measured on an AMD EPYC 9575F with the same MKL build, 10 of
    the 12 cases miss: lambda_max differs by 1 .. 4 ulp (e.g. 5.38748693
    against the fixture's 5.38748503), the weights by 1 .. 5 ulp, and |PE| by
    up to 1e-4 at separated columns and by O(1) inside clusters of equal
    eigenvalues (whose basis is LAPACK's rounding noise); zinc 1 and 6 are
    bitwise there too.  Nothing of it is the pipeline's: the structure test
    above is exact on both hosts, and the device path is held to the same
    fixture by its own rules below.  The figures are printed before the
    assertions."""
    from hlhgat.hodge_dataset import hodge_laplacians
    g, p = _golden(), _pipe(kind)
    b = p.batch([i], device="cpu")
    t = _tag(kind, i) + "/"
    m = hodge_laplacians(p.ei[i], int(p.n[i]))[2]
    ft, fs = FIXED[kind]
    pe = {key: (np.abs(getattr(b, key).numpy()[:, nf:]), np.abs(_padded(g[t + key], nf + 15)[:, nf:]))
          for key, nf in (("x_t", ft), ("x_s", fs))}
    print(t, "lambda_max %.9g fixture %.9g (%d ulp); weights %d / %d ulp; |PE| max diff %.3e / %.3e"
          % (float(m), float(g[t + "maxeig"]), _ulps(m.numpy(), g[t + "maxeig"]),
             _ulps(b.edge_weight_t.numpy(), g[t + "edge_weight_t"]),
             _ulps(b.edge_weight_s.numpy(), g[t + "edge_weight_s"]),
             np.abs(pe["x_t"][0] - pe["x_t"][1]).max(), np.abs(pe["x_s"][0] - pe["x_s"][1]).max()))
    # lambda_max as process() stores it: float32 eigh of the unscaled L0
    assert float(m) == float(g[t + "maxeig"])
    for key in KEYS_W:
        assert np.array_equal(getattr(b, key).numpy(), g[t + key]), key
    for key in ("x_t", "x_s"):
        assert np.array_equal(pe[key][0], pe[key][1]), key


def _check_mlgc_levels(g, t, lv0, lv1, weights):
    """Both levels against the stored get(): indices, the coarse features and
    the cluster maps exact; weights "exact", "close" (1e-6 relative) or None."""
    for lv, b in ((0, lv0), (1, lv1)):
        for key in KEYS_IDX:
            assert np.array_equal(getattr(b, key).cpu().numpy(), g[t + f"l{lv}/{key}"]), (lv, key)
        for key in KEYS_W:
            if weights == "exact":
                assert np.array_equal(getattr(b, key).cpu().numpy(), g[t + f"l{lv}/{key}"]), (lv, key)
            elif weights == "close":
                close(getattr(b, key).cpu(), g[t + f"l{lv}/{key}"], 1e-6, f"l{lv} {key}")
    assert np.array_equal(lv1.x_t.cpu().numpy(), g[t + "l1/x_t"])
    assert np.array_equal(lv1.x_s.cpu().numpy(), g[t + "l1/x_s"])
    # column 0: the cluster maps (inf on an edge inside one cluster)
    for key in ("x_t", "x_s"):
        assert np.array_equal(getattr(lv0, key).cpu().numpy()[:, 0], g[t + f"l0/{key}"][:, 0]), key


@pytest.mark.parametrize("i", [0, 1])
def test_molecule_host_coarsen_structure_matches_reference_get(i):
    """coarsen(mlgc="host") with the stored order: what no LAPACK touches of
    both stored levels (indices, cluster maps, raw columns, coarse features)."""
    g, p = _golden(), _pipe("peptides")
    b = p.batch([i], device="cpu")
    lv0, lv1 = p.coarsen(b, perms=[g[f"p{i}/perm"]], mlgc="host")
    t = f"p{i}/"
    _check_mlgc_levels(g, t, lv0, lv1, weights=None)
    for key, nf in (("x_t", 10), ("x_s", 4)):  # [cluster, raw, PE * random signs]
        got, ref = getattr(lv0, key).numpy(), g[t + f"l0/{key}"]
        assert got.shape == ref.shape, key
        assert np.array_equal(got[:, :nf], ref[:, :nf]), key
    assert b.x_t.shape[1] == 24 and lv0.x_t.shape[1] == 25  # the batch itself is untouched


@pytest.mark.parametrize("i", [0, 1])
def test_molecule_host_coarsen_matches_reference_get(i):
    """Both stored levels bit for bit, weights and |PE| included (LAPACK's
    bits: see test_molecule_host_matches_reference_process; on the EPYC host
    the fine weights are 2 .. 4 ulp and the coarse ones 1 ulp off, and both
    cases miss)."""
    g, p = _golden(), _pipe("peptides")
    b = p.batch([i], device="cpu")
    lv0, lv1 = p.coarsen(b, perms=[g[f"p{i}/perm"]], mlgc="host")
    t = f"p{i}/"
    for lv, lvb in ((0, lv0), (1, lv1)):
        print(t, "level", lv, "weights", [_ulps(getattr(lvb, k).numpy(), g[t + f"l{lv}/{k}"])
                                          for k in KEYS_W], "ulp")
    _check_mlgc_levels(g, t, lv0, lv1, weights="exact")
    for key, nf in (("x_t", 10), ("x_s", 4)):
        got, ref = getattr(lv0, key).numpy(), g[t + f"l0/{key}"]
        assert np.array_equal(np.abs(got[:, nf:]), np.abs(ref[:, nf:])), key


# ---- GPU --------------------------------------------------------------------------------

def _separated_cols(coo, w, n, k=16):
    """PE columns (0-based) whose eigenvalue in the fixture's scaled Laplacian
    is > 1e-3 from both neighbours."""
    L = np.zeros((n, n))
    L[coo[0], coo[1]] = w
    ev = np.linalg.eigvalsh(L)
    out = []
    for j in range(1, min(k, n)):
        gap = min(ev[j] - ev[j - 1], ev[j + 1] - ev[j] if j + 1 < n else np.inf)
        if gap > 1e-3:
            out.append(j - 1)
    return out, min(k, n) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "peptides"])
def test_molecule_device_matches_reference_process(cuda, kind, monkeypatch):
    """One device batch of all the fixture's molecules of a kind, cut back by
    graphs()'s offsets, against the stored graphs."""
    from hlhgat import ops
    monkeypatch.setattr(ops, "_CHECK_SIZES", True)
    g, p = _golden(), _pipe(kind)
    idx = list(range(len(p)))
    ops.check_device_errors()
    b = p.batch(idx, device=cuda)
    ops.check_device_errors()
    for key, v in vars(b).items():
        assert not torch.is_tensor(v) or v.is_contiguous(), key
    assert b.num_node1.is_cuda and b.num_edge1.is_cuda and b.hodge_sorted["edge_index_s"]
    ft, fs = FIXED[kind]
    assert (b.x_t.shape[1], b.x_s.shape[1]) == (ft + 15, fs + 15)
    ns = [g[f"{_tag(kind, i)}/x_t"].shape[0] for i in idx]
    es = [g[f"{_tag(kind, i)}/x_s"].shape[0] for i in idx]
    assert b.num_node1.cpu().tolist() == ns and b.num_edge1.cpu().tolist() == es
    n_off, e_off = np.concatenate([[0], np.cumsum(ns)]), np.concatenate([[0], np.cumsum(es)])
    assert np.array_equal(b.y.cpu().numpy().reshape(-1),
                          np.concatenate([g[f"{_tag(kind, i)}/y"].reshape(-1) for i in idx]))
    # the collated COO against the stored graphs with PairData offsets
    for key, off, wkey in (("edge_index", n_off, None), ("edge_index_t", n_off, "edge_weight_t"),
                           ("edge_index_s", e_off, "edge_weight_s")):
        ref = np.concatenate([g[f"{_tag(kind, i)}/{key}"] + off[i] for i in idx], axis=1)
        assert np.array_equal(getattr(b, key).cpu().numpy(), ref), key
        if wkey:
            ref_w = np.concatenate([g[f"{_tag(kind, i)}/{wkey}"] for i in idx])
            close(getattr(b, wkey).cpu(), ref_w, 1e-6, wkey)
    xt, xs = b.x_t.cpu().numpy(), b.x_s.cpu().numpy()
    for side, x, off, nf, coo in (("node", xt, n_off, ft, "t"), ("edge", xs, e_off, fs, "s")):
        compared = pairs = 0
        for i in idx:
            t = _tag(kind, i) + "/"
            got = x[off[i]:off[i + 1]]
            ref = _padded(g[t + ("x_t" if coo == "t" else "x_s")], nf + 15)
            assert np.array_equal(got[:, :nf], ref[:, :nf]), (side, i)
            rows = got.shape[0]
            cols, m1 = _separated_cols(g[t + f"edge_index_{coo}"], g[t + f"edge_weight_{coo}"], rows)
            assert np.all(got[:, nf + m1:] == 0.0), (side, i)  # past the graph's size
            pe = [nf + c for c in cols]
            close(np.abs(got[:, pe]), np.abs(ref[:, pe]), 1e-4, f"{side} PE |.| of {t}")
            compared += len(cols)
            pairs += m1
        print(kind, side, "PE columns compared:", compared, "of", pairs)
        assert 2 * compared >= pairs, (side, compared, pairs)


@pytest.mark.gpu
def test_molecule_device_coarsen_bitwise_host(cuda):
    g, p = _golden(), _pipe("peptides")
    from hlhgat import ops
    b = p.batch([1, 0], device=cuda)
    perms = [g["p1/perm"], g["p0/perm"]]
    ops.check_device_errors()
    dv = p.coarsen(b, perms=perms, mlgc="device")
    ho = p.coarsen(b, perms=perms, mlgc="host")
    ops.check_device_errors()
    for lv, (d, h) in enumerate(zip(dv, ho)):
        for key in KEYS_IDX + KEYS_W + ("x_t", "x_s", "num_node1", "num_edge1"):
            assert torch.equal(getattr(d, key), getattr(h, key)), (lv, key)
        assert d.num_nodes == h.num_nodes
    assert dv[0].x_t.shape[1] == 25 and b.x_t.shape[1] == 24
    # and against the reference's get() for the second graph of the batch
    one = p.coarsen(p.batch([0], device=cuda), perms=[g["p0/perm"]], mlgc="device")
    _check_mlgc_levels(g, "p0/", one[0], one[1], weights="close")
    # a seed draws the orders: the same seed, the same levels
    a, c = p.coarsen(b, seed=3), p.coarsen(b, seed=3)
    assert torch.equal(a[0].x_t, c[0].x_t) and torch.equal(a[1].edge_index, c[1].edge_index)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "peptides"])
def test_molecule_graphs_forward_bitwise_batch(cuda, kind):
    """graphs() -> PackedGraphs.collate -> the head's eager forward is bitwise
    the forward on batch() of the same molecules."""
    import hlhgat
    from hlhgat.hodge_dataset import PackedGraphs
    p = _pipe(kind)
    graphs = p.graphs(device=cuda)
    assert len(graphs) == len(p) and all(not gr.x_t.is_cuda for gr in graphs)
    # an eigenvector's sign (and the basis of a cluster) follows the graph's
    # place in its launch, so the same molecules in the same order: one chunk.
    # Cut into chunks, everything but those signs is the same.
    for a, c in zip(graphs, p.graphs(device=cuda, chunk=7)):
        for key in KEYS_IDX + KEYS_W + ("y",):
            assert torch.equal(getattr(a, key), getattr(c, key)), key
        assert torch.equal(a.x_t[:, :FIXED[kind][0]], c.x_t[:, :FIXED[kind][0]])
    idx = list(range(len(p)))
    packed = PackedGraphs(graphs, check_hodge=True).collate(idx).to(cuda)
    b = p.batch(idx, device=cuda)
    for key in KEYS_IDX + KEYS_W + ("x_t", "x_s", "num_node1", "num_edge1"):
        assert torch.equal(getattr(packed, key), getattr(b, key)), key
    assert torch.equal(packed.y.view(-1), b.y.view(-1))
    torch.manual_seed(0)
    head = (hlhgat.HL_HGCNN_zinc_dense_int3_pyr if kind == "zinc"
            else hlhgat.HL_HGCNN_pepfunc_dense_int3_pyr)
    m = head(channels=[1, 1], filters=[32, 32], mlp_channels=[64], K=3, keig=15).to(cuda).eval()
    with torch.no_grad():
        out_p, out_b = m(packed), m(b)
    torch.cuda.synchronize()
    assert out_p.shape[0] == len(p) and torch.isfinite(out_b).all()
    assert torch.equal(out_p, out_b)


@pytest.mark.gpu
def test_molecule_coarsen_feeds_attpool_head(cuda):
    """[lv0, lv1] of coarsen() is what the peptides attpool head takes: its
    eager forward runs on it, and the device and host MLGC routes give the
    same bits."""
    import hlhgat
    g, p = _golden(), _pipe("peptides")
    b = p.batch([0, 1], device=cuda)
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_pepfunc_dense_int3_attpool(
        channels=[1, 1], filters=[32, 32], mlp_channels=[64], K=3, pool_loc=0, keig=15).to(cuda).eval()
    with torch.no_grad():
        out_d = m(p.coarsen(b, seed=5, mlgc="device"))
        out_h = m(p.coarsen(b, seed=5, mlgc="host"))
    torch.cuda.synchronize()
    assert out_d.shape == (2, 10) and torch.isfinite(out_d).all()
    assert torch.equal(out_d, out_h)
