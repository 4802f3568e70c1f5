"""Simplex dropout: the mask draw (csrc/simplex.hip) against
its numpy restatement (simplex_ref.py), masked Hodge operators against the
existing kernels on the host-filtered operator, the head against the
reference's own run on the filtered COO (tests/golden/make_golden_tsp_aug.py)
and the augmentation under TrainStep.

Tolerances, per assertion:
  * the draw: bit for bit;
  * masked CSR operator vs the host-filtered operator: torch.equal (the same
    kernels sum the same terms in the same order, plus 0 * x);
  * factored vs CSR: 1e-5 relative forward, 1e-4 gradients (test_gpu_parity's);
  * the head vs the reference fixture: 1e-4 relative (as tsp_model_small).
"""
import copy
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import dropout_ref
import simplex_ref as S
from conftest import close, load_golden
from oracle import hodge_ref as R

T = torch.from_numpy
SEED, STEP = 1234, 7
HEAD_KW = dict(channels=[1, 1], filters=[16, 16], mlp_channels=[32], K=3)
BATCH_KEYS = ("x_t", "x_s", "edge_index_t", "edge_weight_t", "edge_index_s", "edge_weight_s",
              "edge_index", "num_node1", "num_edge1")


def dev(a, d="cuda:0"):
    return (T(a) if isinstance(a, np.ndarray) else a).to(d)


def filtered(ei, w, mask):
    """subgraph(mask, ei, w) without relabelling: entries with both ends kept."""
    m = torch.as_tensor(mask).reshape(-1) != 0
    keep = m[ei[0]] & m[ei[1]]
    return ei[:, keep].contiguous(), w[keep].contiguous(), keep


def sym_graph(n, nnz, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randint(0, n, (nnz,), generator=g)
    c = torch.randint(0, n, (nnz,), generator=g)
    w = torch.randn(nnz, generator=g)
    key = torch.cat([r * n + c, c * n + r])
    key, first = np.unique(key.numpy(), return_index=True)  # one entry per (row, col)
    w2 = torch.cat([w, w])[T(first)]
    return torch.stack([T(key) // n, T(key) % n]).contiguous(), w2.contiguous()


def rand_mask(n, drop, seed):
    return (torch.rand(n, generator=torch.Generator().manual_seed(seed)) >= drop).float()


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(1, 0.5), (130, 0.25), (1027, 0.9)])
def test_ref_special_case_is_feature_dropout_rule(n, p):
    """aug_prob = 1, jitter = 0, no protection: dropout_ref.keep at SITE_E."""
    for k in (0, 3):
        got = S.keep([0, n], n, 1.0, p, 0.0, SEED, STEP, k=k)
        exp = dropout_ref.keep(n, 1, p, SEED, STEP, S.sites(k)[1])[:, 0]
        assert np.array_equal(got, exp.astype(np.float32))


def test_ref_aug_off_protect_and_padding():
    seg, n = [0, 5, 5, 135], 142
    assert np.array_equal(S.keep(seg, n, 0.0, 0.9, 0.1, SEED, STEP)[:135], np.ones(135, np.float32))
    prot = np.zeros(n, np.float32)
    prot[::3] = 2.0
    m = S.keep(seg, n, 1.0, 0.9, 0.1, SEED, STEP, protect=prot)
    assert (m[:135][prot[:135] != 0] == 1).all()
    assert 0 < m[:135].sum() < 135
    assert (m[135:] == 0).all()  # padding rows, protected or not
    assert set(np.unique(m)) <= {0.0, 1.0}


def test_ref_keep_rates():
    """Seed 1234, step 7, k = 0: every rate within 4 sigma of its expectation."""
    G = 4096
    for ap in (0.25, 0.5, 0.75):
        aug, _ = S.graph_draw(G, ap, 0.0, 0.5, SEED, STEP)
        sig = np.sqrt(ap * (1 - ap) / G)
        print("augmented share", ap, aug.mean(), abs(aug.mean() - ap) / sig, "sigma")
        assert abs(aug.mean() - ap) <= 4 * sig
    _, Tg = S.graph_draw(G, 1.0, 0.0, 0.5, SEED, STEP)
    rate = Tg.astype(np.float64) / 2.0 ** 24  # uniform on [0, 0.5)
    sig = 0.5 / np.sqrt(12.0) / np.sqrt(G)
    print("mean rate", rate.mean(), abs(rate.mean() - 0.25) / sig, "sigma")
    assert abs(rate.mean() - 0.25) <= 4 * sig
    assert rate.min() >= 0 and rate.max() < 0.5
    n = 65536
    m = S.keep([0, n], n, 1.0, 0.25, 0.0, SEED, STEP)
    sig = np.sqrt(0.25 * 0.75 / n)
    print("row keep rate", m.mean(), abs(m.mean() - 0.75) / sig, "sigma")
    assert abs(m.mean() - 0.75) <= 4 * sig


@pytest.mark.parametrize("d", [1, 3, 32])
def test_oracle_filtered_coo_equals_zeroed_weights(d):
    """M L M on L's own COO (weights zeroed where an end is dropped) gives the
    oracle exactly what the filtered COO gives."""
    n = 200
    ei, w = sym_graph(n, 1500, seed=d)
    mask = rand_mask(n, 0.3, seed=9)
    ei_f, w_f, keep = filtered(ei, w, mask)
    assert 0 < ei_f.size(1) < ei.size(1)
    w_z = torch.where(keep, w, torch.zeros_like(w))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, d, generator=g)
    ws = [torch.randn(d, d, generator=g) for _ in range(4)]
    b = torch.randn(d, generator=g)
    assert torch.equal(R.propagate(x, ei_f, w_f), R.propagate(x, ei, w_z))
    for conv in (R.laguerre_conv, R.cheb_conv):
        assert torch.equal(conv(x, ei_f, w_f, ws, b), conv(x, ei, w_z, ws, b))


class _D:
    pass


def _check_head_grads(named_grads, g, tol=1e-4):
    for k, grad in named_grads:
        if re.search(r"module_[04]\.bias$", k) and not k.startswith("out."):
            # a conv bias feeding a training-mode BatchNorm: analytically zero
            # gradient, both sides hold fp32 rounding noise only
            assert float(grad.abs().max()) < 1e-3 and float(np.abs(g["grad/" + k]).max()) < 1e-3
            continue
        close(grad.cpu(), g["grad/" + k], tol, "grad " + k)


def test_oracle_head_reproduces_augmented_fixture():
    """RefTSPModel on the fixture's filtered L1 (mask column in x_s) vs the
    reference's own run through dropout_node, at tsp_model_small's tolerance."""
    g = load_golden("tsp_aug_small")
    d = _D()
    for k in BATCH_KEYS:
        setattr(d, k, T(g[k]))
    assert np.array_equal(g["x_s"][:, 1], g["mask"])
    assert (g["mask"][g["y"] != 0] == 1).all() and 0 < g["mask"].sum() < g["mask"].size
    d.edge_index_s, d.edge_weight_s, _ = filtered(d.edge_index_s, d.edge_weight_s, g["mask"])
    assert d.edge_index_s.size(1) == int(g["nnz_filtered"])
    m = R.RefTSPModel(**HEAD_KW)
    m.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")})
    m.train()
    out, s_batch = m(d)
    assert torch.equal(s_batch, T(g["s_batch"]))
    close(out.detach(), g["out"], 1e-5, "out")
    (out * T(g["R"])).sum().backward()
    _check_head_grads(((k, p.grad) for k, p in m.named_parameters()), g)


def test_capi_argument_errors():
    """Argument validation runs before any HIP call; empty input is a no-op."""
    import torch  # noqa: F401,F811
    from hlhgat import _lib
    L = _lib.LIB
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)  # a non-NULL pointer that is never dereferenced
    p += -p % 16
    T24, site = 1 << 24, 0x80000000

    def err(rc, text):
        assert rc == 1
        assert text.encode() in L.hlhgat_last_error(), L.hlhgat_last_error()

    keep = L.hlhgat_simplex_keep
    err(keep(None, 1, 8, None, 0, 0, 0, 0, site, p, p, None, 0, None), "NULL pointer")
    err(keep(p, 1, 8, None, 0, 0, 0, 0, site, None, p, None, 0, None), "NULL pointer")
    err(keep(p, 1, 8, None, 0, 0, 0, 0, site, p, None, None, 0, None), "NULL pointer")
    err(keep(p, 1, 8, None, 0, T24 + 1, 0, 0, site, p, p, None, 0, None), "exceeds 2^24")
    err(keep(p, 1, 8, None, 0, 0, T24 + 1, 0, site, p, p, None, 0, None), "exceeds 2^24")
    err(keep(p, 1, 8, None, 0, 0, 0, T24 + 1, site, p, p, None, 0, None), "exceeds 2^24")
    err(keep(p, 1, 8, None, 0, 0, T24 // 2 + 1, T24 // 2, site, p, p, None, 0, None),
        "Tp + Tj")
    err(keep(p, 1, -1, None, 0, 0, 0, 0, site, p, p, None, 0, None), "bad sizes")
    err(keep(p, -1, 8, None, 0, 0, 0, 0, site, p, p, None, 0, None), "bad sizes")
    err(keep(p, 1, 8, p, 0, 0, 0, 0, site, p, p, None, 0, None), "leading dimension")
    err(keep(p, 1, 8, None, 0, 0, 0, 0, site, p, p, p, 0, None), "leading dimension")
    err(keep(p, 1, 8, None, 0, 0, 0, 0, 5, p, p, None, 0, None), "site")
    err(keep(p, 1, 8, None, 0, 0, 0, 0, site + 1, p, p, None, 0, None), "site")
    assert keep(None, 0, 0, None, 0, T24, T24, 0, site, None, None, None, 0, None) == 0

    csr = L.hlhgat_mask_csr_values
    err(csr(p, p, p, -1, 4, p, p, None), "bad sizes")
    err(csr(p, p, p, 4, -1, p, p, None), "bad sizes")
    for hole in range(5):
        a = [p] * 5
        a[hole] = None
        err(csr(a[0], a[1], a[2], 4, 4, a[3], a[4], None), "NULL pointer")
    assert csr(None, None, None, 0, 0, None, None, None) == 0
    assert csr(None, None, None, 4, 0, None, None, None) == 0

    fac = L.hlhgat_mask_hodge_factor
    err(fac(None, p, p, p, None), "NULL factor")
    d = _lib.HodgeFactorDesc(p, p, p, None, 3, p, p, None, -1)
    err(fac(ctypes.byref(d), p, p, p, None), "n_edges")
    d.n_edges = 4
    err(fac(ctypes.byref(d), None, p, p, None), "NULL pointer")
    err(fac(ctypes.byref(d), p, None, p, None), "NULL pointer")
    err(fac(ctypes.byref(d), p, p, None, None), "NULL pointer")
    d.node_sign = None
    err(fac(ctypes.byref(d), p, p, p, None), "NULL pointer")
    e = _lib.HodgeFactorDesc(None, None, None, None, 0, None, None, None, 0)
    assert fac(ctypes.byref(e), None, None, None, None) == 0


def test_head_state_dict_keys_unchanged():
    import hlhgat
    g = load_golden("tsp_model_small")
    m = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(**HEAD_KW)
    assert m.augment is None
    keys = {k[3:] for k in g if k.startswith("sd/")}
    assert set(m.state_dict()) == keys
    m.augment = hlhgat.nn.SimplexDropout()
    assert set(m.state_dict()) == keys  # no parameters, no buffers
    assert "augment" in dict(m.named_children())
    assert not list(m.augment.parameters()) and not list(m.augment.buffers())


@functools.lru_cache(maxsize=None)
def _two_graphs():
    from hlhgat.hodge_dataset import collate
    from hlhgat.synthetic import tsp_like_graph
    b = collate([tsp_like_graph(40 + s, n=48, k=4, row_order=False) for s in range(2)],
                check_hodge=True)
    b.y = (torch.arange(b.x_s.shape[0]) % 5 == 0).float()
    return b


def _two_graph_batch(device=None):
    b = copy.copy(_two_graphs())
    for k, v in vars(b).items():
        if torch.is_tensor(v):
            setattr(b, k, v.clone())
    return b if device is None else b.to(device)


def test_simplex_dropout_on_cpu_raises():
    import hlhgat
    m = hlhgat.nn.SimplexDropout().train()
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(_two_graph_batch())
    with pytest.raises(ValueError):
        hlhgat.nn.SimplexDropout(p=0.75, jitter=0.5)


# ---------------------------------------------------------------------------
# GPU: the draw kernel
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("protect", [False, True])
@pytest.mark.parametrize("aug_prob", [0.0, 0.5, 1.0])
def test_draw_kernel_bitwise(cuda, aug_prob, protect):
    """Graphs of 5, 0 and 130 rows + 7 padding rows: an empty graph, Philox
    groups straddling graph boundaries, a row count that is no multiple of 4;
    the column at ldc = 2, protect at ldp = 3."""
    from hlhgat import ops
    seg, n, k = [0, 5, 5, 135], 142, 2
    ops.dropout_set_state(SEED, STEP, cuda)
    prot = None
    if protect:
        prot = torch.zeros(n, 3)
        prot[::4, 1] = 1.0
        prot[140, 1] = 1.0  # a protected padding row stays 0
    x = torch.full((n, 2), 7.0, device=cuda)
    mask = torch.full((n,), -1.0, device=cuda)
    pd = prot.to(cuda)[:, 1] if protect else None
    ops.simplex_keep(dev(np.asarray(seg, np.int32)), mask, aug_prob, 0.3, 0.5, site=k, protect=pd,
                     column=x[:, 1])
    exp = S.keep(seg, n, aug_prob, 0.3, 0.5, SEED, STEP, k=k,
                 protect=prot[:, 1].numpy() if protect else None)
    assert np.array_equal(mask.cpu().numpy(), exp)
    assert np.array_equal(x[:, 1].cpu().numpy(), exp)
    assert (x[:, 0] == 7.0).all()
    assert ops.dropout_state(cuda)[:2] == (SEED, STEP)  # the draw advances nothing
    if aug_prob == 1.0 and not protect:
        assert 0 < exp[:135].sum() < 135
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: masked operators
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(name):
    from hlhgat.synthetic import tsp_like_graph
    if name == "l1_small":
        g = tsp_like_graph(40, n=48, k=4, row_order=False)
        return g.edge_index_s, g.edge_weight_s, g.x_s.shape[0]
    if name == "l1_deep":
        g = tsp_like_graph(5, n=300, k=9, row_order=False)
        return g.edge_index_s, g.edge_weight_s, g.x_s.shape[0]
    g = tsp_like_graph(41, n=150, k=5, row_order=False)
    return g.edge_index_t, g.edge_weight_t, g.x_t.shape[0]


def _conv_all(ops, op, x, ws, bias, bn):
    xx = x.clone().requires_grad_(True)
    wl = [w.clone().requires_grad_(True) for w in ws]
    b = bias.clone().requires_grad_(True)
    bn.zero_grad(set_to_none=True)
    y = ops.hodge_poly_conv(xx, op, wl, b, ops.POLY_LAGUERRE, bn=bn, relu=True)
    (y * torch.linspace(-1, 1, y.numel(), device=y.device).view_as(y)).sum().backward()
    return [y.detach(), xx.grad, b.grad] + [w.grad for w in wl] + \
        [bn.weight.grad.clone(), bn.bias.grad.clone()]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 3, 32, 64, 128])
@pytest.mark.parametrize("name", ["l1_small", "l1_deep", "l0"])
def test_masked_csr_operator_equals_filtered_operator(cuda, name, d):
    from hlhgat import ops
    ei, w, n = _graph(name)
    mask = rand_mask(n, 0.3, seed=11)
    ei_f, w_f, _ = filtered(ei, w, mask)
    assert 0 < ei_f.size(1) < ei.size(1)
    ei_m = ops.set_row_mask(ops.mark_hodge(dev(ei)), dev(mask))
    wd = dev(w)
    op_m = ops.hodge_operator(ei_m, wd, n)
    op_f = ops.hodge_operator(ops.mark_hodge(dev(ei_f)), dev(w_f), n)
    op_u = ops.hodge_operator(ops.mark_hodge(dev(ei)), wd, n)
    assert op_m.masked_from is not None and op_m.factor is None
    assert op_m.fwd.nnz == ei.size(1) and op_f.fwd.nnz == ei_f.size(1)
    assert op_m.fwd.val.data_ptr() != op_u.fwd.val.data_ptr()
    assert torch.equal(op_u.fwd.val, wd)  # the unmasked values are left alone
    g = torch.Generator().manual_seed(d)
    x = torch.randn(n, d, generator=g)
    xd = dev(x)
    y = ops.spmm(op_m.fwd, xd)
    assert torch.equal(y, ops.spmm(op_f.fwd, xd))
    assert torch.equal(y.cpu(), R.propagate(x, ei_f, w_f))
    for kind in (ops.POLY_LAGUERRE, ops.POLY_CHEB, ops.POLY_LAGUERRE_DEMO):
        assert torch.equal(ops.poly_basis(op_m, xd, 4, kind), ops.poly_basis(op_f, xd, 4, kind))
    ws = [dev(torch.randn(d, d, generator=g)) for _ in range(4)]
    bias = dev(torch.randn(d, generator=g))
    bn = torch.nn.BatchNorm1d(d).to(cuda).train()
    a = _conv_all(ops, op_m, xd, ws, bias, bn)
    b = _conv_all(ops, op_f, xd, ws, bias, bn)
    for i, (u, v) in enumerate(zip(a, b)):
        assert torch.equal(u, v), (i, (u - v).abs().max())
    ops.check_device_errors()


@pytest.mark.gpu
def test_all_ones_mask_and_refresh(cuda):
    """An all-ones mask is the unmasked operator; refresh_row_mask follows the
    mask in place and allocates nothing."""
    from hlhgat import ops
    ei, w, n = _graph("l1_deep")
    xd = dev(torch.randn(n, 32, generator=torch.Generator().manual_seed(0)))
    wd = dev(w)
    op_u = ops.hodge_operator(ops.mark_hodge(dev(ei)), wd, n)
    mask = torch.ones(n, device=cuda)
    ei_m = ops.set_row_mask(ops.mark_hodge(dev(ei)), mask)
    op_m = ops.hodge_operator(ei_m, wd, n)
    assert torch.equal(op_m.fwd.val, op_u.fwd.val)
    assert torch.equal(ops.spmm(op_m.fwd, xd), ops.spmm(op_u.fwd, xd))
    assert torch.equal(ops.poly_basis(op_m, xd, 4, ops.POLY_LAGUERRE),
                       ops.poly_basis(op_u, xd, 4, ops.POLY_LAGUERRE))
    m2 = rand_mask(n, 0.3, seed=5)
    mask.copy_(dev(m2))
    ptr = op_m.fwd.val.data_ptr()
    op_r = ops.refresh_row_mask(ei_m, wd, n)
    assert op_r is op_m and op_r.fwd.val.data_ptr() == ptr
    assert ops.hodge_operator(ei_m, wd, n) is op_m
    ei_f, w_f, _ = filtered(ei, w, m2)
    op_f = ops.hodge_operator(ops.mark_hodge(dev(ei_f)), dev(w_f), n)
    assert torch.equal(ops.spmm(op_m.fwd, xd), ops.spmm(op_f.fwd, xd))
    ops.clear_caches()  # a rebuilt operator reuses the bound mask's buffers
    assert ops.hodge_operator(ei_m, wd, n).fwd.val.data_ptr() == ptr
    ops.set_row_mask(ei_m, None)
    assert ops.hodge_operator(ei_m, wd, n).masked_from is None
    with pytest.raises(RuntimeError, match="sorted symmetric"):
        ops.set_row_mask(dev(ei), mask)
    ops.check_device_errors()


@functools.lru_cache(maxsize=None)
def _tsp300():
    from hlhgat.synthetic import tsp_like_graph
    return tsp_like_graph(5, n=300, k=9, halo=False)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 32, 128])
@pytest.mark.parametrize("sched", [False, True])
def test_masked_factored_l1_matches_masked_csr(cuda, d, sched):
    """L1 = alpha B1^T B1 with masked sign / alpha tables vs the masked CSR
    operator: 1e-5 relative forward, 1e-4 gradients (as factored vs CSR)."""
    from hlhgat import ops
    from hlhgat.hodge_dataset import hodge_factor_ok
    g = _tsp300()
    n = g.x_s.shape[0]
    assert hodge_factor_ok(g.edge_index, g.x_t.shape[0], g.edge_index_s, g.edge_weight_s)
    mask = dev(rand_mask(n, 0.3, seed=3))
    w = dev(g.edge_weight_s)
    ei_c = ops.set_row_mask(ops.mark_hodge(dev(g.edge_index_s)), mask)
    ei_f = ops.mark_hodge(dev(g.edge_index_s))
    if sched:
        ops.set_row_order(ei_f, g.row_order_s)
    ops.set_hodge_factor(ei_f, dev(g.edge_index), g.x_t.shape[0],
                         g.row_order_t if sched else None)
    ops.set_row_mask(ei_f, mask)
    op_c, op_f = ops.hodge_operator(ei_c, w, n), ops.hodge_operator(ei_f, w, n)
    assert op_c.factor is None and op_f.factor is not None and op_f.masked_from is not None
    base = op_f.masked_from[0]
    assert op_f.factor[2].data_ptr() != base.factor[2].data_ptr()
    assert op_f.factor[0] is base.factor[0] and op_f.factor[4] is base.factor[4]
    gen = torch.Generator().manual_seed(d)
    x = dev(torch.randn(n, d, generator=gen))
    close(ops.hodge_spmm(op_f, x).cpu(), ops.spmm(op_c.fwd, x).cpu(), 1e-5, "factored spmm")
    Tc = ops.poly_basis(op_c, x, 4, ops.POLY_LAGUERRE).cpu()
    Tf = ops.poly_basis(op_f, x, 4, ops.POLY_LAGUERRE).cpu()
    for k in range(3):
        close(Tf[k], Tc[k], 1e-5, f"T_{k + 1}")
    ws = [dev(torch.randn(d, d, generator=gen)) for _ in range(4)]
    bias = dev(torch.randn(d, generator=gen))
    res = []
    for op in (op_c, op_f):
        xx = x.clone().requires_grad_(True)
        wl = [v.clone().requires_grad_(True) for v in ws]
        y = ops.hodge_poly_conv(xx, op, wl, bias, ops.POLY_LAGUERRE)
        (y * torch.linspace(-1, 1, y.numel(), device=cuda).view_as(y)).sum().backward()
        res.append([y.detach().cpu(), xx.grad.cpu()] + [v.grad.cpu() for v in wl])
    for i, (a, c) in enumerate(zip(res[1], res[0])):
        close(a, c, 1e-5 if i == 0 else 1e-4, f"item {i}")
    ops.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 32])
def test_masked_halo_equals_masked_plain(cuda, d):
    from hlhgat import ops
    from hlhgat.hodge_dataset import halo_tiles
    from hlhgat.synthetic import tsp_like_graph
    g = tsp_like_graph(3, n=600, k=6, halo=False)
    ei, w, n, order = g.edge_index_s, g.edge_weight_s, g.x_s.shape[0], g.row_order_s
    mask = dev(rand_mask(n, 0.3, seed=4))
    wd = dev(w)
    ei_p = ops.set_row_mask(ops.set_row_order(ops.mark_hodge(dev(ei)), order), mask)
    ei_h = ops.set_row_mask(ops.set_row_order(ops.mark_hodge(dev(ei)), order), mask)
    ops.set_halo(ei_h, halo_tiles(ei.numpy(), n, order.numpy(), max_rows=7, max_halo=48))
    plain, halo = ops.hodge_operator(ei_p, wd, n), ops.hodge_operator(ei_h, wd, n)
    assert plain.fwd.halo is None and halo.fwd.halo is not None
    base = halo.masked_from[0]
    assert halo.fwd.halo[5].data_ptr() != base.fwd.halo[5].data_ptr()
    assert torch.equal(base.fwd.halo[5], wd[ei_h._hlhgat_halo[5].long()])
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(d))
    y0, y1 = ops.spmm(plain.fwd, dev(x)), ops.spmm(halo.fwd, dev(x))
    assert torch.equal(y0, y1)
    assert torch.equal(y1.cpu(), R.propagate(x, *filtered(ei, w, mask.cpu())[:2]))
    for kind in (ops.POLY_LAGUERRE, ops.POLY_CHEB, ops.POLY_LAGUERRE_DEMO):
        assert torch.equal(ops.poly_basis(plain, dev(x), 4, kind),
                           ops.poly_basis(halo, dev(x), 4, kind))
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: the head against the reference's augmented run
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("factored", [False, True])
def test_tsp_head_with_row_mask_vs_reference_golden(cuda, factored):
    """set_row_mask with the reference's own node_mask on the UNFILTERED L1 and
    the mask column in x_s against the reference's forward / backward on the
    filtered COO: out and every gradient within 1e-4 relative."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.hodge_dataset import Batch, hodge_factor_ok
    g = load_golden("tsp_aug_small")
    m = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(**HEAD_KW)
    m.load_state_dict({k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")})
    m = m.to(cuda).train()
    b = Batch()
    for k in BATCH_KEYS:
        setattr(b, k, dev(g[k]))
    ops.mark_hodge(b.edge_index_s)
    if factored:
        assert hodge_factor_ok(g["edge_index"], g["x_t"].shape[0], g["edge_index_s"],
                               g["edge_weight_s"])
        ops.set_hodge_factor(b.edge_index_s, b.edge_index, b.x_t.shape[0])
    ops.set_row_mask(b.edge_index_s, dev(g["mask"]))
    out, s_batch = m(b)
    op = ops.hodge_operator(b.edge_index_s, b.edge_weight_s, b.x_s.shape[0])
    assert op.masked_from is not None and (op.factor is not None) == factored
    assert torch.equal(s_batch.cpu(), T(g["s_batch"]))
    close(out.detach().cpu(), g["out"], 1e-4, "out")
    (out * dev(g["R"])).sum().backward()
    _check_head_grads(((k, p.grad) for k, p in m.named_parameters()), g)
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: the augmentation under TrainStep
# ---------------------------------------------------------------------------
AUG = dict(aug_prob=0.75, p=0.2, jitter=0.5)


def _aug_head(cuda, sd=None, augment=True):
    import hlhgat
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(**HEAD_KW)
    if sd is not None:
        m.load_state_dict(sd)
    if augment:
        m.augment = hlhgat.nn.SimplexDropout(**AUG)
    return m.to(cuda).train()


def _bce(o, d):
    return torch.nn.functional.binary_cross_entropy_with_logits(o[0].view(-1), d.y.view(-1))


def _expected_mask(b, step):
    return S.keep(b.seg_ptr_s.cpu().numpy(), b.x_s.shape[0], AUG["aug_prob"], AUG["p"],
                  AUG["jitter"], SEED, step, protect=b.y.cpu().numpy())


@pytest.mark.gpu
def test_trainstep_replays_draw_fresh_masks(cuda, monkeypatch):
    from hlhgat import ops, train
    monkeypatch.setattr(train, "KEEP_GRAPHS", True)
    sd = {k: v.clone() for k, v in _aug_head("cpu", augment=False).state_dict().items()}
    losses, masks = {}, []
    for graphs in (True, False):
        m = _aug_head(cuda, sd)
        b = _two_graph_batch(cuda)
        ops.dropout_manual_seed(SEED, cuda)
        st = train.TrainStep(m, _bce, lr=1e-3, graphs=graphs)
        losses[graphs] = []
        for i in range(3):
            losses[graphs].append(st(b).detach().clone())
            torch.cuda.synchronize()
            if graphs:
                src = b if i == 0 else next(iter(st._graphs.values())).batch
                mk = m.augment.mask_of(src).cpu().numpy()
                assert np.array_equal(mk, _expected_mask(b, i + 1)), i
                assert np.array_equal(src.x_s[:, 1].cpu().numpy(), mk)
                assert (mk[b.y.cpu().numpy() != 0] == 1).all()
                masks.append(mk)
        assert ops.dropout_state(cuda)[1] == 3  # one advance per step, replays included
        if graphs:
            assert st.stats["captures"] == 1 and st.stats["replay"] == 2
            assert not any(np.array_equal(masks[i], masks[j]) for i in range(3) for j in range(i))
            # resume: the saved counter continues the stream
            ck = copy.deepcopy(st.state_dict())  # a snapshot: state_dict shares storage
            assert ck["dropout"] == (SEED, 3)
            l4 = st(b).detach().clone()
            ent = next(iter(st._graphs.values()))
            m4 = m.augment.mask_of(ent.batch).clone()
            assert np.array_equal(m4.cpu().numpy(), _expected_mask(b, 4))
            ops.dropout_manual_seed(99, cuda)
            st.load_state_dict(ck)
            assert torch.equal(st(b), l4)
            assert torch.equal(m.augment.mask_of(ent.batch), m4)
            h = ent.graph.raw_cuda_graph()
            n_keep = ops.graph_kernel_count(h, "k_simplex_keep")[1]
            n_csr = ops.graph_kernel_count(h, "k_mask_csr_values")[1]
            n_fac = ops.graph_kernel_count(h, "k_mask_hodge_factor")[1]
            print("captured simplex kernels: draw", n_keep, "csr", n_csr, "factor", n_fac)
            assert n_keep == 1 and n_csr == 1 and n_fac <= 1
            assert ops.graph_kernel_count(h, "k_dropout_advance")[1] == 1
    for a, c in zip(losses[True], losses[False]):
        assert torch.equal(a, c), (losses[True], losses[False])
    ops.check_device_errors()


@pytest.mark.gpu
def test_eval_mode_runs_the_unmasked_operator(cuda):
    from hlhgat import ops
    sd = {k: v.clone() for k, v in _aug_head("cpu", augment=False).state_dict().items()}
    m, twin = _aug_head(cuda, sd), _aug_head(cuda, sd, augment=False)
    b = _two_graph_batch(cuda)
    n = b.x_s.shape[0]
    ops.dropout_set_state(SEED, 1, cuda)
    ops.clear_caches()
    m(b)[0].sum().backward()
    op = ops.hodge_operator(b.edge_index_s, b.edge_weight_s, n)
    assert op.masked_from is not None
    assert np.array_equal(b.x_s[:, 1].cpu().numpy(), _expected_mask(b, 1))
    twin.load_state_dict(m.state_dict())  # the running statistics of m's training forward
    m.eval()
    twin.eval()
    x_s = b.x_s.clone()
    ops.clear_caches()
    with torch.no_grad():
        out = m(b)[0]
        assert ops.hodge_operator(b.edge_index_s, b.edge_weight_s, n).masked_from is None
        assert torch.equal(b.x_s, x_s)
        b2 = _two_graph_batch(cuda)
        b2.x_s.copy_(x_s)
        ops.clear_caches()
        assert torch.equal(out, twin(b2)[0])
    ops.clear_caches()
    ops.check_device_errors()
