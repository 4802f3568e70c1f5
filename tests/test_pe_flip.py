"""PE sign-flip augmentation: the draw (csrc/peflip.hip)
against its numpy restatement (peflip_ref.py), the heads' ``pe_flip`` slot
against the same heads on host-flipped batches, and the augmentation under
TrainStep.

Tolerances, per assertion:
  * the draw, the flip, its backward, module vs host-flipped batch, graph
    replay vs eager vs the per-step host emulation: bit for bit;
  * padded vs unpadded batches: test_train_step.py's padding tolerances
    (outputs rtol 1e-5 / atol 1e-6, gradients 1e-4 of their max);
  * the statistics of the restatement: 4 sigma of a fair coin at the sample
    sizes used (65536 signs: 0.0078; 4096 per column: 0.031; correlation of
    two columns of 4096: 0.0625).
"""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import peflip_ref as P
from conftest import REPO

T = torch.from_numpy
SEED = 1234
ZINC_KW = dict(channels=[1, 1], filters=[32, 32], mlp_channels=[64], K=3, keig=15)
PEP_KW = dict(channels=[1, 1], filters=[16, 32], mlp_channels=[32], K=3, pool_loc=0)


# ---------------------------------------------------------------------------
# CPU: the restatement
# ---------------------------------------------------------------------------
def test_ref_sign_statistics():
    """4096 graphs x 16 columns at seed 1234: a fair, column-wise independent
    coin that changes with the step and with the site."""
    G, C = 4096, 16
    tabs = {(step, k, side): P.signs(G, C, SEED, step, k, side)
            for step in (1, 2) for k in (0, 1) for side in (0, 1)}
    for key, s in tabs.items():
        assert set(np.unique(s)) == {-1.0, 1.0}
        neg = s < 0
        share, cols = neg.mean(), neg.mean(axis=0)
        corr = np.corrcoef(s.astype(np.float64), rowvar=False)
        off = np.abs(corr - np.eye(C)).max()
        print(key, "share", share, "columns", cols.min(), cols.max(), "max |corr|", off)
        assert abs(share - 0.5) <= 0.0078
        assert np.abs(cols - 0.5).max() <= 0.031
        assert off <= 0.0625
    keys = list(tabs)
    for i, a in enumerate(keys):
        for b in keys[:i]:
            differ = (tabs[a] != tabs[b]).mean()
            print(a, b, "differ", differ)
            assert abs(differ - 0.5) <= 0.0078, (a, b)


def test_ref_flip_semantics():
    seg, n = [0, 2, 2, 5], 7  # an empty graph, two padding rows
    x = np.arange(n * 6, dtype=np.float32).reshape(n, 6) + 1
    y = P.flip(x, seg, 2, 3, SEED, 1)
    s = P.signs(3, 3, SEED, 1)
    assert y.shape == (n, 5)
    assert np.array_equal(y[:, :2], x[:, :2])
    assert np.array_equal(y[:2, 2:], x[:2, 2:5] * s[0])
    assert np.array_equal(y[2:5, 2:], x[2:5, 2:5] * s[2])
    assert np.array_equal(y[5:], x[5:, :5])
    assert np.array_equal(P.row_graph(seg, n), [0, 0, 2, 2, 2, -1, -1])
    # a group of four columns shares one Philox call: the table's prefix is stable
    assert np.array_equal(P.signs(3, 7, SEED, 1)[:, :3], s)


def test_module_constructor_and_cpu_behaviour():
    import hlhgat
    F = hlhgat.nn.PESignFlip
    for bad in (dict(node_dim=-1, edge_dim=3), dict(node_dim=21, edge_dim=-3),
                dict(node_dim=21, edge_dim=3, keig=-1), dict(node_dim=21, edge_dim=3, site=-1),
                dict(node_dim=21, edge_dim=3, site=1 << 29),
                dict(node_dim=65537, edge_dim=3), dict(node_dim=21, edge_dim=3, keig=65536)):
        with pytest.raises(ValueError):
            F(**bad)
    m = F(21, 3, 7, site=(1 << 29) - 1)
    assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
    x_t, x_s = torch.randn(5, 28), torch.randn(4, 10)
    m.eval()
    y_t, y_s = m(x_t, x_s, None)
    assert y_t is x_t and y_s is x_s
    m.train()
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(x_t, x_s, None)
    from hlhgat import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.pe_flip(x_t, torch.zeros(2, dtype=torch.int32), 21, 7)
    with pytest.raises(ValueError):
        ops.pe_flip(None, None, 0, 0, site=1 << 29)


def test_symbols_declared_and_exported():
    import torch  # noqa: F401,F811
    from hlhgat import _lib
    lib = ctypes.CDLL(os.path.join(REPO, "hl-hgat_amd", "hlhgat", "libhlhgat.so"))
    for s in ("hlhgat_pe_flip", "hlhgat_pe_signs"):
        assert s in _lib.SIGNATURES
        assert hasattr(lib, s)


def test_capi_argument_errors():
    """Argument validation runs before any HIP call; empty input is a no-op."""
    import torch  # noqa: F401,F811
    from hlhgat import _lib
    L = _lib.LIB
    buf = ctypes.create_string_buffer(96)
    p = ctypes.addressof(buf)  # non-NULL pointers that are never dereferenced
    p += -p % 16
    q = p + 32

    def err(rc, text):
        assert rc == 1
        assert text.encode() in L.hlhgat_last_error(), L.hlhgat_last_error()

    def side(**kw):
        d = dict(x=p, ldx=8, y=q, ldy=8, seg_ptr=p, n_graphs=1, n_rows=4, n_fixed=3, n_flip=5,
                 site=0)
        d.update(kw)
        return _lib.PeSideDesc(*[d[k] for k, _ in _lib.PeSideDesc._fields_])

    def flip(sides, n=None, state=p, snap=q):
        arr = (_lib.PeSideDesc * max(len(sides), 1))(*sides)
        return L.hlhgat_pe_flip(ctypes.cast(arr, ctypes.c_void_p), len(sides) if n is None else n,
                                state, snap, None)

    err(flip([side()], n=0), "n_sides")
    err(flip([side()], n=3), "n_sides")
    err(L.hlhgat_pe_flip(None, 1, p, q, None), "NULL pointer")
    for kw in (dict(n_rows=-1), dict(n_graphs=-1), dict(n_fixed=-1), dict(n_flip=-1),
               dict(n_fixed=65536, n_flip=1, ldx=1 << 20, ldy=1 << 20)):
        err(flip([side(**kw)]), "bad sizes")
        err(flip([side(), side(**kw)]), "on side 1")
    err(flip([side(ldx=7)]), "leading dimension")
    err(flip([side(ldy=7)]), "leading dimension")
    err(flip([side(site=1 << 30)]), "site")
    err(flip([side(x=None)]), "NULL pointer")
    err(flip([side(y=None)]), "NULL pointer")
    err(flip([side(seg_ptr=None)]), "NULL pointer")
    err(flip([side(y=p)]), "alias")
    err(flip([side()], state=None), "NULL pointer")
    err(flip([side()], snap=None), "NULL pointer")
    err(flip([side()], state=p + 4), "8-byte aligned")
    # nothing to move: no launch, pointers never looked at
    assert flip([side(n_rows=0, x=None, y=None, seg_ptr=None)], state=None, snap=None) == 0
    assert flip([side(n_fixed=0, n_flip=0, x=None, y=None), side(n_rows=0)], state=None,
                snap=None) == 0

    sg = L.hlhgat_pe_signs
    err(sg(-1, 4, 0, p, q, None), "bad sizes")
    err(sg(4, -1, 0, p, q, None), "bad sizes")
    err(sg(4, 65537, 0, p, q, None), "bad sizes")
    err(sg(4, 4, 1 << 30, p, q, None), "site")
    err(sg(4, 4, 0, None, q, None), "NULL pointer")
    err(sg(4, 4, 0, p, None, None), "NULL pointer")
    assert sg(0, 4, 0, None, None, None) == 0
    assert sg(4, 0, 0, None, None, None) == 0


def test_heads_carry_an_empty_slot():
    import hlhgat
    heads = [hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**ZINC_KW),
             hlhgat.HL_HGCNN_zinc_dense_poolint3_pyr(**ZINC_KW),
             hlhgat.HL_HGCNN_pepfunc_dense_int3_attpool(**PEP_KW)]
    for m in heads:
        assert m.pe_flip is None
        keys = set(m.state_dict())
        m.pe_flip = hlhgat.nn.PESignFlip(9, 3, 20)
        assert set(m.state_dict()) == keys
        assert "pe_flip" in dict(m.named_children())
    tsp = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(channels=[1], filters=[16], K=2)
    assert not hasattr(tsp, "pe_flip")  # TSP_EigPE.get keeps no PE column


# ---------------------------------------------------------------------------
# GPU: the kernel against the restatement
# ---------------------------------------------------------------------------
def _seg(G, seed):
    """Row pointer of G graphs: empty graphs, one-row graphs and one run of
    more than 1000 rows (several workgroups of 32 rows)."""
    rng = np.random.default_rng(seed)
    if G == 1:
        sizes = [1037]
    elif G == 3:
        sizes = [0, 1, 1100]
    else:
        sizes = rng.integers(0, 6, G)
        sizes[[0, 7, G - 1]] = 0
        sizes[[1, 100]] = 1
        sizes[130] = 1003
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


class _Side:
    """One side of a raw hlhgat_pe_flip call: x the [:, 1:] window of a
    NaN-filled slab and wider than the output, y a window of a NaN-filled slab."""

    def __init__(self, cuda, G, pad, n_fixed, n_flip, word, seed, extra=2):
        self.seg = _seg(G, seed)
        self.n = int(self.seg[-1]) + pad
        self.n_fixed, self.n_flip, self.word = n_fixed, n_flip, word
        w = n_fixed + n_flip
        g = torch.Generator().manual_seed(seed)
        xh = torch.randn(self.n, w + extra, generator=g)
        xh[torch.rand(self.n, w + extra, generator=g) < 0.1] = 0.0  # zeros flip to -0.0
        self.x_host = xh.numpy()
        slab = torch.full((self.n, 1 + w + extra), float("nan"))
        slab[:, 1:] = xh
        self.slab = slab.to(cuda)
        self.x = self.slab[:, 1:]
        self.yslab = torch.full((self.n + 1, w + 3), float("nan"), device=cuda)
        self.y = self.yslab[:self.n, 2:2 + w]
        self.segd = T(self.seg).to(cuda)

    def desc(self):
        from hlhgat import _lib
        return _lib.PeSideDesc(self.x.data_ptr(), self.x.stride(0), self.y.data_ptr(),
                               self.y.stride(0), self.segd.data_ptr(), self.seg.size - 1, self.n,
                               self.n_fixed, self.n_flip, self.word)

    def check(self, seed, step):
        k, side = self.word // 2, self.word % 2
        exp = P.flip(self.x_host, self.seg, self.n_fixed, self.n_flip, seed, step, k, side)
        got = self.yslab.cpu().numpy()
        w = self.n_fixed + self.n_flip
        assert np.array_equal(got[:self.n, 2:2 + w].view(np.uint32), exp.view(np.uint32))
        outside = np.ones(got.shape, bool)
        outside[:self.n, 2:2 + w] = False
        assert np.isnan(got[outside]).all()  # bytes outside y are untouched
        real = int(self.seg[-1])
        assert np.array_equal(got[real:self.n, 2:2 + w].view(np.uint32),
                              self.x_host[real:, :w].view(np.uint32))  # padding rows: a copy
        assert torch.isnan(self.slab[:, 0]).all()


def _raw_flip(sides, state, snap):
    from hlhgat import _lib
    arr = (_lib.PeSideDesc * len(sides))(*[s.desc() for s in sides])
    _lib.check(_lib.LIB.hlhgat_pe_flip(ctypes.cast(arr, ctypes.c_void_p), len(sides),
                                       state.data_ptr(), snap.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "pe_flip")


WIDTHS = [(0, 1), (21, 15), (3, 5), (1, 4), (9, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("G,pad", [(1, 5), (3, 64), (257, 5), (257, 64)])
@pytest.mark.parametrize("wi", range(len(WIDTHS)))
def test_kernel_bitwise(cuda, wi, G, pad):
    """Both sides in one launch (side t: the case's widths at site word 6;
    side s: the next widths, another graph count, word 7), then side t alone
    from the snapshot after the live state moved on."""
    from hlhgat import ops
    step = 7 + wi
    ops.dropout_set_state(SEED, step, cuda)
    st = ops._dropout_st(cuda).dev
    a = _Side(cuda, G, pad, *WIDTHS[wi], word=6, seed=10 * wi + G)
    b = _Side(cuda, {1: 3, 3: 257, 257: 1}[G], 69 - pad, *WIDTHS[(wi + 1) % len(WIDTHS)], word=7,
              seed=10 * wi + G + 1)
    snap = torch.zeros(2, dtype=torch.int64, device=cuda)
    _raw_flip([a, b], st, snap)
    a.check(SEED, step)
    b.check(SEED, step)
    assert snap.tolist() == [SEED, step]
    assert ops.dropout_state(cuda)[:2] == (SEED, step)  # the draw advances nothing
    # one side only, replayed from the snapshot (snap == state)
    ops.dropout_advance(cuda)
    a.yslab.fill_(float("nan"))
    _raw_flip([a], snap, snap)
    a.check(SEED, step)
    assert snap.tolist() == [SEED, step]
    # and at the live state: other signs
    a.yslab.fill_(float("nan"))
    _raw_flip([a], st, snap)
    a.check(SEED, step + 1)
    assert snap.tolist() == [SEED, step + 1]
    ops.check_device_errors()


@pytest.mark.gpu
def test_pe_signs_equals_restatement(cuda):
    from hlhgat import ops
    ops.dropout_set_state(SEED, 3, cuda)
    for G, n_flip, k, side in ((1, 1, 0, 0), (3, 5, 2, 1), (257, 15, 0, 1), (4096, 16, 1, 0),
                               (5, 37, (1 << 29) - 1, 1)):
        got = ops.pe_signs(G, n_flip, site=k, side=side, device=cuda)
        assert np.array_equal(got.cpu().numpy(), P.signs(G, n_flip, SEED, 3, k, side))
    seg = T(_seg(257, 0)).to(cuda)
    assert torch.equal(ops.pe_signs(seg, 15, site=4), ops.pe_signs(257, 15, site=4, device=cuda))
    assert ops.pe_signs(0, 4, device=cuda).shape == (0, 4)
    assert ops.pe_signs(4, 0, device=cuda).shape == (4, 0)
    ops.check_device_errors()


@pytest.mark.gpu
def test_op_forward_and_backward_bitwise(cuda):
    """ops.pe_flip: y == x_host * signs[g(row)]; dx == dy * signs from the
    snapshot after the live state advanced; dropped columns and the window's
    neighbour column get zero gradient; one side at a time."""
    from hlhgat import ops
    seg_t, seg_s = _seg(257, 1), _seg(3, 2)
    n_t, n_s = int(seg_t[-1]) + 5, int(seg_s[-1]) + 64
    g = torch.Generator().manual_seed(0)
    slab = torch.randn(n_t, 1 + 21 + 15 + 2, generator=g).to(cuda).requires_grad_(True)
    x_s = torch.randn(n_s, 3 + 5, generator=g).to(cuda).requires_grad_(True)
    st, ss = T(seg_t).to(cuda), T(seg_s).to(cuda)
    ops.dropout_set_state(SEED, 11, cuda)
    x_t = slab[:, 1:]
    v_t, v_s = slab._version, x_s._version
    y_t, y_s = ops.pe_flip(x_t, st, 21, 15, x_s, ss, 3, 5, site=3)
    exp_t = P.flip(slab.detach().cpu().numpy()[:, 1:], seg_t, 21, 15, SEED, 11, k=3, side=0)
    exp_s = P.flip(x_s.detach().cpu().numpy(), seg_s, 3, 5, SEED, 11, k=3, side=1)
    assert np.array_equal(y_t.detach().cpu().numpy().view(np.uint32), exp_t.view(np.uint32))
    assert np.array_equal(y_s.detach().cpu().numpy().view(np.uint32), exp_s.view(np.uint32))
    assert (slab._version, x_s._version) == (v_t, v_s)
    assert y_t.data_ptr() != slab.data_ptr() and y_s.data_ptr() != x_s.data_ptr()
    # signs as a table: the same statement through ops.pe_signs
    sg = ops.pe_signs(st, 15, site=3, side=0).cpu().numpy()
    rows = P.row_graph(seg_t, n_t)
    real = rows >= 0
    xh = slab.detach().cpu().numpy()[:, 1:]
    assert np.array_equal((xh[real, 21:36] * sg[rows[real]]).view(np.uint32),
                          exp_t[real, 21:].view(np.uint32))
    ops.dropout_advance(cuda)  # the backward must not read the live state
    dy_t = torch.randn(y_t.shape, generator=g).to(cuda)
    dy_s = torch.randn(y_s.shape, generator=g).to(cuda)
    torch.autograd.backward([y_t, y_s], [dy_t, dy_s])
    gs = slab.grad.cpu().numpy()
    assert (gs[:, 0] == 0).all() and (gs[:, 37:] == 0).all()
    exp = P.flip(dy_t.cpu().numpy(), seg_t, 21, 15, SEED, 11, k=3, side=0)
    assert np.array_equal(gs[:, 1:37].view(np.uint32), exp.view(np.uint32))
    exp = P.flip(dy_s.cpu().numpy(), seg_s, 3, 5, SEED, 11, k=3, side=1)
    assert np.array_equal(x_s.grad.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    # one side only, either one; no grad required: no autograd node needed
    only_t, none = ops.pe_flip(x_t.detach(), st, 21, 15, site=3)
    assert none is None and not only_t.requires_grad
    none, only_s = ops.pe_flip(None, None, 0, 0, x_s.detach(), ss, 3, 5, site=3)
    assert none is None
    assert np.array_equal(only_s.cpu().numpy(),
                          P.flip(x_s.detach().cpu().numpy(), seg_s, 3, 5, SEED, 12, k=3, side=1))
    assert np.array_equal(only_t.cpu().numpy(),
                          P.flip(xh, seg_t, 21, 15, SEED, 12, k=3, side=0))
    with pytest.raises(RuntimeError, match="fewer than"):
        ops.pe_flip(x_s.detach(), ss, 3, 6)
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: the heads
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _raw(kind):
    from hlhgat.synthetic import two_level_batch, zinc_like_batch
    if kind == "zinc":
        return zinc_like_batch(7, seed=21)
    return two_level_batch("peptides", 5, seed=3)


def _case(kind):
    """(host batch, model factory, module factory, loss, fine-level accessor)."""
    import hlhgat
    F = torch.nn.functional
    if kind == "zinc":
        return (_raw(kind), lambda: hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**ZINC_KW),
                lambda: hlhgat.nn.PESignFlip(21, 3, 15),
                lambda o, d: F.l1_loss(o.view(-1), d.y.view(-1)))
    return (_raw(kind), lambda: hlhgat.HL_HGCNN_pepfunc_dense_int3_attpool(**PEP_KW),
            lambda: hlhgat.nn.PESignFlip(9, 3, 20),
            lambda o, d: F.binary_cross_entropy_with_logits(o, d[0].y.view(o.shape).float()))


def _fine(b):
    return b[0] if isinstance(b, list) else b


def _to(b, dev):
    """A copy of the host batch (list) on dev; Batch.to moves in place, and the
    host batches are shared between the tests."""
    return [copy.copy(x).to(dev) for x in b] if isinstance(b, list) else copy.copy(b).to(dev)


def _with_features(b, x_t, x_s):
    """A shallow copy of the batch (list) with the fine level's features replaced."""
    f = copy.copy(_fine(b))
    f.x_t, f.x_s = x_t, x_s
    return [f] + list(b[1:]) if isinstance(b, list) else f


def _host_flipped(kind, b, sign_t, sign_s):
    """The batch with its PE columns multiplied by per-graph sign tables
    ([G, keig] numpy) on the host; b stays as it is."""
    f = _fine(b)
    off = 1 if kind == "peptides" else 0  # the cluster column of the attpool levels
    out = []
    for x, seg, fixed, sg in ((f.x_t, f.seg_ptr_t, 21 if kind == "zinc" else 9, sign_t),
                              (f.x_s, f.seg_ptr_s, 3, sign_s)):
        xh = x.detach().cpu().numpy().copy()
        rows = P.row_graph(seg.cpu().numpy(), xh.shape[0])
        real = rows >= 0
        c0 = off + fixed
        xh[real, c0:c0 + sg.shape[1]] = xh[real, c0:c0 + sg.shape[1]] * sg[rows[real]]
        out.append(T(xh).to(x.device))
    return _with_features(b, *out)


def _model(kind, cuda, flip, sd=None):
    _, mk, mk_flip, _ = _case(kind)
    torch.manual_seed(0)
    m = mk()
    if sd is not None:
        m.load_state_dict(sd)
    if flip:
        m.pe_flip = mk_flip()
    return m.to(cuda).train()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "peptides"])
def test_head_with_module_equals_host_flipped_batch(cuda, kind):
    from hlhgat import ops
    raw, _, _, _ = _case(kind)
    b = _to(raw, cuda)
    f = _fine(b)
    keig = 15 if kind == "zinc" else 20
    m, twin = _model(kind, cuda, True), _model(kind, cuda, False)
    ops.dropout_set_state(SEED, 5, cuda)
    sg_t = ops.pe_signs(f.seg_ptr_t, keig, side=0).cpu().numpy()
    sg_s = ops.pe_signs(f.seg_ptr_s, keig, side=1).cpu().numpy()
    assert np.array_equal(sg_t, P.signs(sg_t.shape[0], keig, SEED, 5, 0, 0))
    assert (sg_t < 0).any() and (sg_s < 0).any() and (sg_t > 0).any()
    keep = (f.x_t.clone(), f.x_s.clone(), f.x_t._version, f.x_s._version)
    out = m(b)
    # the caller's batch is not modified
    assert (f.x_t._version, f.x_s._version) == keep[2:]
    assert torch.equal(f.x_t, keep[0]) and torch.equal(f.x_s, keep[1])
    exp = twin(_host_flipped(kind, b, sg_t, sg_s))
    assert torch.equal(out, exp)
    assert not torch.equal(out, _model(kind, cuda, False)(b))  # the flip is not a no-op
    # eval: the stored signs, bit for bit the module-less model (same statistics)
    twin.load_state_dict(m.state_dict())
    m.eval()
    twin.eval()
    with torch.no_grad():
        assert torch.equal(m(b), twin(b))
    ops.check_device_errors()


def _pad(kind, raw):
    from hlhgat.hodge_dataset import level_caps, pad_batch, pad_levels, static_caps
    if kind == "zinc":
        return pad_batch(raw, static_caps(raw, 256))
    return pad_levels(raw, level_caps([raw], 128))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "peptides"])
def test_padded_batch_with_module_matches_unpadded(cuda, kind):
    """pad_batch / pad_levels batches: the padding rows lie beyond seg_ptr[-1]
    and are copied; real rows and every parameter gradient are the unpadded
    batch's at test_train_step.py's padding tolerances."""
    from hlhgat import ops
    raw, _, _, loss = _case(kind)
    padded = _pad(kind, raw)
    assert _fine(padded).x_t.size(0) > _fine(raw).x_t.size(0)
    res = []
    for batch in (raw, padded):
        m = _model(kind, cuda, True)
        d = _to(batch, cuda)
        ops.dropout_set_state(SEED, 5, cuda)
        out = m(d)
        loss(out, d).backward()
        res.append((out.detach().cpu(), {k: p.grad.detach().cpu().clone()
                                         for k, p in m.named_parameters() if p.grad is not None}))
    (o0, g0), (o1, g1) = res
    assert torch.allclose(o0, o1, rtol=1e-5, atol=1e-6), (o0 - o1).abs().max()
    assert set(g0) == set(g1)
    for k in g0:
        scale = g0[k].abs().max().clamp_min(1e-6)
        assert ((g0[k] - g1[k]).abs().max() / scale) < 1e-4, k
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: under TrainStep
# ---------------------------------------------------------------------------
def _params(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "peptides"])
def test_trainstep_replays_draw_fresh_signs(cuda, kind, monkeypatch):
    """Three replayed steps == three eager steps == three module-less eager
    steps on batches flipped on the host by the restatement at (seed, step_s):
    losses and parameters, bit for bit.  One pe_flip kernel in the captured
    step, none without the module."""
    from hlhgat import ops, train
    monkeypatch.setattr(train, "KEEP_GRAPHS", True)
    raw, _, _, loss = _case(kind)
    keig = 15 if kind == "zinc" else 20
    sd = {k: v.clone() for k, v in _model(kind, "cpu", False).state_dict().items()}
    runs = {}
    for mode in ("graphs", "eager", "emulated", "plain-graphs"):
        flip = mode in ("graphs", "eager")
        m = _model(kind, cuda, flip, sd)
        b = _to(raw, cuda)
        ops.dropout_manual_seed(SEED, cuda)
        st = train.TrainStep(m, loss, lr=1e-3, graphs=mode.endswith("graphs"))
        losses = []
        for i in range(3):
            d = b
            if mode == "emulated":
                G = _fine(b).seg_ptr_t.numel() - 1
                d = _host_flipped(kind, b, P.signs(G, keig, SEED, i + 1, 0, 0),
                                  P.signs(G, keig, SEED, i + 1, 0, 1))
            losses.append(st(d).detach().clone())
        torch.cuda.synchronize()
        runs[mode] = (losses, _params(m))
        if flip:
            assert ops.dropout_state(cuda)[:2] == (SEED, 3)  # one advance per step
        if mode.endswith("graphs"):
            assert st.stats["captures"] == 1 and st.stats["replay"] == 2, st.stats
            h = next(iter(st._graphs.values())).graph.raw_cuda_graph()
            n_flip = ops.graph_kernel_count(h, "pe_flip")[1]
            print(mode, "captured pe_flip kernels", n_flip)
            assert n_flip == (1 if flip else 0)
            assert ops.graph_kernel_count(h, "k_dropout_advance")[1] == (1 if flip else 0)
    ref_l, ref_p = runs["graphs"]
    assert not torch.equal(ref_l[0], runs["plain-graphs"][0][0])
    for mode in ("eager", "emulated"):
        ls, ps = runs[mode]
        for a, c in zip(ref_l, ls):
            assert torch.equal(a, c), (mode, ref_l, ls)
        for k in ref_p:
            assert torch.equal(ref_p[k], ps[k]), (mode, k)
    ops.check_device_errors()


@pytest.mark.gpu
def test_trainstep_checkpoint_continues_bitwise(cuda):
    from hlhgat import ops, train
    kind = "zinc"
    raw, _, _, loss = _case(kind)
    sd = {k: v.clone() for k, v in _model(kind, "cpu", False).state_dict().items()}
    b = _to(raw, cuda)
    m = _model(kind, cuda, True, sd)
    ops.dropout_manual_seed(SEED, cuda)
    st = train.TrainStep(m, loss, lr=1e-3, graphs=False)
    for _ in range(2):
        st(b)
    ck = copy.deepcopy(st.state_dict())
    assert ck["dropout"] == (SEED, 2)
    l3 = st(b).detach().clone()
    p3 = _params(m)
    m2 = _model(kind, cuda, True, sd)
    ops.dropout_manual_seed(99, cuda)
    st2 = train.TrainStep(m2, loss, lr=1e-3, graphs=False)
    st2.load_state_dict(ck)
    assert torch.equal(st2(b).detach(), l3)
    p2 = _params(m2)
    for k in p3:
        assert torch.equal(p3[k], p2[k]), k
    ops.check_device_errors()
