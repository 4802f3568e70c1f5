"""Training-mode Dropout on the HIP path (csrc/dropout.hip, ops.dropout).

CPU: the numpy restatement of the mask rule (tests/dropout_ref.py) reproduces
the published Philox4x32-10 known answers and keeps at the stated rate; the
C-ABI validates its arguments; CPU tensors still go to torch.
GPU: mask, values and gradient are bitwise dropout_ref's for every layout; the
mask of a backward is its forward's; a captured step draws fresh masks on
every replay; the HL blocks and the dense heads route their live Dropout
through it (into the slab column block, no copy)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as tnn

import dropout_ref as R
from conftest import close

PS = [0.25, 0.5, 0.9]


# ---------------------------------------------------------------------------
# CPU: the reference mask
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    got = tuple(int(w[0]) for w in R.philox(ctr, key))
    assert got == want, [hex(g) for g in got]


@pytest.mark.parametrize("p", PS)
def test_reference_keep_rates(p):
    """Overall, per-column and per-row keep rates within 6 binomial sigma of
    1 - p (fixed inputs: deterministic; worst case seen 4.7 sigma)."""
    n, d = 4096, 256
    q = 1.0 - R.threshold(p) / 16777216.0
    assert abs(q - (1 - p)) < 2.0 ** -24
    for site in range(4):
        m = R.keep(n, d, p, 1234, 7, site)
        assert m.shape == (n, d) and m.dtype == bool

        def sig(cnt):
            return math.sqrt(p * (1 - p) / cnt)

        assert abs(m.mean() - (1 - p)) <= 6 * sig(n * d)
        assert np.abs(m.mean(axis=0) - (1 - p)).max() <= 6 * sig(n)
        assert np.abs(m.mean(axis=1) - (1 - p)).max() <= 6 * sig(d)


def test_reference_sites_and_steps_are_independent():
    """Masks of two sites, or of two steps, agree on ~p^2 + (1-p)^2 = 0.625 of
    the entries at p = 0.25 (not on all of them)."""
    a = R.keep(64, 64, 0.25, 1234, 7, 0)
    for other in (R.keep(64, 64, 0.25, 1234, 7, 1), R.keep(64, 64, 0.25, 1234, 8, 0),
                  R.keep(64, 64, 0.25, 1235, 7, 0)):
        agree = (a == other).mean()
        assert 0.55 < agree < 0.7, agree
    assert np.array_equal(a, R.keep(64, 64, 0.25, 1234, 7, 0))
    assert np.array_equal(a, R.keep(64, 64, 0.25, 1234, 7 + (1 << 32), 0))  # step mod 2^32


def test_reference_apply_edges():
    x = np.arange(-6, 6, dtype=np.float32).reshape(3, 4)
    assert np.array_equal(R.apply(x, 1.0, 1, 0, 0), np.zeros_like(x))
    y = R.apply(x, 0.5, 1, 0, 0)
    m = R.keep(3, 4, 0.5, 1, 0, 0)
    assert np.array_equal(y, np.where(m, x * np.float32(2.0), np.float32(0)))


def test_rank_seed():
    from hlhgat import ops
    seeds = [ops.dropout_rank_seed(1234, r) for r in range(8)]
    assert len(set(seeds)) == 8
    assert seeds[0] == 1234
    assert ops.dropout_rank_seed(2 ** 64 - 1, 1) == (2 ** 64 - 1 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert all(0 <= s < 2 ** 64 for s in seeds)
    assert ops.dropout_rank_seed(5, 3) == (5 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64


def test_capi_argument_errors():
    """Validation runs before any HIP call (the error-path style of
    tests/test_capi.py): ld < d, a null pointer, T > 2^24."""
    import ctypes
    from hlhgat import _lib
    L = _lib.LIB
    buf = (ctypes.c_int64 * 64)()
    a = ctypes.addressof(buf)
    T = R.threshold(0.25)
    assert L.hlhgat_dropout_fwd(a, 4, 3, 5, T, 1.0, a, 0, a, a, 5, None) == 1  # ldx < d
    assert b"dropout_fwd" in L.hlhgat_last_error()
    assert L.hlhgat_dropout_fwd(a, 5, 3, 5, T, 1.0, a, 0, a, a, 4, None) == 1  # ldy < d
    assert L.hlhgat_dropout_fwd(None, 5, 3, 5, T, 1.0, a, 0, a, a, 5, None) == 1
    assert b"NULL" in L.hlhgat_last_error()
    assert L.hlhgat_dropout_fwd(a, 5, 3, 5, T, 1.0, None, 0, a, a, 5, None) == 1
    assert L.hlhgat_dropout_fwd(a, 5, 3, 5, T, 1.0, a, 0, None, a, 5, None) == 1
    assert L.hlhgat_dropout_fwd(a, 5, 3, 5, T, 1.0, a, 0, a, None, 5, None) == 1
    assert L.hlhgat_dropout_fwd(a, 5, 3, 5, (1 << 24) + 1, 1.0, a, 0, a, a, 5, None) == 1
    assert b"2^24" in L.hlhgat_last_error()
    assert L.hlhgat_dropout_fwd(a, 5, -1, 5, T, 1.0, a, 0, a, a, 5, None) == 1
    assert L.hlhgat_dropout_bwd(a, 4, 3, 5, T, 1.0, a, 0, a, 5, None) == 1  # lddy < d
    assert b"dropout_bwd" in L.hlhgat_last_error()
    assert L.hlhgat_dropout_bwd(a, 5, 3, 5, T, 1.0, a, 0, a, 4, None) == 1  # lddx < d
    assert L.hlhgat_dropout_bwd(None, 5, 3, 5, T, 1.0, a, 0, a, 5, None) == 1
    assert L.hlhgat_dropout_bwd(a, 5, 3, 5, T, 1.0, None, 0, a, 5, None) == 1
    assert L.hlhgat_dropout_bwd(a, 5, 3, 5, T, 1.0, a, 0, None, 5, None) == 1
    assert L.hlhgat_dropout_bwd(a, 5, 3, 5, (1 << 24) + 1, 1.0, a, 0, a, 5, None) == 1
    assert L.hlhgat_dropout_advance(None, None) == 1
    # n * d == 0 is a no-op (no launch, nothing dereferenced)
    assert L.hlhgat_dropout_fwd(None, 5, 0, 5, T, 1.0, None, 0, None, None, 5, None) == 0
    assert L.hlhgat_dropout_bwd(None, 0, 3, 0, T, 1.0, None, 0, None, 0, None) == 0


def test_cpu_tensors_go_to_torch():
    from hlhgat import ops
    x = torch.randn(7, 5)
    torch.manual_seed(3)
    want = torch.nn.functional.dropout(x, 0.4, True)
    torch.manual_seed(3)
    assert torch.equal(ops.dropout(x, 0.4, True), want)
    assert ops.dropout(x, 0.4, False) is x
    assert ops.dropout(x, 0.0, True) is x
    assert ops.dropout_params(0.25) == (1 << 22, 1.0 / 0.75)
    assert ops.dropout_params(1.0) == (1 << 24, 0.0)
    with pytest.raises(ValueError):
        ops.dropout_params(1.5)


def test_cpu_sequential_with_live_dropout_unchanged():
    from hlhgat.nn import Sequential, run_sequential
    torch.manual_seed(0)
    lin, drop = tnn.Linear(6, 6), tnn.Dropout(0.5)
    seq = Sequential("x", [(lin, "x -> x"), (tnn.ReLU(), "x -> x"), (drop, "x -> x")]).train()
    x = torch.randn(9, 6)
    torch.manual_seed(11)
    want = drop(torch.relu(lin(x)))
    torch.manual_seed(11)
    assert torch.equal(seq(x), want)
    torch.manual_seed(12)
    want = torch.nn.functional.dropout(torch.relu(x), 0.5, True)
    torch.manual_seed(12)
    assert torch.equal(run_sequential(tnn.Sequential(tnn.ReLU(), drop), [x]), want)
    seq.eval()
    assert torch.equal(seq(x), torch.relu(lin(x)))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
SEED = 0x1234_5678_9ABC_DEF1  # both key words non-zero


def _reset(ops, seed=SEED, steps=3):
    ops.dropout_manual_seed(seed)
    for _ in range(steps):
        ops.dropout_advance()
    return steps


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n, d", [(1, 1), (3, 5), (7, 64), (129, 96), (257, 4)])
def test_kernels_bitwise_vs_reference(cuda, n, d, p):
    """y, mask and dx equal dropout_ref bit for bit for a contiguous y, an
    aligned column block of a 200-wide slab and a misaligned one (scalar
    path); the backward with a contiguous dy and with dy a column block."""
    from hlhgat import ops
    gen = np.random.default_rng(n * 1000 + d)
    x_np = gen.standard_normal((n, d)).astype(np.float32)
    g_np = gen.standard_normal((n, d)).astype(np.float32)
    step = 3
    want_y = R.apply(x_np, p, SEED, step, 0)
    want_dx = R.apply(g_np, p, SEED, step, 0)
    mask = R.keep(n, d, p, SEED, step, 0)
    G = torch.full((n, 200), float("nan"), device=cuda)
    G[:, 8:8 + d] = _t(g_np, cuda)
    for c0 in (None, 64, 3):
        _reset(ops, steps=step)
        x = _t(x_np, cuda).requires_grad_(True)
        if c0 is None:
            y = ops.dropout(x, p)
            assert y.is_contiguous()
        else:
            slab = torch.full((n, 200), float("nan"), device=cuda)
            y = ops.dropout(x, p, out=slab[:, c0:c0 + d])
            assert y.data_ptr() == slab.data_ptr() + 4 * c0
            assert n == 1 or y.stride(0) == 200  # (a one-row tensor's row stride is arbitrary)
            rest = torch.ones(200, dtype=torch.bool)
            rest[c0:c0 + d] = False
            assert torch.isnan(slab[:, rest.to(cuda)]).all(), "wrote outside its column block"
        assert ops.dropout_state() == (SEED, step, 1)
        got = y.detach().cpu().numpy()
        assert np.array_equal(got, want_y), f"layout {c0}"
        live = x_np != 0
        assert np.array_equal((got != 0)[live], mask[live])
        (dx,) = torch.autograd.grad(y, x, _t(g_np, cuda), retain_graph=True)
        assert np.array_equal(dx.cpu().numpy(), want_dx), f"layout {c0}: contiguous dy"
        (dx,) = torch.autograd.grad(y, x, G[:, 8:8 + d])
        assert np.array_equal(dx.cpu().numpy(), want_dx), f"layout {c0}: column-block dy"
    ops.check_device_errors()


@pytest.mark.gpu
def test_p0_is_identity_and_p1_is_zero(cuda):
    from hlhgat import ops
    _reset(ops)
    x = torch.randn(33, 20, device=cuda, requires_grad=True)
    assert ops.dropout(x, 0.0) is x
    assert ops.dropout(x, 0.7, training=False) is x
    assert ops.dropout_state()[2] == 0  # no site consumed
    y = ops.dropout(x, 1.0)
    assert torch.equal(y, torch.zeros_like(y))
    y.backward(torch.randn_like(y))
    assert torch.equal(x.grad, torch.zeros_like(x))
    with pytest.raises(RuntimeError):
        ops.dropout(x, 0.5, out=torch.empty(33, 21, device=cuda))
    x3 = torch.randn(4, 5, 6, device=cuda)
    _reset(ops)
    y3 = ops.dropout(x3, 0.5)
    assert y3.shape == x3.shape
    assert np.array_equal(y3.cpu().numpy().reshape(20, 6),
                          R.apply(x3.cpu().numpy().reshape(20, 6), 0.5, SEED, 3, 0))


@pytest.mark.gpu
def test_backward_uses_the_forwards_snapshot(cuda):
    from hlhgat import ops
    step = _reset(ops)
    x = torch.randn(129, 96, device=cuda, requires_grad=True)
    y = ops.dropout(x, 0.5)
    ops.dropout_advance()
    ops.dropout_manual_seed(999)
    g = torch.randn(129, 96, device=cuda)
    y.backward(g)
    want = R.apply(g.cpu().numpy(), 0.5, SEED, step, 0)
    assert np.array_equal(x.grad.cpu().numpy(), want)
    assert np.array_equal(x.grad.cpu().numpy() != 0, y.detach().cpu().numpy() != 0)


@pytest.mark.gpu
def test_call_sequence_and_reseeding(cuda):
    from hlhgat import ops
    ones = torch.ones(129, 96, device=cuda)

    def run():
        ops.dropout_manual_seed(42)
        assert ops.dropout_state() == (42, 0, 0)
        a = ops.dropout(ones, 0.25)
        b = ops.dropout(ones, 0.25)
        ops.dropout_advance()
        c = ops.dropout(ones, 0.25)
        assert ops.dropout_state() == (42, 1, 3)
        return [t.cpu().numpy() for t in (a, b, c)]

    a, b, c = run()
    s = R.scale(0.25)
    for got, (step, site) in zip((a, b, c), ((0, 0), (0, 1), (1, 2))):
        assert np.array_equal(got, R.keep(129, 96, 0.25, 42, step, site) * s)
    assert not np.array_equal(a, b) and not np.array_equal(b, c)
    for first, again in zip((a, b, c), run()):
        assert np.array_equal(first, again)
    ops.dropout_manual_seed(2 ** 64 - 3)  # the seed is an unsigned 64-bit value
    assert ops.dropout_state() == (2 ** 64 - 3, 0, 0)
    assert np.array_equal(ops.dropout(ones, 0.25).cpu().numpy(),
                          R.keep(129, 96, 0.25, 2 ** 64 - 3, 0, 0) * s)


@pytest.mark.gpu
def test_graph_replay_draws_fresh_masks(cuda):
    from hlhgat import ops
    ones = torch.ones(129, 96, device=cuda)
    ops.dropout_manual_seed(7)
    ops.dropout_advance()
    ops.dropout(ones, 0.25)  # kernels loaded before the capture
    ops.dropout_manual_seed(7)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.dropout_advance()
        y = ops.dropout(ones, 0.25)
    seed, s0, site = ops.dropout_state()
    assert (seed, s0, site) == (7, 0, 1)  # captured, not run; site 0 is baked in
    s = R.scale(0.25)
    seen = []
    for r in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        assert np.array_equal(got, R.keep(129, 96, 0.25, 7, s0 + r, 0) * s), f"replay {r}"
        seen.append(got)
    assert ops.dropout_state() == (7, 3, 1)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert not np.array_equal(seen[0], seen[2])


# -- blocks and heads --------------------------------------------------------
class _Sites:
    """Records, for every ops.dropout launch inside the context, the site it
    took (by output tensor), so a test can rebuild each mask from dropout_ref."""

    def __init__(self, monkeypatch):
        from hlhgat import ops
        self.calls = []  # (output, site)
        real = ops.dropout

        def spy(x, p, training=True, out=None):
            site = ops._dropout_st(x.device).site if x.is_cuda else None
            y = real(x, p, training, out)
            if y is not x:
                self.calls.append((y, site))
            return y

        monkeypatch.setattr(ops, "dropout", spy)

    def site_of(self, y):
        hit = [s for t, s in self.calls
               if t.data_ptr() == y.data_ptr() and t.shape == y.shape and t.stride() == y.stride()]
        assert len(hit) == 1, f"{len(hit)} dropout launches produced this tensor"
        return hit[0]


@pytest.fixture(scope="module")
def zinc(cuda):
    from hlhgat.synthetic import zinc_like_batch
    return zinc_like_batch(20, seed=4).to(cuda)


def _block_pair(cuda, p):
    from hlhgat.hodge_st_model import _hl_block
    torch.manual_seed(3)
    b0 = _hl_block(16, 16, 32, 2, 0.0)
    bp = _hl_block(16, 16, 32, 2, p)
    bp.load_state_dict(b0.state_dict())
    return b0.to(cuda).train(), bp.to(cuda).train()


@pytest.mark.gpu
def test_hl_block_output_is_masked_p0_output(cuda, zinc, monkeypatch):
    from hlhgat import ops
    p = 0.25
    b0, bp = _block_pair(cuda, p)
    gen = torch.Generator().manual_seed(5)
    xt = torch.randn(zinc.x_t.shape[0], 16, generator=gen).to(cuda)
    xs = torch.randn(zinc.x_s.shape[0], 16, generator=gen).to(cuda)
    args = (xt, zinc.edge_index_t, zinc.edge_weight_t, xs, zinc.edge_index_s, zinc.edge_weight_s)
    with torch.no_grad():
        ops.clear_caches()
        ref_t, ref_s = b0(*args)
        step = _reset(ops)
        rec = _Sites(monkeypatch)
        out_t, out_s = bp(*args)
        torch.cuda.synchronize()
        assert ops.dropout_state() == (SEED, step, 2)
        sites = []
        for out, ref in ((out_t, ref_t), (out_s, ref_s)):
            site = rec.site_of(out)
            sites.append(site)
            want = R.apply(ref.cpu().numpy(), p, SEED, step, site)
            assert np.array_equal(out.cpu().numpy(), want)
            assert (want == 0).mean() > (ref.cpu().numpy() == 0).mean()  # something was dropped
        assert sorted(sites) == [0, 1]  # the node and edge sides use different sites
        bp.eval()
        b0.eval()
        e_t, e_s = bp(*args)
        r_t, r_s = b0(*args)
        assert torch.equal(e_t, r_t) and torch.equal(e_s, r_s)
        assert ops.dropout_state()[2] == 2  # eval consumes no site
    ops.clear_caches()
    ops.check_device_errors()


HEAD_KW = dict(channels=[2], filters=[32], mlp_channels=[32], K=2)


def _head(cuda, p, sd=None):
    import hlhgat
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(dropout_ratio=p, keig=15, **HEAD_KW)
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(cuda).train()


def _loss_and_grads(m, batch):
    from hlhgat import ops
    ops.clear_caches()
    m.zero_grad(set_to_none=True)
    out = m(batch)
    loss = torch.nn.functional.l1_loss(out.view(-1), batch.y.view(-1))
    loss.backward()
    torch.cuda.synchronize()
    ops.clear_caches()
    return out.detach().cpu(), loss.detach().cpu(), {k: v.grad.detach().cpu().clone()
                                                     for k, v in m.named_parameters()}


@pytest.mark.gpu
def test_head_slab_on_and_off_agree_and_append_copies_nothing(cuda, zinc, monkeypatch):
    from hlhgat import ops
    m = _head(cuda, 0.25)
    seen = []
    real_append = ops.DenseConcat.append

    def append(self, y):
        c0 = self.used
        seen.append(y.data_ptr() == self.S.data_ptr() + 4 * c0 and y.stride(0) == self.S.stride(0))
        return real_append(self, y)

    monkeypatch.setattr(ops.DenseConcat, "append", append)
    res = {}
    for slab in (True, False):
        monkeypatch.setattr(ops, "DENSE_SLAB", slab)
        ops.dropout_manual_seed(SEED)
        res[slab] = _loss_and_grads(m, zinc)
        assert ops.dropout_state()[2] == 6  # 3 blocks x 2 sides
    assert len(seen) == 6 and all(seen), seen  # every block output was already in place
    assert torch.equal(res[True][0], res[False][0])  # DenseConcat: forward identity
    assert torch.equal(res[True][1], res[False][1])
    for k, g in res[False][2].items():
        close(res[True][2][k], g, 1e-4, f"grad {k} (slab on vs off)")
    ops.check_device_errors()


@pytest.mark.gpu
def test_head_gradients_match_explicit_mask_twin(cuda, zinc, monkeypatch):
    """The dropout head against a dropout_ratio=0 twin whose block outputs are
    multiplied, in torch ops, by the recorded mask * s."""
    from hlhgat import ops
    p = 0.25
    m = _head(cuda, p)
    twin = _head(cuda, 0.0, sd=m.state_dict())
    step = _reset(ops)
    rec = _Sites(monkeypatch)
    captured = {}
    hooks = [blk.register_forward_hook(lambda mod, a, out, name=name: captured.__setitem__(
        name, [rec.site_of(out[0]), rec.site_of(out[1])]))
        for name, blk in m.named_children() if name.startswith(("HL_init", "NEConv"))]
    out, loss, grads = _loss_and_grads(m, zinc)
    for h in hooks:
        h.remove()
    assert sorted(s for v in captured.values() for s in v) == list(range(6))
    s = float(R.scale(p))

    def masked(name):
        def hook(mod, a, o):
            return [t * _t(R.keep(t.shape[0], t.shape[1], p, SEED, step, site).astype(np.float32)
                           * np.float32(s), cuda) for t, site in zip(o, captured[name])]
        return hook

    for name, blk in twin.named_children():
        if name in captured:
            blk.register_forward_hook(masked(name))
    monkeypatch.setattr(ops, "DENSE_SLAB", False)  # the twin: plain torch.cat, nothing in place
    out2, loss2, grads2 = _loss_and_grads(twin, zinc)
    close(out, out2, 1e-4, "output")
    close(loss, loss2, 1e-4, "loss")
    for k, g in grads2.items():
        close(grads[k], g, 1e-4, f"grad {k}")
    ops.check_device_errors()


@pytest.mark.gpu
def test_mlp_dropout_runs_on_the_hip_path(cuda, zinc):
    """dropout_ratio_mlp reaches ops.dropout through run_mlp_stack: one site
    per readout layer, mask = dropout_ref's (zeros where it drops)."""
    import hlhgat
    from hlhgat import ops
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(dropout_ratio_mlp=0.5, keig=15, **HEAD_KW)
    m = m.to(cuda).train()
    step = _reset(ops)
    ops.clear_caches()
    x, y = m(zinc, if_final_layer=True)
    y.sum().backward()
    torch.cuda.synchronize()
    ops.clear_caches()
    assert ops.dropout_state() == (SEED, step, 1)
    keep = R.keep(x.shape[0], x.shape[1], 0.5, SEED, step, 0)
    assert not (x.detach().cpu().numpy()[~keep] != 0).any()
    assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    m.eval()
    with torch.no_grad():
        m(zinc)
    assert ops.dropout_state()[2] == 1


def _l1(out, b):
    return torch.nn.functional.l1_loss(out.view(-1), b.y.view(-1))


def _three_steps(cuda, zinc, sd, p, lr):
    from hlhgat import ops
    from hlhgat.train import TrainStep
    m = _head(cuda, p, sd=sd)
    ops.dropout_manual_seed(SEED)
    st = TrainStep(m, _l1, lr=lr, graphs=True)
    losses = [float(st(zinc).detach()) for _ in range(3)]
    torch.cuda.synchronize()
    assert st.stats["captures"] == 1 and st.stats["replay"] == 2
    return losses, st


@pytest.mark.gpu
def test_trainstep_replays_draw_fresh_masks_and_repeat_bitwise(cuda, zinc):
    from hlhgat import ops
    sd = {k: v.clone() for k, v in _head("cpu", 0.25).state_dict().items()}
    # lr = 0: the parameters stand still, so only the masks can move the loss
    frozen, _ = _three_steps(cuda, zinc, sd, 0.25, 0.0)
    print("frozen-parameter losses", frozen)
    assert len(set(frozen)) == 3, frozen
    first, st = _three_steps(cuda, zinc, sd, 0.25, 1e-3)
    assert ops.dropout_state()[1] == 3  # one advance per step, replays included
    again, _ = _three_steps(cuda, zinc, sd, 0.25, 1e-3)
    print("losses", first, again)
    assert len(set(first)) == 3, first
    assert first == again  # no atomics: bitwise repeatable
    ops.check_device_errors()


@pytest.mark.gpu
def test_trainstep_without_dropout_captures_no_dropout_kernel(cuda, zinc, monkeypatch):
    """dropout_ratio = 0 captures the graph it always did (no advance launch,
    the same count with the A/B switch off); dropout_ratio > 0 adds exactly
    one launch per site each way and the advance."""
    from hlhgat import ops, train
    monkeypatch.setattr(train, "KEEP_GRAPHS", True)
    sd = {k: v.clone() for k, v in _head("cpu", 0.0).state_dict().items()}

    def counts(p):
        _, st = _three_steps(cuda, zinc, sd, p, 1e-3)
        (ent,) = st._graphs.values()
        h = ent.graph.raw_cuda_graph()
        return ops.graph_kernel_count(h, "k_")[0], ops.graph_kernel_count(h, "k_dropout")[1]

    total0, drop0 = counts(0.0)
    assert drop0 == 0
    monkeypatch.setattr(ops, "HIP_DROPOUT", False)
    assert counts(0.0) == (total0, 0)
    monkeypatch.setattr(ops, "HIP_DROPOUT", True)
    total, drop = counts(0.25)
    assert drop == 6 + 6 + 1  # forward and backward of 3 blocks x 2 sides, one advance
    print("captured kernels: p=0", total0, "p=0.25", total)
    ops.check_device_errors()
