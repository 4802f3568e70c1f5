"""Series of different lengths in one batch: the ragged time layout of
csrc/tconv.hip (hlhgat_tseries_map and the *_ragged entries), per-graph windows
in the FC pass (hlhgat_fc_prepare_windows), Inception1D.forward(x, lengths) and
BrainPipeline.batch(window="per_sample") -- the per-sample windows of
HL-HGAT-DEMO/lib/Hodge_Dataset.py:131-133 as one captured graph.

Shapes: S = 7 series, t_max = 40, the module's default widths (64 channels, 8
per branch, pool 3).  Length set A = [40, 24, 1, 2, 37, 3, 21] sums to 128: a
series boundary falls on the 64-row tile edge, two series are shorter than the
+-2 halo, and 152 rows (whole tiles) are dead.  B = [39, 26, 1, 5, 40, 2, 30]
sums to 143: boundaries at rows 65 and 66 and a partly dead tile.  In every
ragged test the padded input holds NaN at x[s, len[s]:]; op-level tests poison
the dead tail of every input buffer with NaN; valid outputs must be finite and
dead output rows exactly 0.

Fixture: tests/golden/make_golden_ragged.py ran the REFERENCE Inception1D in
eval() on every series alone at its own length.  tests/ragged_ref.py restates
the ragged forward in fp64 with pooled BatchNorm by formula.

Tolerances: conftest.close at 1e-5 for outputs and 1e-4 for gradients, the
project's layer tolerances (tests/test_brain_head.py); x_t / x_s of
the pipeline at the 1e-5 / 4e-6 of tests/test_brain_fc.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ragged_ref as RR
from conftest import close, load_golden

T_ = torch.from_numpy
FIX = "inception1d_ragged"
LENS = {"A": RR.LENS_A, "B": RR.LENS_B}
S, T_MAX, CH, NCH, POOL, SLOPE = 7, RR.T_MAX, 64, 8, 3, 0.1
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _g():
    return load_golden(FIX)


def _sd(dtype=torch.float32):
    g = _g()
    return {k[3:]: (T_(np.asarray(g[k])).to(dtype) if g[k].dtype.kind == "f"
                    else T_(np.asarray(g[k]))) for k in g if k.startswith("sd/")}


def _module(device="cpu", train=False):
    import hlhgat
    mod = hlhgat.Inception1D(CH, NCH, POOL, if_readout=True)
    mod.load_state_dict(_sd(), strict=True)
    mod = mod.to(device)
    return mod.train() if train else mod.eval()


def _x(lens, device="cpu", poison=True):
    x = T_(_g()["x"]).clone()
    if poison:
        for s, n in enumerate(lens):
            x[s, n:] = NAN
    return x.to(device)


def _lens(lens, device="cpu"):
    return torch.tensor(lens, dtype=torch.int32, device=device)


def _soff(lens, m=None):
    if m is not None:
        lens = [(n + 2 * ((m - 1) // 2) - m) // (m - 1) + 1 for n in lens]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), list(lens)


def _compact(rows, cap, fill=NAN):
    """Series rows [len_s, C] stacked compactly into [cap, C], dead tail = fill."""
    cat = torch.cat(rows)
    out = torch.full((cap, cat.shape[1]), fill, dtype=cat.dtype)
    out[:cat.shape[0]] = cat
    return out


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_fixture_margin():
    g = _g()
    assert float(g["margin"]) >= 1e-4 and sum(RR.LENS_A) == 128 and sum(RR.LENS_B) == 143
    assert g["lens_A"].tolist() == RR.LENS_A and g["lens_B"].tolist() == RR.LENS_B


@pytest.mark.parametrize("tag", ["A", "B"])
def test_inception_cpu_ragged_eval_equals_fixture(tag):
    mod = _module()
    with torch.no_grad():
        out = mod(_x(LENS[tag]), _lens(LENS[tag]))
    assert torch.isfinite(out).all()
    close(out, _g()["out_eval_" + tag], 1e-5, "eval out " + tag)


def test_inception_cpu_equal_lengths_equals_dense():
    a, b = _module(train=True), _module(train=True)
    x = _x([T_MAX] * S)
    close(b(x, _lens([T_MAX] * S)).detach(), a(x).detach(), 1e-5, "out")
    for k in ("running_mean", "running_var"):
        for bn in ("bn1", "bn2"):
            close(getattr(getattr(b, bn), k), getattr(getattr(a, bn), k), 1e-5, bn + "." + k)
    with pytest.raises(ValueError, match="if_readout"):
        b.if_readout = False
        b(x, _lens([T_MAX] * S))


def test_ragged_ref_equal_lengths_is_the_dense_module():
    """The fp64 restatement with equal lengths is the module itself."""
    mod = _module(train=True).double()
    x = _x([T_MAX] * S).double()
    want = mod(x).detach()
    got = RR.ragged_forward(_sd(torch.float64), x, [T_MAX] * S, m=POOL, slope=SLOPE)
    close(got, want, 1e-12, "fp64 restatement")


def _fc_pipe(cut=None):
    import hlhgat
    from test_brain_fc import _pipe_levels
    g = load_golden("brainfc_pipe")
    N = g["x"].shape[1]
    series = [s[:, :cut] if cut else s for s in g["x"]]
    y = torch.stack([hlhgat.brain_target(s) for s in g["scores"]])
    return hlhgat.BrainPipeline(series, y, _pipe_levels(g["edge_index"], N)), g


@pytest.mark.parametrize("cut", [None, 290])
def test_pipeline_cpu_per_sample_equals_reference_lines(cut):
    """device="cpu", window="per_sample": the reference's three lines
    (lib/Hodge_Dataset.py:134-137) on every sample with its own draw."""
    pipe, g = _fc_pipe(cut)
    N, T = g["x"].shape[1], (cut or g["x"].shape[2])
    ei = T_(g["edge_index"])
    E = ei.shape[1]
    idx = np.array([2, 0, 1])
    assert pipe.t_max == min(299, T)
    seen = set()
    for seed in range(6):
        w = pipe._windows(idx, "per_sample", seed)
        assert np.array_equal(w, pipe._windows(idx, "per_sample", seed))  # deterministic in seed
        assert w.shape == (3, 2) and (w[:, 0] >= 0).all() and (w[:, 0] < 75).all()
        drawn = np.random.default_rng(seed)
        t0 = drawn.integers(0, 75, size=3)
        ln = drawn.integers(250, 300, size=3)
        assert np.array_equal(w[:, 0], t0) and ((ln >= 250) & (ln < 300)).all()
        # cut at the series end, as the reference's slice is (and at t_max)
        assert np.array_equal(w[:, 1], np.minimum(np.minimum(ln, T - t0), pipe.t_max))
        seen.update(w[:, 1].tolist())
        b = pipe.batch(idx, window="per_sample", seed=seed, device="cpu")
        assert b[0].x_t.shape == (3 * N, pipe.t_max)  # t_max does not depend on the draw
        assert b[0].t_len.dtype == torch.int32
        assert b[0].t_len.tolist() == np.repeat(w[:, 1], N).tolist()
        for k, (i, (tb, n)) in enumerate(zip(idx, w.tolist())):
            f = pipe.series[i][:, tb:tb + n]
            f = (f - f.mean()) / f.std()
            xs = torch.corrcoef(f)[ei[0], ei[1]].view(-1, 1)
            xt = b[0].x_t[k * N:(k + 1) * N]
            assert torch.equal(xt[:, :n], f) and not xt[:, n:].any()
            assert torch.equal(b[0].x_s[k * E:(k + 1) * E], xs)
        assert torch.equal(b[0].y, pipe.targets[T_(idx)])
    assert len(seen) > 3  # the subjects of a batch got windows of their own
    # an explicit [B, 2] array is taken as it is
    b = pipe.batch([1, 2], window=np.array([[3, 100], [40, 250]]), device="cpu")
    assert b[0].t_len.tolist() == [100] * N + [250] * N
    with pytest.raises(ValueError, match="windows"):
        pipe.batch([1, 2], window=np.array([[3, 100], [40, T]]), device="cpu")
    with pytest.raises(ValueError, match="windows"):
        pipe.batch([1], window=np.array([[0, 1]]), device="cpu")


def test_capi_rejects_bad_arguments():
    """HLHGAT_EINVAL and a message before any HIP call (runs without a GPU)."""
    from hlhgat import _lib
    L = _lib.LIB
    buf = (C.c_float * 4096)()
    p = (C.cast(buf, C.c_void_p).value + 15) // 16 * 16

    def desc(S=2, t_max=8, pool=3, t1=None, null=None):
        d = _lib.TSeriesDesc()
        d.n_series, d.pool = S, pool
        d.t_max[0] = t_max
        d.t_max[1] = L.hlhgat_maxpool_time_len(t_max, pool) if t1 is None else t1
        for i in range(2):
            d.soff[i], d.tab[i], d.sid[i] = p, p, p
        d.n_rows = p
        if null == "n_rows":
            d.n_rows = None
        elif null is not None:
            getattr(d, null)[1] = None
        return C.byref(d)

    bi = (C.c_int64 * 1)(4)
    bt = (C.c_int32 * 1)(1)
    bw = (C.c_void_p * 1)(p)
    calls = {
        "map": lambda d: L.hlhgat_tseries_map(p, d, None),
        "pack": lambda d: L.hlhgat_tseries_pack(p, 8, d, 0, p, None),
        "conv": lambda d: L.hlhgat_tconv_fwd_ragged(p, d, 0, 4, p, None, 4, 1, 0, 0, p, None),
        "embed": lambda d: L.hlhgat_tconv_embed_fwd_ragged(p, d, p, None, 4, 5, p, None),
        "wgrad": lambda d: L.hlhgat_tconv_bwd_weight_ragged(p, p, d, 1, 4, 4, 1, 1, bw, bi, bt,
                                                             None, p, 1 << 20, None),
        "pool_f": lambda d: L.hlhgat_leaky_maxpool_time_fwd_ragged(p, d, 4, 0.1, p, p, None),
        "pool_b": lambda d: L.hlhgat_leaky_maxpool_time_bwd_ragged(p, p, p, d, 4, 0.1, p, None),
        "read_f": lambda d: L.hlhgat_time_readout_fwd_ragged(p, d, 4, 0.1, p, p, None),
        "read_b": lambda d: L.hlhgat_time_readout_bwd_ragged(p, p, p, d, 4, 0.1, p, None),
    }

    def bad(rc, word):
        assert rc == 1, (rc, word)
        msg = L.hlhgat_last_error()
        assert msg and word.encode() in msg, (msg, word)

    for name, fn in calls.items():
        bad(fn(None), "NULL map")
        bad(fn(desc(S=-1)), "S < 0")
        bad(fn(desc(t_max=0)), "t_max")
        bad(fn(desc(t1=2)), "t_max[1]")
        bad(fn(desc(pool=1)), "pool")
        for tab in ("soff", "tab", "sid", "n_rows"):
            bad(fn(desc(null=tab)), "NULL table")
    bad(L.hlhgat_tseries_map(None, desc(), None), "NULL tlen")
    bad(L.hlhgat_tseries_pack(p, 7, desc(), 0, p, None), "ldx")
    bad(L.hlhgat_tseries_pack(None, 8, desc(), 0, p, None), "NULL")
    bad(L.hlhgat_tconv_fwd_ragged(p, desc(), 2, 4, p, None, 4, 1, 0, 0, p, None), "stage")
    bad(L.hlhgat_tconv_fwd_ragged(None, desc(), 0, 4, p, None, 4, 1, 0, 0, p, None), "NULL")
    bad(L.hlhgat_tconv_fwd_ragged(p, desc(), 0, 4, p, None, 4, 2, 0, 0, p, None), "taps")

    def win(x=p, ldx=8, G=1, N=4, t0=p, ln=p, t_max=8, ws=p, nbytes=4096):
        return L.hlhgat_fc_prepare_windows(x, ldx, None, G, N, t0, ln, t_max, None, ws, nbytes,
                                           None)

    bad(win(t0=None), "NULL")
    bad(win(ln=None), "NULL")
    bad(win(t_max=0), "t_max")
    bad(win(t_max=1), "T")
    bad(win(G=-1), "G")
    bad(win(t_max=9), "ldx")
    bad(win(x=None), "NULL")
    bad(win(nbytes=64), "workspace")
    assert win(G=0, t0=None, ln=None) == 0
    assert L.hlhgat_version() >= 110 and _lib.DEVERR_TSERIES_LEN == 128


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["A", "B"])
def test_eval_vs_reference(cuda, tag):
    """1. The reference in eval() on every series alone."""
    from hlhgat import ops
    mod = _module(cuda)
    with torch.no_grad():
        out = mod(_x(LENS[tag], cuda), _lens(LENS[tag], cuda))
    assert torch.isfinite(out).all()
    err = close(out.cpu(), _g()["out_eval_" + tag], 1e-5, "eval out " + tag)
    print(f"[ragged eval {tag}] max|diff| {err:.3e}")
    ops.check_device_errors()


def _train_run(cuda, tag):
    lens = LENS[tag]
    mod = _module(cuda, train=True)
    x = _x(lens, cuda).requires_grad_(True)
    out = mod(x, _lens(lens, cuda))
    (out * T_(_g()["R"]).to(cuda)).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().clone(), "grad_x": x.grad.detach().clone()}
    for k, p in mod.named_parameters():
        res["grad/" + k] = p.grad.detach().clone()
    for k, v in mod.state_dict().items():
        if "running" in k:
            res["state/" + k] = v.detach().clone()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["A", "B"])
def test_train_vs_fp64(cuda, tag):
    """2. Train mode against the fp64 restatement with pooled BatchNorm."""
    from hlhgat import ops
    lens = LENS[tag]
    sd = {k: (v.requires_grad_(True) if v.is_floating_point() and "running" not in k else v)
          for k, v in _sd(torch.float64).items()}
    x64 = _x(lens, poison=False).double().requires_grad_(True)
    info = {}
    out64 = RR.ragged_forward(sd, x64, lens, m=POOL, slope=SLOPE, training=True, info=info)
    assert info["margin"] >= 1e-4
    (out64 * T_(_g()["R"]).double()).sum().backward()
    got = _train_run(cuda, tag)
    assert all(torch.isfinite(v).all() for v in got.values())
    err = close(got["out"].cpu(), out64.detach(), 1e-5, "out")
    print(f"[ragged train {tag}] out max|diff| {err:.3e}")
    for s, n in enumerate(lens):  # the padded columns: exactly 0
        assert not got["grad_x"][s, n:].any(), s
    err = close(got["grad_x"].cpu(), x64.grad, 1e-4, "grad_x")
    print(f"[ragged train {tag}] grad_x max|diff| {err:.3e}")
    for k, v in sd.items():
        if not (torch.is_tensor(v) and v.requires_grad):
            continue
        err = close(got["grad/" + k].cpu(), v.grad, 1e-4, "grad " + k)
        print(f"[ragged train {tag}] grad {k} max|diff| {err:.3e}")
    # running statistics: the pooled mean and the UNBIASED variance, n = n_rows
    sd0 = _sd(torch.float64)
    for bn, (mean, unb, n) in info["stats"].items():
        assert n == sum(lens if bn == "bn1" else _soff(lens, POOL)[1])
        close(got[f"state/{bn}.running_mean"].cpu(), 0.9 * sd0[bn + ".running_mean"] + 0.1 * mean,
              1e-5, bn + ".running_mean")
        close(got[f"state/{bn}.running_var"].cpu(), 0.9 * sd0[bn + ".running_var"] + 0.1 * unb,
              1e-5, bn + ".running_var")
    ops.check_device_errors()


def _grads(fn, inputs, gout):
    """fn(*inputs) and the gradients of sum(out * gout) w.r.t. every input."""
    leaves = [t.detach().clone().requires_grad_(True) for t in inputs]
    out = fn(*leaves)
    out.backward(gout)
    return [out.detach()] + [t.grad for t in leaves]


def _branch_params(cuda, cin, couts=(16, 32, 16), taps=(1, 3, 5), seed=0):
    gen = torch.Generator().manual_seed(50 + seed)
    ws = [(torch.randn(co, cin, k, generator=gen) / (cin * k) ** 0.5).to(cuda)
          for co, k in zip(couts, taps)]
    bs = [torch.randn(co, generator=gen).to(cuda) for co in couts]
    return ws, bs


@pytest.mark.gpu
def test_equal_lengths_ops_are_dense_bitwise(cuda):
    """3a. With tlen == t_max layout, tiling and reduction order coincide:
    every ragged op equals its dense twin bit for bit, gradients included."""
    from hlhgat import ops
    tm = ops.time_series_map(_lens([T_MAX] * S, cuda), T_MAX, POOL)
    T2 = ops.maxpool_time_len(T_MAX, POOL)
    assert tm.t_max == (T_MAX, T2)
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(cuda)  # noqa: E731

    def same(a, b, what):
        assert len(a) == len(b)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.isfinite(u).all() and torch.equal(u.reshape(-1), v.reshape(-1)), (what, i)

    # the embedding: [S, T] -> [S*T, 64]
    x = rnd(S, T_MAX)
    we, be = _branch_params(cuda, 1, (CH,), (5,))
    gy = rnd(S * T_MAX, CH)
    same(_grads(lambda x, w, b: ops.temporal_conv_ragged(ops.time_series_pack(x, tm), tm, 0,
                                                         [w], [b]), [x, we[0], be[0]], gy),
         _grads(lambda x, w, b: ops.temporal_conv(x.reshape(S, T_MAX, 1), [w], [b]),
                [x, we[0], be[0]], gy.view(S, T_MAX, CH)), "embedding")
    # the three-branch convolution at both stages: forward, data, weight and bias gradient
    for stage, T in ((0, T_MAX), (1, T2)):
        h = rnd(S * T, CH)
        ws, bs = _branch_params(cuda, CH, seed=stage)
        gy = rnd(S * T, CH)
        same(_grads(lambda h, *p: ops.temporal_conv_ragged(h, tm, stage, p[:3], p[3:]),
                    [h] + ws + bs, gy),
             _grads(lambda h, *p: ops.temporal_conv(h.view(S, T, CH), p[:3], p[3:]),
                    [h] + ws + bs, gy.view(S, T, CH)), f"conv stage {stage}")
    # pool and readout
    h = rnd(S * T_MAX, CH)
    gy = rnd(S * T2, CH)
    same(_grads(lambda h: ops.leaky_maxpool_time_ragged(h, tm, SLOPE), [h], gy),
         _grads(lambda h: ops.leaky_maxpool_time(h.view(S, T_MAX, CH), SLOPE, POOL), [h],
                gy.view(S, T2, CH)), "pool")
    h = rnd(S * T2, 4 * NCH)
    gy = rnd(S, 8 * NCH)
    same(_grads(lambda h: ops.time_readout_ragged(h, tm, SLOPE), [h], gy),
         _grads(lambda h: ops.time_readout(h.view(S, T2, 4 * NCH), SLOPE), [h], gy), "readout")
    ops.check_device_errors()


@pytest.mark.gpu
def test_equal_lengths_module_is_dense(cuda):
    """3b. The whole Inception1D with lengths == t_max against lengths=None."""
    res = []
    for lengths in (None, _lens([T_MAX] * S, cuda)):
        mod = _module(cuda, train=True)
        x = _x([T_MAX] * S, cuda).requires_grad_(True)
        out = mod(x) if lengths is None else mod(x, lengths)
        (out * T_(_g()["R"]).to(cuda)).sum().backward()
        res.append([out.detach(), x.grad] + [p.grad for p in mod.parameters()]
                   + [v for k, v in mod.state_dict().items() if "running" in k])
    bitwise = all(torch.equal(a, b) for a, b in zip(*res))
    print(f"[ragged == dense at equal lengths] bitwise: {bitwise}")
    close(res[1][0].cpu(), res[0][0].cpu(), 1e-5, "out")
    for i, (a, b) in enumerate(zip(res[0][1:], res[1][1:])):
        close(b.cpu(), a.cpu(), 1e-4, f"gradient / state {i}")


def _series_rows(lens, C, gen, m=None):
    n = _soff(lens, m)[1]
    return [torch.randn(k, C, generator=gen) for k in n]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["A", "B"])
def test_ops_vs_per_series_torch(cuda, tag):
    """Every ragged op, forward and backward, against torch's own op on each
    series alone in fp64; NaN in the dead tail of every input buffer, zeros in
    the dead tail of every output."""
    from hlhgat import ops
    lens = LENS[tag]
    tm = ops.time_series_map(_lens(lens, cuda), T_MAX, POOL)
    T2 = tm.t_max[1]
    so0, l0 = _soff(lens)
    so1, l1 = _soff(lens, POOL)
    torch.cuda.synchronize()
    # the tables themselves
    for i, (so, ln, cap) in enumerate(((so0, l0, S * T_MAX), (so1, l1, S * T2))):
        assert tm.soff[i].cpu().tolist() == so.tolist() and int(tm.n_rows[i]) == so[-1]
        tab = np.zeros((cap, 2), dtype=np.int64)
        sid = np.zeros(cap, dtype=np.int64)
        for s, n in enumerate(ln):
            tab[so[s]:so[s] + n, 0], tab[so[s]:so[s] + n, 1], sid[so[s]:so[s] + n] = np.arange(n), n, s
        assert np.array_equal(tm.tab[i].cpu().numpy(), tab)
        assert np.array_equal(tm.sid[i].cpu().numpy(), sid)
    gen = torch.Generator().manual_seed(11)

    def check(got, want_rows, so, tol, what):
        n = so[-1]
        assert torch.isfinite(got[:n]).all(), what
        assert not got[n:].any(), what + ": dead rows"
        close(got[:n].cpu(), torch.cat(want_rows), tol, what)

    def run(ragged_fn, ref_fn, rows_in, params, so_in, so_out, cap_in, cap_out, what,
            per_series_out=True):
        C_in = rows_in[0].shape[1]
        x = _compact(rows_in, cap_in).to(cuda)
        leaves = [x.requires_grad_(True)] + [p.detach().clone().requires_grad_(True)
                                             for p in params]
        out = ragged_fn(*leaves)
        p64 = [p.detach().cpu().double().requires_grad_(True) for p in params]
        r64 = [r.double().requires_grad_(True) for r in rows_in]
        want = [ref_fn(r.t().unsqueeze(0), *p64) for r in r64]  # [1, C, len]
        if per_series_out:
            want_rows = [w[0].t() for w in want]
            gy_rows = [torch.randn(w.shape, generator=gen) for w in want_rows]
            gy = _compact(gy_rows, cap_out).to(cuda)
            check(out.detach(), [w.detach() for w in want_rows], so_out, 1e-5, what)
        else:
            want_rows = want  # [1, 2C] per series
            gy_rows = [torch.randn(w.shape, generator=gen) for w in want_rows]
            gy = torch.cat(gy_rows).to(cuda)
            assert torch.isfinite(out).all()
            close(out.detach().cpu(), torch.cat([w.detach() for w in want]), 1e-5, what)
        out.backward(gy)
        sum((w * g.double()).sum() for w, g in zip(want_rows, gy_rows)).backward()
        check(leaves[0].grad, [r.grad for r in r64], so_in, 1e-4, what + " grad_x")
        assert leaves[0].grad.shape == (cap_in, C_in)
        for i, (a, b) in enumerate(zip(leaves[1:], p64)):
            close(a.grad.cpu(), b.grad, 1e-4, f"{what} grad param {i}")

    def conv_ref(h, *p):
        nb = len(p) // 2
        return torch.cat([F.conv1d(h, w, b, padding=w.shape[2] // 2)
                          for w, b in zip(p[:nb], p[nb:])], dim=1)

    for stage, (so, cap, m) in enumerate(((so0, S * T_MAX, None), (so1, S * T2, POOL))):
        ws, bs = _branch_params(cuda, CH, seed=stage)
        run(lambda h, *p: ops.temporal_conv_ragged(h, tm, stage, p[:3], p[3:]), conv_ref,
            _series_rows(lens, CH, gen, m), ws + bs, so, so, cap, cap, f"conv stage {stage}")
    we, be = _branch_params(cuda, 1, (CH,), (5,))
    run(lambda h, w, b: ops.temporal_conv_ragged(h, tm, 0, [w], [b]), conv_ref,
        _series_rows(lens, 1, gen), we + be, so0, so0, S * T_MAX, S * T_MAX, "embedding")
    run(lambda h: ops.leaky_maxpool_time_ragged(h, tm, SLOPE),
        lambda h: F.max_pool1d(F.leaky_relu(h, SLOPE), POOL, stride=POOL - 1,
                               padding=(POOL - 1) // 2),
        _series_rows(lens, CH, gen), [], so0, so1, S * T_MAX, S * T2, "pool")
    run(lambda h: ops.time_readout_ragged(h, tm, SLOPE),
        lambda h: torch.cat([F.leaky_relu(h, SLOPE).max(dim=-1)[0],
                             F.leaky_relu(h, SLOPE).mean(dim=-1)], dim=-1),
        _series_rows(lens, 4 * NCH, gen, POOL), [], so1, None, S * T2, None, "readout",
        per_series_out=False)
    # pack: NaN past every length is never read; its gradient is 0 there
    x = _x(lens, cuda).requires_grad_(True)
    xc = ops.time_series_pack(x, tm)
    check(xc.detach(), [T_(_g()["x"])[s, :n].reshape(-1, 1) for s, n in enumerate(lens)], so0, 0.0,
          "pack")
    gy = _compact(_series_rows(lens, 1, gen), S * T_MAX).to(cuda)
    xc.backward(gy)
    for s, n in enumerate(lens):
        assert torch.equal(x.grad[s, :n], gy[so0[s]:so0[s] + n, 0]) and not x.grad[s, n:].any()
    ops.check_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("keep", [1, 4])
def test_series_isolation(cuda, keep):
    """4. Same lengths, other data in every series but one: that series'
    convolution rows before the BatchNorm, and its pooled, convolved and read
    out rows given the same BatchNorm output, keep their bits (series 1 of A
    ends on the tile edge at row 64; series 4 starts 3 rows into a tile)."""
    from hlhgat import ops
    lens = LENS["A"]
    mod = _module(cuda)
    tm = ops.time_series_map(_lens(lens, cuda), T_MAX, POOL)
    so0, _ = _soff(lens)
    so1, _ = _soff(lens, POOL)
    r0 = slice(so0[keep], so0[keep + 1])
    r1 = slice(so1[keep], so1[keep + 1])
    gen = torch.Generator().manual_seed(21)

    def front(x):
        h = ops.time_series_pack(x, tm)
        h = ops.temporal_conv_ragged(h, tm, 0, [mod.embedding.weight], [mod.embedding.bias])
        cs = [mod.channel1_1, mod.channel2_1, mod.channel3_1]
        return ops.temporal_conv_ragged(h, tm, 0, [c.weight for c in cs], [c.bias for c in cs])

    def back(h):  # from a BatchNorm output on
        p = ops.leaky_maxpool_time_ragged(h, tm, SLOPE)
        cs = [mod.channel1_2, mod.channel2_2, mod.channel3_2]
        c = ops.temporal_conv_ragged(p, tm, 1, [c.weight for c in cs], [c.bias for c in cs])
        return p, c, ops.time_readout_ragged(c, tm, SLOPE)

    with torch.no_grad():
        x = _x(lens, cuda)
        x2 = (3.0 * torch.randn(S, T_MAX, generator=gen) - 1.0).to(cuda)
        x2[keep] = x[keep]
        for s, n in enumerate(lens):
            x2[s, n:] = NAN
        a, b = front(x), front(x2)
        assert torch.isfinite(a[r0]).all() and torch.equal(a[r0], b[r0])
        assert not torch.equal(a[:so0[-1]], b[:so0[-1]])
        h = _compact(_series_rows(lens, CH, gen), S * T_MAX).to(cuda)
        h2 = _compact(_series_rows(lens, CH, gen), S * T_MAX).to(cuda)
        h2[r0] = h[r0]
        (pa, ca, ya), (pb, cb, yb) = back(h), back(h2)
        assert torch.isfinite(pa[r1]).all() and torch.equal(pa[r1], pb[r1])
        assert torch.isfinite(ca[r1]).all() and torch.equal(ca[r1], cb[r1])
        assert torch.isfinite(ya).all() and torch.equal(ya[keep], yb[keep])
        assert not torch.equal(ya, yb)


@pytest.mark.gpu
def test_deterministic(cuda):
    """5. Two runs of forward + backward on B: the same bits."""
    a, b = _train_run(cuda, "B"), _train_run(cuda, "B")
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_fc_prepare_windows(cuda):
    """6a. z of graph g is hlhgat_fc_prepare of that graph alone with its own
    (t0, len), bit for bit, and 0 past len; the workspace rows too."""
    from hlhgat import ops
    g = load_golden("brainfc_G3N37T70")
    x = T_(g["x"]).to(cuda)
    G, N, T = x.shape
    wins = [(0, 70), (5, 33), (12, 50)]
    t0 = torch.tensor([w[0] for w in wins], dtype=torch.int32, device=cuda)
    ln = torch.tensor([w[1] for w in wins], dtype=torch.int32, device=cuda)
    z = torch.full((G * N, T), NAN, device=cuda)
    prep = ops.fc_prepare(x.view(G * N, T), G, windows=(t0, ln), t_max=T, z=z)
    fc = ops.fc_dense(prep)
    for k, (b, n) in enumerate(wins):
        one = ops.fc_prepare(x[k], 1, window=(b, n))
        zk = prep.z[k * N:(k + 1) * N]
        assert torch.isfinite(zk).all() and torch.equal(zk[:, :n], one.z)
        assert not zk[:, n:].any()
        close(fc[k].cpu(), ops.fc_dense(one)[0].cpu(), 4e-6, f"fc of graph {k}")
    ops.check_device_errors()
    # a window that leaves the row is clamped and reported, nothing is read out of bounds
    ops.clear_device_errors()
    bad = ops.fc_prepare(x.view(G * N, T), G, windows=(t0 + 30, ln), t_max=T)
    torch.cuda.synchronize()
    assert torch.isfinite(bad.z).all()
    assert ops.device_errors() & ops._lib.DEVERR_TSERIES_LEN
    ops.clear_device_errors()


def _tiny_pipe():
    from test_brain_train import _pipe
    return _pipe()[0]


WINDOWS = (np.array([[0, 23], [2, 20]]), np.array([[1, 26], [3, 17]]), np.array([[4, 23], [0, 27]]))
SUBJECTS = ([0, 1], [3, 1], [2, 3])


@pytest.mark.gpu
def test_pipeline_per_sample_vs_cpu(cuda):
    """6b. x_t and x_s of per-sample windows against the CPU path, at the
    tolerances tests/test_brain_fc.py applies to the same two quantities."""
    from hlhgat import ops
    pipe = _tiny_pipe()
    assert pipe.t_max == 27
    for idx, w in zip(SUBJECTS, WINDOWS):
        got = pipe.batch(idx, window=w, device=cuda)
        cpu = pipe.batch(idx, window=w, device="cpu")
        assert got[0].x_t.shape == cpu[0].x_t.shape == (2 * pipe.N, 27)
        assert got[0].t_len.dtype == torch.int32 and torch.equal(got[0].t_len.cpu(), cpu[0].t_len)
        assert float((got[0].x_t.cpu() - cpu[0].x_t).abs().max()) <= 1e-5
        assert float((got[0].x_s.cpu() - cpu[0].x_s).abs().max()) <= 4e-6
        assert torch.equal(got[0].y.cpu(), cpu[0].y)
    ops.check_device_errors()


@pytest.mark.gpu
def test_one_capture_for_every_window(cuda):
    """7. Three batches of 2 subjects with different per-sample windows are
    ONE captured graph, and the replayed steps equal the eager ones bit for
    bit; the same three batches with a window per batch are three graphs."""
    from hlhgat import ops
    from test_brain_train import _train_step
    pipe = _tiny_pipe()
    runs = {}
    for graphs in (False, True):
        step = _train_step(cuda, graphs)
        losses = []
        for i in range(6):
            b = pipe.batch(SUBJECTS[i % 3], window=WINDOWS[i % 3], device=cuda)
            losses.append(step(b).clone())
        runs[graphs] = (losses, {k: v.detach().clone()
                                 for k, v in step.model.state_dict().items()}, dict(step.stats))
        if graphs:
            assert len(step._graphs) == 1
    assert runs[True][2] == {"eager": 1, "captures": 1, "replay": 5}
    for i, (a, b) in enumerate(zip(runs[False][0], runs[True][0])):
        assert torch.isfinite(a) and torch.equal(a, b), (i, float(a), float(b))
    for k in runs[False][1]:
        assert torch.equal(runs[False][1][k], runs[True][1][k]), k
    assert len({float(v) for v in runs[True][0]}) == 6  # the windows matter
    # drawn per batch, every length is a shape of its own
    step = _train_step(cuda, True)
    for idx, w in zip(SUBJECTS, WINDOWS):
        step(pipe.batch(idx, window=(int(w[0, 0]), int(w[:, 1].min())), device=cuda))
    assert len(step._graphs) == 3
    ops.check_device_errors()


@pytest.mark.gpu
def test_bad_lengths_are_clamped_and_reported(cuda):
    """8. A length of 0 and one of t_max + 1 are clamped to 1 and t_max and
    raise the device error word; the run finishes with finite outputs."""
    from hlhgat import ops, _lib
    mod = _module(cuda)
    lens = list(RR.LENS_A)
    lens[2], lens[4] = 0, T_MAX + 1
    x = _x([1 if n == 0 else min(n, T_MAX) for n in lens], cuda)
    ops.check_device_errors()
    with torch.no_grad():
        out = mod(x, _lens(lens, cuda))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and out.shape == (S, 8 * NCH)
    assert ops.device_errors() & _lib.DEVERR_TSERIES_LEN
    with pytest.raises(RuntimeError, match="clamped"):
        ops.check_device_errors()
    ops.clear_device_errors()
    ok = list(RR.LENS_A)
    ok[2], ok[4] = 1, T_MAX
    with torch.no_grad():
        want = mod(x, _lens(ok, cuda))
    assert torch.equal(out, want)
    ops.check_device_errors()
