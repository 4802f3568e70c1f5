"""The DEMO brain model: Inception1D (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:
474-515) on the temporal HIP kernels (csrc/tconv.hip) and HL_HGAT_attpool
(:250-399).

Fixtures: tests/golden/make_golden_brainhead.py ran the REFERENCE's classes on
the CPU.  brain_ref.py restates both on oracle.hodge_ref (fp32 / fp64).

* CPU: brain_ref reproduces every fixture; the product Inception1D on CPU
  tensors does too; state_dict keys, their order and a strict load agree; the
  checkpoint-shaped head has the published checkpoint's 346 entries; every new
  C-ABI entry rejects bad arguments without a GPU.  (The product head has no
  CPU arithmetic -- NodeEdgeInt and the Hodge convs are HIP only -- so its
  numbers are checked on the GPU.)
* GPU (-m gpu): temporal_conv alone vs fp64, series isolation, Inception1D vs
  the fixtures, determinism, no foreign kernels, the head.

Tolerances: conftest.close at 1e-5 for a layer's outputs, 1e-4 for gradients
and whole-head outputs; parameter gradients of the head through
test_baseline_configs._grad_gate.
"""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brain_ref as B
from conftest import close, load_golden
from test_baseline_configs import _cond, _grad_gate, _perturb

T_ = torch.from_numpy
GRAD_CASES = ["inception1d_c64n8m3_N7T23", "inception1d_c16n4m5_N7T23",
              "inception1d_c12n3m3_N5T9", "inception1d_c64n8m3_N3T64"]
LONG, EVAL, HEAD = ("inception1d_c64n8m3_N3T375", "inception1d_c16n4m5_N7T23_eval",
                    "brain_head_small")
HEAD_KW = dict(channels=[1, 1], filters=[8, 16], mlp_channels=[12], K=3, pool_num=1)
CKPT_KW = dict(channels=[2, 2, 2], filters=[32, 64, 128], mlp_channels=[], K=4, pool_num=1,
               num_nodepedge=2815)
KEYS = ("x_t", "x_s", "edge_index_t", "edge_weight_t", "edge_index_s", "edge_weight_s",
        "edge_index", "num_node1", "num_edge1")


def _cfg(name):
    c, n, m = re.match(r"inception1d_c(\d+)n(\d+)m(\d+)_", name).groups()
    return int(c), int(n), int(m)


def _sd(g, dtype=None):
    sd = {k[3:]: T_(np.asarray(g[k])) for k in g if k.startswith("sd/")}
    if dtype is not None:
        sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    return sd


def _sd_keys(g):
    return [k[3:] for k in g if k.startswith("sd/")]


def _bn_fed(k):
    return re.search(r"channel\d_\d\.bias$", k) is not None


def _check_inception_grads(mod, x, g):
    close(x.grad.cpu(), g["grad_x"], 1e-4, "grad_x")
    for k, p in mod.named_parameters():
        ref = np.asarray(g["grad/" + k], dtype=np.float64)
        got = p.grad.detach().cpu().double().reshape(-1).numpy()
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(ref - got).max())
        if _bn_fed(k):  # analytically zero: rounding noise
            assert float(np.abs(got).max()) < 1e-3 * scale, k
        else:
            assert err <= 1e-4 * scale, (k, err, scale)


def _run_inception(cls, name, g, device="cpu", dtype=torch.float32, readout=True):
    C, n, m = _cfg(name)
    mod = cls(C, n, m, if_readout=readout)
    assert list(mod.state_dict().keys()) == _sd_keys(g)
    mod.load_state_dict(_sd(g), strict=True)
    mod = mod.to(device=device, dtype=dtype).train()
    x = T_(g["x"]).to(device=device, dtype=dtype).requires_grad_(True)
    return mod, x, mod(x)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.fixture
def one_thread():
    nt = torch.get_num_threads()
    torch.set_num_threads(1)  # the generator's CPU reduction order
    yield
    torch.set_num_threads(nt)


@pytest.mark.parametrize("cls", ["ref", "product"])
@pytest.mark.parametrize("name", GRAD_CASES)
def test_inception_cpu_reproduces_fixture(name, cls, one_thread):
    import hlhgat
    g = load_golden(name)
    klass = B.RefInception1D if cls == "ref" else hlhgat.Inception1D
    mod, x, out = _run_inception(klass, name, g)
    close(out.detach(), g["out"], 1e-5, "out")
    (out * T_(g["R"])).sum().backward()
    _check_inception_grads(mod, x, g)


@pytest.mark.parametrize("cls", ["ref", "product"])
def test_inception_cpu_forward_only_fixtures(cls, one_thread):
    import hlhgat
    klass = B.RefInception1D if cls == "ref" else hlhgat.Inception1D
    g = load_golden(LONG)
    for readout, key in ((True, "out_readout"), (False, "out_series")):
        with torch.no_grad():
            _, _, out = _run_inception(klass, LONG, g, readout=readout)
        close(out, g[key], 1e-5, key)
    g = load_golden(EVAL)
    mod = klass(*_cfg(EVAL), if_readout=True)
    mod.load_state_dict(_sd(g), strict=True)
    with torch.no_grad():
        close(mod.eval()(T_(g["x"])), g["out"], 1e-5, "eval out")


class _D:
    pass


def _datas(g, dtype=torch.float32, device=None):
    out = []
    for lv in (0, 1):
        d = _D()
        for k in KEYS:
            v = T_(g[f"l{lv}/{k}"])
            if v.is_floating_point():
                v = v.to(dtype)
            setattr(d, k, v if device is None else v.to(device))
        out.append(d)
    for k in ("pos_t", "pos_s"):
        v = T_(g[k]).to(dtype)
        setattr(out[0], k, v if device is None else v.to(device))
    return out


def _head_kw(g):
    return dict(HEAD_KW, num_nodepedge=int(g["sd/mlp0.0.weight"].shape[1]))


def _run_ref_head(g, dtype, eps=0.0, pseed=0, train=True):
    m = B.RefBrainHead(**_head_kw(g))
    m.load_state_dict(_sd(g), strict=True)
    m = m.to(dtype).train(train)
    _perturb(m, eps, pseed)
    outs = m(_datas(g, dtype))
    if train:
        (outs[0] * T_(g["R"]).to(dtype)).sum().backward()
    return m, [o.detach() for o in outs]


def test_ref_head_reproduces_fixture(one_thread):
    g = load_golden(HEAD)
    m, (out, latent, node_att, edge_att) = _run_ref_head(g, torch.float32)
    close(out, g["out"], 1e-5, "out")
    close(latent, g["latent"], 1e-5, "latent")
    close(node_att, g["node_att"], 1e-5, "node_att")
    close(edge_att, g["edge_att"], 1e-5, "edge_att")
    for k, p in m.named_parameters():
        assert "nograd/" + k not in g and p.grad is not None, k
        ref = np.asarray(g["grad/" + k], dtype=np.float64)
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(ref - p.grad.double().reshape(-1).numpy()).max())
        assert err <= 1e-4 * scale, (k, err, scale)


def test_product_head_state_dict_matches_fixture_and_checkpoint():
    import hlhgat
    g = load_golden(HEAD)
    m = hlhgat.HL_HGAT_attpool(**_head_kw(g))
    assert list(m.state_dict().keys()) == _sd_keys(g)
    m.load_state_dict(_sd(g), strict=True)
    man = load_golden("brain_ckpt_manifest")
    m = hlhgat.HL_HGAT_attpool(**CKPT_KW)
    sd = m.state_dict()
    names = [str(s) for s in man["names"]]
    assert len(names) == 346 and list(sd.keys()) == names
    for i, k in enumerate(names):
        shape = tuple(int(v) for v in man["shapes"][i] if v >= 0)
        assert tuple(sd[k].shape) == shape, k
        assert str(sd[k].dtype) == str(man["dtypes"][i]), k
    assert sum(v.numel() for v in sd.values()) == int(man["numel"]) == 859722


def test_head_rejects_graphs_of_different_sizes():
    import hlhgat
    g = load_golden(HEAD)
    m = hlhgat.HL_HGAT_attpool(**_head_kw(g))
    datas = _datas(g)
    datas[0].num_node1 = datas[0].num_node1.clone()
    datas[0].num_node1[0] += 1
    with pytest.raises(ValueError, match="same number of nodes"):
        m(datas, device="cpu")
    with pytest.raises(ValueError, match="levels"):
        m(datas[:1], device="cpu")


def test_capi_rejects_bad_arguments():
    """Every new entry validates on the host before any HIP call: even taps,
    taps > 5, T < 1, C < 1 and null pointers give HLHGAT_EINVAL and a message
    (runs without a GPU)."""
    import ctypes as C
    from hlhgat import _lib
    L = _lib.LIB
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    vp1 = (C.c_void_p * 1)(p.value)
    co1 = (C.c_int64 * 1)(4)
    tb = lambda t: (C.c_int32 * 1)(t)  # noqa: E731

    def pack(taps=5, cin=4, w=vp1, out=p):
        return L.hlhgat_tconv_pack(1, w, co1, tb(1), cin, taps, 0, out, None)

    def fwd(t=5, cin=4, cout=4, taps=5, x=p, w=p, y=p):
        return L.hlhgat_tconv_fwd(x, 1, t, cin, w, None, cout, taps, 0, 0, y, None)

    def embed(t=5, c=4, taps=5, x=p, w=p, y=p):
        return L.hlhgat_tconv_embed_fwd(x, 1, t, w, None, c, taps, y, None)

    def wgrad(t=5, cin=4, cout=4, taps=5, x=p, dy=p, dw=vp1, ws=p):
        return L.hlhgat_tconv_bwd_weight(x, dy, 1, t, cin, cout, taps, 1, dw, co1,
                                         tb(taps if taps in (1, 3, 5) else 1), None, ws, 4096,
                                         None)

    def pool_f(t=5, c=4, x=p, y=p, idx=p):
        return L.hlhgat_leaky_maxpool_time_fwd(x, 1, t, c, 3, 0.1, y, idx, None)

    def pool_b(t=5, c=4, x=p, dy=p, idx=p, dx=p):
        return L.hlhgat_leaky_maxpool_time_bwd(x, dy, idx, 1, t, c, 3, 0.1, dx, None)

    def ro_f(t=5, c=4, x=p, y=p, idx=p):
        return L.hlhgat_time_readout_fwd(x, 1, t, c, 0.1, y, idx, None)

    def ro_b(t=5, c=4, x=p, dy=p, idx=p, dx=p):
        return L.hlhgat_time_readout_bwd(x, dy, idx, 1, t, c, 0.1, dx, None)

    def bad(rc, word):
        assert rc == 1, (rc, word)
        msg = L.hlhgat_last_error()
        assert msg and word.encode() in msg, (msg, word)

    for fn in (pack, fwd, embed, wgrad):  # taps
        bad(fn(taps=4), "taps")
        bad(fn(taps=2), "taps")
        bad(fn(taps=7), "taps")
    for fn in (fwd, embed, wgrad, pool_f, pool_b, ro_f, ro_b):  # T < 1
        bad(fn(t=0), "T")
    for fn in (pool_f, pool_b, ro_f, ro_b, embed):  # C < 1
        bad(fn(c=0), "C")
    for fn in (pack, fwd, wgrad):
        bad(fn(cin=0), "C")
    for fn in (fwd, wgrad):
        bad(fn(cout=0), "C")
    bad(pack(w=None), "NULL")
    bad(pack(out=None), "NULL")
    for kw in ({"x": None}, {"w": None}, {"y": None}):
        bad(fwd(**kw), "NULL")
        bad(embed(**kw), "NULL")
    for kw in ({"x": None}, {"dy": None}, {"dw": None}, {"ws": None}):
        bad(wgrad(**kw), "NULL")
    for kw in ({"x": None}, {"y": None}, {"idx": None}):
        bad(pool_f(**kw), "NULL")
        bad(ro_f(**kw), "NULL")
    for kw in ({"x": None}, {"dy": None}, {"idx": None}, {"dx": None}):
        bad(pool_b(**kw), "NULL")
        bad(ro_b(**kw), "NULL")
    assert L.hlhgat_tconv_bwd_weight_workspace_floats(1, 5, 4, 4, 4) == 0
    assert L.hlhgat_tconv_bwd_weight_workspace_floats(1, 5, 4, 4, 5) >= 5 * 4 * 4 + 4
    assert [L.hlhgat_maxpool_time_len(t, m) for t, m in ((23, 3), (375, 3), (23, 5), (1, 3))] \
        == [12, 188, 6, 1]
    assert L.hlhgat_version() >= 102


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
CONV_SHAPES = [(1, 5, 4, 4, 5),      # T shorter than a tile and equal to the tap count
               (7, 23, 64, 64, 5),   # tiles straddle series boundaries
               (3, 64, 64, 32, 5),   # T a multiple of the tile
               (5, 9, 12, 12, 5),    # ragged channels
               (3, 375, 64, 64, 5),
               (7, 23, 1, 16, 5)]    # the embedding


@pytest.mark.gpu
@pytest.mark.parametrize("N,T,cin,cout,taps", CONV_SHAPES)
def test_temporal_conv_vs_fp64(cuda, N, T, cin, cout, taps):
    """forward, data, weight and bias gradient within 3x the error of torch's
    fp32 CPU conv1d against the same fp64 result (floor 1e-5)."""
    from hlhgat import ops
    gen = torch.Generator().manual_seed(N * 1000 + T)
    x = torch.randn(N, T, cin, generator=gen)
    w = torch.randn(cout, cin, taps, generator=gen) / np.sqrt(cin * taps)
    b = torch.randn(cout, generator=gen)
    R = torch.randn(N, T, cout, generator=gen)

    def cpu(dtype):
        xs, ws, bs = (t.detach().clone().to(dtype).requires_grad_(True) for t in (x, w, b))
        y = F.conv1d(xs.transpose(1, 2), ws, bs, padding=taps // 2).transpose(1, 2)
        (y * R.to(dtype)).sum().backward()
        return [t.detach().double() for t in (y, xs.grad, ws.grad, bs.grad)]

    r64, r32 = cpu(torch.float64), cpu(torch.float32)
    xs, ws, bs = (t.detach().clone().to(cuda).requires_grad_(True) for t in (x, w, b))
    y = ops.temporal_conv(xs, ws, bs)
    (y * R.to(cuda)).sum().backward()
    for what, got, e64, e32 in zip(("y", "dx", "dw", "db"), (y, xs.grad, ws.grad, bs.grad),
                                   r64, r32):
        scale = max(1.0, float(e64.abs().max()))
        err32 = float((e32 - e64).abs().max()) / scale
        err = float((got.detach().cpu().double() - e64).abs().max()) / scale
        print(f"[tconv {N}x{T}x{cin}->{cout}] {what}: err {err:.2e} fp32-cpu {err32:.2e}")
        close(got.detach().cpu(), e64, max(3 * err32, 1e-5), what)
    ops.check_device_errors()


@pytest.mark.gpu
def test_series_isolation(cuda):
    """Replacing one series changes no other series' output bit: a tile that
    crosses a series boundary reads zeros, not its neighbour."""
    import hlhgat
    torch.manual_seed(5)
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(7, 23, generator=gen)
    x2 = x.clone()
    x2[3] = 5.0 * torch.randn(23, generator=gen) + 1.0
    keep = [0, 1, 2, 4, 5, 6]
    for readout in (True, False):
        m = hlhgat.Inception1D(64, 8, 3, if_readout=readout).to(cuda).eval()
        with torch.no_grad():
            a, b = m(x.to(cuda)), m(x2.to(cuda))
        assert torch.equal(a[keep], b[keep])
        assert not torch.equal(a[3], b[3])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_CASES)
def test_inception_vs_fixture(cuda, name):
    import hlhgat
    from hlhgat import ops
    g = load_golden(name)
    mod, x, out = _run_inception(hlhgat.Inception1D, name, g, device=cuda)
    close(out.detach().cpu(), g["out"], 1e-5, "out")
    (out * T_(g["R"]).to(cuda)).sum().backward()
    _check_inception_grads(mod, x, g)
    ops.check_device_errors()


@pytest.mark.gpu
def test_inception_forward_only_fixtures(cuda):
    import hlhgat
    g = load_golden(LONG)
    for readout, key in ((True, "out_readout"), (False, "out_series")):
        with torch.no_grad():
            _, _, out = _run_inception(hlhgat.Inception1D, LONG, g, device=cuda, readout=readout)
        close(out.cpu(), g[key], 1e-5, key)
    g = load_golden(EVAL)
    mod = hlhgat.Inception1D(*_cfg(EVAL), if_readout=True)
    mod.load_state_dict(_sd(g), strict=True)
    mod = mod.to(cuda).eval()
    with torch.no_grad():
        close(mod(T_(g["x"]).to(cuda)).cpu(), g["out"], 1e-5, "eval out")
    # eval mode inside a differentiated graph (running statistics, autograd on)
    x = T_(g["x"]).to(cuda).requires_grad_(True)
    out = mod(x)
    close(out.detach().cpu(), g["out"], 1e-5, "eval out (grad mode)")
    out.sum().backward()
    assert torch.isfinite(x.grad).all()


@pytest.mark.gpu
def test_inception_is_deterministic(cuda):
    import hlhgat
    g = load_golden(GRAD_CASES[0])
    runs = []
    for _ in range(2):
        mod, x, out = _run_inception(hlhgat.Inception1D, GRAD_CASES[0], g, device=cuda)
        (out * T_(g["R"]).to(cuda)).sum().backward()
        runs.append([out.detach(), x.grad] + [p.grad for p in mod.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_inception_runs_no_foreign_kernels(cuda, monkeypatch):
    import hlhgat
    g = load_golden(GRAD_CASES[1])

    def boom(*a, **k):
        raise AssertionError("torch convolution / pooling called on the HIP path")

    monkeypatch.setattr(F, "conv1d", boom)
    monkeypatch.setattr(torch, "conv1d", boom)
    monkeypatch.setattr(F, "max_pool1d", boom)
    C, n, m = _cfg(GRAD_CASES[1])
    mod = hlhgat.Inception1D(C, n, m, if_readout=True)
    mod.load_state_dict(_sd(g), strict=True)
    mod = mod.to(cuda).train()
    for sub in mod.modules():
        if isinstance(sub, (torch.nn.Conv1d, torch.nn.MaxPool1d)):
            sub.register_forward_hook(boom)
            sub.register_forward_pre_hook(boom)
    x = T_(g["x"]).to(cuda).requires_grad_(True)
    out = mod(x)
    (out * T_(g["R"]).to(cuda)).sum().backward()
    close(out.detach().cpu(), g["out"], 1e-5, "out")
    close(x.grad.cpu(), g["grad_x"], 1e-4, "grad_x")


@pytest.mark.gpu
def test_head_vs_fixture_and_fp64(cuda):
    import hlhgat
    from hlhgat import ops
    from hlhgat.train import InferStep
    g = load_golden(HEAD)
    m = hlhgat.HL_HGAT_attpool(**_head_kw(g))
    m.load_state_dict(_sd(g), strict=True)
    m = m.to(cuda).train()
    ops.clear_caches()
    out, latent, node_att, edge_att = m(_datas(g, device=cuda), device=cuda)
    m32, _ = _run_ref_head(g, torch.float32)
    m64, o64 = _run_ref_head(g, torch.float64)
    for what, got, ref64 in zip(("out", "latent", "node_att", "edge_att"),
                                (out, latent, node_att, edge_att), o64):
        close(got.detach().cpu(), g[what], 1e-4, what + " vs reference")
        close(got.detach().cpu(), ref64, 1e-4, what + " vs fp64 restatement")
    (out * T_(g["R"]).to(cuda)).sum().backward()
    cond = _cond(m64, [_run_ref_head(g, torch.float64, 1e-6, s)[0] for s in (0, 1)])
    _grad_gate(m, m32, m64, g, cond, case="cond_brain_head_small")
    ops.check_device_errors()
    # eval mode through InferStep, eagerly (fresh running statistics)
    m.load_state_dict(_sd(g), strict=True)
    step = InferStep(m, graphs=False)
    ops.clear_caches()
    ev = step(_datas(g, device=cuda))
    _, e64 = _run_ref_head(g, torch.float64, train=False)
    for what, got, ref64 in zip(("out", "latent", "node_att", "edge_att"), ev, e64):
        close(got.cpu(), ref64, 1e-4, "eval " + what)
    ops.check_device_errors()
