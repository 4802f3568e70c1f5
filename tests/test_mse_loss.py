"""The MSE loss on HIP (csrc/loss.hip: hlhgat_mse_loss_fwd / _bwd,
ops.mse_loss, hlhgat.nn.MSELoss): the brain notebook's training criterion
(HL-HGAT-DEMO/OHBM_DEMO.ipynb, ``criterion = torch.nn.MSELoss()``).

Bounds of the GPU test, against the same formulas in fp64 on the same fp32
inputs, u = 2^-24:
  loss: (n + 4) u |loss|.  Every term (x_i - y_i)^2 carries 3 roundings (the
    subtraction counts twice through the square, the product once), an n-term
    sum of non-negative terms in any order n - 1, the division 1.
  dx_i: 4 u |dx_i|.  The subtraction, the scalar 2 g / div and the product
    each round once (2 g is exact).
"""
import ctypes as C
import inspect

import pytest
import torch

U = 2.0 ** -24
SIZES = [1, 5, 255, 256, 257, 4099]  # below / at / above one pass of the 256 threads, ragged


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_library_exports_mse_entries():
    from hlhgat import _lib
    from hlhgat._lib import c_f32, c_i32, c_i64, c_vp
    fwd, bwd = _lib.LIB.hlhgat_mse_loss_fwd, _lib.LIB.hlhgat_mse_loss_bwd
    # (x, y, n, div, loss, stream) and (x, y, n, div, gout, dx, stream)
    assert fwd.restype is c_i32 and list(fwd.argtypes) == [c_vp, c_vp, c_i64, c_f32, c_vp, c_vp]
    assert bwd.restype is c_i32 and list(bwd.argtypes) == [c_vp, c_vp, c_i64, c_f32, c_vp, c_vp,
                                                          c_vp]
    assert _lib.LIB.hlhgat_version() >= 106


def test_capi_rejects_bad_arguments():
    """The argument error and a message before any launch (runs without a GPU)."""
    from hlhgat import _lib
    L = _lib.LIB
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value

    def fwd(x=p, y=p, n=4, div=4.0, loss=p):
        return L.hlhgat_mse_loss_fwd(x, y, n, div, loss, None)

    def bwd(x=p, y=p, n=4, div=4.0, gout=p, dx=p):
        return L.hlhgat_mse_loss_bwd(x, y, n, div, gout, dx, None)

    def bad(rc, word):
        assert rc == 1, (rc, word)
        msg = L.hlhgat_last_error()
        assert msg and word.encode() in msg, (msg, word)

    for fn, name in ((fwd, "mse_loss_fwd"), (bwd, "mse_loss_bwd")):
        for kw in ({"x": None}, {"y": None}, {"n": 0}, {"n": -3}, {"div": 0.0}, {"div": -1.0},
                   {"div": float("nan")}):
            bad(fn(**kw), name)
    bad(fwd(loss=None), "mse_loss_fwd")
    bad(bwd(gout=None), "mse_loss_bwd")
    bad(bwd(dx=None), "mse_loss_bwd")


def test_module_on_cpu_is_torch_bitwise():
    import hlhgat
    assert "MSELoss" in hlhgat.nn.__all__ and hlhgat.MSELoss is hlhgat.nn.MSELoss
    assert issubclass(hlhgat.nn.MSELoss, torch.nn.MSELoss)
    assert list(inspect.signature(hlhgat.ops.mse_loss).parameters) == ["input", "target",
                                                                       "reduction"]
    gen = torch.Generator().manual_seed(3)
    for shape in ((7,), (5, 1), (3, 4)):
        for red in ("mean", "sum", "none"):
            y = torch.randn(shape, generator=gen)
            res = []
            for crit in (torch.nn.MSELoss(reduction=red), hlhgat.nn.MSELoss(reduction=red)):
                x = torch.randn(shape, generator=torch.Generator().manual_seed(4))
                x.requires_grad_(True)
                loss = crit(x, y)
                loss.sum().backward()
                res.append((loss.detach(), x.grad))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_ops_have_no_cpu_fallback():
    from hlhgat import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.mse_loss(torch.randn(4), torch.randn(4))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _inputs(n, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=gen) * 3.0 + 0.5
    y = torch.randn(n, generator=gen)
    same = torch.arange(n) % 4 == 1  # some x_i == y_i
    x[same] = y[same]
    return x, y, same


@pytest.mark.gpu
@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("n", SIZES)
def test_mse_vs_fp64(cuda, n, reduction):
    import hlhgat
    from hlhgat import ops
    x, y, same = _inputs(n, 100 + n)
    g = 3.0
    div = float(n) if reduction == "mean" else 1.0
    d64 = x.double() - y.double()
    loss64 = float((d64 * d64).sum() / div)
    dx64 = d64 * (2.0 * g / div)

    def run(crit):
        xd = x.to(cuda).requires_grad_(True)
        loss = crit(xd, y.to(cuda))
        loss.backward(torch.tensor(g, device=cuda))
        return loss.detach().cpu(), xd.grad.cpu()

    loss, dx = run(hlhgat.nn.MSELoss(reduction=reduction))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and dx.shape == x.shape
    err = abs(float(loss.double()) - loss64)
    derr = (dx.double() - dx64).abs()
    ratio = float((derr / dx64.abs().clamp_min(1e-300)).max())
    t_loss, t_dx = run(torch.nn.MSELoss(reduction=reduction))
    print(f"[mse n={n} {reduction}] loss err {err:.3e} bound {(n + 4) * U * abs(loss64):.3e}; "
          f"dx max rel err {ratio / U:.2f} u (bound 4 u); dx bitwise torch's: "
          f"{torch.equal(dx, t_dx)}; loss bitwise torch's: {torch.equal(loss, t_loss)}")
    assert err <= (n + 4) * U * abs(loss64)
    assert bool((derr <= 4 * U * dx64.abs()).all())
    assert bool((dx[same] == 0).all())  # a zero difference gives exactly 0
    # the functional form is the module's path
    xd = x.to(cuda).requires_grad_(True)
    l2 = ops.mse_loss(xd, y.to(cuda), reduction)
    l2.backward(torch.tensor(g, device=cuda))
    assert torch.equal(l2.detach().cpu(), loss) and torch.equal(xd.grad.cpu(), dx)
    # a NaN input: a NaN loss, and a NaN in its own dx only
    k = n // 2
    xn = x.clone()
    xn[k] = float("nan")
    xd = xn.to(cuda).requires_grad_(True)
    ln = hlhgat.nn.MSELoss(reduction=reduction)(xd, y.to(cuda))
    ln.backward(torch.tensor(g, device=cuda))
    gn = xd.grad.cpu()
    assert bool(torch.isnan(ln)) and bool(torch.isnan(gn[k]))
    keep = torch.arange(n) != k
    assert torch.equal(gn[keep], dx[keep])
    ops.check_device_errors()


@pytest.mark.gpu
def test_module_routes(cuda, monkeypatch):
    """HIP for ROCm fp32 tensors of equal shape up to FUSED_MAX elements with
    "mean" / "sum"; torch for everything else."""
    import hlhgat
    from hlhgat import ops
    calls = []
    real = ops.mse_loss
    monkeypatch.setattr(ops, "mse_loss", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    crit = hlhgat.nn.MSELoss()
    assert crit.FUSED_MAX == hlhgat.nn.BCEWithLogitsLoss.FUSED_MAX
    x, y = torch.randn(6, 1, device=cuda), torch.randn(6, 1, device=cuda)

    def hip(c, a, b):
        calls.clear()
        out = c(a, b)
        return bool(calls), out

    assert hip(crit, x, y)[0]
    assert hip(hlhgat.nn.MSELoss(reduction="sum"), x, y)[0]
    assert not hip(hlhgat.nn.MSELoss(reduction="none"), x, y)[0]
    assert not hip(crit, x, y.clone().requires_grad_(True))[0]
    assert not hip(crit, x.double(), y.double())[0]
    assert not hip(crit, x[:0], y[:0])[0]
    with pytest.warns(UserWarning):  # torch broadcasts (and warns); not the HIP route
        assert not hip(crit, x, y.view(-1))[0]
    n = crit.FUSED_MAX
    big, big1 = torch.randn(n, device=cuda), torch.randn(n + 1, device=cuda)
    assert hip(crit, big, torch.zeros_like(big))[0]
    used, out = hip(crit, big1, torch.zeros_like(big1))
    assert not used and torch.isfinite(out)
    # a non-contiguous view goes through a contiguous copy: the same bits
    w = torch.randn(6, 2, device=cuda)
    a = crit(w[:, 0], y.view(-1))
    b = crit(w[:, 0].contiguous(), y.view(-1))
    assert torch.equal(a, b)
    ops.check_device_errors()
