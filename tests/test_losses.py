"""The reduced training losses (csrc/loss.hip): ops.bce_logits_loss,
ops.cross_entropy, hlhgat.nn.FocalLoss / MaskedBCEWithLogitsLoss /
CrossEntropyLoss.

CPU: the numpy fp64 restatement (tests/loss_ref.py) reproduces the fixture the
reference's own FocalLoss and torch's CrossEntropyLoss generated
(tests/golden/losses_small.npz); the modules on CPU tensors are the torch
composition bit for bit; the C-ABI rejects bad arguments before any launch.
GPU: loss, gradient and integer by-products against loss_ref in fp64.

Tolerance gate (GPU): conftest.close(actual, expected, rel) with rel the larger
of the project's constants for this family (1e-5 loss, 1e-6 gradient,
tests/test_torch_ops.py) and four times the error of torch's own fp32
evaluation of the same expression on the same inputs against the same fp64
(measured in the same test; the factor 4 allows for a different but equally
valid summation order)."""
import ctypes

import numpy as np
import pytest
import torch

import loss_ref as R
from conftest import close, load_golden

F = torch.nn.functional
REL_LOSS, REL_GRAD = 1e-5, 1e-6
MODES = {"mean": ("mean", None), "sum": ("sum", None), "focal": ("mean", (0.25, 2.0, 1e4)),
         "focal_g0": ("mean", (0.25, 0.0, 1e4)), "focal_g1.5": ("mean", (0.25, 1.5, 1e4))}
GOUT = 3.0


def _gate(actual, expected, torch_val, const, what):
    """close() at max(const, 4 * torch's fp32 error); prints the figures."""
    e = np.asarray(expected, dtype=np.float64)
    scale = max(1.0, float(np.abs(e).max()) if e.size else 1.0)
    terr = 0.0
    if torch_val is not None:
        t = np.asarray(torch_val, dtype=np.float64)
        terr = (float(np.abs(t - e).max()) if e.size else 0.0) / scale
        assert np.isfinite(terr), f"{what}: torch's fp32 evaluation is not finite"
    rel = max(const, 4.0 * terr)
    a = np.asarray(actual, dtype=np.float64)
    err = (float(np.abs(a - e).max()) if e.size else 0.0) / scale
    print(f"{what}: hip {err:.2e} torch {terr:.2e} gate {rel:.1e}")
    close(actual, expected, rel, what)


def _torch_bce(x, y, m, reduction, focal):
    """The torch fp32 composition (the reference's expression) and its gradient."""
    x = x.detach().clone().requires_grad_(True)
    xs, ys = (x, y) if m is None else (x[m], y[m])
    b = F.binary_cross_entropy_with_logits(xs, ys, reduction=reduction)
    if focal is not None:
        alpha, gamma, scale = focal
        logpt = -b
        pt = torch.exp(logpt)
        b = -((1 - pt) ** gamma) * alpha * logpt * scale
    (b * GOUT).backward()
    return b.detach().cpu().numpy(), x.grad.cpu().numpy()


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
FOCAL_CASES = ("n1", "nan35", "n257", "special")
CE_CASES = ("1x1", "7x10", "5x64")


def test_loss_ref_reproduces_fixture():
    z = load_golden("losses_small")
    for name in FOCAL_CASES:
        x, y, m = (z[f"focal_{name}/{k}"] for k in ("x", "y", "mask"))
        for gamma in (2, 0, 1.5):
            loss, dx, _ = R.bce(x, y, m, ignore_nan=True, focal=(0.25, gamma, 1e4))
            close(loss, z[f"focal_{name}/g{gamma}/loss"], 1e-12, f"{name} g{gamma} loss")
            close(dx, z[f"focal_{name}/g{gamma}/grad"], 1e-12, f"{name} g{gamma} grad")
    for name in CE_CASES:
        x, lab = z[f"ce_{name}/x"], z[f"ce_{name}/label"]
        for red in ("mean", "sum"):
            loss, dx, _ = R.cross_entropy(x, lab, reduction=red)
            close(loss, z[f"ce_{name}/{red}/loss"], 1e-12, f"ce {name} {red} loss")
            close(dx, z[f"ce_{name}/{red}/grad"], 1e-12, f"ce {name} {red} grad")


def test_loss_ref_conventions():
    """Empty selections give 0 / 0; stats are the plain integer counts."""
    x = np.array([1.0, -2.0, 3.0, -4.0])
    y = np.array([1.0, 1.0, 0.0, np.nan])
    loss, dx, st = R.bce(x, y, np.zeros(4), ignore_nan=True)
    assert loss == 0.0 and not dx.any() and st.tolist() == [0, 0, 0, 0]
    _, dx, st = R.bce(x, y, None, ignore_nan=True, reduction="sum")
    assert st.tolist() == [3, 1, 1, 1] and dx[3] == 0.0
    loss, dx, st = R.cross_entropy(np.zeros((2, 3)), np.array([-100, 7]))
    assert loss == 0.0 and not dx.any() and st.tolist() == [0, 0]


def _reference_focal(preds, labels, alpha=0.25, gamma=2, weight=None):
    """lib/Loss_function.py:14-26, restated."""
    logpt = -torch.nn.BCEWithLogitsLoss(weight=weight)(preds, labels)
    pt = torch.exp(logpt)
    return -((1 - pt) ** gamma) * alpha * logpt * 1e4


def test_modules_on_cpu_are_the_torch_composition():
    import hlhgat
    g = torch.Generator().manual_seed(5)
    x = torch.randn(6, 10, generator=g, requires_grad=True)
    y = (torch.rand(6, 10, generator=g) > 0.5).float()
    y[1, 2] = float("nan")
    y[4, 7] = float("nan")
    mask = torch.rand(6, 10, generator=g) > 0.2
    keep = ~torch.isnan(y)
    crit = hlhgat.nn.FocalLoss()
    assert (crit.alpha, crit.gamma, crit.weight, crit.scale, crit.ignore_nan) == (
        0.25, 2, None, 1e4, False)
    assert isinstance(crit.bce_fn, torch.nn.BCEWithLogitsLoss)
    # the reference's call form, the mask form and ignore_nan: one expression
    want = _reference_focal(x[keep], y[keep])
    gw, = torch.autograd.grad(want, x)
    assert torch.equal(crit(x[keep], y[keep]), want)
    got = hlhgat.nn.FocalLoss(ignore_nan=True)(x, y)
    assert torch.equal(got, want)
    assert torch.equal(torch.autograd.grad(got, x)[0], gw)
    assert torch.equal(crit(x, y, mask=keep), want)
    both = mask & keep
    assert torch.equal(hlhgat.nn.FocalLoss(0.5, 1.5, ignore_nan=True)(x, y, mask),
                       _reference_focal(x[both], y[both], 0.5, 1.5))
    w = torch.rand(10, generator=g)
    yz = torch.nan_to_num(y)
    assert torch.equal(hlhgat.nn.FocalLoss(weight=w)(x, yz), _reference_focal(x, yz, weight=w))
    for red in ("mean", "sum", "none"):
        got = hlhgat.nn.MaskedBCEWithLogitsLoss(red, ignore_nan=True)(x, y, mask)
        assert torch.equal(got, F.binary_cross_entropy_with_logits(x[both], y[both],
                                                                   reduction=red))
    assert torch.equal(hlhgat.nn.MaskedBCEWithLogitsLoss()(x, yz),
                       F.binary_cross_entropy_with_logits(x, yz))
    logits = torch.randn(7, 10, generator=g)
    lab = torch.randint(0, 10, (7,), generator=g)
    lab[2] = -100
    ce = hlhgat.nn.CrossEntropyLoss(ignore_index=-100, reduction="mean")
    assert isinstance(ce, torch.nn.CrossEntropyLoss)
    assert torch.equal(ce(logits, lab), F.cross_entropy(logits, lab))
    assert torch.equal(hlhgat.CrossEntropyLoss(reduction="sum", label_smoothing=0.1)(logits, lab),
                       F.cross_entropy(logits, lab, reduction="sum", label_smoothing=0.1))
    assert hlhgat.FocalLoss is hlhgat.nn.FocalLoss
    assert hlhgat.MaskedBCEWithLogitsLoss is hlhgat.nn.MaskedBCEWithLogitsLoss


def test_ops_have_no_cpu_fallback():
    from hlhgat import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.bce_logits_loss(torch.randn(4), torch.ones(4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cross_entropy(torch.randn(4, 3), torch.zeros(4, dtype=torch.int64))


def test_capi_rejects_bad_arguments():
    """Every entry validates before any launch (no device needed)."""
    from hlhgat import _lib
    L = _lib.LIB
    assert L.hlhgat_version() >= 103
    buf = (ctypes.c_double * 8)()
    a = (ctypes.addressof(buf) + 15) & ~15  # a 16-byte aligned host address; never read
    MEAN, SUM, FOCAL = _lib.LOSS_MEAN, _lib.LOSS_SUM, _lib.LOSS_FOCAL
    assert L.hlhgat_loss_workspace_bytes(0) == 0
    assert L.hlhgat_loss_workspace_bytes(16384) == 32
    assert L.hlhgat_loss_workspace_bytes(16385) == 5 * 32
    assert L.hlhgat_loss_workspace_bytes(1 << 30) == 256 * 32

    def fwd(x=a, y=a, mask=None, n=100, red=MEAN, gamma=2.0, ws=None, wsb=0, loss=a, s=a,
            stats=a):
        return L.hlhgat_bce_reduce_fwd(x, y, mask, n, 0, red, 0.25, gamma, 1e4, ws, wsb, loss, s,
                                       stats, None)

    def bwd(x=a, y=a, n=100, red=MEAN, gamma=2.0, s=a, stats=a, gout=a, dx=a):
        return L.hlhgat_bce_reduce_bwd(x, y, None, n, 0, red, 0.25, gamma, 1e4, s, stats, gout,
                                       dx, None)

    for kw in (dict(x=None), dict(y=None), dict(loss=None), dict(s=None), dict(stats=None)):
        assert fwd(**kw) == 1, kw
        assert b"NULL" in L.hlhgat_last_error()
    for kw in (dict(x=None), dict(y=None), dict(s=None), dict(stats=None), dict(gout=None),
               dict(dx=None)):
        assert bwd(**kw) == 1, kw
        assert b"NULL" in L.hlhgat_last_error()
    for f in (fwd, bwd):
        assert f(n=0) == 1 and f(n=-5) == 1
        assert b"outside" in L.hlhgat_last_error()
        assert f(red=3) == 1 and f(red=-1) == 1
        assert b"unknown reduction" in L.hlhgat_last_error()
        assert f(red=FOCAL, gamma=0.5) == 1 and f(red=FOCAL, gamma=-1.0) == 1
        assert f(red=FOCAL, gamma=float("nan")) == 1
        assert b"gamma" in L.hlhgat_last_error()
    assert fwd(n=16385) == 1  # needs a workspace
    assert b"workspace" in L.hlhgat_last_error()
    assert fwd(n=16385, ws=a, wsb=5 * 32 - 1) == 1  # one byte short
    assert fwd(n=1 << 30, ws=a, wsb=255 * 32) == 1

    def ce_fwd(x=a, ld=10, rows=7, cols=10, label=a, red=MEAN, ws=None, wsb=0, loss=a, stats=a):
        return L.hlhgat_cross_entropy_fwd(x, ld, rows, cols, label, -100, red, ws, wsb, loss,
                                          stats, None)

    def ce_bwd(x=a, ld=10, rows=7, cols=10, label=a, red=MEAN, stats=a, gout=a, dx=a, lddx=10):
        return L.hlhgat_cross_entropy_bwd(x, ld, rows, cols, label, -100, red, stats, gout, dx,
                                          lddx, None)

    for kw in (dict(x=None), dict(label=None), dict(loss=None), dict(stats=None)):
        assert ce_fwd(**kw) == 1, kw
        assert b"NULL" in L.hlhgat_last_error()
    for kw in (dict(x=None), dict(label=None), dict(stats=None), dict(gout=None), dict(dx=None)):
        assert ce_bwd(**kw) == 1, kw
        assert b"NULL" in L.hlhgat_last_error()
    for f in (ce_fwd, ce_bwd):
        assert f(rows=0) == 1 and f(rows=-1) == 1
        assert f(cols=0, ld=64) == 1 and f(cols=65, ld=65) == 1
        assert b"C = " in L.hlhgat_last_error()
        assert f(ld=9) == 1
        assert b"ld = 9" in L.hlhgat_last_error()
        assert f(red=FOCAL) == 1 and f(red=7) == 1
        assert b"unknown reduction" in L.hlhgat_last_error()
    assert ce_bwd(lddx=9) == 1
    assert b"lddx" in L.hlhgat_last_error()
    assert ce_fwd(rows=16385) == 1
    assert b"workspace" in L.hlhgat_last_error()
    assert ce_fwd(rows=16385, ws=a, wsb=100) == 1
    assert SUM == 1


# ---------------------------------------------------------------------------
# GPU: the BCE family
# ---------------------------------------------------------------------------
def _labels(g, shape, soft=False):
    u = torch.rand(shape, generator=g)
    return u if soft else (u > 0.6).float()


def _bce_inputs(name):
    """(x, y, mask or None, ignore_nan) on the host; x may be a view."""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, name)))
    if name == "nan35":
        z = load_golden("losses_small")
        return (torch.from_numpy(z["focal_nan35/x"]), torch.from_numpy(z["focal_nan35/y"]),
                torch.from_numpy(z["focal_nan35/mask"]), True)
    if name == "transposed":
        x = (torch.randn(37, 19, generator=g) * 2).t()
        y = _labels(g, (37, 19)).t()
        return x, y, (torch.rand(37, 19, generator=g) > 0.3).t(), False
    if name == "special":
        x = torch.tensor([0.0, -0.0, 30.0, -30.0, 30.0, -30.0, 1e-3, -1e-3, 0.0, -0.0])
        y = torch.tensor([1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.25, 0.75, 0.0, 1.0])
        return x, y, None, False
    if name == "offset4":  # base pointers 4 bytes (mask: 1 byte) past an aligned address
        n = 1003
        return ((torch.randn(n + 1, generator=g) * 2)[1:], _labels(g, n + 1, soft=True)[1:],
                (torch.rand(n + 1, generator=g) > 0.5)[1:], False)
    n = int(name[1:])
    x = torch.randn(n, generator=g) * 2
    y = _labels(g, n, soft=n in (256, 16384))
    mask, ignore_nan = None, False
    if n in (257, 16385, 300001):
        mask = torch.rand(n, generator=g) > 0.25
    if n in (255, 300001):
        y[torch.rand(n, generator=g) > 0.9] = float("nan")
        ignore_nan = True
    return x, y, mask, ignore_nan


_BCE_CACHE = {}


def _bce_case(name):
    """Inputs plus the fp64 reference of every mode, computed once and shared."""
    if name not in _BCE_CACHE:
        x, y, mask, ignore_nan = _bce_inputs(name)
        ref = {k: R.bce(x.numpy(), y.numpy(), None if mask is None else mask.numpy(), ignore_nan,
                        reduction=red, focal=focal, gout=GOUT)
               for k, (red, focal) in MODES.items()}
        _BCE_CACHE[name] = (x, y, mask, ignore_nan, ref)
    return _BCE_CACHE[name]


BCE_CASES = ("n1", "nan35", "n255", "n256", "n257", "n16384", "n16385", "n300001", "transposed",
             "special", "offset4")


@pytest.mark.gpu
@pytest.mark.parametrize("name", BCE_CASES)
def test_bce_family_matches_reference(cuda, name):
    from hlhgat import ops
    x, y, mask, ignore_nan, ref = _bce_case(name)
    xd, yd = x.to(cuda), y.to(cuda)
    md = None if mask is None else mask.to(cuda)
    if name == "transposed":  # .to() keeps the strides of a dense view
        assert not xd.is_contiguous()
    if name == "offset4":
        xd, yd, md = (t.to(cuda)[1:] for t in (torch.cat([x[:1], x]), torch.cat([y[:1], y]),
                                               torch.cat([mask[:1], mask])))
        assert xd.data_ptr() % 16 == 4 and md.data_ptr() % 4 == 1
    sel = torch.from_numpy(R.included(y.numpy(), None if mask is None else mask.numpy(),
                                      ignore_nan)).to(cuda)
    m = None if bool(sel.all()) else sel
    for mode, (red, focal) in MODES.items():
        xg = xd.detach().requires_grad_(True)
        loss, stats = ops.bce_logits_loss(xg, yd, md, ignore_nan=ignore_nan, reduction=red,
                                          focal=focal, return_stats=True)
        (loss * GOUT).backward()
        l_ref, dx_ref, st_ref = ref[mode]
        t_loss, t_grad = _torch_bce(xd, yd, m, red, focal)
        _gate(loss.detach().cpu().numpy(), l_ref, t_loss, REL_LOSS, f"{name} {mode} loss")
        _gate(xg.grad.cpu().numpy(), dx_ref, t_grad, REL_GRAD, f"{name} {mode} grad")
        assert stats.dtype == torch.int64 and stats.cpu().tolist() == st_ref.tolist(), mode
        assert xg.grad.shape == xd.shape


@pytest.mark.gpu
def test_bce_modules_route_to_hip(cuda):
    """The modules on device tensors give the op's bits (every size on HIP:
    no FUSED_MAX), and 0 < gamma < 1 goes to the torch composition."""
    import hlhgat
    from hlhgat import ops
    x, y, mask, ignore_nan, _ = _bce_case("n300001")
    xd, yd, md = x.to(cuda), y.to(cuda), mask.to(cuda)
    want = ops.bce_logits_loss(xd, yd, md, ignore_nan=True, focal=(0.25, 2.0, 1e4))
    assert torch.equal(hlhgat.nn.FocalLoss(ignore_nan=True)(xd, yd, mask=md), want)
    want = ops.bce_logits_loss(xd, yd, md, ignore_nan=True, reduction="sum")
    assert torch.equal(hlhgat.nn.MaskedBCEWithLogitsLoss("sum", True)(xd, yd, md), want)
    # a float mask costs one ATen launch and means the same
    assert torch.equal(hlhgat.nn.MaskedBCEWithLogitsLoss("sum", True)(xd, yd, md.float()), want)
    sel = md & ~torch.isnan(yd)
    got = hlhgat.nn.FocalLoss(gamma=0.5, ignore_nan=True)(xd, yd, md)
    b = F.binary_cross_entropy_with_logits(xd[sel], yd[sel])
    assert torch.equal(got, (1 - torch.exp(-b)) ** 0.5 * 0.25 * b * 1e4)
    with pytest.raises(ValueError, match="gamma"):
        ops.bce_logits_loss(xd, yd, focal=(0.25, 0.5, 1e4))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1000, 20000])
def test_bce_excluded_values_enter_nothing(cuda, n):
    """1e30 / NaN in x and NaN in y at excluded positions: the loss is finite
    and the reference's over the included elements, dx exactly +0.0 there."""
    from hlhgat import ops
    g = torch.Generator().manual_seed(31 + n)
    x = torch.randn(n, generator=g)
    y = (torch.rand(n, generator=g) > 0.5).float()
    mask = torch.rand(n, generator=g) > 0.4
    excl = (~mask).nonzero().view(-1)
    x[excl[0::2]] = 1e30
    x[excl[1::2]] = float("nan")
    y[excl[0::3]] = float("nan")
    inc = mask.nonzero().view(-1)
    y[inc[0::7]] = float("nan")  # missing labels inside the mask: ignore_nan drops them
    x[inc[0::14]] = float("nan")
    sel = torch.from_numpy(R.included(y.numpy(), mask.numpy(), True))
    for mode in ("mean", "focal"):
        red, focal = MODES[mode]
        l_ref, dx_ref, st_ref = R.bce(x.numpy(), y.numpy(), mask.numpy(), True, reduction=red,
                                      focal=focal, gout=GOUT)
        assert np.isfinite(l_ref)
        xg = x.to(cuda).requires_grad_(True)
        loss, stats = ops.bce_logits_loss(xg, y.to(cuda), mask.to(cuda), ignore_nan=True,
                                          reduction=red, focal=focal, return_stats=True)
        (loss * GOUT).backward()
        assert bool(torch.isfinite(loss))
        xc, yc = x.to(cuda), y.to(cuda)
        t_loss, t_grad = _torch_bce(torch.where(sel.to(cuda), xc, torch.zeros_like(xc)),
                                    torch.where(sel.to(cuda), yc, torch.zeros_like(yc)),
                                    sel.to(cuda), red, focal)
        _gate(loss.detach().cpu().numpy(), l_ref, t_loss, REL_LOSS, f"excluded {n} {mode} loss")
        _gate(xg.grad.cpu().numpy(), dx_ref, t_grad, REL_GRAD, f"excluded {n} {mode} grad")
        gx = xg.grad.cpu()[~sel]
        assert torch.equal(gx, torch.zeros_like(gx)) and not bool(torch.signbit(gx).any())
        assert stats.cpu().tolist() == st_ref.tolist()


@pytest.mark.gpu
def test_empty_selection_gives_zero(cuda):
    """All excluded / all ignored: loss 0.0, dx all zero, stats[0] == 0 (torch
    gives NaN; a captured step must survive one all-missing batch)."""
    from hlhgat import ops
    for n in (300, 20000):
        for mode in ("mean", "sum", "focal", "focal_g0"):
            red, focal = MODES[mode]
            x = torch.randn(n, device=cuda, requires_grad=True)
            y = torch.full((n,), float("nan"), device=cuda)
            loss, stats = ops.bce_logits_loss(x, y, ignore_nan=True, reduction=red, focal=focal,
                                              return_stats=True)
            loss.backward()
            assert float(loss) == 0.0 and stats.cpu().tolist() == [0, 0, 0, 0]
            assert torch.equal(x.grad, torch.zeros_like(x.grad))
            x.grad = None
            loss = ops.bce_logits_loss(x, torch.ones(n, device=cuda),
                                       torch.zeros(n, device=cuda, dtype=torch.uint8),
                                       reduction=red, focal=focal)
            loss.backward()
            assert float(loss) == 0.0 and torch.equal(x.grad, torch.zeros_like(x.grad))
    for red in ("mean", "sum"):
        x = torch.randn(9, 10, device=cuda, requires_grad=True)
        lab = torch.full((9,), -100, device=cuda)
        loss, stats = ops.cross_entropy(x, lab, reduction=red, return_stats=True)
        loss.backward()
        assert float(loss) == 0.0 and stats.cpu().tolist() == [0, 0]
        assert torch.equal(x.grad, torch.zeros_like(x.grad))


# ---------------------------------------------------------------------------
# GPU: cross-entropy
# ---------------------------------------------------------------------------
def _ce_case(shape):
    g = torch.Generator().manual_seed(77 + shape[0] * 131 + shape[1])
    R_, C = shape
    x = torch.randn(R_, C, generator=g) * 3
    lab = torch.randint(0, C, (R_,), generator=g)
    if R_ >= 7:
        lab[torch.rand(R_, generator=g) > 0.8] = -100
        x[3] = x[3, 0]  # a row of ties: the lowest index is the argmax
        lab[3] = 0
    return x, lab


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (7, 10), (300, 10), (16385, 3), (5, 64)])
def test_cross_entropy_matches_reference(cuda, shape):
    from hlhgat import ops
    x, lab = _ce_case(shape)
    for red in ("mean", "sum"):
        l_ref, dx_ref, st_ref = R.cross_entropy(x.numpy(), lab.numpy(), reduction=red, gout=GOUT)
        xg = x.to(cuda).requires_grad_(True)
        loss, stats = ops.cross_entropy(xg, lab.to(cuda), reduction=red, return_stats=True)
        (loss * GOUT).backward()
        xt = x.to(cuda).requires_grad_(True)
        lt = F.cross_entropy(xt, lab.to(cuda), reduction=red)
        (lt * GOUT).backward()
        _gate(loss.detach().cpu().numpy(), l_ref, lt.detach().cpu().numpy(), REL_LOSS,
              f"ce {shape} {red}")
        _gate(xg.grad.cpu().numpy(), dx_ref, xt.grad.cpu().numpy(), REL_GRAD,
              f"ce {shape} {red} grad")
        assert stats.dtype == torch.int64 and stats.cpu().tolist() == st_ref.tolist()


@pytest.mark.gpu
def test_cross_entropy_column_block(cuda):
    """A [:, 3:13] block of a [7, 20] tensor is read in place (ld = 20); the
    backward writes the block's columns of a [7, 20] gradient buffer and no
    other."""
    from hlhgat import _lib, ops
    g = torch.Generator().manual_seed(9)
    wide = (torch.randn(7, 20, generator=g) * 2).to(cuda)
    lab = torch.randint(0, 10, (7,), generator=g)
    lab[4] = -100
    l_ref, dx_ref, st_ref = R.cross_entropy(wide[:, 3:13].cpu().numpy(), lab.numpy(), gout=GOUT)
    wg = wide.clone().requires_grad_(True)
    view = wg[:, 3:13]
    assert not view.is_contiguous()
    loss, stats = ops.cross_entropy(view, lab.to(cuda), return_stats=True)
    (loss * GOUT).backward()
    close(loss.detach().cpu().numpy(), l_ref, REL_LOSS, "block loss")
    close(wg.grad[:, 3:13].cpu().numpy(), dx_ref, REL_GRAD, "block grad")
    assert not bool(wg.grad[:, :3].any()) and not bool(wg.grad[:, 13:].any())
    assert stats.cpu().tolist() == st_ref.tolist()
    # the C-ABI with lddx = 20: the other columns keep their contents
    buf = torch.full((7, 20), 777.0, device=cuda)
    gout = torch.tensor([GOUT], device=cuda)
    labd = lab.to(cuda)
    _lib.check(_lib.LIB.hlhgat_cross_entropy_bwd(
        wide.data_ptr() + 12, 20, 7, 10, labd.data_ptr(), -100, _lib.LOSS_MEAN, stats.data_ptr(),
        gout.data_ptr(), buf.data_ptr() + 12, 20,
        torch.cuda.current_stream().cuda_stream), "cross_entropy_bwd")
    torch.cuda.synchronize()
    assert torch.equal(buf[:, 3:13], wg.grad[:, 3:13])
    assert bool((buf[:, :3] == 777.0).all()) and bool((buf[:, 13:] == 777.0).all())


@pytest.mark.gpu
def test_cross_entropy_module_and_wide_fallback(cuda):
    import hlhgat
    from hlhgat import ops
    x, lab = _ce_case((300, 10))
    xd, ld = x.to(cuda), lab.to(cuda)
    assert torch.equal(hlhgat.nn.CrossEntropyLoss()(xd, ld), ops.cross_entropy(xd, ld))
    g = torch.Generator().manual_seed(65)
    xw = torch.randn(12, 65, generator=g).to(cuda)
    lw = torch.randint(0, 65, (12,), generator=g).to(cuda)
    res = []
    for crit in (hlhgat.nn.CrossEntropyLoss(), torch.nn.CrossEntropyLoss()):
        xg = xw.clone().requires_grad_(True)
        loss = crit(xg, lw)
        loss.backward()
        res.append((loss.detach(), xg.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    with pytest.raises(RuntimeError, match="C = 65"):
        ops.cross_entropy(xw, lw)


@pytest.mark.gpu
def test_cross_entropy_bad_label_raises_device_error(cuda):
    """Labels C and -1: no fault, the rows are ignored, and the device error
    word names the label bit."""
    from hlhgat import _lib, ops
    x, lab = _ce_case((7, 10))
    lab[0], lab[2], lab[6] = 10, -1, 4
    l_ref, dx_ref, st_ref = R.cross_entropy(x.numpy(), lab.numpy())
    torch.cuda.synchronize()
    ops.clear_device_errors()
    try:
        xg = x.to(cuda).requires_grad_(True)
        loss, stats = ops.cross_entropy(xg, lab.to(cuda), return_stats=True)
        loss.backward()
        close(loss.detach().cpu().numpy(), l_ref, REL_LOSS, "bad label loss")
        close(xg.grad.cpu().numpy(), dx_ref, REL_GRAD, "bad label grad")
        assert not bool(xg.grad[0].any()) and not bool(xg.grad[2].any())
        assert stats.cpu().tolist() == st_ref.tolist()
        assert ops.device_errors() == _lib.DEVERR_LABEL
        with pytest.raises(RuntimeError, match="label"):
            ops.check_device_errors()
    finally:
        ops.clear_device_errors()
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# GPU: determinism and capture
# ---------------------------------------------------------------------------
def _run_focal(x, y, mask):
    from hlhgat import ops
    xg = x.detach().clone().requires_grad_(True)
    loss, stats = ops.bce_logits_loss(xg, y, mask, ignore_nan=True, focal=(0.25, 2.0, 1e4),
                                      return_stats=True)
    dx, = torch.autograd.grad(loss, xg)
    return loss.detach(), dx, stats


@pytest.mark.gpu
def test_results_are_bitwise_reproducible(cuda):
    """Two runs agree bit for bit, and so does a run on a second stream beside
    another kernel: the grid and the summation order depend on n alone."""
    from hlhgat import ops
    x, y, mask, _, _ = _bce_case("n300001")
    xd, yd, md = x.to(cuda), y.to(cuda), mask.to(cuda)
    first = _run_focal(xd, yd, md)
    second = _run_focal(xd, yd, md)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    big = torch.randn(8192, 8192, device=cuda)
    side = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize()
    for _ in range(2):
        big = big @ big * 1e-3  # keeps the default stream busy for milliseconds
    with torch.cuda.stream(side):
        third = _run_focal(xd, yd, md)
    torch.cuda.synchronize()
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    xc, lab = _ce_case((16385, 3))
    runs = []
    for _ in range(2):
        xg = xc.to(cuda).requires_grad_(True)
        loss = ops.cross_entropy(xg, lab.to(cuda))
        loss.backward()
        runs.append((loss.detach(), xg.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5000, 20000])
def test_masked_focal_captures(cuda, n):
    """Forward + backward of masked focal captured in torch.cuda.graph with
    static x, y, mask: three contents with three included counts, one of them
    zero; every replay is the eager result bit for bit.  (The property the
    feature exists for: out[mask] cannot be captured.)"""
    import hlhgat
    crit = hlhgat.nn.FocalLoss(ignore_nan=True)
    g = torch.Generator().manual_seed(n)
    xs = torch.zeros(n, device=cuda, requires_grad=True)
    ys = torch.zeros(n, device=cuda)
    ms = torch.ones(n, device=cuda, dtype=torch.bool)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up off the capture
        for _ in range(2):
            torch.autograd.grad(crit(xs, ys, mask=ms), xs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s = crit(xs, ys, mask=ms)
        grad_s, = torch.autograd.grad(loss_s, xs)
    counts = []
    for keep in (0.7, 0.0, 0.1):
        x = torch.randn(n, generator=g)
        y = (torch.rand(n, generator=g) > 0.5).float()
        y[torch.rand(n, generator=g) > 0.9] = float("nan")
        mask = torch.rand(n, generator=g) < keep
        with torch.no_grad():
            xs.copy_(x)
            ys.copy_(y)
            ms.copy_(mask)
        graph.replay()
        torch.cuda.synchronize()
        loss_e, grad_e, stats = _run_focal(x.to(cuda), y.to(cuda), mask.to(cuda))
        assert torch.equal(loss_s, loss_e) and torch.equal(grad_s, grad_e), keep
        assert bool(torch.isfinite(loss_s))
        counts.append(int(stats[0]))
    assert counts[1] == 0 and len(set(counts)) == 3, counts


# ---------------------------------------------------------------------------
# GPU: the heads through TrainStep
# ---------------------------------------------------------------------------
def _steps(mk, loss, batches, cuda, graphs, n=3):
    from hlhgat.train import TrainStep
    torch.manual_seed(0)
    m = mk().to(cuda).train()
    st = TrainStep(m, loss, lr=1e-3, graphs=graphs)
    ls = [float(st(batches[i % len(batches)]).detach()) for i in range(n)]
    return ls, {k: v.detach().clone() for k, v in m.state_dict().items()}, st.stats


def _assert_graph_equals_eager(mk, loss, batches, cuda, replays):
    l_e, sd_e, _ = _steps(mk, loss, batches, cuda, False)
    l_g, sd_g, stats = _steps(mk, loss, batches, cuda, True)
    assert stats["replay"] == replays, stats
    assert all(np.isfinite(l_e)), l_e
    assert l_e == l_g
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    return l_e


@pytest.mark.gpu
def test_train_step_pepfunc_focal_ignore_nan(cuda):
    """The tiny peptides head with FocalLoss(ignore_nan=True) and NaNs in y
    (one batch all missing): graph-replayed steps equal eager steps bit for
    bit -- the masked objective inside a captured step."""
    import hlhgat
    from hlhgat.synthetic import two_level_batch
    batches = []
    for i, frac in enumerate((0.3, 1.0, 0.1)):
        b = two_level_batch("peptides", 6, seed=1)
        g = torch.Generator().manual_seed(40 + i)
        b[0].y[torch.rand(b[0].y.shape, generator=g) < frac] = float("nan")
        batches.append([x.to(cuda) for x in b])
    assert bool(torch.isnan(batches[1][0].y).all())
    crit = hlhgat.nn.FocalLoss(ignore_nan=True)
    mk = lambda: hlhgat.HL_HGCNN_pepfunc_dense_int3_attpool(  # noqa: E731
        channels=[1, 1], filters=[16, 32], mlp_channels=[32], K=3, pool_loc=0)
    losses = _assert_graph_equals_eager(mk, lambda o, d: crit(o, d[0].y.view(o.shape)), batches,
                                        cuda, replays=2)
    assert losses[1] == 0.0 and losses[0] > 0.0 and losses[2] > 0.0


@pytest.mark.gpu
def test_train_step_tsp_masked_bce(cuda):
    """The tiny TSP head on a padded batch: MaskedBCEWithLogitsLoss with mask =
    x_s[:, 1] is the ATen expression weight=mask, reduction="sum" / real edge
    count (tests/test_train_step.py) within the gate, and captures."""
    import hlhgat
    from hlhgat.hodge_dataset import collate, pad_batch, static_caps
    from hlhgat.synthetic import tsp_like_graph
    raw = collate([tsp_like_graph(1, n=300, k=6)], check_hodge=False)
    raw.y = (torch.rand(raw.y.shape, generator=torch.Generator().manual_seed(3)) > 0.8).float()
    d = pad_batch(raw, static_caps(raw, 128)).to(cuda)
    assert d.x_s.size(0) > raw.x_s.size(0)
    mk = lambda: hlhgat.HL_HGCNN_TSP_dense_int3_pyr(  # noqa: E731
        channels=[1, 1], filters=[16, 32], mlp_channels=[32], K=3)
    crit = hlhgat.nn.MaskedBCEWithLogitsLoss()
    hip = lambda o, b: crit(o[0].view(-1), b.y.view(-1).float(), mask=b.x_s[:, 1])  # noqa: E731
    aten = lambda o, b: F.binary_cross_entropy_with_logits(  # noqa: E731
        o[0].view(-1), b.y.view(-1).float(), weight=b.x_s[:, 1],
        reduction="sum") / b.num_edge1.sum()
    torch.manual_seed(0)
    m = mk().to(cuda).train()
    logits = m(d)[0].detach().view(-1)
    res = []
    for fn in (hip, aten):
        lg = logits.clone().requires_grad_(True)
        loss = fn((lg,), d)
        g, = torch.autograd.grad(loss * GOUT, lg)
        res.append((loss.detach().cpu().numpy(), g.cpu().numpy()))
    l_ref, dx_ref, _ = R.bce(logits.cpu().numpy(), d.y.view(-1).float().cpu().numpy(),
                             d.x_s[:, 1].cpu().numpy(), gout=GOUT)
    _gate(res[0][0], l_ref, res[1][0], REL_LOSS, "tsp loss")
    _gate(res[0][1], dx_ref, res[1][1], REL_GRAD, "tsp grad")
    _assert_graph_equals_eager(mk, hip, [d], cuda, replays=2)


@pytest.mark.gpu
def test_train_step_cifar_cross_entropy(cuda):
    """The tiny CIFAR head with hlhgat.nn.CrossEntropyLoss: torch's loss within
    the gate, and graph-replayed steps equal eager steps bit for bit."""
    import hlhgat
    from hlhgat.synthetic import two_level_batch
    batches = [[x.to(cuda) for x in two_level_batch("cifar", 6, seed=s)] for s in (1, 1, 1)]
    mk = lambda: hlhgat.HL_HGCNN_CIFAR10SP_dense_int3_attpool(  # noqa: E731
        channels=[1, 1], filters=[16, 32], mlp_channels=[32], K=3, keig=10, pool_loc=0)
    crit = hlhgat.nn.CrossEntropyLoss()
    hip = lambda o, d: crit(o, d[0].y.view(-1).long())  # noqa: E731
    torch.manual_seed(0)
    m = mk().to(cuda).train()
    logits = m(batches[0]).detach()
    lab = batches[0][0].y.view(-1).long()
    res = []
    for fn in (crit, F.cross_entropy):
        lg = logits.clone().requires_grad_(True)
        loss = fn(lg, lab)
        g, = torch.autograd.grad(loss * GOUT, lg)
        res.append((loss.detach().cpu().numpy(), g.cpu().numpy()))
    l_ref, dx_ref, _ = R.cross_entropy(logits.cpu().numpy(), lab.cpu().numpy(), gout=GOUT)
    _gate(res[0][0], l_ref, res[1][0], REL_LOSS, "cifar loss")
    _gate(res[0][1], dx_ref, res[1][1], REL_GRAD, "cifar grad")
    _assert_graph_equals_eager(mk, hip, batches, cuda, replays=2)
