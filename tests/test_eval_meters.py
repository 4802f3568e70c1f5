"""Evaluation meters (csrc/metrics.hip, hlhgat.metrics): per-graph F1, argmax
accuracy, the collector and the regression summary, against the numpy
restatements of tests/meters_ref.py and the fixture meters_small.npz; eager
and replayed inside InferStep.

Bounds.  F1 and accuracy are integer counts and one correctly rounded fp32
division: bitwise / exact.  Every quantity of the regression summary is held
to meters_ref.regression_summary's bound: (N + 4) * 2^-52 * sum |term| for a
plain sum, propagated through the quotients and roots there.  Largest measured
error / bound over N in {2, 255, 256, 257, 5000} on an MI355X: sum_abs 0,
sum_sq 0.001, means 0.001, std 0.058, corr 0.002, mae 0.001, rmse 0.028
(DESIGN §26).
"""
import ctypes

import numpy as np
import pytest
import torch

import meters_ref as R
from conftest import load_golden

GOLD = load_golden("meters_small")
F1_CASES = sorted({k.split("/")[1] for k in GOLD if k.startswith("f1/")})


def _f1_case(name):
    g = {k.split("/")[2]: GOLD[k] for k in GOLD if k.startswith(f"f1/{name}/")}
    return g["logits"], g["labels"].astype(np.float32), g["seg_ptr"], g["f1"], bool(g["bad"])


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check_summary(got, pred, y, what, report=None):
    """got: dict of floats; every quantity within the restatement's bound."""
    value, bound = R.regression_summary(pred, y)
    for k, v in value.items():
        g = got[k]
        if np.isnan(v):
            assert g != g, f"{what}: {k} = {g}, want NaN"
            continue
        err = abs(np.longdouble(g) - v)
        ratio = float(err / bound[k]) if bound[k] > 0 else (0.0 if err == 0 else np.inf)
        print(f"{what}: {k} err {float(err):.3e} bound {float(bound[k]):.3e} ratio {ratio:.3f}")
        if report is not None:
            report[k] = max(report.get(k, 0.0), ratio)
        assert err <= bound[k], f"{what}: {k} = {g!r}, want {float(v)!r}: {float(err):.3e} > " \
                                f"{float(bound[k]):.3e}"


def _reg_inputs(N, seed):
    rng = np.random.default_rng(seed)
    pred = (50 + 15 * rng.standard_normal(N)).astype(np.float32)
    y = (0.6 * (pred - 50) + 50 + 12 * rng.standard_normal(N)).astype(np.float32)
    return pred, y


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_restatement_matches_fixture():
    assert set(F1_CASES) == set(R.f1_cases())
    for name in F1_CASES:
        p, y, ptr, f1, bad = _f1_case(name)
        assert tuple(np.diff(ptr)) == R.F1_SIZES and p.size == ptr[-1] + R.F1_PAD
        assert R.thresholds_clear(p), name
        got, got_bad = R.f1_per_graph(p, y, ptr)
        assert (_bits(got) == _bits(f1)).all() and got_bad == bad, name
        assert f1[0] == 0  # the empty graph
    assert _f1_case("inside")[3][3] == 0  # no positive label, no positive prediction
    assert np.isnan(_f1_case("nonfinite")[0]).sum() == 1
    assert np.isinf(_f1_case("nonfinite")[0]).sum() == 2
    assert (_f1_case("label2")[1] == 2).sum() == 1
    x, lab = GOLD["acc/x"], GOLD["acc/labels"]
    assert (R.argmax_rows(x) == GOLD["acc/argmax"]).all()
    assert (torch.from_numpy(x).argmax(1).numpy() == GOLD["acc/argmax"]).all()
    assert R.argmax_correct(x, lab) == (int(GOLD["acc/correct"]), True)
    value, _ = R.regression_summary(GOLD["reg/pred"], GOLD["reg/y"])
    for k, v in value.items():
        assert np.float64(v) == GOLD[f"reg/{k}"], k


def test_collector_cpu():
    from hlhgat.metrics import Collector
    c = Collector(5, 3, "cpu")
    wide = torch.arange(40, dtype=torch.float32).view(4, 10)
    c.append(wide[:2, 4:7])  # strided source
    c.append(wide[2:, 4:7])
    assert c.rows().shape == (4, 3) and torch.equal(c.rows(), wide[:, 4:7])
    with pytest.raises(RuntimeError, match="do not fit"):
        c.append(wide[:2, :3])
    assert int(c.cursor) == 4 and torch.equal(c.rows(), wide[:, 4:7])  # nothing written
    c.append(wide[:1, :3])  # the exact fill
    assert int(c.cursor) == 5
    c.reset()
    assert c.rows().shape == (0, 3)
    c1 = Collector(3, 1, "cpu")
    c1.append(torch.tensor([1.0, 2.0]))
    c1.append(torch.tensor([[3.0]]))
    assert c1.rows().view(-1).tolist() == [1.0, 2.0, 3.0]


def test_f1_meter_cpu():
    from hlhgat.metrics import F1Meter, f1_per_graph_cpu
    m = F1Meter(64, "cpu")
    want = []
    for name in F1_CASES:
        p, y, ptr, f1, bad = _f1_case(name)
        if bad:
            with pytest.raises(RuntimeError, match="neither 0 nor 1"):
                f1_per_graph_cpu(torch.from_numpy(p), torch.from_numpy(y), ptr.tolist())
            continue
        sizes = torch.from_numpy(np.diff(ptr).astype(np.int64))
        m.update(torch.from_numpy(p).view(-1, 1), torch.from_numpy(y), sizes)
        want.append(f1)
    want = np.concatenate(want)
    assert (_bits(m.per_graph().numpy()) == _bits(want)).all()
    assert m.compute() == float(want.astype(np.float64).mean())
    m.reset()
    assert m.compute() != m.compute()  # NaN: nothing collected


def test_accuracy_meter_cpu():
    from hlhgat.metrics import AccuracyMeter
    x, lab = torch.from_numpy(GOLD["acc/x"]), torch.from_numpy(GOLD["acc/labels"])
    ok = (lab >= 0) & (lab < x.size(1))
    m = AccuracyMeter("cpu")
    m.update(x[ok], lab[ok])
    m.update(x[ok][:7], lab[ok][:7].view(-1, 1))
    want = R.argmax_correct(x[ok].numpy(), lab[ok].numpy())[0] + \
        R.argmax_correct(x[ok][:7].numpy(), lab[ok][:7].numpy())[0]
    assert m.compute() == want / (int(ok.sum()) + 7)
    with pytest.raises(RuntimeError, match="outside"):
        m.update(x, lab)


@pytest.mark.parametrize("N", [0, 1, 2, 257])
def test_regression_meter_cpu(N):
    from hlhgat.metrics import RegressionMeter
    pred, y = _reg_inputs(N, 10 + N)
    m = RegressionMeter(300, "cpu")
    h = N // 2
    m.update(torch.from_numpy(pred[:h]).view(-1, 1), torch.from_numpy(y[:h]))
    m.update(torch.from_numpy(pred[h:]).view(-1, 1), torch.from_numpy(y[h:]).view(-1, 1))
    got = m.compute()
    assert got["n"] == N
    _check_summary(got, pred, y, f"cpu N={N}")
    const = RegressionMeter(300, "cpu")
    const.update(torch.full((256,), 50.0), torch.from_numpy(_reg_inputs(256, 3)[1]))
    r = const.compute()
    assert r["std_pred"] == 0 and r["corr"] != r["corr"]  # a zero deviation: NaN, as torch


def test_capi_argument_errors():
    """Argument validation runs before any HIP call."""
    from hlhgat import _lib
    L = _lib.LIB
    buf = (ctypes.c_float * 8)()
    cur = (ctypes.c_int64 * 2)()
    out = (ctypes.c_double * 8)()
    p, c, o = (ctypes.cast(v, ctypes.c_void_p) for v in (buf, cur, out))

    def bad(rc, text):
        assert rc == 1 and text.encode() in L.hlhgat_last_error(), L.hlhgat_last_error()

    bad(L.hlhgat_collect_rows(p, 1, -1, 1, p, 4, c, None), "< 0")
    bad(L.hlhgat_collect_rows(p, 1, 1, 1, p, -4, c, None), "< 0")
    bad(L.hlhgat_collect_rows(p, 1, 1, 0, p, 4, c, None), "must be positive")
    bad(L.hlhgat_collect_rows(p, 1, 1, -2, p, 4, c, None), "must be positive")
    bad(L.hlhgat_collect_rows(None, 1, 1, 1, p, 4, c, None), "NULL")
    bad(L.hlhgat_collect_rows(p, 1, 1, 1, None, 4, c, None), "NULL")
    bad(L.hlhgat_collect_rows(p, 1, 1, 1, p, 4, None, None), "NULL")
    bad(L.hlhgat_collect_rows(p, 1, 2, 2, p, 4, c, None), "row stride")
    assert L.hlhgat_collect_rows(None, 1, 0, 1, None, 4, None, None) == 0  # n == 0: a no-op
    bad(L.hlhgat_f1_per_graph(p, 1, p, 1, c, -1, 4, p, None), "< 0")
    bad(L.hlhgat_f1_per_graph(p, 1, p, 1, c, 1, -4, p, None), "< 0")
    bad(L.hlhgat_f1_per_graph(p, 1, p, 1, None, 1, 4, p, None), "NULL")
    bad(L.hlhgat_f1_per_graph(p, 1, p, 1, c, 1, 4, None, None), "NULL")
    bad(L.hlhgat_f1_per_graph(None, 1, p, 1, c, 1, 4, p, None), "NULL")
    bad(L.hlhgat_f1_per_graph(p, 0, p, 1, c, 1, 4, p, None), "stride")
    assert L.hlhgat_f1_per_graph(None, 1, None, 1, None, 0, 0, None, None) == 0
    bad(L.hlhgat_argmax_correct(p, 2, -1, 2, c, c, None, None), "< 0")
    bad(L.hlhgat_argmax_correct(p, 2, 1, 0, c, c, None, None), "must be positive")
    bad(L.hlhgat_argmax_correct(None, 2, 1, 2, c, c, None, None), "NULL")
    bad(L.hlhgat_argmax_correct(p, 2, 1, 2, None, c, None, None), "NULL")
    bad(L.hlhgat_argmax_correct(p, 2, 1, 2, c, None, None, None), "NULL")
    bad(L.hlhgat_argmax_correct(p, 1, 2, 2, c, c, None, None), "row stride")
    assert L.hlhgat_argmax_correct(None, 2, 0, 2, None, None, None, None) == 0
    bad(L.hlhgat_regression_summary(p, p, c, -1, o, None), "< 0")
    bad(L.hlhgat_regression_summary(p, p, None, 4, o, None), "NULL")
    bad(L.hlhgat_regression_summary(p, p, c, 4, None, None), "NULL")
    bad(L.hlhgat_regression_summary(None, p, c, 4, o, None), "NULL")
    assert _lib.DEVERR_METER_FULL == 16


def test_infer_step_without_meter_cpu():
    """InferStep on a CPU model: meter=None returns the eval forward as
    before; a meter sees (out, batch) under no_grad and changes nothing."""
    from hlhgat.train import InferStep
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Dropout(0.5), torch.nn.Linear(4, 1))
    m.train()
    x = torch.randn(6, 3)
    with torch.no_grad():
        want = m.eval()(x)
    m.train()
    plain = InferStep(m)
    assert plain.meter is None
    out = plain(x)
    assert torch.equal(out, want) and m.training and not out.requires_grad
    assert plain.stats == {"eager": 1, "replay": 0, "captures": 0}
    seen = []
    with_meter = InferStep(m, meter=lambda o, b: seen.append((o, b, torch.is_grad_enabled())))
    out2 = with_meter(x)
    assert torch.equal(out2, want) and len(seen) == 1
    assert seen[0][0] is out2 and seen[0][1] is x and seen[0][2] is False


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------
def _dev_errors():
    from hlhgat import ops
    torch.cuda.synchronize()
    return ops.device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("name", F1_CASES)
def test_f1_per_graph_bitwise(cuda, name):
    from hlhgat import _lib, ops
    p, y, ptr, f1, bad = _f1_case(name)
    assert R.thresholds_clear(p)
    ops.clear_device_errors()
    wide = torch.zeros(p.size, 3, device=cuda)
    wide[:, 1] = torch.from_numpy(p).to(cuda)
    yd, sp = torch.from_numpy(y).to(cuda), torch.from_numpy(ptr).to(cuda)
    got = ops.f1_per_graph(wide[:, 1:2], yd, sp)             # a column of a wider tensor
    got2 = ops.f1_per_graph(wide[:, 1].contiguous(), yd.view(-1, 1), sp)
    err = _dev_errors()
    try:
        assert (_bits(got.cpu().numpy()) == _bits(f1)).all(), (got.cpu().numpy(), f1)
        assert torch.equal(got, got2)
        assert err == (_lib.DEVERR_METRIC_LABEL if bad else 0)
        if bad:
            with pytest.raises(RuntimeError, match="label"):
                ops.check_device_errors()
    finally:
        ops.clear_device_errors()


@pytest.mark.gpu
@pytest.mark.parametrize("C", [1, 2, 10, 65])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_argmax_correct_exact(cuda, n, C):
    from hlhgat import _lib, ops
    rng = np.random.default_rng(100 * n + C)
    x = (np.round(rng.standard_normal((n, C + 3)) * 2) / 2).astype(np.float32)  # ties
    if C > 1:
        x[0, 1 + rng.integers(C)] = np.nan
        x[n // 2, :] = 0.5                       # a whole row tied
        x[n - 1, 1], x[n - 1, C] = np.nan, np.nan  # two NaNs: the first wins
    xt = torch.from_numpy(x)[:, 1:1 + C]         # strided rows
    am = xt.argmax(1)                            # torch's CPU rule
    lab = am.clone()
    lab[::3] = (lab[::3] + 1) % max(C, 2)        # C == 1: label 1 is out of range
    if n > 4:
        lab[3], lab[4] = -1, C
    oob = bool(((lab < 0) | (lab >= C)).any())
    want = int((am == lab).sum())
    assert R.argmax_correct(xt.numpy(), lab.numpy()) == (want, oob)
    ops.clear_device_errors()
    state = torch.tensor([5, 7], dtype=torch.int64, device=cuda)
    try:
        ops.argmax_correct(xt.to(cuda)[:, :], lab.to(cuda), state[0:1], state[1:2])
        ops.argmax_correct(torch.from_numpy(x).to(cuda)[:, 1:1 + C], lab.to(cuda), state[0:1])
        err = _dev_errors()
        assert state.tolist() == [5 + 2 * want, 7 + n]
        assert err == (_lib.DEVERR_METRIC_LABEL if oob else 0)
    finally:
        ops.clear_device_errors()


@pytest.mark.gpu
def test_collector_gpu(cuda):
    from hlhgat import _lib, ops
    from hlhgat.metrics import Collector
    ops.clear_device_errors()
    try:
        for width in (1, 3, 10):
            src = torch.randn(9, width + 5, device=cuda)
            c = Collector(9, width, cuda)
            c.buf.fill_(-1.0)
            c.append(src[:4, 2:2 + width])
            c.append(src[4:4, 2:2 + width])        # n == 0: a no-op
            c.append(src[4:8, 2:2 + width])
            if width == 1:
                c.append(src[8:9, 2])              # 1-D, strided
            else:
                c.append(src[8:9, 2:2 + width])    # the exact fill
            assert torch.equal(c.rows(), src[:, 2:2 + width]) and int(c.cursor) == 9
            assert _dev_errors() == 0
            before = c.buf.clone()
            c.append(src[:1, 2:2 + width])         # one row too many
            assert _dev_errors() == _lib.DEVERR_METER_FULL
            assert int(c.cursor) == 9 and torch.equal(c.buf, before)
            with pytest.raises(RuntimeError, match="collect_rows"):
                c.rows()
            ops.clear_device_errors()
            c.reset()
            assert c.rows().shape == (0, width)
            c.append(src[:2, 2:2 + width])
            assert torch.equal(c.rows(), src[:2, 2:2 + width])
            assert torch.equal(c.buf[2:], before[2:])  # rows behind the cursor untouched
        big = Collector(6, 2, cuda)                # 5 rows into a cursor at 2: no partial write
        big.append(torch.ones(2, 2, device=cuda))
        big.append(torch.full((5, 2), 3.0, device=cuda))
        assert _dev_errors() == _lib.DEVERR_METER_FULL and int(big.cursor) == 2
        assert float(big.buf[2:].abs().sum()) == 0
    finally:
        ops.clear_device_errors()


REG_RATIOS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 5000])
def test_regression_summary_bounds(cuda, N):
    from hlhgat import ops
    from hlhgat.metrics import RegressionMeter
    pred, y = _reg_inputs(N, 40 + N)
    m = RegressionMeter(5003, cuda)
    m.pred.buf.fill_(1e30)  # what lies behind the cursor must not be read
    m.y.buf.fill_(-1e30)
    ops.clear_device_errors()
    h = N // 3
    m.update(torch.from_numpy(pred[:h]).to(cuda).view(-1, 1), torch.from_numpy(y[:h]).to(cuda))
    m.update(torch.from_numpy(pred[h:]).to(cuda).view(-1, 1), torch.from_numpy(y[h:]).to(cuda))
    got = m.compute()
    again = m.compute()
    assert got["n"] == N
    assert all(got[k] == again[k] or (got[k] != got[k] and again[k] != again[k]) for k in got)
    _check_summary(got, pred, y, f"gpu N={N}", REG_RATIOS)
    print("largest err / bound so far:", {k: round(v, 3) for k, v in REG_RATIOS.items()})
    assert _dev_errors() == 0


@pytest.mark.gpu
def test_regression_summary_degenerate(cuda):
    from hlhgat.metrics import RegressionMeter
    m = RegressionMeter(256, cuda)
    assert m.compute()["n"] == 0 and m.compute()["mean_pred"] != m.compute()["mean_pred"]
    m.update(torch.full((256,), 50.0, device=cuda),
             torch.from_numpy(_reg_inputs(256, 3)[1]).to(cuda))
    r = m.compute()
    assert r["std_pred"] == 0 and r["corr"] != r["corr"] and r["mean_pred"] == 50.0


# ---------------------------------------------------------------------------
# GPU: inside InferStep
# ---------------------------------------------------------------------------
ZINC_KW = dict(channels=[1, 1], filters=[32, 32], mlp_channels=[64], K=3, keig=15)
TSP_KW = dict(channels=[1, 1], filters=[16, 32], mlp_channels=[32], K=3)
CIFAR_KW = dict(channels=[1, 1, 1], filters=[16, 32, 32], mlp_channels=[32], pool_loc=1, K=3,
                keig=10, l=0.5)


def _tsp_batch(seeds, cuda):
    from hlhgat.hodge_dataset import collate, pad_batch, static_caps
    from hlhgat.synthetic import tsp_like_graph
    raw = collate([tsp_like_graph(s, n=200, k=4) for s in seeds], check_hodge=False)
    raw.y = (torch.rand(raw.y.shape, generator=torch.Generator().manual_seed(seeds[0])) > 0.7
             ).float()
    b = pad_batch(raw, static_caps(raw, 128)).to(cuda)
    assert b.x_s.size(0) > int(b.num_edge1.sum())  # trailing padding rows
    return b


def _zinc_batch(seed, cuda):
    from hlhgat.synthetic import zinc_like_batch
    return zinc_like_batch(12, seed=seed).to(cuda)


def _f1_ref(out, b):
    ptr = R.seg_ptr_of(b.num_edge1.cpu().numpy())
    return R.f1_per_graph(out.detach().cpu().numpy(), b.y.cpu().numpy(), ptr)


def _kept_graphs():
    from hlhgat import train

    class Keep:
        def __enter__(self):
            self.was, train.KEEP_GRAPHS = train.KEEP_GRAPHS, True

        def __exit__(self, *a):
            train.KEEP_GRAPHS = self.was
    return Keep()


def _meter_kernels(step, part):
    from hlhgat import ops
    return sum(ops.graph_kernel_count(e.graph.raw_cuda_graph(), part)[1]
               for e in step._graphs.values())


@pytest.mark.gpu
def test_capture_zinc_regression_meter(cuda):
    """One eager call and three replays of InferStep(meter=...) leave the
    meter exactly where four eager updates leave it."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.metrics import RegressionMeter
    from hlhgat.train import InferStep
    torch.manual_seed(0)
    model = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**ZINC_KW).to(cuda).train()
    b = _zinc_batch(5, cuda)
    ops.clear_device_errors()
    meter, eager = RegressionMeter(64, cuda), RegressionMeter(64, cuda)
    with _kept_graphs():
        step = InferStep(model, meter=lambda out, d: meter.update(out, d.y))
        outs = [step(b).clone() for _ in range(4)]
        assert step.stats == {"eager": 1, "replay": 3, "captures": 1}
        assert _meter_kernels(step, "k_collect_rows") == 2
    for o in outs:
        eager.update(o, b.y)
    torch.cuda.synchronize()
    for got, want in ((meter.pred, eager.pred), (meter.y, eager.y)):
        assert int(got.cursor) == int(want.cursor) == 4 * 12
        assert torch.equal(got.buf, want.buf)
    pred = torch.cat(outs).view(-1).cpu().numpy()
    y = b.y.view(-1).repeat(4).cpu().numpy()
    _check_summary(meter.compute(), pred, y, "zinc capture")
    assert _dev_errors() == 0


@pytest.mark.gpu
def test_capture_tsp_f1_meter(cuda):
    import hlhgat
    from hlhgat import ops
    from hlhgat.metrics import F1Meter
    from hlhgat.train import InferStep
    torch.manual_seed(0)
    model = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(**TSP_KW).to(cuda).train()
    b = _tsp_batch((1, 2), cuda)
    ops.clear_device_errors()
    meter, eager = F1Meter(16, cuda), F1Meter(16, cuda)
    with _kept_graphs():
        step = InferStep(model, meter=lambda out, d: meter.update(out[0], d.y, d.num_edge1))
        outs = [step(b)[0].clone() for _ in range(4)]
        assert step.stats == {"eager": 1, "replay": 3, "captures": 1}
        assert _meter_kernels(step, "k_f1_per_graph") == 1
        assert _meter_kernels(step, "k_collect_rows") == 1
    for o in outs:
        eager.update(o, b.y, b.num_edge1, seg_ptr=getattr(b, "seg_ptr_s", None))
    torch.cuda.synchronize()
    assert int(meter.values.cursor) == int(eager.values.cursor) == 8
    assert torch.equal(meter.values.buf, eager.values.buf)
    want = np.concatenate([_f1_ref(o, b)[0] for o in outs])
    assert (_bits(meter.per_graph().cpu().numpy()) == _bits(want)).all()
    assert meter.compute() == float(want.astype(np.float64).mean())
    assert _dev_errors() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zinc", "cifar", "tsp"])
def test_eval_epoch_on_meters(cuda, kind):
    """A two-batch evaluation epoch through InferStep and the meter against
    the reference's test() loop restated with torch on the same outputs."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.metrics import AccuracyMeter, F1Meter, RegressionMeter
    from hlhgat.synthetic import two_level_batch
    from hlhgat.train import InferStep
    torch.manual_seed(0)
    ops.clear_device_errors()
    if kind == "zinc":
        model = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**ZINC_KW)
        batches = [_zinc_batch(s, cuda) for s in (5, 6)]
        meter = RegressionMeter(64, cuda)
        update = lambda out, d: meter.update(out, d.y)  # noqa: E731
    elif kind == "cifar":
        model = hlhgat.HL_HGCNN_CIFAR10SP_dense_int3_attpool(**CIFAR_KW)
        batches = [[x.to(cuda) for x in two_level_batch("cifar", 6, seed=s)] for s in (0, 1)]
        meter = AccuracyMeter(cuda)
        update = lambda out, d: meter.update(out, d[0].y)  # noqa: E731
    else:
        model = hlhgat.HL_HGCNN_TSP_dense_int3_pyr(**TSP_KW)
        batches = [_tsp_batch(s, cuda) for s in ((1, 2), (3, 4))]
        meter = F1Meter(16, cuda)
        update = lambda out, d: meter.update(out[0], d.y, d.num_edge1,  # noqa: E731
                                             seg_ptr=getattr(d, "seg_ptr_s", None))
    model = model.to(cuda).train()
    step = InferStep(model, meter=update)
    outs = []
    for _ in range(2):  # the second epoch replays
        meter.reset()
        outs = []
        for b in batches:
            o = step(b)
            outs.append((o[0] if isinstance(o, tuple) else o).clone())
        got = meter.compute()
    assert step.stats["replay"] >= 2, step.stats
    if kind == "zinc":
        pred = torch.cat(outs).view(-1).cpu()
        y = torch.cat([b.y.view(-1) for b in batches]).cpu()
        assert got["n"] == pred.numel()
        _check_summary(got, pred.numpy(), y.numpy(), "zinc epoch")
        acc = sum(float((o.view(-1).cpu() - b.y.view(-1).cpu()).abs().sum())  # main_zinc...:174
                  for o, b in zip(outs, batches))
        # the loop's own fp32 sums: (n + 2) roundings of 2^-24 each, first order
        assert abs(got["sum_abs"] - acc) <= (pred.numel() + 2) * 2.0 ** -24 * acc
    elif kind == "cifar":
        correct = sum(int((o.cpu().argmax(1) == b[0].y.view(-1).cpu()).sum())
                      for o, b in zip(outs, batches))  # main_cifar10SP...:158
        assert got == correct / sum(o.size(0) for o in outs)
    else:
        y_f1 = np.concatenate([_f1_ref(o, b)[0] for o, b in zip(outs, batches)])
        assert (_bits(meter.per_graph().cpu().numpy()) == _bits(y_f1)).all()
        assert got == float(y_f1.astype(np.float64).mean())
    assert _dev_errors() == 0
