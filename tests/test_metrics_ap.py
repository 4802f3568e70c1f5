"""Average precision on the device (csrc/metrics.hip, hlhgat.metrics.eval_ap)
against tests/golden/ap_small.npz: the reference's eval_ap and scikit-learn's
average_precision_score on small cases (ties across a 256-row chunk boundary,
all-equal scores, signed zeros, NaN labels and invalid classes, a multi-chunk
class, a column block of wider matrices).

The GPU bound per valid class is |ap - fixture| <= (m + 4) * 2^-52 with m the
class's labelled rows: the worst-case rounding of an m-term fp64 sum of terms
in [0, 1] plus two correctly rounded divisions per term (1.1e-12 at m = 5000).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import ap_ref
from conftest import load_golden

CASES = ("n2", "n257_ties", "all_ties", "signed_zero", "nan10", "n5000", "strided")


@pytest.fixture(scope="module")
def gold():
    return load_golden("ap_small")


def _inputs(gold, case):
    """(pred, label) as torch CPU tensors; "strided" as column blocks of the
    wide matrices (non-contiguous views)."""
    if case == "strided":
        c0p, c0l = (int(v) for v in gold["strided/col0"])
        pw = torch.from_numpy(gold["strided/pred_wide"])
        lw = torch.from_numpy(gold["strided/label_wide"])
        return pw[:, c0p:c0p + 10], lw[:, c0l:c0l + 10]
    return torch.from_numpy(gold[f"{case}/pred"]), torch.from_numpy(gold[f"{case}/label"])


def _check(ap, counts, gold, case, bound_of):
    ref, cnt = gold[f"{case}/ap"], gold[f"{case}/counts"]
    ap, counts = np.asarray(ap), np.asarray(counts)
    assert counts.dtype == np.int32 and np.array_equal(counts, cnt), (case, counts, cnt)
    assert np.array_equal(np.isnan(ap), np.isnan(ref)), (case, ap, ref)
    for c in range(len(ref)):
        if not np.isnan(ref[c]):
            err = abs(float(ap[c]) - float(ref[c]))
            print(f"{case} class {c}: m={cnt[c, 0]} |diff|={err:.3e} bound={bound_of(cnt[c, 0]):.3e}")
            assert err <= bound_of(cnt[c, 0]), (case, c, err)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_ap_ref_reproduces_fixture(gold, case):
    pred, label = _inputs(gold, case)
    ap, counts = ap_ref.average_precision(pred.numpy(), label.numpy())
    _check(ap, counts, gold, case, lambda m: 1e-12)
    assert abs(ap_ref.eval_ap(label.numpy(), pred.numpy()) - float(gold[f"{case}/eval_ap"])) <= 1e-12


def test_fixture_cases_are_what_they_claim(gold):
    assert float(gold["signed_zero/ap"][0]) == 0.5
    assert abs(float(gold["all_ties/ap"][0]) - 1.0 / 3.0) <= 1e-15
    assert np.flatnonzero(np.isnan(gold["nan10/ap"])).tolist() == [2, 5, 8]
    vals = gold["nan10/ap"][~np.isnan(gold["nan10/ap"])]
    assert len(vals) == 7 and abs(vals.mean() - float(gold["nan10/eval_ap"])) <= 1e-15


@pytest.mark.parametrize("case", CASES)
def test_eval_ap_cpu_reproduces_fixture(gold, case):
    from hlhgat import metrics
    pred, label = _inputs(gold, case)
    ap, counts = metrics.average_precision_cpu(pred, label)
    _check(ap.numpy(), counts.numpy(), gold, case, lambda m: 1e-12)
    got = metrics.eval_ap(label, pred)
    assert isinstance(got, float)
    assert abs(got - float(gold[f"{case}/eval_ap"])) <= 1e-12


def test_eval_ap_no_valid_class_raises_reference_error():
    import hlhgat
    pred = torch.randn(6, 2)
    label = torch.tensor([[1.0, float("nan")]] * 6)  # no zeros; all unlabelled
    with pytest.raises(RuntimeError, match="No positively labeled data available. Cannot "
                                           "compute Average Precision."):
        hlhgat.eval_ap(label, pred)
    with pytest.raises(RuntimeError, match="No positively labeled data"):
        ap_ref.eval_ap(label.numpy(), pred.numpy())


def test_eval_ap_cpu_nonfinite_score_raises_value_error():
    from hlhgat import metrics
    pred = torch.tensor([[0.5], [float("inf")], [0.1]])
    label = torch.tensor([[1.0], [0.0], [0.0]])
    with pytest.raises(ValueError):
        metrics.eval_ap(label, pred)


def test_capi_rejects_bad_arguments_before_any_launch():
    """NULL pointers, n < 0 and an undersized workspace are refused on the
    host (no GPU needed: nothing is launched or dereferenced)."""
    from hlhgat import _lib
    L = _lib.LIB
    n, Cc = 300, 4
    need = L.hlhgat_average_precision_workspace_bytes(n, Cc)
    assert need >= 2 * 8 * n * Cc + 2 * n * Cc
    assert L.hlhgat_average_precision_workspace_bytes(-1, Cc) == 0
    buf = (C.c_char * 4096)()
    a = C.addressof(buf)
    a += (-a) % 256
    assert L.hlhgat_average_precision(None, Cc, a, Cc, n, Cc, a, a, a, need, None) == 1
    assert b"NULL" in L.hlhgat_last_error()
    assert L.hlhgat_average_precision(a, Cc, None, Cc, n, Cc, a, a, a, need, None) == 1
    assert L.hlhgat_average_precision(a, Cc, a, Cc, n, Cc, None, a, a, need, None) == 1
    assert L.hlhgat_average_precision(a, Cc, a, Cc, n, Cc, a, None, a, need, None) == 1
    assert L.hlhgat_average_precision(a, Cc, a, Cc, n, Cc, a, a, None, need, None) == 1
    assert L.hlhgat_average_precision(a, Cc, a, Cc, -1, Cc, a, a, a, need, None) == 1
    assert b"< 0" in L.hlhgat_last_error()
    assert L.hlhgat_average_precision(a, Cc - 1, a, Cc, n, Cc, a, a, a, need, None) == 1
    assert b"stride" in L.hlhgat_last_error()
    assert L.hlhgat_average_precision(a, Cc, a, Cc, n, Cc, a, a, a, need - 1, None) == 1
    assert b"workspace too small" in L.hlhgat_last_error()


def test_ops_average_precision_has_no_cpu_fallback():
    from hlhgat import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.average_precision(torch.randn(4, 2), torch.zeros(4, 2))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _bound(m):
    return (int(m) + 4) * 2.0 ** -52


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_average_precision_matches_fixture(cuda, gold, case):
    from hlhgat import ops
    pred, label = _inputs(gold, case)
    pd, ld = pred.to(cuda), label.to(cuda)
    if case == "strided":  # read in place through the row strides
        wide_p, wide_l = torch.from_numpy(gold["strided/pred_wide"]).to(cuda), \
            torch.from_numpy(gold["strided/label_wide"]).to(cuda)
        c0p, c0l = (int(v) for v in gold["strided/col0"])
        pd, ld = wide_p[:, c0p:c0p + 10], wide_l[:, c0l:c0l + 10]
        assert not pd.is_contiguous() and not ld.is_contiguous()
    ops.clear_device_errors()
    ap, counts = ops.average_precision(pd, ld)
    assert ap.dtype == torch.float64 and ap.is_cuda and counts.shape == (pred.size(1), 3)
    ap2, counts2 = ops.average_precision(pd, ld)
    torch.cuda.synchronize()
    assert ops.device_errors() == 0
    _check(ap.cpu().numpy(), counts.cpu().numpy(), gold, case, _bound)
    # two calls are bitwise equal
    assert torch.equal(ap.view(torch.int64), ap2.view(torch.int64))
    assert torch.equal(counts, counts2)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["nan10", "n5000", "n257_ties"])
def test_eval_ap_gpu_matches_cpu(cuda, gold, case):
    import hlhgat
    pred, label = _inputs(gold, case)
    cpu = hlhgat.eval_ap(label, pred)
    gpu = hlhgat.eval_ap(label.to(cuda), pred.to(cuda))
    m = int(gold[f"{case}/counts"][:, 0].max())
    print(f"{case}: cpu {cpu!r} gpu {gpu!r} |diff| {abs(cpu - gpu):.3e}")
    assert isinstance(gpu, float) and abs(cpu - gpu) <= _bound(m)
    assert abs(gpu - float(gold[f"{case}/eval_ap"])) <= _bound(m)


@pytest.mark.gpu
def test_single_row_is_invalid(cuda):
    from hlhgat import ops
    ap, counts = ops.average_precision(torch.tensor([[0.7]], device=cuda),
                                       torch.tensor([[1.0]], device=cuda))
    assert math.isnan(float(ap[0])) and counts.cpu().tolist() == [[1, 1, 0]]


@pytest.mark.gpu
def test_bad_label_raises_metric_bit_only(cuda):
    """A label of 2: HLHGAT_DEVERR_METRIC_LABEL in the device error word, the
    row counted as a negative (in neither the positives nor the zeros), and
    nothing else goes wrong."""
    from hlhgat import _lib, ops
    pred = torch.tensor([[0.9], [0.8], [0.1], [0.4]], device=cuda)
    label = torch.tensor([[1.0], [2.0], [0.0], [1.0]], device=cuda)
    ops.clear_device_errors()
    try:
        ap, counts = ops.average_precision(pred, label)
        torch.cuda.synchronize()
        w = C.c_uint32(0)
        assert _lib.LIB.hlhgat_device_errors(C.byref(w)) == 0
        assert w.value == _lib.DEVERR_METRIC_LABEL == 8
        with pytest.raises(RuntimeError, match="average_precision"):
            ops.check_device_errors()
    finally:
        ops.clear_device_errors()
    assert ops.device_errors() == 0
    assert counts.cpu().tolist() == [[4, 2, 1]]
    # order 0.9(+) 0.8(-) 0.4(+) 0.1(-): AP = 1/2 * 1/1 + 1/2 * 2/3
    assert abs(float(ap[0]) - (0.5 + 1.0 / 3.0)) <= _bound(4)


@pytest.mark.gpu
def test_metric_bit_keeps_a_bit_raised_before(cuda):
    """The metric's report keeps what an earlier kernel on the stream
    reported: the cross-entropy label bit (4) and the metric bit (8)."""
    from hlhgat import _lib, ops
    ops.clear_device_errors()
    try:
        ops.cross_entropy(torch.randn(3, 4, device=cuda), torch.tensor([0, 7, 1], device=cuda))
        ops.average_precision(torch.tensor([[0.9], [0.1]], device=cuda),
                              torch.tensor([[3.0], [0.0]], device=cuda))
        torch.cuda.synchronize()
        assert ops.device_errors() == _lib.DEVERR_LABEL | _lib.DEVERR_METRIC_LABEL == 12
    finally:
        ops.clear_device_errors()


@pytest.mark.gpu
def test_workspace_cache_is_bounded(cuda):
    """Eager calls with a different n each time keep at most _AP_WS_MAX
    workspaces; results stay right after evictions."""
    from hlhgat import ops
    g = torch.Generator().manual_seed(9)
    for n in range(20, 20 + 3 * ops._AP_WS_MAX):
        pred = torch.randn(n, 2, generator=g)
        label = (torch.rand(n, 2, generator=g) < 0.5).float()
        label[0], label[1] = 1.0, 0.0
        ap, counts = ops.average_precision(pred.to(cuda), label.to(cuda))
        ref, cnt = ap_ref.average_precision(pred.numpy(), label.numpy())
        assert np.array_equal(counts.cpu().numpy(), cnt)
        assert np.abs(ap.cpu().numpy() - ref).max() <= _bound(n)
        assert len(ops._AP_WS) <= ops._AP_WS_MAX
    assert len(ops._AP_WS) == ops._AP_WS_MAX


@pytest.mark.gpu
def test_infinite_score_raises_value_error(cuda):
    import hlhgat
    from hlhgat import ops
    pred = torch.tensor([[0.5, 0.2], [float("inf"), 0.3], [0.1, 0.9]], device=cuda)
    label = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]], device=cuda)
    ap, _ = ops.average_precision(pred, label)
    assert math.isnan(float(ap[0])) and float(ap[1]) == 0.5
    with pytest.raises(ValueError):
        hlhgat.eval_ap(label, pred)
    # an infinite score in an UNLABELLED row enters nothing
    label[1, 0] = float("nan")
    label[2, 0] = 0.0
    assert hlhgat.eval_ap(label, pred) == 0.75


@pytest.mark.gpu
def test_average_precision_captures_and_replays(cuda, gold):
    """Captured under torch.cuda.graph on static [257, 4] buffers and replayed
    after new data is copied in: the bits of the eager call on that data."""
    from hlhgat import ops
    pred, label = _inputs(gold, "n257_ties")
    sp, sl = pred.to(cuda).clone(), label.to(cuda).clone()
    g2 = torch.Generator().manual_seed(5)
    new_pred = (torch.randn(257, 4, generator=g2) * 2).round() / 2
    new_label = (torch.rand(257, 4, generator=g2) < 0.4).float()
    new_label[torch.rand(257, 4, generator=g2) < 0.2] = float("nan")
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(s):
        ops.average_precision(sp, sl)  # warm-up on the capture stream
    torch.cuda.current_stream(cuda).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ap_g, cnt_g = ops.average_precision(sp, sl)
    sp.copy_(new_pred.to(cuda))
    sl.copy_(new_label.to(cuda))
    graph.replay()
    torch.cuda.synchronize()
    ap_e, cnt_e = ops.average_precision(new_pred.to(cuda), new_label.to(cuda))
    torch.cuda.synchronize()
    assert torch.equal(ap_g.view(torch.int64), ap_e.view(torch.int64))
    assert torch.equal(cnt_g, cnt_e)
    ref, cnt = ap_ref.average_precision(new_pred.numpy(), new_label.numpy())
    assert np.array_equal(cnt_e.cpu().numpy(), cnt)
    assert np.abs(ap_e.cpu().numpy() - ref).max() <= _bound(257)
