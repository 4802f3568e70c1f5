"""Evaluation metrics of the reference's training scripts.

``eval_ap(y_true, y_pred)`` is lib/Hodge_Dataset.py:73-94 of
deepika090/HL-HGAT: scikit-learn's ``average_precision_score`` per class over
the rows whose label is not NaN, averaged over the classes that have at least
one label 1 and one label 0.  On ROCm tensors the per-class values come from
``ops.average_precision`` (csrc/metrics.hip), the mean over the valid classes
is taken on the device, and one small read brings the result to the host.  On
CPU tensors the same definition is evaluated with torch in fp64 (no
scikit-learn import).

Per class, with the m labelled rows sorted by fp32 score, descending, and rows
of equal score (-0.0 == +0.0) forming one threshold group k that ends at the
1-based row r_k with tp_k positives so far, P positives in all:

    AP = sum_k ((tp_k - tp_{k-1}) / P) * (tp_k / r_k)

The other test() loops of the reference run on meters whose ``update`` is a
few launches without a host synchronisation (so it captures into InferStep's
graph and replays with it) and whose ``compute`` is one small read at the end
of the epoch:

    Collector         y_pred.extend(out) / torch.cat(y_preds) on the device
    F1Meter           the TSP loop's per-graph BinaryF1Score and its mean
    AccuracyMeter     the CIFAR loop's argmax(out, 1) == y count
    RegressionMeter   ZINC's summed |out - y|; the notebook's L1, RMSE and
                      mean(z(pred) * z(y))

On CPU tensors every meter evaluates the same definitions with torch and
raises RuntimeError where the device path raises the device error word.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops

__all__ = ["eval_ap", "average_precision_cpu", "Collector", "F1Meter", "AccuracyMeter",
           "RegressionMeter", "f1_per_graph_cpu", "regression_summary_cpu"]

_NO_VALID = "No positively labeled data available. Cannot compute Average Precision."


def average_precision_cpu(pred: torch.Tensor, label: torch.Tensor):
    """(ap [C] fp64, counts [C, 3] int32) of ops.average_precision, evaluated
    on the host with torch in fp64 (any device's tensors are brought over)."""
    pred = pred.detach().to("cpu", torch.float32)
    label = label.detach().to("cpu", torch.float32)
    if pred.dim() != 2 or pred.shape != label.shape:
        raise RuntimeError(f"average_precision wants pred and label [n, C], got "
                           f"{tuple(pred.shape)} and {tuple(label.shape)}")
    C = pred.size(1)
    ap = torch.full((C,), float("nan"), dtype=torch.float64)
    counts = torch.zeros((C, 3), dtype=torch.int32)
    for c in range(C):
        y = label[:, c]
        keep = ~torch.isnan(y)
        y, s = y[keep], pred[keep, c] + 0.0  # + 0.0: -0.0 becomes +0.0
        pos = y == 1
        P, Z = int(pos.sum()), int((y == 0).sum())
        counts[c] = torch.tensor([y.numel(), P, Z], dtype=torch.int32)
        if P == 0 or Z == 0 or not bool(torch.isfinite(s).all()):
            continue
        order = torch.argsort(s, descending=True, stable=True)
        s, tp = s[order], torch.cumsum(pos[order].to(torch.float64), 0)
        end = torch.ones(s.numel(), dtype=torch.bool)
        end[:-1] = s[1:] != s[:-1]
        tp_k = tp[end]
        r_k = torch.nonzero(end).view(-1).to(torch.float64) + 1.0
        d = tp_k - torch.cat([tp_k.new_zeros(1), tp_k[:-1]])
        ap[c] = ((d / P) * (tp_k / r_k)).sum()
    return ap, counts


def eval_ap(y_true: torch.Tensor, y_pred: torch.Tensor) -> float:
    """Average precision averaged over the classes: the reference's
    ``eval_ap(y_true, y_pred)`` (its argument order and its result).  Raises
    the reference's RuntimeError when no class has both a 1 and a 0, and
    ValueError when a labelled row has a non-finite score (scikit-learn
    raises there)."""
    if y_pred.is_cuda:
        ap, counts = ops.average_precision(y_pred, y_true)
    else:
        ap, counts = average_precision_cpu(y_pred, y_true)
    valid = (counts[:, 1] > 0) & (counts[:, 2] > 0)
    nvalid = valid.sum()
    # NaN of a valid class (a non-finite score) must reach the mean: where(), not nansum
    mean = torch.where(valid, ap, torch.zeros_like(ap)).sum() / nvalid.to(torch.float64)
    nv, m = torch.stack([nvalid.to(torch.float64), mean]).tolist()  # the one D2H read
    if nv == 0:
        raise RuntimeError(_NO_VALID)
    if m != m:
        raise ValueError("eval_ap: a labelled row has a non-finite score (Input contains NaN or "
                         "infinity)")
    return m


# ----------------------------------------------------------------------------
# the CPU restatements of the meters' kernels
# ----------------------------------------------------------------------------
def f1_per_graph_cpu(logits: torch.Tensor, label: torch.Tensor, seg_ptr) -> torch.Tensor:
    """f1 [G] fp32 of ops.f1_per_graph, evaluated on the host with torch.  A
    label other than 0 or 1 raises RuntimeError."""
    p = logits.detach().to("cpu", torch.float32).reshape(-1)
    y = label.detach().to("cpu", torch.float32).reshape(-1)
    ptr = [min(max(int(v), 0), p.numel()) for v in seg_ptr]
    out = torch.zeros(max(len(ptr) - 1, 0), dtype=torch.float32)
    for g in range(out.numel()):
        pg, yg = p[ptr[g]:ptr[g + 1]], y[ptr[g]:ptr[g + 1]]
        if not bool(((yg == 0) | (yg == 1)).all()):
            raise RuntimeError("hlhgat: F1Meter: a label that is neither 0 nor 1")
        inside = bool(((pg >= 0) & (pg <= 1)).all())
        pred = (pg > 0.5) if inside else (1.0 / (1.0 + torch.exp(-pg)) > 0.5)
        pos = yg == 1
        tp = int((pred & pos).sum())
        den = int(pred.sum()) + int(pos.sum())  # 2tp + fp + fn
        if den > 0:
            out[g] = torch.tensor(2 * tp, dtype=torch.float32) / torch.tensor(
                den, dtype=torch.float32)
    return out


def regression_summary_cpu(pred: torch.Tensor, y: torch.Tensor) -> dict:
    """The entries of ops.regression_summary (ops.REGRESSION_FIELDS) over all
    of pred / y, evaluated on the host with torch in fp64, two passes."""
    p = pred.detach().to("cpu", torch.float32).reshape(-1).double()
    t = y.detach().to("cpu", torch.float32).reshape(-1).double()
    n = p.numel()
    nan = float("nan")
    d = p - t
    mp, my = (float(p.mean()), float(t.mean())) if n else (nan, nan)
    a, b = p - mp, t - my
    sp = float((a * a).sum() / (n - 1)) ** 0.5 if n > 1 else nan
    sy = float((b * b).sum() / (n - 1)) ** 0.5 if n > 1 else nan
    den = n * (sp * sy) if n > 1 else nan
    corr = (float((a * b).sum()) / den if den != 0 else nan) if n > 1 else nan
    return dict(zip(ops.REGRESSION_FIELDS, [float(n), float(d.abs().sum()), float((d * d).sum()),
                                            mp, my, sp, sy, corr]))


def _device(device) -> torch.device:
    if device is None:
        return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() \
            else torch.device("cpu")
    return torch.device(device)


class Collector:
    """The device-side ``y_pred.extend(out)`` (OHBM_DEMO.ipynb) and the
    ``torch.cat`` of the peptides loop's ``y_preds`` / ``y_trues``
    (main_pepfunc...:201-225): a buffer [capacity, width] fp32 and a cursor,
    both allocated here, outside any graph capture.

    ``append(x)`` appends the rows of x ([n, width], or [n] when width is 1)
    in one launch (ops.collect_rows) and advances the cursor on the device: no
    synchronisation, and a replayed append lands behind the previous one.
    Rows that do not fit are not appended and raise the device error word
    (RuntimeError at once on CPU tensors).  ``rows()`` reads the cursor (the
    one synchronisation) and returns the filled part as a view; ``reset()``
    starts the next epoch."""

    def __init__(self, capacity: int, width: int = 1, device=None):
        if capacity < 0 or width < 1:
            raise ValueError(f"Collector: capacity {capacity} < 0 or width {width} < 1")
        self.device = _device(device)
        self.capacity, self.width = int(capacity), int(width)
        self.buf = torch.zeros((self.capacity, self.width), dtype=torch.float32,
                               device=self.device)
        self.cursor = torch.zeros(1, dtype=torch.int64, device=self.device)

    def append(self, x: torch.Tensor) -> None:
        if self.device.type == "cuda":
            ops.collect_rows(x if x.dtype == torch.float32 else x.float(), self.buf, self.cursor)
            return
        x = x.detach().to(torch.float32)
        if x.dim() == 1 and self.width == 1:
            x = x.view(-1, 1)
        if x.dim() != 2 or x.size(1) != self.width or x.device != self.device:
            raise RuntimeError(f"Collector: x {tuple(x.shape)} on {x.device} does not match the "
                               f"buffer [{self.capacity}, {self.width}] on {self.device}")
        c, n = int(self.cursor), x.size(0)
        if c + n > self.capacity:
            raise RuntimeError(f"Collector: {n} rows do not fit behind {c} of {self.capacity}; "
                               f"none was appended")
        self.buf[c:c + n] = x
        self.cursor += n

    def rows(self) -> torch.Tensor:
        n = int(self.cursor.item())  # the one read; it waits for the appends
        if self.device.type == "cuda":
            ops.check_device_errors(sync=False)
        return self.buf[:n]

    def reset(self) -> None:
        self.cursor.zero_()


class F1Meter:
    """The TSP test() loop's metric (main_TSP_HL_HGCNN_dense_int3_pyr.py:
    331-354): BinaryF1Score() of every graph, collected over the epoch, and
    their mean.  ``update(logits, y, num_edge1)``: one launch for the batch's
    per-graph values (ops.f1_per_graph) and one to collect them; seg_ptr (the
    batch's ``seg_ptr_s``) spares the offsets' cumsum.  ``compute()`` is
    ``y_f1.mean()`` in fp64: one read of the collected values, the mean taken
    on the host (numpy's pairwise sum, a fixed order)."""

    def __init__(self, capacity_graphs: int, device=None):
        self.values = Collector(capacity_graphs, 1, device)
        self.device = self.values.device

    def update(self, logits: torch.Tensor, y: torch.Tensor, num_edge1: torch.Tensor,
               seg_ptr: Optional[torch.Tensor] = None) -> None:
        if seg_ptr is None:
            seg_ptr = torch.zeros(num_edge1.numel() + 1, dtype=torch.int32, device=self.device)
            seg_ptr[1:] = torch.cumsum(num_edge1.to(self.device).view(-1), 0)
        if self.device.type == "cuda":
            f1 = ops.f1_per_graph(logits, y if y.dtype == torch.float32 else y.float(), seg_ptr)
        else:
            f1 = f1_per_graph_cpu(logits, y, seg_ptr.tolist())
        self.values.append(f1)

    def per_graph(self) -> torch.Tensor:
        """The collected per-graph values (a view; one cursor read)."""
        return self.values.rows().view(-1)

    def compute(self) -> float:
        v = self.values
        both = torch.cat([v.cursor.double(), v.buf.view(-1).double()]).cpu().numpy()  # the read
        if self.device.type == "cuda":
            ops.check_device_errors(sync=False)
        n = int(both[0])
        return float(both[1:1 + n].mean()) if n else float("nan")

    def reset(self) -> None:
        self.values.reset()


class AccuracyMeter:
    """The CIFAR test() loop's metric (main_cifar10SP_HL_HGCNN_dense_int3_attpool
    .py:146-161): ``update(out, y)`` adds the rows whose argmax is their label
    and the number of rows to two device counters in one launch
    (ops.argmax_correct); ``compute()`` reads both and returns correct / n."""

    def __init__(self, device=None):
        self.device = _device(device)
        self.state = torch.zeros(2, dtype=torch.int64, device=self.device)  # correct, rows

    def update(self, out: torch.Tensor, y: torch.Tensor) -> None:
        y = y.reshape(-1)
        if self.device.type == "cuda":
            ops.argmax_correct(out, y if y.dtype == torch.int64 else y.long(), self.state[0:1],
                               self.state[1:2])
            return
        y = y.long()
        if out.dim() != 2 or y.numel() != out.size(0):
            raise RuntimeError(f"AccuracyMeter: out {tuple(out.shape)} and y {tuple(y.shape)}")
        if bool(((y < 0) | (y >= out.size(1))).any()):
            raise RuntimeError(f"hlhgat: AccuracyMeter: a label outside [0, {out.size(1)})")
        self.state[0] += int((out.detach().argmax(1) == y).sum())
        self.state[1] += out.size(0)

    def compute(self) -> float:
        correct, n = self.state.tolist()  # the read
        if self.device.type == "cuda":
            ops.check_device_errors(sync=False)
        return correct / n if n else float("nan")

    def reset(self) -> None:
        self.state.zero_()


class RegressionMeter:
    """ZINC's test() loop (main_zinc_HL_HGCNN_dense_int3_pyr.py:165-177) and
    the notebook's train / test cells (OHBM_DEMO.ipynb): ``update(out, y)``
    collects both columns (two launches); ``compute()`` runs
    ops.regression_summary over them and reads its eight numbers: a dict with
    ``mae`` = sum |out - y| / N (ZINC's ``acc / N``; the caller applies its
    ``* 2.0109``), ``rmse`` = sqrt(sum (out - y)^2 / N), ``corr`` =
    mean(z(pred) * z(y)) with the unbiased standard deviations, and the
    entries of ops.REGRESSION_FIELDS (n as an int)."""

    def __init__(self, capacity: int, device=None):
        self.pred = Collector(capacity, 1, device)
        self.y = Collector(capacity, 1, self.pred.device)
        self.device = self.pred.device

    def update(self, out: torch.Tensor, y: torch.Tensor) -> None:
        if out.numel() != y.numel():
            raise RuntimeError(f"RegressionMeter: out {tuple(out.shape)} and y {tuple(y.shape)}")
        self.pred.append(out if out.dim() == 2 and out.size(1) == 1 else out.reshape(-1))
        self.y.append(y if y.dim() == 2 and y.size(1) == 1 else y.reshape(-1))

    def compute(self) -> dict:
        if self.device.type == "cuda":
            s = ops.regression_summary(self.pred.buf.view(-1), self.y.buf.view(-1),
                                       self.pred.cursor)
            r = dict(zip(ops.REGRESSION_FIELDS, s.tolist()))  # the read
            ops.check_device_errors(sync=False)
        else:
            r = regression_summary_cpu(self.pred.rows(), self.y.rows())
        n = r["n"]
        r["mae"] = r["sum_abs"] / n if n else float("nan")
        r["rmse"] = (r["sum_sq"] / n) ** 0.5 if n else float("nan")
        r["n"] = int(n)
        return r

    def reset(self) -> None:
        self.pred.reset()
        self.y.reset()
