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
"""
from __future__ import annotations

import torch

from . import ops

__all__ = ["eval_ap", "average_precision_cpu"]

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
