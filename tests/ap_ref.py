"""numpy fp64 restatement of the per-class average precision of
csrc/metrics.hip (include/hlhgat.h, "evaluation metrics"; DESIGN.md section
24) and of the reference's eval_ap mean over the valid classes.  The GPU
tests compare the kernels against tests/golden/ap_small.npz (the reference's
own eval_ap and scikit-learn's average_precision_score); that fixture pins
this restatement down too."""
import numpy as np

NO_VALID = "No positively labeled data available. Cannot compute Average Precision."


def average_precision(pred, label):
    """(ap [C] float64, counts [C, 3] int32): per column, over the rows whose
    label is not NaN, a stable sort by -score, the cumulative sum of the
    positives, and one threshold group per distinct score (-0.0 == +0.0):
    AP = sum_k ((tp_k - tp_{k-1}) / P) * (tp_k / r_k).  counts = labelled
    rows, labels == 1, labels == 0; a class without a 1 or without a 0, or
    with a non-finite score in a labelled row, is NaN."""
    pred = np.asarray(pred, dtype=np.float32)
    label = np.asarray(label, dtype=np.float32)
    C = pred.shape[1]
    ap = np.full(C, np.nan, dtype=np.float64)
    counts = np.zeros((C, 3), dtype=np.int32)
    for c in range(C):
        keep = ~np.isnan(label[:, c])
        y = label[keep, c]
        s = pred[keep, c].astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0
        pos = y == 1
        P, Z = int(pos.sum()), int((y == 0).sum())
        counts[c] = (y.size, P, Z)
        if P == 0 or Z == 0 or not np.isfinite(s).all():
            continue
        order = np.argsort(-s, kind="stable")
        s = s[order]
        tp = np.cumsum(pos[order].astype(np.float64))
        end = np.r_[s[1:] != s[:-1], True]
        tp_k = tp[end]
        r_k = np.flatnonzero(end).astype(np.float64) + 1.0
        d = np.diff(np.r_[0.0, tp_k])
        ap[c] = np.sum((d / P) * (tp_k / r_k))
    return ap, counts


def eval_ap(y_true, y_pred):
    """The reference's eval_ap(y_true, y_pred): the mean of the valid classes'
    average precision, summed in class order."""
    ap, counts = average_precision(y_pred, y_true)
    vals = [float(ap[c]) for c in range(len(ap)) if counts[c, 1] > 0 and counts[c, 2] > 0]
    if not vals:
        raise RuntimeError(NO_VALID)
    return sum(vals) / len(vals)
