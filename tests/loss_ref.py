"""numpy fp64 restatement of the reduced training losses of csrc/loss.hip
(include/hlhgat.h, "reduced training losses"): loss,
input gradient and the integer by-products.  The GPU tests compare the
kernels against it; tests/golden/losses_small.npz (the reference's own
FocalLoss and torch's CrossEntropyLoss in fp64) pins it down."""
import numpy as np


def _log_sigmoid(x):
    return np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    z = np.exp(-np.abs(x))
    return np.where(x < 0, z / (1.0 + z), 1.0 / (1.0 + z))


def included(y, mask=None, ignore_nan=False):
    """The included set I as a boolean array of y's shape."""
    y = np.asarray(y, dtype=np.float64)
    inc = np.ones(y.shape, bool) if mask is None else np.asarray(mask) != 0
    if ignore_nan:
        inc = inc & ~np.isnan(y)
    return inc


def bce(x, y, mask=None, ignore_nan=False, reduction="mean", focal=None, gout=1.0):
    """(loss, dx, stats) of the BCE-with-logits reduction over the included
    elements.  reduction: "mean" | "sum"; focal = (alpha, gamma, scale) turns
    the mean b into scale * alpha * (1 - exp(-b))**gamma * b.  stats = int64
    [cnt, tp, fp, fn] (prediction x > 0, positive label y > 0.5).  cnt == 0:
    loss 0 and dx 0 (the library's convention; torch gives NaN)."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    inc = included(y, mask, ignore_nan)
    xi, yi = x[inc], y[inc]
    cnt = int(inc.sum())
    pred, pos = xi > 0, yi > 0.5
    stats = np.array([cnt, (pred & pos).sum(), (pred & ~pos).sum(), (~pred & pos).sum()],
                     dtype=np.int64)
    dx = np.zeros(x.shape, dtype=np.float64)
    if cnt == 0:
        return 0.0, dx, stats
    S = float(((1.0 - yi) * xi - _log_sigmoid(xi)).sum())
    if focal is not None:
        assert reduction == "mean"
        alpha, gamma, scale = (float(v) for v in focal)
        b = S / cnt
        om, pt = -np.expm1(-b), np.exp(-b)
        if gamma == 0.0:
            loss, c = scale * alpha * b, scale * alpha / cnt
        else:
            loss = scale * alpha * om ** gamma * b
            c = scale * alpha * (om ** gamma + gamma * om ** (gamma - 1.0) * pt * b) / cnt
    elif reduction == "sum":
        loss, c = S, 1.0
    elif reduction == "mean":
        loss, c = S / cnt, 1.0 / cnt
    else:
        raise ValueError(reduction)
    dx[inc] = gout * c * (_sigmoid(xi) - yi)
    return float(loss), dx, stats


def cross_entropy(x, label, ignore_index=-100, reduction="mean", gout=1.0):
    """(loss, dx, stats) of the row-wise cross-entropy of x [R, C]; a label
    that is ignore_index or outside [0, C) leaves its row out.  stats = int64
    [cnt, correct] (lowest-index argmax equals the label).  cnt == 0: loss 0
    and dx 0."""
    x = np.asarray(x, dtype=np.float64)
    label = np.asarray(label, dtype=np.int64)
    R, C = x.shape
    valid = (label != ignore_index) & (label >= 0) & (label < C)
    cnt = int(valid.sum())
    dx = np.zeros((R, C), dtype=np.float64)
    if cnt == 0:
        return 0.0, dx, np.array([0, 0], dtype=np.int64)
    xv, lv = x[valid], label[valid]
    m = xv.max(axis=1, keepdims=True)
    e = np.exp(xv - m)
    se = e.sum(axis=1, keepdims=True)
    rows = np.arange(cnt)
    loss_r = np.log(se[:, 0]) + m[:, 0] - xv[rows, lv]
    correct = int((xv.argmax(axis=1) == lv).sum())  # numpy argmax: the lowest index
    c = gout if reduction == "sum" else gout / cnt
    g = e / se
    g[rows, lv] -= 1.0
    dx[valid] = c * g
    loss = float(loss_r.sum()) if reduction == "sum" else float(loss_r.sum()) / cnt
    return loss, dx, np.array([cnt, correct], dtype=np.int64)
