"""CPU restatements (numpy only, no hlhgat import) of the evaluation meters'
kernels (csrc/metrics.hip): what tests/test_eval_meters.py holds the HIP path
and the package's own CPU path to, and what tests/golden/make_golden_meters.py
cross-checks against scikit-learn when it writes meters_small.npz.

f1_per_graph restates torchmetrics' BinaryF1Score() with its defaults
(threshold 0.5), whose formatting step is: if any prediction of the call lies
outside [0, 1] the predictions are logits and go through a sigmoid, then
``pred = p > 0.5``.  torchmetrics is not a dependency of the tests, so that
sigmoid / threshold step is restated here, not called.
"""
from __future__ import annotations

import numpy as np

F1_SIZES = (0, 1, 63, 64, 65, 257, 1000)  # rows per graph: wave and block edges
F1_PAD = 37                               # trailing static-shape padding rows
THRESHOLD_GAP = 1e-3


def seg_ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))]).astype(np.int32)


def format_preds(p):
    """BinaryF1Score's predictions for the logits / probabilities p of ONE
    call (one graph): bool [n]."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = bool(np.all((p >= np.float32(0)) & (p <= np.float32(1))))  # a NaN fails
        if inside:
            return p > np.float32(0.5)
        s = np.float32(1) / (np.float32(1) + np.exp(-p, dtype=np.float32))
        return s > np.float32(0.5)


def f1_per_graph(logits, labels, seg_ptr):
    """(f1 [G] float32, bad) -- bad: some graph holds a label other than 0 / 1
    (counted as a negative)."""
    p = np.asarray(logits, np.float32).reshape(-1)
    y = np.asarray(labels, np.float32).reshape(-1)
    ptr = np.clip(np.asarray(seg_ptr, np.int64), 0, p.size)
    f1 = np.zeros(len(ptr) - 1, np.float32)
    bad = False
    for g in range(len(ptr) - 1):
        pg, yg = p[ptr[g]:ptr[g + 1]], y[ptr[g]:ptr[g + 1]]
        bad = bad or bool(np.any((yg != 0) & (yg != 1)))
        pred, pos = format_preds(pg), yg == 1
        tp = int(np.sum(pred & pos))
        fp = int(np.sum(pred & ~pos))
        fn = int(np.sum(~pred & pos))
        den = 2 * tp + fp + fn
        if den > 0:
            f1[g] = np.float32(2 * tp) / np.float32(den)  # one correctly rounded division
    return f1, bad


def thresholds_clear(logits):
    """True iff every finite, nonzero logit is at least THRESHOLD_GAP away from
    both decision points (0.5 for the plain rule, 0 for the sigmoid rule), so
    an expf that differs in its last bits cannot flip a prediction."""
    p = np.asarray(logits, np.float64).reshape(-1)
    p = p[np.isfinite(p) & (p != 0)]
    return bool(np.all(np.abs(p - 0.5) >= THRESHOLD_GAP) and np.all(np.abs(p) >= THRESHOLD_GAP))


def argmax_rows(x):
    """torch's CPU argmax(x, 1): the first index of the greatest value, a NaN
    counting as greatest."""
    x = np.asarray(x, np.float32)
    out = np.zeros(x.shape[0], np.int64)
    for r in range(x.shape[0]):
        best, arg = x[r, 0], 0
        for j in range(1, x.shape[1]):
            if best != best:
                break
            v = x[r, j]
            if v > best or v != v:
                best, arg = v, j
        out[r] = arg
    return out


def argmax_correct(x, labels):
    """(correct, bad) -- bad: a label outside [0, C) (it matches nothing)."""
    x = np.asarray(x, np.float32)
    y = np.asarray(labels, np.int64).reshape(-1)
    bad = bool(np.any((y < 0) | (y >= x.shape[1])))
    return int(np.sum(argmax_rows(x) == y)), bad


def regression_summary(pred, y):
    """Two passes in np.longdouble over the fp32 inputs: the summary's eight
    quantities plus mae and rmse as `value`, and for each the first-order
    worst-case error of computing it in fp64 as `bound`.

    Every plain sum of N terms gets (N + 4) * 2^-52 * sum |term| (an N-term
    fp64 sum in any order, the terms themselves rounded a few times; 2^-52 is
    twice the unit roundoff).  The centred sums also see the computed mean's
    own error e: sum (a_i - e_p)(b_i - e_y) = sum a_i b_i + N e_p e_y.  The
    quotients and roots propagate the relative errors of their operands plus
    2^-52 for their own roundings."""
    ld = np.longdouble
    p, t = np.asarray(pred, np.float32).astype(ld).reshape(-1), \
        np.asarray(y, np.float32).astype(ld).reshape(-1)
    N = p.size
    u2 = ld(2.0) ** -52
    nan = ld("nan")
    value, bound = {}, {}

    def plain(terms):
        return terms.sum() if N else ld(0), (N + 4) * u2 * np.abs(terms).sum() if N else ld(0)

    d = p - t
    value["n"], bound["n"] = ld(N), ld(0)
    value["sum_abs"], bound["sum_abs"] = plain(np.abs(d))
    value["sum_sq"], bound["sum_sq"] = plain(d * d)
    if N == 0:
        for k in ("mean_pred", "mean_y", "std_pred", "std_y", "corr", "mae", "rmse"):
            value[k], bound[k] = nan, nan
        return value, bound
    value["mae"] = value["sum_abs"] / N
    bound["mae"] = bound["sum_abs"] / N + u2 * value["mae"]
    value["rmse"] = np.sqrt(value["sum_sq"] / N)
    bound["rmse"] = value["rmse"] * ((bound["sum_sq"] / value["sum_sq"] / 2 if value["sum_sq"]
                                      else ld(0)) + u2)
    for k, v in (("mean_pred", p), ("mean_y", t)):
        s, b = plain(v)
        value[k] = s / N
        bound[k] = b / N + u2 * abs(value[k])
    a, b = p - value["mean_pred"], t - value["mean_y"]
    e_p, e_y = bound["mean_pred"], bound["mean_y"]
    spp, b_spp = plain(a * a)
    syy, b_syy = plain(b * b)
    spy, b_spy = plain(a * b)
    b_spp, b_syy, b_spy = b_spp + N * e_p * e_p, b_syy + N * e_y * e_y, b_spy + N * e_p * e_y
    if N < 2:
        for k in ("std_pred", "std_y", "corr"):
            value[k], bound[k] = nan, nan
        return value, bound
    rel = {}
    for k, s, bs in (("std_pred", spp, b_spp), ("std_y", syy, b_syy)):
        value[k] = np.sqrt(s / (N - 1))
        rel[k] = (bs / s / 2 if s else ld(0)) + u2
        bound[k] = value[k] * rel[k]
    den = N * value["std_pred"] * value["std_y"]
    if den == 0:
        value["corr"], bound["corr"] = nan, nan
    else:
        value["corr"] = spy / den
        bound["corr"] = b_spy / den + abs(value["corr"]) * (rel["std_pred"] + rel["std_y"] + u2)
    return value, bound


# ---- the F1 cases of the fixture (inputs; the generator adds the expected f1) -------
def _quantised(rng, n, lo, hi):
    """Multiples of 1/4096 in [lo, hi], kept THRESHOLD_GAP away from 0 and 0.5."""
    v = np.round(rng.uniform(lo, hi, n) * 4096) / 4096
    for c in (0.0, 0.5):
        near = np.abs(v - c) < 2 * THRESHOLD_GAP
        v[near] = c + 3 * THRESHOLD_GAP * np.where(rng.random(near.sum()) < 0.5, -1, 1)
    return np.clip(np.round(v * 4096) / 4096, lo, hi).astype(np.float32)


def f1_cases():
    """name -> (logits [E] fp32, labels [E] fp32, seg_ptr [G + 1] int32); E is
    the graphs' rows plus F1_PAD padding rows that belong to no graph (their
    content must not matter: large logits, label 1)."""
    rng = np.random.default_rng(2501)
    ptr = seg_ptr_of(F1_SIZES)
    rows = int(ptr[-1])

    def pad(p, y):
        return (np.concatenate([p, np.full(F1_PAD, 5.0, np.float32)]),
                np.concatenate([y, np.ones(F1_PAD, np.float32)]))

    def labels(p_pos=0.35):
        return (rng.random(rows) < p_pos).astype(np.float32)

    def seg(g):
        return slice(int(ptr[g]), int(ptr[g + 1]))

    out = {}
    # every logit a probability: the plain threshold; graph 3 (64 rows) has no
    # positive label and no positive prediction: 0 / 0
    p, y = np.clip(_quantised(rng, rows, 0.0, 1.0), 3 * 2 ** -10, 1.0), labels()
    p[seg(3)] = np.minimum(p[seg(3)], np.float32(0.25))
    y[seg(3)] = 0
    out["inside"] = pad(p, y) + (ptr,)
    # one logit of graph 4 (65 rows) outside: that graph alone takes the sigmoid
    p2 = p.copy()
    p2[int(ptr[4]) + 17] = np.float32(1.75)
    out["one_outside"] = pad(p2, labels()) + (ptr,)
    # model-like logits times a 0 / 1 edge mask: exact zeros of both signs;
    # graph 2 (63 rows) is masked entirely (all zeros: inside, plain threshold)
    raw = _quantised(rng, rows, -6.0, 6.0)
    mask = (rng.random(rows) < 0.6).astype(np.float32)
    mask[seg(2)] = 0
    out["masked_zeros"] = pad(raw * mask, labels() * mask) + (ptr,)
    # a NaN in graph 5, +inf in graph 6, -inf in graph 4
    p3 = _quantised(rng, rows, 0.0, 1.0)
    p3[int(ptr[5]) + 100] = np.nan
    p3[int(ptr[6]) + 999] = np.inf
    p3[int(ptr[4])] = -np.inf
    out["nonfinite"] = pad(p3, labels()) + (ptr,)
    # a label of 2 (graph 5): a negative, and the error bit
    y4 = labels()
    y4[int(ptr[5]) + 256] = 2.0
    out["label2"] = pad(_quantised(rng, rows, -3.0, 3.0), y4) + (ptr,)
    return out
