"""Golden fixture for the evaluation meters (csrc/metrics.hip: per-graph F1,
argmax accuracy, regression summary).  Build container only (needs
scikit-learn):

    python tests/golden/make_golden_meters.py

Writes meters_small.npz (plain arrays, no pickles):

* f1/<case>/{logits, labels, seg_ptr}: the batches of tests/meters_ref.py's
  f1_cases() -- graphs of 0, 1, 63, 64, 65, 257 and 1000 rows plus padding rows.
* f1/<case>/f1 [G] fp32, f1/<case>/bad: the expected per-graph values.  The
  PREDICTIONS come from meters_ref.format_preds, a restatement of
  torchmetrics' BinaryF1Score formatting step (sigmoid if any logit of the
  graph lies outside [0, 1], then > 0.5): torchmetrics is not installed where
  this runs, so that sigmoid / threshold step is restated, not called.  Given
  those predictions, every value is cross-checked here against
  sklearn.metrics.f1_score(..., zero_division=0).
* acc/{x, labels, argmax, correct}: rows with ties, NaNs, infinities and
  out-of-range labels; argmax is torch's CPU argmax(x, 1).
* reg/{pred, y} fp32 and reg/<quantity> fp64: meters_ref.regression_summary's
  long-double values rounded to fp64.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import meters_ref  # noqa: E402
from make_golden import _save  # noqa: E402


def main():
    from sklearn.metrics import f1_score
    arrays = {}
    for name, (p, y, ptr) in meters_ref.f1_cases().items():
        assert meters_ref.thresholds_clear(p), name
        f1, bad = meters_ref.f1_per_graph(p, y, ptr)
        assert bad == (name == "label2"), name
        for g in range(len(ptr) - 1):
            pg, yg = p[ptr[g]:ptr[g + 1]], y[ptr[g]:ptr[g + 1]]
            if pg.size == 0:
                assert f1[g] == 0
                continue
            sk = f1_score(yg == 1, meters_ref.format_preds(pg), zero_division=0)
            assert np.float32(sk) == f1[g], (name, g, sk, f1[g])
        arrays[f"f1/{name}/logits"] = p
        arrays[f"f1/{name}/labels"] = y.astype(np.uint8)
        arrays[f"f1/{name}/seg_ptr"] = ptr
        arrays[f"f1/{name}/f1"] = f1
        arrays[f"f1/{name}/bad"] = np.bool_(bad)
    # the cases say what they claim to
    c = meters_ref.f1_cases()
    f_in, _ = meters_ref.f1_per_graph(*c["inside"])
    assert f_in[0] == 0 and f_in[3] == 0 and (f_in[[1, 2, 4, 5, 6]] >= 0).all()
    p, y, ptr = c["one_outside"]
    f_one, _ = meters_ref.f1_per_graph(p, y, ptr)
    with np.errstate(over="ignore"):  # every graph through the sigmoid: a per-batch rule
        sig = np.float32(1) / (np.float32(1) + np.exp(-p, dtype=np.float32))
    f_all_sig, _ = meters_ref.f1_per_graph((sig > 0.5).astype(np.float32), y, ptr)
    assert f_one[4] == f_all_sig[4] and f_one[3] != f_all_sig[3] and f_one[5] != f_all_sig[5]
    pz = c["masked_zeros"][0]
    assert np.signbit(pz[pz == 0]).any() and (~np.signbit(pz[pz == 0])).any()

    rng = np.random.default_rng(2502)
    x = (np.round(rng.standard_normal((40, 10)) * 2) / 2).astype(np.float32)  # many ties
    x[3, 4] = np.nan
    x[5, 0] = np.nan
    x[5, 7] = np.nan
    x[6, 9] = np.inf
    x[7, :] = -np.inf
    x[8, :] = 0.25
    x[9, 2], x[9, 6] = 0.0, -0.0
    labels = meters_ref.argmax_rows(x).copy()
    labels[::3] = (labels[::3] + 1) % 10   # wrong on every third row
    labels[11], labels[12] = -1, 10        # out of range: match nothing
    ref = torch.from_numpy(x).argmax(1).numpy()
    assert (ref == meters_ref.argmax_rows(x)).all()
    correct, bad = meters_ref.argmax_correct(x, labels)
    assert bad and correct == int((ref == labels).sum())
    arrays.update({"acc/x": x, "acc/labels": labels, "acc/argmax": ref,
                   "acc/correct": np.int64(correct)})

    pred = (50 + 15 * rng.standard_normal(257)).astype(np.float32)
    y = (0.6 * (pred - 50) + 50 + 12 * rng.standard_normal(257)).astype(np.float32)
    value, _ = meters_ref.regression_summary(pred, y)
    arrays.update({"reg/pred": pred, "reg/y": y})
    arrays.update({f"reg/{k}": np.float64(v) for k, v in value.items()})
    pt, yt = torch.from_numpy(pred), torch.from_numpy(y)
    z = ((pt - pt.mean()) / pt.std()) * ((yt - yt.mean()) / yt.std())
    assert abs(float(z.mean()) - float(value["corr"])) < 1e-5   # the notebook's fp32 corr
    assert abs(float((pt - yt).abs().sum()) - float(value["sum_abs"])) < 1e-4 * 257 * 15
    _save("meters_small", **arrays)


if __name__ == "__main__":
    main()
