"""Golden fixture for the device average precision (csrc/metrics.hip), generated
by the REFERENCE's own eval_ap (lib/Hodge_Dataset.py:73-94) and scikit-learn's
average_precision_score.  Build container only (needs scikit-learn):

    python tests/golden/make_golden_ap.py REFERENCE_ROOT

(REFERENCE_ROOT: a checkout of deepika090/HL-HGAT; lib/Hodge_Dataset.py is
imported behind pyg_standin.py.)

Writes ap_small.npz (plain arrays, no pickles), per case:

* <case>/{pred, label}: fp32 scores and labels [n, C] (NaN = unlabelled), what
  the GPU tests feed the kernel.  The case "strided" stores the WIDE matrices
  (<case>/{pred_wide, label_wide} and <case>/col0: the first column of the
  block) whose column block holds nan10's data.
* <case>/ap [C] fp64: average_precision_score(label[keep, c], pred[keep, c])
  per class over the labelled rows, NaN for a class without a 1 or without a
  0 (where the reference skips the class).
* <case>/counts [C, 3] int32: labelled rows, labels == 1, labels == 0.
* <case>/eval_ap fp64: the reference's eval_ap(label, pred).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _save  # noqa: E402


def _labels(rng, n, C, p_pos=0.3):
    return (rng.random((n, C)) < p_pos).astype(np.float32)


def cases():
    rng = np.random.default_rng(2401)
    out = {}
    out["n2"] = (np.array([[0.3], [-1.2]], np.float32), np.array([[0.0], [1.0]], np.float32))
    pred = (np.round(rng.standard_normal((257, 4)) * 4) / 4).astype(np.float32)
    out["n257_ties"] = (pred, _labels(rng, 257, 4))
    lab = np.zeros((300, 1), np.float32)
    lab[rng.permutation(300)[:100]] = 1.0
    out["all_ties"] = (np.full((300, 1), 0.75, np.float32), lab)
    out["signed_zero"] = (np.array([[-0.0], [0.0]], np.float32),
                          np.array([[0.0], [1.0]], np.float32))
    pred = rng.standard_normal((64, 10)).astype(np.float32)
    lab = _labels(rng, 64, 10, 0.4)
    lab[rng.random((64, 10)) < 0.3] = np.nan
    lab[:, 2] = np.nan                                        # all unlabelled
    lab[:, 5] = np.where(np.isnan(lab[:, 5]), np.nan, 0.0)    # no positives
    lab[:, 8] = np.where(np.isnan(lab[:, 8]), np.nan, 1.0)    # no zeros
    out["nan10"] = (pred, lab)
    pred = (np.round(rng.standard_normal((5000, 3)) * 16) / 16).astype(np.float32)
    out["n5000"] = (pred, _labels(rng, 5000, 3, 0.2))
    return out


INVALID = {"nan10": (2, 5, 8), "strided": (2, 5, 8)}


def main(ref_root):
    import pyg_standin
    pyg_standin.install()
    sys.path.insert(0, ref_root)
    import lib.Hodge_Dataset as ref_ds  # noqa: E402  (reference code)
    from sklearn.metrics import average_precision_score
    arrays = {}

    def record(name, pred, lab):
        C = pred.shape[1]
        ap = np.full(C, np.nan)
        counts = np.zeros((C, 3), np.int32)
        for c in range(C):
            keep = ~np.isnan(lab[:, c])
            y = lab[keep, c]
            counts[c] = (keep.sum(), (y == 1).sum(), (y == 0).sum())
            if counts[c, 1] > 0 and counts[c, 2] > 0:
                ap[c] = average_precision_score(y, pred[keep, c])
        bad = tuple(c for c in range(C) if np.isnan(ap[c]))
        assert bad == INVALID.get(name, ()), (name, bad)  # every other class has a 0 and a 1
        arrays[f"{name}/ap"] = ap
        arrays[f"{name}/counts"] = counts
        arrays[f"{name}/eval_ap"] = np.float64(
            ref_ds.eval_ap(torch.from_numpy(lab), torch.from_numpy(pred)))
        assert abs(arrays[f"{name}/eval_ap"] - np.nanmean(ap)) < 1e-15

    cs = cases()
    for name, (pred, lab) in cs.items():
        arrays[f"{name}/pred"] = pred
        arrays[f"{name}/label"] = lab
        record(name, pred, lab)
    assert abs(arrays["all_ties/ap"][0] - 1.0 / 3.0) < 1e-15
    assert arrays["signed_zero/ap"][0] == 0.5
    # nan10's data as a column block of wider matrices (ldp > C, ldl > C)
    rng = np.random.default_rng(2402)
    pred, lab = cs["nan10"]
    pw = rng.standard_normal((64, 17)).astype(np.float32)
    lw = rng.standard_normal((64, 13)).astype(np.float32)
    pw[:, 3:13] = pred
    lw[:, 2:12] = lab
    arrays["strided/pred_wide"] = pw
    arrays["strided/label_wide"] = lw
    arrays["strided/col0"] = np.array([3, 2], np.int64)
    record("strided", pred, lab)
    _save("ap_small", **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
