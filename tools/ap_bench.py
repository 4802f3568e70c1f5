#!/usr/bin/env python3
"""What the device eval_ap replaces, at the peptides-func epoch shape
(10,873 x 10, about 30 % NaN labels):

  * hlhgat.metrics.eval_ap on device tensors, by hipEvents, the median of 20
    runs after warm-up; ops.average_precision alone, eagerly and replayed from
    a hipGraph (the kernels back to back, without launch gaps).  Per-kernel
    durations: run this tool under `rocprofv3 --kernel-trace --stats --`;
  * the reference route: .cpu() plus one scikit-learn average_precision_score
    per class where scikit-learn is importable, otherwise the numpy
    restatement tests/ap_ref.py, by wall time (median of 20).

Prints one JSON line; --out FILE also writes it.  Reads nothing outside the
repository.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _host_route():
    """(name, fn(label, pred) -> float): what the device metric replaces --
    both tensors brought to the host, then per class with a 0 and a 1 among
    its labelled rows one scikit-learn call (tests/ap_ref.py's counts and NaN
    mask); without scikit-learn, ap_ref itself."""
    import ap_ref
    try:
        from sklearn.metrics import average_precision_score
    except ImportError:
        return "ap_ref (numpy)", lambda lab, pr: ap_ref.eval_ap(lab.cpu().numpy(),
                                                                pr.cpu().numpy())

    def route(label, pred):
        lab, pr = label.cpu().numpy(), pred.cpu().numpy()
        vals = []
        for c in range(lab.shape[1]):
            keep = ~np.isnan(lab[:, c])
            y = lab[keep, c]
            if (y == 1).any() and (y == 0).any():
                vals.append(float(average_precision_score(y, pr[keep, c])))
        if not vals:
            raise RuntimeError(ap_ref.NO_VALID)
        return float(np.mean(vals))
    return "scikit-learn", route


def _event_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10873)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hlhgat
    from hlhgat import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    pred = torch.randn(a.n, a.classes, generator=g)
    label = (torch.rand(a.n, a.classes, generator=g) < 0.1).float()
    label[torch.rand(a.n, a.classes, generator=g) < 0.3] = float("nan")
    pd, ld = pred.to(dev), label.to(dev)

    name, route = _host_route()
    host_val = route(ld, pd)
    dev_val = hlhgat.eval_ap(ld, pd)
    host_ms = []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        route(ld, pd)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    # eval_ap end to end (it ends in a D2H read, so wall time is honest too)
    wall_ms = []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hlhgat.eval_ap(ld, pd)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
    ev_all = _event_ms(lambda: hlhgat.eval_ap(ld, pd), a.runs, a.warmup)
    ev_kernels = _event_ms(lambda: ops.average_precision(pd, ld), a.runs, a.warmup)
    # the same launches replayed from a hipGraph: the kernels without launch gaps
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        ops.average_precision(pd, ld)
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ops.average_precision(pd, ld)
    ev_graph = _event_ms(graph.replay, a.runs, a.warmup)
    res = {
        "shape": [a.n, a.classes], "runs": a.runs,
        "device_eval_ap_ms_events_median": statistics.median(ev_all),
        "device_eval_ap_ms_wall_median": statistics.median(wall_ms),
        "device_average_precision_ms_events_median": statistics.median(ev_kernels),
        "device_average_precision_graph_replay_ms_median": statistics.median(ev_graph),
        "host_route": name,
        "host_route_ms_wall_median": statistics.median(host_ms),
        "host_route_ms_wall_min": min(host_ms),
        "eval_ap_device": dev_val, "eval_ap_host": host_val,
        "abs_diff": abs(dev_val - host_val),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
