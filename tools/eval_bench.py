#!/usr/bin/env python3
"""What the evaluation meters replace, per batch of each test() loop, on the
same device tensors (no model: the loop body behind ``out = model(data)``):

  tsp    4 graphs x ~52k edges: the host route is the reference's loop body
         (main_TSP...:344-347) restated with torch ops -- the per-graph sizes
         read back for unbatch, then per graph BinaryF1Score's formatting,
         counts and one value read; the meter route is F1Meter.update.
  zinc   batches of 128 scalars into an epoch of 10,000: the host route is
         ``(out - y).abs().sum().item()`` per batch (main_zinc...:174) and, at
         the end, the notebook's z-scored correlation, L1 and RMSE over the
         10,000 collected values with torch ops and one read; the meter route
         is RegressionMeter.update per batch and compute() at the end.
  cifar  256 x 10 logits: ``int((out.argmax(1) == y).sum())`` against
         AccuracyMeter.update.

Each route: median of --runs after --warmup.  Host routes end in a read, so
wall time is their measure.  Meter updates are timed eagerly and replayed from
a hipGraph, by hipEvents (device time between the two records) and by wall
time around a synchronise (what a loop that waits for nothing else pays);
compute() by wall time.  Prints one JSON line; --out FILE also writes it.
Reads nothing outside the repository.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _wall_ms(fn, runs, warmup, before=None):
    out = []
    for i in range(warmup + runs):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def _event_ms(fn, runs, warmup, before=None):
    out = []
    for i in range(warmup + runs):
        if before:
            before()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def _graph_of(fn, dev):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fn()
    return g


def _routes(host, update, reset, dev, a):
    reset()  # room for the one update that runs before the capture
    g = _graph_of(update, dev)
    return {
        "host_ms_wall": _wall_ms(host, a.runs, a.warmup),
        "meter_eager_ms_events": _event_ms(update, a.runs, a.warmup, reset),
        "meter_eager_ms_wall": _wall_ms(update, a.runs, a.warmup, reset),
        "meter_replay_ms_events": _event_ms(g.replay, a.runs, a.warmup, reset),
        "meter_replay_ms_wall": _wall_ms(g.replay, a.runs, a.warmup, reset),
    }


def f1_host(out, y, s_batch):
    """The TSP loop body with torch ops: unbatch, then f1() per graph."""
    sizes = torch.bincount(s_batch).tolist()  # unbatch's degree(...).tolist()
    vals = []
    for p, t in zip(out.view(-1).split(sizes), y.view(-1).split(sizes)):
        if bool(((p < 0) | (p > 1)).any()):   # BinaryF1Score's formatting
            p = p.sigmoid()
        pred, pos = p > 0.5, t == 1
        tp = (pred & pos).sum()
        fp = (pred & ~pos).sum()
        fn = (~pred & pos).sum()
        den = 2 * tp + fp + fn
        vals.append(float(torch.where(den > 0, 2 * tp / den.clamp(min=1), den * 0.0)))
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import hlhgat  # noqa: F401
    from hlhgat import ops
    from hlhgat.metrics import AccuracyMeter, F1Meter, RegressionMeter
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    res = {"runs": a.runs, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}

    # TSP: 4 graphs x 52,000 edges, masked logits
    G, E = 4, 52000
    out = (torch.randn(G * E, 1, generator=gen) * 3 *
           (torch.rand(G * E, 1, generator=gen) < 0.9)).to(dev)
    y = (torch.rand(G * E, generator=gen) < 0.2).float().to(dev)
    sizes = torch.full((G,), E, dtype=torch.int64, device=dev)
    s_batch = torch.arange(G, device=dev).repeat_interleave(E)
    f1m = F1Meter(G, dev)
    host_vals = f1_host(out, y, s_batch)
    f1m.update(out, y, sizes)
    assert max(abs(u - v) for u, v in zip(f1m.per_graph().tolist(), host_vals)) < 1e-6
    res["tsp"] = {"shape": [G, E], **_routes(lambda: f1_host(out, y, s_batch),
                                             lambda: f1m.update(out, y, sizes), f1m.reset, dev, a)}
    res["tsp"]["meter_compute_ms_wall"] = _wall_ms(f1m.compute, a.runs, a.warmup)

    # ZINC: batches of 128 into 10,000 collected values
    N, B = 10000, 128
    pred = torch.randn(N, 1, generator=gen).to(dev)
    tgt = (pred.view(-1) * 0.7 + 0.5 * torch.randn(N, generator=gen).to(dev))
    reg = RegressionMeter(N, dev)

    def fill():
        reg.reset()
        reg.update(pred[:N - B], tgt[:N - B])

    def epoch_end_host():
        p, t = pred.view(-1), tgt
        zp, zt = (p - p.mean()) / p.std(), (t - t.mean()) / t.std()
        return torch.stack([(zp * zt).mean(), (p - t).abs().mean(),
                            ((p - t) ** 2).mean().sqrt()]).tolist()
    res["zinc"] = {"shape": [N], "batch": B,
                   **_routes(lambda: (pred[:B].view(-1) - tgt[:B]).abs().sum().item(),
                             lambda: reg.update(pred[N - B:], tgt[N - B:]), fill, dev, a)}
    fill()
    reg.update(pred[N - B:], tgt[N - B:])
    got, want = reg.compute(), epoch_end_host()
    assert got["n"] == N and abs(got["corr"] - want[0]) < 1e-4 and abs(got["mae"] - want[1]) < 1e-4
    res["zinc"]["epoch_end_host_ms_wall"] = _wall_ms(epoch_end_host, a.runs, a.warmup)
    res["zinc"]["meter_compute_ms_wall"] = _wall_ms(reg.compute, a.runs, a.warmup)
    res["zinc"]["meter_summary_ms_events"] = _event_ms(
        lambda: ops.regression_summary(reg.pred.buf.view(-1), reg.y.buf.view(-1), reg.pred.cursor),
        a.runs, a.warmup)

    # CIFAR: 256 x 10
    n, C = 256, 10
    logits = torch.randn(n, C, generator=gen).to(dev)
    lab = torch.randint(0, C, (n,), generator=gen).to(dev)
    acc = AccuracyMeter(dev)
    acc.update(logits, lab)
    assert acc.compute() == int((logits.argmax(1) == lab).sum()) / n
    res["cifar"] = {"shape": [n, C],
                    **_routes(lambda: int((logits.argmax(1) == lab).sum()),
                              lambda: acc.update(logits, lab), acc.reset, dev, a)}
    res["cifar"]["meter_compute_ms_wall"] = _wall_ms(acc.compute, a.runs, a.warmup)
    ops.check_device_errors()

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
