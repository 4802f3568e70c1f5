"""Cost of the molecular data path (hlhgat.pipeline.MoleculePipeline).

On 1000 ZINC-like and 64 peptides-like raw molecules per batch
(pipeline.molecule_raw; sizes as synthetic.zinc_like_graph /
peptides_like_graphs draw them):

  * batch() on the device (median wall ms of --iters batches after a warm-up,
    the device synchronised at both ends) against device="cpu" (the
    reference's arithmetic: three dense float32 eighs per graph) on
    --threads host threads;
  * its stages (MoleculePipeline.PROFILE: every stage boundary synchronises);
  * the hlhgat_eig_pe_edges launch against the hlhgat_eig_pe launch on the
    same batch (hipEvent ms, median);
  * coarsen() with mlgc="device" against mlgc="host" on the peptides batch.

Prints one JSON line and writes it to --out.

    python tools/molecule_bench.py [--iters 7] [--out profiles/molecule_pipeline.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "hl-hgat_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from hlhgat import ops  # noqa: E402
from hlhgat.pipeline import MoleculePipeline, molecule_raw  # noqa: E402


def _raws(kind, count):
    rng = np.random.default_rng(0)
    if kind == "zinc":
        ns = np.clip(np.round(rng.normal(23.2, 4.5, count)), 9, 38).astype(int)
    else:
        ns = np.clip(np.round(rng.normal(150.9, 20.0, count)), 40, 300).astype(int)
    return [molecule_raw(1000 + i, int(n), kind) for i, n in enumerate(ns)]


def _wall_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def _event_ms(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "molecule_pipeline.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(a.threads)
    res = {"device": torch.cuda.get_device_name(dev), "iters": a.iters, "host_threads": a.threads}
    for kind, count, keig in (("zinc", 1000, 16), ("peptides", 64, 21)):
        p = MoleculePipeline(_raws(kind, count), kind=kind, keig=keig)
        idx = list(range(count))
        r = {"graphs": count, "keig": keig, "nodes": int(p.n.sum()), "edges": int(p.m.sum()),
             "max_nodes": int(p.n.max()), "max_edges": int(p.m.max())}
        r["batch_device"] = _wall_ms(lambda: p.batch(idx, device=dev), a.iters)
        t0 = time.perf_counter()
        p.batch(idx, device="cpu")
        r["batch_host_ms"] = (time.perf_counter() - t0) * 1e3
        p.PROFILE, p.stage_ms = True, {}
        for _ in range(a.iters):
            p.batch(idx, device=dev)
        r["stages_ms"] = {k: v / a.iters for k, v in p.stage_ms.items()}
        p.PROFILE = False
        b = p.batch(idx, device=dev)
        ns, es, N = [int(v) for v in p.n], [int(v) for v in p.m], int(p.n.sum())
        ei = b.edge_index
        r["eig_pe"] = _event_ms(lambda: ops.eig_pe(ei, b.num_node1, keig, max_nodes=max(ns),
                                                   n_nodes=N), a.iters)
        r["eig_pe_edges"] = _event_ms(lambda: ops.eig_pe_edges(ei, b.num_node1, b.num_edge1, keig,
                                                               max_edges=max(es), n_nodes=N), a.iters)
        if kind == "peptides":
            r["coarsen_device"] = _wall_ms(lambda: p.coarsen(b, seed=1, mlgc="device"), a.iters)
            r["coarsen_host"] = _wall_ms(lambda: p.coarsen(b, seed=1, mlgc="host"), a.iters)
        ops.check_device_errors()
        res[kind] = r
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
