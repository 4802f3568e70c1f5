"""Cost of simplex dropout in the replayed config-5 training step.

Two TrainSteps on the BASELINE config-5 head and one padded batch of 4 TSP-like
graphs -- one with model.augment = SimplexDropout, one without -- are warmed up
(captured) one after the other and then replayed in alternating blocks in one
process.  Prints one JSON line: ms/step of both, the spread of the unaugmented
step over the repeats, and whether the difference lies inside that spread.

    python tools/tsp_aug_bench.py [--steps 10] [--repeats 5] [--out profiles/tsp_aug_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "hl-hgat_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
import hlhgat  # noqa: E402
from hlhgat import ops  # noqa: E402
from hlhgat.hodge_dataset import pad_batch, static_caps  # noqa: E402
from hlhgat.train import TrainStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--repeats", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graphs", type=int, default=4)
    ap.add_argument("--nodes", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    c = bench.HEADS["cfg5_tsp_pyr"]
    from hlhgat.synthetic import tsp_like_graph
    raw = bench._head_collate("tsp", [tsp_like_graph(i, n=args.nodes) for i in range(args.graphs)])
    caps = static_caps(raw, 512)
    ops.dropout_manual_seed(1234, dev)
    steps = {}
    for name in ("plain", "augmented"):  # one after the other: the gradient bucket is global
        torch.manual_seed(0)
        m = getattr(hlhgat, c["cls"])(**c["kw"])
        if name == "augmented":
            m.augment = hlhgat.nn.SimplexDropout(aug_prob=0.75, p=0.0, jitter=0.5)
        m = m.to(dev).train()
        batch = pad_batch(raw, caps).to(dev)
        st = TrainStep(m, lambda o, d: bench._head_loss("tsp", o, d), lr=1e-3, graphs=True)
        for _ in range(args.warmup):
            st(batch)
        torch.cuda.synchronize()
        steps[name] = (st, batch)
        print(f"[{name}] warm: {st.stats}", file=sys.stderr, flush=True)
    ms = {"plain": [], "augmented": []}
    for _ in range(args.repeats):
        for name, (st, batch) in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st(batch)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    ops.check_device_errors()
    kept = float(steps["augmented"][0].model.augment.mask_of(
        next(iter(steps["augmented"][0]._graphs.values())).batch).mean())
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["plain"]) - min(ms["plain"])
    diff = med["augmented"] - med["plain"]
    res = {"workload": f"BASELINE cfg5_tsp_pyr, {args.graphs} x tsp_like_graph(n={args.nodes}), "
                       "replayed TrainStep", "rows_s": int(raw.x_s.shape[0]),
           "nnz_s": int(raw.edge_index_s.shape[1]), "steps_per_block": args.steps,
           "repeats": args.repeats,
           "ms_per_step": {k: [round(x, 3) for x in v] for k, v in ms.items()},
           "median_ms": {k: round(v, 3) for k, v in med.items()},
           "plain_spread_ms": round(spread, 3), "augmented_minus_plain_ms": round(diff, 3),
           "inside_plain_spread": abs(diff) <= spread,
           "last_mask_keep_share_incl_padding": round(kept, 4),
           "note": "the augmented step trains on masked operators: its arithmetic differs from "
                   "the plain step's only in table values, never in shapes or launches other "
                   "than the draw and the table rewrites"}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
