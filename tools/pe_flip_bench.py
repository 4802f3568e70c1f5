"""Cost of the PE sign flip in the replayed training step.

For the BASELINE config-2 step (the ZINC model on one padded 1000-graph batch)
and for the config-4 peptides attpool head, two TrainSteps -- one with
model.pe_flip = PESignFlip, one without -- are warmed up (captured) one after
the other and then replayed in alternating windows in one process.  Per
workload the result holds the ms/step of both, the run-to-run spread of the
plain step over the windows, the difference of the medians, and the flip
launch timed alone next to a k_copy2d_batched launch of the same bytes.
Prints one JSON line and writes it to --out.

    python tools/pe_flip_bench.py [--steps 20] [--windows 5] [--out profiles/pe_flip.json]
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
from hlhgat.train import TrainStep  # noqa: E402


def _workload(name, dev):
    """(batch on dev, model factory, PESignFlip factory, loss, fine level)."""
    if name == "cfg2_zinc_pyr":
        batches, _, _, _, _ = bench.make_batches(1, 0, dev)
        crit = torch.nn.L1Loss()
        return (batches[0], lambda: hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**bench.MODEL_KW),
                lambda: hlhgat.nn.PESignFlip(21, 3, bench.MODEL_KW["keig"]),
                lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1)), lambda b: b)
    c = bench.HEADS["cfg4_pepfunc_attpool"]
    datas = [x.to(dev) for x in bench._head_batch("peptides", c["graphs"], 0)]
    return (datas, lambda: getattr(hlhgat, c["cls"])(**c["kw"]),
            lambda: hlhgat.nn.PESignFlip(9, 3, 20),
            lambda o, d: bench._head_loss("peptides", o, d), lambda d: d[0])


def _launch_us(fn, chain=32, reps=11):
    """Median device time of one fn() launch: `chain` launches captured into a
    hipGraph (no host work between them), the replay timed with hipEvents."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = ops.own_stream(torch.device("cuda", torch.cuda.current_device()), "capture")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=s):
        for _ in range(chain):
            fn()
    g.replay()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / chain)
    return statistics.median(ts)


def measure(name, dev, args):
    batch, mk, mk_flip, loss, fine = _workload(name, dev)
    ops.dropout_manual_seed(1234, dev)
    steps = {}
    for mode in ("plain", "flipped"):  # one after the other: the gradient bucket is global
        torch.manual_seed(0)
        m = mk()
        if mode == "flipped":
            m.pe_flip = mk_flip()
        m = m.to(dev).train()
        st = TrainStep(m, loss, lr=1e-3, graphs=True)
        for _ in range(args.warmup):
            st(batch)
        torch.cuda.synchronize()
        steps[mode] = st
        print(f"[{name} {mode}] warm: {st.stats}", file=sys.stderr, flush=True)
    ms = {"plain": [], "flipped": []}
    for _ in range(args.windows):
        for mode, st in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                st(batch)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) / args.steps * 1e3)
    ops.check_device_errors()
    # the launch alone, next to a plain copy of the same bytes
    f = fine(batch)
    flip = steps["flipped"].model.pe_flip
    off = 1 if isinstance(batch, list) else 0
    x_t, x_s = f.x_t[:, off:], f.x_s[:, off:]
    k_t, k_s = flip.widths(x_t, x_s)
    y_t, y_s = ops.pe_flip(x_t, f.seg_ptr_t, flip.node_dim, k_t, x_s, f.seg_ptr_s, flip.edge_dim,
                           k_s)
    srcs = [x_t.contiguous(), x_s.contiguous()]
    moved = 2 * 4 * (y_t.numel() + y_s.numel())
    us_flip = _launch_us(lambda: ops.pe_flip(x_t, f.seg_ptr_t, flip.node_dim, k_t, x_s,
                                             f.seg_ptr_s, flip.edge_dim, k_s))
    us_copy = _launch_us(lambda: ops.copy_words_batched(srcs, [y_t, y_s]))
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = max(ms["plain"]) - min(ms["plain"])
    diff = med["flipped"] - med["plain"]
    return {"rows_t": int(x_t.size(0)), "rows_s": int(x_s.size(0)),
            "graphs": int(f.seg_ptr_t.numel() - 1), "widths": [int(y_t.size(1)), int(y_s.size(1))],
            "bytes_moved": moved,
            "ms_per_step": {k: [round(x, 3) for x in v] for k, v in ms.items()},
            "median_ms": {k: round(v, 3) for k, v in med.items()},
            "plain_spread_ms": round(spread, 3), "flipped_minus_plain_ms": round(diff, 4),
            "inside_plain_spread": abs(diff) <= spread,
            "pe_flip_launch_us": round(us_flip, 2), "copy2d_same_bytes_us": round(us_copy, 2),
            "pe_flip_gbs": round(moved / us_flip / 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--windows", type=int, default=5, help="alternating windows per variant")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pe_flip.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"tool": "tools/pe_flip_bench.py", "steps_per_window": args.steps,
           "windows": args.windows, "precision": hlhgat.get_matmul_precision(),
           "note": "replayed TrainStep with and without model.pe_flip, alternating windows in one "
                   "process; the launch-alone figures are one launch of a chain of 32 captured "
                   "into a hipGraph",
           "workloads": {n: measure(n, dev, args)
                         for n in ("cfg2_zinc_pyr", "cfg4_pepfunc_attpool")}}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
