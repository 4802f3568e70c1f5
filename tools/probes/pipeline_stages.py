"""Where the config-3 per-sample pipeline spends its time: SuperpixelPipeline
stage timings (device synchronised at every stage boundary) over a few
256-graph batches, plus pad_levels.

    python tools/probes/pipeline_stages.py [--batches 4] [--mlgc host|device|both]

--mlgc both builds the same batches with MLGC on the host (the default path)
and on the device (ops.mlgc_device) in one process, alternating, and prints
one stage table per route (whole-batch ms included).
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--graphs", type=int, default=256)
    ap.add_argument("--mlgc", choices=["host", "device", "both"], default="host")
    ap.add_argument("--rounds", type=int, default=5, help="--mlgc both: alternations")
    args = ap.parse_args()
    if args.mlgc == "both":
        return compare(args)
    from hlhgat.hodge_dataset import level_caps, pad_levels
    from hlhgat.pipeline import SuperpixelPipeline, superpixel_raw
    G, B = args.graphs, args.batches
    raw = [superpixel_raw(5000 + i) for i in range(B * G)]
    pipe = SuperpixelPipeline(raw, keig=11, aug=True, mlgc=args.mlgc)
    dev = torch.device("cuda:0")
    bs = [pipe.batch(range(b * G, (b + 1) * G), seed=b, device=dev) for b in range(B)]  # warm
    caps = level_caps(bs, 512)
    pipe.PROFILE = True
    pipe.stage_ms = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tp = 0.0
    pads = []
    for b in range(B):
        d = pipe.batch(range(b * G, (b + 1) * G), seed=b, device=dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pad_levels(d, caps)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        pad_levels(d, caps)
        torch.cuda.synchronize()
        pads.append((round((t2 - t1) * 1e3, 2), round((time.perf_counter() - t2) * 1e3, 2)))
        tp += t2 - t1
    print("pad_levels ms (first, again) per batch:", pads, flush=True)
    tot = (time.perf_counter() - t0) / B * 1e3
    # where pad_levels spends its host time (torch.profiler, CPU ops)
    from torch.profiler import ProfilerActivity, profile
    d = pipe.batch(range(0, G), seed=0, device=dev)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU]) as prof:
        pad_levels(d, caps)
        torch.cuda.synchronize()
    print(prof.key_averages().table(sort_by="self_cpu_time_total", row_limit=12), flush=True)
    st = {k: round(v / B, 2) for k, v in pipe.stage_ms.items()}
    st["pad_levels"] = round(tp / B * 1e3, 2)
    print(json.dumps({"ms_per_batch": round(tot, 2), "graphs": G, "stages_ms": st}))


def compare(args):
    """mlgc="host" against mlgc="device" on the same batches, alternating:
    per route the whole-batch ms without stage synchronisation (median and
    spread over the rounds), then the per-stage ms with it."""
    import statistics
    from hlhgat.pipeline import SuperpixelPipeline, superpixel_raw
    G, B = args.graphs, args.batches
    raw = [superpixel_raw(5000 + i) for i in range(B * G)]
    dev = torch.device("cuda:0")
    pipes = {m: SuperpixelPipeline(raw, keig=11, aug=True, mlgc=m) for m in ("host", "device")}
    for p in pipes.values():  # warm
        for b in range(B):
            p.batch(range(b * G, (b + 1) * G), seed=b, device=dev)
    torch.cuda.synchronize()
    whole = {m: [] for m in pipes}
    for _ in range(args.rounds):
        for m, p in pipes.items():
            t0 = time.perf_counter()
            for b in range(B):
                p.batch(range(b * G, (b + 1) * G), seed=b, device=dev)
            torch.cuda.synchronize()
            whole[m].append((time.perf_counter() - t0) / B * 1e3)
    for p in pipes.values():
        p.PROFILE = True
        p.stage_ms = {}
    for _ in range(args.rounds):
        for m, p in pipes.items():
            for b in range(B):
                p.batch(range(b * G, (b + 1) * G), seed=b, device=dev)
    for m, p in pipes.items():
        st = {k: round(v / (B * args.rounds), 3) for k, v in p.stage_ms.items()}
        print(json.dumps({"mlgc": m, "graphs": G, "batches": B, "rounds": args.rounds,
                          "ms_per_batch_median": round(statistics.median(whole[m]), 3),
                          "ms_per_batch_min_max": [round(min(whole[m]), 3), round(max(whole[m]), 3)],
                          "stages_ms": st}), flush=True)


if __name__ == "__main__":
    main()
