"""fp32 against bf16 matmul precision (hlhgat.set_matmul_precision), one process,
the two modes alternated window by window:

  * the isolated projection GEMMs -- forward, data gradient, weight gradient --
    at the config-2 conv and NodeEdgeInt shapes and the config-5 conv shape
    (median microseconds and TF/s of the algorithmic 2 M N K flops);
  * the replayed TrainStep of config 2 (1000 ZINC-like graphs, bench.MODEL_KW)
    and config 5 (4 TSP-like graphs of 10k nodes, bench.HEADS["cfg5_tsp_pyr"]),
    ms per step: median over the windows and the fp32 windows' max - min spread.

    python tools/gemm_bf16_bench.py [--repeats 7] [--steps 20] [--skip-steps]

Random operands, synthetic batches, random-init weights.  Prints one JSON line
and writes profiles/gemm_bf16.json.
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

GEMMS = {  # name: (M, N, reduction widths of the blocks)
    "cfg2_conv": (24900, 64, [64] * 3),
    "cfg2_neint_lin0": (24900, 64, [384, 384]),
    "cfg5_conv": (207000, 128, [128] * 4),
}
MODES = ("fp32", "bf16")


def _split(W, kbs):
    out, o = [], 0
    for k in kbs:
        out.append(W[:, o:o + k])
        o += k
    return out


def bench_gemm(name, dev, repeats, iters):
    import hlhgat
    from hlhgat import ops
    M, N, kbs = GEMMS[name]
    g = torch.Generator(device=dev).manual_seed(1)
    As = [torch.randn(M, k, device=dev, generator=g) for k in kbs]
    W = torch.randn(N, sum(kbs), device=dev, generator=g) / sum(kbs) ** 0.5
    bias = torch.randn(N, device=dev, generator=g)
    G = torch.randn(M, N, device=dev, generator=g)
    Ws = _split(W, kbs)
    out = torch.empty(M, N, device=dev)
    dAs = [torch.empty(M, k, device=dev) for k in kbs]
    dW = torch.empty_like(W)
    dWs = _split(dW, kbs)
    db = torch.empty(N, device=dev)
    ops_ = {"fwd": lambda: ops._proj_fwd(As, Ws, M, N, bias, out),
            "bwd_data": lambda: ops._proj_bwd_data(G, Ws, kbs, dAs),
            "bwd_weight": lambda: ops._proj_bwd_weight(G, As, dWs, db)}
    flops = 2.0 * M * N * sum(kbs)
    res = {"M": M, "N": N, "blocks": kbs}
    for op, fn in ops_.items():
        us = {m: [] for m in MODES}
        for mode in MODES:  # warm-up
            with hlhgat.matmul_precision(mode):
                for _ in range(3):
                    fn()
        for _ in range(repeats):
            for mode in MODES:
                with hlhgat.matmul_precision(mode):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us[mode].append(e0.elapsed_time(e1) * 1e3 / iters)
        res[op] = {}
        for mode in MODES:
            med = statistics.median(us[mode])
            res[op][mode] = {"us": round(med, 2), "tflops": round(flops / med * 1e-6, 2),
                             "us_min": round(min(us[mode]), 2), "us_max": round(max(us[mode]), 2)}
        res[op]["speedup"] = round(res[op]["fp32"]["us"] / res[op]["bf16"]["us"], 3)
    ops.check_device_errors()
    return res


def _config(name, dev):
    """(model factory, batch, loss_fn) of a replayable training configuration."""
    import bench
    import hlhgat
    if name == "cfg2":
        from hlhgat.synthetic import zinc_like_batch
        crit = hlhgat.nn.L1Loss()
        batch = zinc_like_batch(1000, seed=0).to(dev)
        return (lambda: hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**bench.MODEL_KW), batch,
                lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1)),
                "BASELINE config 2: 1000 ZINC-like graphs, bench.MODEL_KW")
    from hlhgat.synthetic import tsp_like_graph
    c = bench.HEADS["cfg5_tsp_pyr"]
    batch = bench._head_collate("tsp", [tsp_like_graph(i) for i in range(c["graphs"])]).to(dev)
    return (lambda: getattr(hlhgat, c["cls"])(**c["kw"]), batch,
            lambda o, d: bench._head_loss("tsp", o, d),
            "BASELINE config 5: 4 TSP-like graphs (10k nodes), cfg5_tsp_pyr")


def bench_step(name, dev, repeats, steps, warmup):
    from hlhgat import ops, train
    from hlhgat.train import TrainStep
    make, batch, loss_fn, what = _config(name, dev)
    keep = train.KEEP_GRAPHS
    train.KEEP_GRAPHS = True
    runs = {}
    try:
        for mode in MODES:  # built and captured one after the other, then only replayed
            torch.manual_seed(0)
            m = make().to(dev).train()
            st = TrainStep(m, loss_fn, lr=1e-3, graphs=True, matmul_precision=mode)
            for _ in range(warmup):
                st(batch)
            torch.cuda.synchronize()
            runs[mode] = st
    finally:
        train.KEEP_GRAPHS = keep
    ms = {m: [] for m in MODES}
    for _ in range(repeats):
        for mode in MODES:
            st = runs[mode]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                loss = st(batch)
            torch.cuda.synchronize()
            ms[mode].append((time.perf_counter() - t0) / steps * 1e3)
    ops.check_device_errors()
    res = {"workload": what, "steps_per_window": steps, "windows": repeats}
    for mode in MODES:
        st = runs[mode]
        counts = [ops.graph_kernel_count(e.graph.raw_cuda_graph(), "bf16")
                  for e in st._graphs.values()]
        res[mode] = {"ms_per_step": round(statistics.median(ms[mode]), 4),
                     "ms_min": round(min(ms[mode]), 4), "ms_max": round(max(ms[mode]), 4),
                     "spread_ms": round(max(ms[mode]) - min(ms[mode]), 4),
                     "graph_kernels": sum(c[0] for c in counts),
                     "bf16_kernels": sum(c[1] for c in counts),
                     "stats": dict(st.stats), "last_loss": float(loss) if mode == MODES[-1]
                     else None}
    gain = res["fp32"]["ms_per_step"] - res["bf16"]["ms_per_step"]
    res["bf16_gain_ms"] = round(gain, 4)
    res["speedup"] = round(res["fp32"]["ms_per_step"] / res["bf16"]["ms_per_step"], 4)
    res["gain_exceeds_fp32_spread"] = bool(gain > res["fp32"]["spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="GEMM launches per timed window")
    ap.add_argument("--steps", type=int, default=20, help="train steps per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--configs", nargs="*", default=["cfg2", "cfg5"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "gemm_bf16.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm GPU"
    dev = torch.device("cuda:0")
    res = {"tool": "tools/gemm_bf16_bench.py", "device": torch.cuda.get_device_name(0),
           "args": {k: v for k, v in vars(args).items() if k != "out"}, "gemm": {}, "step": {}}
    for name in GEMMS:
        res["gemm"][name] = bench_gemm(name, dev, args.repeats, args.iters)
        print(f"[gemm] {name}: {json.dumps(res['gemm'][name])}", file=sys.stderr, flush=True)
    if not args.skip_steps:
        for name in args.configs:
            res["step"][name] = bench_step(name, dev, args.repeats, args.steps, args.warmup)
            print(f"[step] {name}: {json.dumps(res['step'][name])}", file=sys.stderr, flush=True)
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
