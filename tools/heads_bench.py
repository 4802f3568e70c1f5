"""graphs/s (fwd + loss + bwd) of the attention-pooling heads at BASELINE
configs 3 and 4 on one GPU, eager (no hipGraph: the two MLGC levels change
shape every batch).

    python tools/heads_bench.py [--configs cifar peptides] [--steps 10]
                                [--dropout-ratio 0.25 [--ab-rounds 5]]
                                [--loss {aten,hip,reference} [--ab-rounds 5]]

cifar    (config 3): HL_HGCNN_CIFAR10SP_dense_int3_attpool(channels=[2,2,2],
         filters=[64,128,256], mlp=[256], K=4, keig=10, pool_loc=1, l=0.5),
         256 CIFAR-like superpixel graphs (118 nodes, 8-NN) per batch
         (main_cifar10SP...:35-36,186-187), cross-entropy loss.
peptides (config 4): HL_HGCNN_pepfunc_dense_int3_attpool(channels=[2,2,2],
         filters=[64,128,256], mlp=[256], K=6, pool_loc=1), 64 peptide-like
         molecules (~151 atoms) per batch (main_pepfunc...:27-28), BCE loss.
tsp      (config 5): HL_HGCNN_TSP_dense_int3_pyr(channels=[4,4,4],
         filters=[32,64,128], mlp=[256], K=4), 4 TSP-like graphs (10k nodes,
         9-NN) per GPU, BCE on the masked edge logits
         (main_TSP...:316-321 trains a focal-BCE).
--loss picks the objective and where it runs: "aten" (default, the runs as
they always were): cross-entropy / plain BCE composed of ATen ops; "hip": the
same objectives through hlhgat.nn.CrossEntropyLoss / MaskedBCEWithLogitsLoss
(csrc/loss.hip); "reference": what the reference's scripts train -- FocalLoss
for peptides and tsp (lib/Loss_function.py:14-26), cross-entropy for cifar --
written in ATen ops.  With --loss hip or reference, --ab-rounds N times N
interleaved (ATen composition, HIP module) windows of the SAME objective
(reference: hlhgat.nn.FocalLoss is the HIP arm).
Synthetic data, random-init weights.  One JSON line per config.  The L1
operators of cifar / tsp batches run factored (hlhgat_hodge_factor_t) unless
HLHGAT_FACTOR=0.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CONFIGS = {
    "cifar": dict(kind="cifar", graphs=256, cls="HL_HGCNN_CIFAR10SP_dense_int3_attpool",
                  kw=dict(channels=[2, 2, 2], filters=[64, 128, 256], mlp_channels=[256], K=4,
                          keig=10, pool_loc=1, l=0.5), loss="ce"),
    "peptides": dict(kind="peptides", graphs=64, cls="HL_HGCNN_pepfunc_dense_int3_attpool",
                     kw=dict(channels=[2, 2, 2], filters=[64, 128, 256], mlp_channels=[256],
                             K=6, pool_loc=1), loss="bce"),
    "tsp": dict(kind="tsp", graphs=4, cls="HL_HGCNN_TSP_dense_int3_pyr",
                kw=dict(channels=[4, 4, 4], filters=[32, 64, 128], mlp_channels=[256], K=4),
                loss="edge_bce"),
}


def make_batch(kind, graphs, seed):
    from hlhgat.hodge_dataset import collate
    from hlhgat.synthetic import tsp_like_graph, two_level_batch
    if kind == "tsp":
        return collate([tsp_like_graph(seed * graphs + i) for i in range(graphs)],
                       check_hodge=False)
    return two_level_batch(kind, graphs, seed=seed)


def run(name, steps, warmup, n_batches, dev, dropout_ratio=0.0, ab_rounds=0, loss_mode="aten"):
    import hlhgat
    from hlhgat import ops
    F = torch.nn.functional
    c = CONFIGS[name]
    focal = loss_mode == "reference" and c["loss"] != "ce"
    objective = "ce" if c["loss"] == "ce" else ("focal" if focal else "bce")
    hip_crit = (hlhgat.nn.CrossEntropyLoss() if c["loss"] == "ce" else
                hlhgat.nn.FocalLoss() if focal else hlhgat.nn.MaskedBCEWithLogitsLoss())

    def aten_crit(logits, y):
        if c["loss"] == "ce":
            return F.cross_entropy(logits, y)
        b = F.binary_cross_entropy_with_logits(logits, y)
        if not focal:
            return b
        logpt = -b  # lib/Loss_function.py:22-26 with its defaults
        pt = torch.exp(logpt)
        return -((1 - pt) ** 2) * 0.25 * logpt * 1e4

    arm = {"hip": loss_mode == "hip"}  # which arm step() runs; the loss A/B flips it
    loss_ab = ab_rounds if loss_mode != "aten" else 0
    if dropout_ratio:
        c = dict(c, kw=dict(c["kw"], dropout_ratio=dropout_ratio))
    t0 = time.time()
    batches = []
    for s in range(n_batches):
        bb = make_batch(c["kind"], c["graphs"], s)
        # Batch.to also attaches the operator hints (row schedules, halo tiles,
        # hodge factor) that collate recorded
        batches.append(bb.to(dev) if c["kind"] == "tsp" else [b.to(dev) for b in bb])
    t_data = time.time() - t0
    torch.manual_seed(0)
    m = getattr(hlhgat, c["cls"])(**c["kw"]).to(dev).train()
    n_params = sum(p.numel() for p in m.parameters())

    def step(i):
        datas = batches[i % n_batches]
        out = m(datas)
        crit = hip_crit if arm["hip"] else aten_crit
        if c["loss"] == "edge_bce":
            logits, _ = out
            loss = crit(logits.view(-1), datas.y.view(-1).float())
        elif c["loss"] == "ce":
            loss = crit(out, datas[0].y.view(-1).long())
        else:
            loss = crit(out, datas[0].y.view(out.shape))
        m.zero_grad(set_to_none=True)
        loss.backward()

    def window():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps

    ab = {}
    if loss_ab:
        # A/B of the loss in one process, windows interleaved (ATen, HIP, ATen,
        # HIP, ...): the same objective either way
        for flag in (False, True):
            arm["hip"] = flag
            for i in range(warmup):
                step(i)
        ms = {False: [], True: []}
        for _ in range(loss_ab):
            for flag in (False, True):
                arm["hip"] = flag
                ms[flag].append(round(window() * 1e3, 3))
        arm["hip"] = loss_mode == "hip"
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        ab = {"ms_aten_loss": ms[False], "ms_hip_loss": ms[True],
              "median_ms_aten_loss": med[False], "median_ms_hip_loss": med[True],
              "spread_aten_loss": round((max(ms[False]) - min(ms[False])) / med[False], 4),
              "hip_over_aten": round(med[True] / med[False], 4)}
    elif ab_rounds:
        # A/B of ops.HIP_DROPOUT in one process, windows interleaved (off, on,
        # off, on, ...); off = ATen's dropout, the behaviour before ops.dropout
        for flag in (False, True):
            ops.HIP_DROPOUT = flag
            for i in range(warmup):
                step(i)
        ms = {False: [], True: []}
        for _ in range(ab_rounds):
            for flag in (False, True):
                ops.HIP_DROPOUT = flag
                ms[flag].append(round(window() * 1e3, 3))
        ops.HIP_DROPOUT = True
        med = {f: sorted(v)[len(v) // 2] for f, v in ms.items()}
        ab = {"ms_aten_dropout": ms[False], "ms_hip_dropout": ms[True],
              "median_ms_aten_dropout": med[False], "median_ms_hip_dropout": med[True],
              "spread_aten_dropout": round((max(ms[False]) - min(ms[False])) / med[False], 4),
              "hip_over_aten": round(med[True] / med[False], 4)}
    for i in range(warmup):
        step(i)
    dt = window()
    b0 = batches[0] if c["kind"] == "tsp" else batches[0][0]
    op = ops.hodge_operator(b0.edge_index_s, b0.edge_weight_s, b0.x_s.shape[0])
    extra = {"dropout_ratio": dropout_ratio, **ab} if dropout_ratio else dict(ab)
    if loss_mode != "aten":
        extra.update(loss=loss_mode, objective=objective)
    return {**extra, "config": name, "head": c["cls"], "graphs_per_step": c["graphs"],
            "value": round(c["graphs"] / dt, 1), "unit": "graphs/s", "ms_per_step": round(dt * 1e3, 3),
            "mode": "eager fwd+loss+bwd", "params": n_params, "rows_t": int(b0.x_t.shape[0]),
            "rows_s": int(b0.x_s.shape[0]), "nnz_s": int(b0.edge_index_s.shape[1]),
            "data_gen_s": round(t_data, 1), "l1_factored": op.factor is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cifar", "peptides", "tsp"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--dropout-ratio", type=float, default=0.0,
                    help="dropout_ratio of the head (the reference scripts train configs 3-5 "
                         "with 0.25); 0 = the runs as they always were")
    ap.add_argument("--ab-rounds", type=int, default=0,
                    help="with --dropout-ratio or --loss hip / reference: this many "
                         "interleaved (ATen, HIP) windows of --steps steps each, reported per "
                         "window (the loss A/B when --loss is given)")
    ap.add_argument("--loss", choices=("aten", "hip", "reference"), default="aten",
                    help="aten: cross-entropy / BCE in ATen ops (the runs as they always were); "
                         "hip: the same through hlhgat.nn's HIP losses; reference: focal for "
                         "peptides and tsp, in ATen ops")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.configs:
        print(json.dumps(run(name, args.steps, args.warmup, args.batches, dev,
                             args.dropout_ratio,
                             args.ab_rounds if args.dropout_ratio or args.loss != "aten" else 0,
                             args.loss)),
              flush=True)


if __name__ == "__main__":
    main()
