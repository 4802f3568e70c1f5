"""Timings of the DEMO brain model's front end and head on the GPU.

    python tools/brain_bench.py [--out profiles/brain_bench.json] [--reps 20]

(a) Inception1D(64, 8, 3, if_readout=True) forward and forward+backward at
    N = 1340 time courses (5 subjects x 268 regions) of T = 375 steps, and its
    kernels one by one: the convolutions as a fraction of the 157.3 TF fp32
    MFMA peak on their algorithmic flops (the non-zero taps of the three
    branches), max-pool and readout as a fraction of the 8 TB/s HBM peak on
    their algorithmic bytes.
(b) one eager forward+backward of the checkpoint-shaped HL_HGAT_attpool on 5
    copies of tests/golden/brain_skeleton.npz, coarse level from
    hlhgat.hodge_dataset.mlgc_weighted.
(d) the input side (hlhgat.pipeline.BrainPipeline, csrc/fc.hip) at B = 5,
    N = 268, T = 375 on the same skeleton: a batch, the row pass and the two
    correlation epilogues on their own, the dense epilogue on S = 50 subjects
    as a fraction of the fp32 MFMA peak, and a torch-ops restatement on the
    same device (per-subject torch.corrcoef plus the index).
(c) last, in a child process with its own time limit: the same front end on
    torch's conv1d / max_pool1d (MIOpen), for the ratio -- or the note that it
    did not finish.

(e) --train-step, a run of its own (profiles/brain_train_step.json): the
    notebook's training step -- HL_HGAT_attpool at the checkpoint shape on 5
    copies of the skeleton, T = 375, hlhgat.nn.MSELoss, Adam(lr=1e-4,
    weight_decay=1e-4) -- under TrainStep(graphs=False) and
    TrainStep(graphs=True) in the same process: events and wall time per step
    (median of 20 after 5 warm-up steps), and the replayed step's copy of the
    batch into the graph's static buffers (_Captured.load) on its own.

(f) --per-sample-windows, a run of its own (profiles/brain_ragged.json):
    per-sample fMRI windows.  Inception1D at N = 1340 on its
    ragged path with every length 275 against the dense path at T = 275, and
    with lengths drawn in [250, 300) at t_max = 299 against the dense path at
    T = 299: forward and forward + backward, the modes alternated in one
    process, median of --reps.  Then the first --aug-steps augmented training
    steps of (e)'s model at 5 subjects, captures included, wall time:
    window="random" (a graph per drawn length) against window="per_sample"
    (one graph), with the graphs captured and the bytes their static batches
    hold.

Event timing after warm-up, median of --reps runs.
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

PEAK_TF, PEAK_GBS = 157.3, 8000.0
N, T, C, NC, MP = 1340, 375, 64, 8, 3


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


class TorchInception1D(torch.nn.Module):
    """The same computation on torch's own GPU ops (NCT layout)."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.embedding = nn.Conv1d(1, C, 5, padding=2)
        self.s1 = nn.ModuleList([nn.Conv1d(C, C // 4, 1), nn.Conv1d(C, C // 2, 3, padding=1),
                                 nn.Conv1d(C, C // 4, 5, padding=2)])
        self.s2 = nn.ModuleList([nn.Conv1d(C, NC, 1), nn.Conv1d(C, 2 * NC, 3, padding=1),
                                 nn.Conv1d(C, NC, 5, padding=2)])
        self.bn1, self.bn2 = nn.BatchNorm1d(C), nn.BatchNorm1d(4 * NC)
        self.pool = nn.MaxPool1d(MP, stride=MP - 1, padding=(MP - 1) // 2)

    def forward(self, x):
        F = torch.nn.functional
        x = self.embedding(x.unsqueeze(1))
        x = self.pool(F.leaky_relu(self.bn1(torch.cat([c(x) for c in self.s1], 1)), 0.1))
        x = F.leaky_relu(self.bn2(torch.cat([c(x) for c in self.s2], 1)), 0.1)
        return torch.cat([x.max(-1)[0], x.mean(-1)], -1)


def front_end(mod, reps):
    dev = torch.device("cuda:0")
    mod = mod.to(dev).train()
    x = torch.randn(N, T, device=dev)

    def fwd():
        with torch.no_grad():
            return mod(x)

    def fwd_bwd():
        for p in mod.parameters():
            p.grad = None
        mod(x).sum().backward()

    return {"fwd_ms": round(timed(fwd, reps), 4), "fwd_bwd_ms": round(timed(fwd_bwd, reps), 4)}


def kernels(mod, reps):
    """The front end's kernels one at a time, at the shapes of (a)."""
    from hlhgat import ops
    dev = torch.device("cuda:0")
    rows = []

    def conv(name, convs, t):
        cin = convs[0].weight.size(1)
        ws, bs = [c.weight for c in convs], [c.bias for c in convs]
        x = torch.randn(N, t, cin, device=dev, requires_grad=True)
        flops = 2.0 * N * t * cin * sum(w.size(0) * w.size(2) for w in ws)
        with torch.no_grad():
            f = timed(lambda: ops.temporal_conv(x, ws, bs), reps)
        y = ops.temporal_conv(x, ws, bs)
        g = torch.randn_like(y)

        def bwd():
            torch.autograd.grad(y, [x] + ws + bs, g, retain_graph=True)

        b = timed(bwd, reps)
        rows.append({"kernel": name + " fwd", "ms": round(f, 4), "gflop": round(flops / 1e9, 3),
                     "frac_mfma_peak": round(flops / f / 1e9 / PEAK_TF, 4)})
        rows.append({"kernel": name + " bwd (data + weight)", "ms": round(b, 4),
                     "gflop": round(2 * flops / 1e9, 3),
                     "frac_mfma_peak": round(2 * flops / b / 1e9 / PEAK_TF, 4)})

    t2 = ops.maxpool_time_len(T, MP)
    conv("embedding (VALU)", [mod.embedding], T)
    conv("stage 1 conv", [mod.channel1_1, mod.channel2_1, mod.channel3_1], T)
    conv("stage 2 conv", [mod.channel1_2, mod.channel2_2, mod.channel3_2], t2)

    def mem(name, fn_f, x, out_bytes):
        with torch.no_grad():
            f = timed(lambda: fn_f(x), reps)
        y = fn_f(x)
        g = torch.randn_like(y)
        b = timed(lambda: torch.autograd.grad(y, [x], g, retain_graph=True), reps)
        by_f = 4.0 * x.numel() + out_bytes
        by_b = 8.0 * x.numel() + out_bytes  # x, dy + idx, dx
        rows.append({"kernel": name + " fwd", "ms": round(f, 4), "mbytes": round(by_f / 1e6, 2),
                     "frac_hbm_peak": round(by_f / f / 1e6 / PEAK_GBS, 4)})
        rows.append({"kernel": name + " bwd", "ms": round(b, 4), "mbytes": round(by_b / 1e6, 2),
                     "frac_hbm_peak": round(by_b / b / 1e6 / PEAK_GBS, 4)})

    x1 = torch.randn(N, T, C, device=dev, requires_grad=True)
    mem("leaky max-pool", lambda x: ops.leaky_maxpool_time(x, 0.1, MP), x1, 8.0 * N * t2 * C)
    x2 = torch.randn(N, t2, 4 * NC, device=dev, requires_grad=True)
    mem("readout", lambda x: ops.time_readout(x, 0.1), x2, 12.0 * N * 4 * NC)
    return rows


class _Level:
    pass


def skeleton_levels():
    """[fine, coarse] on tests/golden/brain_skeleton.npz (coarse level from
    hlhgat.hodge_dataset.mlgc_weighted) and the fine level's cluster maps."""
    from hlhgat.hodge_dataset import PairData, hodge_coo_from_boundary, mlgc_weighted
    g = np.load(os.path.join(REPO, "tests", "golden", "brain_skeleton.npz"))
    n = int(g["n_nodes"])
    ei = torch.from_numpy(g["edge_index"].astype(np.int64))
    E = ei.shape[1]
    ei_t, w_t, ei_s, w_s = hodge_coo_from_boundary(g["edge_index"], n, float(g["lmax"]))
    gen = torch.Generator().manual_seed(0)
    fine = PairData(x_s=torch.randn(E, 1, generator=gen), edge_index_s=ei_s, edge_weight_s=w_s,
                    x_t=torch.randn(n, T, generator=gen), edge_index_t=ei_t, edge_weight_t=w_t,
                    edge_index=ei)
    fine.num_node1, fine.num_edge1 = n, E
    coarse, c_node, c_edge = mlgc_weighted(fine)
    return fine, coarse, c_node, c_edge


def head(reps):
    import hlhgat
    dev = torch.device("cuda:0")
    B = 5
    fine, coarse, c_node, c_edge = skeleton_levels()
    n, E = int(fine.num_node1), int(fine.num_edge1)
    ei_s = fine.edge_index_s
    n1, E1 = int(coarse.num_node1), int(coarse.num_edge1)

    def level(d, nn_, ne_, xt, xs):
        lv = _Level()
        lv.x_t = torch.cat([xt] * B).to(dev)
        lv.x_s = torch.cat([xs] * B).to(dev)
        for side, cnt in (("t", nn_), ("s", ne_)):
            e = getattr(d, "edge_index_" + side)
            setattr(lv, "edge_index_" + side, torch.cat([e + b * cnt for b in range(B)], 1).to(dev))
            setattr(lv, "edge_weight_" + side,
                    getattr(d, "edge_weight_" + side).repeat(B).to(dev))
        lv.edge_index = torch.cat([torch.as_tensor(d.edge_index) + b * nn_ for b in range(B)],
                                  1).to(dev)
        lv.num_node1 = torch.full((B,), nn_, dtype=torch.int64)
        lv.num_edge1 = torch.full((B,), ne_, dtype=torch.int64)
        return lv

    l0 = level(fine, n, E, fine.x_t, fine.x_s)
    l1 = level(coarse, n1, E1, coarse.x_t, coarse.x_s)
    l0.pos_t = c_node.view(-1).repeat(B).to(dev)
    l0.pos_s = c_edge.view(-1).repeat(B).to(dev)
    m = hlhgat.HL_HGAT_attpool(channels=[2, 2, 2], filters=[32, 64, 128], mlp_channels=[], K=4,
                               pool_num=1, num_nodepedge=n1 + E1).to(dev).train()

    def step():
        for p in m.parameters():
            p.grad = None
        out = m([l0, l1], device=dev)[0]
        out.sum().backward()

    ms = timed(step, max(reps // 4, 5), warmup=2)
    return {"graphs": B, "nodes": n, "edges": E, "coarse_nodes": n1, "coarse_edges": E1,
            "nnz_L1": int(ei_s.shape[1]), "fwd_bwd_ms": round(ms, 3)}


def input_pipeline(reps):
    """(d) the input side at B = 5, N = 268, T = 375 on the same skeleton:
    BrainPipeline.batch (device time by events, host time per call without a
    sync), the row pass and the two correlation epilogues on their own, the
    dense epilogue on S = 50 subjects as a fraction of the fp32 MFMA peak, and
    a torch-ops restatement on the same device (per subject (f - mean) / std,
    torch.corrcoef, the index)."""
    import hlhgat
    from hlhgat import ops
    dev = torch.device("cuda:0")
    B, S = 5, 50
    fine, coarse, c_node, c_edge = skeleton_levels()
    fine.pos_t, fine.pos_s = c_node.view(-1), c_edge.view(-1)
    n, E = int(fine.num_node1), int(fine.num_edge1)
    rng = np.random.default_rng(0)
    series = [((rng.standard_normal((n, 6)) @ rng.standard_normal((6, T))
                + rng.standard_normal((n, T))) * 50 + 1000).astype(np.float32) for _ in range(S)]
    pipe = hlhgat.BrainPipeline(series, np.zeros(S, np.float32), [fine, coarse])
    t0 = time.perf_counter()
    pipe.batch(range(B), device=dev)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - t0  # collation of the level list, uploads
    it = [0]

    def one_batch():
        k = it[0] = (it[0] + B) % S
        return pipe.batch([(k + j) % S for j in range(B)], device=dev)

    batch_ms = timed(one_batch, reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        one_batch()
    host_ms = (time.perf_counter() - t0) * 1e3 / reps
    torch.cuda.synchronize()

    table, tiles = (t.to(dev) for t in ops.fc_pair_table(fine.edge_index, n))
    block = torch.from_numpy(np.stack(series)).to(dev).view(S * n, T)
    x5 = block[:B * n]
    prep5 = ops.fc_prepare(x5, B)
    ws5, z5 = prep5.workspace, prep5.z
    out = torch.empty(B * E, 1, device=dev)
    fc5 = torch.empty(B, n, n, device=dev)
    res = {"graphs": B, "nodes": n, "T": T, "edges": E, "edge_tiles": int(tiles.shape[0]),
           "first_batch_s": round(first_s, 3), "batch_ms": round(batch_ms, 4),
           "batch_host_ms": round(host_ms, 4),
           "prepare_ms": round(timed(lambda: ops.fc_prepare(x5, B, workspace=ws5, z=z5), reps), 4),
           "prepare_no_z_ms": round(timed(lambda: ops.fc_prepare(x5, B, want_z=False,
                                                                 workspace=ws5), reps), 4),
           "edges_ms": round(timed(lambda: ops.fc_edges(prep5, table, E, out=out, tiles=tiles),
                                   reps), 4),
           "dense_ms": round(timed(lambda: ops.fc_dense(prep5, out=fc5), reps), 4)}
    # the cohort-sized dense stack (FC2mask's input)
    prep50 = ops.fc_prepare(block, S, want_z=False)
    fc50 = torch.empty(S, n, n, device=dev)
    ms50 = timed(lambda: ops.fc_dense(prep50, out=fc50), reps)
    nt = -(-n // ops.FC_TILE)
    tp = -(-T // 4) * 4
    run_flops = 2.0 * S * (nt * (nt + 1) // 2) * ops.FC_TILE ** 2 * tp  # the tiles computed
    alg_flops = 2.0 * S * n * n * T                                      # a full [N,T][T,N]
    res["dense_S50"] = {"ms": round(ms50, 4), "gflop_full_product": round(alg_flops / 1e9, 3),
                        "gflop_tiles_run": round(run_flops / 1e9, 3),
                        "frac_mfma_peak_full_product": round(alg_flops / ms50 / 1e9 / PEAK_TF, 4),
                        "frac_mfma_peak_tiles_run": round(run_flops / ms50 / 1e9 / PEAK_TF, 4)}
    ei = fine.edge_index.to(dev)

    def torch_batch():
        xt, xs = [], []
        for b in range(B):
            f = block[b * n:(b + 1) * n]
            f = (f - f.mean()) / f.std()
            xt.append(f)
            xs.append(torch.corrcoef(f)[ei[0], ei[1]].view(-1, 1))
        return torch.cat(xt), torch.cat(xs)

    def torch_dense():
        return torch.stack([torch.corrcoef(block[i * n:(i + 1) * n]) for i in range(S)])

    xt, xs = torch_batch()
    res["torch_ops"] = {"batch_ms": round(timed(torch_batch, reps), 4),
                        "dense_S50_ms": round(timed(torch_dense, reps), 4),
                        "max_abs_diff_x_t": float((xt - z5).abs().max()),
                        "max_abs_diff_x_s": float((xs - ops.fc_edges(prep5, table, E,
                                                                     tiles=tiles)).abs().max())}
    res["torch_ops"]["ratio_batch"] = round(res["torch_ops"]["batch_ms"] / batch_ms, 3)
    res["torch_ops"]["ratio_dense_S50"] = round(res["torch_ops"]["dense_S50_ms"] / ms50, 3)
    return res


def timed_wall(fn, reps, warmup):
    """(event ms, wall ms) per call, medians; the wall time includes the wait
    for the device to finish the call's work."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return round(float(np.median(ev)), 4), round(float(np.median(wall)), 4)


def train_step(reps=20, warmup=5):
    """(e) the notebook's training step, eager against replayed."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.train import TrainStep, batch_key
    dev = torch.device("cuda:0")
    B, S = 5, 10
    fine, coarse, c_node, c_edge = skeleton_levels()
    fine.pos_t, fine.pos_s = c_node.view(-1), c_edge.view(-1)
    n, E = int(fine.num_node1), int(fine.num_edge1)
    n1, E1 = int(coarse.num_node1), int(coarse.num_edge1)
    rng = np.random.default_rng(0)
    series = [((rng.standard_normal((n, 6)) @ rng.standard_normal((6, T))
                + rng.standard_normal((n, T))) * 50 + 1000).astype(np.float32) for _ in range(S)]
    targets = rng.standard_normal(S).astype(np.float32)
    pipe = hlhgat.BrainPipeline(series, targets, [fine, coarse])
    batches = [pipe.batch([(k * B + j) % S for j in range(B)], device=dev) for k in range(2)]
    batches = [[copy.copy(b[0])] + b[1:] for b in batches]
    for b in batches:  # the pipeline reuses its workspace: keep each batch's own values
        b[0].x_t, b[0].x_s = b[0].x_t.clone(), b[0].x_s.clone()
    mse = hlhgat.nn.MSELoss()
    res = {"graphs": B, "nodes": n, "edges": E, "coarse_nodes": n1, "coarse_edges": E1, "T": T,
           "reps": reps, "warmup": warmup, "parent_eager_head_fwd_bwd_ms": 9.87}
    first = {}
    for graphs in (False, True):
        torch.manual_seed(0)
        m = hlhgat.HL_HGAT_attpool(channels=[2, 2, 2], filters=[32, 64, 128], mlp_channels=[],
                                   K=4, pool_num=1, num_nodepedge=n1 + E1).to(dev).train()
        step = TrainStep(m, lambda o, d: mse(o[0], d[0].y.view(-1, 1)), lr=1e-4,
                         weight_decay=1e-4, graphs=graphs)
        first[graphs] = float(step(batches[0]))
        it = [0]

        def one():
            it[0] += 1
            return step(batches[it[0] % len(batches)])

        ev, wall = timed_wall(one, reps, warmup)
        name = "replayed" if graphs else "eager"
        res[name] = {"step_event_ms": ev, "step_wall_ms": wall, "stats": dict(step.stats)}
        ops.check_device_errors()
        if graphs:
            ent = step._graphs[batch_key(batches[0])]
            lev, lwall = timed_wall(lambda: ent.load(batches[(it[0] + 1) % len(batches)]), reps,
                                    warmup)
            tensors = [v for b in batches[0] for k, v in vars(b).items()
                       if torch.is_tensor(v) and not k.startswith("_")]
            res["load"] = {"event_ms": lev, "wall_ms": lwall, "tensors": len(tensors),
                           "mbytes": round(sum(v.numel() * v.element_size()
                                               for v in tensors) / 1e6, 3),
                           "share_of_replayed_step_event": round(lev / ev, 4)}
    res["first_loss_equal"] = first[False] == first[True]
    res["ratio_eager_over_replayed_event"] = round(
        res["eager"]["step_event_ms"] / res["replayed"]["step_event_ms"], 3)
    return res


def _alternated(fns, reps, warmup=3):
    """Median event ms of every fn, the fns taking turns inside one loop."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: round(float(np.median(v)), 4) for k, v in ms.items()}


def ragged_front_end(reps):
    """(f), kernel cost: ragged against dense Inception1D, alternated."""
    import hlhgat
    from hlhgat import ops
    dev = torch.device("cuda:0")
    mod = hlhgat.Inception1D(C, NC, MP, if_readout=True).to(dev).train()
    rng = np.random.default_rng(0)
    out = {}
    for name, t_max, lens in (("equal_275", 275, np.full(N, 275)),
                              ("drawn_250_300", 299, rng.integers(250, 300, size=N))):
        x = torch.randn(N, t_max, device=dev)
        ln = torch.from_numpy(lens.astype(np.int32)).to(dev)

        def run(lengths, grad):
            if not grad:
                with torch.no_grad():
                    return mod(x, lengths)
            for p in mod.parameters():
                p.grad = None
            mod(x, lengths).sum().backward()

        ms = _alternated({"dense_fwd": lambda: run(None, False), "ragged_fwd": lambda: run(ln, False),
                          "dense_fwd_bwd": lambda: run(None, True),
                          "ragged_fwd_bwd": lambda: run(ln, True)}, reps)
        ms["t_max"], ms["dead_row_share"] = t_max, round(1.0 - float(lens.sum()) / (N * t_max), 4)
        ms["ratio_fwd"] = round(ms["ragged_fwd"] / ms["dense_fwd"], 4)
        ms["ratio_fwd_bwd"] = round(ms["ragged_fwd_bwd"] / ms["dense_fwd_bwd"], 4)
        out[name] = ms
    ops.check_device_errors()
    return out


def augmented_replay(steps):
    """(f), replay under augmentation: the first `steps` training steps."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.train import TrainStep
    dev = torch.device("cuda:0")
    B, S = 5, 10
    fine, coarse, c_node, c_edge = skeleton_levels()
    fine.pos_t, fine.pos_s = c_node.view(-1), c_edge.view(-1)
    n1, E1 = int(coarse.num_node1), int(coarse.num_edge1)
    rng = np.random.default_rng(0)
    n = int(fine.num_node1)
    series = [((rng.standard_normal((n, 6)) @ rng.standard_normal((6, T))
                + rng.standard_normal((n, T))) * 50 + 1000).astype(np.float32) for _ in range(S)]
    pipe = hlhgat.BrainPipeline(series, rng.standard_normal(S).astype(np.float32), [fine, coarse])
    mse = hlhgat.nn.MSELoss()
    res = {"graphs": B, "steps": steps}
    for window in ("random", "per_sample"):
        torch.manual_seed(0)
        m = hlhgat.HL_HGAT_attpool(channels=[2, 2, 2], filters=[32, 64, 128], mlp_channels=[],
                                   K=4, pool_num=1, num_nodepedge=n1 + E1).to(dev).train()
        step = TrainStep(m, lambda o, d: mse(o[0], d[0].y.view(-1, 1)), lr=1e-4,
                         weight_decay=1e-4, graphs=True)
        pipe.batch(range(B), window=window, seed=0, device=dev)  # the level list is collated
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            loss = step(pipe.batch([(k * B + j) % S for j in range(B)], window=window, seed=k,
                                   device=dev))
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        held = sum(v.numel() * v.element_size() for ent in step._graphs.values()
                   for b in (ent.batch if isinstance(ent.batch, (list, tuple)) else [ent.batch])
                   for v in vars(b).values() if torch.is_tensor(v))
        res[window] = {"wall_s": round(wall, 3), "ms_per_step": round(wall * 1e3 / steps, 3),
                       "graphs_captured": int(step.stats["captures"]),
                       "graphs_held": len(step._graphs),
                       "static_batch_mbytes": round(held / 1e6, 1),
                       "stats": dict(step.stats), "last_loss": float(loss)}
        ops.check_device_errors()
        del step, m
        torch.cuda.empty_cache()
    return res


def torch_child(args, res):
    """Last GPU step of the run: torch's own ops in a child with a time limit."""
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-only", "--reps",
                            str(args.reps)], capture_output=True, text=True,
                           timeout=args.torch_timeout)
        if r.returncode == 0:
            tt = json.loads(r.stdout.strip().splitlines()[-1])
            tt["ratio_fwd"] = round(tt["fwd_ms"] / res["inception1d_hip"]["fwd_ms"], 3)
            tt["ratio_fwd_bwd"] = round(tt["fwd_bwd_ms"] / res["inception1d_hip"]["fwd_bwd_ms"], 3)
            res["inception1d_torch_ops"] = tt
        else:
            res["inception1d_torch_ops"] = {"error": r.stderr.strip()[-400:]}
    except subprocess.TimeoutExpired:
        res["inception1d_torch_ops"] = {
            "error": f"torch conv1d / max_pool1d did not finish in {args.torch_timeout} s "
                     f"(waited {time.time() - t0:.0f} s)"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "brain_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-only", action="store_true")
    ap.add_argument("--torch-timeout", type=int, default=150)
    ap.add_argument("--skip-head", action="store_true")
    ap.add_argument("--skip-input", action="store_true")
    ap.add_argument("--only-input", action="store_true",
                    help="the input-pipeline leg alone, merged into an existing --out file")
    ap.add_argument("--skip-torch", action="store_true",
                    help="no torch-ops child (e.g. under a kernel trace)")
    ap.add_argument("--train-step", action="store_true",
                    help="the training-step leg alone (eager against replayed), written to "
                         "--train-out")
    ap.add_argument("--train-out", default=os.path.join(REPO, "profiles",
                                                        "brain_train_step.json"))
    ap.add_argument("--per-sample-windows", action="store_true",
                    help="the ragged front end against the dense one and the first augmented "
                         "training steps, written to --ragged-out")
    ap.add_argument("--ragged-out", default=os.path.join(REPO, "profiles", "brain_ragged.json"))
    ap.add_argument("--aug-steps", type=int, default=200)
    args = ap.parse_args()
    if args.per_sample_windows:
        res = {"shape": {"N": N, "in_channels": C, "num_channels": NC, "maxpool": MP},
               "reps": args.reps, "front_end": ragged_front_end(args.reps)}
        if args.aug_steps > 0:
            res["augmented_replay"] = augmented_replay(args.aug_steps)
        os.makedirs(os.path.dirname(args.ragged_out), exist_ok=True)
        with open(args.ragged_out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if args.train_step:
        res = train_step()
        os.makedirs(os.path.dirname(args.train_out), exist_ok=True)
        with open(args.train_out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return
    if args.torch_only:
        print(json.dumps(front_end(TorchInception1D(), args.reps)), flush=True)
        return
    if args.only_input:
        with open(args.out) as f:
            res = json.load(f)
        res["input_pipeline"] = input_pipeline(args.reps)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res["input_pipeline"]))
        return
    import hlhgat
    from hlhgat import _lib, ops
    res = {"shape": {"N": N, "T": T, "in_channels": C, "num_channels": NC, "maxpool": MP},
           "bn_rows": N * T,
           "bn_workspace_bytes": int(_lib.LIB.hlhgat_bn_workspace_bytes(N * T, C))}
    mod = hlhgat.Inception1D(C, NC, MP, if_readout=True)
    res["inception1d_hip"] = front_end(mod, args.reps)
    with torch.no_grad():
        y = mod(torch.randn(N, T, device="cuda:0"))
    res["bn_502500_rows_ok"] = bool(torch.isfinite(y).all())
    ops.check_device_errors()
    res["kernels"] = kernels(mod, args.reps)
    if not args.skip_head:
        res["head_5x_skeleton"] = head(args.reps)
    if not args.skip_input:
        res["input_pipeline"] = input_pipeline(args.reps)
    ops.check_device_errors()
    torch.cuda.synchronize()
    if not args.skip_torch:
        torch_child(args, res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
