"""HL-HGAT training throughput on MI355X (BASELINE.json metric, config 2).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--eager]
                    [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and nothing else: it builds
the batches and the model, runs W warm-up steps, times exactly K steps, writes
the last timed step's results if `--dump-outputs DIR` is given (the loss the
step returned and the training state it left, `DIR/<name>.npy`, float32; the
inputs and the initial weights are seeded, so two builds can be compared
array for array) and prints one short JSON line.  `--full` adds every other
leg to that line: the parity check against the oracle, the kernel rooflines
(stamped eager pass, rocprofv3 child), the config-5 SpMM, the H2D, eval and
loader legs, the CPU oracle baseline and the configs 3-5 heads; the `--no-*`
options drop single legs of a `--full` run.

N > 1: one rank per GPU over RCCL.  Under torch.distributed.run (RANK set)
every rank runs the step directly; run plainly, `--gpus N` starts the N ranks
itself (a child torch.distributed.run on 127.0.0.1, spawned before anything
touches the GPU) and only waits for them.  Every rank checks that the world
size equals --gpus; rank 0 prints the JSON line with n_gpus = world size.
`--dry-run` runs the same launcher, rendezvous, barrier and max-over-ranks
timing on gloo / CPU with a trivial step (the CPU test of the launcher).

A step = one training step of HL_HGCNN_zinc_dense_int3_pyr(channels=[2,2,2],
filters=[64,64,64], mlp=[256,256], K=3, keig=15) on a 1000-graph batch of
synthetic ZINC-like simplex graphs per GPU (weak scaling): the batch is
copied into the step's static buffers, then forward, L1 loss, backward,
gradient all-reduce (N > 1) and Adam.  The batch's CSR / incidence / degree /
segment tables come with it from the data loader (collate), as the
reference's DataLoader hands the step a collated batch; the `loader` leg
times that host work.
Inputs are resident in HBM before the timed region (8 distinct batches,
rotated, padded to one capacity bucket).  The step runs as ONE replayed
hipGraph for every batch of the bucket (hlhgat.train.TrainStep +
hodge_dataset.pad_batch; --eager runs it op by op).  With --full, after the
timed region a short eager pass with hipExtLaunchKernel event stamps on the
SpMM and the projection kernels gives the roofline figures.  Rank 0 prints one
JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

GRAPHS_PER_GPU = 1000
MODEL_KW = dict(channels=[2, 2, 2], filters=[64, 64, 64], mlp_channels=[256, 256], K=3, keig=15)
HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
FP32_MFMA_PEAK_TFS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, spec


def log(*a):
    print(*a, file=sys.stderr, flush=True)


# worker processes generating the synthetic graphs (set by main(): only when
# this file is the program, so that a spawned worker re-imports nothing else)
GEN_PROCS = 1


def _zinc_chunk(seeds):
    """Pool worker: the graphs of `seeds` as plain dicts of numpy arrays (a
    tensor would travel as a shared-memory handle each)."""
    from hlhgat.synthetic import zinc_like_graph
    torch.set_num_threads(1)
    return [{k: v.numpy() if torch.is_tensor(v) else v
             for k, v in vars(zinc_like_graph(s, 15)).items()} for s in seeds]


def zinc_graphs(seeds):
    """zinc_like_graph(s, 15) for every seed, in order.  Each graph is a
    function of its own seed alone, so GEN_PROCS spawned CPU workers (they
    never touch the GPU) build the same graphs, bit for bit, as the serial
    loop; 8000 graphs take ~20 s of Python on one core."""
    import numpy as np
    from hlhgat.hodge_dataset import PairData
    from hlhgat.synthetic import zinc_like_graph
    if GEN_PROCS <= 1 or len(seeds) < 512:
        return [zinc_like_graph(s, 15) for s in seeds]
    import multiprocessing as mp
    chunks = [seeds[i:i + 125] for i in range(0, len(seeds), 125)]
    with mp.get_context("spawn").Pool(GEN_PROCS) as pool:
        parts = pool.map(_zinc_chunk, chunks, chunksize=1)
    return [PairData(**{k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v
                        for k, v in d.items()})
            for part in parts for d in part]


def make_batches(n_batches, rank, device, quantum=512, caps=None):
    """n_batches distinct synthetic 1000-graph batches, padded to ONE capacity
    bucket (the max of their static_caps) so that a single captured hipGraph
    replays every one of them -- as a training loop pads its DataLoader
    batches to the dataset's bucket.  The graphs are packed once
    (hodge_dataset.PackedGraphs, the InMemoryDataset-style storage) and each
    batch is collated by the native loader (hlhgat_collate: bitwise
    collate + pad_batch, tests/test_host.py)."""
    import numpy as np
    from hlhgat.hodge_dataset import PackedGraphs
    graphs = zinc_graphs([(1 + rank * 101 + i) * 1_000_003 + j
                          for i in range(n_batches) for j in range(GRAPHS_PER_GPU)])
    ds = PackedGraphs(graphs, check_hodge=False)
    idxs = [np.arange(i * GRAPHS_PER_GPU, (i + 1) * GRAPHS_PER_GPU) for i in range(n_batches)]
    if caps is None:
        cs = [ds.caps_for(i, quantum) for i in idxs]
        caps = {k: max(c[k] for c in cs) for k in cs[0]}
    real = sum(sum(ds.sizes(i)[:2]) for i in idxs) / n_batches
    return [ds.collate(i, caps).to(device) for i in idxs], caps, real, ds.collate(idxs[0]), ds


def loader_leg(ds, step, caps, device, ms_step, steps=16, depth=2, workers=4, stream=True,
               priority=0, switch_ms=None, slots=None, thread=True):
    """The data loader beside the step (the reference feeds every step from a
    DataLoader with 4 workers and copies the batch in, main_zinc...:151-162,
    223-225).  Here: graphs/s of hlhgat.loader.GraphLoader (native collate +
    padding + batch tables into pinned memory) with W worker threads; the
    Python collate + pad_batch on one core for comparison; and the training
    loop fed by the loader end to end -- collation on 4 threads, the H2D copy
    of batch i+1 on a copy stream while step i runs, the replayed step."""
    import numpy as np
    from hlhgat.hodge_dataset import collate, pad_batch
    from hlhgat.loader import GraphLoader
    n = len(ds) // GRAPHS_PER_GPU
    out = {"graphs_per_batch": GRAPHS_PER_GPU, "batches": n,
           "reference_loop": "torch_geometric DataLoader(num_workers=4) + data.to(device) per step"}
    rates = {}
    for w in (1, 2, 4):
        ld = GraphLoader(ds, GRAPHS_PER_GPU, caps=caps, workers=w, prefetch=2 * w, pin=True)
        list(ld)  # warm (page faults, pinned pool)
        t0 = time.perf_counter()
        nb = 0
        for _ in range(2):
            for _b in ld:
                nb += 1
        rates[str(w)] = round(nb * GRAPHS_PER_GPU / (time.perf_counter() - t0), 1)
    out["native_collate_graphs_per_s"] = rates
    graphs = [ds.graph(i) for i in range(GRAPHS_PER_GPU)]
    t0 = time.perf_counter()
    for _ in range(2):
        pad_batch(collate(graphs, check_hodge=False), caps)
    out["python_collate_graphs_per_s_1core"] = round(2 * GRAPHS_PER_GPU / (time.perf_counter() - t0), 1)
    # the loader-fed loop: GraphLoader(4 threads, pinned; GraphLoader.stream:
    # one collation pool prefetching across epochs) -> StagedFeed (a
    # feeder thread: TrainStep.stage, H2D on a copy stream straight into the
    # static buffers of a captured graph, two batches ahead) -> the replayed
    # step with no copy-in, launched from this thread alone
    from hlhgat.loader import StagedFeed
    ld = GraphLoader(ds, GRAPHS_PER_GPU, caps=caps, workers=workers, prefetch=2 * workers,
                     pin=True)
    cs = torch.cuda.Stream(device=device, priority=priority)
    # one captured graph more than depth + 1: the slot a batch is staged into
    # was released a step earlier, so the feeder rarely waits for it
    slots = slots or depth + 2
    step.stage_slots = max(step.stage_slots, slots)

    def per_epoch():
        while True:
            for b in ld:
                yield b

    feed = StagedFeed(ld.stream() if stream else per_epoch(), step, depth=depth, stream=cs,
                      thread=thread)
    it = iter(feed)
    old_switch = sys.getswitchinterval()
    if switch_ms:
        sys.setswitchinterval(switch_ms * 1e-3)
    host = {"wait_feed": 0.0, "step_call": 0.0}
    warm = step.stage_slots + 1  # the first steps capture the shape's graphs (one per slot)
    for i in range(steps + warm):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host = {k: 0.0 for k in host}
            feed.timing.update(source=0.0, room=0.0, stage=0.0, n=0)
            step.stage_timing.update(dict.fromkeys(step.stage_timing, 0.0))
        ta = time.perf_counter()
        st = next(it)
        tb = time.perf_counter()
        step(st)
        tc = time.perf_counter()
        host["wait_feed"] += tb - ta
        host["step_call"] += tc - tb
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    it.close()  # stops the feeder thread and the loader's collation threads
    sys.setswitchinterval(old_switch)
    torch.cuda.synchronize()
    ops_mod = __import__("hlhgat").ops
    ops_mod.check_device_errors()
    out["loader_fed"] = {"value": round(GRAPHS_PER_GPU / dt, 1), "unit": "graphs/s",
                         "ms_per_step": round(dt * 1e3, 3), "workers": workers, "pinned": True,
                         "across_epochs": bool(stream), "steps": steps, "stage_depth": depth,
                         "copy_stream_priority": priority, "stage_slots": step.stage_slots,
                         "feeder_thread": bool(thread),
                         "gil_switch_ms": switch_ms if switch_ms else round(old_switch * 1e3, 3),
                         "host_ms_per_step": {k: round(v / steps * 1e3, 3) for k, v in host.items()},
                         "feeder_ms_per_batch": {k: round(feed.timing[k] / max(1, feed.timing["n"]) * 1e3, 3)
                                                 for k in ("source", "room", "stage")},
                         "stage_ms_per_batch": {k: round(v / max(1, step.stage_timing["n"]) * 1e3, 3)
                                                for k, v in step.stage_timing.items() if k != "n"},
                         "what": "training steps fed by GraphLoader end to end: native collate "
                                 "on 4 threads, hlhgat.loader.StagedFeed's thread uploading "
                                 "(TrainStep.stage: one H2D copy per batch on a copy stream, "
                                 "straight into the static buffers of one of the shape's "
                                 "captured graphs) two batches ahead, the replayed step (no "
                                 "copy-in) launched from the training thread alone"}
    out["device_resident_ms_per_step"] = round(ms_step, 3)
    return out


# kernel classes of the replayed step whose rooflines the bench reports
# (name regex in the rocprofv3 trace, hlhgat_prof class, bound)
# k_poly_step's call sites, one hlhgat_prof class each (per-call-site census
# below); the kernel's roofline sums them, like the rocprof average does
POLY_SITES = (("Laplacian basis (L0 / L1 Laguerre steps, fwd)", "PROF_POLY"),
              ("adjoint recurrence (basis backward)", "PROF_POLY_ADJ"),
              ("|B1| incidence gather (NodeEdgeInt node rows)", "PROF_INCIDENCE"))
POLY_CLASSES = tuple(c for _, c in POLY_SITES)


def prof_sum(L, names):
    """hlhgat_prof_read summed over the classes `names` (one name or a tuple)"""
    from hlhgat import ops
    names = (names,) if isinstance(names, str) else names
    tot = {"launches": 0, "ms": 0.0, "bytes": 0.0, "flops": 0.0}
    for nm in names:
        p = ops.prof_read(getattr(L, nm))
        for k in tot:
            tot[k] += p[k]
    return tot


def prof_enable_all(L, names, on):
    from hlhgat import ops
    for nm in names:
        for c in ((nm,) if isinstance(nm, str) else nm):
            ops.prof_enable(getattr(L, c), on)


REPLAY_CLASSES = {
    "k_poly_step": (r"k_poly_step<", POLY_CLASSES, "hbm"),
    "k_edge_gather2": (r"k_edge_gather2<", "PROF_GATHER2", "hbm"),
    "k_proj_bwd_fused": (r"k_proj_bwd_fused<", "PROF_PROJ_BWD", "mfma"),
    "k_proj_fwd": (r"k_proj_fwd", "PROF_PROJ", "mfma"),
    "k_proj_bn_fwd": (r"k_proj_bn_fwd", "PROF_PROJ_BN", "mfma"),
    "k_bn_fwd_grid": (r"k_bn_fwd_grid<", "PROF_BN_FWD", "hbm"),
    "k_bn_bwd_reduce": (r"k_bn_bwd_reduce<", "PROF_BN_BWD", "hbm"),
}


def replay_probe(args):
    """Child mode (--replay-probe, run under rocprofv3 by replay_census): the
    timed workload's replayed step -- same model, same capacity bucket, two
    of the batches -- warmed up, captured, then replayed; nothing else."""
    from hlhgat.distributed import init_distributed
    import hlhgat
    from hlhgat.train import TrainStep
    caps = json.loads(args.replay_probe)
    _, _, device = init_distributed("nccl")
    batches, _, _, _, _ = make_batches(2, 0, device, caps=caps)
    torch.manual_seed(0)
    model = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**MODEL_KW).to(device).train()
    crit = hlhgat.nn.L1Loss()
    step = TrainStep(model, lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1)), lr=1e-3,
                     weight_decay=1e-3, graphs=True)
    for i in range(args.warmup + args.steps):
        step(batches[i % 2])
    torch.cuda.synchronize()
    assert step.stats["replay"] >= args.steps, step.stats


def replay_census(caps, eager, steps=12, warmup=4, timeout=300):
    """Kernel durations INSIDE the replayed training step: this script's
    --replay-probe child under `rocprofv3 --kernel-trace` (a child process,
    started after this process's own GPU work; no exec).  Per replayed step
    (delimited by the Adam kernel): dispatches, span, the union of busy time
    over all queues (idle = span - busy), and per kernel class the summed
    duration.  `eager`: the algorithmic bytes / flops per step of each class
    from the stamped eager pass (same launches), so achieved = work per step
    / replayed kernel time per step."""
    import csv
    import re
    import shutil
    import tempfile
    rp = shutil.which("rocprofv3")
    if rp is None:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="hlhgat_replay_")
    cmd = [rp, "--kernel-trace", "-d", d, "-o", "run", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--replay-probe", json.dumps(caps),
           "--steps", str(steps), "--warmup", str(warmup)]
    try:
        r = subprocess.run(cmd, timeout=timeout, stdout=subprocess.DEVNULL,
                           stderr=subprocess.PIPE, env=dict(os.environ, TMPDIR="/tmp"))
        if r.returncode != 0:
            return None, f"replay probe exited {r.returncode}: {r.stderr.decode()[-300:]}"
        traces = [os.path.join(root, f) for root, _, fs in os.walk(d) for f in fs
                  if f.endswith("kernel_trace.csv")]
        if not traces:
            return None, "no kernel trace written"
        rows = sorted(csv.DictReader(open(traces[0])), key=lambda x: int(x["Start_Timestamp"]))
    except (OSError, subprocess.SubprocessError) as e:
        return None, f"replay probe failed: {e}"
    finally:
        shutil.rmtree(d, ignore_errors=True)
    marks = [i for i, x in enumerate(rows) if "k_adam_flat" in x["Kernel_Name"]]
    if len(marks) < steps:
        return None, f"only {len(marks)} steps in the trace"
    sel = list(zip(marks[-steps:-1], marks[-steps + 1:]))  # the last steps-1 full replays
    per = {k: [0.0, 0] for k in REPLAY_CLASSES}
    spans, busys, disp = [], [], []
    for a, b in sel:
        st = rows[a + 1:b + 1]
        iv = sorted((int(x["Start_Timestamp"]), int(x["End_Timestamp"])) for x in st)
        span = iv[-1][1] - iv[0][0] if iv else 0
        busy, cur_s, cur_e = 0, None, None
        for s0, e0 in iv:
            if cur_e is None or s0 > cur_e:
                if cur_e is not None:
                    busy += cur_e - cur_s
                cur_s, cur_e = s0, e0
            else:
                cur_e = max(cur_e, e0)
        if cur_e is not None:
            busy += cur_e - cur_s
        spans.append(span)
        busys.append(busy)
        disp.append(len(st))
        for x in st:
            for k, (pat, _, _) in REPLAY_CLASSES.items():
                if re.search(pat, x["Kernel_Name"]):
                    per[k][0] += (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3
                    per[k][1] += 1
    n = len(sel)
    span_us = sum(spans) / n / 1e3
    busy_us = sum(busys) / n / 1e3
    out = {"steps_traced": n, "dispatches_per_step": round(sum(disp) / n, 1),
           "span_us": round(span_us, 1), "busy_us": round(busy_us, 1),
           "idle_us": round(span_us - busy_us, 1),
           "idle_frac": round((span_us - busy_us) / span_us, 4) if span_us else None,
           "kernels": {}}
    for k, (pat, cls, bound) in REPLAY_CLASSES.items():
        us, cnt = per[k][0] / n, per[k][1] / n
        e = eager.get(k)
        if not cnt or not e:
            continue
        work = e["flops"] if bound == "mfma" else e["bytes"]  # per step
        if bound == "mfma":
            ach, peak, unit = work / (us * 1e-6) / 1e12, FP32_MFMA_PEAK_TFS, "TFLOP/s"
        else:
            ach, peak, unit = work / (us * 1e-6) / 1e9, HBM_PEAK_GBS, "GB/s"
        out["kernels"][k] = {"bound": bound, "achieved": round(ach, 2), "peak": peak,
                             "unit": unit, "frac": round(ach / peak, 4),
                             "launches_per_step": round(cnt, 1),
                             "avg_launch_us": round(us / cnt, 2),
                             "time_per_step_us": round(us, 1),
                             "work_per_step": round(work),
                             "eager_launches_per_step": e["launches"]}
    return out, None


def parity_check(model, batch_dev, batch_cpu, tol=1e-4):
    """The timed workload at full size against the oracle: the first step's
    training-mode forward of the 1000-graph (padded) batch on the HIP path vs
    the oracle (oracle/hodge_ref.py, pinned to the reference's golden vectors)
    on the same, unpadded graphs with the same parameters.  Run on a copy of
    the model (a training-mode forward moves the BatchNorm running stats)."""
    import copy
    from oracle.hodge_ref import RefZincModel
    cores = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or os.cpu_count()
    torch.set_num_threads(cores)
    m = copy.deepcopy(model).train()
    with torch.no_grad():
        out = m(batch_dev).float().cpu()
    ref = RefZincModel(**MODEL_KW)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    with torch.no_grad():
        exp = ref.train()(batch_cpu)
    del m
    scale = max(1.0, float(exp.abs().max()))
    err = float((out - exp).abs().max()) / scale
    return {"graphs": int(batch_cpu.num_graphs), "outputs": int(exp.numel()),
            "max_rel_err": err, "tol": tol, "pass": bool(err <= tol),
            "what": "first-step training-mode forward of the timed 1000-graph batch (padded, "
                    "HIP) vs the oracle on the same unpadded graphs and parameters; "
                    "max|d| / max(1, max|oracle|)"}


def cpu_baseline(batch_cpu, budget_s=15.0):
    """Oracle (pure PyTorch CPU restatement of the reference path) on the host
    cores: same model, same 1000-graph batch, fwd + L1 + bwd + Adam step."""
    from oracle.hodge_ref import RefZincModel
    cores = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or os.cpu_count()
    torch.set_num_threads(cores)
    torch.manual_seed(0)
    m = RefZincModel(**MODEL_KW).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, weight_decay=1e-3)
    crit = torch.nn.L1Loss()

    def step():
        out = m(batch_cpu)
        loss = crit(out.view(-1, 1), batch_cpu.y.view(-1, 1))
        loss.backward()
        opt.step()
        opt.zero_grad()

    step()  # warm-up
    times = []
    t_start = time.perf_counter()
    while len(times) < 3 or (time.perf_counter() - t_start < budget_s and len(times) < 30):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    times.sort()
    med = times[len(times) // 2]
    return {"value": GRAPHS_PER_GPU / med, "unit": "graphs/s", "cores": cores, "kind": "port",
            "sample": f"{len(times)} training steps (fwd+L1+bwd+Adam) of the oracle model on one "
                      f"{GRAPHS_PER_GPU}-graph synthetic ZINC batch, median step {med*1e3:.1f} ms"}


def pmc_traffic(kernel="k_poly_step"):
    """HBM traffic per launch of `kernel` at this workload, from the newest
    committed rocprofv3 PMC summary (profiles/*_pmc_traffic.json, written by
    tools/pmc_traffic.py from two --pmc passes of this bench: FETCH_SIZE x2
    (gfx950 wide-load correction) + WRITE_SIZE, MI355X_MICROARCH.md §HBM).
    Counters cannot be read from inside the timed process, so the figure is
    the committed measurement of the same command; None if absent."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc_traffic.json")))
    for path in reversed(files):
        try:
            with open(path) as f:
                k = json.load(f)["kernels"].get(kernel)
        except (OSError, ValueError, KeyError):
            continue
        if k:
            return k["traffic_bytes"], os.path.relpath(path, REPO)
    return None, None


def cfg5_spmm(device, reps=20):
    """The north-star SpMM roofline at BASELINE configs[4] (TSP-like simplex
    graphs, 4 x 10k nodes per GPU, L1 n ~ 207k rows, nnz ~ 4.1M): Y = L1 X
    and one fused Laguerre step, as the product runs them (dataset row
    schedule + LDS halo tiles), each launch timed with hipExtLaunchKernel
    stamps.  Algorithmic bytes: SpMM 8 nnz + 4 (n+1) + 8 n d,
    step 8 nnz + 4 (n+1) + 12 n d.  A kernel-level figure; config 5's model
    is not the bench workload."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.hodge_dataset import collate
    from hlhgat.synthetic import tsp_like_graph
    b = collate([tsp_like_graph(s) for s in range(4)], check_hodge=False).to(device)
    n, nnz = b.x_s.shape[0], b.edge_index_s.shape[1]
    op = ops.hodge_operator(b.edge_index_s, b.edge_weight_s, n)
    A = op.fwd
    out = {"config": f"BASELINE configs[4]: 4 TSP-like graphs (10k nodes, k=9 NN), L1 n={n} "
                     f"nnz={nnz}; RCM row schedule + LDS halo tiles "
                     f"({'on' if A.halo is not None else 'off'}); factored L1 "
                     f"({'on' if op.factor is not None else 'off'})",
           "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s"}
    for d in (64, 128):
        X = torch.randn(n, d, device=device)
        Z = torch.randn(n, d, device=device)
        Y = torch.empty(n, d, device=device)
        for what, kw in (("spmm", {}),
                         ("laguerre_step", dict(Z=Z, alpha=-1.0, beta=5.0, gamma=-2.0, div=3.0))):
            for _ in range(3):
                ops._poly_step(A, X, Y, **kw)
            torch.cuda.synchronize()
            ops.prof_reset()
            ops.prof_enable(hlhgat._lib.PROF_POLY, True)
            for _ in range(reps):
                ops._poly_step(A, X, Y, **kw)
            torch.cuda.synchronize()
            ops.prof_enable(hlhgat._lib.PROF_POLY, False)
            p = ops.prof_read(hlhgat._lib.PROF_POLY)
            gbs = p["bytes"] / (p["ms"] * 1e-3) / 1e9
            out[f"{what}_d{d}"] = {"achieved": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
                                   "avg_launch_us": round(p["ms"] * 1e3 / p["launches"], 1)}
        if op.factor is None:
            continue
        # factored L1 = alpha B1^T B1 (hlhgat_hodge_factor_t): stage 1 (B1 X, node
        # rows) + stage 2 (fused edge step).  "own" = the factored algorithm's
        # own algorithmic bytes (incidence, X once, Z written and read once,
        # Y and the epilogue operands) over the two launches' summed time: its
        # roofline.  "equiv" = the CSR problem's bytes (incl. the
        # 8 B/nnz CSR the factored path never reads) over the same time: a
        # speed comparison with the CSR rows above, not a roofline.
        work = torch.empty(int(hlhgat._lib.LIB.hlhgat_hodge_factor_work_floats(
            op.factor_nodes, d)), device=device)
        for what, kw, by in (
                ("spmm", {}, 8 * nnz + 4 * (n + 1) + 8 * n * d),
                ("laguerre_step", dict(Z=Z, alpha=-1.0, beta=5.0, gamma=-2.0, div=3.0),
                 8 * nnz + 4 * (n + 1) + 12 * n * d)):
            for _ in range(3):
                ops._hodge_step(op, X, Y, work=work, **kw)
            torch.cuda.synchronize()
            ops.prof_reset()
            classes = (hlhgat._lib.PROF_HODGE_NODE, hlhgat._lib.PROF_HODGE_EDGE)
            for c in classes:
                ops.prof_enable(c, True)
            for _ in range(reps):
                ops._hodge_step(op, X, Y, work=work, **kw)
            torch.cuda.synchronize()
            for c in classes:
                ops.prof_enable(c, False)
            pn, pe = (ops.prof_read(c) for c in classes)
            us = (pn["ms"] + pe["ms"]) * 1e3 / reps
            gbs = by / us / 1e3
            own_gbs = (pn["bytes"] + pe["bytes"]) / ((pn["ms"] + pe["ms"]) * 1e-3) / 1e9
            out[f"factored_{what}_d{d}"] = {
                "own_achieved": round(own_gbs, 1), "own_frac": round(own_gbs / HBM_PEAK_GBS, 4),
                "equiv_achieved": round(gbs, 1), "equiv_frac": round(gbs / HBM_PEAK_GBS, 4),
                "us": round(us, 1),
                "stage1_node": {"us": round(pn["ms"] * 1e3 / reps, 1),
                                "own_frac": round(pn["bytes"] / (pn["ms"] * 1e-3) / 1e9
                                                  / HBM_PEAK_GBS, 4)},
                "stage2_edge": {"us": round(pe["ms"] * 1e3 / reps, 1),
                                "own_frac": round(pe["bytes"] / (pe["ms"] * 1e-3) / 1e9
                                                  / HBM_PEAK_GBS, 4)}}
    return out


def isolated_poly_step(device, batch, reps=20, chain=20):
    """k_poly_step at the bench's own shape OUTSIDE the training step: a
    hipGraph chain of `chain` fused Laguerre steps (d = 64) over the batch's L0
    and L1, kernel-stamped -- what the kernel does with the GPU to itself,
    next to the in-context figure (where the node and edge chains share it)."""
    import hlhgat
    from hlhgat import ops
    tot_b = tot_ms = 0.0
    launches = 0
    for ei, w, n in ((batch.edge_index_t, batch.edge_weight_t, batch.x_t.shape[0]),
                     (batch.edge_index_s, batch.edge_weight_s, batch.x_s.shape[0])):
        A = ops.hodge_operator(ei, w, n).fwd
        X, Z, Y = (torch.randn(n, 64, device=device) for _ in range(3))

        def run():
            for _ in range(chain):
                ops._poly_step(A, X, Y, Z=Z, alpha=-1.0, beta=3.0, gamma=-1.0, div=2.0)
        run()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run()
        torch.cuda.current_stream().wait_stream(s)
        g.replay()
        torch.cuda.synchronize()
        # stamps do not survive capture: time the replays with events instead
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        e1.synchronize()
        tot_ms += e0.elapsed_time(e1)
        launches += reps * chain
        tot_b += reps * chain * (8.0 * A.nnz + 4.0 * (n + 1) + 12.0 * n * 64)
    gbs = tot_b / (tot_ms * 1e-3) / 1e9
    return {"achieved": round(gbs, 1), "frac": round(gbs / HBM_PEAK_GBS, 4),
            "avg_launch_us": round(tot_ms * 1e3 / launches, 2),
            "measured": "hipGraph chain of 20 fused Laguerre steps (d=64) on this batch's L0 "
                        "and L1, replayed 20x, events around the replays"}


def _site(p, steps):
    """one call site's census entry: per step launches, time and bytes"""
    n = max(p["launches"], 1)
    return {"launches_per_step": round(p["launches"] / steps, 1),
            "us_per_step": round(p["ms"] * 1e3 / steps, 1),
            "bytes_per_step": round(p["bytes"] / steps),
            "avg_launch_us": round(p["ms"] * 1e3 / n, 2),
            "gbs": round(p["bytes"] / (p["ms"] * 1e-3) / 1e9, 1) if p["ms"] > 0 else None}


def kernel_roofline(p, bound, note):
    """roofline entry of one event-stamped kernel class (hlhgat_prof_read)"""
    if not p["launches"] or p["ms"] <= 0:
        return None
    sec = p["ms"] * 1e-3
    if bound == "mfma":
        ach, peak, unit = p["flops"] / sec / 1e12, FP32_MFMA_PEAK_TFS, "TFLOP/s"
    else:
        ach, peak, unit = p["bytes"] / sec / 1e9, HBM_PEAK_GBS, "GB/s"
    return {"bound": bound, "achieved": round(ach, 2), "peak": peak, "unit": unit,
            "frac": round(ach / peak, 4), "launches": p["launches"],
            "avg_launch_us": round(p["ms"] * 1e3 / p["launches"], 2),
            "per_launch": round((p["flops"] if bound == "mfma" else p["bytes"]) / p["launches"]),
            "what": note}


# BASELINE configs[2..4] heads: per-GPU batch, model, loss
HEADS = {
    "cfg3_cifar_attpool": dict(kind="cifar", graphs=256, cls="HL_HGCNN_CIFAR10SP_dense_int3_attpool",
                               ref="RefCifarAttPool", cpu_graphs=32,
                               kw=dict(channels=[2, 2, 2], filters=[64, 128, 256],
                                       mlp_channels=[256], K=4, keig=10, pool_loc=1, l=0.5)),
    "cfg4_pepfunc_attpool": dict(kind="peptides", graphs=64, cls="HL_HGCNN_pepfunc_dense_int3_attpool",
                                 ref="RefPepfuncAttPool", cpu_graphs=16,
                                 kw=dict(channels=[2, 2, 2], filters=[64, 128, 256],
                                         mlp_channels=[256], K=6, pool_loc=1)),
    "cfg5_tsp_pyr": dict(kind="tsp", graphs=4, cls="HL_HGCNN_TSP_dense_int3_pyr",
                         ref="RefTSPModel", cpu_graphs=1,
                         kw=dict(channels=[4, 4, 4], filters=[32, 64, 128], mlp_channels=[256],
                                 K=4)),
}


def _head_pool(kind, n, seed=0):
    """A pool of n host graphs (PairData, or MLGC level pairs for the attpool
    heads) of the head's generator; batches are drawn from it."""
    from hlhgat.synthetic import cifar_like_graphs, peptides_like_graphs, tsp_like_graph
    if kind == "tsp":
        return [tsp_like_graph(seed * 1000 + i) for i in range(n)]
    make = {"cifar": cifar_like_graphs, "peptides": peptides_like_graphs}[kind]
    return [make(seed * 1_000_003 + i) for i in range(n)]


def _head_collate(kind, items):
    from hlhgat.hodge_dataset import collate, pool_tables
    if kind == "tsp":
        return collate(items, check_hodge=False)
    datas = [collate([p[0] for p in items], check_hodge=False),
             collate([p[1] for p in items], check_hodge=False)]
    if os.environ.get("HLHGAT_POOL_TABLES", "1") != "0":  # A/B: 0 = sorted in the step
        pool_tables(datas)  # the MLGC cluster CSR, once per batch (not in every step)
    return datas


def _head_batch(kind, graphs, seed):
    """One unpadded batch of `graphs` fresh graphs (the CPU-oracle sample)."""
    return _head_collate(kind, _head_pool(kind, graphs, seed))


def _head_loss(kind, out, datas):
    import hlhgat
    F = torch.nn.functional
    if kind == "tsp":  # main_TSP...:316-321 (BCE on the masked edge logits), mean over
        # the batch's real edges (padding edges carry a zero mask and label)
        return F.binary_cross_entropy_with_logits(
            out[0].view(-1), datas.y.view(-1).float(), reduction="sum") / datas.num_edge1.sum()
    y = datas[0].y
    if kind == "cifar":  # main_cifar10SP: cross entropy
        return F.cross_entropy(out, y.view(-1).long())
    # pepfunc; hlhgat.nn.BCEWithLogitsLoss: torch's module, one HIP launch each way
    return hlhgat.nn.BCEWithLogitsLoss()(out, y.view(out.shape).float())


HEAD_PROF = (("k_poly_step (all call sites)", POLY_CLASSES, "hbm"),
             *((f"k_poly_step: {nm}", c, "hbm") for nm, c in POLY_SITES),
             ("k_edge_gather2 (edge rows gathering their two node rows)", "PROF_GATHER2", "hbm"),
             ("hodge_node (factored L1, B1 X)",
             "PROF_HODGE_NODE", "hbm"), ("hodge_edge (factored L1 edge step)", "PROF_HODGE_EDGE",
             "hbm"), ("k_proj_fwd", "PROF_PROJ", "mfma"), ("k_proj_bn_fwd", "PROF_PROJ_BN", "mfma"),
             ("k_proj_bwd_fused", "PROF_PROJ_BWD",
             "mfma"), ("k_bn_fwd_grid", "PROF_BN_FWD", "hbm"), ("k_bn_bwd_reduce",
             "PROF_BN_BWD", "hbm"))


def _guarded(name, fn, *a):
    """A secondary leg (configs 3-5) that raises leaves its error in the JSON
    line instead of taking the headline figure with it (logged with its
    traceback on stderr)."""
    import traceback
    try:
        return fn(*a)
    except Exception as e:  # noqa: BLE001
        traceback.print_exc()
        log(f"[rank 0] {name} leg FAILED: {e!r}")
        return {"error": repr(e)[:400]}


# CUs the config-3 producer's stream may use (hipExtStreamCreateWithCUMask via
# hlhgat_stream_create); 0 = an unmasked stream of its own
PRODUCER_CUS = int(os.environ.get("HLHGAT_PRODUCER_CUS", "0"))
# the producer stream's HIP priority: "low" (the device's least priority),
# "high", or "0" (default)
PRODUCER_PRIO = os.environ.get("HLHGAT_PRODUCER_PRIO", "0")


def cifar_pipeline_leg(device, c, G, n_batches=8, producer_cus=None, producer_prio=None):
    """Config 3 WITH the reference's per-sample work (its Dataset.get() runs
    every epoch in num_workers DataLoader processes beside training,
    main_cifar10SP...:67-125,214): hlhgat.pipeline.SuperpixelPipeline builds
    each 256-graph batch from raw superpixel samples (dropout_edge
    augmentation, device Hodge builder + lambda_max, batched eigh PE, native
    batched MLGC, both levels on the device) on a producer thread and its own
    stream, pads both levels to one capacity bucket (pad_levels on the
    device), and hands it over; the training step replays ONE captured graph
    for every batch (TrainStep) while the next batch is built.
    Reported: the overlapped rate, and the pipeline alone / the serial sum.
    The producer's stream runs on `producer_cus` CUs only (a CU-masked stream,
    the highest-numbered CUs), so the step's kernels keep the rest of the chip
    and its one-launch BatchNorm grids (<= half the chip's capacity) fit
    beside it; 0 = unmasked."""
    import queue
    import threading
    import hlhgat
    from hlhgat.hodge_dataset import level_caps, pad_levels
    from hlhgat.pipeline import SuperpixelPipeline, superpixel_raw
    from hlhgat.train import TrainStep
    raw = [superpixel_raw(5000 + i) for i in range(n_batches * G)]
    pipe = SuperpixelPipeline(raw, keig=c["kw"]["keig"] + 1, aug=True)

    # the capacity bucket: the levels of every batch the timed run will build
    # (augmentation is seeded, so the pre-pass sees the same shapes); a
    # loader would take the dataset's bucket.  A capture is never made while
    # the producer thread runs (a global-mode capture refuses other threads'
    # allocations), so every timed step must replay.
    caps = level_caps([pipe.batch(range(b * G, (b + 1) * G), seed=b, device=device)
                       for b in range(n_batches)], 512)

    def fit(datas):
        return pad_levels(datas, caps)

    torch.manual_seed(0)
    m = getattr(hlhgat, c["cls"])(**c["kw"]).to(device).train()
    st = TrainStep(m, lambda o, d: _head_loss("cifar", o, d), lr=1e-3, graphs=True)
    main = torch.cuda.current_stream(device)

    from hlhgat import ops
    cus = PRODUCER_CUS if producer_cus is None else int(producer_cus)
    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    cus = min(max(cus, 0), n_cu)
    mask = ops.cu_mask_high(cus, n_cu) if 0 < cus < n_cu else None
    pr = PRODUCER_PRIO if producer_prio is None else str(producer_prio)
    least, greatest = torch.cuda.Stream.priority_range()
    prio = {"low": least, "high": greatest}.get(pr, 0) if mask is None else 0
    # a stream of the library's own (never one of torch's round-robin pool)
    s = ops.own_stream(device, f"producer{cus if mask else ''}p{prio}", cu_mask=mask,
                       priority=prio)

    def produce(q, seeds):
        with torch.cuda.stream(s):
            for k, b in enumerate(seeds):
                datas = fit(pipe.batch(range(b * G, (b + 1) * G), seed=b, device=device))
                for lv in datas:  # consumed on the main stream (the step's copy-in)
                    for v in vars(lv).values():
                        if torch.is_tensor(v) and v.is_cuda:
                            v.record_stream(main)
                ev = torch.cuda.Event()
                ev.record(s)
                q.put((datas, ev))
        q.put(None)

    def run(seeds):
        q = queue.Queue(maxsize=2)
        th = threading.Thread(target=produce, args=(q, seeds), daemon=True)
        th.start()
        n = 0
        while True:
            it = q.get()
            if it is None:
                break
            datas, ev = it
            main.wait_event(ev)
            st(datas)
            n += 1
        th.join()
        return n
    for b in (0, 1):  # warm-up, serial: the eager step + capture of the bucket, a replay
        st(fit(pipe.batch(range(b * G, (b + 1) * G), seed=b, device=device)))
    torch.cuda.synchronize()
    n_cap = st.stats["captures"]
    h0 = ops.bn_giveups()["count"]
    t0 = time.perf_counter()
    nb = run(list(range(n_batches)))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    handovers = ops.bn_giveups()["count"] - h0
    assert st.stats["captures"] == n_cap, "a timed batch left the capacity bucket"
    # the replayed step alone, same graph and batch buffers (no producer)
    last = fit(pipe.batch(range(0, G), seed=0, device=device))
    st(last)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(n_batches):
        st(last)
    torch.cuda.synchronize()
    t_step = (time.perf_counter() - t2) / n_batches
    # the pipeline alone (same producer, no training)
    t1 = time.perf_counter()
    for b in range(n_batches):
        fit(pipe.batch(range(b * G, (b + 1) * G), seed=b, device=device))
    torch.cuda.synchronize()
    t_pipe = time.perf_counter() - t1
    return {"value": round(nb * G / dt, 1), "unit": "graphs/s",
            "ms_per_batch": round(dt / nb * 1e3, 2),
            "step_alone_ms": round(t_step * 1e3, 2),
            "ratio_to_step": round((dt / nb) / t_step, 3),
            "producer_cus": cus if mask else n_cu, "producer_priority": prio,
            "bn_handovers": handovers,
            "pipeline_graphs_per_s": round(n_batches * G / t_pipe, 1),
            "pipeline_ms_per_batch": round(t_pipe / n_batches * 1e3, 1),
            "captures": st.stats["captures"], "replays": st.stats["replay"],
            "caps": caps,
            "what": "raw superpixel samples -> SuperpixelPipeline (dropout_edge, device Hodge "
                    "builder, batched eigh PE, native batched MLGC) on a producer thread + its "
                    "own stream, padded to one capacity bucket -> replayed training step, "
                    "overlapped; batches of " + str(G)}


def heads_leg(device, steps=8, warmup=2, n_batches=8, cpu_budget_s=8.0):
    """BASELINE configs[2..4] on this GPU: graphs/s of a full training step
    (fwd + loss + bwd + Adam) at the per-GPU batch of SURVEY §8d.  n_batches
    DISTINCT batches (random draws from a pool of graphs) padded to ONE
    capacity bucket (hodge_dataset.pad_levels / pad_batch), so
    hlhgat.train.TrainStep captures one hipGraph and replays it for every
    batch -- as a loader padding to the dataset's bucket would; the eager
    step beside it.  Per head: the padding overhead, a kernel roofline
    breakdown from an event-stamped eager step, and the CPU oracle (the same
    head restated in oracle/hodge_ref.py) on a bounded sample."""
    import numpy as np
    import hlhgat
    from hlhgat import ops
    from hlhgat.hodge_dataset import level_caps, pad_batch, pad_levels, static_caps
    from hlhgat.train import TrainStep
    from oracle import hodge_ref as R
    L = hlhgat._lib
    out = {}
    cores = int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or os.cpu_count()
    for name, c in HEADS.items():
        kind, G = c["kind"], c["graphs"]
        handovers0 = ops.bn_giveups()["count"]
        t0 = time.perf_counter()
        pool = _head_pool(kind, 2 * G)
        rng = np.random.RandomState(7)
        raw = [_head_collate(kind, [pool[i] for i in rng.choice(len(pool), G, replace=False)])
               for _ in range(n_batches)]
        if kind == "tsp":
            cs = [static_caps(b, 512) for b in raw]
            caps = {k: max(x[k] for x in cs) for k in cs[0]}
            padded = [pad_batch(b, caps) for b in raw]
            rows = lambda b: b.x_t.size(0) + b.x_s.size(0)  # noqa: E731
        else:
            caps = level_caps(raw, 512)
            padded = [pad_levels(b, caps) for b in raw]
            rows = lambda bl: sum(b.x_t.size(0) + b.x_s.size(0) for b in bl)  # noqa: E731
        overhead = sum(rows(p) for p in padded) / sum(rows(b) for b in raw) - 1
        gen_s = time.perf_counter() - t0
        dev = lambda b: b.to(device) if kind == "tsp" else [x.to(device) for x in b]  # noqa: E731
        batches = [dev(b) for b in padded]
        dts, stats = {}, {}
        for graphs in (False, True):
            torch.manual_seed(0)
            m = getattr(hlhgat, c["cls"])(**c["kw"]).to(device).train()
            st = TrainStep(m, lambda o, d, k=kind: _head_loss(k, o, d), lr=1e-3, graphs=graphs)
            for i in range(warmup):  # graphs: one eager step + the capture
                st(batches[i % n_batches])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(steps):
                st(batches[(warmup + i) % n_batches])
            torch.cuda.synchronize()
            dts[graphs] = (time.perf_counter() - t1) / steps
            stats[graphs] = dict(st.stats)
            if graphs:
                assert st.stats["captures"] == 1 and \
                    st.stats["replay"] == steps + warmup - 1, st.stats
                # kernel breakdown: one event-stamped eager step of the same model
                ops.prof_reset()
                prof_enable_all(L, [cls for _, cls, _ in HEAD_PROF], True)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                st._eager(batches[0])
                torch.cuda.synchronize()
                eager_ms = (time.perf_counter() - t2) * 1e3
                prof_enable_all(L, [cls for _, cls, _ in HEAD_PROF], False)
                brk = {}
                for nm, cls, bound in HEAD_PROF:
                    kr = kernel_roofline(prof_sum(L, cls), bound, "")
                    if kr:
                        kr.pop("what")
                        kr["ms_per_step"] = round(kr["avg_launch_us"] * kr["launches"] / 1e3, 3)
                        brk[nm] = kr
            del m, st
        dt = dts[True]
        r = {"value": round(G / dt, 1), "unit": "graphs/s", "ms_per_step": round(dt * 1e3, 2),
             "graphs_per_step": G, "steps": steps, "head": c["cls"], "model": c["kw"],
             "step": f"fwd + loss + bwd + Adam; {n_batches} distinct batches padded to one "
                     f"capacity bucket, ONE captured hipGraph replayed for all of them",
             "captures": stats[True]["captures"], "padding_overhead": round(overhead, 4),
             "caps": caps,
             "eager_ms_per_step": round(dts[False] * 1e3, 2),
             "eager_value": round(G / dts[False], 1), "data_gen_s": round(gen_s, 1),
             "kernels_eager_step": {"ms": round(eager_ms, 2), "classes": brk}}
        # CPU oracle on a bounded sample: cpu_graphs fresh graphs
        torch.set_num_threads(cores)
        sb = _head_batch(kind, c["cpu_graphs"], 0)
        torch.manual_seed(0)
        mr = getattr(R, c["ref"])(**c["kw"]).train()
        opt = torch.optim.Adam(mr.parameters(), lr=1e-3)

        def cpu_step():
            o = mr(sb)
            _head_loss(kind, o, sb).backward()
            opt.step()
            opt.zero_grad()
        times, t_start = [], time.perf_counter()
        cpu_step()  # warm-up
        while len(times) < 1 or (time.perf_counter() - t_start < cpu_budget_s and len(times) < 10):
            t1 = time.perf_counter()
            cpu_step()
            times.append(time.perf_counter() - t1)
        times.sort()
        med = times[len(times) // 2]
        r["cpu_baseline"] = {"value": round(c["cpu_graphs"] / med, 4), "unit": "graphs/s",
                             "cores": cores, "kind": "port",
                             "sample": f"{len(times)} oracle training steps on {c['cpu_graphs']} "
                                       f"graph(s) of the same generator, median {med * 1e3:.0f} ms"}
        if kind == "cifar":
            r["with_per_sample_work"] = _guarded("cifar pipeline", cifar_pipeline_leg,
                                                 device, c, G)
        # one-launch BatchNorm workgroups that handed over in this head's legs
        r["bn_handovers"] = ops.bn_giveups()["count"] - handovers0
        out[name] = r
        log(f"[heads] {name}: {r['value']} graphs/s replayed, {r['eager_value']} eager, "
            f"padding {overhead:.1%} (CPU oracle {r['cpu_baseline']['value']})")
        del batches
        torch.cuda.empty_cache()
    return out


DUMP_BYTES = 64 * 10**6  # --dump-outputs: at most this much in all


def dump_outputs(path, step, loss):
    """`--dump-outputs DIR`: what the last timed step handed its caller, one
    float32 `DIR/<name>.npy` each -- `loss` (the value TrainStep returned) and
    the training state the step left: `params` and `grads` (TrainStep's flat
    parameter and gradient buckets, in model.parameters() order), the Adam
    moments, and `buffers` (the module's floating-point buffers, the BatchNorm
    running statistics, concatenated in named_buffers() order).  An array that
    would take the dump past DUMP_BYTES is cut to a fixed, seeded sample of
    its elements (ascending indices)."""
    import numpy as np
    if step.device.type == "cuda":
        torch.cuda.synchronize()
    out = {"loss": loss.detach().reshape(-1), "params": step.flat, "grads": step.flat_grad}
    state = step.opt.state.get(step.master, {})
    for k in ("exp_avg", "exp_avg_sq"):
        if torch.is_tensor(state.get(k)):
            out["adam_" + k] = state[k]
    bufs = [b.detach().reshape(-1).float() for _, b in step.model.named_buffers()
            if b.is_floating_point()]
    if bufs:
        out["buffers"] = torch.cat(bufs)
    os.makedirs(path, exist_ok=True)
    room = DUMP_BYTES // (4 * len(out))  # elements per array
    for name, t in out.items():
        a = t.detach().reshape(-1).float().cpu().numpy()
        if a.size > room:
            a = a[np.sort(np.random.RandomState(0).choice(a.size, room, replace=False))]
        np.save(os.path.join(path, name + ".npy"), a)
    log(f"[rank 0] outputs of the last timed step written to {path}: {', '.join(out)}")


WORKLOADS = {"cfg2": None, "cfg3": "cfg3_cifar_attpool", "cfg4": "cfg4_pepfunc_attpool",
             "cfg5": "cfg5_tsp_pyr"}


def head_workload(args, rank, world, device):
    """`--workload cfg3|cfg4|cfg5`: the BASELINE configs[2..4] head as the
    bench's measured step on `world` GPUs, sharded by graph (each rank trains
    its own per-GPU batch of the head's size, weak scaling) through TrainStep:
    captured hipGraph per rank, one-bucket gradient all-reduce over RCCL, HIP
    Adam -- the reference's per-step loop (main_pepfunc...:171-199,
    main_TSP...:357-441) on device-resident batches.  Barrier + synchronise
    around exactly `steps` steps, max over ranks, one JSON line from rank 0."""
    import numpy as np
    import hlhgat
    from hlhgat.distributed import max_over_ranks
    from hlhgat.hodge_dataset import level_caps, pad_batch, pad_levels, static_caps
    from hlhgat.train import TrainStep
    name = WORKLOADS[args.workload]
    c = HEADS[name]
    kind, G = c["kind"], c["graphs"]
    log(f"[rank {rank}] {name}: generating {args.batches} x {G} synthetic graphs")
    pool = _head_pool(kind, 2 * G, seed=rank)  # each rank its own shard of graphs
    rng = np.random.RandomState(7 + rank)
    raw = [_head_collate(kind, [pool[i] for i in rng.choice(len(pool), G, replace=False)])
           for _ in range(args.batches)]
    if kind == "tsp":
        cs = [static_caps(b, 512) for b in raw]
        caps = {k: max(x[k] for x in cs) for k in cs[0]}
    else:
        caps = level_caps(raw, 512)
    if world > 1:
        # one capacity bucket on every rank, the largest of any rank: the same
        # step shape everywhere (padding rows are inert)
        dicts = [caps] if kind == "tsp" else caps
        flat = [(i, k) for i, d in enumerate(dicts) for k in sorted(d)]
        t = torch.tensor([dicts[i][k] for i, k in flat], dtype=torch.int64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        for (i, k), v in zip(flat, t.tolist()):
            dicts[i][k] = int(v)
    if kind == "tsp":
        padded = [pad_batch(b, caps).to(device) for b in raw]
    else:
        padded = [[x.to(device) for x in pad_levels(b, caps)] for b in raw]
    torch.manual_seed(0)
    m = getattr(hlhgat, c["cls"])(**c["kw"]).to(device).train()
    step = TrainStep(m, lambda o, d, k=kind: _head_loss(k, o, d), lr=1e-3,
                     graphs=not args.eager)
    for i in range(args.warmup):
        step(padded[i % len(padded)])
    torch.cuda.synchronize()
    log(f"[rank {rank}] warmup done {step.stats} graphs_off={step.graphs_off}")
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        loss = step(padded[i % len(padded)])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, device)
    hlhgat.ops.check_device_errors()
    if rank == 0 and args.dump_outputs and loss is not None:
        dump_outputs(args.dump_outputs, step, loss)
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        print(json.dumps({
            "metric": f"graphs/sec HL-HGAT fwd+bwd, {name} head, 1/2/4/8 MI355X",
            "value": round(world * G * args.steps / elapsed, 1), "unit": "graphs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "fp32",
            "data": "synthetic simplex graphs of the config's shape (random-init weights)",
            "config": {"workload": f"BASELINE {name}: {c['cls']} {c['kw']}", "graphs_per_gpu": G,
                       "global_batch": world * G, "parallelism": f"dp{world}",
                       "execution": "eager" if args.eager else
                       f"captured hipGraph per rank ({step.stats.get('captures')} capture(s)), "
                       f"replayed, "
                       f"gradient all-reduce over {'RCCL' if world > 1 else 'none'}",
                       "caps": caps},
            "stats": {k: v for k, v in step.stats.items()}}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def eval_leg(model, batches, steps=20):
    """The reference's evaluation loop body (main_zinc...:165-177: model.eval(),
    out = model(data) under torch.no_grad(), per batch) on the timed workload's
    device-resident batches: hlhgat.train.InferStep replays one captured eval
    forward per batch shape; the eager forward beside it."""
    from hlhgat.train import InferStep
    out = {}
    for graphs in (False, True):
        inf = InferStep(model, graphs=graphs)
        for i in range(3):
            inf(batches[i % len(batches)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            inf(batches[i % len(batches)])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        out["replayed" if graphs else "eager"] = {
            "value": round(GRAPHS_PER_GPU / dt, 1), "unit": "graphs/s",
            "ms_per_batch": round(dt * 1e3, 3), "stats": dict(inf.stats)}
    out["what"] = ("model.eval() + torch.no_grad() forward of the timed workload's padded "
                   "1000-graph batches (BatchNorm on running statistics)")
    return out


def h2d_leg(batch_cpu, device, reps=10):
    """The reference's loop copies each batch to the device every step
    (data.to(device)); bench.py's `value` excludes it (inputs resident in
    HBM).  Here: the PCIe time of one padded 1000-graph batch from pinned host
    memory, and the step rate if that copy were serialised with every step."""
    from hlhgat.train import _tensor_items
    items = [(k, v.pin_memory()) for k, v in _tensor_items(batch_cpu)]
    nbytes = sum(v.numel() * v.element_size() for _, v in items)
    for _ in range(2):
        [v.to(device, non_blocking=True) for _, v in items]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        [v.to(device, non_blocking=True) for _, v in items]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    return {"ms_per_batch": round(ms, 3), "bytes": nbytes, "GBps": round(nbytes / ms / 1e6, 1)}


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_ranks(n: int, argv) -> int:
    """Start n ranks of this script under torch.distributed.run (one process
    per GPU, rendezvous on 127.0.0.1) and wait for them.  The parent makes no
    GPU call (it never even initialises HIP), so the children own the
    devices; rank 0's JSON line reaches our stdout through the inherited
    file descriptors.  Returns the launcher's exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={n}", "--master-addr=127.0.0.1",
           f"--master-port={_free_port()}", os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC for RCCL on this host driver
    log(f"[launcher] starting {n} ranks: {' '.join(cmd)}")
    return subprocess.call(cmd, env=env)


def dry_run(args):
    """The multi-rank contract without a GPU: gloo rendezvous, world-size
    check, barrier + timed trivial steps (an all-reduce of a 2.6 MB gradient-
    sized buffer, the size of cfg2's bucket) + max over ranks, one JSON line
    from rank 0 with the bench's keys."""
    from hlhgat.distributed import init_distributed, max_over_ranks
    rank, world, device = init_distributed("gloo")
    if world != args.gpus:
        raise SystemExit(f"bench.py: world size {world} != --gpus {args.gpus}")
    n_par = 650_000  # cfg2's gradient bucket
    if args.workload != "cfg2":  # the head's own bucket (model built on the CPU)
        import hlhgat
        c = HEADS[WORKLOADS[args.workload]]
        n_par = sum(p.numel() for p in getattr(hlhgat, c["cls"])(**c["kw"]).parameters())
    buf = torch.ones(n_par)
    for _ in range(args.warmup):
        if world > 1:
            dist.all_reduce(buf)
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if world > 1:
            dist.all_reduce(buf)
    if world > 1:
        dist.barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0, device)
    if rank == 0:
        print(json.dumps({"metric": METRIC, "value": None, "unit": "graphs/s", "n_gpus": world,
                          "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 3),
                          "dry_run": True, "backend": dist.get_backend() if world > 1 else None,
                          "ranks_seen": world, "workload": args.workload,
                          "bucket_floats": n_par}), flush=True)
    if world > 1:
        dist.destroy_process_group()


METRIC = "graphs/sec HL-HGAT fwd+bwd, ZINC-12k simplex graphs, 1/2/4/8 MI355X"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's results (loss, parameters, gradients, "
                         "Adam moments, BatchNorm buffers) as DIR/<name>.npy, float32")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run every other leg (parity check, "
                         "rooflines, config-5 SpMM, H2D, eval, loader, CPU baseline, configs "
                         "3-5 heads); the --no-* options below drop single legs of it")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--loader-workers", type=int, default=4,
                    help="GraphLoader collation threads (the reference's num_workers=4)")
    ap.add_argument("--loader-per-epoch", action="store_true",
                    help="iterate the loader epoch by epoch instead of GraphLoader.stream")
    ap.add_argument("--loader-depth", type=int, default=2,
                    help="batches StagedFeed uploads ahead of the step (loader leg)")
    ap.add_argument("--loader-slots", type=int, default=None,
                    help="captured graphs per shape the loader leg stages into (default depth + 2)")
    ap.add_argument("--loader-inline", action="store_true",
                    help="stage the loader leg's batches from the training thread (no feeder thread)")
    ap.add_argument("--loader-priority", type=int, default=0,
                    help="priority of the loader leg's copy stream (torch: -1 = high)")
    ap.add_argument("--loader-switch-ms", type=float, default=None,
                    help="Python GIL switch interval during the loader-fed loop (ms)")
    ap.add_argument("--no-loader", action="store_true",
                    help="skip the data-loader leg (native collate rates, loader-fed steps)")
    ap.add_argument("--no-parity-check", action="store_true",
                    help="skip the full-size first-step forward check against the oracle")
    ap.add_argument("--eager", action="store_true", help="no hipGraph replay")
    ap.add_argument("--no-cfg5", action="store_true",
                    help="skip the config-5 (TSP) SpMM roofline measurement")
    ap.add_argument("--no-heads", action="store_true",
                    help="skip the configs 3-5 heads (graphs/s + CPU oracle baseline each)")
    ap.add_argument("--prof-steps", type=int, default=3,
                    help="eager steps with kernel event stamps for the roofline")
    ap.add_argument("--replay-probe", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-replay-census", action="store_true",
                    help="rooflines from the eager stamped pass only (no rocprofv3 child)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / timing contract on gloo + CPU, no model")
    ap.add_argument("--workload", default="cfg2", choices=sorted(WORKLOADS),
                    help="cfg2 (default): BASELINE configs[1], the ZINC model, the headline; "
                         "cfg3 / cfg4 / cfg5: the configs[2..4] head as the measured step "
                         "(sharded by graph over --gpus ranks)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("bench.py: --gpus must be >= 1")
    if args.gpus > 1 and "RANK" not in os.environ:
        # not under torchrun: start the N ranks ourselves, before any GPU call
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    if args.dry_run:
        return dry_run(args)
    if args.replay_probe:
        return replay_probe(args)  # under the profiler: no worker processes to trace
    global GEN_PROCS  # CPU workers for the synthetic graphs, shared between the ranks
    if not any(k.startswith("ROCPROF") for k in os.environ):  # (rocprofv3 would trace them too)
        GEN_PROCS = max(1, min(12, os.cpu_count() or 1) // args.gpus)

    from hlhgat.distributed import init_distributed, max_over_ranks
    rank, world, device = init_distributed("nccl")  # RCCL over xGMI; one process per GPU
    if world != args.gpus:
        raise SystemExit(f"bench.py: world size {world} != --gpus {args.gpus} "
                         f"(launch with --nproc-per-node {args.gpus}, or without torchrun)")
    if args.workload != "cfg2":
        return head_workload(args, rank, world, device)

    import hlhgat
    from hlhgat import ops
    from hlhgat.train import TrainStep

    log(f"[rank {rank}] generating {args.batches} x {GRAPHS_PER_GPU} synthetic graphs")
    batches, caps, real_rows, raw0, dataset = make_batches(args.batches, rank, device)  # per rank
    torch.manual_seed(0)
    model = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**MODEL_KW).to(device).train()
    pcheck = None
    if rank == 0 and args.full and not args.no_parity_check:
        pcheck = parity_check(model, batches[0], raw0)
        log(f"[rank 0] parity check vs oracle (1000 graphs): {pcheck['max_rel_err']:.2e}")
    crit = hlhgat.nn.L1Loss()  # torch.nn.L1Loss, one HIP launch each way

    def loss_fn(out, b):
        return crit(out.view(-1, 1), b.y.view(-1, 1))

    # flat params + one-bucket gradient all-reduce (the only exchange step)
    step = TrainStep(model, loss_fn, lr=1e-3, weight_decay=1e-3, graphs=not args.eager)

    for i in range(args.warmup):
        step(batches[i % len(batches)])
    torch.cuda.synchronize()
    log(f"[rank {rank}] warmup done {step.stats}")

    ops.bn_giveups_reset()  # synchronises: before the timed region
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loss = None
    for i in range(args.steps):
        loss = step(batches[i % len(batches)])
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    elapsed = max_over_ranks(elapsed, device)
    ops.check_device_errors()  # a kernel that reported unusable results voids the run
    giveups_timed = ops.bn_giveups()["count"]
    if rank == 0 and args.dump_outputs and loss is not None:
        dump_outputs(args.dump_outputs, step, loss)  # before any later leg trains on

    ms_step = elapsed / args.steps * 1e3
    value = world * GRAPHS_PER_GPU * args.steps / elapsed
    result = {
        "metric": METRIC,
        "value": round(value, 1), "unit": "graphs/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "fp32",
        "data": "synthetic ZINC-like simplex graphs (random-init weights; no dataset offline)",
        "config": {"workload": "BASELINE configs[1]: ZINC-12k-scale, HL_HGCNN_zinc_dense_int3_pyr "
                               "channels=[2,2,2] filters=[64,64,64] K=3 mlp=[256,256] keig=15; "
                               "step = copy of the device-resident batch into the step's "
                               "static buffers + fwd + L1 + bwd (+ grad all-reduce) + Adam; "
                               "the batch tables (Laplacian / incidence CSRs, degrees, "
                               "segment offsets) are built by the data loader at collate "
                               "time, outside the step (see loader)",
                   "execution": "eager" if args.eager else
                   f"one hipGraph for the capacity bucket (captured in warmup, "
                   f"{step.stats['captures']} capture(s)), replayed for {args.batches} distinct "
                   f"batches padded to it; node/edge chains on 2 streams",
                   "static_caps": caps,
                   "padding_overhead": round((caps["rows_t"] + caps["rows_s"]) / real_rows - 1, 4),
                   "graphs_per_gpu": GRAPHS_PER_GPU, "global_batch": world * GRAPHS_PER_GPU,
                   "parallelism": f"dp{world}"},
    }
    if not args.full:
        # the plain run: the headline figure alone (every other leg: --full)
        if rank == 0:
            result["bn_barrier"] = {"giveups_timed_region": giveups_timed, "wait_us": 1000}
            print(json.dumps(result), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return

    # roofline pass: eager steps, SpMM / projection / BatchNorm launches event-stamped
    L = hlhgat._lib
    classes = (*POLY_CLASSES, "PROF_GATHER2", "PROF_PROJ", "PROF_PROJ_BWD", "PROF_PROJ_BN",
               "PROF_BN_FWD", "PROF_BN_BWD")
    ops.prof_reset()
    prof_enable_all(L, classes, True)
    for i in range(args.prof_steps):
        step._eager(batches[i % len(batches)])
    torch.cuda.synchronize()
    prof_enable_all(L, classes, False)
    ops.check_device_errors()

    poly = prof_sum(L, POLY_CLASSES)
    proj = ops.prof_read(L.PROF_PROJ)

    def gbs(p):
        return p["bytes"] / (p["ms"] * 1e-3) / 1e9 if p["ms"] > 0 else 0.0

    poly_gbs = gbs(poly)
    traffic, traffic_src = pmc_traffic("k_poly_step")
    roofline = {
        "kernel": "k_poly_step (CSR SpMM / fused Laguerre step over L0 and L1, fwd + adjoint, "
                  "and the NodeEdgeInt |B1| gathers)",
        "measured": f"hipExtLaunchKernel start/stop stamps, {args.prof_steps} eager steps after "
                    f"the timed region",
        "bound": "hbm", "achieved": round(poly_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(poly_gbs / HBM_PEAK_GBS, 4), "traffic": traffic,
        "traffic_source": traffic_src,
        "launches": poly["launches"],
        "avg_launch_us": round(poly["ms"] * 1e3 / max(poly["launches"], 1), 2),
        "algorithmic_bytes_per_launch": round(poly["bytes"] / max(poly["launches"], 1)),
        # per call site, per eager step: launches, time, algorithmic bytes
        "call_sites": {nm: _site(prof_sum(L, c), args.prof_steps) for nm, c in POLY_SITES},
    }
    result.update({
        "roofline": roofline,
        "cpu_baseline": None,
        "parity_check": pcheck,
        "rooflines": {k: kernel_roofline(ops.prof_read(c), bound, note) for k, c, bound, note in (
            ("k_proj_fwd", L.PROF_PROJ, "mfma",
             "projection forward (fp32 MFMA, W staged in LDS); flops 2 M N sum K"),
            ("k_proj_bwd_fused", L.PROF_PROJ_BWD, "mfma",
             "Linear backward: weight-gradient split partials + data gradient, one launch; "
             "flops 2 M N (sum K_w + sum K_d)"),
            ("k_proj_bn_fwd", L.PROF_PROJ_BN, "mfma",
             "projection + BatchNorm (+ReLU) forward in one launch; flops 2 M N sum K"),
            ("k_bn_fwd_grid", L.PROF_BN_FWD, "hbm",
             "BatchNorm forward (statistics + normalise, one launch); bytes 8 n C"),
            ("k_bn_bwd_reduce", L.PROF_BN_BWD, "hbm",
             "BatchNorm backward statistics; bytes 12 n C (x, dy, y)"),
            ("k_edge_gather2", L.PROF_GATHER2, "hbm",
             "edge rows gathering their two node rows (NodeEdgeInt x_t2s and the adjoint of "
             "x_s2t); bytes 16 E + 4 E d (2 gathered + out [+ z] [+ out read])"))},
        "spmm_cfg5": None,
        "heads": None,
        "eval": None,
        "h2d": None,
        "loader": None,
    })
    result_eager_rooflines = dict(result["rooflines"])
    if rank == 0:
        roofline["isolated"] = isolated_poly_step(device, batches[0])
    if rank == 0 and world == 1 and not args.eager and not args.no_replay_census:
        # rooflines of the REPLAYED step: kernel time per step from a rocprofv3
        # trace of the replayed workload, work per step from the stamped pass
        eager_work = {}
        for k, (_, cls, _) in REPLAY_CLASSES.items():
            p = prof_sum(L, cls)
            if p["launches"]:
                eager_work[k] = {"bytes": p["bytes"] / args.prof_steps,
                                 "flops": p["flops"] / args.prof_steps,
                                 "launches": p["launches"] / args.prof_steps}
        log("[rank 0] replay census (rocprofv3 child)")
        census, why = replay_census(caps, eager_work)
        if census is None:
            log(f"[rank 0] replay census unavailable: {why}")
            result["step_census"] = {"unavailable": why}
        else:
            kc = census.pop("kernels")
            result["step_census"] = census
            kp = kc.get("k_poly_step")
            if kp:
                eager_fig = {k: roofline[k] for k in ("achieved", "frac", "avg_launch_us",
                                                      "launches", "measured")}
                roofline.update(achieved=kp["achieved"], frac=kp["frac"],
                                avg_launch_us=kp["avg_launch_us"],
                                launches=kp["launches_per_step"],
                                algorithmic_bytes_per_launch=round(
                                    kp["work_per_step"] / kp["launches_per_step"]),
                                measured="kernel durations inside the replayed step "
                                         "(rocprofv3 --kernel-trace of the same workload, "
                                         f"{census['steps_traced']} replays), algorithmic "
                                         "bytes per step from the stamped eager pass")
                roofline["eager"] = eager_fig
            result["rooflines"] = {k: dict(v, what=(result["rooflines"].get(k) or {}).get(
                "what", "")) for k, v in kc.items() if k != "k_poly_step"}
            # the eager-stamped figures, kept apart: `roofline` / `rooflines`
            # (replayed-step durations) are the ones to quote
            result["diagnostics_eager_stamp"] = {k: v for k, v in result_eager_rooflines.items()}
    if rank == 0 and world == 1 and not args.no_cfg5:
        log("[rank 0] config-5 SpMM roofline")
        result["spmm_cfg5"] = cfg5_spmm(device)
    if rank == 0 and world == 1:
        import numpy as np
        h = h2d_leg(dataset.collate(np.arange(GRAPHS_PER_GPU), caps), device)
        h["value_if_serialised"] = round(GRAPHS_PER_GPU / (ms_step + h["ms_per_batch"]) * 1e3, 1)
        result["h2d"] = h
    if rank == 0 and world == 1:
        log("[rank 0] eval leg")
        h0 = ops.bn_giveups()["count"]
        result["eval"] = _guarded("eval", eval_leg, model, batches)
        result["eval"]["bn_handovers"] = ops.bn_giveups()["count"] - h0
    if rank == 0 and world == 1 and not args.no_loader:
        log("[rank 0] loader leg")
        h0 = ops.bn_giveups()["count"]
        result["loader"] = loader_leg(dataset, step, caps, device, ms_step,
                                      depth=args.loader_depth, workers=args.loader_workers,
                                      stream=not args.loader_per_epoch,
                                      priority=args.loader_priority,
                                      switch_ms=args.loader_switch_ms,
                                      slots=args.loader_slots,
                                      thread=not args.loader_inline)
        result["loader"]["bn_handovers"] = ops.bn_giveups()["count"] - h0
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        log("[rank 0] timing the CPU oracle baseline")
        result["cpu_baseline"] = cpu_baseline(raw0)
    if rank == 0 and world == 1 and not args.no_heads:
        log("[rank 0] configs 3-5 heads")
        torch.cuda.synchronize()
        ops.clear_device_errors()
        heads = _guarded("heads", heads_leg, device)
        result["heads"] = heads
    if rank == 0:
        # one-launch BatchNorm workgroups that handed their rows to the
        # finaliser over the whole process (correct results)
        gu = ops.bn_giveups()
        result["bn_barrier"] = {"giveups_timed_region": giveups_timed,
                                "giveups_since_timed_region": gu["count"],
                                "log": gu["log"][:8], "wait_us": 1000}
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
