"""Per-kernel timings of the hlhgat HIP ops at the BASELINE.json shapes.

    python tools/microbench.py [--quick] [--out gpurun_out/microbench.json]

Times each op with HIP events on the current stream (median of R reps after
warm-up) and reports algorithmic bytes / flops per launch (SURVEY.md §8d
formulas) against the MI355X peaks (HBM 8 TB/s, fp32 MFMA 157.3 TF/s).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "hl-hgat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM = 8000.0
MFMA = 157.3


def timeit(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


# [n, d] of the HL block outputs a live Dropout sees: config 2 (ZINC, 1000
# graphs), config 3 (CIFAR10SP, 256 graphs: nodes / edges at level 0) and
# config 5 (TSP, 4 graphs of 10k nodes)
DROPOUT_SHAPES = [("cfg2 nodes", 23259, 64), ("cfg2 edges", 24927, 64),
                  ("cfg3 nodes", 30208, 64), ("cfg3 edges", 143192, 64),
                  ("cfg5 nodes", 40000, 32), ("cfg5 edges", 206858, 32),
                  ("cfg5 edges", 206858, 128)]


def replayed(launch, reps, k=20):
    """us per launch with k launches captured into one hipGraph and replayed:
    the kernels back to back, without the host's per-call enqueue time.
    `launch` issues C-ABI launches only (no autograd, no allocation: an
    autograd backward inside a capture runs on the stream of its forward,
    which for a forward made before the capture is not the capturing stream)."""
    launch()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(k):
            launch()
    us, mn = timeit(g.replay, reps)
    return us / k, mn / k


def dropout_leg(rec, reps, dev):
    """Dropout forward and backward at p = 0.25, contiguous and into / out of
    a column block of a 4d-wide slab.  "replayed": the kernels alone (20
    hlhgat_dropout_fwd / _bwd launches captured and replayed); "eager call":
    one ops.dropout / autograd call with its host enqueue, ATen's beside it.
    GB/s against the 8 n d algorithmic bytes of one pass (read x, write y)."""
    from hlhgat import ops
    from hlhgat._lib import LIB, check
    F = torch.nn.functional
    ops.dropout_manual_seed(1)
    T, s = ops.dropout_params(0.25)
    state = ops._dropout_st(dev).dev
    snap = torch.zeros(2, dtype=torch.int64, device=dev)
    for tag, n, d in DROPOUT_SHAPES:
        by = 8.0 * n * d
        x = torch.randn(n, d, device=dev, requires_grad=True)
        xd = x.detach()
        g = torch.randn(n, d, device=dev)
        out = torch.empty(n, d, device=dev)
        slab = torch.randn(n, 4 * d, device=dev)
        col = slab[:, d:2 * d]

        def fwd(dst):
            check(LIB.hlhgat_dropout_fwd(xd.data_ptr(), d, n, d, T, s, state.data_ptr(), 0,
                                         snap.data_ptr(), dst.data_ptr(), dst.stride(0),
                                         ops._stream(xd)), "dropout_fwd")

        def bwd(src):
            check(LIB.hlhgat_dropout_bwd(src.data_ptr(), src.stride(0), n, d, T, s,
                                         snap.data_ptr(), 0, out.data_ptr(), d,
                                         ops._stream(xd)), "dropout_bwd")

        for name, launch in (("fwd", lambda: fwd(out)), ("fwd into slab", lambda: fwd(col)),
                             ("bwd", lambda: bwd(g)), ("bwd from slab", lambda: bwd(col))):
            us, mn = replayed(launch, reps)
            rec(f"dropout_{name} hip {tag} [{n},{d}] replayed x20", us, mn, by)
        y = ops.dropout(x, 0.25)
        yt = F.dropout(x, 0.25, True)
        for name, fn in (("fwd hip", lambda: ops.dropout(xd, 0.25)),
                         ("bwd hip", lambda: torch.autograd.grad(y, x, g, retain_graph=True)),
                         ("fwd torch", lambda: F.dropout(xd, 0.25, True)),
                         ("bwd torch", lambda: torch.autograd.grad(yt, x, g, retain_graph=True))):
            us, mn = timeit(fn, reps)
            rec(f"dropout_{name} {tag} [{n},{d}] eager call", us, mn, by)

# the reduced losses: cross-entropy [R, C] at the config-3 batch sizes, BCE /
# focal over the config-5 edge logits (4 graphs: 207000 with the padding of
# the static-shape step, 206858 real edges -- not a multiple of 4)
LOSS_CE_SHAPES = [(64, 10), (256, 10)]
LOSS_BCE_SHAPES = [207000, 206858]


def _ab(fa, fb, reps, rounds=5):
    """Interleaved (a, b, a, b, ...) windows of `reps` timed calls each: the
    per-window medians in us, their medians, a's spread and b over a."""
    ms = {"a": [], "b": []}
    for _ in range(rounds):
        for k, fn in (("a", fa), ("b", fb)):
            ms[k].append(round(timeit(fn, reps)[0], 2))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"us_aten": ms["a"], "us_hip": ms["b"], "median_us_aten": med["a"],
            "median_us_hip": med["b"],
            "spread_aten": round((max(ms["a"]) - min(ms["a"])) / med["a"], 4),
            "hip_over_aten": round(med["b"] / med["a"], 4)}


def loss_leg(rec, reps, dev):
    """ops.cross_entropy and ops.bce_logits_loss (mean and focal, masked and
    not) beside the ATen composition of the same objective.  "replayed": the
    kernels alone through the C-ABI (20 forwards / backwards captured and
    replayed), GB/s against the algorithmic bytes (forward: read x, y / label
    [, mask]; backward: the same plus write dx).  "eager call": one forward,
    or forward + backward through autograd, with its host enqueue; the A/B
    windows of the two arms are interleaved."""
    from hlhgat import _lib, ops
    from hlhgat._lib import LIB, check
    F = torch.nn.functional
    gout = torch.ones(1, device=dev)
    loss = torch.empty(1, device=dev)
    ssum = torch.empty(1, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)

    def fwd_bwd(fn, x):
        def run():
            x.grad = None
            fn().backward()
        return run

    for R, C in LOSS_CE_SHAPES:
        x = torch.randn(R, C, device=dev, requires_grad=True)
        xd = x.detach()
        lab = torch.randint(0, C, (R,), device=dev)
        dx = torch.empty(R, C, device=dev)

        def cf():
            check(LIB.hlhgat_cross_entropy_fwd(xd.data_ptr(), C, R, C, lab.data_ptr(), -100,
                                               _lib.LOSS_MEAN, None, 0, loss.data_ptr(),
                                               stats.data_ptr(), ops._stream(xd)), "ce_fwd")

        def cb():
            check(LIB.hlhgat_cross_entropy_bwd(xd.data_ptr(), C, R, C, lab.data_ptr(), -100,
                                               _lib.LOSS_MEAN, stats.data_ptr(), gout.data_ptr(),
                                               dx.data_ptr(), C, ops._stream(xd)), "ce_bwd")

        for name, launch, by in (("fwd", cf, 4.0 * R * C + 8 * R),
                                 ("bwd", cb, 8.0 * R * C + 8 * R)):
            us, mn = replayed(launch, reps)
            rec(f"cross_entropy_{name} hip [{R},{C}] replayed x20", us, mn, by)
        hip = lambda: ops.cross_entropy(x, lab)  # noqa: E731
        aten = lambda: F.cross_entropy(x, lab)  # noqa: E731
        for name, fa, fb in (("fwd", aten, hip), ("fwd+bwd", fwd_bwd(aten, x), fwd_bwd(hip, x))):
            r = _ab(fa, fb, reps)
            rec(f"cross_entropy_{name} [{R},{C}] eager call, aten vs hip", r["median_us_hip"],
                min(r["us_hip"]), None, None, **r)

    for n in LOSS_BCE_SHAPES:
        x = torch.randn(n, device=dev, requires_grad=True)
        xd = x.detach()
        y = (torch.rand(n, device=dev) > 0.5).float()
        mask = torch.rand(n, device=dev) > 0.1
        dx = torch.empty(n, device=dev)
        ws = torch.empty(LIB.hlhgat_loss_workspace_bytes(n), dtype=torch.uint8, device=dev)
        for mtag, mk in (("", None), (" masked", mask)):
            mp = None if mk is None else mk.data_ptr()
            for otag, red, focal in (("bce_mean", _lib.LOSS_MEAN, None),
                                     ("focal", _lib.LOSS_FOCAL, (0.25, 2.0, 1e4))):
                mode = (0, red, 0.25, 2.0, 1e4)

                def bf():
                    check(LIB.hlhgat_bce_reduce_fwd(xd.data_ptr(), y.data_ptr(), mp, n, *mode,
                                                    ws.data_ptr(), ws.numel(), loss.data_ptr(),
                                                    ssum.data_ptr(), stats.data_ptr(),
                                                    ops._stream(xd)), "bce_reduce_fwd")

                def bb():
                    check(LIB.hlhgat_bce_reduce_bwd(xd.data_ptr(), y.data_ptr(), mp, n, *mode,
                                                    ssum.data_ptr(), stats.data_ptr(),
                                                    gout.data_ptr(), dx.data_ptr(),
                                                    ops._stream(xd)), "bce_reduce_bwd")

                nm = 0 if mk is None else n
                for name, launch, by in (("fwd (2 launches)", bf, 8.0 * n + nm),
                                         ("bwd", bb, 12.0 * n + nm)):
                    us, mn = replayed(launch, reps)
                    rec(f"{otag}_{name} hip{mtag} [{n}] replayed x20", us, mn, by)

                def aten():
                    xs, ys = (x, y) if mk is None else (x[mk], y[mk])
                    b = F.binary_cross_entropy_with_logits(xs, ys)
                    if focal is None:
                        return b
                    logpt = -b  # lib/Loss_function.py:22-26
                    pt = torch.exp(logpt)
                    return -((1 - pt) ** focal[1]) * focal[0] * logpt * focal[2]

                hip = lambda: ops.bce_logits_loss(x, y, mk, focal=focal)  # noqa: E731
                for name, fa, fb in (("fwd", aten, hip),
                                     ("fwd+bwd", fwd_bwd(aten, x), fwd_bwd(hip, x))):
                    r = _ab(fa, fb, reps)
                    rec(f"{otag}_{name}{mtag} [{n}] eager call, aten vs hip", r["median_us_hip"],
                        min(r["us_hip"]), None, None, **r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "gpurun_out", "microbench.json"))
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", choices=("dropout", "loss"), default=None,
                    help="run this leg alone (default: every leg)")
    args = ap.parse_args()
    from hlhgat import ops
    from hlhgat.hodge_dataset import collate
    from hlhgat.synthetic import tsp_like_graph, zinc_like_batch

    dev = torch.device("cuda:0")
    res = []

    def rec(name, us, us_min, bytes_=None, flops=None, **kw):
        r = {"op": name, "us": round(us, 2), "us_min": round(us_min, 2)}
        if bytes_:
            r["GBps"] = round(bytes_ / us / 1e3, 1)
            r["hbm_frac"] = round(bytes_ / us / 1e3 / HBM, 4)
        if flops:
            r["TFps"] = round(flops / us / 1e6, 2)
            r["mfma_frac"] = round(flops / us / 1e6 / MFMA, 4)
        r.update(kw)
        res.append(r)
        print(json.dumps(r), flush=True)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    if args.only in ("dropout", "loss"):
        (dropout_leg if args.only == "dropout" else loss_leg)(rec, args.reps, dev)
        save()
        return

    # ---- operators ------------------------------------------------------
    zb = zinc_like_batch(1000, seed=1).to(dev)
    tsp = collate([tsp_like_graph(s) for s in range(4)], check_hodge=False)
    tsp.hodge_sorted = {"edge_index_s": True, "edge_index_t": True}
    tsp = tsp.to(dev)
    shapes = [("zinc_L0", zb.edge_index_t, zb.edge_weight_t, zb.x_t.shape[0], [64]),
              ("zinc_L1", zb.edge_index_s, zb.edge_weight_s, zb.x_s.shape[0], [64]),
              ("tsp4_L1", tsp.edge_index_s, tsp.edge_weight_s, tsp.x_s.shape[0], [32, 64, 128]),
              ("tsp4_L0", tsp.edge_index_t, tsp.edge_weight_t, tsp.x_t.shape[0], [128])]
    for name, ei, w, n, ds in shapes:
        op = ops.hodge_operator(ei, w, n)
        A = op.fwd
        for d in ds:
            X = torch.randn(n, d, device=dev)
            Z = torch.randn(n, d, device=dev)
            Y = torch.empty(n, d, device=dev)
            csr_b = 8 * A.nnz + 4 * (n + 1)
            us, mn = timeit(lambda: ops._poly_step(A, X, Y), args.reps)
            rec(f"spmm {name} d={d}", us, mn, csr_b + 8 * n * d, 2 * A.nnz * d, n=n, nnz=A.nnz)
            us, mn = timeit(lambda: ops._poly_step(A, X, Y, Z=Z, alpha=-1.0, beta=3.0, gamma=-1.0,
                                                   div=2.0), args.reps)
            rec(f"laguerre_step {name} d={d}", us, mn, csr_b + 12 * n * d, 2 * A.nnz * d,
                n=n, nnz=A.nnz)
    # CSR builds (per step work)
    ei, w, n = zb.edge_index_s, zb.edge_weight_s, zb.x_s.shape[0]
    us, mn = timeit(lambda: ops._csr_sorted(ei[0], ei[1], w, n, n), args.reps)
    rec("csr_from_sorted zinc_L1", us, mn)
    us, mn = timeit(lambda: ops._csr_general(ei[1], ei[0], w, n, n), args.reps)
    rec("csr_from_coo(sort) zinc_L1", us, mn)
    us, mn = timeit(lambda: ops.incidence(zb.edge_index.clone(), zb.x_t.shape[0]), args.reps)
    rec("incidence_csr zinc", us, mn)

    # ---- projections ----------------------------------------------------
    for M, N, kbs, tag in [(23259, 64, [64, 64, 64], "conv K=3 d=64"),
                           (23259, 64, [36, 36, 36], "init conv d=36"),
                           (24927, 64, [384, 384], "MSI Linear(768,64)"),
                           (24927, 64, [64], "MSI Linear(64,64)"),
                           (206936, 128, [128] * 4, "tsp conv K=4 d=128")]:
        As = [torch.randn(M, k, device=dev) for k in kbs]
        W = torch.randn(N, sum(kbs), device=dev)
        Ws, o = [], 0
        for k in kbs:
            Ws.append(W[:, o:o + k])
            o += k
        out = torch.empty(M, N, device=dev)
        fl = 2.0 * M * N * sum(kbs)
        by = 4.0 * M * (sum(kbs) + N)
        us, mn = timeit(lambda: ops._proj_fwd(As, Ws, M, N, None, out), args.reps)
        rec(f"proj_fwd {tag}", us, mn, by, fl)
        G = torch.randn(M, N, device=dev)
        dAs = [torch.empty(M, k, device=dev) for k in kbs]
        us, mn = timeit(lambda: ops._proj_bwd_data(G, Ws, kbs, dAs), args.reps)
        rec(f"proj_bwd_data {tag}", us, mn, by, fl)
        dW = torch.empty_like(W)
        dWs, o = [], 0
        for k in kbs:
            dWs.append(dW[:, o:o + k])
            o += k
        db = torch.empty(N, device=dev)
        us, mn = timeit(lambda: ops._proj_bwd_weight(G, As, dWs, db), args.reps)
        rec(f"proj_bwd_weight {tag}", us, mn, by, fl)
        if len(kbs) == 1:
            Wt = W.t().contiguous()
            us, mn = timeit(lambda: torch.mm(As[0], W.t()), args.reps)
            rec(f"torch.mm (hipBLASLt) {tag}", us, mn, by, fl)

    # ---- batch norm --------------------------------------------------------
    for n, C in [(23259, 64), (24927, 64), (1000, 256)]:
        x = torch.randn(n, C, device=dev, requires_grad=True)
        bn = torch.nn.BatchNorm1d(C).to(dev).train()
        us, mn = timeit(lambda: ops.batch_norm_act(x, bn, relu=True), args.reps)
        rec(f"bn_relu_fwd hip [{n},{C}]", us, mn, 8.0 * n * C)
        y = ops.batch_norm_act(x, bn, relu=True)
        g = torch.randn_like(y)
        us, mn = timeit(lambda: torch.autograd.grad(y, x, g, retain_graph=True), args.reps)
        rec(f"bn_relu_bwd hip [{n},{C}]", us, mn, 16.0 * n * C)
        us, mn = timeit(lambda: torch.relu(bn(x)), args.reps)
        rec(f"bn_relu_fwd torch [{n},{C}]", us, mn, 8.0 * n * C)

    # ---- boundary operator / attention ------------------------------------
    inc = ops.incidence(zb.edge_index, zb.x_t.shape[0])
    for d in (64, 384):
        xs = torch.randn(zb.x_s.shape[0], d, device=dev)
        xt = torch.randn(zb.x_t.shape[0], d, device=dev)
        rD = torch.rand(zb.x_t.shape[0], device=dev) + 0.5
        us, mn = timeit(lambda: ops.node_from_edges(xs, inc, rD), args.reps)
        rec(f"node_from_edges d={d}", us, mn, 4.0 * d * (xs.shape[0] + xt.shape[0]))
        us, mn = timeit(lambda: ops.edge_from_nodes(xt, inc), args.reps)
        rec(f"edge_from_nodes d={d}", us, mn, 4.0 * d * (xs.shape[0] + xt.shape[0]))
    q = torch.randn(24927, 96, device=dev)
    us, mn = timeit(lambda: ops.att_score(q[:, :32], q[:, 32:64], q[:, 64:], 0.1, 0.9,
                                          5.656854, ops.SIGMA_SIGMOID), args.reps)
    rec("att_score n=24927 dk=32", us, mn, 4.0 * 24927 * 97)

    # ---- dropout ----------------------------------------------------------
    dropout_leg(rec, args.reps, dev)

    # ---- reduced losses ---------------------------------------------------
    loss_leg(rec, args.reps, dev)
    save()


if __name__ == "__main__":
    main()
