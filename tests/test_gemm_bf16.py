"""bf16 matmul precision of the projections (csrc/proj_bf16.hip; -m gpu).

Contract (include/hlhgat.h, hlhgat_set_gemm_precision): an eligible call equals
the exact products of the RNE-bf16-rounded operands summed in fp32 in some
order -- forward rounds A and W, the data gradient G and W, the weight
gradient G and A; bias, db (from the unrounded G), accumulate adds and the
split reduction are fp32.

1. Integer operands in [-300, 300] with a reduction of at most 128: every
   partial sum is an integer below 2^24, so any order is exact and the device
   result must equal round_bf16 -> fp64 matmul -> fp32 bit for bit.  Pins the
   rounding mode (odd integers above 256 are ties), both operand lane maps,
   the C/D map, the zero fill of the reduction tail, the ragged M / N edges and
   the transposed staging of both gradients.  Operands are column slices of
   NaN-filled slabs: a read outside a view poisons the result, a write outside
   it shows in the slab.
2. Random operands: the error against the fp64 product of the rounded operands
   beyond 1e-6 |A||W|^T is at most 2 x the error of the fp32 kernels run on the
   pre-rounded operands against the same reference (the gate of
   test_proj_big.py).  db is not rounded: each family's db is compared with the
   fp64 column sum of the dC it was given.  Measured on an MI355X: both
   families stay below the floor on every output of every shape (e.g.
   (2500, 64, [768]): out -1.44e-5 / -1.39e-5, dW -1.44e-3 / -1.44e-3), so the
   gate of 2 stands as set and no ratio applies.
3.-7. Another path really runs (counters, different bits), ineligible shapes
   fall back bitwise, the fp32 default is untouched, two runs agree bitwise,
   autograd equals the direct calls, a conv + BatchNorm + ReLU block matches
   the emulated reference, and the whole model sits nearer the bf16-emulating
   CPU oracle than the fp32 one; replay equals eager; overfit still converges.
"""
import pytest
import torch

from bf16_ref import emulate_bf16_linear, emulated_linear, round_bf16
from conftest import close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _restore_fp32():
    import hlhgat
    hlhgat.set_matmul_precision("fp32")
    yield
    hlhgat.set_matmul_precision("fp32")


def _strided(t, dev, pad=float("nan")):
    """t on the device as columns [4, 4 + w) of a slab 8 columns wider."""
    slab = torch.full((t.shape[0], t.shape[1] + 8), pad, device=dev)
    view = slab[:, 4:4 + t.shape[1]]
    view.copy_(t)
    return slab, view


def _pad_untouched(slab):
    return bool(torch.isnan(slab[:, :4]).all() and torch.isnan(slab[:, -4:]).all())


def _split(W, kbs):
    out, o = [], 0
    for k in kbs:
        out.append(W[:, o:o + k])
        o += k
    return out


# ---------------------------------------------------------------------------
# 1. exact data, bitwise
# ---------------------------------------------------------------------------
BLOCKS = [[8], [24], [32], [40], [64], [8, 24, 32], [64, 64]]
MS = [1, 15, 16, 17, 63, 64, 65, 128]
NS = [16, 24, 48, 64, 80, 128]


def _ints(g, *shape):
    return torch.randint(-300, 301, shape, generator=g).float()


def _exact_case(cuda, M, N, kbs, A, W, bias, G, C0, D0):
    """Every entry point on one integer problem against the exact reference;
    bias without accumulate and accumulate without bias (both on, both off)."""
    from hlhgat import ops
    Ar, Wr, Gr = (round_bf16(t).double() for t in (A, W, G))
    what = f"M={M} N={N} kb={kbs}"
    Ad = [_strided(a, cuda)[1] for a in _split(A, kbs)]
    Ws = _split(_strided(W, cuda)[1], kbs)
    Gd = _strided(G, cuda)[1]
    slab, out = _strided(torch.zeros(M, N), cuda)
    ops._proj_fwd(Ad, Ws, M, N, bias.to(cuda), out)
    assert torch.equal(out.cpu(), (Ar @ Wr.t() + bias.double()).float()), what
    assert _pad_untouched(slab), what
    slab, acc = _strided(C0, cuda)
    ops._proj_fwd(Ad, Ws, M, N, None, acc, accumulate=True)
    assert torch.equal(acc.cpu(), (C0.double() + Ar @ Wr.t()).float()), what
    assert _pad_untouched(slab), what
    ref_dA = Gr @ Wr
    pairs = [_strided(torch.zeros(M, k), cuda) for k in kbs]
    ops._proj_bwd_data(Gd, Ws, kbs, [v for _, v in pairs])
    for (slab, v), r in zip(pairs, _split(ref_dA, kbs)):
        assert torch.equal(v.cpu(), r.float()), what
        assert _pad_untouched(slab), what
    pairs = [_strided(d, cuda) for d in _split(D0, kbs)]
    ops._proj_bwd_data(Gd, Ws, kbs, [v for _, v in pairs], accumulate=True)
    for (slab, v), r in zip(pairs, _split(D0.double() + ref_dA, kbs)):
        assert torch.equal(v.cpu(), r.float()), what
        assert _pad_untouched(slab), what
    slab, dW = _strided(torch.zeros(N, sum(kbs)), cuda)
    db = torch.full((N,), float("nan"), device=cuda)
    ops._proj_bwd_weight(Gd, Ad, _split(dW, kbs), db)
    assert torch.equal(dW.cpu(), (Gr.t() @ Ar).float()), what
    assert torch.equal(db.cpu(), G.double().sum(0).float()), what
    assert _pad_untouched(slab), what


@pytest.mark.parametrize("kbs", BLOCKS, ids=lambda k: "x".join(map(str, k)))
def test_exact_integers_bitwise(cuda, kbs):
    import hlhgat
    from hlhgat import ops
    hlhgat.set_matmul_precision("bf16")
    hlhgat.gemm_precision_stats(reset=True)
    g = torch.Generator().manual_seed(1000 * len(kbs) + sum(kbs))
    K = sum(kbs)
    for M in MS:
        for N in NS:
            _exact_case(cuda, M, N, kbs, _ints(g, M, K), _ints(g, N, K), _ints(g, N),
                        _ints(g, M, N), _ints(g, M, N), _ints(g, M, K))
    torch.cuda.synchronize()
    ops.check_device_errors()
    took, fell_back = hlhgat.gemm_precision_stats()
    assert took == 5 * len(MS) * len(NS) and fell_back == 0


def test_identity_times_asymmetric_weight(cuda):
    """A = I returns round_bf16(W)^T element for element (an asymmetric W: a
    transposed or permuted operand map cannot pass), G = I likewise returns
    round_bf16(W) from the data gradient and round_bf16(A) from the weight
    gradient."""
    import hlhgat
    from hlhgat import ops
    hlhgat.set_matmul_precision("bf16")
    g = torch.Generator().manual_seed(3)
    K = 64
    W = _ints(g, 48, K)
    eye = torch.eye(K)
    out = torch.empty(K, 48, device=cuda)
    ops._proj_fwd([eye.to(cuda)], [W.to(cuda)], K, 48, None, out)
    assert torch.equal(out.cpu(), round_bf16(W).t())
    W2 = _ints(g, K, 40)                        # N = 64 rows, 40 reduction columns
    dA = torch.empty(K, 40, device=cuda)
    ops._proj_bwd_data(eye.to(cuda), [W2.to(cuda)], [40], [dA])
    assert torch.equal(dA.cpu(), round_bf16(W2))
    A = _ints(g, K, 24)                         # M = N = 64
    dW = torch.empty(K, 24, device=cuda)
    ops._proj_bwd_weight(eye.to(cuda), [A.to(cuda)], [dW], None)
    assert torch.equal(dW.cpu(), round_bf16(A))
    ops.check_device_errors()


# ---------------------------------------------------------------------------
# 2. random data against the fp32 kernels on pre-rounded operands
# ---------------------------------------------------------------------------
SHAPES = [(777, 64, [40, 96]), (1000, 128, [128] * 4), (513, 256, [448, 448]),
          (2500, 64, [768])]


def _data(M, N, kbs, seed):
    g = torch.Generator().manual_seed(seed)
    As = [torch.randn(M, k, generator=g) for k in kbs]
    W = torch.randn(N, sum(kbs), generator=g) / sum(kbs) ** 0.5
    bias = torch.randn(N, generator=g)
    G = torch.randn(M, N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    return As, W, bias, G, C0


def _run(cuda, prec, As, W, bias, G, C0, kbs):
    import hlhgat
    from hlhgat import ops
    with hlhgat.matmul_precision(prec):
        M, N = G.shape
        Ad = [a.to(cuda) for a in As]
        Wd = W.to(cuda)
        Ws = _split(Wd, kbs)
        out = torch.empty(M, N, device=cuda)
        ops._proj_fwd(Ad, Ws, M, N, bias.to(cuda), out)
        acc = C0.to(cuda).clone()
        ops._proj_fwd(Ad, Ws, M, N, None, acc, accumulate=True)
        Gd = G.to(cuda)
        dAs = [torch.empty(M, k, device=cuda) for k in kbs]
        ops._proj_bwd_data(Gd, Ws, kbs, dAs)
        dW = torch.empty_like(Wd)
        db = torch.empty(N, device=cuda)
        ops._proj_bwd_weight(Gd, Ad, _split(dW, kbs), db)
        # the autograd path (hlhgat_proj_bwd: weight + data in one call)
        Ar = [a.clone().requires_grad_(True) for a in Ad]
        Wr = Wd.clone().requires_grad_(True)
        br = bias.to(cuda).clone().requires_grad_(True)
        y = ops.linear_blocks(Ar, Wr, br)
        y.backward(Gd)
        torch.cuda.synchronize()
    ops.check_device_errors()
    return dict(out=out.cpu(), acc=acc.cpu(), dA=[d.cpu() for d in dAs], dW=dW.cpu(),
                db=db.cpu(), y=y.detach().cpu(), fdA=[a.grad.cpu() for a in Ar],
                fdW=Wr.grad.cpu(), fdb=br.grad.cpu())


def _err(x, ref, mag):
    return float(((x.double() - ref).abs() - 1e-6 * mag).max())


_CASE = {}


def _case(cuda, shape):
    """The data, the fp64 reference and both device runs of one shape (shared
    by the tests below; never modified)."""
    if shape not in _CASE:
        M, N, kbs = shape[0], shape[1], list(shape[2])
        As, W, bias, G, C0 = _data(M, N, kbs, seed=M + N)
        Asr, Wr, Gr = [round_bf16(a) for a in As], round_bf16(W), round_bf16(G)
        A64, W64, G64 = torch.cat(Asr, 1).double(), Wr.double(), Gr.double()
        ref = dict(out=A64 @ W64.t() + bias.double(), acc=C0.double() + A64 @ W64.t(),
                   dA=list((G64 @ W64).split(kbs, 1)), dW=G64.t() @ A64,
                   db=G.double().sum(0), db_rounded=G64.sum(0))
        mag = dict(out=A64.abs() @ W64.abs().t(),
                   dA=list((G64.abs() @ W64.abs()).split(kbs, 1)),
                   dW=G64.abs().t() @ A64.abs(), db=G64.abs().sum(0))
        mag["acc"] = mag["out"]
        _CASE[shape] = dict(
            kbs=kbs, data=(As, W, bias, G, C0), ref=ref, mag=mag,
            bf16=_run(cuda, "bf16", As, W, bias, G, C0, kbs),
            fp32_rounded=_run(cuda, "fp32", Asr, Wr, bias, Gr, C0, kbs))
    return _CASE[shape]


def _key(shape):
    return (shape[0], shape[1], tuple(shape[2]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_data_vs_fp32_kernels_on_rounded_operands(cuda, shape):
    """Gate: err_bf16 <= 2 x err_fp32 beyond the floor, for out, acc, every
    dA_b, dW and db, against the fp64 product of the rounded operands.  The
    fp32 kernels see the pre-rounded operands, so both families sum the same
    exact products and differ in summation order only."""
    c = _case(cuda, _key(shape))
    ref, mag, bf, fp = c["ref"], c["mag"], c["bf16"], c["fp32_rounded"]
    rows = []
    for k in ("out", "acc", "dW"):
        rows.append((k, _err(bf[k], ref[k], mag[k]), _err(fp[k], ref[k], mag[k])))
    # db is summed from the unrounded dC: each run against the column sums of its own dC
    rows.append(("db", _err(bf["db"], ref["db"], mag["db"]),
                 _err(fp["db"], ref["db_rounded"], mag["db"])))
    for b in range(len(c["kbs"])):
        rows.append((f"dA{b}", _err(bf["dA"][b], ref["dA"][b], mag["dA"][b]),
                     _err(fp["dA"][b], ref["dA"][b], mag["dA"][b])))
    print(f"[bf16 vs fp32-on-rounded] M={shape[0]} N={shape[1]} kb={shape[2]}: " +
          ", ".join(f"{k} {eb:.2e}/{es:.2e}" + (f" ({eb / es:.2f}x)" if es > 0 else "")
                    for k, eb, es in rows))
    for k, eb, es in rows:
        assert eb <= max(2 * es, 0.0), (k, eb, es)


# ---------------------------------------------------------------------------
# 3. it really is another path
# ---------------------------------------------------------------------------
def test_bf16_mode_is_another_path(cuda):
    import hlhgat
    shape = _key(SHAPES[0])
    c = _case(cuda, shape)
    As, W, bias, G, C0 = c["data"]
    hlhgat.gemm_precision_stats(reset=True)
    fp32 = _run(cuda, "fp32", As, W, bias, G, C0, c["kbs"])
    assert hlhgat.gemm_precision_stats() == (0, 0)   # fp32 mode books nothing
    bf16 = _run(cuda, "bf16", As, W, bias, G, C0, c["kbs"])
    took, fell_back = hlhgat.gemm_precision_stats(reset=True)
    assert took > 0 and fell_back == 0
    assert not torch.equal(bf16["out"], fp32["out"])
    assert not torch.equal(bf16["dW"], fp32["dW"])
    assert not torch.equal(bf16["dA"][0], fp32["dA"][0])


@pytest.mark.parametrize("kbs", [[18], [36, 100]], ids=["18", "36x100"])
def test_ineligible_shapes_fall_back_bitwise(cuda, kbs):
    import hlhgat
    As, W, bias, G, C0 = _data(333, 64, kbs, seed=11)
    fp32 = _run(cuda, "fp32", As, W, bias, G, C0, kbs)
    hlhgat.gemm_precision_stats(reset=True)
    bf16 = _run(cuda, "bf16", As, W, bias, G, C0, kbs)
    took, fell_back = hlhgat.gemm_precision_stats(reset=True)
    assert took == 0 and fell_back >= 5
    for k in ("out", "acc", "dW", "db", "y", "fdW", "fdb"):
        assert torch.equal(bf16[k], fp32[k]), k
    for k in ("dA", "fdA"):
        for x, y in zip(bf16[k], fp32[k]):
            assert torch.equal(x, y), k


# ---------------------------------------------------------------------------
# 4. the default is untouched   5. determinism   6. autograd
# ---------------------------------------------------------------------------
def _same(a, b):
    for k in a:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), k


def test_fp32_results_survive_a_bf16_interlude(cuda):
    kbs = [64, 64, 64]
    As, W, bias, G, C0 = _data(1500, 64, kbs, seed=21)
    first = _run(cuda, "fp32", As, W, bias, G, C0, kbs)
    between = _run(cuda, "bf16", As, W, bias, G, C0, kbs)
    last = _run(cuda, "fp32", As, W, bias, G, C0, kbs)
    _same(first, last)
    assert not torch.equal(between["out"], first["out"])


def test_bf16_is_deterministic(cuda):
    shape = _key(SHAPES[3])
    c = _case(cuda, shape)
    As, W, bias, G, C0 = c["data"]
    again = _run(cuda, "bf16", As, W, bias, G, C0, c["kbs"])
    _same(c["bf16"], again)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=lambda s: f"{s[0]}x{s[1]}")
def test_autograd_equals_the_direct_calls(cuda, shape):
    r = _case(cuda, _key(shape))["bf16"]
    assert torch.equal(r["y"], r["out"])
    assert torch.equal(r["fdW"], r["dW"]) and torch.equal(r["fdb"], r["db"])
    for x, y in zip(r["fdA"], r["dA"]):
        assert torch.equal(x, y)


def test_conv_bn_relu_block_matches_the_emulated_reference(cuda):
    """HodgeLaguerreConv(64, 64, K=3) -> BatchNorm -> ReLU through forward_bn on
    three ZINC-like graphs.  Reference: the device's own fp32 Laguerre basis,
    the emulated Linear, fp64 BatchNorm; the basis adjoint for dx from the
    basis applied to the identity.  Layer tolerance of DESIGN.md §5: 1e-5 *
    max(1, max|ref|) forward, 1e-4 relative gradients; the fp32-mode output of
    the same block is outside that forward tolerance."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    b = zinc_like_batch(3, seed=1).to(cuda)
    ei, ew, n = b.edge_index_t, b.edge_weight_t, b.x_t.shape[0]
    K, F = 3, 64
    torch.manual_seed(0)
    conv = hlhgat.HodgeLaguerreConv(F, F, K=K).to(cuda)
    bn = torch.nn.BatchNorm1d(F).to(cuda)
    with torch.no_grad():
        conv.bias.normal_()
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    x = torch.randn(n, F, device=cuda)
    G = torch.randn(n, F, device=cuda)
    params = [lin.weight for lin in conv.lins] + [conv.bias, bn.weight, bn.bias]

    def run(prec):
        for p in params:
            p.grad = None
        with hlhgat.matmul_precision(prec):
            xx = x.clone().requires_grad_(True)
            y = conv.forward_bn(xx, ei, ew, bn, relu=True)
            y.backward(G)
            torch.cuda.synchronize()
        return [y.detach().cpu(), xx.grad.cpu()] + [p.grad.cpu().clone() for p in params]

    hlhgat.gemm_precision_stats(reset=True)
    got = run("bf16")
    took, fell_back = hlhgat.gemm_precision_stats(reset=True)
    assert took >= 3 and fell_back == 0
    got32 = run("fp32")
    ops.check_device_errors()

    op = ops.hodge_operator(ei, ew, n)
    T = ops.poly_basis(op, x, K, ops.POLY_LAGUERRE)
    Fi = (n + 63) // 64 * 64
    eye = torch.zeros(n, Fi, device=cuda)
    eye[:, :n] = torch.eye(n, device=cuda)
    P = ops.poly_basis(op, eye, K, ops.POLY_LAGUERRE)[:, :, :n].double().cpu()
    Ts = [t.double().cpu().requires_grad_(True) for t in [x] + list(T)]
    Wk = [lin.weight.detach().double().cpu().requires_grad_(True) for lin in conv.lins]
    cb, bw, bb = (p.detach().double().cpu().requires_grad_(True)
                  for p in (conv.bias, bn.weight, bn.bias))
    z = sum(emulated_linear(t, w) for t, w in zip(Ts, Wk)) + cb
    mean, var = z.mean(0), z.var(0, unbiased=False)
    y = torch.relu((z - mean) / torch.sqrt(var + bn.eps) * bw + bb)
    y.backward(G.double().cpu())
    dx = Ts[0].grad + sum(P[k].t() @ Ts[k + 1].grad for k in range(K - 1))
    want = [y.detach(), dx] + [w.grad for w in Wk] + [cb.grad, bw.grad, bb.grad]
    names = ["y", "dx"] + [f"dW{k}" for k in range(K)] + ["dbias", "dbn_w", "dbn_b"]
    close(got[0], want[0], 1e-5, "y")
    for name, a, e in list(zip(names, got, want))[1:]:
        close(a, e, 1e-4, name)
    scale = max(1.0, float(want[0].abs().max()))
    err32 = float((got32[0].double() - want[0]).abs().max())
    assert err32 > 1e-5 * scale, err32


# ---------------------------------------------------------------------------
# 7. whole model and replay
# ---------------------------------------------------------------------------
MODEL_KW = dict(channels=[2], filters=[64], mlp_channels=[256, 256], K=3, keig=15)


def _dist(x, y):
    return float((x.double() - y.double()).abs().max())


def test_model_sits_nearer_the_bf16_oracle(cuda):
    """d = max|x - y| over the output and over the concatenated parameter
    gradients: the bf16-mode device model is strictly nearer the bf16-emulating
    CPU oracle than the fp32 oracle, the fp32-mode model the other way round."""
    import hlhgat
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    from oracle.hodge_ref import RefZincModel
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**MODEL_KW)
    ref = RefZincModel(**MODEL_KW)
    ref.load_state_dict(m.state_dict())
    ref.train()
    m = m.to(cuda).train()
    names = [k for k, p in ref.named_parameters() if p.requires_grad]
    b_cpu = zinc_like_batch(8, seed=0)
    b = zinc_like_batch(8, seed=0).to(cuda)

    def oracle(emulate):
        ref.zero_grad()
        if emulate:
            with emulate_bf16_linear():
                out = ref(b_cpu)
                torch.nn.functional.l1_loss(out.view(-1), b_cpu.y.view(-1)).backward()
        else:
            out = ref(b_cpu)
            torch.nn.functional.l1_loss(out.view(-1), b_cpu.y.view(-1)).backward()
        gp = dict(ref.named_parameters())
        return out.detach().clone(), torch.cat([gp[k].grad.reshape(-1) for k in names])

    def device(prec):
        m.zero_grad()
        with hlhgat.matmul_precision(prec):
            out = m(b)
            torch.nn.functional.l1_loss(out.view(-1), b.y.view(-1)).backward()
            torch.cuda.synchronize()
        gp = dict(m.named_parameters())
        return out.detach().cpu(), torch.cat([gp[k].grad.reshape(-1).cpu() for k in names])

    o32, g32 = oracle(False)
    o16, g16 = oracle(True)
    d32, dg32 = device("fp32")
    d16, dg16 = device("bf16")
    ops.check_device_errors()
    rows = {"bf16 out": (_dist(d16, o16), _dist(d16, o32)),
            "bf16 grad": (_dist(dg16, g16), _dist(dg16, g32)),
            "fp32 out": (_dist(d32, o32), _dist(d32, o16)),
            "fp32 grad": (_dist(dg32, g32), _dist(dg32, g16))}
    print("[model vs oracles] " + ", ".join(
        f"{k}: own {a:.2e} other {o:.2e} (ratio {a / o:.3f})" for k, (a, o) in rows.items()))
    for k, (own, other) in rows.items():
        assert own < other, (k, own, other)


def _loss_fn():
    import hlhgat
    crit = hlhgat.nn.L1Loss()
    return lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1))


def _train(cuda, batch, prec, graphs, steps=3, lr=1e-3):
    """`steps` optimiser steps of a fresh, identically seeded model; losses,
    final flat parameters, and the captured graphs' bf16 kernel count."""
    import hlhgat
    from hlhgat import ops, train
    from hlhgat.train import TrainStep
    keep = train.KEEP_GRAPHS
    train.KEEP_GRAPHS = True
    try:
        torch.manual_seed(0)
        m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**MODEL_KW).to(cuda).train()
        st = TrainStep(m, _loss_fn(), lr=lr, graphs=graphs, matmul_precision=prec)
        losses = [float(st(batch)) for _ in range(steps)]
        torch.cuda.synchronize()
        n_bf16 = 0
        if graphs:
            for ent in st._graphs.values():
                n_bf16 += ops.graph_kernel_count(ent.graph.raw_cuda_graph(), "bf16")[1]
    finally:
        train.KEEP_GRAPHS = keep
    return dict(losses=losses, flat=st.flat.detach().clone(), bf16_kernels=n_bf16,
                stats=dict(st.stats))


def test_train_step_replay_equals_eager_and_modes_do_not_leak(cuda):
    import hlhgat
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    batch = zinc_like_batch(8, seed=0).to(cuda)
    before = _train(cuda, batch, "fp32", True)
    replayed = _train(cuda, batch, "bf16", True)
    eager = _train(cuda, batch, "bf16", False)
    after = _train(cuda, batch, "fp32", True)
    ops.check_device_errors()
    assert hlhgat.get_matmul_precision() == "fp32"
    assert replayed["stats"]["replay"] == 2 and eager["stats"].get("replay", 0) == 0
    assert replayed["losses"] == eager["losses"]
    assert torch.equal(replayed["flat"], eager["flat"])
    assert replayed["bf16_kernels"] > 0
    assert after["bf16_kernels"] == 0 and before["bf16_kernels"] == 0
    assert after["losses"] == before["losses"]
    assert torch.equal(after["flat"], before["flat"])
    assert replayed["losses"] != before["losses"]


def test_overfit_one_batch_in_both_modes(cuda):
    """30 replayed steps on one batch, lr 1e-3: every loss finite and the bf16
    run's final loss below its first."""
    import math
    from hlhgat.synthetic import zinc_like_batch
    batch = zinc_like_batch(8, seed=0).to(cuda)
    runs = {p: _train(cuda, batch, p, True, steps=30)["losses"] for p in ("fp32", "bf16")}
    for p, ls in runs.items():
        assert all(math.isfinite(v) for v in ls), p
    print("[overfit] final/first: " + ", ".join(
        f"{p} {ls[-1] / ls[0]:.4f} ({ls[0]:.4f} -> {ls[-1]:.4f})" for p, ls in runs.items()))
    assert runs["bf16"][-1] < runs["bf16"][0]
