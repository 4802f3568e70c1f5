"""The brain notebook's loop on the product (HL-HGAT-DEMO/OHBM_DEMO.ipynb,
train(loader) / test(loader)): HL_HGAT_attpool under TrainStep and InferStep
as replayed graphs, hlhgat.nn.MSELoss, Adam(lr=1e-4, weight_decay=1e-4), the
cluster tables BrainPipeline.levels_for builds once.

Shapes: the 24-node skeleton of the brain_head_small fixture with its coarse
level, B = 3 and B = 2 subjects, T = 23 (shorter than one 64-row tile of the
temporal kernels: series boundaries fall inside tiles).
"""
import copy
import functools

import numpy as np
import pytest
import torch

import brain_ref as B
from conftest import load_golden
from test_brain_fc import _head_levels
from test_brain_head import HEAD, _head_kw, _sd

T = 23
BATCHES = ([0, 1, 2], [3, 1, 0], [2, 3])
TABLES = ("pool_rowptr_t", "pool_rows_t", "pool_rowptr_s", "pool_rows_s")


@functools.lru_cache(maxsize=None)
def _pipe():
    import hlhgat
    g = load_golden(HEAD)
    levels = _head_levels(g)
    N = levels[0].x_t.shape[0]
    rng = np.random.default_rng(5)
    series = [((rng.standard_normal((N, 3)) @ rng.standard_normal((3, T + 4))
                + rng.standard_normal((N, T + 4))) * 50 + 1000).astype(np.float32)
              for _ in range(4)]
    y = torch.tensor([0.3, -1.2, 0.8, 2.0])
    return hlhgat.BrainPipeline(series, y, levels), levels


def _model(cuda):
    import hlhgat
    g = load_golden(HEAD)
    torch.manual_seed(0)
    m = hlhgat.HL_HGAT_attpool(**_head_kw(g))
    m.load_state_dict(_sd(g), strict=True)
    return m.to(cuda).train()


def _train_step(cuda, graphs):
    import hlhgat
    from hlhgat.train import TrainStep
    mse = hlhgat.nn.MSELoss()
    return TrainStep(_model(cuda), lambda o, d: mse(o[0], d[0].y.view(-1, 1)), lr=1e-4,
                     weight_decay=1e-4, graphs=graphs)


def _batch(cuda, idx):
    return _pipe()[0].batch(idx, window=(2, T), device=cuda)


_RUNS = {}


def _six_steps(cuda, graphs):
    """Six steps over BATCHES twice: (losses, state_dict after, stats, the
    TrainStep state after three steps); run once per mode."""
    if graphs not in _RUNS:
        from hlhgat import ops
        step = _train_step(cuda, graphs)
        losses, mid = [], None
        for i in range(6):
            losses.append(step(_batch(cuda, BATCHES[i % 3])).clone())
            if i == 2:
                mid = copy.deepcopy(step.state_dict())
        ops.check_device_errors()
        sd = {k: v.detach().clone() for k, v in step.model.state_dict().items()}
        _RUNS[graphs] = (losses, sd, dict(step.stats), mid)
    return _RUNS[graphs]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_graphs", [3, 2])
def test_pos_cluster_tables_equal_stable_sort(n_graphs):
    """The tables levels_for attaches are a stable sort of the fine rows by
    global cluster, inf (dropped) last: the CSR cluster_mean builds."""
    pipe, levels = _pipe()
    lv = pipe.levels_for(n_graphs, "cpu")
    for side, cnt in (("t", "num_node1"), ("s", "num_edge1")):
        pos = np.asarray(getattr(levels[0], "pos_" + side), dtype=np.float64).reshape(-1)
        n_c = int(getattr(levels[1], cnt))
        glob = np.concatenate([pos + b * n_c for b in range(n_graphs)])
        n_coarse = n_graphs * n_c
        assert int(getattr(lv[1], "x_" + side).shape[0]) == n_coarse
        key = np.where(np.isinf(glob), n_coarse, glob).astype(np.int64)
        order = np.argsort(key, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n_coarse + 1))])
        rp, rows = getattr(lv[0], "pool_rowptr_" + side), getattr(lv[0], "pool_rows_" + side)
        assert rp.dtype == torch.int32 and rows.dtype == torch.int32
        assert rp.numel() == n_coarse + 2 and rows.numel() == glob.size
        assert np.array_equal(rp.numpy(), rowptr) and np.array_equal(rows.numpy(), order)
        if side == "s":
            assert np.isinf(pos).any()  # the fixture drops edges: the last bucket is used
            assert int(rp[-1] - rp[-2]) == n_graphs * int(np.isinf(pos).sum())
    assert not any(hasattr(lv[1], k) for k in TABLES)  # the last level pools nowhere


def test_pool_tables_default_is_column_zero():
    """pool_tables without the keyword still reads feature column 0."""
    from hlhgat.hodge_dataset import PairData, pool_tables
    d0 = PairData(x_t=torch.tensor([[1.0, 9.0], [0.0, 9.0], [1.0, 9.0]]),
                  x_s=torch.tensor([[0.0], [float("inf")]]))
    d1 = PairData(x_t=torch.zeros(2, 1), x_s=torch.zeros(1, 1))
    d0.num_node1, d0.num_edge1 = torch.tensor([3]), torch.tensor([2])
    d1.num_node1, d1.num_edge1 = torch.tensor([2]), torch.tensor([1])
    d0.pos_t = torch.tensor([0.0, 0.0, 1.0])  # ignored without pos=True
    pool_tables([d0, d1])
    assert d0.pool_rows_t.tolist() == [1, 0, 2] and d0.pool_rowptr_t.tolist() == [0, 1, 3, 3]
    assert d0.pool_rows_s.tolist() == [0, 1] and d0.pool_rowptr_s.tolist() == [0, 1, 2]
    d0.pos_s = torch.tensor([float("inf"), 0.0])
    pool_tables([d0, d1], pos=True)
    assert d0.pool_rows_t.tolist() == [0, 1, 2] and d0.pool_rowptr_t.tolist() == [0, 2, 3, 3]
    assert d0.pool_rows_s.tolist() == [1, 0] and d0.pool_rowptr_s.tolist() == [0, 1, 2]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_tables_change_no_bits(cuda):
    """The head in train mode on the pipeline's batch (cluster CSR and degree
    from the tables) and on the hand-built list without them (the cluster
    sort and the degree scatter on the device): the same bits."""
    from hlhgat import ops
    from hlhgat.hodge_dataset import collate
    g = load_golden(HEAD)
    _, levels = _pipe()
    N, E = levels[0].x_t.shape[0], levels[0].x_s.shape[0]
    got = _batch(cuda, BATCHES[0])
    assert all(torch.is_tensor(getattr(got[0], k)) and getattr(got[0], k).is_cuda for k in TABLES)
    fine = copy.copy(levels[0])
    fine.x_t, fine.x_s = torch.zeros(N, 1), torch.zeros(E, 1)
    hand = [collate([fine] * 3).to(cuda), collate([levels[1]] * 3).to(cuda)]
    hand[0].x_t, hand[0].x_s = got[0].x_t, got[0].x_s
    for lv in hand:
        for k in TABLES + ("deg_t", "inv_deg_t"):
            if hasattr(lv, k):
                delattr(lv, k)
    m = _model(cuda)
    R = torch.from_numpy(g["R"]).to(cuda)
    runs = []
    for datas in (got, hand):
        for p in m.parameters():
            p.grad = None
        ops.clear_caches()
        outs = m(datas, device=cuda)
        (outs[0] * R).sum().backward()
        runs.append([o.detach().clone() for o in outs]
                    + [p.grad.detach().clone() for p in m.parameters()])
    assert len(runs[0]) == 4 + len(list(m.parameters()))
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.isfinite(a).all() and torch.equal(a, b), i
    ops.check_device_errors()


@pytest.mark.gpu
def test_replay_equals_eager(cuda):
    eager, graph = _six_steps(cuda, False), _six_steps(cuda, True)
    for i, (a, b) in enumerate(zip(eager[0], graph[0])):
        assert torch.isfinite(a) and torch.equal(a, b), (i, float(a), float(b))
    assert list(eager[1]) == list(graph[1])
    assert any(k.endswith("num_batches_tracked") for k in eager[1])
    assert any(k.endswith("running_var") for k in eager[1])
    for k in eager[1]:
        assert torch.equal(eager[1][k], graph[1][k]), k
    # one capture per batch size; every later step of a shape is a replay
    assert graph[2] == {"eager": 2, "captures": 2, "replay": 4}
    assert eager[2] == {"eager": 6, "captures": 0, "replay": 0}
    # the steps moved the model
    g = load_golden(HEAD)
    k = "out.weight"
    assert not torch.equal(graph[1][k].cpu(), _sd(g)[k])


@pytest.mark.gpu
def test_first_loss_vs_fp64_restatement(cuda):
    """The first step's loss against brain_ref.RefBrainHead and F.mse_loss in
    fp64 on the same inputs.  test_head_vs_fixture_and_fp64 holds ``out`` to
    delta = 1e-4 max(1, max|out64|) (conftest.close); through the loss that
    is mean(2 |out64 - y| delta + delta^2)."""
    g = load_golden(HEAD)
    datas = _batch(cuda, BATCHES[0])
    ref = []
    for lv, d in enumerate(datas):
        r = type("D", (), {})()
        for k, v in vars(d).items():
            if torch.is_tensor(v) and not k.startswith("_"):
                v = v.detach().cpu()
                setattr(r, k, v.double() if v.is_floating_point() else v)
        ref.append(r)
    m64 = B.RefBrainHead(**_head_kw(g))
    m64.load_state_dict(_sd(g), strict=True)
    m64 = m64.double().train()
    out64 = m64(ref)[0].detach()
    y = ref[0].y.view(-1, 1)
    want = float(torch.nn.functional.mse_loss(out64, y))
    delta = 1e-4 * max(1.0, float(out64.abs().max()))
    bound = float((2.0 * (out64 - y).abs() * delta + delta ** 2).mean())
    got = float(_six_steps(cuda, False)[0][0])
    print(f"[brain first loss] got {got:.9g} fp64 {want:.9g} |diff| {abs(got - want):.3e} "
          f"bound {bound:.3e}")
    assert abs(got - want) <= bound


@pytest.mark.gpu
def test_eval_replay(cuda):
    import hlhgat
    from hlhgat import ops
    from hlhgat.train import InferStep
    res = {}
    for graphs in (False, True):
        m = _model(cuda)
        meter = hlhgat.RegressionMeter(16, cuda)
        step = InferStep(m, graphs=graphs,
                         meter=lambda o, d, mt=meter: mt.update(o[0].view(-1), d[0].y))
        outs = []
        for i in range(6):
            outs.append([t.clone() for t in step(_batch(cuda, BATCHES[i % 3]))])
        ops.check_device_errors()
        res[graphs] = (outs, meter.compute(), dict(step.stats))
    assert res[True][2] == {"eager": 2, "captures": 2, "replay": 4}
    for i, (a, b) in enumerate(zip(res[False][0], res[True][0])):
        assert len(a) == len(b) == 4
        for u, v in zip(a, b):  # out, latent, node_att, edge_att
            assert torch.isfinite(u).all() and torch.equal(u, v), i
    ma, mb = res[False][1], res[True][1]
    assert ma["n"] == mb["n"] == 16 and set(ma) == set(mb)
    for k in ma:
        assert ma[k] == mb[k] and np.isfinite(ma[k]), (k, ma[k], mb[k])


@pytest.mark.gpu
def test_resume(cuda):
    """state_dict() after three steps, loaded into a fresh TrainStep on a fresh
    model, continues with the uninterrupted run's losses."""
    from hlhgat import ops
    losses, _, _, mid = _six_steps(cuda, True)
    step = _train_step(cuda, True)
    with torch.no_grad():  # a fresh model is not the trained one
        for p in step.params:
            p.add_(0.5)
    step.load_state_dict(mid)
    for i in range(3, 6):
        got = step(_batch(cuda, BATCHES[i % 3]))
        assert torch.equal(got, losses[i]), (i, float(got), float(losses[i]))
    ops.check_device_errors()
