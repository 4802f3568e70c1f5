"""The epoch loop's learning-rate schedule and resume on hlhgat.train.TrainStep.

The reference scripts step ReduceLROnPlateau once per epoch.  With the HIP
Adam the learning rate is one fp64 device scalar that the update kernel reads
(hlhgat_adam_flat_dev*), so an unmodified torch scheduler on ``step.opt``
drives eager and replayed steps alike, through ONE captured graph per batch
shape; ``state_dict`` / ``load_state_dict`` carry it with the moments, the
step count and the dropout counter.

The model and data of tests/test_train_step.py (``_Tiny``) are restated here.
"""
import io

import pytest
import torch


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.b = torch.nn.Linear(7, 1)

    def forward(self, batch):
        return self.b(torch.relu(self.a(batch.x)))


class _B:
    def __init__(self, x, y):
        self.x, self.y = x, y

    def to(self, dev):
        return _B(self.x.to(dev), self.y.to(dev))


def _loss(out, b):
    return torch.nn.functional.l1_loss(out.view(-1), b.y.view(-1))


def _data(seed, n=16):
    g = torch.Generator().manual_seed(seed)
    return _B(torch.randn(n, 5, generator=g), torch.randn(n, generator=g))


LR0, WD = 1e-2, 1e-3
# the metric handed to ReduceLROnPlateau(mode="max", patience=0, factor=0.5):
# the call made before the first step only establishes `best` (the first value
# always counts as an improvement); the falling values after steps 2 and 4 each
# halve the learning rate
METRIC_AFTER = {2: 0.5, 4: 0.25}


def _plateau(opt):
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0, factor=0.5, mode="max")
    sched.step(1.0)
    return sched


def _opt_state(step):
    st = step.opt.state[step.master]
    return {k: st[k].detach().cpu().clone() for k in ("step", "exp_avg", "exp_avg_sq")}


def _tiny_run(dev, graphs, n_steps=6, schedule=True, lr=LR0):
    """n_steps of TrainStep on _Tiny with the plateau schedule; returns
    (parameters, optimiser state, lr, stats, lrs seen after each step)."""
    from hlhgat.train import TrainStep
    torch.manual_seed(0)
    m = _Tiny().to(dev)
    step = TrainStep(m, _loss, lr=lr, weight_decay=WD, graphs=graphs)
    sched = _plateau(step.opt) if schedule else None
    lrs = []
    for i in range(1, n_steps + 1):
        step(_data(i).to(dev))
        if sched is not None and i in METRIC_AFTER:
            sched.step(METRIC_AFTER[i])
        lrs.append(step.lr)
    params = [p.detach().cpu().clone() for p in m.parameters()]
    return params, _opt_state(step), step.lr, dict(step.stats), lrs, step


def _torch_loop(n_steps=6):
    """The reference loop: torch.optim.Adam on the CPU driven by the same
    scheduler and metric."""
    torch.manual_seed(0)
    m = _Tiny()
    opt = torch.optim.Adam(m.parameters(), lr=LR0, weight_decay=WD)
    sched = _plateau(opt)
    for i in range(1, n_steps + 1):
        b = _data(i)
        opt.zero_grad()
        _loss(m(b), b).backward()
        opt.step()
        if i in METRIC_AFTER:
            sched.step(METRIC_AFTER[i])
    return [p.detach().clone() for p in m.parameters()], opt.param_groups[0]["lr"]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_cpu_step_follows_scheduler_and_matches_torch_loop():
    params, _, lr, _, lrs, step = _tiny_run("cpu", graphs=False)
    ref, ref_lr = _torch_loop()
    assert lr == ref_lr == 2.5e-3
    assert lrs == [1e-2, 5e-3, 5e-3, 2.5e-3, 2.5e-3, 2.5e-3]
    for p, r in zip(params, ref):
        assert torch.allclose(p, r, rtol=1e-6, atol=1e-7)
    step.set_lr(1e-4)
    assert step.lr == 1e-4 and step.opt.param_groups[0]["lr"] == 1e-4


def test_cpu_load_state_dict_round_trips():
    from hlhgat.train import TrainStep
    full, full_opt, full_lr, _, _, _ = _tiny_run("cpu", graphs=False, n_steps=5)
    _, _, _, _, _, step = _tiny_run("cpu", graphs=False, n_steps=3)
    buf = io.BytesIO()
    torch.save(step.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf)
    torch.manual_seed(123)
    m = _Tiny()
    resumed = TrainStep(m, _loss, lr=0.5, weight_decay=WD, graphs=False)
    resumed.load_state_dict(sd)
    assert resumed.lr == 5e-3
    assert all(p.data_ptr() == resumed.flat.data_ptr() + 4 * off
               for p, off in zip(resumed.params, resumed._offsets))
    for i in (4, 5):
        resumed(_data(i))
        if i == 4:  # the uninterrupted run's second halving
            resumed.set_lr(2.5e-3)
    assert resumed.lr == full_lr
    for p, r in zip(m.parameters(), full):
        assert torch.equal(p.detach(), r)
    got = _opt_state(resumed)
    for k in full_opt:
        assert torch.equal(got[k], full_opt[k]), k


# ---------------------------------------------------------------------------
# GPU, kernel level
# ---------------------------------------------------------------------------
def _adam_steps(cuda, lrs, wd, prepared, device_lr):
    """3 updates of an n = 1027 buffer with ops.adam_flat; the learning rate
    of step i is lrs[i], passed as a float or through ONE fp64 device scalar
    overwritten in place between the steps."""
    from hlhgat import ops
    n = 1027
    g = torch.Generator().manual_seed(11)
    p = torch.randn(n, generator=g).to(cuda)
    grads = [torch.randn(n, generator=g).to(cuda) for _ in lrs]
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros((), device=cuda)
    gbuf = torch.empty_like(p)
    lr_dev = torch.full((), lrs[0], dtype=torch.float64, device=cuda)
    ptr = lr_dev.data_ptr()
    for lr, gr in zip(lrs, grads):
        if prepared:
            ops.adam_prepare(gbuf, step)  # zeroes the gradient, counts the step
        gbuf.copy_(gr)
        if device_lr:
            lr_dev.fill_(lr)
            assert lr_dev.data_ptr() == ptr
        ops.adam_flat(p, gbuf, m, v, step, lr_dev if device_lr else lr, (0.9, 0.999), 1e-8, wd,
                      prepared=prepared)
    torch.cuda.synchronize()
    return p.cpu(), m.cpu(), v.cpu(), step.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("lrs", [(1e-3, 1e-3, 1e-3), (1e-3, 5e-4, 2.5e-4)])
def test_adam_flat_device_lr_bitwise_float_lr(cuda, lrs, wd, prepared):
    by_value = _adam_steps(cuda, lrs, wd, prepared, device_lr=False)
    by_device = _adam_steps(cuda, lrs, wd, prepared, device_lr=True)
    assert float(by_device[3]) == 3.0
    for a, b, name in zip(by_value, by_device, ("param", "exp_avg", "exp_avg_sq", "step")):
        assert torch.equal(a, b), name
    if len(set(lrs)) > 1:  # the overwritten value was used
        const = _adam_steps(cuda, (lrs[0],) * 3, wd, prepared, device_lr=True)
        assert not torch.equal(const[0], by_device[0])


@pytest.mark.gpu
def test_adam_flat_rejects_a_wrong_lr_tensor(cuda):
    from hlhgat import ops
    p = torch.zeros(8, device=cuda)
    s = torch.zeros((), device=cuda)
    for bad in (torch.tensor(1e-3, device=cuda), torch.tensor(1e-3, dtype=torch.float64),
                torch.zeros(2, dtype=torch.float64, device=cuda)):
        with pytest.raises(RuntimeError):
            ops.adam_flat(p, p.clone(), p.clone(), p.clone(), s, bad, (0.9, 0.999), 1e-8, 0.0)


# ---------------------------------------------------------------------------
# GPU, TrainStep
# ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_plateau_schedule_under_graph_replay(cuda):
    """(a) ReduceLROnPlateau on step.opt halves the learning rate after steps
    2 and 4; the replayed run keeps ONE captured graph and gives the bits of
    the eager run, which matches the torch loop."""
    p_g, o_g, lr_g, stats, lrs_g, step = _tiny_run(cuda, graphs=True)
    assert stats["captures"] == 1 and stats["replay"] == 5, stats
    assert lr_g == 2.5e-3
    assert lrs_g == [1e-2, 5e-3, 5e-3, 2.5e-3, 2.5e-3, 2.5e-3]
    lr_t = step.opt.param_groups[0]["lr"]
    assert torch.is_tensor(lr_t) and lr_t.dtype == torch.float64 and lr_t.is_cuda
    p_e, o_e, lr_e, stats_e, lrs_e, _ = _tiny_run(cuda, graphs=False)
    assert stats_e["captures"] == 0 and lr_e == 2.5e-3 and lrs_e == lrs_g
    for a, b in zip(p_g, p_e):
        assert torch.equal(a, b)
    for k in o_g:
        assert torch.equal(o_g[k], o_e[k]), k
    assert float(o_g["step"]) == 6.0
    ref, ref_lr = _torch_loop()
    assert ref_lr == 2.5e-3
    for a, r in zip(p_g, ref):
        print("max |param - torch loop|", float((a - r).abs().max()))
        assert torch.allclose(a, r, rtol=1e-6, atol=1e-7)
    p_c, _, lr_c, _, _, _ = _tiny_run(cuda, graphs=True, schedule=False)
    assert lr_c == 1e-2
    assert any(not torch.equal(a, c) for a, c in zip(p_g, p_c))


KW = dict(channels=[1, 1], filters=[32, 32], mlp_channels=[64], K=3, keig=15)


def _zinc_run(cuda, graphs, batch):
    import hlhgat
    from hlhgat import ops
    from hlhgat.train import TrainStep
    torch.manual_seed(0)
    m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**KW).to(cuda).train()
    crit = torch.nn.L1Loss()
    step = TrainStep(m, lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1)), lr=1e-3,
                     weight_decay=1e-3, graphs=graphs)
    ops.clear_device_errors()
    losses = []
    for i in range(4):
        losses.append(float(step(batch)))
        if i == 1:
            step.set_lr(2.5e-4)
    torch.cuda.synchronize()
    assert ops.device_errors() == 0
    assert step.lr == 2.5e-4
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    return losses, sd, _opt_state(step), dict(step.stats)


@pytest.mark.gpu
def test_config2_replay_equals_eager_through_a_lr_change(cuda):
    """(b) The config-2 model (deferred reductions, the prepared Adam) with
    the device learning rate changed after step 2: replay == eager, bitwise."""
    from hlhgat.synthetic import zinc_like_batch
    batch = zinc_like_batch(20, seed=3).to(cuda)
    l_e, sd_e, o_e, _ = _zinc_run(cuda, False, batch)
    l_g, sd_g, o_g, st = _zinc_run(cuda, True, batch)
    assert st["captures"] == 1 and st["replay"] == 3, st
    assert l_e == l_g
    for k in sd_e:
        assert torch.equal(sd_e[k], sd_g[k]), k
    for k in o_e:
        assert torch.equal(o_e[k], o_g[k]), k


@pytest.mark.gpu
def test_set_lr_inside_a_capture_raises(cuda):
    """(c)"""
    from hlhgat.train import TrainStep
    torch.manual_seed(0)
    step = TrainStep(_Tiny().to(cuda), _loss, lr=LR0, graphs=True)
    buf = torch.zeros(4, device=cuda)
    s = torch.cuda.Stream(device=cuda)
    s.wait_stream(torch.cuda.current_stream(cuda))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        buf.add_(1.0)
        with pytest.raises(RuntimeError, match="capture"):
            step.set_lr(1e-3)
    torch.cuda.synchronize()
    assert step.lr == LR0
    step.set_lr(1e-3)
    assert step.lr == 1e-3


@pytest.mark.gpu
def test_set_lr_refused_for_captured_torch_adam(cuda, monkeypatch):
    import hlhgat.train as train_mod
    monkeypatch.setattr(train_mod, "HIP_ADAM", False)
    step = train_mod.TrainStep(_Tiny().to(cuda), _loss, lr=LR0, graphs=True)
    with pytest.raises(RuntimeError, match="captured"):
        step.set_lr(1e-3)


# ---------------------------------------------------------------------------
# GPU, resume
# ---------------------------------------------------------------------------
def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf)


@pytest.mark.gpu
def test_resume_is_bitwise_the_uninterrupted_run(cuda):
    """(d) 3 steps (the learning rate halves after step 2), save, load into a
    fresh model and TrainStep, 2 more steps == 5 uninterrupted steps."""
    from hlhgat.train import TrainStep
    p_full, o_full, lr_full, _, _, _ = _tiny_run(cuda, graphs=True, n_steps=5)
    _, _, _, _, _, first = _tiny_run(cuda, graphs=True, n_steps=3)
    sd = _roundtrip(first.state_dict())
    assert sd["opt"]["param_groups"][0]["lr"].dtype == torch.float64
    torch.manual_seed(77)
    m = _Tiny().to(cuda)
    step = TrainStep(m, _loss, lr=0.5, weight_decay=WD, graphs=True)
    lr_ptr = step.opt.param_groups[0]["lr"].data_ptr()
    step.load_state_dict(sd)
    assert step.lr == 5e-3 and step.opt.param_groups[0]["lr"].data_ptr() == lr_ptr
    off = 0
    for p in step.params:  # still views of the flat buffer
        assert p.data_ptr() == step.flat.data_ptr() + 4 * off
        off += p.numel()
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(step.opt, patience=0, factor=0.5,
                                                       mode="max")
    sched.step(0.5)  # best so far; the next falling value halves again
    for i in (4, 5):
        step(_data(i).to(cuda))
        if i in METRIC_AFTER:
            sched.step(METRIC_AFTER[i])
    assert step.lr == lr_full == 2.5e-3
    for p, r in zip(m.parameters(), p_full):
        assert torch.equal(p.detach().cpu(), r)
    got = _opt_state(step)
    for k in o_full:
        assert torch.equal(got[k], o_full[k]), k


HEAD_KW = dict(channels=[2], filters=[32], mlp_channels=[32], K=2, keig=15)
SEED = 0x1234_5678_9ABC_DEF1


def _head(cuda, seed):
    import hlhgat
    torch.manual_seed(seed)
    return hlhgat.HL_HGCNN_zinc_dense_int3_pyr(dropout_ratio=0.25, **HEAD_KW).to(cuda).train()


@pytest.mark.gpu
def test_resume_draws_the_uninterrupted_runs_dropout_masks(cuda):
    """(e) A model with a live Dropout(p = 0.25) on the HIP path, eager steps
    (a mask is a function of seed, step and the launch's site; an eager step
    takes the next sites, so the checkpoint carries the site too): the two
    steps after the resume give the losses and parameters of the uninterrupted
    run, bit for bit."""
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    from hlhgat.train import TrainStep
    batch = zinc_like_batch(20, seed=4).to(cuda)

    def l1(out, b):
        return torch.nn.functional.l1_loss(out.view(-1), b.y.view(-1))

    def run(n, step=None):
        fresh_run = step is None
        if fresh_run:
            ops.dropout_manual_seed(SEED)
            step = TrainStep(_head(cuda, 0), l1, lr=1e-3, graphs=False)
        losses = []
        for i in range(n):
            losses.append(float(step(batch)))
            if fresh_run and i == 1:
                step.set_lr(5e-4)
        return losses, step

    full, s_full = run(5)
    assert len(set(full)) == 5
    p_full = [p.detach().clone() for p in s_full.model.parameters()]
    first, s_first = run(3)
    assert first == full[:3]
    sd = _roundtrip(s_first.state_dict())
    assert sd["dropout"][1] == 3  # (seed, step): one advance per step
    ops.dropout_manual_seed(999)  # the state a new process would start with
    fresh = TrainStep(_head(cuda, 5), l1, lr=1e-3, graphs=False)
    fresh.load_state_dict(sd)
    assert ops.dropout_state()[:2] == tuple(sd["dropout"])
    rest, _ = run(2, step=fresh)
    assert rest == full[3:], (rest, full[3:])
    assert fresh.lr == 5e-4
    for p, r in zip(fresh.model.parameters(), p_full):
        assert torch.equal(p.detach(), r)
    ops.check_device_errors()


@pytest.mark.gpu
def test_resume_under_graphs_with_live_dropout_runs_clean(cuda):
    """A graphs=True run with a live HIP Dropout, saved and resumed into a
    fresh TrainStep: the resumed step runs eagerly once, re-captures ONE graph
    and replays it, the dropout step counter goes on from the checkpoint, the
    losses are finite and differ from step to step (fresh masks), and no
    kernel raises the device error word.  The masks after the re-capture are
    not the uninterrupted run's (a captured step bakes in the sites of its
    capture), so nothing here is compared bitwise."""
    import math
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    from hlhgat.train import TrainStep
    batch = zinc_like_batch(20, seed=4).to(cuda)

    def l1(out, b):
        return torch.nn.functional.l1_loss(out.view(-1), b.y.view(-1))

    ops.clear_device_errors()
    ops.dropout_manual_seed(SEED)
    first = TrainStep(_head(cuda, 0), l1, lr=1e-3, graphs=True)
    for _ in range(3):
        first(batch)
    first.set_lr(5e-4)
    sd = _roundtrip(first.state_dict())
    assert sd["dropout"][1] == 3
    ops.dropout_manual_seed(999)
    fresh = TrainStep(_head(cuda, 5), l1, lr=1e-3, graphs=True)
    fresh.load_state_dict(sd)
    losses = [float(fresh(batch)) for _ in range(3)]
    torch.cuda.synchronize()
    assert fresh.stats == {"eager": 1, "replay": 2, "captures": 1}, fresh.stats
    assert all(math.isfinite(v) for v in losses) and len(set(losses)) == 3, losses
    assert ops.dropout_state()[1] == 6 and fresh.lr == 5e-4
    assert float(fresh.opt.state[fresh.master]["step"]) == 6.0
    assert all(bool(torch.isfinite(p).all()) for p in fresh.model.parameters())
    ops.check_device_errors()


def test_load_state_dict_refused_once_torch_adam_is_captured(monkeypatch):
    """HIP_ADAM = False with graphs: opt.load_state_dict would replace the
    state tensors a captured step addresses, so load_state_dict raises once a
    graph exists (here: an entry put into the step's graph table by hand; the
    check runs before anything is touched)."""
    import hlhgat.train as train_mod
    step = train_mod.TrainStep(_Tiny(), _loss, lr=LR0, graphs=False)
    sd = step.state_dict()
    step.load_state_dict(sd)  # nothing captured: fine
    monkeypatch.setattr(step, "_graphs", {("shape",): object()})
    with pytest.raises(RuntimeError, match="captured steps address"):
        step.load_state_dict(sd)
