"""bench.py --dump-outputs / --full (CPU): what dump_outputs writes for a
TrainStep, its size budget, and that the two options reach the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import torch

from conftest import REPO

NAMES = {"loss", "params", "grads", "adam_exp_avg", "adam_exp_avg_sq", "buffers"}


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(5, 7)
        self.bn = torch.nn.BatchNorm1d(7)
        self.b = torch.nn.Linear(7, 1)

    def forward(self, batch):
        return self.b(torch.relu(self.bn(self.a(batch.x))))


class _B:
    def __init__(self, x, y):
        self.x, self.y = x, y


def _run(steps=3):
    """a seeded eager TrainStep on the CPU: (step, last loss)"""
    from hlhgat.train import TrainStep
    torch.manual_seed(0)
    m = _Net().train()
    step = TrainStep(m, lambda o, b: torch.nn.functional.l1_loss(o.view(-1), b.y.view(-1)),
                     lr=1e-2, weight_decay=1e-3, graphs=False)
    g = torch.Generator().manual_seed(1)
    loss = None
    for _ in range(steps):
        loss = step(_B(torch.randn(16, 5, generator=g), torch.randn(16, generator=g)))
    return step, loss


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_arrays(tmp_path):
    """One float32 .npy per output: the loss the step returned, the flat
    parameters and gradients, the Adam moments and the BatchNorm buffers; a
    second run of the same seeded step writes the same arrays."""
    import bench
    step, loss = _run()
    bench.dump_outputs(str(tmp_path / "a"), step, loss)
    got = _load(tmp_path / "a")
    assert set(got) == NAMES
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    n = sum(p.numel() for p in step.model.parameters())
    assert got["params"].shape == got["grads"].shape == got["adam_exp_avg"].shape == (n,)
    assert np.array_equal(got["loss"], loss.reshape(1).numpy())
    assert np.array_equal(got["params"], step.flat.numpy())
    assert np.array_equal(got["grads"], step.flat_grad.numpy())
    assert np.abs(got["grads"]).max() > 0 and np.abs(got["adam_exp_avg_sq"]).max() > 0
    bn = step.model.bn
    assert np.array_equal(got["buffers"], torch.cat([bn.running_mean, bn.running_var]).numpy())
    step2, loss2 = _run()
    bench.dump_outputs(str(tmp_path / "b"), step2, loss2)
    again = _load(tmp_path / "b")
    for k in NAMES:
        assert np.array_equal(got[k], again[k]), k


def test_dump_outputs_budget(tmp_path, monkeypatch):
    """Past the byte budget an array is cut to a fixed, seeded sample of its
    elements (ascending indices), and the whole dump stays within the budget."""
    import bench
    step, loss = _run()
    assert bench.DUMP_BYTES <= 64 * 10**6  # the real budget: 64 MB in all
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * len(NAMES) * 10)  # 10 elements per array
    bench.dump_outputs(str(tmp_path), step, loss)
    got = _load(tmp_path)
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BYTES
    flat = step.flat.numpy()
    idx = np.sort(np.random.RandomState(0).choice(flat.size, 10, replace=False))
    assert np.array_equal(got["params"], flat[idx])
    assert got["loss"].shape == (1,)


def test_bench_cli_takes_full_and_dump_outputs(tmp_path):
    """--full and --dump-outputs are options of the command line (gloo dry
    run, no GPU); --steps is the number of timed steps the line reports and
    the line carries ms_per_step."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--dry-run",
                        "--steps", "3", "--warmup", "1", "--full", "--dump-outputs",
                        str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=240, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] >= 0
