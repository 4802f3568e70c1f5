"""BatchNorm backward in one launch (k_bn_bwd_grid, hlhgat_set_bn_bwd_one_launch)
against the reduction + apply launches: bitwise equality over the layouts the
kernel distinguishes, the hand-over path (wait bound 0), a launch beside a
kernel that holds most CUs, and the captured training step."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO


class _Switch:
    """hlhgat_set_bn_bwd_one_launch for the duration of a with-block."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from hlhgat import _lib
        self.prior = int(_lib.LIB.hlhgat_get_bn_bwd_one_launch())
        _lib.check(_lib.LIB.hlhgat_set_bn_bwd_one_launch(self.on), "set_bn_bwd_one_launch")

    def __exit__(self, *exc):
        from hlhgat import _lib
        _lib.LIB.hlhgat_set_bn_bwd_one_launch(self.prior)


class _Wait:
    """hlhgat_set_bn_wait_us for the duration of a with-block (default after)."""

    def __init__(self, us):
        self.us = us

    def __enter__(self):
        from hlhgat import _lib
        _lib.check(_lib.LIB.hlhgat_set_bn_wait_us(self.us), "set_bn_wait_us")

    def __exit__(self, *exc):
        from hlhgat import _lib
        _lib.LIB.hlhgat_set_bn_wait_us(1000)


def _inputs(cuda, n, C, seed=0):
    g = torch.Generator(device="cpu").manual_seed(n + C + seed)
    x0 = (torch.randn(n, C, generator=g) * 3 + 1).to(cuda)
    R = torch.randn(n, C, generator=g).to(cuda)
    return x0, R


def _forward(cuda, x0, C, relu, valid):
    """A fresh BatchNorm1d (fixed parameters) and its forward through the HIP path."""
    from hlhgat import ops
    torch.manual_seed(0)
    bn = torch.nn.BatchNorm1d(C).to(cuda).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    x = x0.clone().requires_grad_(True)
    y = ops.batch_norm_act(x, bn, relu=relu, valid=valid)
    return bn, x, y


def _grads(cuda, x0, R, C, relu, valid):
    bn, x, y = _forward(cuda, x0, C, relu, valid)
    (y * R).sum().backward()
    return [x.grad, bn.weight.grad, bn.bias.grad], y.detach(), bn


def _ref_dx(x0, R, y, bn, relu, nv):
    """fp64 torch BatchNorm backward over the valid rows.  The ReLU mask is
    taken from the forward output under test (y > 0), as the kernels take it:
    an element whose pre-activation rounds across 0 in fp32 would otherwise
    flip a whole gradient entry and say nothing about the backward."""
    xd = x0[:nv].double().requires_grad_(True)
    w = bn.weight.detach().double()
    b = bn.bias.detach().double()
    z = torch.nn.functional.batch_norm(xd, None, None, w, b, training=True, eps=bn.eps)
    up = R[:nv].double()
    if relu:
        up = up * (y[:nv] > 0)
    z.backward(up)
    return xd.grad


CASES = [
    # n, C, relu, pad (rows of padding) or None
    (33, 6, True, None),        # one partition: its own finaliser; scalar path
    (700, 64, True, None),      # 11 partitions: flat order
    (4097, 6, True, 5),         # 65 partitions: tree, last group of one; scalar path
    (25600, 64, True, 333),     # the bench's layout: 128 partitions
    (25600, 64, True, 22600),   # n_valid = 3000: whole partitions of padding
    (25600, 64, True, 25600),   # n_valid = 0
    (1000, 256, False, None),   # the readout MLP; y absent
    (2048, 320, True, None),    # two column tiles
    (200000, 64, True, None),   # past the grid cap: two launches either way
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,C,relu,pad", CASES)
def test_bn_bwd_one_launch_bitwise(cuda, n, C, relu, pad):
    """dx, dweight and dbias of the one-launch backward == the two launches,
    bit for bit, and dx against an fp64 torch BatchNorm backward to 1e-5 of
    max|dx| (the forward's tolerance in test_bn_one_launch_bitwise)."""
    from hlhgat import ops
    x0, R = _inputs(cuda, n, C)
    valid = None if pad is None else torch.tensor([n - pad], dtype=torch.int32, device=cuda)
    res = []
    for on in (1, 0):
        with _Switch(on):
            res.append(_grads(cuda, x0, R, C, relu, valid))
    (g1, y1, bn), (g0, y0, _) = res
    ops.check_device_errors()
    assert torch.equal(y1, y0)
    for a, b in zip(g1, g0):
        assert torch.equal(a, b)
    nv = n if pad is None else n - pad
    dx = g1[0]
    assert not dx[nv:].any()
    if nv > 0:
        ref = _ref_dx(x0, R, y1, bn, relu, nv)
        scale = float(ref.abs().max())
        err = float((dx[:nv].double() - ref).abs().max())
        print(f"n={n} C={C}: max|dx - fp64| = {err:.3e}, max|dx| = {scale:.3e}")
        assert err <= 1e-5 * scale, (err, scale)
    else:
        assert not g1[1].any() and not g1[2].any()
    ops.check_device_errors()


@pytest.mark.gpu
def test_bn_bwd_one_launch_strided_bitwise(cuda):
    """dx into a 64-column block of a 192-wide buffer and dy as a 64-column
    block of a 128-wide one (the C ABI, as the Linear backward hands them
    over): the same bits from one launch and from two, nothing written outside
    the block."""
    from hlhgat import _lib, ops
    L = _lib.LIB
    n, C = 25600, 64
    x, R = _inputs(cuda, n, C, seed=1)
    g = torch.Generator(device="cpu").manual_seed(5)
    dyb = torch.randn(n, 128, generator=g).to(cuda)
    dy = dyb[:, 64:128]
    w = (torch.rand(C, generator=g) + 0.5).to(cuda)
    b = torch.randn(C, generator=g).to(cuda)
    y = torch.empty(n, C, device=cuda)
    mean, inv = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
    ws = torch.zeros(int(L.hlhgat_bn_workspace_bytes(n, C)), dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(L.hlhgat_bn_fwd_train(x.data_ptr(), C, n, None, C, w.data_ptr(), b.data_ptr(), None,
                                     None, None, 0.1, 1e-5, 1, y.data_ptr(), C, mean.data_ptr(),
                                     inv.data_ptr(), ws.data_ptr(), ws.numel(), st), "bn_fwd")
    outs = []
    for on in (1, 0):
        buf = torch.full((n, 192), 7.0, device=cuda)
        dx = buf[:, 64:128]
        dw, db = torch.empty(C, device=cuda), torch.empty(C, device=cuda)
        with _Switch(on):
            _lib.check(L.hlhgat_bn_bwd_train(x.data_ptr(), C, y.data_ptr(), C, dy.data_ptr(), 128,
                                             n, None, C, w.data_ptr(), mean.data_ptr(),
                                             inv.data_ptr(), dx.data_ptr(), 192, dw.data_ptr(),
                                             db.data_ptr(), ws.data_ptr(), ws.numel(), st),
                       "bn_bwd")
        torch.cuda.synchronize()
        outs.append((buf, dw, db))
    ops.check_device_errors()
    for a, c in zip(*outs):
        assert torch.equal(a, c)
    buf = outs[0][0]
    assert bool((buf[:, :64] == 7.0).all()) and bool((buf[:, 128:] == 7.0).all())
    assert torch.isfinite(buf[:, 64:128]).all() and bool((buf[:, 64:128] != 7.0).any())
    ops.check_device_errors()


@pytest.mark.gpu
def test_bn_bwd_one_launch_handover_bitwise(cuda):
    """Wait bound 0: every workgroup that finds the coefficients not yet
    published hands its rows to the finaliser, which forms their dx from x, dy
    and y in memory: the bits of the two-launch path, give-ups counted and
    logged under kernel id 3, no device error."""
    from hlhgat import ops
    n, C = 25600, 64
    x0, R = _inputs(cuda, n, C)
    valid = torch.tensor([n - 333], dtype=torch.int32, device=cuda)
    with _Switch(0):
        ref, _, _ = _grads(cuda, x0, R, C, True, valid)
    with _Switch(1):
        bn, x, y = _forward(cuda, x0, C, True, valid)
        loss = (y * R).sum()
        ops.bn_giveups_reset()  # synchronises: the forward's own waits are over
        with _Wait(0):
            loss.backward()
            torch.cuda.synchronize()
        gu = ops.bn_giveups()
    ops.check_device_errors()
    for a, b in zip([x.grad, bn.weight.grad, bn.bias.grad], ref):
        assert torch.equal(a, b)
    assert gu["count"] > 0
    assert gu["log"]
    for r in gu["log"]:
        assert r["kernel"] == 3 and r["arrivals"] <= r["total"] and r["outcome"] in (1, 2), r
    ops.check_device_errors()


_HOG = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from hlhgat import _lib
cus = torch.cuda.get_device_properties(0).multi_processor_count
s = torch.cuda.Stream()
_lib.check(_lib.LIB.hlhgat_test_occupy(cus, cus - 64, 140 * 1024, int(sys.argv[2]),
                                       s.cuda_stream), "test_occupy")
print("hog launched", flush=True)
s.synchronize()
print("hog done", flush=True)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("wait_us", [1000, 0])
def test_bn_bwd_one_launch_beside_cu_hog(cuda, wait_us):
    """The one-launch backward launched while another process's kernel holds
    the LDS of all but 64 CUs for 0.6 s (the pattern of
    test_bn_one_launch_beside_cu_hog): it completes long before the hog ends
    with the bits of the undisturbed run; at wait 0 rows are handed over."""
    import subprocess
    import sys
    import time
    from hlhgat import ops
    ops.check_device_errors()
    n, C = 25600, 64
    x0, R = _inputs(cuda, n, C, seed=2)
    with _Switch(1):
        ref, _, _ = _grads(cuda, x0, R, C, True, None)
        bn, x, y = _forward(cuda, x0, C, True, None)
        loss = (y * R).sum()
        ops.bn_giveups_reset()
        usec = 600000
        pkg = os.path.join(REPO, "hl-hgat_amd")
        hog = subprocess.Popen([sys.executable, "-c", _HOG, pkg, str(usec)],
                               stdout=subprocess.PIPE, text=True)
        try:
            assert hog.stdout.readline().strip() == "hog launched"
            time.sleep(0.1)  # the hog's workgroups are resident
            with _Wait(wait_us):
                t0 = time.perf_counter()
                loss.backward()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            gu = ops.bn_giveups()
        finally:
            rest = hog.communicate(timeout=60)[0]
    assert hog.returncode == 0 and "hog done" in rest
    ops.check_device_errors()
    for a, b in zip([x.grad, bn.weight.grad, bn.bias.grad], ref):
        assert torch.equal(a, b)
    print(f"backward beside the hog (wait {wait_us} us): {dt * 1e3:.1f} ms, "
          f"hand-overs {gu['count']}, log {gu['log'][:4]}")
    assert dt < 0.5 * usec * 1e-6, dt
    if wait_us == 0:
        assert gu["count"] > 0
    ops.check_device_errors()


def _train_run(cuda, batch, on, graphs):
    """Three steps of the config-2 model on `batch`; flat parameters, Adam
    moments and (captured) the kernel counts of the step graph."""
    import bench
    import hlhgat
    from hlhgat import ops, train
    from hlhgat.train import TrainStep
    crit = hlhgat.nn.L1Loss()
    keep = train.KEEP_GRAPHS
    train.KEEP_GRAPHS = True
    try:
        with _Switch(on):
            torch.manual_seed(0)
            m = hlhgat.HL_HGCNN_zinc_dense_int3_pyr(**bench.MODEL_KW).to(cuda).train()
            st = TrainStep(m, lambda o, b: crit(o.view(-1, 1), b.y.view(-1, 1)), lr=1e-3,
                           weight_decay=1e-3, graphs=graphs)
            for _ in range(3):
                st(batch)
            torch.cuda.synchronize()
    finally:
        train.KEEP_GRAPHS = keep
    s = st.opt.state[st.master]
    out = {"flat": st.flat.detach().clone(), "m": s["exp_avg"].clone(),
           "v": s["exp_avg_sq"].clone(), "replays": st.stats.get("replay", 0)}
    if graphs:
        k = apply_n = grid_n = 0
        for ent in st._graphs.values():
            h = ent.graph.raw_cuda_graph()
            k += ops.graph_kernel_count(h, "k_bn_bwd_apply")[0]
            apply_n += ops.graph_kernel_count(h, "k_bn_bwd_apply")[1]
            grid_n += ops.graph_kernel_count(h, "k_bn_bwd_grid")[1]
        out.update(kernels=k, apply=apply_n, grid=grid_n)
    return out


@pytest.mark.gpu
def test_bn_bwd_one_launch_captured_step(cuda):
    """The config-2 model on 8 graphs, three optimiser steps: parameters and
    Adam moments with the one-launch backward == with the two launches, bit
    for bit, eager and replayed; the captured step holds no k_bn_bwd_apply
    and is shorter by exactly the BatchNorm backwards that took the new
    kernel."""
    from hlhgat import ops
    from hlhgat.synthetic import zinc_like_batch
    batch = zinc_like_batch(8, seed=3).to(cuda)
    runs = {(on, gr): _train_run(cuda, batch, on, gr) for on in (1, 0) for gr in (False, True)}
    ops.check_device_errors()
    base = runs[(0, False)]
    for key, r in runs.items():
        for f in ("flat", "m", "v"):
            assert torch.equal(r[f], base[f]), (key, f)
    on, off = runs[(1, True)], runs[(0, True)]
    assert on["replays"] > 0 and off["replays"] > 0
    assert on["apply"] == 0 and on["grid"] > 0
    assert off["grid"] == 0 and off["apply"] > 0
    assert off["kernels"] - on["kernels"] == on["grid"]
    ops.check_device_errors()


def test_bn_bwd_one_launch_exports():
    """The switch is declared, exported and bound with the declared
    signatures, and the setter round-trips through the getter."""
    import torch  # noqa: F401  (shares the HIP runtime, as the product does)
    from hlhgat import _lib
    src = open(os.path.join(REPO, "include", "hlhgat.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+hlhgat_set_bn_bwd_one_launch\s*\(\s*int\s+on\s*\)\s*;", src)
    assert re.search(r"\bint\s+hlhgat_get_bn_bwd_one_launch\s*\(\s*void\s*\)\s*;", src)
    assert _lib.SIGNATURES["hlhgat_set_bn_bwd_one_launch"] == (ctypes.c_int32, [ctypes.c_int32])
    assert _lib.SIGNATURES["hlhgat_get_bn_bwd_one_launch"] == (ctypes.c_int32, [])
    L = _lib.LIB
    assert L.hlhgat_version() >= 104
    prior = int(L.hlhgat_get_bn_bwd_one_launch())
    try:
        for v in (0, 1, 0):
            assert L.hlhgat_set_bn_bwd_one_launch(v) == 0
            assert L.hlhgat_get_bn_bwd_one_launch() == v
        # the common switch is independent of this one
        assert L.hlhgat_get_bn_one_launch() in (0, 1)
    finally:
        L.hlhgat_set_bn_bwd_one_launch(prior)
    assert L.hlhgat_get_bn_bwd_one_launch() == prior
