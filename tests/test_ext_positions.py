"""Argument position -> autograd edge mapping of the composite C++ nodes
(csrc/torch_ext.cpp: conv_bn, bn_act, linear, mlp2, nei_value), away from its
default: every tensor argument that can require grad is frozen in turn, and
each optional one is dropped once.

A backward that reads needs_input_grad at a wrong position, or returns a
gradient in a wrong slot, shows only when the positions and the edges differ,
i.e. when an argument is frozen or absent; with everything requiring grad the
two numberings agree.  Freezing one argument must leave every other gradient
bit for bit what the all-grad run gives (the fused and the separate Linear
gradient launches agree bitwise, test_fused_linear_backward_bitwise).

One ZINC-like graph of three molecules; feature widths 5..18 with at least one
side of every GEMM no multiple of 4 (the row-strided paths).
"""
import functools
import types

import pytest
import torch

from conftest import close
from oracle import hodge_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@functools.lru_cache(None)
def _graph():
    from hlhgat.synthetic import zinc_like_batch
    return zinc_like_batch(3, seed=11)


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bn(C, seed, affine=True):
    bn = torch.nn.BatchNorm1d(C, affine=affine)
    if affine:
        with torch.no_grad():
            bn.weight.copy_(1.0 + _rand(C, seed=seed, scale=0.2))
            bn.bias.copy_(_rand(C, seed=seed + 1, scale=0.3))
    return bn.to(DEV).train()


def _wv(cin, dl, dv, seed):
    """Linear -> BN -> ReLU -> Linear -> BN -> ReLU (a NodeEdgeInt WV_* MLP)."""
    torch.manual_seed(seed)
    nn = torch.nn
    seq = nn.Sequential(nn.Linear(cin, dl), nn.BatchNorm1d(dl), nn.ReLU(), nn.Linear(dl, dv),
                        nn.BatchNorm1d(dv), nn.ReLU())
    with torch.no_grad():
        for i, m in enumerate((seq[1], seq[4])):
            m.weight.copy_(1.0 + _rand(m.num_features, seed=seed + 10 + i, scale=0.2))
            m.bias.copy_(_rand(m.num_features, seed=seed + 20 + i, scale=0.3))
    return seq.to(DEV).train()


# Each problem returns (leaves, run): the tensors that can require grad by
# name, fresh on every call (BatchNorm running statistics move), and a
# function giving the list of outputs.
def _conv(bn=False, bias=True):
    from hlhgat import ops
    b = _graph()
    n = b.x_t.shape[0]
    op = ops.hodge_operator(ops.mark_hodge(b.edge_index_t.to(DEV)), b.edge_weight_t.to(DEV), n)
    leaves = {"x": _rand(n, 6, seed=1).to(DEV)}
    for k in range(3):
        leaves[f"w{k}"] = _rand(10, 6, seed=2 + k, scale=0.3).to(DEV)
    if bias:
        leaves["bias"] = _rand(10, seed=5).to(DEV)
    mod = _bn(10, seed=6) if bn else None
    if bn:
        leaves.update({"bn.weight": mod.weight, "bn.bias": mod.bias})

    def run():
        return [ops.hodge_poly_conv(leaves["x"], op, [leaves[f"w{k}"] for k in range(3)],
                                    leaves.get("bias"), ops.POLY_LAGUERRE, bn=mod, relu=bn)]
    return leaves, run


def _bn_act(affine=True):
    from hlhgat import ops
    n = _graph().x_t.shape[0]
    mod = _bn(18, seed=8, affine=affine)
    leaves = {"x": _rand(n, 18, seed=7, scale=2.0).to(DEV)}
    leaves.update(dict(mod.named_parameters()))
    return leaves, lambda: [ops.batch_norm_act(leaves["x"], mod, relu=True)]


def _linear(bias=True):
    from hlhgat import ops
    n = _graph().x_s.shape[0]
    leaves = {f"a{i}": _rand(n, w, seed=30 + i).to(DEV) for i, w in enumerate((8, 6, 5))}
    leaves["weight"] = _rand(10, 19, seed=33, scale=0.3).to(DEV)
    if bias:
        leaves["bias"] = _rand(10, seed=34).to(DEV)
    return leaves, lambda: [ops.linear_blocks([leaves["a0"], leaves["a1"], leaves["a2"]],
                                              leaves["weight"], leaves.get("bias"))]


def _mlp2():
    from hlhgat import ops
    n = _graph().x_t.shape[0]
    seq = _wv(14, 12, 10, seed=40)
    leaves = {"a0": _rand(n, 6, seed=41).to(DEV), "a1": _rand(n, 8, seed=42).to(DEV)}
    leaves.update(dict(seq.named_parameters()))
    return leaves, lambda: [ops.mlp2([leaves["a0"], leaves["a1"]], seq)]


def _nei(sink=False, packed=False):
    """sink: x_t's gradient goes to a DenseConcat-style slab view (gsink for
    the node side only); packed: the first-Linear weights come prepacked."""
    import hlhgat
    from hlhgat import ops
    b = _graph()
    N, E, d = b.x_t.shape[0], b.x_s.shape[0], 10
    inc = hlhgat.adj2par1(b.edge_index.to(DEV), N, E).incidence()
    rD = ops.reciprocal(R.degree(b.edge_index.reshape(-1), N).to(DEV))
    wv_n, wv_e = _wv(2 * d, 12, 6, seed=50), _wv(2 * d, 12, 6, seed=51)
    leaves = {"x_t": _rand(N, d, seed=52).to(DEV), "x_s": _rand(E, d, seed=53).to(DEV)}
    leaves.update({"n." + k: p for k, p in wv_n.named_parameters()})
    leaves.update({"e." + k: p for k, p in wv_e.named_parameters()})
    slab = torch.full((N, d + 4), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32)

    def run():
        pk = None
        if packed:
            m = types.SimpleNamespace(WV_Node=wv_n, WV_Edge=wv_e)
            ops.nei_prepack([m])
            pk = ops.take_pack(m)
            assert pk is not None
        r = ops.nei_value(leaves["x_t"], leaves["x_s"], inc, rD, wv_n, wv_e,
                          gsink=((slab[:, :d], flag), None) if sink else (None, None), packed=pk)
        assert r is not None
        return list(r)
    run.slab, run.flag = slab, flag
    return leaves, run


_MLP = ["0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias", "4.weight", "4.bias"]
NODES = {
    "conv": (_conv, {}, ["x", "w0", "w1", "w2", "bias"]),
    "conv_bn": (_conv, {"bn": True}, ["x", "w0", "w1", "w2", "bias", "bn.weight", "bn.bias"]),
    "bn_act": (_bn_act, {}, ["x", "weight", "bias"]),
    "linear": (_linear, {}, ["a0", "a1", "a2", "weight", "bias"]),
    "mlp2": (_mlp2, {}, ["a0", "a1"] + _MLP),
    "nei": (_nei, {}, ["x_t", "x_s"] + ["n." + k for k in _MLP] + ["e." + k for k in _MLP]),
}


def _grads(make, freeze=None, **kw):
    leaves, run = make(**kw)
    for k, t in leaves.items():
        t.requires_grad_(k != freeze)
    outs = run()
    sum((o * _rand(*o.shape, seed=90 + i).to(DEV)).sum() for i, o in enumerate(outs)).backward()
    torch.cuda.synchronize()
    return {k: t.grad for k, t in leaves.items()}, [o.detach() for o in outs], run


@functools.lru_cache(None)
def _all_grad(node):
    """Every gradient of the node's problem with everything requiring grad."""
    make, kw, names = NODES[node]
    grads, outs, _ = _grads(make, None, **kw)
    assert sorted(grads) == sorted(names)
    assert all(g is not None for g in grads.values())
    return grads, outs


@pytest.mark.parametrize("node,frozen", [(n, k) for n, v in NODES.items() for k in v[2]])
def test_freeze_one_argument(cuda, node, frozen):
    make, kw, names = NODES[node]
    ref, ref_out = _all_grad(node)
    got, out, _ = _grads(make, frozen, **kw)
    assert got[frozen] is None
    for o, r in zip(out, ref_out):
        assert torch.equal(o, r), (node, frozen, "output")
    for k in names:
        if k != frozen:
            assert got[k] is not None and torch.equal(got[k], ref[k]), (node, frozen, k)


def test_conv_without_bias(cuda):
    b = _graph()
    got, out, _ = _grads(_conv, None, bias=False)
    assert "bias" not in got
    cpu = {k: v.detach().cpu().requires_grad_(True) for k, v in _conv(bias=False)[0].items()}
    ref = R.laguerre_conv(cpu["x"], b.edge_index_t, b.edge_weight_t,
                          [cpu[f"w{k}"] for k in range(3)], None)
    close(out[0].cpu(), ref.detach(), 1e-5, "out")
    (ref * _rand(*ref.shape, seed=90)).sum().backward()
    for k in cpu:
        close(got[k].cpu(), cpu[k].grad, 1e-4, "grad " + k)


def test_linear_blocks_without_bias(cuda):
    got, out, _ = _grads(_linear, None, bias=False)
    assert "bias" not in got
    cpu = {k: v.detach().cpu().double().requires_grad_(True)
           for k, v in _linear(bias=False)[0].items()}
    ref = torch.cat([cpu["a0"], cpu["a1"], cpu["a2"]], 1) @ cpu["weight"].t()
    close(out[0].cpu(), ref.detach(), 1e-5, "out")
    (ref * _rand(*ref.shape, seed=90).double()).sum().backward()
    for k in cpu:
        close(got[k].cpu(), cpu[k].grad, 1e-4 if k == "weight" else 1e-5, "grad " + k)


def test_batch_norm_act_without_affine(cuda):
    got, out, _ = _grads(_bn_act, None, affine=False)
    assert list(got) == ["x"]
    x = _bn_act(affine=False)[0]["x"].detach().cpu().requires_grad_(True)
    ref = torch.relu(torch.nn.functional.batch_norm(x, None, None, None, None, True, 0.1, 1e-5))
    close(out[0].cpu(), ref.detach(), 1e-5, "y")
    (ref * _rand(*ref.shape, seed=90)).sum().backward()
    close(got["x"].cpu(), x.grad, 1e-4, "dx")


def test_nei_value_gsink_one_side(cuda):
    """The node side's input gradient lands in the slab view (first writer:
    overwrites, sets the flag); the edge side has no sink; nothing else moves."""
    ref, ref_out = _all_grad("nei")
    got, out, run = _grads(_nei, None, sink=True)
    d = ref["x_t"].shape[1]
    assert int(run.flag[0]) == 1
    assert torch.equal(run.slab[:, :d], ref["x_t"]) and torch.isnan(run.slab[:, d:]).all()
    for o, r in zip(out, ref_out):
        assert torch.equal(o, r)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k


def test_nei_value_packed(cuda):
    ref, ref_out = _all_grad("nei")
    got, out, _ = _grads(_nei, None, packed=True)
    for o, r in zip(out, ref_out):
        assert torch.equal(o, r)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
