"""CPU emulation of the bf16 matmul precision (hlhgat.set_matmul_precision):
operands rounded to bf16 with round-to-nearest-even, exact products, sums in
fp64.  The numerics contract of include/hlhgat.h (hlhgat_set_gemm_precision):
forward rounds A and W, the data gradient rounds G and W, the weight gradient
rounds G and A; bias and the bias gradient are not rounded."""
import contextlib

import torch


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


def _r64(t: torch.Tensor) -> torch.Tensor:
    """The fp32 value of t rounded to bf16, as fp64 (storage is fp32 on the
    device, so an fp64 reference tensor is brought to fp32 first)."""
    return round_bf16(t.detach().float()).double()


def eligible(in_features: int, out_features: int) -> bool:
    """hlhgat_gemm_bf16_eligible for a contiguous Linear whose operand blocks
    all have a width that divides like in_features."""
    return in_features % 8 == 0 and out_features % 4 == 0


class EmulatedLinear(torch.autograd.Function):
    """y = round(x) round(W)^T + b; dx = round(g) round(W); dW = round(g)^T
    round(x); db = sum g.  Products summed in fp64, results in x's dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        y = _r64(x) @ _r64(weight).t()
        if bias is not None:
            y = y + bias.detach().double()
        return y.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g2 = g.reshape(-1, g.shape[-1])
        x2 = x.reshape(-1, x.shape[-1])
        dx = (_r64(g2) @ _r64(weight)).reshape(x.shape).to(x.dtype)
        dw = (_r64(g2).t() @ _r64(x2)).to(weight.dtype)
        db = g2.double().sum(0).to(g.dtype) if ctx.has_bias else None
        return dx, dw, db


def emulated_linear(x, weight, bias=None):
    return EmulatedLinear.apply(x, weight, bias)


def _nei_forward_projected_first(plain_forward):
    """RefNodeEdgeInt.forward with the value path's first Linear written the
    way the device runs it (ops.nei_value): Linear(cat[mix(a), b]) =
    mix(a W1^T) + b W2^T + bias, the projection BEFORE the |B1| mixing.  The
    same function in exact arithmetic; under bf16 the GEMM operand that gets
    rounded is then a, as on the device, not mix(a)."""
    import torch.nn.functional as F
    from oracle import hodge_ref

    def forward(self, x_t, x_s, par, D):
        if self.only_att:
            return plain_forward(self, x_t, x_s, par, D)
        d = x_t.shape[1]
        lin_t, lin_s = self.WV_Node[0], self.WV_Edge[0]
        p_s2t, p_t2s = hodge_ref.boundary_mix(F.linear(x_t, lin_s.weight[:, :d]),
                                              F.linear(x_s, lin_t.weight[:, :d]), par, D)
        y_t = p_s2t + F.linear(x_t, lin_t.weight[:, d:], lin_t.bias)
        y_s = p_t2s + F.linear(x_s, lin_s.weight[:, d:], lin_s.bias)
        for layer in list(self.WV_Node)[1:]:
            y_t = layer(y_t)
        for layer in list(self.WV_Edge)[1:]:
            y_s = layer(y_s)
        return y_t, y_s

    return forward


@contextlib.contextmanager
def emulate_bf16_linear():
    """The CPU oracle at bf16 matmul precision: every
    torch.nn.functional.linear call (nn.Linear and the oracle's F.linear
    included) whose shape the bf16 kernels would take runs the emulated Linear,
    the others stay fp32, as on the device; and NodeEdgeInt's value path
    places its first GEMM where the device does (before the mixing).  oracle/
    itself is untouched: the hooks are removed on exit."""
    import torch.nn.functional as F
    from oracle import hodge_ref
    plain = F.linear
    plain_nei = hodge_ref.RefNodeEdgeInt.forward

    def linear(x, weight, bias=None):
        if eligible(weight.shape[1], weight.shape[0]) and x.dim() >= 2:
            return emulated_linear(x, weight, bias)
        return plain(x, weight, bias)

    F.linear = linear
    hodge_ref.RefNodeEdgeInt.forward = _nei_forward_projected_first(plain_nei)
    try:
        yield
    finally:
        F.linear = plain
        hodge_ref.RefNodeEdgeInt.forward = plain_nei
