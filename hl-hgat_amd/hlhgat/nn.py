"""PyG-free building blocks with the reference's module names and semantics.

The reference composes its layers with torch_geometric ``Sequential``,
``BatchNorm`` and ``Linear`` (e.g. lib/Hodge_ST_Model.py:556-567,
lib/Hodge_Cheb_Conv.py:462-465); its checkpoints therefore carry keys such as
``HL_init_conv.module_0.lins.0.weight`` and ``.module_1.module.running_mean``
(verified against HL-HGAT-DEMO/weights/HL_HGAT_Brain.pt).  These classes
reproduce those names so reference state_dicts load unchanged.
"""
from __future__ import annotations

import math
import re
from typing import Callable, List, Sequence, Tuple, Union

import torch
import torch.nn as tnn

__all__ = ["Sequential", "BatchNorm", "Linear", "L1Loss", "MSELoss", "BCEWithLogitsLoss",
           "FocalLoss", "MaskedBCEWithLogitsLoss", "CrossEntropyLoss", "glorot",
           "global_mean_pool", "SimplexDropout", "PESignFlip"]


def glorot(t: torch.Tensor) -> None:
    """torch_geometric.nn.inits.glorot: U(-a, a), a = sqrt(6/(fan_in+fan_out))."""
    if t is not None:
        a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
        with torch.no_grad():
            t.uniform_(-a, a)


class Linear(tnn.Module):
    """torch_geometric.nn.dense.linear.Linear (weight [out, in]); the convs only
    use ``.weight`` (bias=False, weight_initializer='glorot',
    lib/Hodge_Cheb_Conv.py:462-465)."""

    def __init__(self, in_channels: int, out_channels: int, bias: bool = True,
                 weight_initializer: str = "glorot", bias_initializer=None):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.weight_initializer = weight_initializer
        self.weight = tnn.Parameter(torch.empty(out_channels, in_channels))
        if bias:
            self.bias = tnn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        if self.weight_initializer == "glorot":
            glorot(self.weight)
        else:
            tnn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            with torch.no_grad():
                self.bias.zero_()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import linear_blocks
        shp = x.shape
        y = linear_blocks([x.reshape(-1, shp[-1])], self.weight, self.bias)
        return y.view(*shp[:-1], self.out_channels)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, "
                f"bias={self.bias is not None})")


class BatchNorm(tnn.Module):
    """torch_geometric.nn.BatchNorm: BatchNorm1d held as ``.module``."""

    def __init__(self, in_channels: int, eps: float = 1e-5, momentum: float = 0.1,
                 affine: bool = True, track_running_stats: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.module = tnn.BatchNorm1d(in_channels, eps, momentum, affine, track_running_stats)

    def reset_parameters(self) -> None:
        self.module.reset_parameters()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from .ops import batch_norm_act
        return batch_norm_act(x, self.module, relu=False)

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.in_channels})"


_ARROW = re.compile(r"\s*->\s*")

# Activation tap (test infrastructure): while TAP is a dict, every ReLU site
# -- fused into a conv / BatchNorm node or not -- records a copy of its output
# under the nn.ReLU module it stands for, one entry per call in call order.
# The frozen-mask gradient checks (tests/test_frozen_mask_grads.py) rebuild
# the ReLU masks of the HIP forward from it.
TAP = None


def tap(mod, y) -> None:
    if TAP is not None and torch.is_tensor(y):
        TAP.setdefault(mod, []).append(y.detach().clone())


class Abs(tnn.Module):
    """x.abs() as a module (the TSP readout's |B1^T x_t|, lib/Hodge_ST_Model.py:
    848): under TAP its input is recorded, so the gradient gates can freeze
    the signs the HIP forward saw (tests/test_frozen_mask_grads.py)."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        tap(self, x)
        return x.abs()


class L1Loss(tnn.L1Loss):
    """torch.nn.L1Loss (the ZINC training loss) whose mean reduction on ROCm
    tensors runs as one HIP launch each way (ops.l1_loss: the same input
    gradient bit for bit).  CPU tensors and other reductions go to torch."""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (self.reduction == "mean" and input.is_cuda and input.dtype == torch.float32
                and input.shape == target.shape and not target.requires_grad
                and input.numel() > 0):
            from . import ops
            return ops.l1_loss(input, target)
        return super().forward(input, target)


class BCEWithLogitsLoss(tnn.BCEWithLogitsLoss):
    """torch.nn.BCEWithLogitsLoss (the peptides-func and TSP training losses)
    whose unweighted "mean" / "sum" reductions on ROCm fp32 tensors run as one
    HIP launch each way (ops.bce_with_logits; the input gradient in ATen's
    arithmetic) up to FUSED_MAX elements: the forward's fixed-order sum is one
    workgroup, which for a per-edge loss (config 5: 207k logits) waits on
    ~800 dependent loads per lane and loses to ATen's grid reduction
    (measured +0.3 ms per config-5 step).  Weights, pos_weight, CPU tensors,
    "none" and larger inputs go to torch."""

    FUSED_MAX = 16384

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (self.weight is None and self.pos_weight is None
                and self.reduction in ("mean", "sum") and input.is_cuda
                and input.dtype == torch.float32 and input.shape == target.shape
                and not target.requires_grad and 0 < input.numel() <= self.FUSED_MAX):
            from . import ops
            return ops.bce_with_logits(input, target, self.reduction)
        return super().forward(input, target)


class MSELoss(tnn.MSELoss):
    """torch.nn.MSELoss (the brain notebook's training criterion,
    OHBM_DEMO.ipynb) whose "mean" / "sum" reductions on ROCm fp32 tensors run
    as one HIP launch each way (ops.mse_loss) up to BCEWithLogitsLoss.FUSED_MAX
    elements, for that class's reason: the forward is one workgroup.  CPU
    tensors, "none", a target that needs a gradient, unequal (broadcast)
    shapes and larger inputs go to torch."""

    FUSED_MAX = BCEWithLogitsLoss.FUSED_MAX

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (self.reduction in ("mean", "sum") and input.is_cuda and target.is_cuda
                and input.dtype == torch.float32 and target.dtype == torch.float32
                and input.shape == target.shape and not target.requires_grad
                and 0 < input.numel() <= self.FUSED_MAX):
            from . import ops
            return ops.mse_loss(input, target, self.reduction)
        return super().forward(input, target)


def _selection(target: torch.Tensor, mask, ignore_nan: bool):
    """The boolean selection of the masked losses, or None for everything."""
    m = None if mask is None else mask.bool()
    if ignore_nan:
        keep = ~torch.isnan(target)
        m = keep if m is None else m & keep
    return m


def _hip_bce(input, target, mask) -> bool:
    """input / target (/ mask) run on ops.bce_logits_loss."""
    return (input.is_cuda and input.dtype == torch.float32 and input.shape == target.shape
            and target.is_cuda and not target.requires_grad and input.numel() > 0
            and (mask is None or (mask.shape == input.shape and mask.is_cuda
                                  and not mask.requires_grad)))


class MaskedBCEWithLogitsLoss(tnn.Module):
    """BCE with logits over a selection of the elements,

        m = mask.bool() & ~isnan(target)       (ignore_nan=True adds the second half)
        F.binary_cross_entropy_with_logits(input[m], target[m], reduction=reduction)

    with the selection made on the device inside the reduction
    (ops.bce_logits_loss): static shapes, so ``criterion(out, y, mask=mask)``
    captures in hlhgat.train.TrainStep where ``criterion(out[mask], y[mask])``
    (a data-dependent gather) cannot.  Every size runs on HIP, in a fixed
    summation order.  An empty selection gives loss 0 and a zero gradient on
    the HIP path (torch: NaN).  CPU tensors, non-fp32 input and
    reduction="none" go to the torch expression above."""

    def __init__(self, reduction: str = "mean", ignore_nan: bool = False):
        super().__init__()
        self.reduction = reduction
        self.ignore_nan = ignore_nan

    def forward(self, input: torch.Tensor, target: torch.Tensor, mask=None) -> torch.Tensor:
        if self.reduction in ("mean", "sum") and _hip_bce(input, target, mask):
            from . import ops
            return ops.bce_logits_loss(input, target, mask, ignore_nan=self.ignore_nan,
                                       reduction=self.reduction)
        m = _selection(target, mask, self.ignore_nan)
        if m is not None:
            input, target = input[m], target[m]
        return tnn.functional.binary_cross_entropy_with_logits(input, target,
                                                               reduction=self.reduction)


class FocalLoss(tnn.Module):
    """The reference's FocalLoss (lib/Loss_function.py:14-26; the peptides-func
    and TSP objective, main_pepfunc...:179-186, main_TSP...:321), a scalar
    function of the MEAN BCE b:  loss = scale * alpha * (1 - exp(-b))**gamma * b
    with the reference's constructor defaults and scale = 1e4.

    ``criterion(out[mask], y[mask])`` works as in the reference (eager).  The
    capture-safe forms are ``criterion(out, y, mask=mask)`` and
    ``FocalLoss(ignore_nan=True)(out, y)`` (mask = ~isnan(y), taken on the
    device): static shapes, one fixed-order HIP reduction at every size
    (ops.bce_logits_loss).  An empty selection gives loss 0 and a zero
    gradient on the HIP path (torch: NaN).  CPU tensors, non-fp32 input, class
    weights and 0 < gamma < 1 go to the reference's torch expression, which on
    CPU reproduces the reference class exactly."""

    def __init__(self, alpha=0.25, gamma=2, weight=None, scale=1e4, ignore_nan=False):
        super().__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.weight = weight
        self.scale = scale
        self.ignore_nan = ignore_nan
        self.bce_fn = tnn.BCEWithLogitsLoss(weight=self.weight)

    def forward(self, preds: torch.Tensor, labels: torch.Tensor, mask=None) -> torch.Tensor:
        if (self.weight is None and (self.gamma == 0 or self.gamma >= 1)
                and _hip_bce(preds, labels, mask)):
            from . import ops
            return ops.bce_logits_loss(preds, labels, mask, ignore_nan=self.ignore_nan,
                                       focal=(self.alpha, self.gamma, self.scale))
        m = _selection(labels, mask, self.ignore_nan)
        if m is not None:
            preds, labels = preds[m], labels[m]
        logpt = -self.bce_fn(preds, labels)
        pt = torch.exp(logpt)
        loss = -((1 - pt) ** self.gamma) * self.alpha * logpt
        return loss * self.scale


class CrossEntropyLoss(tnn.CrossEntropyLoss):
    """torch.nn.CrossEntropyLoss (the CIFAR10SP training loss,
    main_cifar10SP...:137,203; torch's constructor, e.g.
    ``CrossEntropyLoss(ignore_index=-100, reduction="mean")``) whose "mean" /
    "sum" reductions over fp32 logits [R, C <= 64] and class-index targets on
    ROCm run on HIP (ops.cross_entropy: fixed summation order; all rows
    ignored gives 0, not NaN; a label outside [0, C) raises the device error
    word instead of a device assert).  Class weights, label smoothing,
    class-probability targets, C > 64, "none", other shapes and CPU tensors
    go to torch."""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if (self.weight is None and self.label_smoothing == 0.0
                and self.reduction in ("mean", "sum") and input.is_cuda
                and input.dtype == torch.float32 and input.dim() == 2 and target.dim() == 1
                and target.is_cuda and not target.is_floating_point()
                and target.size(0) == input.size(0) and input.size(0) > 0):
            from . import _lib, ops
            if 1 <= input.size(1) <= _lib.CE_MAX_CLASSES:
                return ops.cross_entropy(input, target, ignore_index=self.ignore_index,
                                         reduction=self.reduction)
        return super().forward(input, target)


def _hip_dropout(m, x) -> bool:
    """m is a live nn.Dropout that runs on the HIP path for the device tensor x
    (ops.dropout); ops.HIP_DROPOUT = False leaves it to ATen."""
    from . import ops
    return (isinstance(m, tnn.Dropout) and m.p > 0.0 and m.training and not m.inplace
            and ops.HIP_DROPOUT and torch.is_tensor(x) and x.is_cuda
            and x.dtype == torch.float32)


def _names(s: str) -> List[str]:
    return [t.strip() for t in s.split(",") if t.strip()]


class Sequential(tnn.Module):
    """torch_geometric.nn.Sequential(input_args, [(callable, 'a, b -> c'), ...]).

    Entry i is registered as ``module_{i}`` (modules and plain callables
    alike), arguments are routed by name, and the value of the last entry is
    returned — e.g. the ``lambda x1, x2: [x1, x2]`` tail of every HL block
    (lib/Hodge_ST_Model.py:566)."""

    def __init__(self, input_args: str,
                 modules: Sequence[Union[Tuple[Callable, str], Callable]]):
        super().__init__()
        self.input_args = _names(input_args)
        self._routes: List[Tuple[List[str], List[str]]] = []
        prev_out = list(self.input_args)
        for i, entry in enumerate(modules):
            if isinstance(entry, (tuple, list)):
                fn, desc = entry
                parts = _ARROW.split(desc)
                ins = _names(parts[0])
                outs = _names(parts[1]) if len(parts) > 1 else list(ins)
            else:
                fn, ins, outs = entry, list(prev_out), list(prev_out[:1])
            if isinstance(fn, tnn.Module):
                self.add_module(f"module_{i}", fn)
            else:
                object.__setattr__(self, f"module_{i}", fn)
            self._routes.append((ins, outs))
            prev_out = outs
        self._n = len(modules)
        # Fusions (same result as the modules in turn):
        #  HodgeConv -> BatchNorm [-> ReLU] on one variable: one C++ node
        #  BatchNorm -> ReLU: one fused HIP BN+ReLU op
        self._fuse = [None] * self._n  # (kind, n_entries_consumed)
        i = 0
        while i < self._n:
            m0 = getattr(self, f"module_{i}")
            r0 = self._routes[i]

            def same_var(j):
                return (j < self._n and len(r0[1]) == 1
                        and self._routes[j][0] == r0[1] and self._routes[j][1] == r0[1])

            if hasattr(m0, "forward_bn") and same_var(i + 1) and isinstance(
                    getattr(self, f"module_{i + 1}"), BatchNorm):
                relu = same_var(i + 2) and isinstance(getattr(self, f"module_{i + 2}"), tnn.ReLU)
                self._fuse[i] = ("conv_bn_relu" if relu else "conv_bn", 3 if relu else 2)
            elif isinstance(m0, BatchNorm) and same_var(i + 1) and isinstance(
                    getattr(self, f"module_{i + 1}"), tnn.ReLU):
                self._fuse[i] = ("bn_relu", 2)
            i += self._fuse[i][1] if self._fuse[i] else 1
        self._split = self._two_chains()

    def _two_chains(self):
        """Index s such that entries [0, s) and [s, n-1) touch disjoint
        variables and entry n-1 joins them (the node / edge chains of every
        HL block, lib/Hodge_ST_Model.py:556-566), else None."""
        if self._n < 3:
            return None
        for s in range(1, self._n - 1):
            if any(self._fuse[j] and j + self._fuse[j][1] > s for j in range(s)):
                continue
            a = set().union(*[set(r[0]) | set(r[1]) for r in self._routes[:s]])
            b = set().union(*[set(r[0]) | set(r[1]) for r in self._routes[s:self._n - 1]])
            if not (a & b):
                last_in = set(self._routes[-1][0])
                if last_in & a and last_in & b:
                    return s
        return None

    def _move_sink(self, i, k, pend) -> None:
        """Entry i is a conv (with the k - 1 entries fused into it) that holds
        a one-shot DenseConcat sink (_hlhgat_out).  When a live Dropout follows
        on the same variable -- directly or after one activation (the
        LeakyReLU blocks) -- the sink moves to the Dropout: the conv writes a
        fresh tensor (the y its fused ReLU saved is never overwritten) and the
        Dropout writes the dropped values straight into the slab column block,
        so DenseConcat.append finds them in place."""
        from . import ops
        conv = getattr(self, f"module_{i}")
        sink = getattr(conv, "_hlhgat_out", None)
        r0 = self._routes[i]
        if sink is None or not ops.HIP_DROPOUT or len(r0[1]) != 1:
            return
        var = r0[1]

        def on_var(j):
            return j < self._n and self._routes[j][0] == var and self._routes[j][1] == var

        j = i + k
        if (on_var(j) and self._fuse[j] is None
                and isinstance(getattr(self, f"module_{j}"), (tnn.ReLU, tnn.LeakyReLU))):
            j += 1
        if on_var(j) and self._fuse[j] is None and _hip_dropout(getattr(self, f"module_{j}"),
                                                                sink):
            conv._hlhgat_out = None
            pend[var[0]] = sink

    def _run(self, env, lo, hi):
        out = None
        pend = {}  # variable -> DenseConcat sink moved from its conv to its live Dropout
        i = lo
        while i < hi:
            ins, outs = self._routes[i]
            fn = getattr(self, f"module_{i}")
            fuse = self._fuse[i]
            if fuse is None:
                if isinstance(fn, tnn.Dropout) and (fn.p == 0.0 or not fn.training):
                    out = env[ins[0]]  # identity: no copy kernel
                elif _hip_dropout(fn, env[ins[0]]):
                    from .ops import dropout
                    out = dropout(env[ins[0]], fn.p, True, out=pend.pop(ins[0], None))
                else:
                    if hasattr(fn, "forward_bn"):
                        self._move_sink(i, 1, pend)
                    out = fn(*[env[n] for n in ins])
                    if isinstance(fn, tnn.ReLU):
                        tap(fn, out)
                i += 1
            elif fuse[0] == "bn_relu":
                from .ops import batch_norm_act
                out = batch_norm_act(env[ins[0]], fn.module, relu=True)
                tap(getattr(self, f"module_{i + 1}"), out)
                i += 2
            else:
                bn = getattr(self, f"module_{i + 1}").module
                self._move_sink(i, fuse[1], pend)
                out = fn.forward_bn(*[env[n] for n in ins], bn=bn,
                                    relu=fuse[0] == "conv_bn_relu")
                if fuse[0] == "conv_bn_relu":
                    tap(getattr(self, f"module_{i + 2}"), out)
                i += fuse[1]
            if len(outs) == 1:
                env[outs[0]] = out
            else:
                for n, v in zip(outs, out):
                    env[n] = v
        return out

    def forward(self, *args):
        if len(args) != len(self.input_args):
            raise TypeError(f"Sequential expects {len(self.input_args)} inputs "
                            f"({', '.join(self.input_args)}), got {len(args)}")
        env = dict(zip(self.input_args, args))
        s = self._split
        dev = next((a.device for a in args if torch.is_tensor(a)), None)
        if s is None or dev is None:
            return self._run(env, 0, self._n)
        from .ops import active_chains, fork
        side_env = dict(env)
        ch = active_chains(dev)
        if ch is not None:
            # the block section's two chains (ops.Chains): the edge half on the
            # side stream, no fork wait and no join
            with torch.cuda.stream(ch.side):
                self._run(side_env, s, self._n - 1)
            self._run(env, 0, s)
            for r in self._routes[s:self._n - 1]:
                for k in r[1]:
                    env[k] = side_env[k]
            return self._run(env, self._n - 1, self._n)
        # node chain on the current stream, edge chain on the side stream
        side_in = [env[n] for r in self._routes[s:self._n - 1] for n in r[0]
                   if n in env and torch.is_tensor(env[n])]
        fork(lambda: self._run(env, 0, s), lambda: self._run(side_env, s, self._n - 1),
             side_inputs=side_in, device=dev)
        for r in self._routes[s:self._n - 1]:
            for k in r[1]:
                env[k] = side_env[k]
        return self._run(env, self._n - 1, self._n)

    def __len__(self) -> int:
        return self._n

    def __getitem__(self, i: int):
        return getattr(self, f"module_{i}")


def run_sequential(seq: tnn.Sequential, blocks) -> torch.Tensor:
    """Run an nn.Sequential of Linear / BatchNorm1d / ReLU / Dropout modules on
    the HIP ops: the first Linear consumes ``blocks`` (a list of tensors whose
    concatenation is its input, e.g. cat[x_s2t, x_t] of NodeEdgeInt,
    lib/Hodge_Cheb_Conv.py:307-308) without materialising the cat, and each
    BatchNorm1d followed by ReLU runs as one fused op."""
    from .ops import batch_norm_act, dropout, linear_blocks
    mods = list(seq)
    h = None
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, tnn.Linear):
            h = linear_blocks(blocks if h is None else [h], m.weight, m.bias)
        elif isinstance(m, tnn.BatchNorm1d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], tnn.ReLU)
            h = batch_norm_act(h, m, relu=relu)
            if relu:
                tap(mods[i + 1], h)
            i += relu
        elif isinstance(m, tnn.Dropout) and (m.p == 0.0 or not m.training):
            pass
        elif h is not None and _hip_dropout(m, h):
            h = dropout(h, m.p, True)
        else:
            h = m(h if h is not None else torch.cat(list(blocks), -1))
            if isinstance(m, tnn.ReLU):
                tap(m, h)
        i += 1
    return h


def _bn_relu_layer(mods, i):
    """mods[i:i+3] is Linear -> training-mode BatchNorm1d -> ReLU."""
    from .ops import sync_bn_group
    return (i + 3 <= len(mods) and isinstance(mods[i], tnn.Linear)
            and isinstance(mods[i + 1], tnn.BatchNorm1d) and isinstance(mods[i + 2], tnn.ReLU)
            and (mods[i + 1].training or not mods[i + 1].track_running_stats)
            and sync_bn_group(mods[i + 1]) is None)


MLP_PAIRS = True  # A/B hook: False = run_mlp_stack runs module by module


def run_mlp_stack(seqs, blocks) -> torch.Tensor:
    """The readout MLP of the heads (consecutive nn.Sequential layers Linear ->
    BatchNorm1d -> ReLU -> Dropout, lib/Hodge_ST_Model.py:589-597): identity
    dropouts dropped, every two consecutive Linear -> BN -> ReLU layers run as
    ONE fused node (ops.mlp2: each Linear + BatchNorm in one launch), the rest
    module by module (run_sequential).  The same arithmetic as running the
    layers one by one."""
    from . import ops
    mods = [m for seq in seqs for m in seq
            if not (isinstance(m, tnn.Dropout) and (m.p == 0.0 or not m.training))]
    h, i = None, 0
    while i < len(mods):
        if MLP_PAIRS and _bn_relu_layer(mods, i) and _bn_relu_layer(mods, i + 3):
            tapping = TAP is not None
            if tapping:
                ops._ext.set_tap(True)
            h = ops.mlp2(blocks if h is None else [h], mods[i:i + 6])
            if tapping:
                hidden = ops._ext.take_tap()
                ops._ext.set_tap(False)
                tap(mods[i + 2], hidden[0])
                tap(mods[i + 5], h)
            i += 6
        else:
            j = i + 1
            while j < len(mods) and not (MLP_PAIRS and _bn_relu_layer(mods, j)
                                         and _bn_relu_layer(mods, j + 3)):
                j += 1
            h = run_sequential(tnn.Sequential(*mods[i:j]), blocks if h is None else [h])
            i = j
    return h


def global_mean_pool(x: torch.Tensor, batch: torch.Tensor, size: int = None) -> torch.Tensor:
    """torch_geometric.nn.global_mean_pool over a sorted batch vector
    (PairData batches are graph-contiguous), on the HIP segment-mean kernel."""
    from .ops import segment_mean
    if size is None:
        size = int(batch.max().item()) + 1 if batch.numel() else 0
    counts = torch.bincount(batch, minlength=size)
    ptr = torch.zeros(size + 1, dtype=torch.int32, device=x.device)
    ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return segment_mean(x, ptr, size)


class SimplexDropout(tnn.Module):
    """The structural augmentation of the TSP training set, on the device and
    under graph replay: TSP_EigPE.get with if_aug=True
    (main_TSP_HL_HGCNN_dense_int3_pyr.py:119-139 == lib/Hodge_Dataset.py:
    690-708) sends a share ``aug_prob`` of the samples through dropout_node
    (:73-97), which drops every simplex whose uniform draw is not above the
    sample's rate ``p + U * jitter`` (the reference: p + U / 2) unless it is on
    the tour (y_loc), filters the Laplacian's COO to the surviving simplices
    without relabelling, and appends the keep mask as a column of x.

    Here the operator keeps its shape: ``forward(batch)`` draws the mask of
    every graph of the batch (ops.simplex_keep: counter-based, on the dropout
    state shared with the feature Dropout, so TrainStep's one advance per step
    serves both and a captured step draws fresh masks on every replay), writes
    it into column ``mask_column`` of ``x_<side>`` in place, binds it to
    ``edge_index_<side>`` (ops.set_row_mask) and rewrites the masked operator
    tables (ops.refresh_row_mask): at most 3 launches, 4 with halo tiles.
    ``protect`` names the batch attribute whose non-zero rows are never dropped
    (None: none).  ``site`` is the module's ordinal k: modules with different
    k draw independent masks.  In eval mode nothing is launched and a mask this
    module bound earlier is unbound, so the unmasked operator runs.  Leaving
    the module off reproduces the shipped training scripts, which never pass
    p.  No parameters, no buffers; CPU tensors raise (no CPU path)."""

    def __init__(self, aug_prob: float = 0.75, p: float = 0.0, jitter: float = 0.5,
                 side: str = "s", protect: Union[str, None] = "y", mask_column: Union[int, None] = 1,
                 site: int = 0):
        super().__init__()
        from .ops import simplex_thresholds
        simplex_thresholds(aug_prob, p, jitter)  # range checks
        if side not in ("s", "t"):
            raise ValueError(f"SimplexDropout: side must be 's' or 't' (got {side!r})")
        if not 0 <= int(site) < (1 << 30):
            raise ValueError(f"SimplexDropout: site {site} out of range")
        self.aug_prob, self.p, self.jitter = float(aug_prob), float(p), float(jitter)
        self.side, self.protect, self.mask_column, self.site = side, protect, mask_column, int(site)

    def extra_repr(self) -> str:
        return (f"aug_prob={self.aug_prob}, p={self.p}, jitter={self.jitter}, side={self.side!r}, "
                f"protect={self.protect!r}, mask_column={self.mask_column}, site={self.site}")

    def mask_of(self, batch) -> Union[torch.Tensor, None]:
        """The mask tensor this module draws into for ``batch`` (None before
        the first training forward on it)."""
        ei = getattr(batch, "edge_index_" + self.side)
        return getattr(ei, "_hlhgat_simplex_masks", {}).get(self.site)

    def forward(self, batch):
        from . import ops
        s = self.side
        x, ei, w = (getattr(batch, k + s, None) for k in ("x_", "edge_index_", "edge_weight_"))
        if not (torch.is_tensor(x) and torch.is_tensor(ei) and torch.is_tensor(w)):
            raise RuntimeError(f"SimplexDropout: the batch needs x_{s}, edge_index_{s} and "
                               f"edge_weight_{s}")
        own = getattr(ei, "_hlhgat_simplex_masks", {}).get(self.site)
        if not self.training:
            bound = getattr(ei, "_hlhgat_row_mask", None)
            if own is not None and bound is not None and bound[0] is own:
                ops.set_row_mask(ei, None)
            return batch
        if not (x.is_cuda and ei.is_cuda and w.is_cuda):
            raise RuntimeError("SimplexDropout: the batch must be on a ROCm device (got "
                               f"{x.device}); the HIP path has no CPU fallback")
        seg = getattr(batch, "seg_ptr_" + s, None)
        if not torch.is_tensor(seg):
            raise RuntimeError(f"SimplexDropout: the batch has no seg_ptr_{s} (hodge_dataset."
                               f"collate builds it from the per-graph row counts)")
        n = x.size(0)
        col = None
        if self.mask_column is not None:
            if x.dim() != 2 or not 0 <= self.mask_column < x.size(1):
                raise RuntimeError(f"SimplexDropout: x_{s} {tuple(x.shape)} has no column "
                                   f"{self.mask_column}")
            col = x[:, self.mask_column]
        prot = None
        if self.protect is not None:
            prot = getattr(batch, self.protect, None)
            if not torch.is_tensor(prot) or prot.numel() != n:
                raise RuntimeError(f"SimplexDropout: batch.{self.protect} must hold one entry per "
                                   f"row of x_{s} ({n})")
            prot = prot.view(n)
        if own is None or own.numel() != n or own.device != x.device:
            if not hasattr(ei, "_hlhgat_simplex_masks"):
                ei._hlhgat_simplex_masks = {}
            own = ei._hlhgat_simplex_masks[self.site] = torch.empty(n, device=x.device,
                                                                   dtype=torch.float32)
        ops.simplex_keep(seg, own, self.aug_prob, self.p, self.jitter, self.site, protect=prot,
                         column=col)
        ops.set_row_mask(ei, own)
        ops.refresh_row_mask(ei, w, n)
        return batch


class PESignFlip(tnn.Module):
    """The sign-flip augmentation of the eigenvector positional encoding, on
    the device and under graph replay.  Every stored dataset of the reference
    multiplies the PE columns of x_t and of x_s by fresh random signs in
    ``get()``, per sample and per access (lib/Hodge_Dataset.py:425-440 ZINC,
    :554-569 and :635-650 peptides, :869-881 CIFAR10SP: ``x[:, :dim] *
    cat([ones(n_fixed), -1 + 2 * randint(0, 2, (keig,))])``).

    ``forward(x_t, x_s, batch)`` returns the flipped ``(y_t, y_s)`` of widths
    ``node_dim + keig`` and ``edge_dim + keig`` (the head constructors'
    arguments; ``keig=None`` keeps every stored column): one launch for both
    sides (ops.pe_flip), out of place, so the caller's batch is never
    modified.  One sign per (graph, side, PE column), read off
    ``batch.seg_ptr_t`` / ``batch.seg_ptr_s``; padding rows of a static-shape
    batch are copied.  The draw is counter-based on the dropout state shared
    with the feature Dropout and SimplexDropout, so TrainStep's one advance
    per step serves all three and a captured step draws fresh signs on every
    replay.  ``site`` is the module's ordinal k: modules with different k draw
    independent signs.  The heads that take PE columns carry a ``pe_flip``
    slot (None by default) and apply the module to their feature views first
    thing in ``forward``.

    In eval mode the inputs are returned as they are and nothing is launched.
    The reference's validation and test sets flip too (they run the same
    ``get()``), but eigenvector signs are arbitrary: the stored signs are as
    valid a draw as any, and evaluation stays deterministic.  No parameters,
    no buffers, no state_dict keys; CPU tensors raise in training mode (no
    CPU path)."""

    def __init__(self, node_dim: int, edge_dim: int, keig: Union[int, None] = None,
                 site: int = 0):
        super().__init__()
        from .ops import PE_MAX_WIDTH, PE_SITES
        for name, v in (("node_dim", node_dim), ("edge_dim", edge_dim)):
            if not 0 <= int(v) <= PE_MAX_WIDTH:
                raise ValueError(f"PESignFlip: {name} {v} out of range")
        if keig is not None and not (0 <= int(keig) and int(keig) + max(int(node_dim), int(edge_dim))
                                     <= PE_MAX_WIDTH):
            raise ValueError(f"PESignFlip: keig {keig} out of range")
        if not 0 <= int(site) < PE_SITES:
            raise ValueError(f"PESignFlip: site {site} out of range")
        self.node_dim, self.edge_dim = int(node_dim), int(edge_dim)
        self.keig = None if keig is None else int(keig)
        self.site = int(site)

    def extra_repr(self) -> str:
        return (f"node_dim={self.node_dim}, edge_dim={self.edge_dim}, keig={self.keig}, "
                f"site={self.site}")

    def widths(self, x_t: torch.Tensor, x_s: torch.Tensor) -> Tuple[int, int]:
        """(PE columns flipped on x_t, on x_s)."""
        out = []
        for s, x, fixed in (("t", x_t, self.node_dim), ("s", x_s, self.edge_dim)):
            k = x.size(1) - fixed if self.keig is None else self.keig
            if x.dim() != 2 or k < 0 or x.size(1) < fixed + k:
                raise RuntimeError(f"PESignFlip: x_{s} {tuple(x.shape)} has fewer than {fixed} + "
                                   f"{max(k, 0)} columns (the packers fix the PE width when a "
                                   f"dataset is built)")
            out.append(k)
        return out[0], out[1]

    def forward(self, x_t: torch.Tensor, x_s: torch.Tensor, batch):
        if not self.training:
            return x_t, x_s
        from . import ops
        if not (x_t.is_cuda and x_s.is_cuda):
            raise RuntimeError("PESignFlip: the batch must be on a ROCm device (got "
                               f"{x_t.device}); the HIP path has no CPU fallback")
        seg_t, seg_s = getattr(batch, "seg_ptr_t", None), getattr(batch, "seg_ptr_s", None)
        if not (torch.is_tensor(seg_t) and torch.is_tensor(seg_s)):
            raise RuntimeError("PESignFlip: the batch has no seg_ptr_t / seg_ptr_s (hodge_dataset."
                               "collate builds them from the per-graph row counts)")
        k_t, k_s = self.widths(x_t, x_s)
        return ops.pe_flip(x_t, seg_t, self.node_dim, k_t, x_s, seg_s, self.edge_dim, k_s,
                           site=self.site)
