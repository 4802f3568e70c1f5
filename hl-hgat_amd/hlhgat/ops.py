"""Torch-facing wrappers and autograd Functions over the HIP C-ABI.

Every op here runs a kernel from libhlhgat.so on the caller's current HIP
stream; there is no CPU or eager-PyTorch fallback (tensors must live on a ROCm
device, fp32, with the documented layouts).  The reference semantics each op
reproduces are cited per function (paths relative to deepika090/HL-HGAT).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
import weakref
from dataclasses import dataclass
from typing import Tuple, List, Optional, Sequence

import torch

from . import _lib
from ._lib import LIB, check

try:  # C++ autograd nodes over the same C-ABI (hl-hgat_amd/csrc/torch_ext.cpp)
    from . import _hlhgat_ext as _ext
except ImportError as e:  # pragma: no cover - the build always produces it
    raise ImportError(f"hlhgat: torch extension _hlhgat_ext missing ({e}); run the build "
                      f"(make -C hl-hgat_amd/csrc)") from e

__all__ = [
    "SparseCSR", "HodgeOperator", "Incidence", "hodge_operator", "incidence",
    "mark_hodge", "set_row_mask", "refresh_row_mask", "simplex_keep",
    "spmm", "poly_basis", "hodge_poly_conv", "linear_blocks", "mlp2", "nei_value",
    "batch_norm_act", "check_device_errors", "clear_device_errors", "device_errors",
    "node_from_edges", "edge_from_nodes", "incidence_mm", "att_score", "segment_mean",
    "temporal_conv", "leaky_maxpool_time", "time_readout", "dropout",
    "TimeSeriesMap", "time_series_map", "time_series_pack", "temporal_conv_ragged",
    "leaky_maxpool_time_ragged", "time_readout_ragged",
    "pe_flip", "pe_signs",
    "bce_logits_loss", "cross_entropy", "mse_loss", "average_precision",
    "collect_rows", "f1_per_graph", "argmax_correct", "regression_summary",
    "fc_prepare", "fc_dense", "fc_edges", "fc_pair_table", "FcPrepared", "mlgc_device",
    "POLY_LAGUERRE", "POLY_CHEB", "POLY_LAGUERRE_DEMO", "SIGMA_SIGMOID", "SIGMA_RELU",
]

POLY_LAGUERRE, POLY_CHEB = _lib.POLY_LAGUERRE, _lib.POLY_CHEB
POLY_LAGUERRE_DEMO = _lib.POLY_LAGUERRE_DEMO
SIGMA_SIGMOID, SIGMA_RELU = _lib.SIGMA_SIGMOID, _lib.SIGMA_RELU


# ----------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------
def _stream(t: torch.Tensor) -> int:
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _req_dev(t: torch.Tensor, name: str, dtype=torch.float32) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"hlhgat: {name} must be on a ROCm device (got {t.device}); "
                           f"the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise RuntimeError(f"hlhgat: {name} must be {dtype} (got {t.dtype})")


def _rows2d(t: torch.Tensor, name: str) -> torch.Tensor:
    """Row-major 2-D view with unit inner stride (copy only if needed)."""
    if t.dim() != 2:
        raise RuntimeError(f"hlhgat: {name} must be 2-D (got {tuple(t.shape)})")
    if t.stride(1) != 1 or t.stride(0) < t.size(1):
        t = t.contiguous()
    return t


def _ld(t: torch.Tensor) -> int:
    return max(t.stride(0), t.size(1), 1)


def _arr(ctype, vals):
    return (ctype * len(vals))(*vals)


# ----------------------------------------------------------------------------
# node / edge chain concurrency
# ----------------------------------------------------------------------------
# Every HL block runs two independent chains — the node side on L0 and the edge
# side on L1 (lib/Hodge_ST_Model.py:556-566, lib/Hodge_Cheb_Conv.py:307-308).
# At ZINC scale each launch is latency-bound and fills a fraction of the 256
# CUs, so the edge chain is issued on a second HIP stream and the two overlap.
# Autograd replays each node's backward on the stream its forward used, so the
# backward chains overlap too; captured into a hipGraph the fork/join becomes
# two graph branches.
_SIDE_STREAMS = {}
# HLHGAT_STREAM_FORK=0: every chain on one stream (diagnosis / A-B)
_FORK_ENABLED = os.environ.get("HLHGAT_STREAM_FORK", "1") != "0"


def set_stream_fork(enabled: bool) -> None:
    """Enable / disable issuing the edge chain on a second stream."""
    global _FORK_ENABLED
    _FORK_ENABLED = bool(enabled)


_OWN_STREAMS = {}


def own_stream(device, role: str, cu_mask=None, priority: int = 0) -> torch.cuda.Stream:
    """A HIP stream of this library's own for `role` on `device` (created
    once, non-blocking, never from torch's stream pool).  torch.cuda.Stream()
    hands out its 32 pool streams round-robin, so two unrelated users can get
    the same stream -- e.g. a user's copy stream and a side stream that has
    joined a graph capture, whose uploads would then be captured.  The capture,
    copy and side streams of TrainStep / StagedFeed / the chains are these.
    Created by libhlhgat (hlhgat_stream_create), i.e. by the HIP runtime torch
    loaded.  cu_mask (a list of 32-bit words, bit c = CU c): the stream runs on
    those CUs only (the first call for a role fixes its mask); priority: HIP
    stream priority (lower = higher; 0 = default)."""
    idx = device.index if getattr(device, "index", None) is not None else (
        device if isinstance(device, int) else torch.cuda.current_device())
    s = _OWN_STREAMS.get((idx, role))
    if s is None:
        import ctypes
        h = ctypes.c_void_p()
        if cu_mask:
            words = (ctypes.c_uint32 * len(cu_mask))(*[int(w) & 0xffffffff for w in cu_mask])
            check(LIB.hlhgat_stream_create(idx, 1, 0, words, len(cu_mask), ctypes.byref(h)),
                  "stream_create")
        else:
            check(LIB.hlhgat_stream_create(idx, 1, int(priority), None, 0, ctypes.byref(h)),
                  "stream_create")
        s = torch.cuda.ExternalStream(h.value, device=torch.device("cuda", idx))
        _OWN_STREAMS[(idx, role)] = s
    return s


def cu_mask_high(n_on: int, n_cu: int):
    """A CU mask (32-bit words covering n_cu CUs) with the n_on
    highest-numbered CUs set."""
    words = (n_cu + 31) // 32
    mask = [0] * words
    for c in range(n_cu - n_on, n_cu):
        mask[c // 32] |= 1 << (c % 32)
    return mask


def stream_cu_mask(stream, words: int = 8):
    """The CU mask `stream` runs on (a list of 32-bit words)."""
    import ctypes
    buf = (ctypes.c_uint32 * words)()
    check(LIB.hlhgat_stream_cu_mask(stream.cuda_stream, buf, words), "stream_cu_mask")
    return list(buf)


def side_stream(device: torch.device, slot: int = 0) -> torch.cuda.Stream:
    """Side stream `slot` of the device (0: the edge chains; 1: batch
    preparation that overlaps the first conv)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    s = _SIDE_STREAMS.get((idx, slot))
    if s is None:
        s = own_stream(idx, f"side{slot}")
        _SIDE_STREAMS[(idx, slot)] = s
    return s


def join_capture_streams(device: torch.device) -> int:
    """Make the capturing current stream wait for every side stream (the C++
    fork's and ops.side_stream's) that joined its capture -- the last
    operation of a hipGraph capture (hlhgat.train.TrainStep)."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    extra = [s.cuda_stream for (d, _), s in _SIDE_STREAMS.items() if d == idx]
    return int(_ext.join_capture_streams(idx, extra))


def side_streams_capturing(device: torch.device) -> List[int]:
    """raw handles of the side streams still part of an active capture"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    cand = [s.cuda_stream for (d, _), s in _SIDE_STREAMS.items() if d == idx]
    cand.append(int(_ext.fork_side_stream(idx)))
    return [h for h in cand if _ext.stream_capturing(h)]


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _tensors(v)


_CHAIN = None  # the active Chains, or None
CHAINS_ENABLED = True  # A/B hook: False = a fork / join per HL block


class Chains:
    """The node and edge chains of a model's HL blocks on two streams for the
    whole block section of a forward, instead of a fork / join per block
    (lib/Hodge_ST_Model.py:608-633: each block's node and edge convs are
    independent; only NodeEdgeInt exchanges features between them).

    Inside ``with Chains(device) as ch:`` a two-chain Sequential (an HL block)
    runs its edge half on the side stream without waiting for the main stream
    and without a join, and the fused NodeEdgeInt keeps its edge MLP on the
    side stream (torch_ext.cpp chain mode): the exchange of the two
    first-layer GEMM results is the only cross-stream dependency per block.
    Entering makes the side stream wait for the main stream (the batch, the
    slabs, the weight packs); ``ch.sync_side()`` does so again (e.g. after
    tables built on the main stream); leaving joins the side stream into the
    main stream.  Values are unchanged (the same kernels in the same order on
    each stream).  A cross-stream hazard of a hipGraph capture is caught the
    same way as for ``fork``: the side stream is joined before capture end."""

    def __init__(self, device, enabled: bool = True):
        self.device = device
        self.on = (enabled and CHAINS_ENABLED and _FORK_ENABLED and device is not None
                   and device.type == "cuda" and _ext is not None)

    def __enter__(self):
        global _CHAIN
        if self.on:
            if _CHAIN is not None:
                raise RuntimeError("hlhgat: Chains do not nest")
            self.main = torch.cuda.current_stream(self.device)
            # the C++ fork's side stream: the fused NodeEdgeInt's edge half runs
            # there, so the edge convs must too (one edge stream, no syncs between)
            idx = (self.device.index if self.device.index is not None
                   else torch.cuda.current_device())
            self.side = torch.cuda.ExternalStream(int(_ext.fork_side_stream(idx)),
                                                  device=self.device)
            self.side.wait_stream(self.main)
            _CHAIN = self
            _ext.set_chain(True)
        return self

    def sync_side(self) -> None:
        if self.on:
            self.side.wait_stream(self.main)

    def side_context(self):
        """Issue (and record for autograd) on the edge chain's stream."""
        return torch.cuda.stream(self.side) if self.on else contextlib.nullcontext()

    def to_main(self, *ts):
        """Side-chain tensors handed to the main stream after the join."""
        if self.on:
            for t in _tensors(ts):
                t.record_stream(self.main)
        return ts if len(ts) != 1 else ts[0]

    def __exit__(self, *exc):
        global _CHAIN
        if self.on:
            _ext.set_chain(False)
            _CHAIN = None
            self.main.wait_stream(self.side)
        return False


def active_chains(device):
    """The active Chains on `device`, or None."""
    ch = _CHAIN
    if ch is None or device is None or ch.device != device:
        return None
    return ch


def fork(fn_main, fn_side, side_inputs=(), device=None, slot=0):
    """Run fn_main() on the current stream and fn_side() on the side stream
    concurrently; returns (fn_main(), fn_side()) with the side results ordered
    before anything issued next on the current stream.  Tensors in
    side_inputs (produced on the current stream) are kept alive for the side
    stream's use."""
    if not _FORK_ENABLED or device is None or device.type != "cuda":
        return fn_main(), fn_side()
    main = torch.cuda.current_stream(device)
    side = side_stream(device, slot)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        for t in _tensors(side_inputs):
            t.record_stream(side)
        out_side = fn_side()
    out_main = fn_main()
    main.wait_stream(side)
    for t in _tensors(out_side):
        t.record_stream(main)
    return out_main, out_side


# ----------------------------------------------------------------------------
# sparse operators (CSR) and their per-batch cache
# ----------------------------------------------------------------------------
@dataclass
class SparseCSR:
    rowptr: torch.Tensor  # int32 [n_rows+1]
    col: torch.Tensor     # int32 [nnz]
    val: Optional[torch.Tensor]  # fp32 [nnz] or None (= ones)
    n_rows: int
    n_cols: int
    nnz: int
    order: Optional[torch.Tensor] = None  # int32 [n_rows] row schedule (locality_order)
    valid: Optional[torch.Tensor] = None  # int32 [1]: rows >= valid are static-shape padding
    # halo tiles (tile_ptr, halo_ptr, halo, lcol, max_halo) for the LDS-staged
    # SpMM of large Laplacians (hodge_dataset.halo_tiles; hlhgat_halo_t)
    halo: Optional[tuple] = None


@dataclass
class HodgeOperator:
    """A Laplacian as used by propagate: fwd = CSR keyed by edge_index[1]
    (Y[t] = sum w * X[s]), bwd = its transpose (keyed by edge_index[0]).
    ``factor`` (an L1 = alpha B1^T B1 declared by set_hodge_factor): the 7
    tensors of hlhgat_hodge_factor_t and the node count; the polynomial
    bases then run factored (hlhgat_poly_basis_*_factored)."""
    fwd: SparseCSR
    bwd: SparseCSR
    factor: Optional[tuple] = None
    factor_nodes: int = 0
    # a row-masked view (set_row_mask): (the unmasked operator, the mask, the
    # halo tiles' entry permutation or None); val / sval / the factor's sign
    # and alpha tables are then the masked buffers
    masked_from: Optional[tuple] = None


@dataclass
class Incidence:
    """|B1| of adj2par1 (lib/Hodge_Dataset.py:169-191) for edge_index [2, E]:
    per-node CSR over incident edge ids (ascending) plus the edge list."""
    rowptr: torch.Tensor    # int32 [n_nodes+1]
    edge_ids: torch.Tensor  # int32 [2E]
    edge_index: torch.Tensor  # int64 [2, E] contiguous
    n_nodes: int
    n_edges: int


class _IdCache:
    """Cache keyed on a tensor object's identity + version (entries die with
    the tensor), so a freed-and-reused allocation can never hit stale CSR."""

    def __init__(self):
        self._d = {}

    def get(self, key_tensors: Sequence[torch.Tensor], extra):
        k = (tuple(id(t) for t in key_tensors), extra)
        hit = self._d.get(k)
        if hit is None:
            return None
        versions, value = hit
        if versions != tuple(t._version for t in key_tensors):
            return None
        return value

    def put(self, key_tensors: Sequence[torch.Tensor], extra, value):
        k = (tuple(id(t) for t in key_tensors), extra)
        self._d[k] = (tuple(t._version for t in key_tensors), value)
        for t in key_tensors:
            weakref.finalize(t, self._d.pop, k, None)
        return value

    def clear(self):
        self._d.clear()


_HODGE_CACHE = _IdCache()
_INC_CACHE = _IdCache()
_RCP_CACHE = _IdCache()


def clear_caches() -> None:
    _HODGE_CACHE.clear()
    _INC_CACHE.clear()
    _RCP_CACHE.clear()


def reciprocal(D: torch.Tensor) -> torch.Tensor:
    """(1 / D).view(-1) (lib/Hodge_Cheb_Conv.py:294), computed once per D
    tensor: every NodeEdgeInt of a block group divides by the same degrees.
    Gradients do not flow into D (the reference's D is an integer count)."""
    if D.requires_grad:
        return (1 / D).view(-1)
    pre = getattr(D, "_hlhgat_rcp", None)  # built with the batch (hodge_dataset.node_degree)
    if pre is not None and pre.shape == D.shape and pre.device == D.device:
        return pre.view(-1)
    hit = _RCP_CACHE.get([D], None)
    if hit is not None:
        return hit
    return _RCP_CACHE.put([D], None, (1 / D).view(-1))


def mark_hodge(edge_index: torch.Tensor) -> torch.Tensor:
    """Declare that edge_index/edge_weight describe a symmetric operator whose
    COO is sorted by (row, col) — true for every Laplacian the Hodge builder
    emits via dense_to_sparse (lib/Hodge_Dataset.py:455-456,467-468) and for
    PairData batches of them (block-diagonal, offsets :40-48).  Enables the
    sort-free CSR build and reuse of one CSR for forward and adjoint."""
    edge_index._hlhgat_sorted_symmetric = True  # type: ignore[attr-defined]
    return edge_index


def set_row_order(edge_index: torch.Tensor, order: torch.Tensor) -> torch.Tensor:
    """Attach a row schedule (a permutation of the operator's rows, e.g.
    hodge_dataset.locality_order) to a Laplacian's edge_index: every SpMM /
    polynomial-basis launch over the operator built from it visits rows in
    that order (same results, better L2 locality on large graphs)."""
    edge_index._hlhgat_row_order = order.to(device=edge_index.device,  # type: ignore
                                            dtype=torch.int32).contiguous()
    return edge_index


def set_valid(edge_index: torch.Tensor, n_valid: torch.Tensor, attr: str = "_hlhgat_valid"
              ) -> torch.Tensor:
    """Declare the rows >= n_valid (device int32 [1]) of the operator built
    from edge_index as static-shape padding (hodge_dataset.pad_batch): the
    BatchNorm statistics of its layers use the valid rows only."""
    setattr(edge_index, attr, n_valid.to(device=edge_index.device, dtype=torch.int32).view(1))
    return edge_index


def set_halo(edge_index: torch.Tensor, ht: dict) -> torch.Tensor:
    """Attach halo tiles (hodge_dataset.halo_tiles, built for this operator's
    CSR and row schedule) to a sorted symmetric Laplacian's edge_index: its
    SpMM / polynomial steps then stage each tile's entries and neighbour rows
    in LDS (k_poly_halo; bitwise the same results)."""
    dev = edge_index.device
    i32 = lambda k: ht[k].to(dev, torch.int32).contiguous()  # noqa: E731
    edge_index._hlhgat_halo = (  # type: ignore[attr-defined]
        i32("halo_tile_ptr"), i32("halo_ptr"), i32("halo"), i32("halo_srp"),
        ht["halo_lcol"].to(dev, torch.int16).contiguous(), i32("halo_eperm"),
        [int(v) for v in ht["halo_bounds"]], i32("halo_hdr"))
    return edge_index


# Factored L1 (hlhgat_hodge_factor_t): on for the operators collate declares
# (hodge_dataset.hodge_factor_ok: exact identity, >= FACTOR_MIN_ROW entries per
# row); HLHGAT_FACTOR=0 keeps the bitwise CSR path everywhere.
FACTOR_ENABLED = os.environ.get("HLHGAT_FACTOR", "1") != "0"


def set_hodge_factor(edge_index_s: torch.Tensor, edge_index: torch.Tensor, n_nodes: int,
                     node_order: Optional[torch.Tensor] = None,
                     tables: Optional[tuple] = None) -> torch.Tensor:
    """Declare that the L1 built from (edge_index_s, edge_weight_s) equals
    alpha_e * B1^T B1 with B1 the boundary of ``edge_index`` ([2, E], i < j,
    adj2par1 lib/Hodge_Dataset.py:169-191) on n_nodes nodes -- exactly, as
    every L1 of the Hodge builder is (lib/Hodge_Dataset.py:451-456); the
    caller has checked it (hodge_dataset.hodge_factor_ok).  Polynomial bases
    over it then gather ~4 rows per edge instead of nnz/E (hlhgat.h).
    ``tables`` = (alpha [E] f32, signs [2E] f32 in incidence-CSR order,
    ends [E, 2] int32) built at collate time (hodge_dataset.factor_tables):
    the operator then takes them instead of building them on the device (in
    a captured step, every replay)."""
    edge_index_s._hlhgat_factor = (edge_index, int(n_nodes), node_order,  # type: ignore
                                   tables)
    return edge_index_s


def has_hodge_factor(edge_index_s: torch.Tensor) -> bool:
    """Whether set_hodge_factor declared this L1 (its polynomial bases then
    take the factored path when FACTOR_ENABLED)."""
    return getattr(edge_index_s, "_hlhgat_factor", None) is not None


def _build_factor(op: "HodgeOperator", ei_s: torch.Tensor, w: torch.Tensor, decl) -> None:
    """The device tensors of hlhgat_hodge_factor_t for op (no host sync)."""
    edge_index, n_nodes, node_order, tables = decl
    E = op.fwd.n_rows
    if edge_index.size(1) != E:
        raise RuntimeError(f"hlhgat: hodge factor: B1 has {edge_index.size(1)} edges, "
                           f"L1 has {E} rows")
    inc = incidence(edge_index, n_nodes)
    dev = ei_s.device
    if tables is not None:  # collate-time tables: no device work here
        alpha, signs, ends = tables
        if (alpha.numel() != E or signs.numel() != 2 * E or tuple(ends.shape) != (E, 2)
                or alpha.device != dev or signs.device != dev or ends.device != dev):
            raise RuntimeError("hlhgat: hodge factor tables do not match the operator "
                               f"({alpha.numel()}, {signs.numel()}, {tuple(ends.shape)}; E={E})")
    else:
        diag = ei_s[0] == ei_s[1]
        alpha = torch.zeros(E, device=dev, dtype=torch.float32)
        alpha.index_put_((ei_s[0],), torch.where(diag, w * 0.5, torch.zeros_like(w)),
                         accumulate=True)
        signs = _incidence_signs(inc)
        ends = edge_index.t().to(torch.int32).contiguous()
    none_i = torch.empty(0, dtype=torch.int32, device=dev)
    no = (node_order.to(dev, torch.int32).contiguous() if node_order is not None else none_i)
    eo = op.fwd.order if op.fwd.order is not None else none_i
    op.factor = (inc.rowptr, inc.edge_ids, signs, no, ends, alpha, eo)
    op.factor_nodes = int(n_nodes)


def _attach_halo(a: "SparseCSR", halo) -> None:
    """A.halo = (tile_ptr, halo_ptr, halo, srp, lcol, sval, bounds); sval =
    the CSR values in schedule order, gathered on device once per operator."""
    tp, hp, hc, srp, lcol, eperm, bounds, hdr = halo
    if lcol.numel() != a.nnz:
        raise RuntimeError("hlhgat: halo tiles were built for a different operator")
    sval = None
    if a.val is not None and a.nnz:
        sval = torch.empty_like(a.val)
        check(LIB.hlhgat_gather_f32(a.val.data_ptr(), eperm.data_ptr(), a.nnz,
                                    sval.data_ptr(), _stream(a.val)), "gather_f32")
    a.halo = (tp, hp, hc, srp, lcol, sval, bounds, hdr)


def _halo_desc(A: "SparseCSR"):
    """ctypes pointer to an hlhgat_halo_t for A, or None."""
    if A.halo is None:
        return None
    tp, hp, hc, srp, lc, sval, (mh, mr, mn), hdr = A.halo
    d = _lib.HaloDesc(hdr.data_ptr(), tp.data_ptr(), hp.data_ptr(), hc.data_ptr(), srp.data_ptr(),
                      lc.data_ptr(), _ptr(sval), tp.numel() - 1, mh, mr, mn)
    return C.pointer(d)


def _halo_args(A: "SparseCSR"):
    """The halo arguments of the C++ conv node (Nones when A has none)."""
    if A.halo is None:
        return (None, None, None, None, None, None, [0, 0, 0], None)
    return A.halo


_CHECK_SIZES = os.environ.get("HLHGAT_CHECK_SIZES", "0") == "1"


def hodge_build(edge_index: torch.Tensor, node_counts, lmax: Optional[torch.Tensor] = None,
                steps: int = 64, sizes=None):
    """Hodge Laplacians of a block-diagonal batch ON DEVICE (hlhgat_hodge_*):
    edge_index int64 [2, E] (i < j, PairData offsets), node_counts per graph.
    lmax per graph: given (float, as the reference's eigh result) or computed
    by the on-device Lanczos (fp64, min(n, steps) steps, 1 <= steps <= 1024).
    A graph with n <= steps nodes gets lmax to fp64 rounding.  At the default
    64 steps the kNN graphs of the workloads (k = 8 .. 25, any size, edge
    dropout included), molecule-like trees up to ~450 nodes and grids up to
    20 x 20 stay within 2e-6 relative of a dense fp64 eigh (kNN and those
    grids within ~1e-14); slowly mixing graphs do not -- a path or a long ring
    is off by ~1e-4, a 30 x 30 grid by 2e-6 -- and need steps ~ n (steps =
    min(n, 1024) gives 1e-7 or better on them).  The result never exceeds
    the true lmax.  Returns (ei_t, w_t, ei_s, w_s, lmax) with
    the COO in the reference's dense_to_sparse order (row-major, zeros
    dropped) and entries fl(fl(2 v) / lmax) (lib/Hodge_Dataset.py:451-468).
    sizes = (N, nnz(L0), nnz(L1)) when the caller knows them (nnz(L0) = the
    non-isolated nodes + 2 E, nnz(L1) = sum deg^2 - E): then nothing here
    waits on the device (HLHGAT_CHECK_SIZES=1 compares them with the device's
    own row sizes).  Sizes that do not fit the graph never write past the
    buffers: the build kernels raise HLHGAT_DEVERR_HODGE_SIZE instead
    (check_device_errors reports it)."""
    _req_dev(edge_index, "edge_index", torch.int64)
    dev = edge_index.device
    counts = torch.as_tensor(node_counts, dtype=torch.int64).to(dev)
    B = counts.numel()
    node_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    node_ptr[1:] = torch.cumsum(counts, 0)
    N = int(sizes[0]) if sizes is not None else int(node_ptr[-1].item())
    ei = edge_index.contiguous()
    E = ei.size(1)
    inc = incidence(ei, N)
    st = _stream(ei)
    if lmax is None:
        wsb = int(LIB.hlhgat_hodge_lmax_workspace_bytes(N, steps))
        ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
        lam64 = torch.empty(B, dtype=torch.float64, device=dev)
        check(LIB.hlhgat_hodge_lmax(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr() if E else None,
                                    ei.data_ptr() if E else None, E, N, node_ptr.data_ptr(), B,
                                    steps, lam64.data_ptr(), ws.data_ptr(), wsb, st), "hodge_lmax")
        lam = lam64.to(torch.float32)
    else:
        lam = torch.as_tensor(lmax, dtype=torch.float32).to(dev).reshape(B)
    lam_node = torch.repeat_interleave(lam, counts, output_size=N).contiguous()
    sz0 = torch.empty(N, dtype=torch.int32, device=dev)
    sz1 = torch.empty(E, dtype=torch.int32, device=dev)
    check(LIB.hlhgat_hodge_row_sizes(inc.rowptr.data_ptr(), _ptr(ei) if E else None, E, N,
                                     sz0.data_ptr(), sz1.data_ptr(), st), "hodge_row_sizes")
    rp0 = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    rp1 = torch.zeros(E + 1, dtype=torch.int32, device=dev)
    rp0[1:] = torch.cumsum(sz0, 0)
    rp1[1:] = torch.cumsum(sz1, 0)
    if sizes is not None:
        nnz0, nnz1 = int(sizes[1]), int(sizes[2])
        if _CHECK_SIZES:
            got = (int(node_ptr[-1].item()), int(rp0[-1].item()), int(rp1[-1].item()))
            if got != (N, nnz0, nnz1):
                raise RuntimeError(f"hlhgat: hodge_build sizes {tuple(sizes)} != device {got}")
    else:
        nnz0, nnz1 = int(rp0[-1].item()), int(rp1[-1].item())
    # caller's sizes: zero-filled, so entries past the device's rows (sizes
    # too large: HLHGAT_DEVERR_HODGE_SIZE) hold in-range column 0, never garbage
    alloc = torch.empty if sizes is None else torch.zeros
    c0 = alloc(max(nnz0, 1), dtype=torch.int32, device=dev)
    v0 = alloc(max(nnz0, 1), dtype=torch.float32, device=dev)
    c1 = alloc(max(nnz1, 1), dtype=torch.int32, device=dev)
    v1 = alloc(max(nnz1, 1), dtype=torch.float32, device=dev)
    # the kernels check every row against these capacities (a caller's sizes
    # that do not fit the graph raise HLHGAT_DEVERR_HODGE_SIZE, nothing past
    # the buffers is written)
    check(LIB.hlhgat_hodge_build(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr() if E else None,
                                 _ptr(ei) if E else None, E, N, lam_node.data_ptr(), rp0.data_ptr(),
                                 c0.data_ptr(), v0.data_ptr(), nnz0,
                                 rp1.data_ptr(), c1.data_ptr(), v1.data_ptr(),
                                 nnz1, st), "hodge_build")

    def coo(rp, c, v, n, nnz):
        if sizes is not None:
            # a caller's nnz may not match the device's rows (then the build
            # raised HLHGAT_DEVERR_HODGE_SIZE): the row of entry k by binary
            # search over the clamped row pointers -- repeat_interleave with an
            # output_size other than the sum of the repeats trips torch's
            # device-side assert, a GPU exception that ends the process's context
            rp = rp.clamp(max=nnz)
            k = torch.arange(nnz, device=dev, dtype=torch.int32)
            rows = torch.searchsorted(rp[1:], k, right=True).clamp_(max=max(n - 1, 0))
        else:
            rows = torch.repeat_interleave(torch.arange(n, device=dev), (rp[1:] - rp[:-1]).long(),
                                           output_size=nnz)
        return torch.stack([rows, c[:nnz].long()]), v[:nnz]

    ei_t, w_t = coo(rp0, c0, v0, N, nnz0)
    ei_s, w_s = coo(rp1, c1, v1, E, nnz1)
    return ei_t, w_t, ei_s, w_s, lam


def eig_pe(edge_index: torch.Tensor, node_counts, k: int, max_nodes: Optional[int] = None,
           n_nodes: Optional[int] = None):
    """Eigenvector PE of every graph of a block-diagonal batch and its
    lambda_max, on the device in one launch (hlhgat_eig_pe; the reference's
    per-sample eig_pe(L0) and eigh(L0).max(), lib/Hodge_Dataset.py:97-112,
    :782): edge_index int64 [2, E] (i < j, PairData offsets), node_counts per
    graph (a host sequence, or a device tensor with max_nodes given; n_nodes,
    their sum, spares a device read).  With device counts the host cannot
    check max_nodes: a graph larger than it gets zero pe rows and lmax 0, and
    the kernel raises HLHGAT_DEVERR_EIGPE_SIZE (check_device_errors).
    Returns (pe float32 [N, k - 1]: eigenvectors 1 .. k-1 of each graph's L0,
    ascending, zero columns past a graph's own size; lmax float64 [B])."""
    _req_dev(edge_index, "edge_index", torch.int64)
    dev = edge_index.device
    if torch.is_tensor(node_counts) and node_counts.is_cuda:
        if max_nodes is None:
            raise ValueError("eig_pe: max_nodes is required with device node counts")
        counts = node_counts.to(torch.int64)
        N = None if n_nodes is None else int(n_nodes)
    else:
        host = [int(c) for c in node_counts]
        mx = max(host) if host else 0
        if max_nodes is not None and int(max_nodes) < mx:
            raise ValueError(f"eig_pe: max_nodes {max_nodes} < largest graph {mx}")
        max_nodes = mx if max_nodes is None else int(max_nodes)
        counts = torch.tensor(host, dtype=torch.int64).to(dev)
        N = sum(host)
    B = counts.numel()
    node_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    node_ptr[1:] = torch.cumsum(counts, 0)
    if N is None:
        N = int(node_ptr[-1].item())
    ei = edge_index.contiguous()
    E = ei.size(1)
    inc = incidence(ei, N)
    pe = torch.empty(N, k - 1, dtype=torch.float32, device=dev)
    lmax = torch.empty(B, dtype=torch.float64, device=dev)
    wsb = int(LIB.hlhgat_eig_pe_workspace_bytes(B, int(max_nodes), k))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_eig_pe(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr() if E else None,
                            ei.data_ptr() if E else None, E, N, node_ptr.data_ptr(), B,
                            int(max_nodes), k, pe.data_ptr(), k - 1, lmax.data_ptr(), ws.data_ptr(),
                            wsb, _stream(ei)), "eig_pe")
    return pe, lmax


def _counts_ptr(counts, bound, dev, what):
    """(ptr int64 [B + 1] on dev, bound) of host or device per-graph counts,
    by eig_pe's rules: a device tensor needs the bound given."""
    if torch.is_tensor(counts) and counts.is_cuda:
        if bound is None:
            raise ValueError(f"eig_pe_edges: max_edges is required with device {what} counts")
        c = counts.to(torch.int64)
    else:
        host = [int(x) for x in counts]
        mx = max(host) if host else 0
        if bound is not None and int(bound) < mx:
            raise ValueError(f"eig_pe_edges: max_edges {bound} < largest graph {mx}")
        bound = mx if bound is None else int(bound)
        c = torch.tensor(host, dtype=torch.int64).to(dev)
    ptr = torch.zeros(c.numel() + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(c, 0)
    return ptr, bound


def eig_pe_edges(edge_index: torch.Tensor, node_counts, edge_counts, k: int,
                 max_edges: Optional[int] = None, n_nodes: Optional[int] = None):
    """Edge-side eigenvector PE of every graph of a block-diagonal batch in one
    launch (hlhgat_eig_pe_edges; the molecular datasets' eig_pe(L1),
    lib/Hodge_Dataset.py:458, :587): edge_index int64 [2, E] (i < j, PairData
    offsets, edges grouped by graph), node_counts / edge_counts per graph
    (host sequences, or device tensors with max_edges given; n_nodes, the sum
    of the node counts, spares a device read).  With device edge counts a graph
    with more than max_edges edges gets zero rows and the kernel raises
    HLHGAT_DEVERR_EIGPE_SIZE (check_device_errors).  Returns pe float32
    [E, k - 1]: eigenvectors 1 .. k-1 of each graph's L1 = B1^T B1, ascending,
    zero columns past a graph's own edge count."""
    _req_dev(edge_index, "edge_index", torch.int64)
    dev = edge_index.device
    ei = edge_index.contiguous()
    E = ei.size(1)
    edge_ptr, max_edges = _counts_ptr(edge_counts, max_edges, dev, "edge")
    if torch.is_tensor(node_counts) and node_counts.is_cuda:
        node_ptr, _ = _counts_ptr(node_counts, 0, dev, "node")
        N = int(node_ptr[-1].item()) if n_nodes is None else int(n_nodes)
    else:
        host = [int(c) for c in node_counts]
        node_ptr, _ = _counts_ptr(host, None, dev, "node")
        N = sum(host)
    B = edge_ptr.numel() - 1
    if node_ptr.numel() != B + 1:
        raise ValueError("eig_pe_edges: node_counts and edge_counts differ in length")
    inc = incidence(ei, N)
    # rows the kernel does not own (edges past edge_ptr[-1]) stay zero
    pe = torch.zeros(E, k - 1, dtype=torch.float32, device=dev)
    wsb = int(LIB.hlhgat_eig_pe_edges_workspace_bytes(B, int(max_edges), k))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_eig_pe_edges(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr() if E else None,
                                  ei.data_ptr() if E else None, E, N, node_ptr.data_ptr(),
                                  edge_ptr.data_ptr(), B, int(max_edges), k, pe.data_ptr(), k - 1,
                                  ws.data_ptr(), wsb, _stream(ei)), "eig_pe_edges")
    return pe


def mlgc_device(edge_index: torch.Tensor, node_ptr: torch.Tensor, edge_ptr: torch.Tensor,
                perm: torch.Tensor, weight: Optional[torch.Tensor] = None, one_way: bool = False,
                prune_single: bool = False, drop_isolated: bool = False):
    """One MLGC level for a whole batch on the device, in one launch
    (hlhgat_mlgc_device: the graclus visit loop, the fine -> coarse maps and
    MLGC_Weight's pruning passes; lib/Hodge_Dataset.py:252-275, HL-HGAT-DEMO/
    lib/Hodge_Dataset.py:193-241) -- hodge_dataset.mlgc_batch_flat (and
    mlgc_prune) bit for bit.  edge_index int64 [2, E] (i < j, PairData
    offsets; its cached incidence CSR gives the neighbour lists), node_ptr /
    edge_ptr int64 [G + 1] and perm int64 [N] (local ids per graph) on the
    device, weight float64 [E] or None (ones).  one_way: the matching sees an
    edge from its first end only (MLGC_Weight).  Nothing is read back.
    Returns a hodge_dataset.MLGCBatch of device tensors: c_node float32 [N],
    c_edge float32 [E], ce int64 [2, E] (graph g's local coarse edges at the
    head of its edge slot), cn / cm int64 [G].  Edges or perm entries outside
    their graph raise HLHGAT_DEVERR_MLGC_RANGE (check_device_errors)."""
    from .hodge_dataset import MLGCBatch
    _req_dev(edge_index, "edge_index", torch.int64)
    _req_dev(node_ptr, "node_ptr", torch.int64)
    _req_dev(edge_ptr, "edge_ptr", torch.int64)
    _req_dev(perm, "perm", torch.int64)
    if weight is not None:
        _req_dev(weight, "weight", torch.float64)
    dev = edge_index.device
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise RuntimeError(f"hlhgat: edge_index must be [2, E] (got {tuple(edge_index.shape)})")
    G = node_ptr.numel() - 1
    if G < 0 or edge_ptr.numel() != G + 1:
        raise RuntimeError("hlhgat: mlgc_device: node_ptr and edge_ptr must both have G + 1 entries")
    N, E = perm.numel(), edge_index.size(1)
    if weight is not None and weight.numel() != E:
        raise RuntimeError(f"hlhgat: mlgc_device: weight has {weight.numel()} entries, expected {E}")
    inc = incidence(edge_index, N)
    ei = inc.edge_index
    node_ptr, edge_ptr, perm = node_ptr.contiguous(), edge_ptr.contiguous(), perm.contiguous()
    weight = None if weight is None else weight.contiguous()
    c_node = torch.empty(N, dtype=torch.float32, device=dev)
    c_edge = torch.empty(E, dtype=torch.float32, device=dev)
    ce = torch.zeros(2, E, dtype=torch.int64, device=dev)
    cn = torch.empty(G, dtype=torch.int64, device=dev)
    cm = torch.empty(G, dtype=torch.int64, device=dev)
    wsb = int(LIB.hlhgat_mlgc_device_workspace_bytes(N, E, G))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    flags = ((_lib.MLGC_ONE_WAY if one_way else 0) | (_lib.MLGC_PRUNE_SINGLE if prune_single else 0)
             | (_lib.MLGC_DROP_ISOLATED if drop_isolated else 0))
    check(LIB.hlhgat_mlgc_device(G, node_ptr.data_ptr(), edge_ptr.data_ptr(), inc.rowptr.data_ptr(),
                                 inc.edge_ids.data_ptr() if E else None,
                                 ei.data_ptr() if E else None, E, N, _ptr(weight),
                                 perm.data_ptr() if N else None, flags,
                                 c_node.data_ptr() if N else None, c_edge.data_ptr() if E else None,
                                 ce.data_ptr() if E else None, cn.data_ptr(), cm.data_ptr(),
                                 ws.data_ptr(), wsb, _stream(ei)), "mlgc_device")
    return MLGCBatch(node_ptr, edge_ptr, c_node, c_edge, ce, cn, cm)


def copy_words_batched(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor]) -> None:
    """dst.copy_(src) for contiguous same-size tensors whose byte size is a
    multiple of 4, up to HLHGAT_MAX_COPY_BLOCKS per launch
    (hlhgat_copy2d_batched over 4-byte words), on the current stream."""
    n = len(srcs)
    for i in range(0, n, _lib.MAX_COPY_BLOCKS):
        ss, ds = srcs[i:i + _lib.MAX_COPY_BLOCKS], dsts[i:i + _lib.MAX_COPY_BLOCKS]
        words = [t.numel() * t.element_size() // 4 for t in ss]
        m = len(ss)
        check(LIB.hlhgat_copy2d_batched(
            m, _arr(C.c_void_p, [t.data_ptr() for t in ss]), _arr(C.c_int64, words),
            _arr(C.c_void_p, [t.data_ptr() for t in ds]), _arr(C.c_int64, words),
            _arr(C.c_int64, [1] * m), _arr(C.c_int64, words), _stream(ds[0])), "copy2d_batched")


def _factor_args(op: "HodgeOperator"):
    """The factor arguments of the C++ conv node ([] = CSR path)."""
    if op.factor is None:
        return ([], 0)
    return (list(op.factor), op.factor_nodes)


def _factor_desc(op: "HodgeOperator"):
    nr, ne, ns, no, ends, alpha, eo = op.factor
    return C.pointer(_lib.HodgeFactorDesc(
        nr.data_ptr(), ne.data_ptr() if ne.numel() else None, ns.data_ptr() if ns.numel() else None,
        no.data_ptr() if no.numel() else None, op.factor_nodes, ends.data_ptr(),
        alpha.data_ptr(), eo.data_ptr() if eo.numel() else None, op.fwd.n_rows))


def hodge_spmm(op: "HodgeOperator", X: torch.Tensor) -> torch.Tensor:
    """Y = L1 X through the factorisation (op must carry one; no autograd)."""
    if op.factor is None:
        raise RuntimeError("hlhgat: hodge_spmm needs a factored operator (set_hodge_factor)")
    X = _rows2d(X, "X")
    Y = torch.empty(op.fwd.n_rows, X.size(1), device=X.device, dtype=X.dtype)
    work = torch.empty(int(LIB.hlhgat_hodge_factor_work_floats(op.factor_nodes, X.size(1))),
                       device=X.device)
    check(LIB.hlhgat_hodge_spmm(_factor_desc(op), X.data_ptr(), _ld(X), X.size(1), Y.data_ptr(),
                                _ld(Y), work.data_ptr(), _stream(X)), "hodge_spmm")
    return Y


def _hodge_step(op: "HodgeOperator", X: torch.Tensor, Y: torch.Tensor, *, Z=None, P=None,
                Q=None, alpha=1.0, beta=0.0, gamma=0.0, div=1.0, p=0.0, q=0.0,
                work: Optional[torch.Tensor] = None) -> None:
    """_poly_step with the factored L1 of op (hlhgat_hodge_poly_step)."""
    if work is None:
        work = torch.empty(int(LIB.hlhgat_hodge_factor_work_floats(op.factor_nodes, X.size(1))),
                           device=X.device)
    check(LIB.hlhgat_hodge_poly_step(
        _factor_desc(op), X.data_ptr(), _ld(X), X.size(1), _ptr(Z), _ld(Z) if Z is not None else 0,
        _ptr(P), _ld(P) if P is not None else 0, _ptr(Q), _ld(Q) if Q is not None else 0, alpha,
        beta, gamma, div, p, q, Y.data_ptr(), _ld(Y), work.data_ptr(), _stream(X)),
        "hodge_poly_step")


def _csr_sorted(row: torch.Tensor, col: torch.Tensor, w: Optional[torch.Tensor],
                n_rows: int, n_cols: int) -> SparseCSR:
    nnz = row.numel()
    dev = row.device
    rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    col32 = torch.empty(nnz, dtype=torch.int32, device=dev)
    val = torch.empty(nnz, dtype=torch.float32, device=dev) if w is not None else None
    check(LIB.hlhgat_csr_from_sorted_coo(row.data_ptr(), col.data_ptr(), _ptr(w), nnz,
                                         n_rows, rowptr.data_ptr(), col32.data_ptr(),
                                         _ptr(val), _stream(row)),
          "csr_from_sorted_coo")
    return SparseCSR(rowptr, col32, val, n_rows, n_cols, nnz)


def _csr_general(row: torch.Tensor, col: torch.Tensor, w: Optional[torch.Tensor],
                 n_rows: int, n_cols: int) -> SparseCSR:
    nnz = row.numel()
    dev = row.device
    rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
    col32 = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)[:nnz]
    val = (torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)[:nnz]
           if w is not None else None)
    ws_bytes = int(LIB.hlhgat_csr_workspace_bytes(nnz))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_csr_from_coo(row.data_ptr() if nnz else None,
                                  col.data_ptr() if nnz else None, _ptr(w), nnz, n_rows,
                                  max(n_cols, 1), rowptr.data_ptr(),
                                  col32.data_ptr() if nnz else None, _ptr(val) if nnz else None,
                                  None, ws.data_ptr(), ws_bytes, _stream(row)),
          "csr_from_coo")
    return SparseCSR(rowptr, col32, val, n_rows, n_cols, nnz)


def hodge_operator(edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor],
                   n: int) -> HodgeOperator:
    """CSR pair for PyG propagate over (edge_index, edge_weight) on n nodes.

    propagate (source_to_target, aggr='add', message = norm*x_j,
    lib/Hodge_Cheb_Conv.py:518-519) computes Y[ei[1][e]] += w[e] * X[ei[0][e]],
    i.e. Y = A X with A keyed by ei[1]; its adjoint is keyed by ei[0].  With a
    row mask bound to edge_index (set_row_mask) the operator is M A M: the
    same rowptr / col, masked values."""
    bound = getattr(edge_index, "_hlhgat_row_mask", None)
    if bound is not None:
        return _masked_operator(edge_index, edge_weight, n, bound, refresh=False)
    return _hodge_operator(edge_index, edge_weight, n)


def _hodge_operator(edge_index: torch.Tensor, edge_weight: Optional[torch.Tensor],
                    n: int) -> HodgeOperator:
    _req_dev(edge_index, "edge_index", torch.int64)
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise RuntimeError(f"hlhgat: edge_index must be [2, nnz] (got {tuple(edge_index.shape)})")
    if edge_weight is not None:
        _req_dev(edge_weight, "edge_weight")
        if edge_weight.numel() != edge_index.size(1):
            raise RuntimeError("hlhgat: edge_weight must have one entry per edge")
    keys = [edge_index] + ([edge_weight] if edge_weight is not None else [])
    hit = _HODGE_CACHE.get(keys, n)
    if hit is not None:
        return hit
    ei = edge_index.contiguous()
    w = edge_weight.contiguous() if edge_weight is not None else None
    order = getattr(edge_index, "_hlhgat_row_order", None)
    if order is not None and order.numel() != n:
        raise RuntimeError(f"hlhgat: row schedule has {order.numel()} entries, operator {n} rows")
    valid = getattr(edge_index, "_hlhgat_valid", None)
    if getattr(edge_index, "_hlhgat_sorted_symmetric", False):
        pre = getattr(edge_index, "_hlhgat_csr", None)  # built at collate (set_csr)
        if pre is not None and pre[0].numel() == n + 1 and pre[1].numel() == ei.size(1):
            a = SparseCSR(pre[0], pre[1], w, n, n, ei.size(1))
        else:
            a = _csr_sorted(ei[0], ei[1], w, n, n)
        a.order = order
        a.valid = valid
        halo = getattr(edge_index, "_hlhgat_halo", None)
        if halo is not None:  # built for the COO order = this CSR's entry order
            _attach_halo(a, halo)
        op = HodgeOperator(a, a)
        decl = getattr(edge_index, "_hlhgat_factor", None)
        if decl is not None and FACTOR_ENABLED and w is not None:
            _build_factor(op, ei, w, decl)
    else:
        fwd = _csr_general(ei[1], ei[0], w, n, n)
        bwd = _csr_general(ei[0], ei[1], w, n, n)
        for c in (fwd, bwd):
            c.order = order
            c.valid = valid
        op = HodgeOperator(fwd, bwd)
    return _HODGE_CACHE.put(keys, n, op)


# ----------------------------------------------------------------------------
# Row masks on Hodge operators (simplex dropout, csrc/simplex.hip)
# ----------------------------------------------------------------------------
def set_row_mask(edge_index: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    """Bind a row mask (fp32 [n], non-zero = kept) to a marked (sorted
    symmetric) Laplacian's edge_index: hodge_operator then returns M L M,
    M = diag(mask) -- the operator subgraph(node_mask, edge_index_s,
    edge_weight_s) leaves without relabelling (dropout_node,
    main_TSP_HL_HGCNN_dense_int3_pyr.py:93-95) on the unmasked operator's own
    rowptr / col: its val, the factored L1's sign / alpha tables and the halo
    tiles' sval are masked copies, allocated once per bound mask tensor.  The
    mask is read when the operator is first built and again by every
    refresh_row_mask (after the mask changed in place).  mask = None unbinds."""
    if mask is None:
        if hasattr(edge_index, "_hlhgat_row_mask"):
            del edge_index._hlhgat_row_mask
        return edge_index
    if not getattr(edge_index, "_hlhgat_sorted_symmetric", False):
        raise RuntimeError("hlhgat: set_row_mask needs a sorted symmetric Laplacian "
                           "(mark_hodge); a general operator cannot take a row mask")
    _req_dev(edge_index, "edge_index", torch.int64)
    _req_dev(mask, "mask")
    if mask.dim() != 1 or not mask.is_contiguous() or mask.device != edge_index.device:
        raise RuntimeError(f"hlhgat: mask must be a contiguous 1-D tensor on {edge_index.device} "
                           f"(got {tuple(mask.shape)} on {mask.device})")
    bound = getattr(edge_index, "_hlhgat_row_mask", None)
    if bound is None or bound[0] is not mask:
        edge_index._hlhgat_row_mask = (mask, {})  # type: ignore[attr-defined]
    return edge_index


def refresh_row_mask(edge_index: torch.Tensor, edge_weight: torch.Tensor,
                     n: int) -> HodgeOperator:
    """Rewrite the masked tables of the operator hodge_operator(edge_index,
    edge_weight, n) returns from the bound mask's current values: one launch
    for the CSR values, one for the factor tables of a factored L1, one gather
    for halo tiles; nothing is allocated after the first call.  Returns the
    masked operator."""
    bound = getattr(edge_index, "_hlhgat_row_mask", None)
    if bound is None:
        raise RuntimeError("hlhgat: refresh_row_mask: no mask bound (set_row_mask)")
    return _masked_operator(edge_index, edge_weight, n, bound, refresh=True)


def _masked_operator(edge_index, edge_weight, n: int, bound, refresh: bool) -> HodgeOperator:
    mask, bufs = bound
    if edge_weight is None:
        raise RuntimeError("hlhgat: a row-masked operator needs edge weights")
    if mask.numel() != n:
        raise RuntimeError(f"hlhgat: row mask has {mask.numel()} entries, operator {n} rows")
    keys, extra = [edge_index, edge_weight], (n, "row_mask", id(mask))
    op = _HODGE_CACHE.get(keys, extra)
    fresh = op is None
    if fresh:
        base = _hodge_operator(edge_index, edge_weight, n)
        a = base.fwd

        def buf(name, like):
            t = bufs.get(name)
            if t is None or t.shape != like.shape or t.device != like.device:
                t = bufs[name] = torch.empty_like(like)
            return t

        m = SparseCSR(a.rowptr, a.col, buf("val", a.val), a.n_rows, a.n_cols, a.nnz, a.order,
                      a.valid)
        eperm = None
        if a.halo is not None:
            tp, hp, hc, srp, lcol, sval, bounds, hdr = a.halo
            if sval is not None:
                eperm = edge_index._hlhgat_halo[5]
                sval = buf("sval", sval)
            m.halo = (tp, hp, hc, srp, lcol, sval, bounds, hdr)
        op = HodgeOperator(m, m, masked_from=(base, mask, eperm))
        if base.factor is not None:
            nr, ne, ns, no, ends, alpha, eo = base.factor
            op.factor = (nr, ne, buf("sign", ns), no, ends, buf("alpha", alpha), eo)
            op.factor_nodes = base.factor_nodes
        _HODGE_CACHE.put(keys, extra, op)
    if fresh or refresh:
        base, _, eperm = op.masked_from
        a, st = op.fwd, _stream(mask)
        if a.n_rows and a.nnz:
            check(LIB.hlhgat_mask_csr_values(a.rowptr.data_ptr(), a.col.data_ptr(),
                                             base.fwd.val.data_ptr(), a.n_rows, a.nnz,
                                             mask.data_ptr(), a.val.data_ptr(), st),
                  "mask_csr_values")
            if eperm is not None:
                check(LIB.hlhgat_gather_f32(a.val.data_ptr(), eperm.data_ptr(), a.nnz,
                                            a.halo[5].data_ptr(), st), "gather_f32")
        if op.factor is not None and a.n_rows:
            check(LIB.hlhgat_mask_hodge_factor(_factor_desc(base), mask.data_ptr(),
                                               op.factor[2].data_ptr(), op.factor[5].data_ptr(),
                                               st), "mask_hodge_factor")
    return op


SIMPLEX_SITE = 0x80000000  # site of SimplexDropout k: SIMPLEX_SITE + 2k (graph), + 1 (row)


def simplex_thresholds(aug_prob: float, p: float, jitter: float) -> Tuple[int, int, int]:
    """(Ta, Tp, Tj) = floor(. * 2^24) of the simplex-dropout rule, in double."""
    for name, v in (("aug_prob", aug_prob), ("p", p), ("jitter", jitter)):
        if not 0.0 <= float(v) <= 1.0:
            raise ValueError(f"simplex dropout: {name} has to be between 0 and 1, but got {v}")
    Ta, Tp, Tj = (int(math.floor(float(v) * 16777216.0)) for v in (aug_prob, p, jitter))
    if Tp + Tj > 1 << 24:
        raise ValueError(f"simplex dropout: p + jitter = {p} + {jitter} exceeds 1")
    return Ta, Tp, Tj


def simplex_keep(seg_ptr: torch.Tensor, mask: torch.Tensor, aug_prob: float, p: float,
                 jitter: float, site: int = 0, protect: Optional[torch.Tensor] = None,
                 column: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Draw the keep mask of dropout_node / TSP_EigPE.get
    (main_TSP_HL_HGCNN_dense_int3_pyr.py:84-92, :125-131) for every graph of a
    batch into ``mask`` (fp32 [n_rows], 1 = kept; rows >= seg_ptr[-1] are
    padding and get 0) and, when given, into ``column`` (a strided [n_rows]
    view such as x_s[:, 1]): one launch, counter-based on the shared dropout
    state (dropout_state), so a captured launch draws a fresh mask per replay.
    A graph is augmented with probability aug_prob; its rate is p + U * jitter;
    rows whose ``protect`` entry (a strided fp32 [n_rows] view) is non-zero are
    never dropped.  ``site`` is the module ordinal k."""
    _req_dev(mask, "mask")
    _req_dev(seg_ptr, "seg_ptr", torch.int32)
    if mask.dim() != 1 or not mask.is_contiguous() or seg_ptr.dim() != 1 or seg_ptr.numel() < 1 \
            or not seg_ptr.is_contiguous():
        raise RuntimeError("hlhgat: simplex_keep: mask [n_rows] and seg_ptr [G + 1] must be "
                           "contiguous 1-D tensors")
    n = mask.numel()
    for name, t in (("protect", protect), ("column", column)):
        if t is None:
            continue
        _req_dev(t, name)
        if t.dim() == 2 and t.size(1) == 1:
            t = t[:, 0]
        if t.dim() != 1 or t.numel() != n or (n > 1 and t.stride(0) < 1):
            raise RuntimeError(f"hlhgat: simplex_keep: {name} must be a [n_rows] (strided) view "
                               f"(got {tuple(t.shape)})")
        if name == "protect":
            protect = t
        else:
            column = t
    if not 0 <= int(site) < (1 << 30):
        raise ValueError(f"simplex dropout: site {site} out of range")
    Ta, Tp, Tj = simplex_thresholds(aug_prob, p, jitter)
    st = _dropout_st(mask.device)
    ld = lambda t: max(int(t.stride(0)), 1)  # noqa: E731
    check(LIB.hlhgat_simplex_keep(
        seg_ptr.data_ptr(), seg_ptr.numel() - 1, n, _ptr(protect),
        ld(protect) if protect is not None else 0, Ta, Tp, Tj, SIMPLEX_SITE + 2 * int(site),
        st.dev.data_ptr(), mask.data_ptr(), _ptr(column), ld(column) if column is not None else 0,
        _stream(mask)), "simplex_keep")
    return mask


def set_csr(edge_index: torch.Tensor, rowptr: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """Attach the CSR of a sorted symmetric Laplacian COO built with the batch
    (hodge_dataset.laplacian_csr, at collate): int32 rowptr over edge_index[0]
    and int32 columns; the values are edge_weight itself.  hodge_operator then
    uses it instead of hlhgat_csr_from_sorted_coo (the same arrays, bitwise)."""
    edge_index._hlhgat_csr = (  # type: ignore[attr-defined]
        rowptr.to(device=edge_index.device, dtype=torch.int32).contiguous(),
        col.to(device=edge_index.device, dtype=torch.int32).contiguous())
    return edge_index


def set_incidence(edge_index: torch.Tensor, rowptr: torch.Tensor,
                  edge_ids: torch.Tensor) -> torch.Tensor:
    """Attach the incidence CSR of |B1| built with the batch
    (hodge_dataset.incidence_csr, at collate): ``incidence`` then uses it
    instead of sorting on the device.  It must be the CSR hlhgat_incidence_csr
    builds (rows = nodes, incident edge ids ascending; tests check bitwise)."""
    edge_index._hlhgat_incidence = (  # type: ignore[attr-defined]
        rowptr.to(device=edge_index.device, dtype=torch.int32).contiguous(),
        edge_ids.to(device=edge_index.device, dtype=torch.int32).contiguous())
    return edge_index


def incidence(edge_index: torch.Tensor, n_nodes: int) -> Incidence:
    """Incidence CSR of |B1| built from the undirected edge list (i<j)."""
    _req_dev(edge_index, "edge_index", torch.int64)
    hit = _INC_CACHE.get([edge_index], n_nodes)
    if hit is not None:
        return hit
    ei = edge_index.contiguous()
    E = ei.size(1)
    dev = ei.device
    pre = getattr(edge_index, "_hlhgat_incidence", None)
    if pre is not None:
        rowptr, eids = pre
        if rowptr.numel() != n_nodes + 1 or eids.numel() != 2 * E:
            raise RuntimeError(f"hlhgat: attached incidence CSR has {rowptr.numel() - 1} rows / "
                               f"{eids.numel()} entries, expected {n_nodes} / {2 * E}")
        inc = Incidence(rowptr, eids, ei, n_nodes, E)
        signs = getattr(edge_index, "_hlhgat_inc_signs", None)  # collate-time (factor tables)
        if torch.is_tensor(signs) and signs.numel() == 2 * E and signs.device == dev:
            inc._signs = signs  # type: ignore[attr-defined]
        return _INC_CACHE.put([edge_index], n_nodes, inc)
    rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    eids = torch.empty(max(2 * E, 1), dtype=torch.int32, device=dev)[:2 * E]
    ws_bytes = int(LIB.hlhgat_csr_workspace_bytes(2 * E))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(LIB.hlhgat_incidence_csr(ei.data_ptr() if E else None, E, n_nodes,
                                   rowptr.data_ptr(), eids.data_ptr() if E else None,
                                   ws.data_ptr(), ws_bytes, _stream(ei)),
          "incidence_csr")
    return _INC_CACHE.put([edge_index], n_nodes, Incidence(rowptr, eids, ei, n_nodes, E))


# ----------------------------------------------------------------------------
# raw launches
# ----------------------------------------------------------------------------
def _poly_step(A: SparseCSR, X: torch.Tensor, Y: torch.Tensor, *, rs=None, Z=None, P=None,
               Q=None, alpha=1.0, beta=0.0, gamma=0.0, div=1.0, p=0.0, q=0.0) -> None:
    d = X.size(1)
    check(LIB.hlhgat_poly_step(
        A.rowptr.data_ptr(), A.col.data_ptr() if A.nnz else None, _ptr(A.val) if A.nnz else None,
        _ptr(rs), A.n_rows, A.nnz, _ptr(A.order), _halo_desc(A), X.data_ptr(), _ld(X), d,
        _ptr(Z), _ld(Z) if Z is not None else 0, _ptr(P), _ld(P) if P is not None else 0,
        _ptr(Q), _ld(Q) if Q is not None else 0, alpha, beta, gamma, div, p, q,
        Y.data_ptr(), _ld(Y), _stream(X)), "poly_step")


def spmm(A: SparseCSR, X: torch.Tensor) -> torch.Tensor:
    """Y = A X (no autograd); PyG propagate when A = hodge_operator(...).fwd."""
    _req_dev(X, "X")
    X = _rows2d(X, "X")
    Y = torch.empty(A.n_rows, X.size(1), device=X.device, dtype=X.dtype)
    if A.n_rows:
        check(LIB.hlhgat_spmm(A.rowptr.data_ptr(), A.col.data_ptr() if A.nnz else None,
                              _ptr(A.val) if A.nnz else None, A.n_rows, A.nnz,
                              _ptr(A.order), _halo_desc(A), X.data_ptr(), _ld(X), X.size(1),
                              Y.data_ptr(),
                              _ld(Y),
                              _stream(X)), "spmm")
    return Y


def poly_basis(op: HodgeOperator, X: torch.Tensor, K: int, kind: int) -> torch.Tensor:
    """T_1..T_{K-1} as a [K-1, n, F] slab (no autograd)."""
    n, F = X.size(0), X.size(1)
    T = torch.empty(max(K - 1, 0), n, F, device=X.device, dtype=X.dtype)
    if K > 1 and n > 0 and op.factor is not None:
        work = torch.empty(int(LIB.hlhgat_hodge_factor_work_floats(op.factor_nodes, F)),
                           device=X.device)
        check(LIB.hlhgat_poly_basis_fwd_factored(kind, _factor_desc(op), X.data_ptr(), _ld(X), F,
                                                 K, T.data_ptr(), work.data_ptr(), _stream(X)),
              "poly_basis_fwd_factored")
    elif K > 1 and n > 0:
        A = op.fwd
        check(LIB.hlhgat_poly_basis_fwd(kind, A.rowptr.data_ptr(),
                                        A.col.data_ptr() if A.nnz else None,
                                        _ptr(A.val) if A.nnz else None, n, A.nnz,
                                        _ptr(A.order), _halo_desc(A), X.data_ptr(), _ld(X), F,
                                        K, T.data_ptr(),
                                        _stream(X)), "poly_basis_fwd")
    return T


def _proj_fwd(As: List[torch.Tensor], Ws: List[torch.Tensor], M: int, N: int,
              bias: Optional[torch.Tensor], out: torch.Tensor, accumulate=False) -> None:
    nb = len(As)
    check(LIB.hlhgat_proj_fwd(
        nb, _arr(C.c_void_p, [a.data_ptr() for a in As]), _arr(C.c_int64, [_ld(a) for a in As]),
        _arr(C.c_void_p, [w.data_ptr() for w in Ws]), _arr(C.c_int64, [w.stride(0) for w in Ws]),
        _arr(C.c_int64, [a.size(1) for a in As]), M, N, _ptr(bias), out.data_ptr(), _ld(out),
        int(accumulate), _stream(out)), "proj_fwd")


def _proj_bwd_data(G: torch.Tensor, Ws: List[torch.Tensor], kbs: List[int],
                   dAs: List[torch.Tensor], accumulate=False) -> None:
    nb = len(Ws)
    check(LIB.hlhgat_proj_bwd_data(
        nb, G.data_ptr(), _ld(G), _arr(C.c_void_p, [w.data_ptr() for w in Ws]),
        _arr(C.c_int64, [w.stride(0) for w in Ws]), _arr(C.c_int64, kbs), G.size(0), G.size(1),
        _arr(C.c_void_p, [d.data_ptr() for d in dAs]), _arr(C.c_int64, [_ld(d) for d in dAs]),
        int(accumulate), _stream(G)), "proj_bwd_data")


def _proj_bwd_weight(G: torch.Tensor, As: List[torch.Tensor], dWs: List[torch.Tensor],
                     dbias: Optional[torch.Tensor]) -> None:
    nb = len(As)
    kb = _arr(C.c_int64, [a.size(1) for a in As])
    M, N = G.size(0), G.size(1)
    wsf = int(LIB.hlhgat_proj_bwd_weight_workspace_floats(nb, kb, M, N, int(dbias is not None)))
    ws = torch.empty(max(wsf, 1), device=G.device, dtype=torch.float32)
    check(LIB.hlhgat_proj_bwd_weight(
        nb, G.data_ptr(), _ld(G), _arr(C.c_void_p, [a.data_ptr() for a in As]),
        _arr(C.c_int64, [_ld(a) for a in As]), kb, M, N,
        _arr(C.c_void_p, [d.data_ptr() for d in dWs]), _arr(C.c_int64, [d.stride(0) for d in dWs]),
        _ptr(dbias), 0, ws.data_ptr(), wsf, _stream(G)), "proj_bwd_weight")


# ----------------------------------------------------------------------------
# HodgeLaguerreConv / HodgeChebConv fused forward + hand-written backward
# ----------------------------------------------------------------------------
def _bn_args(bn: Optional[torch.nn.BatchNorm1d]):
    """(weight, bias, running_mean, running_var, num_batches_tracked, momentum,
    eps) for a training-mode BatchNorm1d, torch semantics."""
    track = bn.training and bn.track_running_stats and bn.running_mean is not None
    if track and bn.momentum is None:
        momentum = 1.0 / float(bn.num_batches_tracked.item() + 1)
    else:
        momentum = float(bn.momentum) if bn.momentum is not None else 0.0
    return (bn.weight, bn.bias, bn.running_mean if track else None,
            bn.running_var if track else None, bn.num_batches_tracked if track else None,
            momentum, float(bn.eps))


def _bn_uses_batch_stats(bn) -> bool:
    return bn.training or not bn.track_running_stats


def hodge_poly_conv(x: torch.Tensor, op: HodgeOperator, weights: Sequence[torch.Tensor],
                    bias: Optional[torch.Tensor], kind: int = POLY_LAGUERRE,
                    bn: Optional[torch.nn.BatchNorm1d] = None, relu: bool = False,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = sum_k T_k W_k^T + bias with T_k the Laguerre / Chebyshev basis of
    x over L (lib/Hodge_Cheb_Conv.py:480-515 / :394-439); x may be [N, C] or
    [N, T, C] (3-D inputs propagate over [N, T*C] rows, :493-505).  With
    ``bn`` the following BatchNorm (and ReLU) of the HL block runs inside the
    same C++ autograd node (lib/Hodge_ST_Model.py:556-566).  ``out`` (a
    DenseConcat sink) receives the final output when the conv, BN and ReLU run
    as one node; otherwise it is ignored and the caller copies."""
    _req_dev(x, "x")
    if x.size(0) != op.fwd.n_rows:
        raise RuntimeError(f"hlhgat: x has {x.size(0)} rows but the operator has "
                           f"{op.fwd.n_rows}")
    A, At = op.fwd, op.bwd
    ws = list(weights)
    if bn is not None and x.dim() == 2 and _bn_uses_batch_stats(bn) and sync_bn_group(bn) is None:
        if x.size(0) < 2 and bn.training:
            raise ValueError("Expected more than 1 value per channel when training")
        return _ext.conv_bn(x, A.rowptr, A.col, A.val, At.rowptr, At.col, At.val, A.nnz, kind,
                            ws, bias, *_bn_args(bn), 2 if relu else 1, out, A.order, At.order,
                            A.valid, *_halo_args(A), *_factor_args(op))
    sink = out if (bn is None and not relu and x.dim() == 2) else None
    y = _ext.conv_bn(x, A.rowptr, A.col, A.val, At.rowptr, At.col, At.val, A.nnz, kind, ws,
                     bias, None, None, None, None, None, 0.0, 0.0, 0, sink, A.order, At.order,
                     A.valid, *_halo_args(A), *_factor_args(op))
    if bn is not None:
        y = batch_norm_act(y, bn, relu, valid=A.valid)
    elif relu:
        y = torch.relu(y)
    return y


# ----------------------------------------------------------------------------
# Dense concatenation of the HL blocks in one slab
# ----------------------------------------------------------------------------
DENSE_SLAB = True   # tests set False: the torch.cat concatenation
GRAD_SINK = True


class DenseConcat:
    """The running concatenation x0 = cat[y_0, y_1, ...] of the dense HL
    blocks (lib/Hodge_ST_Model.py:631-632: x_t0 = torch.cat([x_t0, x_t], -1))
    held in ONE preallocated [rows, width] slab.

    Each block output is written straight into its column block (``sink``
    hands the conv a destination; ``append`` copies only when the producer
    could not write there), and ``view()`` returns x0 as a column prefix of the
    slab: no O(depth^2) re-copies in the forward.  In the backward, every
    view's gradient is accumulated into one gradient slab and each block's
    output gradient is handed out as a column block of it, so the per-block
    slice / add / copy kernels of torch.cat's backward disappear too.  Forward
    values are identical to the torch.cat formulation; gradients are the same
    fp32 sums, accumulated in view order (tests: tolerance of the model)."""

    def __init__(self, rows: int, width: int, like: torch.Tensor):
        self.S = torch.empty(rows, width, dtype=torch.float32, device=like.device)
        self.width = width
        # backward-side state shared by the views; it holds no reference to the
        # parts, so the autograd graph and this object do not form a cycle
        self._state = _DenseGrad(self.S)
        self.parts: List[torch.Tensor] = []
        self.cols: List[Tuple[int, int]] = []
        self.owned: List[bool] = []  # part's gradient already handed to a view

    @property
    def used(self) -> int:
        return self.cols[-1][1] if self.cols else 0

    def sink(self, w: int) -> torch.Tensor:
        c0 = self.used
        if c0 + w > self.width:
            raise RuntimeError(f"hlhgat: DenseConcat overflow ({c0}+{w} > {self.width})")
        return self.S[:, c0:c0 + w]

    def append(self, y: torch.Tensor) -> None:
        if y.dim() != 2 or y.size(0) != self.S.size(0):
            raise RuntimeError(f"hlhgat: DenseConcat rows {self.S.size(0)}, got {tuple(y.shape)}")
        c0 = self.used
        c1 = c0 + y.size(1)
        if c1 > self.width:
            raise RuntimeError(f"hlhgat: DenseConcat overflow ({c1} > {self.width})")
        if y.data_ptr() != self.S.data_ptr() + 4 * c0 or y.stride(0) != self.S.stride(0):
            # through .data (its own version counter): columns [c0, c1) are
            # outside every view handed out so far, and a tracked in-place
            # copy would bump the version counter those views share with S
            self.S.data[:, c0:c1].copy_(y.detach())
        self.parts.append(y)
        self.cols.append((c0, c1))
        self.owned.append(False)

    def grad_sink(self) -> Optional[torch.Tensor]:
        """The gradient slab's view of the current x0 = view() (columns
        [0, used)): a consumer whose backward ADDS its input gradient into
        this view (NodeEdgeInt, accumulate_d of hlhgat_proj_bwd) spares the
        view's backward its add.  Returns (view, flag): the host int32 flag
        says whether a gradient has landed in the slab yet -- the first
        writer overwrites, the later ones add, so the slab is never zeroed."""
        if (not GRAD_SINK or not torch.is_grad_enabled()
                or not any(p.requires_grad for p in self.parts)):
            return None
        if self._state.G is None:
            # not zero-filled: the first gradient to land overwrites (flag)
            self._state.G = torch.empty_like(self.S)
            self._state.sink = True
        return self._state.G[:, :self.used], self._state.written

    def view(self) -> torch.Tensor:
        w = self.used
        if not torch.is_grad_enabled() or not any(p.requires_grad for p in self.parts):
            return self.S[:, :w]
        # the first view created after a part was appended is the last of the
        # views to run backward that covers it: it hands out that part's gradient
        ranges = [(c0, c1, not o) for (c0, c1), o in zip(self.cols, self.owned)]
        self.owned = [True] * len(self.owned)
        return _DenseViewFn.apply(self._state, ranges, w, *self.parts)


class _DenseGrad:
    def __init__(self, S: torch.Tensor):
        self.S = S
        self.G: Optional[torch.Tensor] = None
        self.sink = False  # G was handed out as a gradient sink (grad_sink)
        self.written = torch.zeros(1, dtype=torch.int32)  # host flag: G holds a gradient


class _DenseViewFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, ranges, w, *parts):
        ctx.state, ctx.ranges, ctx.w = state, ranges, w
        return state.S[:, :w]

    @staticmethod
    def backward(ctx, g):
        st, w = ctx.state, ctx.w
        if st.G is None:
            # first view to run backward = the widest (created last): it
            # initialises every column the narrower views accumulate into
            st.G = torch.empty_like(st.S)
            st.G[:, :w].copy_(g)
        elif (st.sink and g.data_ptr() == st.G.data_ptr() and g.shape == (st.G.size(0), w)
              and g.stride() == st.G[:, :w].stride()):
            pass  # the consumer already added its gradient into the slab (grad_sink)
        elif st.sink and int(st.written[0]) == 0:
            st.G[:, :w].copy_(g)  # first gradient into a sink slab: overwrite
            st.written[0] = 1
        else:
            st.G[:, :w].add_(g)
        grads = [st.G[:, c0:c1] if own else None for c0, c1, own in ctx.ranges]
        return (None, None, None, *grads)


# ----------------------------------------------------------------------------
# Linear over a split reduction axis (Linear(cat[a, b]) without the cat)
# ----------------------------------------------------------------------------
def linear_blocks(As: Sequence[torch.Tensor], weight: torch.Tensor,
                  bias: Optional[torch.Tensor]) -> torch.Tensor:
    """F.linear(cat(As, -1), weight, bias) with the concatenation folded into
    the MFMA GEMM's reduction axis (lib/Hodge_Cheb_Conv.py:307-308)."""
    if len(As) > _lib.MAX_BLOCKS:
        raise RuntimeError(f"hlhgat: at most {_lib.MAX_BLOCKS} operand blocks")
    _req_dev(weight, "weight")
    return _ext.linear(list(As), weight, bias)


def mlp2(blocks: Sequence[torch.Tensor], seq: torch.nn.Sequential) -> torch.Tensor:
    """NodeEdgeInt WV_* (Linear(2d, dl) -> BN -> ReLU -> Linear(dl, dv) -> BN ->
    ReLU, lib/Hodge_Cheb_Conv.py:276-289) on cat(blocks) as one C++ node."""
    lin0, bn1, _, lin3, bn4, _ = list(seq)
    return _ext.mlp2(list(blocks), lin0.weight, lin0.bias, *_bn_args(bn1)[:5], lin3.weight,
                     lin3.bias, *_bn_args(bn4)[:5], _bn_args(bn1)[5], float(bn1.eps),
                     _bn_args(bn4)[5], float(bn4.eps))


def _mlp2_params(seq: torch.nn.Sequential):
    """The 14 tensors of a reference WV_* MLP (Linear, BN, ReLU, Linear, BN,
    ReLU) in training mode with affine, tracked BN and biased Linears, or
    None when the module differs from that structure."""
    m = list(seq)
    if not (len(m) == 6 and isinstance(m[0], torch.nn.Linear)
            and isinstance(m[1], torch.nn.BatchNorm1d) and isinstance(m[2], torch.nn.ReLU)
            and isinstance(m[3], torch.nn.Linear) and isinstance(m[4], torch.nn.BatchNorm1d)
            and isinstance(m[5], torch.nn.ReLU)):
        return None
    l0, b1, _, l3, b4, _ = m
    for b in (b1, b4):
        if not (b.training and b.affine and b.track_running_stats and b.momentum is not None
                and b.running_mean is not None) or sync_bn_group(b) is not None:
            return None
    if l0.bias is None or l3.bias is None:
        return None
    return ([l0.weight, l0.bias, b1.weight, b1.bias, b1.running_mean, b1.running_var,
             b1.num_batches_tracked, l3.weight, l3.bias, b4.weight, b4.bias, b4.running_mean,
             b4.running_var, b4.num_batches_tracked],
            [float(b1.momentum), float(b1.eps), float(b4.momentum), float(b4.eps)])


def nei_prepack(neints) -> None:
    """Pack the first-Linear weights / biases of every NodeEdgeInt value path
    in `neints` (hodge_cheb_conv.NodeEdgeInt modules) in ONE launch at the
    start of the forward, instead of one pack launch inside each NodeEdgeInt
    on the critical stream; each module consumes its pack once (nei_value)."""
    mods, groups = [], []
    for m in (neints if PREPACK else []):
        pn, pe = _mlp2_params(m.WV_Node), _mlp2_params(m.WV_Edge)
        if pn is None or pe is None or not pn[0][0].is_cuda:
            continue
        mods.append(m)
        groups.append([pn[0][0], pn[0][1], pe[0][0], pe[0][1]])
    global _PACK_EPOCH
    _PACK_EPOCH += 1
    if not mods:
        return
    for m, packed in zip(mods, _ext.nei_prepack(groups)):
        m._hlhgat_packed = (_PACK_EPOCH, packed)


_PACK_EPOCH = 0  # a pack is only used by the forward that built it
# PREPACK = False (tests; HLHGAT_PREPACK=0 for A/B): each NodeEdgeInt packs its
# own weights, each only_att NodeEdgeInt concatenates its K|Q (same results)
PREPACK = os.environ.get("HLHGAT_PREPACK", "1") != "0"


class _AttPackFn(torch.autograd.Function):
    """The only_att NodeEdgeInts' concatenated projections
    (cat[WK_Node; WQ_Node] and cat[WK_Edge; WQ_Edge], weights and biases) of
    a whole forward in ONE batched copy instead of four torch.cat launches
    per module; the backward hands each parameter its rows of the packed
    gradients (views, as torch.cat's backward does)."""

    @staticmethod
    def forward(ctx, n_mod, *params):
        outs, srcs, dsts = [], [], []
        for i in range(n_mod):
            wkn, wqn, bkn, bqn, wke, wqe, bke, bqe = params[8 * i:8 * i + 8]
            for a, b in ((wkn, wqn), (bkn, bqn), (wke, wqe), (bke, bqe)):
                o = torch.empty((a.size(0) + b.size(0),) + tuple(a.shape[1:]), device=a.device,
                                dtype=a.dtype)
                srcs += [a.detach(), b.detach()]
                dsts += [o[:a.size(0)], o[a.size(0):]]
                outs.append(o)
        copy_words_batched(srcs, dsts)
        ctx.n_mod = n_mod
        ctx.rows = [p.size(0) for p in params]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        out = [None]
        for i in range(ctx.n_mod):
            r = ctx.rows[8 * i:8 * i + 8]
            for q, g in enumerate(grads[4 * i:4 * i + 4]):
                k = r[2 * q]  # rows of the pair's first parameter
                if g is None:
                    out += [None, None]
                else:
                    out += [g[:k], g[k:]]
        # params order: wkn, wqn, bkn, bqn, wke, wqe, bke, bqe per module
        return tuple(out)


def att_prepack(neatts) -> None:
    """Pack the K|Q projections of every only_att NodeEdgeInt in `neatts`
    in one launch at the start of the forward (NodeEdgeInt._unfused takes
    its pack once, take_pack's epoch rule)."""
    mods = [m for m in (neatts if PREPACK else [])
            if m.only_att and m.WK_Node.weight.is_cuda and m.WK_Node.bias is not None]
    if not mods:
        return
    params = []
    for m in mods:
        params += [m.WK_Node.weight, m.WQ_Node.weight, m.WK_Node.bias, m.WQ_Node.bias,
                   m.WK_Edge.weight, m.WQ_Edge.weight, m.WK_Edge.bias, m.WQ_Edge.bias]
    global _ATT_EPOCH
    _ATT_EPOCH += 1
    outs = _AttPackFn.apply(len(mods), *params)
    for i, m in enumerate(mods):
        m._hlhgat_att_packed = (outs[4 * i:4 * i + 4], _att_versions(m), _ATT_EPOCH)


_ATT_EPOCH = 0  # the latest att_prepack (a pack is only used until the next one)


def _att_versions(m):
    return tuple(t._version for t in (m.WK_Node.weight, m.WQ_Node.weight, m.WK_Node.bias,
                                      m.WQ_Node.bias, m.WK_Edge.weight, m.WQ_Edge.weight,
                                      m.WK_Edge.bias, m.WQ_Edge.bias))


def take_att_pack(m):
    """The module's (w_t, b_t, w_s, b_s) from the latest att_prepack,
    consumed; None when there is none, a later att_prepack ran, or a
    parameter's version counter moved since (an in-place update)."""
    p, m._hlhgat_att_packed = getattr(m, "_hlhgat_att_packed", None), None
    if p is None or p[2] != _ATT_EPOCH or p[1] != _att_versions(m):
        return None
    if (torch.is_grad_enabled() and m.WK_Node.weight.requires_grad
            and not p[0][0].requires_grad):
        return None  # packed under no_grad, used with gradients
    return p[0]


def take_pack(m) -> Optional[torch.Tensor]:
    """The module's pack from the current forward's nei_prepack, consumed."""
    p, m._hlhgat_packed = getattr(m, "_hlhgat_packed", None), None
    return p[1] if p is not None and p[0] == _PACK_EPOCH else None


def nei_value(x_t: torch.Tensor, x_s: torch.Tensor, inc: "Incidence", rD: torch.Tensor,
              wv_node: torch.nn.Sequential, wv_edge: torch.nn.Sequential,
              valid_t: Optional[torch.Tensor] = None, valid_s: Optional[torch.Tensor] = None,
              gsink=(None, None), packed: Optional[torch.Tensor] = None):
    """NodeEdgeInt value path (lib/Hodge_Cheb_Conv.py:293-295,307-308) as one
    C++ node, first Linear projected before the |B1| gathers (torch_ext.cpp,
    NEIntValueFn); returns (x_t1, x_s1), or None when the WV_* modules are not
    the reference training-mode structure (caller falls back)."""
    pn, pe = _mlp2_params(wv_node), _mlp2_params(wv_edge)
    if pn is None or pe is None:
        return None
    _req_dev(x_t, "x_t")
    _req_dev(x_s, "x_s")
    if x_s.size(0) != inc.n_edges or x_t.size(0) != inc.n_nodes:
        raise RuntimeError(f"hlhgat: x_t/x_s rows ({x_t.size(0)}, {x_s.size(0)}) do not match "
                           f"|B1| ({inc.n_nodes}, {inc.n_edges})")
    if rD.numel() != inc.n_nodes:
        raise RuntimeError(f"hlhgat: D has {rD.numel()} entries, |B1| has {inc.n_nodes} nodes")
    # gsink: the DenseConcat gradient-slab views of x_t / x_s (DenseConcat.grad_sink):
    # their gradients are added straight into the slab by the Linear backward
    (gt, ft), (gs, fs) = [g if g is not None else (None, None) for g in gsink]
    if gt is not None and (gt.shape != x_t.shape or gt.data_ptr() == x_t.data_ptr()):
        gt = ft = None
    if gs is not None and (gs.shape != x_s.shape or gs.data_ptr() == x_s.data_ptr()):
        gs = fs = None
    r = _ext.nei_value(x_t, x_s, inc.rowptr, inc.edge_ids, inc.edge_index,
                       rD.contiguous().view(-1), pn[0], pe[0], *pn[1], *pe[1], valid_t, valid_s,
                       gt, gs, ft, fs, packed)
    return r[0], r[1]


# ----------------------------------------------------------------------------
# boundary operator: x_s2t = (1/D) |B1| x_s ; x_t2s = |B1|^T x_t / 2
# ----------------------------------------------------------------------------
def node_from_edges(x_s: torch.Tensor, inc: Incidence, rD: torch.Tensor) -> torch.Tensor:
    _req_dev(x_s, "x_s")
    _req_dev(rD, "1/D")
    if x_s.size(0) != inc.n_edges:
        raise RuntimeError(f"hlhgat: x_s has {x_s.size(0)} rows, |B1| has {inc.n_edges} edges")
    if rD.numel() != inc.n_nodes:
        raise RuntimeError(f"hlhgat: D has {rD.numel()} entries, |B1| has {inc.n_nodes} nodes")
    return _ext.node_from_edges(x_s, inc.rowptr, inc.edge_ids, inc.edge_index,
                                rD.contiguous().view(-1), inc.n_nodes)


def _incidence_signs(inc: Incidence) -> torch.Tensor:
    """Signed B1 values in incidence-CSR order: for node v's slot of edge e,
    -1 if v = edge_index[0][e] (tail), +1 if v = edge_index[1][e] (head)
    (adj2par1, lib/Hodge_Dataset.py:169-191).  Cached on the Incidence."""
    s = getattr(inc, "_signs", None)
    if s is None:
        dev = inc.rowptr.device
        counts = (inc.rowptr[1:] - inc.rowptr[:-1]).long()
        node = torch.repeat_interleave(torch.arange(inc.n_nodes, device=dev), counts,
                                       output_size=2 * inc.n_edges)
        head = inc.edge_index[1][inc.edge_ids.long()]
        s = torch.where(head == node, 1.0, -1.0).to(torch.float32).contiguous()
        inc._signs = s  # type: ignore[attr-defined]
    return s


class _BoundaryTFn(torch.autograd.Function):
    """y = B1^T x_t (y[e] = x_t[j] - x_t[i]); backward dx = B1 dy."""

    @staticmethod
    def forward(ctx, x_t, inc):
        ctx.inc = inc
        E, d = inc.n_edges, x_t.size(1)
        y = torch.empty(E, d, device=x_t.device, dtype=x_t.dtype)
        if E:
            check(LIB.hlhgat_edge_gather2(inc.edge_index.data_ptr(), E, x_t.data_ptr(), _ld(x_t),
                                          d, None, None, -1.0, 1.0, None, 0, y.data_ptr(),
                                          _ld(y), 0, _stream(x_t)), "edge_gather2(B1^T)")
        return y

    @staticmethod
    def backward(ctx, g):
        inc = ctx.inc
        g = _rows2d(g.contiguous(), "grad")
        A = SparseCSR(inc.rowptr, inc.edge_ids, _incidence_signs(inc), inc.n_nodes,
                      inc.n_edges, 2 * inc.n_edges)
        dx = torch.empty(inc.n_nodes, g.size(1), device=g.device, dtype=g.dtype)
        if inc.n_nodes:
            _poly_step(A, g, dx)
        return dx, None


class _TspReadoutFn(torch.autograd.Function):
    """R = cat([x_s, |B1^T x_t| / 2], -1) where R is a column window of a
    dense slab whose first columns already hold x_s (its last part): only the
    x_t2s half is computed, in one pass; the backward hands x_s its half of
    dR as a view and x_t B1 ((dR2 / 2) * sgn(B1^T x_t))."""

    @staticmethod
    def forward(ctx, x_s, x_t, inc, R):
        cs, E, d = x_s.size(1), inc.n_edges, x_t.size(1)
        ctx.inc, ctx.cs = inc, cs
        ctx.save_for_backward(x_t)
        check(LIB.hlhgat_edge_absdiff(inc.edge_index.data_ptr(), E, x_t.data_ptr(), _ld(x_t), d,
                                      None, 0, R.data_ptr() + 4 * cs, _ld(R), _stream(x_t)),
              "edge_absdiff")
        return R

    @staticmethod
    def backward(ctx, g):
        (x_t,) = ctx.saved_tensors
        inc, cs = ctx.inc, ctx.cs
        g = _rows2d(g, "grad")
        E, d = inc.n_edges, x_t.size(1)
        ge = torch.empty(E, d, device=g.device, dtype=g.dtype)
        check(LIB.hlhgat_edge_absdiff(inc.edge_index.data_ptr(), E, x_t.data_ptr(), _ld(x_t), d,
                                      g.data_ptr() + 4 * cs, _ld(g), ge.data_ptr(), d,
                                      _stream(g)), "edge_absdiff backward")
        A = SparseCSR(inc.rowptr, inc.edge_ids, _incidence_signs(inc), inc.n_nodes,
                      inc.n_edges, 2 * inc.n_edges)
        dx = torch.empty(inc.n_nodes, d, device=g.device, dtype=g.dtype)
        if inc.n_nodes:
            _poly_step(A, ge, dx)
        return g[:, :cs], dx, None, None


def tsp_readout(x_s: torch.Tensor, x_t: torch.Tensor, inc: Incidence,
                R: torch.Tensor) -> torch.Tensor:
    """The TSP head's readout input cat([x_s, |B1^T x_t| / 2], -1)
    (lib/Hodge_ST_Model.py:846-849) into R, a [n_edges, C_s + C_t] window of
    the edge slab whose first C_s columns hold x_s already: bitwise the
    unfused boundary_t / abs / div / cat and their gradients."""
    _req_dev(x_t, "x_t")
    x_t = _rows2d(x_t, "x_t")
    E = inc.n_edges
    if x_t.size(0) != inc.n_nodes or x_s.size(0) != E:
        raise RuntimeError(f"hlhgat: tsp_readout rows ({x_t.size(0)}, {x_s.size(0)}) vs |B1| "
                           f"({inc.n_nodes}, {E})")
    if tuple(R.shape) != (E, x_s.size(1) + x_t.size(1)) or R.stride(1) != 1:
        raise RuntimeError(f"hlhgat: tsp_readout window {tuple(R.shape)} does not fit")
    return _TspReadoutFn.apply(x_s, x_t, inc, R)


def boundary_t(x_t: torch.Tensor, inc: Incidence) -> torch.Tensor:
    """torch.sparse.mm(par_1.transpose(0, 1), x_t) for par_1 = adj2par1(...)
    (lib/Hodge_ST_Model.py:846): per edge (i, j), x_t[j] - x_t[i], summed in
    the coalesced order of the sparse product (tail entry first)."""
    _req_dev(x_t, "x_t")
    x_t = _rows2d(x_t, "x_t")
    if x_t.size(0) != inc.n_nodes:
        raise RuntimeError(f"hlhgat: x_t has {x_t.size(0)} rows, |B1| has {inc.n_nodes} nodes")
    return _BoundaryTFn.apply(x_t, inc)


class _IncidenceMMFn(torch.autograd.Function):
    """One of the four products with B1 of adj2par1 (lib/Hodge_Dataset.py:
    169-191) that torch.sparse.mm forms in the reference: B1 y, |B1| y (node
    rows: incidence CSR, edges ascending = the coalesced order) and B1^T x,
    |B1|^T x (edge rows: tail entry first).  The backward of each is the
    transposed product."""

    @staticmethod
    def forward(ctx, x, inc, transposed, signed):
        ctx.inc, ctx.transposed, ctx.signed = inc, transposed, signed
        return _incidence_mm(x, inc, transposed, signed)

    @staticmethod
    def backward(ctx, g):
        g = _rows2d(g.contiguous(), "grad")
        return _incidence_mm(g, ctx.inc, not ctx.transposed, ctx.signed), None, None, None


def _incidence_mm(x: torch.Tensor, inc: Incidence, transposed: bool, signed: bool):
    d = x.size(1)
    if transposed:  # edge rows: y[e] = c_i x[i] + x[j]
        y = torch.empty(inc.n_edges, d, device=x.device, dtype=x.dtype)
        if inc.n_edges:
            check(LIB.hlhgat_edge_gather2(inc.edge_index.data_ptr(), inc.n_edges, x.data_ptr(),
                                          _ld(x), d, None, None, -1.0 if signed else 1.0, 1.0,
                                          None, 0, y.data_ptr(), _ld(y), 0, _stream(x)),
                  "edge_gather2(B1^T)")
        return y
    A = SparseCSR(inc.rowptr, inc.edge_ids, _incidence_signs(inc) if signed else None,
                  inc.n_nodes, inc.n_edges, 2 * inc.n_edges)
    y = torch.empty(inc.n_nodes, d, device=x.device, dtype=x.dtype)
    if inc.n_nodes:
        _poly_step(A, x, y)
    return y


def incidence_mm(x: torch.Tensor, inc: Incidence, transposed: bool = False,
                 signed: bool = True) -> torch.Tensor:
    """torch.sparse.mm(P, x) for P = adj2par1(...) (signed) or its .abs(), or
    their transposes: bitwise the coalesced sparse product (autograd)."""
    _req_dev(x, "x")
    x = _rows2d(x, "x")
    rows = inc.n_nodes if transposed else inc.n_edges
    if x.size(0) != rows:
        raise RuntimeError(f"hlhgat: B1{'^T' if transposed else ''} product: x has {x.size(0)} "
                           f"rows, expected {rows}")
    return _IncidenceMMFn.apply(x, inc, bool(transposed), bool(signed))


def edge_from_nodes(x_t: torch.Tensor, inc: Incidence) -> torch.Tensor:
    _req_dev(x_t, "x_t")
    if x_t.size(0) != inc.n_nodes:
        raise RuntimeError(f"hlhgat: x_t has {x_t.size(0)} rows, |B1| has {inc.n_nodes} nodes")
    return _ext.edge_from_nodes(x_t, inc.rowptr, inc.edge_ids, inc.edge_index)


# ----------------------------------------------------------------------------
# only_att score
# ----------------------------------------------------------------------------
class _AttScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Qc, Qs, Kr, w_cross, w_self, sqrt_dk, sigma):
        n, dk = Kr.size(0), Kr.size(1)
        a = torch.empty(n, 1, device=Kr.device, dtype=Kr.dtype)
        check(LIB.hlhgat_att_score_fwd(n, dk, Qc.data_ptr(), _ld(Qc), Qs.data_ptr(), _ld(Qs),
                                       Kr.data_ptr(), _ld(Kr), w_cross, w_self, sqrt_dk, sigma,
                                       a.data_ptr(), _stream(Kr)), "att_score_fwd")
        ctx.consts = (w_cross, w_self, sqrt_dk, sigma)
        ctx.save_for_backward(Qc, Qs, Kr, a)
        return a

    @staticmethod
    def backward(ctx, ga):
        Qc, Qs, Kr, a = ctx.saved_tensors
        w_cross, w_self, sqrt_dk, sigma = ctx.consts
        n, dk = Kr.size(0), Kr.size(1)
        ga = ga.contiguous()
        g = torch.empty(3, n, dk, device=Kr.device, dtype=Kr.dtype)
        check(LIB.hlhgat_att_score_bwd(n, dk, Qc.data_ptr(), _ld(Qc), Qs.data_ptr(), _ld(Qs),
                                       Kr.data_ptr(), _ld(Kr), w_cross, w_self, sqrt_dk, sigma,
                                       a.data_ptr(), ga.data_ptr(), g[0].data_ptr(),
                                       g[1].data_ptr(), g[2].data_ptr(), dk, _stream(Kr)),
              "att_score_bwd")
        return g[0], g[1], g[2], None, None, None, None


class _AttScoreKQFn(torch.autograd.Function):
    """_AttScoreFn with K = kq[:, :dk] and Qs = kq[:, dk:2dk] (one GEMM's
    output): the backward returns kq's gradient as ONE [n, 2dk] block, no
    per-slice zero fill + copy + add."""

    @staticmethod
    def forward(ctx, Qc, kq, w_cross, w_self, sqrt_dk, sigma):
        n, dk = kq.size(0), Qc.size(1)
        a = torch.empty(n, 1, device=kq.device, dtype=kq.dtype)
        check(LIB.hlhgat_att_score_fwd(n, dk, Qc.data_ptr(), _ld(Qc), kq.data_ptr() + 4 * dk,
                                       _ld(kq), kq.data_ptr(), _ld(kq), w_cross, w_self, sqrt_dk,
                                       sigma, a.data_ptr(), _stream(kq)), "att_score_fwd")
        ctx.consts = (w_cross, w_self, sqrt_dk, sigma)
        ctx.save_for_backward(Qc, kq, a)
        return a

    @staticmethod
    def backward(ctx, ga):
        Qc, kq, a = ctx.saved_tensors
        w_cross, w_self, sqrt_dk, sigma = ctx.consts
        n, dk = kq.size(0), Qc.size(1)
        ga = ga.contiguous()
        # columns [0, dk) dK, [dk, 2dk) dQs (= d kq), [2dk, 3dk) dQc
        g = torch.empty(n, 3 * dk, device=kq.device, dtype=kq.dtype)
        p = g.data_ptr()
        check(LIB.hlhgat_att_score_bwd(n, dk, Qc.data_ptr(), _ld(Qc), kq.data_ptr() + 4 * dk,
                                       _ld(kq), kq.data_ptr(), _ld(kq), w_cross, w_self, sqrt_dk,
                                       sigma, a.data_ptr(), ga.data_ptr(), p + 8 * dk,
                                       p + 4 * dk, p, 3 * dk, _stream(kq)), "att_score_bwd")
        return g[:, 2 * dk:], g[:, :2 * dk], None, None, None, None


def att_score_kq(Qc, kq, w_cross: float, w_self: float, sqrt_dk: float,
                 sigma: int) -> torch.Tensor:
    """att_score(Qc, kq[:, dk:], kq[:, :dk], ...) with dk = Qc.size(1): the
    key and the self query as the two column halves of one [n, 2dk] GEMM
    output (lib/Hodge_Cheb_Conv.py:299-304)."""
    _req_dev(Qc, "Qc")
    _req_dev(kq, "kq")
    Qc, kq = _rows2d(Qc, "Qc"), _rows2d(kq, "kq")
    if kq.size(1) != 2 * Qc.size(1) or kq.size(0) != Qc.size(0):
        raise RuntimeError(f"hlhgat: att_score_kq: kq {tuple(kq.shape)} vs Qc {tuple(Qc.shape)}")
    return _AttScoreKQFn.apply(Qc, kq, float(w_cross), float(w_self), float(sqrt_dk), int(sigma))


class _RowScaleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, a, out, gsink):
        n, d = x.size(0), x.size(1)
        y = out if out is not None else torch.empty(n, d, device=x.device, dtype=x.dtype)
        check(LIB.hlhgat_row_scale_fwd(n, d, x.data_ptr(), _ld(x), a.data_ptr(), y.data_ptr(),
                                       _ld(y), _stream(x)), "row_scale_fwd")
        ctx.gsink = gsink
        ctx.save_for_backward(x, a)
        return y

    @staticmethod
    def backward(ctx, g):
        x, a = ctx.saved_tensors
        n, d = x.size(0), x.size(1)
        g = _rows2d(g, "grad")
        sink, flag = ctx.gsink if ctx.gsink is not None else (None, None)
        if sink is not None and int(flag[0]) == 0:
            gx = sink  # the first gradient into x's slab: written in place
            flag[0] = 1
        else:
            gx = torch.empty(n, d, device=x.device, dtype=x.dtype)
        ga = torch.empty(n, 1, device=x.device, dtype=x.dtype)
        check(LIB.hlhgat_row_scale_bwd(n, d, x.data_ptr(), _ld(x), a.data_ptr(), g.data_ptr(),
                                       _ld(g), gx.data_ptr(), _ld(gx), ga.data_ptr(),
                                       _stream(x)), "row_scale_bwd")
        return gx, ga, None, None


def row_scale(x: torch.Tensor, a: torch.Tensor, out: Optional[torch.Tensor] = None,
              gsink=None) -> torch.Tensor:
    """x * a for a per-row score a [n, 1] (the NEAtt product, main_pepfunc...:
    134-136): bitwise ATen's product; the backward's da = rowsum(dy * x) is
    one fused pass (fp32, its own summation order).  out: a DenseConcat sink
    for y; gsink: DenseConcat.grad_sink() of x = view(), written in place
    when x's gradient lands there first -- x must then have no other
    consumer (take a fresh view())."""
    _req_dev(x, "x")
    _req_dev(a, "a")
    x = _rows2d(x, "x")
    if a.numel() != x.size(0):
        raise RuntimeError(f"hlhgat: row_scale: a has {a.numel()} entries for {x.size(0)} rows")
    a = a.contiguous()
    if out is not None and (tuple(out.shape) != tuple(x.shape) or out.stride(1) != 1):
        raise RuntimeError(f"hlhgat: row_scale out {tuple(out.shape)} vs x {tuple(x.shape)}")
    if gsink is not None and (gsink[0] is None or gsink[0].shape != x.shape):
        gsink = None
    return _RowScaleFn.apply(x, a, out, gsink)


# ----------------------------------------------------------------------------
# Training-mode feature dropout (counter-based Philox mask, csrc/dropout.hip)
# ----------------------------------------------------------------------------
HIP_DROPOUT = True  # A/B hook: False = a live nn.Dropout runs ATen's dropout

_MASK64 = (1 << 64) - 1


def dropout_rank_seed(seed: int, rank: int) -> int:
    """The seed of data-parallel rank `rank`: (seed + rank * 0x9E3779B97F4A7C15)
    mod 2^64, so the ranks of one job draw different masks (pure host)."""
    return (int(seed) + int(rank) * 0x9E3779B97F4A7C15) & _MASK64


class _DropoutState:
    """Per-device dropout state: {seed, step} as two int64 ON the device (the
    kernels read them, so a captured step sees the advance) and the host-side
    call counter `site` baked into each launch."""

    def __init__(self, device: torch.device):
        self.device = device
        self.rank = 0
        self.site = 0
        self.dev = torch.empty(2, dtype=torch.int64, device=device)
        self.set(torch.initial_seed())

    def set(self, seed: int) -> None:
        s = dropout_rank_seed(seed, self.rank)
        s = s - (1 << 64) if s >= (1 << 63) else s  # the same 64 bits as int64
        self.dev.copy_(torch.tensor([s, 0], dtype=torch.int64))
        self.site = 0

    def next_site(self) -> int:
        s = self.site
        self.site = (s + 1) & 0xffffffff
        return s


_DROPOUT_STATES = {}


def _dropout_device(device) -> torch.device:
    d = torch.device("cuda" if device is None else device)
    if d.type != "cuda":
        raise RuntimeError(f"hlhgat: dropout state lives on a ROCm device (got {d})")
    return torch.device("cuda", torch.cuda.current_device() if d.index is None else d.index)


def _dropout_st(device) -> _DropoutState:
    d = _dropout_device(device)
    st = _DROPOUT_STATES.get(d.index)
    if st is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("hlhgat: the dropout state of a device must exist before a graph "
                               "capture (call ops.dropout_state / dropout_manual_seed first)")
        st = _DROPOUT_STATES[d.index] = _DropoutState(d)
    return st


def dropout_manual_seed(seed: int, device=None) -> None:
    """seed := seed (offset by the rank set with dropout_set_rank), step := 0,
    site := 0 on `device` (default: the current ROCm device)."""
    _dropout_st(device).set(int(seed) & _MASK64)


def dropout_set_state(seed: int, step: int, device=None, site: int = 0) -> None:
    """Restore a checkpointed (seed, step[, site]) as dropout_state returned
    it (the seed already carries the rank offset): one host write and one
    small copy, outside capture.  `site` is the host-side launch counter: an
    eager step draws its masks at the next sites, so eager training resumes
    on the uninterrupted run's masks only with it; a captured step keeps the
    sites it was captured with."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError("hlhgat: dropout_set_state during a graph capture")
    st = _dropout_st(device)
    s = int(seed) & _MASK64
    s = s - (1 << 64) if s >= (1 << 63) else s
    st.dev.copy_(torch.tensor([s, int(step)], dtype=torch.int64))
    st.site = int(site) & 0xffffffff


def dropout_set_rank(rank: int, device=None) -> None:
    """Data-parallel rank of this process (TrainStep, world > 1): the current
    and every later seed of `device` is offset by dropout_rank_seed."""
    st = _dropout_st(device)
    if rank != st.rank:
        seed = (dropout_state(device)[0] - st.rank * 0x9E3779B97F4A7C15) & _MASK64
        st.rank = int(rank)
        st.set(seed)


def dropout_advance(device=None) -> None:
    """step += 1 on the device (one launch on the current stream; captured into
    a graph it advances on every replay): the next step's masks."""
    st = _dropout_st(device)
    check(LIB.hlhgat_dropout_advance(st.dev.data_ptr(),
                                     torch._C._cuda_getCurrentRawStream(st.device.index)),
          "dropout_advance")


def dropout_state(device=None) -> Tuple[int, int, int]:
    """(seed, step, site) of `device` -- seed as an unsigned 64-bit value.
    Synchronises (tests, checkpoints)."""
    st = _dropout_st(device)
    seed, step = st.dev.tolist()
    return seed & _MASK64, step, st.site


def dropout_params(p: float) -> Tuple[int, float]:
    """(T, s) of the mask rule: keep iff (word >> 8) >= T = floor(p * 2^24);
    s = float32(1 / (1 - p)) rounded once from double (0 at p = 1: all dropped)."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    T = int(math.floor(p * 16777216.0))
    s = 0.0 if p == 1.0 else 1.0 / (1.0 - p)
    return T, s


def dropout(x: torch.Tensor, p: float, training: bool = True,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.nn.functional.dropout(x, p, training) for the Dropout that ends
    every HL block (lib/Hodge_ST_Model.py:556-566) as one HIP pass each way:
    the mask is a function of (seed, step, site, element) (csrc/dropout.hip),
    regenerated in the backward instead of stored, and drawn afresh by every
    replay of a captured step (dropout_advance).  Masks are not ATen's: parity
    with the reference under dropout is distributional.  p == 0 or eval
    returns x itself (no launch, no site); CPU tensors go to torch.  out: a
    [n, d] row-strided destination (DenseConcat.sink) for y.  Each launch
    takes the device's next `site`."""
    if p == 0.0 or not training:
        return x
    if not x.is_cuda:
        return torch.nn.functional.dropout(x, p, training)
    _req_dev(x, "x")
    T, s = dropout_params(p)
    shape = x.shape
    x2 = _rows2d(x if x.dim() == 2 else x.reshape(-1, shape[-1] if x.dim() else 1), "x")
    if out is not None and (x.dim() != 2 or tuple(out.shape) != tuple(x2.shape)
                            or out.stride(1) != 1 or out.stride(0) < out.size(1)):
        raise RuntimeError(f"hlhgat: dropout out {tuple(out.shape)} vs x {tuple(x.shape)}")
    if x2.numel() == 0:
        return x if out is None else out
    st = _dropout_st(x.device)
    y = _ext.dropout(x2, T, s, st.dev, st.next_site(), out)  # C++ autograd node
    return y if x.dim() == 2 else y.view(shape)


# ----------------------------------------------------------------------------
# PE sign-flip augmentation (counter-based Philox signs, csrc/peflip.hip)
# ----------------------------------------------------------------------------
PE_SITES = 1 << 29  # module ordinals k; the kernel's site word is 2k + side (side 0 = t, 1 = s)
PE_MAX_WIDTH = 65536  # n_fixed + n_flip


def _pe_site(site: int, side: int) -> int:
    if not 0 <= int(site) < PE_SITES:
        raise ValueError(f"pe_flip: site {site} out of range (0 <= site < 2^29)")
    if side not in (0, 1):
        raise ValueError(f"pe_flip: side must be 0 (t) or 1 (s), got {side!r}")
    return 2 * int(site) + side


def _pe_widths(n_fixed: int, n_flip: int, name: str) -> Tuple[int, int]:
    n_fixed, n_flip = int(n_fixed), int(n_flip)
    if n_fixed < 0 or n_flip < 0 or n_fixed + n_flip > PE_MAX_WIDTH:
        raise ValueError(f"pe_flip: {name}: n_fixed = {n_fixed}, n_flip = {n_flip} (both >= 0, "
                         f"n_fixed + n_flip <= {PE_MAX_WIDTH})")
    return n_fixed, n_flip


def _pe_desc(src, dst, seg, n_fixed, n_flip, site) -> "_lib.PeSideDesc":
    return _lib.PeSideDesc(src.data_ptr(), _ld(src), dst.data_ptr(), _ld(dst), _ptr(seg),
                           0 if seg is None else seg.numel() - 1, src.size(0), n_fixed, n_flip,
                           site)


def _pe_launch(descs, state: torch.Tensor, snap: torch.Tensor, ref: torch.Tensor) -> None:
    arr = (_lib.PeSideDesc * len(descs))(*descs)
    check(LIB.hlhgat_pe_flip(C.cast(arr, C.c_void_p), len(descs), state.data_ptr(),
                             snap.data_ptr(), _stream(ref)), "pe_flip")


class _PEFlipFn(torch.autograd.Function):
    """Both sides in one launch each way; the backward is the forward's entry
    point on dy at the forward's {seed, step} snapshot (no sign table stored)."""

    @staticmethod
    def forward(ctx, x_t, x_s, seg_t, seg_s, meta, state):
        xs, segs = (x_t, x_s), (seg_t, seg_s)
        ref = x_t if x_t is not None else x_s
        ys, descs = [None, None], []
        for i, x in enumerate(xs):
            if x is None:
                continue
            n_fixed, n_flip, site = meta[i]
            ys[i] = torch.empty(x.size(0), n_fixed + n_flip, device=x.device, dtype=x.dtype)
            descs.append(_pe_desc(x, ys[i], segs[i], n_fixed, n_flip, site))
        snap = torch.empty(2, dtype=torch.int64, device=ref.device)
        _pe_launch(descs, state, snap, ref)
        ctx.meta = meta
        ctx.widths = tuple(None if x is None else x.size(1) for x in xs)
        ctx.save_for_backward(snap, seg_t, seg_s)
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, g_t, g_s):
        snap, seg_t, seg_s = ctx.saved_tensors
        segs = (seg_t, seg_s)
        dxs, descs, ref = [None, None], [], None
        for i, g in enumerate((g_t, g_s)):
            if g is None or not ctx.needs_input_grad[i]:
                continue
            n_fixed, n_flip, site = ctx.meta[i]
            g = _rows2d(g, "grad")
            w = n_fixed + n_flip
            if ctx.widths[i] == w:
                dxs[i] = dst = torch.empty(g.size(0), w, device=g.device, dtype=g.dtype)
            else:  # the columns the forward dropped get no gradient
                dxs[i] = torch.zeros(g.size(0), ctx.widths[i], device=g.device, dtype=g.dtype)
                dst = dxs[i][:, :w]
            descs.append(_pe_desc(g, dst, segs[i], n_fixed, n_flip, site))
            ref = g
        if descs:
            _pe_launch(descs, snap, snap, ref)
        return dxs[0], dxs[1], None, None, None, None


def pe_signs(seg_ptr_or_n_graphs, n_flip: int, site: int = 0, side: int = 0,
             device=None) -> torch.Tensor:
    """The [n_graphs, n_flip] table of +1.0 / -1.0 that pe_flip multiplies the
    flipped columns of side `side` (0 = t, 1 = s) of module ordinal `site` by
    at the current dropout state (dropout_state) -- for tests and for logging
    the draw.  The first argument is a seg_ptr tensor ([n_graphs + 1], its
    device is used) or the number of graphs.  One launch; advances nothing."""
    if torch.is_tensor(seg_ptr_or_n_graphs):
        if seg_ptr_or_n_graphs.dim() != 1 or seg_ptr_or_n_graphs.numel() < 1:
            raise RuntimeError("hlhgat: pe_signs: seg_ptr must be a [n_graphs + 1] tensor")
        G = seg_ptr_or_n_graphs.numel() - 1
        device = seg_ptr_or_n_graphs.device if device is None else device
    else:
        G = int(seg_ptr_or_n_graphs)
    _, n_flip = _pe_widths(0, n_flip, "pe_signs")
    if G < 0:
        raise ValueError(f"pe_signs: n_graphs = {G}")
    word = _pe_site(site, side)
    st = _dropout_st(device)
    out = torch.empty(G, n_flip, device=st.device, dtype=torch.float32)
    check(LIB.hlhgat_pe_signs(G, n_flip, word, st.dev.data_ptr(), out.data_ptr(), _stream(out)),
          "pe_signs")
    return out


def pe_flip(x_t: Optional[torch.Tensor], seg_t: Optional[torch.Tensor], fixed_t: int,
            flip_t: int, x_s: Optional[torch.Tensor] = None,
            seg_s: Optional[torch.Tensor] = None, fixed_s: int = 0, flip_s: int = 0,
            site: int = 0) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The sign flip of the eigenvector positional-encoding columns that the
    reference's stored datasets apply per sample in get()
    (lib/Hodge_Dataset.py:425-440: ``x[:, :n_fixed + n_flip] * cat([ones(
    n_fixed), -1 + 2 * randint(0, 2, (n_flip,))])``, one draw for x_t and one
    for x_s) for every graph of a batch: y = (y_t, y_s), both sides in ONE
    launch, out of place (the caller's batch is never modified).  x_<side> is
    [n_rows, >= fixed + flip] fp32 with unit inner stride (a column window
    such as x[:, 1:] is read in place; wider inputs are truncated);
    seg_<side> is the int32 [n_graphs + 1] row pointer of the batch
    (batch.seg_ptr_<side>); rows at or beyond seg[-1] (static-shape padding)
    are copied unflipped.  Either side may be None.  The signs are a function
    of (seed, step, site, side, graph, column) on the shared dropout state
    (dropout_state; csrc/peflip.hip), so a captured launch draws fresh signs
    on every replay; ops.pe_signs returns them.  Differentiable: the backward
    is the same launch on dy at the forward's {seed, step} snapshot.  CPU
    tensors raise (no CPU path)."""
    word_t, word_s = _pe_site(site, 0), _pe_site(site, 1)
    xs, segs, meta = [None, None], [None, None], [None, None]
    for i, (x, seg, nf, nl, word, nm) in enumerate((
            (x_t, seg_t, fixed_t, flip_t, word_t, "t"), (x_s, seg_s, fixed_s, flip_s, word_s, "s"))):
        if x is None:
            continue
        _req_dev(x, "x_" + nm)
        nf, nl = _pe_widths(nf, nl, "x_" + nm)
        if x.dim() != 2 or x.size(1) < nf + nl:
            raise RuntimeError(f"hlhgat: pe_flip: x_{nm} {tuple(x.shape)} has fewer than "
                               f"{nf} + {nl} columns")
        if seg is None:
            raise RuntimeError(f"hlhgat: pe_flip: x_{nm} needs its seg_ptr (int32 [n_graphs + 1])")
        _req_dev(seg, "seg_" + nm, torch.int32)
        if seg.dim() != 1 or seg.numel() < 1 or not seg.is_contiguous() or seg.device != x.device:
            raise RuntimeError(f"hlhgat: pe_flip: seg_{nm} must be a contiguous [n_graphs + 1] "
                               f"tensor on x_{nm}'s device")
        xs[i], segs[i], meta[i] = _rows2d(x, "x_" + nm), seg, (nf, nl, word)
    if xs[0] is None and xs[1] is None:
        return None, None
    if xs[0] is not None and xs[1] is not None and xs[0].device != xs[1].device:
        raise RuntimeError("hlhgat: pe_flip: x_t and x_s must be on one device")
    st = _dropout_st((xs[0] if xs[0] is not None else xs[1]).device)
    return _PEFlipFn.apply(xs[0], xs[1], segs[0], segs[1], tuple(meta), st.dev)


def att_score(Qc, Qs, Kr, w_cross: float, w_self: float, sqrt_dk: float,
              sigma: int) -> torch.Tensor:
    """sigma((w_cross<Qc,K> + w_self<Qs,K>)/sqrt_dk) per row -> [n, 1]
    (lib/Hodge_Cheb_Conv.py:299-304)."""
    for t, nm in ((Qc, "Qc"), (Qs, "Qs"), (Kr, "K")):
        _req_dev(t, nm)
    return _AttScoreFn.apply(_rows2d(Qc, "Qc"), _rows2d(Qs, "Qs"), _rows2d(Kr, "K"),
                             float(w_cross), float(w_self), float(sqrt_dk), int(sigma))


# ----------------------------------------------------------------------------
# temporal front end (HL-HGAT-DEMO Inception1D): channels-last [N, T, C]
# ----------------------------------------------------------------------------
def _branch_arrays(weights):
    couts = [int(w.size(0)) for w in weights]
    tbs = [int(w.size(2)) for w in weights]
    return couts, tbs, _arr(_lib.c_i64, couts), _arr(_lib.c_i32, tbs)


def _tconv_pack(weights, cin: int, taps: int, flip: bool) -> torch.Tensor:
    couts, _, c_couts, c_tbs = _branch_arrays(weights)
    wp = torch.empty(taps * sum(couts) * cin, device=weights[0].device, dtype=torch.float32)
    check(LIB.hlhgat_tconv_pack(len(weights), _arr(_lib.c_vp, [w.data_ptr() for w in weights]),
                                c_couts, c_tbs, cin, taps, 1 if flip else 0, wp.data_ptr(),
                                _stream(wp)), "tconv_pack")
    return wp


def _tconv_bias(biases, couts, device) -> torch.Tensor:
    """The branches' biases as one [sum Cout_b] vector."""
    nb = len(biases)
    if nb == 1:
        return biases[0]
    bias = torch.empty(sum(couts), device=device, dtype=torch.float32)
    offs = [sum(couts[:b]) for b in range(nb)]
    one = [1] * nb
    check(LIB.hlhgat_copy2d_batched(
        nb, _arr(_lib.c_vp, [b.data_ptr() for b in biases]), _arr(_lib.c_i64, couts),
        _arr(_lib.c_vp, [bias.data_ptr() + 4 * o for o in offs]),
        _arr(_lib.c_i64, couts), _arr(_lib.c_i64, one), _arr(_lib.c_i64, couts),
        _stream(bias)), "copy2d_batched")
    return bias


def _tconv_skip(couts, tbs, taps: int) -> Tuple[int, int]:
    """(n1, n3): the output columns of the leading 1-tap / 3-tap branches,
    whose column tiles skip the outer taps."""
    n1 = n3 = 0
    b, nb = 0, len(couts)
    while b < nb and tbs[b] == 1 and taps > 1:
        n1 += couts[b]
        b += 1
    while b < nb and tbs[b] <= 3 and taps > 3:
        n3 += couts[b]
        b += 1
    return n1, n3


class _TemporalConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, nb, *params):
        weights, biases = list(params[:nb]), list(params[nb:])
        has_bias = biases[0] is not None
        N, T, cin = x.shape
        couts, tbs, _, _ = _branch_arrays(weights)
        cout, taps = sum(couts), max(tbs)
        y = torch.empty(N, T, cout, device=x.device, dtype=torch.float32)
        if cin == 1 and nb == 1:
            check(LIB.hlhgat_tconv_embed_fwd(x.data_ptr(), N, T, weights[0].data_ptr(),
                                             _ptr(biases[0]), cout, taps, y.data_ptr(),
                                             _stream(x)), "tconv_embed_fwd")
        else:
            wp = _tconv_pack(weights, cin, taps, False)
            bias = _tconv_bias(biases, couts, x.device) if has_bias else None
            n1, n3 = _tconv_skip(couts, tbs, taps)
            check(LIB.hlhgat_tconv_fwd(x.data_ptr(), N, T, cin, wp.data_ptr(), _ptr(bias), cout,
                                       taps, n1, n3, y.data_ptr(), _stream(x)), "tconv_fwd")
        ctx.nb, ctx.has_bias = nb, has_bias
        ctx.save_for_backward(x, *weights)
        return y

    @staticmethod
    def backward(ctx, g):
        x, *weights = ctx.saved_tensors
        nb = ctx.nb
        N, T, cin = x.shape
        couts, tbs, c_couts, c_tbs = _branch_arrays(weights)
        cout, taps = sum(couts), max(tbs)
        g = g.contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            wt = _tconv_pack(weights, cin, taps, True)
            gx = torch.empty(N, T, cin, device=x.device, dtype=torch.float32)
            check(LIB.hlhgat_tconv_fwd(g.data_ptr(), N, T, cout, wt.data_ptr(), None, cin, taps,
                                       0, 0, gx.data_ptr(), _stream(x)), "tconv_bwd_data")
        gws = [None] * nb
        gbs = [None] * nb
        if any(ctx.needs_input_grad[2:]):
            gws = [torch.empty_like(w) for w in weights]
            gb = (torch.empty(cout, device=x.device, dtype=torch.float32)
                  if ctx.has_bias else None)
            wsf = LIB.hlhgat_tconv_bwd_weight_workspace_floats(N, T, cin, cout, taps)
            ws = torch.empty(max(wsf, 1), device=x.device, dtype=torch.float32)
            check(LIB.hlhgat_tconv_bwd_weight(
                x.data_ptr(), g.data_ptr(), N, T, cin, cout, taps, nb,
                _arr(_lib.c_vp, [w.data_ptr() for w in gws]), c_couts, c_tbs, _ptr(gb),
                ws.data_ptr(), wsf, _stream(x)), "tconv_bwd_weight")
            if gb is not None:
                gbs = list(torch.split(gb, couts))
        return (gx, None, *gws, *gbs)


def temporal_conv(x: torch.Tensor, weights, biases=None) -> torch.Tensor:
    """F.conv1d over time with zero padding taps/2 on channels-last series
    x [N, T, Cin] -> [N, T, sum Cout_b]: the branches ``weights`` (nn.Conv1d
    layout [Cout_b, Cin, taps_b], odd taps_b <= 5) read the same input and
    their outputs are concatenated (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:
    501-509) -- one implicit-GEMM launch on a weight packed on the device."""
    if torch.is_tensor(weights):
        weights = [weights]
        biases = None if biases is None else [biases]
    weights = list(weights)
    nb = len(weights)
    biases = [None] * nb if biases is None else list(biases)
    _req_dev(x, "x")
    if x.dim() != 3:
        raise RuntimeError(f"hlhgat: temporal_conv x must be [N, T, C] (got {tuple(x.shape)})")
    if len(biases) != nb or len({b is None for b in biases}) != 1:
        raise RuntimeError("hlhgat: temporal_conv needs a bias for every branch or for none")
    for w, b in zip(weights, biases):
        _req_dev(w, "weight")
        if w.dim() != 3 or w.size(1) != x.size(2):
            raise RuntimeError(f"hlhgat: temporal_conv weight {tuple(w.shape)} for "
                               f"{x.size(2)} input channels")
        if b is not None:
            _req_dev(b, "bias")
    return _TemporalConvFn.apply(x.contiguous(), nb, *[w.contiguous() for w in weights],
                                 *[None if b is None else b.contiguous() for b in biases])


def maxpool_time_len(T: int, m: int) -> int:
    """Output length of nn.MaxPool1d(m, stride=m-1, padding=(m-1)//2)."""
    return int(LIB.hlhgat_maxpool_time_len(int(T), int(m)))


class _LeakyMaxPoolTimeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope, m):
        N, T, Cc = x.shape
        To = maxpool_time_len(T, m)
        y = torch.empty(N, To, Cc, device=x.device, dtype=torch.float32)
        idx = torch.empty(N, To, Cc, device=x.device, dtype=torch.int32)
        check(LIB.hlhgat_leaky_maxpool_time_fwd(x.data_ptr(), N, T, Cc, m, slope, y.data_ptr(),
                                                idx.data_ptr(), _stream(x)),
              "leaky_maxpool_time_fwd")
        ctx.slope, ctx.m = slope, m
        ctx.save_for_backward(x, idx)
        return y

    @staticmethod
    def backward(ctx, g):
        x, idx = ctx.saved_tensors
        N, T, Cc = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x)
        check(LIB.hlhgat_leaky_maxpool_time_bwd(x.data_ptr(), g.data_ptr(), idx.data_ptr(), N, T,
                                                Cc, ctx.m, ctx.slope, gx.data_ptr(), _stream(x)),
              "leaky_maxpool_time_bwd")
        return gx, None, None


def leaky_maxpool_time(x: torch.Tensor, slope: float, m: int) -> torch.Tensor:
    """MaxPool1d(m, stride=m-1, padding=(m-1)//2)(LeakyReLU(slope)(x)) over the
    time axis of x [N, T, C] -> [N, T', C] (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:
    488, :505); the gradient goes to each window's first maximum."""
    _req_dev(x, "x")
    if x.dim() != 3:
        raise RuntimeError(f"hlhgat: leaky_maxpool_time x must be [N, T, C] "
                           f"(got {tuple(x.shape)})")
    return _LeakyMaxPoolTimeFn.apply(x.contiguous(), float(slope), int(m))


class _TimeReadoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope):
        N, T, Cc = x.shape
        y = torch.empty(N, 2 * Cc, device=x.device, dtype=torch.float32)
        idx = torch.empty(N, Cc, device=x.device, dtype=torch.int32)
        check(LIB.hlhgat_time_readout_fwd(x.data_ptr(), N, T, Cc, slope, y.data_ptr(),
                                          idx.data_ptr(), _stream(x)), "time_readout_fwd")
        ctx.slope = slope
        ctx.save_for_backward(x, idx)
        return y

    @staticmethod
    def backward(ctx, g):
        x, idx = ctx.saved_tensors
        N, T, Cc = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x)
        check(LIB.hlhgat_time_readout_bwd(x.data_ptr(), g.data_ptr(), idx.data_ptr(), N, T, Cc,
                                          ctx.slope, gx.data_ptr(), _stream(x)),
              "time_readout_bwd")
        return gx, None


def time_readout(x: torch.Tensor, slope: float) -> torch.Tensor:
    """[max_t | mean_t] of LeakyReLU(slope)(x) for x [N, T, C] -> [N, 2C]
    (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:509-513)."""
    _req_dev(x, "x")
    if x.dim() != 3:
        raise RuntimeError(f"hlhgat: time_readout x must be [N, T, C] (got {tuple(x.shape)})")
    return _TimeReadoutFn.apply(x.contiguous(), float(slope))


# ----------------------------------------------------------------------------
# ragged time layout (include/hlhgat.h: hlhgat_tseries_t): series of their own
# lengths stacked compactly in buffers of fixed capacity
# ----------------------------------------------------------------------------
@dataclass
class TimeSeriesMap:
    """The device tables of time_series_map.  Stage 0 is the layout before
    the max-pool, stage 1 the one after it: series s owns rows
    [soff[i][s], soff[i][s + 1]) of a buffer of n_series * t_max[i] rows, and
    n_rows[i:i + 1] is the valid-row prefix (ops.batch_norm_act's valid=)."""
    n_series: int
    t_max: Tuple[int, int]
    pool: int
    soff: Tuple[torch.Tensor, torch.Tensor]
    tab: Tuple[torch.Tensor, torch.Tensor]
    sid: Tuple[torch.Tensor, torch.Tensor]
    n_rows: torch.Tensor
    desc: "_lib.TSeriesDesc"

    def capacity(self, stage: int) -> int:
        return self.n_series * self.t_max[stage]

    def valid(self, stage: int) -> torch.Tensor:
        return self.n_rows[stage:stage + 1]


def time_series_map(lengths: torch.Tensor, t_max: int, pool: int = 3) -> TimeSeriesMap:
    """The ragged layout of series with ``lengths`` (int32 [S], device,
    1 <= lengths[s] <= t_max; the per-sample window lengths of
    HL-HGAT-DEMO/lib/Hodge_Dataset.py:131-133) around a max-pool of window
    ``pool``: every table is built on the device in two launches, nothing is
    read back.  A length outside [1, t_max] is clamped and reported through
    check_device_errors."""
    _req_dev(lengths, "lengths", torch.int32)
    if lengths.dim() != 1 or not lengths.is_contiguous():
        raise RuntimeError(f"hlhgat: time_series_map lengths must be contiguous int32 [S] "
                           f"(got {tuple(lengths.shape)})")
    S, t0, m = int(lengths.numel()), int(t_max), int(pool)
    t1 = maxpool_time_len(t0, m) if t0 >= 1 and m >= 2 else 0
    dev = lengths.device
    i32 = dict(device=dev, dtype=torch.int32)
    soff = (torch.empty(S + 1, **i32), torch.empty(S + 1, **i32))
    tab = (torch.empty((S * max(t0, 0), 2), **i32), torch.empty((S * t1, 2), **i32))
    sid = (torch.empty(S * max(t0, 0), **i32), torch.empty(S * t1, **i32))
    n_rows = torch.empty(2, **i32)
    d = _lib.TSeriesDesc()
    d.n_series, d.pool = S, m
    d.t_max[0], d.t_max[1] = t0, t1
    for i in range(2):
        d.soff[i], d.tab[i], d.sid[i] = soff[i].data_ptr(), tab[i].data_ptr(), sid[i].data_ptr()
    d.n_rows = n_rows.data_ptr()
    check(LIB.hlhgat_tseries_map(lengths.data_ptr(), C.byref(d), _stream(lengths)), "tseries_map")
    return TimeSeriesMap(S, (t0, t1), m, soff, tab, sid, n_rows, d)


class _SeriesPackFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tm):
        xc = torch.empty(tm.capacity(0), 1, device=x.device, dtype=torch.float32)
        check(LIB.hlhgat_tseries_pack(x.data_ptr(), x.size(1), C.byref(tm.desc), 0, xc.data_ptr(),
                                      _stream(x)), "tseries_pack")
        ctx.tm, ctx.shape = tm, tuple(x.shape)
        return xc

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gx = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        check(LIB.hlhgat_tseries_pack(g.data_ptr(), ctx.shape[1], C.byref(ctx.tm.desc), 1,
                                      gx.data_ptr(), _stream(g)), "tseries_unpack")
        return gx, None


def time_series_pack(x: torch.Tensor, tm: TimeSeriesMap) -> torch.Tensor:
    """The padded time courses x [S, >= t_max] (x[s, lengths[s]:] is never
    read) as the compact stage-0 column [S * t_max, 1]; the gradient is zero
    in the padded columns."""
    _req_dev(x, "x")
    if x.dim() != 2 or x.size(0) != tm.n_series or x.size(1) < tm.t_max[0]:
        raise RuntimeError(f"hlhgat: time_series_pack x must be [{tm.n_series}, >= {tm.t_max[0]}] "
                           f"(got {tuple(x.shape)})")
    return _SeriesPackFn.apply(x.contiguous(), tm)


def _req_rows(x: torch.Tensor, tm: TimeSeriesMap, stage: int, name: str) -> None:
    _req_dev(x, "x")
    if x.dim() != 2 or x.size(0) != tm.capacity(stage):
        raise RuntimeError(f"hlhgat: {name} x must be [{tm.capacity(stage)}, C] rows of stage "
                           f"{stage} (got {tuple(x.shape)})")


class _TemporalConvRaggedFn(torch.autograd.Function):
    """_TemporalConvFn on the compact rows of one stage of a TimeSeriesMap."""

    @staticmethod
    def forward(ctx, x, tm, stage, nb, *params):
        weights, biases = list(params[:nb]), list(params[nb:])
        has_bias = biases[0] is not None
        M, cin = x.shape
        couts, tbs, _, _ = _branch_arrays(weights)
        cout, taps = sum(couts), max(tbs)
        y = torch.empty(M, cout, device=x.device, dtype=torch.float32)
        d = C.byref(tm.desc)
        if cin == 1 and nb == 1 and stage == 0:
            check(LIB.hlhgat_tconv_embed_fwd_ragged(x.data_ptr(), d, weights[0].data_ptr(),
                                                    _ptr(biases[0]), cout, taps, y.data_ptr(),
                                                    _stream(x)), "tconv_embed_fwd_ragged")
        else:
            wp = _tconv_pack(weights, cin, taps, False)
            bias = _tconv_bias(biases, couts, x.device) if has_bias else None
            n1, n3 = _tconv_skip(couts, tbs, taps)
            check(LIB.hlhgat_tconv_fwd_ragged(x.data_ptr(), d, stage, cin, wp.data_ptr(),
                                              _ptr(bias), cout, taps, n1, n3, y.data_ptr(),
                                              _stream(x)), "tconv_fwd_ragged")
        ctx.tm, ctx.stage, ctx.nb, ctx.has_bias = tm, stage, nb, has_bias
        ctx.save_for_backward(x, *weights)
        return y

    @staticmethod
    def backward(ctx, g):
        x, *weights = ctx.saved_tensors
        tm, stage, nb = ctx.tm, ctx.stage, ctx.nb
        M, cin = x.shape
        couts, tbs, c_couts, c_tbs = _branch_arrays(weights)
        cout, taps = sum(couts), max(tbs)
        g = g.contiguous()
        d = C.byref(tm.desc)
        gx = None
        if ctx.needs_input_grad[0]:
            wt = _tconv_pack(weights, cin, taps, True)
            gx = torch.empty(M, cin, device=x.device, dtype=torch.float32)
            check(LIB.hlhgat_tconv_fwd_ragged(g.data_ptr(), d, stage, cout, wt.data_ptr(), None,
                                              cin, taps, 0, 0, gx.data_ptr(), _stream(x)),
                  "tconv_bwd_data_ragged")
        gws = [None] * nb
        gbs = [None] * nb
        if any(ctx.needs_input_grad[4:]):
            gws = [torch.empty_like(w) for w in weights]
            gb = (torch.empty(cout, device=x.device, dtype=torch.float32)
                  if ctx.has_bias else None)
            wsf = LIB.hlhgat_tconv_bwd_weight_workspace_floats(tm.n_series, tm.t_max[stage], cin,
                                                               cout, taps)
            ws = torch.empty(max(wsf, 1), device=x.device, dtype=torch.float32)
            check(LIB.hlhgat_tconv_bwd_weight_ragged(
                x.data_ptr(), g.data_ptr(), d, stage, cin, cout, taps, nb,
                _arr(_lib.c_vp, [w.data_ptr() for w in gws]), c_couts, c_tbs, _ptr(gb),
                ws.data_ptr(), wsf, _stream(x)), "tconv_bwd_weight_ragged")
            if gb is not None:
                gbs = list(torch.split(gb, couts))
        return (gx, None, None, None, *gws, *gbs)


def temporal_conv_ragged(x: torch.Tensor, tm: TimeSeriesMap, stage: int, weights,
                         biases=None) -> torch.Tensor:
    """temporal_conv on the compact rows x [capacity, Cin] of ``stage`` of a
    TimeSeriesMap -> [capacity, sum Cout_b]: every series is padded with zeros
    at its own two ends (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:501-509 on each
    window alone); dead rows come out as zeros."""
    if torch.is_tensor(weights):
        weights = [weights]
        biases = None if biases is None else [biases]
    weights = list(weights)
    nb = len(weights)
    biases = [None] * nb if biases is None else list(biases)
    _req_rows(x, tm, stage, "temporal_conv_ragged")
    if len(biases) != nb or len({b is None for b in biases}) != 1:
        raise RuntimeError("hlhgat: temporal_conv_ragged needs a bias for every branch or for none")
    for w, b in zip(weights, biases):
        _req_dev(w, "weight")
        if w.dim() != 3 or w.size(1) != x.size(1):
            raise RuntimeError(f"hlhgat: temporal_conv_ragged weight {tuple(w.shape)} for "
                               f"{x.size(1)} input channels")
        if b is not None:
            _req_dev(b, "bias")
    return _TemporalConvRaggedFn.apply(x.contiguous(), tm, int(stage), nb,
                                       *[w.contiguous() for w in weights],
                                       *[None if b is None else b.contiguous() for b in biases])


class _LeakyMaxPoolTimeRaggedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tm, slope):
        Cc = x.size(1)
        y = torch.empty(tm.capacity(1), Cc, device=x.device, dtype=torch.float32)
        idx = torch.empty(tm.capacity(1), Cc, device=x.device, dtype=torch.int32)
        check(LIB.hlhgat_leaky_maxpool_time_fwd_ragged(x.data_ptr(), C.byref(tm.desc), Cc, slope,
                                                       y.data_ptr(), idx.data_ptr(), _stream(x)),
              "leaky_maxpool_time_fwd_ragged")
        ctx.tm, ctx.slope = tm, slope
        ctx.save_for_backward(x, idx)
        return y

    @staticmethod
    def backward(ctx, g):
        x, idx = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.empty_like(x)
        check(LIB.hlhgat_leaky_maxpool_time_bwd_ragged(x.data_ptr(), g.data_ptr(), idx.data_ptr(),
                                                       C.byref(ctx.tm.desc), x.size(1), ctx.slope,
                                                       gx.data_ptr(), _stream(x)),
              "leaky_maxpool_time_bwd_ragged")
        return gx, None, None


def leaky_maxpool_time_ragged(x: torch.Tensor, tm: TimeSeriesMap, slope: float) -> torch.Tensor:
    """leaky_maxpool_time with the map's window on the compact stage-0 rows
    x [capacity_0, C] -> compact stage-1 rows [capacity_1, C]: every series
    pooled over its own length (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:488, :505)."""
    _req_rows(x, tm, 0, "leaky_maxpool_time_ragged")
    return _LeakyMaxPoolTimeRaggedFn.apply(x.contiguous(), tm, float(slope))


class _TimeReadoutRaggedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, tm, slope):
        Cc = x.size(1)
        y = torch.empty(tm.n_series, 2 * Cc, device=x.device, dtype=torch.float32)
        idx = torch.empty(tm.n_series, Cc, device=x.device, dtype=torch.int32)
        check(LIB.hlhgat_time_readout_fwd_ragged(x.data_ptr(), C.byref(tm.desc), Cc, slope,
                                                 y.data_ptr(), idx.data_ptr(), _stream(x)),
              "time_readout_fwd_ragged")
        ctx.tm, ctx.slope = tm, slope
        ctx.save_for_backward(x, idx)
        return y

    @staticmethod
    def backward(ctx, g):
        x, idx = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.empty_like(x)
        check(LIB.hlhgat_time_readout_bwd_ragged(x.data_ptr(), g.data_ptr(), idx.data_ptr(),
                                                 C.byref(ctx.tm.desc), x.size(1), ctx.slope,
                                                 gx.data_ptr(), _stream(x)),
              "time_readout_bwd_ragged")
        return gx, None, None


def time_readout_ragged(x: torch.Tensor, tm: TimeSeriesMap, slope: float) -> torch.Tensor:
    """time_readout on the compact stage-1 rows x [capacity_1, C] -> [S, 2C]:
    the maximum and the mean over every series' own length
    (HL-HGAT-DEMO/lib/Hodge_Cheb_Conv.py:509-513)."""
    _req_rows(x, tm, 1, "time_readout_ragged")
    return _TimeReadoutRaggedFn.apply(x.contiguous(), tm, float(slope))


# ----------------------------------------------------------------------------
# segment mean (global_mean_pool / scatter_mean over sorted or listed members)
# ----------------------------------------------------------------------------
class _SegmentMeanFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seg_ptr, seg_rows, n_seg, out, covering, gsink):
        d = x.size(1)
        if out is None:
            out = torch.empty(n_seg, d, device=x.device, dtype=x.dtype)
        check(LIB.hlhgat_segment_mean_fwd(seg_ptr.data_ptr(), _ptr(seg_rows), n_seg,
                                          x.data_ptr(), _ld(x), d, out.data_ptr(), _ld(out),
                                          _stream(x)), "segment_mean_fwd")
        ctx.meta = (x.size(0), n_seg, seg_rows is not None, covering)
        ctx.gsink = gsink
        ctx.save_for_backward(seg_ptr, seg_rows if seg_rows is not None else seg_ptr)
        return out

    @staticmethod
    def backward(ctx, g):
        seg_ptr, seg_rows = ctx.saved_tensors
        n_rows, n_seg, listed, covering = ctx.meta
        g = _rows2d(g, "grad")
        if covering:
            # every row is listed (the trailing bucket: rows in no cluster,
            # written as zeros): no zero fill; into the slab's gradient when
            # this is the first gradient to land there (DenseConcat.grad_sink)
            sink, flag = ctx.gsink if ctx.gsink is not None else (None, None)
            if sink is not None and int(flag[0]) == 0 and sink.shape == (n_rows, g.size(1)):
                gx = sink
                flag[0] = 1
            else:
                gx = torch.empty(n_rows, g.size(1), device=g.device, dtype=g.dtype)
            check(LIB.hlhgat_pool_mean_bwd(seg_ptr.data_ptr(), seg_rows.data_ptr(), n_seg,
                                           g.data_ptr(), _ld(g), g.size(1), gx.data_ptr(),
                                           _ld(gx), n_rows, _stream(g)), "pool_mean_bwd")
            return gx, None, None, None, None, None, None
        gx = (torch.zeros if listed else torch.empty)(n_rows, g.size(1), device=g.device,
                                                      dtype=g.dtype)
        check(LIB.hlhgat_segment_mean_bwd(seg_ptr.data_ptr(), _ptr(seg_rows) if listed else None,
                                          n_seg, g.data_ptr(), _ld(g), g.size(1), gx.data_ptr(),
                                          _ld(gx), n_rows, _stream(g)), "segment_mean_bwd")
        return gx, None, None, None, None, None, None


class _SegmentMeanCatFn(torch.autograd.Function):
    """cat([segment_mean(x_i, ptr_i) for i], -1) with each mean written
    straight into its column block (no cat launch); contiguous segments."""

    @staticmethod
    def forward(ctx, n_seg, ptrs, side, *xs):
        # side: the edge chain's stream (ops.Chains) for part 0, whose input
        # was produced there and whose gradient is consumed there
        widths = [x.size(1) for x in xs]
        out = torch.empty(n_seg, sum(widths), device=xs[0].device, dtype=xs[0].dtype)
        if side is not None:
            # `out` comes from the main stream's pool: a block main freed may
            # still be read by main's queued kernels, so the side stream's write
            # waits for main
            side.wait_stream(torch.cuda.current_stream(xs[0].device))
            out.record_stream(side)
        c0 = 0
        for i, (x, p, w) in enumerate(zip(xs, ptrs, widths)):
            st = side.cuda_stream if (side is not None and i == 0) else _stream(x)
            check(LIB.hlhgat_segment_mean_fwd(p.data_ptr(), None, n_seg, x.data_ptr(), _ld(x), w,
                                              out.data_ptr() + 4 * c0, _ld(out), st),
                  "segment_mean_fwd")
            c0 += w
        ctx.meta = (n_seg, widths, [x.size(0) for x in xs])
        ctx.side = side
        ctx.save_for_backward(*ptrs)
        return out

    @staticmethod
    def backward(ctx, g):
        n_seg, widths, rows = ctx.meta
        g = _rows2d(g, "grad").contiguous()
        side = ctx.side
        if side is not None:
            side.wait_stream(torch.cuda.current_stream(g.device))
            g.record_stream(side)
        gx, c0 = [], 0
        for i, (p, w, n) in enumerate(zip(ctx.saved_tensors, widths, rows)):
            on_side = side is not None and i == 0
            with (torch.cuda.stream(side) if on_side else contextlib.nullcontext()):
                t = torch.empty(n, w, device=g.device, dtype=g.dtype)
                check(LIB.hlhgat_segment_mean_bwd(p.data_ptr(), None, n_seg,
                                                  g.data_ptr() + 4 * c0, _ld(g), w, t.data_ptr(),
                                                  _ld(t), n, _stream(t)),
                      "segment_mean_bwd")
            if on_side:
                t.record_stream(torch.cuda.current_stream(g.device))
            gx.append(t)
            c0 += w
        return (None, None, None, *gx)


def segment_mean_cat(xs: Sequence[torch.Tensor], seg_ptrs: Sequence[torch.Tensor],
                     n_seg: int, side=None) -> torch.Tensor:
    """torch.cat([segment_mean(x, p, n_seg) for x, p in zip(xs, seg_ptrs)], -1)
    (the readout x = cat(mean_pool(x_s), mean_pool(x_t)),
    lib/Hodge_ST_Model.py:636) without the cat: bitwise the same values."""
    xs = [_rows2d(x, "x") for x in xs]
    for x in xs:
        _req_dev(x, "x")
    for p in seg_ptrs:
        _req_dev(p, "seg_ptr", torch.int32)
        if p.numel() != n_seg + 1:
            raise RuntimeError(f"hlhgat: segment_mean_cat: seg_ptr has {p.numel()} entries, "
                               f"expected {n_seg + 1}")
    return _SegmentMeanCatFn.apply(int(n_seg), list(seg_ptrs), side, *xs)


def segment_mean(x: torch.Tensor, seg_ptr: torch.Tensor, n_seg: int,
                 seg_rows: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                 covering: bool = False, gsink=None) -> torch.Tensor:
    """Mean of x rows per segment.  seg_ptr int32 [n_seg+1]; members are the
    contiguous rows seg_ptr[s]..seg_ptr[s+1] (global_mean_pool over a sorted
    batch vector) or seg_rows[seg_ptr[s]:seg_ptr[s+1]] (scatter_mean).
    covering: seg_ptr has n_seg+2 entries and the extra segment lists the
    rows in no segment, so seg_rows is a permutation of x's rows (the pool
    tables of hodge_dataset.pool_tables); the backward then writes every row
    (zeros for that bucket) without a zero fill, into ``gsink`` (a
    DenseConcat.grad_sink of x) when it is the first gradient there.  out: a
    [n_seg, d] destination (a DenseConcat sink) instead of a new tensor."""
    _req_dev(x, "x")
    _req_dev(seg_ptr, "seg_ptr", torch.int32)
    if seg_rows is not None:
        _req_dev(seg_rows, "seg_rows", torch.int32)
    x = _rows2d(x, "x")
    if covering and (seg_rows is None or seg_ptr.numel() != n_seg + 2
                     or seg_rows.numel() != x.size(0)):
        raise RuntimeError("hlhgat: segment_mean(covering=True) needs seg_ptr [n_seg+2] and "
                           "seg_rows listing every row of x")
    if out is not None and (tuple(out.shape) != (n_seg, x.size(1)) or out.stride(1) != 1
                            or out.device != x.device or out.dtype != x.dtype):
        raise RuntimeError(f"hlhgat: segment_mean out {tuple(out.shape)} does not match "
                           f"({n_seg}, {x.size(1)})")
    if gsink is not None and (gsink[0] is None or gsink[0].shape != x.shape):
        gsink = None
    return _SegmentMeanFn.apply(x, seg_ptr, seg_rows, int(n_seg), out, bool(covering), gsink)


# ----------------------------------------------------------------------------
# BatchNorm1d (training statistics) + optional fused ReLU
# ----------------------------------------------------------------------------
def batch_norm_act(x: torch.Tensor, bn: torch.nn.BatchNorm1d, relu: bool = False,
                   valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bn(x) followed by ReLU when ``relu``; training mode (or no running
    stats) uses the HIP batch-statistics kernels; eval mode the running
    statistics: inference (nothing to differentiate) in one HIP launch
    (hlhgat_bn_apply_running, the ReLU fused), an eval-mode BatchNorm inside
    a differentiated graph through ATen's eval kernel (its autograd)."""
    _req_dev(x, "x")
    if x.dim() != 2:
        raise RuntimeError("hlhgat: batch_norm_act expects [N, C] input")
    use_batch = bn.training or not bn.track_running_stats
    if not use_batch:
        grads = torch.is_grad_enabled() and (
            x.requires_grad or any(t is not None and t.requires_grad
                                   for t in (bn.weight, bn.bias)))
        if not grads and x.size(0) > 0:
            x = _rows2d(x, "x")
            y = torch.empty(x.shape, device=x.device, dtype=x.dtype)
            check(LIB.hlhgat_bn_apply_running(
                x.data_ptr(), _ld(x), x.size(0), x.size(1), _ptr(bn.weight), _ptr(bn.bias),
                bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(bn.eps),
                1 if relu else 0, y.data_ptr(), _ld(y), _stream(x)), "bn_apply_running")
            return y
        y = torch.nn.functional.batch_norm(x, bn.running_mean, bn.running_var, bn.weight,
                                           bn.bias, False, 0.0, bn.eps)
        return torch.relu(y) if relu else y
    if x.size(0) < 2 and bn.training:
        raise ValueError(f"Expected more than 1 value per channel when training, got input "
                         f"size {tuple(x.shape)}")
    if sync_bn_group(bn) is not None:
        return _SyncBatchNormFn.apply(x, bn.weight, bn.bias, bool(relu), valid,
                                      sync_bn_group(bn), _bn_args(bn))
    return _ext.bn_act(x, *_bn_args(bn), bool(relu), valid)


# ----------------------------------------------------------------------------
# SyncBatchNorm (hlhgat.distributed.convert_sync_batchnorm): batch statistics
# over every rank's rows -- the single-process statistics of the whole
# data-parallel batch (parity caveat 1).
# ----------------------------------------------------------------------------
class _SyncGroup:
    """Marker held by a BatchNorm1d in SyncBatchNorm mode: its process group
    (None = the default group)."""

    def __init__(self, group=None):
        self.group = group


def sync_bn_group(bn) -> Optional[_SyncGroup]:
    """The _SyncGroup of a BatchNorm1d in SyncBatchNorm mode (training-mode
    batch statistics only), else None."""
    g = getattr(bn, "_hlhgat_sync", None)
    if g is None or not _bn_uses_batch_stats(bn):
        return None
    return g


def has_sync_bn(module: torch.nn.Module) -> bool:
    """True when a BatchNorm1d of ``module`` normalises in SyncBatchNorm mode
    now (hlhgat.distributed.convert_sync_batchnorm, training mode)."""
    return any(isinstance(m, torch.nn.BatchNorm1d) and sync_bn_group(m) is not None
               for m in module.modules())


_SYNC_WS = {}
_SYNC_WS_RETIRED = []
# SYNCBN_CHAINS (probe only): run SyncBatchNorm models with the persistent
# node / edge chains (ops.Chains) instead of a fork / join per block -- their
# capture under RCCL segfaults in hipStreamEndCapture (round 5; issuing the
# statistics all-reduces from one dedicated stream does not change that,
# round 6: tools/probes/syncbn_capture_probe.py, profiles/r06/)
SYNCBN_CHAINS = os.environ.get("HLHGAT_SYNCBN_CHAINS", "0") == "1"


def _sync_workspace(x: torch.Tensor, n: int, Cc: int) -> torch.Tensor:
    """Zeroed BatchNorm workspace per (device, stream); outgrown ones are
    retired, not freed (a captured graph may still hold the address)."""
    key = (x.device.index, _stream(x))
    need = int(LIB.hlhgat_bn_workspace_bytes(n, Cc))
    ws = _SYNC_WS.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            _SYNC_WS_RETIRED.append(ws)
        ws = torch.zeros(max(need, 1 << 20, 2 * (ws.numel() if ws is not None else 0)),
                         dtype=torch.uint8, device=x.device)
        _SYNC_WS[key] = ws
    return ws


def _sum_over_ranks(t: torch.Tensor, group) -> torch.Tensor:
    """[1, len(t)]: the fp64 sums of every rank, added by an all-reduce (SUM)
    -- RCCL under nccl, which a hipGraph capture records like the attention
    max's all-reduce (an all_gather_into_tensor of the same vector did not
    capture: hipStreamEndCapture segfaulted, ProcessGroupNCCL's watchdog then
    queried an event of the capturing stream; round 4).  Every rank receives
    the same bits; one rank (or no process group) returns t itself, so the
    statistics are bitwise the single-process BatchNorm's."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return t.view(1, -1)
    from .distributed import collectives_on
    if not collectives_on(group):
        return t.view(1, -1)
    out = t.clone()
    # on the current stream (a SyncBatchNorm model's block section runs with
    # per-block fork / join, not ops.Chains: see _PyrHead.forward)
    dist.all_reduce(out, op=dist.ReduceOp.SUM, group=group)
    return out.view(1, -1)


class _SyncBatchNormFn(torch.autograd.Function):
    """BatchNorm1d (+ ReLU) with statistics over all ranks: local fp64 sums
    (hlhgat_bn_sums_fwd) -> all-reduce (SUM) -> apply with the totals
    (hlhgat_bn_sync_fwd_apply, one gathered row).  Backward as torch.nn.SyncBatchNorm: global
    sum g / sum g (x - mean) for dx, local dweight / dbias (DDP averages
    them)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, valid, sg, bn_args):
        _, _, rm, rv, nbt, momentum, eps = bn_args
        x = _rows2d(x, "x")
        n, Cc = x.shape
        y = torch.empty(n, Cc, device=x.device, dtype=x.dtype)
        ws = _sync_workspace(x, n, Cc)
        L = int(LIB.hlhgat_bn_sums_len(Cc))
        sums = torch.empty(L, dtype=torch.float64, device=x.device)
        check(LIB.hlhgat_bn_sums_fwd(x.data_ptr(), _ld(x), y.data_ptr(), _ld(y), n, _ptr(valid),
                                     Cc, sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x)),
              "bn_sums_fwd")
        gathered = _sum_over_ranks(sums, sg.group).contiguous()
        mean = torch.empty(Cc, device=x.device, dtype=x.dtype)
        invstd = torch.empty(Cc, device=x.device, dtype=x.dtype)
        check(LIB.hlhgat_bn_sync_fwd_apply(
            x.data_ptr(), _ld(x), n, _ptr(valid), Cc, gathered.data_ptr(), gathered.size(0),
            _ptr(weight), _ptr(bias), _ptr(rm), _ptr(rv), _ptr(nbt), float(momentum), float(eps),
            int(relu), y.data_ptr(), _ld(y), mean.data_ptr(), invstd.data_ptr(), _stream(x)),
            "bn_sync_fwd_apply")
        ctx.save_for_backward(x, y if relu else None, weight, mean, invstd, valid)
        ctx.sg = sg
        ctx.has_b = bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, weight, mean, invstd, valid = ctx.saved_tensors
        gy = _rows2d(gy, "dy")
        n, Cc = x.shape
        dx = torch.empty_like(x)
        need_w = weight is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_b and ctx.needs_input_grad[2]
        dw = torch.empty(Cc, device=x.device, dtype=x.dtype) if need_w else None
        db = torch.empty(Cc, device=x.device, dtype=x.dtype) if need_b else None
        ws = _sync_workspace(x, n, Cc)
        sums = torch.empty(int(LIB.hlhgat_bn_sums_len(Cc)), dtype=torch.float64, device=x.device)
        check(LIB.hlhgat_bn_sums_bwd(
            x.data_ptr(), _ld(x), _ptr(y), _ld(y) if y is not None else 0, gy.data_ptr(), _ld(gy),
            dx.data_ptr(), _ld(dx), n, _ptr(valid), Cc, mean.data_ptr(), invstd.data_ptr(),
            sums.data_ptr(), _ptr(dw), _ptr(db), ws.data_ptr(), ws.numel(), _stream(x)),
            "bn_sums_bwd")
        gathered = _sum_over_ranks(sums, ctx.sg.group).contiguous()
        check(LIB.hlhgat_bn_sync_bwd_apply(
            x.data_ptr(), _ld(x), _ptr(y), _ld(y) if y is not None else 0, gy.data_ptr(), _ld(gy),
            n, _ptr(valid), Cc, _ptr(weight), mean.data_ptr(), invstd.data_ptr(),
            gathered.data_ptr(), gathered.size(0), dx.data_ptr(), _ld(dx), _stream(x)),
            "bn_sync_bwd_apply")
        return dx, dw, db, None, None, None, None


# ----------------------------------------------------------------------------
# Adam on a flat parameter buffer (hlhgat_adam_flat; hlhgat.train.TrainStep)
# ----------------------------------------------------------------------------
def adam_prepare(grad: torch.Tensor, step: torch.Tensor) -> None:
    """Zero the flat gradient buffer and increment the device step count in
    one launch (hlhgat_adam_prepare); adam_flat(..., prepared=True) then
    uses that count."""
    _req_dev(grad, "grad")
    _req_dev(step, "step")
    if not grad.is_contiguous():
        raise RuntimeError("hlhgat: adam_prepare: grad must be contiguous")
    check(LIB.hlhgat_adam_prepare(grad.data_ptr(), grad.numel(), step.data_ptr(), _stream(grad)),
          "adam_prepare")


def adam_flat(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor,
              exp_avg_sq: torch.Tensor, step: torch.Tensor, lr, betas, eps: float,
              weight_decay: float, prepared: bool = False) -> None:
    """One torch.optim.Adam (fused, capturable) update of a flat fp32 buffer;
    `step` the fp32 step count on device (incremented; prepared=True: already
    incremented by adam_prepare).  `lr` is a Python float (a by-value kernel
    argument: a captured launch keeps it) or a 0-dim / 1-element fp64 tensor
    on the same device, read by the launch itself (hlhgat_adam_flat_dev*: a
    captured launch follows later fills of the tensor).  Equal values give
    equal bits either way."""
    for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"),
                    (exp_avg_sq, "exp_avg_sq"), (step, "step")):
        _req_dev(t, name)
        if not t.is_contiguous():
            raise RuntimeError(f"hlhgat: adam_flat: {name} must be contiguous")
    n = param.numel()
    if not (grad.numel() == exp_avg.numel() == exp_avg_sq.numel() == n):
        raise RuntimeError("hlhgat: adam_flat: buffer sizes differ")
    hyper = (float(betas[0]), float(betas[1]), float(eps), float(weight_decay), _stream(param))
    if torch.is_tensor(lr):
        _req_dev(lr, "lr", torch.float64)
        if lr.numel() != 1 or lr.device != param.device:
            raise RuntimeError(f"hlhgat: adam_flat: a tensor lr must be one fp64 value on "
                               f"{param.device} (got {tuple(lr.shape)} on {lr.device})")
        fn = LIB.hlhgat_adam_flat_dev_prepared if prepared else LIB.hlhgat_adam_flat_dev
        lr_arg = lr.data_ptr()
    else:
        fn = LIB.hlhgat_adam_flat_prepared if prepared else LIB.hlhgat_adam_flat
        lr_arg = float(lr)
    check(fn(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
             step.data_ptr(), lr_arg, *hyper), "adam_flat")


class _L1LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(LIB.hlhgat_l1_loss_fwd(x.data_ptr(), y.data_ptr(), x.numel(), loss.data_ptr(),
                                     _stream(x)), "l1_loss_fwd")
        ctx.save_for_backward(x, y)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(LIB.hlhgat_l1_loss_bwd(x.data_ptr(), y.data_ptr(), x.numel(), g.data_ptr(),
                                     dx.data_ptr(), _stream(x)), "l1_loss_bwd")
        return dx, None


def l1_loss(input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """torch.nn.functional.l1_loss(input, target) (mean) in one launch each way
    (hlhgat_l1_loss_fwd / _bwd): the same input gradient bit for bit; the
    loss value is the fp32 mean summed in a fixed order.  No gradient flows
    into target (the regression labels)."""
    _req_dev(input, "input")
    if input.shape != target.shape:
        raise RuntimeError(f"hlhgat: l1_loss shapes differ: {tuple(input.shape)} vs "
                           f"{tuple(target.shape)}")
    if target.requires_grad:
        raise RuntimeError("hlhgat: l1_loss: target must not require grad")
    if input.numel() == 0:
        raise RuntimeError("hlhgat: l1_loss of an empty tensor")
    x = input.contiguous()
    return _L1LossFn.apply(x, target.to(torch.float32).contiguous())


class _BCELogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, div):
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(LIB.hlhgat_bce_logits_fwd(x.data_ptr(), y.data_ptr(), x.numel(), div,
                                        loss.data_ptr(), _stream(x)), "bce_logits_fwd")
        ctx.div = div
        ctx.save_for_backward(x, y)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(LIB.hlhgat_bce_logits_bwd(x.data_ptr(), y.data_ptr(), x.numel(), ctx.div,
                                        g.data_ptr(), dx.data_ptr(), _stream(x)),
              "bce_logits_bwd")
        return dx, None, None


def bce_with_logits(input: torch.Tensor, target: torch.Tensor,
                    reduction: str = "mean") -> torch.Tensor:
    """F.binary_cross_entropy_with_logits(input, target, reduction=...) for
    "mean" / "sum" without weights, one launch each way
    (hlhgat_bce_logits_fwd / _bwd); the loss value is the fp32 sum in a fixed
    order.  No gradient flows into target (the labels)."""
    _req_dev(input, "input")
    if input.shape != target.shape:
        raise RuntimeError(f"hlhgat: bce_with_logits shapes differ: {tuple(input.shape)} vs "
                           f"{tuple(target.shape)}")
    if target.requires_grad:
        raise RuntimeError("hlhgat: bce_with_logits: target must not require grad")
    if input.numel() == 0:
        raise RuntimeError("hlhgat: bce_with_logits of an empty tensor")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"hlhgat: bce_with_logits reduction {reduction!r}")
    div = float(input.numel()) if reduction == "mean" else 1.0
    return _BCELogitsFn.apply(input.contiguous(), target.to(torch.float32).contiguous(), div)


class _MSELossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, div):
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        check(LIB.hlhgat_mse_loss_fwd(x.data_ptr(), y.data_ptr(), x.numel(), div,
                                      loss.data_ptr(), _stream(x)), "mse_loss_fwd")
        ctx.div = div
        ctx.save_for_backward(x, y)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(LIB.hlhgat_mse_loss_bwd(x.data_ptr(), y.data_ptr(), x.numel(), ctx.div,
                                      g.data_ptr(), dx.data_ptr(), _stream(x)), "mse_loss_bwd")
        return dx, None, None


def mse_loss(input: torch.Tensor, target: torch.Tensor, reduction: str = "mean") -> torch.Tensor:
    """F.mse_loss(input, target, reduction=...) for "mean" / "sum", one launch
    each way (hlhgat_mse_loss_fwd / _bwd): the brain notebook's training
    criterion.  The loss value is the fp32 sum of squares in a fixed order;
    dx = (x - y) * (2 g / div).  No gradient flows into target."""
    _req_dev(input, "input")
    if input.shape != target.shape:
        raise RuntimeError(f"hlhgat: mse_loss shapes differ: {tuple(input.shape)} vs "
                           f"{tuple(target.shape)}")
    if target.requires_grad:
        raise RuntimeError("hlhgat: mse_loss: target must not require grad")
    if input.numel() == 0:
        raise RuntimeError("hlhgat: mse_loss of an empty tensor")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"hlhgat: mse_loss reduction {reduction!r}")
    div = float(input.numel()) if reduction == "mean" else 1.0
    return _MSELossFn.apply(input.contiguous(), target.to(torch.float32).contiguous(), div)


def _loss_workspace(n: int, like: torch.Tensor) -> Optional[torch.Tensor]:
    """The partial-record workspace of the reduced losses (None while one
    workgroup finishes itself): torch.empty on the current stream, so a
    captured step takes it from the graph pool."""
    if n <= _lib.LOSS_ONE_LAUNCH_MAX:
        return None
    return torch.empty(LIB.hlhgat_loss_workspace_bytes(n), device=like.device, dtype=torch.uint8)


class _BCEReduceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mask, ignore_nan, red, alpha, gamma, scale):
        n = x.numel()
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        ssum = torch.empty(1, device=x.device, dtype=torch.float32)
        stats = torch.empty(4, device=x.device, dtype=torch.int64)
        ws = _loss_workspace(n, x)
        check(LIB.hlhgat_bce_reduce_fwd(x.data_ptr(), y.data_ptr(), _ptr(mask), n,
                                        int(ignore_nan), red, alpha, gamma, scale, _ptr(ws),
                                        0 if ws is None else ws.numel(), loss.data_ptr(),
                                        ssum.data_ptr(), stats.data_ptr(), _stream(x)),
              "bce_reduce_fwd")
        ctx.mode = (int(ignore_nan), red, alpha, gamma, scale)
        ctx.save_for_backward(x, y, mask, ssum, stats)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        x, y, mask, ssum, stats = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(x)
        check(LIB.hlhgat_bce_reduce_bwd(x.data_ptr(), y.data_ptr(), _ptr(mask), x.numel(),
                                        *ctx.mode, ssum.data_ptr(), stats.data_ptr(),
                                        g.data_ptr(), dx.data_ptr(), _stream(x)),
              "bce_reduce_bwd")
        return dx, None, None, None, None, None, None, None


def bce_logits_loss(input: torch.Tensor, target: torch.Tensor,
                    mask: Optional[torch.Tensor] = None, *, ignore_nan: bool = False,
                    reduction: str = "mean", focal: Optional[Tuple[float, float, float]] = None,
                    return_stats: bool = False):
    """The torch expression

        m = mask.bool() & ~isnan(target)      (each half only when asked for)
        b = F.binary_cross_entropy_with_logits(input[m], target[m], reduction=reduction)

    without the data-dependent gather: the selection is made on the device
    inside the reduction (hlhgat_bce_reduce_fwd / _bwd), so the shapes are
    static and the call captures into a hipGraph.  ``focal=(alpha, gamma,
    scale)`` (with reduction "mean") returns scale * alpha * (1 - exp(-b)) **
    gamma * b, the reference's FocalLoss (lib/Loss_function.py:14-26) with
    scale = 1e4; gamma is 0 or >= 1.  The input gradient is exactly +0.0 at
    excluded positions, whose input and target values (NaN, inf) enter nothing.

    Unlike torch, an EMPTY selection gives loss 0 and a zero gradient, not
    NaN: one all-missing batch must not poison Adam inside a captured step.

    One or two launches forward (two above 16384 elements), one backward; the
    result is a function of the inputs alone (fixed summation order, bitwise
    equal eager or replayed).  A bool / uint8 mask is read as it is; any other
    dtype costs one ATen launch (mask != 0).  No gradient flows into target or
    mask.  ``return_stats=True`` also returns int64 [cnt, tp, fp, fn] over the
    selection (prediction input > 0, positive target > 0.5): the counts the
    TSP loop's F1 is built from (main_TSP...:346-347)."""
    _req_dev(input, "input")
    if input.shape != target.shape:
        raise RuntimeError(f"hlhgat: bce_logits_loss shapes differ: {tuple(input.shape)} vs "
                           f"{tuple(target.shape)}")
    if target.requires_grad or (mask is not None and mask.requires_grad):
        raise RuntimeError("hlhgat: bce_logits_loss: target / mask must not require grad")
    if input.numel() == 0:
        raise RuntimeError("hlhgat: bce_logits_loss of an empty tensor")
    if focal is not None:
        if reduction != "mean":
            raise ValueError("hlhgat: bce_logits_loss: focal is a function of the mean")
        alpha, gamma, scale = (float(v) for v in focal)
        if not (gamma == 0.0 or gamma >= 1.0):
            raise ValueError(f"hlhgat: bce_logits_loss: focal gamma {gamma} (0 or >= 1)")
        red = _lib.LOSS_FOCAL
    elif reduction in ("mean", "sum"):
        alpha = gamma = scale = 0.0
        red = _lib.LOSS_MEAN if reduction == "mean" else _lib.LOSS_SUM
    else:
        raise ValueError(f"hlhgat: bce_logits_loss reduction {reduction!r}")
    if mask is not None:
        if mask.shape != input.shape or mask.device != input.device:
            raise RuntimeError(f"hlhgat: bce_logits_loss: mask {tuple(mask.shape)} on "
                               f"{mask.device} does not match input {tuple(input.shape)}")
        if mask.dtype == torch.bool:
            mask = mask.contiguous().view(torch.uint8)
        elif mask.dtype == torch.uint8:
            mask = mask.contiguous()
        else:
            mask = (mask != 0).contiguous().view(torch.uint8)
    loss, stats = _BCEReduceFn.apply(input.contiguous(), target.to(torch.float32).contiguous(),
                                     mask, bool(ignore_nan), red, alpha, gamma, scale)
    return (loss, stats) if return_stats else loss


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, label, ignore_index, red):
        rows, cols = x.shape
        ld = x.stride(0) if rows > 1 else cols
        loss = torch.empty((), device=x.device, dtype=torch.float32)
        stats = torch.empty(2, device=x.device, dtype=torch.int64)
        ws = _loss_workspace(rows, x)
        check(LIB.hlhgat_cross_entropy_fwd(x.data_ptr(), ld, rows, cols, label.data_ptr(),
                                           ignore_index, red, _ptr(ws),
                                           0 if ws is None else ws.numel(), loss.data_ptr(),
                                           stats.data_ptr(), _stream(x)), "cross_entropy_fwd")
        ctx.args = (ld, rows, cols, ignore_index, red)
        ctx.save_for_backward(x, label, stats)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, g, _gstats):
        x, label, stats = ctx.saved_tensors
        ld, rows, cols, ignore_index, red = ctx.args
        g = g.contiguous()
        dx = torch.empty((rows, cols), device=x.device, dtype=torch.float32)
        check(LIB.hlhgat_cross_entropy_bwd(x.data_ptr(), ld, rows, cols, label.data_ptr(),
                                           ignore_index, red, stats.data_ptr(), g.data_ptr(),
                                           dx.data_ptr(), cols, _stream(x)),
              "cross_entropy_bwd")
        return dx, None, None, None


def cross_entropy(input: torch.Tensor, label: torch.Tensor, *, ignore_index: int = -100,
                  reduction: str = "mean", return_stats: bool = False):
    """F.cross_entropy(input [R, C], label [R] of class indices, ignore_index=...,
    reduction="mean" | "sum") for C <= 64 on the HIP path
    (hlhgat_cross_entropy_fwd / _bwd): one or two launches forward (two above
    16384 rows), one backward, fixed summation order.  "mean" divides by the
    number of non-ignored rows, as torch does.  A column block of a wider
    tensor (unit column stride) is read in place through its row stride; any
    other layout is made contiguous first.

    Unlike torch, all rows ignored gives loss 0 and a zero gradient, not NaN,
    and a label that is neither ignore_index nor in [0, C) does not
    device-assert: its row is ignored and the device error word is raised
    (check_device_errors / TrainStep then raise RuntimeError).

    No gradient flows into label.  ``return_stats=True`` also returns int64
    [cnt, correct]: the non-ignored rows and those whose (lowest-index) argmax
    is the label, the accuracy the CIFAR loop prints."""
    _req_dev(input, "input")
    if input.dim() != 2 or label.dim() != 1 or label.size(0) != input.size(0):
        raise RuntimeError(f"hlhgat: cross_entropy wants input [R, C] and label [R], got "
                           f"{tuple(input.shape)} and {tuple(label.shape)}")
    if label.is_floating_point() or label.device != input.device:
        raise RuntimeError("hlhgat: cross_entropy: label must hold class indices on the input's "
                           "device")
    rows, cols = input.shape
    if rows == 0:
        raise RuntimeError("hlhgat: cross_entropy of an empty tensor")
    if not 1 <= cols <= _lib.CE_MAX_CLASSES:
        raise RuntimeError(f"hlhgat: cross_entropy: C = {cols} outside [1, "
                           f"{_lib.CE_MAX_CLASSES}] (hlhgat.nn.CrossEntropyLoss sends larger C "
                           f"to torch)")
    if reduction not in ("mean", "sum"):
        raise ValueError(f"hlhgat: cross_entropy reduction {reduction!r}")
    red = _lib.LOSS_MEAN if reduction == "mean" else _lib.LOSS_SUM
    x = input
    if not (x.stride(1) == 1 and (rows == 1 or x.stride(0) >= cols)):
        x = x.contiguous()
    loss, stats = _CrossEntropyFn.apply(x, label.to(torch.int64).contiguous(), int(ignore_index),
                                        red)
    return (loss, stats) if return_stats else loss


# ----------------------------------------------------------------------------
# evaluation metrics (csrc/metrics.hip)
# ----------------------------------------------------------------------------
_AP_WS = {}  # (device, stream, n, C) -> workspace, at most _AP_WS_MAX (oldest out first)
_AP_WS_MAX = 8


def _ap_workspace(x: torch.Tensor, n: int, Cc: int) -> torch.Tensor:
    """The sort workspace of average_precision.  Eager calls share one per
    (device, stream, n, C) -- the epoch loop needs two, train and validation --
    in a cache of at most _AP_WS_MAX entries, so a caller whose n varies from
    call to call does not grow it without bound (a dropped workspace goes back
    to torch's allocator in stream order).  Inside a graph capture the
    workspace is a fresh torch.empty from the graph's own pool, which lives as
    long as the graph and is never handed to an eager call."""
    need = max(int(LIB.hlhgat_average_precision_workspace_bytes(n, Cc)), 256)
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(need, dtype=torch.uint8, device=x.device)
    key = (x.device.index, _stream(x), n, Cc)
    ws = _AP_WS.pop(key, None)
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
    _AP_WS[key] = ws  # most recently used last
    while len(_AP_WS) > _AP_WS_MAX:
        _AP_WS.pop(next(iter(_AP_WS)))
    return ws


def average_precision(pred: torch.Tensor, label: torch.Tensor):
    """(ap [C] fp64, counts [C, 3] int32) on the device: per class (column)
    scikit-learn's average_precision_score over the rows whose label is not
    NaN, the per-class quantity of the reference's eval_ap
    (lib/Hodge_Dataset.py:73-94); counts = labelled rows, labels == 1, labels
    == 0.  A class without a 1 or without a 0, or with a non-finite score in a
    labelled row, gets NaN.  Ties (equal fp32 scores, -0.0 == +0.0) form one
    threshold.  A label that is neither NaN, 0 nor 1 counts as a negative and
    raises the device error word.  pred / label: [n, C]; a column block of a
    wider tensor (unit column stride) is read in place.  No host
    synchronisation: the call captures into a hipGraph.  Not differentiable."""
    _req_dev(pred, "pred")
    if pred.dim() != 2 or pred.shape != label.shape or label.device != pred.device:
        raise RuntimeError(f"hlhgat: average_precision wants pred and label [n, C] on one device, "
                           f"got {tuple(pred.shape)} on {pred.device} and {tuple(label.shape)} on "
                           f"{label.device}")
    n, Cc = pred.shape
    if n * Cc >= 2 ** 31 - 1:
        raise RuntimeError(f"hlhgat: average_precision: n * C = {n * Cc} out of int32 range")
    with torch.no_grad():
        x = _rows2d(pred.detach(), "pred")
        y = _rows2d(label.detach().to(torch.float32), "label")
        ap = torch.empty(Cc, dtype=torch.float64, device=x.device)
        counts = torch.empty((Cc, 3), dtype=torch.int32, device=x.device)
        ws = _ap_workspace(x, n, Cc)
        check(LIB.hlhgat_average_precision(x.data_ptr(), _ld(x), y.data_ptr(), _ld(y), n, Cc,
                                           ap.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _stream(x)), "average_precision")
    return ap, counts


def _req_i64_scalar(t: torch.Tensor, name: str, like: torch.Tensor) -> None:
    _req_dev(t, name, torch.int64)
    if t.numel() != 1 or t.device != like.device:
        raise RuntimeError(f"hlhgat: {name} must hold one int64 on {like.device}")


def collect_rows(x: torch.Tensor, buf: torch.Tensor, cursor: torch.Tensor) -> None:
    """Append the rows of x ([n, d], or [n] when buf is [capacity, 1]) to buf
    [capacity, d] at row ``cursor`` (one int64 on the device) and advance the
    cursor on the device (hlhgat_collect_rows): the device-side
    ``y_pred.extend(out)``.  Rows that do not fit are not written, the cursor
    stays and the device error word is raised.  A strided x (unit column
    stride) is read in place.  No host synchronisation: the call captures, and
    a replay appends behind the previous replay's rows."""
    _req_dev(x, "x")
    _req_dev(buf, "buf")
    if buf.dim() != 2 or not buf.is_contiguous() or buf.device != x.device or buf.size(1) < 1:
        raise RuntimeError(f"hlhgat: collect_rows: buf must be contiguous [capacity, d >= 1] on "
                           f"{x.device}, got {tuple(buf.shape)}")
    _req_i64_scalar(cursor, "cursor", x)
    cap, d = buf.shape
    x = x.detach()
    if x.dim() == 1 and d == 1:
        n, ld = x.size(0), (x.stride(0) if x.size(0) > 1 else 1)
        if ld < 1:
            x, ld = x.contiguous(), 1
    else:
        if x.dim() != 2 or x.size(1) != d:
            raise RuntimeError(f"hlhgat: collect_rows: x {tuple(x.shape)} does not match buf "
                               f"[{cap}, {d}]")
        x = _rows2d(x, "x")
        n, ld = x.size(0), _ld(x)
    check(LIB.hlhgat_collect_rows(x.data_ptr(), ld, n, d, buf.data_ptr(), cap, cursor.data_ptr(),
                                  _stream(x)), "collect_rows")


def _vec_ld(t: torch.Tensor, name: str):
    """A [E] or [E, 1] tensor as (tensor, element stride >= 1)."""
    if t.dim() == 2 and t.size(1) == 1:
        t = t[:, 0]
    if t.dim() != 1:
        raise RuntimeError(f"hlhgat: {name} must be [E] or [E, 1] (got {tuple(t.shape)})")
    if t.size(0) > 1 and t.stride(0) < 1:
        t = t.contiguous()
    return t, (t.stride(0) if t.size(0) > 1 else 1)


def f1_per_graph(logits: torch.Tensor, label: torch.Tensor, seg_ptr: torch.Tensor,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """f1 [G] fp32: torchmetrics' BinaryF1Score() (threshold 0.5) of every
    graph of a batch in one launch (hlhgat_f1_per_graph), the body of the TSP
    test() loop (main_TSP...:344-347).  logits / label: [E] or [E, 1] fp32 (a
    column of a wider tensor is read in place); seg_ptr: int32 [G + 1] row
    offsets, rows from seg_ptr[G] on (padding) belong to no graph.  Per graph:
    if every logit lies in [0, 1] the prediction is ``p > 0.5``, otherwise
    ``sigmoid(p) > 0.5`` (torchmetrics' formatting rule); f1 = 2tp / (2tp + fp
    + fn), 0 for 0 / 0.  A label other than 0 or 1 counts as a negative and
    raises the device error word.  No host synchronisation."""
    _req_dev(logits, "logits")
    _req_dev(label, "label")
    _req_dev(seg_ptr, "seg_ptr", torch.int32)
    x, ldp = _vec_ld(logits.detach(), "logits")
    y, ldy = _vec_ld(label.detach(), "label")
    if x.size(0) != y.size(0) or y.device != x.device or seg_ptr.device != x.device or \
            seg_ptr.dim() != 1 or seg_ptr.numel() < 1 or not seg_ptr.is_contiguous():
        raise RuntimeError(f"hlhgat: f1_per_graph wants logits and label [E] and contiguous "
                           f"seg_ptr [G + 1] on one device, got {tuple(logits.shape)}, "
                           f"{tuple(label.shape)}, {tuple(seg_ptr.shape)}")
    G = seg_ptr.numel() - 1
    if out is None:
        out = torch.empty(G, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or out.device != x.device or out.numel() != G or \
            not out.is_contiguous():
        raise RuntimeError(f"hlhgat: f1_per_graph: out must be contiguous fp32 [{G}] on {x.device}")
    check(LIB.hlhgat_f1_per_graph(x.data_ptr(), ldp, y.data_ptr(), ldy, seg_ptr.data_ptr(), G,
                                  x.size(0), out.data_ptr(), _stream(x)), "f1_per_graph")
    return out


def argmax_correct(out: torch.Tensor, label: torch.Tensor, correct: torch.Tensor,
                   seen: Optional[torch.Tensor] = None) -> None:
    """correct += the rows of out [n, C] whose argmax is label [n] (int64), and
    seen += n: ``correct += int((out.argmax(1) == y).sum())`` of the CIFAR
    loop (main_cifar10SP...:146-161) without the read (hlhgat_argmax_correct).
    correct / seen: one int64 each on the device.  The argmax is the first
    index of the greatest value, NaN greatest.  A label outside [0, C) matches
    nothing and raises the device error word.  No host synchronisation."""
    _req_dev(out, "out")
    _req_dev(label, "label", torch.int64)
    if out.dim() != 2 or out.size(1) < 1 or label.dim() != 1 or label.size(0) != out.size(0) or \
            label.device != out.device:
        raise RuntimeError(f"hlhgat: argmax_correct wants out [n, C >= 1] and label [n] on one "
                           f"device, got {tuple(out.shape)} and {tuple(label.shape)}")
    _req_i64_scalar(correct, "correct", out)
    if seen is not None:
        _req_i64_scalar(seen, "seen", out)
    x = _rows2d(out.detach(), "out")
    y = label.contiguous()
    check(LIB.hlhgat_argmax_correct(x.data_ptr(), _ld(x), x.size(0), x.size(1), y.data_ptr(),
                                    correct.data_ptr(), _ptr(seen), _stream(x)), "argmax_correct")


REGRESSION_FIELDS = ("n", "sum_abs", "sum_sq", "mean_pred", "mean_y", "std_pred", "std_y", "corr")


def regression_summary(pred: torch.Tensor, y: torch.Tensor, count: torch.Tensor,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp64 [8] on the device, in the order of REGRESSION_FIELDS, over the
    first min(count, capacity) values of the contiguous fp32 buffers pred / y
    [capacity] (count: one int64 on the device, a collector's cursor), in one
    launch (hlhgat_regression_summary): N, sum |pred - y|, sum (pred - y)^2,
    the means, the unbiased standard deviations and the notebook's
    mean(z(pred) * z(y)).  Two passes in fp64, fixed order.  No host
    synchronisation."""
    _req_dev(pred, "pred")
    _req_dev(y, "y")
    _req_i64_scalar(count, "count", pred)
    if pred.numel() != y.numel() or y.device != pred.device or not pred.is_contiguous() or \
            not y.is_contiguous():
        raise RuntimeError(f"hlhgat: regression_summary wants contiguous pred and y of one size on "
                           f"one device, got {tuple(pred.shape)} and {tuple(y.shape)}")
    if out is None:
        out = torch.empty(len(REGRESSION_FIELDS), dtype=torch.float64, device=pred.device)
    elif out.dtype != torch.float64 or out.device != pred.device or \
            out.numel() != len(REGRESSION_FIELDS) or not out.is_contiguous():
        raise RuntimeError(f"hlhgat: regression_summary: out must be contiguous fp64 "
                           f"[{len(REGRESSION_FIELDS)}] on {pred.device}")
    check(LIB.hlhgat_regression_summary(pred.data_ptr(), y.data_ptr(), count.data_ptr(),
                                        pred.numel(), out.data_ptr(), _stream(pred)),
          "regression_summary")
    return out


# ----------------------------------------------------------------------------
# brain input: z-scored series and functional connectivity (csrc/fc.hip)
# ----------------------------------------------------------------------------
FC_TILE = 64  # the correlation kernel's tile edge (csrc/fc.hip)


@dataclass
class FcPrepared:
    """What fc_prepare leaves for fc_dense / fc_edges: the workspace with the
    centred unit-norm rows, the shape it was prepared for and, if wanted, z."""
    workspace: torch.Tensor
    n_graphs: int
    n_nodes: int
    T: int
    z: Optional[torch.Tensor]


def fc_prepare(x: torch.Tensor, n_graphs: int, window=None, want_z: bool = True, *,
               n_nodes: Optional[int] = None, graph_rows: Optional[torch.Tensor] = None,
               workspace: Optional[torch.Tensor] = None,
               z: Optional[torch.Tensor] = None, windows=None,
               t_max: Optional[int] = None) -> FcPrepared:
    """The row pass of Brain_MLGC_ALL.get for n_graphs subjects at once
    (HL-HGAT-DEMO/lib/Hodge_Dataset.py:136): x is [n_graphs * N, T_all] (rows
    may be strided), graph g owning rows [g N, (g + 1) N); window = (t0, T)
    selects columns [t0, t0 + T) (None: all).  Returns an FcPrepared whose z
    ([n_graphs * N, T], want_z) is (x - mean_g) / std_g with the graph's mean
    and unbiased std over its window, and whose workspace feeds fc_dense /
    fc_edges.  graph_rows (int64 [n_graphs], device) with n_nodes = N instead
    picks graph g's rows from row graph_rows[g] of a larger x; its values are
    the caller's to bound.  workspace: a uint8 tensor of at least
    hlhgat_fc_workspace_bytes to reuse; z: a contiguous [n_graphs * N, T]
    tensor to fill (want_z).  windows = (t0, len), two contiguous int32
    [n_graphs] device tensors, with t_max (default: every column of x) gives
    every graph its own window [t0[g], t0[g] + len[g]), 2 <= len[g] <= t_max
    (the per-sample crop of :131-135): statistics over the graph's own window,
    z [n_graphs * N, t_max] with zeros past len[g], and an FcPrepared of
    T = t_max.  Not differentiable: these are inputs."""
    _req_dev(x, "x")
    if x.dim() != 2:
        raise RuntimeError(f"hlhgat: fc_prepare wants x [rows, T], got {tuple(x.shape)}")
    x = _rows2d(x.detach(), "x")
    G = int(n_graphs)
    if graph_rows is None:
        if G < 0 or (G > 0 and x.size(0) % G) or (G == 0 and x.size(0)):
            raise RuntimeError(f"hlhgat: fc_prepare: {x.size(0)} rows do not split into "
                               f"{G} graphs")
        N = x.size(0) // G if G else (int(n_nodes) if n_nodes else 1)
        if n_nodes is not None and G and int(n_nodes) != N:
            raise RuntimeError(f"hlhgat: fc_prepare: n_nodes={n_nodes} but x has {N} rows per graph")
    else:
        if n_nodes is None:
            raise RuntimeError("hlhgat: fc_prepare: graph_rows needs n_nodes")
        _req_dev(graph_rows, "graph_rows", torch.int64)
        N = int(n_nodes)
        if graph_rows.numel() != G or not graph_rows.is_contiguous() or N > x.size(0):
            raise RuntimeError(f"hlhgat: fc_prepare: graph_rows must be contiguous int64 [{G}] and "
                               f"n_nodes <= {x.size(0)} rows")
    if windows is not None:
        if window is not None:
            raise RuntimeError("hlhgat: fc_prepare takes window or windows, not both")
        w0, wl = windows
        for t, name in ((w0, "windows[0]"), (wl, "windows[1]")):
            _req_dev(t, name, torch.int32)
            if t.numel() != G or not t.is_contiguous() or t.device != x.device:
                raise RuntimeError(f"hlhgat: fc_prepare: {name} must be contiguous int32 [{G}] on "
                                   f"{x.device}")
        t0, T = 0, int(x.size(1) if t_max is None else t_max)
    else:
        t0, T = (0, x.size(1)) if window is None else (int(window[0]), int(window[1]))
    if t0 < 0 or t0 + T > x.size(1):
        raise RuntimeError(f"hlhgat: fc_prepare: window [{t0}, {t0 + T}) outside the {x.size(1)} "
                           f"columns of x")
    need = max(int(LIB.hlhgat_fc_workspace_bytes(G, N, T)), 16)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=x.device)
    elif workspace.device != x.device or workspace.dtype != torch.uint8 or \
            not workspace.is_contiguous() or workspace.numel() < need:
        raise RuntimeError(f"hlhgat: fc_prepare: workspace must be contiguous uint8 [>= {need}] on "
                           f"{x.device}")
    if not want_z:
        z = None
    elif z is None:
        z = torch.empty((G * N, T), dtype=torch.float32, device=x.device)
    else:
        _req_dev(z, "z")
        if tuple(z.shape) != (G * N, T) or not z.is_contiguous() or z.device != x.device:
            raise RuntimeError(f"hlhgat: fc_prepare: z must be contiguous [{G * N}, {T}] on "
                               f"{x.device}")
    if windows is not None:
        check(LIB.hlhgat_fc_prepare_windows(x.data_ptr(), _ld(x), _ptr(graph_rows), G, N,
                                            windows[0].data_ptr(), windows[1].data_ptr(), T,
                                            _ptr(z), workspace.data_ptr(), workspace.numel(),
                                            _stream(x)), "fc_prepare_windows")
        return FcPrepared(workspace, G, N, T, z)
    check(LIB.hlhgat_fc_prepare(x.data_ptr(), _ld(x), _ptr(graph_rows), G, N, t0, T, _ptr(z),
                                workspace.data_ptr(), workspace.numel(), _stream(x)),
          "fc_prepare")
    return FcPrepared(workspace, G, N, T, z)


def fc_dense(prep: FcPrepared, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fc [G, N, N]: torch.corrcoef of every prepared graph (the FC stack that
    FC2mask thresholds, lib/Hodge_Dataset.py:148-153): exactly symmetric,
    clamped to [-1, 1], NaN on the row, column and diagonal entry of a region
    whose series is constant over the window."""
    G, N = prep.n_graphs, prep.n_nodes
    ws = prep.workspace
    if out is None:
        out = torch.empty((G, N, N), dtype=torch.float32, device=ws.device)
    else:
        _req_dev(out, "out")
        if tuple(out.shape) != (G, N, N) or not out.is_contiguous() or out.device != ws.device:
            raise RuntimeError(f"hlhgat: fc_dense: out must be contiguous [{G}, {N}, {N}] on "
                               f"{ws.device}")
    check(LIB.hlhgat_fc_dense(ws.data_ptr(), G, N, prep.T, out.data_ptr(), _stream(ws)),
          "fc_dense")
    return out


def fc_pair_table(edge_index, n: int):
    """Host tables of one skeleton for fc_edges: (pair2edge, tiles), CPU
    tensors.  pair2edge is int32 [n * n], -1 or the id of edge (i, j) at
    i * n + j; tiles is int32 [n_tiles, 2], the (row tile, column tile) pairs
    of FC_TILE-sized tiles that hold an edge.  edge_index is [2, E] with
    i < j (the skeleton's triu(1).to_sparse().indices()); i >= j, an index
    outside [0, n) and duplicate pairs raise."""
    import numpy as np
    ei = np.asarray(edge_index.cpu() if torch.is_tensor(edge_index) else edge_index,
                    dtype=np.int64)
    n = int(n)
    if ei.ndim != 2 or ei.shape[0] != 2:
        raise ValueError(f"fc_pair_table: edge_index must be [2, E], got {ei.shape}")
    if n <= 0 or n * n >= 2 ** 31:
        raise ValueError(f"fc_pair_table: n = {n} out of range")
    i, j = ei[0], ei[1]
    if ei.shape[1] and (i.min() < 0 or j.max() >= n):
        raise ValueError(f"fc_pair_table: node index outside [0, {n})")
    if (i >= j).any():
        raise ValueError("fc_pair_table: every edge must have i < j")
    key = i * n + j
    if np.unique(key).size != key.size:
        raise ValueError("fc_pair_table: duplicate pairs")
    table = np.full(n * n, -1, dtype=np.int32)
    table[key] = np.arange(key.size, dtype=np.int32)
    nt = (n + FC_TILE - 1) // FC_TILE
    tk = np.unique((i // FC_TILE) * nt + j // FC_TILE)
    tiles = np.stack([tk // nt, tk % nt], 1).astype(np.int32).reshape(-1, 2)
    return torch.from_numpy(table), torch.from_numpy(np.ascontiguousarray(tiles))


def fc_edges(prep: FcPrepared, pair2edge: torch.Tensor, n_edges: int,
             out: Optional[torch.Tensor] = None, tiles: Optional[torch.Tensor] = None
             ) -> torch.Tensor:
    """x_s of Brain_MLGC_ALL.get (lib/Hodge_Dataset.py:137, :142): the
    correlations at the skeleton's pairs only, [G * n_edges, 1], bit for bit
    the entries of fc_dense; the dense stack is never formed.  pair2edge /
    tiles: fc_pair_table's tables on the device (tiles None: every tile pair
    of the upper triangle).  out: a [G * n_edges, 1] tensor to fill, which may
    be one column of a wider slab (rows strided); rows of no edge keep their
    content."""
    G, N, E = prep.n_graphs, prep.n_nodes, int(n_edges)
    ws = prep.workspace
    _req_dev(pair2edge, "pair2edge", torch.int32)
    if pair2edge.numel() != N * N or not pair2edge.is_contiguous() or pair2edge.device != ws.device:
        raise RuntimeError(f"hlhgat: fc_edges: pair2edge must be contiguous int32 [{N * N}] on "
                           f"{ws.device}")
    if tiles is None:
        nt = (N + FC_TILE - 1) // FC_TILE
        tiles = torch.tensor([[r, c] for r in range(nt) for c in range(r, nt)],
                             dtype=torch.int32).to(ws.device)
    _req_dev(tiles, "tiles", torch.int32)
    if tiles.dim() != 2 or tiles.size(1) != 2 or not tiles.is_contiguous() or \
            tiles.device != ws.device:
        raise RuntimeError("hlhgat: fc_edges: tiles must be contiguous int32 [n_tiles, 2]")
    if out is None:
        out = torch.empty((G * E, 1), dtype=torch.float32, device=ws.device)
    else:
        _req_dev(out, "out")
        if out.dim() != 2 or tuple(out.shape) != (G * E, 1) or out.device != ws.device or \
                (out.size(0) > 1 and out.stride(0) < 1):
            raise RuntimeError(f"hlhgat: fc_edges: out must be [{G * E}, 1] on {ws.device}")
    ld = out.stride(0) if out.size(0) > 1 else 1
    check(LIB.hlhgat_fc_edges(ws.data_ptr(), G, N, prep.T, pair2edge.data_ptr(), E,
                              tiles.data_ptr(), tiles.size(0), out.data_ptr(), ld, _stream(ws)),
          "fc_edges")
    return out


# ----------------------------------------------------------------------------
# device error word (include/hlhgat.h: hlhgat_device_errors)
# ----------------------------------------------------------------------------
_DEVERR_TEXT = {
    _lib.DEVERR_HODGE_SIZE: "hodge_build: a Laplacian row would end past the buffers sized "
                            "from the caller's sizes= (duplicate edges or self-loops?); the "
                            "row was not written",
    _lib.DEVERR_LABEL: "cross_entropy (label bit): a label that is neither ignore_index nor "
                       "a class index in [0, C); its row was left out of the loss and the "
                       "gradient",
    _lib.DEVERR_METRIC_LABEL: "average_precision: a label that is neither NaN, 0 nor 1; it was "
                              "counted as a negative",
    _lib.DEVERR_METER_FULL: "collect_rows: the rows did not fit the collector's buffer "
                            "(capacity too small, or no reset() between epochs); none of them "
                            "was appended",
    _lib.DEVERR_BN_STATE: "BatchNorm: an arrival counter was found beyond its total (the "
                          "workspace was written by something else or shared by concurrent "
                          "launches); that launch's statistics are not trusted",
    _lib.DEVERR_EIGPE_SIZE: "eig_pe: a graph has more nodes than max_nodes (eig_pe_edges: more "
                            "edges than max_edges), which sized its workspace slice; its pe "
                            "rows are zero and its lmax is 0",
    _lib.DEVERR_MLGC_RANGE: "mlgc_device: an edge end outside its graph's node range, a perm "
                            "entry outside [0, n) or graph offsets that leave the arrays; the "
                            "offender was treated as absent",
    _lib.DEVERR_TSERIES_LEN: "time_series_map / fc_prepare(windows=): a series length outside "
                             "[1, t_max] or a window that leaves its row; it was clamped into "
                             "range",
}


def device_errors() -> int:
    """The device error word as kernels that have COMPLETED so far left it
    (no synchronisation)."""
    w = C.c_uint32(0)
    check(LIB.hlhgat_device_errors(C.byref(w)), "device_errors")
    return int(w.value)


def clear_device_errors() -> None:
    check(LIB.hlhgat_clear_device_errors(), "clear_device_errors")


def check_device_errors(sync: bool = True) -> None:
    """Raise RuntimeError if a kernel reported results that must not be used
    (sync=True first waits for all queued work on every stream)."""
    if sync and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
    w = device_errors()
    if w:
        what = _DEVERR_TEXT.get(w, f"device error code {w}")
        raise RuntimeError(f"hlhgat: {what}; results since the last clear_device_errors() are "
                           f"invalid")


def bn_giveups() -> dict:
    """Give-ups of the one-launch BatchNorm barrier since the last
    bn_giveups_reset(): a workgroup whose wait for its tile's statistics ran
    out (hlhgat_set_bn_wait_us) and handed its rows to the finalising
    workgroup.  Correct results either way; this is where the time went.
    Synchronises the device."""
    n = C.c_uint32(0)
    check(LIB.hlhgat_bn_wait_timeouts(C.byref(n)), "bn_wait_timeouts")
    recs = (_lib.BnGiveup * _lib.BN_LOG_MAX)()
    logged = C.c_int32(0)
    check(LIB.hlhgat_bn_giveup_log(recs, _lib.BN_LOG_MAX, C.byref(logged)), "bn_giveup_log")
    k = min(int(logged.value), _lib.BN_LOG_MAX)
    log = [{f: int(getattr(recs[i], f)) for f, _ in _lib.BnGiveup._fields_} for i in range(k)]
    return {"count": int(n.value), "log": log}


def bn_giveups_reset() -> None:
    check(LIB.hlhgat_bn_giveup_reset(), "bn_giveup_reset")


# ----------------------------------------------------------------------------
# captured-graph introspection (include/hlhgat.h: hlhgat_graph_kernel_count)
# ----------------------------------------------------------------------------
def graph_kernel_count(graph_handle: int, name_part: str) -> Tuple[int, int]:
    """(kernel nodes, kernel nodes whose name contains name_part) of a
    captured hipGraph (e.g. torch.cuda.CUDAGraph(keep_graph=True).raw_cuda_graph())."""
    k, m = C.c_int64(), C.c_int64()
    check(LIB.hlhgat_graph_kernel_count(C.c_void_p(int(graph_handle)), name_part.encode(),
                                        C.byref(k), C.byref(m)), "graph_kernel_count")
    return int(k.value), int(m.value)


# ----------------------------------------------------------------------------
# live kernel timing (bench.py)
# ----------------------------------------------------------------------------
def prof_enable(kernel_class: int, enable: bool = True) -> None:
    check(LIB.hlhgat_prof_enable(kernel_class, int(enable)), "prof_enable")


def prof_reset() -> None:
    check(LIB.hlhgat_prof_reset(), "prof_reset")


def prof_read(kernel_class: int):
    n = C.c_int64()
    ms, b, f = C.c_double(), C.c_double(), C.c_double()
    check(LIB.hlhgat_prof_read(kernel_class, C.byref(n), C.byref(ms), C.byref(b), C.byref(f)),
          "prof_read")
    return {"launches": n.value, "ms": ms.value, "bytes": b.value, "flops": f.value}
