"""Matmul precision of the dense projections (include/hlhgat.h:
hlhgat_set_gemm_precision), in the style of torch.set_float32_matmul_precision.

"fp32" (the default) runs the fp32 MFMA kernels, bit for bit as without this
switch.  "bf16" rounds the two operands of every eligible projection GEMM to
bf16 (round to nearest even) on load and accumulates the exact products in
fp32; activations, weights, gradients and optimiser state stay fp32.  The
setting is process-wide host state read when a GEMM is launched, forward and
backward alike, so it needs no device and a captured graph keeps the mode it
was captured in.  The brain front end's temporal convolution is fp32 in
either mode.
"""
from __future__ import annotations

import contextlib
from typing import Iterator, Tuple

from ._lib import LIB, check

_MODES = {"fp32": 0, "bf16": 1}  # HLHGAT_GEMM_FP32, HLHGAT_GEMM_BF16
_NAMES = {v: k for k, v in _MODES.items()}


def _mode(name) -> int:
    if name not in _MODES:
        raise ValueError(f"matmul precision must be one of {sorted(_MODES)}, got {name!r}")
    return _MODES[name]


def set_matmul_precision(name: str) -> None:
    check(LIB.hlhgat_set_gemm_precision(_mode(name)), "set_gemm_precision")


def get_matmul_precision() -> str:
    return _NAMES[int(LIB.hlhgat_get_gemm_precision())]


@contextlib.contextmanager
def matmul_precision(name: str) -> Iterator[None]:
    """Run the body at the given precision; the previous one is restored on
    exit, also when the body raises."""
    mode = _mode(name)
    prev = int(LIB.hlhgat_get_gemm_precision())
    check(LIB.hlhgat_set_gemm_precision(mode), "set_gemm_precision")
    try:
        yield
    finally:
        check(LIB.hlhgat_set_gemm_precision(prev), "set_gemm_precision")


def resolve(name) -> str:
    """A step object's fixed precision: `name`, or the global value now."""
    if name is None:
        return get_matmul_precision()
    _mode(name)
    return name


def gemm_bf16_eligible(kb, ld=None, N: int = 4, aligned16: bool = True) -> bool:
    """hlhgat_gemm_bf16_eligible: whether a GEMM call with reduction widths kb
    (and row strides ld) takes the bf16 kernels in bf16 mode."""
    import ctypes as C
    n = len(kb)
    kba = (C.c_int64 * n)(*[int(k) for k in kb])
    lda = (C.c_int64 * n)(*[int(v) for v in ld]) if ld is not None else None
    return bool(LIB.hlhgat_gemm_bf16_eligible(n, kba, lda, int(N), int(bool(aligned16))))


def gemm_precision_stats(reset: bool = False) -> Tuple[int, int]:
    """(GEMM calls sent to the bf16 kernels, calls that fell back to fp32
    while in bf16 mode) since the last reset."""
    import ctypes as C
    out = (C.c_int64 * 2)()
    check(LIB.hlhgat_gemm_precision_stats(out, int(bool(reset))), "gemm_precision_stats")
    return int(out[0]), int(out[1])
