"""The BatchNorm entry points of the C ABI refuse bad arguments before any HIP
call, with rc HLHGAT_EINVAL and a message that starts with the entry point's
name; hlhgat_bn_workspace_bytes keeps its values (the torch extension caches
workspaces by them).  No device is touched: the dummy pointers are never
dereferenced and every call here is refused."""
import ctypes

import pytest

EINVAL = 1
P = 0x1000  # a 16-byte aligned non-NULL pointer that nothing reads
N, C = 8, 8


def _lib():
    import torch  # noqa: F401  (shares the HIP runtime, as the product does)
    from hlhgat import _lib
    return _lib


def _proj_blocks():
    vp2, i2 = ctypes.c_void_p * 2, ctypes.c_int64 * 2
    return dict(nblocks=2, A=vp2(P, P), lda=i2(32, 32), W=vp2(P, P), ldw=i2(32, 32), kb=i2(32, 32))


# entry point -> its arguments in header order with values a call would accept.
# "WS" / "WSB" stand for the workspace and its size.
FWD_TAIL = dict(momentum=0.1, eps=1e-5)
ENTRIES = {
    "bn_stats_train": dict(x=P, ldx=C, n=N, n_valid=None, C=C, running_mean=P, running_var=P,
                           nbt=None, **FWD_TAIL, save_mean=P, save_invstd=P, WS=P, WSB=0,
                           stream=None),
    "bn_apply": dict(x=P, ldx=C, n=N, n_valid=None, C=C, weight=None, bias=None, save_mean=P,
                     save_invstd=P, relu=1, y=P, ldy=C, stream=None),
    "bn_apply_running": dict(x=P, ldx=C, n=N, C=C, weight=None, bias=None, running_mean=P,
                             running_var=P, eps=1e-5, relu=0, y=P, ldy=C, stream=None),
    "bn_fwd_train": dict(x=P, ldx=C, n=N, n_valid=None, C=C, weight=None, bias=None,
                         running_mean=P, running_var=P, nbt=None, **FWD_TAIL, relu=1, y=P, ldy=C,
                         save_mean=P, save_invstd=P, WS=P, WSB=0, stream=None),
    "proj_bn_fwd": dict(nblocks=0, A=None, lda=None, W=None, ldw=None, kb=None, n=N, C=C,
                        bias=None, x=P, ldx=C, n_valid=None, bn_weight=None, bn_bias=None,
                        running_mean=P, running_var=P, nbt=None, **FWD_TAIL, relu=1, y=P, ldy=C,
                        save_mean=P, save_invstd=P, WS=P, WSB=0, stream=None),
    "bn_bwd_train": dict(x=P, ldx=C, y=P, ldy=C, dy=P, lddy=C, n=N, n_valid=None, C=C,
                         weight=None, save_mean=P, save_invstd=P, dx=P, lddx=C, dweight=None,
                         dbias=None, WS=P, WSB=0, stream=None),
    "bn_bwd_reduce": dict(x=P, ldx=C, y=P, ldy=C, dy=P, lddy=C, n=N, n_valid=None, C=C,
                          weight=None, save_mean=P, save_invstd=P, coef=P, dweight=None,
                          dbias=None, WS=P, WSB=0, stream=None),
    "bn_sums_fwd": dict(x=P, ldx=C, y=P, ldy=C, n=N, n_valid=None, C=C, sums=P, WS=P, WSB=0,
                        stream=None),
    "bn_sync_fwd_apply": dict(x=P, ldx=C, n=N, n_valid=None, C=C, gathered=P, world=1,
                              weight=None, bias=None, running_mean=P, running_var=P, nbt=None,
                              **FWD_TAIL, relu=1, y=P, ldy=C, save_mean=P, save_invstd=P,
                              stream=None),
    "bn_sums_bwd": dict(x=P, ldx=C, y=P, ldy=C, dy=P, lddy=C, dx_layout=P, lddx=C, n=N,
                        n_valid=None, C=C, save_mean=P, save_invstd=P, sums=P, dweight=None,
                        dbias=None, WS=P, WSB=0, stream=None),
    "bn_sync_bwd_apply": dict(x=P, ldx=C, y=P, ldy=C, dy=P, lddy=C, n=N, n_valid=None, C=C,
                              weight=None, save_mean=P, save_invstd=P, gathered=P, world=1, dx=P,
                              lddx=C, stream=None),
}

# pointers an entry point cannot do without (hlhgat_bn_apply_running needs both
# running statistics; everywhere else they come as a pair or not at all)
REQUIRED = {
    "bn_stats_train": ["x", "save_mean", "save_invstd"],
    "bn_apply": ["x", "y", "save_mean", "save_invstd"],
    "bn_apply_running": ["x", "y", "running_mean", "running_var"],
    "bn_fwd_train": ["x", "y", "save_mean", "save_invstd"],
    "proj_bn_fwd": ["x", "y", "save_mean", "save_invstd"],
    "bn_bwd_train": ["x", "dy", "dx", "save_mean", "save_invstd"],
    "bn_bwd_reduce": ["x", "dy", "coef", "save_mean", "save_invstd"],
    "bn_sums_fwd": ["x", "sums"],
    "bn_sync_fwd_apply": ["x", "y", "gathered", "save_mean", "save_invstd"],
    "bn_sums_bwd": ["x", "dy", "sums", "save_mean", "save_invstd"],
    "bn_sync_bwd_apply": ["x", "dy", "dx", "gathered", "save_mean", "save_invstd"],
}
PAIRED = ["bn_stats_train", "bn_fwd_train", "proj_bn_fwd", "bn_sync_fwd_apply"]


def _cases():
    out = []
    for name, args in ENTRIES.items():
        for p in REQUIRED[name]:
            out.append((name, f"NULL {p}", {p: None}))
        for ld in (k for k in args if k.startswith("ld") and k not in ("lda", "ldw")):
            out.append((name, f"{ld} < C", {ld: C - 1}))
        if name in PAIRED:
            out.append((name, "running_mean alone", {"running_var": None}))
            out.append((name, "running_var alone", {"running_mean": None}))
        if "WS" in args:
            out.append((name, "NULL workspace", {"WS": None}))
            out.append((name, "short workspace", {"WSB": -1}))
    return out


def test_the_table_covers_the_eleven_entry_points():
    lib = _lib()
    assert len(ENTRIES) == 11
    for name, args in ENTRIES.items():
        assert len(args) == len(lib.SIGNATURES["hlhgat_" + name][1]), name


@pytest.mark.parametrize("name,what,change", _cases(), ids=lambda v: v if isinstance(v, str) else "")
def test_bad_arguments_are_refused_by_name(name, what, change):
    lib = _lib()
    need = lib.LIB.hlhgat_bn_workspace_bytes(N, C)
    args = dict(ENTRIES[name])
    if name == "proj_bn_fwd":
        args.update(_proj_blocks())
    if "WS" in args:
        args["WSB"] = need
    for k, v in change.items():
        args[k] = need + v if k == "WSB" else v
    rc = getattr(lib.LIB, "hlhgat_" + name)(*args.values())
    msg = lib.LIB.hlhgat_last_error().decode()
    assert rc == EINVAL, (name, what, rc, msg)
    assert msg.startswith(name + ":"), (name, what, msg)


@pytest.mark.parametrize("n,c,nbytes", [(1, 1, 185088), (1000, 64, 733952),
                                        (25000, 128, 1291776), (200000, 300, 2791168),
                                        (-1, 4, 0), (4, 0, 0)])
def test_workspace_bytes_are_pinned(n, c, nbytes):
    assert _lib().LIB.hlhgat_bn_workspace_bytes(n, c) == nbytes
