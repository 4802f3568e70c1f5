"""The brain input pipeline: z-scored series and skeleton FC on the device
(csrc/fc.hip, ops.fc_prepare / fc_dense / fc_edges / fc_pair_table),
hodge_dataset.fc2mask and pipeline.BrainPipeline.

Fixtures: tests/golden/make_golden_brainfc.py ran the REFERENCE's own
Brain_MLGC_ALL.get and FC2mask (HL-HGAT-DEMO/lib/Hodge_Dataset.py:130-178) on
the CPU and stored the same formulas in fp64.

Tolerance of the GPU values: max|ours - fp64| <= 4 e_ref + 2^-22 max|fp64|,
e_ref = max|reference fp32 - fp64| of the same case as the fixture records it
(2-5e-7 for x_s, 3e-7-1.3e-6 for x_t): the factor 4 covers a different but
equally valid fp32 summation order, the floor one rounding of the result.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_golden

T_ = torch.from_numpy
CASES = ["brainfc_G3N37T70", "brainfc_G2N21T3", "brainfc_G1N16T64", "brainfc_G2N130T129"]
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _case(name):
    g = load_golden(name)
    G, N, _ = g["x"].shape
    g["G"], g["N"], g["E"] = G, N, g["edge_index"].shape[1]
    g["t0"], g["T"] = int(g["t0"]), int(g["T"])
    return g


def _tol(g, what):
    ref = g["xs64"] if what == "xs" else g["xt64"]
    return 4.0 * float(g["e_ref_" + what]) + 2.0 ** -22 * float(np.abs(ref).max())


def _err(got, ref64):
    return float((got.detach().cpu().double() - T_(np.asarray(ref64))).abs().max())


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_capi_rejects_bad_arguments():
    """HLHGAT_EINVAL and a message before any HIP call (runs without a GPU)."""
    from hlhgat import _lib
    L = _lib.LIB
    buf = (C.c_float * 4096)()
    p = (C.cast(buf, C.c_void_p).value + 15) // 16 * 16  # 16-byte aligned host memory

    def prep(x=p, ldx=8, G=1, N=4, t0=0, T=8, ws=p, nbytes=4096):
        return L.hlhgat_fc_prepare(x, ldx, None, G, N, t0, T, None, ws, nbytes, None)

    def dense(ws=p, G=1, N=4, T=8, fc=p):
        return L.hlhgat_fc_dense(ws, G, N, T, fc, None)

    def edges(ws=p, G=1, N=4, T=8, tab=p, E=3, tiles=p, nt=1, out=p, ld=1):
        return L.hlhgat_fc_edges(ws, G, N, T, tab, E, tiles, nt, out, ld, None)

    def bad(rc, word):
        assert rc == 1, (rc, word)
        msg = L.hlhgat_last_error()
        assert msg and word.encode() in msg, (msg, word)

    for fn in (prep, dense, edges):
        bad(fn(T=1), "T")
        bad(fn(N=0), "N")
        bad(fn(G=-1), "G")
        bad(fn(ws=None), "NULL")
        assert fn(G=0) == 0  # a no-op, whatever the pointers
    assert prep(G=0, x=None, ws=None) == 0
    bad(prep(t0=1), "ldx")          # t0 + T > ldx
    bad(prep(ldx=7), "ldx")
    bad(prep(t0=-1), "t0")
    bad(prep(x=None), "NULL")
    bad(prep(nbytes=64), "workspace")
    bad(prep(ws=p + 4), "aligned")
    bad(dense(fc=None), "NULL")
    bad(edges(E=0), "E")
    bad(edges(E=-3), "E")
    bad(edges(tab=None), "NULL")
    bad(edges(tiles=None), "NULL")
    bad(edges(out=None), "NULL")
    bad(edges(ld=0), "ld")
    assert L.hlhgat_fc_workspace_bytes(3, 37, 70) == 3 * 37 * 72 * 4 + 3 * 37 * 16
    assert L.hlhgat_fc_workspace_bytes(0, 37, 70) == 0
    assert L.hlhgat_fc_workspace_bytes(1, 4, 1) == 0
    assert L.hlhgat_version() >= 105


def test_ops_have_no_cpu_fallback():
    from hlhgat import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fc_prepare(torch.randn(8, 5), 2)
    prep = ops.FcPrepared(torch.zeros(64, dtype=torch.uint8), 1, 4, 5, None)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fc_edges(prep, torch.zeros(16, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fc_dense(prep, out=torch.zeros(1, 4, 4))


@pytest.mark.parametrize("name", CASES)
def test_pair_table(name):
    from hlhgat import ops
    g = _case(name)
    ei, N, E = g["edge_index"], g["N"], g["E"]
    table, tiles = ops.fc_pair_table(ei, N)
    table, tiles = table.numpy(), tiles.numpy()
    assert table.dtype == np.int32 and table.shape == (N * N,) and tiles.dtype == np.int32
    hit = np.flatnonzero(table >= 0)
    # every edge exactly once, at its own pair
    assert np.array_equal(np.sort(table[hit]), np.arange(E))
    assert np.array_equal(hit[np.argsort(table[hit])], ei[0] * N + ei[1])
    want = sorted(set(zip((ei[0] // 64).tolist(), (ei[1] // 64).tolist())))
    assert [tuple(t) for t in tiles.tolist()] == want
    assert all(r <= c for r, c in want)
    if N > 128:  # three 64-row blocks: the skeleton's tile pairs, no more
        assert len(want) <= 6


def test_pair_table_rejects_bad_edges():
    from hlhgat import ops
    ok = np.array([[0, 0, 1], [1, 2, 2]])
    ops.fc_pair_table(ok, 3)
    ops.fc_pair_table(T_(ok), 3)
    for ei, word in ((np.array([[0, 2], [1, 1]]), "i < j"),       # i > j
                     (np.array([[0, 1], [1, 1]]), "i < j"),       # i == j
                     (np.array([[0, 0, 0], [1, 2, 1]]), "duplicate"),
                     (np.array([[0, 0], [1, 3]]), "outside"),
                     (np.array([[-1, 0], [1, 2]]), "outside")):
        with pytest.raises(ValueError, match=word):
            ops.fc_pair_table(ei, 3)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_fc2mask_equals_reference(mode):
    import hlhgat
    g = load_golden("brainfc_mask")
    mask = hlhgat.fc2mask(T_(g["FC"]), threshmode=mode, k_ratio=float(g["k_ratio"]))
    ref = T_(g[f"mask{mode}"])
    assert mask.dtype == ref.dtype and torch.equal(mask, ref)
    assert int(mask.sum()) > 0 and torch.equal(mask, mask.triu(1))


def _pipe_levels(ei, n):
    """A one-level list on the skeleton ei (Laplacians as the notebook's)."""
    from hlhgat.hodge_dataset import PairData, hodge_coo_from_boundary
    deg = np.bincount(ei.reshape(-1), minlength=n)
    ei_t, w_t, ei_s, w_s = hodge_coo_from_boundary(ei, n, float(2 * deg.max()))
    E = ei.shape[1]
    d = PairData(x_s=torch.ones(E, 1), edge_index_s=ei_s, edge_weight_s=w_s,
                 x_t=torch.ones(n, 1), edge_index_t=ei_t, edge_weight_t=w_t,
                 edge_index=T_(ei))
    d.num_node1, d.num_edge1 = n, E
    d.pos_t, d.pos_s = torch.zeros(n), torch.zeros(E)
    return [d]


@pytest.fixture
def one_thread():
    nt = torch.get_num_threads()
    torch.set_num_threads(1)  # the generator's CPU reduction order
    yield
    torch.set_num_threads(nt)


def _get_line_137(x_t, ei):
    """get()'s x_s from its own x_t (lib/Hodge_Dataset.py:137, :142) on the
    machine the test runs on; x_t in torch's own allocation, as get() has it."""
    f = T_(np.ascontiguousarray(x_t)).clone()
    return torch.corrcoef(f)[ei[0], ei[1]].view(-1, 1)


def _xs_bound(stored_xs, x_t64, ei):
    """How far two fp32 evaluations of corrcoef may lie apart: the stored
    reference's own error against fp64 (e_ref, measured here) plus the 4 e_ref
    + 2^-22 granted to any other valid fp32 summation order (module docstring)."""
    ref64 = torch.corrcoef(x_t64)[ei[0], ei[1]]
    e_ref = float((T_(np.asarray(stored_xs)).double().view(-1) - ref64).abs().max())
    return 5.0 * e_ref + 2.0 ** -22


def test_brain_pipeline_cpu_equals_reference_get(one_thread):
    """device="cpu" restates get(): bitwise for ifaug = 0 and, window by
    window, for the draws of ifaug = 1.

    x_t and y are compared bit for bit with the stored outputs of get().  x_s
    is torch.corrcoef of that x_t, a BLAS product whose last bits depend on the
    CPU the library dispatches for, so a stored x_s is bitwise only on the
    machine that generated it (an earlier version of this test compared
    against it and failed on another CPU with x_t equal).  get() computes x_s
    from its x_t by one line (:137), so its x_s on THIS machine is that line
    applied to the stored x_t: the pipeline must equal it bit for bit, and the
    stored x_s must agree within the rounding of two fp32 evaluations."""
    import hlhgat
    g = load_golden("brainfc_pipe")
    S, N, T = g["x"].shape
    ei = T_(g["edge_index"])
    y = torch.stack([hlhgat.brain_target(s) for s in g["scores"]])
    assert y.dtype == torch.float32 and torch.equal(y, T_(g["y"]))
    pipe = hlhgat.BrainPipeline(list(g["x"]), y, _pipe_levels(g["edge_index"], N))
    E = g["edge_index"].shape[1]
    b = pipe.batch([2, 0], device="cpu")
    assert len(b) == 1 and b[0].num_graphs == 2
    assert torch.equal(b[0].x_t, T_(g["xt_full"][[2, 0]]).reshape(2 * N, T))
    assert b[0].x_s.shape == (2 * E, 1) and b[0].x_s.dtype == torch.float32
    for k, i in enumerate((2, 0)):
        got = b[0].x_s[k * E:(k + 1) * E]
        assert torch.equal(got, _get_line_137(g["xt_full"][i], ei))
        err = float((got.view(-1) - T_(g["xs_full"][i])).abs().max())
        bound = _xs_bound(g["xs_full"][i], T_(g["xt_full"][i]).double(), ei)
        print(f"[pipe cpu, subject {i}] |x_s - stored| {err:.2e} (bound {bound:.2e})")
        assert err <= bound
    assert torch.equal(b[0].y, T_(g["y"][[2, 0]]))
    assert torch.equal(b[0].edge_index[:, E:], T_(g["edge_index"]) + N)
    for i, (tb, ln) in enumerate(g["windows"].tolist()):
        b = pipe.batch([i], window=(tb, ln), device="cpu")
        assert torch.equal(b[0].x_t, T_(g[f"xt_aug{i}"]))
        assert torch.equal(b[0].x_s, _get_line_137(g[f"xt_aug{i}"], ei))
        err = float((b[0].x_s.view(-1) - T_(g[f"xs_aug{i}"])).abs().max())
        assert err <= _xs_bound(g[f"xs_aug{i}"], T_(g[f"xt_aug{i}"]).double(), ei)
    # one window per batch, drawn from the seed, inside the reference's ranges
    a = pipe.batch([0, 1], window="random", seed=3, device="cpu")
    b = pipe.batch([0, 1], window="random", seed=3, device="cpu")
    assert torch.equal(a[0].x_t, b[0].x_t) and 250 <= a[0].x_t.shape[1] < 300
    assert a[0].x_t.shape[0] == 2 * N
    with pytest.raises(ValueError, match="window"):
        pipe.batch([0], window=(370, 10), device="cpu")
    with pytest.raises(ValueError, match="outside"):
        pipe.batch([3], device="cpu")


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
_RUNS = {}


def _run(name, cuda, windowed, x=None):
    """prepare + edges + dense of one case into NaN-filled buffers, once per
    (case, layout); x overrides the fixture's series (same shape)."""
    from hlhgat import ops
    key = (name, windowed)
    if x is None and key in _RUNS:
        return _RUNS[key]
    g = _case(name)
    G, N, E, t0, T = g["G"], g["N"], g["E"], g["t0"], g["T"]
    xs = T_(g["x"]) if x is None else x
    if windowed:   # ldx = T + 9, unaligned window
        xd, win = xs.reshape(G * N, -1).to(cuda), (t0, T)
    else:          # the contiguous copy of the window
        xd, win = xs[:, :, t0:t0 + T].reshape(G * N, T).contiguous().to(cuda), None
    table, tiles = (t.to(cuda) for t in ops.fc_pair_table(g["edge_index"], N))
    z = torch.full((G * N, T), NAN, device=cuda)
    out = torch.full((G * E, 1), NAN, device=cuda)
    fc = torch.full((G, N, N), NAN, device=cuda)
    prep = ops.fc_prepare(xd, G, window=win, z=z)
    assert prep.z is z
    assert ops.fc_edges(prep, table, E, out=out, tiles=tiles) is out
    assert ops.fc_dense(prep, out=fc) is fc
    res = dict(z=z, xs=out, fc=fc, xd=xd, win=win, table=table, tiles=tiles)
    if x is None:
        _RUNS[key] = res
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("name", CASES)
def test_values_vs_fp64(cuda, name, windowed):
    g = _case(name)
    r = _run(name, cuda, windowed)
    # every element written (the buffers started as NaN), each edge once
    assert torch.isfinite(r["z"]).all() and torch.isfinite(r["xs"]).all()
    e_xt, e_xs = _err(r["z"], g["xt64"]), _err(r["xs"].view(-1), g["xs64"])
    print(f"[{name} windowed={windowed}] x_t err {e_xt:.2e} (tol {_tol(g, 'xt'):.2e}, reference "
          f"{float(g['e_ref_xt']):.2e})  x_s err {e_xs:.2e} (tol {_tol(g, 'xs'):.2e}, reference "
          f"{float(g['e_ref_xs']):.2e})")
    assert e_xt <= _tol(g, "xt")
    assert e_xs <= _tol(g, "xs")
    # the layout of the input changes no bit
    other = _run(name, cuda, not windowed)
    assert torch.equal(r["z"], other["z"]) and torch.equal(r["xs"], other["xs"])
    assert torch.equal(r["fc"], other["fc"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_bitwise_properties(cuda, name):
    from hlhgat import ops
    g = _case(name)
    G, N, E, T = g["G"], g["N"], g["E"], g["T"]
    r = _run(name, cuda, True)
    fc = r["fc"]
    # the same call twice
    prep = ops.fc_prepare(r["xd"], G, window=r["win"])
    assert torch.equal(prep.z, r["z"])
    assert torch.equal(ops.fc_edges(prep, r["table"], E, tiles=r["tiles"]), r["xs"])
    assert torch.equal(ops.fc_dense(prep), fc)
    # without a tile list (every upper tile pair) the edges are the same bits
    assert torch.equal(ops.fc_edges(prep, r["table"], E), r["xs"])
    # a subject alone equals the subject in the batch
    for s in range(G):
        one = ops.fc_prepare(r["xd"][s * N:(s + 1) * N], 1, window=r["win"])
        assert torch.equal(one.z, r["z"][s * N:(s + 1) * N])
        assert torch.equal(ops.fc_edges(one, r["table"], E, tiles=r["tiles"]),
                           r["xs"][s * E:(s + 1) * E])
    # ... and through graph_rows, picked out of the block in another order
    order = list(range(G))[::-1]
    rows = torch.tensor([s * N for s in order], dtype=torch.int64, device=cuda)
    pick = ops.fc_prepare(r["xd"], G, window=r["win"], n_nodes=N, graph_rows=rows)
    assert torch.equal(pick.z.view(G, N, T), r["z"].view(G, N, T)[order])
    assert torch.equal(ops.fc_edges(pick, r["table"], E, tiles=r["tiles"]).view(G, E),
                       r["xs"].view(G, E)[order])
    # dense: finite, exactly symmetric, equal to the edges at the skeleton's pairs
    assert torch.isfinite(fc).all()
    assert torch.equal(fc, fc.transpose(1, 2))
    ei = T_(g["edge_index"]).to(cuda)
    assert torch.equal(fc[:, ei[0], ei[1]].reshape(-1), r["xs"].view(-1))
    diag = fc.diagonal(dim1=1, dim2=2)
    assert float(diag.max()) <= 1.0 and float(fc.abs().max()) <= 1.0
    assert float((1.0 - diag).max()) <= 4.0 * float(g["e_ref_xs"]) + 2.0 ** -22
    # a column of a wider slab
    slab = torch.full((G * E, 3), NAN, device=cuda)
    ops.fc_edges(prep, r["table"], E, out=slab[:, 1:2], tiles=r["tiles"])
    assert torch.equal(slab[:, 1:2], r["xs"]) and torch.isnan(slab[:, [0, 2]]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["brainfc_G3N37T70", "brainfc_G2N130T129"])
def test_constant_rows_give_nan(cuda, name):
    """An all-zero row and a constant-7 row: NaN on all their edges and on
    their diagonal, every other value within tolerance."""
    g = _case(name)
    G, N, E = g["G"], g["N"], g["E"]
    zero_row, seven_row = 1, N - 2  # the hub row and a row of the last partial tile
    x = T_(g["x"]).clone()
    x[0, zero_row] = 0.0
    x[G - 1, seven_row] = 7.0
    r = _run(name, cuda, True, x=x)
    ei = g["edge_index"]
    dead = np.zeros((G, E), dtype=bool)
    dead[0] = (ei[0] == zero_row) | (ei[1] == zero_row)
    dead[G - 1] |= (ei[0] == seven_row) | (ei[1] == seven_row)
    assert dead.sum() >= N - 2
    xs = r["xs"].view(G, E).cpu()
    assert torch.isnan(xs[T_(dead)]).all()
    live = T_(~dead)
    assert torch.isfinite(xs[live]).all()
    ref = T_(g["xs64"]).view(G, E)
    assert float((xs[live].double() - ref[live]).abs().max()) <= _tol(g, "xs")
    fc = r["fc"].cpu()
    assert torch.equal(torch.isnan(fc), torch.isnan(fc.transpose(1, 2)))
    nan_rows = torch.isnan(fc).all(dim=2)
    want = torch.zeros(G, N, dtype=torch.bool)
    want[0, zero_row] = want[G - 1, seven_row] = True
    assert torch.equal(nan_rows, want)                     # row, column and diagonal
    assert int(torch.isnan(fc).sum()) == 2 * (2 * N - 1)   # and nothing else
    # x_t: the same formula in fp64 on the changed input
    w = x[:, :, g["t0"]:g["t0"] + g["T"]].double()
    z64 = (w - w.mean(dim=(1, 2), keepdim=True)) / w.std(dim=(1, 2), keepdim=True)
    tol = 4.0 * float(g["e_ref_xt"]) + 2.0 ** -22 * float(z64.abs().max())
    assert _err(r["z"], z64.reshape(G * N, -1).numpy()) <= tol


@pytest.mark.gpu
def test_fc2mask_on_the_device_stack(cuda):
    import hlhgat
    from hlhgat import ops
    g = load_golden("brainfc_mask")
    S, N, T = g["x"].shape
    prep = ops.fc_prepare(T_(g["x"]).reshape(S * N, T).to(cuda), S, want_z=False)
    assert prep.z is None
    FC = ops.fc_dense(prep)
    assert float((FC.cpu().double() - T_(g["FC"]).double()).abs().max()) <= 4e-6
    mask = hlhgat.fc2mask(FC, threshmode=1, k_ratio=float(g["k_ratio"]))
    assert mask.device.type == "cuda" and mask.dtype == torch.long
    # the pair at the k-th position is decided by rounding (see the generator)
    m_ref = T_(g["FC"]).mean(dim=0).abs()
    free = (m_ref - float(g["kth"])).abs() <= 1e-6
    assert int(free.sum()) <= 2
    assert torch.equal(mask.cpu()[~free], T_(g["mask1"])[~free])


def _head_levels(g):
    """The per-subject level list behind the brain_head_small fixture (three
    copies of one 24-node skeleton): graph 0 of each collated level."""
    from hlhgat.hodge_dataset import PairData
    out = []
    for lv in (0, 1):
        n, e = int(g[f"l{lv}/num_node1"][0]), int(g[f"l{lv}/num_edge1"][0])
        d = PairData(x_t=T_(g[f"l{lv}/x_t"][:n]), x_s=T_(g[f"l{lv}/x_s"][:e]),
                     edge_index=T_(g[f"l{lv}/edge_index"][:, :e]))
        for side, cnt in (("t", n), ("s", e)):
            ei, w = g[f"l{lv}/edge_index_{side}"], g[f"l{lv}/edge_weight_{side}"]
            keep = ei[0] < cnt
            assert (ei[1][keep] < cnt).all()
            setattr(d, "edge_index_" + side, T_(ei[:, keep]))
            setattr(d, "edge_weight_" + side, T_(w[keep]))
        d.num_node1, d.num_edge1 = n, e
        out.append(d)
    n, e = out[0].x_t.shape[0], out[0].x_s.shape[0]
    out[0].pos_t, out[0].pos_s = T_(g["pos_t"][:n]), T_(g["pos_s"][:e])
    return out


@pytest.mark.gpu
def test_pipeline_batch_vs_hand_built_list(cuda):
    import copy
    import hlhgat
    from hlhgat import ops
    from hlhgat.hodge_dataset import collate
    from hlhgat.train import InferStep
    from test_brain_head import HEAD, KEYS, _head_kw, _sd
    g = load_golden(HEAD)
    levels = _head_levels(g)
    N, E, T = levels[0].x_t.shape[0], levels[0].x_s.shape[0], 23
    rng = np.random.default_rng(5)
    series = [((rng.standard_normal((N, 3)) @ rng.standard_normal((3, T + 4))
                + rng.standard_normal((N, T + 4))) * 50 + 1000).astype(np.float32)
              for _ in range(4)]
    y = torch.arange(4, dtype=torch.float32)
    pipe = hlhgat.BrainPipeline(series, y, levels)
    got = pipe.batch([0, 1, 2], window=(2, T), device=cuda)
    # the device values against the CPU restatement of the reference
    cpu = pipe.batch([0, 1, 2], window=(2, T), device="cpu")
    assert got[0].x_t.shape == (3 * N, T) and got[0].x_s.shape == (3 * E, 1)
    assert float((got[0].x_t.cpu() - cpu[0].x_t).abs().max()) <= 1e-5
    assert float((got[0].x_s.cpu() - cpu[0].x_s).abs().max()) <= 4e-6
    assert torch.equal(got[0].y.cpu(), y[:3])
    # the hand-built list: collate of three copies with the same x_t / x_s
    fine = copy.copy(levels[0])
    fine.x_t, fine.x_s = torch.zeros(N, 1), torch.zeros(E, 1)
    hand = [collate([fine] * 3).to(cuda), collate([levels[1]] * 3).to(cuda)]
    hand[0].x_t, hand[0].x_s = got[0].x_t, got[0].x_s
    for lv in (0, 1):
        for k in KEYS + (("pos_t", "pos_s") if lv == 0 else ()):
            a, b = getattr(got[lv], k), getattr(hand[lv], k)
            assert torch.equal(torch.as_tensor(a).to(cuda), torch.as_tensor(b).to(cuda)), (lv, k)
    # the fixture's own collation is the same structure
    for lv in (0, 1):
        for k in KEYS[2:]:
            assert torch.equal(torch.as_tensor(getattr(got[lv], k)).cpu(),
                               T_(g[f"l{lv}/{k}"])), (lv, k)
    m = hlhgat.HL_HGAT_attpool(**_head_kw(g))
    m.load_state_dict(_sd(g), strict=True)
    m = m.to(cuda).eval()
    step = InferStep(m, graphs=False)
    ops.clear_caches()
    a = [t.clone() for t in step(got)]
    ops.clear_caches()
    b = step(hand)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)
    ops.check_device_errors()
    # a second batch rebuilds nothing: the same structure tensors
    again = pipe.batch([3, 1, 0], window=(2, T), device=cuda)
    for lv in (0, 1):
        for k in KEYS[2:] + (("pos_t", "pos_s") if lv == 0 else ()):
            assert getattr(again[lv], k).data_ptr() == getattr(got[lv], k).data_ptr(), (lv, k)
    assert again[1] is got[1]
    assert torch.equal(again[0].x_t[N:2 * N], got[0].x_t[N:2 * N])      # subject 1 again
    assert torch.equal(again[0].x_s[2 * E:], got[0].x_s[:E])            # subject 0 again
    assert torch.equal(again[0].y.cpu(), y[[3, 1, 0]])
    # series kept on the host, a batch's rows uploaded: the same bits
    host = hlhgat.BrainPipeline(series, y, levels, resident=False)
    h = host.batch([3, 1, 0], window=(2, T), device=cuda)
    assert torch.equal(h[0].x_t, again[0].x_t) and torch.equal(h[0].x_s, again[0].x_s)
    assert torch.equal(h[0].y, again[0].y)
