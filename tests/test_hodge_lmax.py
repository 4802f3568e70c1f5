"""hlhgat_hodge_lmax (k_lanczos_lmax, csrc/hodge.hip), called the way
ops.hodge_build calls it but keeping the fp64 output, against numpy's
eigvalsh of the dense L0 = B1 B1^T (tests/spectral_ref.py):

* graphs with n <= steps nodes (and well-mixing graphs one node larger):
  1e-12 relative -- empty graphs, one node, one edge, stars and complete
  graphs (the invariant-subspace exit), two components, isolated nodes;
* the LDS and the workspace storage path, sizes on both sides of the limit;
* the workload families at the default 64 steps: 2e-6 relative, the bound
  test_device_hodge_builder_matches_reference holds the builder to;
* slowly mixing graphs (paths, rings, a 30 x 30 grid) with steps = min(n,
  1024): 1e-7 relative, the bound test_lanczos_lmax_matches_fp64_eigh_on_
  superpixel_batch uses.  At 64 steps these are off by up to 1.5e-4 (measured
  on an MI355X: paths 1.0e-4 .. 1.5e-4, rings of 444 and 1000 nodes ~1e-4,
  the grid 1.9e-6; the 100-node ring converges);
* in every case the device's value is a Ritz value, so it does not exceed
  the true lambda_max (by more than 1e-12 relative).
"""
import numpy as np
import pytest
import torch

import spectral_ref as S

EMPTY = S.Graph(np.zeros((2, 0), np.int64), 0)


def _lmax(graphs, steps, dev):
    """fp64 lmax [B] of hlhgat_hodge_lmax on the batch."""
    from hlhgat import ops
    from hlhgat._lib import LIB, check
    ei, ns, offs = S.batch(graphs)
    N, B, E = int(offs[-1]), len(ns), ei.shape[1]
    ei = torch.from_numpy(ei).to(dev)
    node_ptr = torch.from_numpy(offs).to(dev)
    inc = ops.incidence(ei, N)
    wsb = int(LIB.hlhgat_hodge_lmax_workspace_bytes(N, steps))
    ws = torch.empty(max(wsb, 8), dtype=torch.uint8, device=dev)
    lam = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    check(LIB.hlhgat_hodge_lmax(inc.rowptr.data_ptr(), inc.edge_ids.data_ptr() if E else None,
                                ei.data_ptr() if E else None, E, N, node_ptr.data_ptr(), B, steps,
                                lam.data_ptr(), ws.data_ptr(), wsb, ops._stream(ei)), "hodge_lmax")
    torch.cuda.synchronize()
    return lam.cpu().numpy()


def _check(graphs, got, rel, what=""):
    """|got - ref| <= rel * ref and got <= ref (1 + 1e-12) per graph (ref = 0:
    got = 0); prints and returns the worst relative error."""
    worst = 0.0
    for i, g in enumerate(graphs):
        ref = g.lmax
        assert got[i] <= ref * (1.0 + 1e-12), (what, i, g.n, got[i], ref)
        assert abs(got[i] - ref) <= rel * ref, (what, i, g.n, got[i], ref)
        if ref > 0:
            worst = max(worst, abs(got[i] - ref) / ref)
    print(f"hodge_lmax {what}: worst relative error {worst:.2e} (bound {rel:.0e})")
    return worst


def _two_components():
    """A 40-node path (lmax < 4) and K_6 (lmax = 6): the larger lmax in the
    smaller component."""
    p, k6 = S.path(40), S.complete(6)
    return S.Graph(np.concatenate([p.ei, k6.ei + p.n], axis=1), p.n + k6.n)


def _exact_cases():
    """(graphs, steps): every graph has n <= steps, or is a ring with chords
    of steps + 1 nodes (converged long before)."""
    small = [EMPTY, S.path(1), S.path(2), S.star(5), S.complete(4), S.path(7), EMPTY,
             S.copies(S.path(1), 3)]
    return [
        ([S.path(1), EMPTY, S.path(1)], 1),
        (small + [S.ring_chords(8, 8), S.path(8), S.copies(S.path(3), 2, isolated=2)], 8),
        (small + [S.star(33), S.star(64), S.complete(17), S.complete(64), _two_components(),
                  S.copies(S.ring_chords(20, 3), 2, isolated=7), S.knn(60, 8, 2, drop=0.5),
                  S.path(64), S.ring(63), S.grid(8), S.ring_chords(64, 64), S.ring_chords(65, 65)], 64),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(3))
def test_lmax_exact_when_steps_cover_the_graph(cuda, case):
    graphs, steps = _exact_cases()[case]
    assert all(g.n <= steps + 1 for g in graphs)
    got = _lmax(graphs, steps, cuda)
    _check(graphs, got, 1e-12, f"exact, steps {steps}")
    assert S.path(2).lmax == pytest.approx(2.0, abs=1e-14) and S.complete(64).lmax == pytest.approx(64.0)


def _lds_bytes(n, nnz):
    """`need` of k_lanczos_lmax (csrc/hodge.hip): three fp64 vectors and the
    local adjacency; the graph runs from the LDS when it is <= 48 KB."""
    return 24 * n + 4 * (n + 1) + 4 * nnz


def _lds_limit():
    """The largest ring-with-chords size (nnz = 4 n) that runs from the LDS."""
    n = 5
    while _lds_bytes(n + 1, 4 * (n + 1)) <= 48 * 1024:
        n += 1
    return n


def test_lds_limit_restated():
    assert _lds_limit() == 1117  # 44 n + 4 <= 49152
    g = S.ring_chords(50, 50)
    assert g.nnz == 4 * g.n and _lds_bytes(g.n, g.nnz) == 44 * 50 + 4


@pytest.mark.gpu
def test_lmax_both_storage_paths(cuda):
    """Rings with chords (nnz = 4 n) just inside and just outside the 48 KB
    LDS limit, in one batch with small graphs.  A ring with n random chords
    mixes fast: the restated recurrence converges to fp64 rounding (<= 1e-15)
    within 64 steps at every size from 97 to 1119, so the bound is 1e-12."""
    n = _lds_limit()
    graphs = [S.path(9), S.ring_chords(n - 1, n - 1), S.ring_chords(n + 1, n + 1), EMPTY,
              S.ring_chords(n, n), S.ring_chords(n + 2, n + 2), S.star(12)]
    in_lds = [_lds_bytes(g.n, g.nnz) <= 48 * 1024 for g in graphs]
    assert in_lds == [True, True, False, True, True, False, True]
    got = _lmax(graphs, 64, cuda)
    _check(graphs, got, 1e-12, "LDS limit")


def _workload_families():
    fam = {"kNN k=8": [S.knn(n, 8, n, drop) for n in (50, 97, 200, 333, 500) for drop in (0.0, 0.5)],
           "kNN k=25": [S.knn(n, 25, n, drop) for n in (50, 97, 200, 333, 500) for drop in (0.0, 0.5)],
           "chain trees": [S.chain_tree(n, n + s) for n in (65, 120, 200, 300, 450) for s in (0, 1)],
           "grids": [S.grid(10), S.grid(15), S.grid(13, 20), S.grid(20)]}
    return fam


@pytest.mark.gpu
def test_lmax_workload_families_at_64_steps(cuda):
    fam = _workload_families()
    graphs = [g for gs in fam.values() for g in gs]
    got = _lmax(graphs, 64, cuda)
    at = 0
    for name, gs in fam.items():
        _check(gs, got[at:at + len(gs)], 2e-6, name + ", 64 steps")
        at += len(gs)


SLOW = {"path100": lambda: S.path(100), "path444": lambda: S.path(444),
        "path1000": lambda: S.path(1000), "ring100": lambda: S.ring(100),
        "ring444": lambda: S.ring(444), "ring1000": lambda: S.ring(1000),
        "grid30x30": lambda: S.grid(30)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SLOW))
def test_lmax_converged_on_request(cuda, name):
    """Slowly mixing graphs with steps = min(n, 1024).  The default 64 steps
    are measured beside it (printed; from below, like every Ritz value)."""
    g = SLOW[name]()
    got = _lmax([g], min(g.n, 1024), cuda)
    _check([g], got, 1e-7, f"{name}, steps {min(g.n, 1024)}")
    got64 = _lmax([g], 64, cuda)
    _check([g], got64, 1.0, f"{name}, 64 steps (measured, not held to a bound)")


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [0, 1025])
def test_lmax_steps_out_of_range_raises(cuda, steps):
    from hlhgat._lib import LIB
    assert LIB.hlhgat_hodge_lmax_workspace_bytes(10, steps) == 0
    with pytest.raises(RuntimeError, match="hodge_lmax"):
        _lmax([S.path(5)], steps, cuda)
