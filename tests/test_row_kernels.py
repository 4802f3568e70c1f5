"""Every vector-width / lane-group instantiation of the row-wise kernels.

k_att_fwd, k_att_bwd, k_row_scale_fwd, k_row_scale_bwd (csrc/attention.hip)
and k_edge_gather2, k_edge_absdiff_fwd/_bwd, k_segment_mean_fwd/_bwd
(csrc/poly.hip) each exist as 21 code objects <V, L>, V in {1, 2, 4} floats
per lane and L in {1, .., 64} lanes per row, picked on the host from the
feature width, the row strides and the pointer alignments.  The placement
table of tests/rowkernel_ref.py reaches all 21 through the C ABI (which
exposes every stride and pointer), with idle lanes, partial last passes,
partial last blocks, one row, and single misaligned operands.

Every buffer carries guard columns left and right of its window and a guard
row above and below it, filled with a NaN of a fixed payload: outputs must
be written inside the window everywhere and nowhere else (bit for bit), and a
load outside an input window would poison the result.

Bounds (u = 2^-24, the unit roundoff of fp32):
  * row_scale y / dx, edge_gather2, edge_absdiff fwd / bwd, segment_mean
    bwd: BITWISE against CPU fp32 torch, one op per rounding (derived: the
    library is built with -ffp-contract=off and divides correctly rounded).
  * segment_mean fwd: BITWISE against the fp32 sum in member order / max(cnt,
    1) (derived: the kernel's own order), and close(1e-6) against fp64
    scatter_mean (the project's tolerance for this op).
  * att_score fwd, ReLU: |out - ref| <= (dk + 4) u S per row, S = (|c1|
    sum|Qc K| + |c2| sum|Qs K|) / sqrt_dk (derived: rowkernel_ref.att_ref).
    Sigmoid: close(1e-5) (project, SURVEY.md 8c: the device expf), finite,
    in [0, 1]; z = 0 gives exactly 0 / 0.5.
  * att_score bwd, ReLU: |g - ref| <= 4 u |ref| elementwise on the rows whose
    fp64 |z| exceeds the forward bound (derived: three roundings for dQc and
    dQs; dK has a fourth, (1 + u)^4 - 1 = 4u + 6u^2, relative to |d1 Qc| +
    |d2 Qs| = |dK| for the sign-matched inputs, the excess 6u^2 needs all
    four roundings at their extreme); z = 0 rows: exactly 0.  Sigmoid:
    close(1e-5) (project).
  * row_scale da: |da - ref| <= (d + 2) u sum|dy x| (derived).
  * B1 products behind the wrappers (the CSR SpMM, not under test here):
    (deg + 2) u sum|terms| (derived).

Largest error seen on an MI355X (gfx950) over the whole file (557 tests,
under 4 s), as a share of the bound where one applies (printed again by
every run with -s):
  * row_scale y / dx, edge_gather2, edge_absdiff fwd / bwd, segment_mean fwd
    / bwd: 0 (bitwise), no guard element disturbed, no window element
    unwritten;
  * segment_mean fwd against fp64: 2.1e-7 of the 1e-6 allowed;
  * att_score fwd: ReLU 0.38 of the bound, sigmoid 8.2e-8 (close form);
  * att_score bwd: ReLU dQc 0.61, dQs 0.60, dK 0.75 of the bound, sigmoid
    1.5e-7 (close form);
  * row_scale da: 0.45 of the bound;  B1 products: 0.37 of the bound;
  * every one of the 9 templates launched all 21 <V, L> (graph node counts
    equal to the table's prediction, none dropped).
"""
import collections

import numpy as np
import pytest
import torch

import rowkernel_ref as R
from conftest import close

gpu = pytest.mark.gpu
CASE_IDS = [c.label() for c in R.CASES]
OPS = tuple(R.OPERANDS)
U = R.U

# largest error per check on this run (printed with -s when the module ends)
OBSERVED = collections.defaultdict(float)


def _seen(what, value):
    OBSERVED[what] = max(OBSERVED[what], float(value))


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(OBSERVED):
        print(f"\nobserved {k}: {OBSERVED[k]:.3e}", end="")
    print()


def _within(actual, ref, bound, what):
    """|actual - ref| <= bound elementwise (fp64); records max err / bound."""
    err = (actual.double() - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements over the bound, worst "
                           f"err {float(err[bad].max()):.3e} vs bound {float(bound[bad].min()):.3e}")
    live = bound > 0
    if live.any():
        _seen(what + " err/bound", (err[live] / bound[live]).max())


# ----------------------------------------------------------------------------
# 1. the placement table (CPU)
# ----------------------------------------------------------------------------
def test_table_spans_the_lattice():
    assert len(set(R.CASES)) == len(R.CASES)
    for op in OPS:
        hit = {R.predict(c, op) for c in R.CASES}
        assert hit == R.LATTICE, (op, sorted(R.LATTICE - hit))
    # without the optional z of edge_gather2 as well
    assert {R.predict(c, "edge_gather2", absent=("z",)) for c in R.CASES} == R.LATTICE


def test_table_has_the_named_cases():
    plain = {(c.d, R.predict(c, "row_scale_fwd")[0]) for c in R.CASES if not c.over}
    for d, v in ((12, 4), (20, 4), (6, 2), (3, 1), (5, 1), (7, 1),       # idle lanes
                 (260, 4), (300, 4), (130, 2), (65, 1), (129, 1), (200, 1),  # partial last pass
                 (1, 1), (36, 4), (36, 2), (36, 1)):
        assert (d, v) in plain, (d, v)
    for d, v in ((12, 4), (20, 4), (6, 2), (3, 1), (5, 1), (7, 1)):
        lanes = -(-d // v)
        assert lanes < R.pick_l(d, v) <= 64
    for d, v in ((260, 4), (300, 4), (130, 2), (65, 1), (129, 1), (200, 1)):
        assert d > 64 * v and d % (64 * v) != 0
    for rows in ("one", "exact"):
        assert sum(c.rows == rows for c in R.CASES) >= 3
    # the att_score_kq gradient block: pointers 0, dk, 2dk floats into [n, 3dk]
    assert any(c.g_block() == (3 * c.d, {"dK": 0, "dQs": c.d, "dQc": 2 * c.d}) for c in R.CASES)
    assert any(c.g_block()[0] != c.d for c in R.CASES)


def test_table_breaks_each_operand_alone():
    """For every operand the dispatch inspects there is a call in which that
    operand alone (its pointer or only its stride) lowers V."""
    for op, names in R.OPERANDS.items():
        for name in names:
            found = False
            for c in R.CASES:
                if {k for k, _ in c.over} & set(names) != {name}:
                    continue
                without = _without(c, name)
                found |= R.predict(c, op)[0] < R.predict(without, op)[0] == 4
            assert found, (op, name)
    # a stride alone (pointer still aligned) for ldg and for z
    assert any(dict(c.over).get("dQc") == (0, 2) for c in R.CASES)
    assert any(dict(c.over).get("z") == (0, 2) for c in R.CASES)


def _without(c, name):
    return c._replace(over=tuple((k, v) for k, v in c.over if k != name))


def test_row_counts():
    for op in OPS:
        for c in R.CASES:
            l, n = R.predict(c, op)[1], R.n_rows(c, op)
            per_block = 256 // l
            if c.rows == "std":
                assert n > 2 * per_block and n % per_block == 1 and n <= 2 * 256 + 1
            else:
                assert n == (1 if c.rows == "one" else per_block)


# ----------------------------------------------------------------------------
# references against each other (CPU)
# ----------------------------------------------------------------------------
def test_att_reference_matches_the_oracle():
    from oracle import hodge_ref
    D = R.att_data(R.C(36), "att_fwd")
    lam, dk = 0.25, 36
    for sigma, fn in ((R.SIGMOID, torch.sigmoid), (R.RELU, torch.relu)):
        want = hodge_ref.att_score(D.Qc.double(), D.Qs.double(), D.K.double(), lam, dk, fn)
        got = R.att_ref(D.Qc, D.Qs, D.K, 1 - lam, lam, float(np.sqrt(dk)), sigma)[0]
        close(got, want.view(-1), 1e-14, "att_ref vs oracle")


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_att_references_agree(case):
    """fp32 against fp64 inside the stated bounds, the planted rows are what
    they claim, and at most 1 % of the rows are left out of the ReLU
    gradient bound (from the fp64 reference alone)."""
    d = case.d
    D = R.att_data(case, "att_bwd")
    c = (R.W_CROSS, R.W_SELF, D.sq)
    out64, z, S = R.att_ref(D.Qc, D.Qs, D.K, *c, R.RELU)
    for r in D.zero_rows:
        assert z[r] == 0 and S[r] == 0
    for r in D.sat_rows:
        assert 99.0 < abs(float(z[r])) < 101.0
    if D.sat_rows:
        assert z[D.sat_rows[0]] > 0 > z[D.sat_rows[1]]
    if D.n > 8:
        assert (z < 0).any() and (z > 0).any()
    checked = R.relu_checked_rows(D, d)
    skipped = D.n - int(checked.sum()) - len(D.zero_rows)
    assert 0 <= skipped <= 0.01 * D.n, (skipped, D.n)
    out32, gqc, gqs, gk = R.att_fp32(D.Qc, D.Qs, D.K, *c, R.RELU, D.da)
    assert ((out32.double() - out64).abs() <= R.att_fwd_bound(d, S)).all()
    for got, ref in zip((gqc, gqs, gk), R.att_bwd_ref(D.Qc, D.Qs, D.K, *c, R.RELU, D.da)):
        assert ((got.double() - ref).abs() <= R.relu_bwd_bound(ref))[checked].all()
        assert not got[list(D.zero_rows)].any()
    out32, gqc, gqs, gk = R.att_fp32(D.Qc, D.Qs, D.K, *c, R.SIGMOID, D.da)
    s64 = R.att_ref(D.Qc, D.Qs, D.K, *c, R.SIGMOID)[0]
    assert torch.isfinite(s64).all() and (s64 >= 0).all() and (s64 <= 1).all()
    close(out32, s64, 1e-5, "sigmoid")
    for got, ref in zip((gqc, gqs, gk), R.att_bwd_ref(D.Qc, D.Qs, D.K, *c, R.SIGMOID, D.da)):
        close(got, ref, 1e-5, "sigmoid grad")


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_other_references_agree(case):
    D = R.scale_data(case, "row_scale_bwd")
    da, bound = R.row_scale_da_ref(D.dy, D.x)
    assert (((D.dy * D.x).sum(1).double() - da).abs() <= bound).all()
    close(R.row_scale_fwd(D.x, D.a), D.x.double() * D.a.double().unsqueeze(1), 1e-7, "row_scale")
    E = R.edge_data(case, "edge_absdiff_bwd")
    dd = -E.x[E.ei[0]] + E.x[E.ei[1]]
    assert int((dd == 0).sum()) >= min(E.n, 3) * case.d
    assert (E.x[2:4] == 0).all() and int(torch.signbit(E.x[2:4]).sum()) == case.d
    assert R.same_bits(R.absdiff_bwd(E), (E.g * 0.5) * torch.sgn(dd))
    assert R.same_bits(R.absdiff_fwd(E), dd.abs() / 2)
    i, j = E.ei
    full = (R.CA * (E.sa[i].double()[:, None] * E.x[i].double())
            + R.CB * (E.sb[j].double()[:, None] * E.x[j].double()) + E.z.double() + E.prev.double())
    close(R.gather2_ref(E, 1, 1, 1, 1), full, 1e-6, "gather2")
    S = R.seg_data(case, "segment_mean_fwd")
    assert set(R.SEG_LENS) >= {0, 1, 7, 8, 9, 16, 17, 40} and (S.n < 8 or set(S.lens.tolist()) == set(R.SEG_LENS))
    for listed in (False, True):
        m = R.member_rows(S, listed)
        close(R.segment_mean_seq(S.x, S.lens, m), R.segment_mean_f64(S.x, S.lens, m), 1e-6, "seg")
    assert sorted(S.rows.tolist()) == list(range(S.n_rows))


def test_fill_cases_cover_the_strides():
    rs = R.fill_ranges()
    assert {n for n, _, _ in rs} == {1023, 1024, 1025, 2500}
    assert {lo for _, lo, _ in rs} == {0, 7, 1100}
    big = [(lo, hi) for n, lo, hi in rs if n == 2500]
    for lo in (0, 7, 1100):
        his = {hi for l, hi in big if l == lo}
        assert lo in his and 2500 in his                       # empty, and up to n_rows
        assert {2047, 2048, 2049} <= his                       # around a multiple of 1024
    assert {1023, 1024, 1025} <= {hi for l, hi in big if l < 1000}
    for n, lo, hi in rs:
        p = R.split_range(lo, hi, n + lo + hi)
        assert p[0] == lo and p[-1] == hi and (p[1:] >= p[:-1]).all()
    for nz in (1, 1024, 1025, 2300):
        ptr, rows = R.pool_table(3001, nz, nz)
        assert ptr[-1] - ptr[-2] == nz and sorted(rows.tolist()) == list(range(3001))


# ----------------------------------------------------------------------------
# device plumbing
# ----------------------------------------------------------------------------
def _poison(cuda, n):
    """Leave NaN in the caching allocator's next blocks, so a torch.empty
    that is not fully written shows up."""
    for _ in range(4):
        t = torch.full((n,), float("nan"), device=cuda)
        del t


class Win:
    """A [n, d] window at column `off` of a [n + 2, ld] device buffer of
    sentinels: one guard row above and below, guard columns left and right."""

    def __init__(self, cuda, n, d, off, ld, data=None):
        assert 0 <= off and off + d <= ld
        self.n, self.d, self.off, self.ld = n, d, off, ld
        self.buf = torch.full((n + 2, ld), R.SENTINEL, dtype=torch.int32,
                              device=cuda).view(torch.float32)
        self.wins = [(off, d)]
        if data is not None:
            assert tuple(data.shape) == (n, d)
            self.buf[1:n + 1, off:off + d] = data.to(cuda)
        self.ptr = self.buf.data_ptr() + 4 * (ld + off)
        assert self.buf.data_ptr() % 16 == 0

    def view(self):
        return self.buf[1:self.n + 1, self.off:self.off + self.d]

    def at(self, off):
        """Pointer of another window of the same rows (att_score_bwd's block)."""
        self.wins.append((off, self.d))
        return self.buf.data_ptr() + 4 * (self.ld + off)

    def read(self, off=None, written=None):
        """The window after the launch: guards intact bit for bit, and every
        element (of the rows in `written`, default all) written."""
        off = self.off if off is None else off
        host = R.bits(self.buf.cpu())
        guard = torch.ones_like(host, dtype=torch.bool)
        for o, d in self.wins:
            guard[1:self.n + 1, o:o + d] = False
        assert (host[guard] == R.SENTINEL).all(), "a guard element was overwritten"
        w = host[1:self.n + 1, off:off + self.d]
        rows = torch.ones(self.n, dtype=torch.bool) if written is None else written
        assert (w[rows] != R.SENTINEL).all(), "an element of the window was not written"
        assert (w[~rows] == R.SENTINEL).all(), "a row outside the op's range was written"
        return w.view(torch.float32).clone()


def _win(cuda, case, name, n, data=None):
    off, ld = case.at(name)
    return Win(cuda, n, case.d, off, ld, data)


def _vec(cuda, n, data=None):
    """A length-n vector with a guard element on each side (read()[0])."""
    return Win(cuda, 1, n, 1, n + 2, None if data is None else data.view(1, n))


class Run:
    """The launches of one op at one placement: calls = [((V, L), fn)], and
    check() compares what they wrote."""

    def __init__(self, op, case):
        self.op, self.case, self.calls, self.checks, self.keep = op, case, [], [], []

    def call(self, fn, absent=()):
        self.calls.append((R.predict(self.case, self.op, absent), fn))

    def launch(self):
        for _, fn in self.calls:
            fn()

    def check(self):
        for fn in self.checks:
            fn()


def _lib():
    from hlhgat import ops
    from hlhgat._lib import LIB, check
    return LIB, check, ops._stream


def _dev(cuda, t):
    return t.to(cuda)


def prep_att_fwd(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("att_fwd", case), case.d
    D = R.att_data(case, "att_fwd")
    n = D.n
    w = {nm: _win(cuda, case, nm, n, getattr(D, nm)) for nm in ("Qc", "Qs", "K")}
    for sigma in (R.SIGMOID, R.RELU):
        out = _vec(cuda, n)
        run.call(lambda sigma=sigma, out=out: check(LIB.hlhgat_att_score_fwd(
            n, d, w["Qc"].ptr, w["Qc"].ld, w["Qs"].ptr, w["Qs"].ld, w["K"].ptr, w["K"].ld,
            R.W_CROSS, R.W_SELF, D.sq, sigma, out.ptr, stream(out.buf)), "att_score_fwd"))
        run.checks.append(lambda sigma=sigma, out=out: _check_att_fwd(D, d, sigma, out.read()[0]))
    return run


def _check_att_fwd(D, d, sigma, got):
    ref, _, S = R.att_ref(D.Qc, D.Qs, D.K, R.W_CROSS, R.W_SELF, D.sq, sigma)
    zero = list(D.zero_rows)
    if sigma == R.RELU:
        _within(got, ref, R.att_fwd_bound(d, S), "att_score fwd relu")
        assert not got[zero].any()
    else:
        assert torch.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
        _seen("att_score fwd sigmoid close", close(got, ref, 1e-5, "att_score fwd sigmoid"))
        assert (got[zero] == 0.5).all()
        if D.sat_rows:
            assert got[D.sat_rows[0]] == 1.0 and got[D.sat_rows[1]] < 1e-30


def prep_att_bwd(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("att_bwd", case), case.d
    D = R.att_data(case, "att_bwd")
    n = D.n
    w = {nm: _win(cuda, case, nm, n, getattr(D, nm)) for nm in ("Qc", "Qs", "K")}
    da = _dev(cuda, D.da)
    ldg, cols = case.g_block()
    for sigma in (R.SIGMOID, R.RELU):
        a = torch.empty(n, device=cuda)
        # the forward output the backward reads: the device's own, made now
        check(LIB.hlhgat_att_score_fwd(
            n, d, w["Qc"].ptr, w["Qc"].ld, w["Qs"].ptr, w["Qs"].ld, w["K"].ptr, w["K"].ld,
            R.W_CROSS, R.W_SELF, D.sq, sigma, a.data_ptr(), stream(a)), "att_score_fwd")
        G = Win(cuda, n, d, cols["dK"], ldg)
        pqs, pqc = G.at(cols["dQs"]), G.at(cols["dQc"])
        run.keep.append((a, da))
        run.call(lambda sigma=sigma, a=a, G=G, pqs=pqs, pqc=pqc: check(LIB.hlhgat_att_score_bwd(
            n, d, w["Qc"].ptr, w["Qc"].ld, w["Qs"].ptr, w["Qs"].ld, w["K"].ptr, w["K"].ld,
            R.W_CROSS, R.W_SELF, D.sq, sigma, a.data_ptr(), da.data_ptr(), pqc, pqs, G.ptr, ldg,
            stream(a)), "att_score_bwd"))
        run.checks.append(lambda sigma=sigma, G=G: _check_att_bwd(
            D, d, sigma, [G.read(cols[nm]) for nm in ("dQc", "dQs", "dK")]))
    return run


def _check_att_bwd(D, d, sigma, got):
    refs = R.att_bwd_ref(D.Qc, D.Qs, D.K, R.W_CROSS, R.W_SELF, D.sq, sigma, D.da)
    if sigma == R.SIGMOID:
        for g, ref, nm in zip(got, refs, ("dQc", "dQs", "dK")):
            _seen("att_score bwd sigmoid close", close(g, ref, 1e-5, "att_score bwd sigmoid " + nm))
        return
    rows = R.relu_checked_rows(D, d)
    for g, ref, nm in zip(got, refs, ("dQc", "dQs", "dK")):
        _within(g[rows], ref[rows], R.relu_bwd_bound(ref[rows]), "att_score bwd relu " + nm)
        assert not g[list(D.zero_rows)].any(), "ReLU gradient at z = 0"
        assert torch.isfinite(g).all()


def _bitwise(got, want, what):
    assert R.same_bits(got, want), (
        f"{what}: {int((R.bits(got) != R.bits(want)).sum())} of {got.numel()} elements differ, "
        f"max|diff| {float((got.double() - want.double()).abs().max()):.3e}")
    _seen(what + " (bitwise) max|diff|", 0.0)


def prep_row_scale_fwd(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("row_scale_fwd", case), case.d
    D = R.scale_data(case, "row_scale_fwd")
    x, y, a = _win(cuda, case, "x", D.n, D.x), _win(cuda, case, "y", D.n), _dev(cuda, D.a)
    run.keep.append(a)
    run.call(lambda: check(LIB.hlhgat_row_scale_fwd(D.n, d, x.ptr, x.ld, a.data_ptr(), y.ptr, y.ld,
                                                    stream(a)), "row_scale_fwd"))
    run.checks.append(lambda: _bitwise(y.read(), R.row_scale_fwd(D.x, D.a), "row_scale y"))
    return run


def prep_row_scale_bwd(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("row_scale_bwd", case), case.d
    D = R.scale_data(case, "row_scale_bwd")
    x, dy, dx = (_win(cuda, case, "x", D.n, D.x), _win(cuda, case, "dy", D.n, D.dy),
                 _win(cuda, case, "dx", D.n))
    a, da = _dev(cuda, D.a), _vec(cuda, D.n)
    run.keep.append(a)
    run.call(lambda: check(LIB.hlhgat_row_scale_bwd(D.n, d, x.ptr, x.ld, a.data_ptr(), dy.ptr, dy.ld,
                                                    dx.ptr, dx.ld, da.ptr, stream(a)),
                           "row_scale_bwd"))

    def chk():
        _bitwise(dx.read(), R.row_scale_dx(D.dy, D.a), "row_scale dx")
        ref, bound = R.row_scale_da_ref(D.dy, D.x)
        _within(da.read()[0], ref, bound, "row_scale da")
    run.checks.append(chk)
    return run


def prep_edge_gather2(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("edge_gather2", case), case.d
    D = R.edge_data(case, "edge_gather2")
    x, z = _win(cuda, case, "x", D.m, D.x), _win(cuda, case, "z", D.n, D.z)
    ei, sa, sb = _dev(cuda, D.ei), _dev(cuda, D.sa), _dev(cuda, D.sb)
    run.keep.append((ei, sa, sb))
    for use_sa, use_sb, use_z, acc in R.GATHER_COMBOS:
        out = _win(cuda, case, "out", D.n, D.prev if acc else None)
        run.call(lambda a=(use_sa, use_sb, use_z, acc), out=out: check(LIB.hlhgat_edge_gather2(
            ei.data_ptr(), D.n, x.ptr, x.ld, d, sa.data_ptr() if a[0] else None,
            sb.data_ptr() if a[1] else None, R.CA, R.CB, z.ptr if a[2] else None,
            z.ld if a[2] else 0, out.ptr, out.ld, a[3], stream(ei)), "edge_gather2"),
            absent=() if use_z else ("z",))
        run.checks.append(lambda a=(use_sa, use_sb, use_z, acc), out=out: _bitwise(
            out.read(), R.gather2_ref(D, *a), "edge_gather2"))
    return run


def _prep_absdiff(case, cuda, bwd):
    LIB, check, stream = _lib()
    op = "edge_absdiff_bwd" if bwd else "edge_absdiff_fwd"
    run, d = Run(op, case), case.d
    D = R.edge_data(case, op)
    x, out = _win(cuda, case, "x", D.m, D.x), _win(cuda, case, "out", D.n)
    g = _win(cuda, case, "g", D.n, D.g) if bwd else None
    ei = _dev(cuda, D.ei)
    run.keep.append(ei)
    run.call(lambda: check(LIB.hlhgat_edge_absdiff(
        ei.data_ptr(), D.n, x.ptr, x.ld, d, g.ptr if bwd else None, g.ld if bwd else 0,
        out.ptr, out.ld, stream(ei)), op))
    run.checks.append(lambda: _bitwise(out.read(), R.absdiff_bwd(D) if bwd else R.absdiff_fwd(D), op))
    return run


def prep_edge_absdiff_fwd(case, cuda):
    return _prep_absdiff(case, cuda, False)


def prep_edge_absdiff_bwd(case, cuda):
    return _prep_absdiff(case, cuda, True)


def prep_segment_mean_fwd(case, cuda):
    LIB, check, stream = _lib()
    run, d = Run("segment_mean_fwd", case), case.d
    D = R.seg_data(case, "segment_mean_fwd")
    x = _win(cuda, case, "x", D.n_rows, D.x)
    ptr, ptr_l, rows = _dev(cuda, D.ptr), _dev(cuda, D.ptr_listed), _dev(cuda, D.rows)
    run.keep.append((ptr, ptr_l, rows))
    for listed in (False, True):
        out = _win(cuda, case, "out", D.n)
        run.call(lambda listed=listed, out=out: check(LIB.hlhgat_segment_mean_fwd(
            (ptr_l if listed else ptr).data_ptr(), rows.data_ptr() if listed else None, D.n,
            x.ptr, x.ld, d, out.ptr, out.ld, stream(ptr)), "segment_mean_fwd"))

        def chk(listed=listed, out=out):
            m, got = R.member_rows(D, listed), out.read()
            _bitwise(got, R.segment_mean_seq(D.x, D.lens, m), "segment_mean fwd")
            _seen("segment_mean fwd close vs fp64",
                  close(got, R.segment_mean_f64(D.x, D.lens, m), 1e-6, "segment_mean fwd"))
        run.checks.append(chk)
    return run


def prep_segment_mean_bwd(case, cuda):
    """hlhgat_segment_mean_bwd over contiguous segments (it zero-fills the
    uncovered rows) and over listed members (it writes the members only: the
    caller zero-fills), and hlhgat_pool_mean_bwd (listed, zero bucket)."""
    LIB, check, stream = _lib()
    run, d = Run("segment_mean_bwd", case), case.d
    D = R.seg_data(case, "segment_mean_bwd")
    N, total = D.n_rows, int(D.lens.sum())
    dout = _win(cuda, case, "dout", D.n, D.dout)
    ptr, ptr_l, rows = _dev(cuda, D.ptr), _dev(cuda, D.ptr_listed), _dev(cuda, D.rows)
    run.keep.append((ptr, ptr_l, rows))
    member_grad = R.segment_mean_bwd(D.dout, D.lens)
    for how in ("contiguous", "listed", "pool"):
        dx = _win(cuda, case, "dx", N)
        fn = LIB.hlhgat_pool_mean_bwd if how == "pool" else LIB.hlhgat_segment_mean_bwd
        run.call(lambda how=how, dx=dx, fn=fn: check(fn(
            (ptr if how == "contiguous" else ptr_l).data_ptr(),
            None if how == "contiguous" else rows.data_ptr(), D.n, dout.ptr, dout.ld, d,
            dx.ptr, dx.ld, N, stream(ptr)), "segment_mean_bwd " + how))

        def chk(how=how, dx=dx):
            m = R.member_rows(D, how != "contiguous")
            want = torch.zeros(N, d)
            want[m] = member_grad
            written = torch.ones(N, dtype=torch.bool)
            if how == "listed":
                written[:] = False
                written[m] = True
            got = dx.read(written=written)
            _bitwise(got[written], want[written], "segment_mean bwd")
        run.checks.append(chk)
    assert total > 0
    return run


PREP = {op: globals()["prep_" + op] for op in OPS}


# ----------------------------------------------------------------------------
# 2. values of every op at every placement
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("op", OPS)
def test_values(cuda, op, case):
    run = PREP[op](case, cuda)
    run.launch()
    torch.cuda.synchronize()
    run.check()


# ----------------------------------------------------------------------------
# 3. the zero-fill strides of k_segment_mean_bwd
# ----------------------------------------------------------------------------
FILL_PLACE = {3: (1, 0), 24: (4, 4)}  # d: (off, pad): V = 1 / L = 4 and V = 4 / L = 8


@gpu
@pytest.mark.parametrize("d", sorted(FILL_PLACE))
def test_zero_fill_contiguous(cuda, d):
    """More rows than the 1024 fill groups: each group strides over the rows
    and skips the covered range [lo, hi) in one step."""
    LIB, check, stream = _lib()
    off, pad = FILL_PLACE[d]
    jobs = []
    for n_rows, lo, hi in R.fill_ranges():
        ptr = R.split_range(lo, hi, n_rows + lo + hi)
        n_seg = ptr.numel() - 1
        g = torch.Generator().manual_seed(n_rows + 3 * lo + 7 * hi)
        dout = torch.randn(n_seg, d, generator=g)
        dptr, dd = ptr.to(cuda), Win(cuda, n_seg, d, off, off + d + pad, dout)
        dx = Win(cuda, n_rows, d, off, off + d + pad)
        check(LIB.hlhgat_segment_mean_bwd(dptr.data_ptr(), None, n_seg, dd.ptr, dd.ld, d, dx.ptr,
                                          dx.ld, n_rows, stream(dptr)), "segment_mean_bwd")
        jobs.append((n_rows, lo, hi, ptr, dout, dx, dptr, dd))
    # no segment at all: every row is zero-filled
    dptr0 = torch.tensor([5], dtype=torch.int32, device=cuda)
    dx0 = Win(cuda, 2500, d, off, off + d + pad)
    check(LIB.hlhgat_segment_mean_bwd(dptr0.data_ptr(), None, 0, None, d, d, dx0.ptr, dx0.ld, 2500,
                                      stream(dptr0)), "segment_mean_bwd")
    torch.cuda.synchronize()
    assert not dx0.read().view(torch.int32).any()
    for n_rows, lo, hi, ptr, dout, dx, _, _ in jobs:
        lens = (ptr[1:] - ptr[:-1]).long()
        want = torch.zeros(n_rows, d)
        want[lo:hi] = R.segment_mean_bwd(dout, lens)
        got = dx.read()
        assert not torch.isnan(got).any(), (n_rows, lo, hi)
        _bitwise(got, want, "segment_mean bwd")


@gpu
@pytest.mark.parametrize("d", sorted(FILL_PLACE))
def test_zero_fill_listed(cuda, d):
    """hlhgat_pool_mean_bwd with a zero bucket of up to 2300 rows: past 1024
    rows each fill group takes a second and third member of the bucket."""
    LIB, check, stream = _lib()
    off, pad = FILL_PLACE[d]
    n_rows, jobs = 3001, []
    for n_zero in (1, 1024, 1025, 2300):
        ptr, rows = R.pool_table(n_rows, n_zero, 11 * n_zero + d)
        n_seg = ptr.numel() - 2
        dout = torch.randn(n_seg, d, generator=torch.Generator().manual_seed(n_zero))
        dptr, drows = ptr.to(cuda), rows.to(cuda)
        dd, dx = Win(cuda, n_seg, d, off, off + d + pad, dout), Win(cuda, n_rows, d, off, off + d + pad)
        check(LIB.hlhgat_pool_mean_bwd(dptr.data_ptr(), drows.data_ptr(), n_seg, dd.ptr, dd.ld, d,
                                       dx.ptr, dx.ld, n_rows, stream(dptr)), "pool_mean_bwd")
        jobs.append((n_zero, ptr, rows, dout, dx, dptr, drows, dd))
    torch.cuda.synchronize()
    for n_zero, ptr, rows, dout, dx, _, _, _ in jobs:
        lens = (ptr[1:-1] - ptr[:-2]).long()
        want = torch.zeros(n_rows, d)
        want[rows[:n_rows - n_zero].long()] = R.segment_mean_bwd(dout, lens)
        got = dx.read()
        assert not torch.isnan(got).any(), n_zero
        assert not got[rows[n_rows - n_zero:].long()].view(torch.int32).any(), n_zero
        _bitwise(got, want, "segment_mean bwd")


# ----------------------------------------------------------------------------
# 4. the lattice is launched
# ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("op", OPS)
def test_lattice_is_launched(cuda, op):
    """Capture every table case of one kernel template into one graph and
    count its kernel nodes by instantiation: the host dispatch agrees with
    the documented rule and drops no launch."""
    from hlhgat import ops
    runs = [PREP[op](c, cuda) for c in R.CASES]
    want = collections.Counter(pair for r in runs for pair, _ in r.calls)
    assert set(want) == R.LATTICE
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        for r in runs:
            r.launch()
    h = graph.raw_cuda_graph()
    got = {(v, l): ops.graph_kernel_count(h, f"{R.KERNEL[op]}ILi{v}ELi{l}EE")[1] for v, l in R.LATTICE}
    assert got == dict(want)
    launches = sum(len(r.calls) for r in runs)
    assert sum(got.values()) == launches == ops.graph_kernel_count(h, "k_")[0]


# ----------------------------------------------------------------------------
# 5. the autograd wrappers hand the kernels the strides the table assumes
# ----------------------------------------------------------------------------
WRAP_CASES = [c for c in R.CASES if (c.d, c.off, c.pad) in ((1, 1, 1), (6, 2, 2), (36, 3, 0), (130, 2, 0))
              and not c.over and c.rows == "std"]


def test_wrapper_cases_are_table_cases():
    assert sorted(c.d for c in WRAP_CASES) == [1, 6, 36, 130]


def _leaf(w):
    """The window as a strided leaf (rows ld apart, pointer 4 * off bytes in)."""
    t = w.view().detach().requires_grad_(True)
    assert t.stride(0) == w.ld and t.data_ptr() == w.ptr
    return t


@gpu
@pytest.mark.parametrize("case", WRAP_CASES, ids=[c.label() for c in WRAP_CASES])
@pytest.mark.parametrize("sigma", [R.SIGMOID, R.RELU])
def test_wrapped_att_score(cuda, case, sigma):
    from hlhgat import ops
    d, D = case.d, R.att_data(case, "att_fwd")
    n = D.n
    w = {nm: _leaf(_win(cuda, case, nm, n, getattr(D, nm))) for nm in ("Qc", "Qs", "K")}
    # kq = [K | Qs] as one strided [n, 2d] window
    off, pad = case.off, case.pad
    kqw = Win(cuda, n, 2 * d, off, off + 2 * d + pad, torch.cat([D.K, D.Qs], 1))
    kq, qc2 = _leaf(kqw), _leaf(_win(cuda, case, "Qc", n, D.Qc))
    consts = (R.W_CROSS, R.W_SELF, D.sq, sigma)
    _poison(cuda, 4 * n * d)
    a1 = ops.att_score(w["Qc"], w["Qs"], w["K"], *consts)
    a2 = ops.att_score_kq(qc2, kq, *consts)
    assert a1.shape == (n, 1) and torch.equal(a1, a2)
    _check_att_fwd(D, d, sigma, a1.detach().cpu().view(-1))
    _poison(cuda, 4 * 3 * n * d)
    a1.backward(D.da.to(cuda).view(n, 1))
    a2.backward(D.da.to(cuda).view(n, 1))
    g1 = [w[nm].grad.cpu() for nm in ("Qc", "Qs", "K")]
    _check_att_bwd(D, d, sigma, g1)
    g2 = [qc2.grad.cpu(), kq.grad[:, d:].cpu(), kq.grad[:, :d].cpu()]
    for a, b in zip(g1, g2):
        assert R.same_bits(a, b)


@gpu
@pytest.mark.parametrize("case", WRAP_CASES, ids=[c.label() for c in WRAP_CASES])
def test_wrapped_row_scale(cuda, case):
    from hlhgat import ops
    D = R.scale_data(case, "row_scale_fwd")
    x, out = _leaf(_win(cuda, case, "x", D.n, D.x)), _win(cuda, case, "y", D.n)
    a = D.a.to(cuda).view(-1, 1).requires_grad_(True)
    y = ops.row_scale(x, a, out=out.view())
    assert y.data_ptr() == out.ptr
    _bitwise(out.read(), R.row_scale_fwd(D.x, D.a), "row_scale y")
    dy = _win(cuda, case, "dy", D.n, D.dy)
    _poison(cuda, 4 * D.n * case.d)
    y.backward(dy.view())
    _bitwise(x.grad.cpu(), R.row_scale_dx(D.dy, D.a), "row_scale dx")
    ref, bound = R.row_scale_da_ref(D.dy, D.x)
    _within(a.grad.cpu().view(-1), ref, bound, "row_scale da")


def _b1_apply(ge, ei, m):
    """fp64 (B1 ge, bound): dx[v] = sum_{e: head v} ge[e] - sum_{e: tail v}
    ge[e]; up to deg - 1 sums and a sign per term: (deg + 2) u sum|ge|."""
    ge = ge.double()
    dx = torch.zeros(m, ge.size(1), dtype=torch.float64).index_add_(0, ei[1], ge).index_add_(0, ei[0], -ge)
    mag = torch.zeros_like(dx).index_add_(0, ei[1], ge.abs()).index_add_(0, ei[0], ge.abs())
    deg = torch.zeros(m, dtype=torch.float64).index_add_(0, ei.reshape(-1), torch.ones(ei.numel(), dtype=torch.float64))
    return dx, (deg + 2).unsqueeze(1) * U * mag


def _simple_graph(E):
    """EdgeData with an undirected simple edge list (i < j) for ops.incidence."""
    i = torch.minimum(E.ei[0], E.ei[1])
    j = torch.maximum(E.ei[0], E.ei[1])
    j = torch.where(i == j, (j + 1) % E.m, j)
    i, j = torch.minimum(i, j), torch.maximum(i, j)
    # nodes 0 and 1 carry the same features, nodes 2 and 3 opposite zeros
    return E._replace(ei=torch.stack([i, j]).contiguous())


@gpu
@pytest.mark.parametrize("case", WRAP_CASES, ids=[c.label() for c in WRAP_CASES])
def test_wrapped_boundary_products(cuda, case):
    """boundary_t, incidence_mm(transposed=True) and tsp_readout with an odd
    cs (the window pointer is then 4 * cs bytes off) on a strided x_t."""
    from hlhgat import ops
    d = case.d
    E = _simple_graph(R.edge_data(case, "edge_absdiff_fwd"))
    inc = ops.incidence(E.ei.to(cuda), E.m)
    i, j = E.ei
    gy = E.g.to(cuda)
    for how in ("boundary_t", "signed", "unsigned"):
        x = _leaf(_win(cuda, case, "x", E.m, E.x))
        _poison(cuda, 4 * E.n * d)
        if how == "boundary_t":
            y = ops.boundary_t(x, inc)
        else:
            y = ops.incidence_mm(x, inc, transposed=True, signed=how == "signed")
        want = E.x[i] + E.x[j] if how == "unsigned" else -E.x[i] + E.x[j]
        _bitwise(y.detach().cpu(), want, "edge_gather2")
        y.backward(gy)
        ref, bound = _b1_apply(E.g, E.ei, E.m)
        if how == "unsigned":
            ref = torch.zeros_like(ref).index_add_(0, j, E.g.double()).index_add_(0, i, E.g.double())
        _within(x.grad.cpu(), ref, bound, "B1 product")
    cs = 3
    x = _leaf(_win(cuda, case, "x", E.m, E.x))
    xs = torch.randn(E.n, cs, generator=torch.Generator().manual_seed(d)).to(cuda).requires_grad_(True)
    slab = Win(cuda, E.n, cs + d, 4, 4 + cs + d + 1)
    slab.view()[:, :cs] = xs.detach()
    out = ops.tsp_readout(xs, x, inc, slab.view())
    assert out.data_ptr() == slab.ptr
    got = slab.read()
    _bitwise(got[:, cs:], R.absdiff_fwd(E), "edge_absdiff_fwd")
    assert torch.equal(got[:, :cs], xs.detach().cpu())
    W = torch.randn(E.n, cs + d, generator=torch.Generator().manual_seed(d + 1))
    _poison(cuda, 4 * E.n * d)
    out.backward(W.to(cuda))
    assert torch.equal(xs.grad.cpu(), W[:, :cs])
    ge = R.absdiff_bwd(E._replace(g=W[:, cs:].contiguous()))
    ref, bound = _b1_apply(ge, E.ei, E.m)
    _within(x.grad.cpu(), ref, bound, "B1 product")


@gpu
@pytest.mark.parametrize("case", WRAP_CASES, ids=[c.label() for c in WRAP_CASES])
def test_wrapped_segment_mean_covering(cuda, case):
    from hlhgat import ops
    D = R.seg_data(case, "segment_mean_fwd")
    x, out = _leaf(_win(cuda, case, "x", D.n_rows, D.x)), _win(cuda, case, "out", D.n)
    y = ops.segment_mean(x, D.ptr_listed.to(cuda), D.n, D.rows.to(cuda), out=out.view(), covering=True)
    assert y.data_ptr() == out.ptr
    m = R.member_rows(D, True)
    _bitwise(out.read(), R.segment_mean_seq(D.x, D.lens, m), "segment_mean fwd")
    _poison(cuda, 4 * D.n_rows * case.d)
    y.backward(_win(cuda, case, "dout", D.n, D.dout).view())
    want = torch.zeros(D.n_rows, case.d)
    want[m] = R.segment_mean_bwd(D.dout, D.lens)
    _bitwise(x.grad.cpu(), want, "segment_mean bwd")
