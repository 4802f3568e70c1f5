"""CPU side of tests/test_row_kernels.py: the placement table of the row-wise
kernels (csrc/attention.hip, csrc/poly.hip), the (V, L) pair each placement
must dispatch to, deterministic inputs and the references.

V and L follow the rule the kernel sources document ("Widest vector width V
in {4,2,1} that divides d and every row stride and keeps every base pointer
aligned; lanes per row = next pow2 of d/V (<= 64)"), restated here without
calling the library.

References: the elementwise ops and the sequential segment sum are CPU fp32
torch, one op per rounding (the library is built with -ffp-contract=off), so
the kernels must match them bit for bit; the dot products (att_score,
row_scale's da) are fp64 with a derived forward-error bound."""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24           # unit roundoff of fp32 (round to nearest)
SENTINEL = 0x7FC0DEAD    # a quiet NaN with a payload no kernel produces

SIGMOID, RELU = 0, 1     # HLHGAT_SIGMA_*
W_CROSS, W_SELF = float(np.float32(0.7)), float(np.float32(0.3))
CA, CB = float(np.float32(-1.25)), float(np.float32(0.3))

# operands whose stride and base pointer the host dispatch inspects
OPERANDS = {
    "att_fwd": ("Qc", "Qs", "K"),
    "att_bwd": ("Qc", "Qs", "K", "dK", "dQs", "dQc"),
    "row_scale_fwd": ("x", "y"),
    "row_scale_bwd": ("x", "dy", "dx"),
    "edge_gather2": ("x", "out", "z"),
    "edge_absdiff_fwd": ("x", "out"),
    "edge_absdiff_bwd": ("x", "g", "out"),
    "segment_mean_fwd": ("x", "out"),
    "segment_mean_bwd": ("dout", "dx"),
}
# kernel template of each op (the mangled name carries <V, L> as ILi{V}ELi{L}EE)
KERNEL = {
    "att_fwd": "k_att_fwd", "att_bwd": "k_att_bwd",
    "row_scale_fwd": "k_row_scale_fwd", "row_scale_bwd": "k_row_scale_bwd",
    "edge_gather2": "k_edge_gather2",
    "edge_absdiff_fwd": "k_edge_absdiff_fwd", "edge_absdiff_bwd": "k_edge_absdiff_bwd",
    "segment_mean_fwd": "k_segment_mean_fwd", "segment_mean_bwd": "k_segment_mean_bwd",
}
G_BLOCK = ("dK", "dQs", "dQc")  # column order of att_score_bwd's one gradient block

LATTICE = frozenset((v, l) for v in (1, 2, 4) for l in (1, 2, 4, 8, 16, 32, 64))


class Case(namedtuple("Case", "d off pad over rows")):
    """Every operand is base[:, off:off + d] of a [n, off + d + pad] buffer;
    `over` gives single operands their own (off, pad).  rows: "std" =
    2 * (256 / L) + 1, "one" = 1, "exact" = 256 / L."""

    def at(self, name):
        """(column offset, row stride) of operand `name`."""
        off, pad = dict(self.over).get(name, (self.off, self.pad))
        return off, off + self.d + pad

    def g_block(self):
        """att_score_bwd writes dK, dQs, dQc into ONE buffer with one ldg: the
        three windows side by side, each with its own (off, pad).  All (0, 0)
        is the att_score_kq layout (columns 0, dk, 2dk of a [n, 3dk] block)."""
        cols, c = {}, 0
        for name in G_BLOCK:
            off, ld = self.at(name)
            cols[name] = c + off
            c += ld
        return c, cols

    def label(self):
        o = "".join(f"-{k}{a}.{b}" for k, (a, b) in self.over)
        return f"d{self.d}o{self.off}p{self.pad}{o}" + ("" if self.rows == "std" else "-" + self.rows)


def C(d, off=0, pad=0, rows="std", **over):
    return Case(d, off, pad, tuple(sorted(over.items())), rows)


CASES = (
    # V = 4: d, every offset and every stride a multiple of 4
    C(4), C(8, 4, 0), C(12, 0, 4), C(20, 4, 8), C(36, 0, 0), C(64, 4, 4), C(128, 0, 4),
    C(256, 4, 0), C(260), C(300, 0, 4),
    # V = 2
    C(2, 2, 0), C(4, 2, 0), C(6), C(6, 2, 2), C(16, 2, 0), C(32, 0, 2), C(36, 2, 0), C(64, 2, 2),
    C(128, 0, 2), C(130), C(130, 2, 0),
    # V = 1
    C(1), C(1, 1, 1), C(2, 1, 0), C(3), C(5, 1, 0), C(7, 0, 2), C(16, 1, 0), C(32, 0, 1),
    C(36, 3, 0), C(64, 3, 0), C(65), C(129, 1, 1), C(200, 0, 1),
    # one operand alone breaks the alignment of an otherwise V = 4 call:
    # a misaligned pointer (1, 3) / (2, 2), or only an odd / even stride (0, 2)
    C(8, Qc=(1, 3), x=(1, 3), dout=(1, 3)),
    C(8, Qs=(2, 2), y=(2, 2), dx=(2, 2), out=(2, 2)),
    C(8, K=(0, 2), dy=(0, 2), z=(0, 2), g=(0, 2)),
    C(8, dQc=(1, 3), z=(1, 3), g=(2, 2), dx=(0, 1)),
    C(8, dQs=(2, 2), dy=(1, 3), out=(0, 1)),
    C(8, dK=(2, 2), x=(0, 2)),
    C(8, dQc=(0, 2), y=(0, 1), dout=(0, 2)),
    # one row, and exactly one full block
    C(8, 4, 0, rows="one"), C(130, rows="one"), C(3, rows="one"),
    C(12, 0, 4, rows="exact"), C(5, 1, 0, rows="exact"), C(6, rows="exact"),
)


def pick_v(d, placements):
    for v in (4, 2):
        if d % v == 0 and all(off % v == 0 and ld % v == 0 for off, ld in placements):
            return v
    return 1


def pick_l(d, v):
    lanes, l = -(-d // v), 1
    while l < lanes:
        l *= 2
    return min(l, 64)


def placements(case, op, absent=()):
    out = []
    for name in OPERANDS[op]:
        if name in absent:
            continue
        if op == "att_bwd" and name in G_BLOCK:
            ldg, cols = case.g_block()
            out.append((cols[name], ldg))
        else:
            out.append(case.at(name))
    return out


def predict(case, op, absent=()):
    """(V, L) the documented rule gives this call."""
    v = pick_v(case.d, placements(case, op, absent))
    return v, pick_l(case.d, v)


def n_rows(case, op):
    l = predict(case, op)[1]
    return {"std": 2 * (256 // l) + 1, "one": 1, "exact": 256 // l}[case.rows]


def _gen(case, op):
    return torch.Generator().manual_seed(zlib.crc32(repr((tuple(case), op)).encode()))


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


# ----------------------------------------------------------------------------
# att_score
# ----------------------------------------------------------------------------
def att_ref(Qc, Qs, K, c1, c2, sq, sigma):
    """fp64 (out [n], z [n], S [n]):  z = (c1<Qc,K> + c2<Qs,K>) / sq and
    S = (|c1| sum|Qc K| + |c2| sum|Qs K|) / sq, the scale of z's rounding
    error:  dk products and dk - 1 sums per dot product (<= dk u each,
    whatever the summation order), c1 *, +, / sq: |z32 - z| <= (dk + 4) u S."""
    Qc, Qs, K = Qc.double(), Qs.double(), K.double()
    z = (c1 * (Qc * K).sum(1) + c2 * (Qs * K).sum(1)) / sq
    S = (abs(c1) * (Qc * K).abs().sum(1) + abs(c2) * (Qs * K).abs().sum(1)) / sq
    out = torch.sigmoid(z) if sigma == SIGMOID else torch.relu(z)
    return out, z, S


def att_fwd_bound(dk, S):
    return (dk + 4) * U * S


def att_bwd_ref(Qc, Qs, K, c1, c2, sq, sigma, da):
    """fp64 (dQc, dQs, dK) of sum(da * out)."""
    out, z, _ = att_ref(Qc, Qs, K, c1, c2, sq, sigma)
    dz = da.double() * (out * (1.0 - out) if sigma == SIGMOID else (z > 0).double())
    dzs = (dz / sq).unsqueeze(1)
    return c1 * dzs * K.double(), c2 * dzs * K.double(), c1 * dzs * Qc.double() + c2 * dzs * Qs.double()


def att_fp32(Qc, Qs, K, c1, c2, sq, sigma, da=None):
    """The kernels' arithmetic in CPU fp32 (torch's own summation order)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    z = (f(c1) * (Qc * K).sum(1) + f(c2) * (Qs * K).sum(1)) / f(sq)
    out = 1.0 / (1.0 + torch.exp(-z)) if sigma == SIGMOID else torch.relu(z)
    if da is None:
        return out
    dz = da * (out * (1.0 - out)) if sigma == SIGMOID else torch.where(out > 0, da, torch.zeros(()))
    dzs = dz / f(sq)
    d1, d2 = (f(c1) * dzs).unsqueeze(1), (f(c2) * dzs).unsqueeze(1)
    return out, d1 * K, d2 * K, d1 * Qc + d2 * Qs


AttData = namedtuple("AttData", "n Qc Qs K da sq zero_rows sat_rows")


@functools.lru_cache(maxsize=None)
def att_data(case, op):
    """Inputs of one att_score call.  Qs shares Qc's signs elementwise, so
    with w_cross, w_self > 0 the two terms of dK never cancel and its error
    stays relative to |dK| (see relu_bwd_bound).  Planted rows (n >= 8):
    0 all zero, 1 Qc = Qs = 0 under a live K (z = 0 with a non-zero key),
    2 and 3 scaled to z = +100 and -100."""
    n, d, g = n_rows(case, op), case.d, _gen(case, "att")
    Qc = torch.randn(n, d, generator=g)
    Qs = torch.randn(n, d, generator=g).abs() * torch.where(Qc >= 0, 1.0, -1.0)
    K = torch.randn(n, d, generator=g)
    da = torch.randn(n, generator=g)
    sq = float(np.float32(np.sqrt(d)))
    zero_rows, sat_rows = [], []
    if n >= 8:
        for r, sgn in ((2, 1.0), (3, -1.0)):
            K[r] = Qc[r]
            z0 = float(att_ref(Qc[r:r + 1], Qs[r:r + 1], K[r:r + 1], W_CROSS, W_SELF, sq, RELU)[1])
            K[r] = (K[r].double() * (sgn * 100.0 / z0)).float()
            sat_rows.append(r)
        Qc[1] = 0.0
        Qs[1] = 0.0
        zero_rows.append(1)
    if n > 1:
        Qc[0] = 0.0
        Qs[0] = 0.0
        K[0] = 0.0
        zero_rows.append(0)
    return AttData(n, Qc, Qs, K, da, sq, tuple(zero_rows), tuple(sat_rows))


def relu_checked_rows(data, d):
    """Rows whose ReLU mask no forward rounding can flip: fp64 |z| above the
    forward bound.  The planted z = 0 rows are checked for an exactly zero
    gradient instead."""
    _, z, S = att_ref(data.Qc, data.Qs, data.K, W_CROSS, W_SELF, data.sq, RELU)
    return z.abs() > att_fwd_bound(d, S)


def relu_bwd_bound(ref):
    """dQc = (c1 * (dz / sq)) * K: three roundings, (1 + u)^3 - 1 < 4u.  dK =
    d1 * Qc + d2 * Qs adds one more, relative to |d1 Qc| + |d2 Qs|, which is
    |dK| for the sign-matched inputs of att_data."""
    return 4 * U * ref.abs()


# ----------------------------------------------------------------------------
# row_scale
# ----------------------------------------------------------------------------
ScaleData = namedtuple("ScaleData", "n x a dy")


@functools.lru_cache(maxsize=None)
def scale_data(case, op):
    n, g = n_rows(case, op), _gen(case, "scale")
    return ScaleData(n, torch.randn(n, case.d, generator=g), torch.randn(n, generator=g),
                     torch.randn(n, case.d, generator=g))


def row_scale_fwd(x, a):
    return x * a.unsqueeze(1)


def row_scale_dx(dy, a):
    return dy * a.unsqueeze(1)


def row_scale_da_ref(dy, x):
    """fp64 (da, bound): d products and d - 1 sums in any order."""
    p = dy.double() * x.double()
    return p.sum(1), (x.size(1) + 2) * U * p.abs().sum(1)


# ----------------------------------------------------------------------------
# edge gathers
# ----------------------------------------------------------------------------
EdgeData = namedtuple("EdgeData", "n m ei x sa sb z prev g")

# (sa, sb, z, accumulate): the eight on/off combinations, and each scale alone
GATHER_COMBOS = tuple((s, s, z, acc) for s in (0, 1) for z in (0, 1) for acc in (0, 1)) + \
    ((1, 0, 1, 0), (0, 1, 0, 1))


@functools.lru_cache(maxsize=None)
def edge_data(case, op):
    """n edges over m nodes.  Edges 0 and 1 are loops, node 1 copies node 0
    (edge 2), node 2 alternates +0.0 / -0.0 and node 3 is its negation
    (edges 3 to 5): x_i == x_j exactly, the sgn = 0 branch."""
    n, d, g = n_rows(case, op), case.d, _gen(case, "edge")
    m = n // 2 + 4
    ei = torch.randint(0, m, (2, n), generator=g)
    x = torch.randn(m, d, generator=g)
    x[1] = x[0]
    x[2] = torch.where(torch.arange(d) % 2 == 0, 0.0, -0.0)
    x[3] = -x[2]
    for e, (i, j) in enumerate(((5 % m, 5 % m), (m - 1, m - 1), (0, 1), (2, 2), (2, 3), (3, 2))):
        if e < n - 1 or n == 1 and e == 0:
            ei[0, e], ei[1, e] = i, j
    r = lambda *s: torch.randn(*s, generator=g)
    return EdgeData(n, m, ei.contiguous(), x, r(m), r(m), r(n, d), r(n, d), r(n, d))


def gather2_ref(D, use_sa, use_sb, use_z, acc):
    """ca*(sa[i]*x[i]) + cb*(sb[j]*x[j]), then + z, then + out (fp32, one op
    per rounding; an absent scale is a multiplication by 1.0, exact)."""
    i, j = D.ei[0], D.ei[1]
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    xi = D.sa[i].unsqueeze(1) * D.x[i] if use_sa else D.x[i]
    xj = D.sb[j].unsqueeze(1) * D.x[j] if use_sb else D.x[j]
    o = f(CA) * xi + f(CB) * xj
    if use_z:
        o = D.z + o
    if acc:
        o = D.prev + o
    return o


def _sgn(dd):
    one = torch.ones(())
    return torch.where(dd > 0, one, torch.where(dd < 0, -one, 0 * one))


def absdiff_fwd(D):
    return (-D.x[D.ei[0]] + D.x[D.ei[1]]).abs() * 0.5


def absdiff_bwd(D):
    return (D.g * 0.5) * _sgn(-D.x[D.ei[0]] + D.x[D.ei[1]])


# ----------------------------------------------------------------------------
# segment mean
# ----------------------------------------------------------------------------
SEG_LENS = (8, 0, 1, 7, 9, 16, 17, 40)  # around the 8-row unrolled sum
SEG_LEAD, SEG_TAIL = 2, 3               # rows no segment covers

SegData = namedtuple("SegData", "n lens ptr ptr_listed rows n_rows x dout")


@functools.lru_cache(maxsize=None)
def seg_data(case, op):
    """n segments of the lengths SEG_LENS in turn.  Contiguous: members are
    rows ptr[s]..ptr[s+1], ptr[0] = SEG_LEAD, SEG_TAIL rows behind the last.
    Listed: rows[ptr_listed[s]:ptr_listed[s+1]] of a permutation of all
    rows; the bucket after the last segment lists the rows in no segment."""
    n, g = n_rows(case, op), _gen(case, "seg")
    lens = torch.tensor([SEG_LENS[s % len(SEG_LENS)] for s in range(n)])
    cum = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])
    total = int(cum[-1])
    N = SEG_LEAD + total + SEG_TAIL
    rows = torch.randperm(N, generator=g).to(torch.int32)
    ptr_listed = torch.cat([cum, torch.tensor([N])]).to(torch.int32)
    return SegData(n, lens, (SEG_LEAD + cum).to(torch.int32), ptr_listed, rows, N,
                   torch.randn(N, case.d, generator=g), torch.randn(n, case.d, generator=g))


def member_rows(D, listed):
    """[total] row of every member, segment by segment in member order."""
    total = int(D.lens.sum())
    return D.rows[:total].long() if listed else SEG_LEAD + torch.arange(total)


def segment_mean_seq(x, lens, members):
    """fp32 sum in member order from 0.0, then / max(cnt, 1)."""
    lens = lens.long()
    start = torch.cat([torch.zeros(1, dtype=torch.long), lens.cumsum(0)])[:-1]
    acc = torch.zeros(lens.numel(), x.size(1), dtype=x.dtype)
    for t in range(int(lens.max()) if lens.numel() else 0):
        live = lens > t
        acc[live] = acc[live] + x[members[start[live] + t]]
    return acc / lens.clamp(min=1).to(x.dtype).unsqueeze(1)


def segment_mean_f64(x, lens, members):
    """torch_scatter.scatter_mean in fp64 (oracle.hodge_ref.scatter_mean)."""
    from oracle.hodge_ref import scatter_mean
    if lens.numel() == 0 or int(lens.sum()) == 0:
        return torch.zeros(lens.numel(), x.size(1), dtype=torch.float64)
    index = torch.repeat_interleave(torch.arange(lens.numel()), lens.long())
    return scatter_mean(x.double()[members], index, dim_size=lens.numel())


def segment_mean_bwd(dout, lens):
    """[total, d]: dout[s] / max(cnt, 1) for each member, in member order."""
    q = dout / lens.clamp(min=1).to(dout.dtype).unsqueeze(1)
    return torch.repeat_interleave(q, lens.long(), dim=0)


# ----------------------------------------------------------------------------
# the zero fill of k_segment_mean_bwd (1024 lane groups, then strides)
# ----------------------------------------------------------------------------
def fill_ranges():
    """(n_rows, lo, hi): covered ranges ending before, at and after a
    multiple of 1024, at n_rows, and empty ones."""
    out = []
    for n in (1023, 1024, 1025, 2500):
        for lo in (0, 7, 1100):
            if lo > n:
                continue
            for hi in (lo, 1000, 1023, 1024, 1025, 1500, 2047, 2048, 2049, n):
                if lo <= hi <= n and (n, lo, hi) not in out:
                    out.append((n, lo, hi))
    return out


def split_range(lo, hi, seed):
    """int32 ptr of segments (lengths 0..40) that tile [lo, hi)."""
    g = torch.Generator().manual_seed(seed)
    ptr = [lo]
    while ptr[-1] < hi:
        ptr.append(min(hi, ptr[-1] + int(torch.randint(0, 41, (1,), generator=g))))
    if len(ptr) == 1:
        ptr.append(lo)  # one empty segment
    return torch.tensor(ptr, dtype=torch.int32)


def pool_table(n_rows, n_zero, seed):
    """(ptr int32 [n_seg + 2], rows int32 [n_rows]): a permutation of the
    rows cut into segments of 1..40 members and a trailing bucket of n_zero
    rows scattered through the range."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(n_rows, generator=g).to(torch.int32)
    ptr, live = [0], n_rows - n_zero
    while ptr[-1] < live:
        ptr.append(min(live, ptr[-1] + int(torch.randint(1, 41, (1,), generator=g))))
    return torch.tensor(ptr + [n_rows], dtype=torch.int32), rows
