"""numpy restatement of the PE sign-flip draw of csrc/peflip.hip (DESIGN.md
§32) on top of dropout_ref.philox.  The GPU tests compare the kernel against
it bit for bit.

  graph g, flipped column j:
    w    = word (j & 3) of philox({g, 0x50450000 + (j >> 2), site, step lo},
                                  {seed lo, seed hi})
    sign = (w >> 31) ? -1.0 : +1.0
  site = 2k + side (k: the module's ordinal, side 0 = t, 1 = s)
  rows >= seg_ptr[G] (padding): unflipped
"""
import numpy as np

from dropout_ref import philox

COUNTER = 0x50450000


def site_word(k=0, side=0):
    return 2 * int(k) + int(side)


def signs(G, n_flip, seed, step, k=0, side=0):
    """float32 [G, n_flip] of +1 / -1."""
    out = np.ones((G, n_flip), dtype=np.float32)
    if G == 0 or n_flip == 0:
        return out
    groups = (n_flip + 3) // 4
    g = np.repeat(np.arange(G, dtype=np.uint32), groups)
    q = np.tile(np.arange(groups, dtype=np.uint32), G)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox([g, np.uint32(COUNTER) + q, np.uint32(site_word(k, side)),
                np.uint32(int(step) & 0xFFFFFFFF)], [seed & 0xFFFFFFFF, seed >> 32])
    w = np.stack(w, axis=1).reshape(G, groups * 4)[:, :n_flip]
    out[(w >> np.uint32(31)) != 0] = -1.0
    return out


def row_graph(seg_ptr, n_rows):
    """int64 [n_rows]: the graph of every row, -1 for rows in no graph."""
    seg = np.asarray(seg_ptr, dtype=np.int64)
    r = np.arange(n_rows, dtype=np.int64)
    g = np.searchsorted(seg[1:], r, side="right")
    G = seg.size - 1
    ok = (g < G) & (r >= seg[np.minimum(g, G - 1)] if G else False)
    return np.where(ok, g, -1)


def flip(x, seg_ptr, n_fixed, n_flip, seed, step, k=0, side=0):
    """y = x[:, :n_fixed + n_flip] * sign in float32; padding rows unchanged."""
    x = np.asarray(x, dtype=np.float32)[:, :n_fixed + n_flip].copy()
    g = row_graph(seg_ptr, x.shape[0])
    s = signs(len(seg_ptr) - 1, n_flip, seed, step, k, side)
    real = g >= 0
    x[real, n_fixed:] = x[real, n_fixed:] * s[g[real]]
    return x
