"""numpy restatement of the simplex-dropout draw of csrc/simplex.hip (DESIGN.md
§28) on top of dropout_ref.philox.  The GPU tests compare the kernel against it
bit for bit.

  graph g:  (a0, a1, ., .) = philox({g, 0, SITE_G, step lo}, key)
            aug_g = (a0 >> 8) < Ta;  T_g = Tp + ((uint64(a1 >> 8) * Tj) >> 24)
  row e:    u_e = word (e & 3) of philox({(e>>2) lo, (e>>2) hi, SITE_E, step lo},
                  key) >> 8
            keep_e = !aug_g || u_e >= T_g || protect[e] != 0
  rows >= seg_ptr[G]: 0
  SITE_G = 0x80000000 + 2k, SITE_E = SITE_G + 1 (k: the module's ordinal)
"""
import numpy as np

from dropout_ref import philox, threshold

_U32 = np.uint64(0xFFFFFFFF)
SITE0 = 0x80000000


def sites(k=0):
    return SITE0 + 2 * int(k), SITE0 + 2 * int(k) + 1


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return [seed & 0xFFFFFFFF, seed >> 32]


def graph_draw(G, aug_prob, p, jitter, seed, step, k=0):
    """(aug [G] bool, T [G] uint32): which graphs are augmented, and their
    integer drop thresholds."""
    Ta, Tp, Tj = threshold(aug_prob), threshold(p), threshold(jitter)
    assert Tp + Tj <= 1 << 24
    g = np.arange(G, dtype=np.uint32)
    a = philox([g, np.uint32(0), np.uint32(sites(k)[0]), np.uint32(int(step) & 0xFFFFFFFF)],
               _key(seed))
    aug = (a[0] >> np.uint32(8)) < np.uint32(Ta) if G else np.zeros(0, bool)
    T = np.uint64(Tp) + (((a[1] >> np.uint32(8)).astype(np.uint64) * np.uint64(Tj))
                         >> np.uint64(24))
    return np.asarray(aug, bool)[:G], T.astype(np.uint32)[:G]


def row_words(n_rows, seed, step, k=0):
    """u_e for e < n_rows (uint32, 24 bits)."""
    q = np.arange((n_rows + 3) // 4, dtype=np.uint64)
    w = philox([(q & _U32).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                np.uint32(sites(k)[1]), np.uint32(int(step) & 0xFFFFFFFF)], _key(seed))
    return (np.stack(w, axis=1).reshape(-1)[:n_rows] >> np.uint32(8)).astype(np.uint32)


def keep(seg_ptr, n_rows, aug_prob, p, jitter, seed, step, k=0, protect=None):
    """float32 [n_rows] mask of {0, 1}."""
    seg = np.asarray(seg_ptr, dtype=np.int64)
    G = seg.size - 1
    assert n_rows >= seg[-1]
    aug, T = graph_draw(G, aug_prob, p, jitter, seed, step, k)
    u = row_words(n_rows, seed, step, k)
    out = np.zeros(n_rows, dtype=np.float32)
    prot = np.zeros(n_rows, bool) if protect is None else np.asarray(protect).reshape(-1) != 0
    for g in range(G):
        s = slice(int(seg[g]), int(seg[g + 1]))
        out[s] = (~aug[g]) | (u[s] >= T[g]) | prot[s]
    return out
