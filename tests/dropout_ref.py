"""numpy restatement of the dropout mask rule of csrc/dropout.hip (DESIGN.md,
"Training-mode dropout"): Philox4x32-10 over (element group, site, step) keyed
by the seed.  The GPU tests compare the kernels against it bit for bit."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def _mulhilo(m, c):
    prod = np.uint64(m) * c.astype(np.uint64)  # < 2^64: exact
    return (prod >> np.uint64(32)).astype(np.uint32), (prod & _U32).astype(np.uint32)


def philox(counter, key):
    """Philox4x32-10.  counter: 4 uint32 arrays (or scalars) of one shape,
    key: 2 uint32 scalars; returns the 4 output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint32)) for w in counter]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(w, shape).copy() for w in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        hi0, lo0 = _mulhilo(M0, c[0])
        hi1, lo1 = _mulhilo(M1, c[2])
        c = [hi1 ^ c[1] ^ np.uint32(k0), lo1, hi0 ^ c[3] ^ np.uint32(k1), lo0]
        k0 = (k0 + W0) & 0xFFFFFFFF
        k1 = (k1 + W1) & 0xFFFFFFFF
    return c


def threshold(p):
    """T = floor(p * 2^24), computed in double."""
    return int(np.floor(float(p) * 16777216.0))


def scale(p):
    """s = float32(1 / (1 - p)): computed in double, rounded once (0 at p = 1)."""
    return np.float32(0.0) if float(p) == 1.0 else np.float32(1.0 / (1.0 - float(p)))


def keep(n, d, p, seed, step, site):
    """Boolean [n, d] keep mask: element e = row * d + col takes word e & 3 of
    philox({g lo, g hi, site, step lo}, {seed lo, seed hi}), g = e >> 2, and is
    kept iff (word >> 8) >= T."""
    total = n * d
    g = np.arange((total + 3) // 4, dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox([(g & _U32).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                    np.uint32(int(site) & 0xFFFFFFFF), np.uint32(int(step) & 0xFFFFFFFF)],
                   [seed & 0xFFFFFFFF, seed >> 32])
    w = np.stack(words, axis=1).reshape(-1)[:total]
    return ((w >> np.uint32(8)) >= np.uint32(threshold(p))).reshape(n, d)


def apply(x, p, seed, step, site):
    """y = keep ? x * s : 0 in float32."""
    x = np.asarray(x, dtype=np.float32)
    m = keep(x.shape[0], x.shape[1], p, seed, step, site)
    return np.where(m, x * scale(p), np.float32(0.0)).astype(np.float32)
