"""Plain-numpy statements of what sf_chol_plan_solve_half / _quadform / _sample (sf_sample.hip) compute: the Philox4x32-10 normal
generator exactly as include/sparseframe_flat.h specifies it, and the supernodal half solves over the reference layout.

Element (i, s) of the infinite normal matrix -- i = permuted row, s = global sample index -- depends on (seed, i, s) alone:
counter (i lo, i hi, p lo, p hi) with p = s >> 1, key (seed lo, seed hi), four output words -> two uniforms -> one Box-Muller pair;
the even s of a pair takes the cosine, the odd one the sine."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; returns the four output words as uint64 arrays < 2^32"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m32, sh = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0          # 32 x 32 -> 64 bits, exact in uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> sh) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _uniform(a, b):
    k = ((a >> np.uint64(5)) << np.uint64(26)) + (b >> np.uint64(6))         # 27 + 26 bits
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def normals(seed, n, first, k):
    """the (n, k) block of rows 0 .. n - 1 and samples first .. first + k - 1 of the stream `seed`"""
    seed, first = int(seed), int(first)
    out = np.empty((n, k), dtype=np.float64)
    if k == 0:
        return out
    i = np.arange(n, dtype=np.uint64)
    for p in range(first >> 1, ((first + k - 1) >> 1) + 1):
        r0, r1, r2, r3 = philox4x32_10((i & np.uint64(MASK), i >> np.uint64(32), p & MASK, p >> 32), (seed & MASK, seed >> 32))
        rad = np.sqrt(-2.0 * np.log(_uniform(r0, r1)))
        th = 6.283185307179586 * _uniform(r2, r3)
        for s, v in ((2 * p, rad * np.cos(th)), (2 * p + 1, rad * np.sin(th))):
            if first <= s < first + k:
                out[:, s - first] = v
    return out


def half_solve(sym, Lsx, B, which):
    """L^-1 B (which = "L") or L^-T B ("Lt") for B of shape (n,) or (n, k): the supernodal sweep over the reference layout (panel s at
    Lsxp[s], nsrow x nscol column-major, rows Lsi[Lsip[s]:Lsip[s + 1]], the first nscol of them the supernode's own columns)"""
    g = (lambda key: sym[key]) if isinstance(sym, dict) else (lambda key: getattr(sym, key))
    Super, Lsip, Lsi, Lsxp = (np.asarray(g(key)) for key in ("Super", "Lsip", "Lsi", "Lsxp"))
    nsuper = int(g("nsuper"))
    X = np.array(B, dtype=np.float64, copy=True)
    one = X.ndim == 1
    if one:
        X = X.reshape(-1, 1)
    if which not in ("L", "Lt"):
        raise ValueError(which)
    for s in (range(nsuper) if which == "L" else range(nsuper - 1, -1, -1)):
        nscol = int(Super[s + 1] - Super[s])
        nsrow = int(Lsip[s + 1] - Lsip[s])
        rows = Lsi[Lsip[s]:Lsip[s + 1]]
        P = Lsx[Lsxp[s]:Lsxp[s] + nsrow * nscol].reshape(nscol, nsrow).T         # nsrow x nscol
        D = np.tril(P[:nscol])
        own, below = rows[:nscol], rows[nscol:]
        if which == "L":
            X[own] = np.linalg.solve(D, X[own])
            X[below] -= P[nscol:] @ X[own]
        else:
            X[own] = np.linalg.solve(D.T, X[own] - P[nscol:].T @ X[below])
    return X[:, 0] if one else X
