"""The contracts of `scone_grad_sqnorm` and `scone_grad_ctl_set` (include/scone_hip.h, "gradient norm, clipping and skipped
steps") in numpy float64, written from the header alone: loops over lanes, tiles and threads in the order the header states.
numpy's float64 `+`, `*`, `/` and `sqrt` are IEEE and correctly rounded, one rounding each; `x * x` of a widened fp32 is exact.
The only vectorisation is ACROSS rows (every row is independent), never along a sum.
"""

import numpy as np

LANES, TILE, THREADS = 64, 1024, 256


def row_sq(g):
    """Q_r of every row of `g` (fp32 [n, d]): lane (j / 4) % 64, ascending j, then the butterfly s = 32 .. 1."""
    g = np.asarray(g, dtype=np.float32)
    n, d = g.shape
    x = g.astype(np.float64)
    a = np.zeros((n, LANES), dtype=np.float64)                     # +0.0
    with np.errstate(all="ignore"):
        for j in range(d):
            lane = (j // 4) % LANES
            a[:, lane] = a[:, lane] + x[:, j] * x[:, j]
        partner = np.arange(LANES)
        for s in (32, 16, 8, 4, 2, 1):
            a = a + a[:, partner ^ s]                              # all lanes at once
    return a[:, 0].copy()


def tree(b):
    """b_t = b_t + b_(t + s) for t < s, s = 128 .. 1; the sum is b_0."""
    b = np.array(b, dtype=np.float64)
    assert b.shape == (THREADS,)
    with np.errstate(all="ignore"):
        s = THREADS // 2
        while s >= 1:
            for t in range(s):
                b[t] = b[t] + b[t + s]
            s //= 2
    return b[0]


def tile_sq(q):
    """P_k of every tile of the row sums `q` ([n] float64): thread t adds Q_(1024k + t + 256i), i = 0 .. 3, in range."""
    q = np.asarray(q, dtype=np.float64)
    n = len(q)
    tiles = (n + TILE - 1) // TILE
    p = np.zeros(tiles, dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(tiles):
            b = np.zeros(THREADS, dtype=np.float64)
            for t in range(THREADS):
                for i in range(TILE // THREADS):
                    r = TILE * k + t + THREADS * i
                    if r < n:
                        b[t] = b[t] + q[r]
            p[k] = tree(b)
    return p


def total_sq(p):
    """The total of the tile sums: thread t adds P_(t + 256i) in ascending i, then the tree.  No tile: +0.0."""
    p = np.asarray(p, dtype=np.float64)
    b = np.zeros(THREADS, dtype=np.float64)
    with np.errstate(all="ignore"):
        for t in range(THREADS):
            for k in range(t, len(p), THREADS):
                b[t] = b[t] + p[k]
    return tree(b)


def sqnorm(g):
    """(total, Q [n], P [ceil(n / 1024)]) of fp32 `g` [n, d]."""
    q = row_sq(g)
    p = tile_sq(q)
    return total_sq(p), q, p


def ctl(terms, grad_scale=1.0, max_norm=np.inf, skip_nonfinite=False):
    """The five fields of the control block."""
    with np.errstate(all="ignore"):
        total = np.float64(0.0)
        for x in terms:
            total = total + np.float64(x)
        norm64 = np.sqrt(total) * np.abs(np.float64(grad_scale))
        c = np.float64(max_norm) / (norm64 + np.float64(1e-6))
        coef = np.float32(c) if c < 1.0 else np.float32(1.0)       # a NaN compares false
        norm = np.float32(norm64)
    return {"sqnorm": total, "norm": norm, "coef": coef, "skip": int(bool(skip_nonfinite) and not np.isfinite(total)), "reserved": 0}


def scratch_doubles(n):
    return n + (n + TILE - 1) // TILE


def value_mix(n, d, seed=None):
    """fp32 [n, d]: magnitudes 2^-70 .. 2^60 with random mantissas and both signs; about 1 % subnormals; and, in every eighth
    row, about 2 % of values between 1.5e38 and 3e38 (their squares overflow fp32 and dominate the total, so the ORDER of the
    tile and total sums shows in it; the other rows show the order inside a row).  Element [0, 0] is 3e38 itself."""
    rng = np.random.default_rng(1000 * n + d if seed is None else seed)
    mant = 1.0 + rng.random((n, d))
    expo = rng.integers(-70, 61, size=(n, d))
    sign = np.where(rng.random((n, d)) < 0.5, -1.0, 1.0)
    g = (sign * mant * np.exp2(expo.astype(np.float64))).astype(np.float32)
    sub = rng.random((n, d)) < 0.01
    g[sub] = (sign[sub] * rng.integers(1, 1 << 23, size=int(sub.sum())) * 2.0 ** -149).astype(np.float32)
    huge = (rng.random((n, d)) < 0.02) & ((np.arange(n) % 8) == 0)[:, None]
    g[huge] = (sign[huge] * 3e38 * (0.5 + 0.5 * rng.random(int(huge.sum())))).astype(np.float32)
    if n and d:
        g[0, 0] = np.float32(3e38)
    return g


def bits64(x):
    return np.asarray(x, dtype=np.float64).reshape(-1).view(np.uint64)
