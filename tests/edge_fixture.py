"""Edge-value inputs of the lookup, in plain numpy: the tables, vocabularies and token streams behind tests/golden/edge.npz
(written by tests/golden/make_golden.py, which also records what the REFERENCE computes from them) and the same tables at any
wider dim for the GPU tests, where the reference does not exist and the oracle stands in for it.

A row is cut into bands of columns, one value class per band; the class of column j is CLASSES[j % 64], so a row of any width
that is a multiple of 64 carries every class in every 64-column stretch (every lane segment of the wave kernels):

  a  integer multiples of 2^-149 below 2^-137: sums exact, quotients subnormal -- the mean's ties live here
  b  +-[2^-127, 2^-120]: quotients on both sides of FLT_MIN
  c  +-3e38 and +-1.5e38: finite values, sums that overflow to +-inf or cancel back, by the ORDER of the sum
  d  literal +inf / -inf / NaN entries among normals, inf + -inf among them
  e  one constant per column (the sum of K of them is exact, so the mean is the constant again) on the fp16 / bf16 rounding
     boundaries: 65504, 65519, 65520, 2^-24, 2^-25, 1.5 * 2^-24, odd multiples of half an fp16 ulp at 1.0 and at 2^-14,
     low-16-bits = 0x8000 bf16 ties with an even and an odd upper half
  f  standard normals: the control
"""

import numpy as np

DIM = 64
CLASSES = "a" * 12 + "b" * 10 + "c" * 10 + "d" * 8 + "e" * 12 + "f" * 12
assert len(CLASSES) == DIM

E_CONSTANTS = np.array([
    65504.0, 65519.0, 65520.0,                       # fp16 max; just below / exactly on the tie to inf
    2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24,         # smallest fp16 subnormal; the tie to zero; the tie between 1 and 2 units
    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,           # fp16 ties at 1.0: even neighbour below / above
    2.0 ** -14 + 2.0 ** -25, 2.0 ** -14 + 3 * 2.0 ** -25,   # the same at the smallest fp16 normal
    1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8,             # bf16 ties (low 16 bits 0x8000): upper half even / odd
], dtype=np.float32)
assert len(E_CONSTANTS) == CLASSES.count("e")


def band(name, d=DIM):
    """Column indices of one band in a row of width d."""
    return np.asarray([j for j in range(d) if CLASSES[j % DIM] == name], dtype=np.int64)


def vocabulary(max_n):
    """(keys[N, max_n] uint32, lens[N] uint8), row number == f-gram id.  max_n = 3: f-grams over the tokens {0, 1, 2};
    max_n = 4: over {0, 1} plus a token 2 that is in no f-gram.  Some f-grams are left out so that every list length
    K = 0 .. max_n (max_n + 1) / 2 occurs in streams(); every f-gram over {0, 1} that is not listed below is kept, so runs
    of 0s and 1s give the full cover (K = 6 resp. 10)."""
    import itertools
    grams = []
    if max_n == 3:
        left_out = {(0, 0, 1), (1, 1), (2,), (2, 2), (0, 2), (2, 2, 2), (2, 2, 0), (2, 2, 1), (0, 2, 2), (1, 2, 2), (2, 0, 2),
                    (2, 1, 2), (0, 2, 0), (1, 2, 1), (2, 1, 1)}
        alphabet = (0, 1, 2)
    else:
        assert max_n == 4
        left_out = {(0, 1, 1), (1, 0, 0, 1), (1, 1, 1, 1), (1, 0, 1, 0)}
        alphabet = (0, 1)
    for n in range(1, max_n + 1):
        for g in itertools.product(alphabet, repeat=n):
            if g not in left_out:
                grams.append(g)
    keys = np.zeros((len(grams), max_n), dtype=np.uint32)
    lens = np.zeros(len(grams), dtype=np.uint8)
    for i, g in enumerate(grams):
        keys[i, :len(g)] = g
        lens[i] = len(g)
    return keys, lens


STREAM_SHAPES = ((1, 1), (1, 2), (2, 3), (3, 7), (2, 33), (4, 64))     # T below max_n, T % 4 != 0, and two ordinary ones


def streams(max_n, seed=0):
    """Token batches [B, T] over {0, 1, 2}: mostly runs of 0 / 1 (full covers), token 2 sprinkled in (short lists, K = 0)."""
    rng = np.random.default_rng(1000 * max_n + seed)
    out = []
    for B, T in STREAM_SHAPES:
        tok = rng.choice(3, size=(B, T), p=[0.46, 0.46, 0.08]).astype(np.int64)
        if T >= 16:
            tok[0, :12] = np.asarray([0, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 1])[:12]
            tok[-1, -6:] = 2                                     # a run without any f-gram
            tok[1, 4:4 + T // 3] = 0                             # a run of full covers at either max_n
        out.append(tok)
    return out


def table(n_rows, d=DIM, seed=0):
    """The fp32 table [n_rows, d]; d a multiple of 4 (columns beyond the last whole 64 just continue the pattern)."""
    rng = np.random.default_rng(77 + seed)
    t = np.zeros((n_rows, d), dtype=np.float32)
    cls = np.asarray([CLASSES[j % DIM] for j in range(d)])
    for j in range(d):
        c = cls[j]
        if c == "a":
            col = (rng.integers(1, 2 ** 12, size=n_rows) * 2.0 ** -149).astype(np.float32)
        elif c == "b":
            col = (rng.choice([-1.0, 1.0], size=n_rows) * (1.0 + rng.random(n_rows)) * 2.0 ** rng.integers(-127, -120, size=n_rows)
                   ).astype(np.float32)
        elif c == "c":
            col = rng.choice(np.asarray([3e38, -3e38, 1.5e38, -1.5e38], dtype=np.float32), size=n_rows, p=[0.3, 0.3, 0.2, 0.2])
        elif c == "d":
            col = rng.standard_normal(n_rows).astype(np.float32)
            k = (j % DIM) - CLASSES.index("d")
            if k == 0:
                col[rng.integers(0, n_rows, size=max(1, n_rows // 8))] = np.inf
            elif k == 1:
                col[rng.integers(0, n_rows, size=max(1, n_rows // 8))] = -np.inf
            elif k == 2:
                col[rng.integers(0, n_rows, size=max(1, n_rows // 8))] = np.nan
            else:
                u = rng.random(n_rows)
                col[u < 0.15] = np.inf
                col[(u >= 0.15) & (u < 0.30)] = -np.inf
                col[(u >= 0.30) & (u < 0.34)] = np.nan
        elif c == "e":
            col = np.full(n_rows, E_CONSTANTS[(j % DIM) - CLASSES.index("e")], dtype=np.float32)
        else:
            col = rng.standard_normal(n_rows).astype(np.float32)
        t[:, j] = col
    return t


def wte_wpe(vocab, n_pos, d=DIM, seed=0):
    """Token and position embedding tables holding -0.0, +-inf, +-65504 and ordinary values, so that (wte + mean) + wpe is
    exercised at the edges of the output range too.  Row 0 of each is all ordinary values."""
    rng = np.random.default_rng(991 + seed)
    pool = np.asarray([-0.0, 0.0, np.inf, -np.inf, 65504.0, -65504.0], dtype=np.float32)

    def one(rows):
        x = rng.standard_normal((rows, d)).astype(np.float32)
        u = rng.random((rows, d))
        pick = pool[rng.integers(0, len(pool), size=(rows, d))]
        x = np.where(u < 0.3, pick, x).astype(np.float32)
        x[0] = rng.standard_normal(d).astype(np.float32)
        return x

    return one(vocab), one(n_pos)


def same_bits(got, want):
    """The comparison of every edge test: the NaN positions are equal and every other element has equal bits (sign of zero and
    of infinity included; NaN payloads are not compared).  Works on float16 / float32 arrays and on bf16 passed as uint16
    bit patterns (is_bf16_bits=True is implied by dtype uint16)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.uint16:                                  # bf16 bits
        gn = ((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)
        wn = ((want & 0x7F80) == 0x7F80) & ((want & 0x007F) != 0)
        return bool(np.array_equal(gn, wn) and np.array_equal(got[~gn], want[~wn]))
    gn, wn = np.isnan(got), np.isnan(want)
    view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(view)[~gn], want.view(view)[~wn]))


def first_difference(got, want):
    """A short description of the first differing element (for assertion messages)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} vs {want.shape}"
    g, w = got.astype(np.float64) if got.dtype != np.uint16 else got, want.astype(np.float64) if want.dtype != np.uint16 else want
    if got.dtype == np.uint16:
        bad = got != want
    else:
        view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
        bad = (got.view(view) != want.view(view)) & ~(np.isnan(got) & np.isnan(want))
    idx = np.argwhere(bad)
    if len(idx) == 0:
        return "no difference"
    i = tuple(idx[0])
    cols = np.unique(idx[:, -1] % DIM)
    return (f"{len(idx)} of {bad.size} differ; first at {i}: got {g[i]!r} want {w[i]!r}; "
            f"bands {''.join(sorted(set(CLASSES[c] for c in cols)))}")
