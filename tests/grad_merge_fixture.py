"""The numpy statement of gradient accumulation (include/scone_hip.h, "gradient accumulation"): host only.

A sparse row gradient is (ids [n] int64 ascending and distinct, rows [n, d] fp32).  `merge_map` is `scone_grad_merge_map`,
`merge_rows` is `scone_grad_merge_rows`; `merge` is both.  A row one operand has is that row, bit for bit (copied as uint32
words: -0.0 and NaN payloads survive); a row both have is `a + b`, one numpy float32 add, `a` the first operand (numpy keeps
fp32 subnormals and fuses nothing).  ABSENT is the library's 0xFFFFFFFF.
"""

import numpy as np

ABSENT = np.uint32(0xFFFFFFFF)


def is_valid(ids):
    ids = np.asarray(ids, dtype=np.int64)
    return bool((np.diff(ids) > 0).all())


def merge_map(ids_a, ids_b):
    """(ids [n_out] int64, src_a [n_out] uint32, src_b [n_out] uint32, pos_a [n_a] uint32, pos_b [n_b] uint32)."""
    a, b = np.asarray(ids_a, dtype=np.int64), np.asarray(ids_b, dtype=np.int64)
    assert is_valid(a) and is_valid(b), "the contract covers ascending lists of distinct ids only"
    ids = np.union1d(a, b).astype(np.int64)                    # signed order
    pos_a = np.searchsorted(ids, a).astype(np.uint32)
    pos_b = np.searchsorted(ids, b).astype(np.uint32)
    src_a = np.full(len(ids), ABSENT, dtype=np.uint32)
    src_b = np.full(len(ids), ABSENT, dtype=np.uint32)
    src_a[pos_a] = np.arange(len(a), dtype=np.uint32)
    src_b[pos_b] = np.arange(len(b), dtype=np.uint32)
    return ids, src_a, src_b, pos_a, pos_b


def merge_rows(src_a, src_b, rows_a, rows_b):
    """fp32 [n_out, d]."""
    rows_a, rows_b = np.asarray(rows_a, dtype=np.float32), np.asarray(rows_b, dtype=np.float32)
    d = rows_a.shape[1]
    assert rows_b.shape[1] == d
    out = np.zeros((len(src_a), d), dtype=np.uint32)
    has_a, has_b = src_a != ABSENT, src_b != ABSENT
    assert (has_a | has_b).all()
    only_a, only_b, both = has_a & ~has_b, has_b & ~has_a, has_a & has_b
    out[only_a] = rows_a.view(np.uint32)[src_a[only_a]]
    out[only_b] = rows_b.view(np.uint32)[src_b[only_b]]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out[both] = (rows_a[src_a[both]] + rows_b[src_b[both]]).astype(np.float32).view(np.uint32)
    return out.view(np.float32)


def merge(ids_a, rows_a, ids_b, rows_b):
    """(ids, rows) of the sum of the two sparse gradients."""
    ids, src_a, src_b, _, _ = merge_map(ids_a, ids_b)
    return ids, merge_rows(src_a, src_b, rows_a, rows_b)


def merge_dict(ids_a, rows_a, ids_b, rows_b):
    """The same by another road, for the fixture's own test: a dict keyed by id, filled row by row."""
    acc = {}
    for i, r in zip(np.asarray(ids_a).tolist(), np.asarray(rows_a, dtype=np.float32)):
        acc[i] = r.copy()
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i, r in zip(np.asarray(ids_b).tolist(), np.asarray(rows_b, dtype=np.float32)):
            acc[i] = (acc[i] + r).astype(np.float32) if i in acc else r.copy()
    ids = np.array(sorted(acc), dtype=np.int64)
    d = np.asarray(rows_a).shape[1]
    rows = np.stack([acc[i] for i in ids.tolist()]) if len(ids) else np.zeros((0, d), dtype=np.float32)
    return ids, rows.astype(np.float32)


def same_bits(got, want):
    """Equal as uint32 words, except that a NaN matches any NaN (payloads are not part of the contract for a + b)."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))


def edge_rows(n, d, seed):
    """fp32 [n, d] normal values salted with -0.0, +0.0, subnormals, +-inf and NaN."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    if x.size:
        specials = np.array([-0.0, 0.0, 1e-45, -1e-45, 1.1754942e-38, -5.9e-39, np.inf, -np.inf, np.nan, 3.4028235e38, -3.4028235e38],
                            dtype=np.float32)
        at = rng.random(x.shape) < 0.3
        x[at] = rng.choice(specials, size=int(at.sum()))
    return x
