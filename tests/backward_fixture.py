"""The numpy statement of the lookup's backward (include/scone_hip.h, "backward"): host only, parameterised by the chunk C.

A batch is its CSR id lists over the ntok positions (`off [ntok + 1]`, `ids`), in the reference's order.  A reference is
(row, position p, place k in the list of p); the reference stream is the lists back to back, i.e. in (p, k) order.

    K_p   = off[p + 1] - off[p]                         the FULL list length, whatever the handle owns
    c     = fp32(g[p, :]) * (fp32(1) / fp32(K_p))       mean: one rounded reciprocal per position, one rounded product per element
    c     = fp32(g[p, :])                               sum
    order = np.argsort(rows, kind="stable")             the references of a row stay in (p, k) order
    a row's references are cut into chunks of C; a chunk's partial is a = +0; a = a + c in order; a row with one chunk gets
    that partial, a row with several gets acc = +0; acc = acc + partial_j in chunk order

Only references whose row lies in [row_begin, row_end) count; ids outside [0, n_rows) are skipped.  Every operation is a numpy
float32 operation on arrays (a multiply and an add are separate roundings; numpy fuses nothing).
"""

import numpy as np


def references(off, ids, row_begin=0, row_end=None, n_rows=None):
    """(rows [n_refs], positions [n_refs]) of the owned references in (p, k) order, and K [ntok] (full list lengths)."""
    off = np.asarray(off, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    K = np.diff(off)
    pos = np.repeat(np.arange(len(K), dtype=np.int64), K)
    hi = np.iinfo(np.int64).max if row_end is None else int(row_end)
    keep = (ids >= int(row_begin)) & (ids < hi) & (ids >= 0)
    if n_rows is not None:
        keep &= ids < int(n_rows)
    return ids[keep], pos[keep], K


def contributions(g, K, reduce):
    """fp32 [ntok, d]: the contribution every reference of position p makes (rows of positions with K = 0 are never used)."""
    g32 = np.asarray(g).astype(np.float32)
    if reduce == "sum":
        return g32
    assert reduce == "mean"
    w = np.float32(1.0) / np.maximum(K, 1).astype(np.float32)
    return (g32 * w[:, None]).astype(np.float32)


def backward_rows(off, ids, g, reduce, C, row_begin=0, row_end=None, n_rows=None, reverse=False, chunked=True):
    """(row_ids [U] int64 ascending, grad_rows [U, d] fp32) of the contract.  `reverse` walks every row's references backwards
    and `chunked=False` sums a row in one chain: two WRONG models, for the preconditions of the GPU tests."""
    rows, pos, K = references(off, ids, row_begin, row_end, n_rows)
    c = contributions(g, K, reduce)
    d = c.shape[1]
    order = np.argsort(rows, kind="stable")
    srows, spos = rows[order], pos[order]
    row_ids, starts = np.unique(srows, return_index=True)
    ends = np.append(starts[1:], len(srows))
    out = np.zeros((len(row_ids), d), dtype=np.float32)
    step = int(C) if chunked else max(len(srows), 1)
    for u, (b, e) in enumerate(zip(starts.tolist(), ends.tolist())):
        ps = spos[b:e][::-1] if reverse else spos[b:e]
        partials = []
        for j in range(0, len(ps), step):
            a = np.zeros(d, dtype=np.float32)
            for p in ps[j:j + step]:
                a = a + c[p]
            partials.append(a)
        if len(partials) == 1:
            out[u] = partials[0]
        else:
            acc = np.zeros(d, dtype=np.float32)
            for a in partials:
                acc = acc + a
            out[u] = acc
    return row_ids.astype(np.int64), out


def backward_rows_f64(off, ids, g, reduce, row_begin=0, row_end=None, n_rows=None):
    """The same sums in float64 with exact weights, plus what the error bound needs: (row_ids, sums f64 [U, d],
    sum |c| f64 [U, d], references per row [U])."""
    rows, pos, K = references(off, ids, row_begin, row_end, n_rows)
    g64 = np.asarray(g).astype(np.float32).astype(np.float64)
    c = g64 if reduce == "sum" else g64 / np.maximum(K, 1)[:, None]
    row_ids, inv, counts = np.unique(rows, return_inverse=True, return_counts=True)
    sums = np.zeros((len(row_ids), c.shape[1]))
    mags = np.zeros_like(sums)
    np.add.at(sums, inv, c[pos])
    np.add.at(mags, inv, np.abs(c[pos]))
    return row_ids.astype(np.int64), sums, mags, counts


def row_lengths(off, ids, row_begin=0, row_end=None, n_rows=None):
    """(row_ids, references per row)."""
    rows, _, _ = references(off, ids, row_begin, row_end, n_rows)
    return np.unique(rows, return_counts=True)


def positions_with_a_duplicate(off, ids):
    """Number of positions whose list holds some id twice."""
    off = np.asarray(off, dtype=np.int64)
    n = 0
    for p in range(len(off) - 1):
        seg = ids[off[p]:off[p + 1]]
        n += len(np.unique(seg)) < len(seg)
    return n
