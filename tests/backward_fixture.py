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
float32 operation on arrays (a multiply and an add are separate roundings; numpy fuses nothing; fp32 denormals are kept).

The caller's offsets are taken as the header states them (`clamp_offsets`): with total = off[ntok], list p is ids[lo:hi],
lo = off[p] clamped into [0, total], hi = off[p + 1] clamped into [lo, total]; K_p = hi - lo.  Offsets that decrease give lists
that overlap.  For well-formed offsets this is the identity.
"""

import numpy as np


def clamp_offsets(off):
    """(lo [ntok], hi [ntok]): the header's clamp of the caller's offsets (total = off[ntok]; a negative total is refused by
    the library and is no input here)."""
    off = np.asarray(off, dtype=np.int64)
    total = int(off[-1])
    assert total >= 0
    lo = np.clip(off[:-1], 0, total)
    hi = np.minimum(np.maximum(off[1:], lo), total)
    return lo, hi


def references(off, ids, row_begin=0, row_end=None, n_rows=None):
    """(rows [n_refs], positions [n_refs]) of the owned references in (p, k) order, and K [ntok] (full, clamped list lengths)."""
    ids = np.asarray(ids, dtype=np.int64)
    lo, hi = clamp_offsets(off)
    K = hi - lo
    pos = np.repeat(np.arange(len(K), dtype=np.int64), K)
    first = np.cumsum(K) - K                                   # where list p starts in the stream of all lists back to back
    ids = ids[np.repeat(lo - first, K) + np.arange(int(K.sum()), dtype=np.int64)]
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


def flush(x):
    """fp32 denormals -> zero of the same sign (what a flush-to-zero unit makes of them)."""
    x = np.asarray(x, dtype=np.float32)
    tiny = (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny)
    return np.where(tiny, np.copysign(np.float32(0), x), x).astype(np.float32)


def backward_rows(off, ids, g, reduce, C, row_begin=0, row_end=None, n_rows=None, reverse=False, chunked=True,
                  neg_zero_start=False, flush_denormals=False):
    """(row_ids [U] int64 ascending, grad_rows [U, d] fp32) of the contract.  Four WRONG models, for the preconditions of the
    GPU tests: `reverse` walks every row's references backwards, `chunked=False` sums a row in one chain, `neg_zero_start`
    starts a chunk's partial at -0.0 (what is left when the `+0 +` of the first add is dropped: a row whose contributions are all
    -0 comes out -0), `flush_denormals` flushes fp32 denormals to zero in the inputs and results of the products and sums."""
    rows, pos, K = references(off, ids, row_begin, row_end, n_rows)
    ftz = flush if flush_denormals else (lambda x: x)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if flush_denormals and reduce == "mean":
            w = np.float32(1.0) / np.maximum(K, 1).astype(np.float32)
            c = flush(flush(np.asarray(g).astype(np.float32)) * w[:, None])
        else:
            c = ftz(contributions(g, K, reduce))
        return _sum_rows(rows, pos, c, C, reverse, chunked, neg_zero_start, ftz)


def _sum_rows(rows, pos, c, C, reverse, chunked, neg_zero_start, ftz):
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
            a = np.full(d, -0.0 if neg_zero_start else 0.0, dtype=np.float32)
            for p in ps[j:j + step]:
                a = ftz(a + c[p])
            partials.append(a)
        if len(partials) == 1:
            out[u] = partials[0]
        else:
            acc = np.zeros(d, dtype=np.float32)
            for a in partials:
                acc = ftz(acc + a)
            out[u] = acc
    return row_ids.astype(np.int64), out


def backward_rows_short(off, ids, g, reduce, row_begin=0, row_end=None, n_rows=None):
    """backward_rows for batches in which no row has more than two references (asserted), without the per-row loop:
    (+0 + c[p0]) + c[p1], every operation a float32 array operation.  One chunk per row whatever C >= 2 is."""
    rows, pos, K = references(off, ids, row_begin, row_end, n_rows)
    c = contributions(g, K, reduce)
    order = np.argsort(rows, kind="stable")
    srows, spos = rows[order], pos[order]
    row_ids, starts, lens = np.unique(srows, return_index=True, return_counts=True)
    assert len(lens) == 0 or lens.max() <= 2
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out = np.zeros((len(row_ids), c.shape[1]), dtype=np.float32) + c[spos[starts]]
        two = lens == 2
        out[two] = out[two] + c[spos[starts[two] + 1]]
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
