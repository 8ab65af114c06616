"""The contract of `scone_embed_rows` (include/scone_hip.h, "the fused lookup over a batch's LIVE rows") restated on the host, in
numpy, from oracle/ref_port.py alone: scatter the widened live rows into a zero [N, d] array at their ids and look the batch up
in that array with the oracle.  An id that is not listed simply leaves its dense row zero: it adds +0.0 and stays in K.

`wrong_model_drops_unlisted` is deliberately NOT the contract: it takes unlisted ids out of the lists, so K shrinks with them.
The tests use it to show that their unlisted-id batch can tell the two apart.
"""

import numpy as np

from oracle import ref_port as R


def batch(max_n, B, T, seed=0):
    """(keys, lens, tok [B, T] int64): a vocabulary of tests/test_gpu_walk_shapes.py and a batch drawn as its batches are."""
    import test_gpu_walk_shapes as WS
    keys, lens = WS._vocabulary(max_n)
    rng = np.random.default_rng(7000 + 100 * B + T + max_n + 1000003 * seed)
    return keys, lens, rng.choice(WS.VOCAB + 1, size=(B, T), p=WS.TOKEN_P).astype(np.int64)


def unlisted(live):
    """The live ids with every third, the first and the last taken out (the unlisted-id tests)."""
    keep = np.ones(len(live), dtype=bool)
    keep[::3] = False
    keep[0] = keep[-1] = False
    return live[keep]


def widen(rows_t):
    """fp32 numpy values of a torch fp32 / fp16 / bf16 tensor (exact)."""
    return rows_t.detach().float().cpu().numpy()


def dense(n_rows, row_ids, rows32):
    """Zero [N, d] fp32 with rows32[u] at row_ids[u]."""
    row_ids = np.asarray(row_ids, dtype=np.int64)
    out = np.zeros((int(n_rows), rows32.shape[1]), dtype=np.float32)
    if row_ids.size:
        out[row_ids] = rows32
    return out


def sequences(tok, cu=None):
    """The batch as a list of 1-D token arrays: the rows of a rectangle, or the sequences of a packed stream."""
    tok = np.asarray(tok)
    if cu is None:
        return [row for row in tok.reshape(-1, tok.shape[-1])]
    cu = np.asarray(cu, dtype=np.int64)
    return [tok[cu[s]:cu[s + 1]] for s in range(len(cu) - 1)]


def lists(keys, lens, max_n, tok, cu=None):
    """CSR id lists (offsets [ntok + 1], ids) of the batch in the reference's order; no window crosses a sequence."""
    if cu is None:
        tok = np.asarray(tok, dtype=np.int64)
        return R.hits_to_csr(R.match_hits(keys, lens, tok.reshape(-1, tok.shape[-1]), max_n))
    offs, ids, base = [np.zeros(1, dtype=np.int64)], [], 0
    for seq in sequences(tok, cu):
        if len(seq) == 0:
            continue
        off, i = R.hits_to_csr(R.match_hits(keys, lens, np.asarray(seq, dtype=np.int64)[None, :], max_n))
        offs.append(off[1:] + base)
        ids.append(i)
        base += int(off[-1])
    return np.concatenate(offs), (np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64))


def paper_lists(keys, lens, max_n, tok, cu=None):
    """CSR lists of lookup_mode longest_suffix: zero or one id per position (what a backward plan of such a handle holds)."""
    f2id = R._key_dict(keys, lens)
    hit = []
    for seq in sequences(tok, cu):
        hit += R.paper_lookup(f2id, max_n, np.asarray(seq, dtype=np.int64).tolist())
    hit = np.asarray(hit, dtype=np.int64).reshape(-1)
    off = np.zeros(len(hit) + 1, dtype=np.int64)
    np.cumsum(hit >= 0, out=off[1:])
    return off, hit[hit >= 0]


def default_positions(tok, cu=None):
    return np.concatenate([np.arange(len(s)) for s in sequences(tok, cu)] or [np.zeros(0, dtype=np.int64)])


def fgram(keys, lens, max_n, tok, cu, table32, mode, reduce):
    """The f-gram part, fp32 [ntok, d]: cover -> the reduced rows; longest_suffix -> (rows, mask of matched tokens)."""
    if mode == "cover":
        off, ids = lists(keys, lens, max_n, tok, cu)
        return R.embed_numpy(table32, off, ids, reduce)
    f2id = R._key_dict(keys, lens)
    rows, matched = [], []
    for seq in sequences(tok, cu):
        if len(seq) == 0:
            continue
        seq = np.asarray(seq, dtype=np.int64)
        rows.append(R.paper_embed(f2id, max_n, seq[None, :], table32)[0])
        matched.append(np.asarray(R.paper_lookup(f2id, max_n, seq.tolist())) >= 0)
    return np.concatenate(rows), np.concatenate(matched)


def combine(fg, mode, base32, wpe32, pid):
    """(base + fg) + wpe[pos] in fp32, as tests/test_gpu_embed_base.py::_combine; base32 / wpe32 None: the term is omitted
    (the kernel adds a row of +0.0)."""
    if mode == "cover":
        e = fg if base32 is None else base32 + fg
        if base32 is None:
            e = np.float32(0) + e
    else:
        rows, matched = fg
        b = np.zeros_like(rows) if base32 is None else base32
        e = np.float32(0) + np.where(matched[:, None], rows, b)
    if wpe32 is None:
        return (e + np.float32(0)).astype(np.float32)
    return (e + wpe32[np.asarray(pid).reshape(-1)]).astype(np.float32)


def expected(keys, lens, max_n, n_rows, tok, cu, row_ids, rows32, mode, reduce, base32=None, wpe32=None, pid=None):
    """fp32 [ntok, d]: what scone_embed_rows writes before its one rounding to the output type."""
    fg = fgram(keys, lens, max_n, tok, cu, dense(n_rows, row_ids, rows32), mode, reduce)
    if wpe32 is not None and pid is None:
        pid = default_positions(tok, cu)
    return combine(fg, mode, base32, wpe32, pid)


def wrong_model_drops_unlisted(keys, lens, max_n, n_rows, tok, cu, row_ids, rows32, reduce, base32=None, wpe32=None, pid=None):
    """NOT the contract (cover mode): unlisted ids are taken out of the lists, so the mean divides by the listed hits only."""
    off, ids = lists(keys, lens, max_n, tok, cu)
    listed = np.isin(ids, np.asarray(row_ids, dtype=np.int64))
    seg = np.repeat(np.arange(len(off) - 1), np.diff(off))
    k = np.bincount(seg[listed], minlength=len(off) - 1)
    off2 = np.zeros(len(off), dtype=np.int64)
    np.cumsum(k, out=off2[1:])
    fg = R.embed_numpy(dense(n_rows, row_ids, rows32), off2, ids[listed], reduce)
    if wpe32 is not None and pid is None:
        pid = default_positions(tok, cu)
    return combine(fg, "cover", base32, wpe32, pid)
