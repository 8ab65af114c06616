"""Inputs and expectations for out-of-range token and position ids, in plain numpy (host only; no HIP code is involved).

Every lookup kernel carries its own copy of one guard: `wte[tok]` / `wpe[pos]` are read only for ids inside `[0, vocab)` /
`[0, n_pos)`; any other id contributes a row of +0.0 and raises bit 0 of the status word.  This module builds the batches that
tests/test_gpu_bad_ids.py sends through every copy of that guard, and what the outcome has to be:

    token term     wte[tok[p]] if 0 <= tok[p] < vocab, else +0.0        (a dense base: base[p], no vocabulary, no check)
    position term  wpe[pos]    if 0 <= pos    < n_pos, else +0.0        (pos: the caller's id, or the place inside the sequence)
    f-gram term    the oracle's id lists on the RAW tokens -- a negative token matches nothing, a token >= vocab still matches
                   every f-gram that contains it (the index knows nothing of wte)
    out            cast((token_term + fg) + position_term), fp32, rounded once; in longest_suffix mode a matched f-gram
                   replaces the token term
    status         bit 0 iff some position of the call has a bad id whose table was given; no other bit

Set-up: the vocabularies of tests/test_gpu_walk_shapes.py (f-grams over the tokens {0, 1, 2}, token 3 in wte and in no f-gram)
and its batches / those of tests/test_gpu_varlen.py, with two more alphabet tokens, `OOV = (4, 67)`, that occur in unigram,
bigram, trigram and 4-gram keys appended to those vocabularies but lie OUTSIDE wte: wte keeps its 4 rows (`VOCAB`), so 4 is
`vocab` and 67 is `vocab + G - 1`.  Tables are quantised on the host (oracle/ref_port.py, bf16_fixture, mxfp4_fixture).

Bad token values: -1, -G, vocab, vocab + G - 1.  Bad position values: -1, -G, n_pos, n_pos + G - 1.  No id is farther than
G = 64 rows outside its table: the GPU tests put wte / wpe in the middle of an allocation with G sentinel rows on either side,
so a kernel that lost its guard reads the sentinel and fails a comparison instead of faulting.

Where the bad ids go (`_placements`), most wanted first, until a tenth of the batch carries one:

  1. the first position of the batch: token -1 (K = 0);
  2. the last one: a position id, or token -G with default positions.  It is the tail i >= T - T % 4 of its sequence and the
     remainder launch of a packed traversal;
  3. a token >= vocab behind a token 0 / 1 in a sequence behind the first: the bigram (a, 4) ends there, so K > 0, the
     neighbour's lists contain it and the paper's lookup matches it; a workgroup that walks several sequences meets it through
     its prefetched token;
  4. the first / last / tail positions of a middle sequence, of the second and of the third one, one position with both ids bad;
  5. random positions over the whole batch, each bad value in turn.

One sequence (`clean_seq`) is kept free of bad ids: the slice launches (finalize, the shard halves) use it to show that ids
OUTSIDE a slice raise nothing.  With default positions the position id cannot be chosen: there the bad ones are the places
i >= n_pos of a wpe shorter than the longest sequence (`positions="short"`).
"""

import collections
import functools
import os
import sys

import numpy as np

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import mxfp4_fixture as MX  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, alphabet, batches, host quantisation)

G = 64                                  # guard rows around wte / wpe on the device = the farthest a bad id may lie outside
VOCAB = WS.VOCAB + 1                    # rows of wte: the tokens 0..3
OOV = (VOCAB, VOCAB + G - 1)            # alphabet tokens that occur in f-gram keys and are >= vocab
BAD_TOKENS = (-1, -G, VOCAB, VOCAB + G - 1)
N_POS = 64                              # rows of wpe with explicit positions
WPE_ROWS = 640                          # rows generated; a case passes the first n_pos of them
MAX_BAD_SHARE = 0.10
MAX_RANDOM = 48
RECTS = {"9x37": (9, 37), "33x3": (33, 3), "7x5": (7, 5), "7x37": (7, 37), "1243x37": (1243, 37)}
PACKED = ("small", "tiny")


def bad_positions(n_pos):
    return (-1, -G, n_pos, n_pos + G - 1)


# ------------------------------------------------------------------ vocabulary and tables
@functools.lru_cache(maxsize=None)
def vocabulary(max_n):
    """(keys, lens) of tests/test_gpu_walk_shapes.py plus f-grams that contain a token >= vocab; row number == id."""
    keys, lens = WS._vocabulary(max_n)
    grams = [(OOV[0],)]
    for t in OOV:
        grams += [(0, t), (1, t), (t, 0), (t, 2), (0, t, 1), (t, 1, 1), (2, 0, t), (1, t, 0, 0), (0, 1, 2, t)]
    grams = [g for g in grams if len(g) <= max_n]
    k2 = np.zeros((len(grams), max_n), dtype=np.uint32)
    l2 = np.zeros(len(grams), dtype=np.uint8)
    for i, g in enumerate(grams):
        k2[i, :len(g)] = g
        l2[i] = len(g)
    return np.concatenate([keys, k2]), np.concatenate([lens, l2])


def stored(table, fmt):
    """What the table format holds, as fp32 (the oracle runs on this)."""
    if fmt == "bf16":
        return BF.stored(table)
    if fmt == "mxfp4":
        return MX.stored(table)
    return WS._stored(table, fmt)


@functools.lru_cache(maxsize=None)
def tables(fmt, d, max_n):
    """(fp32 rows given to the handle, the same rows as the format stores them, wte[VOCAB, d], wpe[WPE_ROWS, d])."""
    rng = np.random.default_rng(29 * d + max_n)
    table = rng.standard_normal((len(vocabulary(max_n)[1]), d)).astype(np.float32)
    wte = rng.standard_normal((VOCAB, d)).astype(np.float32)
    wpe = rng.standard_normal((WPE_ROWS, d)).astype(np.float32)
    return table, stored(table, fmt), wte, wpe


# ------------------------------------------------------------------ batches
@functools.lru_cache(maxsize=None)
def clean_batch(batch, max_n):
    """(tokens [total], cu [n + 1], random position ids [total] in [0, N_POS)), all int64, every id in range."""
    if batch in RECTS:
        B, T = RECTS[batch]
        if WS.SHAPES.get(T) == (B, T):
            tok, pos = WS._batch(max_n, T)[:2]
        else:
            rng = np.random.default_rng(100 * B + T + max_n)
            tok = rng.choice(WS.VOCAB + 1, size=(B, T), p=WS.TOKEN_P).astype(np.int64)
            pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
        return tok.reshape(-1).copy(), np.arange(B + 1, dtype=np.int64) * T, pos.reshape(-1).copy()
    tok, cu, pos = VL._batch(batch)
    return tok.copy(), cu.copy(), pos % N_POS


Scenario = collections.namedtuple(
    "Scenario", "batch max_n positions tok cu pos pid n_pos bad_tok bad_pos clean_seq")
# tok [total]: token ids with the bad ones in place.  pos: the explicit position ids [total] the call is given, or None.
# pid [total]: the position id every token ends up with.  n_pos: rows of wpe.  bad_tok / bad_pos: bool [total].
# clean_seq: (lo, hi) of a sequence without any bad id (None where every sequence has one).


def _tail(lo, hi):
    """A position i >= T - T % 4 of the sequence [lo, hi) (its last one when T % 4 == 0)."""
    T = hi - lo
    return lo + (T - T % 4 if T % 4 else T - 1)


def _rows_of_wpe(positions, longest):
    if positions == "explicit":
        return N_POS
    if positions == "default":
        return max(N_POS, longest)                          # long enough: no default position is out of range
    return longest - (2 if longest <= G else 10)            # "short": the last 2 (10) places of the longest sequence are


Place = collections.namedtuple("Place", "p tok pos")       # position p gets the token id `tok` and / or the position id `pos`


def _placements(tok, seqs, clean, total, n_pos, explicit, seed):
    """Where the bad ids go, most wanted first (the module docstring's order).  `hot` is returned too: a token >= vocab behind a
    token 0 / 1 of its sequence, whose predecessor must keep its token."""
    bt, bp = BAD_TOKENS, bad_positions(n_pos)
    s1, s2, mid = seqs[1], seqs[2], seqs[len(seqs) // 2]
    hot = next((p for lo, hi in seqs[1:] if (lo, hi) != clean
                for p in range(lo + 1, min(hi, total - 1)) if tok[p - 1] in (0, 1)), None)
    assert hot is not None
    places = [
        Place(0, bt[0], None),                              # first of the batch: a negative token, K = 0
        # last of the batch = the tail of the last sequence = the remainder launch of a packed traversal
        Place(total - 1, None, bp[2]) if explicit else Place(total - 1, bt[1], None),
        Place(hot, bt[2], None),                            # the bigram (a, vocab) ends here: K > 0, the paper's lookup matches
        Place(mid[0], None, bp[0]),                         # first of a middle sequence
        Place(mid[1] - 1, bt[1], None),                     # last of it
        Place(s2[0], bt[3], None),                          # first of the third sequence
        Place(s1[1] - 1, None, bp[1]),                      # last of the second
        Place(_tail(*s2), None, bp[3]),                     # tails: i >= T - T % 4
        Place(_tail(*mid), bt[2], None),
        Place(s1[0], bt[3], bp[2]),                         # both ids bad on one position
        Place(_tail(*s1), bt[0], None),
        Place(seqs[-1][0], None, bp[3]),                    # first of the last sequence
    ]
    rng = np.random.default_rng(seed)                       # ... and random positions over the whole batch, each value in turn
    for k, p in enumerate(rng.integers(0, total, size=MAX_RANDOM).tolist()):
        places.append(Place(p, bt[k % 4], None) if k % 2 == 0 else Place(p, None, bp[(k // 2) % 4]))
    return places, hot


@functools.lru_cache(maxsize=None)
def scenario(batch, max_n, positions):
    """positions: "explicit" (caller's ids, bad ones among them), "default" (the place inside the sequence, wpe long enough:
    no bad position) or "short" (default positions and a wpe shorter than the longest sequence)."""
    tok, cu, pos = clean_batch(batch, max_n)
    tok, pos = tok.copy(), pos.copy()
    total = int(cu[-1])
    explicit = positions == "explicit"
    seqs = [(int(cu[s]), int(cu[s + 1])) for s in range(len(cu) - 1) if cu[s + 1] > cu[s]]
    longest = max(hi - lo for lo, hi in seqs)
    default_pid = VL._default_positions(cu)
    n_pos = _rows_of_wpe(positions, longest)
    assert n_pos <= WPE_ROWS and (explicit or longest - 1 < n_pos + G)
    # at most a tenth of the batch carries a bad id, the default positions >= n_pos included
    budget = int(MAX_BAD_SHARE * total) - (0 if explicit else int((default_pid >= n_pos).sum()))
    assert budget >= 3, (batch, positions, budget)
    nxt = len(seqs) // 2 + 1                                # the sequence behind the middle one stays clean
    clean = seqs[nxt] if positions != "short" and nxt < len(seqs) - 1 else None
    places, hot = _placements(tok, seqs, clean, total, n_pos, explicit, seed=7000 + total + max_n)
    bad_tok, bad_pos = np.zeros(total, dtype=bool), np.zeros(total, dtype=bool)
    for p, t, q in places:
        if int((bad_tok | bad_pos).sum()) >= budget:
            break
        taken = bad_tok[p] or bad_pos[p]
        in_clean = clean is not None and clean[0] <= p < clean[1]
        breaks_hot = p == hot - 1 and t is not None         # the token in front of `hot` is half of its bigram
        if taken or in_clean or breaks_hot:
            continue
        if not explicit:
            if t is None:
                continue                                    # a default position cannot be chosen
            q = None
        if t is not None:
            tok[p], bad_tok[p] = t, True
        if q is not None:
            pos[p], bad_pos[p] = q, True
    if explicit:
        pid = pos
    else:
        pid, pos = default_pid, None
        bad_pos = default_pid >= n_pos
    assert np.array_equal(bad_tok, (tok < 0) | (tok >= VOCAB)) and np.array_equal(bad_pos, (pid < 0) | (pid >= n_pos))
    return Scenario(batch, max_n, positions, tok, cu, pos, pid, n_pos, bad_tok, bad_pos, clean)


# ------------------------------------------------------------------ the oracle's f-gram term
@functools.lru_cache(maxsize=None)
def lists(batch, max_n, positions):
    """CSR id lists over the flattened positions on the RAW tokens, every sequence matched on its own: (offsets, ids)."""
    sc = scenario(batch, max_n, positions)
    keys, lens = vocabulary(max_n)
    if batch in RECTS:
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, sc.tok.reshape(RECTS[batch]), max_n))
        return np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    offs, ids, base = [np.zeros(1, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], 0
    for s in range(len(sc.cu) - 1):
        if sc.cu[s + 1] > sc.cu[s]:
            off, i = R.hits_to_csr(R.match_hits(keys, lens, sc.tok[None, sc.cu[s]:sc.cu[s + 1]], max_n))
            offs.append(off[1:] + base)
            ids.append(i)
            base += off[-1]
    return np.concatenate(offs).astype(np.int64), np.concatenate(ids).astype(np.int64)


@functools.lru_cache(maxsize=None)
def suffix_ids(batch, max_n, positions):
    """The paper's lookup: id of the longest f-gram (n >= 2) that ends at the token, -1 where none does; int64 [total]."""
    sc = scenario(batch, max_n, positions)
    f2id = R._key_dict(*vocabulary(max_n))
    out = np.full(len(sc.tok), -1, dtype=np.int64)
    for s in range(len(sc.cu) - 1):
        lo, hi = int(sc.cu[s]), int(sc.cu[s + 1])
        if hi > lo:
            out[lo:hi] = R.paper_lookup(f2id, max_n, sc.tok[lo:hi].tolist())
    return out


def fgram(sc, fmt, d, mode, reduce, rows=None):
    """(fp32 [n, d] f-gram term of the flattened positions `rows` (None: all), bool [n]: it REPLACES the token term)."""
    table = tables(fmt, d, sc.max_n)[1]
    rows = np.arange(len(sc.tok)) if rows is None else np.asarray(rows, dtype=np.int64)
    if mode == "longest_suffix":
        fid = suffix_ids(sc.batch, sc.max_n, sc.positions)[rows]
        off = np.zeros(len(rows) + 1, dtype=np.int64)
        np.cumsum(fid >= 0, out=off[1:])
        return R.embed_numpy(table, off, fid[fid >= 0], "sum"), fid >= 0
    off, ids = lists(sc.batch, sc.max_n, sc.positions)
    # R.embed_numpy reduces every list on its own: run it once per DISTINCT list and deal the rows back (the same values)
    kmax = sc.max_n * (sc.max_n + 1) // 2
    counts = np.diff(off)[rows]
    padded = np.full((len(rows), kmax), -1, dtype=np.int64)
    for k in range(kmax):
        m = counts > k
        padded[m, k] = ids[off[rows[m]] + k]
    uniq, inverse = np.unique(padded, axis=0, return_inverse=True)
    uoff = np.zeros(len(uniq) + 1, dtype=np.int64)
    np.cumsum((uniq >= 0).sum(axis=1), out=uoff[1:])
    return R.embed_numpy(table, uoff, uniq[uniq >= 0], reduce)[inverse.reshape(-1)], np.zeros(len(rows), dtype=bool)


def expected(sc, fmt, d, mode, reduce, wte32=None, wpe32=None, base32=None, rows=None, pid=None):
    """fp32 [n, d]: (token_term + fg) + position_term for the flattened positions `rows` (None: all).  wte32 [VOCAB, d] /
    wpe32 [n_pos, d]: the fp32 upcasts of the tensors the kernel is given (None: the term is +0.0).  base32 [n, d]: a dense base,
    one row per OUTPUT row.  pid [n]: the position id of every output row (None: the scenario's)."""
    rows = np.arange(len(sc.tok)) if rows is None else np.asarray(rows, dtype=np.int64)
    fg, replaces = fgram(sc, fmt, d, mode, reduce, rows)
    zero = np.zeros((1, d), dtype=np.float32)
    if base32 is not None:
        assert wte32 is None and base32.shape == (len(rows), d)
        w = base32
    elif wte32 is not None:
        assert wte32.shape == (VOCAB, d)
        t = sc.tok[rows]
        w = np.concatenate([wte32, zero])[np.where((t >= 0) & (t < VOCAB), t, VOCAB)]       # every bad id: the appended zero row
    else:
        w = zero
    w = np.where(replaces[:, None], np.float32(0), w).astype(np.float32)
    pe = zero
    if wpe32 is not None:
        assert wpe32.shape == (sc.n_pos, d)
        q = sc.pid[rows] if pid is None else np.asarray(pid, dtype=np.int64)
        pe = np.concatenate([wpe32, zero])[np.where((q >= 0) & (q < sc.n_pos), q, sc.n_pos)]
    out = (w + fg) + pe
    assert out.dtype == np.float32
    return out


def status_bit(sc, wte, wpe, rows=None, pid=None):
    """Bit 0 iff a position of the call (`rows`; None: all) has a bad id whose table is given."""
    rows = slice(None) if rows is None else np.asarray(rows, dtype=np.int64)
    bad_pos = sc.bad_pos[rows] if pid is None else (np.asarray(pid) < 0) | (np.asarray(pid) >= sc.n_pos)
    return int((wte and bool(sc.bad_tok[rows].any())) or (wpe and bool(bad_pos.any())))


@functools.lru_cache(maxsize=None)
def selection(batch, max_n, positions, clean_only=False):
    """Flattened positions for `select=`: every bad position and its neighbours plus 100 random ones, shuffled (repeats occur);
    clean_only: positions WITHOUT a bad id only -- the bad tokens of the batch are then all unselected."""
    sc = scenario(batch, max_n, positions)
    total = len(sc.tok)
    bad = np.nonzero(sc.bad_tok | sc.bad_pos)[0]
    rng = np.random.default_rng(900 + total + max_n)
    sel = np.concatenate([bad, np.clip(bad - 1, 0, total - 1), np.clip(bad + 1, 0, total - 1), rng.integers(0, total, size=100)])
    if clean_only:
        sel = sel[~(sc.bad_tok | sc.bad_pos)[sel]]
    rng.shuffle(sel)
    return sel.astype(np.int64)


# ------------------------------------------------------------------ the scenarios the GPU tests may use
def _used():
    out = []
    for max_n in (3, 4):
        for batch in list(RECTS) + list(PACKED):
            kinds = ["explicit", "default"]
            if batch in ("9x37", "1243x37") or batch in PACKED:
                kinds.append("short")               # T = 3 / 5: a wpe shorter than T makes more than a tenth of the ids bad
            out += [(batch, max_n, k) for k in kinds]
    return out


USED = _used()


def used(batch, max_n, positions):
    """The scenario, for the GPU tests: only those tests/test_bad_ids_host.py has checked."""
    assert (batch, max_n, positions) in USED, (batch, max_n, positions)
    return scenario(batch, max_n, positions)
