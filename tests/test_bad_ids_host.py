"""CPU: the batches of tests/bad_ids_fixture.py do what tests/test_gpu_bad_ids.py relies on, by the oracle alone.

For every scenario the GPU tests may use (`bad_ids_fixture.USED`): a bad token sits on a position with K > 0 and on one with
K = 0; a token >= vocab lies inside a matched f-gram that also covers a neighbouring position, and the paper's lookup matches on
a position with a bad token; bad position ids sit on tokens with good token ids and the reverse; at most a tenth of the
positions carry a bad id (the rest is what the isolation check checks); no id is farther than G rows outside its table; the
first and the last position of the batch, a later sequence, the first and the last position of a sequence and a tail
position i >= T - T % 4 carry one (in every batch, 7 x 5 included), and one sequence carries none.
Over all scenarios every bad value (-1, -G, vocab, vocab + G - 1; -1, -G, n_pos, n_pos + G - 1) occurs.  The expectation
itself is checked against `oracle.ref_port.combine` on tables with one zero row appended (this file runs without a GPU).
"""

import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bad_ids_fixture as BI  # noqa: E402


def _seq_of(sc, p):
    s = int(np.searchsorted(sc.cu, p, side="right")) - 1
    return int(sc.cu[s]), int(sc.cu[s + 1])


def _is_tail(sc, p):
    """Position p is one of the last T % 4 of its sequence: i >= T - T % 4 (a wave group that is only partly filled)."""
    lo, hi = _seq_of(sc, p)
    T = hi - lo
    return p - lo >= T - T % 4


@pytest.mark.parametrize("batch,max_n,positions", BI.USED, ids=["-".join(str(x) for x in u) for u in BI.USED])
def test_scenario_meets_what_the_gpu_tests_rely_on(batch, max_n, positions):
    sc = BI.used(batch, max_n, positions)
    total = len(sc.tok)
    assert total == int(sc.cu[-1]) and sc.pid.shape == (total,)
    off, _ = BI.lists(batch, max_n, positions)
    K = np.diff(off)
    assert K.shape == (total,)
    # bad tokens on K > 0 and on K = 0
    assert (K[sc.bad_tok] > 0).any() and (K[sc.bad_tok] == 0).any()
    # a token >= vocab inside a matched f-gram of length >= 2: it covers a neighbouring position too
    f2id = R._key_dict(*BI.vocabulary(max_n))
    covered = False
    for p in np.nonzero(sc.tok >= BI.VOCAB)[0].tolist():
        lo, hi = _seq_of(sc, p)
        for n in range(2, max_n + 1):
            for s in range(max(lo, p - n + 1), min(p, hi - n) + 1):
                covered = covered or tuple(int(x) for x in sc.tok[s:s + n]) in f2id
    assert covered
    # ... and the paper's lookup matches on a bad token: the f-gram row replaces the (absent) token row, the bit is still raised
    assert (BI.suffix_ids(batch, max_n, positions)[sc.bad_tok] >= 0).any()
    assert (BI.suffix_ids(batch, max_n, positions)[sc.bad_tok] < 0).any()
    # bad position ids on good tokens and the reverse
    if positions != "default":
        assert (sc.bad_pos & ~sc.bad_tok).any()
    else:
        assert not sc.bad_pos.any()
    assert (sc.bad_tok & ~sc.bad_pos).any()
    # the isolation check has something to check
    n_bad = int((sc.bad_tok | sc.bad_pos).sum())
    assert 3 <= n_bad <= BI.MAX_BAD_SHARE * total, (n_bad, total)
    # no id farther than G rows outside its table
    assert sc.tok.min() >= -BI.G and sc.tok.max() <= BI.VOCAB + BI.G - 1
    assert sc.pid.min() >= -BI.G and sc.pid.max() <= sc.n_pos + BI.G - 1
    assert set(sc.tok[sc.bad_tok].tolist()) <= set(BI.BAD_TOKENS) and not (sc.tok[~sc.bad_tok] >= BI.VOCAB).any()
    if positions == "explicit":
        assert set(sc.pid[sc.bad_pos].tolist()) <= set(BI.bad_positions(sc.n_pos))
        assert np.array_equal(sc.pos, sc.pid)
    else:
        assert sc.pos is None
        assert np.array_equal(sc.pid, np.concatenate([np.arange(sc.cu[s + 1] - sc.cu[s]) for s in range(len(sc.cu) - 1)]))
    # where they are
    bad = sc.bad_tok | sc.bad_pos
    assert bad[0] and bad[total - 1]
    first_lo, first_hi = _seq_of(sc, 0)
    assert bad[first_hi:].any()                                   # a sequence other than the first
    where = np.nonzero(bad)[0].tolist()
    tails = [p for p in where if _is_tail(sc, p)]
    firsts = [p for p in where if p == _seq_of(sc, p)[0]]
    lasts = [p for p in where if p + 1 == _seq_of(sc, p)[1]]
    assert tails and firsts and lasts                             # in every batch, the 35 tokens of 7 x 5 included
    if n_bad >= 6:                                                # (7 x 5 has room for three bad ids)
        assert len(firsts) >= 2 and len(tails) >= 2 and len(lasts) >= 2
    if positions != "short":
        lo, hi = sc.clean_seq
        assert 0 < lo < hi and not bad[lo:hi].any() and bad[:lo].any()
    else:
        assert sc.clean_seq is None


def test_every_bad_value_occurs():
    toks, poss = set(), set()
    for u in BI.USED:
        sc = BI.used(*u)
        toks |= set(sc.tok[sc.bad_tok].tolist())
        if u[2] == "explicit":
            poss |= {("lo", int(v)) if v < 0 else ("hi", int(v - sc.n_pos)) for v in sc.pid[sc.bad_pos].tolist()}
    assert toks == set(BI.BAD_TOKENS)
    assert poss == {("lo", -1), ("lo", -BI.G), ("hi", 0), ("hi", BI.G - 1)}
    for max_n in (3, 4):
        keys, lens = BI.vocabulary(max_n)
        for t in BI.OOV:                                           # two alphabet tokens >= vocab in bigram and trigram keys
            assert t >= BI.VOCAB
            for n in (2, 3):
                assert ((keys[lens == n] == t).any(axis=1)).any()


@pytest.mark.parametrize("batch,positions", [("9x37", "explicit"), ("9x37", "short"), ("tiny", "explicit"), ("small", "short")])
@pytest.mark.parametrize("max_n", [3, 4])
def test_expectation_equals_the_oracles_combine_with_a_zero_row_appended(batch, max_n, positions):
    """`expected` (cover mode) against the straight road: R.embed_numpy on the full lists, then R.combine with every bad id mapped
    to a zero row appended to wte / wpe."""
    sc = BI.used(batch, max_n, positions)
    fmt, d = "int8", 64
    _, stored, wte, wpe = BI.tables(fmt, d, max_n)
    wpe = wpe[:sc.n_pos]
    off, ids = BI.lists(batch, max_n, positions)
    for reduce in ("mean", "sum"):
        fg = R.embed_numpy(stored, off, ids, reduce)
        zero = np.zeros((1, d), dtype=np.float32)
        t = np.where(sc.bad_tok, BI.VOCAB, sc.tok)
        q = np.where(sc.bad_pos, sc.n_pos, sc.pid)
        want = R.combine(torch.from_numpy(t[None]), torch.from_numpy(fg[None]), torch.from_numpy(np.concatenate([wte, zero])),
                         torch.from_numpy(np.concatenate([wpe, zero])), position_ids=torch.from_numpy(q[None])).numpy()[0]
        got = BI.expected(sc, fmt, d, "cover", reduce, wte32=wte, wpe32=wpe)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        rows = BI.selection(batch, max_n, positions)
        assert np.array_equal(BI.expected(sc, fmt, d, "cover", reduce, wte32=wte, wpe32=wpe, rows=rows), want[rows])
    # the paper's lookup: the f-gram row where one ends at the token, the token row elsewhere, zeros for a bad token
    got = BI.expected(sc, fmt, d, "longest_suffix", "mean", wte32=wte, wpe32=wpe)
    fid = BI.suffix_ids(batch, max_n, positions)
    for p in np.nonzero(sc.bad_tok | sc.bad_pos)[0].tolist() + [1, 2, 3]:
        e = stored[fid[p]] if fid[p] >= 0 else (zero[0] if sc.bad_tok[p] else wte[sc.tok[p]])
        pe = zero[0] if sc.bad_pos[p] else wpe[sc.pid[p]]
        assert np.array_equal(got[p], (np.float32(0) + e) + pe)


def test_status_bit_and_selections():
    sc = BI.used("9x37", 3, "explicit")
    assert BI.status_bit(sc, True, True) == 1 and BI.status_bit(sc, False, False) == 0
    assert BI.status_bit(sc, True, False) == 1 and BI.status_bit(sc, False, True) == 1
    lo, hi = sc.clean_seq
    assert BI.status_bit(sc, True, True, rows=np.arange(lo, hi)) == 0
    sel = BI.selection("9x37", 3, "explicit")
    assert len(np.unique(sel)) < len(sel) and (np.diff(sel) < 0).any() and (sc.bad_tok[sel]).any() and sc.bad_pos[sel].any()
    clean = BI.selection("9x37", 3, "explicit", clean_only=True)
    assert len(clean) >= 100 and BI.status_bit(sc, True, True, rows=clean) == 0 and sc.bad_tok.any()
    dflt = BI.used("9x37", 3, "default")
    assert BI.status_bit(dflt, False, True) == 0 and BI.status_bit(dflt, True, True) == 1
