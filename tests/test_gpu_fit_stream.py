"""GPU: the streaming fit (scone_fit_state; FitState, NGramExtractor.fit_gpu(chunk_tokens=...)) gives the reference's f-gram
list -- same keys, same ids, same counts -- for every chunking, growth history, shard order and merge order.

References: the golden fit results captured from the reference (tests/golden/match.npz), the host `fit` (a Counter), and the
one-shot `scone_fit`.  Everything is exact: no tolerance anywhere.  Run with ``-m gpu`` on an MI355X.
"""

import ctypes as C
import functools
import os
from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SETTINGS = ((3, 2, 50_000), (4, 1, 20_000), (2, 5, 10**9))           # (max_n, min_freq, max_f_grams)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ------------------------------------------------------------------ shared references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def _corpus():
    """The 702-text Zipf corpus of test_fit_gpu_large_corpus_vs_host_fit."""
    from scone_amd import synthetic as S
    rng = np.random.default_rng(4)
    cdf = S.zipf_cdf(5000)
    return tuple(tuple(S.zipf_tokens(rng, cdf, int(rng.integers(1, 600))).tolist()) for _ in range(700)) + ((), (3,))


@functools.lru_cache(maxsize=None)
def _counter(max_n, lo=0, hi=None):
    """The reference's fit loop over texts [lo, hi): (Counter in insertion order, text of every n-gram's first insertion)."""
    from scone_amd import NGramExtractor
    ex = NGramExtractor(max_n=max_n)
    counter, first_text = Counter(), {}
    for t, text in enumerate(_corpus()[lo:hi]):
        grams = ex.extract_all_n_grams(list(text))
        for g in grams:
            first_text.setdefault(g, t)
        counter.update(grams)
    return counter, first_text


def _as_arrays(pairs, max_n):
    keys = np.zeros((len(pairs), max_n), dtype=np.uint32)
    lens = np.zeros(len(pairs), dtype=np.uint8)
    for i, (g, _) in enumerate(pairs):
        keys[i, :len(g)] = g
        lens[i] = len(g)
    return keys, lens, np.array([c for _, c in pairs], dtype=np.uint64)


def _host_fit(counter, max_n, min_freq, max_f):
    """NGramExtractor.fit's list (n_gram_extractor.py:91-99) with its counts."""
    return _as_arrays([(g, c) for g, c in counter.most_common(max_f) if c >= min_freq], max_n)


def _assert_result(got, want, what):
    keys, lens, counts = got[:3]
    assert np.array_equal(lens, want[1]), what
    assert np.array_equal(keys, want[0]), what
    assert counts.dtype == np.uint64 and np.array_equal(counts, want[2]), what


def _chunks(texts, chunk_tokens):
    from scone_amd import NGramExtractor
    return list(NGramExtractor._chunks(texts, chunk_tokens))


def _sorted_export(state):
    keys, lens, counts, first = state.export()
    order = np.lexsort(tuple(keys[:, j] for j in range(keys.shape[1] - 1, -1, -1)) + (lens,))
    return keys[order], lens[order], counts[order], first[order]


def _assert_same_export(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _pow2_at_least(x, floor=1024):
    p = floor
    while p < x:
        p <<= 1
    return p


# ------------------------------------------------------------------ 1. pinned by the reference
@pytest.mark.parametrize("chunk_tokens", [1, 7, 10**9])
def test_stream_matches_reference_order_on_every_golden_corpus(golden_dir, chunk_tokens):
    from scone_amd import NGramExtractor
    z = np.load(os.path.join(golden_dir, "match.npz"))
    seen_max_n = set()
    for c in z["cases"]:
        flat, cl = z[f"{c}_corpus_flat"], z[f"{c}_corpus_lens"]
        min_freq, max_f = (int(x) for x in z[f"{c}_fit_args"])
        corpus, p = [], 0
        for n in cl:
            corpus.append(flat[p:p + n].tolist())
            p += n
        max_n = int(z[f"{c}_max_n"])
        seen_max_n.add(max_n)
        ex = NGramExtractor(max_n=max_n, min_freq=min_freq, max_f_grams=max_f).fit_gpu(iter(corpus), verbose=False,
                                                                                      chunk_tokens=chunk_tokens)
        keys, lens = ex.key_arrays()
        assert np.array_equal(lens, z[f"{c}_lens"]), c
        assert np.array_equal(keys, z[f"{c}_keys"]), c
        assert ex.counts.dtype == np.uint64 and len(ex.counts) == len(lens)
    assert seen_max_n == {1, 2, 3, 4}


# ------------------------------------------------------------------ 2. chunk invariance at size
@pytest.mark.parametrize("max_n,min_freq,max_f", SETTINGS)
def test_chunk_invariance_on_the_zipf_corpus(max_n, min_freq, max_f):
    from scone_amd import NGramExtractor
    corpus = _corpus()
    counter, first_text = _counter(max_n)
    want = _host_fit(counter, max_n, min_freq, max_f)

    # the case that breaks a wrong seq_base: equal counts whose first insertions lie in different chunks
    sizes = [off.size - 1 for _, off in _chunks(corpus, 4096)]
    chunk_of = np.repeat(np.arange(len(sizes)), sizes)
    kept = [g for g, c in counter.most_common(max_f) if c >= min_freq]
    ties = sum(1 for a, b in zip(kept, kept[1:])
               if counter[a] == counter[b] and chunk_of[first_text[a]] != chunk_of[first_text[b]])
    assert ties >= 100, ties

    one = NGramExtractor(max_n=max_n, min_freq=min_freq, max_f_grams=max_f).fit_gpu(corpus, verbose=False)
    assert np.array_equal(one.key_arrays()[0], want[0]) and np.array_equal(one.counts.astype(np.uint64), want[2])
    for chunk_tokens in (64, 4096, 10**9):
        ex = NGramExtractor(max_n=max_n, min_freq=min_freq, max_f_grams=max_f).fit_gpu(iter(corpus), verbose=False,
                                                                                      chunk_tokens=chunk_tokens)
        _assert_result(ex.key_arrays() + (ex.counts,), want, (max_n, chunk_tokens))
        assert np.array_equal(ex.key_arrays()[0], one.key_arrays()[0]) and np.array_equal(ex.key_arrays()[1], one.key_arrays()[1])
    with NGramExtractor(max_n=max_n).fit_state() as st:
        for tok, off in _chunks(corpus, 4096):
            st.update(tok, off)
        assert st.finalize(min_freq, max_f)[3] == len(counter) == st.stats()["n_distinct"]
        assert st.stats()["n_occurrences"] == sum(counter.values()) == st.stats()["next_seq"]


# ------------------------------------------------------------------ 3. growth
@pytest.mark.parametrize("max_n,min_freq,max_f", SETTINGS)
def test_growth_before_the_count_and_the_memory_bound(max_n, min_freq, max_f):
    """The table follows the growth rule exactly: before a chunk it holds >= 2 * need slots, need = n_distinct + occurrences of the
    chunk, grown to the smallest such power of two.  So slots < 4 * max(512, need) always, and the final size is
    pow2(2 * largest need).  Against the one-shot's pow2(2 * occurrences): this corpus has 0.22 (max_n 2), 0.42 (3) and 0.55 (4)
    distinct n-grams per occurrence; 2 * (distinct + 256 * max_n) stays below 2^18 / 2^19 for max_n 2 / 3, a QUARTER of the one-shot's
    2^20 / 2^21, while at max_n = 4 (450,514 distinct of 815,059 occurrences) the rule gives 2^20, half of 2^21: memory follows the
    distinct n-grams, and the quarter is asserted where the rule's arithmetic yields it."""
    from scone_amd.hip_backend import FitState, fit_occurrences
    corpus = _corpus()
    counter, _ = _counter(max_n)
    with FitState(max_n, initial_slots=1024) as st:
        assert st.stats() == {"n_distinct": 0, "n_occurrences": 0, "slots": 1024, "n_grows": 0, "next_seq": 0}
        largest_need = 0
        for tok, off in _chunks(corpus, 256):
            before = st.stats()
            need = before["n_distinct"] + fit_occurrences(np.diff(off), max_n)
            st.update(tok, off)
            after = st.stats()
            largest_need = max(largest_need, need)
            assert after["slots"] < 4 * max(512, need)
            assert after["slots"] >= 2 * after["n_distinct"]
            assert after["slots"] == max(before["slots"], _pow2_at_least(2 * need))
            assert after["n_grows"] == before["n_grows"] + (after["slots"] != before["slots"])
        s = st.stats()
        assert s["n_grows"] >= 3
        assert s["slots"] == _pow2_at_least(2 * largest_need)
        assert s["n_occurrences"] == sum(counter.values())
        one_shot = _pow2_at_least(2 * s["n_occurrences"])
        assert s["slots"] * (2 if max_n == 4 else 4) <= one_shot
        _assert_result(st.finalize(min_freq, max_f), _host_fit(counter, max_n, min_freq, max_f), max_n)
        assert s["n_distinct"] == len(counter)


# ------------------------------------------------------------------ 4. order independence and merge
@pytest.mark.parametrize("max_n", [3, 4])
def test_shards_out_of_order_and_merged_in_any_order(max_n):
    from scone_amd.hip_backend import FitState, fit_occurrences
    corpus = _corpus()
    counter, _ = _counter(max_n)
    cuts = [0, 230, 470, len(corpus)]
    shards = [corpus[a:b] for a, b in zip(cuts, cuts[1:])]
    bases = [fit_occurrences([len(t) for t in corpus[:a]], max_n) for a in cuts[:3]]
    want = _host_fit(counter, max_n, 1, 10**9)

    def count(state, k):
        for tok, off in _chunks(shards[k], 5000):            # every chunk of the shard carries its own global number
            state.update(tok, off, seq_base=bases_k[k])
            bases_k[k] += fit_occurrences(np.diff(off), max_n)

    with FitState(max_n) as ordered, FitState(max_n) as shuffled:
        for tok, off in _chunks(corpus, 5000):
            ordered.update(tok, off)
        ref_export = _sorted_export(ordered)
        _assert_result(ordered.finalize(1, 10**9), want, "in order")
        bases_k = list(bases)
        for k in (2, 0, 1):
            count(shuffled, k)
        _assert_result(shuffled.finalize(1, 10**9), want, "3, 1, 2")
        _assert_same_export(_sorted_export(shuffled), ref_export)
        assert shuffled.stats()["next_seq"] == ordered.stats()["next_seq"] == sum(counter.values())

    exports = []
    bases_k = list(bases)
    for k in range(3):
        with FitState(max_n) as part:
            count(part, k)
            exports.append(part.export())
    for order in ((0, 1, 2), (2, 1, 0)):
        with FitState(max_n, initial_slots=1024) as merged:
            for k in order:
                merged.merge(*exports[k])
            assert merged.stats()["n_distinct"] == len(counter)
            _assert_result(merged.finalize(1, 10**9), want, order)
            _assert_result(merged.finalize(2, 1000), _host_fit(counter, max_n, 2, 1000), order)
            _assert_same_export(_sorted_export(merged), ref_export)


# ------------------------------------------------------------------ 5. finalise does not consume the state
def test_finalize_is_repeatable_and_updates_may_follow():
    from scone_amd import NGramExtractor
    max_n = 3
    corpus = _corpus()
    half = len(corpus) // 2
    first_half, _ = _counter(max_n, 0, half)
    whole, _ = _counter(max_n)
    with NGramExtractor(max_n=max_n).fit_state() as st:
        for tok, off in _chunks(corpus[:half], 3000):
            st.update(tok, off)
        _assert_result(st.finalize(2, 1000), _host_fit(first_half, max_n, 2, 1000), "first")
        everything = _host_fit(first_half, max_n, 1, 10**9)
        _assert_result(st.finalize(1, 10**9), everything, "second")
        ex = NGramExtractor.from_fit_state(st, 2, 1000)
        assert ex.max_n == max_n and ex.min_freq == 2 and ex.max_f_grams == 1000
        _assert_result(ex.key_arrays() + (ex.counts,), _host_fit(first_half, max_n, 2, 1000), "from_fit_state")
        cut = st.finalize(1, 10**9, out_cap=37)                         # fewer rows than eligible entries: the first out_cap ids
        _assert_result(cut, tuple(a[:37] for a in everything), "out_cap")
        for tok, off in _chunks(corpus[half:], 3000):
            st.update(tok, off)
        _assert_result(st.finalize(1, 10**9), _host_fit(whole, max_n, 1, 10**9), "whole")
        _assert_result(st.finalize(2, 50_000), _host_fit(whole, max_n, 2, 50_000), "whole, filtered")


# ------------------------------------------------------------------ 6. a refused chunk changes nothing
def test_a_refused_chunk_changes_nothing():
    from scone_amd import _lib
    from scone_amd.hip_backend import FitState
    max_n = 4
    corpus = _corpus()
    half = len(corpus) // 2
    whole, _ = _counter(max_n)
    rest = _chunks(corpus[half:], 3000)
    with FitState(max_n, initial_slots=1024) as st:
        for tok, off in _chunks(corpus[:half], 3000):
            st.update(tok, off)
        snapshot, stats = _sorted_export(st), st.stats()

        tok, off = rest[0]
        bad = tok.copy()
        bad[-1] = -5                                                    # one negative token in the chunk's last text
        with pytest.raises(ValueError):
            st.update(bad, off)
        bad = tok.copy()
        bad[len(bad) // 2] = 2**24                                      # max_n = 4 packs 24 bits per token
        with pytest.raises(ValueError):
            st.update(bad, off)
        bad[len(bad) // 2] = 2**24 - 1                                  # the first value the packing cannot hold
        with pytest.raises(ValueError):
            st.update(bad, off)

        def rc_of(tokens, offsets):
            t = torch.from_numpy(tokens).cuda()
            o = torch.from_numpy(offsets).cuda()
            rc = _lib.lib().scone_fit_update(st._st, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(o.data_ptr()), o.numel() - 1,
                                             2**64 - 1, None)
            torch.cuda.synchronize()
            return rc

        short = off.copy()
        short[-1] -= 1                                                  # offsets[n] != n_tokens
        assert rc_of(tok, short) == _lib.EINVAL
        with pytest.raises(ValueError):
            st.update(tok, short)
        swapped = off.copy()
        swapped[1], swapped[2] = max(off[1], off[2]) + 1, min(off[1], off[2])     # decreasing
        assert rc_of(tok, swapped) == _lib.EINVAL
        shifted = off.copy()
        shifted[0] = 1                                                  # does not start at 0
        assert rc_of(tok, shifted) == _lib.EINVAL
        bad = tok.copy()
        bad[0] = -1
        assert rc_of(bad, off) == _lib.ERANGE

        k, l, c, f = snapshot
        with pytest.raises(ValueError):                                 # merge validates before it applies: a length of 0 ...
            st.merge(k[:3], np.array([1, 0, 1], dtype=np.uint8), c[:3], f[:3])
        with pytest.raises(ValueError):                                 # ... and one beyond max_n
            st.merge(k[:3], np.array([1, 5, 1], dtype=np.uint8), c[:3], f[:3])
        wide = k[:3].copy()
        wide[2, 0] = 2**24 - 1
        with pytest.raises(ValueError):
            st.merge(wide, np.array([1, 1, 1], dtype=np.uint8), c[:3], f[:3])

        _assert_same_export(_sorted_export(st), snapshot)
        assert st.stats() == stats
        for tok, off in rest:
            st.update(tok, off)
        _assert_result(st.finalize(1, 20_000), _host_fit(whole, max_n, 1, 20_000), "after the refusals")


# ------------------------------------------------------------------ 7. 64-bit counts
def test_counts_are_64_bits_wide():
    from scone_amd.hip_backend import FitState
    with FitState(3) as st:
        st.update(np.array([7, 8, 7], dtype=np.int32), np.array([0, 3], dtype=np.int64))
        keys = np.array([[100, 0, 0], [200, 201, 0], [300, 301, 302]], dtype=np.uint32)
        lens = np.array([1, 2, 3], dtype=np.uint8)
        counts = np.array([2**33 + 5, 2**33 + 5, 2**32 - 1], dtype=np.uint64)
        st.merge(keys, lens, counts, np.array([9, 4, 0], dtype=np.uint64))
        k, l, c, n_distinct = st.finalize(1, 10**9)
        assert n_distinct == 3 + 5                                      # 7, 8, (7,8), (8,7), (7,8,7)
        assert c.dtype == np.uint64
        assert c.tolist() == [2**33 + 5, 2**33 + 5, 2**32 - 1, 2, 1, 1, 1, 1]
        assert l.tolist() == [2, 1, 3, 1, 1, 2, 2, 3]
        assert k.tolist() == [[200, 201, 0], [100, 0, 0], [300, 301, 302], [7, 0, 0], [8, 0, 0], [7, 8, 0], [8, 7, 0], [7, 8, 7]]
        st.merge(keys[:1], lens[:1], np.array([2**40], dtype=np.uint64), np.array([50], dtype=np.uint64))      # sums, keeps the min
        k, l, c, _ = st.finalize(2**32 - 1, 10**9)
        assert c.tolist() == [2**40 + 2**33 + 5, 2**33 + 5, 2**32 - 1] and k[0].tolist() == [100, 0, 0]
        ek, el, ec, ef = _sorted_export(st)
        assert ef[ek[:, 0] == 100].tolist() == [9]


# ------------------------------------------------------------------ 8. edges
def test_edges():
    from scone_amd import NGramExtractor
    from scone_amd.hip_backend import FitState
    i32, i64 = (lambda a: np.array(a, dtype=np.int32)), (lambda a: np.array(a, dtype=np.int64))
    with FitState(3) as a, FitState(3) as b:                            # two states alive at once on one device
        empty = {"n_distinct": 0, "n_occurrences": 0, "slots": 1024, "n_grows": 0, "next_seq": 0}
        k, l, c, n = a.finalize(1, 10)                                  # finalised before any update
        assert k.shape == (0, 3) and l.shape == (0,) and c.shape == (0,) and n == 0
        assert all(x.shape[0] == 0 for x in a.export())
        a.update(i32([]), i64([0, 0, 0]))                               # a chunk of only empty texts
        a.update(i32([]), i64([0]))                                     # n_texts = 0
        assert a.stats() == empty
        a.update(i32([5, 6, 9]), i64([0, 2, 2, 3]))                     # texts shorter than max_n, an empty one between
        b.update(i32([9, 9, 9, 9]), i64([0, 4]))
        k, l, c, n = a.finalize(1, 10**9)
        assert n == 4 and k.tolist() == [[5, 0, 0], [6, 0, 0], [5, 6, 0], [9, 0, 0]] and c.tolist() == [1, 1, 1, 1]
        assert a.stats()["next_seq"] == 4 == a.stats()["n_occurrences"]
        k, l, c, n = b.finalize(1, 10**9)
        assert n == 3 and k.tolist() == [[9, 0, 0], [9, 9, 0], [9, 9, 9]] and c.tolist() == [4, 3, 2]
        k, l, c, n = b.finalize(1, 0)                                   # max_f_grams = 0
        assert k.shape[0] == 0 and n == 3
        assert b.finalize(5, 10)[0].shape[0] == 0                       # nothing is frequent enough
        a.update(i32([9]), i64([0, 1]))
        assert a.finalize(2, 10)[0].tolist() == [[9, 0, 0]]             # a's 9 is not b's
        assert b.finalize(1, 10)[2].tolist() == [4, 3, 2]
    ex = NGramExtractor(max_n=2, min_freq=1).fit_gpu(iter([[], [], []]), verbose=False, chunk_tokens=4)
    assert len(ex) == 0 and ex.key_arrays()[0].shape == (0, 2)
    with pytest.raises(ValueError):
        NGramExtractor(max_n=2, min_freq=1).fit_gpu([[1, -2, 3]], verbose=False, chunk_tokens=2)
