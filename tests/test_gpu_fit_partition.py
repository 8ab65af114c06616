"""GPU: the key-hash partitioned fit (scone_fit_update_part / scone_fit_finalize_seq; FitState.update(part=, n_parts=),
FitState.finalize(with_first=True), NGramExtractor.fit_gpu(partitions=P)).  A part's state holds exactly the keys of its part
with their whole counts and first numbers; the parts' own selections, merged, give the host fit's list -- same keys, same ids,
same counts; a part's memory follows its own distinct keys.

References: the host `fit` (a Counter), the unpartitioned streaming state fed the same chunks, the numpy restatement of the
partition function (tests/fit_partition_fixture.py) and the reference-pinned golden lists (tests/golden/match.npz).  Everything
is exact: no tolerance anywhere.  The corpus is streamed in chunks of 2048 tokens.  Run with ``-m gpu`` on an MI355X.
"""

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_partition_fixture as FX  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ------------------------------------------------------------------ shared references (computed once, never modified)
@functools.lru_cache(maxsize=None)
def _dev_chunks():
    """The corpus in chunks of 2048 tokens, resident on the device: ((tokens int32, offsets int64, occurrences per max_n), ...)"""
    from scone_amd.hip_backend import fit_occurrences
    return tuple((torch.from_numpy(tok).cuda(), torch.from_numpy(off).cuda(),
                  {m: fit_occurrences(np.diff(off), m) for m in (1, 3, 4)}) for tok, off in FX.chunks())


def _sorted_export(state):
    return FX.sort_rows(*state.export())


@functools.lru_cache(maxsize=None)
def _whole(max_n):
    """The unpartitioned streaming state fed the same chunks: its sorted export and its stats."""
    from scone_amd.hip_backend import FitState
    with FitState(max_n, initial_slots=1024) as st:
        for tok, off, _ in _dev_chunks():
            st.update(tok, off)
        export, stats = _sorted_export(st), st.stats()
    keys, lens, counts = FX.sort_rows(*FX.distinct(max_n))               # the Counter's, in the same order
    assert np.array_equal(export[0], keys) and np.array_equal(export[1], lens) and np.array_equal(export[2], counts)
    assert stats["n_distinct"] == len(lens) and stats["n_occurrences"] == int(counts.sum()) == stats["next_seq"]
    return export, stats


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def _assert_fit(ex, want, what):
    keys, lens = ex.key_arrays()
    assert np.array_equal(lens, want[1]), what
    assert np.array_equal(keys, want[0]), what
    assert ex.counts.dtype == np.uint64 and np.array_equal(ex.counts, want[2]), what


# ------------------------------------------------------------------ 1. what a part holds
@pytest.mark.parametrize("n_parts", [2, 3, 8])
@pytest.mark.parametrize("max_n", [1, 3, 4])
def test_a_part_holds_exactly_its_keys_with_whole_counts_and_first_numbers(max_n, n_parts):
    from scone_amd.hip_backend import FitState, fit_partition
    export, stats = _whole(max_n)
    part_of = fit_partition(export[0], export[1], max_n, n_parts)
    assert np.array_equal(part_of, FX.partition(export[0], export[1], max_n, n_parts))
    n_distinct = 0
    for p in range(n_parts):
        with FitState(max_n, initial_slots=1024) as st:
            for tok, off, _ in _dev_chunks():
                st.update(tok, off, part=p, n_parts=n_parts)
            got, s = _sorted_export(st), st.stats()
        mine = part_of == p
        _same(got, tuple(a[mine] for a in export))                      # keys, lengths, counts (= the Counter's), first numbers
        assert s["n_distinct"] == int(mine.sum())
        assert s["next_seq"] == stats["next_seq"] and s["n_occurrences"] == stats["n_occurrences"]
        n_distinct += s["n_distinct"]
    assert n_distinct == stats["n_distinct"]


# ------------------------------------------------------------------ 2. end to end
@pytest.mark.parametrize("n_parts", [2, 8])
@pytest.mark.parametrize("max_n,min_freq,max_f", [(3, 1, 100_000), (3, 2, 10**7), (4, 5, 500), (1, 1, 10**7)])
def test_fit_gpu_with_partitions_gives_the_host_fit(max_n, min_freq, max_f, n_parts):
    from scone_amd import NGramExtractor
    want = FX.host_fit(max_n, min_freq, max_f)
    if (max_n, min_freq, max_f) == (3, 1, 100_000):
        # the list is cut inside the group of count-1 n-grams, whose ids are decided by first numbers ACROSS parts: the group
        # has kept and dropped members, and each side lies in at least two parts
        keys, lens, counts = FX.host_fit(max_n, 1, 10**7)
        assert len(want[1]) == max_f < len(lens) and counts[max_f - 1] == counts[max_f] == 1
        group = counts == counts[max_f]
        kept = np.arange(len(lens)) < max_f
        part_of = FX.partition(keys, lens, max_n, n_parts)
        assert len(np.unique(part_of[group & kept])) >= 2 and len(np.unique(part_of[group & ~kept])) >= 2
    ex = NGramExtractor(max_n=max_n, min_freq=min_freq, max_f_grams=max_f).fit_gpu(FX.corpus(), verbose=False,
                                                                                  chunk_tokens=FX.CHUNK_TOKENS, partitions=n_parts)
    _assert_fit(ex, want, (max_n, min_freq, max_f, n_parts))


def test_partitions_match_reference_order_on_every_golden_corpus(golden_dir):
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
        ex = NGramExtractor(max_n=max_n, min_freq=min_freq, max_f_grams=max_f).fit_gpu(corpus, verbose=False, chunk_tokens=7,
                                                                                      partitions=3)
        keys, lens = ex.key_arrays()
        assert np.array_equal(lens, z[f"{c}_lens"]), c
        assert np.array_equal(keys, z[f"{c}_keys"]), c
        assert ex.counts.dtype == np.uint64 and len(ex.counts) == len(lens)
    assert seen_max_n == {1, 2, 3, 4}


# ------------------------------------------------------------------ 3. memory follows the part's own distinct keys
@pytest.mark.parametrize("max_n,n_parts", [(3, 8), (4, 3)])
def test_a_part_grows_by_its_own_history(max_n, n_parts):
    """The growth rule of scone_fit_update, per part: before a chunk the table holds >= 2 * need slots, need = the part's
    n_distinct + ALL occurrences of the chunk, grown to the smallest such power of two.  At max_n = 3 and 8 parts a part holds
    at most 1.008 x 254,924 / 8 = 32,120 keys and a chunk at most 3 x (2047 + 599) occurrences, so 2 * need < 2^17, while the
    unpartitioned state needs at least 2 x 254,924 slots, 2^19: a quarter, asserted where the arithmetic yields it."""
    from scone_amd.hip_backend import FitState
    _, whole = _whole(max_n)
    largest = 0
    for p in range(n_parts):
        with FitState(max_n, initial_slots=1024) as st:
            largest_need = 0
            for tok, off, occ in _dev_chunks():
                before = st.stats()
                need = before["n_distinct"] + occ[max_n]
                st.update(tok, off, part=p, n_parts=n_parts)
                after = st.stats()
                largest_need = max(largest_need, need)
                assert after["slots"] == max(before["slots"], FX.pow2_at_least(2 * need))
                assert after["slots"] < 4 * max(512, largest_need) and after["slots"] >= 2 * after["n_distinct"]
                assert after["n_grows"] == before["n_grows"] + (after["slots"] != before["slots"])
            s = st.stats()
            assert s["slots"] == FX.pow2_at_least(2 * largest_need) and s["n_grows"] >= 3
            largest = max(largest, s["slots"])
    print("max_n %d, %d parts: largest part %d slots, unpartitioned %d" % (max_n, n_parts, largest, whole["slots"]))
    if (max_n, n_parts) == (3, 8):
        assert largest <= 2**17 and whole["slots"] >= 2**19
        assert 4 * largest <= whole["slots"]
    else:
        assert largest < whole["slots"]


# ------------------------------------------------------------------ 4. one part of one is the plain update
def test_part_0_of_1_is_the_plain_update():
    from scone_amd.hip_backend import FitState
    export, stats = _whole(3)
    with FitState(3, initial_slots=1024) as st:
        for tok, off, _ in _dev_chunks():
            st.update(tok, off, part=0, n_parts=1)
        _same(_sorted_export(st), export)
        assert st.stats() == stats


# ------------------------------------------------------------------ 5. the state does not remember partitions
def test_both_parts_of_every_chunk_into_one_state():
    from scone_amd.hip_backend import FitState
    max_n = 3
    export, stats = _whole(max_n)
    with FitState(max_n, initial_slots=1024) as st:
        base = 0
        for tok, off, occ in _dev_chunks():
            st.update(tok, off, seq_base=base, part=0, n_parts=2)
            st.update(tok, off, seq_base=base, part=1, n_parts=2)
            base += occ[max_n]
        _same(_sorted_export(st), export)
        s = st.stats()
        assert s["n_distinct"] == stats["n_distinct"] and s["next_seq"] == stats["next_seq"]
        assert s["n_occurrences"] == 2 * stats["n_occurrences"]          # occurrences FED: every chunk went in twice


# ------------------------------------------------------------------ 6. a refused call changes nothing
def test_a_refused_partitioned_update_changes_nothing():
    from scone_amd import _lib
    from scone_amd.hip_backend import FitState
    chunks = _dev_chunks()
    with FitState(4, initial_slots=1024) as st:
        for tok, off, _ in chunks[:40]:
            st.update(tok, off, part=1, n_parts=3)
        snapshot, stats = _sorted_export(st), st.stats()
        assert stats["n_distinct"] > 10_000
        tok, off, _ = chunks[40]

        def rc_of(tokens, part, n_parts):
            rc = _lib.lib().scone_fit_update_part(st._st, C.c_void_p(tokens.data_ptr()), tokens.numel(), C.c_void_p(off.data_ptr()),
                                                  off.numel() - 1, 2**64 - 1, part, n_parts, None)
            torch.cuda.synchronize()
            return rc

        assert rc_of(tok, 3, 3) == _lib.EINVAL                          # part = n_parts
        assert rc_of(tok, 0, 0) == _lib.EINVAL                          # n_parts = 0
        bad = tok.clone()
        bad[-1] = -5
        assert rc_of(bad, 1, 3) == _lib.ERANGE                          # a negative token, valid part arguments
        bad[-1] = 2**24 - 1                                             # max_n = 4: the first value the packing cannot hold
        assert rc_of(bad, 1, 3) == _lib.ERANGE
        with pytest.raises(ValueError):
            st.update(tok, off, part=3, n_parts=3)
        with pytest.raises(ValueError):
            st.update(tok, off, part=0, n_parts=0)
        with pytest.raises(ValueError):
            st.update(bad, off, part=1, n_parts=3)
        with pytest.raises(ValueError):
            st.update(tok, off, part=1)                                 # both or neither
        with pytest.raises(ValueError):
            st.update(tok, off, n_parts=3)
        _same(_sorted_export(st), snapshot)
        assert st.stats() == stats
        assert rc_of(tok, 1, 3) == _lib.OK                              # and the state goes on counting
        assert st.stats()["next_seq"] > stats["next_seq"]


# ------------------------------------------------------------------ 7. scone_fit_finalize_seq
def test_finalize_seq_is_finalize_plus_first_numbers():
    from scone_amd import _lib
    from scone_amd.hip_backend import FitState
    max_n = 3
    with FitState(max_n) as st:
        for tok, off, _ in _dev_chunks():
            st.update(tok, off, part=2, n_parts=3)
        ek, el, ec, ef = st.export()
        first_of = {(int(l),) + tuple(int(x) for x in k): int(f) for k, l, f in zip(ek, el, ef)}
        for min_freq, max_f in ((1, 10**9), (2, 5000), (1, 20_000), (50, 10)):
            plain = st.finalize(min_freq, max_f)
            seq = st.finalize(min_freq, max_f, with_first=True)
            assert len(plain) == 4 and len(seq) == 5 and seq[3] == plain[3]
            _same(seq[:3], plain[:3])
            assert len(plain[1]) == min(max_f, int((ec >= min_freq).sum())) > 0
            assert seq[4].dtype == np.uint64
            assert seq[4].tolist() == [first_of[(int(l),) + tuple(int(x) for x in k)] for k, l in zip(seq[0], seq[1])]
            again = st.finalize(min_freq, max_f, with_first=True)       # a second call gives the same rows
            _same(again[:3] + again[4:], seq[:3] + seq[4:])
            same_count = seq[2][1:] == seq[2][:-1]                      # the list's order: count descending, first ascending
            assert (seq[2][1:] <= seq[2][:-1]).all() and (seq[4][1:][same_count] > seq[4][:-1][same_count]).all()

        # NULL d_first_out / d_counts_out are accepted
        want = st.finalize(2, 5000, with_first=True)
        n = len(want[1])
        keys = torch.zeros((n, max_n), dtype=torch.int32, device="cuda")
        lens = torch.zeros(n, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        first = torch.zeros(n, dtype=torch.int64, device="cuda")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        for c, f in ((counts, None), (None, first), (None, None)):
            keys.zero_(), lens.zero_(), counts.zero_(), first.zero_()
            n_out = C.c_uint64(0)
            rc = _lib.lib().scone_fit_finalize_seq(st._st, 2, 5000, ptr(keys), ptr(lens), ptr(c), ptr(f), n, C.byref(n_out), None)
            torch.cuda.synchronize()
            assert rc == _lib.OK and n_out.value == n
            assert np.array_equal(keys.cpu().numpy().view(np.uint32), want[0]) and np.array_equal(lens.cpu().numpy(), want[1])
            assert np.array_equal(counts.cpu().numpy().view(np.uint64), want[2] if c is not None else np.zeros(n, dtype=np.uint64))
            assert np.array_equal(first.cpu().numpy().view(np.uint64), want[4] if f is not None else np.zeros(n, dtype=np.uint64))
        # a selection is what merge takes
        with FitState(max_n) as other:
            other.merge(want[0], want[1], want[2], want[4])
            _same(other.finalize(2, 5000, with_first=True)[:3], want[:3])


# ------------------------------------------------------------------ 8. parts without any key
def test_empty_parts():
    from scone_amd import NGramExtractor
    from scone_amd.hip_backend import FitState, fit_partition
    tok, off = np.array([3], dtype=np.int32), np.array([0, 1], dtype=np.int64)
    home = int(fit_partition(np.array([[3]], dtype=np.uint32), np.array([1], dtype=np.uint8), 1, 8)[0])
    for p in range(8):
        with FitState(1) as st:
            st.update(tok, off, part=p, n_parts=8)
            s = st.stats()
            assert s["n_distinct"] == (p == home) and s["n_occurrences"] == 1 == s["next_seq"] and s["slots"] == 1024
            k, l, c, n, f = st.finalize(1, 10, with_first=True)
            if p == home:
                assert k.tolist() == [[3]] and l.tolist() == [1] and c.tolist() == [1] and f.tolist() == [0] and n == 1
            else:
                assert k.shape == (0, 1) and l.shape == (0,) and c.shape == (0,) and f.shape == (0,) and n == 0
                assert all(x.shape[0] == 0 for x in st.export())
    host = NGramExtractor(max_n=1, min_freq=1).fit([[3]], verbose=False)
    ex = NGramExtractor(max_n=1, min_freq=1).fit_gpu([[3]], verbose=False, chunk_tokens=FX.CHUNK_TOKENS, partitions=8)
    assert np.array_equal(ex.key_arrays()[0], host.key_arrays()[0]) and np.array_equal(ex.key_arrays()[1], host.key_arrays()[1])
    assert ex.counts.tolist() == [1]
    ex = NGramExtractor(max_n=2, min_freq=1).fit_gpu([[], []], verbose=False, chunk_tokens=4, partitions=4)
    assert len(ex) == 0 and ex.key_arrays()[0].shape == (0, 2)
