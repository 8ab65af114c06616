"""CPU: the key-hash partitioned fit.  scone_fit_partition / scone_fit_update_part / scone_fit_finalize_seq are declared, bound
and exported; the partition function equals its numpy restatement (tests/fit_partition_fixture.py) and is balanced; the
refusals that need no device; the driver of `NGramExtractor.fit_gpu(partitions=P)` against a fake state."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_partition_fixture as FX  # noqa: E402

from scone_amd import NGramExtractor, _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["scone_fit_partition", "scone_fit_update_part", "scone_fit_finalize_seq"]


def _header():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    return re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)     # comments blanked, positions kept


# ------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_and_exported_with_matching_arguments(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/scone_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert len(argtypes) == len(args), name
    for text, ct in zip(args, argtypes):
        if text.startswith("uint64_t *h_"):
            assert ct is C.POINTER(_lib._U64), text            # host result
        elif "*" in text or text.startswith("scone_stream_t"):
            assert ct is _lib._P, text
        else:
            want = {"int32_t": _lib._I32, "int64_t": _lib._I64, "uint32_t": _lib._U32, "uint64_t": _lib._U64}[text.split()[0]]
            assert ct is want, text
    assert hasattr(_lib.lib(), name)


def test_argument_names_are_the_contract():
    def names(fn):
        decl = re.search(r"%s\s*\(([^)]*)\)" % fn, _header()).group(1)
        return [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names("scone_fit_partition") == ["h_keys", "h_lens", "n", "max_n", "n_parts", "h_part_out"]
    assert names("scone_fit_update_part") == ["st", "d_tokens", "n_tokens", "d_text_offsets", "n_texts", "seq_base", "part",
                                              "n_parts", "stream"]
    assert names("scone_fit_finalize_seq") == ["st", "min_freq", "max_f_grams", "d_keys_out", "d_lens_out", "d_counts_out",
                                               "d_first_out", "out_cap", "h_n_out", "stream"]


def test_declared_in_the_fit_section_and_the_abi_version_is_still_2():
    raw = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    h = _header()
    lo = re.search(r"\bint\s+scone_fit\s*\(", h).start()
    hi = raw.index("/* ---- table: rows")
    for name in NAMES:
        assert lo < re.search(r"\b%s\s*\(" % name, h).start() < hi, name
    assert re.findall(r"\bint\s+(scone_\w+)\s*\(", h)[-1] == "scone_embed_select"
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", h)
    assert _lib.ABI_VERSION == 2 and _lib.lib().scone_abi_version() == 2
    # the partition formula is part of the contract: it is written out in the header
    assert "part = (uint32_t)(((scone_hash_key(lo, ext) >> 32) * (uint64_t)n_parts) >> 32)" in raw


# ------------------------------------------------------------------ the partition function
def _c_partition(keys, lens, max_n, n_parts, out=None):
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    lens = np.ascontiguousarray(lens, dtype=np.uint8)
    if out is None:
        out = np.zeros(lens.shape[0], dtype=np.uint32)
    rc = _lib.lib().scone_fit_partition(keys.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p), lens.shape[0], max_n,
                                        n_parts, out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("max_n", [1, 3, 4])
def test_partition_equals_the_numpy_restatement_on_every_distinct_n_gram(max_n):
    from scone_amd.hip_backend import fit_partition
    keys, lens, _ = FX.distinct(max_n)
    if max_n in FX.N_DISTINCT:
        assert lens.shape[0] == FX.N_DISTINCT[max_n]
    assert sum(len(t) for t in FX.corpus()) == FX.N_TOKENS
    for n_parts in (1, 2, 3, 8, 64, 2**32 - 1):
        rc, got = _c_partition(keys, lens, max_n, n_parts)
        assert rc == _lib.OK
        want = FX.partition(keys, lens, max_n, n_parts)
        assert np.array_equal(got, want), n_parts
        assert int(got.max()) < n_parts
        if n_parts == 1:
            assert not got.any()
        if n_parts == 2**32 - 1:
            assert len(np.unique(got)) > 0.99 * len(got)                   # the whole upper half of the hash is used
    assert np.array_equal(fit_partition(keys, lens, max_n, 8), FX.partition(keys, lens, max_n, 8))


@pytest.mark.parametrize("max_n", [3, 4])
def test_partition_is_balanced(max_n):
    """A condition on the partition function, not a measurement: the fullest part holds at most 1.05 x the mean number of
    distinct keys (this formula: at most 1.008 on this corpus)."""
    keys, lens, _ = FX.distinct(max_n)
    for n_parts in (2, 3, 8):
        rc, part = _c_partition(keys, lens, max_n, n_parts)
        assert rc == _lib.OK
        sizes = np.bincount(part, minlength=n_parts)
        assert sizes.sum() == len(lens)
        worst = sizes.max() / (len(lens) / n_parts)
        print("max_n %d, n_parts %d: fullest part / mean = %.4f" % (max_n, n_parts, worst))
        assert worst <= 1.05, (max_n, n_parts, worst)


def test_partition_refusals_write_nothing():
    keys = np.array([[1, 2, 3, 4], [5, 6, 0, 0], [7, 0, 0, 0]], dtype=np.uint32)
    lens = np.array([4, 2, 1], dtype=np.uint8)
    mark = np.full(3, 0xABCD1234, dtype=np.uint32)

    def refused(code, k=keys, l=lens, max_n=4, n_parts=8):
        out = mark.copy()
        rc, out = _c_partition(k, l, max_n, n_parts, out)
        assert rc == code and np.array_equal(out, mark)

    assert _c_partition(keys, lens, 4, 8)[0] == _lib.OK
    refused(_lib.EINVAL, n_parts=0)
    refused(_lib.EINVAL, l=np.array([4, 2, 0], dtype=np.uint8))            # a length of 0, in the LAST row: rows before it unwritten
    refused(_lib.EINVAL, l=np.array([4, 2, 5], dtype=np.uint8))            # max_n + 1
    refused(_lib.EINVAL, k=keys[:, :3], l=np.array([3, 2, 4], dtype=np.uint8), max_n=3)
    refused(_lib.EINVAL, max_n=0)
    refused(_lib.EINVAL, max_n=5)
    wide = keys.copy()
    wide[2, 0] = 2**24 - 1                                                 # the first token max_n = 4 cannot pack
    refused(_lib.ERANGE, k=wide)
    wide[2, 0] = 2**24 - 2
    assert _c_partition(wide, lens, 4, 8)[0] == _lib.OK
    lib = _lib.lib()
    p = keys.ctypes.data_as(C.c_void_p)
    assert lib.scone_fit_partition(None, p, 3, 4, 8, p) == _lib.EINVAL     # null arrays with n > 0
    assert lib.scone_fit_partition(p, None, 3, 4, 8, p) == _lib.EINVAL
    assert lib.scone_fit_partition(p, p, 3, 4, 8, None) == _lib.EINVAL
    assert lib.scone_fit_partition(None, None, 0, 4, 8, None) == _lib.OK   # n = 0 needs no arrays
    from scone_amd.hip_backend import fit_partition
    with pytest.raises(ValueError):
        fit_partition(keys, lens, 4, 0)
    with pytest.raises(IndexError):
        fit_partition(wide + 1, lens, 4, 8)
    with pytest.raises(ValueError):
        fit_partition(keys, lens, 3, 8)                                    # keys are not [n, max_n]


def test_null_state_without_device_work():
    lib = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_uint64(7)
    assert lib.scone_fit_update_part(None, p, 2, p, 1, 0, 0, 2, None) == _lib.EINVAL
    assert lib.scone_fit_finalize_seq(None, 1, 10, p, p, p, p, 4, C.byref(n), None) == _lib.EINVAL
    assert n.value == 7


# ------------------------------------------------------------------ the driver of fit_gpu(partitions=P)
class _PlainState:
    """The fake state of test_fit_stream_host.py: update(tokens, offsets) and finalize(min_freq, max_f_grams) take no more."""
    log = None

    def __init__(self, max_n, device=None, initial_slots=0):
        self.max_n = max_n
        _PlainState.log.append(("open",))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _PlainState.log.append(("close",))

    def update(self, tokens, text_offsets):
        _PlainState.log.append(("update", np.array(tokens).tolist(), np.array(text_offsets).tolist()))

    def finalize(self, min_freq, max_f_grams):
        _PlainState.log.append(("finalize", min_freq, max_f_grams))
        return (np.zeros((0, self.max_n), dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64), 0)


class _PartState:
    """Stands in for hip_backend.FitState on the partitioned route: records every call; next_seq advances by the tokens fed
    (max_n = 1: one occurrence per token), whatever the part."""
    log = None
    opened = 0

    def __init__(self, max_n, device=None, initial_slots=0):
        self.max_n, self.next_seq, self.id = max_n, 0, _PartState.opened
        _PartState.opened += 1
        _PartState.log.append(("open", self.id))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _PartState.log.append(("close", self.id))

    def update(self, tokens, text_offsets, seq_base=None, part=None, n_parts=None):
        assert seq_base is None
        self.next_seq += len(tokens)
        _PartState.log.append(("update", self.id, part, n_parts, np.array(tokens).tolist(), np.array(text_offsets).tolist()))

    def stats(self):
        return {"next_seq": self.next_seq}

    def finalize(self, min_freq, max_f_grams, with_first=False):
        _PartState.log.append(("finalize", self.id, min_freq, max_f_grams, with_first))
        res = (np.full((1, self.max_n), self.id, dtype=np.uint32), np.ones(1, dtype=np.uint8), np.ones(1, dtype=np.uint64), 1)
        return res + (np.full(1, 100 + self.id, dtype=np.uint64),) if with_first else res

    def merge(self, keys, lens, counts, first):
        _PartState.log.append(("merge", self.id, keys.tolist(), lens.tolist(), counts.tolist(), first.tolist()))


CORPUS = [[1, 2, 3], [], [4], [5, 6, 7, 8, 9], [10]]


def _fake(monkeypatch, cls):
    from scone_amd import hip_backend
    monkeypatch.setattr(hip_backend, "FitState", cls)
    cls.log, cls.opened = [], 0


@pytest.mark.parametrize("partitions", [None, 1])
def test_no_partitions_is_the_streaming_route_called_as_before(monkeypatch, partitions):
    _fake(monkeypatch, _PlainState)
    ex = NGramExtractor(max_n=2, min_freq=3, max_f_grams=9).fit_gpu(iter(CORPUS), verbose=False, chunk_tokens=4,
                                                                     partitions=partitions)
    assert len(ex) == 0
    assert _PlainState.log == [("open",), ("update", [1, 2, 3, 4], [0, 3, 3, 4]), ("update", [5, 6, 7, 8, 9], [0, 5]),
                               ("update", [10], [0, 1]), ("finalize", 3, 9), ("close",)]


def test_three_partitions_make_three_passes_then_merge_then_finalise(monkeypatch):
    _fake(monkeypatch, _PartState)
    ex = NGramExtractor(max_n=1, min_freq=3, max_f_grams=9).fit_gpu(CORPUS, verbose=False, chunk_tokens=4, partitions=3)
    chunks = [([1, 2, 3, 4], [0, 3, 3, 4]), ([5, 6, 7, 8, 9], [0, 5]), ([10], [0, 1])]
    want = []
    for p in range(3):                                                     # a fresh state per part, closed before the next
        want += [("open", p)] + [("update", p, p, 3, t, o) for t, o in chunks] + [("finalize", p, 3, 9, True), ("close", p)]
    want += [("open", 3)] + [("merge", 3, [[p]], [1], [1], [100 + p]) for p in range(3)]
    want += [("finalize", 3, 3, 9, False), ("close", 3)]
    assert _PartState.log == want
    assert ex.key_arrays()[0].tolist() == [[3]] and ex.counts.dtype == np.uint64


def test_a_callable_corpus_gives_every_pass(monkeypatch):
    _fake(monkeypatch, _PartState)
    calls = []

    def corpus():
        calls.append(1)
        return iter(CORPUS)                                                # a one-shot iterator per call is enough

    NGramExtractor(max_n=1).fit_gpu(corpus, verbose=False, chunk_tokens=100, partitions=2)
    assert len(calls) == 2
    assert [e[:4] for e in _PartState.log if e[0] == "update"] == [("update", 0, 0, 2), ("update", 1, 1, 2)]


def test_a_one_shot_iterator_is_refused_before_any_state_is_opened(monkeypatch):
    _fake(monkeypatch, _PartState)
    with pytest.raises(TypeError):
        NGramExtractor(max_n=1).fit_gpu((t for t in CORPUS), verbose=False, chunk_tokens=4, partitions=2)
    with pytest.raises(TypeError):
        NGramExtractor(max_n=1).fit_gpu(iter(CORPUS), verbose=False, chunk_tokens=4, partitions=2)
    assert _PartState.log == [] and _PartState.opened == 0


def test_a_corpus_that_changes_between_passes_is_an_error(monkeypatch):
    _fake(monkeypatch, _PartState)
    calls = []

    def corpus():
        calls.append(1)
        return CORPUS if len(calls) == 1 else CORPUS[:-1]

    with pytest.raises(RuntimeError, match="the corpus changed between passes"):
        NGramExtractor(max_n=1).fit_gpu(corpus, verbose=False, chunk_tokens=4, partitions=2)
    assert not any(e[0] == "merge" for e in _PartState.log)


def test_partitions_need_chunk_tokens_and_at_least_one_part(monkeypatch):
    _fake(monkeypatch, _PartState)
    with pytest.raises(ValueError):
        NGramExtractor(max_n=1).fit_gpu(CORPUS, verbose=False, partitions=2)
    with pytest.raises(ValueError):
        NGramExtractor(max_n=1).fit_gpu(CORPUS, verbose=False, partitions=1)
    with pytest.raises(ValueError):
        NGramExtractor(max_n=1).fit_gpu(CORPUS, verbose=False, chunk_tokens=4, partitions=0)
    assert _PartState.log == []
