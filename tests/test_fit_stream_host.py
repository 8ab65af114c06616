"""CPU: the streaming fit (scone_fit_create / _update / _stats / _finalize / _export / _merge / _destroy) is declared, bound and
exported; its refusals that need no device; `fit_occurrences`; the chunk planner of `NGramExtractor.fit_gpu(chunk_tokens=...)`."""

import ctypes as C
import os
import re

import numpy as np
import pytest

from scone_amd import NGramExtractor, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["scone_fit_create", "scone_fit_destroy", "scone_fit_update", "scone_fit_stats", "scone_fit_finalize", "scone_fit_export",
         "scone_fit_merge"]


def _header():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    return re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)     # comments blanked, positions kept


# ------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_and_exported_with_matching_arguments(name):
    m = re.search(r"\b(int|void)\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/scone_hip.h"
    args = [a.strip() for a in m.group(2).split(",")]
    res, argtypes = _lib.SIGNATURES[name]
    assert res is (C.c_int if m.group(1) == "int" else None)
    assert len(argtypes) == len(args), name
    for text, ct in zip(args, argtypes):
        if "**" in text:                                       # the created state
            assert ct is C.POINTER(_lib._P), text
        elif text.startswith("uint64_t *h_") or (name == "scone_fit_stats" and text.startswith("uint64_t *")):
            assert ct is C.POINTER(_lib._U64), text            # host results
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
    assert names("scone_fit_create") == ["device", "max_n", "initial_slots", "out"]
    assert names("scone_fit_update") == ["st", "d_tokens", "n_tokens", "d_text_offsets", "n_texts", "seq_base", "stream"]
    assert names("scone_fit_stats") == ["st", "n_distinct", "n_occurrences", "slots", "n_grows", "next_seq"]
    assert names("scone_fit_finalize") == ["st", "min_freq", "max_f_grams", "d_keys_out", "d_lens_out", "d_counts_out", "out_cap",
                                           "h_n_out", "stream"]
    assert names("scone_fit_export") == ["st", "d_keys_out", "d_lens_out", "d_counts_out", "d_first_out", "out_cap", "h_n_out",
                                         "stream"]
    assert names("scone_fit_merge") == ["st", "d_keys", "d_lens", "d_counts", "d_first", "n", "stream"]


def test_declared_between_scone_fit_and_the_table_section():
    raw = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    h = _header()
    lo = re.search(r"\bint\s+scone_fit\s*\(", h).start()
    hi = raw.index("/* ---- table: rows")
    assert lo < hi
    for name in NAMES:
        pos = re.search(r"\b%s\s*\(" % name, h).start()
        assert lo < pos < hi, name
    assert re.search(r"typedef\s+struct\s+scone_fit_state\s+scone_fit_state\s*;", h)
    assert re.findall(r"\bint\s+(scone_\w+)\s*\(", h)[-1] == "scone_embed_select"


def test_abi_version_is_still_2():
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", _header())
    assert _lib.ABI_VERSION == 2 and _lib.lib().scone_abi_version() == 2


def test_null_state_and_bad_create_arguments_without_device_work():
    lib = _lib.lib()
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    n = C.c_uint64(7)
    assert lib.scone_fit_update(None, p, 2, p, 1, 0, None) == _lib.EINVAL
    assert lib.scone_fit_finalize(None, 1, 10, p, p, p, 4, C.byref(n), None) == _lib.EINVAL
    assert lib.scone_fit_export(None, p, p, p, p, 4, C.byref(n), None) == _lib.EINVAL
    assert lib.scone_fit_merge(None, p, p, p, p, 1, None) == _lib.EINVAL
    assert lib.scone_fit_stats(None, C.byref(n), None, None, None, None) == _lib.EINVAL
    assert n.value == 7
    lib.scone_fit_destroy(None)                                            # no-op
    st = C.c_void_p(0)
    assert lib.scone_fit_create(0, 0, 0, C.byref(st)) == _lib.EINVAL and not st.value
    assert lib.scone_fit_create(0, 5, 0, C.byref(st)) == _lib.EINVAL and not st.value
    assert lib.scone_fit_create(0, 3, 0, None) == _lib.EINVAL


# ------------------------------------------------------------------ fit_occurrences
def test_fit_occurrences_equals_a_brute_force_count():
    from scone_amd.hip_backend import fit_occurrences
    for max_n in range(1, 5):
        ex = NGramExtractor(max_n=max_n)
        per_len = [len(ex.extract_all_n_grams(list(range(L)))) for L in range(10)]
        for L in range(10):
            assert fit_occurrences([L], max_n) == per_len[L], (L, max_n)
        assert fit_occurrences(range(10), max_n) == sum(per_len)
        assert fit_occurrences([], max_n) == 0
        assert fit_occurrences(np.array([9, 0, 3, 1]), max_n) == per_len[9] + per_len[0] + per_len[3] + per_len[1]


# ------------------------------------------------------------------ the chunk planner
class _FakeState:
    """Stands in for hip_backend.FitState: records every update and how far the corpus generator had been advanced."""
    log = None

    def __init__(self, max_n, device=None, initial_slots=0):
        self.max_n = max_n

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass

    def update(self, tokens, text_offsets, seq_base=None):
        assert seq_base is None
        _FakeState.log.append((np.array(tokens), np.array(text_offsets), _FakeState.pulled[0]))

    def finalize(self, min_freq, max_f_grams):
        return (np.zeros((0, self.max_n), dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64), 0)


def _plan(monkeypatch, corpus, chunk_tokens, max_n=3):
    from scone_amd import hip_backend
    monkeypatch.setattr(hip_backend, "FitState", _FakeState)
    _FakeState.log, _FakeState.pulled = [], [0]

    def gen():
        for t in corpus:
            _FakeState.pulled[0] += 1
            yield t

    ex = NGramExtractor(max_n=max_n, min_freq=1).fit_gpu(gen(), verbose=False, chunk_tokens=chunk_tokens)
    return ex, _FakeState.log


CORPUS = [[1, 2, 3], [], [4], [5, 6, 7, 8, 9, 10, 11, 12, 13], [], [], [14, 15], [16], [17, 18, 19, 20], [], [21]]


@pytest.mark.parametrize("chunk_tokens", [1, 2, 4, 5, 7, 10**9])
def test_chunk_planner_hands_over_whole_texts_lazily(monkeypatch, chunk_tokens):
    ex, log = _plan(monkeypatch, CORPUS, chunk_tokens)
    assert len(ex) == 0 and ex.counts.dtype == np.uint64
    texts_seen, first = [], True
    for k, (tok, off, pulled) in enumerate(log):
        assert tok.dtype == np.int32 and off.dtype == np.int64
        assert off[0] == 0 and off[-1] == tok.size and (np.diff(off) >= 0).all()
        texts = [tok[off[i]:off[i + 1]].tolist() for i in range(off.size - 1)]
        if k < len(log) - 1:
            assert tok.size >= chunk_tokens                                # a full chunk ...
            assert tok.size - len(texts[-1]) < chunk_tokens                # ... closed by the text that filled it
        texts_seen += texts
        assert pulled == len(texts_seen)                                   # nothing pulled beyond this chunk's texts
        if first:
            assert pulled == len(texts)
            first = False
    assert texts_seen == CORPUS                                            # whole texts, in order, empty ones in place
    if chunk_tokens == 10**9:
        assert len(log) == 1
    if chunk_tokens == 1:
        # every non-empty text closes a chunk; the empty ones travel in front of the next non-empty one
        assert [t.size for t, _, _ in log] == [3, 1, 9, 2, 1, 4, 1]
        assert log[1][1].tolist() == [0, 0, 1] and log[3][1].tolist() == [0, 0, 0, 2]


def test_chunk_planner_a_long_text_is_a_chunk_by_itself(monkeypatch):
    _, log = _plan(monkeypatch, [[1], list(range(50)), [2], [3]], 2)
    assert [t.size for t, _, _ in log] == [51, 2]
    _, log = _plan(monkeypatch, [list(range(50)), [2]], 4)
    assert [t.size for t, _, _ in log] == [50, 1]


def test_chunk_planner_trailing_empty_texts_and_an_empty_corpus(monkeypatch):
    _, log = _plan(monkeypatch, [[1, 2], [], []], 2)
    assert [(t.size, o.tolist()) for t, o, _ in log] == [(2, [0, 2]), (0, [0, 0, 0])]
    _, log = _plan(monkeypatch, [], 8)
    assert log == []


def test_chunk_planner_refuses_a_bad_token_before_the_update_of_its_chunk(monkeypatch):
    with pytest.raises(ValueError):
        _plan(monkeypatch, [[1, 2], [3, 4], [5, -6], [7]], 4)
    assert len(_FakeState.log) == 1 and _FakeState.log[0][0].tolist() == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        _plan(monkeypatch, [[1, 2**31 - 1]], 4)
    assert _FakeState.log == []
    with pytest.raises(ValueError):
        _plan(monkeypatch, [[1]], 0)


def test_chunk_tokens_none_keeps_the_one_shot_route(monkeypatch):
    """chunk_tokens=None must not touch FitState: it goes through hip_backend.fit_gpu (scone_fit) as before."""
    from scone_amd import hip_backend
    monkeypatch.setattr(hip_backend, "FitState", None)
    called = []

    def fake_fit_gpu(tokens, offsets, max_n, min_freq, max_f, device=None):
        called.append((tokens.tolist(), offsets.tolist(), max_n, min_freq, max_f))
        return (np.zeros((0, max_n), dtype=np.uint32), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint32), 0)

    monkeypatch.setattr(hip_backend, "fit_gpu", fake_fit_gpu)
    NGramExtractor(max_n=2, min_freq=3, max_f_grams=9).fit_gpu([[1, 2], [], [3]], verbose=False)
    assert called == [([1, 2, 3], [0, 2, 2, 3], 2, 3, 9)]
