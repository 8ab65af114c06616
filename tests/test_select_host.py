"""CPU: `scone_embed_select` exists in the header, the binding and the built library with the argument order the header
documents, refuses a null handle, leaves the ABI version alone; `SconeTable.embed_select` exists;
`EmbeddingCache.embed_tokens(select=...)` raises its `ValueError`s before any device work; `EmbeddingCache.last_positions`
equals a plain Python loop (this file runs on a machine without a GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from scone_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "scone_embed_select"


def _header():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_declared_bound_and_exported():
    assert re.search(r"\bint\s+%s\s*\(" % NAME, _header()), f"{NAME} is not declared in include/scone_hip.h"
    assert NAME in _lib.SIGNATURES
    assert hasattr(_lib.lib(), NAME)


def test_argument_order_of_the_header_and_the_binding():
    decl = re.search(r"int\s+%s\s*\(([^)]*)\)" % NAME, _header()).group(1)
    args = [a.strip() for a in decl.split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == [
        "h", "d_tok", "total_tokens", "T", "d_cu_seqlens", "n_seqs", "d_sel", "n_sel", "d_wte", "vocab", "d_base", "d_wpe",
        "n_pos", "d_pos", "reduce", "d_out", "out_dtype", "stream"]
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == len(args)
    for text, ct in zip(args, argtypes):
        if "*" in text or text.startswith("scone_stream_t"):
            assert ct is _lib._P, text
        elif text.startswith("int64_t"):
            assert ct is _lib._I64, text
        else:
            assert text.startswith("int32_t") and ct is _lib._I32, text
    # the last declaration of the header: the entry point was appended
    names = re.findall(r"\bint\s+(scone_\w+)\s*\(", _header())
    assert names[-1] == NAME


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 2 and _lib.lib().scone_abi_version() == 2
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", _header())


def test_null_handle_is_einval():
    lib = _lib.lib()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.scone_embed_select(None, p, 8, 4, None, 0, p, 2, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, p,
                                  _lib.DT_F32, None) == _lib.EINVAL
    assert lib.scone_embed_select(None, p, 8, 0, p, 2, p, 2, None, 0, p, None, 0, None, _lib.REDUCE_MEAN, p, _lib.DT_F16,
                                  None) == _lib.EINVAL
    assert lib.scone_embed_select(None, None, 0, 0, None, 0, None, 0, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, None,
                                  _lib.DT_F32, None) == _lib.EINVAL


def test_scone_table_has_the_method():
    from scone_amd.hip_backend import SconeTable
    assert callable(getattr(SconeTable, "embed_select"))


# ------------------------------------------------------------------ EmbeddingCache.embed_tokens(select=...): host-side refusals
class _NoDevice(Exception):
    pass


def _cache(monkeypatch, mode="cover", d=16):
    """A cache whose device table must never be asked for."""
    from scone_amd import EmbeddingCache, NGramExtractor
    keys = np.asarray([[1, 0], [1, 2]], dtype=np.uint32)
    lens = np.asarray([1, 2], dtype=np.uint8)
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=2), d, lookup_mode=mode)
    cache.cache_embeddings([0, 1], torch.zeros(2, d), verbose=False)

    def boom(*a, **k):
        raise _NoDevice("device work before the argument check")
    monkeypatch.setattr(cache, "to_device", boom)
    return cache


def test_select_refusals_come_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    tok = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        cache.embed_tokens(torch.zeros(10, dtype=torch.int32), select=[1, 2])             # 1-D ids without cu_seqlens
    with pytest.raises(ValueError, match="1-D packed"):
        cache.embed_tokens(tok, cu_seqlens=[0, 3, 10], select=[1, 2])
    with pytest.raises(ValueError, match="end at"):
        cache.embed_tokens(torch.zeros(10, dtype=torch.int32), cu_seqlens=[0, 3, 9], select=[1, 2])
    with pytest.raises(ValueError, match="1-D list"):
        cache.embed_tokens(tok, select=[[1, 2], [3, 4]])
    with pytest.raises(ValueError, match="integers"):
        cache.embed_tokens(tok, select=[0.5, 1.0])
    with pytest.raises(ValueError, match="integers"):
        cache.embed_tokens(tok, select=torch.tensor([0.5, 1.0]))
    for shape in ((2, 5, 16), (10, 16), (3, 24), (2, 16)):
        with pytest.raises(ValueError, match="base="):
            cache.embed_tokens(tok, select=[9, 4, 4], base=torch.zeros(shape))
    with pytest.raises(ValueError, match="base="):
        cache.embed_tokens(tok, select=[9, 4], base=torch.zeros(2, 16), wte=torch.zeros(4, 16))
    with pytest.raises(ValueError, match="position_ids="):
        cache.embed_tokens(tok, select=[9, 4], wpe=torch.zeros(8, 16), position_ids=torch.zeros((2, 5), dtype=torch.int64))
    with pytest.raises(ValueError, match="out="):
        cache.embed_tokens(tok, select=[9, 4], out=torch.zeros(2, 5, 16))


def test_longest_suffix_cache_refuses_base_with_select_before_device_work(monkeypatch):
    cache = _cache(monkeypatch, mode="longest_suffix")
    tok = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="table.embed_select"):
        cache.embed_tokens(tok, select=[9, 4], base=torch.zeros(2, 16))
    with pytest.raises(_NoDevice):                                               # without base= the call takes its road
        cache.embed_tokens(tok, select=[9, 4], wpe=torch.zeros(8, 16))


def test_a_valid_call_reaches_the_device(monkeypatch):
    """The control of the refusals above: well-formed arguments get as far as the device table."""
    cache = _cache(monkeypatch)
    tok = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(_NoDevice):
        cache.embed_tokens(tok, select=[9, 4, 4], base=torch.zeros(3, 16), wpe=torch.zeros(8, 16),
                           position_ids=torch.tensor([1, 2, 3]))
    with pytest.raises(_NoDevice):
        cache.embed_tokens(torch.zeros(10, dtype=torch.int32), cu_seqlens=[0, 3, 10], select=np.asarray([9, 2]))
    with pytest.raises(_NoDevice):
        cache.embed_tokens(tok, select=torch.tensor([], dtype=torch.int64))


# ------------------------------------------------------------------ last_positions
def _last_positions_loop(cu, k):
    out = []
    for s in range(len(cu) - 1):
        lo, hi = int(cu[s]), int(cu[s + 1])
        for p in range(max(lo, hi - k), hi):
            out.append(p)
    return out


@pytest.mark.parametrize("k", [1, 2, 4, 7, 100])
def test_last_positions_equals_a_plain_loop(k):
    from scone_amd import EmbeddingCache
    rng = np.random.default_rng(k)
    cases = [[0], [0, 0, 0], [0, 5], [0, 0, 1, 1, 4, 4, 4, 30, 30], [0, 3, 3, 3]]
    cases.append(np.concatenate([[0], np.cumsum(rng.integers(0, 9, size=200))]).tolist())
    for cu in cases:
        want = _last_positions_loop(cu, k)
        for form in (cu, np.asarray(cu, dtype=np.int64), torch.tensor(cu, dtype=torch.int32)):
            got = EmbeddingCache.last_positions(form, k)
            assert got.dtype == torch.int32 and got.dim() == 1 and not got.is_cuda
            assert got.tolist() == want, (cu[:12], k)
    lens = np.diff(cases[-1])
    assert (lens == 0).any() and lens.max() == 8 and (lens == 1).any()            # empty sequences; k = 2.. is longer than some, k = 100 than all


@pytest.mark.parametrize("B,T,k", [(1, 1, 1), (3, 5, 1), (3, 5, 2), (4, 2, 3), (0, 7, 1), (5, 0, 2), (64, 512, 4)])
def test_last_positions_of_a_rectangle(B, T, k):
    from scone_amd import EmbeddingCache
    want = _last_positions_loop([b * T for b in range(B + 1)], k)
    assert EmbeddingCache.last_positions((B, T), k).tolist() == want
    assert EmbeddingCache.last_positions(torch.Size((B, T)), k).tolist() == want
    assert EmbeddingCache.last_positions((B, T)).tolist() == _last_positions_loop([b * T for b in range(B + 1)], 1)


def test_last_positions_refusals():
    from scone_amd import EmbeddingCache
    with pytest.raises(ValueError, match="k must"):
        EmbeddingCache.last_positions([0, 3], 0)
    with pytest.raises(ValueError, match="decrease"):
        EmbeddingCache.last_positions([0, 5, 3], 1)
    with pytest.raises(ValueError, match="start at 0"):
        EmbeddingCache.last_positions([1, 5], 1)
    with pytest.raises(ValueError):
        EmbeddingCache.last_positions((1, 2, 3), 1)
