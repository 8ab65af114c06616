"""CPU: the dense-base entry points (`scone_embed_base`, `scone_embed_base_varlen`) exist in the header, the binding and the
built library, refuse a null handle, and `EmbeddingCache.embed_tokens(base=...)` raises its `ValueError`s before any device
work (this file runs on a machine without a GPU)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from scone_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scone_embed_base", "scone_embed_base_varlen")


def _header():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_and_exported(name):
    assert re.search(r"\bint\s+%s\s*\(" % name, _header()), f"{name} is not declared in include/scone_hip.h"
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)


def test_signatures_are_the_wte_calls_without_the_vocabulary():
    """d_base takes the place of (d_wte, vocab): one pointer for a pointer and an int64."""
    for base, wte in (("scone_embed_base", "scone_embed"), ("scone_embed_base_varlen", "scone_embed_varlen")):
        res_b, args_b = _lib.SIGNATURES[base]
        res_w, args_w = _lib.SIGNATURES[wte]
        assert res_b is res_w and len(args_b) == len(args_w) - 1
        k = {"scone_embed": 5, "scone_embed_varlen": 6}[wte]                # position of `vocab`
        assert args_w[k] is _lib._I64 and args_w[k - 1] is _lib._P
        assert list(args_b) == list(args_w[:k]) + list(args_w[k + 1:])
    decl = re.search(r"int\s+scone_embed_base\s*\(([^)]*)\)", _header()).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "d_tok", "B", "T", "d_base", "d_wpe", "n_pos", "d_pos", "reduce", "d_out", "out_dtype", "stream"]
    decl = re.search(r"int\s+scone_embed_base_varlen\s*\(([^)]*)\)", _header()).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "d_tok", "d_cu_seqlens", "n_seqs", "total_tokens", "d_base", "d_wpe", "n_pos", "d_pos", "reduce", "d_out",
        "out_dtype", "stream"]


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 2 and _lib.lib().scone_abi_version() == 2
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", _header())


def test_null_handle_is_einval():
    lib = _lib.lib()
    buf = (C.c_int32 * 8)()
    p = C.cast(buf, C.c_void_p)
    assert lib.scone_embed_base(None, p, 1, 4, p, None, 0, None, _lib.REDUCE_MEAN, p, _lib.DT_F32, None) == _lib.EINVAL
    assert lib.scone_embed_base(None, None, 0, 0, None, None, 0, None, _lib.REDUCE_MEAN, None, _lib.DT_F32, None) == _lib.EINVAL
    assert lib.scone_embed_base_varlen(None, p, p, 1, 4, p, None, 0, None, _lib.REDUCE_MEAN, p, _lib.DT_F32, None) == _lib.EINVAL
    assert lib.scone_embed_base_varlen(None, None, None, 0, 0, None, None, 0, None, _lib.REDUCE_MEAN, None, _lib.DT_F32,
                                       None) == _lib.EINVAL


def test_scone_table_has_the_methods():
    from scone_amd.hip_backend import SconeTable
    for name in ("embed_base", "embed_base_varlen", "match_csr", "gather_reduce"):
        assert callable(getattr(SconeTable, name))


# ------------------------------------------------------------------ EmbeddingCache.embed_tokens(base=...): host-side refusals
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


def test_wrong_base_shape_is_refused_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    tok = torch.zeros((2, 5), dtype=torch.int32)
    for shape in ((2, 5, 24), (5, 2, 16), (10, 16), (2, 5)):
        with pytest.raises(ValueError, match="base must be"):
            cache.embed_tokens(tok, base=torch.zeros(shape))
    with pytest.raises(ValueError, match="base must be"):
        cache.embed_tokens(torch.zeros(5, dtype=torch.int32), base=torch.zeros(5, 16))      # [T] ids: base is [1, T, d]


def test_wte_together_with_base_is_refused_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    with pytest.raises(ValueError, match="base="):
        cache.embed_tokens(torch.zeros((2, 5), dtype=torch.int32), base=torch.zeros(2, 5, 16), wte=torch.zeros(4, 16))


def test_packed_base_must_be_total_by_d_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    tok = torch.zeros(8, dtype=torch.int32)
    for shape in ((1, 8, 16), (8, 24), (7, 16), (2, 4, 16)):
        with pytest.raises(ValueError, match="base="):
            cache.embed_tokens(tok, cu_seqlens=[0, 3, 8], base=torch.zeros(shape))
    with pytest.raises(ValueError, match="base="):                              # the right shape, but not on the device
        cache.embed_tokens(tok, cu_seqlens=[0, 3, 8], base=torch.zeros(8, 16))
    with pytest.raises(ValueError, match="1-D"):
        cache.embed_tokens(tok.view(2, 4), cu_seqlens=[0, 3, 8], base=torch.zeros(8, 16))


def test_longest_suffix_cache_refuses_the_new_keywords_before_device_work(monkeypatch):
    cache = _cache(monkeypatch, mode="longest_suffix")
    tok, base = torch.zeros((2, 5), dtype=torch.int32), torch.zeros(2, 5, 16)
    for kw in (dict(wpe=torch.zeros(8, 16)), dict(position_ids=torch.zeros((2, 5), dtype=torch.int64)), dict(out=torch.zeros(2, 5, 16))):
        with pytest.raises(ValueError, match="table.embed_base"):
            cache.embed_tokens(tok, base=base, **kw)
    with pytest.raises(ValueError, match="table.embed_base"):
        cache.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8], base=torch.zeros(8, 16))
    with pytest.raises(_NoDevice):                                               # the plain call still takes its road
        cache.embed_tokens(tok, base=base)


def test_a_valid_call_reaches_the_device(monkeypatch):
    """The control of the refusals above: well-formed arguments get as far as the device table."""
    cache = _cache(monkeypatch)
    with pytest.raises(_NoDevice):
        cache.embed_tokens(torch.zeros((2, 5), dtype=torch.int32), base=torch.zeros(2, 5, 16), wpe=torch.zeros(8, 16))
