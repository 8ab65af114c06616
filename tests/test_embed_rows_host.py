"""CPU: the live-row entry points (`scone_embed_rows`, `scone_embed_rows_varlen`) exist in the header, the binding and the built
library and refuse a null handle; `SconeTable.embed_rows`, `EmbeddingCache.live_rows` and `EmbeddingCache.bake` raise their
refusals before any device work; and tests/embed_rows_fixture.py, the host statement of the contract that the GPU tests compare
against, agrees with the oracle where every row is listed and differs from its deliberately wrong twin where ids are unlisted
(this file runs on a machine without a GPU)."""

import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R
from scone_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import embed_rows_fixture as ER  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("scone_embed_rows", "scone_embed_rows_varlen")


def _header():
    text = open(os.path.join(ROOT, "include", "scone_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", NAMES)
def test_declared_bound_and_exported(name):
    assert re.search(r"\bint\s+%s\s*\(" % name, _header()), f"{name} is not declared in include/scone_hip.h"
    assert name in _lib.SIGNATURES
    assert hasattr(_lib.lib(), name)


def test_signatures_and_struct_follow_the_header():
    decl = re.search(r"int\s+scone_embed_rows\s*\(([^)]*)\)", _header()).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "live", "d_tok", "B", "T", "d_wte", "vocab", "d_base", "d_wpe", "n_pos", "d_pos", "reduce", "d_out", "out_dtype", "stream"]
    decl = re.search(r"int\s+scone_embed_rows_varlen\s*\(([^)]*)\)", _header()).group(1)
    assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == [
        "h", "live", "d_tok", "d_cu_seqlens", "n_seqs", "total_tokens", "d_wte", "vocab", "d_base", "d_wpe", "n_pos", "d_pos",
        "reduce", "d_out", "out_dtype", "stream"]
    assert len(_lib.SIGNATURES["scone_embed_rows"][1]) == 15 and len(_lib.SIGNATURES["scone_embed_rows_varlen"][1]) == 16
    body = re.search(r"typedef\s+struct\s+scone_live_rows\s*\{([^}]*)\}", _header()).group(1)
    fields = [f.split()[-1].lstrip("*") for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in _lib.SconeLiveRows._fields_] == ["struct_size", "dtype", "d_row_ids", "d_rows", "n", "d_n"]
    assert C.sizeof(_lib.SconeLiveRows) == 40 and _lib.LIVE_ROWS_MAX == 2**31 - 1


def test_abi_version_is_unchanged():
    assert _lib.ABI_VERSION == 2 and _lib.lib().scone_abi_version() == 2
    assert re.search(r"#define\s+SCONE_ABI_VERSION\s+2\b", _header())


def test_null_handle_is_einval():
    lib = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p)
    live = _lib.SconeLiveRows(C.sizeof(_lib.SconeLiveRows), _lib.DT_F32, p, p, 1, None)
    assert lib.scone_embed_rows(None, C.byref(live), p, 1, 4, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, p, _lib.DT_F32,
                                None) == _lib.EINVAL
    assert lib.scone_embed_rows(None, None, None, 0, 0, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, None, _lib.DT_F32,
                                None) == _lib.EINVAL
    assert lib.scone_embed_rows_varlen(None, C.byref(live), p, p, 1, 4, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, p,
                                       _lib.DT_F32, None) == _lib.EINVAL
    assert lib.scone_embed_rows_varlen(None, None, None, None, 0, 0, None, 0, None, None, 0, None, _lib.REDUCE_MEAN, None,
                                       _lib.DT_F32, None) == _lib.EINVAL


def test_exported_from_the_package():
    import scone_amd
    from scone_amd.hip_backend import SconeTable
    assert "LiveFGramBatch" in scone_amd.__all__ and callable(scone_amd.LiveFGramBatch)
    assert callable(SconeTable.embed_rows)
    for name in ("f_gram_keys", "live_rows", "bake"):
        assert callable(getattr(scone_amd.EmbeddingCache, name))


# ------------------------------------------------------------------ refusals before device work
class _NoDevice(Exception):
    pass


class _Table:
    """`SconeTable.embed_rows` on an object whose device (the first thing the device work asks for) must never be asked for."""
    dim = 16

    @property
    def device(self):
        raise _NoDevice("device work before the argument check")

    def embed_rows(self, *a, **k):
        from scone_amd.hip_backend import SconeTable
        return SconeTable.embed_rows(self, *a, **k)


def _args(U=3, d=16, B=2, T=5):
    return torch.zeros((B, T), dtype=torch.int32), torch.arange(U, dtype=torch.int64), torch.zeros(U, d)


def test_table_embed_rows_refuses_before_device_work():
    from scone_amd.hip_backend import SconeInvalidArgument
    t = _Table()
    tok, ids, rows = _args()
    with pytest.raises(SconeInvalidArgument, match="exclusive"):
        t.embed_rows(tok, ids, rows, wte=torch.zeros(4, 16), base=torch.zeros(2, 5, 16))
    for bad in (torch.zeros(3, 24), torch.zeros(4, 16), torch.zeros(3, 16, 1), torch.zeros(48)):
        with pytest.raises(SconeInvalidArgument, match="rows must be"):
            t.embed_rows(tok, ids, bad)
    for bad in (torch.zeros(3, 16, dtype=torch.float64), torch.zeros(3, 16, dtype=torch.int32)):
        with pytest.raises(SconeInvalidArgument, match="rows must be float32, float16 or bfloat16"):
            t.embed_rows(tok, ids, bad)
    for bad in (ids.to(torch.int32), ids.float(), ids.view(3, 1)):
        with pytest.raises(SconeInvalidArgument, match="row_ids must be"):
            t.embed_rows(tok, bad, rows)
    packed = torch.zeros(8, dtype=torch.int32)
    for shape in ((1, 8, 16), (8, 24), (7, 16), (2, 4, 16)):
        with pytest.raises(SconeInvalidArgument, match="base must hold"):
            t.embed_rows(packed, ids, rows, cu_seqlens=[0, 3, 8], base=torch.zeros(shape))
    with pytest.raises(SconeInvalidArgument, match="1-D"):
        t.embed_rows(packed.view(2, 4), ids, rows, cu_seqlens=[0, 3, 8])
    with pytest.raises(SconeInvalidArgument, match="cu_seqlens"):
        t.embed_rows(packed, ids, rows, cu_seqlens=[0, 9, 8])
    with pytest.raises(SconeInvalidArgument, match="reduce"):
        t.embed_rows(tok, ids, rows, reduce="max")
    with pytest.raises(SconeInvalidArgument, match="n must be"):
        t.embed_rows(tok, ids, rows, n=3)
    with pytest.raises(_NoDevice):                                   # the control: a valid call reaches the device
        t.embed_rows(tok, ids, rows)
    with pytest.raises(_NoDevice):
        t.embed_rows(packed, ids, rows, cu_seqlens=[0, 3, 8], reduce="sum")


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


def test_live_rows_refuses_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    with pytest.raises(ValueError, match="1-D"):
        cache.live_rows(torch.zeros((2, 4), dtype=torch.int32), cu_seqlens=[0, 3, 8])
    with pytest.raises(ValueError, match="cu_seqlens"):
        cache.live_rows(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 7])
    with pytest.raises(ValueError, match="input_ids must be"):
        cache.live_rows(torch.zeros((2, 2, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="integers"):
        cache.live_rows(torch.zeros((2, 4)))
    with pytest.raises(ValueError, match="% 8"):
        _cache(monkeypatch, d=12).live_rows(torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(_NoDevice):                                   # the control
        cache.live_rows(torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(_NoDevice):
        cache.live_rows(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8])


def test_bake_refuses_before_device_work(monkeypatch):
    cache = _cache(monkeypatch)
    with pytest.raises(ValueError, match="callable"):
        cache.bake(torch.zeros(2, 16))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="chunk_rows"):
            cache.bake(lambda t, n: torch.zeros(len(n), 16), chunk_rows=bad)
    with pytest.raises(_NoDevice):                                   # the control
        cache.bake(lambda t, n: torch.zeros(len(n), 16), chunk_rows=1)


def test_f_gram_keys_are_built_from_the_key_arrays_and_cached(monkeypatch):
    cache = _cache(monkeypatch)
    tokens, lens = cache.f_gram_keys("cpu")
    assert tokens.dtype == torch.int64 and lens.dtype == torch.int64
    assert tokens.tolist() == [[1, 0], [1, 2]] and lens.tolist() == [1, 2]
    again = cache.f_gram_keys("cpu")
    assert again[0] is tokens and again[1] is lens
    from scone_amd import EmbeddingCache, NGramExtractor
    dirty = np.asarray([[5, 9], [1, 2]], dtype=np.uint32)            # a key array with leftovers beyond lens
    c2 = EmbeddingCache(NGramExtractor.from_arrays(dirty, np.asarray([1, 2], dtype=np.uint8), max_n=2), 16)
    assert c2.f_gram_keys("cpu")[0].tolist() == [[5, 0], [1, 2]]


# ------------------------------------------------------------------ the fixture itself
def _world(max_n=3, B=3, T=13, d=8):
    keys, lens, tok = ER.batch(max_n, B, T)
    table = np.random.default_rng(5).standard_normal((len(lens), d)).astype(np.float32)
    return keys, lens, tok, table


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_fixture_equals_the_oracle_when_every_row_is_listed(reduce):
    keys, lens, tok, table = _world()
    n = table.shape[0]
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, 3))
    want = R.embed_numpy(table, off, ids, reduce)
    got = ER.expected(keys, lens, 3, n, tok, None, np.arange(n), table, "cover", reduce)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), (np.float32(0) + want).view(np.uint32))
    live = np.unique(ids)                                           # only the rows the batch hits: the same answer
    got = ER.expected(keys, lens, 3, n, tok, None, live, table[live], "cover", reduce)
    assert np.array_equal(got.view(np.uint32), (np.float32(0) + want).view(np.uint32))
    cu = np.asarray([0, 13, 13, 14, 39])                            # packed: an empty and a one-token sequence
    offp, idsp = ER.lists(keys, lens, 3, tok.reshape(-1), cu)
    assert len(offp) == 40 and offp[-1] == len(idsp) and not np.array_equal(offp, off)
    f2id = R._key_dict(keys, lens)
    rows, matched = ER.fgram(keys, lens, 3, tok, None, table, "longest_suffix", reduce)
    assert np.array_equal(rows, R.paper_embed(f2id, 3, tok, table).reshape(-1, 8)) and 0 < matched.sum() < matched.size


def test_the_wrong_model_differs_on_the_unlisted_id_batch():
    """The batch and the dropped ids of tests/test_gpu_embed_rows.py's unlisted-id test: every third id, the first and the last."""
    keys, lens, tok, table = _world()
    n = table.shape[0]
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, 3))
    live = np.unique(ids)
    listed = ER.unlisted(live)
    assert len(listed) < len(live) - 2 and live[0] not in listed and live[-1] not in listed
    right = ER.expected(keys, lens, 3, n, tok, None, listed, table[listed], "cover", "mean")
    wrong = ER.wrong_model_drops_unlisted(keys, lens, 3, n, tok, None, listed, table[listed], "mean")
    assert not np.array_equal(right, wrong)
    k = np.diff(off)
    partly = np.asarray([0 < np.isin(ids[off[p]:off[p + 1]], listed).sum() < k[p] for p in range(len(k))])
    assert partly.any() and (np.abs(right[partly]) < np.abs(wrong[partly])).any()      # the contract keeps the full divisor
    all_listed = ER.wrong_model_drops_unlisted(keys, lens, 3, n, tok, None, live, table[live], "mean")
    assert np.array_equal(all_listed, ER.expected(keys, lens, 3, n, tok, None, live, table[live], "cover", "mean"))
