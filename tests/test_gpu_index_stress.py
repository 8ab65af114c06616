"""Every f-gram matcher against a crowded, full, wide-token index.

The states come from tests/index_model.py (crowded buckets at load 0.75; tables filled to exactly their capacity of 4, 64 and 1024
slots with bitmap false positives in the batch; present / absent keys that differ only in `ext`; token ids around and far above
2^18 with a run that saturates the probe queue of a whole tile; duplicate keys spread over build chunks).  That each state IS what
its name says is proved on the CPU by tests/test_index_model_host.py, with a host model that is itself held to the product's
header -- nothing of that model is part of the expectation here.

The expectation is the oracle's (oracle/ref_port.py: Python dicts, no hashing scheme of ours): `R.match_hits` / `R.hits_to_csr`
for the id lists, `R.embed_numpy` for the vectors, `R.paper_embed` for the paper's lookup; a packed batch is every sequence
matched alone.  fp32 table with Gaussian rows, fp32 output, no wte (wide tokens have no row there), wpe at the default
positions: `(0 + f-gram part) + wpe[place in the sequence]`, compared bit for bit -- a wrong id, a missing id or a wrong order
changes bits.  Handles are `SconeTable`s with the state's explicit `index_capacity`.

The five pieces of device code that read the index, and what reaches them here:
  1 k_match (probe_index per thread)            match, match_csr
  2 k_match_ell<3/4> (stage_starts, resolve_queue, compact_record)
                                                 shard_gather_match (the raw records), embed with SCONE_FUSED_MAX_TOKENS=0, embed_partial
  3 k_match_ell_varlen<3/4>                      embed_varlen with SCONE_FUSED_MAX_TOKENS=0
  4 scone_lookup_key inside k_embed_fused        embed / embed_varlen in one launch (d = 768)
  5 scone_lookup_key inside the select kernel    embed_select, rectangular and packed
After every case `status()` is 0."""

import functools
import os
import sys
import types
import zlib

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

D = 768
GUARD = 64
STATES = [s[0] for s in M.states()]
PAPER_STATES = [s for s in STATES if s.startswith(("shared_lo", "wide")) and s.endswith(("n3", "n4"))]
CHUNK_ORDER = (2, 0, 1)                 # the order the three host chunks are submitted in


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@pytest.fixture(params=["one_launch", "two_kernels"])
def lookup_form(request, monkeypatch):
    """SCONE_FUSED_MAX_TOKENS is read when a handle is created: unset, batches up to 32768 tokens take the one-launch kernel
    (k_embed_fused: matcher 4); 0 sends every batch through k_match_ell / k_match_ell_varlen + k_embed_wave (matchers 2, 3)."""
    if request.param == "two_kernels":
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    else:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    return request.param


# ------------------------------------------------------------------ host only: inputs and the oracle's answers
def _lists(keys, lens, max_n, seqs):
    """CSR id lists over the concatenated positions of `seqs`, every sequence matched on its own."""
    offs, ids, base = [np.zeros(1, dtype=np.int64)], [], 0
    for seq in seqs:
        if len(seq) == 0:
            continue
        o, i = R.hits_to_csr(R.match_hits(keys, lens, np.asarray(seq, dtype=np.int64)[None, :], max_n))
        offs.append(o[1:] + base)
        ids.append(i)
        base += int(o[-1])
    return np.concatenate(offs), (np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name):
    max_n, keys, lens, capacity, batch, facts = M.state(name)
    c = types.SimpleNamespace(name=name, max_n=max_n, keys=keys, lens=lens, capacity=capacity, batch=batch, facts=facts, n=len(lens))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    c.table = rng.standard_normal((c.n, D)).astype(np.float32)
    B, T = batch.rect.shape
    seq_lens = np.diff(batch.cu)
    c.wpe = rng.standard_normal((max(T, int(seq_lens.max())), D)).astype(np.float32)
    c.hits = R.match_hits(keys, lens, batch.rect, max_n)
    c.off, c.ids = R.hits_to_csr(c.hits)
    c.ids = c.ids.astype(np.int64)
    c.pos = np.tile(np.arange(T), B)
    c.poff, c.pids = _lists(keys, lens, max_n, M.sequences(batch, "packed"))
    c.ppos = np.concatenate([np.arange(n) for n in seq_lens])
    assert len(c.off) == B * T + 1 and len(c.poff) == len(batch.packed) + 1
    assert len(c.ids) > 0 and len(c.pids) > 0
    return c


def _want(c, form, reduce="mean", own=None):
    off, ids, pos = (c.off, c.ids, c.pos) if form == "rect" else (c.poff, c.pids, c.ppos)
    fg = R.embed_numpy(c.table, off, ids, reduce)
    return ((np.float32(0) + fg) + c.wpe[pos]).astype(np.float32)


def _paper_want(c, form):
    f2id = R._key_dict(c.keys, c.lens)
    if form == "rect":
        return R.paper_embed(f2id, c.max_n, c.batch.rect, c.table, wpe=c.wpe).reshape(-1, D)
    rows = [R.paper_embed(f2id, c.max_n, np.asarray(s)[None, :], c.table, wpe=c.wpe)[0] for s in M.sequences(c.batch, "packed") if len(s)]
    return np.concatenate(rows)


# ------------------------------------------------------------------ handles
def _new(c, dim=D, **kw):
    from scone_amd.hip_backend import SconeTable
    return SconeTable(c.max_n, c.n, dim, "fp32", index_capacity=c.capacity, **kw)


def _store(t, c):
    if t.dim:
        t.store_f32(torch.from_numpy(c.table[t.row_begin:t.row_end]), row0=t.row_begin)
    return t


def _build_chunks(t, c):
    """(a) index_build in three host chunks, submitted in a shuffled order, with their true id0"""
    b = c.facts["chunk_bounds"]
    for k in CHUNK_ORDER:
        t.index_build(c.keys[b[k]:b[k + 1]], c.lens[b[k]:b[k + 1]], id0=b[k])
    return t


def _build_device(t, c):
    """(b) index_build_device: one launch over all keys"""
    keys = torch.from_numpy(c.keys.view(np.int32)).cuda().contiguous()
    lens = torch.from_numpy(c.lens).cuda().contiguous()
    t.index_build_device(keys, lens, id0=0)
    torch.cuda.synchronize()
    return t


def _handle(c, dim=D, **kw):
    return _store(_build_chunks(_new(c, dim, **kw), c), c)


def _guarded(n, dt=torch.float32, fill=float("nan"), width=D):
    buf = torch.full((n + GUARD, width), fill, dtype=dt, device="cuda")
    return buf, buf[:n]


def _same(got, want, tag):
    g = got.detach().cpu().numpy().reshape(want.shape)
    bad = np.argwhere((g.view(np.uint32) != want.view(np.uint32)).any(axis=1)).reshape(-1)
    assert len(bad) == 0, f"{tag}: {len(bad)} of {len(want)} rows differ from the oracle; first positions {bad[:8].tolist()}"


def _guard_ok(buf, n):
    tail = buf[n:]
    assert bool(torch.isnan(tail).all()) if tail.is_floating_point() else bool((tail == -7).all()), "a guard row behind the output was written"


def _tokens(c, form):
    if form == "rect":
        return torch.from_numpy(c.batch.rect), None
    return torch.from_numpy(c.batch.packed), torch.from_numpy(c.batch.cu.astype(np.int32))


def _records(t, c):
    """The raw k_match_ell records of the rectangle, all sequences: int32 [B * T, W]."""
    B, T = c.batch.rect.shape
    W = t.ell_width()
    assert W == (8 if c.max_n <= 3 else 16)
    buf, out = _guarded(B * T, torch.int32, -7, W)
    t.shard_gather_match(torch.from_numpy(c.batch.rect), 0, B, out)
    torch.cuda.synchronize()
    _guard_ok(buf, B * T)
    return out.cpu().numpy()


# ------------------------------------------------------------------ matcher 1: k_match
@pytest.mark.parametrize("name", STATES)
def test_match_and_match_csr(name):
    c = _case(name)
    t = _handle(c, dim=0)
    nk, cap, dups = t.index_stats()
    assert (nk, cap, dups) == (c.facts["n_distinct"], c.capacity, c.n - c.facts["n_distinct"])
    assert t.index_blob_sizes() == (16 * c.capacity, 4 * M.UNI_CAP, M.bloom_bits(c.capacity) // 8)
    tok = torch.from_numpy(c.batch.rect)
    hits = t.match(tok).cpu().numpy()
    assert np.array_equal(hits, c.hits), f"{name}: {int((hits != c.hits).sum())} window ids differ from the oracle"
    off, ids = t.match_csr(tok)
    assert np.array_equal(off.cpu().numpy(), c.off) and np.array_equal(ids.cpu().numpy(), c.ids)
    assert t.status() == 0


# ------------------------------------------------------------------ matcher 2: k_match_ell, the raw records
@pytest.mark.parametrize("name", STATES)
def test_tiled_match_records(name):
    """Per position: ids [0, K) equal the oracle's list in order, the count word is K | K << 8.  Unused words are not asserted."""
    c = _case(name)
    t = _handle(c, dim=0)
    rec = _records(t, c)
    W = rec.shape[1]
    K = np.diff(c.off)
    assert K.max() <= W - 2
    assert np.array_equal(rec[:, W - 2], K | (K << 8)), f"{name}: {int((rec[:, W - 2] != (K | (K << 8))).sum())} count words differ"
    want = np.full((len(K), W - 2), -1, dtype=np.int64)
    tix = np.repeat(np.arange(len(K)), K)
    want[tix, np.arange(len(c.ids)) - c.off[:-1][tix]] = c.ids
    used = np.arange(W - 2)[None, :] < K[:, None]
    assert np.array_equal(rec[:, :W - 2][used], want[used]), f"{name}: ids of {int((rec[:, :W - 2] != want)[used].sum())} list places differ"
    assert t.status() == 0


# ------------------------------------------------------------------ matchers 2 and 4: embed, both forms
@pytest.mark.parametrize("name", STATES)
def test_embed(name, lookup_form):
    c = _case(name)
    t = _handle(c)
    tok, _ = _tokens(c, "rect")
    wpe = torch.from_numpy(c.wpe).cuda()
    for reduce in ("mean", "sum"):
        buf, out = _guarded(tok.numel())
        t.embed(tok, wpe=wpe, reduce=reduce, out=out)
        _same(out, _want(c, "rect", reduce), f"{name}-{lookup_form}-{reduce}")
        _guard_ok(buf, tok.numel())
    assert t.status() == 0


# ------------------------------------------------------------------ matchers 3 and 4: embed_varlen, both forms
@pytest.mark.parametrize("name", STATES)
def test_embed_varlen(name, lookup_form):
    """Every token gets what it gets when its sequence is looked up alone."""
    c = _case(name)
    t = _handle(c)
    tok, cu = _tokens(c, "packed")
    wpe = torch.from_numpy(c.wpe).cuda()
    for reduce in ("mean", "sum"):
        buf, out = _guarded(tok.numel())
        t.embed_varlen(tok, cu, wpe=wpe, reduce=reduce, out=out)
        _same(out, _want(c, "packed", reduce), f"{name}-{lookup_form}-{reduce}")
        _guard_ok(buf, tok.numel())
    assert t.status() == 0


# ------------------------------------------------------------------ matcher 5: embed_select
@pytest.mark.parametrize("name", STATES)
def test_embed_select(name):
    """All positions in a shuffled order, rectangular and packed."""
    c = _case(name)
    t = _handle(c)
    wpe = torch.from_numpy(c.wpe).cuda()
    for form in ("rect", "packed"):
        tok, cu = _tokens(c, form)
        sel = np.random.default_rng(tok.numel()).permutation(tok.numel())
        assert (np.diff(sel) < 0).any()
        buf, out = _guarded(len(sel))
        t.embed_select(tok, torch.from_numpy(sel), cu_seqlens=cu, wpe=wpe, out=out)
        _same(out, _want(c, form)[sel], f"{name}-{form}")
        _guard_ok(buf, len(sel))
    assert t.status() == 0


# ------------------------------------------------------------------ matcher 2 on a row shard: embed_partial
@pytest.mark.parametrize("name", STATES)
def test_embed_partial_on_the_middle_third(name):
    """Counts are the oracle's FULL K; the partial sums are the sequential sums over the rows the handle owns."""
    c = _case(name)
    lo, hi = c.n // 3, max(2 * c.n // 3, c.n // 3 + 1)
    t = _handle(c, row_begin=lo, row_end=hi)
    partial, counts = t.embed_partial(torch.from_numpy(c.batch.rect))
    K = np.diff(c.off)
    assert np.array_equal(counts.cpu().numpy(), K)
    own = (c.ids >= lo) & (c.ids < hi)
    tix = np.repeat(np.arange(len(K)), K)
    off_own = np.zeros(len(K) + 1, dtype=np.int64)
    np.cumsum(np.bincount(tix[own], minlength=len(K)), out=off_own[1:])
    assert 0 < own.sum() < len(own), "the shard owns none or all of the batch's rows"
    _same(partial, R.embed_numpy(c.table, off_own, c.ids[own], "sum"), name)
    assert t.status() == 0


# ------------------------------------------------------------------ paper mode
@pytest.mark.parametrize("name", PAPER_STATES)
def test_paper_mode(name, lookup_form):
    """lookup_mode="longest_suffix" against R.paper_embed: embed (both forms) and embed_select (rectangular and packed)."""
    c = _case(name)
    t = _handle(c, lookup_mode="longest_suffix")
    wpe = torch.from_numpy(c.wpe).cuda()
    tok, _ = _tokens(c, "rect")
    want = _paper_want(c, "rect")
    matched = np.asarray([i >= 0 for row in c.batch.rect for i in R.paper_lookup(R._key_dict(c.keys, c.lens), c.max_n, row.tolist())])
    assert 64 <= matched.sum() <= len(matched) - 64
    buf, out = _guarded(tok.numel())
    t.embed(tok, wpe=wpe, out=out)
    _same(out, want, f"{name}-{lookup_form}-embed")
    _guard_ok(buf, tok.numel())
    for form in ("rect", "packed"):
        tok, cu = _tokens(c, form)
        sel = np.random.default_rng(tok.numel() + 1).permutation(tok.numel())
        buf, out = _guarded(len(sel))
        t.embed_select(tok, torch.from_numpy(sel), cu_seqlens=cu, wpe=wpe, out=out)
        _same(out, (want if form == "rect" else _paper_want(c, "packed"))[sel], f"{name}-select-{form}")
        _guard_ok(buf, len(sel))
    assert t.status() == 0


# ------------------------------------------------------------------ three ways to build each state
@pytest.mark.parametrize("name", STATES)
def test_three_builds_give_one_index(name, monkeypatch):
    monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    c = _case(name)
    a = _handle(c)
    b = _store(_build_device(_new(c), c), c)
    slots, uni, bloom, n_keys, cap = a.index_export()
    assert (n_keys, cap) == (c.facts["n_distinct"], c.capacity)
    cc = _new(c)
    cc.index_import(slots, uni, bloom, n_keys)
    _store(cc, c)
    n_dups = c.n - c.facts["n_distinct"]
    assert a.index_stats() == (c.facts["n_distinct"], c.capacity, n_dups) == b.index_stats()
    assert cc.index_stats()[:2] == (c.facts["n_distinct"], c.capacity)
    tok = torch.from_numpy(c.batch.rect)
    wpe = torch.from_numpy(c.wpe).cuda()
    want = _want(c, "rect")
    first = None
    for how, t in (("chunks", a), ("device", b), ("import", cc)):
        hits = t.match(tok).cpu().numpy()
        assert np.array_equal(hits, c.hits), (name, how)
        rec = _records(t, c)
        buf, out = _guarded(tok.numel())
        t.embed(tok, wpe=wpe, out=out)
        _same(out, want, f"{name}-{how}")
        _guard_ok(buf, tok.numel())
        if first is None:
            first = (rec, out.cpu().numpy())
        else:
            assert np.array_equal(rec, first[0]), (name, how, "records")
            assert np.array_equal(out.cpu().numpy().view(np.uint32), first[1].view(np.uint32)), (name, how, "embed")
        assert t.status() == 0


# ------------------------------------------------------------------ what a build refuses
@pytest.mark.parametrize("name", [s for s in STATES if s.startswith("full")])
def test_one_key_more_than_the_capacity_is_refused(name):
    c = _case(name)
    extra = np.zeros((1, c.max_n), dtype=np.uint32)
    extra[0, :2] = (59999, 59998)                       # no state's vocabulary holds both
    assert (59999, 59998) not in M.distinct_keys(c.keys, c.lens)
    keys, lens = np.concatenate([c.keys, extra]), np.concatenate([c.lens, np.asarray([2], dtype=np.uint8)])
    with pytest.raises(MemoryError, match="index full"):
        _new(c, dim=0).index_build(keys, lens)
    t = _new(c, dim=0)                                  # the table itself fills to the brim without an error
    t.index_build(c.keys, c.lens)
    assert t.index_stats() == (c.capacity, c.capacity, 0) and t.status() == 0


@pytest.mark.parametrize("token", [2**24 - 1, 2**24, 2**31 - 1])
def test_a_max_n_4_key_with_an_unpackable_token_is_refused(token):
    from scone_amd.hip_backend import SconeTable
    for place in range(4):
        keys = np.asarray([[1, 2, 3, 4], [5, 6, 7, 8]], dtype=np.uint32)
        keys[1, place] = token
        t = SconeTable(4, 2, index_capacity=64)
        with pytest.raises(IndexError, match="not representable"):
            t.index_build(keys, np.asarray([4, 4], dtype=np.uint8))
    t = SconeTable(4, 2, index_capacity=64)
    keys[1, 3] = 2**24 - 2                              # the largest token the layout holds
    t.index_build(keys, np.asarray([4, 4], dtype=np.uint8))
    assert t.index_stats()[0] == 2 and t.status() == 0
