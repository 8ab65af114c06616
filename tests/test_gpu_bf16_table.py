"""The bfloat16 table format (SCONE_FMT_BF16) on the GPU: the quantiser, every lookup kernel family, both placements, the native
file.  Run with ``-m gpu`` on an MI355X.

As in tests/test_gpu_walk_shapes.py: tables are quantised on the HOST (tests/bf16_fixture.py, held to torch's conversion by
tests/test_bf16_format_host.py), the expectation is the oracle (oracle/ref_port.py `embed_numpy` / `paper_embed`) on the
dequantised fp32 table, output buffers are pre-filled with NaN, and there is NO tolerance: a bf16 row dequantises to the fp32
value `bits << 16` exactly, the kernels sum those in list order in fp32 as the oracle does, so fp32 output equals the oracle's
bit for bit and fp16 / bf16 output equals that fp32 result rounded once.  bf16 is the one reduced format for which that holds
in every output dtype and at the edges of the fp32 range (sums that overflow, subnormal quotients: the guarded division).

  quantiser          cache_embeddings / store_f32_ids / upload / download / get_embeddings / from_synthetic
  k_embed_fused      d = 768 / 1024 / 1280 x max_n = 3 / 4, both lookup modes, default and explicit positions, one packed call
  k_embed_wave       the same dims with SCONE_FUSED_MAX_TOKENS=0 (position row in LDS at default positions: bit 4 of
                     SCONE_HIOCC_MASK), and two multi-sequence walks
  k_embed_wave_any   d = 64 / 136 / 2048 / 4096, one walk
  k_embed_csr_wave   gather_reduce at d = 768 (lists of 0, 1, 10 and 23 ids: embed_token_long above 10), k_embed at d = 64
  shard              embed_partial + finalize on a handle that owns the middle third of the ids
  placements         pinned host memory read in place, and through the HBM cache of cold rows
  edge values        tests/edge_fixture.py's tables, in both lookup forms
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import edge_fixture as E  # noqa: E402
import walk_geometry as G  # noqa: E402
import test_gpu_walk_shapes as W  # noqa: E402  (its vocabularies, batches and regime assertions: computed once, shared)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
VOCAB, N_POS = W.VOCAB, W.N_POS


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


@pytest.fixture
def one_launch(monkeypatch):
    monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)


@pytest.fixture
def two_kernels(monkeypatch):
    """Read when a handle is created: every batch goes through k_match_ell + the large-batch kernel."""
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")


# ------------------------------------------------------------------ inputs and expectations (host only)
@functools.lru_cache(maxsize=None)
def _tables(d, max_n):
    """(fp32 rows given to the handle, their bf16 bits, the fp32 values those bits stand for, wte, wpe)."""
    rng = np.random.default_rng(31 * d + max_n)
    table = rng.standard_normal((W.N_ROWS[max_n], d)).astype(np.float32)
    bits = BF.to_bf16_bits(table)
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return table, bits, BF.from_bf16_bits(bits), wte, wpe


def _cache(keys, lens, max_n, table, **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    c = EmbeddingCache(ex, table.shape[1], table_format="bf16", **kw)
    c.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return c


def _raw_bits(table_handle, n):
    return BF.rows_as_bits(table_handle.download(0, n)[0])


def _want(stored, keys, lens, max_n, tok, reduce="mean", mode="cover", wte_t=None, wpe_t=None, pos=None):
    """fp32 [B, T, d]: the oracle on the dequantised table; (wte + f-gram) + wpe from the fp32 upcasts of what the kernel gets."""
    B, T = tok.shape
    d = stored.shape[1]
    wte32 = wte_t.float().cpu().numpy() if wte_t is not None else None
    wpe32 = wpe_t.float().cpu().numpy() if wpe_t is not None else None
    pid = pos if pos is not None else np.broadcast_to(np.arange(T), (B, T))
    with np.errstate(over="ignore", invalid="ignore"):
        if mode == "cover":
            off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
            fg = R.embed_numpy(stored, off, ids, reduce).reshape(B, T, d)
            if wte32 is None and wpe32 is None:
                return fg
            return R.combine(torch.from_numpy(tok), torch.from_numpy(fg),
                             torch.from_numpy(wte32) if wte32 is not None else torch.zeros((VOCAB + 1, d)),
                             torch.from_numpy(wpe32) if wpe32 is not None else torch.zeros((N_POS, d)),
                             position_ids=torch.from_numpy(np.array(pid))).numpy()
        e = R.paper_embed(R._key_dict(keys, lens), max_n, tok, stored, wte=wte32)          # (0 + e) + 0
        return e + wpe32[pid] if wpe32 is not None else e


def _lookup(cache, tok, dt, **kw):
    """embed_tokens into a caller's buffer pre-filled with NaN."""
    B, T = tok.shape
    out = torch.full((B, T, cache.embedding_dim), float("nan"), dtype=dt, device="cuda")
    got = cache.embed_tokens(torch.from_numpy(tok), out_dtype=dt, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    return out


def _assert_same(got, want32, dt, what):
    g, w = W._bits(got), W._bits(W._to(want32, dt).reshape(got.shape))
    assert E.same_bits(g, w), (what, E.first_difference(g, w))


def _tokens(rng, B, T):
    return rng.choice(VOCAB + 1, size=(B, T), p=W.TOKEN_P).astype(np.int64)


# ------------------------------------------------------------------ the quantiser and the raw-row entry points
@functools.lru_cache(maxsize=None)
def _edge_rows():
    """48 rows x 64 of edge values: tests/edge_fixture.py's table (subnormals, +-3e38, inf, NaN, the bf16 ties) on top, the
    fixture's own list (both tie patterns, +-max finite, the first value that rounds to inf, fp32 subnormals, +-0, NaNs with
    high and low payloads) and random bit patterns below."""
    rng = np.random.default_rng(48)
    t = E.table(48, 64, seed=5)
    ev = BF.edge_values()
    t[40:46] = np.resize(ev, 6 * 64).reshape(6, 64)
    t[46:48] = rng.integers(0, 2 ** 32, size=128, dtype=np.uint64).astype(np.uint32).view(np.float32).reshape(2, 64)
    lens = rng.integers(1, 4, size=48).astype(np.uint8)
    keys = rng.integers(0, 40, size=(48, 3)).astype(np.uint32)
    keys[np.arange(3)[None, :] >= lens[:, None]] = 0
    return t, keys, lens


def test_quantiser_rounds_to_nearest_even_like_the_host_statement():
    from scone_amd.hip_backend import SconeTable
    rows, keys, lens = _edge_rows()
    want = BF.to_bf16_bits(rows)
    assert BF.is_nan_bits(want).any() and (want == 0x8000).any() and (want == 0x7F80).any() and (want == 0xFF80).any()
    cache = _cache(keys, lens, 3, rows)
    got = _raw_bits(cache.table, 48)
    assert BF.same_bf16_bits(got, want), ("cache_embeddings", np.argwhere(got != want)[:6].tolist())
    assert ((got[BF.is_nan_bits(got)] & 0x0040) != 0).all(), "a stored NaN is a quiet NaN"
    # store_f32_ids: a permuted id list
    perm = np.random.default_rng(1).permutation(48)
    t = SconeTable(3, 48, 64, "bfloat16")
    t.store_f32(torch.from_numpy(rows[perm]), ids=torch.from_numpy(perm))
    assert BF.same_bf16_bits(_raw_bits(t, 48), want) and t.status() == 0
    # get_embeddings: bits << 16
    back = cache.get_embeddings(list(range(48))).numpy()
    assert back.dtype == np.float32 and E.same_bits(back, BF.from_bf16_bits(want))
    # a torch.bfloat16 source leaves exactly its bits in the table
    src = torch.from_numpy(rows).bfloat16()
    c2 = _cache(keys, lens, 3, rows)
    c2.cache_embeddings(list(range(48)), src, verbose=False)
    src_bits = src.view(torch.int16).numpy().view(np.uint16)
    assert BF.same_bf16_bits(_raw_bits(c2.table, 48), src_bits)
    # upload / download move raw bits, NaN payloads included
    raw = np.random.default_rng(2).integers(0, 2 ** 16, size=(48, 64), dtype=np.uint64).astype(np.uint16)
    t.upload(raw)
    assert np.array_equal(_raw_bits(t, 48), raw)
    assert E.same_bits(t.gather_rows(torch.arange(48)).cpu().numpy(), BF.from_bf16_bits(raw))


def test_synthetic_fill_rounds_the_same_fp32_value_as_the_other_formats():
    from scone_amd import EmbeddingCache, NGramExtractor
    n, d, seed, scale = 300, 768, 7, 0.02 / 127
    keys, lens = W._vocabulary(3)
    cache = EmbeddingCache.from_synthetic(NGramExtractor.from_arrays(keys, lens, max_n=3), d, table_format="bf16", seed=seed,
                                          base_scale=scale, n_rows=n)
    ids = np.arange(n, dtype=np.int64)
    f32 = R.synth_rows_i8(seed, ids, d).astype(np.float32) * R.synth_scale_f16(seed, ids, scale).astype(np.float32)[:, None]
    got = _raw_bits(cache.table, n)
    assert np.array_equal(got, BF.to_bf16_bits(f32))
    assert np.array_equal(cache.table.gather_rows(torch.from_numpy(ids)).cpu().numpy(), BF.stored(f32))


# ------------------------------------------------------------------ k_embed_fused: one launch
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_one_launch_kernel(one_launch, d, max_n):
    keys, lens = W._vocabulary(max_n)
    table, bits, stored, wte, wpe = _tables(d, max_n)
    rng = np.random.default_rng(d + max_n)
    k = 0
    for mode in ("cover", "longest_suffix"):
        cache = _cache(keys, lens, max_n, table, lookup_mode=mode)
        assert G.takes_one_launch("bf16", d, 3 * 17)
        if mode == "cover":
            assert np.array_equal(_raw_bits(cache.table, len(lens)), bits)
        for B, T in ((3, 17), (3, 1), (3, 2), (3, 3)):
            tok = _tokens(rng, B, T)
            for pos in (None, rng.integers(0, N_POS, size=(B, T)).astype(np.int64)):
                dt = DTYPES[k % 3]
                k += 1
                wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
                out = _lookup(cache, tok, dt, wte=wte_t, wpe=wpe_t, position_ids=None if pos is None else torch.from_numpy(pos))
                want = _want(stored, keys, lens, max_n, tok, "mean", mode, wte_t, wpe_t, pos)
                _assert_same(out, want, dt, (d, max_n, mode, B, T, "default" if pos is None else "position_ids", str(dt)))
            out = _lookup(cache, tok, torch.float32, reduce="sum")
            _assert_same(out, _want(stored, keys, lens, max_n, tok, "sum", mode), torch.float32, (d, max_n, mode, B, T, "rows only, sum"))
        assert cache.table.status() == 0
    # one packed call: an empty and a one-token sequence among ordinary ones; every token as its sequence alone gives it
    cache = _cache(keys, lens, max_n, table)
    lengths = [5, 0, 1, 11, 0]
    seqs = [_tokens(rng, 1, n)[0] for n in lengths]
    packed, cu = cache.pack_sequences(seqs)
    assert cu.tolist() == [0, 5, 5, 6, 17, 17]
    for dt in DTYPES:
        wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
        out = torch.full((17, d), float("nan"), dtype=dt, device="cuda")
        cache.embed_tokens(packed, cu_seqlens=cu, wte=wte_t, wpe=wpe_t, out=out)
        want = np.concatenate([_want(stored, keys, lens, max_n, s[None, :], "mean", "cover", wte_t, wpe_t)[0] for s in seqs if len(s)])
        _assert_same(out, want, dt, (d, max_n, "packed", str(dt)))
    assert cache.table.status() == 0


# ------------------------------------------------------------------ k_embed_wave: two kernels
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_wave_kernel(two_kernels, d, max_n):
    """[4, 37]: with and without wte, mean and sum, default positions (the high-occupancy variant: the position row in LDS)
    and explicit ones, the three output dtypes in rotation."""
    keys, lens = W._vocabulary(max_n)
    table, _, stored, wte, wpe = _tables(d, max_n)
    cache = _cache(keys, lens, max_n, table)
    assert G.kernel_family("bf16", d) == "k_embed_wave" and not G.takes_one_launch("bf16", d, 4 * 37, fused_max_tokens=0)
    rng = np.random.default_rng(2 * d + max_n)
    tok = _tokens(rng, 4, 37)
    pos = rng.integers(0, N_POS, size=(4, 37)).astype(np.int64)
    k = 0
    for with_wte in (True, False):
        for reduce in ("mean", "sum"):
            for p in (None, pos):
                dt = DTYPES[k % 3]
                k += 1
                wte_t, wpe_t = (W._to(wte, dt).cuda() if with_wte else None), W._to(wpe, dt).cuda()
                out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                want = _want(stored, keys, lens, max_n, tok, reduce, "cover", wte_t, wpe_t, p)
                _assert_same(out, want, dt, (d, max_n, with_wte, reduce, "default" if p is None else "position_ids", str(dt)))
    out = _lookup(cache, tok, torch.float16)
    _assert_same(out, _want(stored, keys, lens, max_n, tok), torch.float16, (d, max_n, "rows only"))
    assert cache.table.status() == 0


def _walk(family, d, T, positions, dt):
    """One multi-sequence walk of tests/test_gpu_walk_shapes.py's batches on a bf16 table (max_n = 3)."""
    max_n = 3
    B, T = W.SHAPES[T]
    W._assert_regime(family, "bf16", d, B, T)
    keys, lens = W._vocabulary(max_n)
    table, _, stored, wte, wpe = _tables(d, max_n)
    tok, pos, _, off, ids = W._batch(max_n, T)
    hist = np.bincount(np.diff(off), minlength=7)
    assert (hist > 0).all(), hist.tolist()
    cache = _cache(keys, lens, max_n, table)
    wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
    p = pos if positions == "random" else None
    out = _lookup(cache, tok, dt, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
    fg = R.embed_numpy(stored, off, ids, "mean").reshape(B, T, d)
    pid = p if p is not None else np.broadcast_to(np.arange(T), (B, T))
    want = R.combine(torch.from_numpy(tok), torch.from_numpy(fg), wte_t.float().cpu(), wpe_t.float().cpu(),
                     position_ids=torch.from_numpy(np.array(pid))).numpy()
    assert np.isfinite(want).all()
    g, w = W._bits(out), W._bits(W._to(want, dt))
    assert E.same_bits(g, w), f"{family}-bf16-d{d}-{B}x{T}-pos_{positions}: {W._differing(g, w, B, T)}"
    assert cache.table.status() == 0


@pytest.mark.parametrize("d,T,positions,dtype", [(768, 5, "random", torch.float16), (1280, 37, "default", torch.bfloat16)])
def test_wave_kernel_walks_several_sequences(two_kernels, d, T, positions, dtype):
    _walk("k_embed_wave", d, T, positions, dtype)


# ------------------------------------------------------------------ k_embed_wave_any: every other d % 8 == 0
@pytest.mark.parametrize("d", [64, 136, 2048, 4096])
def test_any_dim_kernel(d):
    k = 0
    for max_n in (3, 4):
        keys, lens = W._vocabulary(max_n)
        table, bits, stored, wte, wpe = _tables(d, max_n)
        assert G.kernel_family("bf16", d) == "k_embed_wave_any" and not G.takes_one_launch("bf16", d, 5 * 16)
        rng = np.random.default_rng(3 * d + max_n)
        tok = _tokens(rng, 5, 16)
        pos = rng.integers(0, N_POS, size=(5, 16)).astype(np.int64)
        for mode in ("cover", "longest_suffix"):
            cache = _cache(keys, lens, max_n, table, lookup_mode=mode)
            assert np.array_equal(_raw_bits(cache.table, len(lens)), bits)
            for reduce in ("mean", "sum"):
                for p in (None, pos):
                    dt = DTYPES[k % 3]
                    k += 1
                    wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
                    out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                    want = _want(stored, keys, lens, max_n, tok, reduce, mode, wte_t, wpe_t, p)
                    _assert_same(out, want, dt, (d, max_n, mode, reduce, "default" if p is None else "position_ids", str(dt)))
            assert cache.table.status() == 0


def test_any_dim_kernel_walks_several_sequences(two_kernels):
    _walk("k_embed_wave_any", 2048, 16, "random", torch.float32)


# ------------------------------------------------------------------ caller-supplied lists
@pytest.mark.parametrize("d", [768, 64])
def test_csr_lists(d):
    """gather_reduce: k_embed_csr_wave at d = 768 (a list of 23 ids goes through embed_token_long), the lane-group k_embed with
    its CSR id source at d = 64; with and without a dense base."""
    max_n = 4
    keys, lens = W._vocabulary(max_n)
    table, _, stored, _, _ = _tables(d, max_n)
    n = len(lens)
    cache = _cache(keys, lens, max_n, table)
    rng = np.random.default_rng(d)
    ks = [0, 1, 10, 23, 6, 11, 0, 23, 3, 10, 2, 1]
    off = np.zeros(len(ks) + 1, dtype=np.int64)
    np.cumsum(ks, out=off[1:])
    ids = rng.integers(0, n, size=int(off[-1])).astype(np.int64)
    ids[off[3]:off[3] + 5] = ids[off[3]]                          # a repeated id
    base = rng.standard_normal((len(ks), d)).astype(np.float32)
    for reduce in ("mean", "sum"):
        fg = R.embed_numpy(stored, off, ids, reduce)
        for dt in DTYPES:
            out = cache.table.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, out_dtype=dt)
            _assert_same(out, fg, dt, (d, reduce, str(dt), "lists"))
            b = W._to(base, dt)
            out = cache.table.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), reduce, base=b, out_dtype=dt)
            _assert_same(out, b.float().numpy() + fg, dt, (d, reduce, str(dt), "lists + base"))
    # embed_tokens(base=...): the match produces the lists
    tok = _tokens(rng, 3, 17)
    bb = W._to(rng.standard_normal((3, 17, d)).astype(np.float32), torch.float16)
    out = cache.embed_tokens(torch.from_numpy(tok), base=bb.cuda())
    _assert_same(out, bb.float().numpy() + _want(stored, keys, lens, max_n, tok), torch.float16, (d, "embed_tokens(base)"))
    assert cache.table.status() == 0


# ------------------------------------------------------------------ a row shard
@pytest.mark.parametrize("d", [768, 64])
def test_partial_sums_and_finalize_of_a_row_shard(d):
    """A handle that owns the middle third of the ids: embed_partial gives the fp32 sum over the OWNED rows of every list and the
    full hit count; finalize divides by it and combines (k_finalize_wave at 768, k_embed's finalize mode at 64)."""
    from scone_amd.hip_backend import SconeTable
    max_n = 3
    keys, lens = W._vocabulary(max_n)
    table, bits, stored, wte, wpe = _tables(d, max_n)
    n = len(lens)
    lo, hi = n // 3, 2 * n // 3
    t = SconeTable(max_n, n, d, "bf16", row_begin=lo, row_end=hi)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(table[lo:hi]), row0=lo)
    assert np.array_equal(BF.rows_as_bits(t.download(lo, hi - lo)[0]), bits[lo:hi])
    rng = np.random.default_rng(5 * d)
    B, T = 4, 37
    tok = _tokens(rng, B, T)
    pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
    want_sums, kown = W._own_sums(stored, off, ids, lo, hi)
    kfull = np.diff(off)
    assert (kown < kfull).any() and (kown > 0).any()
    sums = torch.full((B * T, d), float("nan"), dtype=torch.float32, device="cuda")
    counts = torch.full((B * T,), W.SENTINEL, dtype=torch.int32, device="cuda")
    t.embed_partial(torch.from_numpy(tok), out=(sums, counts))
    assert np.array_equal(counts.cpu().numpy(), kfull)
    assert E.same_bits(sums.cpu().numpy(), want_sums), E.first_difference(sums.cpu().numpy(), want_sums)
    kf = kfull.astype(np.float32)[:, None]
    mean = np.where(kf > 1, want_sums / np.maximum(kf, np.float32(1)), want_sums).astype(np.float32).reshape(B, T, d)
    for dt in DTYPES:
        wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
        out = torch.full((B * T, d), float("nan"), dtype=dt, device="cuda")
        t.finalize(sums, counts, torch.from_numpy(tok), 0, B * T, wte=wte_t, wpe=wpe_t, position_ids=torch.from_numpy(pos),
                   out_dtype=dt, out=out)
        want = R.combine(torch.from_numpy(tok), torch.from_numpy(mean), wte_t.float().cpu(), wpe_t.float().cpu(),
                         position_ids=torch.from_numpy(pos)).numpy()
        _assert_same(out, want.reshape(B * T, d), dt, (d, str(dt), "finalize"))
    assert t.status() == 0


# ------------------------------------------------------------------ placements
@pytest.mark.parametrize("stage_tokens", [0, 1024])
def test_pinned_host_table(stage_tokens):
    """Rows >= 16 live in pinned host memory: read in place by the lookup kernel, or (stage_tokens > 0) through the HBM cache of
    cold rows.  Both work by row bytes."""
    d, max_n = 768, 3
    keys, lens = W._vocabulary(max_n)
    table, bits, stored, wte, wpe = _tables(d, max_n)
    cache = _cache(keys, lens, max_n, table, placement="pinned_host", hot_rows=16, stage_tokens=stage_tokens)
    assert np.array_equal(_raw_bits(cache.table, len(lens)), bits)
    rng = np.random.default_rng(64 + stage_tokens)
    tok = _tokens(rng, 4, 64)
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
    assert (ids >= 16).any() and (ids < 16).any()
    for dt in DTYPES:
        wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
        out = _lookup(cache, tok, dt, wte=wte_t, wpe=wpe_t)
        torch.cuda.synchronize()
        _assert_same(out, _want(stored, keys, lens, max_n, tok, "mean", "cover", wte_t, wpe_t), dt, (stage_tokens, str(dt)))
    if stage_tokens:
        assert cache.table.stage_counters()["rows_copied"] > 0
    assert cache.table.status() == 0


# ------------------------------------------------------------------ edge values
@pytest.mark.parametrize("form", ["one_launch", "two_kernels"])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values(form, max_n, monkeypatch):
    """tests/edge_fixture.py's table rounded to bf16 by the fixture first (so the handle stores exactly what it is given): sums
    of +-3e38 that overflow to +-inf by the order of the sum (a bf16 holds 3.39e38), inf - inf, subnormal quotients at K = 6
    and 10 (the guarded division), -0.0, NaN rows; mean and sum, three output dtypes, alone and with wte + wpe."""
    if form == "two_kernels":
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    else:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    d = 768
    keys, lens = E.vocabulary(max_n)
    n = len(lens)
    table = BF.stored(E.table(n, d, seed=max_n))
    assert np.isinf(table).any() and np.isnan(table).any() and (np.abs(table[np.isfinite(table)]) > 1e38).any()
    assert ((table != 0) & (np.abs(table) < 1.1754944e-38)).any()
    cache = _cache(keys, lens, max_n, table)
    assert BF.same_bf16_bits(_raw_bits(cache.table, n), BF.to_bf16_bits(table)), "device table differs"
    wte, wpe = E.wte_wpe(3, 64, d, seed=max_n)
    rng = np.random.default_rng(9 + max_n)
    kmax, overflowed, tiny = 0, False, False
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        kmax = max(kmax, int(np.diff(off).max()))
        pos = rng.integers(0, 64, size=(B, T)).astype(np.int64)
        for reduce in ("mean", "sum"):
            fg = _want(table, keys, lens, max_n, tok, reduce)
            overflowed |= bool(np.isinf(fg[..., E.band("c", d)]).any())
            tiny |= bool(((fg != 0) & (np.abs(fg) < 1.1754944e-38)).any())
            for dt in DTYPES:
                tag = (form, max_n, f"stream {si} {B}x{T}", reduce, str(dt))
                _assert_same(_lookup(cache, tok, dt, reduce=reduce), fg, dt, tag + ("rows only",))
                wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
                for p in (None, pos):
                    out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                    want = _want(table, keys, lens, max_n, tok, reduce, "cover", wte_t, wpe_t, p)
                    _assert_same(out, want, dt, tag + ("wte+wpe", "default" if p is None else "position_ids"))
    assert kmax == max_n * (max_n + 1) // 2 and overflowed and tiny       # K = 6 / 10, an overflowed sum and a subnormal result occurred


# ------------------------------------------------------------------ the native file
def test_native_file_round_trip(one_launch, tmp_path):
    from scone_amd import EmbeddingCache
    rng = np.random.default_rng(200)
    n, d, max_n = 200, 768, 3
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, VOCAB, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    table = rng.standard_normal((n, d)).astype(np.float32)
    table[:3, :39] = BF.edge_values()[None, :]
    cache = _cache(keys, lens, max_n, table)
    raw = _raw_bits(cache.table, n)
    assert BF.same_bf16_bits(raw, BF.to_bf16_bits(table))
    path = str(tmp_path / "bf16_table")
    cache.save_native(path, chunk_rows=64)
    again = EmbeddingCache.load_native(path, chunk_rows=48)
    assert again.table_format == "bf16" and again.table.fmt == 4
    assert np.array_equal(_raw_bits(again.table, n), raw)
    tok = _tokens(rng, 3, 17)
    a = _lookup(cache, tok, torch.float32)
    b = _lookup(again, tok, torch.float32)
    assert E.same_bits(a.cpu().numpy(), b.cpu().numpy())
    _assert_same(b, _want(BF.from_bf16_bits(raw), keys, lens, max_n, tok), torch.float32, "lookup from the loaded table")
