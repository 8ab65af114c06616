"""The MXFP4 table format (SCONE_FMT_MXFP4: E2M1 elements, one E8M0 scale per 32) on the GPU: the decode of all 4,096 (code,
scale byte) pairs through every kernel family, the quantiser, every lookup form, both placements, the shard paths, the native
file.  Run with ``-m gpu`` on an MI355X.

As in tests/test_gpu_bf16_table.py: tables are quantised on the HOST (tests/mxfp4_fixture.py, its two statements held to each
other by tests/test_mxfp4_format_host.py), the expectation is the oracle (oracle/ref_port.py `embed_numpy` / `paper_embed`) on
the dequantised fp32 table, output buffers are pre-filled with NaN, and there is NO tolerance: an E2M1 value times 2^(X-127)
is exact in fp32 wherever it is finite, the kernels sum those values in list order in fp32 as the oracle does, so fp32 output
equals the oracle's bit for bit and fp16 / bf16 output equals that fp32 result rounded once.

  exhaustive decode  256 rows uploaded raw, row X has scale byte X in every block and the 16 codes cycling: gather_rows and a
                     K = 1 sum lookup through k_embed (d = 128, CSR lists), k_embed_fused / k_embed_wave / k_embed_csr_wave
                     (d = 1024) and k_embed_wave_any (d = 2048) -- the test that licenses the hardware convert
  quantiser          store_f32 / store_f32_ids / cache_embeddings on the fixture's edge rows, download in logical order,
                     get_embeddings, the synthetic fill against its restatement
  k_embed_fused      d = 1024 in one launch (768 / 1280: the any-dim kernel, as INT4), max_n = 3 / 4, both modes, packed batches
  k_embed_wave       d = 1024 with SCONE_FUSED_MAX_TOKENS=0 (the position row in LDS at default positions: bit 5 of
                     SCONE_HIOCC_MASK), one multi-sequence walk per large-batch kernel
  k_embed_wave_any   d = 128 / 384 / 2048 / 4096 (and 768 / 1280 above)
  lists              gather_reduce at d = 1024 (0, 1, 10 and 23 ids: embed_token_long above 10) and 128, with a dense base
  shard              embed_partial + finalize of a middle-third shard; record and column exchange between three shards
  placements         pinned host memory read in place, and through the HBM cache of cold rows
  edge values        raw blocks at both ends of the scale range: sums that overflow by order, inf - inf, NaN blocks, -0,
                     subnormal sums and quotients at K = 6 and 10
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mxfp4_fixture as MX  # noqa: E402
import edge_fixture as E  # noqa: E402
import walk_geometry as G  # noqa: E402
import test_gpu_walk_shapes as W  # noqa: E402  (its vocabularies, batches and regime assertions: computed once, shared)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
VOCAB, N_POS = W.VOCAB, W.N_POS
GEOM = "int4"       # tests/walk_geometry.py names the rule by its first user: MXFP4 has INT4's payload geometry and follows it


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
    """(fp32 rows given to the handle, payload, scale bytes, the fp32 values they stand for, wte, wpe).  Every block of 32 gets
    its own magnitude (2^-12 .. 2^12), so the scale bytes differ along a row and between rows."""
    rng = np.random.default_rng(37 * d + max_n)
    n = W.N_ROWS[max_n]
    table = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-12, 13, size=(n, d // 32)).repeat(32, axis=1))).astype(np.float32)
    payload, scales = MX.quantize(table)
    assert len(np.unique(scales)) > 20
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return table, payload, scales, MX.dequantize(payload, scales), wte, wpe


def _cache(keys, lens, max_n, table, **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    c = EmbeddingCache(ex, table.shape[1], table_format="mxfp4", **kw)
    c.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return c


def _raw_cache(keys, lens, max_n, payload, scales, **kw):
    """A cache whose table holds exactly these bytes (SconeTable.upload: the road of an existing MX checkpoint)."""
    from scone_amd import EmbeddingCache, NGramExtractor
    ex = NGramExtractor.from_arrays(keys, lens, max_n=max_n)
    c = EmbeddingCache(ex, payload.shape[1] * 2, table_format="mxfp4", keep_host_copy=False, **kw)
    c.to_device().upload(payload, scales)
    c._present[:] = True
    return c


def _holds(handle, payload, scales, row0=0):
    gp, gs = handle.download(row0, len(payload))
    assert gp.dtype == np.uint8 and gs.dtype == np.uint8 and gs.shape == scales.shape
    assert np.array_equal(gs, scales), ("scale bytes", np.argwhere(gs != scales)[:5].tolist())
    assert np.array_equal(gp, payload), ("payload", np.argwhere(gp != payload)[:5].tolist())


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


# ------------------------------------------------------------------ all 4,096 (code, scale byte) pairs
def _decode_table(d):
    """256 rows: row X has scale byte X in every block, the 16 codes cycle through the elements (shifted by one per payload
    dword and per row, so every code meets every nibble position of a dword)."""
    e = np.arange(d)
    codes = ((e[None, :] + e[None, :] // 8 + np.arange(256)[:, None]) % 16).astype(np.uint8)
    scales = np.arange(256, dtype=np.uint8)[:, None].repeat(d // 32, axis=1)
    return MX.pack(codes), np.ascontiguousarray(scales)


@pytest.mark.parametrize("d", [128, 1024, 2048])
def test_exhaustive_decode(d, monkeypatch):
    """Every (code, X) pair read back by gather_rows and by a K = 1 `sum` lookup of each kernel family that serves this d: the
    row itself must come out -- the subnormal factor at X = 0, +-inf from the large codes at X >= 253, NaN for all 16 codes at
    X = 255, -0 from code 0x8 -- in fp32, bit for bit."""
    payload, scales = _decode_table(d)
    want = MX.dequantize(payload, scales)
    assert np.isnan(want[255]).all() and np.isinf(want[253:255]).any() and (np.abs(want[0][want[0] != 0]) < 1.1754944e-38).any()
    keys = np.zeros((256, 3), dtype=np.uint32)
    keys[:, 0] = np.arange(256)
    lens = np.ones(256, dtype=np.uint8)                                   # 256 unigrams: token t -> row t, alone (K = 1)
    tok = np.random.default_rng(d).permutation(256).reshape(4, 64).astype(np.int64)
    ids = tok.reshape(-1)
    off = np.arange(257, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        summed = R.embed_numpy(want, off, ids, "sum")                     # 0 + value, as the oracle and the kernels start: -0 -> +0
    assert E.same_bits(summed[want[ids] != 0], want[ids][want[ids] != 0]) and not np.signbit(summed[want[ids] == 0]).any()
    assert np.array_equal(R.hits_to_csr(R.match_hits(keys, lens, tok, 3))[1], ids)
    for form in ("one_launch", "two_kernels"):
        if form == "two_kernels":
            monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
        else:
            monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
        cache = _raw_cache(keys, lens, 3, payload, scales)
        t = cache.table
        _holds(t, payload, scales)
        assert E.same_bits(t.gather_rows(torch.arange(256)).cpu().numpy(), want), "gather_rows"
        # d = 128 / 2048: k_embed_wave_any in both forms; d = 1024: k_embed_fused, then k_embed_wave
        assert G.takes_one_launch(GEOM, d, 256, fused_max_tokens=G.FUSED_MAX_TOKENS if form == "one_launch" else 0) == (d == 1024 and form == "one_launch")
        for reduce in ("sum", "mean"):
            out = _lookup(cache, tok, torch.float32, reduce=reduce).cpu().numpy().reshape(256, d)
            assert E.same_bits(out, summed), (form, d, reduce, E.first_difference(out, summed))
        # caller-supplied lists: k_embed_csr_wave at d = 1024, the lane-group k_embed elsewhere
        out = t.gather_reduce(torch.from_numpy(off), torch.from_numpy(ids), "sum", out_dtype=torch.float32).cpu().numpy()
        assert E.same_bits(out, summed), (form, d, "lists", E.first_difference(out, summed))
        assert t.status() == 0


# ------------------------------------------------------------------ the quantiser and the raw-row entry points
def test_quantiser_on_the_device_is_the_fixtures():
    from scone_amd.hip_backend import SconeTable
    rng = np.random.default_rng(48)
    for d in (128, 1024):                                                  # 1024: the scales are permuted inside the table
        rows = np.concatenate([MX.edge_rows(d, seed=d), E.table(24, d, seed=5),
                               (rng.standard_normal((12, d)) * np.exp2(rng.integers(-140, 125, size=(12, d // 32)).repeat(32, axis=1))).astype(np.float32)])
        n = len(rows)
        payload, scales = MX.quantize(rows)
        assert (scales == 255).any() and (scales == 0).any() and (scales == 252).any() and (scales == 127).any()
        t = SconeTable(3, n, d, "mxfp4")
        t.store_f32(torch.from_numpy(rows))
        _holds(t, payload, scales)
        perm = rng.permutation(n)
        t2 = SconeTable(3, n, d, "mxfp4")
        t2.store_f32(torch.from_numpy(rows[perm]), ids=torch.from_numpy(perm))
        _holds(t2, payload, scales)
        assert t.status() == 0 and t2.status() == 0
        assert E.same_bits(t.gather_rows(torch.arange(n)).cpu().numpy(), MX.dequantize(payload, scales))
        # upload / download move raw bytes in logical order; float4 / e8m0 tensors are taken as their bytes
        raw_p = rng.integers(0, 256, size=(n, d // 2), dtype=np.uint8)
        raw_s = rng.integers(0, 256, size=(n, d // 32), dtype=np.uint8)
        t.upload(raw_p, raw_s)
        _holds(t, raw_p, raw_s)
        assert E.same_bits(t.gather_rows(torch.arange(n)).cpu().numpy(), MX.dequantize(raw_p, raw_s))
        t2.upload(torch.from_numpy(raw_p).view(torch.float4_e2m1fn_x2).cuda(), torch.from_numpy(raw_s).view(torch.float8_e8m0fnu).cuda())
        _holds(t2, raw_p, raw_s)
        _holds(t2, raw_p[5:9], raw_s[5:9], row0=5)
        with pytest.raises(ValueError, match="mxfp4 upload"):
            t.upload(raw_p, None)
    # cache_embeddings / get_embeddings
    keys, lens = W._vocabulary(3)
    table, payload, scales, stored, _, _ = _tables(128, 3)
    cache = _cache(keys, lens, 3, table)
    _holds(cache.table, payload, scales)
    back = cache.get_embeddings(list(range(len(lens)))).numpy()
    assert back.dtype == np.float32 and E.same_bits(back, stored)


@pytest.mark.parametrize("d", [1024, 384])
def test_synthetic_fill_is_its_restatement(d):
    from scone_amd import EmbeddingCache, NGramExtractor
    n, seed, scale = 300, 7, 0.02 / 127
    keys, lens = W._vocabulary(3)
    cache = EmbeddingCache.from_synthetic(NGramExtractor.from_arrays(keys, lens, max_n=3), d, table_format="mxfp4", seed=seed,
                                          base_scale=scale, n_rows=n)
    payload, scales = MX.synthetic(seed, np.arange(n), d, scale)
    e = int(np.floor(np.log2(scale))) + 127
    assert set(np.unique(scales).tolist()) == {e - 1, e, e + 1}
    _holds(cache.table, payload, scales)
    if d % 128 == 0:
        assert np.array_equal(R.synth_rows_i4(seed, np.arange(n, dtype=np.int64), d, scale)[0], payload), "the payload words are the ones INT4 gets"
    assert E.same_bits(cache.table.gather_rows(torch.arange(n)).cpu().numpy(), MX.dequantize(payload, scales))


# ------------------------------------------------------------------ one launch
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_one_launch_form(one_launch, d, max_n):
    """Batches far below the one-launch limit: k_embed_fused at d = 1024; at 768 / 1280 the nibble formats have no specialised
    kernel and the same calls take k_match_ell + k_embed_wave_any."""
    keys, lens = W._vocabulary(max_n)
    table, payload, scales, stored, wte, wpe = _tables(d, max_n)
    rng = np.random.default_rng(d + max_n)
    k = 0
    for mode in ("cover", "longest_suffix"):
        cache = _cache(keys, lens, max_n, table, lookup_mode=mode)
        assert G.takes_one_launch(GEOM, d, 3 * 17) == (d == 1024)
        if mode == "cover":
            _holds(cache.table, payload, scales)
        for B, T in ((4, 37), (3, 1), (3, 2), (3, 3)):
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
    # one packed call (cu_seqlens): an empty and a one-token sequence among ordinary ones
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


# ------------------------------------------------------------------ two kernels
@pytest.mark.parametrize("d", [768, 1024, 1280])
@pytest.mark.parametrize("max_n", [3, 4])
def test_two_kernel_form(two_kernels, d, max_n):
    """[4, 37]: with and without wte / wpe, mean and sum, default positions (d = 1024: the high-occupancy variant, the position
    row in LDS) and explicit ones, the three output dtypes in rotation.  k_embed_wave at 1024, k_embed_wave_any at 768 / 1280."""
    keys, lens = W._vocabulary(max_n)
    table, _, _, stored, wte, wpe = _tables(d, max_n)
    cache = _cache(keys, lens, max_n, table)
    assert G.kernel_family(GEOM, d) == ("k_embed_wave" if d == 1024 else "k_embed_wave_any")
    assert not G.takes_one_launch(GEOM, d, 4 * 37, fused_max_tokens=0)
    rng = np.random.default_rng(2 * d + max_n)
    tok = _tokens(rng, 4, 37)
    pos = rng.integers(0, N_POS, size=(4, 37)).astype(np.int64)
    k = 0
    for with_wte, with_wpe in ((True, True), (False, True), (True, False)):
        for reduce in ("mean", "sum"):
            for p in (None, pos):
                dt = DTYPES[k % 3]
                k += 1
                wte_t = W._to(wte, dt).cuda() if with_wte else None
                wpe_t = W._to(wpe, dt).cuda() if with_wpe else None
                if not with_wpe:
                    p = None
                out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                want = _want(stored, keys, lens, max_n, tok, reduce, "cover", wte_t, wpe_t, p)
                _assert_same(out, want, dt, (d, max_n, with_wte, with_wpe, reduce, "default" if p is None else "position_ids", str(dt)))
    out = _lookup(cache, tok, torch.float16)
    _assert_same(out, _want(stored, keys, lens, max_n, tok), torch.float16, (d, max_n, "rows only"))
    assert cache.table.status() == 0


def _walk(family, d, T, positions, dt):
    """One multi-sequence walk of tests/test_gpu_walk_shapes.py's batches on an MXFP4 table (max_n = 3)."""
    max_n = 3
    B, T = W.SHAPES[T]
    W._assert_regime(family, GEOM, d, B, T)
    keys, lens = W._vocabulary(max_n)
    table, _, _, stored, wte, wpe = _tables(d, max_n)
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
    assert E.same_bits(g, w), f"{family}-mxfp4-d{d}-{B}x{T}-pos_{positions}: {W._differing(g, w, B, T)}"
    assert cache.table.status() == 0


@pytest.mark.parametrize("family,d,T,positions,dtype", [("k_embed_wave", 1024, 5, "default", torch.float16),
                                                        ("k_embed_wave_any", 2048, 16, "random", torch.float32)])
def test_large_batch_kernels_walk_several_sequences(two_kernels, family, d, T, positions, dtype):
    _walk(family, d, T, positions, dtype)


# ------------------------------------------------------------------ k_embed_wave_any: every other d % 128 == 0
@pytest.mark.parametrize("d", [128, 384, 2048, 4096])
def test_any_dim_kernel(d):
    k = 0
    for max_n in (3, 4):
        keys, lens = W._vocabulary(max_n)
        table, payload, scales, stored, wte, wpe = _tables(d, max_n)
        assert G.kernel_family(GEOM, d) == "k_embed_wave_any" and not G.takes_one_launch(GEOM, d, 5 * 16)
        rng = np.random.default_rng(3 * d + max_n)
        tok = _tokens(rng, 5, 16)
        pos = rng.integers(0, N_POS, size=(5, 16)).astype(np.int64)
        for mode in ("cover", "longest_suffix"):
            cache = _cache(keys, lens, max_n, table, lookup_mode=mode)
            _holds(cache.table, payload, scales)
            for reduce in ("mean", "sum"):
                for p in (None, pos):
                    dt = DTYPES[k % 3]
                    k += 1
                    wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
                    out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                    want = _want(stored, keys, lens, max_n, tok, reduce, mode, wte_t, wpe_t, p)
                    _assert_same(out, want, dt, (d, max_n, mode, reduce, "default" if p is None else "position_ids", str(dt)))
            assert cache.table.status() == 0


# ------------------------------------------------------------------ caller-supplied lists
@pytest.mark.parametrize("d", [1024, 128])
def test_csr_lists(d):
    """gather_reduce: k_embed_csr_wave at d = 1024 (a list of 23 ids goes through embed_token_long), the lane-group k_embed with
    its CSR id source at d = 128; with and without a dense base; embed_tokens(base=...) and out == base."""
    max_n = 4
    keys, lens = W._vocabulary(max_n)
    table, _, _, stored, _, _ = _tables(d, max_n)
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
    # embed_tokens(base=...): the match produces the lists; then in place, out is base
    tok = _tokens(rng, 3, 17)
    bb = W._to(rng.standard_normal((3, 17, d)).astype(np.float32), torch.float16)
    want = bb.float().numpy() + _want(stored, keys, lens, max_n, tok)
    out = cache.embed_tokens(torch.from_numpy(tok), base=bb.cuda())
    _assert_same(out, want, torch.float16, (d, "embed_tokens(base)"))
    buf = bb.cuda().clone()
    out = cache.embed_tokens(torch.from_numpy(tok), base=buf, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    _assert_same(buf, want, torch.float16, (d, "embed_tokens(base), in place"))
    assert cache.table.status() == 0


# ------------------------------------------------------------------ a row shard
@pytest.mark.parametrize("d", [1024, 128])
def test_partial_sums_and_finalize_of_a_row_shard(d):
    """A handle that owns the middle third of the ids: embed_partial gives the fp32 sum over the OWNED rows of every list and the
    full hit count; finalize divides by it and combines (k_finalize_wave at 1024, k_embed's finalize mode at 128)."""
    from scone_amd.hip_backend import SconeTable
    max_n = 3
    keys, lens = W._vocabulary(max_n)
    table, payload, scales, stored, wte, wpe = _tables(d, max_n)
    n = len(lens)
    lo, hi = n // 3, 2 * n // 3
    t = SconeTable(max_n, n, d, "mxfp4", row_begin=lo, row_end=hi)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(table[lo:hi]), row0=lo)
    _holds(t, payload[lo:hi], scales[lo:hi], row0=lo)
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


@pytest.mark.parametrize("head", [0, 20])
def test_row_exchange_between_three_shards_on_one_gpu(head):
    """Records [payload | scales | row id] and columns (payload rows | scales | hash fragments) between three shards, with and
    without a replicated head: every form equals the oracle on the dequantised table, as the unsharded table does."""
    from scone_amd.distributed import shard_range
    from scone_amd.hip_backend import SconeTable
    d, max_n, world = 1024, 3, 3
    keys, lens = W._vocabulary(max_n)
    table, payload, scales, stored, wte, wpe = _tables(d, max_n)
    n = len(lens)
    rng = np.random.default_rng(77 + head)
    B, T = 4, 37
    tok_np = _tokens(rng, B, T)
    tok = torch.from_numpy(tok_np)
    wte_t, wpe_t = W._to(wte, torch.float16).cuda(), W._to(wpe, torch.float16).cuda()
    want = _want(stored, keys, lens, max_n, tok_np, "mean", "cover", wte_t, wpe_t).reshape(B * T, d)
    full = SconeTable(max_n, n, d, "mxfp4")
    full.index_build(keys, lens)
    full.store_f32(torch.from_numpy(table))
    _assert_same(full.embed(tok, wte=wte_t, wpe=wpe_t).reshape(B * T, d), want, torch.float16, "unsharded")
    shards = []
    for r in range(world):
        a, b = shard_range(n, r, world)
        s = SconeTable(max_n, n, d, "mxfp4", row_begin=a, row_end=b)
        s.index_build(keys, lens)
        s.store_f32(torch.from_numpy(table[a:b]), row0=a)
        if head:
            s.shard_set_head(head)
            s.shard_head_store_f32(torch.from_numpy(table[:head]), row0=0)
        shards.append(s)
    assert shards[0].shard_record_bytes() >= d // 2 + d // 32 + 8
    sends = [s.shard_gather_pack(s.shard_gather_plan(tok)) for s in shards]
    recv = torch.cat([sends[r] for r in (2, 0, 1)]).contiguous()
    got = shards[1].shard_gather_embed(tok, recv, wte=wte_t, wpe=wpe_t, out_dtype=torch.float16)
    _assert_same(got, want, torch.float16, ("records", head))
    cnts = [s.shard_gather_plan(tok) for s in shards]
    slots = [SconeTable.cols_frag_slots(c) for c in cnts]
    rb, fo = [sum(cnts[:r]) for r in range(world)], [sum(slots[:r]) for r in range(world)]
    tot, pb, sb = sum(cnts), shards[0].payload_bytes(), shards[0].scale_bytes()
    assert (pb, sb) == (d // 2, d // 32)
    c_rows = torch.empty((max(tot, 1), pb), dtype=torch.uint8, device="cuda")
    c_sc = torch.empty((head + max(tot, 1), sb), dtype=torch.uint8, device="cuda")
    c_fr = torch.empty(sum(slots), dtype=torch.int64, device="cuda")
    for r, s in enumerate(shards):
        s.shard_cols_pack(0, cnts[r], c_rows[rb[r]:rb[r] + cnts[r]], c_sc[head + rb[r]:head + rb[r] + cnts[r]], c_fr[fo[r]:fo[r] + slots[r]])
    if head:
        shards[2].shard_head_scales_into(c_sc)
    got = torch.full((B * T, d), float("nan"), dtype=torch.float16, device="cuda")
    shards[2].shard_cols_embed(tok, 0, B, c_rows, tot, c_sc, c_fr, fo, slots, rb, got, wte=wte_t, wpe=wpe_t)
    _assert_same(got, want, torch.float16, ("columns", head))
    assert all(s.status() == 0 for s in shards)


# ------------------------------------------------------------------ placements
@pytest.mark.parametrize("stage_tokens", [0, 1024])
def test_pinned_host_table(stage_tokens):
    """Rows >= 16 live in pinned host memory: read in place by the lookup kernel, or (stage_tokens > 0) through the HBM cache of
    cold rows.  Both work by row bytes.  Read in place, the scales are the table's own (always in HBM); the cache keeps its OWN
    copy of a cold row's scales beside the row, filled by the kernel that copies the row (k_stage_copy) -- at d = 1024 that is 32
    bytes per row; tests/test_gpu_wide_rows.py runs the widths at which a row has more than 128."""
    d, max_n = 1024, 3
    keys, lens = W._vocabulary(max_n)
    table, payload, scales, stored, wte, wpe = _tables(d, max_n)
    cache = _cache(keys, lens, max_n, table, placement="pinned_host", hot_rows=16, stage_tokens=stage_tokens)
    _holds(cache.table, payload, scales)
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
def _edge_blocks(n, d, seed):
    """Raw rows whose blocks sit at the ends of the scale range, one class per block (block j: class j % 6):
      0  X in 0..3, any code: subnormal values (multiples of 2^-128), sums exact, quotients subnormal with ties
      1  X in 250..252, any code: finite values up to 6 * 2^125 whose sums overflow to +-inf or cancel back, by the order
      2  X = 253 / 254: the large codes are +-inf themselves, inf - inf among the sums
      3  X = 255 in every eighth row: NaN blocks among ordinary ones
      4  code 0 / 0x8 only: +-0 sums
      5  X near 127: the control"""
    rng = np.random.default_rng(seed)
    nb = d // 32
    codes = rng.integers(0, 16, size=(n, d), dtype=np.uint8)
    X = np.zeros((n, nb), dtype=np.uint8)
    for j in range(nb):
        c = j % 6
        X[:, j] = (rng.integers(0, 4, size=n), rng.integers(250, 253, size=n), rng.integers(253, 255, size=n),
                   np.where(np.arange(n) % 8 == 3, 255, rng.integers(120, 135, size=n)), rng.integers(0, 255, size=n),
                   rng.integers(120, 135, size=n))[c]
        if c == 4:
            codes[:, 32 * j:32 * j + 32] &= 8
    return MX.pack(codes), X


@pytest.mark.parametrize("form", ["one_launch", "two_kernels"])
@pytest.mark.parametrize("max_n", [3, 4])
def test_edge_values(form, max_n, monkeypatch):
    """tests/edge_fixture.py's vocabularies and streams (K up to 6 resp. 10) on raw edge blocks: mean and sum, three output
    dtypes, alone and with wte + wpe that hold -0, +-inf and +-65504 themselves."""
    if form == "two_kernels":
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    else:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    d = 1024
    keys, lens = E.vocabulary(max_n)
    n = len(lens)
    payload, scales = _edge_blocks(n, d, seed=max_n)
    table = MX.dequantize(payload, scales)
    cols = lambda c: np.concatenate([np.arange(32 * j, 32 * j + 32) for j in range(d // 32) if j % 6 == c])      # noqa: E731
    assert np.isinf(table[:, cols(2)]).any() and np.isnan(table[:, cols(3)]).any() and np.isfinite(table[:, cols(1)]).all()
    assert ((table[:, cols(0)] != 0) & (np.abs(table[:, cols(0)]) < 1.1754944e-38)).any() and np.signbit(table[:, cols(4)]).any()
    cache = _raw_cache(keys, lens, max_n, payload, scales)
    _holds(cache.table, payload, scales)
    wte, wpe = E.wte_wpe(3, 64, d, seed=max_n)
    rng = np.random.default_rng(9 + max_n)
    kmax, overflowed, tiny, cancelled = 0, False, False, False
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
        kmax = max(kmax, int(np.diff(off).max()))
        pos = rng.integers(0, 64, size=(B, T)).astype(np.int64)
        for reduce in ("mean", "sum"):
            fg = _want(table, keys, lens, max_n, tok, reduce)
            overflowed |= bool(np.isinf(fg[..., cols(1)]).any())
            cancelled |= bool(np.isnan(fg[..., cols(2)]).any())
            tiny |= bool(((fg[..., cols(0)] != 0) & (np.abs(fg[..., cols(0)]) < 1.1754944e-38)).any())
            for dt in DTYPES:
                tag = (form, max_n, f"stream {si} {B}x{T}", reduce, str(dt))
                _assert_same(_lookup(cache, tok, dt, reduce=reduce), fg, dt, tag + ("rows only",))
                wte_t, wpe_t = W._to(wte, dt).cuda(), W._to(wpe, dt).cuda()
                for p in (None, pos):
                    out = _lookup(cache, tok, dt, reduce=reduce, wte=wte_t, wpe=wpe_t, position_ids=None if p is None else torch.from_numpy(p))
                    want = _want(table, keys, lens, max_n, tok, reduce, "cover", wte_t, wpe_t, p)
                    _assert_same(out, want, dt, tag + ("wte+wpe", "default" if p is None else "position_ids"))
    # K = 6 / 10, a sum of finite values that overflowed, inf - inf, and a subnormal result occurred
    assert kmax == max_n * (max_n + 1) // 2 and overflowed and cancelled and tiny
    assert cache.table.status() == 0


# ------------------------------------------------------------------ the native file
def test_native_file_round_trip(one_launch, tmp_path):
    from scone_amd import EmbeddingCache
    rng = np.random.default_rng(200)
    n, d, max_n = 200, 1024, 3
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, VOCAB, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    table = (rng.standard_normal((n, d)) * np.exp2(rng.integers(-12, 13, size=(n, d // 32)).repeat(32, axis=1))).astype(np.float32)
    table[:12] = MX.edge_rows(d, seed=3)
    cache = _cache(keys, lens, max_n, table)
    payload, scales = MX.quantize(table)
    _holds(cache.table, payload, scales)
    path = str(tmp_path / "mxfp4_table")
    cache.save_native(path, chunk_rows=64)
    again = EmbeddingCache.load_native(path, chunk_rows=48)
    assert again.table_format == "mxfp4" and again.table.fmt == 5
    _holds(again.table, payload, scales)
    tok = _tokens(rng, 3, 17)
    a = _lookup(cache, tok, torch.float32)
    b = _lookup(again, tok, torch.float32)
    assert E.same_bits(a.cpu().numpy(), b.cpu().numpy())
    _assert_same(b, _want(MX.dequantize(payload, scales), keys, lens, max_n, tok), torch.float32, "lookup from the loaded table")
