"""The fused lookup onto a dense base (`scone_embed_base`, `scone_embed_base_varlen`, `embed_tokens(base=...)`) against the oracle.

    out[p] = cast((base[p] + reduce_k row_k) + wpe[pos[p]])          (paper mode: a matched f-gram REPLACES base[p])

Expectations come from oracle/ref_port.py on the host-dequantised table: `R.match_hits` -> `R.hits_to_csr` -> `R.embed_numpy`
in cover mode, `R.paper_embed` for the paper's lookup, packed batches one sequence at a time (the helpers of
tests/test_gpu_varlen.py), combined as `(base + fg) + wpe[pos]` in fp32.  The bar has no tolerance -- fp32 output is bit-equal,
fp16 / bf16 output equals the expectation rounded once -- because the arithmetic body is the one the `wte` road runs
(`embed_token` / `embed_units` / `k_embed`); what is new is WHICH row is the base row, and `base` is i.i.d. random per element,
so a row taken from the wrong position cannot pass.

Every call writes into the first rows of a NaN-filled buffer with 64 guard rows that must still be NaN afterwards, and
`table.status()` must be 0.  Each shape is the smallest that reaches the code named in its test: the walk of several sequences
per workgroup (12301 x 3), tail waves with i >= T (1243 x 37, 7 x 5), the three places that launch on a SLICE of the batch and
must move the base pointer with it (staged chunks, the remainder launch of a packed batch, the SCONE_VARLEN_T traversal).
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
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches and their per-sequence oracle)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, host quantisation, rounding, bit views)

pytestmark = pytest.mark.gpu

VOCAB, TOKEN_P, DTYPES = WS.VOCAB, WS.TOKEN_P, WS.DTYPES
N_POS = 64
GUARD = 64
MODES = ("cover", "longest_suffix")
FORMATS_1024 = [("fp32", 1024), ("fp16", 1024), ("int8", 1024), ("int4", 1024), ("bf16", 1024)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _form(monkeypatch, form):
    """SCONE_FUSED_MAX_TOKENS is read when a handle is created."""
    if form == "two_kernels":
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")
    else:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)


# ------------------------------------------------------------------ inputs and expectations (host only)
def _stored(table, fmt):
    return BF.stored(table) if fmt == "bf16" else WS._stored(table, fmt)


@functools.lru_cache(maxsize=None)
def _tables(fmt, d, max_n):
    """(fp32 rows given to the handle, the same rows as the format stores them, wpe[N_POS, d])."""
    rng = np.random.default_rng(13 * d + max_n)
    table = rng.standard_normal((WS.N_ROWS[max_n], d)).astype(np.float32)
    return table, _stored(table, fmt), rng.standard_normal((N_POS, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(B, T, max_n):
    """Tokens [B, T], random positions [B, T], CSR id lists.  The walk shapes are those of tests/test_gpu_walk_shapes.py."""
    if WS.SHAPES.get(T) == (B, T):
        tok, pos, _, off, ids = WS._batch(max_n, T)
        return tok, pos, off, ids
    rng = np.random.default_rng(100 * B + T + max_n)
    tok = rng.choice(VOCAB + 1, size=(B, T), p=TOKEN_P).astype(np.int64)
    pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
    off, ids = R.hits_to_csr(R.match_hits(*WS._vocabulary(max_n), tok, max_n))
    return tok, pos, off, ids


@functools.lru_cache(maxsize=None)
def _base32(n, d, seed=0):
    return np.random.default_rng(9000 + n + d + seed).standard_normal((n, d)).astype(np.float32)


@functools.lru_cache(maxsize=2)
def _fgram(fmt, d, max_n, B, T, mode, reduce):
    """fp32 [B * T, d] f-gram part; longest_suffix: (rows, mask of matched tokens)."""
    stored = _tables(fmt, d, max_n)[1]
    tok, _, off, ids = _batch(B, T, max_n)
    if mode == "cover":
        return R.embed_numpy(stored, off, ids, reduce)
    f2id = R._key_dict(*WS._vocabulary(max_n))
    matched = np.asarray([R.paper_lookup(f2id, max_n, row.tolist()) for row in tok]) >= 0
    return R.paper_embed(f2id, max_n, tok, stored).reshape(B * T, d), matched.reshape(-1)


def _combine(fg, mode, base_t, wpe_t, pid):
    """(base + fg) + wpe[pos] in fp32 from the fp32 upcasts of the tensors the kernel is given; fg replaces base where the paper's
    lookup matched."""
    b32 = base_t.float().cpu().numpy().reshape(-1, base_t.shape[-1])
    if mode == "cover":
        e = b32 + fg
    else:
        rows, matched = fg
        e = np.where(matched[:, None], rows, b32)
    if wpe_t is None:
        return e
    return e + wpe_t.float().cpu().numpy()[np.asarray(pid).reshape(-1)]


def _handle(fmt, d, max_n, mode="cover", **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = WS._vocabulary(max_n)
    table = _tables(fmt, d, max_n)[0]
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt, lookup_mode=mode, **kw)
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return cache


def _guarded(n, d, dt):
    buf = torch.full((n + GUARD, d), float("nan"), dtype=dt, device="cuda")
    return buf, buf[:n]


def _assert_guard(buf, n):
    assert bool(torch.isnan(buf[n:]).all()), "a guard row behind the output was written"


def _assert_bits(out, want32, dt, tag):
    assert want32.dtype == np.float32 and np.isfinite(want32).all()
    g, w = WS._bits(out.reshape(want32.shape)), WS._bits(WS._to(want32, dt))
    assert E.same_bits(g, w), f"{tag}: {VL._differing(g, w)}"


def _run_rect(fmt, d, max_n, B, T, mode, reduce, positions, dtype, wpe, via="table", table=None, **handle_kw):
    """One rectangular lookup onto a dense base against the oracle.  via="table": SconeTable.embed_base; "cache": embed_tokens."""
    tok, pos, _, _ = _batch(B, T, max_n)
    dt = DTYPES[dtype]
    base_t = WS._to(_base32(B * T, d), dt).cuda()
    wpe_t = WS._to(_tables(fmt, d, max_n)[2], dt).cuda() if wpe else None
    cache = _handle(fmt, d, max_n, mode, **handle_kw) if table is None else None
    t = cache.table if table is None else table
    buf, out = _guarded(B * T, d, dt)
    pid_t = torch.from_numpy(pos) if (positions == "random" and wpe) else None
    if via == "cache":
        assert mode == "cover"
        got = cache.embed_tokens(torch.from_numpy(tok), base=base_t.view(B, T, d), reduce=reduce, wpe=wpe_t, position_ids=pid_t,
                                 out=out, check=True)
    else:
        got = t.embed_base(torch.from_numpy(tok), base_t, wpe=wpe_t, position_ids=pid_t, reduce=reduce, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == dt
    pid = pos if pid_t is not None else np.broadcast_to(np.arange(T), (B, T))
    want = _combine(_fgram(fmt, d, max_n, B, T, mode, reduce), mode, base_t, wpe_t, pid)
    tag = f"{fmt}-d{d}-n{max_n}-{B}x{T}-{mode}-{reduce}-pos_{positions}-{dtype}-wpe{int(wpe)}-{via}"
    _assert_bits(out, want, dt, tag)
    _assert_guard(buf, B * T)
    assert t.status() == 0
    return cache


# ------------------------------------------------------------------ 1. the one-launch form (k_embed_fused)
def _one_launch_cases():
    out, rot = [], ("fp32", "fp16", "bf16")
    k = 0
    for fmt, d in FORMATS_1024 + [("int8", 768), ("fp16", 1280)]:
        for B, T in ((6, 37), (3, 5)):
            max_n = (3, 4)[k % 2]
            mode = MODES[(k // 2) % 2]
            reduce = "sum" if (mode == "cover" and k % 3 == 0) else "mean"
            positions = ("default", "random")[(k // 2 + k) % 2]
            out.append((fmt, d, max_n, B, T, mode, reduce, positions, rot[k % 3], k % 4 != 3))
            k += 1
    # both modes at max_n = 3 and 4 with both kinds of positions, whatever the rotation above gave them
    for j, (max_n, mode, positions) in enumerate((n, m, p) for n in (3, 4) for m in MODES for p in ("default", "random")):
        out.append(("int8", 1024, max_n, 6, 37, mode, "mean", positions, rot[j % 3], True))
    uniq = list(dict.fromkeys(out))
    return [pytest.param(*c, id="-".join(str(x) for x in c[:9]) + f"-wpe{int(c[9])}") for c in uniq]


@pytest.mark.parametrize("fmt,d,max_n,B,T,mode,reduce,positions,dtype,wpe", _one_launch_cases())
def test_one_launch_form(monkeypatch, fmt, d, max_n, B, T, mode, reduce, positions, dtype, wpe):
    """k_embed_fused: the base row is indexed by p; tok[p] still feeds the match windows."""
    _form(monkeypatch, "one_launch")
    _run_rect(fmt, d, max_n, B, T, mode, reduce, positions, dtype, wpe, via="cache" if mode == "cover" else "table")


# ------------------------------------------------------------------ 2. the two-kernel form (k_match_ell + k_embed_wave)
def _two_kernel_cases():
    out, rot = [], ("fp16", "fp32", "bf16")
    k = 0
    for fmt, d in [("int8", 768), ("fp16", 1024), ("fp32", 768), ("int4", 1024), ("bf16", 1024)]:
        for B, T in ((12301, 3), (1243, 37), (7, 5)):
            max_n = (3, 4)[(k // 3 + k) % 2]
            mode = MODES[1] if k % 5 == 4 else MODES[0]
            reduce = "sum" if (mode == "cover" and k % 4 == 1) else "mean"
            positions = ("default", "random")[k % 2]          # default: the HIOCC instantiation; random: explicit positions
            out.append((fmt, d, max_n, B, T, mode, reduce, positions, rot[k % 3], k % 7 != 6))
            k += 1
    # the headline instantiation and its explicit-position twin on both walk shapes
    for B, T in ((12301, 3), (1243, 37)):
        for positions in ("default", "random"):
            out.append(("int8", 768, 3, B, T, "cover", "mean", positions, "fp16", True))
    uniq = list(dict.fromkeys(out))
    return [pytest.param(*c, id="-".join(str(x) for x in c[:9]) + f"-wpe{int(c[9])}") for c in uniq]


@pytest.mark.parametrize("fmt,d,max_n,B,T,mode,reduce,positions,dtype,wpe", _two_kernel_cases())
def test_two_kernel_form(monkeypatch, fmt, d, max_n, B, T, mode, reduce, positions, dtype, wpe):
    """k_embed_wave: the walk p += T gives the base row.  12301 x 3 makes a workgroup walk several sequences; 1243 x 37 and
    7 x 5 leave tail waves with i >= T."""
    _form(monkeypatch, "two_kernels")
    if (B, T) == (12301, 3):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert WS.G.wave(B, T, cus).seqs_per_block > 1
    _run_rect(fmt, d, max_n, B, T, mode, reduce, positions, dtype, wpe)


def test_cu_reserve_masked_stream(monkeypatch):
    """The lookup kernel on the handle's masked stream, tied into the caller's stream by two events."""
    _form(monkeypatch, "two_kernels")
    cache = _handle("int8", 768, 3)
    cache.table.set_cu_reserve(16)
    assert cache.table.cu_reserve()[0] == 16
    _run_rect("int8", 768, 3, 1243, 37, "cover", "mean", "default", "fp16", True, table=cache.table)


@pytest.mark.parametrize("mode,positions", [("cover", "default"), ("longest_suffix", "random")])
def test_any_dim_kernel(monkeypatch, mode, positions):
    """k_embed_wave_any (d % 8 == 0 outside 768 / 1024 / 1280): fp16, d = 4096."""
    _form(monkeypatch, "two_kernels")
    _run_rect("fp16", 4096, 3, 5, 9, mode, "mean", positions, "fp16", True)


@pytest.mark.parametrize("dtype,wpe", [("fp32", True), ("fp16", False)])
def test_lane_group_fallback(dtype, wpe):
    """k_embed (d % 8 != 0): fp32 table, d = 20."""
    _run_rect("fp32", 20, 3, 4, 7, "cover", "mean", "random", dtype, wpe)


# ------------------------------------------------------------------ 3. shard ownership
@functools.lru_cache(maxsize=None)
def _shard_setup(d):
    rng = np.random.default_rng(2200)
    n, vocab, max_n = 3000, 13, 3
    lens = rng.integers(1, max_n + 1, size=n).astype(np.uint8)
    keys = rng.integers(0, vocab, size=(n, max_n)).astype(np.uint32)
    keys[np.arange(max_n)[None, :] >= lens[:, None]] = 0
    table = rng.standard_normal((n, d)).astype(np.float32)
    return keys, lens, table, vocab


@pytest.mark.parametrize("form,B,T", [("two_kernels", 7, 37), ("one_launch", 6, 37)])
def test_row_shard_owns_part_of_the_ids(monkeypatch, form, B, T):
    """row_begin, row_end = 1000, 2200: owned rows only, divisor = the full K."""
    from scone_amd.hip_backend import SconeTable
    _form(monkeypatch, form)
    lo, hi, d, max_n, dt = 1000, 2200, 768, 3, torch.float32
    keys, lens, table, vocab = _shard_setup(d)
    rng = np.random.default_rng(B * T)
    tok = rng.integers(0, vocab, size=(B, T)).astype(np.int64)
    pos = rng.integers(0, N_POS, size=(B, T)).astype(np.int64)
    off, ids = R.hits_to_csr(R.match_hits(keys, lens, tok, max_n))
    stored = WS._stored(table, "int8")
    sums, kown = WS._own_sums(stored, off, ids, lo, hi)
    kfull = np.diff(off)
    assert (kown < kfull).any() and (kown > 0).any() and (kfull > 1).any()
    kf = kfull.astype(np.float32)[:, None]
    fg = np.where(kf > 1, sums / np.maximum(kf, np.float32(1)), sums).astype(np.float32)
    t = SconeTable(max_n, len(lens), d, "int8", row_begin=lo, row_end=hi)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(table[lo:hi]), row0=lo)
    base_t = torch.from_numpy(_base32(B * T, d, seed=1)).cuda()
    wpe_t = torch.from_numpy(_tables("int8", d, max_n)[2]).cuda()
    buf, out = _guarded(B * T, d, dt)
    t.embed_base(torch.from_numpy(tok), base_t, wpe=wpe_t, position_ids=torch.from_numpy(pos), out=out)
    _assert_bits(out, _combine(fg, "cover", base_t, wpe_t, pos), dt, f"shard-{form}")
    _assert_guard(buf, B * T)
    assert t.status() == 0


# ------------------------------------------------------------------ 4. packed batches
def _expected_packed(batch, fmt, d, max_n, mode, reduce, positions, base_t, wpe_t):
    tok, cu, pos = VL._batch(batch)
    fg = VL._fgram_oracle(batch, fmt, d, max_n, mode, reduce)
    if mode == "cover":
        rows, which = fg
        fg = rows[which]
    pid = pos % N_POS if positions == "random" else VL._default_positions(cu)
    return _combine(fg, mode, base_t, wpe_t, pid)


def _run_packed(monkeypatch, form, varlen_t, fmt, d, max_n, mode, reduce, positions, dtype, via):
    _form(monkeypatch, form)
    if varlen_t is None:
        monkeypatch.delenv("SCONE_VARLEN_T", raising=False)
    else:
        monkeypatch.setenv("SCONE_VARLEN_T", str(varlen_t))
    tok, cu, pos = VL._batch("small")
    total = int(cu[-1])
    if varlen_t:
        assert total > 3 * varlen_t and total % varlen_t != 0      # a main launch of several rows AND a remainder launch
    dt = DTYPES[dtype]
    _, _, _, wpe32 = VL._tables(fmt, d, max_n)
    wpe_t = WS._to(wpe32[:N_POS + 3000], dt).cuda()                  # the default position is p - cu[s]: up to the longest sequence
    base_t = WS._to(_base32(total, d, seed=2), dt).cuda()
    cache = VL._handle(fmt, d, max_n, mode)
    buf, out = _guarded(total, d, dt)
    cu32 = torch.from_numpy(cu.astype(np.int32))
    pid_t = torch.from_numpy(pos % N_POS) if positions == "random" else None
    if via == "cache":
        got = cache.embed_tokens(torch.from_numpy(tok), cu_seqlens=cu32, base=base_t, reduce=reduce, wpe=wpe_t, position_ids=pid_t,
                                 out=out, check=True)
    else:
        got = cache.table.embed_base_varlen(torch.from_numpy(tok), cu32.cuda(), base_t, wpe=wpe_t, position_ids=pid_t,
                                            reduce=reduce, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (total, d)
    want = _expected_packed("small", fmt, d, max_n, mode, reduce, positions, base_t, wpe_t)
    _assert_bits(out, want, dt, f"packed-{form}-T{varlen_t}-{fmt}-d{d}-n{max_n}-{mode}-{reduce}-pos_{positions}-{dtype}-{via}")
    _assert_guard(buf, total)
    assert cache.table.status() == 0


@pytest.mark.parametrize("fmt,d,max_n,mode,reduce,positions,dtype,via", [
    ("int8", 768, 3, "cover", "mean", "default", "fp16", "cache"),
    ("fp16", 1024, 4, "longest_suffix", "mean", "random", "fp32", "table"),
    ("fp32", 1280, 3, "cover", "sum", "random", "bf16", "cache"),
])
def test_packed_one_launch(monkeypatch, fmt, d, max_n, mode, reduce, positions, dtype, via):
    """k_embed_fused<VARLEN> on the small batch of tests/test_gpu_varlen.py."""
    VL._assert_small_batch_shape(max_n)
    _run_packed(monkeypatch, "one_launch", None, fmt, d, max_n, mode, reduce, positions, dtype, via)


@pytest.mark.parametrize("varlen_t", [37, None])
@pytest.mark.parametrize("fmt,d,max_n,mode,positions,dtype,via", [
    ("int8", 768, 3, "cover", "default", "fp16", "cache"),
    ("fp16", 1024, 4, "longest_suffix", "random", "fp32", "table"),
    ("int8", 2048, 3, "cover", "default", "fp32", "table"),           # k_embed_wave_any
])
def test_packed_two_kernels(monkeypatch, varlen_t, fmt, d, max_n, mode, positions, dtype, via):
    """SCONE_VARLEN_T=37: the main launch walks [total / 37, 37] and a remainder launch takes the tokens left over -- its tok, pos,
    records, out AND base start main_tok rows in.  Unset: the stream as one row."""
    _run_packed(monkeypatch, "two_kernels", varlen_t, fmt, d, max_n, mode, "mean", positions, dtype, via)


@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
@pytest.mark.parametrize("B,T,max_n", [(1243, 37, 4), (7, 5, 3)])
def test_rectangle_as_packed_batch_is_bit_identical(monkeypatch, B, T, max_n, form):
    """cu = arange(B + 1) * T: embed_base_varlen equals embed_base on the same handle, bit for bit."""
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0" if form == "two_kernels" else str(1 << 20))
    d, dt = 768, torch.float16
    tok = torch.from_numpy(_batch(B, T, max_n)[0].astype(np.int32)).cuda()
    base_t = WS._to(_base32(B * T, d, seed=3), dt).cuda()
    wpe_t = WS._to(_tables("int8", d, max_n)[2], dt).cuda()
    t = _handle("int8", d, max_n).table
    want = torch.full((B, T, d), float("nan"), dtype=dt, device="cuda")
    t.embed_base(tok, base_t, wpe=wpe_t, out=want)
    assert not bool(torch.isnan(want).any())
    buf, out = _guarded(B * T, d, dt)
    cu = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
    t.embed_base_varlen(tok.view(-1), cu, base_t, wpe=wpe_t, out=out)
    g, w = WS._bits(out), WS._bits(want.view(B * T, d))
    assert E.same_bits(g, w), VL._differing(g, w)
    _assert_guard(buf, B * T)
    assert t.status() == 0


# ------------------------------------------------------------------ 5. pinned-host tables
def test_staged_pinned_host_table_moves_the_base_with_every_chunk():
    """stage_tokens = 128, T = 37: chunks of 3 sequences, B = 7 -> 3 chunks, the last of one sequence.  Every chunk is a launch on a
    slice of the batch: its tok, pos, out and base start t0 rows in."""
    fmt, d, max_n, B, T = "int8", 768, 3, 7, 37
    cache = _handle(fmt, d, max_n, placement="pinned_host", hot_rows=16, stage_tokens=128)
    t = cache.table
    before = t.stage_counters()["chunks"]
    _run_rect(fmt, d, max_n, B, T, "cover", "mean", "random", "fp16", True, table=t)
    c = t.stage_counters()
    assert c["chunk_tokens"] // T == 3 and c["chunks"] - before == 3, c
    _run_rect(fmt, d, max_n, B, T, "cover", "sum", "default", "fp32", False, table=t)


def test_pinned_host_table_read_in_place(monkeypatch):
    _form(monkeypatch, "two_kernels")
    _run_rect("int8", 768, 3, 6, 37, "cover", "mean", "default", "fp16", True, placement="pinned_host", hot_rows=16)


# ------------------------------------------------------------------ 6. in place
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("form,B,T", [("two_kernels", 1243, 37), ("one_launch", 6, 37)])
def test_out_is_base(monkeypatch, form, B, T, dtype):
    """d_out == d_base: the same bits as out of place (a wave reads the words of row p in the lanes that store them)."""
    _form(monkeypatch, form)
    fmt, d, max_n, dt = "int8", 768, 3, DTYPES[dtype]
    tok = torch.from_numpy(_batch(B, T, max_n)[0])
    t = _handle(fmt, d, max_n).table
    wpe_t = WS._to(_tables(fmt, d, max_n)[2], dt).cuda()
    base_t = WS._to(_base32(B * T, d, seed=4), dt).cuda()
    want = t.embed_base(tok, base_t, wpe=wpe_t).clone()
    buf, rows = _guarded(B * T, d, dt)
    rows.copy_(base_t)
    got = t.embed_base(tok, rows, wpe=wpe_t, out=rows)
    assert got.data_ptr() == rows.data_ptr()
    g, w = WS._bits(rows), WS._bits(want.view(B * T, d))
    assert E.same_bits(g, w), VL._differing(g, w)
    assert not E.same_bits(WS._bits(base_t), w)                  # the lookup changed the rows
    _assert_guard(buf, B * T)
    # ... and through embed_tokens(out=base), packed
    cache_rows = base_t.clone()
    cu = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
    t.embed_base_varlen(tok.view(-1), cu, cache_rows, wpe=wpe_t, out=cache_rows)
    assert E.same_bits(WS._bits(cache_rows), w)
    assert t.status() == 0


@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
def test_partial_overlap_is_refused(monkeypatch, form):
    """base shifted by one row inside one allocation: SCONE_EINVAL through SconeTable, the buffer untouched."""
    _form(monkeypatch, form)
    fmt, d, max_n, B, T, dt = "int8", 768, 3, 6, 37, torch.float16
    tok = torch.from_numpy(_batch(B, T, max_n)[0])
    t = _handle(fmt, d, max_n).table
    buf = WS._to(_base32(B * T + 1, d, seed=5), dt).cuda()
    before = buf.clone()
    cu = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
    for base, out in ((buf[:B * T], buf[1:]), (buf[1:], buf[:B * T])):
        with pytest.raises(ValueError, match="overlaps"):
            t.embed_base(tok, base, out=out)
        with pytest.raises(ValueError, match="overlaps"):
            t.embed_base_varlen(tok.view(-1), cu, base, out=out)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int16), before.view(torch.int16))
    assert t.status() == 0


# ------------------------------------------------------------------ 7. identity with the earlier road
@pytest.mark.parametrize("form", ["one_launch", "two_kernels"])
@pytest.mark.parametrize("fmt", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [768, 1024, 1280])
def test_identity_with_match_csr_plus_gather_reduce(monkeypatch, form, fmt, d):
    """Cover mode: embed_base(tok, base) == gather_reduce(*match_csr(tok), base=base), bit for bit, on the edge-value inputs
    tests/test_gpu_edge_values.py feeds to embed_tokens(base=...): signed zeros, NaN payloads, infinities, subnormals."""
    _form(monkeypatch, form)
    max_n = 3
    keys, lens = E.vocabulary(max_n)
    table = E.table(len(lens), d, seed=9)
    from scone_amd import EmbeddingCache, NGramExtractor
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt)
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    t = cache.table
    for si, tok in enumerate(E.streams(max_n)):
        B, T = tok.shape
        bb, _ = E.wte_wpe(B * T, 1, d, seed=20 + si)
        tok_t = torch.from_numpy(tok)
        for reduce in ("mean", "sum"):
            for dt in DTYPES.values():
                b = WS._to(bb, dt).cuda()
                want = t.gather_reduce(*t.match_csr(tok_t), reduce, base=b, out_dtype=dt)
                buf, out = _guarded(B * T, d, dt)
                t.embed_base(tok_t, b, reduce=reduce, out=out)
                assert E.same_bits(WS._bits(out), WS._bits(want)), (fmt, d, si, reduce, str(dt), E.first_difference(WS._bits(out), WS._bits(want)))
                got = cache.embed_tokens(tok_t, base=b.view(B, T, d), reduce=reduce)
                assert got.dtype == dt and E.same_bits(WS._bits(got.view(B * T, d)), WS._bits(want))
    assert t.status() == 0


# ------------------------------------------------------------------ 8. routing of embed_tokens(base=...)
def _count_match_csr(monkeypatch):
    from scone_amd.hip_backend import SconeTable
    calls, real = [], SconeTable.match_csr

    def counted(self, tok):
        calls.append(tuple(tok.shape))
        return real(self, tok)
    monkeypatch.setattr(SconeTable, "match_csr", counted)
    return calls


def test_cover_cache_does_not_take_the_csr_road(monkeypatch):
    from scone_amd.hip_backend import SconeTable

    def refuse(self, tok):
        raise AssertionError("embed_tokens(base=) went through SconeTable.match_csr")
    cache = _handle("int8", 768, 3)
    monkeypatch.setattr(SconeTable, "match_csr", refuse)
    _run_rect("int8", 768, 3, 6, 37, "cover", "mean", "default", "fp16", False, via="cache")
    tok = torch.from_numpy(_batch(3, 5, 3)[0])
    base = torch.from_numpy(_base32(15, 768)).view(3, 5, 768)
    got = cache.embed_tokens(tok, base=base)                           # a host base is converted, as before
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 5, 768) and got.is_cuda
    want = _combine(_fgram("int8", 768, 3, 3, 5, "cover", "mean"), "cover", base.view(15, 768), None, None)
    _assert_bits(got, want, torch.float32, "host base")


def test_longest_suffix_cache_keeps_the_csr_road(monkeypatch):
    calls = _count_match_csr(monkeypatch)
    B, T, d, max_n = 3, 5, 768, 3
    cache = _handle("int8", d, max_n, "longest_suffix")
    tok = torch.from_numpy(_batch(B, T, max_n)[0])
    base_t = torch.from_numpy(_base32(B * T, d)).cuda()
    got = cache.embed_tokens(tok, base=base_t.view(B, T, d))
    assert calls == [(B, T)]
    # today's result exactly: base + the mean of ALL covering f-grams
    want = _combine(_fgram("int8", d, max_n, B, T, "cover", "mean"), "cover", base_t, None, None)
    _assert_bits(got, want, torch.float32, "longest_suffix cache, earlier road")
    wpe_t = torch.from_numpy(_tables("int8", d, max_n)[2]).cuda()
    for kw in (dict(wpe=wpe_t), dict(position_ids=torch.zeros((B, T), dtype=torch.int64)), dict(out=torch.empty_like(base_t))):
        with pytest.raises(ValueError, match="table.embed_base"):
            cache.embed_tokens(tok, base=base_t.view(B, T, d), **kw)
    with pytest.raises(ValueError, match="table.embed_base"):
        cache.embed_tokens(tok.view(-1), base=base_t, cu_seqlens=[0, 7, 15])
    assert calls == [(B, T)] and cache.table.status() == 0


# ------------------------------------------------------------------ 9. the status word
@pytest.mark.parametrize("form", ["one_launch", "two_kernels"])
def test_status_bit_is_for_positions_only(monkeypatch, form):
    """A token id of 2^31 - 1 (and a negative one) matches nothing and raises no bit: there is no vocabulary.  A position id equal
    to n_pos raises bit 0 and reads a row of zeros."""
    _form(monkeypatch, form)
    fmt, d, max_n, B, T, dt = "int8", 768, 3, 6, 37, torch.float32
    tok, pos, _, _ = _batch(B, T, max_n)
    tok = tok.copy()
    tok[1, 3], tok[4, 0], tok[5, T - 1] = 2**31 - 1, -5, 2**31 - 1
    off, ids = R.hits_to_csr(R.match_hits(*WS._vocabulary(max_n), np.where(tok > VOCAB, VOCAB, np.where(tok < 0, VOCAB, tok)), max_n))
    fg = R.embed_numpy(_tables(fmt, d, max_n)[1], off, ids, "mean")      # token VOCAB is in no f-gram either
    t = _handle(fmt, d, max_n).table
    base_t = torch.from_numpy(_base32(B * T, d, seed=6)).cuda()
    wpe_t = torch.from_numpy(_tables(fmt, d, max_n)[2]).cuda()
    buf, out = _guarded(B * T, d, dt)
    t.embed_base(torch.from_numpy(tok.astype(np.int32)), base_t, wpe=wpe_t, position_ids=torch.from_numpy(pos), out=out)
    assert t.status() == 0
    _assert_bits(out, _combine(fg, "cover", base_t, wpe_t, pos), dt, f"wide tokens-{form}")
    bad = pos.copy()
    bad[2, 2] = N_POS
    t.embed_base(torch.from_numpy(tok.astype(np.int32)), base_t, wpe=wpe_t, position_ids=torch.from_numpy(bad), out=out)
    assert t.status() & 1
    want = _combine(fg, "cover", base_t, wpe_t, pos)
    want[2 * T + 2] = (base_t.float().cpu().numpy()[2 * T + 2] + fg[2 * T + 2])
    _assert_bits(out, want, dt, f"position n_pos-{form}")
    _assert_guard(buf, B * T)
    assert t.status() == 0
