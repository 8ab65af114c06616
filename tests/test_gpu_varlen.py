"""Packed variable-length batches (`scone_embed_varlen`, `embed_tokens(..., cu_seqlens=...)`) against the oracle.

The packed call promises: token p of sequence s gets exactly what the rectangular call gives it when sequence s is passed
alone.  So the expectation is built on the host ONE SEQUENCE AT A TIME -- `R.match_hits(keys, lens, tok[None, cu[s]:cu[s+1]],
max_n)` -> `R.hits_to_csr` -> `R.embed_numpy` (`R.paper_embed` for the paper's lookup) -- concatenated, and combined as
`(wte + fg) + wpe[pos]` in fp32.  (The per-sequence CSR lists are concatenated and `R.embed_numpy` runs once per distinct
list: it reduces every token's list on its own, so the values are those of one call per sequence.)

The bar has no tolerance: fp32 output equals the expectation bit for bit, fp16 / bf16 output equals it rounded once.  Every
call writes into the first `total` rows of a NaN-filled buffer of `total + 64` rows; the 64 guard rows must still be NaN
afterwards and `table.status()` must be 0.

Set-up as in tests/test_gpu_walk_shapes.py (its 3-token vocabularies plus a fourth token in no f-gram, its N_ROWS, tables
quantised on the host by oracle/ref_port.py, `edge_fixture.same_bits`).

Preconditions, asserted on the CPU before the GPU's answer is looked at: matching the packed stream as ONE sequence changes the
id list of a token within max_n - 1 of the boundary at two thirds or more of the interior boundaries (a window that crosses a
boundary cannot go unnoticed), and every list length 0..max_n(max_n+1)/2 occurs in cover mode.

The small batch (~3,000 tokens) has sequences of exactly one default tile of the match kernel (254 positions for max_n <= 3,
253 for 4), one token less, one more and two tiles -- consecutive boundaries keep, lose or gain one position against the tile
grid -- empty sequences at the front, in a run and at the very end, sequences shorter than max_n and sequences longer than two
tiles.  Every alignment of a sequence boundary to a tile boundary is met by the SCONE_MATCH_TILE = 7 / 5 cases.
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_fixture as E  # noqa: E402
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, host quantisation, rounding, bit views)

pytestmark = pytest.mark.gpu

VOCAB, TOKEN_P, N_ROWS, DTYPES = WS.VOCAB, WS.TOKEN_P, WS.N_ROWS, WS.DTYPES
N_POS = 3072                 # rows of wpe: more than the longest sequence here (3001) -- the default position is p - cu[s]
GUARD = 64
SMALL_HEAD = [0, 1, 2, 3, 0, 0, 5, 1, 1, 7, 254, 253, 255, 1, 508, 2, 4, 3, 600, 0]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


def _two_kernels(monkeypatch):
    """SCONE_FUSED_MAX_TOKENS=0 is read when a handle is created: match kernel + large-batch kernel whatever the size."""
    monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", "0")


def _one_launch(monkeypatch, limit=None):
    if limit is None:
        monkeypatch.delenv("SCONE_FUSED_MAX_TOKENS", raising=False)
    else:
        monkeypatch.setenv("SCONE_FUSED_MAX_TOKENS", str(limit))


# ------------------------------------------------------------------ inputs and expectations (host only)
@functools.lru_cache(maxsize=None)
def _lengths(batch):
    if batch == "small":
        rng = np.random.default_rng(20249)        # the first seed from 20240 on whose 60th length is 0: an empty sequence at the very end
        return tuple(SMALL_HEAD + rng.integers(0, 38, size=60).tolist())
    if batch == "tiny":                       # below any plausible row length of the gather traversal
        return (0, 17, 3, 0, 1, 29, 11, 0)    # 61 tokens
    assert batch == "large"                   # ~40,000 tokens, a prime total: a main part AND a remainder of any factorisation
    rng = np.random.default_rng(20241)
    lens = rng.integers(0, 38, size=1640).tolist()
    for at, n in ((100, 3001), (777, 2999), (1500, 3000)):
        lens.insert(at, n)
    total = sum(lens)
    want = total
    while any(want % k == 0 for k in range(2, int(want ** 0.5) + 1)):
        want += 1
    lens[-1] += want - total
    return tuple(lens)


@functools.lru_cache(maxsize=None)
def _batch(batch):
    """Packed tokens [total], cu [n + 1], random positions [total] (all int64 numpy)."""
    lens = np.asarray(_lengths(batch), dtype=np.int64)
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cu[1:])
    rng = np.random.default_rng({"small": 31, "tiny": 32, "large": 33}[batch])
    tok = rng.choice(VOCAB + 1, size=int(cu[-1]), p=TOKEN_P).astype(np.int64)
    pos = rng.integers(0, N_POS, size=int(cu[-1])).astype(np.int64)
    return tok, cu, pos


def _csr_of(tok2d, max_n):
    keys, lens = WS._vocabulary(max_n)
    return R.hits_to_csr(R.match_hits(keys, lens, tok2d, max_n))


@functools.lru_cache(maxsize=None)
def _lists(batch, max_n):
    """CSR id lists of the packed batch, every sequence matched on its own: (offsets [total + 1], ids)."""
    tok, cu, _ = _batch(batch)
    offs, ids, base = [np.zeros(1, dtype=np.int64)], [], 0
    for s in range(len(cu) - 1):
        if cu[s + 1] == cu[s]:
            continue
        off, i = _csr_of(tok[None, cu[s]:cu[s + 1]], max_n)
        offs.append(off[1:] + base)
        ids.append(i)
        base += off[-1]
    return np.concatenate(offs), (np.concatenate(ids) if ids else np.zeros(0, dtype=np.int64))


@functools.lru_cache(maxsize=None)
def _tables(fmt, d, max_n):
    """(fp32 rows given to the handle, the same rows as the format stores them, wte[VOCAB + 1, d], wpe[N_POS, d])."""
    rng = np.random.default_rng(11 * d + max_n)
    table = rng.standard_normal((N_ROWS[max_n], d)).astype(np.float32)
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return table, WS._stored(table, fmt), wte, wpe


@functools.lru_cache(maxsize=2)
def _fgram_oracle(batch, fmt, d, max_n, mode, reduce):
    """The f-gram part, fp32.  cover: (the reduced rows of the distinct lists [u, d], every token's list number [total]).  longest_suffix: (row of the longest f-gram ending at the token
    or zeros, the mask of matched tokens)."""
    stored = _tables(fmt, d, max_n)[1]
    tok, cu, _ = _batch(batch)
    if mode == "cover":
        # R.embed_numpy reduces every token's list on its own, so it is run once per DISTINCT list (a 4-token alphabet has few
        # hundred of them) and the rows are dealt back to the tokens: the same values, without ten passes over [total, d]
        off, ids = _lists(batch, max_n)
        kmax = max_n * (max_n + 1) // 2
        padded = np.full((len(off) - 1, kmax), -1, dtype=np.int64)
        counts = np.diff(off)
        for k in range(kmax):
            m = counts > k
            padded[m, k] = ids[off[:-1][m] + k]
        uniq, inverse = np.unique(padded, axis=0, return_inverse=True)
        ucounts = (uniq >= 0).sum(axis=1)
        uoff = np.zeros(len(uniq) + 1, dtype=np.int64)
        np.cumsum(ucounts, out=uoff[1:])
        return R.embed_numpy(stored, uoff, uniq[uniq >= 0], reduce), inverse.reshape(-1)
    f2id = R._key_dict(*WS._vocabulary(max_n))
    parts, matched = [], []
    for s in range(len(cu) - 1):
        seq = tok[cu[s]:cu[s + 1]]
        if len(seq):
            parts.append(R.paper_embed(f2id, max_n, seq[None, :], stored)[0])
            matched.append(np.asarray(R.paper_lookup(f2id, max_n, seq.tolist())) >= 0)
    return np.concatenate(parts), np.concatenate(matched)


def _default_positions(cu):
    total = int(cu[-1])
    seq = np.searchsorted(cu, np.arange(total), side="right") - 1
    return np.arange(total) - cu[seq]


def _expected(batch, fmt, d, max_n, mode, reduce, positions, wte_t, wpe_t):
    """fp32 [total, d]: (wte + f-gram) + wpe[pos] from the fp32 upcasts of the wte / wpe the kernel is given (None: term 0)."""
    tok, cu, pos = _batch(batch)
    fg = _fgram_oracle(batch, fmt, d, max_n, mode, reduce)
    pid = pos if positions == "random" else _default_positions(cu)
    zero = np.zeros((1, d), dtype=np.float32)
    wpe_rows = wpe_t.float().cpu().numpy()[pid] if wpe_t is not None else zero
    if mode == "cover":
        rows, which = fg
        if wte_t is None:
            return (zero + rows)[which] + wpe_rows
        # wte[tok] + fg once per distinct (token, list) pair, dealt back to the tokens
        pair, back = np.unique(which * (VOCAB + 1) + tok, return_inverse=True)
        return (wte_t.float().cpu().numpy()[pair % (VOCAB + 1)] + rows[pair // (VOCAB + 1)])[back.reshape(-1)] + wpe_rows
    e, matched = fg
    if wte_t is not None:
        e = np.where(matched[:, None], e, wte_t.float().cpu().numpy()[tok])
    return e + wpe_rows


# ------------------------------------------------------------------ preconditions
def _assert_small_batch_shape(max_n):
    lens = np.asarray(_lengths("small"))
    _, cu, _ = _batch("small")
    tile = 256 - (2 if max_n <= 3 else 3)
    assert lens[0] == 0 and lens[-1] == 0 and (lens[4:6] == 0).all()            # empty at the front, in a run, at the end
    assert (lens[lens > 0] < max(max_n, 2)).any() and (lens > 2 * tile).any()
    assert 2900 <= cu[-1] <= 3200
    assert {tile - 1, tile, tile + 1, 2 * tile} & set(lens.tolist())              # a tile, one less, one more, two tiles


def _assert_boundaries_matter(batch, max_n):
    """Matching the packed stream as ONE sequence changes a list near >= 2/3 of the interior boundaries."""
    if max_n < 2:
        return
    tok, cu, _ = _batch(batch)
    off, ids = _lists(batch, max_n)
    off1, ids1 = _csr_of(tok[None, :], max_n)
    total = int(cu[-1])
    differs = np.zeros(total, dtype=bool)
    for p in range(total):
        differs[p] = not np.array_equal(ids[off[p]:off[p + 1]], ids1[off1[p]:off1[p + 1]])
    inner = sorted(set(cu.tolist()) - {0, total})
    changed = sum(bool(differs[max(0, b - (max_n - 1)):b + (max_n - 1)].any()) for b in inner)
    assert len(inner) >= 60 and 3 * changed >= 2 * len(inner), (max_n, changed, len(inner))


def _assert_every_list_length(batch, max_n):
    off, _ = _lists(batch, max_n)
    kmax = max_n * (max_n + 1) // 2
    hist = np.bincount(np.diff(off), minlength=kmax + 1)
    assert len(hist) == kmax + 1 and (hist > 0).all(), f"list lengths 0..{kmax}: {hist.tolist()}"


def _handle(fmt, d, max_n, mode="cover", **kw):
    from scone_amd import EmbeddingCache, NGramExtractor
    keys, lens = WS._vocabulary(max_n)
    table = _tables(fmt, d, max_n)[0]
    cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=fmt, lookup_mode=mode, **kw)
    cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
    return cache


def _guarded(total, d, dt):
    buf = torch.full((total + GUARD, d), float("nan"), dtype=dt, device="cuda")
    return buf, buf[:total]


def _assert_guard(buf, total):
    assert bool(torch.isnan(buf[total:]).all()), "a guard row behind the output was written"


def _differing(got, want):
    view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere((got.view(view) != want.view(view)).any(axis=1)).reshape(-1)
    return f"{len(bad)} of {got.shape[0]} tokens differ; first packed positions: {bad[:8].tolist()}"


def _run(batch, fmt, d, max_n, mode, reduce, positions, dtype, wte, wpe, cu_on="device", **handle_kw):
    tok, cu, pos = _batch(batch)
    total = int(cu[-1])
    if batch == "small":
        _assert_small_batch_shape(max_n)
        _assert_boundaries_matter(batch, max_n)
    if batch != "tiny":
        _assert_every_list_length(batch, max_n)
    _, _, wte32, wpe32 = _tables(fmt, d, max_n)
    dt = DTYPES[dtype]
    wte_t = WS._to(wte32, dt).cuda() if wte else None
    wpe_t = WS._to(wpe32, dt).cuda() if wpe else None
    cache = _handle(fmt, d, max_n, mode, **handle_kw)
    buf, out = _guarded(total, d, dt)
    cu32 = torch.from_numpy(cu.astype(np.int32))
    got = cache.embed_tokens(torch.from_numpy(tok), cu_seqlens=cu32.cuda() if cu_on == "device" else cu32, reduce=reduce,
                             wte=wte_t, wpe=wpe_t, position_ids=torch.from_numpy(pos) if positions == "random" else None,
                             out_dtype=dt, out=out)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (total, d)
    want = _expected(batch, fmt, d, max_n, mode, reduce, positions if wpe else "default", wte_t, wpe_t)
    assert want.shape == (total, d) and want.dtype == np.float32 and np.isfinite(want).all()
    g, w = WS._bits(out), WS._bits(WS._to(want, dt))
    tag = f"{batch}-{fmt}-d{d}-n{max_n}-{mode}-{reduce}-pos_{positions}-{dtype}-wte{int(wte)}-wpe{int(wpe)}"
    assert E.same_bits(g, w), f"{tag}: {_differing(g, w)}"
    _assert_guard(buf, total)
    assert cache.table.status() == 0
    return cache


# ------------------------------------------------------------------ 1. the two-kernel form
SETUPS = [("int8", 768), ("fp16", 1024), ("fp32", 1280), ("int4", 1024), ("int8", 2048), ("fp32", 136)]   # the last two: k_embed_wave_any
MODES = ("cover", "longest_suffix")


def _two_kernel_cases():
    out, rot = [], ("fp32", "fp16", "bf16")
    k = 0
    for s, (fmt, d) in enumerate(SETUPS):
        for max_n in (1, 2, 3, 4):
            mode = MODES[(s + max_n) % 2]
            reduce = "sum" if (mode == "cover" and (s + max_n // 2) % 2) else "mean"
            positions = ("default", "random")[(s + (max_n + 1) // 2) % 2]
            out.append((fmt, d, max_n, mode, reduce, positions, rot[k % 3], k % 5 != 4, True))
            k += 1
    # max_n = 3 / 4 in both modes with both kinds of positions, whatever the rotation above gave them
    for j, (max_n, mode, positions) in enumerate((n, m, p) for n in (3, 4) for m in MODES for p in ("default", "random")):
        fmt, d = SETUPS[j % len(SETUPS)]
        out.append((fmt, d, max_n, mode, "mean", positions, rot[(j + 1) % 3], True, True))
    # without wpe (no position array at all), with and without wte
    out.append(("int8", 768, 3, "cover", "mean", "default", "fp16", True, False))
    out.append(("fp16", 1024, 4, "longest_suffix", "mean", "default", "fp32", False, False))
    out.append(("int8", 2048, 4, "cover", "sum", "default", "bf16", True, False))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [pytest.param(*c, id="-".join(str(x) for x in c[:7]) + f"-wte{int(c[7])}-wpe{int(c[8])}") for c in uniq]


@pytest.mark.parametrize("fmt,d,max_n,mode,reduce,positions,dtype,wte,wpe", _two_kernel_cases())
def test_two_kernel_form(monkeypatch, fmt, d, max_n, mode, reduce, positions, dtype, wte, wpe):
    """k_match_ell_varlen + k_embed_wave / k_embed_wave_any on the small batch."""
    _two_kernels(monkeypatch)
    _run("small", fmt, d, max_n, mode, reduce, positions, dtype, wte, wpe)


# ------------------------------------------------------------------ 2. tiny match tiles: a tile boundary at every alignment
@pytest.mark.parametrize("tile", [7, 5])
@pytest.mark.parametrize("max_n,mode,positions", [(3, "cover", "default"), (4, "cover", "random"),
                                                  (3, "longest_suffix", "random"), (4, "longest_suffix", "default")])
def test_match_tile_boundaries_everywhere(monkeypatch, tile, max_n, mode, positions):
    """SCONE_MATCH_TILE=7 / 5: hundreds of tile boundaries fall inside and between sequences, so the halo threads meet every
    alignment of a sequence boundary."""
    _two_kernels(monkeypatch)
    monkeypatch.setenv("SCONE_MATCH_TILE", str(tile))
    _run("small", "int8", 768, max_n, mode, "mean", positions, "fp32", True, True)


# ------------------------------------------------------------------ 3. the one-launch form
@pytest.mark.parametrize("positions", ["default", "random"])
@pytest.mark.parametrize("max_n", [3, 4])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fmt,d,dtype", [("int8", 768, "fp16"), ("fp16", 1024, "fp32"), ("fp32", 1280, "bf16")])
def test_one_launch_form(monkeypatch, fmt, d, dtype, mode, max_n, positions):
    """k_embed_fused's packed form (default SCONE_FUSED_MAX_TOKENS: the small batch is far below it)."""
    _one_launch(monkeypatch)
    _run("small", fmt, d, max_n, mode, "mean", positions, dtype, True, True, cu_on=("device", "host")[max_n % 2])


# ------------------------------------------------------------------ 4. the large-batch traversal
@pytest.mark.parametrize("row", [None, 512, 37])
@pytest.mark.parametrize("fmt,d,max_n,dtype", [("int8", 768, 3, "fp32"), ("fp16", 4096, 4, "fp16")])
def test_large_batch_traversal(monkeypatch, fmt, d, max_n, dtype, row):
    """~40,000 tokens with a prime total: the default traversal (the stream as one row) and, with SCONE_VARLEN_T = 512 / 37, a
    main part [total / T', T'] that persistent workgroups walk plus a remainder launch."""
    _two_kernels(monkeypatch)
    if row is None:
        monkeypatch.delenv("SCONE_VARLEN_T", raising=False)
    else:
        monkeypatch.setenv("SCONE_VARLEN_T", str(row))
    total = int(_batch("large")[1][-1])
    assert 38_000 < total < 48_000 and all(total % k for k in range(2, int(total ** 0.5) + 1))
    assert sum(n >= 2999 for n in _lengths("large")) == 3
    _run("large", fmt, d, max_n, "cover", "mean", "default", dtype, True, True)


@pytest.mark.parametrize("fmt,d,max_n", [("int8", 768, 3), ("fp16", 4096, 4)])
def test_batch_shorter_than_one_traversal_row(monkeypatch, fmt, d, max_n):
    _two_kernels(monkeypatch)
    assert int(_batch("tiny")[1][-1]) == 61
    _run("tiny", fmt, d, max_n, "cover", "mean", "default", "fp32", True, True)


# ------------------------------------------------------------------ 5. a rectangle passed as a packed batch
@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
@pytest.mark.parametrize("B,T,max_n", [(12301, 3, 3), (1243, 37, 4), (7, 5, 3)])
def test_rectangle_as_packed_batch_is_bit_identical(monkeypatch, B, T, max_n, form, dtype):
    """cu = arange(B + 1) * T: the packed call equals embed_tokens(tok.view(B, T)) on the same handle, bit for bit."""
    if form == "two_kernels":
        _two_kernels(monkeypatch)
    else:
        _one_launch(monkeypatch, 1 << 20)       # the limit is honoured: every shape here takes one launch
    d, dt = 768, DTYPES[dtype]
    rng = np.random.default_rng(B + T)
    tok = torch.from_numpy(rng.choice(VOCAB + 1, size=B * T, p=TOKEN_P).astype(np.int32)).cuda()
    _, _, wte32, wpe32 = _tables("int8", d, max_n)
    wte_t, wpe_t = WS._to(wte32, dt).cuda(), WS._to(wpe32, dt).cuda()
    cache = _handle("int8", d, max_n)
    want = torch.full((B, T, d), float("nan"), dtype=dt, device="cuda")
    cache.embed_tokens(tok.view(B, T), wte=wte_t, wpe=wpe_t, out_dtype=dt, out=want)
    buf, out = _guarded(B * T, d, dt)
    cu = (torch.arange(B + 1, dtype=torch.int32) * T).cuda()
    cache.embed_tokens(tok, cu_seqlens=cu, wte=wte_t, wpe=wpe_t, out_dtype=dt, out=out)
    g, w = WS._bits(out), WS._bits(want.view(B * T, d))
    assert not bool(torch.isnan(want).any())
    assert E.same_bits(g, w), _differing(g, w)
    _assert_guard(buf, B * T)
    assert cache.table.status() == 0


# ------------------------------------------------------------------ 6. single sequences and degenerate input
@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
@pytest.mark.parametrize("T", [1, 2, 300])
def test_single_sequence_equals_the_rectangular_call(monkeypatch, form, T):
    _two_kernels(monkeypatch) if form == "two_kernels" else _one_launch(monkeypatch)
    d, max_n, dt = 1024, 4, torch.float32
    tok = torch.from_numpy(np.random.default_rng(T).choice(VOCAB + 1, size=T, p=TOKEN_P).astype(np.int32)).cuda()
    _, _, wte32, wpe32 = _tables("fp16", d, max_n)
    wte_t, wpe_t = torch.from_numpy(wte32).cuda(), torch.from_numpy(wpe32).cuda()
    cache = _handle("fp16", d, max_n)
    want = cache.embed_tokens(tok.view(1, T), wte=wte_t, wpe=wpe_t)
    buf, out = _guarded(T, d, dt)
    cache.embed_tokens(tok, cu_seqlens=[0, T], wte=wte_t, wpe=wpe_t, out=out)
    assert E.same_bits(WS._bits(out), WS._bits(want.view(T, d)))
    _assert_guard(buf, T)
    assert cache.table.status() == 0


@pytest.mark.parametrize("cu", [[0], [0, 0, 0, 0]])
def test_no_tokens_is_a_no_op(monkeypatch, cu):
    _two_kernels(monkeypatch)
    cache = _handle("int8", 768, 3)
    table = cache.table
    table.profile_enable(True)
    table.profile_read(reset=True)
    empty = torch.zeros(0, dtype=torch.int32, device="cuda")
    for cu_seqlens in (cu, torch.tensor(cu, dtype=torch.int32).cuda()):
        out = cache.embed_tokens(empty, cu_seqlens=cu_seqlens)
        assert tuple(out.shape) == (0, 768) and out.dtype == torch.float32
    launches, _ = table.profile_read(reset=True)
    table.profile_enable(False)
    assert launches == 0 and table.status() == 0


@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
def test_trailing_empty_sequences_are_accepted(monkeypatch, form):
    _two_kernels(monkeypatch) if form == "two_kernels" else _one_launch(monkeypatch)
    d, max_n = 768, 3
    seq = np.random.default_rng(5).choice(VOCAB + 1, size=41, p=TOKEN_P).astype(np.int32)
    tok = torch.from_numpy(np.concatenate([seq[:30], seq[30:]])).cuda()
    _, _, wte32, wpe32 = _tables("int8", d, max_n)
    wte_t, wpe_t = torch.from_numpy(wte32).cuda(), torch.from_numpy(wpe32).cuda()
    cache = _handle("int8", d, max_n)
    want = torch.cat([cache.embed_tokens(tok[None, :30], wte=wte_t, wpe=wpe_t)[0],
                      cache.embed_tokens(tok[None, 30:], wte=wte_t, wpe=wpe_t)[0]])
    buf, out = _guarded(41, d, torch.float32)
    cache.embed_tokens(tok, cu_seqlens=[0, 30, 41, 41, 41, 41], wte=wte_t, wpe=wpe_t, out=out)
    assert E.same_bits(WS._bits(out), WS._bits(want))
    _assert_guard(buf, 41)
    assert cache.table.status() == 0


def test_table_read_in_place_from_pinned_host_memory(monkeypatch):
    """placement='pinned_host' with stage_tokens = 0: the row store serves the packed call like any other."""
    _two_kernels(monkeypatch)
    _run("small", "int8", 768, 3, "cover", "mean", "default", "fp16", True, True, placement="pinned_host", hot_rows=16)


# ------------------------------------------------------------------ 7. refusals
def test_refuses_a_dim_that_is_no_multiple_of_8():
    from scone_amd.hip_backend import SconeError
    cache = _handle("fp32", 100, 3)
    buf, out = _guarded(8, 100, torch.float32)
    with pytest.raises(SconeError, match="d % 8"):
        cache.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8], out=out)
    assert bool(torch.isnan(buf).all()) and cache.table.status() == 0


def test_refuses_a_staged_pinned_host_table():
    from scone_amd.hip_backend import SconeError
    cache = _handle("int8", 768, 3, placement="pinned_host", hot_rows=16, stage_tokens=1024)
    buf, out = _guarded(8, 768, torch.float32)
    with pytest.raises(SconeError, match="stage_tokens"):
        cache.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8], out=out)
    assert bool(torch.isnan(buf).all())


def test_refuses_host_boundaries_with_a_wrong_end():
    cache = _handle("int8", 768, 3)
    buf, out = _guarded(8, 768, torch.float32)
    with pytest.raises(ValueError, match="end at"):
        cache.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=torch.tensor([0, 3, 7]), out=out)
    with pytest.raises(ValueError, match="base="):
        cache.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8], base=torch.zeros(8, 768))
    assert bool(torch.isnan(buf).all()) and cache.table.status() == 0


# ------------------------------------------------------------------ 8. pack_sequences end to end
@pytest.mark.parametrize("form", ["two_kernels", "one_launch"])
def test_pack_sequences_end_to_end(monkeypatch, form):
    _two_kernels(monkeypatch) if form == "two_kernels" else _one_launch(monkeypatch)
    from scone_amd import EmbeddingCache
    d, max_n = 1280, 3
    rng = np.random.default_rng(77)
    seqs = [rng.choice(VOCAB + 1, size=n, p=TOKEN_P).tolist() for n in (4, 0, 1, 19, 2, 0, 33, 7)]
    _, _, wte32, wpe32 = _tables("fp16", d, max_n)
    wte_t, wpe_t = torch.from_numpy(wte32).half().cuda(), torch.from_numpy(wpe32).half().cuda()
    cache = _handle("fp16", d, max_n)
    ids, cu = EmbeddingCache.pack_sequences(seqs)
    total = ids.shape[0]
    buf, out = _guarded(total, d, torch.float16)
    cache.embed_tokens(ids, cu_seqlens=cu, wte=wte_t, wpe=wpe_t, out=out, check=True)
    want = torch.cat([cache.embed_tokens(torch.tensor([s], dtype=torch.int32), wte=wte_t, wpe=wpe_t)[0] for s in seqs if s])
    assert E.same_bits(WS._bits(out), WS._bits(want))
    _assert_guard(buf, total)
    assert cache.table.status() == 0
