"""The fused lookup at chosen positions (`scone_embed_select`, `SconeTable.embed_select`, `embed_tokens(..., select=...)`)
against the oracle.

The call promises: for j in [0, n_sel), p = sel[j], `out[j]` holds exactly the bits the full lookup over the same tokens writes
to its row p -- with the dense base row, the caller's position id and the output row of OUTPUT j.  The expectation never passes
through HIP code: per j, in fp32 numpy, `(base_row_j + fg[sel[j]]) + wpe[pos_j]`, `fg` from `R.embed_numpy` over the id lists of
every sequence matched on its own (`R.paper_embed` for the paper's lookup, where a matched f-gram replaces the base row).
No tolerance: fp32 output equals the expectation bit for bit, fp16 / bf16 output equals it rounded once.  Every call writes into
a NaN-filled buffer of `n_sel + 64` rows; the 64 guard rows must still be NaN afterwards and `table.status()` must be 0.

Set-up as in tests/test_gpu_varlen.py (the walk-shapes vocabularies and alphabet, tables quantised on the host by
oracle/ref_port.py / bf16_fixture / mxfp4_fixture, `edge_fixture.same_bits`).  Batches: rectangles of 9 x 37, 33 x 3 (T below
max_n = 4) and 50 x 1 tokens drawn by `np.random.default_rng(77 * T + max_n)`, and the packed batches "tiny" (61 tokens, 8
sequences, three of them empty) and "small" (2,961 tokens, 80 sequences) of the varlen suite.

`sel` holds, shuffled: the first and last max_n positions of every non-empty sequence, for every list length K that occurs in the
batch the first position that has it, and 200 random positions drawn with replacement.  Preconditions, asserted on the CPU before
the GPU's answer is looked at: `sel` contains duplicates, is not sorted and covers every K of the batch; and -- the varlen
suite's precondition, read as that suite reads it -- at two thirds or more of the interior sequence boundaries a SELECTED position
within max_n - 1 of the boundary would get another list if the batch were matched as one sequence (per position the bar could not
be met: of the max_n positions selected on either side of a boundary the outermost one lies beyond the reach of every window
that crosses it), so a window that crosses a boundary cannot go unnoticed.  As in the varlen suite the share is asserted on the
batches that have boundaries to take a share of (its "small" with 74 interior boundaries, 33 x 3 with 32, 50 x 1 with 49); 9 x 37
has 8 and "tiny" 4, where one boundary is 12 / 25 points of the share -- there at least one crossing window must exist.
"""

import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_fixture as BF  # noqa: E402
import edge_fixture as E  # noqa: E402
import mxfp4_fixture as MX  # noqa: E402
import test_gpu_varlen as VL  # noqa: E402  (helpers only: the packed batches and their per-sequence id lists)
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, host quantisation, rounding, bit views)

pytestmark = pytest.mark.gpu

VOCAB, TOKEN_P, N_ROWS, DTYPES = WS.VOCAB, WS.TOKEN_P, WS.N_ROWS, WS.DTYPES
N_POS = 3072
GUARD = 64
RECTS = {"r37": (9, 37), "r3": (33, 3), "r1": (50, 1)}
PACKED = ("tiny", "small")
MODES = ("cover", "longest_suffix")
HIST_9x37_N4 = [25, 4, 9, 25, 28, 39, 73, 68, 40, 19, 3]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ------------------------------------------------------------------ inputs and expectations (host only)
def _stored(table, fmt):
    if fmt == "bf16":
        return BF.stored(table)
    if fmt == "mxfp4":
        return MX.stored(table)
    return WS._stored(table, fmt)


@functools.lru_cache(maxsize=None)
def _tables(fmt, d, max_n):
    """(fp32 rows given to the handle, the same rows as the format stores them, wte[VOCAB + 1, d], wpe[N_POS, d])."""
    rng = np.random.default_rng(13 * d + max_n)
    table = rng.standard_normal((N_ROWS[max_n], d)).astype(np.float32)
    wte = rng.standard_normal((VOCAB + 1, d)).astype(np.float32)
    wpe = rng.standard_normal((N_POS, d)).astype(np.float32)
    return table, _stored(table, fmt), wte, wpe


@functools.lru_cache(maxsize=None)
def _batch(batch, max_n):
    """(tokens [total] int64, cu [n + 1] int64); a rectangle is cu = arange(B + 1) * T."""
    if batch in RECTS:
        B, T = RECTS[batch]
        rng = np.random.default_rng(77 * T + max_n)
        tok = rng.choice(VOCAB + 1, size=(B, T), p=TOKEN_P).astype(np.int64).reshape(-1)
        return tok, np.arange(B + 1, dtype=np.int64) * T
    tok, cu, _ = VL._batch(batch)
    return tok, cu


@functools.lru_cache(maxsize=None)
def _lists(batch, max_n):
    """CSR id lists over the flattened positions, every sequence matched on its own (cover mode)."""
    if batch in RECTS:
        tok, _ = _batch(batch, max_n)
        off, ids = VL._csr_of(tok.reshape(RECTS[batch]), max_n)
        return np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    off, ids = VL._lists(batch, max_n)
    return np.asarray(off, dtype=np.int64), np.asarray(ids, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _sel(batch, max_n):
    """The selection of the module docstring, int64 [n_sel]."""
    tok, cu = _batch(batch, max_n)
    off, _ = _lists(batch, max_n)
    total = int(cu[-1])
    parts = []
    for s in range(len(cu) - 1):
        lo, hi = int(cu[s]), int(cu[s + 1])
        if hi > lo:
            parts.append(np.arange(lo, min(lo + max_n, hi)))
            parts.append(np.arange(max(hi - max_n, lo), hi))
    counts = np.diff(off)
    parts.append(np.asarray([int(np.argmax(counts == k)) for k in np.unique(counts)]))
    rng = np.random.default_rng(1000 * total + max_n)
    parts.append(rng.integers(0, total, size=200))
    sel = np.concatenate(parts).astype(np.int64)
    rng.shuffle(sel)
    return sel


def _assert_preconditions(batch, max_n):
    tok, cu = _batch(batch, max_n)
    off, ids = _lists(batch, max_n)
    sel = _sel(batch, max_n)
    total = int(cu[-1])
    counts = np.diff(off)
    assert sel.min() >= 0 and sel.max() < total
    assert len(np.unique(sel)) < len(sel), "sel holds no duplicates"
    assert (np.diff(sel) < 0).any(), "sel is sorted"
    assert set(np.unique(counts[sel]).tolist()) == set(np.unique(counts).tolist()), "sel misses a list length of the batch"
    kmax = max_n * (max_n + 1) // 2
    if batch == "r37":
        hist = np.bincount(counts, minlength=kmax + 1)
        assert (hist > 0).all(), f"list lengths 0..{kmax}: {hist.tolist()}"
        if max_n == 4:
            assert hist.tolist() == HIST_9x37_N4
    if batch == "small" and max_n == 4:
        assert (np.bincount(counts, minlength=kmax + 1) > 0).all()
    if batch == "tiny":
        assert total == 61 and len(cu) == 9 and int((np.diff(cu) == 0).sum()) == 3
    if batch == "small":
        assert total == 2961 and len(cu) == 81
    if max_n < 2:
        return
    # a window that crosses a boundary cannot go unnoticed
    off1, ids1 = VL._csr_of(tok[None, :], max_n)
    differs = np.asarray([not np.array_equal(ids[off[p]:off[p + 1]], ids1[off1[p]:off1[p + 1]]) for p in range(total)])
    chosen = np.zeros(total, dtype=bool)
    chosen[sel] = True
    inner = sorted(set(cu.tolist()) - {0, total})
    for b in inner:
        assert chosen[max(0, b - (max_n - 1)):b + (max_n - 1)].all(), "a position next to a boundary is not selected"
    changed = sum(bool(differs[max(0, b - (max_n - 1)):b + (max_n - 1)].any()) for b in inner)
    if len(inner) >= 30:
        assert 3 * changed >= 2 * len(inner), (batch, max_n, changed, len(inner))
    else:           # 8 boundaries (9 x 37) or 4 ("tiny"): a share of so few is noise (5 of 8 at max_n = 2); some window must cross
        assert len(inner) >= 3 and changed >= 1, (batch, max_n, changed, len(inner))


def _default_positions(cu, sel):
    seq = np.searchsorted(cu, sel, side="right") - 1
    return sel - cu[seq]


def _fgram(batch, fmt, d, max_n, mode, reduce, sel, own=None):
    """fp32 [n_sel, d]: the f-gram part of every selected position, and the mask of positions whose base row it replaces."""
    stored = _tables(fmt, d, max_n)[1]
    tok, cu = _batch(batch, max_n)
    if mode == "cover":
        off, ids = _lists(batch, max_n)
        counts = np.diff(off)[sel]
        soff = np.zeros(len(sel) + 1, dtype=np.int64)
        np.cumsum(counts, out=soff[1:])
        sids = np.concatenate([ids[off[p]:off[p + 1]] for p in sel]) if len(sel) else np.zeros(0, dtype=np.int64)
        if own is None:
            return R.embed_numpy(stored, soff, sids, reduce), np.zeros(len(sel), dtype=bool)
        sums, kown = WS._own_sums(stored, soff, sids, *own)          # owned rows only, divisor = full K
        assert (kown < counts).any() and (kown > 0).any()
        kf = counts.astype(np.float32)[:, None]
        if reduce == "mean":
            sums = np.where(kf > 1, sums / np.maximum(kf, np.float32(1)), sums).astype(np.float32)
        return sums, np.zeros(len(sel), dtype=bool)
    assert own is None
    f2id = R._key_dict(*WS._vocabulary(max_n))
    rows = np.zeros((int(cu[-1]), d), dtype=np.float32)
    matched = np.zeros(int(cu[-1]), dtype=bool)
    for s in range(len(cu) - 1):
        seq = tok[cu[s]:cu[s + 1]]
        if len(seq):
            rows[cu[s]:cu[s + 1]] = R.paper_embed(f2id, max_n, seq[None, :], stored)[0]
            matched[cu[s]:cu[s + 1]] = np.asarray(R.paper_lookup(f2id, max_n, seq.tolist())) >= 0
    return rows[sel], matched[sel]


def _expected(batch, fmt, d, max_n, mode, reduce, sel, pid, wte_t, base_t, wpe_t, own=None):
    """fp32 [n_sel, d]: (base_row_j + fg[sel[j]]) + wpe[pos_j] from the fp32 upcasts of what the kernel is given."""
    tok, _ = _batch(batch, max_n)
    fg, replaced = _fgram(batch, fmt, d, max_n, mode, reduce, sel, own)
    base = np.zeros((len(sel), d), dtype=np.float32)
    if wte_t is not None:
        base = wte_t.float().cpu().numpy()[tok[sel]]
    if base_t is not None:
        base = base_t.float().cpu().numpy().reshape(len(sel), d)
    base = np.where(replaced[:, None], np.float32(0), base)
    wpe_rows = wpe_t.float().cpu().numpy()[pid] if wpe_t is not None else np.zeros((1, d), dtype=np.float32)
    return ((base + fg) + wpe_rows).astype(np.float32)


def _cache(fmt, d, max_n, mode="cover", **kw):
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


def _differing(got, want):
    view = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    bad = np.argwhere((got.view(view) != want.view(view)).any(axis=1)).reshape(-1)
    return f"{len(bad)} of {got.shape[0]} rows differ; first j: {bad[:8].tolist()}"


def _tok_and_cu(batch, max_n):
    """What the public call gets: ([B, T] ids, None) or ([total] ids, cu)."""
    tok, cu = _batch(batch, max_n)
    if batch in RECTS:
        return torch.from_numpy(tok.reshape(RECTS[batch])), None
    return torch.from_numpy(tok), torch.from_numpy(cu.astype(np.int32))


def _inputs(batch, fmt, d, max_n, dtype, basek, positions, wpe, sel, seed=0):
    """(wte_t, base_t, wpe_t, explicit positions or None, the position of every output) for a case."""
    _, cu = _batch(batch, max_n)
    _, _, wte32, wpe32 = _tables(fmt, d, max_n)
    dt = DTYPES[dtype]
    rng = np.random.default_rng(17 * len(sel) + seed)
    wte_t = WS._to(wte32, dt).cuda() if basek == "wte" else None
    base_t = WS._to(rng.standard_normal((len(sel), d)).astype(np.float32), dt).cuda() if basek == "base" else None
    wpe_t = WS._to(wpe32, dt).cuda() if wpe else None
    pos = None
    if positions == "explicit" and wpe:
        # all positions distinct: duplicated sel entries get DIFFERENT positions, so a kernel that indexed the positions by p
        # could not serve them
        assert len(sel) <= N_POS
        pos = rng.permutation(N_POS)[:len(sel)].astype(np.int64)
    pid = pos if pos is not None else _default_positions(cu, sel)
    return wte_t, base_t, wpe_t, pos, pid


def _run(batch, fmt, d, max_n, mode, reduce, positions, dtype, basek, wpe=True, sel=None, inplace=False, via="cache", **handle_kw):
    if sel is None:
        _assert_preconditions(batch, max_n)
        sel = _sel(batch, max_n)
    n_sel = len(sel)
    dt = DTYPES[dtype]
    wte_t, base_t, wpe_t, pos, pid = _inputs(batch, fmt, d, max_n, dtype, basek, positions, wpe, sel)
    want = _expected(batch, fmt, d, max_n, mode, reduce, sel, pid, wte_t, base_t, wpe_t)
    assert want.shape == (n_sel, d) and want.dtype == np.float32 and np.isfinite(want).all()
    cache = _cache(fmt, d, max_n, mode, **handle_kw)
    buf, out = _guarded(n_sel, d, dt)
    if inplace:
        out.copy_(base_t)
        base_t = out
    tok, cu = _tok_and_cu(batch, max_n)
    kw = dict(wte=wte_t, base=base_t, wpe=wpe_t, position_ids=None if pos is None else torch.from_numpy(pos), reduce=reduce,
              out_dtype=dt, out=out)
    if via == "cache" and not (mode == "longest_suffix" and base_t is not None):
        got = cache.embed_tokens(tok, cu_seqlens=cu, select=torch.from_numpy(sel), **kw)
    else:                                                       # the paper's lookup onto a dense base is the table's call
        got = cache.to_device().embed_select(tok, torch.from_numpy(sel), cu_seqlens=cu, **kw)
    assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n_sel, d)
    g, w = WS._bits(out), WS._bits(WS._to(want, dt))
    tag = f"{batch}-{fmt}-d{d}-n{max_n}-{mode}-{reduce}-pos_{positions}-{dtype}-{basek}-wpe{int(wpe)}"
    assert E.same_bits(g, w), f"{tag}: {_differing(g, w)}"
    _assert_guard(buf, n_sel)
    assert cache.table.status() == 0
    return cache


# ------------------------------------------------------------------ 1. formats, dims and the lookup settings in rotation
SPECIALISED = [("fp32", 1024), ("fp16", 1024), ("int8", 1024), ("int4", 1024), ("bf16", 1024), ("mxfp4", 1024),
               ("fp32", 768), ("fp16", 768), ("bf16", 768), ("int8", 768), ("fp16", 1280)]
ANY_D = [("fp16", 64), ("fp32", 136), ("int8", 48), ("int8", 2048), ("bf16", 520), ("int4", 1280), ("int4", 2048),
         ("mxfp4", 768), ("mxfp4", 2048)]
SETUPS = SPECIALISED + ANY_D
BATCHES = ("r37", "small", "r3", "tiny", "r1")


def _cases():
    out, rot = [], ("fp32", "fp16", "bf16")
    k = 0
    for s, (fmt, d) in enumerate(SETUPS):
        for max_n in (1, 2, 3, 4):
            mode = MODES[(s + max_n) % 2]
            reduce = "sum" if (mode == "cover" and (s + max_n // 2) % 2) else "mean"
            positions = ("default", "explicit")[(s + (max_n + 1) // 2) % 2]
            basek = ("wte", "base", "none")[(k + s) % 3]
            out.append((fmt, d, max_n, BATCHES[k % 5], mode, reduce, positions, rot[k % 3], basek, True))
            k += 1
    # max_n = 3 / 4 in both modes with both kinds of positions, rectangular and packed, whatever the rotation above gave them
    combos = [(n, m, p, b) for n in (3, 4) for m in MODES for p in ("default", "explicit") for b in ("r37", "small")]
    for j, (max_n, mode, positions, batch) in enumerate(combos):
        fmt, d = SETUPS[(7 * j) % len(SETUPS)]
        out.append((fmt, d, max_n, batch, mode, "mean", positions, rot[(j + 1) % 3], ("base", "wte", "none")[j % 3], True))
    # T below max_n = 4 on both bodies, and without wpe (no position at all)
    out.append(("int8", 768, 4, "r3", "cover", "mean", "explicit", "fp16", "base", True))
    out.append(("fp16", 64, 4, "r3", "cover", "mean", "default", "fp32", "wte", True))
    out.append(("int8", 768, 3, "small", "cover", "mean", "default", "fp16", "wte", False))
    out.append(("mxfp4", 2048, 4, "r37", "longest_suffix", "mean", "default", "bf16", "base", False))
    out.append(("fp32", 136, 4, "tiny", "cover", "sum", "default", "fp32", "none", False))
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return [pytest.param(*c, id="-".join(str(x) for x in c[:9]) + f"-wpe{int(c[9])}") for c in uniq]


def test_the_rotation_meets_every_setting():
    cases = [c.values for c in _cases()]
    assert {(c[0], c[1]) for c in cases} == set(SETUPS)
    for body in (SPECIALISED, ANY_D):
        mine = [c for c in cases if (c[0], c[1]) in body]
        assert {c[2] for c in mine} == {1, 2, 3, 4} and {c[4] for c in mine} == set(MODES)
        assert {c[7] for c in mine} == set(DTYPES) and {c[8] for c in mine} == {"wte", "base", "none"}
        assert {c[6] for c in mine} == {"default", "explicit"} and {c[5] for c in mine} == {"mean", "sum"}
        assert {c[3] for c in mine} == set(BATCHES)
        assert {(c[2], c[4], c[3] in RECTS) for c in mine} >= {(n, m, r) for n in (3, 4) for m in MODES for r in (True, False)}


@pytest.mark.parametrize("fmt,d,max_n,batch,mode,reduce,positions,dtype,basek,wpe", _cases())
def test_selected_rows_equal_the_oracle(fmt, d, max_n, batch, mode, reduce, positions, dtype, basek, wpe):
    _run(batch, fmt, d, max_n, mode, reduce, positions, dtype, basek, wpe)


# ------------------------------------------------------------------ 2. sizes
@pytest.mark.parametrize("n_sel", [1, 3, 5, "4x"])
@pytest.mark.parametrize("batch,fmt,d,max_n,dtype", [("r37", "int8", 768, 3, "fp16"), ("tiny", "fp16", 2048, 4, "fp32")])
def test_sizes(batch, fmt, d, max_n, dtype, n_sel):
    """A partly filled workgroup (1, 3, 5 = 4 + 1 waves) and more outputs than tokens (4 x total)."""
    total = int(_batch(batch, max_n)[1][-1])
    if n_sel == "4x":
        sel = np.random.default_rng(total).integers(0, total, size=4 * total).astype(np.int64)
        assert len(np.unique(sel)) > total // 2
    else:
        sel = _sel(batch, max_n)[:n_sel]
    _run(batch, fmt, d, max_n, "cover", "mean", "explicit", dtype, "base", sel=sel)


def test_one_call_is_one_launch_and_nothing_to_do_is_none():
    """One launch at a specialised dim and at any d; n_sel == 0 and total == 0 launch nothing."""
    for fmt, d, max_n in (("int8", 768, 3), ("fp16", 4096, 4), ("int4", 1280, 3)):
        cache = _cache(fmt, d, max_n)
        table = cache.to_device()
        tok, cu = _tok_and_cu("small", max_n)
        sel = torch.from_numpy(_sel("small", max_n))
        table.profile_enable(True)
        table.profile_read(reset=True)
        table.embed_select(tok, sel, cu_seqlens=cu)
        launches, _ = table.profile_read(reset=True)
        assert launches == 1, (fmt, d, launches)
        out = table.embed_select(tok, sel[:0], cu_seqlens=cu)
        assert tuple(out.shape) == (0, d)
        out = table.embed_select(torch.zeros((0, 5), dtype=torch.int32), sel[:0])
        assert tuple(out.shape) == (0, d)
        buf, out = _guarded(4, d, torch.float32)
        table.embed_select(torch.zeros(0, dtype=torch.int32), torch.tensor([0, 1, 2, 3]), cu_seqlens=[0], out=out)
        assert bool(torch.isnan(buf).all())
        launches, _ = table.profile_read(reset=True)
        table.profile_enable(False)
        assert launches == 0 and table.status() == 0


# ------------------------------------------------------------------ 3. in place, pinned host rows, a row shard
@pytest.mark.parametrize("batch,fmt,d,max_n,mode,dtype", [("r37", "int8", 768, 3, "cover", "fp16"),
                                                          ("small", "bf16", 520, 4, "cover", "bf16"),
                                                          ("tiny", "fp16", 1024, 4, "longest_suffix", "fp32")])
def test_in_place_out_is_base(batch, fmt, d, max_n, mode, dtype):
    _run(batch, fmt, d, max_n, mode, "mean", "explicit", dtype, "base", inplace=True)


@pytest.mark.parametrize("fmt,d", [("int8", 768), ("int8", 2048)])
def test_table_read_in_place_from_pinned_host_memory(fmt, d):
    """placement='pinned_host' with stage_tokens = 0: the row store serves the call like any other."""
    _run("small", fmt, d, 3, "cover", "mean", "default", "fp16", "wte", placement="pinned_host", hot_rows=16)


@pytest.mark.parametrize("batch,fmt,d,max_n,reduce,dtype", [("r37", "int8", 768, 3, "mean", "fp32"),
                                                            ("small", "fp16", 2048, 4, "mean", "fp16"),
                                                            ("r37", "mxfp4", 1024, 4, "sum", "bf16")])
def test_handle_that_owns_part_of_the_rows(batch, fmt, d, max_n, reduce, dtype):
    """row_begin / row_end: the sum runs over the OWNED rows of every list, the mean divides by the full K."""
    from scone_amd.hip_backend import SconeTable
    _assert_preconditions(batch, max_n)
    sel = _sel(batch, max_n)
    keys, lens = WS._vocabulary(max_n)
    table = _tables(fmt, d, max_n)[0]
    n = len(lens)
    lo, hi = n // 3, 2 * n // 3
    t = SconeTable(max_n, n, d, fmt, row_begin=lo, row_end=hi)
    t.index_build(keys, lens)
    t.store_f32(torch.from_numpy(table[lo:hi]), row0=lo)
    dt = DTYPES[dtype]
    wte_t, base_t, wpe_t, pos, pid = _inputs(batch, fmt, d, max_n, dtype, "base", "explicit", True, sel)
    want = _expected(batch, fmt, d, max_n, "cover", reduce, sel, pid, wte_t, base_t, wpe_t, own=(lo, hi))
    tok, cu = _tok_and_cu(batch, max_n)
    buf, out = _guarded(len(sel), d, dt)
    t.embed_select(tok, torch.from_numpy(sel), cu_seqlens=cu, base=base_t, wpe=wpe_t, position_ids=torch.from_numpy(pos),
                   reduce=reduce, out_dtype=dt, out=out)
    g, w = WS._bits(out), WS._bits(WS._to(want, dt))
    assert E.same_bits(g, w), _differing(g, w)
    _assert_guard(buf, len(sel))
    assert t.status() == 0


# ------------------------------------------------------------------ 4. the contract as worded: the full lookup's rows at sel
@pytest.mark.parametrize("batch,fmt,d,max_n,mode,dtype,basek", [("r37", "int8", 768, 3, "cover", "fp16", "wte"),
                                                               ("small", "fp16", 2048, 4, "cover", "bf16", "base"),
                                                               ("small", "int8", 1024, 4, "longest_suffix", "fp32", "wte")])
def test_equals_the_rows_of_the_full_lookup(batch, fmt, d, max_n, mode, dtype, basek):
    _assert_preconditions(batch, max_n)
    sel = _sel(batch, max_n)
    dt = DTYPES[dtype]
    tok_np, cu_np = _batch(batch, max_n)
    total = int(cu_np[-1])
    _, _, wte32, wpe32 = _tables(fmt, d, max_n)
    wpe_t = WS._to(wpe32, dt).cuda()
    wte_t = WS._to(wte32, dt).cuda() if basek == "wte" else None
    full_base = None
    if basek == "base":
        full_base = WS._to(np.random.default_rng(3).standard_normal((total, d)).astype(np.float32), dt).cuda()
    cache = _cache(fmt, d, max_n, mode)
    tok, cu = _tok_and_cu(batch, max_n)
    if cu is None:
        B, T = RECTS[batch]
        full = cache.embed_tokens(tok, wte=wte_t, wpe=wpe_t, base=None if full_base is None else full_base.view(B, T, d),
                                  out_dtype=dt).reshape(total, d)
    else:
        full = cache.embed_tokens(tok, cu_seqlens=cu, wte=wte_t, wpe=wpe_t, base=full_base, out_dtype=dt)
    assert not bool(torch.isnan(full).any())
    sel_t = torch.from_numpy(sel).cuda()
    buf, out = _guarded(len(sel), d, dt)
    cache.embed_tokens(tok, cu_seqlens=cu, select=sel_t, wte=wte_t, wpe=wpe_t,
                       base=None if full_base is None else full_base.index_select(0, sel_t), out_dtype=dt, out=out)
    g, w = WS._bits(out), WS._bits(full.index_select(0, sel_t))
    assert E.same_bits(g, w), _differing(g, w)
    _assert_guard(buf, len(sel))
    assert cache.table.status() == 0


# ------------------------------------------------------------------ 5. positions outside the batch
@pytest.mark.parametrize("batch,fmt,d,max_n", [("r37", "int8", 768, 3), ("small", "fp16", 2048, 4)])
def test_positions_outside_the_batch_are_left_unwritten(batch, fmt, d, max_n):
    sel = _sel(batch, max_n).copy()
    total = int(_batch(batch, max_n)[1][-1])
    bad = np.asarray([0, 5, 6, 7, 40, len(sel) - 1])
    sel[bad] = [-1, total, 2**31 - 1, -1, total, 2**31 - 1]
    good = np.setdiff1d(np.arange(len(sel)), bad)
    dt = torch.float16
    wte_t, base_t, wpe_t, pos, pid = _inputs(batch, fmt, d, max_n, "fp16", "base", "explicit", True, sel[good], seed=1)
    want = _expected(batch, fmt, d, max_n, "cover", "mean", sel[good], pid, wte_t, base_t, wpe_t)
    base_all = torch.zeros((len(sel), d), dtype=dt, device="cuda")
    base_all[torch.from_numpy(good).cuda()] = base_t
    pos_all = np.zeros(len(sel), dtype=np.int64)
    pos_all[good] = pos
    cache = _cache(fmt, d, max_n)
    table = cache.to_device()
    tok, cu = _tok_and_cu(batch, max_n)
    buf, out = _guarded(len(sel), d, dt)
    table.embed_select(tok, torch.from_numpy(sel), cu_seqlens=cu, base=base_all, wpe=wpe_t,
                       position_ids=torch.from_numpy(pos_all), out_dtype=dt, out=out)
    got = out.cpu()
    assert bool(torch.isnan(got[torch.from_numpy(bad)]).all()), "a row of a position outside the batch was written"
    g, w = WS._bits(got[torch.from_numpy(good)]), WS._bits(WS._to(want, dt))
    assert E.same_bits(g, w), _differing(g, w)
    _assert_guard(buf, len(sel))
    assert table.status() & 1
    assert table.status() == 0                                   # reading the status cleared it
    with pytest.raises(IndexError):
        cache.embed_tokens(tok, cu_seqlens=cu, select=torch.from_numpy(sel), check=True)


# ------------------------------------------------------------------ 6. refusals
def _raw(table, **kw):
    """scone_embed_select with every argument valid (a [2, 4] rectangle, two positions, fp32 out) but the ones overridden."""
    from scone_amd import _lib
    d = table.dim
    keep = dict(tok=torch.zeros(8, dtype=torch.int32, device="cuda"), sel=torch.tensor([1, 6], dtype=torch.int32, device="cuda"),
                out=torch.full((2 + GUARD, d), float("nan"), device="cuda"), cu=None, wte=None, base=None, wpe=None)
    a = dict(total=8, T=4, n_seqs=0, n_sel=2, vocab=0, n_pos=0, reduce=_lib.REDUCE_MEAN, out_dtype=_lib.DT_F32)
    buf = keep["out"]
    for k, v in kw.items():
        (keep if k in keep else a)[k] = v
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = _lib.lib().scone_embed_select(table._h, ptr(keep["tok"]), a["total"], a["T"], ptr(keep["cu"]), a["n_seqs"], ptr(keep["sel"]),
                                       a["n_sel"], ptr(keep["wte"]), a["vocab"], ptr(keep["base"]), ptr(keep["wpe"]), a["n_pos"],
                                       None, a["reduce"], ptr(keep["out"]), a["out_dtype"],
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _lib.OK or bool(torch.isnan(buf).all()), "a refused call wrote to the output"
    return rc, _lib.lib().scone_last_error(table._h).decode()


def test_every_refusal_of_the_c_call_names_its_reason():
    from scone_amd import _lib
    table = _cache("int8", 768, 3).to_device()
    rows = torch.zeros((4, 768), device="cuda")
    cu = torch.tensor([0, 3, 8], dtype=torch.int32, device="cuda")
    assert _raw(table)[0] == _lib.OK                                                   # the control: the valid call
    for kw, reason in ((dict(tok=None), "null"), (dict(sel=None), "null"), (dict(out=None), "null"),
                       (dict(total=-8), "negative"), (dict(n_sel=-1), "negative"), (dict(cu=cu, n_seqs=-2), "negative"),
                       (dict(total=2**31), r"2\^31"), (dict(T=0), "rectangle"), (dict(T=-4), "rectangle"), (dict(T=3), "rectangle"),
                       (dict(reduce=7), "reduce"), (dict(out_dtype=9), "out_dtype"),
                       (dict(wte=rows, vocab=0), "vocab"), (dict(wpe=rows, n_pos=0), "n_pos"),
                       (dict(wte=rows, vocab=4, base=rows), "exclusive")):
        rc, msg = _raw(table, **kw)
        assert rc == _lib.EINVAL and re.search(reason, msg), (kw.keys(), rc, msg)
    assert _raw(table, cu=cu, n_seqs=2, T=0)[0] == _lib.OK                             # a packed batch ignores T
    assert table.status() == 0


def test_refusals_come_back_as_scone_invalid_argument():
    from scone_amd.hip_backend import SconeInvalidArgument
    tok = torch.zeros((2, 4), dtype=torch.int32)
    sel = torch.tensor([1, 6, 6])
    cache = _cache("int8", 768, 3)
    table = cache.to_device()
    buf, out = _guarded(4, 768, torch.float32)
    with pytest.raises(SconeInvalidArgument, match="overlaps"):                       # base and out one row apart
        table.embed_select(tok, sel, base=buf[1:4], out=buf[0:3])
    with pytest.raises(SconeInvalidArgument, match="exclusive"):
        table.embed_select(tok, sel, base=torch.zeros((3, 768), device="cuda"), wte=torch.zeros((4, 768), device="cuda"), out=out[:3])
    with pytest.raises(ValueError, match="base="):
        cache.embed_tokens(tok, select=sel, base=torch.zeros((3, 768)), wte=torch.zeros((4, 768), device="cuda"), out=out[:3])
    assert bool(torch.isnan(buf).all()) and table.status() == 0
    odd = _cache("fp32", 100, 3)                                                       # d % 8 != 0
    buf, out = _guarded(3, 100, torch.float32)
    with pytest.raises(SconeInvalidArgument, match="d % 8"):
        odd.embed_tokens(tok, select=sel, out=out)
    assert bool(torch.isnan(buf).all()) and odd.table.status() == 0
    staged = _cache("int8", 768, 3, placement="pinned_host", hot_rows=16, stage_tokens=1024)
    buf, out = _guarded(3, 768, torch.float32)
    with pytest.raises(SconeInvalidArgument, match="stage_tokens"):
        staged.embed_tokens(tok, select=sel, out=out)
    with pytest.raises(SconeInvalidArgument, match="stage_tokens"):
        staged.embed_tokens(torch.zeros(8, dtype=torch.int32), cu_seqlens=[0, 3, 8], select=sel, out=out)
    assert bool(torch.isnan(buf).all())


# ------------------------------------------------------------------ 7. last_positions end to end
def test_last_positions_feed_a_decoding_step():
    """The last min(2, len) tokens of every sequence of a ragged batch equal the tail of each sequence looked up alone."""
    from scone_amd import EmbeddingCache
    d, max_n = 1280, 3
    rng = np.random.default_rng(78)
    seqs = [rng.choice(VOCAB + 1, size=n, p=TOKEN_P).tolist() for n in (4, 0, 1, 19, 2, 0, 33, 7)]
    _, _, wte32, wpe32 = _tables("fp16", d, max_n)
    wte_t, wpe_t = torch.from_numpy(wte32).half().cuda(), torch.from_numpy(wpe32).half().cuda()
    cache = _cache("fp16", d, max_n)
    ids, cu = EmbeddingCache.pack_sequences(seqs)
    sel = EmbeddingCache.last_positions(cu, 2)
    assert sel.tolist() == [2, 3, 4, 22, 23, 24, 25, 57, 58, 64, 65]
    buf, out = _guarded(len(sel), d, torch.float16)
    cache.embed_tokens(ids, cu_seqlens=cu, select=sel, wte=wte_t, wpe=wpe_t, out=out, check=True)
    want = torch.cat([cache.embed_tokens(torch.tensor([s], dtype=torch.int32), wte=wte_t, wpe=wpe_t)[0][-2:] for s in seqs if s])
    assert E.same_bits(WS._bits(out), WS._bits(want))
    _assert_guard(buf, len(sel))
    assert cache.table.status() == 0
