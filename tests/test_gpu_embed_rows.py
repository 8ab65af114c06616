"""`scone_embed_rows` / `scone_embed_rows_varlen` (include/scone_hip.h, "the fused lookup over a batch's LIVE rows") on the GPU.

The bar is bit equality in every case: fp32 output equal, fp16 / bf16 output equal to the fp32 expectation rounded once.  Every
result is compared twice: with tests/embed_rows_fixture.py (the contract restated in numpy over oracle/ref_port.py), and with the
existing lookups -- `SconeTable.embed` / `embed_base` / their packed forms -- on a table of the rows' own type that holds the same
rows at the same ids (code of the parent commit, not code under test).  Every call writes into a NaN-filled buffer followed by 64
guard rows that must stay NaN, and `table.status()` must be 0 unless the case says otherwise.

Vocabularies and the way batches are drawn are those of tests/test_gpu_walk_shapes.py.  Shapes are the smallest that reach each
piece of k_embed_rows (scone_amd/csrc/scone_embed_rows.h): token groups of 8 (record width 8) and 4 (width 16) that are partly
filled, one batch long enough for the grid-stride loop, one / 65 / 96 units per row, and live lists of 1, 2 and 2^k - 1, 2^k,
2^k + 1 ids for the lower-bound search.
"""

import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_port as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_fixture as BW  # noqa: E402
import edge_fixture as E  # noqa: E402
import embed_rows_fixture as ER  # noqa: E402
import stream_fixture as SF  # noqa: E402
import test_gpu_walk_shapes as WS  # noqa: E402  (helpers only: vocabularies, rounding)

pytestmark = pytest.mark.gpu

GUARD = 64
N_POS = WS.N_POS
DT = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
INT64_MAX = 2**63 - 1


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from scone_amd import _lib
    _lib.lib()          # fail loudly if the extension is missing


# ------------------------------------------------------------------ inputs and expectations (host only)
@functools.lru_cache(maxsize=None)
def _table32(rows_dtype, d, max_n):
    """fp32 [N, d] values that the row type holds exactly, and wte [VOCAB + 1, d], wpe [N_POS, d] in fp32."""
    rng = np.random.default_rng(31 * d + max_n)
    t = torch.from_numpy(rng.standard_normal((WS.N_ROWS[max_n], d)).astype(np.float32)).to(DT[rows_dtype]).float().numpy()
    return t, rng.standard_normal((WS.VOCAB + 1, d)).astype(np.float32), rng.standard_normal((N_POS, d)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _batch(max_n, B, T):
    keys, lens, tok = ER.batch(max_n, B, T)
    off, ids = ER.lists(keys, lens, max_n, tok)
    return tok, off, ids, np.unique(ids)


@functools.lru_cache(maxsize=None)
def _handle(rows_dtype, d, max_n, mode="cover", varlen_t=None):
    """A table of the rows' own type that holds _table32 (the comparison handle; embed_rows itself never reads its rows)."""
    from scone_amd import EmbeddingCache, NGramExtractor
    if varlen_t is not None:
        os.environ["SCONE_VARLEN_T"] = str(varlen_t)          # read when the handle is created
    try:
        keys, lens = WS._vocabulary(max_n)
        cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format=rows_dtype, lookup_mode=mode)
        table = _table32(rows_dtype, d, max_n)[0]
        cache.cache_embeddings(list(range(table.shape[0])), torch.from_numpy(table), verbose=False)
        cache.to_device()
    finally:
        if varlen_t is not None:
            del os.environ["SCONE_VARLEN_T"]
    return cache


def _guarded(n, d, dt):
    buf = torch.full((n + GUARD, d), float("nan"), dtype=dt, device="cuda")
    return buf, buf[:n]


def _assert_bits(out, want32, dt, tag):
    assert want32.dtype == np.float32 and np.isfinite(want32).all()
    g, w = WS._bits(out.reshape(want32.shape)), WS._bits(WS._to(want32, dt))
    bad = np.argwhere((g != w).any(axis=1))
    assert E.same_bits(g, w), f"{tag}: {len(bad)} of {len(g)} rows differ, first {bad[:6].ravel().tolist()}"


def _assert_preconditions(off, ids, live):
    """The batch has a position with K == 0, one with K >= 3, one that lists an id twice, and hits on the first and last live id."""
    k = np.diff(off)
    assert (k == 0).any() and (k >= 3).any()
    assert BW.positions_with_a_duplicate(off, ids) > 0
    assert live[0] in ids and live[-1] in ids and len(live) >= 3


def _run(max_n, B, T, d, rows_dtype, out_dtype, mode="cover", reduce="mean", form="wte_wpe", positions="default", cu=None,
         inplace=False, live=None, rows32=None, n=None, status=0, varlen_t=None, tok=None, compare_table=True, tag=""):
    """One lookup over live rows against the fixture and (every hit listed) against the table lookups.  `live` / `rows32`
    default to the batch's distinct ids and their rows of _table32; `n`: a device count."""
    keys, lens = WS._vocabulary(max_n)
    if tok is None:
        tok = _batch(max_n, B, T)[0]
    tok = tok.reshape(-1) if cu is not None else tok
    ntok = tok.size
    off, ids = ER.lists(keys, lens, max_n, tok, cu)
    table32, wte32, wpe32 = _table32(rows_dtype, d, max_n)
    all_live = np.unique(ids)
    if live is None:
        live = all_live
    if rows32 is None:
        rows32 = table32[live]
    rdt, odt = DT[rows_dtype], DT[out_dtype]
    cache = _handle(rows_dtype, d, max_n, mode, varlen_t)
    t = cache.table
    assert t.status() == 0
    rng = np.random.default_rng(ntok + d)
    wte_t = WS._to(wte32, odt).cuda() if form == "wte_wpe" else None
    wpe_t = WS._to(wpe32, odt).cuda() if form in ("wte_wpe", "base_wpe") else None
    base_t = WS._to(rng.standard_normal((ntok, d)).astype(np.float32), odt).cuda() if form in ("base_wpe", "base") else None
    pos = rng.integers(0, N_POS, size=tok.shape).astype(np.int64) if (positions == "random" and wpe_t is not None) else None
    ids_t = torch.from_numpy(np.ascontiguousarray(live)).cuda()
    rows_t = torch.from_numpy(np.ascontiguousarray(rows32)).to(rdt).cuda()
    tok_t = torch.from_numpy(tok)
    cu_t = None if cu is None else torch.from_numpy(np.asarray(cu, dtype=np.int32))
    # ---- expectation
    if wte_t is not None:
        base32 = wte_t.float().cpu().numpy()[tok.reshape(-1)]
    else:
        base32 = None if base_t is None else base_t.float().cpu().numpy()
    n_live = len(live) if n is None else min(int(n), len(live))
    want = ER.expected(keys, lens, max_n, table32.shape[0], tok, cu, live[:n_live], ER.widen(rows_t)[:n_live], mode, reduce,
                       base32=base32, wpe32=None if wpe_t is None else wpe_t.float().cpu().numpy(), pid=pos)
    # ---- the call under test
    if inplace:
        buf = torch.full((ntok + GUARD, d), float("nan"), dtype=odt, device="cuda")
        buf[:ntok] = base_t
        out = base_arg = buf[:ntok]
    else:
        buf, out = _guarded(ntok, d, odt)
        base_arg = base_t
    n_t = None if n is None else torch.tensor([int(n)], dtype=torch.int64, device="cuda")
    got = t.embed_rows(tok_t, ids_t, rows_t, n=n_t, cu_seqlens=cu_t, wte=wte_t, wpe=wpe_t, base=base_arg,
                       pos=None if pos is None else torch.from_numpy(pos), reduce=reduce, out_dtype=odt, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == odt
    tag = tag or f"n{max_n}-{B}x{T}-d{d}-{rows_dtype}->{out_dtype}-{mode}-{reduce}-{form}-pos_{positions}"
    _assert_bits(out, want, odt, tag + " (fixture)")
    assert bool(torch.isnan(buf[ntok:]).all()), f"{tag}: a guard row behind the output was written"
    assert t.status() == status, tag
    assert t.status() == 0                                           # the bits are read once
    # ---- the same rows in a table: the existing lookups
    if compare_table and n_live == len(all_live) and np.array_equal(live[:n_live], all_live):
        kw = dict(position_ids=None if pos is None else torch.from_numpy(pos), reduce=reduce, out_dtype=odt)
        if base_t is not None:
            ref = (t.embed_base(tok_t, base_t, wpe=wpe_t, **kw) if cu is None
                   else t.embed_base_varlen(tok_t, cu_t.cuda(), base_t, wpe=wpe_t, **kw))
        else:
            ref = (t.embed(tok_t, wte=wte_t, wpe=wpe_t, **kw) if cu is None
                   else t.embed_varlen(tok_t, cu_t.cuda(), wte=wte_t, wpe=wpe_t, **kw))
        assert E.same_bits(WS._bits(out.reshape(ntok, d)), WS._bits(ref.reshape(ntok, d))), tag + " (table lookup)"
        assert t.status() == 0
    return out


# ------------------------------------------------------------------ token groups, record widths, row widths
@pytest.mark.parametrize("B,T", [(1, 1), (1, 7), (3, 13), (7, 5)])
@pytest.mark.parametrize("max_n", [1, 3, 4])
def test_token_groups(max_n, B, T):
    """1 x 1 and 1 x 7 are shorter than a group of 8 (1 x 7 longer than one of 4); 3 x 13 and 7 x 5 are no multiples of 8 or 4."""
    if (B, T) == (3, 13) and max_n >= 3:
        _assert_preconditions(*_batch(max_n, B, T)[1:])
    _run(max_n, B, T, 768, "fp32", "fp32")
    _run(max_n, B, T, 8, "bf16", "fp16", form="base_wpe", positions="random")


@pytest.mark.parametrize("max_n", [3, 4])
def test_grid_stride_loop(max_n):
    """2048 x 32 tokens: 8192 groups of 8 (16384 of 4), four to a workgroup, on a grid capped at 6 workgroups per compute unit
    (scone_embed_rows.h): every wave takes a second group -- asserted from the box's own CU count."""
    B, T = 2048, 32
    groups = B * T // (64 // (8 if max_n <= 3 else 16))
    assert groups // 4 > 6 * torch.cuda.get_device_properties(0).multi_processor_count
    _assert_preconditions(*_batch(max_n, B, T)[1:])
    _run(max_n, B, T, 64, "fp16", "bf16", form="base")


@pytest.mark.parametrize("d", [8, 520, 768])
@pytest.mark.parametrize("max_n", [3, 4])
def test_row_widths(d, max_n):
    """d = 8: one lane has work; 520: 65 units, a second trip of the unit loop for lane 0 only; 768: 96 units."""
    _run(max_n, 3, 13, d, "fp32", "fp16")
    _run(max_n, 3, 13, d, "fp16", "fp32", reduce="sum", form="base")


# ------------------------------------------------------------------ search edges
@functools.lru_cache(maxsize=None)
def _prefix_with(U, max_n=4):
    """A token stream [1, L], cut so that its live list has exactly U ids."""
    keys, lens = WS._vocabulary(max_n)
    for seed in range(400):
        tok = ER.batch(max_n, 1, 96, seed=seed)[2]
        hits = R.match_hits(keys, lens, tok, max_n)
        for L in range(1, tok.shape[1] + 1):
            seen = set()
            for n in range(1, max_n + 1):
                seen.update(int(x) for x in hits[n - 1, 0, :max(L - n + 1, 0)] if x >= 0)
            if len(seen) == U:
                return tok[:, :L].copy()
            if len(seen) > U:
                break
    raise AssertionError(f"no prefix with {U} live ids")


@pytest.mark.parametrize("U", [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33])
def test_search_edges(U):
    tok = _prefix_with(U)
    keys, lens = WS._vocabulary(4)
    live = np.unique(ER.lists(keys, lens, 4, tok)[1])
    assert len(live) == U                                             # the truncation hit the value
    _run(4, 1, tok.shape[1], 8, "fp32", "fp32", tok=tok, form="none", tag=f"U={U}")
    _run(4, 1, tok.shape[1], 8, "bf16", "bf16", tok=tok, form="base", reduce="sum", tag=f"U={U} base")


# ------------------------------------------------------------------ dtypes and forms
@pytest.mark.parametrize("rows_dtype", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("out_dtype", ["fp32", "fp16", "bf16"])
def test_dtypes(rows_dtype, out_dtype):
    _run(3, 3, 13, 768, rows_dtype, out_dtype, form="wte_wpe")
    _run(4, 7, 5, 520, rows_dtype, out_dtype, form="base_wpe", positions="random", reduce="sum")


@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
@pytest.mark.parametrize("form", ["wte_wpe", "base_wpe", "base", "none"])
def test_forms(mode, reduce, form):
    _run(3, 3, 13, 768, "bf16", "fp16", mode=mode, reduce=reduce, form=form)
    if form in ("wte_wpe", "base_wpe"):
        _run(4, 3, 13, 520, "fp32", "fp32", mode=mode, reduce=reduce, form=form, positions="random")


@pytest.mark.parametrize("mode", ["cover", "longest_suffix"])
@pytest.mark.parametrize("out_dtype", ["fp32", "fp16"])
def test_out_is_base(mode, out_dtype):
    _run(3, 3, 13, 768, "fp16", out_dtype, mode=mode, form="base_wpe", inplace=True)
    _run(4, 7, 5, 8, "fp32", out_dtype, mode=mode, form="base", inplace=True)


# ------------------------------------------------------------------ packed batches
CU = np.asarray([0, 13, 13, 14, 30, 39])        # an empty and a one-token sequence


@pytest.mark.parametrize("max_n", [3, 4])
@pytest.mark.parametrize("form,positions,mode", [("wte_wpe", "default", "cover"), ("base_wpe", "random", "cover"),
                                                 ("base", "default", "longest_suffix"), ("none", "default", "cover"),
                                                 ("wte_wpe", "default", "longest_suffix")])
def test_packed(max_n, form, positions, mode):
    _run(max_n, 3, 13, 768, "bf16", "fp16", mode=mode, form=form, positions=positions, cu=CU)
    _run(max_n, 3, 13, 8, "fp32", "fp32", mode=mode, form=form, positions=positions, cu=CU, reduce="sum")


@pytest.mark.parametrize("form", ["base_wpe", "wte_wpe"])
def test_packed_with_a_remainder_launch(form):
    """SCONE_VARLEN_T = 16 on 39 tokens: a main launch of two rows and a remainder of 7 -- base, out, tok, pos and the records
    move together."""
    assert CU[-1] > 2 * 16 and CU[-1] % 16 != 0
    _run(3, 3, 13, 520, "fp16", "fp16", form=form, cu=CU, varlen_t=16)
    _run(4, 3, 13, 520, "fp16", "fp32", form=form, cu=CU, varlen_t=16, inplace=form == "base_wpe", positions="random")


# ------------------------------------------------------------------ unlisted ids
@pytest.mark.parametrize("max_n", [3, 4])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_unlisted_ids(max_n, reduce):
    """Every third id, the first and the last are dropped from the list: their hits add +0.0, K stays the full count, and
    SCONE_ST_BAD_ID is raised once."""
    from scone_amd import _lib
    keys, lens = WS._vocabulary(max_n)
    tok, off, ids, live = _batch(max_n, 3, 13)
    listed = ER.unlisted(live)
    table32 = _table32("fp32", 768, max_n)[0]
    out = _run(max_n, 3, 13, 768, "fp32", "fp32", reduce=reduce, form="base", live=listed, status=_lib.ST_BAD_ID)
    if reduce == "mean":
        rng = np.random.default_rng(tok.size + 768)          # _run's base
        base32 = WS._to(rng.standard_normal((tok.size, 768)).astype(np.float32), torch.float32).numpy()
        wrong = ER.wrong_model_drops_unlisted(keys, lens, max_n, table32.shape[0], tok, None, listed, table32[listed], reduce,
                                              base32=base32)
        assert not E.same_bits(out.cpu().numpy(), wrong)
    _run(max_n, 3, 13, 8, "bf16", "fp16", reduce=reduce, form="wte_wpe", live=listed, status=_lib.ST_BAD_ID)


@pytest.mark.parametrize("cu", [None, CU], ids=["rect", "packed"])
def test_no_live_rows(cu):
    """n = 0: every hit is unlisted (null id and row pointers are fine)."""
    from scone_amd import _lib
    _run(3, 3, 13, 768, "fp32", "fp16", form="base_wpe", cu=cu, live=np.zeros(0, dtype=np.int64),
         rows32=np.zeros((0, 768), dtype=np.float32), status=_lib.ST_BAD_ID)


# ------------------------------------------------------------------ the count on the device
@pytest.mark.parametrize("max_n", [3, 4])
def test_device_count(max_n):
    from scone_amd import _lib
    tok, off, ids, live = _batch(max_n, 3, 13)
    U, d = len(live), 768
    table32 = _table32("bf16", d, max_n)[0]
    cap_ids = np.concatenate([live, np.full(100, INT64_MAX, dtype=np.int64)])
    cap_rows = np.concatenate([table32[live], np.full((100, d), np.nan, dtype=np.float32)])
    plain = _run(max_n, 3, 13, d, "bf16", "fp32", form="base_wpe")
    # *d_n = U on a capacity of U + 100 whose tail is NaN rows under INT64_MAX ids: the bits of the plain call
    out = _run(max_n, 3, 13, d, "bf16", "fp32", form="base_wpe", live=cap_ids, rows32=cap_rows, n=U)
    assert E.same_bits(out.cpu().numpy(), plain.cpu().numpy())
    # *d_n = U // 2: the upper half is unlisted
    _run(max_n, 3, 13, d, "bf16", "fp32", form="base_wpe", live=cap_ids, rows32=cap_rows, n=U // 2, status=_lib.ST_BAD_ID)
    # *d_n > n: the count clamps to n
    out = _run(max_n, 3, 13, d, "bf16", "fp32", form="base_wpe", n=U + 1000)
    assert E.same_bits(out.cpu().numpy(), plain.cpu().numpy())


# ------------------------------------------------------------------ stream order
def test_stream_order():
    """The rows are filled on a producer stream behind a delay; the call, on another stream, follows an event and returns while
    the delay runs; its result is right with nothing but that stream synchronised."""
    max_n, B, T, d = 3, 3, 13, 768
    keys, lens = WS._vocabulary(max_n)
    tok, off, ids, live = _batch(max_n, B, T)
    table32, _, wpe32 = _table32("fp16", d, max_n)
    cache = _handle("fp16", d, max_n)
    t = cache.table
    dev = torch.device("cuda")
    truth = torch.from_numpy(table32[live]).to(torch.float16).to(dev)
    poison = (truth.float() * 0.5 + 1.0).to(torch.float16)
    rows = poison.clone()
    ids_t = torch.from_numpy(live).to(dev)
    tok_t = torch.from_numpy(tok).to(dev, torch.int32)
    wpe_t = WS._to(wpe32, torch.float16).to(dev)
    base_t = WS._to(np.random.default_rng(3).standard_normal((B * T, d)).astype(np.float32), torch.float16).to(dev)
    P = SF.side_stream(t, tag="rows-producer")
    S = SF.side_stream(t, beside=(P,), tag="rows-consumer")
    SF.warm_delay()
    with torch.cuda.stream(S):                                       # warm-up: module load, the stream's match workspace
        t.embed_rows(tok_t, ids_t, rows, base=base_t, wpe=wpe_t)
    S.synchronize()
    torch.cuda.synchronize()
    filled = torch.cuda.Event()
    buf, out = _guarded(B * T, d, torch.float16)
    with torch.cuda.stream(P):
        SF.delay()
        rows.copy_(truth, non_blocking=True)
        filled.record(P)
    with torch.cuda.stream(S):
        S.wait_event(filled)
        got = t.embed_rows(tok_t, ids_t, rows, base=base_t, wpe=wpe_t, out=out)
        returned_early = not filled.query()
        rows.copy_(poison, non_blocking=True)                        # a kernel that runs later than S says reads this
        snap = got.clone()
    S.synchronize()
    assert returned_early, "scone_embed_rows synchronised (or the delay was too short to tell)"
    want = ER.expected(keys, lens, max_n, table32.shape[0], tok, None, live, ER.widen(truth), "cover", "mean",
                       base32=base_t.float().cpu().numpy(), wpe32=wpe_t.float().cpu().numpy())
    _assert_bits(snap, want, torch.float16, "stream order")
    assert bool(torch.isnan(buf[B * T:]).all())
    assert t.status() == 0


# ------------------------------------------------------------------ entry errors
def _raw_call(t, live, tok, B, T, out, out_dtype, *, wte=None, vocab=0, base=None, wpe=None, n_pos=0, reduce=None, cu=None,
              n_seqs=0, total=0, null_live=False):
    from scone_amd import _lib as L
    p = lambda x: None if x is None else (x if isinstance(x, int) else x.data_ptr())  # noqa: E731
    reduce = L.REDUCE_MEAN if reduce is None else reduce
    lp = None if null_live else C.byref(live)
    s = torch.cuda.current_stream().cuda_stream
    if cu is None:
        return L.lib().scone_embed_rows(t._h, lp, p(tok), B, T, p(wte), vocab, p(base), p(wpe), n_pos, None, reduce, p(out),
                                        out_dtype, s)
    return L.lib().scone_embed_rows_varlen(t._h, lp, p(tok), p(cu), n_seqs, total, p(wte), vocab, p(base), p(wpe), n_pos, None,
                                           reduce, p(out), out_dtype, s)


def test_entry_errors():
    """Every refusal of the header: SCONE_EINVAL, a text that names the reason, the output untouched."""
    from scone_amd import _lib as L
    from scone_amd.hip_backend import SconeTable
    max_n, B, T, d = 3, 3, 13, 64
    keys, lens = WS._vocabulary(max_n)
    tok_np, off, ids, live = _batch(max_n, B, T)
    t = _handle("fp32", d, max_n).table
    tok = torch.from_numpy(tok_np).to("cuda", torch.int32)
    ids_t = torch.from_numpy(live).cuda()
    rows = torch.zeros((len(live) + 1, d), dtype=torch.float32, device="cuda")
    out = torch.full((B * T + 1, d), float("nan"), dtype=torch.float32, device="cuda")
    other = torch.zeros((B * T + 1, d), dtype=torch.float32, device="cuda")
    cu = torch.tensor([0, 13, 39], dtype=torch.int32, device="cuda")

    def live_of(**kw):
        f = dict(struct_size=C.sizeof(L.SconeLiveRows), dtype=L.DT_F32, d_row_ids=ids_t.data_ptr(), d_rows=rows.data_ptr(),
                 n=len(live), d_n=None)
        f.update(kw)
        return L.SconeLiveRows(f["struct_size"], f["dtype"], f["d_row_ids"], f["d_rows"], f["n"], f["d_n"])

    def refused(rc, table, *words):
        text = L.lib().scone_last_error(table._h).decode()
        assert rc == L.EINVAL, (rc, text, words)
        assert all(w in text for w in words), (text, words)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), f"the output was written by a refused call ({words})"

    ok = live_of()
    F32 = L.DT_F32
    for who, kw in (("scone_embed_rows", {}), ("scone_embed_rows_varlen", dict(cu=cu, n_seqs=2, total=B * T))):
        call = functools.partial(_raw_call, **kw)
        refused(call(t, ok, tok, B, T, out, F32, null_live=True), t, who, "null live")
        refused(call(t, live_of(d_row_ids=None), tok, B, T, out, F32), t, who, "null pointer", "d_row_ids")
        refused(call(t, live_of(d_rows=None), tok, B, T, out, F32), t, who, "null pointer", "d_rows")
        refused(call(t, ok, None, B, T, out, F32), t, who, "null pointer", "d_tok")
        refused(call(t, ok, tok, B, T, None, F32), t, who, "null pointer", "d_out")
        refused(call(t, live_of(struct_size=24), tok, B, T, out, F32), t, who, "struct_size")
        refused(call(t, live_of(dtype=7), tok, B, T, out, F32), t, who, "bad dtype")
        refused(call(t, ok, tok, B, T, out, 9), t, who, "bad out_dtype")
        refused(call(t, ok, tok, B, T, out, F32, reduce=5), t, who, "bad reduce")
        refused(call(t, live_of(n=2**31), tok, B, T, out, F32), t, who, "2^31 - 1")
        refused(call(t, live_of(d_rows=rows.data_ptr() + 4), tok, B, T, out, F32), t, who, "16-byte aligned")
        refused(call(t, ok, tok, B, T, out, F32, wte=other, vocab=4, base=other), t, who, "exclusive")
        refused(call(t, ok, tok, B, T, out, F32, wte=other, vocab=0), t, who, "without vocab")
        refused(call(t, ok, tok, B, T, out, F32, wpe=other, n_pos=0), t, who, "without vocab/n_pos")
        refused(call(t, ok, tok, B, T, out, F32, base=out.data_ptr() + 4 * d), t, who, "overlaps")
    refused(_raw_call(t, ok, tok, -1, T, out, F32), t, "scone_embed_rows", "negative B or T")
    refused(_raw_call(t, ok, tok, B, T, out, F32, cu=cu, n_seqs=-1, total=B * T), t, "scone_embed_rows_varlen", "negative")
    refused(_raw_call(t, ok, tok, B, T, out, F32, cu=cu, n_seqs=2, total=2**31), t, "scone_embed_rows_varlen", "2^31 - 1")
    refused(_raw_call(t, ok, tok, B, T, out, F32, cu=0, n_seqs=2, total=B * T), t, "scone_embed_rows_varlen", "d_cu_seqlens")
    # an empty batch returns before `live` and the pointers are looked at
    assert _raw_call(t, None, None, 0, 5, None, F32, null_live=True) == L.OK
    assert _raw_call(t, None, None, B, T, None, F32, cu=cu, n_seqs=0, total=0, null_live=True) == L.OK
    # handles: a row shard, a dim that is no multiple of 8, an index without a table
    shard = SconeTable(max_n, WS.N_ROWS[max_n], d, "fp32", row_begin=10, row_end=40)
    shard.index_build(keys, lens)
    refused(_raw_call(shard, ok, tok, B, T, out, F32), shard, "scone_embed_rows", "row-sharded")
    odd = SconeTable(max_n, WS.N_ROWS[max_n], 100, "fp32")
    odd.index_build(keys, lens)
    refused(_raw_call(odd, ok, tok, B, T, out, F32), odd, "scone_embed_rows", "dim % 8")
    bare = SconeTable(max_n, WS.N_ROWS[max_n], 0, "fp32")
    bare.index_build(keys, lens)
    refused(_raw_call(bare, ok, tok, B, T, out, F32, cu=cu, n_seqs=2, total=B * T), bare, "scone_embed_rows_varlen", "dim > 0")
    assert t.status() == 0


def test_pinned_host_and_staged_handles_are_accepted():
    """The table is never read: a handle whose rows live in pinned host memory, read in place or staged, looks live rows up."""
    from scone_amd import EmbeddingCache, NGramExtractor
    max_n, B, T, d = 3, 3, 13, 768
    keys, lens = WS._vocabulary(max_n)
    tok, off, ids, live = _batch(max_n, B, T)
    table32 = _table32("fp32", d, max_n)[0]
    want = ER.expected(keys, lens, max_n, table32.shape[0], tok, None, live, table32[live], "cover", "mean")
    for stage in (0, 128):
        cache = EmbeddingCache(NGramExtractor.from_arrays(keys, lens, max_n=max_n), d, table_format="int8", placement="pinned_host",
                               hot_rows=16, stage_tokens=stage)
        cache.cache_embeddings(list(range(table32.shape[0])), torch.zeros(table32.shape), verbose=False)   # rows that would be wrong
        buf, out = _guarded(B * T, d, torch.float32)
        cache.table.embed_rows(torch.from_numpy(tok), torch.from_numpy(live), torch.from_numpy(table32[live]), out=out)
        _assert_bits(out, want, torch.float32, f"pinned_host stage_tokens={stage}")
        assert bool(torch.isnan(buf[B * T:]).all()) and cache.table.status() == 0
